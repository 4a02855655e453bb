#!/usr/bin/env python3
"""Spectrogram / localised-atom norm benchmark on the device: one JSON line per case.

    python tools/features_bench.py [--sizes 10000 100000] [--M 100] [--norm-sizes 1000000] [--nf 1 4 8 100]
                                   [--width 64] [--out FILE]

spectrogram lines: wall time of features.compute_spectrogram(Sensor(N), M) (host clock, best of --reps after a
warm-up; the graph and lmax are set up before), and the device time of its sqnorms calls.
norms lines: one gspx_cheby_sqnorms_dev call on an identity panel of --width columns of Sensor(N), order 30: the time of
the k_combine_sqnorm phase (ctx.last_timing()["combine_ms"], one batch) against one read of the kept stack
(M N width elements) at the read-only rate ctx.bench_read measures in the same run, and the fp64 flop/s it reaches
(2 Nf M + 2 Nf flop per stack element column, i.e. forming and squaring every output element).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(rec, outf):
    line = json.dumps(rec)
    print(line, flush=True)
    if outf:
        outf.write(line + "\n")
        outf.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[10_000, 100_000])
    ap.add_argument("--M", type=int, default=100)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--norm-sizes", type=int, nargs="*", default=[1_000_000])
    ap.add_argument("--nf", type=int, nargs="+", default=[1, 4, 8, 100])
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from pygsp_amd import engine, features, filters, graphs
    outf = open(a.out, "a") if a.out else None
    for N in a.norm_sizes:
        G = graphs.Sensor(N, seed=0)
        G.estimate_lmax("bounds")
        dev = G.device_graph(np.float64)
        M = 31
        stack_bytes = 8.0 * M * N * a.width
        read_gbps = dev.ctx.bench_read(int(min(stack_bytes, 4 << 30)), passes=10)
        bx = dev.ctx.alloc(N * a.width * 8)
        try:
            dev.ctx.identity_panel(bx, N, 0, a.width, np.float64)
            for nf in a.nf:
                kern = features.spectrogram_kernels(G, None, nf)
                C = filters._as_coeff_matrix(filters.compute_cheby_coeff(filters.Filter(G, kern), m=M - 1))
                dev.cheby_sqnorms_dev(C, bx.ptr, a.width, G.lmax)  # warm-up
                best = None
                for _ in range(3):
                    dev.cheby_sqnorms_dev(C, bx.ptr, a.width, G.lmax)
                    t = dev.ctx.last_timing()
                    best = t if best is None or t["combine_ms"] < best["combine_ms"] else best
                read_ms = stack_bytes / (read_gbps * 1e9) * 1e3
                flop = (2.0 * nf * M + 2.0 * nf) * N * a.width
                emit({"case": "sqnorms_sensor{}_w{}_nf{}".format(N, a.width, nf), "N": N, "width": a.width, "Nf": nf,
                      "M": M, "norms_kernel_ms": best["combine_ms"], "steps_ms": best["steps_ms"],
                      "total_ms": best["total_ms"], "stack_read_ms_at_bench_read": read_ms,
                      "bench_read_GBps": read_gbps, "norms_vs_one_read": best["combine_ms"] / read_ms,
                      "fp64_tflops": flop / (best["combine_ms"] * 1e-3) / 1e12}, outf)
        finally:
            bx.free()
    for N in a.sizes:
        G = graphs.Sensor(N, seed=0)
        G.estimate_lmax("bounds")
        features.compute_spectrogram(G, M=a.M)  # warm-up (workspaces, coefficients' tables)
        walls = []
        for _ in range(a.reps):
            t = time.perf_counter()
            features.compute_spectrogram(G, M=a.M)
            walls.append(time.perf_counter() - t)
        emit({"case": "spectrogram_sensor{}_M{}".format(N, a.M), "N": N, "M": a.M, "wall_s_best": min(walls),
              "wall_s": walls, "device_ms_last": getattr(G, "_gspx_last_kernel_ms", None)}, outf)


if __name__ == "__main__":
    main()
