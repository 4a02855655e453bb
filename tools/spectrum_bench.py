#!/usr/bin/env python3
"""Spectral-density (kernel polynomial method) benchmark on the device: one JSON line per case.

    python tools/spectrum_bench.py [--n 1000000] [--k 8] [--probes 32] [--orders 63 127 255] [--dtype float64]
                                   [--eigvalsh 2000 4000] [--out FILE]

moments lines: one gspx_cheby_moments_dev call on --probes resident +-1 vectors of Sensor(n, k), order + 1 moments
(best of three after a warm-up): the device time of the call and its split into recurrence steps (ctx.last_timing()
["steps_ms"]) and the k_slot_dots phase (["combine_ms"], the reduction of the partials included); the bytes that
phase reads (every kept slot once, the first slot of every chunk but chunk 0 twice: chunks of 16 slots, of 8 for
fp32 panels of an even width) and the rate that makes,
beside the read-only rate ctx.bench_read measures in the same run.
density line: wall time of Graph.estimate_spectral_density (probes built on the host, uploaded, one call), host clock.
eigvalsh lines: np.linalg.eigvalsh of the dense Laplacian of Sensor(N, k) on the host, for comparison.
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
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--probes", type=int, default=32)
    ap.add_argument("--orders", type=int, nargs="*", default=[63, 127, 255])
    ap.add_argument("--dtype", default="float64", choices=["float64", "float32"])
    ap.add_argument("--eigvalsh", type=int, nargs="*", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from pygsp_amd import graphs, spectrum
    outf = open(a.out, "a") if a.out else None
    dtype = np.dtype(a.dtype)
    if a.orders:
        G = graphs.Sensor(a.n, k=a.k, seed=0, compute_dtype=dtype.type)
        G.estimate_lmax("bounds")
        dev = G.device_graph(dtype.type)
        d = G.to_device(spectrum.probes(G.N, a.probes, 0))
        try:
            for order in a.orders:
                M = order + 1
                S = M // 2 + 1
                stack_bytes = float(dtype.itemsize) * S * G.N * a.probes
                chunk = 8 if dtype.itemsize == 4 and a.probes % 2 == 0 else 16  # DOTS_CS, csrc/gspx_poly.hip.h
                read_bytes = stack_bytes * (S + (S - 1 + chunk - 1) // chunk - 1) / S
                read_gbps = dev.ctx.bench_read(int(min(stack_bytes, 4 << 30)), passes=10)
                dev.cheby_moments_dev(d.ptr, a.probes, G.lmax, M)  # warm-up (workspaces)
                best = None
                for _ in range(3):
                    dev.cheby_moments_dev(d.ptr, a.probes, G.lmax, M)
                    t = dev.ctx.last_timing()
                    best = t if best is None or t["total_ms"] < best["total_ms"] else best
                emit({"case": "moments_sensor{}_k{}_w{}_order{}_{}".format(G.N, a.k, a.probes, order, dtype.name),
                      "N": G.N, "probes": a.probes, "order": order, "moments": M, "slots": S, "steps": S - 1,
                      "total_ms": best["total_ms"], "steps_ms": best["steps_ms"], "dots_ms": best["combine_ms"],
                      "copy_in_ms": best["permute_ms"], "ms_per_step": best["steps_ms"] / (S - 1),
                      "stack_bytes": stack_bytes, "dots_read_bytes": read_bytes,
                      "dots_read_GBps": read_bytes / (best["combine_ms"] * 1e-3) / 1e9, "bench_read_GBps": read_gbps,
                      "step_kinds": dev.ctx.last_step_kinds()}, outf)
        finally:
            d.free()
        order = a.orders[0]
        G.estimate_spectral_density(order=order, n_vectors=a.probes)  # warm-up
        walls = []
        for _ in range(2):
            t = time.perf_counter()
            sd = G.estimate_spectral_density(order=order, n_vectors=a.probes)
            walls.append(time.perf_counter() - t)
        emit({"case": "density_sensor{}_k{}_w{}_order{}_{}".format(G.N, a.k, a.probes, order, dtype.name), "N": G.N,
              "probes": a.probes, "order": order, "wall_s_best": min(walls), "wall_s": walls,
              "device_ms_last": getattr(G, "_gspx_last_kernel_ms", None), "median_eigenvalue": sd.quantile(0.5),
              "lmax": G.lmax, "mu1_stderr": float(sd.mu_stderr[1])}, outf)
    for n in a.eigvalsh:
        from oracle import cheby_oracle as orc
        from oracle import knn_oracle as knn
        L = orc.laplacian(knn.knn_weights(knn.sensor_coords(n, seed=0), a.k)[0]).toarray()
        t = time.perf_counter()
        e = np.linalg.eigvalsh(L)
        emit({"case": "eigvalsh_sensor{}_k{}".format(n, a.k), "N": n, "wall_s": time.perf_counter() - t,
              "median_eigenvalue": float(np.median(e))}, outf)


if __name__ == "__main__":
    main()
