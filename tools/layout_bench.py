#!/usr/bin/env python3
"""Spring layout benchmark on the device: one JSON line per case.

    python tools/layout_bench.py [--N 10000 100000] [--dim 2 3] [--iters 50] [--graphs sensor er] [--out FILE]
    python tools/layout_bench.py --reference path/to/pygsp [--ref-N 1000 2000] [--out FILE]     (host, no GPU)

Device cases: Sensor(N, seed=0) and ErdosRenyi(N, p = 10 / N, seed=0) (about ten neighbours per vertex), float64 graph,
start positions from default_rng(0).uniform, k = sqrt(1 / N), `iters` iterations in one gspx_layout_spring_dev call on
positions that stay on the device (best of 3 after a warm-up of 2 iterations).  Reported: ms per iteration, pair
interactions per second (N^2 per iteration: every ordered pair, i = j included, as the kernel walks them), and fp64
operations per second of the all-pairs kernel against the 78.6 TFLOP/s vector peak that profiles/features.md uses.
Operation count per ordered pair, a fused multiply-add counted as two: dim subtractions, d^2 (1 multiplication, dim - 1
FMA), 1 max, 1 reciprocal, two Newton steps (4 FMA), 1 multiplication by k^2, dim FMA into the sums - 20 operations
in 2-D (13 instructions), 25 in 3-D (16 instructions).  The O(nnz) attraction and the update are not counted.
The wall line times Graph.set_coordinates() (50 iterations, upload, download, rescaling) on ErdosRenyi(--wall-N).

--reference: the real pygsp's own ``set_coordinates('spring', seed=0)`` on Sensor(N, seed=0), wall seconds on the host
(an O(N^2) Python loop per iteration: quote a run next to the device numbers, it cannot run where there is no pygsp).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP64_TFLOPS = 78.6
OPS_PER_PAIR = {2: 20, 3: 25}


def emit(rec, outf):
    line = json.dumps(rec)
    print(line, flush=True)
    if outf:
        outf.write(line + "\n")
        outf.flush()


def reference_times(path, sizes, outf):
    sys.path.insert(0, path)
    os.environ.setdefault("MPLBACKEND", "agg")
    from pygsp import graphs
    for N in sizes:
        G = graphs.Sensor(N, seed=0)
        t = time.perf_counter()
        G.set_coordinates("spring", seed=0)
        wall = time.perf_counter() - t
        emit({"case": "reference_sensor{}".format(N), "N": N, "dim": 2, "iterations": 50, "host_wall_s": wall,
              "ms_per_iteration": wall / 50 * 1e3, "pairs_per_s": 50.0 * N * N / wall}, outf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--dim", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--graphs", nargs="+", default=["sensor", "er"], choices=["sensor", "er"])
    ap.add_argument("--wall-N", type=int, default=100_000)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--ref-N", type=int, nargs="+", default=[1000, 2000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    outf = open(a.out, "a") if a.out else None
    if a.reference:
        return reference_times(a.reference, a.ref_N, outf)
    from pygsp_amd import engine, graphs
    for N in a.N:
        for kind in a.graphs:
            G = graphs.Sensor(N, seed=0) if kind == "sensor" else graphs.ErdosRenyi(N, p=10.0 / N, seed=0)
            dev = G.device_graph(np.float64)
            k = float(np.sqrt(1.0 / N))
            for dim in a.dim:
                start = engine.DeviceArray.from_host(dev.ctx, np.random.default_rng(0).uniform(size=(N, dim)))
                dev.layout_spring(start, k, iterations=2)[0].free()  # warm-up
                best = None
                for _ in range(3):
                    out, report = dev.layout_spring(start, k, iterations=a.iters)
                    finite = bool(np.isfinite(np.asarray(out)).all())
                    out.free()
                    if best is None or report["kernel_ms"] < best["kernel_ms"]:
                        best = report
                start.free()
                per_it = best["kernel_ms"] / a.iters
                pairs = float(N) * N / (per_it * 1e-3)
                emit({"case": "layout_{}{}_dim{}".format(kind, N, dim), "N": N, "nnz": int(G.W.nnz), "dim": dim,
                      "iterations": a.iters, "splits": best["splits"], "device_ms": best["kernel_ms"],
                      "ms_per_iteration": per_it, "pairs_per_s": pairs, "ops_per_pair": OPS_PER_PAIR[dim],
                      "fp64_TFLOPS": pairs * OPS_PER_PAIR[dim] / 1e12,
                      "fraction_of_fp64_vector_peak": pairs * OPS_PER_PAIR[dim] / 1e12 / PEAK_FP64_TFLOPS,
                      "finite": finite}, outf)
    if a.wall_N:
        G = graphs.ErdosRenyi(a.wall_N, p=10.0 / a.wall_N)
        t = time.perf_counter()
        G.set_coordinates()
        wall = time.perf_counter() - t
        c = G.coords
        emit({"case": "set_coordinates_er{}".format(a.wall_N), "N": a.wall_N, "wall_s": wall,
              "device_ms": G.layout_report["kernel_ms"], "shape": list(c.shape), "finite": bool(np.isfinite(c).all()),
              "min": float(c.min()), "max": float(c.max())}, outf)


if __name__ == "__main__":
    main()
