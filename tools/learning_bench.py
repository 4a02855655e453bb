#!/usr/bin/env python3
"""classification_tikhonov_simplex benchmark on the device: one JSON line per case.

    python tools/learning_bench.py [--N 1000000] [--classes 2 4 10] [--host-N 100000] [--host-iters 20] [--out FILE]

Sensor(N, seed=0), 10 % of the vertices measured (seeded), random labels.  Per number of classes C, two solver runs
(after a warm-up): the default rule (rtol 1e-3) and a fixed 200 iterations (every other criterion off), each with the
device time of the whole call (DeviceGraph.tikhonov_simplex's ms: labels, X_0, the loop, the permutation back) and
that time over the iterations.  In the same run: L X alone on an N x C panel (gspx_laplacian_apply_dev, best of 5) and
the read-only rate of ctx.bench_read, so that an iteration can be set against its parts:
  step kernel bytes   4 panels read (X_{k-1}, X_{k-2}, L X_{k-1}, L X_{k-2}), 1 written (X_k), 4 N bytes of labels
  product bytes       1 panel read, 1 written, the CSR (12 bytes per stored entry + 4 N of row pointers)
  model_ms            L X time + step kernel bytes / bench_read rate;  target: iteration <= 1.5 model_ms
The host line times the numpy restatement of the iteration (tests/learning_helpers.py) at --host-N, per iteration.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def emit(rec, outf):
    line = json.dumps(rec)
    print(line, flush=True)
    if outf:
        outf.write(line + "\n")
        outf.flush()


def problem(N, C, seed=0):
    rng = np.random.default_rng(seed + 1)
    M = rng.random(N) < 0.1
    y = rng.integers(0, C, N).astype(float)
    y[M] = rng.permutation(np.arange(M.sum()) % C)  # (every class present)
    return y, M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1_000_000)
    ap.add_argument("--classes", type=int, nargs="+", default=[2, 4, 10])
    ap.add_argument("--tau", type=float, default=0.5)
    ap.add_argument("--host-N", type=int, default=100_000)
    ap.add_argument("--host-iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from pygsp_amd import graphs, learning
    outf = open(a.out, "a") if a.out else None
    G = graphs.Sensor(a.N, seed=0)
    G.estimate_lmax()
    dev = G.device_graph(np.float64)
    N = G.N
    nnz = int(G.W.nnz) + N  # stored entries of L: the edges both ways and the diagonal
    read_gbps = dev.ctx.bench_read(1 << 30, passes=10)
    for C in a.classes:
        y, M = problem(N, C)
        panel = 8.0 * N * C
        step_bytes = 5 * panel + 4.0 * N
        product_bytes = 2 * panel + 12.0 * nnz + 4.0 * N
        bx, by = dev.ctx.alloc(int(panel)), dev.ctx.alloc(int(panel))
        try:
            dev.ctx.identity_panel(bx, N, 0, C, np.float64)
            lx_ms = min(dev.laplacian_apply_dev(bx.ptr, by.ptr, C) for _ in range(6))
        finally:
            bx.free()
            by.free()
        model_ms = lx_ms + step_bytes / (read_gbps * 1e9) * 1e3
        learning.simplex_solve(G, y, M, a.tau, rtol=None, maxit=5)  # warm-up
        for rule, opts in (("default", {}), ("maxit200", dict(rtol=None, maxit=200))):
            t = time.perf_counter()
            _, info = learning.simplex_solve(G, y, M, a.tau, **opts)
            wall = time.perf_counter() - t
            per_it = info["ms"] / info["niter"]
            emit({"case": "simplex_sensor{}_C{}_{}".format(N, C, rule), "N": N, "C": C, "tau": a.tau,
                  "niter": info["niter"], "crit": info["crit"], "device_ms": info["ms"], "wall_s": wall,
                  "ms_per_iteration": per_it, "lx_ms": lx_ms, "bench_read_GBps": read_gbps,
                  "step_kernel_bytes": step_bytes, "product_bytes": product_bytes, "model_ms": model_ms,
                  "iteration_vs_model": per_it / model_ms,
                  "iteration_GBps_model_bytes": (step_bytes + product_bytes) / (per_it * 1e-3) / 1e9}, outf)
    # the host baseline: the numpy restatement, fixed iterations
    import learning_helpers as lh
    H = graphs.Sensor(a.host_N, seed=0)
    H.estimate_lmax()
    L = H.L.tocsr().astype(np.float64)
    for C in (4,):
        y, M = problem(H.N, C)
        labels, n = learning.simplex_labels(y, M)
        t = time.perf_counter()
        lh.solve(L, labels, n, a.tau, learning.simplex_step(H, a.tau), rtol=None, maxit=a.host_iters)
        wall = time.perf_counter() - t
        emit({"case": "host_numpy_sensor{}_C{}".format(H.N, C), "N": H.N, "C": C, "iterations": a.host_iters,
              "wall_s": wall, "ms_per_iteration": wall / a.host_iters * 1e3}, outf)


if __name__ == "__main__":
    main()
