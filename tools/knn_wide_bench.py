#!/usr/bin/env python3
"""Neighbour-graph construction beyond 64 dimensions (profiles/knn_wide.md): engine.knn_graph at N = 100k, k = 10 in
64 (the narrow build), 128, 256 and 1024 dimensions beside scipy's cKDTree on the same host.  Needs a GPU.

usage: tools/knn_wide_bench.py wide          build_ms (median of 5 after a warm-up; default sweep, and fp64 forced),
                                             search statistics, cKDTree (300 query rows, scaled to N), identity check
       tools/knn_wide_bench.py narrow        the 100k x 16 cloud of tests/test_gpu_5_knn.py::test_highdim_scale, 5 runs
                                             (GSPX_LIB_PATH names another build of the library to compare with)
       tools/knn_wide_bench.py one D         two builds per sweep precision at dimension D: the workload for a
                                             `rocprofv3 --kernel-trace --stats` or `--pmc` run of its own
One JSON line per record."""
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pygsp_amd import _capi, engine  # noqa: E402

N, K = 100000, 10


def search_stats(ctx, X, k):
    lib = _capi.load()
    h = ctypes.c_void_p()
    _capi.check(lib.gspx_knn_build(ctx._h, X.shape[0], X.shape[1], _capi.ptr(X), k, 0.0, 0, 0, ctypes.byref(h)))
    out = np.zeros(4)
    _capi.check(lib.gspx_knn_search_stats(h, _capi.ptr(out)))
    lib.gspx_knn_destroy(h)
    return dict(sample=int(out[0]), capacity=int(out[1]), mean_candidates=float(out[2]), exact_scans=int(out[3]))


def build_times(ctx, X, n):
    engine.knn_graph(X, K, ctx=ctx)  # warm-up
    return [engine.knn_graph(X, K, ctx=ctx)[2]["build_ms"] for _ in range(n)]


def cloud(d):
    return np.ascontiguousarray(np.random.default_rng(d).standard_normal((N, d)))


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "wide"
    ctx = engine.default_context(0)
    if mode == "narrow":
        rng = np.random.default_rng(1)
        X = rng.standard_normal((N, 16))
        X = np.ascontiguousarray(X[np.argsort(X[:, 0])])
        r = build_times(ctx, X, 5)
        print(json.dumps({"mode": "narrow", "lib": _capi.LIB_PATH, "build_ms": r, "median": float(np.median(r))}),
              flush=True)
    elif mode == "wide":
        from scipy import spatial
        for d in (64, 128, 256, 1024):
            X = cloud(d)
            rec = {"mode": "wide", "N": N, "k": K, "d": d}
            for f32 in (1, 0):
                ctx.set_option("knn_f32", f32)
                r = build_times(ctx, X, 5 if f32 else 3)
                rec["build_ms_f32opt%d" % f32], rec["median_f32opt%d" % f32] = r, float(np.median(r))
            ctx.set_option("knn_f32", 1)
            rec["stats"] = search_stats(ctx, X, K)
            t0 = time.perf_counter()
            W, sg, info = engine.knn_graph(X, K, ctx=ctx, neighbors=True)
            rec["wall_s_with_download"] = time.perf_counter() - t0
            rows = np.random.default_rng(0).choice(N, 300, replace=False)
            t0 = time.perf_counter()
            tree = spatial.cKDTree(X)
            t1 = time.perf_counter()
            D, NN = tree.query(X[rows], k=K + 1)
            t2 = time.perf_counter()
            rec["ckdtree_build_s"], rec["ckdtree_query300_s"] = t1 - t0, t2 - t1
            rec["ckdtree_scaled_to_N_s"] = (t2 - t1) * N / 300 + (t1 - t0)
            rec["equal_to_ckdtree"] = bool(np.array_equal(info["NN"][rows], NN[:, 1:])
                                           and np.array_equal(info["D"][rows], D[:, 1:]))
            print(json.dumps(rec), flush=True)
    elif mode == "one":
        X = cloud(int(sys.argv[2]))
        for f32 in (1, 0):
            ctx.set_option("knn_f32", f32)
            engine.knn_graph(X, K, ctx=ctx)
            engine.knn_graph(X, K, ctx=ctx)
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
