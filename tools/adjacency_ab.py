#!/usr/bin/env python3
"""Every device builder of an adjacency, and the other callers of scan_exclusive, under ONE build of libgspx (the one
GSPX_LIB_PATH names, else the tree's): for comparing two builds of the library, one process each.

    python tools/adjacency_ab.py dump OUT.npz     the CSR arrays of every builder on seeded inputs
    python tools/adjacency_ab.py compare A.npz B.npz   bitwise equality of two dumps (exit status 1 when they differ)
    python tools/adjacency_ab.py time [--repeats 7] [--tag NAME]   one JSON line: median build_ms / kernel_ms

dump: knn_graph (2-D and 8-D), radius_graph, sbm_graph, DeviceGraph.setup with edge_list and components, line_graph,
kron(adjacency=True), learn_log_degrees(adjacency=True) and coarsen, at the sizes of the test suite.  time: build_ms of
knn_graph on bench.py's cloud (10^6 uniform points, k = 8) and of sbm_graph (10^6 vertices, ten blocks), kernel_ms of
coarsen on Sensor(10^6, k=8) under its heavy-edge matching (level 0 of profiles/coarsen_bench.jsonl) and of line_graph
on Sensor(10^5, k=8) (profiles/linegraph_bench.jsonl), each the median of `repeats` calls after two warm-up calls.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def csr(out, name, W):
    W = W.download() if hasattr(W, "download") else W
    out[name + "_indptr"], out[name + "_indices"], out[name + "_data"] = W.indptr, W.indices, W.data


def dump(path):
    from pygsp_amd import engine, graphs, reduction
    ctx, rng, out = engine.default_context(0), np.random.default_rng(5), {}
    X2, X8 = rng.uniform(0, 1, (5000, 2)), rng.uniform(0, 1, (1500, 8))
    W2 = engine.knn_graph(X2, 6, ctx=ctx)[0]
    csr(out, "knn2", W2)
    csr(out, "knn8", engine.knn_graph(X8, 8, ctx=ctx)[0])
    csr(out, "radius2", engine.radius_graph(X2, 0.03, ctx=ctx)[0])
    csr(out, "radius8", engine.radius_graph(X8, 0.6, ctx=ctx)[0])
    z = np.sort(rng.integers(0, 3, 2000))
    M = np.full((3, 3), 0.002) + np.eye(3) * 0.018
    csr(out, "sbm", engine.sbm_graph(z, M, seed=11, ctx=ctx)[0])
    csr(out, "sbm_directed", engine.sbm_graph(z, M, seed=11, ctx=ctx, directed=True, self_loops=True)[0])
    dev = engine.DeviceGraph.setup(W2, coords=X2, order="morton", ctx=ctx)[0]
    csr(out, "setup_L", dev.download_l())
    out["setup_rowptr"], out["setup_col"] = dev.download_internal()
    out["edge_src"], out["edge_dst"], out["edge_w"] = dev.edge_list()
    csr(out, "line", engine.line_graph(dev)[0])
    G = graphs.Sensor(2000, k=10, seed=4)
    gd = G.device_graph()
    lnew, Wk, iters, _ = gd.kron(np.arange(0, G.N, 3), 0.0, rtol=1e-10, adjacency=True)
    out["kron_L"], out["kron_iters"] = lnew, iters
    csr(out, "kron", Wk)
    src = G.get_edge_list()[0]
    zz = rng.uniform(0.2, 1.8, src.size)
    P, _, Wl, _ = gd.learn_log_degrees(zz / zz.mean(), 1.0, 1.0, 0.02, tol=None, maxit=200, adjacency=True)
    out["learn_P"] = np.asarray(P)
    csr(out, "learn", Wl)
    parent, nc = reduction.parent_of(gd.match_heavy_edges()[0])
    csr(out, "coarsen", gd.coarsen(parent, nc)[0])
    out["components"] = dev.components()[1]
    np.savez(path, **out)
    print("dumped", len(out), "arrays to", path)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = [k for k in sorted(set(A.files) | set(B.files))
           if k not in A.files or k not in B.files or A[k].dtype != B[k].dtype or A[k].shape != B[k].shape or A[k].tobytes() != B[k].tobytes()]
    print(json.dumps({"arrays": len(A.files), "differ": bad}))
    return 1 if bad else 0


def time_builders(repeats, tag):
    from pygsp_amd import engine, graphs, reduction
    ctx = engine.default_context(0)
    med = lambda f: float(np.median([f() for _ in range(repeats + 2)][2:]))  # noqa: E731

    def knn():
        W, _, info = engine.knn_graph(coords, 8, ctx=ctx, keep_on_device=True)
        W.close()
        return info["build_ms"]

    def sbm():
        W, ms = engine.sbm_graph(z, M, seed=3, ctx=ctx, keep_on_device=True)
        W.close()
        return ms

    def built(call):
        W, info = call()
        W.close()
        return info["kernel_ms"]

    coords = np.random.default_rng(42).uniform(0, 1, (1000000, 2))
    z = np.sort(np.random.default_rng(1).integers(0, 10, 1000000))
    M = np.full((10, 10), 2e-6) + np.eye(10) * 1.8e-5
    rec = {"library": tag, "repeats": repeats, "knn_build_ms": med(knn), "sbm_build_ms": med(sbm)}
    gd = graphs.Sensor(1000000, k=8, seed=0).device_graph()
    parent, nc = reduction.parent_of(gd.match_heavy_edges()[0])
    rec["coarsen_kernel_ms"] = med(lambda: built(lambda: gd.coarsen(parent, nc)))
    ld = graphs.Sensor(100000, k=8, seed=0).device_graph()
    rec["linegraph_kernel_ms"] = med(lambda: built(lambda: engine.line_graph(ld)))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["dump", "compare", "time"])
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--tag", default=os.environ.get("GSPX_LIB_PATH") or "tree")
    a = ap.parse_args()
    if a.mode == "dump":
        dump(a.paths[0])
    elif a.mode == "compare":
        sys.exit(compare(a.paths[0], a.paths[1]))
    else:
        time_builders(a.repeats, a.tag)
