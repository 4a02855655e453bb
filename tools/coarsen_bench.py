#!/usr/bin/env python3
"""Graph coarsening and pooling on the device (pygsp_amd.reduction.coarsen, engine.segment_pool) measured level by
level: one JSON line per record.

    python tools/coarsen_bench.py [--points 1000000] [--k 8] [--levels 3] [--repeats 7] [--no-host] [--out FILE]

Workload: Sensor(points, k), `levels` levels of heavy-edge matching.  Per level a "level" record: vertices, stored
entries, rounds, the matched share of the vertices, the device time of the matching and of the coarse-graph build
(kernel_ms of gspx_match_heavy_edges / gspx_coarsen_build), the wall time of reduction.coarsen's whole level (set-up of
the coarse graph included), and - unless --no-host - the wall time of the numpy restatements
(reduction.heavy_edge_matching_host, reduction.coarsen_host) and of scipy's P^T W P on this host, all on the same graph.
Per level, width (32, 64) and dtype (float32, float64) a "pool" record: the median kernel_ms of gspx_segment_pool_dev
(max) and of its vjp, the GB/s over the bytes they must move (pool: read N x width, write Nc x width; vjp of max: read
N x width and Nc x width, write N x width), gspx_bench_read of the same run, and the same pooling composed from
torch.index_select and amax on the same GPU in the same process (CUDA events, median), forward only.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

try:  # torch before libgspx (pygsp_amd.nn's import order), when it is there
    import pygsp_amd.nn  # noqa: F401
    import torch
except ImportError:
    torch = None

import numpy as np  # noqa: E402
from scipy import sparse  # noqa: E402


def median(values):
    return float(np.median(np.asarray(values, dtype=np.float64)))


def torch_pool_ms(parent, n_coarse, n_fine, width, dtype, repeats):
    """index_select of a padded (cluster, member) table and amax over the members: median ms by CUDA events."""
    if torch is None or not torch.cuda.is_available():
        return None
    order = np.argsort(parent, kind="stable")
    sizes = np.bincount(parent, minlength=n_coarse)
    start = np.r_[0, np.cumsum(sizes)[:-1]]
    most = int(sizes.max())
    slot = np.minimum(np.arange(most)[None, :], sizes[:, None] - 1)
    table = torch.from_numpy(order[start[:, None] + slot].reshape(-1)).cuda()
    x = torch.randn((n_fine, width), dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    times = []
    for _ in range(repeats + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        y = torch.index_select(x, 0, table).reshape(n_coarse, most, width).amax(dim=1)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    del y
    return median(times[2:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from pygsp_amd import engine, graphs, reduction

    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    t0 = time.perf_counter()
    G = graphs.Sensor(args.points, k=args.k, seed=0)
    ctx = G.context
    emit({"record": "graph", "points": args.points, "k": args.k, "vertices": G.N, "edges": int(G.n_edges),
          "setup_s": time.perf_counter() - t0})
    Gs, parents = [G], []
    for level in range(args.levels):
        fine = Gs[-1]
        t0 = time.perf_counter()
        C = reduction.coarsen(fine, levels=1)
        wall = time.perf_counter() - t0
        info, parent, coarse = C.info[0], C.parents[0], C.graphs[1]
        rec = {"record": "level", "level": level, "vertices": fine.N, "coarse_vertices": coarse.N,
               "rounds": info["rounds"], "pairs": info["pairs"], "matched_share": 2.0 * info["pairs"] / fine.N,
               "match_kernel_ms": info["kernel_ms"], "build_kernel_ms": info["build_kernel_ms"],
               "coarsen_wall_ms": wall * 1e3}
        if not args.no_host:
            W = sparse.csr_matrix(fine.W, dtype=np.float64)
            rec["stored_entries"] = int(W.nnz)
            d = fine.device_graph(np.float64).download_dw()
            t0 = time.perf_counter()
            mate, rounds, pairs = reduction.heavy_edge_matching_host(W, d)
            rec["match_host_ms"] = (time.perf_counter() - t0) * 1e3
            rec["host_equals_device"] = bool(np.array_equal(reduction.parent_of(mate)[0], parent) and
                                             rounds == info["rounds"])
            t0 = time.perf_counter()
            Wc = reduction.coarsen_host(W, parent)
            rec["build_host_ms"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            P = sparse.csr_matrix((np.ones(fine.N), (np.arange(fine.N), parent)), shape=(fine.N, coarse.N))
            S = sparse.csr_matrix(P.T @ W @ P)
            S.setdiag(0)
            S.eliminate_zeros()
            rec["build_scipy_ms"] = (time.perf_counter() - t0) * 1e3
            Wd = sparse.csr_matrix(coarse.W)
            rec["build_equals_host"] = bool(np.array_equal(Wd.indptr, Wc.indptr) and np.array_equal(Wd.indices, Wc.indices)
                                            and np.array_equal(Wd.data, Wc.data))
        emit(rec)
        Gs.append(coarse)
        parents.append(parent)

    read_gbps = ctx.bench_read(1 << 30)
    emit({"record": "bench_read", "gbps": read_gbps})
    for level, parent in enumerate(parents):
        n_fine, n_coarse = Gs[level].N, Gs[level + 1].N
        seg = engine.Segments.from_parent(ctx, parent, n_coarse)
        for dtype in (np.float32, np.float64):
            item = np.dtype(dtype).itemsize
            for width in (32, 64):
                x = engine.DeviceArray.from_host(ctx, np.random.default_rng(0).standard_normal((n_fine, width)), dtype)
                y = engine.DeviceArray.empty(ctx, (n_coarse, width, 1), dtype)
                gx = engine.DeviceArray.empty(ctx, (n_fine, width, 1), dtype)
                fwd = [engine.segment_pool_dev(ctx, seg, "max", dtype, width, x.ptr, y.ptr)
                       for _ in range(args.repeats + 2)][2:]
                bwd = [engine.segment_pool_vjp_dev(ctx, seg, "max", dtype, width, x.ptr, y.ptr, gx.ptr)
                       for _ in range(args.repeats + 2)][2:]
                fbytes = (n_fine + n_coarse) * width * item
                bbytes = (2 * n_fine + n_coarse) * width * item
                tms = torch_pool_ms(parent, n_coarse, n_fine, width, dtype, args.repeats)
                emit({"record": "pool", "level": level, "dtype": np.dtype(dtype).name, "width": width,
                      "vertices": n_fine, "coarse_vertices": n_coarse, "pool_ms": median(fwd),
                      "pool_gbps": fbytes / median(fwd) / 1e6, "vjp_ms": median(bwd),
                      "vjp_gbps": bbytes / median(bwd) / 1e6, "bench_read_gbps": read_gbps, "torch_ms": tms,
                      "torch_gbps": None if not tms else fbytes / tms / 1e6})
                for a in (x, y, gx):
                    a.free()
    if args.out:
        with open(args.out, "w") as f:
            for rec in records:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
