#!/usr/bin/env python3
"""Graph learning on the device (pygsp_amd.graph_learning) measured step by step: one JSON line per workload.

    python tools/graphlearn_bench.py [--points 1000000] [--cloud 100000 64] [--k 8] [--candidates 24]
                                     [--numpy-iterations 3] [--out FILE]

Workloads: uniform 2-D points (Sensor-style) and a standard normal cloud of --cloud points x dimensions.  Per workload
the steps of graphs.LearnedGraph are run one by one: the candidate k-NN pattern on the device, theta for k from the
builder's sorted distances, z on the device, the solver to tol 1e-5.  Reported: E, iterations, device ms per iteration
(events around the loop, polls included), the bytes one iteration moves - counted here from E and N, `compulsory` (every
array once) and `nominal` (every gather counted as a miss) -, the resulting GB/s beside gspx_bench_read of the same run,
the wall time of the call, and the time per iteration of the numpy restatement (tests/graphlearn_helpers.py) on this
host at the same size.  An iteration is three launches (edge pass, vertex pass, rule kernel); the host reads the done
flag every 4 iterations.
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


def iteration_bytes(E, N):
    """Bytes of one iteration of gspx_learn_log_degrees_dev (csrc/gspx_graphlearn.hip.h), per pass."""
    edge = {"stream": 16 * E + 8 * E + 8 * E + 16 * E,  # (w, P) read, z, endpoints, (w, P) written
            "gather_compulsory": 16 * N, "gather_nominal": 32 * E}  # (v, p) of both endpoints
    vertex = {"stream": 8 * N + 4 * E + 2 * 16 * N + 2 * 8 * N,  # offsets, tedge, (v, p) and d read and written
              "gather_compulsory": 16 * E, "gather_nominal": 32 * E}  # (w, P) of every edge from both of its ends
    comp = edge["stream"] + edge["gather_compulsory"] + vertex["stream"] + vertex["gather_compulsory"]
    nom = edge["stream"] + edge["gather_nominal"] + vertex["stream"] + vertex["gather_nominal"]
    return {"edge_pass": edge, "vertex_pass": vertex, "compulsory": comp, "nominal": nom}


def measure(name, X, k, candidates, numpy_iterations):
    import graphlearn_helpers as gl
    from pygsp_amd import engine, graph_learning, graphs

    ctx = engine.default_context(0)
    N = X.shape[0]
    t0 = time.perf_counter()
    pattern, _, found = engine.knn_graph(X, candidates, ctx=ctx, neighbors=True, symmetrize="maximum",
                                         keep_on_device=True)
    knn_ms = (time.perf_counter() - t0) * 1e3
    lo, hi = graph_learning.theta_bounds(found["D"], k)
    theta = float(np.sqrt(lo * hi))
    base = graphs.Graph(pattern, reorder="none", tiles=False, ctx=ctx)
    dev = base.device_graph()
    src, dst, _ = dev.edge_list()
    E = src.size
    dmax = int((np.bincount(src, minlength=N) + np.bincount(dst, minlength=N)).max())
    gamma = 0.5 / (2.0 + np.sqrt(2.0 * dmax))
    xd = engine.DeviceArray.from_host(ctx, X * np.sqrt(theta))
    dev.edge_sqdist(xd)  # warm-up
    t0 = time.perf_counter()
    zd = dev.edge_sqdist(xd)
    ctx.sync()
    sqdist_ms = (time.perf_counter() - t0) * 1e3
    dev.learn_log_degrees(zd, 1.0, 1.0, gamma, tol=None, maxit=8)  # warm-up
    t0 = time.perf_counter()
    P, _, W, info = dev.learn_log_degrees(zd, 1.0, 1.0, gamma, tol=1e-5, maxit=20000, adjacency=True)
    wall_ms = (time.perf_counter() - t0) * 1e3
    fixed = dev.learn_log_degrees(zd, 1.0, 1.0, gamma, tol=None, maxit=200)[3]  # 200 iterations, 49 polls
    nnz = W.nnz
    read_gbps = ctx.bench_read(1 << 30)
    by = iteration_bytes(E, N)
    ms_it = info["ms"] / max(info["niter"], 1)
    z = np.asarray(zd)
    t0 = time.perf_counter()
    gl.solve(src.astype(np.int64), dst.astype(np.int64), N, z, 1.0, 1.0, gamma, tol=None, maxit=numpy_iterations)
    numpy_ms_it = (time.perf_counter() - t0) * 1e3 / numpy_iterations
    return {"workload": name, "vertices": N, "features": X.shape[1], "k": k, "candidates": candidates, "theta": theta,
            "edges": int(E), "max_degree": dmax, "gamma": gamma, "knn_build_wall_ms": round(knn_ms, 1),
            "edge_sqdist_wall_ms": round(sqdist_ms, 3), "iterations_to_tol_1e-5": info["niter"], "crit": info["crit"],
            "device_ms": round(info["ms"], 3), "device_ms_per_iteration": round(ms_it, 5),
            "device_ms_per_iteration_200_fixed": round(fixed["ms"] / 200, 5),
            "call_wall_ms_with_adjacency": round(wall_ms, 2), "launches_per_iteration": 3, "poll_every": 4,
            "bytes_per_iteration": by, "gbps_compulsory": round(by["compulsory"] / ms_it / 1e6, 1),
            "gbps_nominal": round(by["nominal"] / ms_it / 1e6, 1), "bench_read_gbps": round(read_gbps, 1),
            "learned_edges": int(nnz // 2), "mean_neighbours": round(nnz / N, 3),
            "numpy_ms_per_iteration": round(numpy_ms_it, 2), "speedup_per_iteration": round(numpy_ms_it / ms_it, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--cloud", type=int, nargs=2, default=[100_000, 64])
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--candidates", type=int, default=24)
    ap.add_argument("--numpy-iterations", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    cases = []
    if a.points > 0:
        cases.append(("sensor_2d", lambda: rng.uniform(0, 1, (a.points, 2))))
    if a.cloud[0] > 0:
        cases.append(("cloud_{}d".format(a.cloud[1]), lambda: rng.standard_normal((a.cloud[0], a.cloud[1]))))
    outf = open(a.out, "a") if a.out else None
    for name, make in cases:
        line = json.dumps(measure(name, make(), a.k, a.candidates, a.numpy_iterations))
        print(line, flush=True)
        if outf:
            outf.write(line + "\n")
            outf.flush()


if __name__ == "__main__":
    main()
