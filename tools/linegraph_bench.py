#!/usr/bin/env python3
"""Line graphs on the device against the host construction they replace: one JSON line per size.

    python tools/linegraph_bench.py [--vertices 10000 100000 1000000] [--knn 8] [--reps 5] [--host-max 100000]
                                    [--out FILE]

Per size, G = Sensor(N, k) built on the device.  After one warm-up of each step, --reps timed runs of
  builder     engine.line_graph(G.device_graph()): kernel_ms (device events around the length pass, the scan and the
              fill) and the wall time of the call (host clock; the call ends in a stream synchronise);
  line graph  graphs.LineGraph(G): the builder plus the set-up of LG on the adjacency where it lies (checks, vertex
              order, Laplacian, gather tiles) and the midpoint coordinates - wall time;
  host        for N <= --host-max: graphs.line_graph_host on G.get_edge_list() (scipy: indicator matrix, sparse
              product, minus the identity - the reference's construction) followed by graphs.Graph(W, coords) - wall
              time, and whether the device adjacency equals the host one.
Each figure is reported as median, minimum and maximum over the runs.  `fill_bytes` is the byte model of the fill
kernel: 12 bytes (one int32 column, one float64 value) per stored entry; the fill kernel's own time comes from a
kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tools/linegraph_bench.py ...), not from here.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(values):
    return {"median": round(float(np.median(values)), 3), "min": round(float(min(values)), 3),
            "max": round(float(max(values)), 3)}


def timed(fn, reps):
    """Wall times in ms of `reps` runs of fn after one warm-up run, and the last result."""
    out = fn()
    times = []
    for _ in range(reps):
        del out
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return times, out


def measure(N, k, reps, with_host):
    from pygsp_amd import engine, graphs
    G = graphs.Sensor(N, k=k, seed=0)
    dev = G.device_graph()
    n_vertices, nnz = engine.line_graph_size(dev)
    kernel_ms = []

    def builder():
        W, info = engine.line_graph(dev)
        kernel_ms.append(info["kernel_ms"])
        return W

    builder_ms, W = timed(builder, reps)
    W.close()
    linegraph_ms, LG = timed(lambda: graphs.LineGraph(G), reps)
    row = {"vertices": N, "knn": k, "edges": int(G.n_edges), "line_graph_vertices": n_vertices,
           "line_graph_stored_entries": nnz, "fill_bytes": 12 * nnz, "reps": reps,
           "kernel_ms": spread(kernel_ms[1:]), "builder_wall_ms": spread(builder_ms),
           "line_graph_wall_ms": spread(linegraph_ms), "reordered": bool(LG.setup_report["reordered"]),
           "tiles": LG.tile_stats is not None}
    if with_host:
        sources, targets, _ = G.get_edge_list()

        def host():
            adjacency, touches = graphs.line_graph_host(sources, targets, G.N)
            return graphs.Graph(adjacency, coords=touches.dot(G.coords) / 2)

        host_ms, HG = timed(host, max(1, min(reps, 3)))
        row["host_scipy_then_graph_wall_ms"] = spread(host_ms)
        A, B = LG.W, HG.W
        row["same_adjacency"] = bool(np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
                                     and np.array_equal(A.data, B.data))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, nargs="*", default=[10_000, 100_000, 1_000_000])
    ap.add_argument("--knn", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-max", type=int, default=100_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    outf = open(a.out, "a") if a.out else None
    for N in a.vertices:
        line = json.dumps(measure(N, a.knn, a.reps, N <= a.host_max))
        print(line, flush=True)
        if outf:
            outf.write(line + "\n")
            outf.flush()


if __name__ == "__main__":
    main()
