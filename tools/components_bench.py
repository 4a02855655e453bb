#!/usr/bin/env python3
"""Connected components on the device against the host path they replace: one JSON line per graph.

    python tools/components_bench.py [--vertices 1000000] [--knn 8] [--er-degrees 0.5 1 2] [--reps 3] [--out FILE]

Graphs are built on the device and keep their W there: Sensor(N, k) and ErdosRenyi(N, p = c / N) for every c of
--er-degrees (many components).  Per graph:
  device   is_connected() (the count alone comes back) and connected_components() (count and N int32 labels):
           wall time of the call on a fresh cache (host clock, best of --reps), the rounds run, the library's
           round cap, the device time of the whole call and per round;
  host     what the same two calls cost before: the download of W (once per graph, G.W) plus
           scipy.sparse.csgraph.connected_components on it (best of --reps);
and whether both give the same labels.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best(fn, reps):
    times, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return min(times), out


def measure(name, G, reps):
    from scipy.sparse import csgraph

    def fresh(method):
        def call():
            G._flags.pop("connected", None)
            G._flags.pop("components", None)
            return getattr(G, method)()
        return call

    fresh("is_connected")()  # warm-up: first launches, allocations
    connected_ms, connected = best(fresh("is_connected"), reps)
    count_report = dict(G.components_report)
    labels_ms, (n, labels) = best(fresh("connected_components"), reps)
    report = dict(G.components_report)
    assert G._adj_host is None, "W was downloaded by the device path"
    t0 = time.perf_counter()
    W = G.W
    download_ms = (time.perf_counter() - t0) * 1e3
    scipy_ms, (n_ref, ref) = best(lambda: csgraph.connected_components(W, directed=False), reps)
    return {"graph": name, "vertices": G.N, "stored_entries": int(W.nnz), "components": n,
            "device_is_connected_ms": round(connected_ms, 3), "device_connected_components_ms": round(labels_ms, 3),
            "rounds": report["rounds"], "round_cap": report["round_cap"],
            "kernel_ms": round(report["kernel_ms"], 3), "kernel_ms_count_only": round(count_report["kernel_ms"], 3),
            "kernel_ms_per_round": round(report["kernel_ms"] / max(report["rounds"], 1), 4),
            "host_download_w_ms": round(download_ms, 1), "host_scipy_ms": round(scipy_ms, 1),
            "host_total_ms": round(download_ms + scipy_ms, 1),
            "bytes_device_path": 4 * G.N, "bytes_host_path": int(W.data.nbytes + W.indices.nbytes + W.indptr.nbytes),
            "same_labels": bool(n == n_ref and np.array_equal(labels, ref) and connected == (n_ref == 1))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=1_000_000)
    ap.add_argument("--knn", type=int, default=8)
    ap.add_argument("--er-degrees", type=float, nargs="*", default=[0.5, 1.0, 2.0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from pygsp_amd import graphs
    outf = open(a.out, "a") if a.out else None
    N = a.vertices
    cases = [("sensor_k{}".format(a.knn), lambda: graphs.Sensor(N, k=a.knn, seed=0))]
    cases += [("er_p{:g}/N".format(c), lambda c=c: graphs.ErdosRenyi(N=N, p=c / N, seed=1)) for c in a.er_degrees]
    for name, build in cases:
        line = json.dumps(measure(name, build(), a.reps))
        print(line, flush=True)
        if outf:
            outf.write(line + "\n")
            outf.flush()


if __name__ == "__main__":
    main()
