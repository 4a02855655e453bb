#!/usr/bin/env python3
"""k-means and spectral clustering on the device (pygsp_amd.clustering) measured: one JSON line per record.

    python tools/cluster_bench.py [--points 1000000] [--iters 10] [--repeats 5] [--sizes 100000,1000000]
                                  [--clusters 16] [--no-kernels] [--no-e2e] [--torch-only] [--out FILE]

"kmeans" records, one per (d, C) in {16, 25, 64} x {8, 64} on `points` Gaussian rows (balanced clusters; real
embeddings are not): the device time (kernel_ms of gspx_kmeans_dev, HIP events around the whole loop, the host's look
at the changed count each iteration included) of one assignment alone (max_iter = 0) and of `iters` iterations, best
of `repeats` after a warm-up call each.  From them: assign_ms (the max_iter = 0 call), iter_ms = (the long call -
assign_ms) / updates made, update_ms = iter_ms - assign_ms; the assignment's 3 N C d flops per second beside the fp64
vector peak (78.6 TFLOP/s counts a fused multiply-add as two; the kernel may fuse nothing, so half of it is its
ceiling), and the update's one read of X beside gspx_bench_read of the same run.
"e2e" records: the wall time of clustering.spectral_clustering(Sensor(N, k = 8), clusters, features) for both feature
kinds (the Fourier basis is computed inside the first call and timed with it; a solver that raises is recorded as
"failed"), split into embedding and k-means, and the wall time of scipy.cluster.vq.kmeans2(minit='++') on the downloaded
row-normalised features on this host.
--torch-only (a process of its own, so that torch and libgspx do not share one): "torch" records, one Lloyd iteration
as torch.cdist + argmin + index_add_ in fp64 on the same card, CUDA events, best of `repeats`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SHAPES = [(d, c) for d in (16, 25, 64) for c in (8, 64)]
FP64_VECTOR_PEAK_TFLOPS = 78.6


def torch_records(points, repeats, emit):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("--torch-only needs a GPU")
    for d, c in SHAPES:
        x = torch.randn((points, d), dtype=torch.float64, device="cuda")
        cent = x[:c].clone()
        times = []
        for _ in range(repeats + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            labels = torch.cdist(x, cent).argmin(dim=1)
            sums = torch.zeros((c, d), dtype=torch.float64, device="cuda").index_add_(0, labels, x)
            counts = torch.bincount(labels, minlength=c).clamp(min=1)
            new = sums / counts[:, None]
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        del new
        emit({"record": "torch", "points": points, "d": d, "clusters": c, "iter_ms": min(times[2:])})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--clusters", type=int, default=16)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--torch-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    if args.torch_only:
        torch_records(args.points, args.repeats, emit)
    else:
        from pygsp_amd import clustering, engine, graphs
        ctx = engine.default_context()
        if not args.no_kernels:
            read_gbps = ctx.bench_read(1 << 30)
            emit({"record": "bench_read", "gbps": read_gbps})
            N = args.points
            for d, c in SHAPES:
                rows = np.random.default_rng(d).standard_normal((N, d))
                X, init = engine.DeviceArray.from_host(ctx, rows), rows[:c].copy()

                def run(max_iter):
                    best = None
                    for _ in range(args.repeats + 1):  # (the first call warms up)
                        res = clustering.kmeans_dev(ctx, X.ptr, N, d, d, c, init=init, max_iter=max_iter)
                        best = res if best is None or res.kernel_ms < best.kernel_ms else best
                    return best
                one, many = run(0), run(args.iters)
                assign_ms = one.kernel_ms
                iter_ms = (many.kernel_ms - assign_ms) / max(many.n_iter, 1)
                update_ms = iter_ms - assign_ms
                tflops = 3.0 * N * c * d / assign_ms / 1e9
                emit({"record": "kmeans", "points": N, "d": d, "clusters": c, "updates": many.n_iter,
                      "converged": many.converged, "assign_ms": assign_ms, "iter_ms": iter_ms, "update_ms": update_ms,
                      "assign_tflops": tflops, "assign_share_of_fp64_vector_peak": tflops / FP64_VECTOR_PEAK_TFLOPS,
                      "update_read_gbps": N * d * 8 / update_ms / 1e6, "bench_read_gbps": read_gbps,
                      "assign_rows": clustering.assign_rows(d), "update_rows": clustering.update_rows()})
                X.free()
        if not args.no_e2e:
            from scipy.cluster.vq import kmeans2
            k = args.clusters
            for N in [int(v) for v in args.sizes.split(",") if v]:
                t0 = time.perf_counter()
                G = graphs.Sensor(N, k=8, seed=0)
                G.estimate_lmax()
                emit({"record": "graph", "vertices": G.N, "setup_s": time.perf_counter() - t0})
                for kind in ("fourier", "compressive"):
                    t0 = time.perf_counter()
                    try:
                        res = clustering.spectral_clustering(G, k, features=kind)
                    except ValueError as err:
                        emit({"record": "e2e", "vertices": G.N, "features": kind, "clusters": k, "failed": str(err)})
                        continue
                    whole = time.perf_counter() - t0
                    t0 = time.perf_counter()
                    F = clustering.spectral_embedding(G, k, kind)
                    ctx.sync()
                    embed = time.perf_counter() - t0  # (a second embedding: the Fourier basis is there by now)
                    clustering.rows_normalize_dev(ctx, F.ptr, *F.shape)
                    t0 = time.perf_counter()
                    again = clustering.kmeans(F, k)
                    km = time.perf_counter() - t0
                    host = np.asarray(F).reshape(F.shape)
                    t0 = time.perf_counter()
                    kmeans2(host, k, minit="++", seed=0)
                    scipy_s = time.perf_counter() - t0
                    emit({"record": "e2e", "vertices": G.N, "features": kind, "clusters": k, "d": F.shape[1], "lambda_k": res.lambda_k,
                          "spectral_clustering_s": whole, "embedding_again_s": embed, "kmeans_s": km,
                          "kmeans_kernel_ms": again.kernel_ms, "n_iter": again.n_iter, "converged": again.converged,
                          "inertia": again.inertia, "scipy_kmeans2_s": scipy_s})
                    F.free()
    if args.out:
        with open(args.out, "a") as f:
            for rec in records:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
