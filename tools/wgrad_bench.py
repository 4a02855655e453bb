#!/usr/bin/env python3
"""The edge-weight gradient of a Chebyshev filter on the device: one JSON line per invocation.

    python tools/wgrad_bench.py [--n 1000000] [--k 8] [--signals 64] [--order 30] [--dtype float64] [--candidates 24]
                                [--reps 5] [--once] [--out FILE]
    python tools/wgrad_bench.py --torch-baseline [--n 200000] ...

One invocation measures Sensor(n, k, seed 0) with resident signals, one filter, after two warm-up calls of every shape,
`reps` timed calls each; every time is the call's own device time (events around its launches), median and minimum:

  forward_ms    gspx_cheby_filter_dev, analysis
  vjp_ms        the two existing gradients: the synthesis call on the cotangent plus gspx_cheby_cross_moments_dev
  own_ms        gspx_cheby_laplacian_grad_dev on the graph's own edges, gdiag and goff; own_steps_ms its M - 2 recurrence
                steps and own_hook_ms everything after them (the copy of the cotangent, the M - 1 Clenshaw steps, and
                k_pair_cross / k_row_cross after each: the "combine" phase of ctx.last_timing())
  cand_ms       the same call on the candidate pattern: the edges of Sensor(n, candidates, seed 0), the same points
  pair_bytes    what k_pair_cross reads per order, counted from the shapes: four rows of the batch per pair and the two
                indices; row_bytes: the two panels k_row_cross streams
  bench_read_GBps  the read-only stream rate ctx.bench_read measures in the same run

The split of own_hook_ms per kernel comes from a kernel trace of this script with --once (one call of each shape):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o stats -- python tools/wgrad_bench.py --once

--torch-baseline: the same gradient from torch.sparse autograd on the GPU (the weights a leaf, L assembled as a sparse
COO tensor, the recurrence by torch.sparse.mm), wall time of forward + backward around synchronisations and the peak
memory torch reports; run it in a process of its own, at an n that fits."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(reps, call):
    """Device ms of `reps` calls after two warm-ups: (median, min)."""
    for _ in range(2 if reps > 1 else 0):
        call()
    t = [float(call()) for _ in range(reps)]
    return statistics.median(t), min(t)


def torch_baseline(a):
    sys.path.insert(0, ROOT)
    import pygsp_amd.nn  # noqa: F401 (torch first: one HIP runtime in the process)
    import numpy as np
    import torch
    from pygsp_amd import graphs
    dtype = np.dtype(a.dtype)
    tdtype = torch.float64 if dtype == np.float64 else torch.float32
    G = graphs.Sensor(a.n, k=a.k, seed=0)
    G.estimate_lmax("bounds")
    s, t, w0 = G.get_edge_list()
    N, M, lmax = G.N, a.order + 1, float(G.lmax)
    rng = np.random.default_rng(0)
    c = torch.from_numpy(rng.standard_normal(M) * 0.8 ** np.arange(M)).to("cuda", tdtype)
    x = torch.from_numpy(rng.standard_normal((N, a.signals))).to("cuda", tdtype)
    cot = torch.from_numpy(rng.standard_normal((N, a.signals))).to("cuda", tdtype)
    st, tt = torch.from_numpy(s.astype(np.int64)).cuda(), torch.from_numpy(t.astype(np.int64)).cuda()
    diag = torch.arange(N, device="cuda")
    idx = torch.stack([torch.cat([diag, st, tt]), torch.cat([diag, tt, st])])
    w = torch.from_numpy(w0).to("cuda", tdtype).requires_grad_()
    rec = {"case": "wgrad_torch_sparse_sensor{}_k{}_w{}_order{}_{}".format(N, a.k, a.signals, a.order, dtype.name),
           "N": N, "edges": int(s.size), "signals": a.signals, "order": a.order, "torch": torch.__version__}

    def once():
        w.grad = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = torch.zeros(N, dtype=tdtype, device="cuda").index_add(0, st, w).index_add(0, tt, w)
        # Lt = (2 / lmax) L - I, L = D - W
        vals = torch.cat([(2.0 / lmax) * d - 1.0, (-2.0 / lmax) * w, (-2.0 / lmax) * w])
        Lt = torch.sparse_coo_tensor(idx, vals, (N, N)).coalesce()
        T0, T1 = x, torch.sparse.mm(Lt, x)
        y = 0.5 * c[0] * T0 + c[1] * T1
        for k in range(2, M):
            T0, T1 = T1, 2.0 * torch.sparse.mm(Lt, T1) - T0
            y = y + c[k] * T1
        (y * cot).sum().backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    try:
        torch.cuda.reset_peak_memory_stats()
        med, low = timed(a.reps, once)
        rec.update(forward_backward_ms=med, forward_backward_ms_min=low,
                   peak_bytes=int(torch.cuda.max_memory_allocated()), grad_abs_max=float(w.grad.abs().max()))
    except Exception as e:  # (a size that does not fit, an operator torch.sparse does not differentiate: the record says so)
        rec["error"] = "{}: {}".format(type(e).__name__, str(e)[:300])
    return rec


def engine_run(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    from pygsp_amd import _capi, engine, graphs
    dtype = np.dtype(a.dtype)
    G = graphs.Sensor(a.n, k=a.k, seed=0, compute_dtype=dtype.type)
    G.estimate_lmax("bounds")
    dev = G.device_graph(dtype.type)
    ctx, N, w, M = dev.ctx, G.N, a.signals, a.order + 1
    cs, ct, _ = graphs.Sensor(a.n, k=a.candidates, seed=0).get_edge_list()
    cand = np.ascontiguousarray(np.stack([cs, ct]), dtype=np.int32)
    E, P = dev.n_edges(), cand.shape[1]
    rng = np.random.default_rng(0)
    c = rng.standard_normal((1, M)) * 0.8 ** np.arange(M)
    x = G.to_device(rng.standard_normal((N, w)))
    y = engine.DeviceArray.empty(ctx, (N, w, 1), dtype)
    gx = engine.DeviceArray.empty(ctx, (N, w, 1), dtype)
    bp, bd, bo = ctx.upload(cand), ctx.alloc(8 * N), ctx.alloc(8 * max(E, P))
    rec = {"case": "wgrad_sensor{}_k{}_w{}_order{}_{}".format(N, a.k, w, a.order, dtype.name), "N": N, "signals": w,
           "order": a.order, "edges": E, "candidate_pairs": P, "reps": a.reps}
    try:
        med, low = timed(a.reps, lambda: dev.cheby_filter_dev(c, x.ptr, y.ptr, w, G.lmax, _capi.ANALYSIS))
        rec.update(forward_ms=med, forward_ms_min=low)
        syn, _ = timed(a.reps, lambda: dev.cheby_filter_dev(c, y.ptr, gx.ptr, w, G.lmax, _capi.SYNTHESIS))
        cross, _ = timed(a.reps, lambda: dev.cheby_cross_moments_dev(x.ptr, y.ptr, w, 1, G.lmax, M)[1])
        rec.update(synthesis_ms=syn, cross_ms=cross, vjp_ms=syn + cross)
        for name, args, pairs in (("own", (None, None, 0), E), ("cand", (bp.ptr, bp.ptr + 4 * P, P), P)):
            parts = []

            def call():
                ms = dev.cheby_laplacian_grad_dev(c, x.ptr, y.ptr, w, G.lmax, *args, gdiag_ptr=bd.ptr, goff_ptr=bo.ptr)
                parts.append(ctx.last_timing())
                return ms

            med, low = timed(a.reps, call)
            parts = parts[-a.reps:]
            rec.update({name + "_ms": med, name + "_ms_min": low,
                        name + "_steps_ms": statistics.median(p["steps_ms"] for p in parts),
                        name + "_hook_ms": statistics.median(p["combine_ms"] for p in parts),
                        name + "_pair_bytes_per_order": float(pairs) * (4.0 * w * dtype.itemsize + 8.0),
                        name + "_over_forward": med / rec["forward_ms"]})
        rec.update(row_bytes_per_order=2.0 * N * w * dtype.itemsize, step_kinds=ctx.last_step_kinds(),
                   bench_read_GBps=ctx.bench_read(int(min(float(dtype.itemsize) * N * w * 8, 4 << 30)), passes=10))
    finally:
        for b in (x, y, gx, bp, bd, bo):
            b.free()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--signals", type=int, default=64)
    ap.add_argument("--order", type=int, default=30)
    ap.add_argument("--candidates", type=int, default=24)
    ap.add_argument("--dtype", default="float64", choices=["float64", "float32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="one call of each shape, no warm-up (for a kernel trace)")
    ap.add_argument("--torch-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.once:
        a.reps = 1
    rec = torch_baseline(a) if a.torch_baseline else engine_run(a)
    rec["record"] = "wgrad_bench"
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
