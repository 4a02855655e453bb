#!/usr/bin/env python3
"""Backward pass of the Chebyshev filter on the device: one JSON line per invocation.

    python tools/autograd_bench.py --nf 1 [--n 1000000] [--k 8] [--signals 64] [--order 30] [--dtype float64]
                                   [--reps 7] [--forward-only] [--tree DIR] [--label NAME] [--out FILE]

One invocation measures one bank width on Sensor(n, k, seed 0) with resident signals, after two warm-up calls of every
shape, `reps` timed calls each; every time is the call's own device time (events around its launches, read after the
stream synchronise that ends the call), reported as median and minimum:

  forward_ms    gspx_cheby_filter_dev, analysis, nf filters
  synthesis_ms  gspx_cheby_filter_dev, synthesis with the same coefficients on the cotangent's planes (d/dx)
  cross_ms      gspx_cheby_cross_moments_dev (d/dc), and inside it steps_ms (the M - 1 recurrence steps) and dots_ms
                (k_slot_cross_dots and k_dots_reduce of every plane pass: the "combine" phase of ctx.last_timing())
  dots_read_bytes  what the dot kernel reads, counted from the shapes: per pass of at most 8 planes every slot once and
                the pass's planes once per chunk of slots - 8 slots, 16 in a pass of one or two planes, half that for
                fp32 panels of an even width
  bench_read_GBps  the read-only stream rate ctx.bench_read measures in the same run
  backward_over_forward  (synthesis + cross) / forward, medians

--forward-only times the forward call alone and uses nothing this feature added; with --tree it measures the pygsp_amd
of ANOTHER checkout (built there), so the forward call of two commits can be timed in one run, alternating.
A GPU run gives every invocation its own time limit and chains them, e.g.

    timeout -k 10 300 python tools/autograd_bench.py --nf 1 --out profiles/autograd_bench.jsonl && \\
    timeout -k 10 300 python tools/autograd_bench.py --nf 6 --out profiles/autograd_bench.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np


def timed(reps, call):
    """Device ms of `reps` calls after two warm-ups: (median, min, all)."""
    for _ in range(2):
        call()
    t = [float(call()) for _ in range(reps)]
    return statistics.median(t), min(t), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--signals", type=int, default=64)
    ap.add_argument("--order", type=int, default=30)
    ap.add_argument("--nf", type=int, default=1)
    ap.add_argument("--dtype", default="float64", choices=["float64", "float32"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--forward-only", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from pygsp_amd import _capi, engine, graphs

    dtype = np.dtype(a.dtype)
    G = graphs.Sensor(a.n, k=a.k, seed=0, compute_dtype=dtype.type)
    G.estimate_lmax("bounds")
    dev = G.device_graph(dtype.type)
    ctx, N, w, M, nf = dev.ctx, G.N, a.signals, a.order + 1, a.nf
    rng = np.random.default_rng(0)
    c = rng.standard_normal((nf, M)) * 0.8 ** np.arange(M)
    x = G.to_device(rng.standard_normal((N, w)))
    y = engine.DeviceArray.empty(ctx, (N, w, nf), dtype)
    rec = {"case": "autograd_sensor{}_k{}_w{}_order{}_nf{}_{}".format(N, a.k, w, a.order, nf, dtype.name),
           "label": a.label, "N": N, "signals": w, "order": a.order, "nf": nf, "reps": a.reps}
    try:
        med, low, every = timed(a.reps, lambda: dev.cheby_filter_dev(c, x.ptr, y.ptr, w, G.lmax, _capi.ANALYSIS))
        rec.update(forward_ms=med, forward_ms_min=low, forward_ms_all=every, forward_step_kinds=ctx.last_step_kinds())
        if not a.forward_only:
            # the cotangent: the forward's own output planes, as good as any
            gx = engine.DeviceArray.empty(ctx, (N, w, 1), dtype)
            med, low, _ = timed(a.reps, lambda: dev.cheby_filter_dev(c, y.ptr, gx.ptr, w, G.lmax, _capi.SYNTHESIS))
            rec.update(synthesis_ms=med, synthesis_ms_min=low)
            parts = []

            def cross():
                _, ms = dev.cheby_cross_moments_dev(x.ptr, y.ptr, w, nf, G.lmax, M)
                parts.append(ctx.last_timing())
                return ms

            med, low, _ = timed(a.reps, cross)
            parts = parts[2:]
            steps = statistics.median(p["steps_ms"] for p in parts)
            dots = statistics.median(p["combine_ms"] for p in parts)
            vec = 2 if dtype.itemsize == 4 and w % 2 == 0 else 1
            passes = [min(8, nf - f0) for f0 in range(0, nf, 8)]  # CROSS_PASS, CROSS_FEW, cross_cs: csrc/gspx_poly.hip.h
            panels = sum(M + here * -(-M // ((16 if here <= 2 else 8) // vec)) for here in passes)
            read = float(dtype.itemsize) * N * w * panels
            rec.update(cross_ms=med, cross_ms_min=low, steps_ms=steps, dots_ms=dots, copy_in_ms=parts[-1]["permute_ms"],
                       cross_step_kinds=ctx.last_step_kinds(), dots_read_bytes=read,
                       dots_read_GBps=read / (dots * 1e-3) / 1e9,
                       bench_read_GBps=ctx.bench_read(int(min(float(dtype.itemsize) * N * w * M, 4 << 30)), passes=10),
                       backward_ms=rec["synthesis_ms"] + med,
                       backward_over_forward=(rec["synthesis_ms"] + med) / rec["forward_ms"],
                       cross_over_forward=med / rec["forward_ms"])
            gx.free()
    finally:
        x.free()
        y.free()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
