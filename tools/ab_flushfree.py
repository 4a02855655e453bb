#!/usr/bin/env python3
"""A/B of the flush-free builds of k_step_tile (option tile_acc_builds, 1 against 0 = the general build for every
step), alternating in ONE process on one box, on the headline graph (Sensor 1M, k = 8; Heat order 30, device resident):
    [GSPX_LIB_PATH=<build>] python tools/ab_flushfree.py [rounds] > ab.jsonl
one JSON line per (dtype, row bytes, evaluation): row bytes 256 / 512 / 768 select the one-chunk, two-chunk and
several-chunk builds (NCOL 1 / 2 / 0); evaluations: the recurrence call (18 of its 30 launches are flush-free), the
Newton and the product form (all of theirs).  Per value: median, min and max of the call's step time (HIP events) over
the rounds, and whether the two values left the same bits in y."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pygsp_amd import engine, filters, graphs  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
lib = os.path.basename(os.environ.get("GSPX_LIB_PATH", "libgspx.so"))
ctx = engine.default_context(0)
for dtype in (np.float64, np.float32):
    elt = np.dtype(dtype).itemsize
    G = graphs.Sensor(1000000, k=8, seed=42, compute_dtype=dtype)
    G.estimate_lmax("bounds")
    lmax = float(G.lmax)
    c = np.atleast_2d(filters.compute_cheby_coeff(filters.Heat(G, 50), m=30))
    dev = G.device_graph()
    nodes, dcoef = filters.cheb_to_newton(c[0])
    program = filters.cheb_to_product(c[0], dtype) if filters.product_guard(c[0], dtype)[1].get("finite") else None
    for rowb in (512, 256, 768):
        nsig = rowb // elt
        x = np.random.default_rng(0).standard_normal((G.N, nsig)).astype(dtype)
        bx, by = ctx.upload(x), ctx.alloc(x.nbytes)
        calls = {"recurrence": lambda: dev.cheby_filter_dev(c, bx.ptr, by.ptr, nsig, lmax),
                 "newton": lambda: dev.newton_filter_dev(nodes, dcoef, bx.ptr, by.ptr, nsig, lmax)}
        if program is not None:
            calls["product"] = lambda: dev.program_filter_dev(program, bx.ptr, by.ptr, nsig, lmax)
        for name, call in calls.items():
            if name != "recurrence" and rowb != 512:
                continue
            ms, out = {0: [], 1: []}, {}
            for rep in range(rounds + 1):
                for v in (0, 1):
                    ctx.set_option("tile_acc_builds", v)
                    for i in range(3):
                        call()
                        if rep and i:  # the first round and the first call after a switch warm up
                            ms[v].append(ctx.last_timing()["steps_ms"])
                    if rep == rounds:
                        out[v] = by.download(x.shape, dtype)
            ctx.set_option("tile_acc_builds", 1)
            m0, m1 = float(np.median(ms[0])), float(np.median(ms[1]))
            print(json.dumps({"lib": lib, "dtype": np.dtype(dtype).name, "row_bytes": rowb, "nsig": nsig,
                              "evaluation": name, "launches": ctx.last_timing()["step_launches"],
                              "general_ms": [round(m0, 4), round(min(ms[0]), 4), round(max(ms[0]), 4)],
                              "flushfree_ms": [round(m1, 4), round(min(ms[1]), 4), round(max(ms[1]), 4)],
                              "gain_pct": round(100.0 * (m0 / m1 - 1.0), 2),
                              "same_bits": bool(np.array_equal(out[0], out[1]))}), flush=True)
        del bx, by
