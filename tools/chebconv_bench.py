#!/usr/bin/env python3
"""The Chebyshev graph convolution on the device: one JSON line per measured shape.

    python tools/chebconv_bench.py [--n 1000000] [--k 8] [--batch 1] [--features 16,32,64] [--orders 5,25]
                                   [--dtype float64] [--reps 7] [--torch] [--out FILE]

Sensor(n, k, seed 0), resident signals, Fin = Fout = F.  Per (F, K), after two warm-up calls of every shape, `reps`
timed calls each; every device time is the call's own (events around its launches, read after the stream synchronise
that ends the call), reported as median and minimum:

  conv_ms        gspx_cheby_conv_dev: K + 1 Clenshaw steps, each fed by one k_group_mix
  synthesis_ms   gspx_cheby_filter_dev in synthesis mode with Nf = 1 at the same width B F and order: the same Clenshaw
                 steps without the mixing - conv_over_synthesis is what the mix kernel adds
  predicted_ratio  from the bytes: a synthesis step gathers b_{k+1} and reads b_{k+2} and its input panel, writes b_k
                 (four panel passes) and reads the matrix once; the convolution adds one read of X and one write of
                 U_k per order (the step's input-panel read is U_k's)
  backward_ms    conv_dev with theta transposed (d/dX) + gspx_cheby_cross_grams_dev (d/dtheta); of the latter steps_ms
                 (the K recurrence steps) and gram_ms (k_slot_cross_gram and the second pass: the "combine" phase of
                 ctx.last_timing())
  gram_read_bytes  what k_slot_cross_gram reads, counted from the shapes: every slot once per 64-wide block of Fout,
                 the cotangent once per chunk of slots and 64-wide block of Fin; gram_read_GBps beside
                 bench_read_GBps, the read-only stream rate ctx.bench_read measures in the same run

--torch measures, per (F, K) and in float64 or float32 alike, the same layer composed of torch ops on the same GPU - a
torch.sparse recurrence that keeps the K + 1 panels for autograd, plus einsum - forward + backward wall time around a
synchronise and torch's peak allocated memory, beside nn.cheby_conv's on the same tensors.  That mode imports
pygsp_amd.nn (and so torch) before anything loads libgspx.  A GPU run gives every invocation its own time limit and
chains them, e.g.

    timeout -k 10 400 python tools/chebconv_bench.py --dtype float64 --out profiles/chebconv.jsonl && \\
    timeout -k 10 400 python tools/chebconv_bench.py --dtype float32 --out profiles/chebconv.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(reps, call):
    """Device ms of `reps` calls after two warm-ups: (median, min)."""
    for _ in range(2):
        call()
    t = [float(call()) for _ in range(reps)]
    return statistics.median(t), min(t)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def gram_tiles(F):  # csrc/gspx_conv.hip.h
    return 1 if F <= 16 else 2 if F <= 32 else 4


def device_cases(a, np, G, dtype):
    from pygsp_amd import _capi, engine
    dev = G.device_graph(dtype.type)
    ctx, N, B = dev.ctx, G.N, a.batch
    rng = np.random.default_rng(0)
    matrix = float(dev.nnz_internal) * (dtype.itemsize + 1)  # values and the 8-bit tile positions, once per step
    for F in a.features:
        x = G.to_device(rng.standard_normal((N, B * F)))
        y = engine.DeviceArray.empty(ctx, (N, B * F), dtype)
        gx = engine.DeviceArray.empty(ctx, (N, B * F), dtype)
        try:
            for K in a.orders:
                M = K + 1
                theta = rng.standard_normal((M, F, F)) / np.sqrt(F) * (0.8 ** np.arange(M))[:, None, None]
                c = rng.standard_normal((1, M)) * 0.8 ** np.arange(M)
                rec = {"case": "chebconv_sensor{}_k{}_B{}_F{}_K{}_{}".format(N, a.k, B, F, K, dtype.name), "N": N, "B": B,
                       "F": F, "K": K, "dtype": dtype.name, "reps": a.reps}
                med, low = timed(a.reps, lambda: dev.cheby_conv_dev(theta, x.ptr, y.ptr, B, G.lmax))
                rec.update(conv_ms=med, conv_ms_min=low, conv_step_kinds=ctx.last_step_kinds())
                med, low = timed(a.reps, lambda: dev.cheby_filter_dev(c, x.ptr, gx.ptr, B * F, G.lmax, _capi.SYNTHESIS))
                panel = float(dtype.itemsize) * N * B * F
                rec.update(synthesis_ms=med, synthesis_ms_min=low, synthesis_step_kinds=ctx.last_step_kinds(),
                           conv_over_synthesis=rec["conv_ms"] / med,
                           predicted_ratio=(6 * panel + matrix) / (4 * panel + matrix))
                tht = np.ascontiguousarray(theta.transpose(0, 2, 1))
                med, low = timed(a.reps, lambda: dev.cheby_conv_dev(tht, y.ptr, gx.ptr, B, G.lmax))
                rec.update(conv_transposed_ms=med)
                parts = []

                def grams():
                    _, ms = dev.cheby_cross_grams_dev(x.ptr, y.ptr, B, F, F, G.lmax, M)
                    parts.append(ctx.last_timing())
                    return ms

                med, low = timed(a.reps, grams)
                parts = parts[2:]
                steps = statistics.median(p["steps_ms"] for p in parts)
                gram = statistics.median(p["combine_ms"] for p in parts)
                t = gram_tiles(F)
                blocks, chunks = -(-F // (16 * t)), -(-M // (16 // (t * t)))
                read = panel * (M * blocks + chunks * blocks)
                rec.update(cross_grams_ms=med, cross_grams_ms_min=low, steps_ms=steps, gram_ms=gram,
                           gram_read_bytes=read, gram_read_GBps=read / (gram * 1e-3) / 1e9,
                           bench_read_GBps=ctx.bench_read(int(min(panel * M, 4 << 30)), passes=10),
                           backward_ms=rec["conv_transposed_ms"] + med,
                           backward_over_forward=(rec["conv_transposed_ms"] + med) / rec["conv_ms"])
                emit(rec, a.out)
        finally:
            for d in (x, y, gx):
                d.free()


def torch_cases(a, np, G, dtype):
    import torch
    from pygsp_amd import nn
    tdtype = torch.float64 if dtype.itemsize == 8 else torch.float32
    N, B = G.N, a.batch
    L = G.L.tocoo()
    half = G.lmax / 2.0
    Lt = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([L.row, L.col]).astype(np.int64)),
                                 torch.from_numpy(np.asarray(L.data, dtype=np.float64) / half), size=L.shape).coalesce()
    Lt = Lt.to(device="cuda", dtype=tdtype)
    layout = "coo"
    try:  # the faster layout where this torch build multiplies it
        csr = Lt.to_sparse_csr()
        torch.sparse.mm(csr, torch.zeros((N, 1), dtype=tdtype, device="cuda"))
        Lt, layout = csr, "csr"
    except RuntimeError:
        pass

    def composed(theta, x):
        """sum_k T_k(Lt) x theta_k with the K + 1 panels alive for autograd: what a user writes today."""
        flat = x.reshape(N, -1)
        T = [flat, torch.sparse.mm(Lt, flat) - flat]
        for _ in range(2, theta.shape[0]):
            T.append(2.0 * (torch.sparse.mm(Lt, T[-1]) - T[-1]) - T[-2])
        return sum(torch.einsum("nbi,io->nbo", t.reshape(x.shape), theta[k]) for k, t in enumerate(T))

    def run(layer, theta, x, w):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        theta.grad = x.grad = None
        (layer(theta, x) * w).sum().backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    gen = torch.Generator().manual_seed(0)
    for F in a.features:
        x = torch.randn((N, B, F), dtype=tdtype, generator=gen).cuda().requires_grad_()
        w = torch.randn((N, B, F), dtype=tdtype, generator=gen).cuda()
        for K in a.orders:
            theta = (torch.randn((K + 1, F, F), dtype=torch.float64, generator=gen) / F ** 0.5).cuda().requires_grad_()
            rec = {"case": "chebconv_torch_sensor{}_k{}_B{}_F{}_K{}_{}".format(N, a.k, B, F, K, dtype.name), "N": N,
                   "B": B, "F": F, "K": K, "dtype": dtype.name, "reps": a.reps, "sparse_layout": layout}
            for name, layer in (("engine", lambda t, s: nn.cheby_conv(G, t, s)),
                                ("torch", lambda t, s: composed(t.to(tdtype), s))):
                runs = [run(layer, theta, x, w) for _ in range(a.reps + 2)][2:]
                rec[name + "_fwd_bwd_ms"] = statistics.median(r[0] for r in runs)
                rec[name + "_fwd_bwd_ms_min"] = min(r[0] for r in runs)
                rec[name + "_peak_MiB"] = max(r[1] for r in runs)
                if name == "engine":
                    rec["engine_path"] = nn.last_path
                    ge = (theta.grad.detach().clone(), x.grad.detach().clone())
                else:
                    rec["theta_grad_rel_diff"] = float((theta.grad - ge[0]).abs().max() / ge[0].abs().max())
                    rec["x_grad_rel_diff"] = float((x.grad - ge[1]).abs().max() / ge[1].abs().max())
            rec["torch_over_engine"] = rec["torch_fwd_bwd_ms"] / rec["engine_fwd_bwd_ms"]
            emit(rec, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--features", type=lambda s: [int(v) for v in s.split(",")], default=[16, 32, 64])
    ap.add_argument("--orders", type=lambda s: [int(v) for v in s.split(",")], default=[5, 25])
    ap.add_argument("--dtype", default="float64", choices=["float64", "float32"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.torch:
        import pygsp_amd.nn  # noqa: F401 (torch before libgspx: one HIP runtime in the process)
    import numpy as np
    from pygsp_amd import graphs

    dtype = np.dtype(a.dtype)
    G = graphs.Sensor(a.n, k=a.k, seed=0, compute_dtype=dtype.type)
    G.estimate_lmax("bounds")
    (torch_cases if a.torch else device_cases)(a, np, G, dtype)


if __name__ == "__main__":
    main()
