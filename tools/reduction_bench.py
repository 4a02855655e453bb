#!/usr/bin/env python3
"""Measure pygsp_amd.reduction on the device: Kron reduction of Sensor(N, k=8) with the even vertices kept, and
interpolate on the headline graph (Sensor N=1e6, k=8, 64 float64 signals, half the vertices kept).  Every leg runs in
a fresh process, best of 3 after a warm-up; one JSON object per leg on stdout (and appended to --out).

usage (GPU box):  python tools/reduction_bench.py [--legs kron4096,kron16384,kron32768,interp] [--out FILE]
usage (any host): PYGSP_PATH=path/to/reference python tools/reduction_bench.py --legs reference
                  (the reference's own kron_reduction / interpolate on the host's cores, N = 1000 .. 4000)"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def best(fn, n=3):
    fn()  # warm-up
    runs = []
    for _ in range(n):
        t0 = time.perf_counter()
        r = fn()
        runs.append((time.perf_counter() - t0, r))
    return min(runs, key=lambda p: p[0])


def device_graph(N):
    from pygsp_amd import engine, graphs
    W, coords = graphs.sensor_weights(N, k=8, seed=42)
    dev = engine.DeviceGraph.from_w(W, dtype=np.float64, perm=engine.locality_order(W, coords),
                                    ctx=engine.default_context(0))
    if N >= 4096:
        dev.build_gather_tiles()  # what graphs.Graph does for a graph of this size
    return dev, W


def leg_kron(N):
    dev, W = device_graph(N)
    ind = np.arange(0, N, 2)
    nk = ind.size
    wall, (_, A, iters, info) = best(lambda: dev.kron(ind, 0.0, dense=False, adjacency=True))
    gbps = dev.ctx.bench_copy(nk * nk * 8)
    copy_ms = 2 * nk * nk * 8 / gbps / 1e6
    return {"leg": "kron", "graph": "Sensor(N=%d, k=8)" % N, "nk": int(nk), "rtol": 1e-10,
            "iterations": [int(iters.min()), int(iters.max())], "whole_call_ms": wall * 1e3,
            "kernel_ms": info["kernel_ms"], "solve_ms": info["solve_ms"], "rows_ms": info["rows_ms"],
            "finalise_ms": info["finalise_ms"], "W_nnz": int(A.nnz), "batches": -(-nk // 256),
            "bench_copy_GBps": gbps, "copy_of_nk2_doubles_ms": copy_ms,
            "finalise_over_copy": info["finalise_ms"] / copy_ms}


def leg_interp(N=1000000, nsig=64):
    from pygsp_amd import filters
    dev, W = device_graph(N)
    ctx = dev.ctx
    rng = np.random.default_rng(0)
    mask = np.zeros(N)
    mask[::2] = 1
    F = rng.standard_normal((N, nsig))
    bm, bf, bx, ba = ctx.upload(mask), ctx.upload(F), ctx.alloc(F.nbytes), ctx.alloc(F.nbytes)
    eps = 0.005
    out = {"leg": "interp", "graph": "Sensor(N=%d, k=8)" % N, "nsig": nsig, "kept": int(mask.sum()), "reg_eps": eps}

    def call(x, a, maxiter=None):
        return dev.schur_cg_dev(eps, bm.ptr, bf.ptr, x, a, nsig, maxiter=maxiter)

    _, (iters, ms) = best(lambda: call(bx.ptr, None))
    out["exact"] = {"ms": ms, "iterations": [int(iters.min()), int(iters.max())]}
    _, (iters, ms) = best(lambda: call(None, ba.ptr))
    out["alpha"] = {"ms": ms, "iterations": [int(iters.min()), int(iters.max())]}
    out["ms_per_iteration"] = ms / (int(iters.max()) + 2)
    # the frame without the iteration (maxiter = 0): nothing stored | x stored | the kept rows of A x
    frame = {k: min(call(*p, maxiter=0)[1] for _ in range(4)) for k, p in
             (("none", (None, None)), ("x", (bx.ptr, None)), ("alpha", (None, ba.ptr)))}
    lap = min(dev.laplacian_apply_dev(bf.ptr, bx.ptr, nsig) for _ in range(4))
    out["frame_ms"] = frame
    out["kept_rows_ms"] = frame["alpha"] - frame["none"]
    out["laplacian_apply_ms"] = lap
    out["kept_rows_over_laplacian_apply"] = out["kept_rows_ms"] / lap
    # the Green's kernel at order 100 on the zero-filled alpha
    lmax = 2.0 * float(W.sum(axis=0).max())  # (the degree bound: the timing does not depend on it)
    c = filters._as_coeff_matrix(filters.compute_cheby_coeff(
        filters.Filter(type("G", (), {"lmax": lmax, "N": N})(), lambda x: 1.0 / (eps + x)), m=100))
    green = min(dev.cheby_filter_dev(c, ba.ptr, bx.ptr, nsig, lmax, 0) for _ in range(3))
    out["green_order100_ms"] = green
    out["chebyshev_total_ms"] = out["alpha"]["ms"] + green
    return out


def leg_reference():
    sys.path.insert(0, os.environ["PYGSP_PATH"])
    os.environ.setdefault("MPLBACKEND", "agg")
    from pygsp import graphs, reduction
    rows = []
    for N in (1000, 2000, 4000):
        G = graphs.Sensor(N, k=8, seed=42)
        G.estimate_lmax()
        G.mr = {}
        ind = np.arange(0, N, 2)
        f = np.random.default_rng(0).standard_normal((ind.size, 1))
        t_k, _ = best(lambda: reduction.kron_reduction(G, ind), 1)
        t_i, _ = best(lambda: reduction.interpolate(G, f, ind), 1)
        rows.append({"N": N, "kron_reduction_ms": t_k * 1e3, "interpolate_1col_ms": t_i * 1e3})
    return {"leg": "reference", "where": "HOST (the reference's scipy code on this machine's cores)", "rows": rows}


def run_leg(name):
    if name.startswith("kron"):
        return leg_kron(int(name[4:]))
    return {"interp": leg_interp, "reference": leg_reference}[name]()


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--legs", default="kron4096,kron16384,kron32768,interp")
    p.add_argument("--leg", help="run this one leg in this process")
    p.add_argument("--out")
    p.add_argument("--leg-timeout", type=int, default=300, help="seconds a leg's process may take")
    a = p.parse_args()
    if a.leg:
        print(json.dumps(run_leg(a.leg)))
        sys.exit(0)
    for leg in a.legs.split(","):  # a fresh process per leg
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg], capture_output=True, text=True,
                               timeout=a.leg_timeout)
        except subprocess.TimeoutExpired:
            print(json.dumps({"leg": leg, "failed": "no result after %d s" % a.leg_timeout}), flush=True)
            sys.exit(124)
        line = r.stdout.strip().splitlines()[-1] if r.returncode == 0 and r.stdout.strip() else json.dumps(
            {"leg": leg, "failed": r.returncode, "stderr": r.stderr[-2000:]})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
        if r.returncode != 0:
            sys.exit(r.returncode)  # nothing more is started on the device after a failure
