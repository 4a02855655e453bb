#!/usr/bin/env python3
"""Graph total-variation prox benchmark on the device: one JSON line per case.

    python tools/prox_tv_bench.py [--N 1000000] [--nsig 1 8 64] [--gamma 0.5] [--host-N 1000000] [--out FILE]

Sensor(N, seed=0), float64, standard normal signals.  Per width, after a warm-up: a fixed 50 iterations (rtol off,
maxit 50), device time of the call over 50 = ms per iteration, next to the sum of one gspx_grad_dev and one
gspx_div_dev on panels of the same shapes in the same run (best of 6 each): the two products are the floor any
iteration pays, and their code is the stand-alone operators'.  Algorithmic bytes of one iteration, every panel counted
once per read and once per write, plus the index arrays:
  k_tv_div         reads u (E), a (V), x (V); writes a (V), zt (V); eoff, toff (8 N), tedge (4 E), cs, ct (16 E)
  k_tv_grad_step   reads zt (V, the gathered target rows not counted again), g, u, u_prev (3 E); writes g, u_next (2 E);
                   perm / eoff (8 N), edst (4 E), cs, ct (16 E)
with V = 8 N Nsig and E = 8 n_edges Nsig bytes, set against the read-only rate of ctx.bench_read in that run.
The wall line times one default-rule call at --host-N x 8 on the device against the numpy / scipy restatement
(tests/prox_tv_helpers.py) of the same call on the host.
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


def emit(rec, outf):
    line = json.dumps(rec)
    print(line, flush=True)
    if outf:
        outf.write(line + "\n")
        outf.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1_000_000)
    ap.add_argument("--nsig", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--gamma", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-N", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from pygsp_amd import graphs, optimization
    outf = open(a.out, "a") if a.out else None
    G = graphs.Sensor(a.N, seed=0)
    G.estimate_lmax()
    dev = G.device_graph(np.float64)
    N, E = G.N, dev.n_edges()
    read_gbps = dev.ctx.bench_read(1 << 30, passes=10)
    step = optimization.tv_step(G)
    rng = np.random.default_rng(0)
    for S in a.nsig:
        x = rng.standard_normal((N, S))
        V, P = 8.0 * N * S, 8.0 * E * S
        div_bytes = P + 4 * V + 8.0 * N + 20.0 * E
        grad_bytes = V + 5 * P + 8.0 * N + 20.0 * E
        bx, by, bz = dev.ctx.alloc(int(V)), dev.ctx.alloc(int(P)), dev.ctx.alloc(int(V))
        try:
            bx.upload(np.ascontiguousarray(x))
            grad_ms = min(dev.grad_dev(bx.ptr, by.ptr, S) for _ in range(6))
            div_ms = min(dev.div_dev(by.ptr, bz.ptr, S) for _ in range(6))
            dev.prox_tv_dev(bx.ptr, bz.ptr, S, a.gamma, step, rtol=None, maxit=5)  # warm-up
            info = min((dev.prox_tv_dev(bx.ptr, bz.ptr, S, a.gamma, step, rtol=None, maxit=a.iters) for _ in range(3)),
                       key=lambda i: i["ms"])
        finally:
            for b in (bx, by, bz):
                b.free()
        per_it = info["ms"] / info["niter"]
        emit({"case": "prox_tv_sensor{}_S{}".format(N, S), "N": N, "n_edges": E, "Nsig": S, "gamma": a.gamma,
              "niter": info["niter"], "crit": info["crit"], "device_ms": info["ms"], "ms_per_iteration": per_it,
              "grad_ms": grad_ms, "div_ms": div_ms, "iteration_vs_grad_plus_div": per_it / (grad_ms + div_ms),
              "bench_read_GBps": read_gbps, "div_kernel_bytes": div_bytes, "grad_step_kernel_bytes": grad_bytes,
              "iteration_GBps_algorithmic": (div_bytes + grad_bytes) / (per_it * 1e-3) / 1e9,
              "fraction_of_read_rate": (div_bytes + grad_bytes) / (per_it * 1e-3) / 1e9 / read_gbps}, outf)
    # wall time of one default-rule call, device against the restatement on the host
    import prox_tv_helpers as th
    H = G if a.host_N == a.N else graphs.Sensor(a.host_N, seed=0)
    if H is not G:
        H.estimate_lmax()
    H.compute_differential_operator()
    x = rng.standard_normal((H.N, 8))
    optimization.prox_tv_solve(x, a.gamma, H, tol=None, maxit=3)  # warm-up
    t = time.perf_counter()
    z, info = optimization.prox_tv_solve(x, a.gamma, H)
    wall_dev = time.perf_counter() - t
    t = time.perf_counter()
    zr, ir = th.solve(H.D, x, a.gamma, optimization.tv_step(H))
    wall_host = time.perf_counter() - t
    emit({"case": "default_rule_sensor{}_S8".format(H.N), "N": H.N, "Nsig": 8, "gamma": a.gamma,
          "niter": info["niter"], "crit": info["crit"], "host_niter": ir["niter"], "device_wall_s": wall_dev,
          "device_ms": info["ms"], "host_wall_s": wall_host, "speedup": wall_host / wall_dev,
          "max_abs_difference": float(np.abs(z - zr).max())}, outf)


if __name__ == "__main__":
    main()
