#!/usr/bin/env python3
"""The full Fourier basis on the device against the host's eigh: one JSON line per graph size (recorded in
profiles/eigh_bench.jsonl, read in profiles/eigh.md).

    python tools/eigh_bench.py [--N 1024 2048 4096 8192] [--limit 600] [--out FILE]

Per N, on Sensor(N, k=8, seed=0) with the float64 device graph, in one child process of its own under one time limit:
  * ``fourier.device_full_basis`` twice (the first call also pays the allocations): wall seconds of each, and of the
    second the solver's own figures - device milliseconds per stage (subproblems, column updates, row updates,
    off-norms, finish), forming the dense L, sweeps, pairs skipped per sweep;
  * ``np.linalg.eigh`` of the same matrix in the same process on the same host, with the threads the environment gives
    it (best of 2);
  * the three accuracy figures of the device result: eigenvalues against that eigh, max |L U - U diag(e)| and
    max |U^T U - I|, the first two over s = max(lambda_max, 1).
After a failed or timed-out case the script stops: nothing more is started on the GPU.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def case(N):
    from pygsp_amd import fourier, graphs
    G = graphs.Sensor(N, k=8, seed=0)
    dev = G.device_graph(np.float64)
    walls, last = [], None
    for _ in range(2):
        t = time.perf_counter()
        e, U, U_dev, stats = fourier.device_full_basis(dev)
        walls.append(time.perf_counter() - t)
        dev.ctx.give(U_dev.buf)
        last = (e, U, stats)
    e, U, stats = last
    L = G.L.toarray().astype(np.float64)
    host = []
    for _ in range(2):
        t = time.perf_counter()
        lam, _ = np.linalg.eigh(L)
        host.append(time.perf_counter() - t)
    s = max(float(lam[-1]), 1.0)
    rec = {"case": "full_basis", "N": N, "k": 8, "cpus": os.cpu_count(), "threads": os.environ.get("OMP_NUM_THREADS"),
           "device_wall_s_first": walls[0], "device_wall_s": walls[1], "host_eigh_s": min(host),
           "host_over_device": min(host) / walls[1],
           "solver_wall_ms": stats["ms_wall"], "form_L_ms": stats["ms_form"],
           "ms_sub": stats["ms_sub"], "ms_cols": stats["ms_cols"], "ms_rows": stats["ms_rows"], "ms_off": stats["ms_off"],
           "ms_finish": stats["ms_finish"], "sweeps": stats["sweeps"], "pairs_rotated": stats["pairs_rotated"],
           "pairs_skipped": stats["pairs_skipped"], "skipped_per_sweep": stats["skipped_per_sweep"],
           "off_rel": stats["off_rel"], "residual_2norm": stats["residual"],
           "eigenvalue_err_over_s": float(np.max(np.abs(e - lam))) / s,
           "residual_max_over_s": float(np.max(np.abs(L @ U - U * e[None, :]))) / s,
           "orthonormality": float(np.max(np.abs(U.T @ U - np.eye(N))))}
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--N", type=int, nargs="*", default=[1024, 2048, 4096, 8192])
    ap.add_argument("--limit", type=float, default=600.0, help="seconds one graph size may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.case is not None:
        return case(args.case)
    outf = open(args.out, "a") if args.out else None
    for N in args.N:
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(N)], capture_output=True,
                                 text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print("N = {}: no result within {} s; stopping".format(N, args.limit), file=sys.stderr)
            return 1
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
        if res.returncode != 0 or not lines:
            print("N = {}: exit status {}; stopping\n{}".format(N, res.returncode, res.stderr[-2000:]), file=sys.stderr)
            return 1
        print(lines[-1], flush=True)
        if outf:
            outf.write(lines[-1] + "\n")
            outf.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
