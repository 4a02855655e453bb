#!/usr/bin/env python3
"""Exact Fourier filtering on the device: one JSON line per case (recorded in profiles/exact_bench.jsonl).

    python tools/exact_bench.py [--N 8192] [--signals 64] [--filters 6] [--modulation-N 2048 4096] [--out FILE]

Analysis case: N x `signals` standard-normal signals, a MexicanHat bank of `filters` kernels, and a dense ORTHOGONAL U
that costs O(N^2) to make (two Householder reflections: the eigensolve is not what is timed) with sorted eigenvalues
drawn in [0, lmax].  Timed, after 3 warm-up calls, best and median of 10:
  * the two device calls (HIP events: Gram U^T x to the device, spectral apply) and the whole
    ``filter(method='exact')`` with device arrays in and out (wall) and numpy in and out (wall, with both PCIe legs);
  * the same arithmetic in numpy on this host's CPUs (best of 3);
  * the only route before this path existed: ``G.gft`` / ``G.igft`` of host arrays around the multiply, as filter.py:299-301
    (best of 3).
The apply kernel's U traffic is reported twice against the 8 TB/s HBM peak: `u_once` counts U read once (N * N * 8 bytes,
what a kernel that loops the filters over one staged chunk would move) and `u_issued` what this kernel asks for: U once
per filter and per 64-column tile (mostly served by L2).

Modulation case (localisation first) on Sensor(N, seed=0) with Heat(10): device kernel ms and wall seconds of
``Modulation.filter`` (best of 3 after one warm-up; the host eigh for the basis is reported apart).  The reference's
loop was timed on a host at N = 123 and 400 (0.21 s, 0.88 s); `reference_extrapolated_s` scales the N = 400 figure by
(N / 400)^3 - an EXTRAPOLATION, the reference is not run here.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
REFERENCE_LOOP_S = {123: 0.21, 400: 0.88}  # Modulation.filter of the reference, measured on a host CPU


def emit(rec, outf):
    line = json.dumps(rec)
    print(line, flush=True)
    if outf:
        outf.write(line + "\n")
        outf.flush()


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t, r))
    walls = sorted(w for w, _ in out)
    return walls[0], walls[len(walls) // 2], [r for _, r in out]


def householder_basis(N, rng):
    """(I - 2 v v^T)(I - 2 w w^T): dense, orthogonal to rounding, O(N^2) to form."""
    v, w = rng.standard_normal(N), rng.standard_normal(N)
    v, w = v / np.linalg.norm(v), w / np.linalg.norm(w)
    U = np.identity(N) - 2.0 * np.outer(w, w)
    U -= 2.0 * np.outer(v, v @ U)
    return U


def analysis_case(N, S, Nf, outf):
    from pygsp_amd import filters, fourier, graphs
    rng = np.random.default_rng(0)
    G = graphs.Sensor(N, seed=0)
    G.estimate_lmax("bounds")
    lmax = G.lmax
    G._release_basis_dev()
    G._e, G._U = np.sort(rng.uniform(0, lmax, N)), householder_basis(N, rng)
    G._e[0] = 0.0
    bank = filters.MexicanHat(G, Nf=Nf)
    H = bank.evaluate(G.e)
    x = rng.standard_normal((N, S))
    dx = G.to_device(x)
    dev, U = G._basis_on_device()
    ctx = dev.ctx

    ms = {"gram": [], "apply": []}

    def device_calls():
        hat, g = filters._exact_gft(G, dx, S, 1)
        out, a = filters._exact_apply(G, hat, H, False)
        hat.free()
        out.free()
        ms["gram"].append(g)
        ms["apply"].append(a)

    timed(device_calls, 3, 10)
    gram_ms, apply_ms = sorted(ms["gram"][3:]), sorted(ms["apply"][3:])

    def resident():
        bank.filter(dx, method="exact").free()
        ctx.sync()

    res_best, res_med, _ = timed(resident, 3, 10)
    host_best, host_med, outs = timed(lambda: bank.filter(x, method="exact"), 3, 10)
    y = outs[-1]

    def numpy_same():
        hat = G.U.T @ x
        return np.stack([G.U @ (H[g][:, None] * hat) for g in range(Nf)], axis=2)

    np_best, _, refs = timed(numpy_same, 0, 3)
    err = float(np.max(np.abs(y - refs[-1])) / np.max(np.abs(refs[-1])))

    def host_transforms():  # filter.py:299-301 with the host gft / igft: what method='exact' could use before
        s = G.gft(x[:, :, None])
        s = np.matmul(s, np.expand_dims(H.T, 1))
        return G.igft(s)

    old_best, _, olds = timed(host_transforms, 0, 3)
    err_old = float(np.max(np.abs(y - olds[-1])) / np.max(np.abs(olds[-1])))
    u_bytes = 8.0 * N * N
    tiles = Nf * ((S + 63) // 64)
    emit({"case": "exact_analysis", "N": N, "signals": S, "filters": Nf, "cpus": os.cpu_count(),
          "threads": os.environ.get("OMP_NUM_THREADS"),
          "gram_ms_best": gram_ms[0], "gram_ms_median": gram_ms[len(gram_ms) // 2],
          "apply_ms_best": apply_ms[0], "apply_ms_median": apply_ms[len(apply_ms) // 2],
          "device_resident_wall_ms_best": res_best * 1e3, "device_resident_wall_ms_median": res_med * 1e3,
          "numpy_in_out_wall_ms_best": host_best * 1e3, "numpy_in_out_wall_ms_median": host_med * 1e3,
          "numpy_same_arithmetic_ms_best": np_best * 1e3, "host_gft_igft_route_ms_best": old_best * 1e3,
          "rel_err_vs_numpy": err, "rel_err_vs_host_route": err_old,
          "apply_fp64_TFLOPS": 2.0 * N * N * S * Nf / (apply_ms[0] * 1e-3) / 1e12,
          "gram_u_GBs": u_bytes / (gram_ms[0] * 1e-3) / 1e9,
          "apply_u_once_GBs": u_bytes / (apply_ms[0] * 1e-3) / 1e9,
          "apply_u_once_fraction_of_8TBs": u_bytes / (apply_ms[0] * 1e-3) / 1e9 / HBM_PEAK_GBS,
          "apply_u_issued_GBs": tiles * u_bytes / (apply_ms[0] * 1e-3) / 1e9,
          "apply_u_issued_fraction_of_8TBs": tiles * u_bytes / (apply_ms[0] * 1e-3) / 1e9 / HBM_PEAK_GBS}, outf)
    dx.free()


def modulation_case(N, outf):
    from pygsp_amd import filters, graphs
    G = graphs.Sensor(N, seed=0)
    t = time.perf_counter()
    G.compute_fourier_basis()
    eigh_s = time.perf_counter() - t
    s = np.random.default_rng(1).standard_normal(N)
    bank = filters.Modulation(G, filters.Heat(G, scale=10))
    kernel_ms = []

    def run():
        y = bank.filter(s)
        kernel_ms.append(G._gspx_last_kernel_ms)
        return y

    best, med, outs = timed(run, 1, 3)
    emit({"case": "modulation_localize_first", "N": N, "host_eigh_s": eigh_s, "wall_s_best": best, "wall_s_median": med,
          "device_kernel_ms_best": min(kernel_ms[1:]), "finite": bool(np.isfinite(outs[-1]).all()),
          "gram_fp64_TFLOPS": 2.0 * N ** 3 / (min(kernel_ms[1:]) * 1e-3) / 1e12,
          "reference_measured_s": REFERENCE_LOOP_S,
          "reference_extrapolated_s": REFERENCE_LOOP_S[400] * (N / 400.0) ** 3,
          "reference_note": "EXTRAPOLATED from the N = 400 host measurement by (N / 400)^3; not run here"}, outf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--signals", type=int, default=64)
    ap.add_argument("--filters", type=int, default=6)
    ap.add_argument("--modulation-N", type=int, nargs="*", default=[2048, 4096])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    outf = open(a.out, "a") if a.out else None
    if a.N:
        analysis_case(a.N, a.signals, a.filters, outf)
    for N in a.modulation_N:
        modulation_case(N, outf)


if __name__ == "__main__":
    main()
