"""Partial Fourier bases on the device: one compact JSON line per case.

    python tools/fourier_bench.py                      # Sensor(1e5), Sensor(1e6) x k in (16, 64) + the scipy baseline
    python tools/fourier_bench.py --cases 100000:16 --scipy 20000,50000 --scipy-timeout 600

Device cases (Graph.compute_fourier_basis(n_eigenvectors=k, method='device') on Sensor(N, k=8 neighbours, seed=0)):
N, k, p; iterations, total filter degree, whole-call ms; ms in the polynomial steps, L X, Gram, combine and residual
(HIP events of each entry point's kernel_ms: device work only, the small host copies of Q / theta / the
Gram excluded); the new kernels' achieved bytes/s and flop/s from their shapes with the
bound each is measured against; the worst residual / b and ||U^T U - I||.

The scipy baseline is the reference's own call, eigsh(L, k, which='SM') (fourier.py:174-175), on the same graph built
on the host, in a child process with a time limit of its own: "did not finish in T s" where it does not.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# bounds the kernels are measured against: HBM3E peak of the MI355X (8 TB/s, AMD's figure) and AMD's spec figure for
# the fp64 matrix-core rate (78.6 TFLOP/s) - the latter has not been measured in this project
HBM_BYTES_PER_S = 8.0e12
FP64_MFMA_FLOPS_UNMEASURED = 78.6e12


def device_case(N, k, neighbours, tol):
    import numpy as np

    from pygsp_amd import graphs
    G = graphs.Sensor(N, k=neighbours, seed=0)
    G.device_graph(np.float64)
    t0 = time.perf_counter()
    G.compute_fourier_basis(n_eigenvectors=k, method="device", tol=tol)
    wall_ms = (time.perf_counter() - t0) * 1e3
    st = G.fourier_stats
    b = float(G._get_upper_bound())
    U = G.U
    ortho = float(np.max(np.abs(U.T @ U - np.eye(k))))
    kernels = {}
    for key in ("gram", "combine", "resid"):
        ms = st["ms"][key]
        s = ms / 1e3 if ms > 0 else float("nan")
        # gram / combine: the flop rate against the (unmeasured) fp64 matrix-core figure and the byte rate against
        # HBM; at p ~ 100 columns the Gram sits near the balance point (2 p^2 N flop over 16 p N bytes = p / 8
        # flop/byte against 78.6e12 / 8e12 ~ 10), so both are reported
        kernels[key] = {"calls": st["calls"][key], "ms": round(ms, 3),
                        "GB_per_s": round(st["bytes"][key] / s / 1e9, 1),
                        "GFLOP_per_s": round(st["flops"][key] / s / 1e9, 1),
                        "frac_of_hbm_peak": round(st["bytes"][key] / s / HBM_BYTES_PER_S, 3),
                        "frac_of_fp64_mfma_spec_unmeasured": round(st["flops"][key] / s / FP64_MFMA_FLOPS_UNMEASURED, 4)}
    kernel_total = sum(st["ms"].values())
    return {"case": "device", "N": N, "k": k, "p": st["p"], "neighbours": neighbours, "tol": tol,
            "iterations": st["iterations"], "total_degree": st["total_degree"], "degrees": st["degrees"],
            "wall_ms": round(wall_ms, 1), "poly_ms": round(st["ms"]["poly"], 1), "lap_ms": round(st["ms"]["lap"], 1),
            "gram_ms": round(st["ms"]["gram"], 1), "combine_ms": round(st["ms"]["combine"], 1),
            "resid_ms": round(st["ms"]["resid"], 1), "copy_ms": round(st["ms"]["copy"], 1), "kernel_ms": round(kernel_total, 1),
            "poly_share_of_wall": round(st["ms"]["poly"] / wall_ms, 3),
            "poly_share_of_kernels": round(st["ms"]["poly"] / kernel_total, 3),
            "shifted_cholqr": st.get("shifted_cholqr", 0),
            "worst_residual_over_b": st["worst_residual"] / b, "orthonormality": ortho, "kernels": kernels}


SCIPY_CHILD = r"""
import sys, time, json
sys.path.insert(0, {root!r})
import numpy as np
from scipy import sparse
from scipy.sparse import linalg as splinalg
from pygsp_amd.graphs import sensor_weights
W = sensor_weights({N}, k={nb}, seed=0, return_coords=False)
W = sparse.csr_matrix(W)
L = sparse.csr_matrix(sparse.diags(np.asarray(W.sum(axis=1)).ravel()) - W)
t0 = time.perf_counter()
e, U = splinalg.eigsh(L, {k}, which="SM")
ms = (time.perf_counter() - t0) * 1e3
r = np.linalg.norm(L @ U - U * e, axis=0).max()
print(json.dumps({{"ms": ms, "worst_residual": float(r)}}))
"""


def scipy_case(N, k, neighbours, timeout):
    code = SCIPY_CHILD.format(root=ROOT, N=N, nb=neighbours, k=k)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")  # host only
    t0 = time.perf_counter()
    try:
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired:
        return {"case": "scipy_eigsh_SM", "N": N, "k": k, "finished": False,
                "note": "did not finish in {} s".format(timeout)}
    if out.returncode != 0:
        return {"case": "scipy_eigsh_SM", "N": N, "k": k, "finished": False, "error": out.stderr.strip()[-300:]}
    res = json.loads(out.stdout.strip().splitlines()[-1])
    return {"case": "scipy_eigsh_SM", "N": N, "k": k, "finished": True, "eigsh_ms": round(res["ms"], 1),
            "worst_residual": res["worst_residual"], "child_wall_s": round(time.perf_counter() - t0, 1)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="100000:16,100000:64,1000000:16,1000000:64",
                    help="device cases N:k, comma separated")
    ap.add_argument("--neighbours", type=int, default=8)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--scipy", default="20000,50000,100000", help="sizes of the scipy baseline ('' for none)")
    ap.add_argument("--scipy-k", default="16,64")
    ap.add_argument("--scipy-timeout", type=float, default=600)
    args = ap.parse_args(argv)
    for case in filter(None, args.cases.split(",")):
        N, k = (int(v) for v in case.split(":"))
        print(json.dumps(device_case(N, k, args.neighbours, args.tol)), flush=True)
    for N in filter(None, args.scipy.split(",")):
        for k in filter(None, args.scipy_k.split(",")):
            print(json.dumps(scipy_case(int(N), int(k), args.neighbours, args.scipy_timeout)), flush=True)


if __name__ == "__main__":
    main()
