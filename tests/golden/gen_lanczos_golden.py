#!/usr/bin/env python3
"""Generate tests/golden/lanczos_*.npz from the REAL reference (pygsp v0.6.1, the checkout named by $PYGSP_PATH).

    PYGSP_PATH=path/to/reference python tests/golden/gen_lanczos_golden.py

The reference's lanczos_op cannot run as shipped (it reads f.g, which Filter no longer has), so the expected outputs
are its own lanczos(L.toarray(), order, x), one column at a time, followed by the composition of lanczos_op:
eigendecomposition of H, negative Ritz values set to zero, V Uh (f_i(Eh) * Uh^T (V^T x)) per filter.  H is symmetric:
eigh stands for the reference's eig.  lmax is the reference's 'bounds' estimate (deterministic).
The fixtures are committed; tests read them, never the reference.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.environ["PYGSP_PATH"])
os.environ.setdefault("MPLBACKEND", "agg")
from pygsp import filters, graphs  # noqa: E402
from pygsp.filters.approximations import lanczos  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CASES = (("heat10", 30), ("mexicanhat6", 20), ("heat50", 60))


def reference_lanczos_op(f, L, x, order):
    Nf = f.Nf
    y = np.zeros((L.shape[0] * Nf, x.shape[1]))
    N = L.shape[0]
    for j in range(x.shape[1]):
        V, H, _ = lanczos(L, order, x[:, j])
        Eh, Uh = np.linalg.eigh(H)
        Eh[Eh < 0] = 0
        fe = np.asarray(f.evaluate(Eh)).reshape(Nf, -1)
        VU = V @ Uh
        for i in range(Nf):
            y[i * N:(i + 1) * N, j] = VU @ (fe[i] * (Uh.T @ (V.T @ x[:, j])))
    return y


def make(name, G):
    out = {}
    W = G.W.tocsr()
    W.sort_indices()
    out["W_indptr"], out["W_indices"], out["W_data"] = W.indptr.astype(np.int32), W.indices.astype(np.int32), W.data
    out["W_shape"] = np.array(W.shape)
    rng = np.random.default_rng(7)
    out["x1"] = rng.standard_normal(G.N)
    out["x5"] = rng.standard_normal((G.N, 5))
    for lap in ("combinatorial", "normalized"):
        G.compute_laplacian(lap)
        G.estimate_lmax("bounds")
        out["lmax_" + lap] = np.float64(G.lmax)
        L = G.L.toarray()
        for fname, order in CASES:
            if fname == "heat10":
                f = filters.Heat(G, scale=10)
            elif fname == "heat50":
                f = filters.Heat(G, scale=50)
            else:
                f = filters.MexicanHat(G, Nf=6)
            key = "{}_{}".format(lap, fname)
            out[key + "_order"] = np.int64(order)
            out[key + "_y1"] = reference_lanczos_op(f, L, out["x1"][:, None], order)[:, 0]
            out[key + "_y5"] = reference_lanczos_op(f, L, out["x5"], order)
    np.savez_compressed(os.path.join(OUT, "lanczos_{}.npz".format(name)), **out)


if __name__ == "__main__":
    make("sensor123", graphs.Sensor(123, seed=42))
    make("logo", graphs.Logo())
