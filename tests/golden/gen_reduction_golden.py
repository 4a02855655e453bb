#!/usr/bin/env python3
"""Generate tests/golden/reduction.npz by running the REAL reference (pygsp v0.6.1, the checkout named by
$PYGSP_PATH): reduction.kron_reduction, interpolate, graph_multiresolution, pyramid_analysis / pyramid_synthesis.

    PYGSP_PATH=path/to/reference python tests/golden/gen_reduction_golden.py

Kron cases, graph g in {k64, k300} = Sensor(N, seed=3): <g>_W_* (CSR parts), <g>_coords, and per kept set s in `sets`
(even indices, the polarity set of the last eigenvector, a shuffled third, 5 random vertices): <g>_<s>_ind,
<g>_<s>_L0 / _L1 = the matrix form kron_reduction(L + sigma I, ind) for sigma = `shifts`[0 / 1], and <g>_<s>_GW, the
W of the Graph form (sigma = 0).  A dense symmetric matrix is stored as its upper triangle, row-major (<name>_triu,
see `pack`; tests/reduction_helpers.py: `unpack`); one that is not symmetric is stored whole.
Interpolate cases on k64, sets even and third: i_<s>_f (nk, 3), i_<s>_Kf = K_reg f, i_<s>_cheb (order 100) and
i_<s>_exact (method='exact'), with G.mr = {} and a Fourier basis; i_lmax, i_e (the eigenvalues), `reg_eps`.  The
reference's legacy `_analysis` stacks the Nv columns of a result into (N Nv, 1); they are stored as (N, Nv).
Pyramid case: graph_multiresolution(Sensor(64, seed=3), 2, sparsify=False, compute_full_eigen=True): p_idx<l>,
p_W<l> (level l = 1, 2, packed like the others), p_lmax (levels 0..2), p_f (64, 2), p_ca<l>, p_pe<l>, p_rec.  The
reference is run on one column of p_f at a time and the results are put side by side: given both columns at once it
indexes the stacked result with the kept vertices and so carries only column 0 to the next level.
Arrays only; the fixture is committed, tests read it, never the reference.
"""
import os
import sys

import numpy as np
from scipy import sparse

sys.path.insert(0, os.environ["PYGSP_PATH"])
os.environ.setdefault("MPLBACKEND", "agg")
from pygsp import graphs, reduction  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SHIFTS = (0.0, 0.005)
REG_EPS = 0.005


def csr_parts(M, prefix):
    M = sparse.csr_matrix(M)
    M.sum_duplicates()
    M.sort_indices()
    return {prefix + "_indptr": M.indptr.astype(np.int32), prefix + "_indices": M.indices.astype(np.int32),
            prefix + "_data": M.data.astype(np.float64), prefix + "_shape": np.array(M.shape)}


def dense_of(M):
    return np.asarray(M.todense() if sparse.issparse(M) else M, dtype=np.float64)


def pack(out, name, M):
    """A dense matrix: its upper triangle when it equals its transpose bit for bit, else all of it."""
    M = dense_of(M)
    if np.array_equal(M, M.T):
        out[name + "_triu"] = M[np.triu_indices(M.shape[0])]
    else:
        out[name] = M


def columns(stacked, n):
    """(N Nv, 1), the columns one below the other, as (N, Nv)."""
    return np.asarray(stacked).reshape(-1, n).T.copy()


def kept_sets(G):
    N = G.N
    rng = np.random.default_rng(100 + N)
    V = np.array(G.U[:, -1])
    V *= np.sign(V[0])
    return {"even": np.arange(0, N, 2), "polarity": np.nonzero(V >= 0)[0], "third": rng.permutation(N)[:N // 3],
            "five": rng.choice(N, 5, replace=False)}


def main():
    out = {"shifts": np.array(SHIFTS), "reg_eps": np.float64(REG_EPS), "sets": np.array(["even", "polarity", "third", "five"])}
    for N in (64, 300):
        g = "k%d" % N
        G = graphs.Sensor(N, seed=3)
        G.compute_fourier_basis()
        out.update(csr_parts(G.W, g + "_W"))
        out[g + "_coords"] = np.asarray(G.coords)
        for s, ind in kept_sets(G).items():
            out["%s_%s_ind" % (g, s)] = ind.astype(np.int64)
            for k, sigma in enumerate(SHIFTS):
                pack(out, "%s_%s_L%d" % (g, s, k), reduction.kron_reduction(G.L + sigma * sparse.eye(N), ind))
            Gn = reduction.kron_reduction(G, ind)
            assert np.allclose(Gn.coords, G.coords[ind])
            pack(out, "%s_%s_GW" % (g, s), Gn.W)

    G = graphs.Sensor(64, seed=3)
    G.compute_fourier_basis()
    G.mr = {}
    out["i_lmax"], out["i_e"] = np.float64(G.lmax), np.asarray(G.e)
    rng = np.random.default_rng(7)
    for s in ("even", "third"):
        ind = kept_sets(G)[s]
        f = rng.standard_normal((ind.size, 3))
        out["i_%s_f" % s] = f
        out["i_%s_Kf" % s] = np.asarray(reduction.kron_reduction(G.L + REG_EPS * sparse.eye(G.N), ind).dot(f))
        out["i_%s_cheb" % s] = columns(reduction.interpolate(G, f, ind, order=100, reg_eps=REG_EPS), G.N)
        out["i_%s_exact" % s] = columns(reduction.interpolate(G, f, ind, reg_eps=REG_EPS, method="exact"), G.N)

    G = graphs.Sensor(64, seed=3)
    Gs = reduction.graph_multiresolution(G, 2, sparsify=False, compute_full_eigen=True)
    out["p_lmax"] = np.array([g.lmax for g in Gs])
    for l in (1, 2):
        out["p_idx%d" % l] = np.asarray(Gs[l].mr["idx"]).astype(np.int64)
        pack(out, "p_W%d" % l, Gs[l].W)
    f = np.random.default_rng(8).standard_normal((64, 2))
    runs = []
    for c in range(f.shape[1]):
        ca, pe = reduction.pyramid_analysis(Gs, f[:, [c]])
        runs.append((ca, pe, reduction.pyramid_synthesis(Gs, ca[2], pe)[0]))
    out["p_f"] = f
    out["p_rec"] = np.hstack([np.asarray(r[2]).reshape(64, 1) for r in runs])
    for l in range(3):
        out["p_ca%d" % l] = np.hstack([np.asarray(r[0][l]).reshape(-1, 1) for r in runs])
    for l in range(2):
        out["p_pe%d" % l] = np.hstack([np.asarray(r[1][l]).reshape(-1, 1) for r in runs])
    path = os.path.join(OUT, "reduction.npz")
    np.savez_compressed(path, **out)
    print("reduction.npz: {} arrays, {} bytes".format(len(out), os.path.getsize(path)))
    for k in sorted(out):
        print(" ", k, np.shape(out[k]))


if __name__ == "__main__":
    main()
