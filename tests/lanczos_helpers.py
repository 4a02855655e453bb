"""The numpy backend of pygsp_amd.lanczos (the algorithm restated on a scipy Laplacian, column by column), host
stand-ins for graphs and filters, and the dense reference filters the tests compare with."""
import types

import numpy as np
from scipy import sparse

from fourier_helpers import laplacian, ring, upper_bound  # noqa: F401  (re-exported for the lanczos tests)
from pygsp_amd import filters


class NumpyBackend:
    """pygsp_amd.lanczos's backend interface on a scipy Laplacian.  X is a host (N, n) array, Y a host (Nf N, n)
    array; the stack V of a batch is (order, N, width).  krylov() is the contract of DESIGN.md "Lanczos filtering",
    step for step: the three-term step, one full reorthogonalisation against q_0..q_k, the breakdown test."""

    def __init__(self, L, width=256):
        self.L = sparse.csr_matrix(L, dtype=np.float64)
        self.N = self.L.shape[0]
        self.width = int(width)
        self.batches = []

    def batch_width(self, order):
        return self.width

    def krylov(self, X, c0, c1, order, breakdown):
        x = np.asarray(X[:, c0:c1], dtype=np.float64)
        N, n = x.shape
        V = np.zeros((order, N, n))
        alpha, beta, proj = np.zeros((order, n)), np.zeros((order, n)), np.zeros((order, n))
        steps = np.zeros(n, dtype=np.int32)
        for c in range(n):
            xc = x[:, c]
            nx = np.linalg.norm(xc)
            beta[0, c] = nx
            if not (nx > 0 and np.isfinite(nx)):
                continue
            q = xc / nx
            V[0, :, c] = q
            w = self.L @ q
            alpha[0, c] = q @ w
            r = w - alpha[0, c] * q
            m = 1
            for k in range(1, order):
                b = np.linalg.norm(r)
                beta[k, c] = b
                if b <= breakdown:
                    break
                q = r / b
                V[k, :, c] = q
                w = self.L @ q - b * V[k - 1, :, c]
                alpha[k, c] = q @ w
                r = w - alpha[k, c] * q
                Vk = V[:k + 1, :, c]
                r = r - Vk.T @ (Vk @ r)
                m = k + 1
            steps[c] = m
            proj[:, c] = V[:, :, c] @ xc
        self.batches.append((c0, c1))
        return V, alpha, beta, proj, steps

    def combine(self, V, weights, Y, c0, c1):
        N = self.N
        for f in range(weights.shape[0]):
            Y[f * N:(f + 1) * N, c0:c1] = np.einsum("jnc,jc->nc", V, weights[f])

    def free(self, V):
        pass


def host_filter(kind, lmax, Nf=6):
    """This package's Heat(scale) ('heat<scale>') or MexicanHat(Nf) ('mexicanhat') on a host stand-in graph that only
    carries lmax (all the kernels read at construction)."""
    G = types.SimpleNamespace(lmax=float(lmax), N=None)
    if kind.startswith("heat"):
        return filters.Heat(G, scale=float(kind[4:]))
    return filters.MexicanHat(G, Nf=Nf)


def run_numpy(L, f, x, order, bound, width=256):
    """The driver on the numpy backend: (y of shape (Nf N,) or (Nf N, n), the backend, the driver's stats)."""
    x = np.asarray(x, dtype=np.float64)
    one_d = x.ndim == 1
    X = x[:, None] if one_d else x
    be = NumpyBackend(L, width)
    from pygsp_amd import lanczos
    Y = np.zeros((be.N * int(f.Nf), X.shape[1]))
    stats = lanczos.filter_columns(be, f, X, X.shape[1], order, bound, Y)
    return (Y[:, 0] if one_d else Y), be, stats


def exact_filter(L, f, x):
    """Dense eigh filtering y_i = U f_i(e) U^T x, filter-major rows (the reference's method='exact' layout)."""
    e, U = np.linalg.eigh(np.asarray(sparse.csr_matrix(L).toarray()))
    e[e < 0] = 0
    fe = np.asarray(f.evaluate(e)).reshape(int(f.Nf), -1)
    x = np.asarray(x, dtype=np.float64)
    X = x[:, None] if x.ndim == 1 else x
    Y = np.concatenate([U @ (fe[i][:, None] * (U.T @ X)) for i in range(int(f.Nf))])
    return Y[:, 0] if x.ndim == 1 else Y


def complete(n):
    return sparse.csr_matrix(np.ones((n, n)) - np.eye(n))


def star(n):
    W = sparse.lil_matrix((n, n))
    W[0, 1:] = 1
    W[1:, 0] = 1
    return sparse.csr_matrix(W)


def csr_from(g, prefix):
    return sparse.csr_matrix((g[prefix + "_data"], g[prefix + "_indices"], g[prefix + "_indptr"]),
                             shape=tuple(g[prefix + "_shape"]))


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))
