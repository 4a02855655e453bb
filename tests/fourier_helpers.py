"""Test-side pieces of the partial Fourier basis: the solver's backend in numpy (the product has no host backend),
the small graphs the solver is checked on, and the comparison against a dense eigendecomposition."""
import numpy as np
from scipy import sparse


class NumpyBackend:
    """pygsp_amd.fourier's backend interface on a scipy Laplacian.  poly() evaluates the program rows exactly as
    gspx_poly_program_dev defines them (old_is_x = 0): h_{s+1} = scale (2 t) h_s + beta h_s + gamma h_{s-1},
    t = (2 / b) L - I, gamma_0 ignored."""

    def __init__(self, L, b):
        self.L, self.N, self.b = sparse.csr_matrix(L, dtype=np.float64), L.shape[0], float(b)

    def width(self, X):
        return X.shape[1]

    def from_host(self, a):
        return np.array(a, dtype=np.float64)

    def to_host(self, X):
        return np.array(X)

    def view(self, X, j0, j1):
        return X[:, j0:j1]

    def free(self, X):
        pass

    def poly(self, program, X):
        old = cur = np.asarray(X)
        for s, (sc, be, ga) in enumerate(np.asarray(program)):
            two_t = (4.0 / self.b) * (self.L @ cur) - 2.0 * cur
            new = sc * two_t + be * cur + (ga * old if s > 0 else 0.0)
            old, cur = cur, new
        return np.array(cur)

    def lap(self, X):
        return np.asarray(self.L @ X)

    def gram(self, A, B):
        return np.asarray(A).T @ np.asarray(B)

    def combine(self, X, Q, out=None):
        Y = np.asarray(X) @ np.asarray(Q)
        if out is None:
            return Y
        out[...] = Y
        return out

    def copy(self, X, out=None):
        if out is None:
            return np.array(X)
        out[...] = X
        return out

    def resid(self, X, LX, theta):
        return np.linalg.norm(np.asarray(LX) - np.asarray(X) * np.asarray(theta)[None, :], axis=0)


def laplacian(W, lap_type):
    W = sparse.csr_matrix(W, dtype=np.float64)
    d = np.asarray(W.sum(axis=1)).ravel()
    if lap_type == "combinatorial":
        return sparse.csr_matrix(sparse.diags(d) - W)
    dis = np.zeros_like(d)
    dis[d > 0] = 1 / np.sqrt(d[d > 0])
    return sparse.csr_matrix(sparse.eye(W.shape[0]) - sparse.diags(dis) @ W @ sparse.diags(dis))


def upper_bound(W, lap_type):
    """2 for normalized Laplacians, 2 max degree (a rigorous bound of lambda_max) for combinatorial ones."""
    return 2.0 if lap_type == "normalized" else 2.0 * float(np.asarray(sparse.csr_matrix(W).sum(axis=1)).max())


def ring(n):
    i = np.arange(n)
    W = sparse.coo_matrix((np.ones(n), (i, (i + 1) % n)), shape=(n, n))
    return sparse.csr_matrix(W + W.T)


def path(n, w=None):
    i = np.arange(n - 1)
    w = np.ones(n - 1) if w is None else w
    W = sparse.coo_matrix((w, (i, i + 1)), shape=(n, n))
    return sparse.csr_matrix(W + W.T)


def grid(n, m=None):
    """The n x m 4-neighbour grid: eigenvalues of multiplicity two and close clusters."""
    m = n if m is None else m
    return sparse.csr_matrix(sparse.kronsum(path(m), path(n)))


def three_components():
    """A ring, a path and a weighted path side by side: eigenvalue 0 three times."""
    rng = np.random.default_rng(3)
    return sparse.csr_matrix(sparse.block_diag([ring(40), path(50), path(30, rng.uniform(0.5, 2.0, 29))]))


def check_against_dense(L, b, e, U, tol=1e-10, ortho=1e-12, gap=1e-3, subspace=1e-6):
    """Eigenvalues within tol * b of eigh, U^T U = I within `ortho`, and the subspace of every cluster of eigenvalues
    (consecutive ones closer than gap * b) equal to eigh's wherever the cluster is separated by more than gap * b
    from the rest of the spectrum (sin theta <= residual / gap)."""
    k = len(e)
    lam, V = np.linalg.eigh(L.toarray() if sparse.issparse(L) else L)
    assert np.max(np.abs(e - lam[:k])) <= tol * b, np.max(np.abs(e - lam[:k])) / b
    assert np.max(np.abs(U.T @ U - np.eye(k))) <= ortho
    start = 0
    checked = 0
    for i in range(1, k + 1):
        if i < k and lam[i] - lam[i - 1] <= gap * b:
            continue
        lo_ok = start == 0 or lam[start] - lam[start - 1] > gap * b
        hi_ok = i < len(lam) and lam[i] - lam[i - 1] > gap * b
        if lo_ok and hi_ok:
            Pu = U[:, start:i] @ U[:, start:i].T
            Pv = V[:, start:i] @ V[:, start:i].T
            assert np.linalg.norm(Pu - Pv, 2) <= subspace, (start, i)
            checked += 1
        start = i
    return checked
