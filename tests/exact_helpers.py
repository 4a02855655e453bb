"""Shared by the exact-filtering tests: the fixture, a numpy restatement of what the device computes, and host
stand-ins for the two device calls (so the shape algebra and the refusals are testable without a GPU)."""
import numpy as np
from scipy import sparse

from conftest import csr_from, load_golden
from pygsp_amd import filters, graphs

_golden = {}


def golden():
    """tests/golden/exact_sensor123.npz, loaded once."""
    if "g" not in _golden:
        npz = load_golden("exact_sensor123.npz")
        _golden["g"] = {k: npz[k] for k in npz.files}
    return _golden["g"]


def golden_graph(**kwargs):
    """Sensor(123, seed=42) of the fixture with the reference's own e, U and lmax injected (needs a device)."""
    g = golden()
    G = graphs.Graph(csr_from(g, "W"), **kwargs)
    inject_basis(G, g["e"], g["U"])
    return G


def inject_basis(G, e, U):
    G._release_basis_dev()
    G._e, G._U = np.array(e), np.array(U)
    G._lmax, G._lmax_method = float(e[-1]), "fourier"


class HostGraph:
    """What the exact path reads from a Graph, without a device: the fixture's graph with the reference's basis, and
    the mirror Graph's own host transforms and coherence."""

    def __init__(self):
        g = golden()
        W = csr_from(g, "W")
        self.W, self.L = W, sparse.csr_matrix(sparse.diags(np.ravel(W.sum(1))) - W)
        self.N = self.n_vertices = W.shape[0]
        self.e, self.U, self.lmax = np.array(g["e"]), np.array(g["U"]), float(g["e"][-1])

    _check_signal, gft, igft = graphs.Graph._check_signal, graphs.Graph.gft, graphs.Graph.igft
    coherence = graphs.Graph.coherence

    def compute_fourier_basis(self, n_eigenvectors=None):
        self.e, self.U = np.linalg.eigh(self.L.toarray())


# ---- the restatement: the same matrices in numpy ---------------------------------------------------------------
def gram(A, B, r=None, alpha=1.0):
    """alpha A^T diag(r) B."""
    A = A if r is None else A * np.asarray(r)[:, None]
    return alpha * (A.T @ B)


def apply_planes(U, hat, H, mode):
    """hat: planes (F, n, w) of coefficients; H (Nf, n).  Returns planes (Nf, N, w) (analysis), (1, N, w) (synthesis:
    the H-weighted planes summed in filter order) or (1, N, w) (plain)."""
    if mode == "plain":
        return (U @ hat[0])[None]
    if mode == "analysis":
        return np.stack([U @ (H[g][:, None] * hat[0]) for g in range(H.shape[0])])
    Q = np.zeros_like(hat[0])
    for f in range(H.shape[0]):
        Q = Q + H[f][:, None] * hat[f]
    return (U @ Q)[None]


def exact_filter(U, H, cube):
    """Filter.filter(method='exact') on a cube (N, Nsig, Nfeat) -> (N, Nsig, Nf) or (N, Nsig, 1), not squeezed."""
    planes = np.moveaxis(cube, 2, 0)
    hat = np.stack([gram(U, p) for p in planes])
    out = apply_planes(U, hat, H, "synthesis" if cube.shape[2] != 1 else "analysis")
    return np.moveaxis(out, 0, 2)


def chebyshev_atoms(G, kernel, order=30):
    """p(L) of the identity, p the order-`order` Chebyshev polynomial of the one-filter bank `kernel` (host recurrence,
    approximations.py:99-112): column i is kernel.localize(i) / sqrt(N)."""
    c = filters.compute_cheby_coeff(kernel, m=order)
    L = sparse.csr_matrix(G.L, dtype=np.float64)
    N, a = G.N, G.lmax / 2.0
    old, cur = np.identity(N), (L @ np.identity(N) - a * np.identity(N)) / a
    acc = 0.5 * c[0] * old + c[1] * cur
    for k in range(2, order + 1):
        new = (2.0 / a) * (L @ cur - a * cur) - old
        acc = acc + c[k] * new
        old, cur = cur, new
    return acc


def modulation_localized(G, kernel, s):
    """Y = sqrt(N) (diag(s) T)^T U with T = sqrt(N) p(L): the matrix form of modulation.py:173-176."""
    root = np.sqrt(G.N)
    return gram(chebyshev_atoms(G, kernel), G.U, r=s, alpha=root * root)


# ---- host stand-ins for the device calls -----------------------------------------------------------------------
class HostPlanes:
    """What the stubs pass around in place of an engine.DeviceArray: planes [feature][vertex][signal] on the host."""

    def __init__(self, planes):
        self.planes_ = np.array(planes, dtype=np.float64)
        F, N, S = self.planes_.shape
        self.cube, self.dtype = (N, S, F), np.dtype(np.float64)
        self.shape = tuple(d for d in self.cube if d != 1)

    def numpy(self):
        return np.moveaxis(self.planes_, 0, 2).reshape(self.shape)

    def free(self):
        pass


def stub_device_calls(monkeypatch):
    """Replace the upload and the two device calls of filters._filter_exact by the restatement on host planes."""
    monkeypatch.setattr(filters, "_exact_upload", lambda G, cube: HostPlanes(np.moveaxis(cube, 2, 0)))

    def gft(G, a, S, F):
        N = a.cube[0]
        planes = np.moveaxis(np.moveaxis(a.planes_, 0, 2).reshape(N, S, F), 2, 0)
        return HostPlanes([gram(G.U, p) for p in planes]), 0.0

    def apply(G, hat, H, synthesis):
        return HostPlanes(apply_planes(G.U, hat.planes_, H, "synthesis" if synthesis else "analysis")), 0.0

    monkeypatch.setattr(filters, "_exact_gft", gft)
    monkeypatch.setattr(filters, "_exact_apply", apply)
