"""The numpy restatement behind the edge-weight gradient tests (gspx_cheby_laplacian_grad_dev,
filters.cheby_op_vjp_laplacian / cheby_op_vjp_weights, pygsp_amd.nn.WeightedGraph): the recurrence slots, the Clenshaw
sequence of the cotangent, the two restrictions of dl/dL and the two chain rules to the pair weights, with the sparse L;
the same function of the weights in dense torch (for autograd); and a stand-in device object and graph that compute
with the restatement.  Everything in fp64."""
import numpy as np
from scipy import sparse

from autograd_helpers import OracleDevice
from oracle import cheby_oracle as orc
from spectrum_helpers import slots


def laplacian_grad_direct(L, lmax, coeffs, x, z, pairs, need_diag=True):
    """(gdiag (N,), goff (P,)) for y_f = c_f0/2 x + sum_k c_fk T_k(Lt) x and cotangent planes z (Nf, N, Nsig):
    Gbar = (2/lmax) sum_{k=1}^{M-1} phi_k b_k t_{k-1}^T with b_k = u_k + 2 Lt b_{k+1} - b_{k+2}, u_k = sum_f c_fk z_f;
    gdiag[i] = Gbar_ii, goff[p] = Gbar_st + Gbar_ts, summed over the columns.  pairs: (2, P) integers."""
    c = np.atleast_2d(np.asarray(coeffs, dtype=np.float64))
    x = np.asarray(x, dtype=np.float64).reshape(L.shape[0], -1)
    z = np.asarray(z, dtype=np.float64).reshape(c.shape[0], L.shape[0], -1)
    M, a = c.shape[1], lmax / 2.0
    s, t = np.asarray(pairs[0], dtype=np.int64), np.asarray(pairs[1], dtype=np.int64)
    T = slots(L, lmax, x, M - 1)
    gdiag, goff = np.zeros(L.shape[0]), np.zeros(s.size)
    b1, b2 = np.zeros_like(x), np.zeros_like(x)  # b_{k+1}, b_{k+2}
    for k in range(M - 1, 0, -1):
        u = np.einsum("f,fns->ns", c[:, k], z)
        b = u + (2.0 / a) * (L.dot(b1) - a * b1) - b2
        phi = (1.0 if k == 1 else 2.0) * 2.0 / lmax
        gdiag += phi * (b * T[k - 1]).sum(1)
        goff += phi * ((b[s] * T[k - 1][t]).sum(1) + (b[t] * T[k - 1][s]).sum(1))
        b1, b2 = b, b1
    return (gdiag if need_diag else None), goff


def weights_chain(W, lap_type, gdiag, goff_pairs, pairs, goff_edges=None):
    """dl/dw (P,) from the two restrictions: combinatorial gdiag[s] + gdiag[t] - goff; normalized through the entry
    -w sigma_s sigma_t and the degrees of both endpoints (goff_edges: goff over the upper-triangle edge list of W)."""
    s, t = np.asarray(pairs[0], dtype=np.int64), np.asarray(pairs[1], dtype=np.int64)
    if lap_type == "combinatorial":
        return gdiag[s] + gdiag[t] - goff_pairs
    C = sparse.triu(W, format="coo")
    d = np.ravel(W.sum(axis=1))
    sigma = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
    flow = goff_edges * C.data * sigma[C.row] * sigma[C.col]
    R = np.bincount(C.row, weights=flow, minlength=W.shape[0]) + np.bincount(C.col, weights=flow, minlength=W.shape[0])
    delta = np.where(d > 0, R / (2.0 * np.where(d > 0, d, 1.0)), 0.0)
    return -goff_pairs * sigma[s] * sigma[t] + delta[s] + delta[t]


def weights_grad_direct(W, lap_type, lmax, coeffs, x, z, pairs):
    """dl/dw (P,) of the pairs by the restatement, L built from W with the oracle."""
    L = orc.laplacian(W, lap_type)
    C = sparse.triu(W, format="coo")
    gdiag, gp = laplacian_grad_direct(L, lmax, coeffs, x, z, pairs)
    _, ge = laplacian_grad_direct(L, lmax, coeffs, x, z, np.stack([C.row, C.col]))
    return weights_chain(W, lap_type, gdiag, gp, pairs, ge)


def adjacency_of(N, pairs, w):
    """The symmetric CSR adjacency with weight w[p] on pair p (zeros dropped)."""
    w = np.asarray(w, dtype=np.float64)
    keep = w != 0
    s, t, w = np.asarray(pairs[0])[keep], np.asarray(pairs[1])[keep], w[keep]
    W = sparse.coo_matrix((np.concatenate([w, w]), (np.concatenate([s, t]), np.concatenate([t, s]))), shape=(N, N)).tocsr()
    W.sort_indices()
    return W


def torch_filter_dense(torch, N, pairs, w, lap_type, lmax, coeffs, x):
    """(Nf, N, Nsig): the filter of dense torch tensors, W assembled from the leaf vector `w` of pair weights - what
    autograd differentiates.  coeffs (Nf, M), x (N, Nsig) torch float64."""
    s, t = torch.as_tensor(np.asarray(pairs[0], dtype=np.int64)), torch.as_tensor(np.asarray(pairs[1], dtype=np.int64))
    W = torch.zeros((N, N), dtype=torch.float64)
    W = W.index_put((s, t), w, accumulate=True).index_put((t, s), w, accumulate=True)
    d = W.sum(1)
    if lap_type == "combinatorial":
        L = torch.diag(d) - W
    else:
        sig = torch.where(d > 0, d.clamp(min=1e-300) ** -0.5, torch.zeros_like(d))
        L = torch.diag((d > 0).to(torch.float64)) - sig[:, None] * W * sig[None, :]
    Lt = (2.0 / lmax) * L - torch.eye(N, dtype=torch.float64)
    T0, T1 = x, Lt @ x
    y = 0.5 * coeffs[:, 0, None, None] * T0[None] + coeffs[:, 1, None, None] * T1[None]
    for k in range(2, coeffs.shape[1]):
        T0, T1 = T1, 2.0 * (Lt @ T1) - T0
        y = y + coeffs[:, k, None, None] * T1[None]
    return y


class WgradDevice(OracleDevice):
    """Stands in for engine.DeviceGraph where filters.cheby_op_vjp_weights and the torch layer need one: the host-array
    call contract of cheby_filter and cheby_cross_moments (autograd_helpers.OracleDevice) and of cheby_laplacian_grad,
    arithmetic by the restatements.  pair_counts: the length of the pair list of every cheby_laplacian_grad call."""

    def __init__(self, W, lap_type, dtype=np.float64):
        super().__init__(orc.laplacian(W, lap_type), dtype)
        self.W, self.pair_counts = W, []

    def cheby_laplacian_grad(self, coeffs, x, z, lmax, pairs=None, need_diag=True):
        self.calls.append("laplacian_grad")
        if pairs is None:
            C = sparse.triu(self.W, format="coo")
            pairs = np.stack([C.row, C.col])
        self.pair_counts.append(np.shape(pairs)[1])
        gdiag, goff = laplacian_grad_direct(self.L, lmax, coeffs, x, z, pairs, need_diag)
        return gdiag, goff, 0.0


class WgradGraph:
    """What filters and nn read from a Graph - N, lmax, lap_type, W, is_directed, get_edge_list, device_graph,
    _check_signal - over a WgradDevice."""
    compute_dtype = np.dtype(np.float64)

    def __init__(self, W, lmax, lap_type="combinatorial", directed=False):
        self.W, self.N, self.lmax, self.lap_type, self._directed = W, W.shape[0], float(lmax), lap_type, directed
        self.dev = WgradDevice(W, lap_type)

    def is_directed(self):
        return self._directed

    def get_edge_list(self):
        C = sparse.triu(self.W, format="coo")
        return C.row, C.col, C.data

    def device_graph(self, dtype=None):
        return self.dev

    def _check_signal(self, s):
        s = np.asanyarray(s)
        if s.shape[0] != self.N:
            raise ValueError("First dimension must be the number of vertices G.N = {}, got {}.".format(self.N, s.shape))
        return s
