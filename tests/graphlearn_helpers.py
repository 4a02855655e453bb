"""A numpy restatement of graph learning from smooth signals (pygsp_amd.graph_learning, DESIGN.md "Graph learning"; the
device side is csrc/gspx_graphlearn.hip.h), written from the math; the CPU and GPU tests compare against it.

The log-degree model (Kalofolias 2016) on a fixed undirected pattern without self-loops.  Edge e = (s_e, t_e), s_e < t_e,
in Graph.get_edge_list order; (S w)_i = sum of w over the edges at vertex i, (S^T v)_e = v_s + v_t.  Over w >= 0 minimise

    F(w) = 2 z^T w - a sum_i log (S w)_i + b ||w||^2,   a > 0, b >= 0          (vertices without edges take no part)

by forward-backward-forward primal-dual iterations with the fixed step gamma = step / (2 b + sqrt(2 dmax)), from w_0
(zeros unless given) and v_0 = S w_0; for k = 1, 2, ...

    Y = w - gamma (2 b w + S^T v)          y = v + gamma S w
    P = max(0, Y - 2 gamma z)              p = prox(y)
    Q = P - gamma (2 b P + S^T p)          q = p + gamma S P
    w <- w - Y + Q                         v <- v - y + q

prox(y) = (y - r) / 2 for y <= 0 and -2 a gamma / (y + r) for y > 0, r = sqrt(y^2 + 4 a gamma).  Stop after iteration k
when ||w_k - w_{k-1}|| <= tol ||w_k|| and ||v_k - v_{k-1}|| <= tol ||v_k|| ('TOL'; tol None: off) or k >= maxit
('MAXIT').  The result is P of the last iteration.
"""
import numpy as np
from scipy import sparse


def pattern_edges(W):
    """(sources, targets) of the upper triangle of W in row-major order: Graph.get_edge_list of an undirected graph."""
    C = sparse.triu(sparse.csr_matrix(W), k=1, format="coo")
    order = np.lexsort((C.col, C.row))
    return C.row[order].astype(np.int64), C.col[order].astype(np.int64)


def gamma_for(src, dst, N, b, step=0.5):
    dmax = int((np.bincount(src, minlength=N) + np.bincount(dst, minlength=N)).max()) if src.size else 0
    return step / (2.0 * b + np.sqrt(2.0 * dmax))


def prox(y, a, gamma):
    r = np.sqrt(y * y + 4 * a * gamma)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(y <= 0, (y - r) / 2, -2 * a * gamma / (y + r))


def solve(src, dst, N, z, a, b, gamma, tol=1e-5, maxit=10000, w0=None, dtype=np.float64):
    """The iteration and its stopping rule in `dtype` arithmetic.  Returns (P, w, info): info has niter, crit ('TOL' or
    'MAXIT'), history (niter x 4: ||dw||, ||w||, ||dv||, ||v||) and the dual iterate v."""
    src, dst = np.asarray(src), np.asarray(dst)
    E = src.size
    z = np.asarray(z, dtype=dtype)
    a, b, gamma = dtype(a), dtype(b), dtype(gamma)
    fast = dtype is np.float64 or dtype == np.float64
    Sm = sparse.csr_matrix((np.ones(2 * E), (np.concatenate([src, dst]), np.concatenate([np.arange(E)] * 2))),
                           shape=(N, E)) if fast else None
    connected = (np.bincount(src, minlength=N) + np.bincount(dst, minlength=N)) > 0

    def S(w):
        if fast:
            return Sm @ w
        out = np.zeros(N, dtype=dtype)
        np.add.at(out, src, w)
        np.add.at(out, dst, w)
        return out

    def St(v):
        return v[src] + v[dst]

    w = np.zeros(E, dtype=dtype) if w0 is None else np.array(w0, dtype=dtype)
    v = S(w)
    hist = []
    P = np.zeros(E, dtype=dtype)
    k = 0
    if E == 0:
        return P, w, {"niter": 0, "crit": None, "history": np.zeros((0, 4)), "v": v}
    while True:
        k += 1
        Y = w - gamma * (2 * b * w + St(v))
        y = v + gamma * S(w)
        P = np.maximum(0, Y - 2 * gamma * z)
        p = np.where(connected, prox(y, a, gamma), 0).astype(dtype)
        Q = P - gamma * (2 * b * P + St(p))
        q = p + gamma * S(P)
        wn = w - Y + Q
        vn = v - y + q
        row = (np.sqrt(np.sum((wn - w) ** 2)), np.sqrt(np.sum(wn ** 2)), np.sqrt(np.sum((vn - v) ** 2)),
               np.sqrt(np.sum(vn ** 2)))
        hist.append(row)
        w, v = wn, vn
        crit = None
        if tol is not None and tol >= 0 and row[0] <= tol * row[1] and row[2] <= tol * row[3]:
            crit = "TOL"
        elif k >= maxit:
            crit = "MAXIT"
        if crit:
            return P, w, {"niter": k, "crit": crit, "history": np.array(hist, dtype=dtype), "v": v}


def objective(src, dst, N, z, a, b, w):
    d = np.bincount(src, weights=w, minlength=N) + np.bincount(dst, weights=w, minlength=N)
    connected = (np.bincount(src, minlength=N) + np.bincount(dst, minlength=N)) > 0
    return 2 * np.dot(z, w) - a * np.sum(np.log(d[connected])) + b * np.dot(w, w)


def kkt_residual(src, dst, N, z, a, b, P):
    """The projected gradient of F at the feasible point P: the gradient 2 z - a (1 / d_s + 1 / d_t) + 2 b P, d = S P,
    on the positive entries and its negative part on the zero entries.  Zero exactly at the solution; F is 2b-strongly
    convex, so ||P - w*||_2 <= ||residual||_2 / (2 b)."""
    P = np.asarray(P)
    d = np.zeros(N, dtype=P.dtype)
    np.add.at(d, src, P)
    np.add.at(d, dst, P)
    grad = 2 * np.asarray(z, dtype=P.dtype) - a * (1 / d[src] + 1 / d[dst]) + 2 * b * P
    return np.where(P > 0, grad, np.minimum(grad, 0))


def assert_rule_is_decisive(info, tol, margin=1e-6):
    """A condition on the INPUTS of a comparison of iteration counts (the idiom of fista_helpers): at every iteration
    of the restatement each residual stays a relative `margin` away from tol times its norm, so that rounding
    differences between two implementations cannot move niter."""
    for k, (dw, nw, dv, nv) in enumerate(np.asarray(info["history"], dtype=np.float64), start=1):
        for value, th in ((dw, tol * nw), (dv, tol * nv)):
            assert abs(value - th) >= margin * abs(th), (k, value, th)


def theta_bounds_rows(D, k):
    """Per row of D ((N, m) sorted neighbour distances, m > k >= 2; the point itself is not among them): with Z = D^2
    and b_k the sum of the k smallest, the single-vertex problem min theta z^T w - log(sum w) + ||w||^2 / 2 keeps exactly
    k edges for theta in [lo, hi): lo = 1 / sqrt(k Z_{k+1}^2 - b_k Z_{k+1}), hi = 1 / sqrt(k Z_k^2 - b_k Z_k) (1-based;
    Kalofolias & Perraudin 2019).  Returns (lo, hi, ok): ok marks the rows whose two radicands are positive."""
    D = np.asarray(D, dtype=np.float64)
    Z = D * D
    bk = Z[:, :k].sum(axis=1)
    rlo = k * Z[:, k] ** 2 - bk * Z[:, k]
    rhi = k * Z[:, k - 1] ** 2 - bk * Z[:, k - 1]
    ok = (rlo > 0) & (rhi > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 1 / np.sqrt(rlo), 1 / np.sqrt(rhi), ok


def theta_bounds(D, k):
    """Geometric means of lo and hi over the rows whose radicands are positive."""
    lo, hi, ok = theta_bounds_rows(D, k)
    if not ok.any():
        raise ValueError("no row has a positive radicand")
    return float(np.exp(np.mean(np.log(lo[ok])))), float(np.exp(np.mean(np.log(hi[ok]))))


def single_vertex_solution(zrow, theta, k):
    """w_j = max(0, 1 / s - theta z_j) with s^2 + theta b_k s - k = 0, b_k the sum of the k smallest z."""
    bk = np.sort(zrow)[:k].sum()
    s = (-theta * bk + np.sqrt(theta * theta * bk * bk + 4 * k)) / 2
    return np.maximum(0, 1 / s - theta * zrow)


def sensor_like(N, k, seed):
    """Uniform 2-D points and their symmetric k-NN pattern (host KD-tree): (points, src, dst, z) with z the squared
    edge lengths scaled to mean 1."""
    from scipy import spatial
    pts = np.random.default_rng(seed).uniform(0, 1, (N, 2))
    _, nbr = spatial.cKDTree(pts).query(pts, k=k + 1)
    A = sparse.csr_matrix((np.ones(N * k), (np.repeat(np.arange(N), k), nbr[:, 1:].ravel())), shape=(N, N))
    src, dst = pattern_edges(A + A.T)
    z = np.sum((pts[src] - pts[dst]) ** 2, axis=1)
    return pts, src, dst, z / z.mean()
