"""What the modules that pin the Lanczos combine, the squared norms, grad / div and L x at small shapes share
(tests/test_gpu_u_*.py): plain numpy restatements with the error bounds that go with them, and the tiny graphs.
tests/test_operator_pins_host.py checks every one of them against a slower direct formula, without a GPU."""
import numpy as np
from scipy import sparse

from conftest import rel_err
from gpu_helpers import random_graph, upper_lmax
from oracle import cheby_oracle as orc

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


# ---- Lanczos: y_f = sum_j w[f][j] V_j and V^T x ------------------------------------------------------------------
def combine_reference(V, w):
    """V (order, N, n), w (Nf, order, n) -> (ref, bound), both (Nf, N, n) longdouble, rows in the order of V's:
    ref[f, i, c] = sum_j w[f, j, c] V[j, i, c] and bound = (order + 1) eps (|w| . |V|), the bound of an order-term
    float64 sum of float64 products in any order, fused or not."""
    V, w = np.asarray(V, dtype=LD), np.asarray(w, dtype=LD)
    ref = np.einsum("fjc,jic->fic", w, V)
    mag = np.einsum("fjc,jic->fic", np.abs(w), np.abs(V))
    return ref, (V.shape[0] + 1) * LD(EPS) * mag


def projection_reference(V, x):
    """V (order, N, n) and x (N, n) in one row order -> (proj, bound), both (order, n) longdouble:
    proj[j, c] = sum_i V[j, i, c] x[i, c], bound = (N + 2) eps (|V|^T |x|)."""
    V, x = np.asarray(V, dtype=LD), np.asarray(x, dtype=LD)
    proj = np.einsum("jic,ic->jc", V, x)
    mag = np.einsum("jic,ic->jc", np.abs(V), np.abs(x))
    return proj, (V.shape[1] + 2) * LD(EPS) * mag


def caller_rows(a, perm, axis):
    """The rows (axis `axis`) of an internal-order array in the caller's order: internal row i is the caller's row
    perm[i] (DeviceGraph.download_perm; None: the same order)."""
    if perm is None:
        return a
    out = np.empty_like(a)
    idx = [slice(None)] * a.ndim
    idx[axis] = np.asarray(perm)
    out[tuple(idx)] = a
    return out


def shuffled_order(rng, n):
    """A random vertex permutation (int32) that is not the identity, which the library would drop (n = 1: the only
    one there is)."""
    perm = rng.permutation(n).astype(np.int32)
    if n > 1 and np.array_equal(perm, np.arange(n)):
        perm = np.roll(perm, 1)
    return perm


# ---- squared norms of a Chebyshev bank, the recurrence carried in float32 ----------------------------------------
def bank_coefficients(nf, M, seed):
    """(nf, M) coefficients that decay like 1 / sqrt(k + 1): every order carries weight far above any tolerance, so a
    wrong slot at a high order shows, and the outputs stay of order one."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nf, M)) / np.sqrt(np.arange(1, M + 1))


def sqnorms_carried(L, lmax, C, x, dtype):
    """(Nf, w) float64: s[f][j] = sum_rows (sum_k c'_fk T_k[row][j])^2 with c'_f0 = c_f0 / 2, the T_k carried in
    `dtype` (the matrix, lmax / 2 and the panels in it; the oracle's order of operations), every y formed from the
    float64 coefficients, squared and summed in float64 at least.  float32: what a float32 graph can give at best;
    longdouble (a dense matrix: scipy's sparse product has none): what to measure the float64 oracle with."""
    C = np.atleast_2d(np.asarray(C, dtype=np.float64))
    M = C.shape[1]
    dt = np.dtype(dtype)
    wide = np.float64 if dt.itemsize <= 8 else dt
    A = sparse.csr_matrix(L, dtype=dt) if dt.itemsize <= 8 else np.asarray(sparse.csr_matrix(L).toarray(), dtype=dt)
    a = dt.type(float(lmax)) / dt.type(2)
    two_over_a = dt.type(2) / a
    T = [np.ascontiguousarray(x, dtype=dt)]
    T.append((A.dot(T[0]) - a * T[0]) / a)
    for k in range(2, M):
        T.append(two_over_a * (A.dot(T[k - 1]) - a * T[k - 1]) - T[k - 2])
    assert all(t.dtype == dt for t in T)
    T = np.stack(T[:M]).astype(wide)
    cp = C.astype(wide)
    cp[:, 0] *= 0.5
    y = np.tensordot(cp, T, axes=(1, 0))
    return np.einsum("fnw,fnw->fw", y, y).astype(np.float64)


def sqnorms_bar(L, lmax, C, x, dtype, ref, tol):
    """(bar, figure) for the device's squared norms from M >= 128 coefficients, where the project has no tolerance
    of its own: `ref` is the float64 oracle's result on x (already rounded to `dtype`), tol the bar of the short
    recurrences (gpu_helpers.TOL).
    float32: figure = rel_err of the float32 recurrence above against the oracle; the device gets max(tol, 4 figure) -
    the factor 4 covers another summation order within a row and the FMA contraction.
    float64: figure = rel_err of the oracle against the longdouble recurrence, i.e. the oracle's own error; the device
    keeps tol unless the oracle itself misses it, and then gets 4 figure as well."""
    if np.dtype(dtype) == np.float32:
        figure = rel_err(sqnorms_carried(L, lmax, C, x, np.float32), ref)
        return max(tol, 4 * figure), figure
    figure = rel_err(ref, sqnorms_carried(L, lmax, C, x, np.longdouble))
    return (tol if figure <= tol else 4 * figure), figure


def oracle_sqnorms(L, lmax, C, x):
    """The float64 oracle's squared norms (cheby_op, then the sum of squares), as test_gpu_e_features has them."""
    y = orc.cheby_op(L, lmax, C, x).reshape(np.atleast_2d(C).shape[0], L.shape[0], -1)
    return np.einsum("fnw,fnw->fw", y, y)


LONG_NF, LONG_M, LONG_W = (1, 9, 100), (128, 129, 200, 256), 5
_LONG = {}


def long_case(nf, M, dtype):
    """(L, lmax, coefficients, the 257 x 5 input rounded to dtype, the float64 oracle's squared norms) of the
    M >= 128 cases, computed once per process."""
    key = (nf, M, np.dtype(dtype).name)
    if key not in _LONG:
        W = random_graph(257, 4, seed=257)
        L, lmax = orc.laplacian(W), upper_lmax(W)
        C = bank_coefficients(nf, M, seed=1000 * nf + M)
        x = np.random.default_rng(M).standard_normal((257, LONG_W)).astype(dtype).astype(np.float64)
        _LONG[key] = (W, L, lmax, C, x, oracle_sqnorms(L, lmax, C, x))
    return _LONG[key]


def no_polynomials(lmax):
    """tile_helpers.case without an oracle run: the modules here compute their own references."""
    return {}


# ---- tiny graphs -------------------------------------------------------------------------------------------------
def symmetric(rows, cols, vals, n):
    A = sparse.coo_matrix((np.asarray(vals, dtype=np.float64), (rows, cols)), shape=(n, n))
    W = sparse.csr_matrix(A + A.T)
    W.sum_duplicates()
    W.sort_indices()
    return W


def path_graph(n, seed=0):
    """A weighted path on n vertices (n = 1: one vertex without an edge)."""
    w = np.random.default_rng(seed).uniform(0.5, 1.5, max(n - 1, 0))
    return symmetric(np.arange(n - 1), np.arange(1, n), w, n)


def star_graph(leaves, hub_last=False, seed=0):
    """A weighted star: the hub is vertex 0 (every edge of the edge list has it as its source) or, with hub_last, the
    last vertex (every edge has it as its target)."""
    n = leaves + 1
    w = np.random.default_rng(seed).uniform(0.5, 1.5, leaves)
    if hub_last:
        return symmetric(np.arange(leaves), np.full(leaves, n - 1), w, n)
    return symmetric(np.zeros(leaves, dtype=np.int64), np.arange(1, n), w, n)


def isolated_vertex_graph():
    """6 vertices, vertex 3 without an edge: a triangle 0-1-2 with a tail 2-4-5."""
    return symmetric([0, 1, 0, 2, 4], [1, 2, 2, 4, 5], [1.0, 0.5, 2.0, 0.25, 1.5], 6)


def edgeless_graph(n):
    return sparse.csr_matrix((n, n), dtype=np.float64)


def directed_graph(n=40, seed=7):
    A = sparse.random(n, n, 0.1, random_state=seed, format="csr")
    A.setdiag(0)
    A.eliminate_zeros()
    A.sort_indices()
    return A


def self_loop_graph(n=40, seed=8):
    S = sparse.random(n, n, 0.06, random_state=seed, format="csr")
    S = (S + S.T).tolil()
    S.setdiag(np.where(np.arange(n) % 7 == 0, 0.5, 0.0))
    S = S.tocsr()
    S.eliminate_zeros()
    S.sort_indices()
    return S
