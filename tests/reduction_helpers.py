"""A numpy restatement of the two device entry points behind pygsp_amd.reduction (gspx_schur_cg_dev and
gspx_kron_build, csrc/gspx_schur.hip.h) on top of the conjugate-gradient restatement of tests/cg_helpers.py, as
tests/dirichlet_helpers.py is for the harmonic extension, and the problems the CPU and GPU tests share.

    A = L + shift I, kept set k (mask), eliminated set u.  EMBEDDED in N rows:
    A_emb = P_u A P_u,  b = -(L (mask * f)) * ~mask,  x = cg.solve(A_emb, b) + mask * f,  alpha = mask * (A x)
    kron:  f = the indicator columns of ind;  S = (A X)[ind];  Lnew = (S + S^T) / 2;  W = max(0, -offdiag(Lnew))

The a-priori bound (ISSUE: per column j): ||delta||_2 <= ||A_ku||_2 rtol ||b_j||_2 / lambda_min(A_uu), plus a rounding
floor of 1e-13 max|ref|; without the ||A_ku|| factor for the extension x itself.
"""
import functools

import numpy as np
from scipy import sparse

import cg_helpers as cg
import dirichlet_helpers as dh
from learning_helpers import laplacian

X64_TOL, X32_TOL = cg.X64_TOL, cg.X32_TOL
RTOL_RANGE = dh.RTOL_RANGE
FLOOR = 1e-13


def shifted(L, shift):
    return sparse.csr_matrix(L + shift * sparse.identity(L.shape[0], format="csr"))


def extension(L, shift, mask, f, rtol, atol=0.0, maxiter=None, dt=np.float64, acc=np.float64):
    """(x, alpha, iterations, seq) for the Laplacian L (float64 sparse): x the shifted harmonic extension of f (read at
    kept rows only), alpha = A x at the kept rows and zero elsewhere, both (N, n) in dt."""
    keep = np.asarray(mask).reshape(-1) != 0
    f = np.asarray(f)
    f2 = f[:, None] if f.ndim == 1 else f
    L = sparse.csr_matrix(L)
    A = shifted(L, shift)
    Pu = sparse.diags((~keep).astype(np.float64))
    fl = np.where(keep[:, None], f2, 0.0).astype(dt)
    b = np.where(keep[:, None], 0.0, -np.asarray(L.astype(dt) @ fl)).astype(dt)
    xu, iters, seq = cg.solve(sparse.csr_matrix(Pu @ A @ Pu), b, rtol=rtol, atol=atol, maxiter=maxiter, dt=dt, acc=acc)
    x = np.where(keep[:, None], fl, xu)
    alpha = np.where(keep[:, None], np.asarray(A.astype(dt) @ x), 0.0).astype(dt)
    return x, alpha, iters, seq


def kron(L, shift, ind, rtol, maxiter=None, acc=np.longdouble):
    """(Lnew dense (nk, nk), W csr, iterations per kept vertex, seq): vertex ind[c] becomes vertex c."""
    ind = np.asarray(ind)
    N = L.shape[0]
    mask = np.zeros(N, dtype=bool)
    mask[ind] = True
    F = np.zeros((N, ind.size))
    F[ind, np.arange(ind.size)] = 1.0
    _, alpha, iters, seq = extension(L, shift, mask, F, rtol, maxiter=maxiter, acc=acc)
    S = alpha[ind]
    Lnew = (S + S.T) / 2
    return Lnew, adjacency_of(Lnew), iters, seq


def adjacency_of(Lnew):
    Wd = np.maximum(0.0, -Lnew)
    np.fill_diagonal(Wd, 0.0)
    W = sparse.csr_matrix(Wd)
    W.eliminate_zeros()
    return W


def direct(L, shift, ind):
    """The reference's formula (reduction.py:350-362) with a dense solve, float64."""
    A = shifted(L, shift).toarray()
    ind = np.asarray(ind)
    comp = np.setdiff1d(np.arange(A.shape[0]), ind)
    S = A[np.ix_(ind, ind)]
    if comp.size:
        S = S - A[np.ix_(ind, comp)] @ np.linalg.solve(A[np.ix_(comp, comp)], A[np.ix_(comp, ind)])
    return (S + S.T) / 2


def bounds(L, shift, ind, B, rtol, with_aku=True):
    """The a-priori bound per column of B (nk x n, the kept values in `ind` order): [||A_ku||_2] rtol ||A_uk B_j||_2 /
    lambda_min(A_uu), from the matrices themselves (eigvalsh / svd); zeros when nothing is eliminated."""
    A = shifted(L, shift).toarray()
    ind = np.asarray(ind)
    comp = np.setdiff1d(np.arange(A.shape[0]), ind)
    B = np.asarray(B, dtype=np.float64)
    if comp.size == 0:
        return np.zeros(B.shape[1])
    Auk = A[np.ix_(comp, ind)]
    lmin = float(np.linalg.eigvalsh(A[np.ix_(comp, comp)]).min())
    out = rtol * np.linalg.norm(Auk @ B, axis=0) / lmin
    return out * np.linalg.norm(Auk, 2) if with_aku else out


def within(x, ref, bound):
    """(ok, largest ratio): per column ||x - ref||_2 <= bound + FLOOR max|ref|."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    x, ref = (x[:, None], ref[:, None]) if x.ndim == 1 else (x, ref)
    lim = np.asarray(bound) + FLOOR * np.max(np.abs(ref), initial=0.0)
    err = np.linalg.norm(x - ref, axis=0)
    ratio = np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0))
    return bool((err <= lim).all()), float(ratio.max(initial=0.0))


def split_shift(M):
    """(W, sigma) when the sparse matrix M is Lap(W) + sigma I - symmetric, non-positive off-diagonals, one constant
    non-negative row sum - else None.  The rule of pygsp_amd.reduction.split_laplacian, restated."""
    M = sparse.csr_matrix(M, dtype=np.float64)
    if M.shape[0] != M.shape[1] or abs(M - M.T).max() != 0:
        return None
    off = M - sparse.diags(M.diagonal())
    off.eliminate_zeros()
    if off.nnz and off.data.max() > 0:
        return None
    rows = np.asarray(M.sum(axis=1)).ravel()
    sigma = float(np.median(rows)) if rows.size else 0.0
    scale = max(float(abs(M).max()), 1.0)
    if sigma < -1e-12 * scale or np.abs(rows - sigma).max() > 1e-12 * scale * max(M.shape[0], 1) ** 0.5:
        return None
    return sparse.csr_matrix(-off), max(sigma, 0.0)


def unpack(g, name):
    """A dense matrix of tests/golden/reduction.npz: stored whole, or as the upper triangle of a symmetric one."""
    if name in g.files:
        return np.asarray(g[name], dtype=np.float64)
    tri = g[name + "_triu"]
    n = int(round((np.sqrt(8 * tri.size + 1) - 1) / 2))
    M = np.zeros((n, n))
    M[np.triu_indices(n)] = tri
    return M + np.triu(M, 1).T


def golden_kron_cases(g):
    """(graph name, set name, shift index) of every Kron case of the fixture."""
    return [(gr, str(s), k) for gr in ("k64", "k300") for s in g["sets"] for k in range(len(g["shifts"]))]


# ---- the problems ---------------------------------------------------------------------------------------------------
def kept_set(name, N):
    """'even', 'third' (a shuffled third), 'one', 'five', 'all' (shuffled) or an integer count (shuffled)."""
    rng = np.random.default_rng(11 * N + 5)
    if name == "even":
        return np.arange(0, N, 2)
    if name == "one":
        return np.array([N // 2])
    count = {"third": max(N // 3, 1), "five": min(5, N), "all": N}.get(name, name)
    return rng.permutation(N)[:int(count)]


class Problem:
    """A graph of dirichlet_helpers (W, perm; 'split': two sensor graphs side by side, no vertex of the second one
    kept), a kept set and a shift; f: 3 signal columns on all N rows (NaN outside the kept set in nan_f)."""

    def __init__(self, kind, N, kept, shift):
        src = dh.problem(kind, N, 3)
        self.key, self.N, self.shift = (kind, N, kept, shift), N, shift
        self.W, self.perm, self.L = src.W, src.perm, laplacian(src.W)
        self.ind = kept_set(kept, 64 if kind == "split" else N)
        self.mask = np.zeros(N, dtype=bool)
        self.mask[self.ind] = True
        self.f = src.y[:, :3] * 1e6 if src.y.shape[1] >= 3 else src.y  # (columns 0-2 of cg.right_hand_sides: 1e-6 .. 1e-4)
        self.nan_f = np.where(self.mask[:, None], self.f, np.nan)


@functools.lru_cache(maxsize=None)
def problem(kind, N, kept, shift):
    return Problem(kind, N, kept, shift)


SHIFTS = (0.0, 0.005)
TINY = tuple(("random", N, kept, s) for N in (1, 2, 5) for kept in ("one", "all") for s in SHIFTS)
SENSORS = tuple(("sensor", N, kept, s) for N in (63, 64, 65, 300) for kept in ("even", "third") for s in SHIFTS)
BATCH_EDGE = tuple(("sensor", 600, nk, 0.005) for nk in (255, 256, 257))
TILE_EDGE = tuple(("sensor", 300, nk, 0.0) for nk in (63, 64, 65, 129))
# (one kept vertex at shift 0 is ONE_KEPT_UNSHIFTED: its exact result is the 1 x 1 zero matrix, what is computed is
# the cancellation of a degree against itself, and a deviation relative to the result has no meaning - the GPU test
# measures that one against the scale of the operands)
ALL_KEPT, ONE_KEPT, ONE_KEPT_UNSHIFTED = ("sensor", 65, "all", 0.005), ("sensor", 300, "one", 0.005), ("sensor", 300, "one", 0.0)
SPLIT = tuple(("split", 129, "third", s) for s in SHIFTS)
KRON_PROBLEMS = TINY + SENSORS + BATCH_EDGE + TILE_EDGE + (ALL_KEPT, ONE_KEPT) + SPLIT
BASE = ("sensor", 300, "third", 0.005)
# float32 (schur_cg only): the 300-vertex problems whose two float32 restatements - sums in float64 and in float32 -
# agree within X32_TOL / 10, the rule X32_TOL was made by (tests/test_reduction_host.py: test_fp32_admission).  One
# kept vertex of 300 at shift 0.005 is not admitted: 65 iterations on a block whose smallest eigenvalue is near the
# shift, and the two restatements already differ by 1.7e-6.
FP32_CANDIDATES = tuple(k for k in SENSORS if k[1] == 300) + (ONE_KEPT,)
FP32_EXCLUDED = (ONE_KEPT,)
FP32_PROBLEMS = tuple(k for k in FP32_CANDIDATES if k not in FP32_EXCLUDED)


def _acc(dtype):
    return np.longdouble if np.dtype(dtype) == np.float64 else np.float64


@functools.lru_cache(maxsize=None)
def kron_reference(key):
    """(Lnew, W, iterations, rtol) of the restatement at the rtol cg.pick_rtol chooses in [1e-11, 1e-9] from the
    residual sequences of a run down to 1e-11."""
    pb = problem(*key)
    lo, hi = RTOL_RANGE[np.dtype(np.float64)]
    seq = kron(pb.L, pb.shift, pb.ind, lo)[3]
    rtol, _ = cg.pick_rtol(seq, lo, hi)
    Lnew, W, iters, _ = kron(pb.L, pb.shift, pb.ind, rtol)
    return Lnew, W, iters, rtol


@functools.lru_cache(maxsize=None)
def schur_reference(key, dtype):
    """(x, alpha, iterations, rtol) of the restatement for the problem's f, rtol picked as above in the dtype's range."""
    pb = problem(*key)
    lo, hi = RTOL_RANGE[np.dtype(dtype)]
    seq = extension(pb.L, pb.shift, pb.mask, pb.f, lo, dt=dtype, acc=_acc(dtype))[3]
    rtol, _ = cg.pick_rtol(seq, lo, hi)
    x, alpha, iters, _ = extension(pb.L, pb.shift, pb.mask, pb.f, rtol, dt=dtype, acc=_acc(dtype))
    return x, alpha, iters, rtol
