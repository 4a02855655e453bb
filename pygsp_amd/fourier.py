"""Partial graph Fourier bases: the k smallest eigenpairs of L by Chebyshev-filtered subspace iteration (ChFSI,
Zhou & Saad 2007).  What ``Graph.compute_fourier_basis(n_eigenvectors=k)`` runs on the device (DESIGN.md section
"Partial Fourier bases").
The full basis (``method='jacobi'``: block Jacobi on the dense L, gspx_sym_eig_dev) is at the end of the file (DESIGN.md
section "The full Fourier basis").

The loop is host Python over a small backend: only p x p matrices reach the host (Cholesky and eigh on p <= 512).
The backend does every N x p pass:

    poly(program, X)        the Chebyshev filter, a gspx_poly_program_dev program (old_is_x = 0, lmax = b)
    lap(X)                  L X (gspx_laplacian_apply_dev)
    gram(A, B)              A^T B to the host (gspx_panel_gram_dev)
    combine(X, Q, out)      X Q, optionally into a column view of another panel (gspx_panel_combine_dev)
    resid(X, LX, theta)     ||LX_i - theta_i X_i|| (gspx_panel_residual_norms_dev)
    copy(X, out)            X into a whole panel or a column view (gspx_panel_copy_dev)
    empty / view / from_host / to_host / free   panel bookkeeping

``DeviceBackend`` is the product's.  There is no host backend here: the tests carry a numpy one, so the algorithm is
testable without a GPU and the product keeps no CPU fallback.
"""
import math

import numpy as np
from scipy import linalg as sla

# a partial request goes to the device when the graph is this large and the block is this narrow against it
AUTO_MIN_VERTICES = 2048
AUTO_MAX_BLOCK_FRACTION = 0.25
MAX_BLOCK = 512          # widest panel of the solver's primitives (gram to the host, combine, residuals, copy)
BLOCK_QUANTUM = 16       # the block is rounded up to a multiple of this (why not 32)
AMPLIFICATION_LIMIT = 1e6  # largest ratio one filter may put between the first and the slowest active vector


def block_width(k, n_vertices=None):
    """p = k + g, g >= max(8, ceil(k / 4)) guard vectors, rounded up to a multiple of BLOCK_QUANTUM (at most the
    number of vertices).  The device solver takes blocks of at most MAX_BLOCK columns (k <= 409)."""
    k = int(k)
    p = k + max(8, -(-k // 4))
    p = -(-p // BLOCK_QUANTUM) * BLOCK_QUANTUM
    if n_vertices is not None:
        p = min(p, int(n_vertices))
    return p


def use_device(n_vertices, k):
    """method='auto': the device solver for large graphs and narrow blocks, dense eigh otherwise."""
    p = block_width(k)
    return n_vertices >= AUTO_MIN_VERTICES and p <= MAX_BLOCK and p <= AUTO_MAX_BLOCK_FRACTION * n_vertices


def sigmas(a0, a, b, m):
    """The scaling factors sigma_1..sigma_m of the scaled Chebyshev filter of degree m on [a, b] with scaling point
    a0 < a: sigma_1 = e / (a0 - c), sigma_{s+1} = 1 / (2 / sigma_1 - sigma_s)."""
    c, e = (a + b) / 2.0, (b - a) / 2.0
    out = [e / (a0 - c)]
    for _ in range(1, m):
        out.append(1.0 / (2.0 / out[0] - out[-1]))
    return out


def filter_program(a0, a, b, m):
    """(m, 3) rows (scale, beta, gamma) of gspx_poly_program_dev (old_is_x = 0, lmax = b, t = (2 / b) L - I;
    h_{s+1} = scale (2 t) h_s + beta h_s + gamma h_{s-1}) evaluating Y_m of the recurrence
        Y_1 = (sigma_1 / e)(L - c) X,   Y_{s+1} = (2 sigma_{s+1} / e)(L - c) Y_s - sigma_s sigma_{s+1} Y_{s-1},
    c = (a + b) / 2, e = (b - a) / 2: Y_m = C_m(t) X / C_m(t(a0)), t(x) = (x - c) / e."""
    c, e = (a + b) / 2.0, (b - a) / 2.0
    sg = sigmas(a0, a, b, m)
    rows = [(sg[0] * b / (4 * e), sg[0] * (b / 2 - c) / e, 0.0)]
    for s in range(1, m):
        rows.append((sg[s] * b / (2 * e), 2 * sg[s] * (b / 2 - c) / e, -sg[s - 1] * sg[s]))
    return np.array(rows, dtype=np.float64)


def choose_degree(theta, resid, active, a, b, tol_abs, bounds):
    """Degree of the next filter: enough for the slowest unconverged wanted vector j to reach the tolerance,
    cosh(m acosh|t_j|) >= r_j / tol_abs with t_j = (theta_j - c) / e (the damped interval [a, b] maps into [-1, 1]),
    capped so that the first active vector is amplified at most AMPLIFICATION_LIMIT times more than that slowest one
    (the filtered block stays well conditioned for CholQR2), and kept within `bounds`."""
    lo, hi = bounds
    c, e = (a + b) / 2.0, (b - a) / 2.0
    if not active:
        return lo
    rate = lambda th: math.acosh(max(abs((th - c) / e), 1.0 + 1e-15))
    needs = [(math.acosh(max(resid[j] / tol_abs, 1.0)) / rate(theta[j]), j) for j in active]
    need, slow = max(needs)
    m = int(math.ceil(need))
    first = min(active)
    if slow != first:
        spread = rate(theta[first]) - rate(theta[slow])
        if spread > 0:
            m = min(m, int(math.log(AMPLIFICATION_LIMIT) / spread))
    return int(min(max(m, lo), hi))


class SolveStats(dict):
    """Counters of one solve (iterations, total degree, ms per backend operation)."""


def cholqr(be, Z, stats):
    """Orthonormal columns spanning Z (N x p), by CholQR2: R from the Gram's Cholesky factor (after diagonal
    scaling), Z R^-1 through combine, twice.  A Gram that is not numerically positive definite gets a shifted pass
    first (shifted CholQR3: Cholesky of G + s I, s = 11 (N p + p (p + 1)) u ||G||_2), then the two plain ones."""
    p = be.width(Z)
    cur, owned, plain, shifted = Z, False, 0, 0
    while plain < 2:
        G = be.gram(cur, cur)
        G = (G + G.T) / 2
        d = np.sqrt(np.maximum(np.diag(G), np.finfo(float).tiny))
        Gs = G / d[:, None] / d[None, :]
        try:
            R = np.linalg.cholesky(Gs).T
            plain += 1
        except np.linalg.LinAlgError:
            if shifted >= 3:
                raise ValueError("the filtered block has lost rank: CholQR cannot orthonormalise it")
            s = 11 * (be.N * p + p * (p + 1)) * np.finfo(float).eps * np.linalg.norm(Gs, 2)
            R = np.linalg.cholesky(Gs + s * np.eye(p)).T
            shifted += 1
            stats["shifted_cholqr"] = stats.get("shifted_cholqr", 0) + 1
        Rinv = sla.solve_triangular(R, np.eye(p), lower=False) / d[:, None]
        nxt = be.combine(cur, Rinv)
        if owned:
            be.free(cur)
        cur, owned = nxt, True
    return cur


def rayleigh_ritz(be, Q):
    """H = Q^T (L Q), eigh on the host; X = Q W and L X = (L Q) W through combine (no second sparse product)."""
    LQ = be.lap(Q)
    H = be.gram(Q, LQ)
    theta, W = np.linalg.eigh((H + H.T) / 2)
    X, LX = be.combine(Q, W), be.combine(LQ, W)
    be.free(LQ)
    return theta, X, LX


def solve(be, k, b, *, tol=1e-10, maxiter=100, seed=0, degree=(10, 300), p=None):
    """The k smallest eigenpairs of the symmetric operator of backend `be`, whose spectrum lies in [0, b].
    Returns (e ascending (k,), X (panel N x p: the first k columns are the eigenvectors), stats).
    ValueError when maxiter iterations do not bring every residual ||L u_i - e_i u_i|| under tol * b."""
    N = be.N
    k = int(k)
    if not 1 <= k <= N:
        raise ValueError("n_eigenvectors must be in 1..{}, got {}".format(N, k))
    p = block_width(k, N) if p is None else int(p)
    if not k <= p <= min(N, MAX_BLOCK):
        raise ValueError("block width {} out of range for k = {} and N = {}".format(p, k, N))
    lo, hi = int(degree[0]), int(degree[1])
    if not 1 <= lo <= hi:
        raise ValueError("degree bounds must satisfy 1 <= low <= high, got {}".format(degree))
    b = float(b)
    tol_abs = float(tol) * b
    stats = SolveStats(iterations=0, total_degree=0, degrees=[])
    # start block: seeded, in the caller's vertex order
    X0 = be.from_host(np.random.default_rng(seed).standard_normal((N, p)))
    Q = cholqr(be, X0, stats)
    be.free(X0)
    theta, X, LX = rayleigh_ritz(be, Q)
    be.free(Q)
    resid = be.resid(X, LX, theta)
    it = 0
    while True:
        # every exit checks all k residuals: a locked column still takes part in CholQR and Rayleigh-Ritz, which can
        # mix it with nearby unconverged ones, so the lock is rebuilt from the current residuals each iteration
        conv = resid[:k] <= tol_abs
        worst = float(np.max(resid[:k]))
        if conv.all():
            break
        if it >= int(maxiter):
            be.free(X)
            be.free(LX)
            raise ValueError("The subspace iteration did not converge in {} iterations: worst residual {:.3e} "
                             "against the tolerance {:.3e} (tol * b).  Raise maxiter or the degree bounds."
                             .format(maxiter, worst, tol_abs))
        nlock = int(np.argmin(conv))  # the leading converged columns (conv is not all True here)
        it += 1
        stats["iterations"] = it
        # filter: damp [a, b], a = the largest Ritz value; scaling point = the smallest unlocked one
        a = float(theta[-1])
        a0 = float(theta[nlock])
        if not a0 < a < b:
            a = min(max(a, a0 + 1e-12 * b), b * (1 - 1e-12))
        active = [j for j in range(nlock, k) if not conv[j]]
        m = choose_degree(theta, resid, active, a, b, tol_abs, (lo, hi))
        prog = filter_program(min(a0, a - 1e-12 * b), a, b, m)
        stats["total_degree"] += m
        stats["degrees"].append(m)
        be.free(LX)
        if nlock == 0:
            Z = be.poly(prog, X)
            be.free(X)
        else:  # the locked leading columns are not filtered: the others are copied out, filtered and copied back
            T = be.copy(be.view(X, nlock, p))
            F = be.poly(prog, T)
            be.free(T)
            be.copy(F, out=be.view(X, nlock, p))
            be.free(F)
            Z = X
        Q = cholqr(be, Z, stats)
        be.free(Z)
        theta, X, LX = rayleigh_ritz(be, Q)
        be.free(Q)
        resid = be.resid(X, LX, theta)
    be.free(LX)
    stats["worst_residual"] = worst
    stats["residuals"] = np.asarray(resid[:k], dtype=np.float64)
    return np.asarray(theta[:k], dtype=np.float64), X, stats


def sign_fix(U):
    """Signs s (one per column) that make each column's largest-magnitude entry positive (the lowest index on ties)."""
    if U.shape[0] == 0:
        return np.ones(U.shape[1])
    # the largest entry against the smallest decides without an index (two contiguous reductions instead of a strided
    # argmax: 0.03 s against 0.5 s on a 4096-wide basis); only an exact tie between them needs the lowest index
    top, low = U.max(axis=0), -U.min(axis=0)
    s = np.where(top > low, 1.0, -1.0)
    for c in np.nonzero(top == low)[0]:
        s[c] = np.sign(U[np.argmax(np.abs(U[:, c])), c])
    s[s == 0] = 1.0
    return s


def finish_partial(e, U):
    """The partial-result rules of Graph.compute_fourier_basis: e ascending, e[0] within 1e-5 of zero and then
    zero (fourier.py:181-182), every column's largest-magnitude entry positive.  In place; returns the signs."""
    if not -1e-5 < e[0] < 1e-5:
        raise ValueError("The smallest eigenvalue {} is not zero (|e[0]| >= 1e-5).".format(e[0]))
    e[0] = 0
    s = sign_fix(U)
    U *= s[None, :]
    return s


# ---- the device backend -----------------------------------------------------------------------------------------
class DevicePanel:
    """N x width fp64 columns on the device, row-major with leading dimension ld (a column view shares its owner's
    buffer)."""

    def __init__(self, buf, ptr, width, ld, owner=True):
        self.buf, self.ptr, self.width, self.ld, self.owner = buf, int(ptr), int(width), int(ld), owner


class DeviceBackend:
    """The solver's backend on a float64 engine.DeviceGraph: the program path, L X and the four panel primitives.
    Milliseconds per operation (the HIP events each entry point reports) are summed in `ms`."""

    def __init__(self, dev, b):
        if dev.dtype != np.float64:
            raise TypeError("the Fourier solver runs on the float64 device graph")
        self.dev, self.ctx, self.N, self.b = dev, dev.ctx, dev.N, float(b)
        self.ms = {"poly": 0.0, "lap": 0.0, "gram": 0.0, "combine": 0.0, "resid": 0.0, "copy": 0.0}
        self.calls = {key: 0 for key in self.ms}
        self.bytes = {"gram": 0.0, "combine": 0.0, "resid": 0.0}
        self.flops = {"gram": 0.0, "combine": 0.0, "resid": 0.0}

    def width(self, X):
        return X.width

    def empty(self, w):
        buf = self.ctx.take(max(self.N * int(w) * 8, 16))
        return DevicePanel(buf, buf.ptr, w, w)

    def from_host(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        X = self.empty(arr.shape[1])
        if arr.size:
            X.buf.upload(arr)
        return X

    def to_host(self, X):
        if X.ld != X.width:
            raise ValueError("to_host needs a whole panel")
        if self.N * X.width == 0:
            return np.zeros((self.N, X.width))
        return X.buf.download((self.N, X.width), np.float64)

    def view(self, X, j0, j1):
        return DevicePanel(X.buf, X.ptr + 8 * int(j0), int(j1) - int(j0), X.ld, owner=False)

    def free(self, X):
        if X is not None and X.owner and X.buf is not None:
            buf, X.buf = X.buf, None
            self.ctx.give(buf)

    def poly(self, program, X):
        if X.ld != X.width:
            raise ValueError("the program path takes whole panels")
        Y = self.empty(X.width)
        self.ms["poly"] += self.dev.program_filter_dev(program, X.ptr, Y.ptr, X.width, self.b, old_is_x=False)
        self.calls["poly"] += 1
        return Y

    def lap(self, X):
        if X.ld != X.width:
            raise ValueError("L X takes whole panels")
        Y = self.empty(X.width)
        self.ms["lap"] += self.dev.laplacian_apply_dev(X.ptr, Y.ptr, X.width)
        self.calls["lap"] += 1
        return Y

    def gram(self, A, B):
        C, ms = panel_gram(self.ctx, self.N, A.ptr, A.ld, A.width, B.ptr, B.ld, B.width)
        self._count("gram", ms, 8.0 * self.N * (A.width + B.width), 2.0 * self.N * A.width * B.width)
        return C

    def combine(self, X, Q, out=None):
        Q = np.asarray(Q, dtype=np.float64)
        Y = self.empty(Q.shape[1]) if out is None else out
        ms = panel_combine(self.ctx, self.N, X.ptr, X.ld, X.width, Q, Y.ptr, Y.ld)
        self._count("combine", ms, 8.0 * self.N * (X.width + Q.shape[1]), 2.0 * self.N * X.width * Q.shape[1])
        return Y

    def copy(self, X, out=None):
        Y = self.empty(X.width) if out is None else out
        if Y.width != X.width:
            raise ValueError("copy between panels of different widths")
        self.ms["copy"] += panel_copy(self.ctx, self.N, X.ptr, X.ld, X.width, Y.ptr, Y.ld)
        self.calls["copy"] += 1
        return Y

    def resid(self, X, LX, theta):
        if X.ld != LX.ld:
            raise ValueError("residual norms need panels of one leading dimension")
        out, ms = panel_residual_norms(self.ctx, self.N, X.ptr, LX.ptr, X.ld, X.width, theta)
        self._count("resid", ms, 16.0 * self.N * X.width, 4.0 * self.N * X.width)
        return out

    def _count(self, key, ms, nbytes, flops):
        self.ms[key] += ms
        self.calls[key] += 1
        self.bytes[key] += nbytes
        self.flops[key] += flops


# ---- thin bindings of the three entry points ----------------------------------------------------------------------
def panel_gram(ctx, N, a_ptr, lda, na, b_ptr, ldb, nb):
    """(A^T B as a host (na, nb) array, kernel ms) for device panels A, B (gspx_panel_gram_dev)."""
    import ctypes

    from . import _capi
    C = np.zeros((int(na), int(nb)), dtype=np.float64)
    ms = ctypes.c_double(0)
    ctx.call(_capi.load().gspx_panel_gram_dev, ctx._h, int(N), ctypes.c_void_p(a_ptr), int(lda), int(na),
             ctypes.c_void_p(b_ptr), int(ldb), int(nb), _capi.ptr(C), ctypes.byref(ms))
    return C, ms.value


def panel_combine(ctx, N, x_ptr, ldx, p, Q, y_ptr, ldy):
    """Y = X Q on the device (gspx_panel_combine_dev); Q a host (p, q) array.  Returns the kernel ms."""
    import ctypes

    from . import _capi
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    if Q.ndim != 2 or Q.shape[0] != int(p):
        raise ValueError("Q must be ({}, q), got {}".format(p, Q.shape))
    ms = ctypes.c_double(0)
    ctx.call(_capi.load().gspx_panel_combine_dev, ctx._h, int(N), ctypes.c_void_p(x_ptr), int(ldx), int(p),
             _capi.ptr(Q), int(Q.shape[1]), ctypes.c_void_p(y_ptr), int(ldy), ctypes.byref(ms))
    return ms.value


def panel_gram_to(ctx, N, a_ptr, lda, na, b_ptr, ldb, nb, c_ptr, ldc, rowscale_ptr=None, alpha=1.0):
    """C = alpha A^T diag(r) B written to the device matrix at `c_ptr` (leading dimension ldc), any widths
    (gspx_panel_gram_to_dev); `rowscale_ptr`: N doubles on the device, or None.  Returns the kernel ms."""
    import ctypes

    from . import _capi
    ms = ctypes.c_double(0)
    ctx.call(_capi.load().gspx_panel_gram_to_dev, ctx._h, int(N), ctypes.c_void_p(a_ptr), int(lda), int(na),
             ctypes.c_void_p(b_ptr), int(ldb), int(nb), ctypes.c_void_p(rowscale_ptr), float(alpha),
             ctypes.c_void_p(c_ptr), int(ldc), ctypes.byref(ms))
    return ms.value


SPECTRAL_PLAIN, SPECTRAL_ANALYSIS, SPECTRAL_SYNTHESIS = 0, 1, 2


def spectral_apply(ctx, N, u_ptr, ldu, n, s_ptr, lds, w, y_ptr, ldy, mode=SPECTRAL_PLAIN, nf=1, h_ptr=None):
    """Y_g = U (diag(h_g) S) on the device (gspx_spectral_apply_dev): plain (Y = U S), analysis (nf output planes) or
    synthesis (nf coefficient planes summed into one); U, S, the nf x n multipliers and Y are device pointers.
    Returns the kernel ms."""
    import ctypes

    from . import _capi
    ms = ctypes.c_double(0)
    ctx.call(_capi.load().gspx_spectral_apply_dev, ctx._h, int(N), ctypes.c_void_p(u_ptr), int(ldu), int(n),
             ctypes.c_void_p(s_ptr), int(lds), int(w), int(mode), int(nf), ctypes.c_void_p(h_ptr),
             ctypes.c_void_p(y_ptr), int(ldy), ctypes.byref(ms))
    return ms.value


def panel_copy(ctx, N, x_ptr, ldx, w, y_ptr, ldy):
    """Y[:, :w] = X[:, :w] on the device (gspx_panel_copy_dev).  Returns the kernel ms."""
    import ctypes

    from . import _capi
    ms = ctypes.c_double(0)
    ctx.call(_capi.load().gspx_panel_copy_dev, ctx._h, int(N), ctypes.c_void_p(x_ptr), int(ldx), int(w),
             ctypes.c_void_p(y_ptr), int(ldy), ctypes.byref(ms))
    return ms.value


def panel_residual_norms(ctx, N, x_ptr, lx_ptr, ld, p, theta):
    """(||LX_i - theta_i X_i|| for i < p, kernel ms) (gspx_panel_residual_norms_dev)."""
    import ctypes

    from . import _capi
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    if theta.shape != (int(p),):
        raise ValueError("theta must have {} entries".format(p))
    out = np.zeros(int(p), dtype=np.float64)
    ms = ctypes.c_double(0)
    ctx.call(_capi.load().gspx_panel_residual_norms_dev, ctx._h, int(N), ctypes.c_void_p(x_ptr),
             ctypes.c_void_p(lx_ptr), int(ld), int(p), _capi.ptr(theta), _capi.ptr(out), ctypes.byref(ms))
    return out, ms.value


def device_partial_basis(dev, k, b, *, tol=1e-10, maxiter=100, seed=0, degree=(10, 300)):
    """The k smallest eigenpairs of a float64 DeviceGraph by ChFSI on the device.  Returns (e, U host (N, k),
    U_dev (DevicePanel N x k, contiguous), stats) with the partial-result rules applied (finish_partial)."""
    be = DeviceBackend(dev, b)
    e, X, stats = solve(be, k, b, tol=tol, maxiter=maxiter, seed=seed, degree=degree)
    try:
        U0 = be.copy(be.view(X, 0, k))
    finally:
        be.free(X)
    U = be.to_host(U0)
    stats["theta0"] = float(e[0])  # (before the partial-result rule sets it to zero)
    s = finish_partial(e, U)
    U_dev = be.combine(U0, np.diag(s))  # the same signs on the device copy (a multiplication by +-1: exact)
    be.free(U0)
    stats["ms"], stats["calls"] = dict(be.ms), dict(be.calls)
    stats["bytes"], stats["flops"] = dict(be.bytes), dict(be.flops)
    stats["p"] = block_width(k, dev.N)
    return e, U, U_dev, stats


# ---- the full basis: dense symmetric eigensolver on the device (gspx_eig.hip.h) --------------
FULL_TOL = 1e-13        # stop when off(A) <= tol ||A||_F (and no row's off-diagonal norm exceeds tol max |a_ii|)
FULL_MAX_SWEEPS = 30
FULL_SLAB = 1024        # identity columns per L X call when the dense L is formed, as filters.frame_panels
_EIG_INFO = ("sweeps", "off_rel", "pairs_rotated", "pairs_skipped", "ms_sub", "ms_cols", "ms_rows", "ms_off",
             "ms_finish", "ms_wall", "residual", "pad_mass")


def sym_eig(ctx, n, a_ptr, lda, v_ptr, ldv, tol=FULL_TOL, max_sweeps=FULL_MAX_SWEEPS):
    """Every eigenpair of the symmetric n x n fp64 device matrix at `a_ptr` (leading dimension lda, only read) by block
    Jacobi (gspx_sym_eig_dev): the eigenvectors go to the device matrix at `v_ptr` (leading dimension ldv), in columns,
    ascending.  Returns (e host (n,), stats); ValueError when max_sweeps sweeps do not converge."""
    import ctypes

    from . import _capi
    e = np.zeros(int(n), dtype=np.float64)
    info = np.zeros(len(_EIG_INFO), dtype=np.float64)
    per_sweep = np.zeros(max(int(max_sweeps), 1), dtype=np.int64)
    ctx.call(_capi.load().gspx_sym_eig_dev, ctx._h, int(n), ctypes.c_void_p(a_ptr), int(lda), ctypes.c_void_p(v_ptr),
             int(ldv), _capi.ptr(e), float(tol), int(max_sweeps), _capi.ptr(info), _capi.ptr(per_sweep))
    stats = SolveStats(zip(_EIG_INFO, (float(v) for v in info)))
    for key in ("sweeps", "pairs_rotated", "pairs_skipped"):
        stats[key] = int(stats[key])
    stats["skipped_per_sweep"] = [int(v) for v in per_sweep[:stats["sweeps"]]]
    return e, stats


def sym_eig_schedule(n_blocks):
    """The block pairs of one sweep over n_blocks blocks, as a list of rounds of (i, j) pairs, i < j
    (gspx_sym_eig_schedule_describe: host only, no device)."""
    import ctypes

    from . import _capi
    lib, rounds = _capi.load(), ctypes.c_int(0)
    _capi.check(lib.gspx_sym_eig_schedule_describe(int(n_blocks), None, ctypes.byref(rounds)))
    per_round = int(n_blocks) // 2
    pairs = np.zeros((rounds.value, per_round, 2), dtype=np.int32)
    _capi.check(lib.gspx_sym_eig_schedule_describe(int(n_blocks), _capi.ptr(pairs), ctypes.byref(rounds)))
    return [[(int(i), int(j)) for i, j in rnd] for rnd in pairs]


def panel_scale_cols(ctx, N, x_ptr, ldx, w, s):
    """X[:, c] *= s[c] on the device (gspx_panel_scale_cols_dev); s a host (w,) array."""
    import ctypes

    from . import _capi
    s = np.ascontiguousarray(s, dtype=np.float64)
    if s.shape != (int(w),):
        raise ValueError("s must have {} entries".format(w))
    ctx.call(_capi.load().gspx_panel_scale_cols_dev, ctx._h, int(N), ctypes.c_void_p(x_ptr), int(ldx), int(w),
             _capi.ptr(s))


def device_full_basis(dev, *, tol=FULL_TOL, max_sweeps=FULL_MAX_SWEEPS):
    """All N eigenpairs of a float64 DeviceGraph on the device.  The dense L is formed there in the caller's vertex
    order (identity slabs of at most FULL_SLAB columns through L X, copied into place), solved by sym_eig, and signed
    by sign_fix on the host copy and the device copy alike.  Returns (e, U host (N, N), U_dev (DevicePanel N x N,
    contiguous), stats); e[0] is set to 0 when |e[0]| < 1e-9, as the host eigh branch does."""
    be = DeviceBackend(dev, 1.0)
    ctx, N = dev.ctx, dev.N
    A, U_dev = be.empty(N), be.empty(N)
    try:
        slab = min(FULL_SLAB, max(N, 1))
        deltas, LX = ctx.take(max(N * slab * 8, 16)), ctx.take(max(N * slab * 8, 16))
        try:
            for j0 in range(0, N, slab):
                w = min(slab, N - j0)
                ctx.identity_panel(deltas, N, j0, w, np.float64)
                be.ms["lap"] += dev.laplacian_apply_dev(deltas.ptr, LX.ptr, w)
                for c0 in range(0, w, MAX_BLOCK):  # (panel_copy takes at most MAX_BLOCK columns)
                    cw = min(MAX_BLOCK, w - c0)
                    be.ms["copy"] += panel_copy(ctx, N, LX.ptr + 8 * c0, w, cw, A.ptr + 8 * (j0 + c0), N)
        finally:
            ctx.give(deltas)
            ctx.give(LX)
        e, stats = sym_eig(ctx, N, A.ptr, N, U_dev.ptr, N, tol=tol, max_sweeps=max_sweeps)
    except BaseException:
        be.free(U_dev)
        raise
    finally:
        be.free(A)
    U = be.to_host(U_dev)
    s = sign_fix(U)
    U *= s[None, :]
    panel_scale_cols(ctx, N, U_dev.ptr, N, N, s)  # (a multiplication by +-1: exact, so the two copies stay equal)
    stats["theta0"] = float(e[0]) if N else 0.0
    if N and abs(e[0]) < 1e-9:
        e[0] = 0
    stats["ms_form"] = be.ms["lap"] + be.ms["copy"]
    return e, U, U_dev, stats
