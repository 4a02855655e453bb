"""Lanczos filtering: ``y_i = V Uh f_i(Eh) Uh^T V^T x`` per signal column, with V the orthonormal Krylov basis of L
from x and H = V^T L V = Uh Eh Uh^T (the reference's approximations.lanczos / lanczos_op; DESIGN.md section
"Lanczos filtering").  What ``pygsp_amd.filters.lanczos_op`` runs.

The driver is host Python over a small backend; only order x Nsig arrays reach the host:

    batch_width(order)                      columns per Krylov batch (the stack must fit the workspace budget)
    krylov(X, c0, c1, order, breakdown)     the stack of columns c0:c1 -> (V, alpha, beta, proj, steps)
    combine(V, weights, Y, c0, c1)          Y[f N + n, c0:c1] = sum_j weights[f, j] V_j[n]
    free(V)

``DeviceBackend`` is the product's (gspx_lanczos_krylov_dev / gspx_lanczos_combine_dev).  There is no host backend
here: the tests carry a numpy one, so the driver is testable without a GPU and the product keeps no CPU fallback.
"""
import ctypes

import numpy as np

BREAKDOWN_FACTOR = 64  # a column stops at step k when beta_k <= 64 eps b (b: the upper bound of lambda_max)
MAX_WIDTH = 256         # widest column batch of the device entry points


def breakdown_threshold(bound):
    return BREAKDOWN_FACTOR * np.finfo(np.float64).eps * float(bound)


def max_batch_width(N, order, ws_limit_mb, max_batch=0):
    """Columns per batch: the `order` stack panels and three work panels of N x width fp64 within ws_limit_mb, one
    panel below 2 GiB, at most MAX_WIDTH (the bound gspx_lanczos_krylov_dev checks, computed the same way)."""
    rowb = max(int(N) * 8, 1)
    width = ((1 << 31) - 65536) // rowb
    budget = max(int(ws_limit_mb), 1) << 20
    width = min(width, max(1, budget // (rowb * (int(order) + 3))))
    if max_batch > 0:
        width = min(width, int(max_batch))
    if width >= 4:
        width &= ~3
    return max(1, min(width, MAX_WIDTH))


def tridiagonal(alpha, beta, m):
    """The m x m symmetric tridiagonal H of one column: alpha[:m] on the diagonal, beta[1:m] beside it."""
    H = np.diag(np.asarray(alpha[:m], dtype=np.float64))
    if m > 1:
        off = np.asarray(beta[1:m], dtype=np.float64)
        H += np.diag(off, 1) + np.diag(off, -1)
    return H


def evaluate(f, x):
    """f.evaluate at the points x as an (Nf, len(x)) array (a single-filter pygsp Filter may return (len(x),))."""
    Nf = int(f.Nf)
    return np.asarray(f.evaluate(np.asarray(x, dtype=np.float64)), dtype=np.float64).reshape(Nf, -1)


def ritz_weights(f, alpha, beta, proj, steps):
    """Per column c with Krylov dimension m = steps[c]: eigh(H) = (Eh, Uh), Eh[Eh < 0] = 0, and the coefficients
    w_i = Uh (f_i(Eh) * Uh^T proj[:m, c]) of the stack, so that y_i = sum_j w_i[j] q_j.  Columns of one m share
    one batched eigh; f.evaluate is called once, on the Ritz values of all columns.
    Returns weights (Nf, order, n) (zero beyond m; all zero for m = 0) and the Ritz values per column."""
    order, n = alpha.shape
    Nf = int(f.Nf)
    weights = np.zeros((Nf, order, n))
    steps = np.asarray(steps, dtype=np.int64)
    groups = {}
    for c in range(n):
        if steps[c] > 0:
            groups.setdefault(int(steps[c]), []).append(c)
    if not groups:
        return weights, [np.zeros(0) for _ in range(n)]
    eig = {}
    flat = []
    for m, cols in groups.items():
        H = np.stack([tridiagonal(alpha[:, c], beta[:, c], m) for c in cols])
        Eh, Uh = np.linalg.eigh(H)
        Eh[Eh < 0] = 0
        eig[m] = (Eh, Uh)
        flat.append(Eh.ravel())
    fe_all = evaluate(f, np.concatenate(flat))
    ritz = [np.zeros(0) for _ in range(n)]
    at = 0
    for m, cols in groups.items():
        Eh, Uh = eig[m]
        fe = fe_all[:, at:at + Eh.size].reshape(Nf, len(cols), m)
        at += Eh.size
        for t, c in enumerate(cols):
            u = Uh[t]
            coef = u.T @ proj[:m, c]
            weights[:, :m, c] = (fe[:, t, :] * coef[None, :]) @ u.T
            ritz[c] = Eh[t]
    return weights, ritz


def filter_columns(be, f, X, n, order, bound, Y):
    """The driver: columns of X in batches of be.batch_width(order); Y receives the Nf N x n result."""
    order = int(order)
    if order < 1:
        raise ValueError("order must be >= 1, got {}".format(order))
    thr = breakdown_threshold(bound)
    width = be.batch_width(order)
    stats = {"batches": 0, "steps": np.zeros(n, dtype=np.int64)}
    for c0 in range(0, n, width):
        c1 = min(n, c0 + width)
        V, alpha, beta, proj, steps = be.krylov(X, c0, c1, order, thr)
        try:
            weights, _ = ritz_weights(f, alpha, beta, proj, steps)
            be.combine(V, weights, Y, c0, c1)
        finally:
            be.free(V)
        stats["batches"] += 1
        stats["steps"][c0:c1] = steps
    return stats


# ---- the device backend -----------------------------------------------------------------------------------------
class DeviceBackend:
    """The driver's backend on a float64 engine.DeviceGraph.  X and Y are (device pointer, leading dimension)
    pairs of N x n (X) and Nf N x n (Y) fp64 arrays in the caller's vertex order; the stacks come from the context's
    pool.  Milliseconds of the two entry points (HIP events) are summed in `ms`; with phases=True the Krylov call
    also times every launch (`phase_ms`)."""

    PHASES = ("permute", "product", "three_term", "dots", "update", "projection")

    def __init__(self, dev, phases=False):
        if dev.dtype != np.float64:
            raise TypeError("Lanczos filtering runs on the float64 device graph")
        self.dev, self.ctx, self.N = dev, dev.ctx, dev.N
        self.ms = {"krylov": 0.0, "combine": 0.0}
        self.phases = phases
        self.phase_ms = dict.fromkeys(self.PHASES, 0.0)

    def batch_width(self, order):
        return max_batch_width(self.N, order, self.ctx.get_option("ws_limit_mb"), self.ctx.get_option("max_batch"))

    def krylov(self, X, c0, c1, order, breakdown):
        from . import _capi
        x_ptr, ldx = X
        n = c1 - c0
        V = self.ctx.take(max(order * self.N * n * 8, 16))
        alpha, beta, proj = (np.zeros((order, n)) for _ in range(3))
        steps = np.zeros(n, dtype=np.int32)
        ph = np.zeros(len(self.PHASES)) if self.phases else None
        ms = ctypes.c_double(0)
        try:
            self.ctx.call(_capi.load().gspx_lanczos_krylov_dev, self.dev._h, int(order), int(n),
                          ctypes.c_void_p(x_ptr + 8 * c0), int(ldx), float(breakdown), ctypes.c_void_p(V.ptr),
                          _capi.ptr(alpha), _capi.ptr(beta), _capi.ptr(proj), _capi.ptr(steps), _capi.ptr(ph),
                          ctypes.byref(ms))
        except BaseException:
            self.ctx.give(V)
            raise
        self.ms["krylov"] += ms.value
        if ph is not None:
            for k, v in zip(self.PHASES, ph):
                self.phase_ms[k] += float(v)
        return (V, order, n), alpha, beta, proj, steps

    def combine(self, V, weights, Y, c0, c1):
        from . import _capi
        buf, order, n = V
        y_ptr, ldy = Y
        w = np.ascontiguousarray(weights, dtype=np.float64)
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_lanczos_combine_dev, self.dev._h, int(order), int(n), ctypes.c_void_p(buf.ptr),
                      int(w.shape[0]), _capi.ptr(w), ctypes.c_void_p(y_ptr + 8 * c0), int(ldy), ctypes.byref(ms))
        self.ms["combine"] += ms.value

    def free(self, V):
        self.ctx.give(V[0])


def device_basis(dev, x, order, breakdown=0.0):
    """(V (N, order, n) in the caller's vertex order, alpha (order, n), beta (order, n), steps (n,)) of the host
    panel x (N, n), n <= 256, on a float64 DeviceGraph: the Krylov stacks to the host, for tests at small N."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    N, n = x.shape
    be = DeviceBackend(dev)
    bx = dev.ctx.upload(x) if x.size else None
    try:
        V, alpha, beta, _, steps = be.krylov((bx.ptr if bx else 0, n), 0, n, int(order), breakdown)
        try:
            stack = V[0].download((int(order), N, n), np.float64) if N * n else np.zeros((int(order), N, n))
        finally:
            be.free(V)
    finally:
        if bx is not None:
            bx.free()
    perm = dev.download_perm()
    out = np.empty_like(stack)
    if perm is None:
        out[:] = stack
    else:
        out[:, perm, :] = stack  # (internal row i is the caller's row perm[i])
    return np.moveaxis(out, 0, 1), alpha, beta, steps.astype(np.int64)
