"""A numpy restatement of the harmonic-extension solver (gspx_dirichlet_cg_dev, csrc/gspx_ops.hip.h: dirichlet_cg_t)
on top of the conjugate-gradient restatement of tests/cg_helpers.py, and the problems the CPU and GPU tests share.

    x = y on the measured vertices;  L_uu x_u = -L_ul y_l on the others, solved EMBEDDED in N rows:
    A = P_u L P_u,  P_u = diag(~mask),   b = -(L (mask * y)) * ~mask,   x = cg.solve(A, b) + mask * y

b and every iterate are zero on the measured rows, so cg.solve on A is CG on the block L_uu.  b is formed in the
vectors' dtype, as the device forms it.
"""
import functools

import numpy as np
from scipy import sparse
from scipy.sparse import csgraph
from scipy.sparse.linalg import spsolve

import cg_helpers as cg
from learning_helpers import laplacian

# 10 x the largest deviation of x between the two float32 restatements (float32 vectors with float64 sums and with
# float32 sums) over FP32_PROBLEMS: tests/test_dirichlet_host.py measures it (test_fp32_tolerance: 3.81e-7) and
# profiles/dirichlet_cg.md records it.  The factor 10, as for cg.X32_TOL: the device's product adds in a third order.
X32_TOL = 3.9e-6
X64_TOL = cg.X64_TOL  # the two float64 restatements differ by 7e-16 on these inputs
RTOL_RANGE = {np.dtype(np.float64): (1e-11, 1e-9), np.dtype(np.float32): (1e-5, 1e-3)}


def embedded(W, mask, y, dt=np.float64):
    """(A, b, y_l): A = P_u L P_u in float64 CSR, b = -(L y_l) on the unmeasured rows and y_l = mask * y, both N x n
    in `dt`.  y is selected, not multiplied: NaN at an unmeasured row does not get through."""
    keep = np.asarray(mask).reshape(-1) != 0
    y = np.asarray(y)
    y2 = y[:, None] if y.ndim == 1 else y
    L = laplacian(W)
    Pu = sparse.diags((~keep).astype(np.float64))
    yl = np.where(keep[:, None], y2, 0.0).astype(dt)
    b = np.where(keep[:, None], 0.0, -np.asarray(L.astype(dt) @ yl)).astype(dt)
    return sparse.csr_matrix(Pu @ L @ Pu), b, yl


def harmonic(W, mask, y, rtol, atol=0.0, maxiter=None, dt=np.float64, acc=np.float64):
    """The restatement: (x (N, n) in dt, iterations per column, seq) with seq as cg.solve returns it."""
    A, b, yl = embedded(W, mask, y, dt)
    x, iters, seq = cg.solve(A, b, rtol=rtol, atol=atol, maxiter=maxiter, dt=dt, acc=acc)
    keep = np.asarray(mask).reshape(-1) != 0
    return np.where(keep[:, None], yl, x), iters, seq


def blocks(W, mask, y):
    """(L_uu, -L_ul y_l, lambda_min(L_uu)) in float64; y (N, n)."""
    keep = np.asarray(mask).reshape(-1) != 0
    L = laplacian(W)
    Luu = L[~keep][:, ~keep].tocsc()
    rhs = -np.asarray(L[~keep][:, keep] @ np.asarray(y, dtype=np.float64)[keep])
    return Luu, rhs, float(np.linalg.eigvalsh(Luu.toarray()).min())


def direct(W, mask, y):
    """spsolve(L_uu, -L_ul y_l) put back among the measured values: what the reference computes (learning.py:349-367)."""
    keep = np.asarray(mask).reshape(-1) != 0
    Luu, rhs, _ = blocks(W, mask, y)
    x = np.where(keep[:, None], y, 0.0).astype(np.float64)
    x[~keep] = spsolve(Luu, rhs).reshape(rhs.shape)
    return x


def error_bound(W, mask, y, rtol):
    """||x - x*||_2 <= ||r||_2 / lambda_min(L_uu) with ||r||_2 < rtol ||b||_2, per column."""
    _, rhs, lmin = blocks(W, mask, y)
    return rtol * np.linalg.norm(rhs, axis=0) / lmin


# ---- the problems ---------------------------------------------------------------------------------------------------
class Problem:
    """W and y of a cg.problem with a mask of its own (about 40 % measured unless `measured` says all or none).
    kind 'split': a 64- and a 65-vertex sensor graph side by side, no vertex of the second one measured."""

    def __init__(self, kind, N, ncols, measured=None):
        self.key = (kind, N, ncols, measured)
        if kind == "split":
            a, b = cg.problem("sensor", 64, 0.3, ncols), cg.problem("sensor", 65, 0.3, ncols)
            assert N == a.N + b.N
            self.W = sparse.block_diag([a.W, b.W], format="csr")
            self.y = np.vstack([a.y, b.y])
        else:
            src = cg.problem(kind, N, 0.3, ncols)
            self.W, self.y = src.W, src.y
        self.N, self.ncols = N, ncols
        self.mask = np.random.default_rng(7 * N + 1).uniform(size=N) > 0.6
        if measured is not None:
            self.mask[:] = measured
        elif kind == "split":
            self.mask[64:] = False
        else:  # (a component without a measured vertex keeps x = 0: fine for CG, singular for the direct solve)
            _, comp = csgraph.connected_components(self.W, directed=False)
            first = np.unique(comp, return_index=True)[1]
            self.mask[first[np.bincount(comp, weights=self.mask) == 0]] = True
        self.perm = np.random.default_rng(N).permutation(N).astype(np.int32)
        self.nan_y = np.where(self.mask[:, None], self.y, np.nan)


@functools.lru_cache(maxsize=None)
def problem(kind, N, ncols, measured=None):
    return Problem(kind, N, ncols, measured)


MAIN = tuple(("sensor", N, 12) for N in (300, 3000))
WIDTHS = (1, 5, 64, 256, 257, 300)
WIDE = tuple(("sensor", 300, ld) for ld in WIDTHS)
SMALL = tuple(("random" if N < 7 else "sensor", N, ld) for N in (1, 2, 5, 63, 64, 65, 257) for ld in (1, 5, 64))
SMALL += (("random", 1, 5, True), ("random", 1, 5, False))  # N = 1, measured and not
ALL_MEASURED, NONE_MEASURED, SPLIT = ("sensor", 300, 12, True), ("sensor", 300, 12, False), ("split", 129, 12)
BASE = MAIN[0]  # the batch of the NaN, cap, frozen-column and determinism tests
FP64_PROBLEMS = MAIN + WIDE + SMALL + (ALL_MEASURED, NONE_MEASURED, SPLIT)
FP32_PROBLEMS = MAIN + WIDE


def _acc(dtype):
    return np.longdouble if np.dtype(dtype) == np.float64 else np.float64


@functools.lru_cache(maxsize=None)
def probe(key, dtype):
    """The residual sequences of the reference (vectors in dtype; sums in longdouble for float64, in float64 for
    float32) run down to the low end of the dtype's RTOL_RANGE, the rtol cg.pick_rtol chooses from them, its gap."""
    pb = problem(*key)
    lo, hi = RTOL_RANGE[np.dtype(dtype)]
    _, _, seq = harmonic(pb.W, pb.mask, pb.y, rtol=lo, dt=dtype, acc=_acc(dtype))
    rtol, gap = cg.pick_rtol(seq, lo, hi)
    return seq, rtol, gap


@functools.lru_cache(maxsize=None)
def reference(key, dtype, atol=0.0, maxiter=None, rtol=None):
    """(x, iterations, seq, rtol) of the reference for a problem at the rtol of probe() (or the one given)."""
    pb = problem(*key)
    if rtol is None:
        rtol = probe(key, dtype)[1]
    x, iters, seq = harmonic(pb.W, pb.mask, pb.y, rtol=rtol, atol=atol, maxiter=maxiter, dt=dtype, acc=_acc(dtype))
    return x, iters, seq, rtol


def pick_atol(key, dtype):
    """An atol among the norms of the scaled right-hand sides, as far as possible (relative) from every ||r_k|| of
    every column, and that distance.  The columns' own counts differ little (one matrix, relative thresholds); under
    this atol the small columns stop at once and the others after a number of iterations that grows with their scale."""
    pb = problem(*key)
    seq = probe(key, dtype)[0]
    b = embedded(pb.W, pb.mask, pb.y, dtype)[1]
    bn = np.sqrt(np.sum(b.astype(np.longdouble) ** 2, axis=0)).astype(np.float64)
    return cg.pick_rtol([s * n for s, n in zip(seq, bn)], 2e-1, 2e0)


def golden_cases(g):
    """(name, W, mask, y with NaN where unmeasured, the reference's answer) for reg_tau0 and class_tau0 of the
    ops_sensor123 fixture."""
    from conftest import csr_from
    W, mask = csr_from(g, "W"), g["mask"].astype(bool)
    lab = g["labels"].astype(float)
    lab[~mask] = np.nan
    return (("reg_tau0", W, mask, g["measures"], g["reg_tau0"]), ("class_tau0", W, mask, lab, g["class_tau0"]))


def one_hot_measured(labels, mask):
    """The right-hand side classification_tikhonov builds: one-hot rows of the measured labels (unmeasured: class 0,
    as learning.py:246-247 leaves them; they are never read)."""
    lab = np.where(mask, np.nan_to_num(labels), 0).astype(int)
    return (lab[:, None] == np.arange(lab.max() + 1)[None, :]).astype(np.float64)
