"""The batched conjugate-gradient solver of regression_tikhonov (gspx_tikhonov_cg_dev: k_cg_*, k_coldot_partial,
block_colsum, sum_parts and the host loop tikhonov_t) against the numpy restatement of tests/cg_helpers.py: iteration
counts exactly, iterates to the reference's own precision, frozen columns bit for bit.  Every rtol / atol comes from
pick_rtol: tests/test_cg_host.py checks on the CPU that no residual of any column lies within 1e-3 (relative) of it,
that the restatement agrees with scipy's cg and with itself in longdouble, and which problems float32 is asked for.
All calls go through engine.DeviceGraph.tikhonov_cg, with and without a vertex permutation.

Tolerances (cg_helpers): float64 x within 1e-9 per column of the restatement with longdouble sums (200 x what two
precisions of the reference differ by); float32 x within X32_TOL of the restatement with float32 vectors and float64
sums; the true residual ||b - A x|| in longdouble at most thr (1 + 1e-3), float64 only (in float32 the recurrence's
residual and the true one part at the rounding level of the vectors, which is not small against 1e-3 thr).
"""
import numpy as np
import pytest

import cg_helpers as cg
from pygsp_amd import engine

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
XTOL = {F64: cg.X64_TOL, F32: cg.X32_TOL}
SEEN = {}  # largest deviation of x per dtype over the file (printed by every check; profiles/tikhonov_cg.md)


@pytest.fixture(scope="module")
def devices():
    """One DeviceGraph per (graph, dtype, permuted or not), destroyed at the end of the module."""
    ctx = engine.default_context(0)
    made = {}

    def get(key, dtype, permuted):
        pb = cg.problem(*key)
        k = (key[0], pb.N, dtype, permuted)
        if k not in made:
            made[k] = engine.DeviceGraph.from_w(pb.W, dtype=dtype, perm=pb.perm if permuted else None, ctx=ctx)
        return made[k]

    yield get
    for dev in made.values():
        dev.destroy()


def check(devices, key, dtype, atol=0.0, maxiter=None, rtol=None, xtol=None, residual=True):
    """Both vertex orders of one problem against reference(): counts, x per column, zero columns, true residual.
    Returns the device's (x, iters) of the unpermuted graph."""
    pb = cg.problem(*key)
    xr, itr, _, rt = cg.reference(key, dtype, atol=atol, maxiter=maxiter, rtol=rtol)
    xtol = XTOL[dtype] if xtol is None else xtol
    for permuted in (True, False):
        x, iters, _ = devices(key, dtype, permuted).tikhonov_cg(pb.tau, pb.mask, pb.y, rtol=rt, atol=atol,
                                                                 maxiter=maxiter)
        assert x.shape == pb.y.shape and x.dtype == dtype and iters.shape == (pb.ncols,)
        err = cg.col_err(x, xr)
        SEEN[dtype] = max(SEEN.get(dtype, 0.0), float(err.max()))
        print("%s %s perm=%d: iters %d..%d, x deviation %.2e (file so far %.2e)" % (
            key, np.dtype(dtype).name, permuted, iters.min(), iters.max(), err.max(), SEEN[dtype]))
        assert np.array_equal(iters, itr), (key, permuted, np.flatnonzero(iters != itr), iters, itr)
        assert (err <= xtol).all(), (key, permuted, int(np.argmax(err)), float(err.max()))
        assert not x[:, itr == 0].any()
        if residual and dtype == F64:
            bn = np.sqrt(np.sum(pb.B.astype(np.longdouble) ** 2, axis=0)).astype(np.float64)
            thr = np.maximum(atol, rt * bn)
            res = cg.true_residual(pb.A, pb.B, x)
            done = itr < (10 * pb.N if maxiter is None else maxiter)  # (a capped column promises nothing)
            assert (res[done] <= thr[done] * (1 + cg.RES_SLACK)).all(), (key, permuted, res / np.maximum(thr, 1e-300))
    return x, iters


@pytest.mark.parametrize("key", cg.MAIN, ids=str)
def test_counts_and_iterates_fp64(devices, key):
    _, iters = check(devices, key, F64)
    assert iters[cg.ZERO_PATTERN] == 0 and len(set(iters[iters > 0])) >= 2  # the columns stop at different iterations


@pytest.mark.parametrize("key", [k for k in cg.MAIN if k in cg.FP32_PROBLEMS], ids=str)
def test_counts_and_iterates_fp32(devices, key):
    check(devices, key, F32)


@pytest.mark.parametrize("ld,dtype", [(ld, F64) for ld in cg.WIDTHS] +
                         [(k[3], F32) for k in cg.WIDE if k in cg.FP32_PROBLEMS])
def test_widths_on_the_shared_thread_map(devices, ld, dtype):
    """ldp = 1 .. 256 with rstep = 256 .. 1, then column batches of 256 + 1, 256 + 44 and 256 + 256 + 1: c0, the
    strides of y + c0 and x + c0, iters[c0 + c]."""
    check(devices, ("sensor", 300, 0.3, ld), dtype)


@pytest.mark.parametrize("key", cg.SMALL + cg.SMALL_UNMEASURED, ids=str)
def test_rows_below_and_around_one_workgroup(devices, key):
    """nred = max(1, N / 64) is 1 or 4, rstep can exceed N, the four-rows-in-flight loops run only their tails."""
    _, iters = check(devices, key, F64)
    pb = cg.problem(*key)
    if pb.N == 1:  # an isolated vertex: 1 iteration when measured, 0 when not
        assert np.array_equal(iters, np.where(pb.B[0] != 0, 1, 0)) and (pb.mask[0] or not iters.any())


def test_frozen_columns_stay_frozen_bit_for_bit(devices):
    pb = cg.problem(*cg.BASE)
    _, _, _, rtol = cg.reference(cg.BASE, F64)
    for permuted in (True, False):
        dev = devices(cg.BASE, F64, permuted)
        full, kc, _ = dev.tikhonov_cg(pb.tau, pb.mask, pb.y, rtol=rtol)
        assert np.array_equal(kc, cg.reference(cg.BASE, F64)[1])
        for k in sorted(set(int(v) for v in kc if v > 0)):
            x, iters, _ = dev.tikhonov_cg(pb.tau, pb.mask, pb.y, rtol=rtol, maxiter=k)
            assert np.array_equal(iters, np.minimum(kc, k)), (k, iters)
            done = kc <= k
            assert done.any() and np.array_equal(x[:, done], full[:, done]), (k, permuted)
            if (~done).any():  # the capped columns are still on their way
                assert (cg.col_err(x[:, ~done], full[:, ~done]) > 0).all()


def test_caps(devices):
    pb = cg.problem(*cg.BASE)
    nz = np.arange(pb.ncols) != cg.ZERO_PATTERN
    x0, it0 = check(devices, cg.BASE, F64, maxiter=0)
    assert not x0.any() and not it0.any()
    _, it3 = check(devices, cg.BASE, F64, maxiter=3, xtol=1e-12)
    assert np.array_equal(it3, np.where(nz, 3, 0))
    _, it30 = check(devices, cg.BASE, F64, rtol=0.0, maxiter=30)
    assert np.array_equal(it30, np.where(nz, 30, 0))


def test_atol_between_the_columns(devices):
    pb = cg.problem(*cg.BASE)
    atol, _ = cg.pick_atol(cg.BASE, F64)
    x, iters = check(devices, cg.BASE, F64, atol=atol)
    below = np.linalg.norm(pb.B, axis=0) < atol
    assert below.sum() > 1 and not iters[below].any() and not x[:, below].any() and (iters[~below] > 0).all()


@pytest.mark.parametrize("ld", [33, 300])
def test_two_calls_give_the_same_bytes(devices, ld):
    key = ("sensor", 300, 0.3, ld)
    pb = cg.problem(*key)
    rtol = cg.reference(key, F64)[3]
    for dtype in (F64, F32):
        dev = devices(key, dtype, True)
        a, ia, _ = dev.tikhonov_cg(pb.tau, pb.mask, pb.y, rtol=rtol)
        b, ib, _ = dev.tikhonov_cg(pb.tau, pb.mask, pb.y, rtol=rtol)
        assert a.tobytes() == b.tobytes() and np.array_equal(ia, ib)
