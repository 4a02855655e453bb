"""The harmonic-extension solver (gspx_dirichlet_cg_dev: k_dirichlet_values / _select / _rhs / _merge around the
conjugate-gradient loop it shares with gspx_tikhonov_cg_dev) against the numpy restatement of
tests/dirichlet_helpers.py: iteration counts exactly, x to the reference's own precision, measured rows bit-equal to y,
zero columns untouched.  Every rtol / atol comes from cg.pick_rtol; tests/test_dirichlet_host.py checks on the CPU that
no residual of any column lies within 1e-3 (relative) of it and that two precisions of the restatement agree on every
count.  All calls go through engine.DeviceGraph.dirichlet_cg, with and without a vertex permutation.

Tolerances (dirichlet_helpers): float64 x within 1e-9 per column of the restatement with longdouble sums (its two
precisions differ by 7e-16); float32 x within X32_TOL of the restatement with float32 vectors and float64 sums.
"""
import numpy as np
import pytest

import cg_helpers as cg
import dirichlet_helpers as dh
from conftest import load_golden
from pygsp_amd import engine, graphs, learning

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
XTOL = {F64: dh.X64_TOL, F32: dh.X32_TOL}
SEEN = {}  # largest deviation of x per dtype over the file (printed by every check; profiles/dirichlet_cg.md)


@pytest.fixture(scope="module")
def devices():
    """One DeviceGraph per (graph, dtype, permuted or not), destroyed at the end of the module."""
    ctx = engine.default_context(0)
    made = {}

    def get(key, dtype, permuted):
        pb = dh.problem(*key)
        k = (key[0], pb.N, dtype, permuted)
        if k not in made:
            made[k] = engine.DeviceGraph.from_w(pb.W, dtype=dtype, perm=pb.perm if permuted else None, ctx=ctx)
        return made[k]

    yield get
    for dev in made.values():
        dev.destroy()


def check(devices, key, dtype, atol=0.0, maxiter=None, rtol=None, xtol=None):
    """Both vertex orders of one problem against reference(): counts, x per column, measured rows, zero columns.
    Returns the device's (x, iters) of the unpermuted graph."""
    pb = dh.problem(*key)
    xr, itr, _, rt = dh.reference(key, dtype, atol=atol, maxiter=maxiter, rtol=rtol)
    xtol = XTOL[dtype] if xtol is None else xtol
    for permuted in (True, False):
        x, iters, _ = devices(key, dtype, permuted).dirichlet_cg(pb.mask, pb.y, rtol=rt, atol=atol, maxiter=maxiter)
        assert x.shape == pb.y.shape and x.dtype == dtype and iters.shape == (pb.ncols,)
        err = cg.col_err(x, xr)
        SEEN[dtype] = max(SEEN.get(dtype, 0.0), float(err.max(initial=0.0)))
        print("%s %s perm=%d: iters %d..%d, x deviation %.2e (file so far %.2e)" % (
            key, np.dtype(dtype).name, permuted, iters.min(), iters.max(), err.max(initial=0.0), SEEN[dtype]))
        assert np.array_equal(iters, itr), (key, permuted, np.flatnonzero(iters != itr), iters, itr)
        assert (err <= xtol).all(), (key, permuted, int(np.argmax(err)), float(err.max()))
        assert x[pb.mask].tobytes() == pb.y[pb.mask].astype(dtype).tobytes()
        assert not x[:, ~pb.y[pb.mask].any(axis=0)].any()
    return x, iters


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("key", dh.MAIN, ids=str)
def test_counts_and_iterates(devices, key, dtype):
    _, iters = check(devices, key, dtype)
    assert iters[cg.ZERO_PATTERN] == 0 and (np.delete(iters, cg.ZERO_PATTERN) > 0).all()
    if key == dh.MAIN[1] and dtype == F64:  # the columns stop at different iterations
        assert len(set(iters[iters > 0])) >= 2


@pytest.mark.parametrize("ld,dtype", [(ld, dt) for dt in (F64, F32) for ld in dh.WIDTHS])
def test_widths_on_the_shared_thread_map(devices, ld, dtype):
    """ldp = 1 .. 256, then column batches of 256 + 1 and 256 + 44: c0 > 0, the strides of y + c0 and x + c0,
    iters[c0 + c], the merge before the padded output path."""
    check(devices, ("sensor", 300, ld), dtype)


@pytest.mark.parametrize("key", dh.SMALL, ids=str)
def test_rows_below_and_around_one_workgroup(devices, key):
    _, iters = check(devices, key, F64)
    if dh.problem(*key).N == 1:  # nothing to solve either way: x = y when measured, 0 when not
        assert not iters.any()


@pytest.mark.parametrize("key", [dh.ALL_MEASURED, dh.NONE_MEASURED], ids=str)
def test_all_and_none_measured(devices, key):
    pb = dh.problem(*key)
    for dtype in (F64, F32):
        x, iters = check(devices, key, dtype)
        assert not iters.any() and np.array_equal(x, pb.y.astype(dtype) if pb.mask.all() else np.zeros_like(x))


def test_a_component_without_a_measured_vertex_stays_zero(devices):
    pb = dh.problem(*dh.SPLIT)
    x, iters = check(devices, dh.SPLIT, F64)
    assert not x[64:].any() and iters.max() > 0 and x[:64][~pb.mask[:64]].any()


def test_nan_at_unmeasured_rows_is_never_read(devices):
    pb = dh.problem(*dh.BASE)
    assert np.isnan(pb.nan_y[~pb.mask]).all()
    for dtype in (F64, F32):
        rtol = dh.reference(dh.BASE, dtype)[3]
        for permuted in (True, False):
            dev = devices(dh.BASE, dtype, permuted)
            a, ia, _ = dev.dirichlet_cg(pb.mask, pb.nan_y, rtol=rtol)
            b, ib, _ = dev.dirichlet_cg(pb.mask, pb.y, rtol=rtol)
            assert np.isfinite(a).all() and a.tobytes() == b.tobytes() and np.array_equal(ia, ib)


def test_caps(devices):
    pb = dh.problem(*dh.BASE)
    nz = np.arange(pb.ncols) != cg.ZERO_PATTERN
    x0, it0 = check(devices, dh.BASE, F64, maxiter=0)
    assert np.array_equal(x0, np.where(pb.mask[:, None], pb.y, 0.0)) and not it0.any()
    _, it3 = check(devices, dh.BASE, F64, maxiter=3)
    assert np.array_equal(it3, np.where(nz, 3, 0))


def test_frozen_columns_stay_frozen_bit_for_bit(devices):
    """Under the atol of dh.pick_atol the columns of BASE stop after 0 to 22 iterations (on their own they all take
    33): a smaller maxiter leaves every column that was done by then exactly as the full run leaves it."""
    pb = dh.problem(*dh.BASE)
    rtol = dh.reference(dh.BASE, F64)[3]
    atol, _ = dh.pick_atol(dh.BASE, F64)
    _, kc = check(devices, dh.BASE, F64, atol=atol)
    assert len(set(kc)) >= 5
    for permuted in (True, False):
        dev = devices(dh.BASE, F64, permuted)
        full, kf, _ = dev.dirichlet_cg(pb.mask, pb.y, rtol=rtol, atol=atol)
        assert np.array_equal(kf, kc)
        for k in sorted(set(int(v) for v in kc if v > 0)):
            x, iters, _ = dev.dirichlet_cg(pb.mask, pb.y, rtol=rtol, atol=atol, maxiter=k)
            assert np.array_equal(iters, np.minimum(kc, k)), (k, iters)
            done = kc <= k
            assert done.any() and np.array_equal(x[:, done], full[:, done]), (k, permuted)
            if (~done).any():  # the capped columns are still on their way
                assert (cg.col_err(x[:, ~done], full[:, ~done]) > 0).all()


@pytest.mark.parametrize("ld", [12, 300])
def test_two_calls_give_the_same_bytes(devices, ld):
    key = ("sensor", 300, ld)
    pb = dh.problem(*key)
    for dtype in (F64, F32):
        rtol = dh.reference(key, dtype)[3]
        dev = devices(key, dtype, True)
        a, ia, _ = dev.dirichlet_cg(pb.mask, pb.y, rtol=rtol)
        b, ib, _ = dev.dirichlet_cg(pb.mask, pb.y, rtol=rtol)
        assert a.tobytes() == b.tobytes() and np.array_equal(ia, ib)


def test_the_references_goldens_through_the_learners():
    """reg_tau0 and class_tau0 of ops_sensor123.npz (the reference's spsolve) through the public functions on a
    float64 graphs.Graph at the default rtol 1e-10, within ||x - x*|| <= rtol ||b|| / lambda_min(L_uu)."""
    (_, W, mask, y, ref), (_, _, _, lab, cref) = dh.golden_cases(load_golden("ops_sensor123.npz"))
    G = graphs.Graph(W, compute_dtype=F64)
    x = learning.regression_tikhonov(G, y, mask, tau=0, solver="cg")
    err, bound = np.linalg.norm(x - ref), dh.error_bound(W, mask, np.nan_to_num(y)[:, None], 1e-10)[0]
    print("reg_tau0: error / bound %.3f" % (err / bound))
    assert x.shape == ref.shape and err <= bound and x[mask].tobytes() == y[mask].tobytes()
    X = learning.classification_tikhonov(G, lab, mask, tau=0, solver="cg")
    err, bound = np.linalg.norm(X - cref, axis=0), dh.error_bound(W, mask, dh.one_hot_measured(lab, mask), 1e-10)
    print("class_tau0: error / bound %s" % (err / bound))
    assert X.shape == cref.shape and (err <= bound).all()
    assert np.array_equal(np.argmax(X, axis=1), np.argmax(cref, axis=1))
    with pytest.raises(NotImplementedError):  # without the keyword tau = 0 is refused as before
        learning.regression_tikhonov(G, y, mask, tau=0)
