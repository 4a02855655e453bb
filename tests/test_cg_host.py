"""The numpy restatement of the batched Tikhonov CG solver (tests/cg_helpers.py) and the inputs of
tests/test_gpu_h_tikhonov_cg.py, checked without a device: the reference has to be right before it judges the kernels.
Against scipy's own cg, against itself with longdouble sums, the decidability of every stopping test the GPU file
relies on, and which problems float32 may be asked to reproduce count for count."""
import numpy as np
import pytest
from scipy.sparse.linalg import cg as scipy_cg

import cg_helpers as cg


def _seq_dev(sa, sb, t):
    """Largest deviation between two families of residual sequences over their common indices, relative to the value
    or to the threshold t they are compared with, whichever is larger (a residual at rounding level, far below t,
    decides nothing)."""
    dev = 0.0
    for a, b in zip(sa, sb):
        m = min(len(a), len(b))
        if m:
            dev = max(dev, float(np.max(np.abs(a[:m] - b[:m]) / np.maximum(a[:m], t))))
    return dev


@pytest.fixture(scope="module")
def fp32_pairs():
    """Per float32 candidate: the restatement with float64 sums and with float32 sums, at the candidate's rtol."""
    out = {}
    for key in cg.FP32_CANDIDATES:
        pb = cg.problem(*key)
        _, rtol, gap = cg.probe(key, np.float32)
        out[key] = (gap, rtol, cg.solve(pb.A, pb.B, rtol=rtol, dt=np.float32, acc=np.float64),
                    cg.solve(pb.A, pb.B, rtol=rtol, dt=np.float32, acc=np.float32))
    return out


def test_pick_rtol():
    t, gap = cg.pick_rtol([np.array([1.0, 1e-2, 3e-5, 1e-5, 1e-7]), np.array([]), np.array([1.0, 2e-5])], 1e-6, 1e-4)
    assert t == pytest.approx(0.5 * (1e-7 + 1e-5)) and gap == pytest.approx((1e-5 - 1e-7) / (1e-5 + 1e-7))
    t, gap = cg.pick_rtol([np.array([1.0, 3e-5, 2e-5, 4e-6]), np.array([1.0, 6e-5])], 1e-5, 1e-4)
    assert t == pytest.approx(1.2e-5) and gap == pytest.approx(2 / 3)  # (the midpoint of 4e-6 and 2e-5)
    t, gap = cg.pick_rtol([np.array([1.0, 5e-7])], 1e-6, 1e-4)  # nothing inside: the far end from 5e-7
    assert t == 1e-4 and gap == pytest.approx(1 - 5e-3)
    assert cg.pick_rtol([np.array([])], 1e-6, 1e-4)[1] == np.inf


def test_restatement_edges():
    pb = cg.problem(*cg.BASE)
    x, iters, seq = cg.solve(pb.A, pb.B, rtol=1e-5)
    z = cg.ZERO_PATTERN
    assert iters[z] == 0 and not x[:, z].any() and len(seq[z]) == 0
    assert all(len(s) == k + 1 for c, (s, k) in enumerate(zip(seq, iters)) if c != z)
    assert all(s[-1] < 1e-5 <= s[:-1].min() for c, s in enumerate(seq) if c != z)
    assert (cg.true_residual(pb.A, pb.B, x) <= 1e-5 * (1 + cg.RES_SLACK) * np.linalg.norm(pb.B, axis=0)).all()
    x0, it0, _ = cg.solve(pb.A, pb.B, maxiter=0)
    assert not x0.any() and not it0.any()
    x3, it3, _ = cg.solve(pb.A, pb.B, maxiter=3)
    assert np.array_equal(it3, np.where(np.arange(12) == z, 0, 3))
    x1, it1, _ = cg.solve(pb.A, pb.B[:, 2], rtol=1e-5)  # a 1-D right-hand side, and the columns are independent
    assert it1.shape == (1,) and it1[0] == iters[2] and cg.col_err(x1, x[:, [2]])[0] <= 1e-12


@pytest.mark.parametrize("key", cg.MAIN + cg.SMALL[8::4], ids=str)
def test_against_scipy(key):
    """float64 vectors and sums: scipy's iteration count (by its callback) and its x, single columns."""
    pb = cg.problem(*key)
    rtol = cg.probe(key, np.float64)[1]
    x, iters, _ = cg.solve(pb.A, pb.B, rtol=rtol)
    for c in sorted({0, pb.ncols // 2, cg.ZERO_PATTERN, cg.CONST_PATTERN, 11} & set(range(pb.ncols))):
        calls = []
        xs, info = scipy_cg(pb.A, pb.B[:, c], rtol=rtol, atol=0.0, maxiter=10 * pb.N, callback=lambda xk: calls.append(1))
        assert info == 0 and len(calls) == iters[c], (key, c)
        assert cg.col_err(xs[:, None], x[:, [c]])[0] <= 1e-12, (key, c)


@pytest.mark.parametrize("key", cg.FP64_PROBLEMS, ids=str)
def test_longdouble_sums_and_decidability(key):
    """Sums in float64 and in longdouble: identical counts, x to 1e-10; and the rtol the GPU tests use lies at least
    MIN_GAP (relative) from every residual of every non-zero column."""
    pb = cg.problem(*key)
    seq, rtol, gap = cg.probe(key, np.float64)
    assert cg.RTOL_RANGE[0] <= rtol <= cg.RTOL_RANGE[1] and gap >= cg.MIN_GAP, (key, rtol, gap)
    xl, itl, sl, _ = cg.reference(key, np.float64)
    x, it, s = cg.solve(pb.A, pb.B, rtol=rtol)
    assert np.array_equal(it, itl), key
    assert cg.col_err(x, xl).max() <= 1e-10, key
    assert _seq_dev(s, sl, rtol) <= 1e-2 * gap, key
    zero = ~pb.B.any(axis=0)
    assert not itl[zero].any() and (itl[~zero] >= 1).all() and not xl[:, zero].any()
    if pb.N == 1:  # an isolated vertex: one iteration when it is measured, none when it is not
        assert np.array_equal(itl, np.where(zero, 0, 1)) and zero.all() == (not pb.mask[0])


def test_base_thresholds_are_decidable():
    """The atol of the threshold test: between the norms of the 1e-2 and the 1e0 column, MIN_GAP from every ||r_k||."""
    pb = cg.problem(*cg.BASE)
    atol, gap = cg.pick_atol(cg.BASE, np.float64)
    bn = np.linalg.norm(pb.B, axis=0)
    assert gap >= cg.MIN_GAP and 0 < (bn < atol).sum() - 1 < 11 and (bn > atol).sum() >= 5  # (-1: the zero column)
    _, iters, _, _ = cg.reference(cg.BASE, np.float64, atol=atol)
    assert not iters[bn < atol].any() and (iters[bn > atol] > 0).all()
    assert len(set(cg.reference(cg.BASE, np.float64)[1])) >= 5  # the frozen-column test has counts to tell apart


def test_fp32_admission(fp32_pairs):
    """A problem is used in float32 only if float32 vectors with float64 sums and with float32 sums give identical
    counts and residual sequences within 1 % of the gap of its rtol, and that gap is at least MIN_GAP."""
    refused = []
    for key, (gap, rtol, (xa, ia, sa), (xb, ib, sb)) in fp32_pairs.items():
        if not (gap >= cg.MIN_GAP and np.array_equal(ia, ib) and _seq_dev(sa, sb, rtol) < 1e-2 * gap):
            refused.append(key)
    assert tuple(refused) == cg.FP32_EXCLUDED
    assert set(cg.FP32_PROBLEMS) == set(cg.FP32_CANDIDATES) - set(refused)


def test_fp32_tolerance(fp32_pairs):
    """X32_TOL is 10 x the largest deviation of x between the two float32 restatements on the admitted problems."""
    worst = max(cg.col_err(fp32_pairs[key][3][0], fp32_pairs[key][2][0]).max() for key in cg.FP32_PROBLEMS)
    print("largest float32 x deviation between the restatements: %.3e" % worst)
    assert 10 * worst <= cg.X32_TOL < 11 * worst
    # what the GPU file compares with is the float64-sum one, at the same rtol
    for key in cg.FP32_PROBLEMS:
        assert np.array_equal(cg.reference(key, np.float32)[1], fp32_pairs[key][2][1])
