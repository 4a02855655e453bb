"""The numpy restatement of the harmonic-extension solver (tests/dirichlet_helpers.py) and the inputs of
tests/test_gpu_j_dirichlet_cg.py, checked without a device: decidability of every stopping test the GPU file relies on,
the restatement against a direct sparse solve and against the reference's own answers (reg_tau0 / class_tau0 of
ops_sensor123.npz) within ||x - x*|| <= rtol ||b|| / lambda_min(L_uu), its edge cases, the float32 tolerance, and the
Python layer (learning.regression_tikhonov(..., solver="cg"), plugin.install(..., harmonic=True)) on a fake device."""
import types

import numpy as np
import pytest

import cg_helpers as cg
import dirichlet_helpers as dh
import learning_helpers as lh
from conftest import load_golden
from pygsp_amd import learning, plugin

F64, F32 = np.float64, np.float32


@pytest.fixture(scope="module")
def golden():
    return dh.golden_cases(load_golden("ops_sensor123.npz"))


@pytest.fixture(scope="module")
def fp32_pairs():
    """Per float32 problem: the restatement with float64 sums and with float32 sums, at the problem's rtol."""
    out = {}
    for key in dh.FP32_PROBLEMS:
        pb = dh.problem(*key)
        _, rtol, gap = dh.probe(key, F32)
        out[key] = (gap, rtol, dh.harmonic(pb.W, pb.mask, pb.y, rtol=rtol, dt=F32, acc=F64),
                    dh.harmonic(pb.W, pb.mask, pb.y, rtol=rtol, dt=F32, acc=F32))
    return out


@pytest.mark.parametrize("key", dh.FP64_PROBLEMS, ids=str)
def test_decidability_fp64(key):
    """Sums in float64 and in longdouble: identical counts; the rtol the GPU tests use lies at least MIN_GAP
    (relative) from every residual of every non-zero column."""
    pb = dh.problem(*key)
    _, rtol, gap = dh.probe(key, F64)
    lo, hi = dh.RTOL_RANGE[np.dtype(F64)]
    assert lo <= rtol <= hi and gap >= cg.MIN_GAP, (key, rtol, gap)
    xl, itl, _, _ = dh.reference(key, F64)
    x, it, _ = dh.harmonic(pb.W, pb.mask, pb.y, rtol=rtol)
    dev = cg.col_err(x, xl).max()
    print("%s: rtol %.2e gap %.3f iterations %d..%d, float64 against longdouble sums %.1e" % (
        key, rtol, gap, itl.min(), itl.max(), dev))
    assert np.array_equal(it, itl), key
    assert dev <= 1e-4 * dh.X64_TOL, key  # (four orders of margin under the GPU file's tolerance)
    assert np.array_equal(xl[pb.mask], pb.y[pb.mask])
    zero = ~pb.y[pb.mask].any(axis=0)
    assert not itl[zero].any() and not xl[:, zero].any()


def test_decidability_fp32(fp32_pairs):
    for key, (gap, rtol, (xa, ia, _), (xb, ib, _)) in fp32_pairs.items():
        lo, hi = dh.RTOL_RANGE[np.dtype(F32)]
        assert lo <= rtol <= hi and gap >= cg.MIN_GAP and np.array_equal(ia, ib), (key, rtol, gap, ia, ib)
        assert np.array_equal(dh.reference(key, F32)[1], ia)  # what the GPU file compares with: the float64-sum one


def test_fp32_tolerance(fp32_pairs):
    """X32_TOL is 10 x the largest deviation of x between the two float32 restatements over the float32 problems."""
    worst = max(cg.col_err(p[3][0], p[2][0]).max() for p in fp32_pairs.values())
    print("largest float32 x deviation between the restatements: %.3e" % worst)
    assert 10 * worst <= dh.X32_TOL < 11 * worst


def test_columns_stop_at_different_iterations():
    """One matrix and relative thresholds: the non-zero columns of a batch need nearly the same number of iterations
    (the same one at N = 300).  They differ at N = 3000, and under the atol of the frozen-column test, which lies
    MIN_GAP from every ||r_k||, the counts of BASE spread over at least five values."""
    for key in dh.MAIN:
        for dtype in (F64, F32):
            assert dh.reference(key, dtype)[1][cg.ZERO_PATTERN] == 0
    it = dh.reference(dh.MAIN[1], F64)[1]
    assert len(set(it[it > 0])) >= 2, it
    atol, gap = dh.pick_atol(dh.BASE, F64)
    it = dh.reference(dh.BASE, F64, atol=atol)[1]
    print("atol %.3e gap %.3f counts %s" % (atol, gap, it))
    assert gap >= cg.MIN_GAP and len(set(it)) >= 5, (gap, it)
    pb = dh.problem(*dh.BASE)
    itd = dh.harmonic(pb.W, pb.mask, pb.y, rtol=dh.reference(dh.BASE, F64)[3], atol=atol)[1]
    assert np.array_equal(it, itd)  # float64 sums and longdouble sums agree under it too


@pytest.mark.parametrize("key", dh.MAIN + dh.WIDE[1:2] + dh.SMALL[7:8] + dh.SMALL[10:21:3], ids=str)
def test_against_a_direct_solve(key):
    pb = dh.problem(*key)
    x, iters, _, rtol = dh.reference(key, F64)
    err = np.linalg.norm(x - dh.direct(pb.W, pb.mask, pb.y), axis=0)
    bound = dh.error_bound(pb.W, pb.mask, pb.y, rtol)
    print("%s: error / bound at most %.3f" % (key, np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
    assert (err <= bound).all(), (key, err / np.maximum(bound, 1e-300))
    assert (iters < 10 * pb.N).all()


def test_a_sparse_mask_converges_too():
    """10 % measured at N = 300: lambda_min(L_uu) is small, CG takes longer, the bound still holds."""
    pb = dh.problem(*dh.BASE)
    mask = np.random.default_rng(300).uniform(size=300) > 0.9
    x, iters, _ = dh.harmonic(pb.W, mask, pb.y, rtol=1e-10)
    err = np.linalg.norm(x - dh.direct(pb.W, mask, pb.y), axis=0)
    assert (err <= dh.error_bound(pb.W, mask, pb.y, 1e-10)).all() and iters.max() > dh.reference(dh.BASE, F64)[1].max()


def test_against_the_references_goldens(golden):
    """reg_tau0 and class_tau0 were computed by the reference's spsolve: the restatement at the Python layer's
    default rtol lies within the bound of them."""
    for name, W, mask, y, ref in golden:
        Y = dh.one_hot_measured(y, mask) if name == "class_tau0" else np.nan_to_num(y)[:, None]
        x, iters, _ = dh.harmonic(W, mask, Y, rtol=1e-10)
        err = np.linalg.norm(x - ref.reshape(x.shape), axis=0)
        bound = dh.error_bound(W, mask, Y, 1e-10)
        print("%s: iterations %s, error / bound %s, lambda_min %.3f" % (name, iters, err / bound, dh.blocks(W, mask, Y)[2]))
        assert (err <= bound).all() and (iters > 0).all()
        if name == "class_tau0":
            assert np.array_equal(np.argmax(x, axis=1), np.argmax(ref, axis=1))


def test_restatement_edges():
    pb = dh.problem(*dh.ALL_MEASURED)
    x, it, _, _ = dh.reference(dh.ALL_MEASURED, F64)
    assert np.array_equal(x, pb.y) and not it.any()
    x, it, _, _ = dh.reference(dh.NONE_MEASURED, F64)
    assert not x.any() and not it.any()
    pb = dh.problem(*dh.SPLIT)
    x, it, _, _ = dh.reference(dh.SPLIT, F64)
    assert not x[64:].any() and x[:64][~pb.mask[:64]].any() and it.max() > 0
    assert not pb.mask[64:].any() and np.array_equal(x[pb.mask], pb.y[pb.mask])
    pb = dh.problem(*dh.BASE)
    x0, it0, _ = dh.harmonic(pb.W, pb.mask, pb.y, rtol=1e-10, maxiter=0)
    assert np.array_equal(x0, np.where(pb.mask[:, None], pb.y, 0.0)) and not it0.any()
    xn, itn, _ = dh.harmonic(pb.W, pb.mask, pb.nan_y, rtol=1e-10)  # NaN at every unmeasured row: never read
    xz, itz, _ = dh.harmonic(pb.W, pb.mask, pb.y, rtol=1e-10)
    assert np.isfinite(xn).all() and xn.tobytes() == xz.tobytes() and np.array_equal(itn, itz)
    x1, it1, _ = dh.harmonic(pb.W, pb.mask, pb.y[:, 2], rtol=1e-10)  # 1-D y; the columns are independent
    assert x1.shape == (pb.N, 1) and it1[0] == itz[2] and cg.col_err(x1, xz[:, [2]])[0] <= 1e-12


# ---- the Python layer on a fake device ------------------------------------------------------------------------------
class _FakeDevice:
    """Stands in for the device graph: the restatement on the host."""

    def __init__(self, W):
        self.W, self.dtype = W, np.dtype(np.float64)
        self.calls = []

    def dirichlet_cg(self, mask, y, rtol=None, atol=0.0, maxiter=None):
        self.calls.append((np.array(mask), np.array(y), rtol, atol, maxiter))
        x, iters, _ = dh.harmonic(self.W, mask, y, rtol=1e-10 if rtol is None else rtol, atol=atol, maxiter=maxiter)
        return (x[:, 0] if np.ndim(y) == 1 else x), iters, 0.0

    def tikhonov_cg(self, *args, **kwargs):
        raise AssertionError("tau = 0 must not reach the tau > 0 solver")


class _Graph:
    def __init__(self, W, dev):
        self.L, self.N, self.n_vertices, self._dev = lh.laplacian(W), W.shape[0], W.shape[0], dev

    def device_graph(self, dtype=None):
        return self._dev


def test_regression_with_solver_cg_on_a_fake_device(golden):
    name, W, mask, y, ref = golden[0]
    assert np.isnan(y[~mask]).all()
    dev = _FakeDevice(W)
    G = _Graph(W, dev)
    expect, _, _ = dh.harmonic(W, mask, np.nan_to_num(y), rtol=1e-10)
    x = learning.regression_tikhonov(G, y, mask, tau=0, solver="cg")
    assert x.shape == (G.N,) and np.array_equal(x, expect[:, 0])
    assert np.isfinite(dev.calls[0][1]).all() and dev.calls[0][2:] == (None, 0.0, None)
    assert np.linalg.norm(x - ref) <= dh.error_bound(W, mask, np.nan_to_num(y)[:, None], 1e-10)[0]
    Y2 = np.column_stack([y, 2 * y])
    x2 = learning.regression_tikhonov(G, Y2, mask, solver="cg")  # tau = 0 is the default
    assert x2.shape == (G.N, 2) and np.array_equal(x2, dh.harmonic(W, mask, np.nan_to_num(Y2), rtol=1e-10)[0])
    assert np.isnan(Y2[~mask]).all() and cg.col_err(x2[:, :1], x[:, None])[0] < 1e-12  # (the input is kept)
    learning.regression_tikhonov(G, y, mask, tau=0, solver="cg", rtol=1e-6, atol=1e-3, maxiter=7)
    assert dev.calls[-1][2:] == (1e-6, 1e-3, 7)


def test_classification_with_solver_cg_on_a_fake_device(golden):
    name, W, mask, lab, ref = golden[1]
    G = _Graph(W, _FakeDevice(W))
    X = learning.classification_tikhonov(G, lab, mask, tau=0, solver="cg")
    assert X.shape == ref.shape and np.array_equal(np.argmax(X, axis=1), np.argmax(ref, axis=1))
    assert (np.linalg.norm(X - ref, axis=0) <= dh.error_bound(W, mask, dh.one_hot_measured(lab, mask), 1e-10)).all()


def test_solver_argument(golden):
    name, W, mask, y, ref = golden[0]
    dev = _FakeDevice(W)
    G = _Graph(W, dev)
    with pytest.raises(ValueError, match="solver"):
        learning.regression_tikhonov(G, y, mask, tau=0, solver="lu")
    with pytest.raises(ValueError, match="solver"):
        learning.regression_tikhonov(G, y, mask, tau=0.5, solver="lu")
    with pytest.raises(ValueError, match="M should be of size"):  # the size check comes first, as in the reference
        learning.regression_tikhonov(G, y, mask[:-1], tau=0, solver="lu")
    with pytest.raises(NotImplementedError, match='solver="cg"'):
        learning.regression_tikhonov(G, y, mask, tau=0)
    with pytest.raises(NotImplementedError):
        learning.regression_tikhonov(G, y, mask, tau=-1.0, solver="cg")
    assert dev.calls == []


def _standin_pygsp():
    """A pygsp-shaped module: what install() touches, and a learning module whose classification_tikhonov looks
    regression_tikhonov up at call time (learning.py:248-251)."""
    mod = types.ModuleType("pygsp_standin")
    mod.filters = types.ModuleType("pygsp_standin.filters")
    mod.filters.approximations = types.ModuleType("pygsp_standin.filters.approximations")
    mod.filters.approximations.cheby_op = lambda *a: "reference cheby_op"
    learn = types.ModuleType("pygsp_standin.learning")
    learn.original_calls = []

    def regression_tikhonov(G, y, M, tau=0):
        learn.original_calls.append(tau)
        return "reference regression"

    def classification_tikhonov(G, y, M, tau=0):
        return learn.regression_tikhonov(G, dh.one_hot_measured(y, M), M, tau)

    learn.regression_tikhonov = regression_tikhonov
    learn.classification_tikhonov_simplex = lambda G, y, M, tau=0.1, **kwargs: "reference simplex"
    learn.classification_tikhonov = classification_tikhonov
    mod.learning = learn
    return mod


def test_install_with_harmonic_serves_tau_zero(golden, monkeypatch):
    name, W, mask, y, ref = golden[0]
    lab, cref = golden[1][3], golden[1][4]
    dev = _FakeDevice(W)
    monkeypatch.setattr(plugin, "device_graph_for", lambda G, ctx=None, dtype=None: dev)
    L = lh.laplacian(W)
    G = types.SimpleNamespace(L=L, N=L.shape[0], n_vertices=L.shape[0])
    mod = _standin_pygsp()
    original = mod.learning.regression_tikhonov
    with pytest.raises(ValueError, match="harmonic"):
        plugin.install(mod, harmonic=True)
    assert mod.learning.regression_tikhonov is original
    plugin.install(mod, learning=True, harmonic=True)
    try:
        x = mod.learning.regression_tikhonov(G, y, mask)  # tau = 0, the reference's default
        expect, _, _ = dh.harmonic(W, mask, np.nan_to_num(y), rtol=1e-10)
        assert np.array_equal(x, expect[:, 0]) and dev.calls[0][2:] == (None, 0.0, None)
        X = mod.learning.classification_tikhonov(G, lab, mask, tau=0)  # follows at call time
        assert np.array_equal(np.argmax(X, axis=1), np.argmax(cref, axis=1))
        assert mod.learning.original_calls == []
        # tau < 0 and a dense L: the saved original
        assert mod.learning.regression_tikhonov(G, y, mask, tau=-1) == "reference regression"
        Gd = types.SimpleNamespace(L=L.toarray(), N=L.shape[0], n_vertices=L.shape[0])
        assert mod.learning.regression_tikhonov(Gd, y, mask, tau=0) == "reference regression"
        assert mod.learning.original_calls == [-1, 0]
        # installing again without the flag hands tau = 0 back
        plugin.install(mod, learning=True)
        assert mod.learning.regression_tikhonov(G, y, mask, tau=0) == "reference regression"
        assert mod.learning.original_calls == [-1, 0, 0] and len(dev.calls) == 2
    finally:
        plugin.uninstall(mod)
    assert mod.learning.regression_tikhonov is original and plugin._SAVED not in mod.learning.__dict__
