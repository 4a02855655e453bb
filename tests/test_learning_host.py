"""classification_tikhonov_simplex without a device: the numpy restatement of the iteration (tests/learning_helpers.py)
against the math, the projection against a sort-based formula, the Python layer's input handling and the plugin seam
on a fake device, and the C entry point's argument checks."""
import ctypes
import types

import numpy as np
import pytest
from scipy import sparse
from scipy.sparse import linalg as splinalg

import learning_helpers as lh
from conftest import load_golden
from pygsp_amd import _capi, learning, plugin


@pytest.fixture(scope="module")
def golden():
    W, labels, C = lh.golden_problem(load_golden("ops_sensor123.npz"))
    L = lh.laplacian(W)
    lmax = float(np.linalg.eigvalsh(L.toarray()).max())
    return L, labels, C, lmax


def test_golden_tight_solve_is_a_fixed_point(golden):
    L, labels, C, lmax = golden
    tau = 0.1
    step = 0.5 / (1 + tau * lmax)
    X, info = lh.solve(L, labels, C, tau, step, rtol=None, xtol=1e-14, maxit=20000)
    assert info["crit"] == "XTOL"
    assert lh.fixed_point_residual(L, X, labels, C, tau, step) < 1e-10
    assert X.min() >= 0 and np.abs(X.sum(axis=1) - 1).max() < 1e-13


def _projected_gradient(L, labels, C, tau, step, iters):
    """Plain projected gradient from the uniform point: no acceleration, another start."""
    m = (labels >= 0).astype(np.float64)
    Y = lh.one_hot(labels, C)
    X = np.full((labels.size, C), 1.0 / C)
    for _ in range(iters):
        Xn = lh.project_simplex(X - step * lh.gradient(L, X, m, Y, tau))
        if np.abs(Xn - X).max() < 1e-15:
            return Xn
        X = Xn
    return X


def test_golden_agrees_with_projected_gradient(golden):
    L, labels, C, lmax = golden
    tau = 0.1
    step = 0.5 / (1 + tau * lmax)
    X, _ = lh.solve(L, labels, C, tau, step, rtol=None, xtol=1e-14, maxit=20000)
    P = _projected_gradient(L, labels, C, tau, step, 200000)
    assert lh.fixed_point_residual(L, P, labels, C, tau, step) < 1e-11
    assert np.abs(X - P).max() < 1e-8


def test_default_rule_and_the_objective(golden):
    """The default rule stops on RTOL; obj_k is f(X_k) and the rule's arithmetic is what the docstring states."""
    L, labels, C, lmax = golden
    tau = 0.5
    step = 0.5 / (1 + tau * lmax)
    X, info = lh.solve(L, labels, C, tau, step)
    assert info["crit"] == "RTOL" and info["niter"] >= 2
    obj = info["objective"]
    assert len(obj) == info["niter"] + 1
    m = (labels >= 0).astype(np.float64)
    assert obj[-1] == pytest.approx(lh.objective(L, X, m, lh.one_hot(labels, C), tau), rel=1e-13)
    rel = np.abs(np.diff(obj)) / obj[1:]
    assert rel[-1] < 1e-3 and (rel[:-1] >= 1e-3).all()
    _, info7 = lh.solve(L, labels, C, tau, step, rtol=None, maxit=7)
    assert (info7["niter"], info7["crit"]) == (7, "MAXIT")


def _sort_projection(z):
    """The sort-based formula: u sorted descending, rho = the largest j with u_j - (sum_{i<=j} u_i - 1) / j > 0,
    theta = (sum_{i<=rho} u_i - 1) / rho."""
    u = np.sort(z)[::-1]
    css = np.cumsum(u)
    j = np.arange(1, z.size + 1)
    rho = j[u - (css - 1) / j > 0][-1]
    return np.maximum(z - (css[rho - 1] - 1) / rho, 0)


@pytest.mark.parametrize("C", list(range(1, 18)) + [31, 32, 33, 63, 64, 65, 100, 128, 129, 200, 255, 256])
def test_projection_matches_the_sort_formula(C):
    rng = np.random.default_rng(C)
    rows = [rng.standard_normal(C) * s for s in (1e-3, 1.0, 10.0)]
    rows += [np.full(C, 0.3), np.full(C, -2.0), np.round(rng.standard_normal(C) * 2) / 2]  # all equal, ties
    rows += [np.where(rng.random(C) < 0.5, 1.0, 0.0)]
    Z = np.array(rows)
    P = lh.project_simplex(Z)
    for z, p in zip(Z, P):
        ref = _sort_projection(z)
        assert np.abs(p - ref).max() < 1e-13 * max(1.0, np.abs(z).max())
        assert p.min() >= 0 and abs(p.sum() - 1) < 1e-12


class _FakeDevice:
    """Stands in for the float64 device graph: the restatement on the host."""

    def __init__(self, L):
        self.L = L
        self.calls = []

    def tikhonov_simplex(self, tau, step, labels, n_classes, **opts):
        self.calls.append((tau, step, np.array(labels), n_classes, opts))
        return lh.solve(self.L, labels, n_classes, tau, step, **opts)

    def tikhonov_cg(self, tau, mask, y, rtol=1e-5, atol=0.0, maxiter=None):
        A = sparse.diags(np.asarray(mask, dtype=np.float64)) + tau * self.L
        y2 = y.reshape(y.shape[0], -1)
        x = np.column_stack([splinalg.cg(A, y2[:, i], rtol=rtol, atol=atol)[0] for i in range(y2.shape[1])])
        return (x[:, 0] if y.ndim == 1 else x), None, 0.0


class _Graph:
    """What classification_tikhonov_simplex reads of a graph: n_vertices, lmax, device_graph(float64)."""

    def __init__(self, L, lmax, dev):
        self.L, self.lmax, self.N, self.n_vertices = L, lmax, L.shape[0], L.shape[0]
        self._dev = dev
        self.dtypes = []

    def device_graph(self, dtype=None):
        self.dtypes.append(np.dtype(dtype))
        return self._dev


def test_public_function_on_a_fake_device(golden):
    L, labels, C, lmax = golden
    G = _Graph(L, lmax, _FakeDevice(L))
    g = load_golden("ops_sensor123.npz")
    M = g["mask"]
    y = g["labels"].astype(float)
    y[~M] = np.nan  # allowed at unmeasured vertices, as in the reference's docstring example
    X = learning.classification_tikhonov_simplex(G, y, M, tau=0.1, verbosity="NONE")
    assert X.shape == (L.shape[0], C) and X.dtype == np.float64
    assert G.dtypes == [np.dtype(np.float64)]
    tau, step, lab, n, opts = G._dev.calls[0]
    assert step == 0.5 / (1 + 0.1 * lmax) and n == C and opts == {}
    np.testing.assert_array_equal(lab, labels)
    ref, _ = lh.solve(L, labels, C, 0.1, step)
    np.testing.assert_array_equal(X, ref)
    learning.classification_tikhonov_simplex(G, y, M, tau=0.1, rtol=None, xtol=1e-9, maxit=50, atol=None, dtol=0.0)
    assert G._dev.calls[-1][4] == {"rtol": None, "xtol": 1e-9, "maxit": 50, "atol": None, "dtol": 0.0}


def test_input_errors_come_before_device_work(golden):
    L, labels, C, lmax = golden
    dev = _FakeDevice(L)
    G = _Graph(L, lmax, dev)
    M = labels >= 0
    y = np.maximum(labels, 0)
    with pytest.raises(TypeError):
        learning.classification_tikhonov_simplex(G, y, M, tau=0.1, step=0.3)
    with pytest.raises(ValueError, match="Tau should be greater than 0."):
        learning.classification_tikhonov_simplex(G, y, M, tau=0)
    with pytest.raises(ValueError, match="Tau should be greater than 0."):
        learning.classification_tikhonov_simplex(G, y, M, tau=-1.0)
    with pytest.raises(ValueError, match="M should be of size"):
        learning.classification_tikhonov_simplex(G, y, M[:-1], tau=0.1)
    bad = y.copy()
    bad[np.flatnonzero(M)[0]] = -1  # a negative measured label: the reference would index the last column
    with pytest.raises(ValueError, match=">= 0"):
        learning.classification_tikhonov_simplex(G, bad, M, tau=0.1)
    nan = y.astype(float)
    nan[np.flatnonzero(M)[0]] = np.nan
    with pytest.raises(ValueError):
        learning.classification_tikhonov_simplex(G, nan, M, tau=0.1)
    assert dev.calls == []
    # negative labels at UNMEASURED vertices are zeroed first, as in the reference
    neg = y.copy()
    neg[~M] = -5
    learning.classification_tikhonov_simplex(G, neg, M, tau=0.1)
    np.testing.assert_array_equal(dev.calls[0][2], labels)


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

    def classification_tikhonov_simplex(G, y, M, tau=0.1, **kwargs):
        raise ImportError("Cannot import pyunlocbox")

    def classification_tikhonov(G, y, M, tau=0):
        Y = lh.one_hot(np.asarray(y, dtype=int), int(np.max(y)) + 1)
        return learn.regression_tikhonov(G, Y, M, tau)

    learn.regression_tikhonov = regression_tikhonov
    learn.classification_tikhonov_simplex = classification_tikhonov_simplex
    learn.classification_tikhonov = classification_tikhonov
    mod.learning = learn
    return mod


def test_plugin_seam_on_a_standin(golden, monkeypatch):
    L, labels, C, lmax = golden
    dev = _FakeDevice(L)
    monkeypatch.setattr(plugin, "device_graph_for", lambda G, ctx=None, dtype=None: dev)
    G = types.SimpleNamespace(L=L, lmax=lmax, N=L.shape[0], n_vertices=L.shape[0])
    mod = _standin_pygsp()
    originals = (mod.learning.regression_tikhonov, mod.learning.classification_tikhonov_simplex)
    M = labels >= 0
    y = np.maximum(labels, 0)
    plugin.install(mod)  # without the flag the learning module stays as it is
    assert (mod.learning.regression_tikhonov, mod.learning.classification_tikhonov_simplex) == originals
    plugin.install(mod, learning=False)
    assert (mod.learning.regression_tikhonov, mod.learning.classification_tikhonov_simplex) == originals
    plugin.install(mod, learning=True)
    try:
        X = mod.learning.classification_tikhonov_simplex(G, y, M, tau=0.1)  # no pyunlocbox needed
        ref, _ = lh.solve(L, labels, C, 0.1, 0.5 / (1 + 0.1 * lmax))
        np.testing.assert_array_equal(X, ref)
        # regression: tau > 0 and a sparse L on the device; classification_tikhonov follows at call time
        x = mod.learning.regression_tikhonov(G, y.astype(float), M, tau=0.5)
        A = (sparse.diags(M.astype(float)) + 0.5 * L).toarray()
        np.testing.assert_allclose(x, np.linalg.solve(A, np.where(M, y, 0.0)), rtol=1e-4, atol=1e-6)
        Xc = mod.learning.classification_tikhonov(G, y, M, tau=0.5)
        assert Xc.shape == (L.shape[0], C)
        assert mod.learning.original_calls == []
        # tau <= 0 and a dense L: the saved original
        assert mod.learning.regression_tikhonov(G, y, M, tau=0) == "reference regression"
        Gd = types.SimpleNamespace(L=L.toarray(), lmax=lmax, N=L.shape[0], n_vertices=L.shape[0])
        assert mod.learning.regression_tikhonov(Gd, y, M, tau=0.5) == "reference regression"
        assert mod.learning.original_calls == [0, 0.5]
    finally:
        plugin.uninstall(mod)
    assert (mod.learning.regression_tikhonov, mod.learning.classification_tikhonov_simplex) == originals
    assert plugin._SAVED not in mod.learning.__dict__


def test_entry_point_refuses_bad_arguments_without_a_device():
    lib = _capi.load()
    lab = np.zeros(4, dtype=np.int32)
    x = np.zeros(8)
    obj = np.zeros(301)
    n, c, ms = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_double()

    def call(tau=0.1, step=0.2, classes=2, rtol=1e-3, atol=-1.0, dtol=-1.0, xtol=-1.0, maxit=200, out=obj):
        return lib.gspx_tikhonov_simplex_dev(None, tau, step, _capi.ptr(lab), classes, rtol, atol, dtol, xtol, maxit,
                                             _capi.ptr(x), ctypes.byref(n), ctypes.byref(c), _capi.ptr(out),
                                             ctypes.byref(ms))

    for kw, what in ((dict(tau=0.0), "tau"), (dict(tau=float("inf")), "tau"), (dict(step=-1.0), "step"),
                     (dict(step=float("nan")), "step"), (dict(maxit=0), "maxit"), (dict(classes=0), "n_classes"),
                     (dict(classes=257), "n_classes"), (dict(xtol=float("nan")), "NaN"), (dict(out=None), "null"),
                     ({}, "null graph")):
        with pytest.raises(ValueError, match=what):
            _capi.check(call(**kw))
    # the refusals that every FISTA entry point makes, word for word as before the solvers shared one argument check
    # (the float32-graph and 2 GiB refusals need a graph: test_refusals_that_need_a_graph in tests/test_gpu_f_learning.py)
    for kw, text in ((dict(step=-1.0), "tikhonov_simplex: step must be positive and finite"),
                     (dict(maxit=0), "tikhonov_simplex: maxit must be 1..10000000 (got 0)"),
                     (dict(maxit=10000001), "tikhonov_simplex: maxit must be 1..10000000 (got 10000001)"),
                     (dict(classes=257), "tikhonov_simplex: n_classes must be 1..256 (got 257)"),
                     (dict(xtol=float("nan")),
                      "tikhonov_simplex: a tolerance is NaN (a negative one disables its criterion)"),
                     (dict(out=None), "tikhonov_simplex: null host output"),
                     ({}, "null graph")):
        with pytest.raises(ValueError) as e:
            _capi.check(call(**kw))
        assert str(e.value) == text
    # in the order of before: tau, step, maxit, n_classes, tolerances, host outputs, graph
    order = (dict(tau=0.0), dict(step=0.0), dict(maxit=0), dict(classes=0), dict(rtol=float("nan")), dict(out=None))
    for i, what in enumerate(("tau", "step", "maxit", "n_classes", "NaN", "null host")):
        bad = {}
        for later in order[i:]:
            bad.update(later)
        with pytest.raises(ValueError, match=what):
            _capi.check(call(**bad))
