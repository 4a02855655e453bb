"""classification_tikhonov_simplex on the device (gspx_tikhonov_simplex_dev) against the numpy restatement of the
iteration (tests/learning_helpers.py): the same niter and stopping criterion, objective sequences within 1e-12
relative, X within 1e-10, on the golden graph and on sensor graphs up to 100k vertices; every projection build;
determinism; the float32 mirror graph; the real pygsp through plugin.install(learning=True) where one is importable.
Needs a real MI355X: `-m gpu`."""
import ctypes
import importlib.util

import numpy as np
import pytest

import learning_helpers as lh
from conftest import load_golden
from pygsp_amd import _capi, graphs, learning

pytestmark = pytest.mark.gpu


def _check(dev_out, ref_out):
    (X, info), (Xr, ir) = dev_out, ref_out
    assert (info["niter"], info["crit"]) == (ir["niter"], ir["crit"])
    obj, objr = info["objective"], ir["objective"]
    assert obj.shape == objr.shape
    assert np.abs(obj - objr).max() <= 1e-12 * np.abs(objr).max()
    assert np.abs(X - Xr).max() < 1e-10
    assert X.min() >= 0 and np.abs(X.sum(axis=1) - 1).max() < 1e-12


def _sensor_problem(N, C, seed=0, frac=0.1):
    G = graphs.Sensor(N, seed=seed)
    G.estimate_lmax()
    rng = np.random.default_rng(seed + 1)
    measured = rng.random(N) < frac
    y = rng.integers(0, C, N).astype(float)
    y[measured] = np.arange(measured.sum()) % C  # (every class present)
    y[~measured] = np.nan
    return G, y, measured


@pytest.fixture(scope="module")
def golden_graph():
    g = load_golden("ops_sensor123.npz")
    W, labels, C = lh.golden_problem(g)
    G = graphs.Graph(W)
    G.estimate_lmax()
    return G, g, labels, C


def _runs(G, y, M, tau, **opts):
    labels, C = learning.simplex_labels(y, M)
    step = learning.simplex_step(G, tau)
    dev = learning.simplex_solve(G, y, M, tau, **opts)
    ref = lh.solve(G.L, labels, C, tau, step, **opts)
    return dev, ref


def _rule_cases(G, y, M, tau):
    """The default rule, then atol, dtol, xtol and maxit each set to fire on its own, at thresholds that no value of
    the restatement's sequence lies near."""
    yield {}
    _, free = lh.solve(G.L, *learning.simplex_labels(y, M), tau, learning.simplex_step(G, tau), rtol=None, maxit=12)
    obj, dx = free["objective"], free["dx"]
    yield dict(rtol=None, atol=lh.threshold_between(obj, 8))
    yield dict(rtol=None, dtol=lh.threshold_between(np.abs(np.diff(obj)), 7))
    yield dict(rtol=None, xtol=lh.threshold_between(dx, 6))
    yield dict(rtol=None, maxit=9)


def test_golden_graph_every_rule(golden_graph):
    G, g, labels, C = golden_graph
    M = g["mask"]
    y = g["labels"].astype(float)
    for tau in (0.1, 2.0):
        crits = []
        for opts in _rule_cases(G, y, M, tau):
            dev, ref = _runs(G, y, M, tau, **opts)
            _check(dev, ref)
            crits.append(dev[1]["crit"])
        assert crits == ["RTOL", "ATOL", "DTOL", "XTOL", "MAXIT"]


@pytest.mark.parametrize("N,C", [(10_000, 3), (100_000, 4)])
def test_sensor_graphs_every_rule(N, C):
    G, y, M = _sensor_problem(N, C)
    crits = []
    for opts in _rule_cases(G, y, M, 0.5):
        dev, ref = _runs(G, y, M, 0.5, **opts)
        _check(dev, ref)
        crits.append(dev[1]["crit"])
    assert crits == ["RTOL", "ATOL", "DTOL", "XTOL", "MAXIT"]


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 8, 10, 16, 17, 64, 65, 256])
def test_every_projection_build(C):
    """C <= 16: a row per thread (builds 2, 4, 8, 16); 17..64 and 65..256: a row per wave (1 and 4 values per lane)."""
    G, y, M = _sensor_problem(5000, C, seed=C, frac=0.3)
    dev, ref = _runs(G, y, M, 0.3, rtol=None, maxit=5)
    _check(dev, ref)
    assert dev[0].shape == (G.N, C)


def test_tight_solve_meets_the_residual_bound(golden_graph):
    G, g, labels, C = golden_graph
    X, info = learning.simplex_solve(G, g["labels"], g["mask"], 0.1, rtol=None, xtol=1e-14, maxit=20000)
    assert info["crit"] == "XTOL"
    assert lh.fixed_point_residual(G.L, X, labels, C, 0.1, learning.simplex_step(G, 0.1)) < 1e-10


def test_repeated_calls_give_identical_bits():
    G, y, M = _sensor_problem(100_000, 10, seed=4)
    a = learning.simplex_solve(G, y, M, 0.5, rtol=None, maxit=40)
    b = learning.simplex_solve(G, y, M, 0.5, rtol=None, maxit=40)
    assert a[0].tobytes() == b[0].tobytes()
    assert a[1]["objective"].tobytes() == b[1]["objective"].tobytes()
    c = learning.simplex_solve(G, y, M, 0.5)  # the default rule: the result is one of the capped run's iterates
    d = learning.simplex_solve(G, y, M, 0.5)
    assert c[0].tobytes() == d[0].tobytes() and c[1]["niter"] == d[1]["niter"]


def test_float32_mirror_graph_gives_the_float64_result():
    G64, y, M = _sensor_problem(20_000, 4, seed=2)
    G32 = graphs.Sensor(20_000, seed=2, compute_dtype=np.float32)
    G32._lmax = G64.lmax  # (the same step on both)
    X64 = learning.classification_tikhonov_simplex(G64, y, M, tau=0.5)
    X32 = learning.classification_tikhonov_simplex(G32, y, M, tau=0.5)
    assert X32.dtype == np.float64
    assert X32.tobytes() == X64.tobytes()


def test_refusals_that_need_a_graph():
    """The two shared refusals that the host test cannot reach, word for word as before the solvers shared one argument
    check: a float32 graph, and a panel past 2 GiB (N > 1048544 at 256 classes; it fires before anything is allocated
    or read, so the label buffer stands in for the result pointer)."""
    from scipy import sparse
    n = 1_048_600
    big = graphs.Graph(sparse.diags([np.ones(n - 1), np.ones(n - 1)], [1, -1]).tocsr()).device_graph(np.float64)
    small32 = graphs.Graph(sparse.diags([np.ones(4), np.ones(4)], [1, -1]).tocsr(),
                           compute_dtype=np.float32).device_graph(np.float32)
    obj = np.zeros(201)
    niter, crit, ms = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_double()
    for dev, classes, text in (
            (small32, 2, "tikhonov_simplex: the graph computes in float32; the solver needs the float64 graph"),
            (big, 256, "tikhonov_simplex: an N x n_classes panel exceeds 2 GiB")):
        with dev.ctx._temporaries() as t:
            lab = t.upload(np.zeros(dev.N, dtype=np.int32))
            with pytest.raises(ValueError) as e:
                _capi.check(_capi.load().gspx_tikhonov_simplex_dev(
                    dev._h, 0.1, 0.2, ctypes.c_void_p(lab.ptr), classes, 1e-3, -1.0, -1.0, -1.0, 200,
                    ctypes.c_void_p(lab.ptr), ctypes.byref(niter), ctypes.byref(crit), _capi.ptr(obj), ctypes.byref(ms)))
        assert str(e.value) == text


@pytest.mark.skipif(importlib.util.find_spec("pygsp") is None, reason="needs an importable pygsp next to the GPU")
def test_real_pygsp_through_the_seam():
    import pygsp

    from pygsp_amd import plugin
    G = pygsp.graphs.Sensor(500, seed=0)
    G.estimate_lmax()
    rng = np.random.default_rng(0)
    M = rng.random(G.N) < 0.2
    y = rng.integers(0, 3, G.N).astype(float)
    plugin.install(pygsp, learning=True)
    try:
        X = pygsp.learning.classification_tikhonov_simplex(G, y, M, tau=0.1)
        x = pygsp.learning.regression_tikhonov(G, y, M, tau=0.5)
    finally:
        plugin.uninstall(pygsp)
    labels, C = learning.simplex_labels(y, M)
    Xr, _ = lh.solve(G.L.astype(np.float64), labels, C, 0.1, 0.5 / (1 + 0.1 * G.lmax))
    assert np.abs(X - Xr).max() < 1e-10
    A = (np.diag(M.astype(float)) + 0.5 * G.L.toarray())
    np.testing.assert_allclose(x, np.linalg.solve(A, np.where(M, y, 0.0)), rtol=1e-4, atol=1e-6)
