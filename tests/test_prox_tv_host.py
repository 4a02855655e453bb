"""The graph total-variation prox without a device: the numpy restatement of the iteration (tests/prox_tv_helpers.py)
against a closed form and against the duality gap; the argument handling of pygsp_amd.optimization.prox_tv on a fake
device graph; the plugin seam on a pygsp-shaped stand-in; the C signature."""
import ctypes
import types

import numpy as np
import pytest
from scipy import sparse

import prox_tv_helpers as th
from oracle import knn_oracle as knn
from pygsp_amd import _capi, optimization, plugin


@pytest.mark.parametrize("w", [1.0, 0.3, 4.0])
@pytest.mark.parametrize("gamma", [0.05, 0.5, 5.0])
def test_two_vertices_closed_form(w, gamma):
    """One edge of weight w: z = x + c (1, -1), c = clip((x_1 - x_0) / 2, +-gamma sqrt(w))."""
    W = sparse.csr_matrix(np.array([[0.0, w], [w, 0.0]]))
    D = th.incidence(W)
    lmax = 2.0 * w
    for x in (np.array([0.2, 1.5]), np.array([1.0, -0.7]), np.array([0.4, 0.4])):
        z, info = th.solve(D, x, gamma, 1.0 / (2.0 * lmax), rtol=None, xtol=1e-15, maxit=5000)
        c = np.clip((x[1] - x[0]) / 2.0, -gamma * np.sqrt(w), gamma * np.sqrt(w))
        assert np.abs(z - (x + c * np.array([1.0, -1.0]))).max() < 1e-12


@pytest.fixture(scope="module")
def sensor300():
    W = knn.knn_weights(knn.sensor_coords(300, seed=0), 6)[0]
    D = th.incidence(W)
    lmax = float(np.linalg.eigvalsh((D @ D.T).toarray())[-1])
    return W, D, lmax


@pytest.mark.parametrize("gamma", [0.05, 0.5])
def test_tight_run_closes_the_duality_gap(sensor300, gamma):
    W, D, lmax = sensor300
    x = np.random.default_rng(0).standard_normal((300, 3))
    z, info = th.solve(D, x, gamma, 1.0 / (2.0 * lmax), rtol=None, xtol=1e-13, maxit=400000)
    assert info["crit"] == "XTOL"
    assert np.abs(info["u"]).max() <= gamma
    assert info["objective"][-1] == pytest.approx(th.primal_objective(x, z, gamma, D), rel=1e-12)
    assert th.duality_gap(x, z, gamma, D) <= 1e-9 * info["objective"][-1]


class _FakeDevice:
    """Stands in for the float64 device graph: the restatement on the host."""

    def __init__(self, D):
        self.D = D
        self.calls = []

    def prox_tv(self, x, gamma, step, **opts):
        self.calls.append((np.array(x), gamma, step, opts))
        return th.solve(self.D, x, gamma, step, **opts)


class _Graph:
    """What prox_tv reads of a graph: n_vertices, lmax, W, is_directed, device_graph(float64)."""

    def __init__(self, W, lmax, dev):
        self.W, self.lmax, self.N, self.n_vertices = W, lmax, W.shape[0], W.shape[0]
        self._dev = dev
        self.dtypes = []

    def is_directed(self):
        return False

    def device_graph(self, dtype=None):
        self.dtypes.append(np.dtype(dtype))
        return self._dev


def test_public_function_on_a_fake_device(sensor300):
    W, D, lmax = sensor300
    G = _Graph(W, lmax, _FakeDevice(D))
    rng = np.random.default_rng(1)
    x = rng.standard_normal((300, 3))
    z = optimization.prox_tv(x, 0.1, G, verbosity="NONE", use_matrix=False)
    assert z.shape == x.shape and z.dtype == np.float64
    assert G.dtypes == [np.dtype(np.float64)]
    _, gamma, step, opts = G._dev.calls[0]
    assert gamma == 0.1 and step == 1.0 / (2.0 * lmax) and opts == {"rtol": 10e-4, "maxit": 200}
    assert optimization.tv_step(G, 3) == 1.0 / (2.0 * lmax * 3)
    np.testing.assert_array_equal(z, th.solve(D, x, 0.1, step)[0])
    # tol is the reference's name for rtol; nu scales the step; the other tolerances travel as keywords
    optimization.prox_tv(x, 0.1, G, nu=2, tol=None, maxit=7, xtol=1e-9, atol=None, dtol=0.0)
    _, _, step2, opts2 = G._dev.calls[-1]
    assert step2 == 1.0 / (2.0 * lmax * 2)
    assert opts2 == {"rtol": None, "maxit": 7, "xtol": 1e-9, "atol": None, "dtol": 0.0}
    # one-dimensional in, one-dimensional out
    z1, info = optimization.prox_tv_solve(x[:, 0], 0.1, G)
    assert z1.shape == (300,) and info["crit"] == "RTOL"
    assert G._dev.calls[-1][0].shape == (300,)


def test_wide_panels_go_in_batches_of_256(sensor300):
    W, D, lmax = sensor300
    G = _Graph(W, lmax, _FakeDevice(D))
    x = np.random.default_rng(2).standard_normal((300, 600))
    z, infos = optimization.prox_tv_solve(x, 0.2, G, tol=None, maxit=3)
    assert [c[0].shape[1] for c in G._dev.calls] == [256, 256, 88]
    assert isinstance(infos, list) and len(infos) == 3
    np.testing.assert_array_equal(z[:, 512:], th.solve(D, x[:, 512:], 0.2, 1.0 / (2.0 * lmax), rtol=None, maxit=3)[0])
    np.testing.assert_array_equal(z[:, :256], th.solve(D, x[:, :256], 0.2, 1.0 / (2.0 * lmax), rtol=None, maxit=3)[0])


def test_input_errors_come_before_device_work(sensor300):
    W, D, lmax = sensor300
    dev = _FakeDevice(D)
    G = _Graph(W, lmax, dev)
    x = np.zeros(300)
    with pytest.raises(NotImplementedError):
        optimization.prox_tv(x, 0.1, G, A=lambda v: v)
    with pytest.raises(NotImplementedError):
        optimization.prox_tv(x, 0.1, G, At=lambda v: v)
    with pytest.raises(ValueError, match="gamma"):
        optimization.prox_tv(x, -0.1, G)
    with pytest.raises(ValueError, match="gamma"):
        optimization.prox_tv(x, float("nan"), G)
    with pytest.raises(ValueError, match="gamma"):
        optimization.prox_tv(x, float("inf"), G)
    with pytest.raises(TypeError, match="step"):
        optimization.prox_tv(x, 0.1, G, step=0.3)
    with pytest.raises(ValueError, match="shape"):
        optimization.prox_tv(np.zeros(299), 0.1, G)
    assert dev.calls == []


def _standin_pygsp(with_optimization=True):
    mod = types.ModuleType("pygsp_standin")
    mod.filters = types.ModuleType("pygsp_standin.filters")
    mod.filters.approximations = types.ModuleType("pygsp_standin.filters.approximations")
    mod.filters.approximations.cheby_op = lambda *a: "reference cheby_op"
    if with_optimization:
        opt = types.ModuleType("pygsp_standin.optimization")

        def prox_tv(x, gamma, G, A=None, At=None, nu=1, tol=10e-4, maxit=200, use_matrix=True):
            raise NameError("name 'verbose' is not defined")  # (what the reference's function does)

        opt.prox_tv = prox_tv
        mod.optimization = opt
    return mod


def test_plugin_seam_on_a_standin(sensor300, monkeypatch):
    W, D, lmax = sensor300
    dev = _FakeDevice(D)
    monkeypatch.setattr(plugin, "device_graph_for", lambda G, ctx=None, dtype=None: dev)
    G = types.SimpleNamespace(W=W, lmax=lmax, N=300, n_vertices=300, is_directed=lambda: False)
    mod = _standin_pygsp()
    original = mod.optimization.prox_tv
    x = np.random.default_rng(3).standard_normal(300)
    plugin.install(mod)  # without the flag the optimization module stays as it is
    assert mod.optimization.prox_tv is original
    plugin.install(mod, optimization=True)
    try:
        assert mod.optimization.prox_tv is not original
        z = mod.optimization.prox_tv(x, 0.3, G, tol=1e-4)
        np.testing.assert_array_equal(z, th.solve(D, x, 0.3, 1.0 / (2.0 * lmax), rtol=1e-4)[0])
        plugin.install(mod, optimization=False)  # asking again without the flag puts the original back
        assert mod.optimization.prox_tv is original
        plugin.install(mod, optimization=True)
    finally:
        plugin.uninstall(mod)
    assert mod.optimization.prox_tv is original
    assert plugin._SAVED not in mod.optimization.__dict__
    bare = _standin_pygsp(with_optimization=False)
    try:
        with pytest.raises(ValueError, match="optimization"):
            plugin.install(bare, optimization=True)
    finally:
        plugin.uninstall(bare)


def test_c_signature_is_declared():
    assert "gspx_prox_tv_dev" in _capi.SIGNATURES
    assert len(_capi.SIGNATURES["gspx_prox_tv_dev"][1]) == 15


def test_entry_point_refuses_bad_arguments_without_a_device():
    lib = _capi.load()
    x = np.zeros(8)
    obj = np.zeros(201)
    n, c, ms = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_double()

    def call(gamma=0.1, step=0.2, nsig=2, rtol=1e-3, atol=-1.0, dtol=-1.0, xtol=-1.0, maxit=200, out=obj):
        return lib.gspx_prox_tv_dev(None, gamma, step, nsig, _capi.ptr(x), _capi.ptr(x), rtol, atol, dtol, xtol, maxit,
                                    ctypes.byref(n), ctypes.byref(c), _capi.ptr(out), ctypes.byref(ms))

    for kw, what in ((dict(gamma=-1.0), "gamma"), (dict(gamma=float("nan")), "gamma"), (dict(step=0.0), "step"),
                     (dict(step=float("inf")), "step"), (dict(maxit=0), "maxit"), (dict(nsig=0), "signals"),
                     (dict(nsig=257), "signals"), (dict(dtol=float("nan")), "NaN"), (dict(out=None), "null"),
                     ({}, "null graph")):
        with pytest.raises(ValueError, match=what):
            _capi.check(call(**kw))
    # the refusals that every FISTA entry point makes, word for word as before the solvers shared one argument check
    # (the float32-graph and 2 GiB refusals need a graph: test_refusals_that_need_a_graph in tests/test_gpu_i_prox_tv.py)
    for kw, text in ((dict(step=0.0), "prox_tv: step must be positive and finite"),
                     (dict(maxit=0), "prox_tv: maxit must be 1..10000000 (got 0)"),
                     (dict(maxit=10000001), "prox_tv: maxit must be 1..10000000 (got 10000001)"),
                     (dict(nsig=257), "prox_tv: number of signals must be 1..256 (got 257)"),
                     (dict(dtol=float("nan")), "prox_tv: a tolerance is NaN (a negative one disables its criterion)"),
                     (dict(out=None), "prox_tv: null host output"),
                     ({}, "null graph")):
        with pytest.raises(ValueError) as e:
            _capi.check(call(**kw))
        assert str(e.value) == text
    # in the order of before: gamma, step, maxit, number of signals, tolerances, host outputs, graph
    order = (dict(gamma=-1.0), dict(step=0.0), dict(maxit=0), dict(nsig=0), dict(rtol=float("nan")), dict(out=None))
    for i, what in enumerate(("gamma", "step", "maxit", "signals", "NaN", "null host")):
        bad = {}
        for later in order[i:]:
            bad.update(later)
        with pytest.raises(ValueError, match=what):
            _capi.check(call(**bad))
