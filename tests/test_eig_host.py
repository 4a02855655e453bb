"""The full-basis eigensolver without a GPU: the sweep schedule the library reports, its argument checks, the numpy
restatement of the algorithm against the accuracy bars, and the routing of Graph.compute_fourier_basis(method='jacobi')
and plugin.install(full_basis=True) with the device solver replaced by that restatement."""
import ctypes
import types

import numpy as np
import pytest
from scipy import sparse

import eig_helpers as eh
from conftest import csr_from
from fourier_helpers import laplacian, upper_bound
from oracle import knn_oracle as knn
from pygsp_amd import _capi, fourier, graphs, plugin

BAR = 1e-13


@pytest.mark.parametrize("nb", [1, 2, 3, 7, 8, 20])
def test_schedule_visits_every_pair_once(nb):
    rounds = fourier.sym_eig_schedule(nb)
    assert len(rounds) == -(-nb // 2) * 2 - 1
    seen = []
    for r, rnd in enumerate(rounds):
        assert len(rnd) == nb // 2
        blocks = [b for pair in rnd for b in pair]
        assert len(set(blocks)) == len(blocks), "a block appears twice in round {}".format(r)
        assert all(0 <= i < j < nb for i, j in rnd)
        assert rnd == eh.round_robin(nb, r)  # the restatement walks the same order
        seen += rnd
    assert sorted(seen) == [(i, j) for i in range(nb) for j in range(i + 1, nb)]


def test_argument_errors_need_no_device():
    lib = _capi.load()
    fake_a, fake_v = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)  # never dereferenced: the checks fail first
    e = np.zeros(8)

    def refused(rc, words):
        with pytest.raises(ValueError):
            _capi.check(rc)
        assert words in _capi.last_error(), _capi.last_error()

    eig = lib.gspx_sym_eig_dev
    refused(eig(None, 8, fake_a, 8, fake_v, 8, _capi.ptr(e), 1e-13, 30, None, None), "null context")
    refused(eig(None, -1, fake_a, 8, fake_v, 8, _capi.ptr(e), 1e-13, 30, None, None), "negative order")
    refused(eig(None, 32769, fake_a, 32769, fake_v, 32769, _capi.ptr(e), 1e-13, 30, None, None), "at most 32768")
    refused(eig(None, 8, fake_a, 7, fake_v, 8, _capi.ptr(e), 1e-13, 30, None, None), "leading dimension")
    refused(eig(None, 8, fake_a, 8, fake_v, 7, _capi.ptr(e), 1e-13, 30, None, None), "leading dimension")
    refused(eig(None, 8, None, 8, fake_v, 8, _capi.ptr(e), 1e-13, 30, None, None), "null matrix")
    refused(eig(None, 8, fake_a, 8, None, 8, _capi.ptr(e), 1e-13, 30, None, None), "null matrix")
    refused(eig(None, 8, fake_a, 8, fake_v, 8, None, 1e-13, 30, None, None), "null matrix")
    for tol in (0.0, -1e-13, float("nan"), float("inf")):
        refused(eig(None, 8, fake_a, 8, fake_v, 8, _capi.ptr(e), tol, 30, None, None), "tol must be positive")
    refused(eig(None, 8, fake_a, 8, fake_v, 8, _capi.ptr(e), 1e-13, 0, None, None), "max_sweeps")
    overlapping = ctypes.c_void_p((1 << 20) + 8 * 60)  # begins inside A's 8 x 8 span
    refused(eig(None, 8, fake_a, 8, overlapping, 8, _capi.ptr(e), 1e-13, 30, None, None), "must not alias")
    # n = 0 with null pointers gets as far as the context check
    refused(eig(None, 0, None, 0, None, 0, None, 1e-13, 30, None, None), "null context")
    rounds = ctypes.c_int(0)
    refused(lib.gspx_sym_eig_schedule_describe(0, None, ctypes.byref(rounds)), "n_blocks")
    refused(lib.gspx_sym_eig_schedule_describe(1025, None, ctypes.byref(rounds)), "n_blocks")
    refused(lib.gspx_sym_eig_schedule_describe(4, None, None), "null output")
    scale = lib.gspx_panel_scale_cols_dev
    refused(scale(None, 4, fake_a, 8, 8, _capi.ptr(e)), "null context")
    refused(scale(None, -1, fake_a, 8, 8, _capi.ptr(e)), "negative number of rows")
    refused(scale(None, 4, fake_a, 7, 8, _capi.ptr(e)), "leading dimension")
    refused(scale(None, 4, None, 8, 8, _capi.ptr(e)), "null panel")
    assert _capi.ERR_NOCONV == 7


@pytest.mark.parametrize("case", ["sensor123", "random300"])
def test_restatement_meets_the_bars(golden_sensor123, case):
    if case == "sensor123":  # ragged: 123 = 3 * 32 + 27, four blocks with five padding rows
        A = csr_from(golden_sensor123, "Lcomb").toarray()
    else:                    # ten blocks, twelve padding rows, indefinite
        R = np.random.default_rng(300).standard_normal((300, 300))
        A = (R + R.T) / 2
    e, U, stats = eh.sym_eig(A)
    de, res, orth = eh.bars(A, e, U)
    print("{}: {} sweeps, eigenvalues {:.2e}, residual {:.2e}, orthonormality {:.2e}".format(case, stats["sweeps"], de,
                                                                                           res, orth))
    assert de <= BAR and res <= BAR and orth <= BAR
    assert stats["pad_mass"] == 0.0 and np.all(np.diff(e) >= 0) and stats["sweeps"] <= 14
    assert len(stats["skipped_per_sweep"]) == stats["sweeps"]
    with pytest.raises(ValueError):
        eh.sym_eig(A, max_sweeps=1)


def test_restatement_on_matrices_that_need_no_sweep():
    d = np.random.default_rng(1).standard_normal(70)
    e, U, stats = eh.sym_eig(np.diag(d))
    assert stats["sweeps"] == 0 and np.array_equal(e, np.sort(d)) and np.array_equal(np.abs(U).sum(0), np.ones(70))
    e, U, stats = eh.sym_eig(np.zeros((5, 5)))
    assert stats["sweeps"] == 0 and np.array_equal(U, np.eye(5)) and not e.any()


# ---- Graph-level rules, the device solver replaced by the restatement ----------------------------------------------
def _host_graph(monkeypatch, W):
    monkeypatch.setattr(graphs.Graph, "_setup_on_device", lambda self, adj: False)
    monkeypatch.setattr(graphs.Graph, "compute_laplacian", lambda self, lap_type="combinatorial": None)
    G = graphs.Graph(W, reorder="none", tiles=False)
    G._L = laplacian(W, "combinatorial")
    monkeypatch.setattr(graphs.Graph, "_get_upper_bound", lambda self: upper_bound(self.W, self.lap_type))
    calls, given = [], []
    ctx = types.SimpleNamespace(give=given.append)

    def device_full_basis(dev, **kw):
        calls.append(kw)
        e, U, stats = eh.sym_eig(G._L.toarray())
        U = U * fourier.sign_fix(U)[None, :]
        e[0] = 0
        return e, U, types.SimpleNamespace(buf="panel"), stats

    def device_partial_basis(dev, k, b, **kw):
        raise AssertionError("method='jacobi' must not reach the partial solver")

    monkeypatch.setattr(fourier, "device_full_basis", device_full_basis)
    monkeypatch.setattr(fourier, "device_partial_basis", device_partial_basis)
    monkeypatch.setattr(graphs.Graph, "device_graph", lambda self, dtype=None: types.SimpleNamespace(ctx=ctx))
    return G, calls, given


def test_jacobi_routing_and_bookkeeping(monkeypatch):
    W = sparse.csr_matrix(knn.knn_weights(knn.sensor_coords(70, seed=1), 6)[0])
    G, calls, given = _host_graph(monkeypatch, W)
    lam = np.linalg.eigvalsh(G._L.toarray())
    # the default and 'auto' stay the host's eigh
    G.compute_fourier_basis()
    assert calls == [] and G._U_dev is None and G._lmax_method == "fourier" and G.fourier_stats is None
    G._forget_spectrum()
    G.compute_fourier_basis(method="auto")
    G.compute_fourier_basis(70, method="device")
    assert calls == []
    G._forget_spectrum()
    # 'jacobi', full: the solver's panel is kept, lmax comes from the spectrum
    G.compute_fourier_basis(method="jacobi", tol=1e-12, maxiter=20)
    assert calls == [{"tol": 1e-12, "max_sweeps": 20}]
    assert G.U.shape == (70, 70) and G.e[0] == 0 and np.allclose(G.e, lam, atol=1e-12)
    assert G._lmax == G.e[-1] and G._lmax_method == "fourier" and G.fourier_stats["sweeps"] >= 1
    dev, panel = G._U_dev
    assert panel.buf == "panel" and G._basis_on_device() is G._U_dev
    G.compute_fourier_basis(method="jacobi")  # cached
    assert len(calls) == 1
    G._forget_spectrum()
    assert G._U_dev is None and G._U is None and G._lmax is None and given == ["panel"] and panel.buf is None
    # 'jacobi', k < N: solved in full, sliced under the partial-result rules; lmax left alone, no N x N panel kept
    G.compute_fourier_basis(n_eigenvectors=9, method="jacobi")
    assert calls[1] == {"tol": fourier.FULL_TOL, "max_sweeps": fourier.FULL_MAX_SWEEPS}
    assert G.U.shape == (70, 9) and G.e.shape == (9,) and G.e[0] == 0 and G._lmax is None and G._U_dev is None
    assert given == ["panel", "panel"]
    idx = np.argmax(np.abs(G.U), axis=0)
    assert np.all(G.U[idx, np.arange(9)] > 0) and np.allclose(G.e, np.r_[0, lam[1:9]], atol=1e-12)
    G.compute_fourier_basis(n_eigenvectors=4, method="jacobi")  # a cached basis of at least k vectors is kept
    assert len(calls) == 2 and G.U.shape == (70, 9)
    G.compute_fourier_basis(method="jacobi")  # the full one replaces the slice
    assert len(calls) == 3 and G.U.shape == (70, 70) and G._lmax == G.e[-1]
    with pytest.raises(ValueError):
        G.compute_fourier_basis(n_eigenvectors=0, method="jacobi")
    with pytest.raises(ValueError):
        G.compute_fourier_basis(n_eigenvectors=71, method="jacobi")


def test_plugin_routes_full_requests(monkeypatch):
    """install(fourier=True, full_basis=True) on a pygsp-shaped stand-in: full requests of graphs of at least
    plugin.FULL_BASIS_MIN_VERTICES vertices go to the device solver and land in _e / _U / _lmax with the panel cached
    for the exact path; smaller graphs and partial requests do what install(fourier=True) does; uninstall restores."""
    original_calls = []

    class Graph:
        def __init__(self, n):
            self.n_vertices = self.N = n
            self._U = self._e = self._lmax = None

        def compute_fourier_basis(self, n_eigenvectors=None):
            original_calls.append((self.N, n_eigenvectors))

        @property
        def U(self):
            return self._U

        def _get_upper_bound(self):
            return 2.0

    mod = types.ModuleType("pygsp")
    mod.filters = types.ModuleType("pygsp.filters")
    mod.filters.approximations = types.ModuleType("pygsp.filters.approximations")
    mod.filters.approximations.cheby_op = lambda *a: None
    mod.graphs = types.ModuleType("pygsp.graphs")
    mod.graphs.Graph = Graph
    orig = Graph.compute_fourier_basis
    full_calls, partial_calls = [], []
    big = plugin.FULL_BASIS_MIN_VERTICES
    assert big >= 1024

    def device_full_basis(dev, **kw):
        full_calls.append((dev, kw))
        n = big
        return np.arange(n, dtype=float) * 1e-7, np.eye(n), types.SimpleNamespace(buf=object()), {}

    def device_partial_basis(dev, k, b, **kw):
        partial_calls.append(k)
        buf = types.SimpleNamespace(free=int)
        return np.arange(k, dtype=float), np.ones((4096, k)), types.SimpleNamespace(buf=buf), {}

    monkeypatch.setattr(fourier, "device_full_basis", device_full_basis)
    monkeypatch.setattr(fourier, "device_partial_basis", device_partial_basis)
    dev = ("dev", np.dtype(np.float64))
    monkeypatch.setattr(plugin, "device_graph_for", lambda G, ctx=None, dtype=None: dev)
    with pytest.raises(ValueError, match="full_basis=True needs fourier=True"):
        plugin.install(mod, full_basis=True)
    assert Graph.compute_fourier_basis is orig
    try:
        plugin.install(mod, fourier=True, full_basis=True)
        G = Graph(big)
        G.compute_fourier_basis()
        assert full_calls == [(dev, {})]
        assert G._U.shape == (big, big) and G._e[0] == 0 and G._lmax == G._e[-1] and G._lmax_method == "fourier"
        held = G.__dict__["_gspx_basis"]
        assert held[0] is G._U and held[1] is dev
        assert plugin.basis_on_device_for(G) == (dev, held[2])  # the exact path finds the solver's panel
        G.compute_fourier_basis(n_eigenvectors=big)  # cached
        assert len(full_calls) == 1 and original_calls == []
        Graph(big - 1).compute_fourier_basis()        # below the threshold: the original
        Graph(4096).compute_fourier_basis(16)         # partial: the partial solver, as fourier=True alone
        Graph(100).compute_fourier_basis(10)          # small and partial: the original
        assert original_calls == [(big - 1, None), (100, 10)] and partial_calls == [16] and len(full_calls) == 1
        plugin.install(mod, fourier=True)             # full_basis off again: full requests are the original's
        Graph(big).compute_fourier_basis()
        assert original_calls[-1] == (big, None) and len(full_calls) == 1
    finally:
        plugin.uninstall(mod)
    assert Graph.compute_fourier_basis is orig and "_gspx_saved" not in Graph.__dict__
