"""Partial Fourier bases without a GPU: the subspace iteration of pygsp_amd.fourier on a numpy backend against dense
eigh, the filter's program rows against Chebyshev polynomials on scalars, the Graph-level rules (caching, signs,
e[0], gft / igft) with the device solver replaced by the numpy one, the plugin seam on a pygsp-shaped stand-in, and
the argument errors of the four panel entry points."""
import ctypes
import types

import numpy as np
import pytest
from scipy import sparse

from fourier_helpers import (NumpyBackend, check_against_dense, grid, laplacian, path, ring, three_components,
                             upper_bound)
from oracle import knn_oracle as knn
from pygsp_amd import _capi, fourier, graphs, plugin

GRAPHS = {
    "ring": (lambda: ring(64), 9),
    "path": (lambda: path(80), 10),
    "sensor300": (lambda: sparse.csr_matrix(knn.knn_weights(knn.sensor_coords(300, seed=1), 6)[0]), 12),
    "three_components": (three_components, 8),
}


@pytest.mark.parametrize("lap_type", ["combinatorial", "normalized"])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_solver_matches_dense_eigh(name, lap_type):
    make, k = GRAPHS[name]
    W = make()
    L, b = laplacian(W, lap_type), upper_bound(W, lap_type)
    e, X, stats = fourier.solve(NumpyBackend(L, b), k, b, tol=1e-10)
    U = X[:, :k]
    assert np.all(np.diff(e) >= 0)
    assert stats["worst_residual"] <= 1e-10 * b
    assert np.all(np.linalg.norm(L @ U - U * e, axis=0) <= 1e-10 * b * (1 + 1e-6))
    check_against_dense(L, b, e, U)
    if name == "three_components":
        assert np.all(np.abs(e[:3]) <= 1e-10 * b) and e[3] > 1e-3


@pytest.mark.parametrize("name", ["grid30", "two_grids_and_a_ring"])
def test_every_returned_residual_meets_the_tolerance(name):
    """Close Ritz values: Rayleigh-Ritz mixes locked columns with unconverged neighbours, so a column that met the
    tolerance can lose it again.  The solver returns only when all k residuals are under tol * b at the same time."""
    if name == "grid30":
        W, k = grid(30), 9
    else:
        W, k = sparse.csr_matrix(sparse.block_diag([grid(20), grid(20) * (1 + 1e-6), ring(60)])), 16
    L, b = laplacian(W, "combinatorial"), upper_bound(W, "combinatorial")
    for seed in range(4):
        e, X, stats = fourier.solve(NumpyBackend(L, b), k, b, seed=seed)
        U = X[:, :k]
        assert stats["worst_residual"] <= 1e-10 * b
        assert np.all(np.linalg.norm(L @ U - U * e, axis=0) <= 1e-10 * b * (1 + 1e-6)), seed
        check_against_dense(L, b, e, U)


def test_solver_is_seeded():
    W = ring(64)
    L, b = laplacian(W, "combinatorial"), 4.0
    e1, X1, _ = fourier.solve(NumpyBackend(L, b), 6, b, seed=3)
    e2, X2, _ = fourier.solve(NumpyBackend(L, b), 6, b, seed=3)
    assert np.array_equal(e1, e2) and np.array_equal(X1, X2)


def test_solver_raises_when_maxiter_runs_out():
    W = sparse.csr_matrix(knn.knn_weights(knn.sensor_coords(300, seed=1), 6)[0])
    L, b = laplacian(W, "combinatorial"), upper_bound(W, "combinatorial")
    with pytest.raises(ValueError, match="worst residual"):
        fourier.solve(NumpyBackend(L, b), 12, b, maxiter=1, degree=(2, 2))


def test_block_width():
    assert fourier.block_width(1) == 16 and fourier.block_width(8) == 16 and fourier.block_width(9) == 32
    assert fourier.block_width(16) == 32 and fourier.block_width(64) == 80 and fourier.block_width(32) == 48
    for k in range(1, 400):
        p = fourier.block_width(k)
        assert p - k >= max(8, -(-k // 4)) and p % fourier.BLOCK_QUANTUM == 0
    assert fourier.block_width(409) == 512 and fourier.block_width(410) > 512
    assert fourier.block_width(10, n_vertices=20) == 20
    assert fourier.use_device(100000, 64) and fourier.use_device(100000, 409) and not fourier.use_device(100000, 410)
    assert not fourier.use_device(2047, 4) and not fourier.use_device(4096, 1000)


@pytest.mark.parametrize("m", [1, 2, 3, 7, 30, 120])
def test_program_rows_are_the_scaled_chebyshev_filter(m):
    """The (scale, beta, gamma) rows, run through the program recurrence on a scalar 'Laplacian' lam, give
    C_m(t(lam)) / C_m(t(a0)), t(x) = (x - c) / e, c = (a + b) / 2, e = (b - a) / 2."""
    a0, a, b = 0.05, 0.6, 2.0
    prog = fourier.filter_program(a0, a, b, m)
    assert prog.shape == (m, 3)
    c, e = (a + b) / 2, (b - a) / 2
    cheb = lambda t: np.polynomial.chebyshev.chebval(t, [0] * m + [1])
    for lam in np.linspace(0, b, 41):
        old = cur = 1.0
        for s, (sc, be, ga) in enumerate(prog):
            new = sc * (2 * ((2 / b) * lam - 1)) * cur + be * cur + (ga * old if s else 0.0)
            old, cur = cur, new
        ref = cheb((lam - c) / e) / cheb((a0 - c) / e)
        assert abs(cur - ref) <= 1e-12 * max(1.0, abs(ref)), (lam, cur, ref)
    # the issue's closed forms of the first rows
    sg = fourier.sigmas(a0, a, b, m)
    assert np.isclose(prog[0, 0], sg[0] * b / (4 * e)) and np.isclose(prog[0, 1], sg[0] * (b / 2 - c) / e)
    if m > 1:
        assert np.isclose(prog[1, 2], -sg[0] * sg[1]) and np.isclose(prog[1, 0], sg[1] * b / (2 * e))


def test_degree_choice_within_bounds():
    theta = np.array([0.0, 0.01, 0.02, 0.5, 1.0])
    resid = np.array([1e-3, 1e-3, 1e-3, 1e-3, 1e-3])
    m = fourier.choose_degree(theta, resid, [1, 2], 1.0, 2.0, 1e-10, (10, 300))
    assert 10 <= m <= 300
    assert fourier.choose_degree(theta, resid, [1, 2], 1.0, 2.0, 1e-10, (10, 12)) <= 12
    assert fourier.choose_degree(theta, resid, [], 1.0, 2.0, 1e-10, (7, 300)) == 7


def test_sign_rule_and_e0():
    U = np.array([[0.1, -0.5, 0.3], [-0.9, 0.5, -0.3], [0.2, 0.1, 0.0]])
    e = np.array([3e-7, 0.5, 1.0])
    s = fourier.finish_partial(e, U)
    assert e[0] == 0 and list(s) == [-1, -1, 1]
    assert U[1, 0] == 0.9 and U[0, 1] == 0.5 and U[0, 2] == 0.3  # ties: the lowest index decides
    with pytest.raises(ValueError):
        fourier.finish_partial(np.array([2e-5, 1.0]), np.eye(2))


# ---- Graph-level rules, the device solver replaced by the numpy one ------------------------------------------------
def _host_graph(monkeypatch, W, lap_type="combinatorial"):
    """A graphs.Graph whose device calls are stand-ins: L on the host, the solver on the numpy backend."""
    monkeypatch.setattr(graphs.Graph, "_setup_on_device", lambda self, adj: False)
    monkeypatch.setattr(graphs.Graph, "compute_laplacian", lambda self, lap_type="combinatorial": None)
    G = graphs.Graph(W, lap_type=lap_type, reorder="none", tiles=False)
    G._L = laplacian(W, lap_type)
    monkeypatch.setattr(graphs.Graph, "_get_upper_bound", lambda self: upper_bound(self.W, self.lap_type))
    calls = []

    def device_partial_basis(dev, k, b, **kw):
        calls.append((k, kw))
        e, X, stats = fourier.solve(NumpyBackend(G._L, b), k, b, **kw)
        U = np.array(X[:, :k])
        fourier.finish_partial(e, U)
        return e, U, types.SimpleNamespace(buf=None), stats

    monkeypatch.setattr(fourier, "device_partial_basis", device_partial_basis)
    monkeypatch.setattr(graphs.Graph, "device_graph", lambda self, dtype=None: None)
    return G, calls


def test_partial_basis_routing_and_caching(monkeypatch):
    W = sparse.csr_matrix(knn.knn_weights(knn.sensor_coords(300, seed=1), 6)[0])
    G, calls = _host_graph(monkeypatch, W)
    G.compute_fourier_basis(n_eigenvectors=10, method="device")
    assert len(calls) == 1 and G.U.shape == (300, 10) and G.e.shape == (10,) and G._lmax is None
    assert G.e[0] == 0 and np.all(np.diff(G.e) >= 0)
    idx = np.argmax(np.abs(G.U), axis=0)
    assert np.all(G.U[idx, np.arange(10)] > 0)
    lam, V = np.linalg.eigh(G._L.toarray())
    assert np.allclose(G.e, np.r_[0, lam[1:10]], atol=1e-9)
    # a cached basis of at least k vectors is kept, whatever the method
    G.compute_fourier_basis(n_eigenvectors=4)
    G.compute_fourier_basis(n_eigenvectors=10, method="dense")
    assert len(calls) == 1 and G.U.shape == (300, 10)
    # a larger request recomputes; 'auto' on a 300-vertex graph is the dense branch
    G.compute_fourier_basis(n_eigenvectors=12)
    assert len(calls) == 1 and G.U.shape == (300, 12) and G._lmax is None
    assert np.allclose(G.e, np.r_[0, lam[1:12]], atol=1e-12)
    idx = np.argmax(np.abs(G.U), axis=0)
    assert np.all(G.U[idx, np.arange(12)] > 0)
    # the full basis keeps today's behaviour: lmax from the spectrum
    G.compute_fourier_basis()
    assert G.U.shape == (300, 300) and G._lmax_method == "fourier" and G._lmax == G.e[-1]
    G._forget_spectrum()
    assert G._U is None and G._e is None and G._U_dev is None
    with pytest.raises(ValueError):
        G.compute_fourier_basis(n_eigenvectors=0)
    with pytest.raises(ValueError):
        G.compute_fourier_basis(n_eigenvectors=5, method="arpack")


def test_auto_sends_large_graphs_to_the_device(monkeypatch):
    W = ring(4096)
    G, calls = _host_graph(monkeypatch, W)
    G.compute_fourier_basis(n_eigenvectors=4, tol=1e-8, seed=5)
    assert [c[0] for c in calls] == [4] and calls[0][1]["seed"] == 5 and calls[0][1]["tol"] == 1e-8
    assert G.U.shape == (4096, 4) and G.e[0] == 0


def test_gft_igft_host(monkeypatch):
    W = sparse.csr_matrix(knn.knn_weights(knn.sensor_coords(60, seed=2), 5)[0])
    G, _ = _host_graph(monkeypatch, W)
    G.compute_fourier_basis()
    rng = np.random.default_rng(0)
    for shape in [(60,), (60, 5), (60, 5, 3)]:
        s = rng.standard_normal(shape)
        s_hat = G.gft(s)
        assert s_hat.shape == shape
        assert np.array_equal(s_hat, np.tensordot(np.conjugate(G.U), s, ([0], [0])))
        assert np.max(np.abs(G.igft(s_hat) - s)) < 1e-10  # the round trip of fourier.py:218-223
        assert np.array_equal(G.igft(s), np.tensordot(G.U, s, ([1], [0])))
    with pytest.raises(ValueError):
        G.gft(np.zeros(59))
    # a partial basis: coefficients (k, ...) and back
    G._forget_spectrum()
    G.compute_fourier_basis(n_eigenvectors=7, method="dense")
    s = rng.standard_normal((60, 4))
    assert G.gft(s).shape == (7, 4) and G.igft(G.gft(s)).shape == (60, 4)
    with pytest.raises(ValueError):
        G.igft(np.zeros((60, 4)))


def test_plugin_routes_partial_requests(monkeypatch):
    """install(fourier=True) on a pygsp-shaped stand-in: partial requests that 'auto' sends to the device go to the
    device solver and land in _e / _U, everything else calls the saved original; uninstall restores it."""
    original_calls = []

    class Graph:
        def __init__(self, n):
            self.n_vertices = self.N = n
            self._U = self._e = None

        def compute_fourier_basis(self, n_eigenvectors=None):
            original_calls.append(n_eigenvectors)

        def estimate_lmax(self, method="lanczos"):
            return "reference"

        def _get_upper_bound(self):
            return 2.0

    mod = types.ModuleType("pygsp")
    mod.filters = types.ModuleType("pygsp.filters")
    mod.filters.approximations = types.ModuleType("pygsp.filters.approximations")
    mod.filters.approximations.cheby_op = lambda *a: None
    mod.graphs = types.ModuleType("pygsp.graphs")
    mod.graphs.Graph = Graph
    orig = Graph.compute_fourier_basis
    device_calls = []

    class Buf:
        def free(self):
            device_calls.append("freed")

    def device_partial_basis(dev, k, b, **kw):
        device_calls.append((dev, k, b))
        return np.arange(k, dtype=float), np.ones((4096, k)), types.SimpleNamespace(buf=Buf()), {}

    monkeypatch.setattr(fourier, "device_partial_basis", device_partial_basis)
    monkeypatch.setattr(plugin, "device_graph_for", lambda G, ctx=None, dtype=None: ("dev", np.dtype(dtype)))
    try:
        plugin.install(mod, fourier=False)
        assert Graph.compute_fourier_basis is orig
        plugin.install(mod, fourier=True, lmax="device")
        G = Graph(4096)
        G.compute_fourier_basis(n_eigenvectors=16)
        assert device_calls[0] == (("dev", np.dtype(np.float64)), 16, 2.0) and G._U.shape == (4096, 16)
        G.compute_fourier_basis(n_eigenvectors=8)  # cached
        assert len([c for c in device_calls if c != "freed"]) == 1
        G.compute_fourier_basis()  # full: the original
        G.compute_fourier_basis(n_eigenvectors=4096)
        Graph(100).compute_fourier_basis(n_eigenvectors=10)  # small graph: the original
        Graph(4096).compute_fourier_basis(n_eigenvectors=2000)  # block wider than N / 4: the original
        assert original_calls == [None, 4096, 10, 2000]
        assert Graph.estimate_lmax is plugin._estimate_lmax_on_device
        plugin.install(mod, fourier=True)  # lmax back to the reference, fourier kept
        assert Graph.estimate_lmax(G) == "reference" and Graph.compute_fourier_basis is not orig
    finally:
        plugin.uninstall(mod)
    assert Graph.compute_fourier_basis is orig and "_gspx_saved" not in Graph.__dict__


def test_panel_entry_points_refuse_bad_arguments_without_a_device():
    lib = _capi.load()
    c = np.zeros((4, 4))
    q = np.eye(4)
    t = np.zeros(4)
    fake = ctypes.c_void_p(1 << 20)  # a non-null panel address: never dereferenced, the checks fail first

    def refused(rc, words):
        with pytest.raises(ValueError):
            _capi.check(rc)
        assert words in _capi.last_error(), _capi.last_error()

    gram, comb, res = lib.gspx_panel_gram_dev, lib.gspx_panel_combine_dev, lib.gspx_panel_residual_norms_dev
    # null context, everything else valid
    refused(gram(None, 10, fake, 4, 4, fake, 4, 4, _capi.ptr(c), None), "null context")
    refused(comb(None, 10, fake, 4, 4, _capi.ptr(q), 4, ctypes.c_void_p(1 << 30), 4, None), "null context")
    refused(res(None, 10, fake, fake, 4, 4, _capi.ptr(t), _capi.ptr(t), None), "null context")
    # widths out of range
    for na, nb in ((0, 4), (4, 0), (513, 4), (4, 513)):
        refused(gram(None, 10, fake, 600, na, fake, 600, nb, _capi.ptr(c), None), "widths")
        refused(comb(None, 10, fake, 600, na, _capi.ptr(q), nb, ctypes.c_void_p(1 << 30), 600, None), "widths")
    refused(res(None, 10, fake, fake, 600, 0, _capi.ptr(t), _capi.ptr(t), None), "width")
    refused(res(None, 10, fake, fake, 600, 513, _capi.ptr(t), _capi.ptr(t), None), "width")
    # leading dimensions, negative N, null pointers
    refused(gram(None, 10, fake, 3, 4, fake, 4, 4, _capi.ptr(c), None), "leading dimension")
    refused(comb(None, 10, fake, 4, 4, _capi.ptr(q), 4, ctypes.c_void_p(1 << 30), 3, None), "leading dimension")
    refused(res(None, 10, fake, fake, 3, 4, _capi.ptr(t), _capi.ptr(t), None), "leading dimension")
    refused(gram(None, -1, fake, 4, 4, fake, 4, 4, _capi.ptr(c), None), "negative")
    refused(gram(None, 10, None, 4, 4, fake, 4, 4, _capi.ptr(c), None), "null panel")
    refused(gram(None, 10, fake, 4, 4, fake, 4, 4, None, None), "null output")
    refused(comb(None, 10, fake, 4, 4, None, 4, ctypes.c_void_p(1 << 30), 4, None), "null Q")
    refused(comb(None, 10, fake, 4, 4, _capi.ptr(q), 4, None, 4, None), "null panel")
    refused(res(None, 10, fake, None, 4, 4, _capi.ptr(t), _capi.ptr(t), None), "null panel")
    refused(res(None, 10, fake, fake, 4, 4, None, _capi.ptr(t), None), "null theta")
    cp = lib.gspx_panel_copy_dev
    refused(cp(None, 10, fake, 4, 4, ctypes.c_void_p(1 << 30), 4, None), "null context")
    refused(cp(None, 10, fake, 600, 0, ctypes.c_void_p(1 << 30), 600, None), "width")
    refused(cp(None, 10, fake, 600, 513, ctypes.c_void_p(1 << 30), 600, None), "width")
    refused(cp(None, 10, fake, 3, 4, ctypes.c_void_p(1 << 30), 4, None), "leading dimension")
    refused(cp(None, -1, fake, 4, 4, ctypes.c_void_p(1 << 30), 4, None), "negative")
    refused(cp(None, 10, fake, 4, 4, None, 4, None), "null panel")
    refused(cp(None, 10, fake, 8, 4, ctypes.c_void_p((1 << 20) + 32), 8, None), "alias")
    # Y overlapping X: the same address, and a column view inside X's rows
    refused(comb(None, 10, fake, 4, 4, _capi.ptr(q), 4, fake, 4, None), "alias")
    refused(comb(None, 10, fake, 8, 4, _capi.ptr(q), 4, ctypes.c_void_p((1 << 20) + 32), 8, None), "alias")
