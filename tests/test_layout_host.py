"""The spring layout, the parts that need no GPU: the numpy restatement of tests/layout_helpers.py against the goldens
of the real reference, the measurement the device tolerances rest on, the condition on the inputs that keeps the two
branches of the iteration away from their thresholds, the host bookkeeping of pygsp_amd.layout around the iterations,
every refusal, and the plugin's layout row.

Measured (printed by the tests below; also in profiles/layout.md): fp64 in a permuted, chunked order against longdouble
differ by at most 6.7e-16 over the 150 teacher-forced steps and one free iteration, and by at most 4.8e-15 after five
free iterations - within SPREAD_STEP = 1.2e-15 and SPREAD_FIVE = 5.4e-14 of layout_helpers."""
import ctypes
import logging
import types

import numpy as np
import pytest
from scipy import sparse

import layout_helpers as lh
from pygsp_amd import _capi, graphs, layout, plugin


@pytest.mark.parametrize("name", lh.MAIN + lh.EDGE)
def test_restatement_equals_the_reference_after_one_and_five_iterations(name):
    c = lh.case(name)
    for mode in ("reference", "permuted"):
        one = lh.run(c.A, c.pos0, c.k, 1, fixed=c.fixed, mode=mode)[-1]
        five = lh.run(c.A, c.pos0, c.k, 5, fixed=c.fixed, mode=mode)[-1]
        print("%s %s: after 1 %.2e, after 5 %.2e" % (name, mode, lh.dev(one, c.pos1), lh.dev(five, c.pos5)))
        assert lh.dev(one, c.pos1) <= lh.SPREAD_STEP and lh.dev(five, c.pos5) <= lh.SPREAD_FIVE
        if c.fixed:
            assert one[c.fixed].tobytes() == c.pos0[c.fixed].tobytes() == c.pos5[c.fixed].tobytes()
    if name in ("single", "coincident"):  # nothing moves: one vertex; two vertices on one point
        assert np.array_equal(c.pos1, c.pos0) and np.array_equal(c.pos5, c.pos0)
    if name == "ring257":  # the isolated vertices are only repelled: they move
        assert not c.A[257:].any() and (np.abs(c.pos1[257:] - c.pos0[257:]).max(axis=1) > 0).all()


@pytest.mark.parametrize("name", lh.MAIN)
def test_every_teacher_forced_step_and_the_condition_on_the_inputs(name):
    """From the reference's own positions before each of the 50 iterations the restatement lands on the reference's
    next positions; on the way no pair distance and no displacement length comes near 0.01 (1e-6, relative: measured
    1.7e-4 and 2.2e-2), so a summation order cannot flip a branch - while the short-displacement branch IS taken and
    clamped pairs DO occur."""
    c = lh.case(name)
    assert c.traj.shape == (lh.RUN + 1, c.N, c.dim) and np.array_equal(c.traj[0], c.pos0)
    info, worst = {}, {"reference": 0.0, "permuted": 0.0}
    for i, t in enumerate(lh.temperatures(lh.RUN)):
        for mode in worst:
            out = lh.step(c.A, c.traj[i], c.k, t, c.fixed, mode, info if mode == "reference" else None)
            worst[mode] = max(worst[mode], lh.dev(out, c.traj[i + 1]))
    print("%s: teacher-forced %s, %s" % (name, worst, info))
    assert max(worst.values()) <= lh.SPREAD_STEP
    assert info["pair_gap"] > 1e-6 and info["len_gap"] > 1e-6
    assert info["short"] >= 1 and info["clamped"] >= 1


def test_the_subclamp_pair_exists():
    c = lh.case("subclamp")
    assert abs(np.linalg.norm(c.pos0[0] - c.pos0[1]) - 0.003) < 1e-12 and c.A[0, 1] == 1
    info = {}
    lh.step(c.A, c.pos0, c.k, lh.T0, info=info)
    assert info["clamped"] == 2 and info["pair_gap"] > 1e-6


def test_the_spread_the_device_tolerances_rest_on():
    """fp64 summed in a permuted, chunked order against longdouble, over every step of every case: the yardstick.
    The device gets MARGIN times these constants (layout_helpers)."""
    step = five = 0.0
    for name in lh.MAIN + lh.EDGE:
        c = lh.case(name)
        runs = {m: lh.run(c.A, c.pos0, c.k, 5, fixed=c.fixed, mode=m) for m in ("permuted", "longdouble")}
        step = max(step, lh.dev(runs["permuted"][0], runs["longdouble"][0]))
        five = max(five, lh.dev(runs["permuted"][-1], runs["longdouble"][-1]))
        if c.traj is not None:
            for i, t in enumerate(lh.temperatures(lh.RUN)):
                a, b = (lh.step(c.A, c.traj[i], c.k, t, c.fixed, m) for m in ("permuted", "longdouble"))
                step = max(step, lh.dev(a, b))
    print("spread of one step %.2e (SPREAD_STEP %.2e), of five iterations %.2e (SPREAD_FIVE %.2e)" % (
        step, lh.SPREAD_STEP, five, lh.SPREAD_FIVE))
    assert 0 < step <= lh.SPREAD_STEP and 0 < five <= lh.SPREAD_FIVE
    assert (lh.SPREAD_STEP, lh.SPREAD_FIVE, lh.MARGIN) == (1.2e-15, 5.4e-14, 100)
    assert lh.DEV_STEP_TOL == 100 * 1.2e-15 and lh.DEV_FIVE_TOL == 100 * 5.4e-14


def _standin_graph(W, directed=False):
    """A pygsp_amd.graphs.Graph that never touches a device: what set_coordinates and the routes read."""
    G = graphs.Graph.__new__(graphs.Graph)
    G.logger = logging.getLogger("test_layout_host")
    G._adj_host, G._adj_dev, G._flags = sparse.csr_matrix(W), None, {"directed": directed}
    G.n_vertices = G.N = G._adj_host.shape[0]
    return G


def test_the_wrapper_bookkeeping_against_the_complete_goldens():
    """seed -> start positions, k, cooling, then mean-then-lim rescaling and the centre, around the restatement's
    iterations.  The rescaling multiplies by scale / lim and subtracts a mean: 4 scale / lim times the spread of five
    iterations (lim from the restatement's own positions)."""
    c, npz = lh.case("sensor64"), lh.golden()
    G = _standin_graph(c.W)
    start = np.random.default_rng(3).uniform(size=(c.N, 2))
    raw = lh.run(c.A, start, np.sqrt(1.0 / c.N), 5)[-1]
    lim = max(0, *(raw - raw.mean(axis=0)).max(axis=0))
    for key, kwargs, scale in (("full_a", {}, 1.0), ("full_b", {"scale": 2, "center": [[1, -1]]}, 2.0)):
        got, report = layout.fruchterman_reingold(G, lh.iterate(c.A), seed=3, iterations=5, **kwargs)
        d = lh.dev(got, npz[key])
        print("%s: deviation %.2e, bound %.2e" % (key, d, 4 * scale / lim * lh.SPREAD_FIVE))
        assert report == {"iterations": 5} and got.shape == npz[key].shape and d <= 4 * scale / lim * lh.SPREAD_FIVE
    a, b = npz["full_a"], npz["full_b"]
    assert abs(a.mean(axis=0)).max() <= 1e-12 and a.max() == 1.0
    assert abs((b - [1, -1]).mean(axis=0)).max() <= 1e-12 and abs((b - [1, -1]).max() - 2.0) <= 1e-15
    # a centre of the wrong size is reported and replaced by the origin (_layout.py:139-141)
    got = layout.fruchterman_reingold(G, lh.iterate(c.A), seed=3, iterations=5, center=[[1, 2, 3]]).coords
    assert lh.dev(got, a) <= 4 / lim * lh.SPREAD_FIVE
    # fixed vertices and user positions: k = dom_size / sqrt(N), no rescaling (the case fixed300)
    f = lh.case("fixed300")
    got = layout.fruchterman_reingold(_standin_graph(f.W), lh.iterate(f.A), pos=f.pos0, fixed=f.fixed, iterations=5,
                                      seed=5).coords
    assert lh.dev(got, f.pos5) <= lh.SPREAD_FIVE and got[f.fixed].tobytes() == f.pos0[f.fixed].tobytes()


def test_rescale_layout_keeps_the_mean_then_lim_statement_order():
    """lim is the largest SIGNED coordinate, taken axis by axis right after that axis lost its mean, from 0."""
    pos = np.array([[0.0, 5.0], [1.0, 5.5], [5.0, 9.0]])
    want = pos - pos.mean(axis=0)
    want *= 3.0 / want.max()
    assert np.array_equal(layout.rescale_layout(pos.copy(), scale=3.0), want)
    lopsided = np.array([[-9.0], [1.0], [2.0]])  # the largest coordinate, not the largest magnitude
    assert layout.rescale_layout(lopsided.copy()).max() == 1.0 and layout.rescale_layout(lopsided.copy()).min() < -1.0


def test_the_host_kinds_bit_for_bit():
    G = _standin_graph(sparse.csr_matrix((7, 7)))
    G.set_coordinates("line1D")
    assert np.array_equal(G.coords, np.arange(7))
    G.set_coordinates("line2D")
    assert np.array_equal(G.coords, np.stack([np.arange(7), np.zeros(7)], axis=1))
    G.set_coordinates("ring2D")
    angle = np.arange(7) * 2 * np.pi / 7
    assert G.coords.tobytes() == np.stack([np.cos(angle), np.sin(angle)], axis=1).tobytes()
    for kind, dim in (("random2D", 2), ("random3D", 3)):
        G.set_coordinates(kind, seed=11)
        assert G.coords.tobytes() == np.random.default_rng(11).uniform(size=(7, dim)).tobytes()
    for given in (np.arange(7.0), np.ones((7, 2)), np.ones((7, 3)), np.ones((7, 1, 3))):
        G.set_coordinates(given)
        assert np.array_equal(G.coords, np.asarray(given).squeeze())
    # the eigenmap kinds: columns 1..2 / 1..3 of a basis of 3 / 4 vectors
    asked = []
    G.compute_fourier_basis = lambda n_eigenvectors: asked.append(n_eigenvectors)
    G._U = np.arange(35.0).reshape(7, 5)
    G.set_coordinates("laplacian_eigenmap2D")
    assert np.array_equal(G.coords, G._U[:, 1:3])
    G.set_coordinates("laplacian_eigenmap3D")
    assert np.array_equal(G.coords, G._U[:, 1:4]) and asked == [3, 4]


def test_every_refusal():
    W = sparse.csr_matrix(np.array([[0., 1., 0.], [1., 0., 2.], [0., 2., 0.]]))
    G = _standin_graph(W)
    for bad in (np.ones((4, 2)), np.ones((3, 4)), np.ones((3, 2, 2)), np.ones((2,))):
        with pytest.raises(ValueError, match="Expecting coordinates to be of size N, Nx2, or Nx3."):
            G.set_coordinates(bad)
    with pytest.raises(ValueError, match="Unexpected argument kind=spiral."):
        G.set_coordinates("spiral")
    with pytest.raises(NotImplementedError, match="community2D"):
        G.set_coordinates("community2D")
    # the routes that stay off the device: never a device call (there is none here), never a silent fallback
    with pytest.raises(NotImplementedError, match="2 and 3 dimensions"):
        G.set_coordinates("spring", dim=4)
    with pytest.raises(NotImplementedError, match="undirected"):
        _standin_graph(sparse.csr_matrix(np.array([[0., 1.], [0., 0.]])), directed=True).set_coordinates()
    with pytest.raises(NotImplementedError, match="negative weights"):
        _standin_graph(sparse.csr_matrix(np.array([[0., -1.], [-1., 0.]])))._fruchterman_reingold()
    reported = _standin_graph(W)
    reported.setup_report = {"negative": 1}  # the device set-up counted them: W is not read again
    assert "negative" in layout.device_route(reported, 2) and layout.device_route(G, 3) is None
    # the library refuses a null graph before any device work
    ms = ctypes.c_double(0)
    with pytest.raises(ValueError, match="null graph"):
        _capi.check(_capi.load().gspx_layout_spring_dev(None, 2, 1.0, None, 1, 0.1, 0.05, None, ctypes.byref(ms)))
    n = ctypes.c_int64(0)
    with pytest.raises(ValueError):
        _capi.check(_capi.load().gspx_layout_splits(None, ctypes.byref(n)))


def test_capi_prototypes():
    P, D = ctypes.c_void_p, ctypes.c_double
    assert _capi.SIGNATURES["gspx_layout_spring_dev"] == (
        ctypes.c_int, [P, ctypes.c_int, D, P, ctypes.c_int64, D, D, P, ctypes.POINTER(D)])
    assert _capi.SIGNATURES["gspx_layout_splits"] == (ctypes.c_int, [P, ctypes.POINTER(ctypes.c_int64)])


def test_the_eigenvalue_gaps_the_eigenmap_test_relies_on():
    """Sensor(123, seed=42): eigenvalues 0 .. 4 of L are separated by more than 1e-3, so the eigenvectors 1 .. 3 are
    determined up to sign to about 1e-10 / 1e-3 of the solver's residual (tests/test_gpu_k_layout.py)."""
    W = graphs.sensor_weights(123, seed=42, return_coords=False)
    L = sparse.diags(np.asarray(W.sum(axis=1)).ravel()) - W
    e = np.linalg.eigvalsh(L.toarray())
    print("eigenvalues 0..4: %s" % e[:5])
    assert (np.diff(e[:5]) > 1e-3).all()


def _standin_module():
    class Graph:
        N = 3

        def _fruchterman_reingold(self, dim=2, k=None, pos=None, fixed=[], iterations=50, scale=1.0, center=None,
                                  seed=None):
            return ("ref spring", dim, iterations)

        def is_connected(self):
            return "ref connected"

    mod = types.ModuleType("pygsp")
    mod.graphs = types.ModuleType("pygsp.graphs")
    mod.graphs.Graph = Graph
    mod.filters = types.ModuleType("pygsp.filters")
    mod.filters.approximations = types.ModuleType("pygsp.filters.approximations")
    mod.filters.approximations.cheby_op = mod.filters.cheby_op = lambda *a, **k: "ref cheby"
    return mod


def test_plugin_layout_row_is_opt_in_and_restored():
    mod = _standin_module()
    Graph = mod.graphs.Graph
    own = (Graph._fruchterman_reingold, Graph.is_connected)
    assert plugin._LAYOUT == ("_fruchterman_reingold",)
    try:
        plugin.install(mod)
        assert (Graph._fruchterman_reingold, Graph.is_connected) == own
        plugin.install(mod, layout=True)
        assert Graph._fruchterman_reingold is plugin._fruchterman_reingold_on_device and Graph.is_connected is own[1]
        assert set(vars(Graph)[plugin._SAVED]) == set(plugin._LAYOUT)
        plugin.install(mod, layout=True)  # again: the saved original is still the package's own
        assert vars(Graph)[plugin._SAVED]["_fruchterman_reingold"] is own[0]
        # a directed graph, negative weights, four dimensions and a graph without vertices reach the original
        g = Graph()
        g.is_directed = lambda: True
        assert g._fruchterman_reingold(iterations=7) == ("ref spring", 2, 7)
        g.is_directed, g.W = (lambda: False), sparse.csr_matrix(np.array([[0., -1., 0.], [-1., 0., 0.], [0., 0., 0.]]))
        assert g._fruchterman_reingold() == ("ref spring", 2, 50)
        g.W = abs(g.W)
        assert g._fruchterman_reingold(dim=4) == ("ref spring", 4, 50)
        g.N = 0
        assert g._fruchterman_reingold(3) == ("ref spring", 3, 50)
        plugin.install(mod, topology=True)
        assert Graph._fruchterman_reingold is own[0] and Graph.is_connected is not own[1]
        plugin.install(mod, layout=True)
    finally:
        plugin.uninstall(mod)
    assert (Graph._fruchterman_reingold, Graph.is_connected) == own and not hasattr(Graph, plugin._SAVED)
    bare = _standin_module()
    del bare.graphs
    with pytest.raises(ValueError, match="layout=True"):
        plugin.install(bare, layout=True)
    plugin.uninstall(bare)


@pytest.mark.skipif(_capi.device_count() > 0, reason="checks the no-device behaviour")
def test_layout_fails_loudly_without_device():
    """No CPU fallback: without a HIP device the spring layout raises, it does not quietly run numpy."""
    c = lh.case("sensor64")
    with pytest.raises(_capi.GspxError):
        graphs.Graph(c.W).set_coordinates()
