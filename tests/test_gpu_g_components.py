"""Connected components on the device (gspx_graph_components; Graph.connected_components / is_connected /
extract_components / subgraph): against what the real reference recorded (tests/golden/components.npz) and against
scipy.sparse.csgraph.connected_components on W.  Labels are numbered by smallest vertex on both sides, so every
comparison is integer or sparse-matrix equality.  `-m gpu`."""
import ctypes
import types

import numpy as np
import pytest
from scipy import sparse
from scipy.sparse import csgraph

from conftest import csr_from, load_golden
from gpu_helpers import ctx, random_graph  # noqa: F401 (ctx is a fixture)
from oracle import cheby_oracle as orc
from pygsp_amd import _capi, engine, graphs, plugin

pytestmark = pytest.mark.gpu


def _same_csr(A, B):
    A, B = sparse.csr_matrix(A), sparse.csr_matrix(B)
    A.sort_indices()
    B.sort_indices()
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(A.data, B.data))


def _scipy_labels(W):
    n, labels = csgraph.connected_components(W, directed=False)
    return int(n), labels.astype(np.int32)


def _round_cap(N):
    cap = ctypes.c_int(0)
    _capi.check(_capi.load().gspx_components_round_cap(N, ctypes.byref(cap)))
    return cap.value


def _check_against_scipy(G, W):
    n_ref, ref = _scipy_labels(W)
    n, labels = G.connected_components()
    assert labels.dtype == np.int32 and labels.shape == (W.shape[0],)
    assert n == n_ref and np.array_equal(labels, ref)
    assert G.is_connected() == (n_ref == 1)
    report = G.components_report
    assert 1 <= report["rounds"] <= report["round_cap"] == _round_cap(W.shape[0])
    return report


@pytest.fixture(scope="module")
def golden():
    return load_golden("components.npz")


# ---- what the reference recorded ------------------------------------------------------------------------------
def test_golden_cases(golden):
    """Every recorded case: is_connected, the labels behind it, and the children of extract_components - vertex
    lists, adjacencies, coordinates - equal the reference's."""
    g = golden
    assert len(g["cases"]) >= 7
    for name in g["cases"]:
        W = csr_from(g, name + "_W")
        coords = g[name + "_coords"] if name + "_coords" in g else None
        G = graphs.Graph(W, coords=coords)
        assert G.is_directed() == bool(g[name + "_directed"]), name
        assert G.is_connected() == bool(g[name + "_connected"]), name
        if G.is_directed():
            with pytest.raises(NotImplementedError, match="Directed graphs not supported yet."):
                G.extract_components()
            continue
        n, labels = G.connected_components()
        assert n == int(g[name + "_n"]), name
        assert (n, labels.tolist()) == (_scipy_labels(W)[0], _scipy_labels(W)[1].tolist()), name
        parts = G.extract_components()
        assert len(parts) == n
        for i, part in enumerate(parts):
            key = "{}_k{}".format(name, i)
            assert isinstance(part.info["orig_idx"], list)
            assert np.array_equal(part.info["orig_idx"], g[key + "_idx"]), key
            assert np.all(labels[g[key + "_idx"]] == i), key
            assert _same_csr(part.W, csr_from(g, key + "_W")), key
            assert part.lap_type == G.lap_type and part.is_connected()
            if coords is not None:
                assert np.array_equal(part.coords, g[key + "_coords"]), key


def test_golden_subgraph(golden):
    """The doctest of Graph.subgraph (graph.py:234-244): vertices in the order given, signals sliced; a boolean
    indicator selects the same vertices in ascending order."""
    g = golden
    G = graphs.Graph(csr_from(g, "doctest_connected_W"), lap_type="normalized", compute_dtype=np.float32)
    G.signals["s"] = np.array([10., 11., 12., 13.])
    sub = G.subgraph([0, 2, 1])
    assert _same_csr(sub.W, csr_from(g, "doctest_subgraph_W"))
    assert np.array_equal(sub.W.toarray(), [[0., 0., 3.], [0., 0., 4.], [3., 4., 0.]])
    assert np.array_equal(sub.signals["s"], g["doctest_subgraph_signal"])
    assert sub.lap_type == "normalized" and sub.compute_dtype == np.float32 and not hasattr(sub, "coords")
    mask = G.subgraph(np.array([True, True, True, False]))
    assert _same_csr(mask.W, G.W[:3, :][:, :3]) and mask.N == 3
    assert G.is_weighted() and not G.has_loops()
    assert graphs.Graph(csr_from(g, "loops_only_W")).has_loops()
    assert not graphs.Graph(sparse.csr_matrix(np.array([[0, 1], [1, 0]]))).is_weighted()


# ---- against scipy on W ---------------------------------------------------------------------------------------
def _union_of_sensors(sizes, seed):
    parts = [graphs.sensor_weights(n, k=6, seed=seed + i) for i, n in enumerate(sizes)]
    W = sparse.block_diag([p[0] for p in parts], format="csr")
    coords = np.concatenate([p[1] + 2.0 * i for i, p in enumerate(parts)])
    order = np.random.default_rng(seed).permutation(W.shape[0])
    W = sparse.csr_matrix(W[order, :][:, order])
    W.sort_indices()
    return W, coords[order]


_cache = {}


def _differential_graph(name):
    if name not in _cache:
        if name == "logo":
            _cache[name] = (csr_from(load_golden("logo_heat50.npz"), "W"), None)
        elif name == "sensor123":
            g = load_golden("sensor123.npz")
            _cache[name] = (csr_from(g, "W"), g["coords"])
        elif name == "union50k":
            _cache[name] = _union_of_sensors([20000, 12000, 9000, 6000, 3000, 17, 9], seed=7)  # (every part has more than k vertices)
        else:  # Erdos-Renyi at N = 1M, p = 1 / N: hundreds of thousands of components, many isolated vertices
            _cache[name] = (graphs.ErdosRenyi(N=1000000, p=1e-6, seed=5).W, None)
    return _cache[name]


# ('hilbert' where there are coordinates)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("lap_type", ["combinatorial", "normalized"])
@pytest.mark.parametrize("name,reorder", [("logo", "none"), ("sensor123", "none"), ("sensor123", "hilbert"),
                                          ("union50k", "none"), ("union50k", "hilbert"), ("er1m", "none")])
def test_labels_equal_scipy(name, reorder, lap_type, dtype):
    W, coords = _differential_graph(name)
    G = graphs.Graph(W, lap_type=lap_type, coords=coords, compute_dtype=dtype, reorder=reorder, tiles=False)
    if name == "union50k":
        assert G.setup_report["reordered"] == (reorder == "hilbert")
    _check_against_scipy(G, W)
    if name == "er1m":
        n, labels = G.connected_components()
        assert n > 300000 and np.count_nonzero(np.bincount(labels) == 1) > 100000


def test_path_graph_stays_within_the_round_cap():
    """The diameter case: a path of 200,000 vertices with shuffled labels.  Neighbour-minimum propagation would need
    as many rounds as the path is long; hooking with pointer shortening stays within the library's own bound."""
    N = 200000
    order = np.random.default_rng(3).permutation(N)
    W = sparse.coo_matrix((np.ones(N - 1), (order[:-1], order[1:])), shape=(N, N))
    W = sparse.csr_matrix(W + W.T)
    G = graphs.Graph(W, reorder="none", tiles=False)
    report = _check_against_scipy(G, W)
    assert G.connected_components()[0] == 1
    cap = _round_cap(N)
    print("path of {}: {} rounds, cap {}, {:.3f} ms".format(N, report["rounds"], cap, report["kernel_ms"]))
    assert report["rounds"] <= cap < N // 1000
    # the same path in its own order: the longest chains the shortening pass can meet
    W = sparse.diags([np.ones(N - 1), np.ones(N - 1)], [-1, 1], format="csr")
    report = _check_against_scipy(graphs.Graph(W, reorder="none", tiles=False), W)
    print("sorted path of {}: {} rounds, {:.3f} ms".format(N, report["rounds"], report["kernel_ms"]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cancelling_weights_are_labelled_on_w(dtype, caplog):
    """lap_type='normalized' with negative weights: vertex 0 has dw == 0 and loses its row of L (graph.py:621-628),
    but W still joins 1 and 2 through it.  Components are those of W."""
    W = np.zeros((7, 7))
    for i, j, w in ((0, 1, 1.0), (0, 2, -1.0), (1, 3, 2.0), (4, 5, 1.5)):
        W[i, j] = W[j, i] = w
    W = sparse.csr_matrix(W)
    for lap_type in ("normalized", "combinatorial"):
        G = graphs.Graph(W, lap_type=lap_type, compute_dtype=dtype)
        n, labels = G.connected_components()
        assert n == 3 and labels.tolist() == [0, 0, 0, 0, 1, 1, 2] == _scipy_labels(W)[1].tolist()
        assert not G.is_connected()
        assert [p.info["orig_idx"] for p in G.extract_components()] == [[0, 1, 2, 3], [4, 5], [6]]


def test_entry_point_edges(ctx):
    """The C entry points themselves: count alone (null labels), a device labels array, N = 1, N = 0, a Laplacian
    uploaded as it is, and null arguments."""
    lib = _capi.load()
    W = random_graph(3000, 1.5, seed=9, isolated=40)
    n_ref, ref = _scipy_labels(W)
    dev = engine.DeviceGraph.from_w(W, ctx=ctx)
    n, labels, report = dev.components(labels=False)
    assert n == n_ref and labels is None and report["rounds"] <= report["round_cap"]
    n, labels, _ = dev.components()
    assert n == n_ref and np.array_equal(labels, ref)
    buf = ctx.alloc(4 * W.shape[0])
    count, rounds, ms = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_double(0)
    _capi.check(lib.gspx_graph_components_dev(dev._h, ctypes.c_void_p(buf.ptr), ctypes.byref(count), ctypes.byref(rounds),
                                              ctypes.byref(ms)))
    assert count.value == n_ref and np.array_equal(buf.download((W.shape[0],), np.int32), ref)
    assert rounds.value == report["rounds"] and ms.value > 0
    buf.free()
    # the Laplacian uploaded as it is (bit-parity mode), with an internal order
    perm = np.random.default_rng(1).permutation(W.shape[0]).astype(np.int32)
    n, labels, _ = engine.DeviceGraph.from_l(orc.laplacian(W), perm=perm, ctx=ctx).components()
    assert n == n_ref and np.array_equal(labels, ref)
    for N in (0, 1):
        n, labels, report = engine.DeviceGraph.from_w(sparse.csr_matrix((N, N)), ctx=ctx).components()
        assert n == N and labels.tolist() == [0] * N and report["rounds"] == N and report["round_cap"] == 1
    with pytest.raises(ValueError):
        _capi.check(lib.gspx_graph_components_dev(dev._h, None, None, None, None))
    assert [_round_cap(N) for N in (0, 1, 2, 3, 4, 5, 1 << 20, (1 << 20) + 1)] == [1, 1, 3, 5, 5, 7, 41, 43]


# ---- nothing is downloaded --------------------------------------------------------------------------------------
def test_connectivity_does_not_download_w(ctx):
    """A generator's W stays on the device through is_connected() and connected_components(): the labels come from
    the Laplacian that is already there.  The same for one trial of the block models' connected=True loop."""
    G = graphs.Sensor(200000, k=8, seed=3)
    assert G._adj_host is None and G._adj_dev is not None
    connected = G.is_connected()
    assert G._adj_host is None and G._adj_dev is not None
    n, labels = G.connected_components()
    assert G._adj_host is None and G._adj_dev is not None
    n_ref, ref = _scipy_labels(G.W)  # (downloads now)
    assert (n, connected) == (n_ref, n_ref == 1) and np.array_equal(labels, ref)
    # one trial of StochasticBlockModel(..., connected=True), as graphs.py builds it
    z = np.sort(np.random.default_rng(0).integers(0, 3, 20000))
    M = np.full((3, 3), 2e-5) + np.eye(3) * 4e-4
    W, _ = engine.sbm_graph(z, M, seed=11, ctx=ctx, keep_on_device=True)
    trial = graphs.Graph(W, reorder="none", tiles=False, ctx=ctx)
    connected = trial.is_connected()
    assert trial._adj_host is None and trial._adj_dev is not None
    assert connected == (_scipy_labels(trial.W)[0] == 1)
    sbm = graphs.StochasticBlockModel(N=3000, k=3, p=0.05, q=0.01, connected=True, seed=2)
    assert sbm.is_connected() and _scipy_labels(sbm.W)[0] == 1


# ---- directed graphs keep the host route ----------------------------------------------------------------------
def test_directed_graphs(golden):
    rng = np.random.default_rng(4)
    for n, density in ((60, 0.02), (60, 0.08), (8, 0.5)):
        W = sparse.random(n, n, density, random_state=rng, format="csr")
        W.setdiag(0)
        W.eliminate_zeros()
        G = graphs.Graph(W)
        assert G.is_directed()
        n_ref, ref = csgraph.connected_components(W, directed=True, connection="strong")
        assert G.is_connected() == (n_ref == 1)
        assert G.connected_components()[0] == n_ref and np.array_equal(G.connected_components()[1], ref)
        with pytest.raises(NotImplementedError, match="Directed graphs not supported yet."):
            G.extract_components()
    ring = sparse.csr_matrix(np.roll(np.eye(5), 1, axis=1))
    assert graphs.Graph(ring).is_connected() and graphs.Graph(ring).is_directed()


# ---- children are working device graphs -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_children_are_device_graphs(dtype):
    W, coords = _union_of_sensors([5000, 2500, 700], seed=21)
    G = graphs.Graph(W, lap_type="combinatorial", coords=coords, compute_dtype=dtype, reorder="hilbert", tiles=False)
    G.signals["ramp"] = np.arange(G.N, dtype=np.float64)
    G.signals["pair"] = np.random.default_rng(0).standard_normal((G.N, 2))
    G.plotting["vertex_size"] = 7
    parts = G.extract_components()
    n_ref, ref = _scipy_labels(W)
    assert len(parts) == n_ref == 3
    seen = np.concatenate([p.info["orig_idx"] for p in parts])
    assert np.array_equal(np.sort(seen), np.arange(G.N))
    for i, part in enumerate(parts):
        idx = np.asarray(part.info["orig_idx"])
        assert np.array_equal(idx, np.flatnonzero(ref == i))
        assert _same_csr(part.W, W[idx, :][:, idx])
        assert part.compute_dtype == np.dtype(dtype) and part.reorder == "hilbert" and part.lap_type == G.lap_type
        assert part.plotting == G.plotting and part.context is G.context
        L = orc.laplacian(part.W).astype(dtype)
        assert _same_csr(part.L, L) if dtype == np.float64 else abs(part.L - L).max() < 5e-6
        assert part.is_connected() and part.connected_components()[0] == 1
        assert np.array_equal(part.coords, coords[idx])
        assert np.array_equal(part.signals["ramp"], idx.astype(np.float64))
        assert np.array_equal(part.signals["pair"], G.signals["pair"][idx])
        assert part.dirichlet_energy(np.ones(part.N)) < 1e-3


# ---- the plugin seam --------------------------------------------------------------------------------------------
def _standin_pygsp(calls):
    """A pygsp-shaped module whose Graph has the reference's topology surface, computed by scipy on the host."""
    class Graph:
        def __init__(self, W, lap_type="combinatorial", coords=None):
            self.W = self.A = sparse.csr_matrix(W)
            self.N = self.n_vertices = self.W.shape[0]
            self.lap_type, self._connected, self.signals = lap_type, None, {}
            if coords is not None:
                self.coords = coords
            self.L = orc.laplacian(sparse.csr_matrix((self.W + self.W.T) / 2), lap_type)

        def is_directed(self):
            return (self.W != self.W.T).nnz != 0

        def is_connected(self):
            calls["is_connected"] += 1
            if self._connected is None:
                self._connected = csgraph.connected_components(self.W, directed=True, connection="strong")[0] == 1
            return self._connected

        def subgraph(self, vertices):
            calls["subgraph"] += 1
            return Graph(self.W[vertices, :][:, vertices], self.lap_type)

        def extract_components(self):
            calls["extract_components"] += 1
            if self.is_directed():
                raise NotImplementedError("Directed graphs not supported yet.")
            n, labels = csgraph.connected_components(self.W, directed=False)
            parts = []
            for c in range(n):
                parts.append(self.subgraph(np.flatnonzero(labels == c).tolist()))
                parts[-1].info = {"orig_idx": np.flatnonzero(labels == c).tolist()}
            return parts

    mod = types.ModuleType("pygsp")
    mod.graphs = types.ModuleType("pygsp.graphs")
    mod.graphs.Graph = Graph
    mod.filters = types.ModuleType("pygsp.filters")
    mod.filters.approximations = types.ModuleType("pygsp.filters.approximations")
    mod.filters.approximations.cheby_op = mod.filters.cheby_op = lambda G, c, s, **k: None
    return mod


def test_plugin_topology_seam(golden):
    calls = {"is_connected": 0, "extract_components": 0, "subgraph": 0}
    mod = _standin_pygsp(calls)
    Graph = mod.graphs.Graph
    own = (Graph.is_connected, Graph.extract_components)
    try:
        plugin.install(mod)
        assert (Graph.is_connected, Graph.extract_components) == own  # opt-in
        plugin.install(mod, topology=True)
        assert Graph.is_connected.__module__ == Graph.extract_components.__module__ == "pygsp_amd.plugin"
        for name in ("union4", "isolated", "loops_only", "doctest_connected"):
            for lap_type in ("combinatorial", "normalized"):
                W = csr_from(golden, name + "_W")
                G = Graph(W, lap_type)
                assert G.is_connected() == bool(golden[name + "_connected"]) and G._connected is G.is_connected()
                parts = G.extract_components()
                assert len(parts) == int(golden[name + "_n"])
                for i, part in enumerate(parts):
                    assert type(part) is Graph  # built by the package's own subgraph
                    assert part.info["orig_idx"] == golden["{}_k{}_idx".format(name, i)].tolist()
                    assert _same_csr(part.W, csr_from(golden, "{}_k{}_W".format(name, i)))
        assert calls["is_connected"] == calls["extract_components"] == 0 and calls["subgraph"] > 0
        # a directed graph reaches the originals
        D = Graph(csr_from(golden, "doctest_directed_W"))
        assert D.is_connected() is False and calls["is_connected"] == 1
        with pytest.raises(NotImplementedError):
            D.extract_components()
        assert calls["extract_components"] == 1
    finally:
        plugin.uninstall(mod)
    assert (Graph.is_connected, Graph.extract_components) == own and not hasattr(Graph, plugin._SAVED)
