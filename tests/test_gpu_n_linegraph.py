"""Line graphs on the device (gspx_linegraph_size / gspx_linegraph_build; engine.line_graph, graphs.LineGraph): against
what the real reference recorded (tests/golden/linegraph.npz) and against the numpy restatement of
tests/linegraph_helpers.py.  Every comparison of a matrix or of coordinates is exact; the one inexact comparison is
the filtered edge signal.  `-m gpu`."""
import ctypes
import logging
import types

import numpy as np
import pytest
from scipy import sparse

from conftest import csr_from, load_golden, rel_err
from gpu_helpers import ctx  # noqa: F401 (a fixture)
from linegraph_helpers import edge_list, line_graph, random_simple, same_csr, star, with_edge_count
from oracle import cheby_oracle as orc
from pygsp_amd import _capi, engine, filters, graphs, plugin

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
# the filtered panels of tests/test_gpu_4_ops.py: relative error against the largest entry
TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 3e-5}


@pytest.fixture(scope="module")
def golden():
    return load_golden("linegraph.npz")


def _free_device_bytes():
    """Free memory of the current device as the HIP runtime reports it (the runtime libgspx itself is linked to)."""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert ctypes.CDLL(path).hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def _build(dev):
    """gspx_linegraph_build on its own: (status, handle, kernel_ms)."""
    h, ms = ctypes.c_void_p(), ctypes.c_double(-1.0)
    rc = _capi.load().gspx_linegraph_build(dev._h, ctypes.byref(h), ctypes.byref(ms))
    return rc, h, ms.value


# ---- what the reference recorded ------------------------------------------------------------------------------
def test_golden_cases(golden, caplog):
    g = golden
    assert len(g["cases"]) >= 10
    for name in (str(c) for c in g["cases"]):
        lap_type = str(g[name + "_lap_type"])
        coords = g[name + "_coords"] if name + "_coords" in g else None
        G = graphs.Graph(csr_from(g, name + "_W"), lap_type=lap_type, coords=coords)
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            LG = graphs.LineGraph(G, lap_type=lap_type)
        warned = any("considered unweighted to build a binary line graph" in r.getMessage() for r in caplog.records)
        assert warned == G.is_weighted(), name
        on_device = not (bool(g[name + "_directed"]) or bool(g[name + "_loops"]))
        assert (LG.line_graph_info is not None) == on_device, name
        assert LG.N == LG.n_vertices == G.Ne == int(g[name + "_n_edges"]), name
        assert LG.n_edges == LG.Ne == int(g[name + "_LG_n_edges"]), name
        assert same_csr(LG.W, csr_from(g, name + "_LG")), name
        assert LG.lap_type == lap_type and LG.plotting == G.plotting
        if coords is None:
            assert not hasattr(LG, "coords"), name
        else:
            assert np.array_equal(LG.coords, g[name + "_LG_coords"]), name
    assert "weighted" in [str(c) for c in g["cases"]] and graphs.Graph(csr_from(g, "weighted_W")).is_weighted()


# ---- the route -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lap_type", ["combinatorial", "normalized"])
def test_route_stays_on_the_device(golden, lap_type):
    W, coords = csr_from(golden, "sensor30_W"), golden["sensor30_coords"]
    G = graphs.Graph(W, lap_type=lap_type, coords=coords)
    LG = graphs.LineGraph(G, lap_type=lap_type)
    assert LG._adj_dev is not None and LG._adj_host is None
    assert isinstance(LG._adj_dev, engine.DeviceAdjacency) and LG.line_graph_info["kernel_ms"] > 0
    report = LG.setup_report
    assert report["asymmetric"] == 0 and report["self_loops"] == 0 and report["zeros"] == 0
    A, midpoints = line_graph(W, coords)
    ref = graphs.Graph(A, lap_type=lap_type, coords=midpoints)
    assert same_csr(LG.L, ref.L)
    assert LG._adj_dev is not None  # (the Laplacian came from the device: W is still there)
    assert same_csr(LG.W, A) and LG._adj_dev is None and LG._adj_host is not None
    assert np.array_equal(LG.coords, midpoints) and np.array_equal(LG.dw, ref.dw)
    assert LG.A.nnz == A.nnz and np.array_equal(LG.d, np.diff(A.indptr))


# ---- shapes where the kernel can go wrong ----------------------------------------------------------------------
_SHAPES = {
    "random2_sparse": lambda: random_simple(2, 0.02, 1), "random2_dense": lambda: random_simple(2, 0.5, 4),
    "random65_sparse": lambda: random_simple(65, 0.02, 2), "random65_dense": lambda: random_simple(65, 0.5, 5),
    "random300_sparse": lambda: random_simple(300, 0.02, 3), "random300_dense": lambda: random_simple(300, 0.5, 6),
    "star300": lambda: star(300), "star70_path": lambda: star(70, tail=3),
    "edges255": lambda: with_edge_count(255, 7), "edges256": lambda: with_edge_count(256, 8),
    "edges257": lambda: with_edge_count(257, 9),
}
_restated = {}


def _shape(name):
    if name not in _restated:
        W = _SHAPES[name]()
        _restated[name] = (W, line_graph(W)[0])
    return _restated[name]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(_SHAPES))
def test_shapes_equal_the_restatement(name, dtype):
    W, A = _shape(name)
    if name == "star300":
        assert np.all(np.diff(A.indptr) == 298)
    if name == "star70_path":
        assert {1, 2, 69} <= set(np.diff(A.indptr).tolist())
    if name.startswith("edges"):
        assert A.shape[0] == int(name[5:])
    G = graphs.Graph(W, compute_dtype=dtype)
    dev = G.device_graph()
    assert engine.line_graph_size(dev) == (A.shape[0], A.nnz)
    if A.shape[0] == 0:  # (two vertices and no edge)
        return
    got, info = engine.line_graph(dev, keep_on_device=False)
    assert same_csr(got, A) and got.data.dtype == np.float64
    again, _ = engine.line_graph(dev, keep_on_device=False)  # the same bits on a second call
    assert same_csr(again, got)
    LG = graphs.LineGraph(G, compute_dtype=dtype)
    assert LG._adj_dev is not None and LG.N == G.Ne and LG.n_edges == A.nnz // 2
    assert same_csr(LG.W, A)


def test_internal_order_keeps_the_edge_numbering():
    """A graph the engine reorders internally (Hilbert curve): its line graph still numbers the edges as
    get_edge_list does, in the caller's vertex order."""
    G = graphs.Sensor(4096, k=6, seed=5, reorder="hilbert")
    assert G.setup_report["reordered"]
    LG = graphs.LineGraph(G)
    assert LG._adj_dev is not None
    W = G.W
    A, midpoints = line_graph(W, G.coords)
    sources, targets, _ = G.get_edge_list()
    assert np.array_equal(edge_list(W)[0], sources) and np.array_equal(edge_list(W)[1], targets)
    assert same_csr(LG.W, A) and np.array_equal(LG.coords, midpoints)


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_signals_land_where_they_belong(dtype):
    """y = G.grad(x) lives on the edges in get_edge_list order - the line graph's vertex order: a heat filter on the
    line graph gives what the same filter gives on the restated line graph."""
    G = graphs.Sensor(400, k=6, seed=11, compute_dtype=dtype)
    LG = graphs.LineGraph(G, compute_dtype=dtype)
    y = G.grad(np.random.default_rng(0).standard_normal(G.N))
    assert y.shape == (LG.N,)
    ref_graph = graphs.Graph(line_graph(G.W)[0], compute_dtype=dtype)
    for graph in (LG, ref_graph):
        graph.estimate_lmax("bounds")
    assert LG.lmax == ref_graph.lmax
    out = filters.Heat(LG, 5).filter(y)
    ref = filters.Heat(ref_graph, 5).filter(y)
    err = rel_err(out, ref)
    print("heat filter on the line graph, {}: relative error {:.3e}".format(np.dtype(dtype).name, err))
    assert out.shape == y.shape and err < TOL[np.dtype(dtype)]


# ---- sizes ------------------------------------------------------------------------------------------------------
def test_size_refusal_allocates_nothing(ctx):
    """The smallest case beyond 32 bits: a star of 46 343 vertices has 46 342 edges and 46 342 * 46 341 =
    2 147 534 622 > 2^31 - 1 stored entries in its line graph (25 GB of columns and values).  The size call counts
    them in 64 bits; the build refuses before it allocates anything of the output."""
    G = graphs.Graph(star(46343), reorder="none", tiles=False, ctx=ctx)
    dev = G.device_graph()
    assert engine.line_graph_size(dev) == (46342, 2147534622)  # (also builds the edge tables, once)
    pooled, free = ctx.pooled_bytes(), _free_device_bytes()
    rc, h, _ = _build(dev)
    assert rc == _capi.ERR_INVALID and not h.value
    message = _capi.last_error()
    assert "46342" in message and "2147534622" in message
    with pytest.raises(ValueError, match="2147534622"):
        graphs.LineGraph(G)
    with pytest.raises(ValueError, match="46342"):
        engine.line_graph(dev)
    after_pooled, after_free = ctx.pooled_bytes(), _free_device_bytes()
    print("pooled bytes {} -> {}, free device bytes {} -> {}".format(pooled, after_pooled, free, after_free))
    assert after_pooled == pooled and after_free == free
    # one vertex fewer fits: only its size is taken here
    fits = graphs.Graph(star(46342), reorder="none", tiles=False, ctx=ctx)
    assert engine.line_graph_size(fits.device_graph()) == (46341, 2147441940)
    assert 2147441940 <= 2 ** 31 - 1


def test_no_edges_gives_an_empty_handle(ctx):
    G = graphs.Graph(sparse.csr_matrix((5, 5)), ctx=ctx)
    dev = G.device_graph()
    assert engine.line_graph_size(dev) == (0, 0)
    rc, h, ms = _build(dev)
    assert rc == _capi.OK and h.value and ms == 0.0
    nnz = ctypes.c_int64(-1)
    _capi.check(_capi.load().gspx_knn_info(h, ctypes.byref(nnz), None, None))
    indptr = np.full(1, -1, dtype=np.int32)
    _capi.check(_capi.load().gspx_knn_download_w(h, _capi.ptr(indptr), None, None))
    _capi.load().gspx_knn_destroy(h)
    assert nnz.value == 0 and indptr.tolist() == [0]
    W, _ = engine.line_graph(dev, keep_on_device=False)
    assert W.shape == (0, 0) and W.nnz == 0


def test_refused_graphs(ctx):
    """A graph uploaded as L has no degrees to take edges from; a graph that carries a caller's edge list (directed,
    self-loops) belongs to the host route; null arguments."""
    lib = _capi.load()
    W = random_simple(20, 0.3, 12)
    from_l = engine.DeviceGraph.from_l(orc.laplacian(W), ctx=ctx)
    with pytest.raises(ValueError, match="created from W"):
        engine.line_graph_size(from_l)
    rc, h, _ = _build(from_l)
    assert rc == _capi.ERR_INVALID and not h.value
    dev = engine.DeviceGraph.from_w(W, ctx=ctx)
    src, dst = edge_list(W)
    dev.set_edge_list(src, dst, np.ones(src.size), directed=False)
    with pytest.raises(ValueError, match="edge list"):
        engine.line_graph(dev)
    with pytest.raises(ValueError, match="edge list"):
        engine.line_graph_size(dev)
    n = ctypes.c_int64(0)
    assert lib.gspx_linegraph_size(None, ctypes.byref(n), ctypes.byref(n)) == _capi.ERR_INVALID
    assert lib.gspx_linegraph_size(dev._h, None, None) == _capi.ERR_INVALID
    assert lib.gspx_linegraph_build(dev._h, None, None) == _capi.ERR_INVALID


# ---- the plugin seam --------------------------------------------------------------------------------------------
def _standin_pygsp(calls):
    """A pygsp-shaped module whose LineGraph forms its adjacency on the host, as the reference does."""
    class Graph:
        def __init__(self, adjacency, lap_type="combinatorial", coords=None, plotting={}):
            self.W = sparse.csr_matrix(adjacency)
            self.N = self.n_vertices = self.W.shape[0]
            directed = (self.W != self.W.T).nnz != 0
            self.n_edges = self.Ne = self.W.nnz if directed else sparse.triu(self.W).nnz
            self.lap_type, self.plotting = lap_type, plotting
            if coords is not None:
                self.coords = coords
            self.L = orc.laplacian(sparse.csr_matrix((self.W + self.W.T) / 2), lap_type)

        def is_directed(self):
            return (self.W != self.W.T).nnz != 0

        def is_weighted(self):
            return not np.all(self.W.data == 1)

        def get_edge_list(self):
            C = self.W.tocoo() if self.is_directed() else sparse.triu(self.W, format="coo")
            return C.row, C.col, C.data

    class LineGraph(Graph):
        def __init__(self, graph, **kwargs):
            calls["LineGraph"] += 1
            sources, targets, _ = graph.get_edge_list()
            adjacency, touches = graphs.line_graph_host(sources, targets, graph.N)
            coords = touches.dot(graph.coords) / 2 if hasattr(graph, "coords") else None
            super().__init__(adjacency, coords=coords, plotting=graph.plotting, **kwargs)

    mod = types.ModuleType("pygsp")
    mod.graphs = types.ModuleType("pygsp.graphs")
    mod.graphs.Graph, mod.graphs.LineGraph = Graph, LineGraph
    mod.filters = types.ModuleType("pygsp.filters")
    mod.filters.approximations = types.ModuleType("pygsp.filters.approximations")
    mod.filters.approximations.cheby_op = mod.filters.cheby_op = lambda G, c, s, **k: None
    return mod


def test_plugin_linegraph_seam(golden):
    calls = {"LineGraph": 0}
    mod = _standin_pygsp(calls)
    Graph, LineGraph = mod.graphs.Graph, mod.graphs.LineGraph
    own = LineGraph.__init__
    try:
        plugin.install(mod)
        assert LineGraph.__init__ is own  # opt-in
        plugin.install(mod, linegraph=True)
        assert LineGraph.__init__ is not own and LineGraph.__init__.__module__ == "pygsp_amd.plugin"
        for name in ("path4", "star6", "two_parts_isolated", "weighted", "sensor30", "sensor30_normalized"):
            lap_type = str(golden[name + "_lap_type"])
            coords = golden[name + "_coords"] if name + "_coords" in golden else None
            G = Graph(csr_from(golden, name + "_W"), lap_type, coords, {"vertex_size": 3})
            LG = LineGraph(G, lap_type=lap_type)
            assert type(LG) is LineGraph and LG.lap_type == lap_type and LG.plotting == {"vertex_size": 3}
            assert same_csr(LG.W, csr_from(golden, name + "_LG")) and LG.W.dtype.kind == "i", name
            assert LG.N == G.n_edges and LG.n_edges == int(golden[name + "_LG_n_edges"])
            if coords is not None:
                assert np.array_equal(LG.coords, golden[name + "_LG_coords"])
            else:
                assert not hasattr(LG, "coords")
        assert calls["LineGraph"] == 0
        # directed graphs and self-loops reach the package's own code
        for served, name in enumerate(("directed_antiparallel", "self_loop"), start=1):
            LG = LineGraph(Graph(csr_from(golden, name + "_W")))
            assert calls["LineGraph"] == served and same_csr(LG.W, csr_from(golden, name + "_LG"))
        plugin.install(mod)  # the flag off again: the original is back
        assert LineGraph.__init__ is own
        plugin.install(mod, linegraph=True)
    finally:
        plugin.uninstall(mod)
    assert LineGraph.__init__ is own and not hasattr(LineGraph, plugin._SAVED)
