"""Line graphs without a GPU: the restatement the device tests compare with (tests/linegraph_helpers.py) against what
the real reference recorded (tests/golden/linegraph.npz), the host route of graphs.LineGraph against the same
records - directed graphs and self-loops included - and the two properties of the unweighted view, Graph.A and
Graph.d, on the reference's docstring examples."""
import numpy as np
import pytest
from scipy import sparse

from conftest import csr_from, load_golden
from linegraph_helpers import edge_list, line_graph, random_simple, same_csr, star, with_edge_count
from pygsp_amd import engine, graphs, plugin


@pytest.fixture(scope="module")
def golden():
    return load_golden("linegraph.npz")


def _bare_graph(W):
    """A Graph around W without a device: what A, d and is_directed read."""
    G = graphs.Graph.__new__(graphs.Graph)
    G._adj_host, G._adj_dev, G._flags, G._A, G._d = sparse.csr_matrix(W), None, {}, None, None
    return G


def test_golden_holds_the_cases():
    g = load_golden("linegraph.npz")
    assert {"path4", "triangle", "star6", "two_parts_isolated", "single_edge", "weighted", "sensor30",
            "sensor30_normalized", "directed_antiparallel", "self_loop"} <= set(str(c) for c in g["cases"])
    assert bool(g["directed_antiparallel_directed"]) and bool(g["self_loop_loops"])
    # the star's line graph is K6; a single edge gives one vertex and no edge
    assert np.array_equal(csr_from(g, "star6_LG").toarray(), 1 - np.eye(6, dtype=np.int64))
    assert csr_from(g, "single_edge_LG").shape == (1, 1) and csr_from(g, "single_edge_LG").nnz == 0
    assert str(g["sensor30_normalized_lap_type"]) == "normalized"


def test_restatement_equals_the_reference(golden):
    g = golden
    seen = 0
    for name in (str(c) for c in g["cases"]):
        if bool(g[name + "_directed"]) or bool(g[name + "_loops"]):
            continue
        seen += 1
        coords = g[name + "_coords"] if name + "_coords" in g else None
        A, midpoints = line_graph(csr_from(g, name + "_W"), coords)
        assert same_csr(A, csr_from(g, name + "_LG")), name
        assert A.shape[0] == int(g[name + "_n_edges"]) and A.nnz == 2 * int(g[name + "_LG_n_edges"]), name
        if coords is not None:
            assert np.array_equal(midpoints, g[name + "_LG_coords"]), name
    assert seen >= 8


def test_host_route_equals_the_reference(golden):
    """graphs.line_graph_host - the route of directed graphs and self-loops - on EVERY recorded case, from the edge
    list Graph.get_edge_list would give: all stored entries of a directed graph, else the upper triangle with the
    diagonal."""
    g = golden
    for name in (str(c) for c in g["cases"]):
        W = csr_from(g, name + "_W")
        C = W.tocoo() if bool(g[name + "_directed"]) else sparse.triu(W, format="coo")
        assert C.row.size == int(g[name + "_n_edges"]), name
        A, touches = graphs.line_graph_host(C.row, C.col, W.shape[0])
        assert same_csr(A, csr_from(g, name + "_LG")), name
        if name + "_coords" in g:
            assert np.array_equal(touches.dot(g[name + "_coords"]) / 2, g[name + "_LG_coords"]), name
    # the recorded quirks: the antiparallel pair is joined once (a boolean product), the self-loop carries -1
    assert csr_from(g, "directed_antiparallel_LG").toarray().tolist() == [[0, 1, 1], [1, 0, 1], [1, 1, 0]]
    loop = csr_from(g, "self_loop_LG")
    assert loop.diagonal().tolist() == [0, 0, 0, -1, 0] and loop[3].nnz == 1


def test_restatement_on_the_device_test_shapes():
    """The shapes of tests/test_gpu_n_linegraph.py: row lengths are deg(s) + deg(t) - 2 and the matrix is symmetric."""
    for W in (star(300), star(70, tail=3), random_simple(65, 0.5, 1), with_edge_count(257, 2)):
        A, _ = line_graph(W)
        src, dst = edge_list(W)
        deg = W.getnnz(axis=1)
        assert np.array_equal(np.diff(A.indptr), deg[src] + deg[dst] - 2)
        assert (A != A.T).nnz == 0 and not A.diagonal().any() and np.all(A.data == 1.0)
    assert with_edge_count(255, 3).nnz == 510
    lengths = np.diff(line_graph(star(70, tail=3))[0].indptr)
    assert {1, 2, 69, 68} == set(lengths.tolist())


def test_the_surface_exists():
    assert issubclass(graphs.LineGraph, graphs.Graph)
    assert isinstance(graphs.Graph.A, property) and isinstance(graphs.Graph.d, property)
    assert callable(engine.line_graph) and callable(engine.line_graph_size)
    import inspect
    assert inspect.signature(plugin.install).parameters["linegraph"].default is False
    assert list(inspect.signature(graphs.LineGraph.__init__).parameters) == ["self", "graph", "kwargs"]


def test_degree_docstring_examples():
    """graph.py:729-781: the examples of Graph.d, undirected then directed; A is W > 0."""
    G = _bare_graph([[0, 1, 0], [1, 0, 2], [0, 2, 0]])
    assert G.d.tolist() == [1, 2, 1] and str(G.d) == "[1 2 1]"
    assert G.d is G.d
    G = _bare_graph([[0, 1, 0], [0, 0, 2], [0, 2, 0]])
    assert G.d.tolist() == [0.5, 1.5, 1.0] and str(G.d) == "[0.5 1.5 1. ]"
    A = G.A
    assert A.dtype == bool and A.toarray().tolist() == [[False, True, False], [False, False, True], [False, True, False]]
    assert G.A is A
    G._adjacency = sparse.csr_matrix(np.array([[0, 3.0], [3.0, 0]]))  # W replaced: both caches go
    assert G._A is None and G._d is None and G.d.tolist() == [1, 1] and G.A.nnz == 2
