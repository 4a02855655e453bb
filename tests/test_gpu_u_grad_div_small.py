"""grad = D^T x and div = D y (gspx_grad_dev / gspx_div_dev; grad_div_t of gspx_ops.hip.h) on graphs of a handful of
vertices, against oracle/ops_oracle.py - whose D is built from W, not from the device's edge arrays - at the bars of
test_gpu_4_ops (1e-12 / 3e-5).

Which kernel a case launches (grad_div_t): the vertex walk k_grad_v / k_div_v (<double, 2> / <float, 4>) iff the width
is a multiple of 16 bytes of elements, N >= 8 and edge_vertex_walk is on; else k_grad / k_div.  So
- N 1, 4, 5, 6 and 7 take the plain kernels at every width, N = 8 and 9 (per_xcd = 1 and 2: XCD ranges far below one
  workgroup pass, ranges past N at 9) the walk at the even widths, N = 65, 257, 1027 a ragged last range;
- fp64 widths 1 and 3 and 65 are plain (cw 1, 4, 64 with a second column pass); 2, 4, 6, 16, 64, 128, 130, 200 walk
  in groups of 1, 2, 4 (an idle lane), 8, 32, 64, 64 (a second chunk pass of one lane) and 64 lanes; fp32 widths 1 and
  3 are plain, 4, 8, 12, 20, 256, 260 walk in groups of 1, 2, 4 (idle), 8 (idle), 64 and 64 (a second pass of one);
- the stars give the four-in-flight loops every remainder of the degree mod 4 on the source side (hub = vertex 0: all
  edges leave it) and on the target side (hub = last vertex: all edges end in it); the random graphs carry a hub row
  of up to 300 edges and two isolated vertices.
Every walked case is repeated with edge_vertex_walk = 0 and held to 4 eps of the walk's result, as
test_oracle_sensor20k does.  Caller edge lists (a directed graph, a graph with self-loops) go in through Graph and
through DeviceGraph.set_edge_list, with and without a vertex permutation."""
import numpy as np
import pytest
from scipy import sparse

from conftest import rel_err
from gpu_helpers import ctx, random_graph  # noqa: F401 (ctx: fixture)
from operator_pins_helpers import (directed_graph, edgeless_graph, isolated_vertex_graph, path_graph, self_loop_graph,
                                   shuffled_order, star_graph)
from oracle import ops_oracle as ops
from pygsp_amd import engine, graphs

pytestmark = pytest.mark.gpu

TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 3e-5}  # test_gpu_4_ops.TOL
WIDTHS = {np.dtype(np.float64): [1, 2, 3, 4, 6, 16, 64, 65, 128, 130, 200],
          np.dtype(np.float32): [1, 3, 4, 8, 12, 20, 256, 260]}
GRAPHS = {"path5": lambda: path_graph(5), "path7": lambda: path_graph(7), "path9": lambda: path_graph(9),
          "isolated6": isolated_vertex_graph, "edgeless4": lambda: edgeless_graph(4), "one": lambda: edgeless_graph(1)}
for _deg in (12, 13, 14, 15):
    GRAPHS["star{}".format(_deg + 1)] = lambda d=_deg: star_graph(d, seed=d)
    GRAPHS["star{}-hub-last".format(_deg + 1)] = lambda d=_deg: star_graph(d, hub_last=True, seed=d)
for _n in (7, 8, 9, 65, 257, 1027):
    GRAPHS["rand{}".format(_n)] = lambda n=_n: random_graph(n, 4, 900 + n, hub=True, isolated=2)
_WORST = {}


def note(test, dtype, err, where):
    key = (test, np.dtype(dtype).name)
    if err >= _WORST.get(key, (-1.0, None))[0]:
        _WORST[key] = (err, where)


def teardown_module(module):
    for (test, dt), (err, where) in sorted(_WORST.items()):
        print("\nworst {:<34s} {:<8s} {:.2e} of max |ref| at {}".format(test, dt, err, where), end="")
    print()
    _WORST.clear()


def walks(N, nsig, dtype):
    return N >= 8 and nsig % (16 // np.dtype(dtype).itemsize) == 0


def check_grad_div(ctx, dev, D, N, dtype, widths, rng, where):
    """grad and div of dev against the oracle's D at every width; the edge-order kernels against the walk."""
    dt = np.dtype(dtype)
    tol, E = TOL[dt], D.shape[1]
    assert dev.n_edges() == E, where
    for nsig in widths:
        X = rng.standard_normal((N, nsig)).astype(dtype)
        Y = dev.grad(X)
        assert Y.shape == (E, nsig) and Y.dtype == dt and np.all(np.isfinite(Y)), (where, nsig)
        err = rel_err(Y.astype(np.float64), ops.grad(D, X.astype(np.float64)))
        note("grad", dtype, err, (where, nsig))
        assert err < tol, (where, nsig, "grad", err)
        Yin = rng.standard_normal((E, nsig)).astype(dtype)  # (not grad's output: div gets an input of its own)
        Z = dev.div(Yin)
        assert Z.shape == (N, nsig) and Z.dtype == dt and np.all(np.isfinite(Z)), (where, nsig)
        err = rel_err(Z.astype(np.float64), ops.div(D, Yin.astype(np.float64)))
        note("div", dtype, err, (where, nsig))
        assert err < tol, (where, nsig, "div", err)
        if E == 0:
            assert not Z.any(), (where, nsig)  # exact zeros, every row written
        assert Y.tobytes() == dev.grad(X).tobytes() and Z.tobytes() == dev.div(Yin).tobytes(), (where, nsig)
        if walks(N, nsig, dtype):
            ctx.set_option("edge_vertex_walk", 0)  # the edge-order kernels: same sums, same order
            try:
                e_grad, e_div = rel_err(dev.grad(X), Y), rel_err(dev.div(Yin), Z)
            finally:
                ctx.set_option("edge_vertex_walk", 1)
            note("edge order against the walk", dtype, max(e_grad, e_div), (where, nsig))
            assert e_grad < 4 * np.finfo(dtype).eps and e_div < 4 * np.finfo(dtype).eps, (where, nsig, e_grad, e_div)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_grad_div_on_tiny_graphs(ctx, name, dtype):
    W = GRAPHS[name]()
    N = W.shape[0]
    rng = np.random.default_rng(sorted(GRAPHS).index(name))
    for lap_type in ("combinatorial", "normalized"):
        D = ops.differential_operator(W, lap_type)
        L = ops.laplacian(W, lap_type)
        for perm in (shuffled_order(rng, N), None):
            dev = engine.DeviceGraph.from_w(W, lap_type, dtype=dtype, perm=perm, ctx=ctx)
            try:
                where = (name, lap_type, perm is not None)
                check_grad_div(ctx, dev, D, N, dtype, WIDTHS[np.dtype(dtype)], rng, where)
                # div(grad(x)) = L x (difference.py:38-45), one signal and four
                for nsig in (1, 4):
                    X = rng.standard_normal((N, nsig)).astype(dtype)
                    err = rel_err(dev.div(dev.grad(X)), L.dot(X.astype(np.float64)))
                    note("div(grad(x)) against L x", dtype, err, (where, nsig))
                    assert err < TOL[np.dtype(dtype)] * 10, (where, nsig, err)
            finally:
                dev.destroy()


def test_switch_to_the_walk_at_eight_vertices(ctx):
    """N = 7 stays on the edge-order kernels whatever the option says - the same bytes with the walk on and off -
    and N = 8 takes the walk at an even width; both match the oracle (test_grad_div_on_tiny_graphs holds them to it)."""
    for N, name in ((7, "rand7"), (8, "rand8")):
        W = GRAPHS[name]()
        D = ops.differential_operator(W)
        dev = engine.DeviceGraph.from_w(W, dtype=np.float64, ctx=ctx)
        try:
            X = np.random.default_rng(N).standard_normal((N, 4))
            Y = dev.grad(X)
            assert rel_err(Y, ops.grad(D, X)) < 1e-12 and rel_err(dev.div(Y), ops.div(D, Y)) < 1e-12
            ctx.set_option("edge_vertex_walk", 0)
            try:
                Y0 = dev.grad(X)
            finally:
                ctx.set_option("edge_vertex_walk", 1)
            if N < 8:
                assert Y0.tobytes() == Y.tobytes()
            assert rel_err(Y0, Y) < 4 * np.finfo(np.float64).eps
        finally:
            dev.destroy()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["directed", "self-loops"])
def test_caller_edge_lists_with_a_vertex_permutation(ctx, kind, dtype):
    """A directed graph (every stored entry an edge, D / sqrt(2)) and an undirected one with self-loops (edges whose two
    D values cancel): the edge list of Graph.get_edge_list handed to the device by Graph and by
    DeviceGraph.set_edge_list, widths 4 (the walk) and 5 (the plain kernels), with and without a vertex permutation.
    L = D D^T holds for both kinds and both Laplacian types (tests/test_operator_pins_host.py checks it on these very
    graphs), so div(grad(x)) is held to the oracle's L x as well."""
    W = directed_graph() if kind == "directed" else self_loop_graph()
    N = W.shape[0]
    directed = kind == "directed"
    assert ((W != W.T).nnz != 0) == directed and (W.diagonal().any() != directed)
    rng = np.random.default_rng(40 + directed)
    src, dst, wts = ops.get_edge_list(W)
    Wsym = sparse.csr_matrix((W + W.T) / 2) if directed else W
    tol = TOL[np.dtype(dtype)]
    for lap_type in ("combinatorial", "normalized"):
        D = ops.differential_operator(W, lap_type)
        L = ops.laplacian(W, lap_type)
        assert D.shape[1] == src.size
        for perm in (shuffled_order(rng, N), None):
            G = graphs.Graph(W, lap_type=lap_type, compute_dtype=dtype, tiles=False, ctx=ctx,
                             reorder="none" if perm is None else perm.tolist())
            assert G.is_directed() == directed and G.Ne == src.size
            by_graph = G._device_differential()
            assert (by_graph.download_perm() is not None) == (perm is not None)
            by_hand = engine.DeviceGraph.from_w(Wsym, lap_type, dtype=dtype, perm=perm, ctx=ctx)
            by_hand.set_edge_list(src, dst, wts, directed)
            try:
                for how, dev in (("Graph", by_graph), ("set_edge_list", by_hand)):
                    where = (kind, lap_type, perm is not None, how)
                    check_grad_div(ctx, dev, D, N, dtype, (4, 5), rng, where)
                    for nsig in (4, 5):
                        X = rng.standard_normal((N, nsig)).astype(dtype)
                        err = rel_err(dev.div(dev.grad(X)), L.dot(X.astype(np.float64)))
                        note("caller edges: div(grad(x)), L x", dtype, err, (where, nsig))
                        assert err < tol * 10, (where, nsig, err)
            finally:
                by_hand.destroy()
