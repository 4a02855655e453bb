"""Graph learning on the device (gspx_edge_sqdist_dev, gspx_learn_log_degrees_dev, pygsp_amd.graph_learning) against the
numpy restatement tests/graphlearn_helpers.py: edge distances within the bound of an F-term sum; P, w and the residual
history after fixed iteration counts within 1e-12 on the edge cases of both passes (one edge, a path, a star longer
than a workgroup in both numberings, an isolated vertex, edge counts off the workgroup size, an internal vertex order,
a warm start); the same niter and criterion where the restatement's rule is decisive; identical bytes on identical
calls; the adjacency bit for bit; LearnedGraph's neighbour counts; the refusals.  Needs a real MI355X: `-m gpu`."""
import numpy as np
import pytest
from scipy import sparse

import graphlearn_helpers as gl
from conftest import rel_err
from pygsp_amd import engine, graph_learning, graphs

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _star(leaves, centre_first):
    n = leaves + 1
    c = 0 if centre_first else leaves
    others = np.arange(1, n) if centre_first else np.arange(leaves)
    A = sparse.coo_matrix((np.ones(leaves), (np.full(leaves, c), others)), shape=(n, n))
    return sparse.csr_matrix(A + A.T)


def _path(n):
    A = sparse.coo_matrix((np.ones(n - 1), (np.arange(n - 1), np.arange(1, n))), shape=(n, n))
    return sparse.csr_matrix(A + A.T)


def _with_isolated():
    W = sparse.lil_matrix(_path(7))
    W[3, :] = 0
    W[:, 3] = 0  # vertex 3 loses its two edges
    W[2, 4] = W[4, 2] = 1.0
    return sparse.csr_matrix(W)


GRAPHS = {
    "single_edge": lambda: graphs.Graph(_path(2)),
    "path5": lambda: graphs.Graph(_path(5)),
    "star300_centre_first": lambda: graphs.Graph(_star(300, True)),
    "star300_centre_last": lambda: graphs.Graph(_star(300, False)),
    "isolated_vertex": lambda: graphs.Graph(_with_isolated()),
    "sensor300": lambda: graphs.Sensor(300, k=8, seed=3),
    "sensor2000": lambda: graphs.Sensor(2000, k=10, seed=4, reorder="none"),
    "sensor2000_morton": lambda: graphs.Sensor(2000, k=10, seed=4, reorder="morton"),
}


class Problem:
    """A graph, its edge list, z of mean 1 and the step; the restatement's results by (maxit, warm start), computed
    once."""

    def __init__(self, name):
        self.G = GRAPHS[name]()
        src, dst, _ = self.G.get_edge_list()
        self.src, self.dst, self.N = src.astype(np.int64), dst.astype(np.int64), self.G.N
        rng = np.random.default_rng(len(name))
        z = rng.uniform(0.2, 1.8, self.src.size)
        self.z = z / z.mean()
        self.w0 = rng.uniform(0.0, 1.0, self.src.size)
        self.gamma = gl.gamma_for(self.src, self.dst, self.N, 1.0)
        self.dev = self.G.device_graph()
        self._ref = {}

    def ref(self, maxit, warm=False, tol=None):
        key = (maxit, warm, tol)
        if key not in self._ref:
            self._ref[key] = gl.solve(self.src, self.dst, self.N, self.z, 1.0, 1.0, self.gamma, tol=tol, maxit=maxit,
                                      w0=self.w0 if warm else None)
        return self._ref[key]


_problems = {}


def problem(name):
    if name not in _problems:
        _problems[name] = Problem(name)
    return _problems[name]


# ---- edge_sqdist ------------------------------------------------------------------------------------------------
def _sqdist_reference(G, X):
    src, dst, _ = G.get_edge_list()
    d = X[src].astype(np.longdouble) - X[dst].astype(np.longdouble)
    return np.sum(d * d, axis=1)


@pytest.mark.parametrize("F", [1, 3, 64, 65, 257])
def test_edge_sqdist_within_the_bound_of_an_f_term_sum(F):
    """Every entry within 2 F eps relative: F squares of rounded differences (3 roundings of eps / 2 each) and an F-term
    sum of non-negative terms ((F - 1) eps / 2), whatever its order - derived, not measured."""
    G = graphs.Sensor(37, k=4, seed=1)
    X = np.random.default_rng(F).standard_normal((37, F))
    z = G.device_graph().edge_sqdist(X)
    ref = _sqdist_reference(G, X)
    assert z.shape == (G.n_edges,) and z.dtype == np.float64
    err = np.max(np.abs(z - ref) / ref)
    print("F =", F, "max relative error", float(err), "bound", 2 * F * EPS)
    assert err <= 2 * F * EPS


def test_edge_sqdist_with_an_internal_vertex_order_and_device_arrays():
    G = graphs.Sensor(500, k=5, seed=2, reorder="morton")
    assert G._internal_order() is not None
    X = np.random.default_rng(0).standard_normal((500, 6))
    ref = _sqdist_reference(G, X)
    dev = G.device_graph()
    z = dev.edge_sqdist(X)
    assert np.max(np.abs(z - ref) / ref) <= 2 * 6 * EPS
    zd = dev.edge_sqdist(G.to_device(X))
    assert isinstance(zd, engine.DeviceArray) and np.array_equal(np.asarray(zd), z)
    assert np.array_equal(dev.edge_sqdist(X[:, 0]), dev.edge_sqdist(X[:, :1]))  # a vector is one feature


# ---- fixed iteration counts -------------------------------------------------------------------------------------
def _compare(out, ref, what):
    """P and w within 1e-12 max|P| of the restatement; each of the four history sequences within 1e-12 relative in the
    project's metric (conftest.rel_err: the largest deviation over the largest entry of the sequence, as the objective
    sequences of the FISTA solvers are compared).  Entry by entry a residual norm cannot be held to 1e-12: ||w_k -
    w_{k-1}|| is a difference of numbers of size ||w||, known to eps ||w||, and has fallen to 1e-9 ||w|| and less on the
    small graphs after 300 iterations (measured: 3e-8 entrywise on the 7-vertex graph, 2.7e-16 in absolute terms)."""
    (P, w, _, info), (Pr, wr, ir) = out, ref
    scale = np.max(np.abs(Pr))
    eP, ew = np.max(np.abs(P - Pr)), np.max(np.abs(w - wr))
    h, hr = info["history"], np.asarray(ir["history"], dtype=np.float64)
    assert h.shape == hr.shape == (ir["niter"], 4)
    eh = max(rel_err(h[:, c], hr[:, c]) for c in range(4))
    print(what, "max|P|", scale, "err P", eP, "err w", ew, "history rel err", eh)
    assert info["niter"] == ir["niter"] and info["crit"] == ir["crit"]
    assert eP <= 1e-12 * scale and ew <= 1e-12 * scale
    assert eh <= 1e-12
    assert P.min() >= 0


@pytest.mark.parametrize("maxit", [1, 2, 50, 300])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_fixed_iteration_counts_match_the_restatement(name, maxit):
    p = problem(name)
    out = p.dev.learn_log_degrees(p.z, 1.0, 1.0, p.gamma, tol=None, maxit=maxit)
    _compare(out, p.ref(maxit), "{} maxit {}".format(name, maxit))
    assert out[3]["crit"] == "MAXIT"


@pytest.mark.parametrize("maxit", [1, 2, 50, 300])
def test_warm_start_matches_the_restatement(maxit):
    p = problem("sensor300")
    out = p.dev.learn_log_degrees(p.z, 1.0, 1.0, p.gamma, tol=None, maxit=maxit, w0=p.w0)
    _compare(out, p.ref(maxit, warm=True), "warm start maxit {}".format(maxit))


def test_isolated_vertex_and_star_reach_the_optimum():
    """Run to tol 1e-9, both problems meet the optimality conditions to what the restatement reaches."""
    for name in ("isolated_vertex", "star300_centre_last"):
        p = problem(name)
        P, _, _, info = p.dev.learn_log_degrees(p.z, 1.0, 1.0, p.gamma, tol=1e-9, maxit=20000)
        Pr, _, ir = p.ref(20000, tol=1e-9)
        res = np.max(np.abs(gl.kkt_residual(p.src, p.dst, p.N, p.z, 1.0, 1.0, P)))
        resr = np.max(np.abs(gl.kkt_residual(p.src, p.dst, p.N, p.z, 1.0, 1.0, Pr)))
        print(name, "niter", info["niter"], ir["niter"], "KKT", res, resr)
        assert info["crit"] == "TOL" and res <= 10 * resr


# ---- stopping ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [1e-3, 1e-5])
def test_stopping_rule_matches_the_restatement(tol):
    p = problem("sensor300")
    ref = p.ref(10000, tol=tol)
    gl.assert_rule_is_decisive(ref[2], tol)
    out = p.dev.learn_log_degrees(p.z, 1.0, 1.0, p.gamma, tol=tol, maxit=10000)
    print("tol", tol, "niter", out[3]["niter"], ref[2]["niter"], "crit", out[3]["crit"], ref[2]["crit"])
    assert ref[2]["crit"] == "TOL"
    assert (out[3]["niter"], out[3]["crit"]) == (ref[2]["niter"], ref[2]["crit"])
    _compare(out, ref, "tol {}".format(tol))


def test_maxit_is_reported():
    p = problem("sensor300")
    info = p.dev.learn_log_degrees(p.z, 1.0, 1.0, p.gamma, tol=1e-5, maxit=9)[3]
    assert (info["niter"], info["crit"]) == (9, "MAXIT") and info["history"].shape == (9, 4) and info["ms"] > 0


def test_public_function_runs_the_same_iteration():
    p = problem("sensor300")
    w, info = graph_learning.learn_weights(p.G, Z=p.z, tol=1e-5)
    Pr, wr, ir = p.ref(10000, tol=1e-5)
    assert info["niter"] == ir["niter"] and np.max(np.abs(w - Pr)) <= 1e-12 * Pr.max()
    assert np.max(np.abs(info["w_last"] - wr)) <= 1e-12 * Pr.max()
    X = np.random.default_rng(1).standard_normal((p.N, 5))
    theta = 0.37
    zx = np.sum((X[p.src] - X[p.dst]) ** 2, axis=1) * theta
    wx, infox = graph_learning.learn_weights(p.G, X, theta=theta, tol=None, maxit=100)
    Px, _, _ = gl.solve(p.src, p.dst, p.N, zx, 1.0, 1.0, p.gamma, tol=None, maxit=100)
    # (z differs from the host's by the rounding of the scaled signals: a few eps of z, far below the bound)
    assert np.max(np.abs(wx - Px)) <= 1e-12 * Px.max()


# ---- reproducibility --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sensor2000_morton", "star300_centre_first"])
def test_identical_calls_give_identical_bytes(name):
    p = problem(name)
    a = p.dev.learn_log_degrees(p.z, 1.0, 1.0, p.gamma, tol=1e-5, maxit=400)
    b = p.dev.learn_log_degrees(p.z, 1.0, 1.0, p.gamma, tol=1e-5, maxit=400)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[3]["history"].tobytes() == b[3]["history"].tobytes() and a[3]["niter"] == b[3]["niter"]


# ---- adjacency --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sensor300", "star300_centre_last", "isolated_vertex", "sensor2000_morton"])
def test_adjacency_is_the_host_assembly_of_p(name):
    p = problem(name)
    P, _, Wd, info = p.dev.learn_log_degrees(p.z, 1.0, 1.0, p.gamma, tol=1e-5, maxit=2000, adjacency=True)
    assert isinstance(Wd, engine.DeviceAdjacency)
    half = sparse.coo_matrix((P, (p.src, p.dst)), shape=(p.N, p.N))
    host = sparse.csr_matrix(half + half.T)
    host.eliminate_zeros()
    host.sort_indices()
    G = graphs.Graph(Wd)  # adopts the handle where it lies
    W = G.W
    assert W.nnz == host.nnz == 2 * np.count_nonzero(P)
    assert np.array_equal(W.indptr, host.indptr) and np.array_equal(W.indices, host.indices)
    assert W.data.tobytes() == host.data.tobytes()  # bit for bit, and hence equal to its transpose
    assert np.all(W.data > 0) and W.has_sorted_indices and W.diagonal().max() == 0
    assert (W != W.T).nnz == 0
    L = sparse.diags(np.ravel(host.sum(axis=1))) - host
    assert abs(G.L - L).max() <= 1e-13


# ---- LearnedGraph -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 5, 8])
def test_learned_graph_keeps_about_k_neighbours(k):
    X = np.random.default_rng(11).uniform(0, 1, (500, 2))
    G = graphs.LearnedGraph(X, k=k, candidates=16)
    assert G._adj_dev is not None  # W has not crossed PCIe yet
    W = G.W
    mean = W.getnnz(axis=1).mean()
    print("k", k, "mean neighbours", mean, "theta", G.theta, "niter", G.learn_info["niter"], "candidates",
          G.candidate_edges)
    assert k - 1 <= mean <= k + 1
    assert (W != W.T).nnz == 0 and W.data.min() > 0 and W.diagonal().max() == 0
    assert G.learn_info["crit"] == "TOL" and G.N == 500 and G.coords.shape == (500, 2)
    assert G.candidate_edges >= W.nnz // 2
    y = G.L @ np.ones(500)
    assert np.max(np.abs(y)) < 1e-12 * G.dw.max()
    assert W.getnnz(axis=1).min() >= 1  # the log barrier leaves no vertex without an edge


def test_learned_graph_from_a_wide_cloud():
    """80 dimensions: the wide neighbour search and the run-time feature loop of the distance kernel."""
    X = np.random.default_rng(12).standard_normal((300, 80))
    G = graphs.LearnedGraph(X, k=5, candidates=16)
    W = G.W
    mean = W.getnnz(axis=1).mean()
    print("wide cloud: mean neighbours", mean, "theta", G.theta, "niter", G.learn_info["niter"])
    assert (W != W.T).nnz == 0 and W.data.min() > 0 and W.getnnz(axis=1).min() >= 1
    assert G.coords.shape == (300, 3) and G.learn_info["crit"] == "TOL"
    # a given theta is used as it is
    G2 = graphs.LearnedGraph(X, k=5, candidates=16, theta=G.theta)
    assert G2.W.data.tobytes() == W.data.tobytes()


# ---- refusals ---------------------------------------------------------------------------------------------------
def test_refusals():
    p = problem("path5")
    z = p.z
    f32 = graphs.Graph(_path(5), compute_dtype=np.float32)
    with pytest.raises(ValueError, match="float32"):
        f32.device_graph().learn_log_degrees(z, 1.0, 1.0, 0.1)
    with pytest.raises(ValueError, match="float32"):
        f32.device_graph().edge_sqdist(np.ones((5, 2)))
    with pytest.raises(ValueError, match="float64"):
        graph_learning.learn_weights(f32, Z=z)
    D = sparse.csr_matrix(np.triu(_path(5).toarray()))
    directed = graphs.Graph(D)
    with pytest.raises(ValueError, match="directed"):
        graph_learning.learn_weights(directed, Z=np.ones(directed.n_edges))
    with pytest.raises(ValueError, match="edge list"):  # the engine level: the graph carries the directed edge list
        directed._device_differential().learn_log_degrees(np.ones(directed.n_edges), 1.0, 1.0, 0.1)
    loops = _path(5).tolil()
    loops[2, 2] = 1.0
    looped = graphs.Graph(sparse.csr_matrix(loops))
    with pytest.raises(ValueError, match="edge list"):
        graph_learning.learn_weights(looped, Z=np.ones(looped.n_edges))
    from_l = engine.DeviceGraph.from_l(p.G.L)
    with pytest.raises(ValueError, match="created from"):
        from_l.learn_log_degrees(z, 1.0, 1.0, 0.1)
    for kw in (dict(a=0.0), dict(a=-1.0), dict(b=-1.0), dict(step=0.0), dict(step=1.0)):
        with pytest.raises(ValueError):
            graph_learning.learn_weights(p.G, Z=z, **kw)
    for a, b, gamma, tol, maxit in ((0.0, 1.0, 0.1, 1e-5, 10), (np.inf, 1.0, 0.1, 1e-5, 10), (1.0, -1.0, 0.1, 1e-5, 10),
                                    (1.0, 1.0, 0.0, 1e-5, 10), (1.0, 1.0, 0.1, np.nan, 10), (1.0, 1.0, 0.1, 1e-5, 0),
                                    (1.0, 1.0, 0.1, 1e-5, 10 ** 7 + 1)):
        with pytest.raises(ValueError):
            p.dev.learn_log_degrees(z, a, b, gamma, tol=tol, maxit=maxit)
    for bad in (np.nan, -0.5):
        zb = z.copy()
        zb[1] = bad
        with pytest.raises(ValueError, match="negative or NaN"):
            p.dev.learn_log_degrees(zb, 1.0, 1.0, 0.1)  # the device pass
        with pytest.raises(ValueError, match="negative or NaN"):
            graph_learning.learn_weights(p.G, Z=zb)
    with pytest.raises(ValueError, match="exactly one"):
        graph_learning.learn_weights(p.G)
    with pytest.raises(ValueError, match="exactly one"):
        graph_learning.learn_weights(p.G, np.ones((5, 2)), Z=z)
    with pytest.raises(ValueError):
        p.dev.learn_log_degrees(z[:-1], 1.0, 1.0, 0.1)
    with pytest.raises(ValueError):
        p.dev.edge_sqdist(np.ones((4, 2)))
    with pytest.raises(ValueError):
        p.dev.edge_sqdist(np.ones((5, 4097)))
    X = np.random.default_rng(0).uniform(0, 1, (200, 2))
    with pytest.raises(ValueError, match="exceed"):
        graphs.LearnedGraph(X, k=8, candidates=8)
    with pytest.raises(ValueError, match="at most"):
        graphs.LearnedGraph(X, k=8, candidates=65)
    # the graph still works after every refusal
    assert p.dev.learn_log_degrees(z, 1.0, 1.0, p.gamma, tol=None, maxit=3)[3]["niter"] == 3


def test_edgeless_graph_returns_at_once():
    G = graphs.Graph(sparse.csr_matrix((4, 4)))
    P, w, W, info = G.device_graph().learn_log_degrees(np.zeros(0), 1.0, 1.0, 0.5, adjacency=True)
    assert P.shape == w.shape == (0,) and info["niter"] == 0 and info["crit"] is None and W.nnz == 0
    assert G.device_graph().edge_sqdist(np.ones((4, 3))).shape == (0,)
