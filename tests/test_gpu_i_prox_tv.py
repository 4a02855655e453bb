"""The graph total-variation prox on the device (gspx_prox_tv_dev) against the numpy restatement of the iteration
(tests/prox_tv_helpers.py): the same niter and stopping criterion, objective sequences within 1e-12 relative, z within
1e-10, on the golden graph with every criterion, on every lane build, on the edge cases of the edge walk, on sensor
graphs up to 100k vertices, on a directed graph and one with self-loops; determinism; the float32 mirror graph; device
arrays; convergence to the duality gap; the entry point's refusals; the real pygsp through
plugin.install(optimization=True) where one is importable.  Before every comparison the restatement's own sequence is
checked to keep a relative 1e-6 between each compared quantity and its threshold (a condition on the inputs), so
rounding cannot move niter.  Needs a real MI355X: `-m gpu`."""
import importlib.util

import numpy as np
import pytest
from scipy import sparse

import learning_helpers as lh
import prox_tv_helpers as th
from conftest import load_golden
from pygsp_amd import graphs, optimization

pytestmark = pytest.mark.gpu


def _check(dev_out, ref_out):
    (z, info), (zr, ir) = dev_out, ref_out
    print("niter", info["niter"], ir["niter"], "crit", info["crit"], ir["crit"], "obj err",
          np.abs(info["objective"][:2] - ir["objective"][:2]).max(), "z err", np.abs(z - zr).max())
    assert (info["niter"], info["crit"]) == (ir["niter"], ir["crit"])
    obj, objr = info["objective"], ir["objective"]
    assert obj.shape == objr.shape
    assert np.abs(obj - objr).max() <= 1e-12 * np.abs(objr).max()
    assert z.shape == zr.shape and np.abs(z - zr).max() < 1e-10


def _rule(opts):
    return dict(rtol=opts.get("rtol", 1e-3), atol=opts.get("atol"), dtol=opts.get("dtol"), xtol=opts.get("xtol"),
                maxit=opts.get("maxit", 200))


def _device_runs(dev, D, x, gamma, step, **opts):
    """The engine-level call and the restatement, the latter checked to be decisive first."""
    ref = th.solve(D, x, gamma, step, **_rule(opts))
    th.assert_rule_is_decisive(ref[1], **_rule(opts))
    return dev.prox_tv(x, gamma, step, **_rule(opts)), ref


def _runs(G, x, gamma, **opts):
    """The public function (tol is its name for rtol) and the restatement on G.D."""
    rule = _rule(opts)
    ref = th.solve(G.D, x, gamma, optimization.tv_step(G), **rule)
    th.assert_rule_is_decisive(ref[1], **rule)
    kw = {k: v for k, v in opts.items() if k in ("atol", "dtol", "xtol")}
    return optimization.prox_tv_solve(x, gamma, G, tol=rule["rtol"], maxit=rule["maxit"], **kw), ref


def _with_d(G, dense_lmax=False):
    if dense_lmax:
        G._lmax = float(np.linalg.eigvalsh(G.L.toarray())[-1])
    else:
        G.estimate_lmax()
    G.compute_differential_operator()
    return G


@pytest.fixture(scope="module")
def golden_graph():
    W, _, _ = lh.golden_problem(load_golden("ops_sensor123.npz"))
    return _with_d(graphs.Graph(W))


@pytest.fixture(scope="module")
def sensor2000():
    return _with_d(graphs.Sensor(2000, seed=0))


def _rule_cases(G, x, gamma):
    """The default rule, then atol, dtol, xtol and maxit each set to fire on its own, at thresholds that no value of
    the restatement's sequence lies near."""
    yield {}
    _, free = th.solve(G.D, x, gamma, optimization.tv_step(G), rtol=None, maxit=12)
    obj, dx = free["objective"], free["dx"]
    yield dict(rtol=None, atol=th.threshold_between(obj, 8))
    yield dict(rtol=None, dtol=th.threshold_between(np.abs(np.diff(obj)), 7))
    yield dict(rtol=None, xtol=th.threshold_between(dx, 6))
    yield dict(rtol=None, maxit=9)


@pytest.mark.parametrize("gamma", [0.05, 0.5])
def test_golden_graph_every_rule(golden_graph, gamma):
    G = golden_graph
    x = np.random.default_rng(0).standard_normal((G.N, 3))
    crits = []
    for opts in _rule_cases(G, x, gamma):
        dev, ref = _runs(G, x, gamma, **opts)
        _check(dev, ref)
        crits.append(dev[1]["crit"])
    assert crits == ["RTOL", "ATOL", "DTOL", "XTOL", "MAXIT"]


@pytest.mark.parametrize("nsig", [1, 2, 3, 4, 5, 8, 16, 17, 64, 256])
def test_every_lane_build(sensor2000, nsig):
    """Even widths run 16-byte lanes (1, 2, 4, ... 64 lanes per vertex, 256 columns two passes of 64), odd widths
    8-byte lanes."""
    G = sensor2000
    x = np.random.default_rng(nsig).standard_normal((G.N, nsig))
    dev, ref = _runs(G, x, 0.3, rtol=None, maxit=5)
    _check(dev, ref)
    assert dev[0].shape == (G.N, nsig)


def _path(n):
    return sparse.diags([np.arange(1.0, n), np.arange(1.0, n)], [1, -1]).tocsr()


def _edge_case_graphs():
    iso = sparse.lil_matrix((6, 6))
    for i, j, w in ((0, 1, 1.0), (1, 2, 0.5), (2, 4, 2.0), (4, 5, 1.5), (0, 5, 0.7)):  # vertex 3 has no edge
        iso[i, j] = iso[j, i] = w
    yield "isolated vertex", iso.tocsr()
    yield "path of 5", _path(5)  # vertex 0 is only a source, vertex 4 only a target
    yield "no edges", sparse.csr_matrix((4, 4))
    yield "one vertex", sparse.csr_matrix((1, 1))


@pytest.mark.parametrize("name,W", list(_edge_case_graphs()), ids=[n for n, _ in _edge_case_graphs()])
@pytest.mark.parametrize("nsig", [1, 2, 3])
def test_edge_cases_of_the_edge_walk(name, W, nsig):
    G = graphs.Graph(W)
    dev = G.device_graph(np.float64)
    D = dev.differential_operator()
    assert D.shape == (W.shape[0], sparse.triu(W, k=1).nnz)
    x = np.random.default_rng(5).standard_normal((W.shape[0], nsig))
    out, ref = _device_runs(dev, D, x, 0.4, 0.11)
    _check(out, ref)
    if D.shape[1] == 0:
        assert out[1]["niter"] == 1 and np.array_equal(out[0], x)
    out, ref = _device_runs(dev, D, x, 0.4, 0.11, rtol=None, maxit=6)
    _check(out, ref)
    out, ref = _device_runs(dev, D, x, 0.0, 0.11)  # gamma = 0: u stays 0, every objective is 0, the rule fires at once
    _check(out, ref)
    assert out[1]["niter"] == 1 and np.array_equal(out[0], x)


def test_vertex_count_off_the_group_size():
    G = _with_d(graphs.Sensor(1027, seed=3))
    x = np.random.default_rng(6).standard_normal((G.N, 4))
    _check(*_runs(G, x, 0.3))
    _check(*_runs(G, x[:, :3], 0.3, rtol=None, maxit=7))


@pytest.mark.parametrize("N", [10_000, 100_000])
def test_sensor_graphs_default_rule(N):
    G = _with_d(graphs.Sensor(N, seed=0))
    x = np.random.default_rng(N).standard_normal((N, 4))
    dev, ref = _runs(G, x, 0.5)
    _check(dev, ref)
    assert dev[1]["crit"] == "RTOL"


def test_directed_graph_and_self_loops():
    A = sparse.random(200, 200, 0.03, random_state=7, format="csr")
    A.setdiag(0)
    A.eliminate_zeros()
    Gd = _with_d(graphs.Graph(A), dense_lmax=True)
    assert Gd.is_directed() and Gd.D.shape == (200, A.nnz)
    S = sparse.random(200, 200, 0.02, random_state=8, format="csr")
    S = (S + S.T).tolil()
    S.setdiag(np.where(np.arange(200) % 7 == 0, 0.5, 0.0))
    S = S.tocsr()
    S.eliminate_zeros()
    Gl = _with_d(graphs.Graph(S), dense_lmax=True)
    assert not Gl.is_directed() and Gl.D.shape[1] == sparse.triu(S).nnz
    for G in (Gd, Gl):
        x = np.random.default_rng(9).standard_normal((200, 4))
        _check(*_runs(G, x, 0.2))
        _check(*_runs(G, x, 0.2, rtol=None, maxit=15))


def test_repeated_calls_give_identical_bits(sensor2000):
    G = sensor2000
    x = np.random.default_rng(11).standard_normal((G.N, 8))
    a = optimization.prox_tv_solve(x, 0.5, G, tol=None, maxit=40)
    b = optimization.prox_tv_solve(x, 0.5, G, tol=None, maxit=40)
    assert a[0].tobytes() == b[0].tobytes()
    assert a[1]["objective"].tobytes() == b[1]["objective"].tobytes()
    c = optimization.prox_tv_solve(x, 0.5, G)
    d = optimization.prox_tv_solve(x, 0.5, G)
    assert c[0].tobytes() == d[0].tobytes() and c[1]["niter"] == d[1]["niter"]
    assert c[1]["objective"].tobytes() == a[1]["objective"][:c[1]["niter"] + 1].tobytes()


def test_float32_graph_gives_the_float64_result():
    G64 = graphs.Sensor(5000, seed=2)
    G64.estimate_lmax()
    G32 = graphs.Sensor(5000, seed=2, compute_dtype=np.float32)
    G32._lmax = G64.lmax  # (the same step on both)
    x = np.random.default_rng(12).standard_normal((5000, 2))
    z64 = optimization.prox_tv(x, 0.3, G64)
    z32 = optimization.prox_tv(x, 0.3, G32)
    assert z32.dtype == np.float64 and z32.tobytes() == z64.tobytes()


def test_device_array_in_device_array_out(sensor2000):
    from pygsp_amd import engine
    G = sensor2000
    x = np.random.default_rng(13).standard_normal((G.N, 6))
    z, info = optimization.prox_tv_solve(x, 0.3, G)
    zd, infod = optimization.prox_tv_solve(G.to_device(x, np.float64), 0.3, G)
    assert isinstance(zd, engine.DeviceArray) and zd.shape == x.shape
    assert np.asarray(zd).tobytes() == z.tobytes() and infod["niter"] == info["niter"]
    z1 = optimization.prox_tv(G.to_device(x[:, 0], np.float64), 0.3, G)
    assert isinstance(z1, engine.DeviceArray) and z1.shape == (G.N,)
    assert np.asarray(z1).tobytes() == optimization.prox_tv(x[:, 0], 0.3, G).tobytes()


@pytest.mark.parametrize("gamma", [0.05, 0.5])
def test_tight_solve_closes_the_duality_gap(golden_graph, gamma):
    G = golden_graph
    x = np.random.default_rng(0).standard_normal((G.N, 3))
    z, info = optimization.prox_tv_solve(x, gamma, G, tol=None, xtol=1e-13, maxit=400000)
    assert info["crit"] == "XTOL"
    gap = th.duality_gap(x, z, gamma, G.D)
    print("niter", info["niter"], "gap", gap, "objective", info["objective"][-1])
    assert gap <= 1e-9 * info["objective"][-1]


def test_entry_point_errors(sensor2000):
    G = sensor2000
    dev = G.device_graph(np.float64)
    dev32 = graphs.Graph(_path(5), compute_dtype=np.float32).device_graph(np.float32)
    with dev.ctx._temporaries() as t:
        b = t.alloc(G.N * 8 * 4)
        with pytest.raises(ValueError, match="float32"):
            dev32.prox_tv_dev(b.ptr, b.ptr, 1, 0.1, 0.1)
        with pytest.raises(ValueError, match="signals"):
            dev.prox_tv_dev(b.ptr, b.ptr, 0, 0.1, 0.1)
        with pytest.raises(ValueError, match="signals"):
            dev.prox_tv_dev(b.ptr, b.ptr, 257, 0.1, 0.1)
        with pytest.raises(ValueError, match="step"):
            dev.prox_tv_dev(b.ptr, b.ptr, 4, 0.1, 0.0)
        with pytest.raises(ValueError, match="step"):
            dev.prox_tv_dev(b.ptr, b.ptr, 4, 0.1, -1.0)
        with pytest.raises(ValueError, match="NaN"):
            dev.prox_tv_dev(b.ptr, b.ptr, 4, 0.1, 0.1, xtol=float("nan"))
    with pytest.raises(ValueError, match="float64"):
        dev32.prox_tv(np.zeros(5), 0.1, 0.1)


def test_refusals_that_need_a_graph():
    """The two shared refusals that the host test cannot reach, word for word as before the solvers shared one argument
    check: a float32 graph, and a panel past 2 GiB (N > 1048544 at 256 columns; it fires before anything is allocated
    or read, so a small buffer stands in for both panels)."""
    n = 1_048_600
    big = graphs.Graph(sparse.diags([np.ones(n - 1), np.ones(n - 1)], [1, -1]).tocsr()).device_graph(np.float64)
    small32 = graphs.Graph(_path(5), compute_dtype=np.float32).device_graph(np.float32)
    for dev, nsig, text in (
            (small32, 1, "prox_tv: the graph computes in float32; the solver needs the float64 graph"),
            (big, 256, "prox_tv: an N x Nsig or n_edges x Nsig panel exceeds 2 GiB")):
        with dev.ctx._temporaries() as t:
            b = t.alloc(4096)
            with pytest.raises(ValueError) as e:
                dev.prox_tv_dev(b.ptr, b.ptr, nsig, 0.1, 0.1)
        assert str(e.value) == text


@pytest.mark.skipif(importlib.util.find_spec("pygsp") is None, reason="needs an importable pygsp next to the GPU")
def test_real_pygsp_through_the_seam():
    import pygsp

    from pygsp_amd import plugin
    G = pygsp.graphs.Sensor(500, seed=0)
    G.estimate_lmax()
    G.compute_differential_operator()
    x = np.random.default_rng(0).standard_normal((G.N, 3))
    plugin.install(pygsp, optimization=True)
    try:
        z = pygsp.optimization.prox_tv(x, 0.1, G)
    finally:
        plugin.uninstall(pygsp)
    zr, _ = th.solve(sparse.csc_matrix(G.D, dtype=np.float64), x, 0.1, 1.0 / (2.0 * G.lmax))
    assert np.abs(z - zr).max() < 1e-10
