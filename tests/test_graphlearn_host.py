"""CPU tests of graph learning: the numpy restatement (graphlearn_helpers) against the optimality conditions of the
problem it claims to solve, the theta interval against the closed-form single-vertex solution, and the argument errors
of pygsp_amd.graph_learning that need no device."""
import numpy as np
import pytest

import graphlearn_helpers as gl
from pygsp_amd import graph_learning


@pytest.fixture(scope="module", params=[64, 300])
def solved(request):
    """Sensor-like points, a k-NN pattern, z of mean 1; the restatement at tol 1e-9 in float64 and in longdouble."""
    N = request.param
    _, src, dst, z = gl.sensor_like(N, 8, seed=N)
    gamma = gl.gamma_for(src, dst, N, 1.0)
    out = {}
    for dtype in (np.float64, np.longdouble):
        P, _, info = gl.solve(src, dst, N, z, 1.0, 1.0, gamma, tol=1e-9, maxit=20000, dtype=dtype)
        assert info["crit"] == "TOL"
        out[dtype] = (P, info)
    return N, src, dst, z, out


def test_restatement_meets_the_optimality_conditions(solved):
    """At tol 1e-9 the projected gradient (the gradient on the positive entries of P, its negative part on the zero
    entries) is as small as longdouble arithmetic makes it on the same input, within a factor 10."""
    N, src, dst, z, out = solved
    res = {}
    for dtype, (P, info) in out.items():
        assert P.min() >= 0 and np.count_nonzero(P == 0) > 0  # feasible, with exact zeros
        res[dtype] = float(np.max(np.abs(gl.kkt_residual(src, dst, N, z, 1.0, 1.0, P))))
        print("N = {}: {} iterations in {}, KKT residual {:.3e}".format(N, info["niter"], np.dtype(dtype).name,
                                                                         res[dtype]))
    assert res[np.float64] <= 10 * res[np.longdouble]
    # and the two runs stop at the same iteration, bits apart
    assert out[np.float64][1]["niter"] == out[np.longdouble][1]["niter"]


def test_scaling_law(solved):
    """P(z, a, b) = sqrt(a / b) P(z / sqrt(a b), 1, 1).  Both sides are feasible points of 2b- resp. 2-strongly convex
    problems, so each lies within ||projected gradient||_2 / (2 b) of its solution: the bound asserted is the sum of the
    two, the agreement measured is printed."""
    N, src, dst, z, _ = solved
    a, b = 2.5, 0.4
    c = np.sqrt(a / b)
    P1, _, i1 = gl.solve(src, dst, N, z, a, b, gl.gamma_for(src, dst, N, b), tol=1e-9, maxit=50000)
    P2, _, i2 = gl.solve(src, dst, N, z / np.sqrt(a * b), 1.0, 1.0, gl.gamma_for(src, dst, N, 1.0), tol=1e-9,
                         maxit=50000)
    assert i1["crit"] == i2["crit"] == "TOL"
    r1 = np.linalg.norm(gl.kkt_residual(src, dst, N, z, a, b, P1))
    r2 = np.linalg.norm(gl.kkt_residual(src, dst, N, z / np.sqrt(a * b), 1.0, 1.0, P2))
    bound = r1 / (2 * b) + c * r2 / 2
    diff = np.linalg.norm(P1 - c * P2)
    print("N = {}: ||P(z, a, b) - c P(z / sqrt(ab), 1, 1)||_2 = {:.3e} (bound {:.3e}), max |P| = {:.3f}".format(
        N, diff, bound, P1.max()))
    assert diff <= bound
    assert np.array_equal(P1 > 0, P2 > 0) or diff < 1e-6 * P1.max()


def test_isolated_vertices_take_no_part():
    src, dst = np.array([0, 1]), np.array([1, 3])  # vertex 2 of 5 and vertex 4 have no edge
    P, w, info = gl.solve(src, dst, 5, np.array([0.5, 1.0]), 1.0, 1.0, gl.gamma_for(src, dst, 5, 1.0), tol=1e-9)
    assert info["crit"] == "TOL" and np.all(info["v"][[2, 4]] == 0) and np.all(np.isfinite(P)) and P.min() > 0


def test_theta_interval_keeps_exactly_k_edges():
    """For random sorted rows and 2 <= k < m the closed-form single-vertex solution at sqrt(lo hi) has exactly k
    positive entries."""
    rng = np.random.default_rng(5)
    for trial in range(2000):
        m = int(rng.integers(3, 30))
        k = int(rng.integers(2, m))
        D = np.sort(rng.uniform(0.01, 1.0, (1, m)) ** rng.uniform(0.5, 3), axis=1)
        lo, hi, ok = gl.theta_bounds_rows(D, k)
        assert ok[0] and lo[0] < hi[0]
        w = gl.single_vertex_solution(D[0] ** 2, np.sqrt(lo[0] * hi[0]), k)
        assert np.count_nonzero(w > 0) == k, (trial, m, k)


def test_theta_bounds_matches_its_restatement_and_refuses_bad_input():
    rng = np.random.default_rng(6)
    D = np.sort(rng.uniform(0.1, 1.0, (50, 12)), axis=1)
    D[7] = 0.3  # a row without a positive radicand is left out
    for k in (2, 5, 11):
        np.testing.assert_allclose(graph_learning.theta_bounds(D, k), gl.theta_bounds(D, k), rtol=1e-13)
        lo, hi = graph_learning.theta_bounds(D, k)
        assert 0 < lo < hi
    with pytest.raises(ValueError):
        graph_learning.theta_bounds(np.full((4, 6), 0.5), 3)
    for bad_k in (1, 12, 13):
        with pytest.raises(ValueError):
            graph_learning.theta_bounds(D, bad_k)
    with pytest.raises(ValueError):
        graph_learning.theta_bounds(D[0], 3)


class _Pattern:
    """What learn_weights asks of a graph before it touches the device."""
    compute_dtype = np.dtype(np.float64)
    n_vertices, n_edges = 4, 3

    def is_directed(self):
        return False


@pytest.mark.parametrize("kwargs", [dict(a=0.0), dict(a=-1.0), dict(a=np.inf), dict(b=-0.1), dict(step=0.0),
                                    dict(step=1.0), dict(step=1.5), dict(theta=0.0), dict(theta=np.nan)])
def test_learn_weights_refuses_bad_parameters(kwargs):
    with pytest.raises(ValueError):
        graph_learning.learn_weights(_Pattern(), Z=np.ones(3), **kwargs)


def test_learn_weights_wants_exactly_one_of_x_and_z():
    with pytest.raises(ValueError, match="exactly one"):
        graph_learning.learn_weights(_Pattern())
    with pytest.raises(ValueError, match="exactly one"):
        graph_learning.learn_weights(_Pattern(), np.ones((4, 2)), Z=np.ones(3))


def test_learn_weights_refuses_float32_and_directed_graphs():
    f32 = _Pattern()
    f32.compute_dtype = np.dtype(np.float32)
    with pytest.raises(ValueError, match="float64"):
        graph_learning.learn_weights(f32, Z=np.ones(3))
    directed = _Pattern()
    directed.is_directed = lambda: True
    with pytest.raises(ValueError, match="directed"):
        graph_learning.learn_weights(directed, Z=np.ones(3))


@pytest.mark.parametrize("kwargs", [dict(k=5, candidates=5), dict(k=5, candidates=4), dict(k=30, candidates=65),
                                    dict(k=1), dict(k=5, a=0.0), dict(k=5, b=-1.0), dict(k=20, candidates=60)])
def test_learned_graph_refuses_bad_arguments_before_the_device(kwargs):
    X = np.random.default_rng(0).uniform(0, 1, (50, 2))
    with pytest.raises(ValueError):
        graph_learning.LearnedGraph(X, **kwargs)  # (the last one: 50 points cannot have 60 candidates each)


def test_learned_graph_is_exported_from_graphs():
    from pygsp_amd import graphs
    assert graphs.LearnedGraph is graph_learning.LearnedGraph
