"""The numpy restatements behind graph coarsening (reduction.heavy_edge_matching_host, reduction.coarsen_host,
reduction.parent_of) on hand-worked cases and on their properties, and the argument errors that need no device.  The
GPU tests (tests/test_gpu_z_coarsen.py) compare the device with these restatements exactly."""
import numpy as np
import pytest
from scipy import sparse

import coarsen_helpers as ch
from pygsp_amd import engine, reduction

METRICS = ("normalized_cut", "weight")


def pairs_of(mate):
    return sorted((int(i), int(m)) for i, m in enumerate(mate) if i < m)


@pytest.mark.parametrize("metric", METRICS)
def test_two_and_three_vertex_paths(metric):
    mate, rounds, pairs = reduction.heavy_edge_matching_host(ch.path(2), metric=metric)
    assert mate.tolist() == [1, 0] and (rounds, pairs) == (1, 1)
    # equal scores on both edges: the middle vertex proposes to the smaller index
    mate, rounds, pairs = reduction.heavy_edge_matching_host(ch.path(3), metric=metric)
    assert mate.tolist() == [1, 0, 2] and (rounds, pairs) == (1, 1)
    # a heavier second edge wins under both metrics: 0.5 (2 + 1/2.5) = 1.2 < 2 (1/2.5 + 1/2) = 1.8
    mate, _, _ = reduction.heavy_edge_matching_host(ch.path(3, [0.5, 2.0]), metric=metric)
    assert mate.tolist() == [0, 2, 1]


@pytest.mark.parametrize("metric", METRICS)
def test_triangle_tie_break(metric):
    mate, rounds, pairs = reduction.heavy_edge_matching_host(ch.triangle(), metric=metric)
    assert mate.tolist() == [1, 0, 2] and (rounds, pairs) == (1, 1)


@pytest.mark.parametrize("metric", METRICS)
def test_star_matches_exactly_one_pair(metric):
    mate, rounds, pairs = reduction.heavy_edge_matching_host(ch.star(5), metric=metric)
    assert pairs_of(mate) == [(0, 1)] and (rounds, pairs) == (1, 1)
    W = ch.star(40, seed=3)
    mate, rounds, pairs = reduction.heavy_edge_matching_host(W, metric="weight")
    assert pairs_of(mate) == [(0, 1 + int(np.argmax(W[0].toarray().ravel()[1:])))] and (rounds, pairs) == (1, 1)


@pytest.mark.parametrize("metric", METRICS)
def test_ring_of_seven(metric):
    mate, rounds, pairs = reduction.heavy_edge_matching_host(ch.ring(7), metric=metric)
    assert pairs_of(mate) == [(0, 1), (2, 3), (4, 5)] and mate[6] == 6 and (rounds, pairs) == (3, 3)


def test_increasing_path_needs_half_as_many_rounds_as_vertices():
    W = ch.increasing_path(64)
    mate, rounds, pairs = reduction.heavy_edge_matching_host(W, metric="weight")
    assert (rounds, pairs) == (32, 32)
    assert pairs_of(mate) == [(k, k + 1) for k in range(0, 64, 2)]
    # stopped after one round: the far pair alone, the rest singletons
    mate, rounds, pairs = reduction.heavy_edge_matching_host(W, metric="weight", max_rounds=1)
    assert pairs_of(mate) == [(62, 63)] and (rounds, pairs) == (1, 1)
    mate, rounds, pairs = reduction.heavy_edge_matching_host(W, metric="weight", max_rounds=0)
    assert mate.tolist() == list(range(64)) and (rounds, pairs) == (0, 0)


@pytest.mark.parametrize("metric", METRICS)
def test_isolated_vertices_stay_single(metric):
    W = ch.with_isolated()
    mate, rounds, pairs = reduction.heavy_edge_matching_host(W, metric=metric)
    assert pairs_of(mate) == [(2, 4), (7, 8)] and (rounds, pairs) == (1, 2)
    parent, nc = reduction.parent_of(mate)
    assert parent.tolist() == [0, 1, 2, 3, 2, 4, 5, 6, 6] and nc == 7
    Wc = reduction.coarsen_host(W, parent)
    assert Wc.shape == (7, 7) and pairs_of_matrix(Wc) == {(1, 2): 0.5, (2, 4): 1.0}
    # an edgeless graph: nothing matches, every vertex is its own cluster
    mate, rounds, pairs = reduction.heavy_edge_matching_host(sparse.csr_matrix((5, 5)), metric=metric)
    assert mate.tolist() == [0, 1, 2, 3, 4] and (rounds, pairs) == (0, 0)
    assert reduction.coarsen_host(sparse.csr_matrix((5, 5)), np.arange(5)).nnz == 0


def pairs_of_matrix(W):
    C = sparse.triu(W).tocoo()
    return {(int(r), int(c)): float(v) for r, c, v in zip(C.row, C.col, C.data)}


def test_self_loops_are_no_candidates_and_leave_no_diagonal():
    W = ch.path(3).tolil()
    W[2, 2] = 50.0
    W = W.tocsr()
    mate, _, _ = reduction.heavy_edge_matching_host(W)
    assert mate.tolist() == [1, 0, 2]
    Wc = reduction.coarsen_host(W, reduction.parent_of(mate)[0])
    assert Wc.toarray().tolist() == [[0.0, 1.0], [1.0, 0.0]]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", ["ring7", "increasing_path64", "isolated", "random", "hub", "two_hubs"])
def test_properties_of_matching_and_coarse_graph(case, metric):
    if case == "random":
        W = ch.random_simple(400, 6, seed=5)
    elif case == "hub":
        W = ch.star(150, seed=1) + sparse.block_diag([sparse.csr_matrix((1, 1)), ch.random_simple(150, 4, seed=2)])
        W = sparse.csr_matrix(W)
    elif case == "two_hubs":
        W = ch.two_hubs()
    else:
        W = ch.HAND_CASES[case]()
    levels = ch.host_levels(W, 3, metric)
    for mate, rounds, pairs, parent, nc, Wc in levels:
        ch.check_matching(W, mate, pairs)
        ch.check_maximal(W, mate)
        ch.check_parent(mate, parent, nc)
        assert nc == W.shape[0] - pairs and Wc.shape == (nc, nc)
        ch.check_coarse(Wc, W, parent)
        assert abs(Wc.sum() - (W.sum() - 2 * sum(W[i, m] for i, m in enumerate(mate) if i < m))) <= 1e-12 * W.sum()
        W = Wc


def test_coarsen_host_takes_clusters_of_any_size():
    ptr, idx, parent = ch.mixed_partition(40, seed=2)
    W = ch.random_simple(parent.size, 8, seed=9)
    ch.check_coarse(reduction.coarsen_host(W, parent), W, parent)


def test_given_degrees_change_the_scores():
    """d is what the scores divide by: with d = 1 everywhere the normalized cut orders edges as the weights do."""
    W = ch.random_simple(200, 5, seed=4)
    a = reduction.heavy_edge_matching_host(W, np.ones(200), "normalized_cut")
    b = reduction.heavy_edge_matching_host(W, None, "weight")
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def test_argument_errors():
    directed = sparse.csr_matrix(np.array([[0, 1.0], [0, 0]]))
    with pytest.raises(ValueError):
        reduction.heavy_edge_matching_host(directed)
    with pytest.raises(ValueError):
        reduction.coarsen_host(directed, np.zeros(2, dtype=int))
    with pytest.raises(ValueError):
        reduction.heavy_edge_matching_host(ch.path(3), metric="cut")
    with pytest.raises(ValueError):
        reduction.heavy_edge_matching_host(ch.path(3), max_rounds=-1)
    with pytest.raises(ValueError):
        reduction.heavy_edge_matching_host(ch.path(3), d=np.ones(2))
    for parent in (np.zeros(2, dtype=int), np.array([0, 1, 3]), np.array([0, -1, 1]), np.array([0.0, 1.0, 1.0]),
                   np.zeros((3, 1), dtype=int)):
        with pytest.raises(ValueError):
            reduction.coarsen_host(ch.path(3), parent)
    with pytest.raises(ValueError):
        engine.check_parent([0, 2, 2], 3, 3)  # cluster 1 has no member
    with pytest.raises(ValueError):
        engine.check_parent([0, 1, 2], 3, 2)

    class Directed:
        lap_type, N = "combinatorial", 2

        def is_directed(self):
            return True

    with pytest.raises(ValueError):
        reduction.coarsen(Directed())
    with pytest.raises(ValueError):
        reduction.coarsen(Directed(), metric="cut")
    with pytest.raises(TypeError):
        reduction.coarsen(ch.path(3))


def test_pooling_restatement_on_a_worked_example():
    ptr, idx = np.array([0, 2, 3, 6]), np.array([1, 4, 0, 2, 3, 5])
    x = np.array([[5.0], [1.0], [2.0], [2.0], [3.0], [-1.0]])
    assert ch.pool_host(ptr, idx, x, "max").ravel().tolist() == [3.0, 5.0, 2.0]
    assert ch.pool_host(ptr, idx, x, "sum").ravel().tolist() == [4.0, 5.0, 3.0]
    assert ch.pool_host(ptr, idx, x, "mean").ravel().tolist() == [2.0, 5.0, 1.0]
    g = np.array([[10.0], [20.0], [30.0]])
    # tied maxima (rows 2 and 3 of the last segment): the first member alone receives the cotangent
    assert ch.pool_vjp_host(ptr, idx, g, x, "max").ravel().tolist() == [20.0, 0.0, 30.0, 0.0, 10.0, 0.0]
    assert ch.pool_vjp_host(ptr, idx, g, None, "sum").ravel().tolist() == [20.0, 10.0, 30.0, 30.0, 10.0, 30.0]
    assert ch.pool_vjp_host(ptr, idx, g, None, "mean").ravel().tolist() == [20.0, 5.0, 10.0, 10.0, 5.0, 10.0]


def test_segments_are_checked_on_the_host():
    class NoDevice:
        def upload(self, a):
            return a

    seg = engine.Segments.from_parent(NoDevice(), [1, 0, 1, 2, 0], 3)
    assert seg.ptr.tolist() == [0, 2, 4, 5] and seg.idx.tolist() == [1, 4, 0, 2, 3] and seg.sizes.tolist() == [2, 2, 1]
    for ptr, idx in (([0, 2, 2, 3], [0, 1, 2]),      # an empty segment
                     ([0, 2, 3], [1, 0, 2]),         # members do not ascend
                     ([0, 2, 3], [0, 0, 2]),         # a row twice
                     ([0, 2, 4], [0, 1, 2]),         # ptr past idx
                     ([1, 2, 3], [0, 1, 2])):
        with pytest.raises(ValueError):
            engine.Segments(NoDevice(), ptr, idx)
