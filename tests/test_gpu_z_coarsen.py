"""Graph coarsening and pooling on the device (gspx_match_heavy_edges, gspx_coarsen_build, gspx_segment_pool_dev and
its vjp, pygsp_amd.reduction.coarsen, pygsp_amd.nn.GraphPool).

Matching: the device's mate, round count and pair count equal reduction.heavy_edge_matching_host EXACTLY, the
restatement scoring with the device's own download_dw(); with and without an internal vertex order, which must agree.
Coarse graph: indptr, indices and data equal reduction.coarsen_host bit for bit.  Pooling: equal to the numpy restatement
of tests/coarsen_helpers.py bit for bit in both dtypes.  The torch functions run in a fresh child process
(tests/coarsen_child.py) that imports pygsp_amd.nn first."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import sparse

import coarsen_helpers as ch
from conftest import rel_err
from oracle import cheby_oracle as orc
from pygsp_amd import engine, filters, graphs, reduction
from test_gpu_4_ops import TOL as OPS_TOL

pytestmark = pytest.mark.gpu

F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
METRICS = ("normalized_cut", "weight")
MODES = ("max", "mean", "sum")
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "coarsen_child.py")

CASES = dict(ch.HAND_CASES)
CASES.update({
    "star1000": lambda: ch.star(1000, seed=7),        # a hub row longer than a wave and than a workgroup
    "star1000_equal": lambda: ch.star(1000),          # ... every score tied: the tie-break across lanes
    "two_hubs": ch.two_hubs,                           # long coarse rows whose entries are sums
    "sensor300": lambda: graphs.Sensor(300, seed=3).W,
    "random3000": lambda: ch.random_simple(3000, 8, seed=11),  # several workgroups
})
WS = {}


def adjacency(case):
    if case not in WS:
        WS[case] = sparse.csr_matrix(CASES[case](), dtype=np.float64)
    return WS[case]


@pytest.fixture(scope="module")
def devices():
    """One float64 DeviceGraph per (case, permuted or not), destroyed at the end of the module."""
    ctx = engine.default_context(0)
    made = {}

    def get(case, permuted):
        if (case, permuted) not in made:
            W = adjacency(case)
            perm = np.random.default_rng(5).permutation(W.shape[0]).astype(np.int32) if permuted else None
            made[case, permuted] = engine.DeviceGraph.from_w(W, dtype=np.float64, perm=perm, ctx=ctx)
        return made[case, permuted]

    yield get
    for dev in made.values():
        dev.destroy()


# ---- matching -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_matching_equals_the_restatement(devices, case, metric):
    W = adjacency(case)
    seen = []
    for permuted in (False, True):
        dev = devices(case, permuted)
        mate, info = dev.match_heavy_edges(metric)
        ref, rounds, pairs = reduction.heavy_edge_matching_host(W, dev.download_dw(), metric)
        print("%s %s perm=%d: N %d, rounds %d, pairs %d, %.3f ms" % (case, metric, permuted, W.shape[0], info["rounds"],
                                                                     info["pairs"], info["kernel_ms"]))
        assert np.array_equal(mate, ref), (case, metric, permuted, np.flatnonzero(mate != ref)[:10])
        assert (info["rounds"], info["pairs"]) == (rounds, pairs)
        assert info["singletons"] == W.shape[0] - 2 * pairs
        ch.check_matching(W, mate, pairs)
        ch.check_maximal(W, mate)
        seen.append(mate)
    assert np.array_equal(seen[0], seen[1])  # the internal order plays no part


def test_matching_hand_results(devices):
    assert devices("triangle", False).match_heavy_edges()[0].tolist() == [1, 0, 2]
    mate, info = devices("star5", True).match_heavy_edges()
    assert mate.tolist() == [1, 0, 2, 3, 4, 5] and (info["rounds"], info["pairs"]) == (1, 1)
    mate, info = devices("ring7", False).match_heavy_edges("weight")
    assert mate.tolist() == [1, 0, 3, 2, 5, 4, 6] and (info["rounds"], info["pairs"]) == (3, 3)
    mate, info = devices("increasing_path64", True).match_heavy_edges("weight")
    assert (info["rounds"], info["pairs"], info["singletons"]) == (32, 32, 0)


@pytest.mark.parametrize("max_rounds", [0, 1, 5])
def test_max_rounds_on_the_increasing_path(devices, max_rounds):
    W = adjacency("increasing_path64")
    for permuted in (False, True):
        dev = devices("increasing_path64", permuted)
        mate, info = dev.match_heavy_edges("weight", max_rounds=max_rounds)
        ref, rounds, pairs = reduction.heavy_edge_matching_host(W, dev.download_dw(), "weight", max_rounds)
        assert np.array_equal(mate, ref) and (info["rounds"], info["pairs"]) == (rounds, pairs) == (max_rounds,) * 2
        ch.check_matching(W, mate, pairs)


def test_matching_argument_errors(devices):
    dev = devices("path3", False)
    with pytest.raises(ValueError):
        dev.match_heavy_edges("cut")
    with pytest.raises(ValueError):
        dev.match_heavy_edges(max_rounds=-2)
    f32 = engine.DeviceGraph.from_w(adjacency("path3"), dtype=np.float32, ctx=dev.ctx)
    normalized = engine.DeviceGraph.from_w(adjacency("path3"), "normalized", ctx=dev.ctx)
    try:
        with pytest.raises(ValueError):
            f32.match_heavy_edges()
        with pytest.raises(ValueError):
            normalized.match_heavy_edges()
        with pytest.raises(ValueError):
            normalized.coarsen([0, 0, 1], 2)
    finally:
        f32.destroy()
        normalized.destroy()
    for parent, nc in (([0, 0], 1), ([0, 0, 2], 2), ([0, 0, 2], 3), ([0, -1, 1], 2)):
        with pytest.raises(ValueError):
            dev.coarsen(parent, nc)


# ---- coarse graph ---------------------------------------------------------------------------------------------------
def same_bits(A, B):
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(A.data, B.data))


@pytest.mark.parametrize("case", sorted(CASES))
def test_coarse_graph_equals_the_restatement_bit_for_bit(devices, case):
    W = adjacency(case)
    for permuted in (False, True):
        dev = devices(case, permuted)
        mate, _ = dev.match_heavy_edges()
        parent, nc = reduction.parent_of(mate)
        ch.check_parent(mate, parent, nc)
        Wd, info = dev.coarsen(parent, nc)
        assert Wd.shape == (nc, nc)
        Wc = Wd.download()
        ref = reduction.coarsen_host(W, parent)
        print("%s perm=%d: %d -> %d vertices, %d -> %d entries, %.3f ms" % (case, permuted, W.shape[0], nc, W.nnz, Wc.nnz,
                                                                            info["kernel_ms"]))
        assert same_bits(Wc, ref), (case, permuted)
        assert same_bits(Wc, sparse.csr_matrix(Wc.T))
        ch.check_coarse(Wc, W, parent)


def test_coarse_graph_of_clusters_of_any_size(devices):
    """Clusters of one to eight members, and the whole graph in one cluster: the same kernels, the same bits."""
    W = adjacency("random3000")
    dev = devices("random3000", True)
    parent = np.unique(np.random.default_rng(8).integers(0, 1100, 3000), return_inverse=True)[1].astype(np.int32)
    nc = int(parent.max()) + 1
    assert np.bincount(parent).min() == 1 and np.bincount(parent).max() >= 5
    Wc = dev.coarsen(parent, nc)[0].download()
    assert same_bits(Wc, reduction.coarsen_host(W, parent)) and same_bits(Wc, sparse.csr_matrix(Wc.T))
    ref = ch.scipy_coarse(W, parent)  # (up to 8 x 8 terms per entry: n eps with n <= 64 on either side)
    assert np.array_equal(Wc.indices, ref.indices) and np.max(np.abs(Wc.data - ref.data) / ref.data) <= 128 * 2.0 ** -53
    one = dev.coarsen(np.zeros(3000, dtype=np.int32), 1)[0]
    assert one.shape == (1, 1) and one.nnz == 0


@pytest.fixture(scope="module")
def sensor_levels():
    G = graphs.Sensor(300, seed=3)
    return G, reduction.coarsen(G, levels=2)


def test_two_levels_of_a_sensor_graph(sensor_levels):
    G, C = sensor_levels
    assert C.graphs[0] is G and len(C.graphs) == 3 and len(C.parents) == 2 and len(C.info) == 2
    for level in range(2):
        fine, coarse = C.graphs[level], C.graphs[level + 1]
        d = fine.device_graph(np.float64).download_dw()
        mate, rounds, pairs = reduction.heavy_edge_matching_host(fine.W, d)
        parent, nc = reduction.parent_of(mate)
        assert np.array_equal(C.parents[level], parent) and C.parents[level].dtype == np.int32
        info = C.info[level]
        assert (info["rounds"], info["pairs"], info["singletons"]) == (rounds, pairs, fine.N - 2 * pairs)
        assert info["kernel_ms"] > 0 and coarse.N == nc
        assert same_bits(sparse.csr_matrix(coarse.W), reduction.coarsen_host(fine.W, parent))
        assert coarse.lap_type == fine.lap_type and coarse.compute_dtype == fine.compute_dtype
        assert coarse.plotting.keys() == fine.plotting.keys() and all(coarse.plotting[k] is fine.plotting[k] for k in fine.plotting)
        want = np.stack([np.asarray(fine.coords)[parent == c].mean(axis=0) for c in range(nc)])
        assert np.array_equal(coarse.coords, want)
    composed = C.parents[1][C.parents[0]]
    assert np.array_equal(C.parent(0, 2), composed)
    seg = C.segments(0, 2)
    assert seg is C.segments(0, None) and seg.n_fine == 300 and seg.n_coarse == C.graphs[2].N
    assert 1 <= seg.sizes.min() and seg.sizes.max() <= 4 and np.array_equal(composed[seg.idx], np.repeat(
        np.arange(seg.n_coarse), seg.sizes))


def test_heat_filter_on_the_coarse_graph(sensor_levels):
    _, C = sensor_levels
    for G1 in C.graphs[1:]:
        G1.estimate_lmax()
        x = np.random.default_rng(G1.N).standard_normal((G1.N, 5))
        y = filters.Heat(G1, 10).filter(x, method="chebyshev", order=30)
        ref = orc.filter_chebyshev(orc.laplacian(G1.W), G1.lmax, [orc.heat_kernel(10, G1.lmax)], x, 30)
        err = rel_err(y, ref)
        print("Heat on G with %d vertices: deviation %.2e" % (G1.N, err))
        assert err < OPS_TOL[F64]


def test_normalized_laplacian_and_float32_are_carried_over():
    G = graphs.Sensor(120, seed=2, lap_type="normalized", compute_dtype=np.float32)
    C = reduction.coarsen(G, levels=1, metric="weight")
    G1 = C.graphs[1]
    assert G1.lap_type == "normalized" and G1.compute_dtype == np.float32
    mate, rounds, pairs = reduction.heavy_edge_matching_host(G.W, None, "weight")
    parent, _ = reduction.parent_of(mate)
    assert np.array_equal(C.parents[0], parent) and same_bits(sparse.csr_matrix(G1.W), reduction.coarsen_host(G.W, parent))


def test_a_level_that_matches_nothing():
    G = graphs.Graph(sparse.csr_matrix((6, 6), dtype=np.float64))
    C = reduction.coarsen(G, levels=2)
    for level in range(2):
        assert C.parents[level].tolist() == list(range(6))
        assert (C.info[level]["rounds"], C.info[level]["pairs"], C.info[level]["singletons"]) == (0, 0, 6)
        assert C.graphs[level + 1].N == 6 and C.graphs[level + 1].W.nnz == 0
    x = np.arange(12.0).reshape(6, 2)
    assert np.array_equal(C.pool(x), x) and np.array_equal(C.unpool(x, 0, 1), x)
    # a graph whose edges are all matched away: the next level has no edge left and still comes back
    C = reduction.coarsen(graphs.Graph(ch.from_edges(4, [(0, 1, 1.0), (2, 3, 2.0)])), levels=2)
    assert [g.N for g in C.graphs] == [4, 2, 2] and C.graphs[2].W.nnz == 0 and C.parents[1].tolist() == [0, 1]
    with pytest.raises(ValueError):
        reduction.coarsen(graphs.Graph(sparse.csr_matrix(np.array([[0, 1.0], [0, 0]]))))


# ---- pooling --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def partitions(sensor_levels):
    """name -> (engine.Segments, ptr, idx): mixed sizes 1..4 over several workgroups, the composed two-level table of a
    real coarsening, and one segment that holds every row."""
    ctx = engine.default_context(0)
    _, C = sensor_levels
    out = {}
    ptr, idx, _ = ch.mixed_partition(300, seed=4)
    out["mixed"] = (engine.Segments(ctx, ptr, idx), ptr, idx)
    seg = C.segments(0, 2)
    out["composed"] = (seg, seg.ptr, seg.idx)
    out["one"] = (engine.Segments(ctx, [0, 5], np.arange(5)), np.array([0, 5]), np.arange(5))
    return out


def panel(rows, width, dtype, seed, ties=False):
    rng = np.random.default_rng(seed)
    if ties:  # few distinct values: most segments hold their maximum more than once
        return rng.integers(0, 2, (rows, width)).astype(dtype)
    return rng.standard_normal((rows, width)).astype(dtype)


@pytest.mark.parametrize("dtype", [F64, F32], ids=str)
@pytest.mark.parametrize("width", [1, 3, 16, 64, 65, 200])
@pytest.mark.parametrize("name", ["mixed", "composed", "one"])
def test_pooling_equals_the_restatement_exactly(partitions, name, width, dtype):
    seg, ptr, idx = partitions[name]
    ctx = seg.ctx
    for ties in (False, True):
        x = panel(seg.n_fine, width, dtype, width + ties, ties)
        g = panel(seg.n_coarse, width, dtype, 1000 + width)
        for mode in MODES:
            y = engine.segment_pool(ctx, seg, x, mode)
            ref = ch.pool_host(ptr, idx, x, mode)
            assert y.dtype == dtype and y.shape == ref.shape and np.array_equal(y, ref), (name, width, mode, ties)
            gx = engine.segment_pool_vjp(ctx, seg, g, x if mode == "max" else None, mode)
            gref = ch.pool_vjp_host(ptr, idx, g, x, mode)
            assert gx.dtype == dtype and gx.shape == gref.shape and np.array_equal(gx, gref), (name, width, mode, ties)
            if mode == "max" and ties:  # one member per segment and column receives the cotangent, the first maximum
                assert np.array_equal(ch.pool_host(ptr, idx, (gx != 0).astype(dtype), "sum"), (g != 0).astype(dtype))
        up = engine.segment_unpool(ctx, seg, g)
        assert np.array_equal(up, ch.pool_vjp_host(ptr, idx, g, None, "sum"))
        assert np.array_equal(engine.segment_pool(ctx, seg, up, "max"), g)  # pool(unpool(y)) = y
        parent = np.empty(seg.n_fine, dtype=np.int64)
        parent[idx] = np.repeat(np.arange(seg.n_coarse), np.diff(ptr))
        assert np.array_equal(engine.segment_unpool(ctx, seg, engine.segment_pool(ctx, seg, x, "sum")),
                              ch.pool_host(ptr, idx, x, "sum")[parent])


@pytest.mark.parametrize("dtype", [F64, F32], ids=str)
def test_pooling_device_arrays_and_other_shapes(sensor_levels, dtype):
    """numpy arrays and engine.DeviceArray give the same bits: (N,), (N, S) and the feature planes of (N, S, F)."""
    _, C = sensor_levels
    seg = C.segments(0, 2)
    for shape in ((300,), (300, 6), (300, 4, 3)):
        x = np.random.default_rng(len(shape)).standard_normal(shape).astype(dtype)
        g = np.random.default_rng(9).standard_normal((seg.n_coarse,) + shape[1:]).astype(dtype)
        for mode in MODES:
            y = C.pool(x, mode=mode)
            assert y.dtype == dtype and np.array_equal(y, ch.pool_host(seg.ptr, seg.idx, x, mode))
            xd = engine.DeviceArray.from_host(seg.ctx, x, dtype)
            yd = C.pool(xd, mode=mode)
            assert isinstance(yd, engine.DeviceArray) and yd.shape == y.shape and yd.dtype == dtype
            assert np.array_equal(np.asarray(yd), y.astype(np.float64))
            gd = engine.DeviceArray.from_host(seg.ctx, g, dtype)
            gx = C.pool_vjp(g, x, mode=mode)
            gxd = C.pool_vjp(gd, xd, mode=mode)
            assert np.array_equal(gx, ch.pool_vjp_host(seg.ptr, seg.idx, g, x, mode))
            assert isinstance(gxd, engine.DeviceArray) and np.array_equal(np.asarray(gxd), gx.astype(np.float64))
        ud = C.unpool(engine.DeviceArray.from_host(seg.ctx, g, dtype))
        assert isinstance(ud, engine.DeviceArray) and np.array_equal(np.asarray(ud), C.unpool(g).astype(np.float64))
        assert np.array_equal(C.unpool(g), g[C.parent(0, 2)])
    one = C.pool(np.ones((C.graphs[1].N, 2)), lo=1, hi=2, mode="sum")
    assert np.array_equal(one[:, 0], C.segments(1, 2).sizes)
    with pytest.raises(ValueError):
        C.pool(np.ones((299, 2)))
    with pytest.raises(ValueError):
        C.pool(np.ones((300, 2)), mode="median")
    with pytest.raises(ValueError):
        C.pool(np.ones((300, 2)), lo=2, hi=2)
    with pytest.raises(ValueError):
        C.pool_vjp(np.ones((seg.n_coarse, 2)), None, mode="max")


# ---- torch ----------------------------------------------------------------------------------------------------------
def test_graph_pool_on_torch_tensors_in_a_fresh_process():
    run = subprocess.run(["timeout", "-k", "10", "180", sys.executable, CHILD], capture_output=True, text=True)
    print(run.stdout)
    print(run.stderr, file=sys.stderr)
    assert run.returncode == 0, "the child ended with status {}:\n{}".format(run.returncode, run.stderr[-4000:])
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, run.stdout
    record = json.loads(lines[0])
    if "skip" in record:
        pytest.skip(record["skip"])
    assert record["paths"] and all(p == "zero_copy" for p in record["paths"].values()), record
    assert all(record["gradcheck"].values()), record
    assert all(e == 0.0 for e in record["cpu_equals_gpu"].values()), record
    assert all(e < 1e-11 for e in record["network"].values()), record
