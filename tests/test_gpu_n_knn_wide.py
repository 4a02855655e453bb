"""Device nearest-neighbour graphs of clouds with MORE than 64 columns (the wide kernels of gspx_knn_bf.hip.h: a
run-time dimension loop in the MFMA sweep, one wave per query in the exact stages), ImgPatches / Grid2dImgPatches on
them.  Needs a real MI355X: `-m gpu`.

The bars are those of tests/test_gpu_5_knn.py: neighbour lists and distances equal scipy's KD-tree bit for bit
(cKDTree sums squared differences in four running sums and a remainder in any dimension, and the exact stages do the
same), weights to 1e-12 relative, sigma to 1e-13 (the mean is summed in another order).
"""
import ctypes
import functools

import numpy as np
import pytest
from scipy import spatial

from conftest import csr_from, load_golden, rel_err
from gpu_helpers import TOL, ctx  # noqa: F401 (ctx is a fixture: the default context)
from oracle import cheby_oracle as orc
from oracle import knn_oracle as knn
from pygsp_amd import _capi, engine, filters, graphs

pytestmark = pytest.mark.gpu


def cloud(N, d):
    rng = np.random.default_rng(N + d)
    return rng.standard_normal((N, d)) * rng.uniform(0.5, 2.0, d) + rng.uniform(-1, 1, d)


@functools.lru_cache(maxsize=None)
def oracle_of(N, d, k):
    """The cloud and the KD-tree's answer, computed once for all precisions of the sweep."""
    X = cloud(N, d)
    X.setflags(write=False)
    return (X,) + knn.knn_weights(X, k)


def check_against(ctx, X, k, ref):
    Wr, sr, NNr, Dr = ref
    W, sg, info = engine.knn_graph(X, k, ctx=ctx, neighbors=True)
    np.testing.assert_array_equal(info["NN"], NNr)
    np.testing.assert_array_equal(info["D"], Dr)           # bit for bit
    assert abs(sg - sr) <= 1e-13 * sr
    assert W.nnz == Wr.nnz and W.has_sorted_indices
    np.testing.assert_array_equal(W.indptr, Wr.indptr)
    np.testing.assert_array_equal(W.indices, Wr.indices)
    assert np.max(np.abs(W.data - Wr.data) / Wr.data) < 1e-12
    assert abs(W - W.T).max() == 0


def search_stats(ctx, X, k):
    lib = _capi.load()
    h = ctypes.c_void_p()
    Xc = np.ascontiguousarray(X, dtype=np.float64)
    _capi.check(lib.gspx_knn_build(ctx._h, Xc.shape[0], Xc.shape[1], _capi.ptr(Xc), k, 0.0, 0, 0, ctypes.byref(h)))
    out = np.zeros(4)
    _capi.check(lib.gspx_knn_search_stats(h, _capi.ptr(out)))
    lib.gspx_knn_destroy(h)
    return dict(sample=int(out[0]), capacity=int(out[1]), mean_candidates=float(out[2]), exact_scans=int(out[3]))


def swept_not_scanned(st, N, k):
    """Nearly every query was served by its candidate list (a build that sent everybody to the exact scan would
    pass the comparisons too)."""
    return st["exact_scans"] <= N // 1000 and k <= st["mean_candidates"] <= st["capacity"]


# one dimension past the narrow builds; a remainder of 1 and of 0 modulo 4 and modulo the 4-step LDS chunk; 1024
# (the default rule picks the fp32 sweep) and the limit 4096 (it keeps the fp64 one); a cloud small enough for the
# exact scan
@pytest.mark.parametrize("N,d,k", [(3000, 65, 9), (2500, 100, 10), (2000, 128, 16), (1500, 257, 12), (800, 1024, 7),
                                   (300, 4096, 5), (70, 200, 9)])
def test_wide_oracle(ctx, N, d, k):
    X, *ref = oracle_of(N, d, k)
    for f32 in (0, 2, 1):
        ctx.set_option("knn_f32", f32)
        try:
            check_against(ctx, X, k, ref)
            st = search_stats(ctx, X, k)
        finally:
            ctx.set_option("knn_f32", 1)
        if N > 4 * k + 64:
            assert swept_not_scanned(st, N, k), (f32, st)


@pytest.mark.parametrize("d", [96, 160])
def test_wide_two_sweeps(ctx, d):
    """8192 points: a sample of 2048 (stride 4), every second tile in the first sweep, the refinement stage in between,
    capacity 161 - about 31 candidates per query, at most 69 (numpy emulation of the plan)."""
    N, k = 8192, 10
    X = cloud(N, d)
    W, sg, info = engine.knn_graph(X, k, ctx=ctx, neighbors=True)
    st = search_stats(ctx, X, k)
    assert st["sample"] == 2048 and st["capacity"] == 161, st
    assert swept_not_scanned(st, N, k), st
    rows = np.random.default_rng(d).choice(N, 400, replace=False)
    D, NN = spatial.KDTree(X).query(X[rows], k=k + 1)
    np.testing.assert_array_equal(info["NN"][rows], NN[:, 1:])
    np.testing.assert_array_equal(info["D"][rows], D[:, 1:])
    assert abs(W - W.T).max() == 0


def test_wide_clusters_ties_and_other_metrics(ctx):
    rng = np.random.default_rng(8)
    # five tight clusters in 80-D: a query's bound admits its whole cluster, the lists overflow, the exact scan
    # takes over (default: the fp64 sweep - |x|^2 is huge against the distances; then the fp32 one, forced)
    Xc = (rng.standard_normal((5, 80)) * 50)[rng.integers(0, 5, 3000)] + 1e-3 * rng.standard_normal((3000, 80))
    ref = knn.knn_weights(Xc, 8)
    check_against(ctx, Xc, 8, ref)
    ctx.set_option("knn_f32", 2)
    try:
        check_against(ctx, Xc, 8, ref)
    finally:
        ctx.set_option("knn_f32", 1)
    # a 0/1 cloud in 68-D: squared distances are small whole numbers - ties everywhere
    Xb = rng.integers(0, 2, (1500, 68)).astype(np.float64)
    W, sg, info = engine.knn_graph(Xb, 8, ctx=ctx, neighbors=True)
    D, NN = knn.knn_query(Xb, 8)
    np.testing.assert_array_equal(info["D"], D[:, 1:])       # the distances are unambiguous
    d_chk = np.sqrt(((Xb[:, None, :] - Xb[info["NN"]]) ** 2).sum(-1))   # (whole numbers: exact in any order)
    np.testing.assert_array_equal(d_chk, info["D"])
    assert (info["NN"] != np.arange(1500)[:, None]).all()
    same = info["D"][:, 1:] == info["D"][:, :-1]
    assert same.any() and (info["NN"][:, 1:][same] > info["NN"][:, :-1][same]).all()
    # the metrics without a product form: every query takes the exact scan
    X = cloud(1500, 70)
    for metric in ("manhattan", "max_dist"):
        W, sg, info = engine.knn_graph(X, 7, ctx=ctx, neighbors=True, metric=metric)
        D, NN = knn.knn_query(X, 7, metric)
        np.testing.assert_array_equal(info["NN"], NN[:, 1:])
        np.testing.assert_array_equal(info["D"], D[:, 1:])


@pytest.mark.parametrize("N,d", [(3000, 65), (1500, 200)])
def test_wide_radius_oracle(ctx, N, d):
    X = cloud(N, d)
    eps = float(np.quantile(spatial.distance.pdist(X[:400]), 0.01))
    W, sg, _ = engine.radius_graph(X, eps, ctx=ctx)
    Wr, sr = knn.radius_weights(X, eps)
    assert W.nnz == Wr.nnz and W.nnz > 0, (N, d, W.nnz, Wr.nnz)
    assert np.array_equal(W.indptr, Wr.indptr) and np.array_equal(W.indices, Wr.indices)
    assert abs(sg - sr) <= 1e-12 * sr and np.max(np.abs(W.data - Wr.data) / Wr.data) < 1e-11
    with pytest.raises(ValueError, match="No neighbors"):
        engine.radius_graph(X[:500], 1e-3, ctx=ctx)


def image(seed, shape):
    """gen_knn_wide_golden.py's image()."""
    rng = np.random.default_rng(seed)
    ramp = 4.0 * np.add.outer(np.arange(shape[0]), np.arange(shape[1]))
    return (ramp.reshape(ramp.shape + (1,) * (len(shape) - 2)) + rng.integers(0, 64, shape)).astype(np.float64)


def test_wide_golden(ctx):
    """The reference's ImgPatches (75-D RGB and 81-D grey patches), Grid2dImgPatches, a 300-D manhattan NNGraph and a
    96-D radius graph (tests/golden/knn_wide.npz, generated from the real pygsp)."""
    g = load_golden("knn_wide.npz")
    rgb, grey = image(21, (20, 24, 3)), image(22, (18, 22))
    G = graphs.ImgPatches(rgb, patch_shape=(5, 5), k=10, ctx=ctx)
    np.testing.assert_array_equal(G.Xin, g["feat_rgb"])
    Wref = csr_from(g, "W_rgb")
    assert G.Xin.shape[1] == 75 and G.W.nnz == Wref.nnz and abs(G.W - Wref).max() < 1e-14
    assert abs(G.sigma - float(g["sigma_rgb"])) < 1e-13
    G = graphs.ImgPatches(grey, patch_shape=(9,), k=8, ctx=ctx)
    np.testing.assert_allclose(G.coords, g["coords_grey"], rtol=0, atol=1e-13)
    Wref = csr_from(g, "W_grey")
    assert G.Xin.shape[1] == 81 and G.W.nnz == Wref.nnz and abs(G.W - Wref).max() < 1e-14
    assert abs(G.sigma - float(g["sigma_grey"])) < 1e-13
    G = graphs.Grid2dImgPatches(rgb, patch_shape=(5, 5), k=10, ctx=ctx)
    Wref = csr_from(g, "W_gridrgb")
    assert G.N == 480 and G.W.nnz == Wref.nnz and abs(G.W - Wref).max() < 1e-14
    np.testing.assert_array_equal(G.coords, G.Gg.coords)
    G = graphs.NNGraph(np.random.default_rng(23).standard_normal((600, 300)), k=9, dist_type="minkowski", order=1,
                       ctx=ctx)
    Wref = csr_from(g, "W_x300")
    assert G.W.nnz == Wref.nnz and abs(G.W - Wref).max() < 1e-14 and abs(G.sigma - float(g["sigma_x300"])) < 1e-13
    G = graphs.NNGraph(np.random.default_rng(24).standard_normal((500, 96)), NNtype="radius", epsilon=0.3, ctx=ctx)
    Wref = csr_from(g, "W_r96")
    assert G.W.nnz == Wref.nnz == int(g["nnz_r96"]) and abs(G.W - Wref).max() < 1e-12
    assert abs(G.sigma - float(g["sigma_r96"])) < 1e-13


def test_wide_cloud_through_the_graph(ctx):
    """4608 points in 96-D: large enough for the device set-up with a curve order (it is handed the leading columns),
    then Laplacian and a Chebyshev filter on the graph."""
    X = cloud(4608, 96)
    G = graphs.NNGraph(X, k=10, ctx=ctx)
    assert G._adj_dev is not None and G.setup_report["built"]   # W never left the device
    Wr = knn.knn_weights(knn.preprocess(X), 10)[0]
    L = orc.laplacian(Wr)
    assert G.L.nnz == L.nnz and abs(G.L - L).max() < 1e-12 * max(1.0, L.diagonal().max())
    G.estimate_lmax("bounds")
    x = np.random.default_rng(0).standard_normal((G.N, 3))
    y = filters.Heat(G, 10).filter(x, method="chebyshev", order=10)
    ref = orc.filter_chebyshev(L, G.lmax, [orc.heat_kernel(10, G.lmax)], x, 10)
    assert rel_err(y, ref) < TOL[np.dtype(np.float64)]


def test_wide_limits(ctx):
    with pytest.raises(ValueError, match="4096"):
        engine.knn_graph(np.zeros((100, 4097)), 3, ctx=ctx)
    with pytest.raises(ValueError, match="4096"):
        engine.radius_graph(np.zeros((100, 4097)), 1.0, ctx=ctx)
    with pytest.raises(ValueError, match="k <= 64"):
        engine.knn_graph(cloud(200, 70), 65, ctx=ctx)
