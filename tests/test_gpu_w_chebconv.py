"""The Chebyshev graph convolution on the device (gspx_cheby_conv_dev / k_group_mix, gspx_cheby_cross_grams_dev /
k_slot_cross_gram, filters.cheby_conv, filters.cheby_conv_vjp): every edge of the two dense kernels' tiles against the
numpy restatement order by order, padded panels, tiny graphs, an internal vertex order, tile and plain steps, column
batches of whole samples, the adjoint identities with the device's own forward, the bridge to cheby_op, the argument
errors - and identical bits from identical calls wherever a convolution or a Gram is computed."""
import numpy as np
import pytest

from chebconv_helpers import bridge_theta, conv_direct, cross_grams_direct, recurrence
from conftest import rel_err
from gpu_helpers import TOL, ctx, random_graph, upper_lmax  # noqa: F401 (ctx: fixture)
from oracle import cheby_oracle as orc
from pygsp_amd import filters, graphs
from scipy import sparse

pytestmark = pytest.mark.gpu

F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
# k_group_mix takes 16 logical rows and 16-wide tiles of Fout per product, 4 elements of Fin per step, and has a build
# for Fin <= 32 and one above; k_slot_cross_gram takes 16-, 32- or 64-wide tiles of either dimension (two tiles from 65)
PAIRS = [(1, 1), (3, 5), (5, 3), (4, 15), (15, 4), (16, 17), (17, 16), (33, 64), (64, 33), (65, 4), (128, 128)]


def graph_of(W, dtype=np.float64):
    G = graphs.Graph(W, compute_dtype=dtype)
    G._lmax = upper_lmax(W)
    return G


def rounded(a, dtype):
    return np.asarray(a).astype(dtype).astype(np.float64)


def draw_theta(rng, M, fin, fout):
    return rng.standard_normal((M, fin, fout)) / np.sqrt(fin)


def device_conv(G, theta, x, dtype=np.float64):
    """Two identical gspx_cheby_conv_dev calls on x uploaded in `dtype` (their bits compared), and the reference on x and
    theta rounded to it."""
    dev = G.device_graph(dtype)
    y, _ = dev.cheby_conv(theta, x, G.lmax)
    y2, _ = dev.cheby_conv(theta, x, G.lmax)
    assert np.array_equal(y, y2)  # identical calls, identical bits
    return y, conv_direct(orc.laplacian(G.W), G.lmax, rounded(x, dtype), rounded(theta, dtype))


def device_grams(G, x, z, M, dtype=np.float64):
    dev = G.device_graph(dtype)
    g, _ = dev.cheby_cross_grams(x, z, G.lmax, M)
    g2, _ = dev.cheby_cross_grams(x, z, G.lmax, M)
    assert g.dtype == np.float64 and np.array_equal(g, g2)
    return g, cross_grams_direct(orc.laplacian(G.W), G.lmax, rounded(x, dtype), rounded(z, dtype), M)


@pytest.fixture(scope="module")
def hub_graphs():
    W = random_graph(3000, 8, seed=5, hub=True, isolated=2)
    return {F64: graph_of(W, np.float64), F32: graph_of(W, np.float32)}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("fin,fout", PAIRS)
def test_mix_and_gram_edges(hub_graphs, dtype, fin, fout):
    G, tol = hub_graphs[np.dtype(dtype)], TOL[np.dtype(dtype)]
    L = orc.laplacian(G.W)
    rng = np.random.default_rng(1000 * fin + fout)
    worst_y = worst_g = 0.0
    for B in (1, 2, 3):
        x, z = rng.standard_normal((G.N, B, fin)), rng.standard_normal((G.N, B, fout))
        T = recurrence(L, G.lmax, rounded(x, dtype), 14)  # shared by every M below
        zr = rounded(z, dtype)
        for M in (2, 3, 13, 14):
            theta = draw_theta(rng, M, fin, fout)
            dev = G.device_graph(dtype)
            y, _ = dev.cheby_conv(theta, x, G.lmax)
            y2, _ = dev.cheby_conv(theta, x, G.lmax)
            ref = sum(np.einsum("nbi,io->nbo", T[k], rounded(theta[k], dtype)) for k in range(M))
            assert y.shape == (G.N, B, fout) and y.dtype == np.dtype(dtype) and np.array_equal(y, y2)
            err = rel_err(y, ref)
            worst_y = max(worst_y, err)
            assert err < tol, (B, M, err)
            g, _ = dev.cheby_cross_grams(x, z, G.lmax, M)
            g2, _ = dev.cheby_cross_grams(x, z, G.lmax, M)
            assert g.shape == (M, fin, fout) and g.dtype == np.float64 and np.array_equal(g, g2)
            for k in range(M):  # order by order: a slot that met another order's rows would hide in the max-norm
                err = rel_err(g[k], np.einsum("nbi,nbo->io", T[k], zr))
                worst_g = max(worst_g, err)
                assert err < tol, (B, M, k, err)
        # order by order for the convolution too: theta with one order alone must give that order's term
        theta = draw_theta(rng, 14, fin, fout)
        for k in range(14):
            only = np.zeros_like(theta)
            only[k] = theta[k]
            y, _ = G.device_graph(dtype).cheby_conv(only, x, G.lmax)
            err = rel_err(y, np.einsum("nbi,io->nbo", T[k], rounded(theta[k], dtype)))
            worst_y = max(worst_y, err)
            assert err < tol, (B, k, err)
    print("chebconv {} {}x{}: conv {:.2e}, grams {:.2e}".format(np.dtype(dtype).name, fin, fout, worst_y, worst_g))


@pytest.mark.parametrize("N", [1, 63, 65, 257])
def test_tiny_graphs(N):
    W = random_graph(N, 4, seed=N) if N > 1 else sparse.csr_matrix((1, 1))
    G = graphs.Graph(W, compute_dtype=np.float64)
    G._lmax = upper_lmax(W) if N > 1 else 1.0  # (one isolated vertex: L = 0, any positive lmax)
    rng = np.random.default_rng(N)
    x, z = rng.standard_normal((N, 2, 3)), rng.standard_normal((N, 2, 2))
    for M in (2, 3, 4):
        y, ref = device_conv(G, draw_theta(rng, M, 3, 2), x)
        g, gref = device_grams(G, x, z, M)
        assert y.shape == (N, 2, 2) and rel_err(y, ref) < TOL[F64], M
        assert g.shape == (M, 3, 2) and rel_err(g, gref) < TOL[F64], M


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_internal_vertex_order_and_padded_panels(ctx, dtype):
    """The work panels are in the graph's internal order, x, y and the cotangent are not; and widths that are not whole
    16-byte pieces (3, 15, 5, 9 columns) run the tile steps on zero-padded panels."""
    G = graphs.Sensor(5000, seed=0, tiles=True, reorder="morton", compute_dtype=dtype)
    G.estimate_lmax("bounds")
    perm = G.device_graph(dtype).download_perm()
    assert perm is not None and not np.array_equal(perm, np.arange(G.N))
    assert G.device_graph(dtype).ctx is ctx
    rng = np.random.default_rng(0)
    for B, fin, fout in ((1, 5, 3), (3, 3, 5), (1, 3, 5), (3, 5, 3), (2, 4, 8)):
        x, z = rng.standard_normal((G.N, B, fin)), rng.standard_normal((G.N, B, fout))
        y, ref = device_conv(G, draw_theta(rng, 9, fin, fout), x, dtype)
        kinds = ctx.last_step_kinds()
        g, gref = device_grams(G, x, z, 9, dtype)
        ey, eg = rel_err(y, ref), rel_err(g, gref)
        print("internal order {} B {} {}x{}: conv {:.2e}, grams {:.2e}".format(np.dtype(dtype).name, B, fin, fout, ey, eg))
        assert ey < TOL[np.dtype(dtype)] and eg < TOL[np.dtype(dtype)]
        assert kinds == {"tile": 9, "plain": 0}, kinds  # M Clenshaw steps, on the gather tiles the graph carries


def test_tile_and_plain_steps(ctx):
    G = graphs.Sensor(40_000, seed=3)
    G.estimate_lmax("bounds")
    rng = np.random.default_rng(3)
    x, z = rng.standard_normal((G.N, 2, 8)), rng.standard_normal((G.N, 2, 8))
    theta = draw_theta(rng, 6, 8, 8)
    y, ref = device_conv(G, theta, x)
    tiled = ctx.last_step_kinds()
    g, gref = device_grams(G, x, z, 6)
    ctx.set_option("tile_gather", 0)
    try:
        yp, _ = device_conv(G, theta, x)
        plain = ctx.last_step_kinds()
        gp, _ = device_grams(G, x, z, 6)
    finally:
        ctx.set_option("tile_gather", 1)
    assert G.device_graph(np.float64).ctx is ctx
    assert rel_err(y, ref) < TOL[F64] and rel_err(yp, ref) < TOL[F64]
    assert rel_err(g, gref) < TOL[F64] and rel_err(gp, gref) < TOL[F64]
    assert tiled["plain"] == 0 and tiled["tile"] > 0 and plain["tile"] == 0 and plain["plain"] > 0, (tiled, plain)


def test_column_batches_hold_whole_samples(ctx):
    W = random_graph(5000, 6, seed=7, isolated=1)
    G = graph_of(W)
    rng = np.random.default_rng(7)
    x, z = rng.standard_normal((G.N, 4, 5)), rng.standard_normal((G.N, 4, 3))
    theta = draw_theta(rng, 8, 5, 3)
    y, ref = device_conv(G, theta, x)
    g, gref = device_grams(G, x, z, 8)
    ctx.set_option("max_batch", 8)  # narrower than two samples of five features: one sample per batch, four batches
    try:
        y4, _ = device_conv(G, theta, x)
        g4, _ = device_grams(G, x, z, 8)
        ctx.set_option("max_batch", 3)  # narrower than one sample: still one sample per batch
        y1, _ = device_conv(G, theta, x)
        g1, _ = device_grams(G, x, z, 8)
    finally:
        ctx.set_option("max_batch", 0)
    assert G.device_graph(np.float64).ctx is ctx
    for got in (y, y4, y1):
        assert rel_err(got, ref) < TOL[F64]
    for got in (g, g4, g1):
        assert rel_err(got, gref) < TOL[F64]
    assert np.array_equal(g4, g1)


def dot(a, b):
    return float(np.vdot(np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()))


def test_adjointness_with_the_device_forward(hub_graphs):
    """<cot, Y> is linear in X and in theta: <grad_X, dX> = <cot, cheby_conv(theta, dX)> and
    <grad_theta, dtheta> = <cot, cheby_conv(dtheta, X)>, forward and backward both on the device."""
    G = hub_graphs[F64]
    rng = np.random.default_rng(8)
    decay = (0.8 ** np.arange(15))[:, None, None]
    theta, dtheta = draw_theta(rng, 15, 6, 5) * decay, draw_theta(rng, 15, 6, 5) * decay
    x, dx, cot = rng.standard_normal((G.N, 3, 6)), rng.standard_normal((G.N, 3, 6)), rng.standard_normal((G.N, 3, 5))
    gx, gt = filters.cheby_conv_vjp(G, theta, x, cot)
    assert gx.shape == x.shape and gt.shape == theta.shape and gt.dtype == np.float64
    rhs_x, rhs_t = dot(cot, filters.cheby_conv(G, theta, dx)), dot(cot, filters.cheby_conv(G, dtheta, x))
    ex, et = abs(dot(gx, dx) - rhs_x) / abs(rhs_x), abs(dot(gt, dtheta) - rhs_t) / abs(rhs_t)
    print("cancellation: |rhs| / (|g| |d|) = {:.2e} (signal), {:.2e} (theta)".format(
        abs(rhs_x) / (np.linalg.norm(gx) * np.linalg.norm(dx)), abs(rhs_t) / (np.linalg.norm(gt) * np.linalg.norm(dtheta))))
    print("adjointness: signal {:.2e}, theta {:.2e}".format(ex, et))
    assert ex < 1e-10 and et < 1e-10


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bridge_to_cheby_op(hub_graphs, dtype):
    G = hub_graphs[np.dtype(dtype)]
    rng = np.random.default_rng(9)
    c, x = rng.standard_normal(12) * 0.8 ** np.arange(12), rng.standard_normal((G.N, 4))
    y = filters.cheby_conv(G, bridge_theta(c, 4), x)
    ref = filters.cheby_op(G, c, x)
    err = rel_err(y, ref)
    print("bridge {}: {:.2e}".format(np.dtype(dtype).name, err))
    assert y.shape == (G.N, 4) and err < TOL[np.dtype(dtype)]


def test_argument_errors(hub_graphs, ctx):
    G = hub_graphs[F64]
    dev = G.device_graph(np.float64)
    a, b = ctx.alloc(G.N * 129 * 8), ctx.alloc(G.N * 129 * 8)
    try:
        with pytest.raises(ValueError, match="same buffer"):
            dev.cheby_conv_dev(np.ones((3, 2, 2)), a.ptr, a.ptr, 1, G.lmax)
        with pytest.raises(ValueError, match="1 to 128 features"):
            dev.cheby_conv_dev(np.ones((3, 129, 1)), a.ptr, b.ptr, 1, G.lmax)
        with pytest.raises(ValueError, match="1 to 128 features"):
            dev.cheby_cross_grams_dev(a.ptr, b.ptr, 1, 1, 129, G.lmax, 3)
        with pytest.raises(ValueError, match="2 to 256"):
            dev.cheby_conv_dev(np.ones((257, 1, 1)), a.ptr, b.ptr, 1, G.lmax)
        with pytest.raises(ValueError, match="2 to 256"):
            dev.cheby_cross_grams_dev(a.ptr, b.ptr, 1, 1, 1, G.lmax, 257)
        with pytest.raises(TypeError):
            dev.cheby_conv_dev(np.ones((1, 2, 2)), a.ptr, b.ptr, 1, G.lmax)
        with pytest.raises(TypeError):
            dev.cheby_cross_grams_dev(a.ptr, b.ptr, 1, 2, 2, G.lmax, 1)
        with pytest.raises(TypeError):
            filters.cheby_conv(G, np.ones((3, 2, 2)), G.to_device(np.ones((G.N, 2))))
        y, _ = dev.cheby_conv(np.ones((2, 2, 2)), np.zeros((G.N, 0, 2)), G.lmax)  # no samples: nothing happens
        assert y.shape == (G.N, 0, 2)
    finally:
        a.free()
        b.free()
