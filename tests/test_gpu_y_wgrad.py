"""gspx_cheby_laplacian_grad_dev, filters.cheby_op_vjp_laplacian / cheby_op_vjp_weights and Filter.filter_vjp_weights on
the GPU against the numpy restatement (wgrad_helpers) on inputs rounded to the compute dtype, and against central
differences of the device's own forward.  Coefficients are standard_normal * 0.8^k: with those, float32 panels alone
move the restatement by 3e-7 to 4e-6 on these graphs, a factor of 5 under the fp32 bar."""
import numpy as np
import pytest
from scipy import sparse

from conftest import rel_err
from gpu_helpers import TOL, ctx, random_graph, upper_lmax  # noqa: F401 (ctx: fixture)
from oracle import cheby_oracle as orc
from pygsp_amd import filters, graphs
from wgrad_helpers import laplacian_grad_direct, weights_grad_direct

pytestmark = pytest.mark.gpu

F64, F32 = np.dtype(np.float64), np.dtype(np.float32)


def graph_of(W, dtype=np.float64, lap_type="combinatorial"):
    G = graphs.Graph(W, lap_type=lap_type, compute_dtype=dtype)
    G._lmax = upper_lmax(W) if lap_type == "combinatorial" else 2.0
    return G


def coeffs_of(rng, nf, M):
    return rng.standard_normal((nf, M)) * 0.8 ** np.arange(M)


def edges_of(G):
    s, t, _ = G.get_edge_list()
    return np.stack([s, t])


def device_grad(G, c, x, z, pairs=None, dtype=np.float64, need_diag=True):
    """One gspx_cheby_laplacian_grad_dev call on x, z uploaded in `dtype`, and the reference on both rounded to it:
    (gdiag, goff, reference gdiag, reference goff)."""
    gd, go, _ = G.device_graph(dtype).cheby_laplacian_grad(c, x, z, G.lmax, pairs, need_diag)
    r = (lambda a: np.asarray(a).astype(dtype).astype(np.float64))
    rd, ro = laplacian_grad_direct(orc.laplacian(G.W, G.lap_type), G.lmax, c, r(x), r(z),
                                   edges_of(G) if pairs is None else pairs)
    return gd, go, rd, ro


def random_pairs(rng, N, P, hub=None):
    """(2, P) pairs s != t with repeats and both orientations; `hub`: that vertex in the first min(P, 300) pairs."""
    s = rng.integers(0, N, P)
    t = (s + 1 + rng.integers(0, N - 1, P)) % N
    if hub is not None:
        n = min(P, 300)
        s[:n] = hub
        t[:n] = (hub + 1 + rng.integers(0, N - 1, n)) % N
        t[1:n:2], s[1:n:2] = s[1:n:2].copy(), t[1:n:2].copy()
    if P >= 4:
        s[-1], t[-1] = s[0], t[0]  # a repeat
        s[-2], t[-2] = t[1], s[1]  # and one the other way round
    return np.stack([s, t]).astype(np.int32)


@pytest.fixture(scope="module")
def hub_graphs():
    W = random_graph(3000, 8, seed=5, hub=True, isolated=2)
    return {F64: graph_of(W, np.float64), F32: graph_of(W, np.float32)}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nsig", [1, 3, 5, 6, 67, 130])
def test_laplacian_grad_widths(hub_graphs, dtype, nsig):
    G = hub_graphs[np.dtype(dtype)]
    tol = TOL[np.dtype(dtype)]
    rng = np.random.default_rng(nsig)
    x, z, c = rng.standard_normal((G.N, nsig)), rng.standard_normal((2, G.N, nsig)), coeffs_of(rng, 2, 14)
    for pairs in (None, random_pairs(rng, G.N, 1000, hub=0)):
        gd, go, rd, ro = device_grad(G, c, x, z, pairs, dtype)
        gd2, go2, _, _ = device_grad(G, c, x, z, pairs, dtype)
        ed, eo = rel_err(gd, rd), rel_err(go, ro)
        print("laplacian grad {} nsig {} {}: gdiag {:.2e} goff {:.2e}".format(
            np.dtype(dtype).name, nsig, "own edges" if pairs is None else "pair list", ed, eo))
        assert gd.shape == (G.N,) and go.shape == ro.shape and gd.dtype == go.dtype == np.float64
        assert ed < tol and eo < tol
        assert np.array_equal(gd, gd2) and np.array_equal(go, go2)  # identical calls, identical bits
        # each output on its own: the other pointer null
        none, go3, _, _ = device_grad(G, c, x, z, pairs, dtype, need_diag=False)
        assert none is None and np.array_equal(go3, go)


@pytest.mark.parametrize("N", [1, 2, 63, 65, 257])
def test_laplacian_grad_small_graphs(N):
    W = random_graph(N, 4, seed=N) if N > 2 else sparse.csr_matrix(np.array([[0.0, 0.7], [0.7, 0.0]])[:N, :N])
    G = graph_of(W)
    if N == 1:
        G._lmax = 1.0  # (one isolated vertex: L = 0, any positive lmax)
    rng = np.random.default_rng(N)
    for nsig in (1, 4, 5):
        x = rng.standard_normal((N, nsig))
        pairs = random_pairs(rng, N, 9) if N > 1 else np.zeros((2, 0), dtype=np.int32)
        for nf in (1, 3):
            z = rng.standard_normal((nf, N, nsig))
            for M in (2, 3, 4):  # M = 2: the phi_1 term alone; M = 3: the first phi = 2
                c = coeffs_of(rng, nf, M)
                gd, go, rd, ro = device_grad(G, c, x, z, pairs)
                assert gd.shape == (N,) and rel_err(gd, rd) < TOL[F64], (nsig, nf, M)
                assert go.shape == (pairs.shape[1],) and (N == 1 or rel_err(go, ro) < TOL[F64]), (nsig, nf, M)
                gd, go, rd, ro = device_grad(G, c, x, z)
                assert go.shape == ro.shape and (ro.size == 0 or rel_err(go, ro) < TOL[F64]), (nsig, nf, M)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("P", [0, 1, 255, 256, 257])
def test_laplacian_grad_pair_counts(hub_graphs, dtype, P):
    G = hub_graphs[np.dtype(dtype)]
    dev = G.device_graph(dtype)
    rng = np.random.default_rng(P)
    x, z, c = rng.standard_normal((G.N, 6)), rng.standard_normal((1, G.N, 6)), coeffs_of(rng, 1, 9)
    pairs = random_pairs(rng, G.N, P)
    gd, go, rd, ro = device_grad(G, c, x, z, pairs, dtype)
    assert go.shape == (P,) and rel_err(gd, rd) < TOL[np.dtype(dtype)]
    assert P == 0 or rel_err(go, ro) < TOL[np.dtype(dtype)]
    # goff null: gdiag alone, the same bits
    bx, bz = dev.ctx.upload(x.astype(dtype)), dev.ctx.upload(z.astype(dtype))
    bp, bd = dev.ctx.upload(pairs if P else np.zeros(4, dtype=np.int32)), dev.ctx.alloc(8 * G.N)
    try:
        dev.cheby_laplacian_grad_dev(c, bx.ptr, bz.ptr, 6, G.lmax, bp.ptr, bp.ptr + 4 * P, P, bd.ptr, None)
        assert np.array_equal(bd.download((G.N,), np.float64), gd)
    finally:
        for b in (bx, bz, bp, bd):
            b.free()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_laplacian_grad_a_list_naming_the_hub_300_times(hub_graphs, dtype):
    G = hub_graphs[np.dtype(dtype)]
    rng = np.random.default_rng(300)
    x, z, c = rng.standard_normal((G.N, 12)), rng.standard_normal((3, G.N, 12)), coeffs_of(rng, 3, 31)
    pairs = random_pairs(rng, G.N, 300, hub=0)
    assert np.all((pairs[0] == 0) | (pairs[1] == 0))
    gd, go, rd, ro = device_grad(G, c, x, z, pairs, dtype)
    err = rel_err(go, ro)
    print("hub list {}: {:.2e}".format(np.dtype(dtype).name, err))
    assert err < TOL[np.dtype(dtype)] and rel_err(gd, rd) < TOL[np.dtype(dtype)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_laplacian_grad_slot_and_plane_counts(dtype):
    W = random_graph(700, 6, seed=11, isolated=1)
    G = graph_of(W, dtype)
    rng = np.random.default_rng(11)
    pairs = random_pairs(rng, G.N, 400)
    for nsig in (5, 6):
        x = rng.standard_normal((G.N, nsig))
        for nf, Ms in ((1, (15, 16, 17, 33)), (2, (16,)), (9, (17,))):
            z = rng.standard_normal((nf, G.N, nsig))
            for M in Ms:
                gd, go, rd, ro = device_grad(G, coeffs_of(rng, nf, M), x, z, pairs, dtype)
                assert rel_err(gd, rd) < TOL[np.dtype(dtype)] and rel_err(go, ro) < TOL[np.dtype(dtype)], (nsig, nf, M)


def test_laplacian_grad_column_batches(ctx):
    W = random_graph(5000, 6, seed=7, isolated=1)
    G = graph_of(W)
    rng = np.random.default_rng(7)
    x, z, c = rng.standard_normal((G.N, 20)), rng.standard_normal((3, G.N, 20)), coeffs_of(rng, 3, 21)
    pairs = random_pairs(rng, G.N, 2000)
    gd, go, rd, ro = device_grad(G, c, x, z, pairs)
    ctx.set_option("max_batch", 8)  # three column batches
    try:
        gd3, go3, _, _ = device_grad(G, c, x, z, pairs)
    finally:
        ctx.set_option("max_batch", 0)
    assert G.device_graph(np.float64).ctx is ctx
    assert rel_err(gd, rd) < TOL[F64] and rel_err(go, ro) < TOL[F64]
    assert rel_err(gd3, rd) < TOL[F64] and rel_err(go3, ro) < TOL[F64] and rel_err(go3, go) < TOL[F64]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_laplacian_grad_in_an_internal_vertex_order(dtype):
    """The slots and the Clenshaw panels are in the graph's internal order; the pairs, the cotangent and gdiag are not."""
    G = graphs.Sensor(5000, seed=0, tiles=True, reorder="morton", compute_dtype=dtype)
    G.estimate_lmax("bounds")
    perm = G.device_graph(dtype).download_perm()
    assert perm is not None and not np.array_equal(perm, np.arange(G.N))
    rng = np.random.default_rng(0)
    pairs = random_pairs(rng, G.N, 1500)
    for nsig in (4, 5):  # (5: a padded width on the tile kernels)
        x, z, c = rng.standard_normal((G.N, nsig)), rng.standard_normal((2, G.N, nsig)), coeffs_of(rng, 2, 12)
        for p in (None, pairs):
            gd, go, rd, ro = device_grad(G, c, x, z, p, dtype)
            ed, eo = rel_err(gd, rd), rel_err(go, ro)
            print("internal order {} nsig {}: gdiag {:.2e} goff {:.2e}".format(np.dtype(dtype).name, nsig, ed, eo))
            assert ed < TOL[np.dtype(dtype)] and eo < TOL[np.dtype(dtype)]


def test_laplacian_grad_tile_and_plain_steps(ctx):
    G = graphs.Sensor(40_000, seed=3)
    G.estimate_lmax("bounds")
    rng = np.random.default_rng(3)
    x, z, c = rng.standard_normal((G.N, 16)), rng.standard_normal((2, G.N, 16)), coeffs_of(rng, 2, 20)
    gd, go, rd, ro = device_grad(G, c, x, z)
    tiled = ctx.last_step_kinds()
    ctx.set_option("tile_gather", 0)
    try:
        gdp, gop, _, _ = device_grad(G, c, x, z)
        plain = ctx.last_step_kinds()
    finally:
        ctx.set_option("tile_gather", 1)
    assert G.device_graph(np.float64).ctx is ctx
    assert rel_err(gd, rd) < TOL[F64] and rel_err(go, ro) < TOL[F64]
    assert rel_err(gdp, rd) < TOL[F64] and rel_err(gop, ro) < TOL[F64]
    # 20 orders: 18 recurrence steps into 19 kept slots, then 19 Clenshaw steps
    assert tiled == {"tile": 37, "plain": 0} and plain == {"tile": 0, "plain": 37}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_bad_pair_raises_and_leaves_the_outputs_untouched(hub_graphs, dtype):
    G = hub_graphs[np.dtype(dtype)]
    dev = G.device_graph(dtype)
    rng = np.random.default_rng(1)
    x, z, c = rng.standard_normal((G.N, 4)).astype(dtype), rng.standard_normal((1, G.N, 4)).astype(dtype), coeffs_of(rng, 1, 6)
    bx, bz = dev.ctx.upload(x), dev.ctx.upload(z)
    bd, bo = dev.ctx.upload(np.full(G.N, 7.0)), dev.ctx.upload(np.full(3, 7.0))
    try:
        for bad in ([[1, 2, G.N], [2, 3, 4]], [[1, 2, 3], [2, -1, 4]], [[1, 5, 3], [2, 5, 4]]):
            bp = dev.ctx.upload(np.array(bad, dtype=np.int32))
            try:
                with pytest.raises(ValueError, match="vertex couple"):
                    dev.cheby_laplacian_grad_dev(c, bx.ptr, bz.ptr, 4, G.lmax, bp.ptr, bp.ptr + 12, 3, bd.ptr, bo.ptr)
            finally:
                bp.free()
            assert np.all(bd.download((G.N,), np.float64) == 7.0) and np.all(bo.download((3,), np.float64) == 7.0)
        with pytest.raises(ValueError, match="come together"):
            dev.cheby_laplacian_grad_dev(c, bx.ptr, bz.ptr, 4, G.lmax, bd.ptr, None, 3, bd.ptr, bo.ptr)
    finally:
        for b in (bx, bz, bd, bo):
            b.free()


# ---- the Python functions ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lap_type", ["combinatorial", "normalized"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_cheby_op_vjp_weights_against_the_restatement(lap_type, dtype):
    W = random_graph(3000, 8, seed=5, hub=True)
    G = graph_of(W, dtype, lap_type)
    rng = np.random.default_rng(2)
    c, x, cot = coeffs_of(rng, 2, 14), rng.standard_normal((G.N, 6)), rng.standard_normal((2 * G.N, 6))
    extra = random_pairs(rng, G.N, 500)
    r = (lambda a: np.asarray(a).astype(dtype).astype(np.float64))
    for pairs in (None, extra):
        grad = filters.cheby_op_vjp_weights(G, c, x, cot, pairs=pairs)
        p = edges_of(G) if pairs is None else pairs
        ref = weights_grad_direct(W, lap_type, G.lmax, c, r(x), r(cot).reshape(2, G.N, 6), p)
        err = rel_err(grad, ref)
        print("vjp_weights {} {} {}: {:.2e}".format(lap_type, np.dtype(dtype).name, "own" if pairs is None else "pairs", err))
        assert grad.shape == (p.shape[1],) and grad.dtype == np.float64 and err < TOL[np.dtype(dtype)]
    gdiag, goff = filters.cheby_op_vjp_laplacian(G, c, x, cot)
    assert gdiag.shape == (G.N,) and goff.shape == (G.n_edges,)


@pytest.mark.parametrize("lap_type", ["combinatorial", "normalized"])
def test_cheby_op_vjp_weights_against_differences_of_the_device_forward(lap_type):
    """Two edges and one non-edge: (loss(w + h) - loss(w - h)) / 2h of the device's own forward on a Graph rebuilt with
    the perturbed W and the SAME lmax; step 1e-5, bar 1e-6 relative to the largest entry of the gradient."""
    W = random_graph(400, 6, seed=13)
    lmax = 1.5 * upper_lmax(W) if lap_type == "combinatorial" else 2.0
    G = graphs.Graph(W, lap_type=lap_type)
    G._lmax = lmax
    rng = np.random.default_rng(13)
    c, x, cot = coeffs_of(rng, 2, 12), rng.standard_normal((400, 3)), rng.standard_normal((800, 3))
    E = edges_of(G)
    non = next((s, t) for s in range(400) for t in range(s + 1, 400) if W[s, t] == 0)
    pairs = np.array([[E[0, 3], E[0, 200], non[0]], [E[1, 3], E[1, 200], non[1]]], dtype=np.int32)
    grad = filters.cheby_op_vjp_weights(G, c, x, cot, pairs=pairs)
    scale = np.abs(filters.cheby_op_vjp_weights(G, c, x, cot)).max()

    def loss(p, h):
        Wp = sparse.lil_matrix(W)
        Wp[pairs[0, p], pairs[1, p]] += h
        Wp[pairs[1, p], pairs[0, p]] += h
        Gp = graphs.Graph(sparse.csr_matrix(Wp), lap_type=lap_type)
        Gp._lmax = lmax
        return float((cot * filters.cheby_op(Gp, c, x)).sum())

    for p in range(3):
        h = 1e-5
        fd = (loss(p, h) - loss(p, -h)) / (2 * h)  # (the non-edge at weight -h: a negative weight only warns)
        print("{} pair {}: {:.6e} against {:.6e}".format(lap_type, p, grad[p], fd))
        assert abs(fd - grad[p]) < 1e-6 * scale


@pytest.mark.parametrize("lap_type", ["combinatorial", "normalized"])
def test_filter_vjp_weights_synthesis_is_the_swapped_analysis_call(lap_type):
    W = random_graph(1000, 6, seed=2)
    G = graph_of(W, np.float64, lap_type)
    bank = filters.MexicanHat(G, Nf=3)
    rng = np.random.default_rng(6)
    s, cot = rng.standard_normal((G.N, 4)), rng.standard_normal((G.N, 4, 3))
    pairs = random_pairs(rng, G.N, 200)
    ana = bank.filter_vjp_weights(s, cot, order=20, pairs=pairs)
    syn = bank.filter_vjp_weights(cot, s, order=20, pairs=pairs)
    assert ana.shape == (200,) and np.array_equal(ana, syn)
    c = filters._as_coeff_matrix(filters.compute_cheby_coeff(bank, m=20))
    ref = weights_grad_direct(W, lap_type, G.lmax, c, s, np.moveaxis(cot, 2, 0), pairs)
    assert rel_err(ana, ref) < TOL[F64]


def test_laplacian_grad_on_a_million_vertices():
    G = graphs.Sensor(1_000_000, seed=0)
    G.estimate_lmax("bounds")
    rng = np.random.default_rng(0)
    x, z, c = rng.standard_normal((G.N, 4)), rng.standard_normal((1, G.N, 4)), coeffs_of(rng, 1, 8)
    gd, go, _ = G.device_graph().cheby_laplacian_grad(c, x, z, G.lmax)
    E = edges_of(G)
    pick = rng.choice(E.shape[1], 64, replace=False)
    rd, ro = laplacian_grad_direct(orc.laplacian(G.W), G.lmax, c, x, z, E[:, pick])
    assert go.shape == (E.shape[1],) and rel_err(go[pick], ro) < TOL[F64] and rel_err(gd, rd) < TOL[F64]
