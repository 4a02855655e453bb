"""Graph reduction on the device (gspx_schur_cg_dev, gspx_kron_build, pygsp_amd.reduction).

Against the numpy restatement of tests/reduction_helpers.py: iteration counts exactly - every rtol comes from
cg.pick_rtol over [1e-11, 1e-9] ([1e-5, 1e-3] for float32), as in the harmonic-extension tests - and values within
cg.X64_TOL / cg.X32_TOL by conftest.rel_err.  Against what the reference computed (tests/golden/reduction.npz): the
a-priori bound of tests/test_reduction_host.py at rtol 1e-10, per column
||delta||_2 <= ||A_ku||_2 rtol ||b_j||_2 / lambda_min(A_uu) + 1e-13 max|ref|, without the ||A_ku|| factor for the
extension itself and times max|p(lambda)| over the fixture's eigenvalues for the Chebyshev route, p the package's own
order-100 approximant of the Green's kernel.  Every deviation is printed; profiles/reduction.md records them.
"""
import numpy as np
import pytest
from scipy import sparse

import reduction_helpers as rh
from conftest import csr_from, load_golden, rel_err
from learning_helpers import laplacian
from pygsp_amd import engine, filters, graphs, reduction

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
XTOL = {F64: rh.X64_TOL, F32: rh.X32_TOL}
RTOL = 1e-10
SEEN = {}


def seen(what, value):
    SEEN[what] = max(SEEN.get(what, 0.0), float(value))
    return "%.2e (file so far %.2e)" % (value, SEEN[what])


@pytest.fixture(scope="module")
def g():
    return load_golden("reduction.npz")


@pytest.fixture(scope="module")
def devices():
    """One DeviceGraph per (graph, dtype, permuted or not), destroyed at the end of the module."""
    ctx = engine.default_context(0)
    made = {}

    def get(key, dtype, permuted):
        pb = rh.problem(*key)
        k = (key[0], pb.N, dtype, permuted)
        if k not in made:
            made[k] = engine.DeviceGraph.from_w(pb.W, dtype=dtype, perm=pb.perm if permuted else None, ctx=ctx)
        return made[k]

    yield get
    for dev in made.values():
        dev.destroy()


def check_adjacency(W, Lnew):
    """W of a Kron reduction: canonical CSR, empty diagonal, no stored zero or negative value, its transpose bit for
    bit, and max(0, -offdiag(Lnew)) exactly."""
    W = W.download() if isinstance(W, engine.DeviceAdjacency) else W
    assert W.has_sorted_indices and W.shape == Lnew.shape
    assert not W.diagonal().any() and (W.nnz == 0 or W.data.min() > 0)
    assert (W != W.T).nnz == 0 and np.array_equal(Lnew, Lnew.T)
    assert np.array_equal(W.toarray(), rh.adjacency_of(Lnew).toarray())
    return W


@pytest.mark.parametrize("key", rh.KRON_PROBLEMS, ids=str)
def test_kron_against_the_restatement(devices, key):
    pb = rh.problem(*key)
    Lref, Wref, itr, rt = rh.kron_reference(key)
    for permuted in (True, False):
        Lnew, W, iters, _ = devices(key, F64, permuted).kron(pb.ind, pb.shift, rtol=rt, adjacency=True)
        err = rel_err(Lnew, Lref)
        print("%s perm=%d: nk %d, iters %d..%d, Lnew deviation %s" % (
            key, permuted, pb.ind.size, iters.min(), iters.max(), seen("kron", err)))
        assert np.array_equal(iters, itr), (key, permuted, np.flatnonzero(iters != itr), iters, itr)
        assert Lnew.shape == Lref.shape and err <= rh.X64_TOL, (key, permuted, err)
        W = check_adjacency(W, Lnew)
        assert rel_err(W.toarray(), Wref.toarray()) <= rh.X64_TOL
        assert np.array_equal(Lnew == 0, Lref == 0)  # what the iteration never reaches: exact zeros on both sides


def test_one_kept_vertex_without_a_shift(devices):
    """The exact result is the 1 x 1 zero matrix: the degree of the vertex cancels against A_ku A_uu^-1 A_uk.  Counts as
    the restatement's; the value within X64_TOL of the operands' scale (max |L|), and W is empty."""
    key = rh.ONE_KEPT_UNSHIFTED
    pb = rh.problem(*key)
    Lref, _, itr, rt = rh.kron_reference(key)
    for permuted in (True, False):
        Lnew, W, iters, _ = devices(key, F64, permuted).kron(pb.ind, 0.0, rtol=rt, adjacency=True)
        print("one kept vertex, shift 0: %r against %r, iters %d" % (Lnew[0, 0], Lref[0, 0], iters[0]))
        assert np.array_equal(iters, itr) and Lnew.shape == (1, 1) and W.nnz == 0
        assert abs(Lnew[0, 0] - Lref[0, 0]) <= rh.X64_TOL * abs(pb.L).max()


def test_kron_pieces_on_request(devices):
    pb = rh.problem(*rh.BASE)
    dev, rt = devices(rh.BASE, F64, True), rh.kron_reference(rh.BASE)[3]
    both = dev.kron(pb.ind, pb.shift, rtol=rt, adjacency=True)
    only_l = dev.kron(pb.ind, pb.shift, rtol=rt)
    only_w = dev.kron(pb.ind, pb.shift, rtol=rt, dense=False, adjacency=True)
    assert only_l[1] is None and only_w[0] is None
    assert both[0].tobytes() == only_l[0].tobytes()
    A, B = both[1].download(), only_w[1].download()
    assert A.indptr.tobytes() == B.indptr.tobytes() and A.indices.tobytes() == B.indices.tobytes()
    assert A.data.tobytes() == B.data.tobytes()  # (and two calls give the same bytes)
    with pytest.raises(ValueError):
        devices(rh.BASE, F32, True).kron(pb.ind)
    limit = dev.ctx.get_option("ws_limit_mb")
    dev.ctx.set_option("ws_limit_mb", 1)
    try:
        with pytest.raises(ValueError, match="ws_limit_mb"):
            dev.kron(np.arange(pb.N), 0.0)  # 300 x 300 doubles and five 300 x 256 panels: 3.6 MiB
    finally:
        dev.ctx.set_option("ws_limit_mb", limit)


SCHUR_KEYS = tuple(k for k in rh.SENSORS if k[1] in (65, 300)) + rh.SPLIT + (rh.ALL_KEPT, rh.ONE_KEPT) + rh.TINY[:4]


# (float32: the problems tests/test_reduction_host.py admits, reduction_helpers.FP32_PROBLEMS)
SCHUR_CASES = [(k, F64) for k in SCHUR_KEYS] + [(k, F32) for k in rh.FP32_PROBLEMS]


@pytest.mark.parametrize("key,dtype", SCHUR_CASES, ids=str)
def test_schur_cg_against_the_restatement(devices, key, dtype):
    pb = rh.problem(*key)
    xr, ar, itr, rt = rh.schur_reference(key, dtype)
    for permuted in (True, False):
        x, alpha, iters, _ = devices(key, dtype, permuted).schur_cg(pb.shift, pb.mask, pb.f, rtol=rt)
        ex, ea = rel_err(x, xr), rel_err(alpha, ar)
        print("%s %s perm=%d: iters %d..%d, x deviation %s, alpha deviation %s" % (
            key, np.dtype(dtype).name, permuted, iters.min(), iters.max(), seen("x" + np.dtype(dtype).name, ex),
            seen("alpha" + np.dtype(dtype).name, ea)))
        assert x.dtype == dtype and alpha.dtype == dtype and x.shape == pb.f.shape
        assert np.array_equal(iters, itr), (key, permuted, iters, itr)
        assert ex <= XTOL[dtype] and ea <= XTOL[dtype], (key, permuted, ex, ea)
        assert x[pb.mask].tobytes() == pb.f[pb.mask].astype(dtype).tobytes()
        assert not alpha[~pb.mask].any() and not np.signbit(alpha[~pb.mask]).any()  # exact zeros
        if key[0] == "split":  # the component that touches no kept vertex
            assert not x[64:].any() and x[:64][~pb.mask[:64]].any()


def test_schur_cg_kinds_of_call(devices):
    """Shift 0 gives the bytes of dirichlet_cg; two calls give the same bytes; NaN at eliminated rows of f is harmless;
    a 1-D f."""
    for key in (rh.BASE, ("sensor", 300, "third", 0.0)):
        pb = rh.problem(*key)
        for dtype in (F64, F32):
            rt = rh.schur_reference(key, dtype)[3]
            for permuted in (True, False):
                dev = devices(key, dtype, permuted)
                x, alpha, it, _ = dev.schur_cg(pb.shift, pb.mask, pb.f, rtol=rt)
                x2, alpha2, it2, _ = dev.schur_cg(pb.shift, pb.mask, pb.nan_f, rtol=rt)
                assert np.isfinite(x2).all() and x.tobytes() == x2.tobytes() and alpha.tobytes() == alpha2.tobytes()
                assert np.array_equal(it, it2)
                x0, _, it0, _ = dev.schur_cg(0.0, pb.mask, pb.f, rtol=rt)
                xd, itd, _ = dev.dirichlet_cg(pb.mask, pb.f, rtol=rt)
                assert x0.tobytes() == xd.tobytes() and np.array_equal(it0, itd)
                x1, a1, _, _ = dev.schur_cg(pb.shift, pb.mask, pb.f[:, 1], rtol=rt)  # (another thread map: not the bytes)
                assert x1.shape == a1.shape == (pb.N,)
                assert rel_err(x1, x[:, 1]) <= XTOL[dtype] and rel_err(a1, alpha[:, 1]) <= XTOL[dtype]
    with pytest.raises(ValueError):
        dev.schur_cg(-1.0, pb.mask, pb.f)


# ---- against the reference's results -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_graphs(g):
    return {gr: graphs.Graph(csr_from(g, gr + "_W"), coords=g[gr + "_coords"], plotting={"vertex_size": 7},
                             compute_dtype=F64) for gr in ("k64", "k300")}


def test_kron_meets_the_bound_on_every_case_of_the_fixture(g, golden_graphs):
    for gr, s, k in rh.golden_kron_cases(g):
        G, shift, ind = golden_graphs[gr], float(g["shifts"][k]), g["%s_%s_ind" % (gr, s)]
        L = laplacian(csr_from(g, gr + "_W"))
        bound = rh.bounds(L, shift, ind, np.eye(ind.size), RTOL)
        ref = rh.unpack(g, "%s_%s_L%d" % (gr, s, k))
        out = reduction.kron_reduction(sparse.csr_matrix(L + shift * sparse.identity(G.N)), ind)  # the matrix form
        Lnew = out.toarray()
        ok, ratio = rh.within(Lnew, ref, bound)
        print("%s %s shift %g: Lnew error / bound %s" % (gr, s, shift, seen("Lnew / bound", ratio)))
        assert sparse.isspmatrix_csr(out) and ok, (gr, s, k, ratio)
        assert not (Lnew != 0)[ref == 0].any()
        assert not ((Lnew == 0) & (np.abs(ref) > (bound + rh.FLOOR * np.abs(ref).max())[None, :])).any()
        if shift == 0:  # the Graph form
            Gn = reduction.kron_reduction(G, ind)
            assert Gn._adj_dev is not None and Gn.N == ind.size and Gn.lap_type == "combinatorial"
            assert np.array_equal(Gn.coords, g[gr + "_coords"][ind]) and Gn.plotting == G.plotting
            W = check_adjacency(Gn.W, G.device_graph().kron(ind, 0.0, RTOL)[0])  # (the same device graph: the same bits)
            ok, ratio = rh.within(W.toarray(), np.maximum(rh.unpack(g, "%s_%s_GW" % (gr, s)), 0.0), bound)
            print("%s %s: W error / bound %s" % (gr, s, seen("W / bound", ratio)))
            assert ok, (gr, s, ratio)
            assert abs(Gn.L - laplacian(W)).max() <= 1e-13 * abs(Gn.L).max()


def cheb_response(G, eps, order, lam):
    """max |p(lambda)| of the package's own order-`order` approximant of 1 / (eps + x) on G (lmax as set)."""
    c = filters.compute_cheby_coeff(filters.Filter(G, lambda x: 1.0 / (eps + x)), m=order)
    t = 2.0 * np.asarray(lam) / G.lmax - 1.0
    return float(np.abs(np.polynomial.chebyshev.chebval(t, np.concatenate([[c[0] / 2], c[1:]]))).max())


@pytest.mark.parametrize("s", ["even", "third"])
def test_interpolate_against_the_fixture(g, golden_graphs, s):
    G, ind, f, eps = golden_graphs["k64"], g["k64_%s_ind" % s], g["i_%s_f" % s], float(g["reg_eps"])
    L = laplacian(csr_from(g, "k64_W"))
    G._lmax, G._lmax_method = float(g["i_lmax"]), "lanczos"  # the lmax the reference used
    mask = np.zeros(G.N, dtype=bool)
    mask[ind] = True
    full = np.zeros((G.N, 3))
    full[ind] = f
    alpha = G.device_graph().schur_cg(eps, mask, full, rtol=RTOL)[1]
    b_alpha = rh.bounds(L, eps, ind, f, RTOL)
    ok, ratio = rh.within(alpha[ind], g["i_%s_Kf" % s], b_alpha)
    print("alpha error / bound %s" % seen("alpha / bound", ratio))
    assert ok and not alpha[~mask].any(), ratio
    x = reduction.interpolate(G, f, ind, reg_eps=eps, method="exact")
    ok, ratio = rh.within(x, g["i_%s_exact" % s], rh.bounds(L, eps, ind, f, RTOL, with_aku=False))
    print("exact error / bound %s" % seen("exact / bound", ratio))
    assert x.shape == (G.N, 3) and ok and np.array_equal(x[ind], f), ratio
    y = reduction.interpolate(G, f, ind, order=100, reg_eps=eps)
    ok, ratio = rh.within(y, g["i_%s_cheb" % s], b_alpha * cheb_response(G, eps, 100, g["i_e"]))
    print("chebyshev error / bound %s" % seen("chebyshev / bound", ratio))
    assert y.shape == (G.N, 3) and ok, ratio
    # shapes and kinds: (nk,) in gives (N, 1) out; a DeviceArray in gives a DeviceArray out, the same numbers
    y1 = reduction.interpolate(G, f[:, 0], ind, order=100, reg_eps=eps)
    assert y1.shape == (G.N, 1) and rh.within(y1, g["i_%s_cheb" % s][:, :1], b_alpha[:1] * cheb_response(G, eps, 100, g["i_e"]))[0]
    fd = engine.DeviceArray.from_host(G.context, f)
    yd = reduction.interpolate(G, fd, ind, order=100, reg_eps=eps)
    assert isinstance(yd, engine.DeviceArray) and yd.shape == (G.N, 3) and np.array_equal(np.asarray(yd), y)


def test_pyramid_against_the_fixture(g, golden_graphs):
    """graph_multiresolution with the fixture's kept sets replayed through the callable; the reference's own graphs for
    the transform, so that what differs is the interpolation's solve: per level the Chebyshev bound above for the
    signal that is interpolated there, and the sum of the levels' bounds for the synthesis."""
    G = graphs.Graph(csr_from(g, "k64_W"), coords=g["k64_coords"], compute_dtype=F64)
    Gs = reduction.graph_multiresolution(G, 2, sparsify=False, downsampling_method=lambda G, l: g["p_idx%d" % (l + 1)])
    assert [H.N for H in Gs] == [64, 29, 14]
    orig = np.arange(64)
    for l in (1, 2):
        orig = orig[g["p_idx%d" % l]]
        assert np.array_equal(Gs[l].mr["idx"], g["p_idx%d" % l]) and np.array_equal(Gs[l].mr["orig_idx"], orig)
        assert Gs[l].mr["level"] == l - 1 and "K_reg" not in Gs[l].mr and "green_kernel" in Gs[l - 1].mr
    with pytest.raises(NotImplementedError, match="graph_sparsify"):
        reduction.graph_multiresolution(G, 2)
    # the levels as the reference has them, each reduced from the reference's finer level
    ref_W = [csr_from(g, "k64_W")] + [sparse.csr_matrix(np.maximum(rh.unpack(g, "p_W%d" % l), 0.0)) for l in (1, 2)]
    Rs = [graphs.Graph(W, compute_dtype=F64) for W in ref_W]
    for l in (1, 2):
        ind = g["p_idx%d" % l]
        Lf = laplacian(ref_W[l - 1])
        ok, ratio = rh.within(reduction.kron_reduction(Rs[l - 1], ind).W.toarray(), ref_W[l].toarray(),
                              rh.bounds(Lf, 0.0, ind, np.eye(ind.size), RTOL))
        print("level %d: W error / bound %s" % (l, seen("pyramid W / bound", ratio)))
        assert ok, (l, ratio)
        Rs[l].mr = {"idx": ind}
    for l in range(3):
        Rs[l]._lmax, Rs[l]._lmax_method = float(g["p_lmax"][l]), "lanczos"
    f, eps = g["p_f"], 0.005
    ca, pe = reduction.pyramid_analysis(Rs, f)
    rec, _ = reduction.pyramid_synthesis(Rs, ca[2], pe)
    level_bound = []
    for l in range(2):  # the interpolation of level l: ca[l + 1] from the kept vertices of Rs[l]
        Lf, ind = laplacian(ref_W[l]), g["p_idx%d" % (l + 1)]
        lam = np.linalg.eigvalsh(Lf.toarray())
        level_bound.append(rh.bounds(Lf, eps, ind, g["p_ca%d" % (l + 1)], RTOL) * max(
            cheb_response(Rs[l], eps, 100, lam), cheb_response(Rs[l], eps, 30, lam)))
    checks = [("ca1", ca[1], g["p_ca1"], level_bound[0]), ("ca2", ca[2], g["p_ca2"], level_bound[0] + level_bound[1]),
              ("pe0", pe[0], g["p_pe0"], level_bound[0]), ("pe1", pe[1], g["p_pe1"], level_bound[0] + level_bound[1]),
              ("rec", rec, g["p_rec"], 2 * (level_bound[0] + level_bound[1]))]
    for name, got, ref, bound in checks:
        ok, ratio = rh.within(got, ref, bound)
        print("%s: error / bound %s" % (name, seen("pyramid / bound", ratio)))
        assert got.shape == ref.shape and ok, (name, ratio)
    # a signal comes back from its own pyramid - on the device-built levels too, 1-D signals as (N, 1) - when the
    # synthesis interpolates at the order the analysis did (the defaults are the reference's: 100 there, 30 here)
    for levels, sig in ((Rs, f), (Gs, f), (Gs, f[:, 0])):
        ca, pe = reduction.pyramid_analysis(levels, sig)
        rec, cas = reduction.pyramid_synthesis(levels, ca[-1], pe, order=100)
        sig2 = sig.reshape(64, -1)
        assert rec.shape == sig2.shape and pe[0].shape == sig2.shape and len(cas) == 3
        err = np.abs(rec - sig2).max() / np.abs(sig2).max()
        print("reconstruction: %s" % seen("reconstruction", err))
        assert err <= 1e-12
    with pytest.raises(NotImplementedError):
        reduction.pyramid_synthesis(Gs, ca[-1], pe, least_squares=True)


def test_the_real_pygsp_seam():
    pygsp = pytest.importorskip("pygsp")
    from pygsp import reduction as ref_reduction
    from pygsp_amd import plugin
    g = load_golden("reduction.npz")
    G = pygsp.graphs.Graph(csr_from(g, "k64_W"), coords=g["k64_coords"])
    ind, f = g["k64_even_ind"], g["i_even_f"]
    G.estimate_lmax()
    G.mr = {}
    want = ref_reduction.kron_reduction(G, ind)
    want_i = ref_reduction.interpolate(G, f[:, 0], ind)
    plugin.install(reduction=True)
    try:
        got = ref_reduction.kron_reduction(G, ind)
        assert isinstance(got, pygsp.graphs.Graph) and got.N == ind.size
        L = laplacian(csr_from(g, "k64_W"))
        assert rh.within(got.W.toarray(), np.maximum(want.W.toarray(), 0), rh.bounds(L, 0.0, ind, np.eye(ind.size), RTOL))[0]
        M = G.L + 0.005 * sparse.identity(G.N)
        assert rh.within(ref_reduction.kron_reduction(M, ind).toarray(), rh.unpack(g, "k64_even_L1"),
                         rh.bounds(L, 0.005, ind, np.eye(ind.size), RTOL))[0]
        got_i = ref_reduction.interpolate(G, f[:, 0], ind)
        bound = rh.bounds(L, 0.005, ind, f[:, :1], RTOL) * cheb_response(G, 0.005, 100, np.linalg.eigvalsh(L.toarray()))
        assert got_i.shape == want_i.shape and rh.within(got_i, want_i, bound)[0]
        # what does not qualify goes to the original: a normalized Laplacian raises its NotImplementedError
        with pytest.raises(NotImplementedError):
            ref_reduction.kron_reduction(pygsp.graphs.Graph(csr_from(g, "k64_W"), lap_type="normalized"), ind)
    finally:
        plugin.uninstall()
    assert ref_reduction.kron_reduction.__module__ == "pygsp.reduction"
