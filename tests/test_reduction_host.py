"""pygsp_amd.reduction on the host: the numpy restatement of the two device entry points (tests/reduction_helpers.py)
against what the reference computed (tests/golden/reduction.npz), and everything of the module that is decided before
the device is touched - the split of Lap(W) + sigma I, the host route, argument errors, the pyramid's bookkeeping.

The bound is a-priori, per column j: ||delta||_2 <= ||A_ku||_2 rtol ||b_j||_2 / lambda_min(A_uu) + 1e-13 max|ref|,
computed here from the fixture's own matrices (reduction_helpers.bounds); no tuned constant.  Measured: the restatement
stays at or below 0.23 of it (printed by the first test).
"""
import numpy as np
import pytest
from scipy import sparse

import reduction_helpers as rh
from conftest import csr_from, load_golden
from learning_helpers import laplacian
from pygsp_amd import engine, reduction

RTOL = 1e-10


@pytest.fixture(scope="module")
def g():
    return load_golden("reduction.npz")


@pytest.fixture(scope="module")
def solved(g):
    """The restatement at rtol 1e-10 for every Kron case of the fixture, computed once: key -> (L, shift, ind, Lnew, W,
    bound per column)."""
    out = {}
    for gr, s, k in rh.golden_kron_cases(g):
        L, shift, ind = laplacian(csr_from(g, gr + "_W")), float(g["shifts"][k]), g["%s_%s_ind" % (gr, s)]
        Lnew, W, iters, _ = rh.kron(L, shift, ind, RTOL)
        out[(gr, s, k)] = (L, shift, ind, Lnew, W, rh.bounds(L, shift, ind, np.eye(ind.size), RTOL), iters)
    return out


def test_restatement_meets_the_bound_on_every_kron_case(g, solved):
    worst = 0.0
    for (gr, s, k), (_, _, ind, Lnew, _, bound, iters) in solved.items():
        ref = rh.unpack(g, "%s_%s_L%d" % (gr, s, k))
        ok, ratio = rh.within(Lnew, ref, bound)
        print("%s %s shift %g: nk %d, iterations %d..%d, error / bound %.3f" % (
            gr, s, g["shifts"][k], ind.size, iters.min(), iters.max(), ratio))
        worst = max(worst, ratio)
        assert Lnew.shape == ref.shape and ok, (gr, s, k, ratio)
        assert np.array_equal(Lnew, Lnew.T)
    print("largest error / bound: %.3f" % worst)


def test_pattern_is_the_references_less_what_lies_under_the_bound(g, solved):
    for (gr, s, k), (_, _, _, Lnew, _, bound, _) in solved.items():
        ref = rh.unpack(g, "%s_%s_L%d" % (gr, s, k))
        assert not (Lnew != 0)[ref == 0].any(), (gr, s, k)  # every non-zero here is one of the reference
        lim = bound + rh.FLOOR * np.abs(ref).max()
        missing = (Lnew == 0) & (np.abs(ref) > lim[None, :])
        assert not missing.any(), (gr, s, k, int(missing.sum()))


def test_graph_form_adjacency(g, solved):
    for (gr, s, k), (_, _, _, _, W, bound, _) in solved.items():
        if g["shifts"][k] != 0:
            continue
        ref = rh.unpack(g, "%s_%s_GW" % (gr, s))
        ok, ratio = rh.within(W.toarray(), np.maximum(ref, 0.0), bound)
        assert ok, (gr, s, ratio)
        assert not W.diagonal().any() and W.nnz and W.data.min() > 0 and abs(W - W.T).max() == 0
        # what the reference keeps and this drops: negative weights from rounding, all under the floor
        assert ref.min() > -rh.FLOOR * np.abs(ref).max()


@pytest.mark.parametrize("s", ["even", "third"])
def test_interpolate_needs_no_k_reg(g, s):
    L, ind, f = laplacian(csr_from(g, "k64_W")), g["k64_%s_ind" % s], g["i_%s_f" % s]
    eps = float(g["reg_eps"])
    F, mask = np.zeros((64, f.shape[1])), np.zeros(64, dtype=bool)
    F[ind], mask[ind] = f, True
    x, alpha, _, _ = rh.extension(L, eps, mask, F, RTOL)
    ok, ratio = rh.within(alpha[ind], g["i_%s_Kf" % s], rh.bounds(L, eps, ind, f, RTOL))
    assert ok and not alpha[~mask].any(), ratio
    ok, ratio = rh.within(x, g["i_%s_exact" % s], rh.bounds(L, eps, ind, f, RTOL, with_aku=False))
    assert ok and np.array_equal(x[ind], f), ratio
    # the reference's default route approximates the Green's kernel at order 100: percents away from the exact one
    assert 1e-3 < np.abs(g["i_%s_cheb" % s] - g["i_%s_exact" % s]).max() < 1.0


def test_split_of_a_shifted_laplacian(g):
    W = csr_from(g, "k64_W")
    L = laplacian(W)
    for sigma in (0.0, 0.005, 2.5):
        for split in (reduction.split_laplacian, rh.split_shift):
            Wp, sp = split(L + sigma * sparse.identity(64))
            assert abs(Wp - W).max() < 1e-14 and abs(sp - sigma) < 1e-13
    bad = sparse.lil_matrix(L)
    j = int(W[0].indices[0])  # a neighbour of vertex 0
    bad[0, j] = bad[j, 0] = 0.5  # a positive off-diagonal
    lop = sparse.lil_matrix(L)
    lop[0, j] = lop[0, j] * 2  # not symmetric
    rows = L + sparse.diags(np.arange(64) * 1e-3)  # no constant row sum
    for M in (bad, lop, rows, L - 0.1 * sparse.identity(64)):
        assert reduction.split_laplacian(M.tocsr()) is None and rh.split_shift(M.tocsr()) is None


def test_other_matrices_take_the_host_route(g):
    L = laplacian(csr_from(g, "k64_W"))
    M = sparse.csr_matrix(L + sparse.diags(1.0 + np.arange(64) * 1e-2))
    ind = g["k64_third_ind"]
    out = reduction.kron_reduction(M, ind)  # no device here: the host route alone can answer
    A = M.toarray()
    comp = np.setdiff1d(np.arange(64), ind)
    ref = A[np.ix_(ind, ind)] - A[np.ix_(ind, comp)] @ np.linalg.solve(A[np.ix_(comp, comp)], A[np.ix_(comp, ind)])
    assert sparse.issparse(out) and np.abs(out.toarray() - ref).max() < 1e-12
    everything = reduction.kron_reduction(M, np.arange(64)[::-1].copy())
    assert np.abs(everything.toarray() - A[::-1, ::-1]).max() == 0


class StubGraph:
    """What the argument checks read of a graph - no device behind it."""

    def __init__(self, L, lap_type="combinatorial", directed=False):
        self.L, self.N, self.n_vertices, self.lap_type, self._directed = L, L.shape[0], L.shape[0], lap_type, directed
        self.plotting, self._U, self.lmax_calls = {}, None, 0

    def is_directed(self):
        return self._directed

    def estimate_lmax(self):
        self.lmax_calls += 1


BAD_IND = ([], [3, 3], [-1, 2], [0, 64], [[0, 1]], [0.5, 1.0], [True, False])


def test_argument_errors_come_before_the_device(g):
    L = laplacian(csr_from(g, "k64_W"))
    with pytest.raises(NotImplementedError, match="normalized"):
        reduction.kron_reduction(StubGraph(L, "normalized"), [0, 1])
    with pytest.raises(NotImplementedError, match="undirected"):
        reduction.kron_reduction(StubGraph(L, directed=True), [0, 1])
    for ind in BAD_IND:
        with pytest.raises(ValueError):
            engine.check_kept(ind, 64)
        with pytest.raises(ValueError):
            reduction.kron_reduction(StubGraph(L), ind)
        with pytest.raises(ValueError):
            reduction.kron_reduction(L, ind)
        with pytest.raises(ValueError):
            reduction.interpolate(StubGraph(L), np.zeros(max(len(ind), 1)), ind)
    with pytest.raises(TypeError):
        reduction.kron_reduction(L.toarray(), [0, 1])
    with pytest.raises(ValueError, match="f_subsampled"):
        reduction.interpolate(StubGraph(L), np.zeros(3), [0, 1])
    with pytest.raises(ValueError, match="Unknown method"):
        reduction.interpolate(StubGraph(L), np.zeros(2), [0, 1], method="lanczos")
    assert np.array_equal(engine.check_kept(np.array([5, 2, 9]), 10), [5, 2, 9])


def test_what_is_not_provided_says_so(g):
    G = StubGraph(laplacian(csr_from(g, "k64_W")))
    with pytest.raises(NotImplementedError, match="graph_sparsify"):
        reduction.graph_multiresolution(G, 2)  # the default call, as the reference's on a current SciPy
    with pytest.raises(NotImplementedError, match="downsampling"):
        reduction.graph_multiresolution(G, 2, sparsify=False, downsampling_method="random")
    with pytest.raises(NotImplementedError, match="reduction method"):
        reduction.graph_multiresolution(G, 2, sparsify=False, reduction_method="sum")
    assert G.lmax_calls == 0 and not hasattr(G, "mr")
    with pytest.raises(NotImplementedError, match="least-squares"):
        reduction.pyramid_synthesis([G, G], np.zeros(64), [np.zeros(64)], least_squares=True)
    with pytest.raises(ValueError, match="PYRAMID ANALYSIS"):
        reduction.pyramid_analysis([G, G], np.zeros(63))
    with pytest.raises(ValueError, match="different shapes"):
        reduction.pyramid_synthesis([G, G], np.zeros(64), [])
    assert not hasattr(reduction, "graph_sparsify") and not hasattr(reduction, "tree_multiresolution")


def test_replay_of_the_fixtures_idx_through_a_callable(g, monkeypatch):
    """graph_multiresolution's bookkeeping with the kept sets fixed by a callable and kron_reduction replaced by the
    restatement: idx, orig_idx, level and green_kernel per level, the levels' W against the reference's."""
    L0 = laplacian(csr_from(g, "k64_W"))
    asked = []

    def host_kron(G, ind, **kwargs):
        return StubGraph(laplacian(rh.kron(G.L, 0.0, ind, RTOL)[1]))

    def replay(G, level):
        asked.append((G.N, level))
        return g["p_idx%d" % (level + 1)]

    monkeypatch.setattr(reduction, "kron_reduction", host_kron)
    Gs = reduction.graph_multiresolution(StubGraph(L0), 2, sparsify=False, downsampling_method=replay)
    assert [G.N for G in Gs] == [64, 29, 14] and asked == [(64, 0), (29, 1)]
    assert all(G.lmax_calls == 1 for G in Gs)
    orig = np.arange(64)
    for l in (1, 2):
        orig = orig[g["p_idx%d" % l]]
        mr = Gs[l].mr
        assert np.array_equal(mr["idx"], g["p_idx%d" % l]) and np.array_equal(mr["orig_idx"], orig)
        assert mr["level"] == l - 1 and "K_reg" not in mr
        assert float(Gs[l - 1].mr["green_kernel"].evaluate(np.array([0.0]))[0, 0]) == 1.0 / 0.005
    assert "green_kernel" not in Gs[2].mr
    # each level against the reference's, reduced from the reference's own finer level (the a-priori bound is for one
    # reduction of one matrix)
    finer = L0
    for l in (1, 2):
        ind, ref = g["p_idx%d" % l], np.maximum(rh.unpack(g, "p_W%d" % l), 0.0)
        ok, ratio = rh.within(rh.kron(finer, 0.0, ind, RTOL)[1].toarray(), ref, rh.bounds(finer, 0.0, ind, np.eye(ind.size), RTOL))
        assert ok, (l, ratio)
        finer = laplacian(sparse.csr_matrix(ref))
    W1 = (sparse.diags(Gs[1].L.diagonal()) - Gs[1].L).toarray()
    assert np.array_equal(W1, rh.kron(L0, 0.0, g["p_idx1"], RTOL)[1].toarray())


def test_largest_eigenvector_set_is_the_references(g):
    G = StubGraph(laplacian(csr_from(g, "k64_W")))
    assert np.array_equal(reduction._largest_eigenvector_set(G), g["p_idx1"])  # eigsh on the host
    G._U = G.U = np.linalg.eigh(G.L.toarray())[1]
    assert np.array_equal(reduction._largest_eigenvector_set(G), g["p_idx1"])  # the basis that is there


def test_the_seam_routes_what_does_not_qualify_to_the_original():
    """plugin.install(reduction=True) on a pygsp-shaped stand-in: both names are replaced, inputs the device route
    does not take reach the package's own functions with their arguments, uninstall puts the originals back."""
    import types
    from pygsp_amd import plugin
    calls = []
    mod = types.ModuleType("standin")
    mod.filters = types.ModuleType("standin.filters")
    mod.filters.approximations = types.ModuleType("standin.filters.approximations")
    mod.filters.approximations.cheby_op = mod.filters.cheby_op = lambda *a, **k: None
    mod.graphs = types.ModuleType("standin.graphs")
    mod.graphs.Graph = type("Graph", (StubGraph,), {})
    mod.reduction = types.ModuleType("standin.reduction")
    mod.reduction.kron_reduction = lambda G, ind: calls.append(("kron", ind)) or "original kron"
    mod.reduction.interpolate = lambda G, f, keep, order=100, reg_eps=0.005, **kw: (
        calls.append(("interpolate", order, reg_eps, kw)) or "original interpolate")
    originals = (mod.reduction.kron_reduction, mod.reduction.interpolate)
    L = laplacian(csr_from(load_golden("reduction.npz"), "k64_W"))
    plugin.install(mod)
    assert (mod.reduction.kron_reduction, mod.reduction.interpolate) == originals  # opt-in
    plugin.install(mod, reduction=True)
    try:
        assert mod.reduction.kron_reduction is not originals[0] and mod.reduction.interpolate is not originals[1]
        normalized, directed = mod.graphs.Graph(L, "normalized"), mod.graphs.Graph(L, directed=True)
        dense = mod.graphs.Graph(L.toarray())
        for G, ind in ((normalized, [0, 1]), (directed, [0, 1]), (dense, [0, 1]), (mod.graphs.Graph(L), [0, 0]),
                       (L + sparse.diags(np.arange(64.0)), [0, 1]), (L.toarray(), [0, 1])):
            assert mod.reduction.kron_reduction(G, ind) == "original kron" and calls.pop() == ("kron", ind)
        G = mod.graphs.Graph(L)
        for f, keep, kw in ((np.zeros(3), [0, 1], {}), (np.zeros(2), [0, 99], {}), (np.zeros(2), [0, 1], {"method": "lanczos"}),
                            (np.zeros(2), [0, 1], {"i": 0}), (np.zeros((2, 1, 1)), [0, 1], {})):
            assert mod.reduction.interpolate(G, f, keep, order=7, **kw) == "original interpolate"
            assert calls.pop() == ("interpolate", 7, 0.005, kw)
        assert mod.reduction.interpolate(dense, np.zeros(2), [0, 1]) == "original interpolate"
    finally:
        plugin.uninstall(mod)
    assert (mod.reduction.kron_reduction, mod.reduction.interpolate) == originals


def test_fp32_admission():
    """X32_TOL is ten times what two float32 restatements differ by; a problem on which they differ by more than a
    tenth of it cannot be held to it.  Counts agree between the two on every candidate."""
    from conftest import rel_err
    for key in rh.FP32_CANDIDATES:
        pb = rh.problem(*key)
        x, alpha, iters, rtol = rh.schur_reference(key, np.float32)
        x2, alpha2, iters2, _ = rh.extension(pb.L, pb.shift, pb.mask, pb.f, rtol, dt=np.float32, acc=np.float32)
        dev = max(rel_err(x2, x), rel_err(alpha2, alpha))
        print("%s: iterations %s, the two float32 restatements differ by %.2e" % (key, iters, dev))
        assert np.array_equal(iters, iters2)
        assert (dev <= rh.X32_TOL / 10) == (key not in rh.FP32_EXCLUDED), (key, dev)
