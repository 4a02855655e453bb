"""The helpers of tests/test_gpu_u_*.py (operator_pins_helpers.py, tile_helpers.expected_kinds_lx) against slower
direct formulas, without a GPU: a wrong helper must not hide a wrong kernel.  Also where the float32 figures of
test_gpu_u_sqnorms_small.py come from: test_float32_figures_of_the_long_recurrences prints them."""
import math

import numpy as np
import pytest
from scipy import sparse

from conftest import rel_err
from gpu_helpers import TOL, random_graph, upper_lmax
from operator_pins_helpers import (EPS, LD, LONG_M, LONG_NF, bank_coefficients, caller_rows, combine_reference,
                                   directed_graph, edgeless_graph, isolated_vertex_graph, long_case, oracle_sqnorms,
                                   path_graph, projection_reference, self_loop_graph, shuffled_order, sqnorms_bar,
                                   sqnorms_carried, star_graph)
from oracle import cheby_oracle as orc
from oracle import ops_oracle as ops
from tile_helpers import expected_kinds_lx


def test_combine_reference_against_exact_sums():
    rng = np.random.default_rng(0)
    order, N, n, Nf = 5, 4, 3, 3
    V, w = rng.standard_normal((order, N, n)), rng.standard_normal((Nf, order, n))
    ref, bound = combine_reference(V, w)
    assert ref.shape == bound.shape == (Nf, N, n) and ref.dtype == LD
    for f in range(Nf):
        for i in range(N):
            for c in range(n):
                terms = [w[f, j, c] * V[j, i, c] for j in range(order)]  # (each product rounded once: 1 eps of |term|)
                exact, mag = math.fsum(terms), math.fsum(abs(t) for t in terms)
                assert abs(float(ref[f, i, c]) - exact) <= 2 * EPS * mag
                assert abs(float(bound[f, i, c]) - (order + 1) * EPS * mag) <= 4 * EPS * float(bound[f, i, c])


def test_combine_bound_leaves_room_for_a_float64_sum():
    """A float64 left-to-right sum on the CPU sits far inside the bound at the largest order anyone runs (60)."""
    rng = np.random.default_rng(1)
    order, N, n, Nf = 60, 257, 65, 9
    V, w = rng.standard_normal((order, N, n)), rng.standard_normal((Nf, order, n))
    ref, bound = combine_reference(V, w)
    y = np.zeros((Nf, N, n))
    for j in range(order):
        y += w[:, j, None, :] * V[None, j]
    worst = float(np.max(np.abs(y.astype(LD) - ref) / bound))
    print("float64 left-to-right sum: {:.3f} of the bound".format(worst))
    assert worst < 0.25


def test_combine_bound_sees_index_slips():
    """What a wrong index in k_lz_combine would give misses the bound by many orders of magnitude on the inputs the
    GPU module draws: a dropped last panel, the weights of the neighbouring filter, column or panel, rows written
    through the inverse of the vertex order."""
    rng = np.random.default_rng(4)
    order, N, n, Nf = 8, 70, 17, 9
    V, w = rng.standard_normal((order, N, n)), rng.standard_normal((Nf, order, n))
    ref, bound = combine_reference(V, w)
    perm = shuffled_order(rng, N)
    want, lim = caller_rows(ref, perm, 1), caller_rows(bound, perm, 1)
    good = caller_rows(np.einsum("fjc,jic->fic", w, V), perm, 1)
    assert np.all(np.abs(good.astype(LD) - want) <= lim)
    slips = {"dropped panel": np.einsum("fjc,jic->fic", w[:, :-1], V[:-1]),
             "next filter": np.einsum("fjc,jic->fic", np.roll(w, 1, axis=0), V),
             "next column": np.einsum("fjc,jic->fic", np.roll(w, 1, axis=2), V),
             "next panel": np.einsum("fjc,jic->fic", np.roll(w, 1, axis=1), V)}
    for name, y in slips.items():
        miss = np.abs(caller_rows(y, perm, 1).astype(LD) - want) / lim
        assert float(np.median(miss)) > 1e10, name
    # y[i] = internal[perm[i]] instead of y[perm[i]] = internal[i]
    inverse = np.einsum("fjc,jic->fic", w, V)[:, perm, :]
    assert float(np.median(np.abs(inverse.astype(LD) - want) / lim)) > 1e10


def test_projection_reference_against_exact_sums():
    rng = np.random.default_rng(2)
    order, N, n = 4, 7, 3
    V, x = rng.standard_normal((order, N, n)), rng.standard_normal((N, n))
    x[:, 1] = 0
    proj, bound = projection_reference(V, x)
    assert proj.shape == bound.shape == (order, n)
    for j in range(order):
        for c in range(n):
            terms = [V[j, i, c] * x[i, c] for i in range(N)]
            exact, mag = math.fsum(terms), math.fsum(abs(t) for t in terms)
            assert abs(float(proj[j, c]) - exact) <= 2 * EPS * mag
            assert abs(float(bound[j, c]) - (N + 2) * EPS * mag) <= 4 * EPS * float(bound[j, c])
    assert not proj[:, 1].any() and not bound[:, 1].any()


def test_caller_rows():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((2, 6, 3))
    perm = rng.permutation(6)
    out = caller_rows(a, perm, 1)
    for i in range(6):
        assert np.array_equal(out[:, perm[i], :], a[:, i, :])
    assert caller_rows(a, None, 1) is a
    b = rng.standard_normal((6, 3))
    assert np.array_equal(caller_rows(b, perm, 0)[perm], b)


def test_shuffled_order_is_never_the_identity():
    for n in (1, 2, 3, 5):
        for seed in range(40):
            perm = shuffled_order(np.random.default_rng(seed), n)
            assert perm.dtype == np.int32 and np.array_equal(np.sort(perm), np.arange(n))
            assert n == 1 or not np.array_equal(perm, np.arange(n))


def test_panel_of_an_empty_edge_signal():
    """DeviceGraph._panel (host code): the (0, w) edge signal of an edgeless graph keeps its w columns - div then
    returns N x w zeros; reshape(0, -1) used to raise here (found by test_gpu_u_grad_div_small)."""
    from pygsp_amd import engine
    dev = engine.DeviceGraph(None, None, 4, np.float32)
    x2, one_d = dev._panel(np.zeros((0, 5)), 0, "div")
    assert x2.shape == (0, 5) and x2.dtype == np.float32 and not one_d
    x2, one_d = dev._panel(np.zeros(0), 0, "div")
    assert x2.shape == (0, 1) and one_d
    x2, one_d = dev._panel(np.arange(8.0), 8, "grad")
    assert x2.shape == (8, 1) and one_d
    x2, one_d = dev._panel(np.arange(24.0).reshape(4, 3, 2), 4, "grad")
    assert x2.shape == (4, 6) and not one_d and np.array_equal(x2[1], np.arange(6, 12))
    with pytest.raises(ValueError):
        dev._panel(np.zeros((3, 2)), 4, "grad")


def direct_sqnorms(L, lmax, C, x):
    """The definition, column by column and filter by filter, on the dense matrix in float64:
    p_f(L) x = c_f0 / 2 x + sum_k c_fk T_k(2 L / lmax - I) x, then the sum of squares."""
    A = 2.0 * np.asarray(L.toarray()) / lmax - np.eye(L.shape[0])
    out = np.zeros((C.shape[0], x.shape[1]))
    for j in range(x.shape[1]):
        T = [x[:, j], A @ x[:, j]]
        for k in range(2, C.shape[1]):
            T.append(2.0 * (A @ T[k - 1]) - T[k - 2])
        for f in range(C.shape[0]):
            y = 0.5 * C[f, 0] * T[0]
            for k in range(1, C.shape[1]):
                y = y + C[f, k] * T[k]
            out[f, j] = float(y @ y)
    return out


@pytest.mark.parametrize("N", [1, 63, 257])
def test_sqnorms_carried_against_the_definition(N):
    W = random_graph(N, 4, seed=N) if N > 1 else sparse.csr_matrix((1, 1))
    L, lmax = orc.laplacian(W), (upper_lmax(W) if N > 1 else 1.0)
    x = np.random.default_rng(N).standard_normal((N, 3)).astype(np.float32).astype(np.float64)
    for nf, M in ((1, 2), (3, 3), (9, 31)):
        C = bank_coefficients(nf, M, seed=M)
        want = direct_sqnorms(L, lmax, C, x)
        assert rel_err(oracle_sqnorms(L, lmax, C, x), want) < 1e-12
        assert rel_err(sqnorms_carried(L, lmax, C, x, np.float64), want) < 1e-12
        assert rel_err(sqnorms_carried(L, lmax, C, x, np.longdouble), want) < 1e-12
        s32 = sqnorms_carried(L, lmax, C, x, np.float32)
        assert s32.dtype == np.float64 and rel_err(s32, want) < TOL[np.dtype(np.float32)]
        if N > 1:  # (really carried in float32: the float64 result is not reproduced)
            assert rel_err(s32, want) > 1e-9


def test_float32_figures_of_the_long_recurrences():
    """The figures behind the bars of test_gpu_u_sqnorms_small.test_long_recurrences, on its very inputs
    (operator_pins_helpers.long_case): the float32 recurrence against the float64 oracle, and the oracle against the
    longdouble recurrence.  The rule (sqnorms_bar): float32 gets max(TOL, 4 x figure); float64 keeps TOL as long as the
    oracle's own error stays below it - asserted here, so the GPU module never has to widen float64."""
    for nf in LONG_NF:
        for M in LONG_M:
            for dtype in (np.float32, np.float64):
                _, L, lmax, C, x, ref = long_case(nf, M, dtype)
                bar, fig = sqnorms_bar(L, lmax, C, x, dtype, ref, TOL[np.dtype(dtype)])
                print("sqnorms Nf {:3d} M {:3d} {:<8s} figure {:.2e} bar {:.2e}".format(
                    nf, M, np.dtype(dtype).name, fig, bar))
                assert np.isfinite(fig) and bar >= TOL[np.dtype(dtype)]
                if dtype == np.float64:
                    assert fig <= TOL[np.dtype(dtype)] and bar == TOL[np.dtype(dtype)]
                else:
                    assert fig < 1e-3  # (BASELINE.json's float32 bar: the rule stays far inside it)


def test_expected_kinds_lx():
    tile, plain = {"tile": 1, "plain": 0}, {"tile": 0, "plain": 1}
    assert expected_kinds_lx(4, 8) == tile and expected_kinds_lx(2, 8) == tile and expected_kinds_lx(4, 4) == tile
    assert expected_kinds_lx(3, 8) == plain and expected_kinds_lx(1, 8) == plain and expected_kinds_lx(6, 4) == plain
    assert expected_kinds_lx(4, 8, tile_gather=0) == plain and expected_kinds_lx(4, 8, tiles=False) == plain
    # off the fused route but still one batch on the tile kernel: the count is the same, the route is not
    for kw in (dict(fuse_input=0), dict(slow_blocks=1), dict(x_offset=8), dict(in_place=True)):
        assert expected_kinds_lx(4, 8, **kw) == tile
    # column batches: 20 fp64 columns in batches of 3 -> six batches of an odd width, then two columns at column 18
    assert expected_kinds_lx(20, 8, max_batch=3) == {"tile": 1, "plain": 6}
    assert expected_kinds_lx(19, 8, max_batch=3) == {"tile": 0, "plain": 7}
    assert expected_kinds_lx(20, 8, max_batch=4) == {"tile": 5, "plain": 0}
    assert expected_kinds_lx(20, 8, max_batch=8) == {"tile": 3, "plain": 0}
    assert expected_kinds_lx(20, 8, max_batch=7) == {"tile": 5, "plain": 0}  # (7 rounds down to 4)
    # fp32: batches of 3 never hold whole pieces; 6 columns are no whole pieces either, so y's rows rule the tile out
    assert expected_kinds_lx(8, 4, max_batch=3) == {"tile": 0, "plain": 3}
    assert expected_kinds_lx(6, 4, max_batch=4) == {"tile": 0, "plain": 2}
    assert expected_kinds_lx(12, 4, max_batch=8) == {"tile": 2, "plain": 0}
    # one column more than a batch: a last batch of one fp64 column is below a piece
    assert expected_kinds_lx(9, 8, max_batch=8) == {"tile": 0, "plain": 2}  # (9 columns: y's rows are no whole pieces)
    assert expected_kinds_lx(10, 8, max_batch=8) == {"tile": 2, "plain": 0}
    assert expected_kinds_lx(2, 8, tile_min_row=32) == plain


def test_tiny_graphs():
    for n in (1, 5, 9):
        W = path_graph(n)
        assert W.shape == (n, n) and W.nnz == 2 * (n - 1) and (W != W.T).nnz == 0
        assert np.array_equal(np.diff(W.indptr), [0] if n == 1 else [1] + [2] * (n - 2) + [1])
    for leaves in (12, 13, 14, 15):
        for hub_last in (False, True):
            W = star_graph(leaves, hub_last, seed=leaves)
            hub = leaves if hub_last else 0
            deg = np.diff(W.indptr)
            assert W.shape == (leaves + 1,) * 2 and deg[hub] == leaves and np.all(np.delete(deg, hub) == 1)
            src, dst, _ = ops.get_edge_list(W)
            assert src.size == leaves and np.all((dst if hub_last else src) == hub)
    W = isolated_vertex_graph()
    assert np.array_equal(np.diff(W.indptr), [2, 2, 3, 0, 2, 1]) and (W != W.T).nnz == 0
    assert edgeless_graph(4).nnz == 0 and ops.differential_operator(edgeless_graph(4)).shape == (4, 0)


def test_caller_edge_graphs_keep_l_equal_d_dt():
    """The directed and the self-loop graph of test_gpu_u_grad_div_small: what they are, and that L = D D^T holds on
    them for both Laplacian types - so div(grad(x)) may be held to the oracle's L x there."""
    A, S = directed_graph(), self_loop_graph()
    assert A.shape == S.shape == (40, 40)
    assert (A != A.T).nnz != 0 and not A.diagonal().any()
    assert (S != S.T).nnz == 0 and np.count_nonzero(S.diagonal()) == 6
    for W in (A, S):
        for lap_type in ("combinatorial", "normalized"):
            D, L = ops.differential_operator(W, lap_type), ops.laplacian(W, lap_type)
            assert abs(D.dot(D.T) - L).max() < 1e-14
