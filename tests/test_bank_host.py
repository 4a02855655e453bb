"""Host-side checks of what the wide-bank tests on the GPU rest on (tests/test_gpu_t_wide_banks.py, helpers in
tests/bank_helpers.py): the numpy restatements of the recurrence and of the Clenshaw synthesis agree with the oracle on
every bank of that module, filter by filter; the banks and the synthesis inputs can see the slips the module is there
to catch (a dropped panel, swapped coefficient rows, a filter index without its pass offset); the restated rules of
which launches take the tile kernel and of the column batches give the counts the module asserts.  No GPU.

Bar of the GPU module: gpu_helpers.TOL * 10 = 1e-10 (float64) / 2e-4 (float32) of every filter plane's own
max |reference|.

1. Restatements.  run_recurrence and run_clenshaw in the compute dtype must stay 10 times inside that bar, every
   filter plane on its own.  Measured here on 4 columns of rand65, hub3001 and sensor4097, the banks of (filters,
   order) = (7, 12), (8, 12), (9, 12), (16, 12), (17, 12), (33, 12), (40, 30) - the Clenshaw run of 33 and of 40 panels
   and sensor4097 included (the module prints the worst with -s):
       run_recurrence  float64 1.2e-14   float32 3.7e-6
       run_clenshaw    float64 4.6e-15   float32 1.3e-6
   54 times and more inside the bar; the generator's ratio 0.75 stays.

2. Sensitivity, numpy only, nothing of the library is mutated.  Figures are the least over every choice of panel, pair
   or filter, as multiples of the float32 bar 2e-4; each must exceed 100, and each is asserted on every graph:
                                       rand65    hub3001   sensor4097
       9 filters   dropped panel         672       495        795      of max |synthesis|
                   swapped rows         2292       934       2681      of the plane's max |reference|
                   f0 + f read as f     6441      6596       6501
       33 filters  dropped panel         155       225        172
                   swapped rows         1474       706       1339
                   f0 + f read as f     3790      2825       3029
   The dropped-panel figures decided the weights of the synthesis panels (bank_helpers.wide_synthesis_inputs).  With
   2^-(f mod 4), the first rule, the 33 panels on hub3001 sum to max |synthesis| = 5.5 on the hub's row and the lightest
   panel (weight 1/8) moves the result by 1.3e-2 of it, 64 bars; 2^-(f mod 3) gives 99.9 on sensor4097.  The factor 100
   stands, so the panels weigh 2^-(f mod 2): 1, 1/2, 1, 1/2, ... - no two panels alike still, by their rotation.

3. and 4.  tile_helpers.expected_kinds_recurrence for 7 to 40 filters and bank_helpers.batch_width / batches against
   counts worked out by hand from gspx_poly.hip.h (filter_dev_t, work_panels, batch_width).  The 2 GiB window of a
   synthesis, window(planes = nf), binds on no graph this small - 40 panels of 4097 rows of 36 float64 columns are
   47 MB - and is not restated."""
import numpy as np
import pytest

import bank_helpers as bh
from gpu_helpers import TOL
from oracle import cheby_oracle as orc
from recurrence_helpers import run_clenshaw, run_recurrence
from tile_helpers import expected_kinds_recurrence

NSIG = 4
INSIDE = 10.0
SENSITIVE = 100.0 * TOL[np.dtype(np.float32)] * 10  # 100 times the float32 bar


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    bh.report()


# ---- 1: the restatements -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("graph", bh.GRAPHS)
def test_restatements_match_the_oracle_filter_by_filter(graph, dtype):
    for nf, order in bh.BANKS:
        c = bh.synthesis_case(graph, nf, order)
        at = (graph, "nf=%d" % nf, "order=%d" % order)
        y = run_recurrence(c["L"], c["lmax"], c["coeffs"], c["x"][:, :NSIG], dtype)
        assert y.dtype == np.dtype(dtype)
        bh.hold_per_filter("run_recurrence", dtype, y, c["ana"][:, :, :NSIG], at, inside=INSIDE)
        z = run_clenshaw(c["L"], c["lmax"], c["coeffs"], c["s"][:, :, :NSIG], dtype)
        assert z.dtype == np.dtype(dtype)
        bh.hold_per_filter("run_clenshaw", dtype, z, c["syn"][:, :NSIG], at, inside=INSIDE)


def test_banks_and_inputs_are_what_they_claim():
    for nf, order in bh.BANKS:
        c = bh.bank(nf, order)
        assert c.shape == (nf, order + 1) and np.allclose(np.abs(c).sum(axis=1), 1.0, rtol=0, atol=1e-15)
        assert all(len(set(c[:, k])) == nf for k in range(order + 1))  # every filter differs in every coefficient
        assert np.array_equal(c, bh.bank(nf, order))
    x = bh.signals("rand65")
    assert x.shape == (65, 48) and np.array_equal(x.astype(np.float32).astype(np.float64), x)
    s = bh.wide_synthesis_inputs(x, 40)
    assert s.shape == (40, 65, 48) and np.array_equal(s.astype(np.float32).astype(np.float64), s)
    assert np.array_equal(s[0], x) and np.array_equal(s[1][:, 0], x[:, 5] / 2) and np.array_equal(s[11][:, 47], x[:, 6] / 2)
    assert np.array_equal(s[4][:, 3], x[:, 23]) and len({s[f][:, :1].tobytes() for f in range(40)}) == 40
    assert [np.abs(s[f]).max() / np.abs(x).max() for f in range(40)] == [1.0, 0.5] * 20
    # the reference made from the analysis is the oracle's synthesis of those panels, filter by filter
    c = bh.synthesis_case("rand65", 9, 12)
    direct = sum(orc.cheby_op(c["L"], c["lmax"], c["coeffs"][f], c["s"][f]) for f in range(9))
    assert np.max(np.abs(direct - c["syn"])) <= 1e-14 * np.max(np.abs(direct))


# ---- 2: the inputs can see the slips -------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [9, 33])
@pytest.mark.parametrize("graph", bh.GRAPHS)
def test_inputs_see_a_dropped_panel_swapped_rows_and_a_lost_pass_offset(graph, nf):
    c = bh.synthesis_case(graph, nf, 12)
    ana, syn = c["ana"], c["syn"]
    scale = np.abs(ana).max(axis=(1, 2))
    # a synthesis that leaves panel f out
    drop = min(np.abs(syn - bh.wide_synthesis_reference(ana, drop=(f,))).max() for f in range(nf)) / np.abs(syn).max()
    # coefficient rows a and b swapped: plane a holds p_b(L) x
    swap = min(np.abs(ana[a] - ana[b]).max() / scale[a] for a in range(nf) for b in range(nf) if a != b)
    # a pass of 8 filters from f0 on that reads (or writes) filter f0 + f as f
    shift = min(np.abs(ana[f0 + f] - ana[f]).max() / scale[f0 + f]
                for f0 in range(8, nf, 8) for f in range(min(8, nf - f0)))
    print("\n{} nf={}: dropped panel {:.0f}, swapped rows {:.0f}, lost pass offset {:.0f} float32 bars".format(
        graph, nf, drop / 2e-4, swap / 2e-4, shift / 2e-4), end="")
    assert drop > SENSITIVE and swap > SENSITIVE and shift > SENSITIVE, (graph, nf, drop, swap, shift)


# ---- 3: which launches take the tile kernel ------------------------------------------------------------------------
def test_the_launch_kind_rule_for_wide_banks():
    ek = expected_kinds_recurrence

    def tile(n):
        return {"tile": n, "plain": 0}

    def plain(n):
        return {"tile": 0, "plain": n}

    for nf in range(7, 41):
        for elt in (8, 4):
            for w in (1, 2, 3, 4, 6, 8, 20, 34):
                # deferred analysis (combine = 0 and 2 alike): K steps on the tiles, direct or padded, but for one column
                want = plain(12) if w == 1 else tile(12)
                assert ek(w, elt, nf, 12) == ek(w, elt, nf, 12, combine=2) == want, (nf, elt, w)
                assert ek(w, elt, nf, 12, tile_gather=0) == plain(12)
                # the fused flush of several filters: plain kernels at every width
                assert ek(w, elt, nf, 12, combine=1) == plain(12), (nf, elt, w)
                # synthesis: K + 1 Clenshaw steps, nf K steps of the per-filter loop
                want = plain if w == 1 else tile
                assert ek(w, elt, nf, 12, "synthesis") == want(13), (nf, elt, w)
                assert ek(w, elt, nf, 12, "synthesis", synthesis=1) == want(12 * nf), (nf, elt, w)
                assert ek(w, elt, nf, 12, "synthesis", combine=1) == want(13)  # (combine: analysis only)
                assert ek(w, elt, nf, 12, "synthesis", tile_gather=0) == plain(13)
            assert ek(20, elt, nf, 30) == tile(30)
            # column batches 8 + 8 + 4 of 20 signals: every batch whole pieces at a 16-byte aligned column of y
            assert ek(20, elt, nf, 12, max_batch=8) == tile(36)
            assert ek(20, elt, nf, 12, max_batch=8, combine=1) == plain(36)
            assert ek(6, elt, nf, 12, max_batch=1, combine=1) == plain(72)  # one-column batches
    # padded against direct work panels decide the combine's lane vector (bank_helpers.combine_vec)
    assert [bh.combine_vec(w, 8, w % 2 != 0) for w in (1, 2, 3, 4, 6, 8, 20, 34)] == [1, 1, 1, 1, 1, 1, 1, 2]
    assert [bh.combine_vec(w, 4, w % 4 != 0) for w in (1, 2, 3, 4, 6, 8, 20, 34)] == [1, 1, 1, 1, 1, 1, 1, 1]
    assert [bh.combine_vec(w, 4, False) for w in (1, 2, 3, 4, 6, 8, 20, 34)] == [1, 1, 1, 1, 1, 1, 1, 2]
    assert bh.combine_vec(8, 4, False, vec=4) == 4 and bh.combine_vec(20, 4, False, vec=4) == 4
    assert bh.combine_vec(8, 8, False, vec=4) == 1 and bh.combine_vec(8, 8, False, vec=2) == 2
    assert bh.combine_vec(6, 4, False, vec=4) == 1 and bh.combine_vec(6, 4, False, vec=2) == 2
    # the plain kernel of a batch (choose_shape)
    for elt in (8, 4):
        assert [bh.plain_kernel(w, elt) for w in (1, 2, 3, 4)] == ["narrow"] * 4
        assert [bh.plain_kernel(w, elt, 1) for w in (4, 6, 8, 20, 34)] == ["narrow"] + ["panel"] * 4
        assert [bh.plain_kernel(w, elt, 5) for w in (4, 6, 8, 20, 34)] == ["narrow"] + ["lds"] * 4
        assert [bh.plain_kernel(w, elt, 2) for w in (6, 8, 20, 34)] == ["narrow"] * 4
    assert [bh.plain_kernel(w, 8) for w in (6, 8, 20, 34)] == ["lds", "lds", "lds", "panel"]
    assert [bh.plain_kernel(w, 4) for w in (6, 8, 20, 34)] == ["lds"] * 4


# ---- 4: the column batches -----------------------------------------------------------------------------------------
def test_the_batch_width_rule():
    """Worked out by hand from batch_width and filter_dev_t: rowb = N elt bytes per work column; the window
    (2^31 - 65536) / rowb, the budget (ws_limit_mb << 20) / (rowb panels), panels = M for a deferred call and 2 + Nf for a
    fused one, max_batch; a width of 4 and more that does not take the whole call is rounded down to a multiple of 4."""
    bw, bt = bh.batch_width, bh.batches
    # no limit but the window: (2^31 - 65536) / (4097 * 8) = 65518 columns
    assert bw(4097, 8, 13, 20) == 65518 == (2 ** 31 - 65536) // (4097 * 8) and bt(4097, 8, 13, 20) == [20]
    # section C: 33 filters on 20 signals, max_batch = 8 -> 8 + 8 + 4, deferred (13 panels) and fused (35) alike
    for elt in (8, 4):
        for n in (65, 3001, 4097):
            assert bt(n, elt, 13, 20, max_batch=8) == [8, 8, 4] and bt(n, elt, 35, 20, max_batch=8) == [8, 8, 4]
    assert bt(4097, 8, 13, 20, max_batch=7) == [4] * 5 and bt(4097, 8, 13, 20, max_batch=3) == [3] * 6 + [2]
    assert bt(4097, 8, 13, 20, max_batch=20) == [20] and bt(4097, 8, 13, 21, max_batch=20) == [20, 1]
    # the fused bank of 33 on sensor4097 under ws_limit_mb = 1: 2^20 / (4097 * 8 * 35) = 0.91 and 2^20 / (4097 * 4 * 35)
    # = 1.83 columns - one-column batches in both dtypes
    assert bw(4097, 8, 35, 6, ws_limit_mb=1) == 1 and bw(4097, 4, 35, 6, ws_limit_mb=1) == 1
    assert bt(4097, 8, 35, 6, ws_limit_mb=1) == [1] * 6 and bt(4097, 4, 35, 6, ws_limit_mb=1) == [1] * 6
    # 7 and 9 filters: 2^20 / (4097 * 8 * 9) = 3.55 -> 3, 2^20 / (4097 * 4 * 11) = 5.8 -> 5, 4 when the call has more
    assert bw(4097, 8, 9, 6, ws_limit_mb=1) == 3 and bw(4097, 4, 11, 6, ws_limit_mb=1) == 4
    assert bt(4097, 4, 11, 6, ws_limit_mb=1) == [4, 2] and bw(4097, 4, 11, 5, ws_limit_mb=1) == 5
    # smaller graphs keep whole calls under the same limit: 2^20 / (65 * 8 * 35) = 57
    assert bt(65, 8, 35, 34, ws_limit_mb=1) == [34] and bw(3001, 8, 35, 34, ws_limit_mb=1) == 1
    assert bw(4097, 8, 35, 6, ws_limit_mb=0) == 1  # (a limit below 1 MB counts as 1 MB)
