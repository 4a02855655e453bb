"""Filter banks wider than one combine pass - 7 to 40 filters - on every device route of the Chebyshev path and on the
Lanczos combine, at small shapes: the deferred combine (k_combine, 8 filters per pass), the fused flush of all
accumulators inside the plain step kernels (combine = 1), column batches of a wide bank, the Clenshaw synthesis reading
Nf extra input panels per step on the tile kernels and on the plain ones, the per-filter synthesis loop,
k_lz_combine<FB> over several passes, and the seams (Filter.filter with host and device arrays, the pipelined host
call, replay).  `-m gpu`.  The whole module runs with graph_launch = 0 - every call eager, counting its own launches -
but the replay test.

Graphs: rand65 (2 blocks), hub3001 (47 blocks, a slow block) and sensor4097 (65 blocks) of tile_helpers, tiles from both
builders where tiles matter, both dtypes; 48 signal columns and banks of bank_helpers (coefficients that do not depend
on the graph; the oracle's float64 analysis once per graph and bank).  Widths 1, 2, 3, 4, 6, 8, 20, 34: the narrow
kernel, direct tiles, padded tiles (3 pads to 4, 6 to 8 and 34 to 36 in float32), the regrouped 48- / 80- / 160-byte
rows (6 and 20 float64 columns, 20 float32 columns).  An order-12 bank runs K = 12 steps, its Clenshaw synthesis
K + 1 = 13, its per-filter synthesis Nf K.

Every call asserts Context.last_step_kinds() as an equality against the restated rule (tile_helpers.
expected_kinds_recurrence; tests/test_bank_host.py checks that rule by hand for 7 to 40 filters) and every filter plane
on its own against the oracle (bank_helpers.hold_per_filter): max |y_f - ref_f| / max |ref_f| under gpu_helpers.TOL * 10
= 1e-10 (float64) / 2e-4 (float32).  A maximum over the whole bank would let one small plane be wrong.  The same steps
in numpy in the compute dtype stay within 1.2e-14 / 3.7e-6 of the oracle, per filter (tests/test_bank_host.py), and
that module asserts on every graph that the inputs see a dropped panel, swapped coefficient rows and a lost pass offset
by 100 float32 bars and more (the least: 155 for a dropped panel of 33, which is why the synthesis panels weigh
2^-(f mod 2) and not 2^-(f mod 4); see bank_helpers.wide_synthesis_inputs).  The 2 GiB window of the synthesis
(work_panels' window(planes = nf)) binds on no graph this small: 40 panels of 4097 x 36 float64 are 47 MB.

Which test is the deterministic runner of which kernel choice:
    k_combine, f0 > 0, VEC 1 (full pass, short pass, 2 to 5 passes)    A  test_deferred_analysis_of_wide_banks, every
                                                                          width but 34; through perm and without:
                                                                          test_deferred_analysis_without_an_internal_order
    k_combine, f0 > 0, VEC 2                                            A  the same, width 34 (float64 on tiles, both
                                                                          dtypes on the plain kernels);
                                                                          test_combine_lane_vectors_beyond_one_pass
    k_combine, f0 > 0, VEC 4                                            A  test_combine_lane_vectors_beyond_one_pass,
                                                                          float32, vec = 4, widths 8 and 20
    k_combine, padded pitch (ldw > ld), f0 > 0                          A  widths 3 (both dtypes), 2, 6 and 34 (float32)
    40 filters (5 full passes) at order 30                              A  test_forty_filters_at_order_thirty
    nf-way flush in k_step_narrow                                       B  test_fused_flush_of_wide_banks, widths 1 to 4,
                                                                          and kernel = 2 at widths 8 and 20
    nf-way flush in k_step_lds                                          B  kernel = 5 (and 0) at widths 6, 8, 20, 34
    nf-way flush in k_step_panel                                        B  kernel = 1 at widths 6, 8, 20, 34 (and
                                                                          kernel = 0 at 34 float64 columns)
    column batches of a wide bank, y planes of pitch 20                 C  test_column_batches_of_a_wide_bank
    the one-column-batch collapse (narrow kernel, 33-way flush)         C  test_a_small_workspace_collapses_the_fused_bank
    nin >= 9 on the 1- / 2- / 4-lane tile builds                        D  test_clenshaw_synthesis_of_wide_banks, rows of
                                                                          16 / 32 / 64 bytes (float64 widths 2, 4, 8;
                                                                          float32 4, 8 and the padded 2, 3, 6)
    nin >= 9 on the 4- / 8- / 16-lane builds regrouped to 3 / 5 / 10    D  rows of 48 / 80 / 160 bytes (6 and 20 float64
      pieces                                                              columns, 20 float32 columns)
    nin >= 9 on 16 lanes with two column passes (NCOL 2)                D  width 34 in float64: rows of 272 bytes (float32:
                                                                          144 bytes, padded to 36 columns)
    nin >= 9 with a slow block (plain gather inside the tile kernel)    D  hub3001
    nin >= 9 in k_step_narrow / k_step_lds / k_step_panel (MODE 2)      D  tile_gather = 0: widths 1 to 4 and kernel = 2 /
                                                                          kernel = 5 (and 0) / kernel = 1
    the per-filter synthesis loop, 9 filters                            D  test_per_filter_synthesis_of_nine
    k_lz_combine<2>, <4> short and full, <8> short and full             E  test_lanczos_combine_passes, Nf = 2 / 3, 4 / 5, 8
    k_lz_combine<8>, gy = 2 with a short last pass, gy = 3              E  Nf = 9 / 17
    Filter.filter, (N, Nsig, Nf) layout, host and device arrays         F  test_public_filter_call_of_nine_kernels
    pipelined host call of a 9-filter bank                              F  test_pipelined_host_call_of_nine_filters
    recorded and replayed call of 17 filters                            F  test_replayed_call_of_seventeen_filters
Which k_combine<T, VEC> a call runs is established by reading, not by the run: last_step_kinds() counts step launches
and nothing reports the combine's instantiation.  The VEC column above is bank_helpers.combine_vec, a restatement of
choose_shape, vec_cap and launch_combine's `padded ? 1 : vec` in gspx_poly.hip.h (kernel = 2, which forces vec = 1, is
not used in section A).  Were the dispatch to fall back to VEC 1 with right values, these tests would still pass.

Worst per-filter figures on an MI355X, of the plane's own max |reference| (the module's report prints them at the end
of a run with -s; the run's output is profiles/wide_banks_pytest_gpu.log), float64 / float32:
    A  deferred bank on tiles and on plain kernels 8.0e-15 / 6.2e-6, without an internal order 7.9e-15 / 6.3e-6,
       40 filters at order 30 6.2e-15 / 5.1e-6, vec = 2 8.0e-15 / 4.5e-6, vec = 4 4.5e-6 (float32)
    B  fused flush in k_step_narrow 6.5e-15 / 6.0e-6, k_step_lds 6.5e-15 / 4.4e-6, k_step_panel 6.7e-15 / 4.4e-6
    C  batches of 8 + 8 + 4 4.7e-15 / 3.7e-6 (one batch the same), one-column batches 1.1e-15 / 9.2e-7, batched
       against one batch 7.4e-16 / 3.9e-7
    D  Clenshaw synthesis on tiles 3.2e-15 / 2.3e-6, in k_step_narrow 3.9e-15 / 2.3e-6, k_step_lds and k_step_panel
       3.9e-15 / 3.1e-6, per-filter loop 2.0e-15 / 1.4e-6
    E  Lanczos combine 1.2e-14 (float64 only; lanczos_helpers.rel_err of each filter's block of N rows, under that
       module's bar of 1e-10)
    F  Filter.filter with host and with device arrays 3.3e-15 / 3.1e-6, one-shot and pipelined host call
       4.3e-15 / 3.5e-6 (the same bits), replay 9.0e-16 / 8.5e-7 (the same bits)
All of it 31 times and more inside the bar.  The module takes 10 s (197 tests, 0.3 s the slowest).

A one-off observation, not reproducible from the repository: on a scratch build, never committed, with the pass offset
f0 dropped from the coefficient index of k_combine and k_lz_combine and the filter index of the fused flush and of the
extra input panels taken modulo 8 (values only; no address or launch shape changed), the cases of 9 filters and more
of this module failed, while the recurrence, kernels, fuzz, Lanczos and configs modules passed."""
import numpy as np
import pytest

import bank_helpers as bh
import tile_helpers
from gpu_helpers import ctx, random_graph  # noqa: F401 (ctx is a fixture)
from lanczos_helpers import laplacian, run_numpy
from lanczos_helpers import rel_err as lz_rel_err
from oracle import cheby_oracle as orc
from pygsp_amd import _capi, engine, filters, graphs
from tile_helpers import DTYPES, OPTIONS, expected_kinds_recurrence

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 3, 4, 6, 8, 20, 34]
K = 12
BASE = dict(OPTIONS, graph_launch=0)  # every call eager: last_step_kinds() counts the call's own launches
hold = bh.hold_per_filter


def options(ctx, **kw):
    return tile_helpers.options(ctx, base=BASE, **kw)


def device_graph(ctx, name, dtype, builder):
    return tile_helpers.device_graph(ctx, name, dtype, builder, bh.NO_POLYNOMIALS)


@pytest.fixture(scope="module", autouse=True)
def report(ctx):
    """Eager calls for the whole module.  After it: the worst per-filter deviation per test and dtype; the device
    graphs, the cases and the Lanczos graph go."""
    ctx.set_option("graph_launch", 0)
    yield
    bh.report()
    tile_helpers.finish()
    LZ.clear()


def tile(n):
    return {"tile": n, "plain": 0}


def plain(n):
    return {"tile": 0, "plain": n}


def analysis(ctx, dev, c, w, kinds, test, where, ref=True):
    """One host-array analysis of the first w columns: its launches must be exactly `kinds`, every filter plane within
    the bar of the oracle's (ref=False: the caller compares bits with a call that was held)."""
    x = np.ascontiguousarray(c["x"][:, :w])
    y, _ = dev.cheby_filter(c["coeffs"], x, c["lmax"], _capi.ANALYSIS)
    where = (where, "w=%d" % w, "nf=%d" % c["coeffs"].shape[0])
    assert ctx.last_step_kinds() == kinds, (where, ctx.last_step_kinds(), kinds)
    assert y.shape == (c["coeffs"].shape[0], c["n"], w), where
    if ref:
        hold(test, dev.dtype, y, c["ana"][:, :, :w], where)
    return y


def synthesis(ctx, dev, c, w, kinds, test, where):
    """One host-array synthesis of the first w columns of every input panel."""
    s = np.ascontiguousarray(c["s"][:, :, :w])
    y, _ = dev.cheby_filter(c["coeffs"], s, c["lmax"], _capi.SYNTHESIS)
    where = (where, "w=%d" % w, "nf=%d" % c["coeffs"].shape[0])
    assert ctx.last_step_kinds() == kinds, (where, ctx.last_step_kinds(), kinds)
    hold(test, dev.dtype, y, c["syn"][:, :w], where)
    return y


# ---- A: the deferred combine beyond one pass -----------------------------------------------------------------------
def deferred_at_every_width(ctx, dev, c, at, tiles_too, plain_too, test):
    elt, nf, steps = dev.dtype.itemsize, c["coeffs"].shape[0], c["K"]
    for w in WIDTHS:
        if tiles_too:
            kinds = expected_kinds_recurrence(w, elt, nf, steps)
            y0 = analysis(ctx, dev, c, w, kinds, test + " on tiles", at)
            if plain_too:  # (the combine does not depend on who built the tiles: once per graph and dtype)
                with options(ctx, combine=2):
                    y2 = analysis(ctx, dev, c, w, kinds, test, at + ("combine=2",), ref=False)
                assert np.array_equal(y0, y2), (at, w, "combine = 0 against 2 on tiles")
        if plain_too:
            with options(ctx, tile_gather=0):
                p0 = analysis(ctx, dev, c, w, plain(steps), test + " on plain kernels", at)
                with options(ctx, combine=2):
                    p2 = analysis(ctx, dev, c, w, plain(steps), test, at + ("combine=2",), ref=False)
            assert np.array_equal(p0, p2), (at, w, "combine = 0 against 2 on plain kernels")


@pytest.mark.parametrize("nf", [7, 8, 9, 16, 17, 33])
@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", bh.GRAPHS)
def test_deferred_analysis_of_wide_banks(ctx, graph, dtype, builder, nf):
    """k_combine once per 8 filters: a short first pass (7), a full one (8), f0 = 8 with 1 filter (9), two full passes
    (16), f0 = 16 (17), five passes (33); combine = 0 and 2 are the same call."""
    c = bh.case(graph, nf, K)
    dev = device_graph(ctx, graph, dtype, builder)
    at = (graph, np.dtype(dtype).name, builder)
    deferred_at_every_width(ctx, dev, c, at, True, builder == "host", "A deferred bank")


@pytest.mark.parametrize("dtype", DTYPES)
def test_forty_filters_at_order_thirty(ctx, dtype):
    c = bh.case("hub3001", 40, 30)
    dev = device_graph(ctx, "hub3001", dtype, "host")
    at = ("hub3001", np.dtype(dtype).name)
    y0 = analysis(ctx, dev, c, 20, tile(30), "A 40 filters at order 30", at)
    with options(ctx, combine=2):
        assert np.array_equal(y0, analysis(ctx, dev, c, 20, tile(30), "A", at, ref=False))
    with options(ctx, tile_gather=0):
        analysis(ctx, dev, c, 20, plain(30), "A 40 filters at order 30", at + ("plain",))


@pytest.mark.parametrize("nf", [9, 33])
@pytest.mark.parametrize("dtype", DTYPES)
def test_deferred_analysis_without_an_internal_order(ctx, dtype, nf):
    """k_combine writes y through perm; hub3001 in its own order has none (perm == nullptr: orow = row)."""
    c = bh.case("hub3001", nf, K)
    dev = engine.DeviceGraph.from_w(c["W"], c["lap"], dtype=dtype, perm=None, ctx=ctx)
    try:
        assert dev.download_perm() is None
        st = dev.build_gather_tiles()
        assert st["nb"] == 47, st
        at = ("hub3001 in its own order", np.dtype(dtype).name)
        deferred_at_every_width(ctx, dev, c, at, True, True, "A no internal order")
    finally:
        dev.destroy()


@pytest.mark.parametrize("nf", [9, 17])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", ["hub3001", "sensor4097"])
def test_combine_lane_vectors_beyond_one_pass(ctx, graph, dtype, nf):
    """The option vec gives the deferred combine of a direct tile batch a lane vector of its own choice (the tile steps
    have their own shapes): k_combine<T, 2> at widths 6 to 34, k_combine<float, 4> at widths 8 and 20 - rows of y and
    slot rows are whole 16-byte pieces there - with f0 = 8 and 16."""
    c = bh.case(graph, nf, K)
    dt = np.dtype(dtype)
    dev = device_graph(ctx, graph, dtype, "device")
    per = 16 // dt.itemsize
    ran = set()
    for vec in (2, 4):
        for w in WIDTHS:
            padded = w % per != 0
            if bh.combine_vec(w, dt.itemsize, padded, vec) != vec:
                continue
            ran.add((vec, w))
            with options(ctx, vec=vec):
                analysis(ctx, dev, c, w, tile(K), "A combine with vec = %d" % vec, (graph, dt.name))
    want = {(2, 6), (2, 8), (2, 20), (2, 34)} if per == 2 else {(2, 8), (2, 20), (4, 8), (4, 20)}
    assert ran == want, ran


# ---- B: the fused flush of all accumulators ------------------------------------------------------------------------
def kernels_at(w, narrow_up_to):
    """The settings of `kernel` a width runs: 0 alone up to 4 columns (the narrow kernel whatever is asked), else the
    automatic choice, the panel kernel, the LDS kernel and - up to `narrow_up_to` columns - the narrow kernel forced."""
    if w <= 4:
        return (0,)
    return (0, 1, 5) + ((2,) if w in narrow_up_to else ())


@pytest.mark.parametrize("nf", [7, 9, 33])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", bh.GRAPHS)
def test_fused_flush_of_wide_banks(ctx, graph, dtype, nf):
    """combine = 1: every step that flushes loops over all nf accumulators (wts[3 f ..], racc + f plane_r, y + f plane_y
    in the last one) - plain launches only, in k_step_narrow, k_step_lds and k_step_panel."""
    c = bh.case(graph, nf, K)
    dt = np.dtype(dtype)
    dev = device_graph(ctx, graph, dtype, "host")
    for w in WIDTHS:
        assert expected_kinds_recurrence(w, dt.itemsize, nf, K, combine=1) == plain(K)
        for kernel in kernels_at(w, (8, 20)):
            name = bh.plain_kernel(w, dt.itemsize, kernel)
            with options(ctx, combine=1, kernel=kernel):
                analysis(ctx, dev, c, w, plain(K), "B fused flush, " + name, (graph, dt.name, "kernel=%d" % kernel))


# ---- C: column batches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", bh.GRAPHS)
def test_column_batches_of_a_wide_bank(ctx, graph, dtype):
    """33 filters on 20 signals in batches of 8 + 8 + 4: every batch combines into y planes of pitch 20 at its own
    column.  Deferred on tiles and on plain kernels, and the fused flush."""
    nf, w = 33, 20
    c = bh.case(graph, nf, K)
    dt = np.dtype(dtype)
    dev = device_graph(ctx, graph, dtype, "device")
    assert bh.batches(c["n"], dt.itemsize, K + 1, w, max_batch=8) == [8, 8, 4]
    assert bh.batches(c["n"], dt.itemsize, 2 + nf, w, max_batch=8) == [8, 8, 4]
    for opts, kind in (({}, tile), ({"tile_gather": 0}, plain), ({"combine": 1}, plain)):
        at = (graph, dt.name, str(opts))
        with options(ctx, **opts):
            one = analysis(ctx, dev, c, w, kind(K), "C one batch", at)
            assert ctx.last_timing()["step_launches"] == K, at
            with options(ctx, max_batch=8):
                assert expected_kinds_recurrence(w, dt.itemsize, nf, K, max_batch=8, **opts) == kind(3 * K)
                many = analysis(ctx, dev, c, w, kind(3 * K), "C batches of 8 + 8 + 4", at)
                assert ctx.last_timing()["step_launches"] == 3 * K, at
        hold("C batched against one batch", dtype, many, one.astype(np.float64), at)


@pytest.mark.parametrize("nf", [9, 33])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_small_workspace_collapses_the_fused_bank(ctx, dtype, nf):
    """ws_limit_mb = 1 on sensor4097: a fused bank budgets 2 + Nf work panels per signal, so 33 filters leave room for
    one column per batch - the narrow kernel with a 33-way flush, six batches for six signals - and 9 filters for
    batches of 2 (float64) or 4 + 2 (float32)."""
    w = 6
    c = bh.case("sensor4097", nf, K)
    dt = np.dtype(dtype)
    dev = device_graph(ctx, "sensor4097", dtype, "host")
    cols = bh.batches(c["n"], dt.itemsize, 2 + nf, w, ws_limit_mb=1)
    assert cols == ([1] * 6 if nf == 33 else ([2, 2, 2] if dt.itemsize == 8 else [4, 2])), cols
    at = ("sensor4097", dt.name, "batches %s" % cols)
    with options(ctx, combine=1):
        one = analysis(ctx, dev, c, w, plain(K), "C one batch", at)
        with options(ctx, ws_limit_mb=1):
            many = analysis(ctx, dev, c, w, plain(len(cols) * K), "C small workspace", at)
            assert ctx.last_timing()["step_launches"] == len(cols) * K, at
    hold("C batched against one batch", dtype, many, one.astype(np.float64), at)


# ---- D: synthesis --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [7, 9, 17, 33])
@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", bh.GRAPHS)
def test_clenshaw_synthesis_of_wide_banks(ctx, graph, dtype, builder, nf):
    """Every Clenshaw step adds nin = Nf input panels to its row: on the tile INS builds through one buffer window of
    panel_bytes * nin (flavour 2), in the plain MODE 2 rows through racc + f * plane_r.  K + 1 launches."""
    c = bh.synthesis_case(graph, nf, K)
    dt = np.dtype(dtype)
    dev = device_graph(ctx, graph, dtype, builder)
    at = (graph, dt.name, builder)
    for w in WIDTHS:
        kinds = expected_kinds_recurrence(w, dt.itemsize, nf, K, "synthesis")
        assert kinds == (plain(K + 1) if w == 1 else tile(K + 1))
        synthesis(ctx, dev, c, w, kinds, "D Clenshaw synthesis on tiles", at)
        if builder != "host":
            continue
        for kernel in kernels_at(w, (6, 8)):
            name = bh.plain_kernel(w, dt.itemsize, kernel)
            with options(ctx, tile_gather=0, kernel=kernel):
                synthesis(ctx, dev, c, w, plain(K + 1), "D Clenshaw synthesis, " + name, at + ("kernel=%d" % kernel,))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", bh.GRAPHS)
def test_per_filter_synthesis_of_nine(ctx, graph, dtype):
    """synthesis = 1: one single-filter recurrence per input panel, accumulated on the device - Nf K launches."""
    nf = 9
    c = bh.synthesis_case(graph, nf, K)
    dt = np.dtype(dtype)
    dev = device_graph(ctx, graph, dtype, "device")
    at = (graph, dt.name)
    with options(ctx, synthesis=1):
        for w in WIDTHS:
            kinds = expected_kinds_recurrence(w, dt.itemsize, nf, K, "synthesis", synthesis=1)
            assert kinds == (plain(nf * K) if w == 1 else tile(nf * K))
            synthesis(ctx, dev, c, w, kinds, "D per-filter synthesis on tiles", at)
            with options(ctx, tile_gather=0):
                synthesis(ctx, dev, c, w, plain(nf * K), "D per-filter synthesis on plain kernels", at)


# ---- E: the Lanczos combine ----------------------------------------------------------------------------------------
LZ = {}


def lanczos_case():
    """A 2000-vertex hub graph with an internal order (reverse Cuthill-McKee: the combine writes y through perm), its
    Laplacian and 64 signals."""
    if not LZ:
        W = random_graph(2000, 8, seed=2000, hub=True)
        G = graphs.Graph(W, compute_dtype=np.float64, reorder="rcm")
        G.estimate_lmax("bounds")
        perm = G.device_graph(np.float64).download_perm()
        assert perm is not None and not np.array_equal(perm, np.arange(2000))
        LZ.update(G=G, L=laplacian(W, "combinatorial"), x=np.random.default_rng(6).standard_normal((2000, 64)))
    return LZ["G"], LZ["L"], LZ["x"]


@pytest.mark.parametrize("nv", [1, 5, 64])
@pytest.mark.parametrize("nf", [2, 3, 4, 5, 8, 9, 17])
def test_lanczos_combine_passes(nf, nv):
    """gspx_lanczos_combine_dev: k_lz_combine<2> (Nf = 2), <4> short and full (3, 4), <8> short and full (5, 8),
    gy = 2 with a short last pass (9), gy = 3 (17); heat kernels at Nf distinct scales, every filter block of N rows
    on its own against the numpy backend at that module's bar."""
    G, L, x = lanczos_case()
    N, order = G.N, 20
    f = filters.Filter(G, [orc.heat_kernel(s, G.lmax) for s in np.geomspace(2.0, 60.0, nf)])
    assert f.Nf == nf
    s = x[:, 0] if nv == 1 else x[:, :nv]
    y = filters.lanczos_op(f, s, order=order)
    ref, _, _ = run_numpy(L, f, s, order, G._get_upper_bound())
    assert y.shape == ref.shape == ((N * nf,) if nv == 1 else (N * nf, nv))
    errs = [lz_rel_err(y[i * N:(i + 1) * N], ref[i * N:(i + 1) * N]) for i in range(nf)]
    worst = int(np.argmax(errs))
    bh.record("E Lanczos combine", np.float64, errs[worst], ("nf=%d" % nf, "nv=%d" % nv, "filter %d" % worst),
              metric="lanczos_helpers.rel_err of the filter's block of N rows, bar 1e-10,")
    assert max(errs) <= 1e-10, (nf, nv, errs)


# ---- F: the seams --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_public_filter_call_of_nine_kernels(ctx, dtype):
    """Filter.filter of a 9-kernel bank: analysis (N, Nsig) -> (N, Nsig, 9), synthesis of that analysis -> (N, Nsig),
    with host arrays and with a DeviceArray in and out, every filter plane against the oracle's filter.py."""
    dt = np.dtype(dtype)
    W, lap, L, lmax, _, _ = tile_helpers.graph_matrix("hub3001")
    G = graphs.Graph(W, lap_type=lap, compute_dtype=dtype, ctx=ctx)
    # The oracle's reference below is the Chebyshev approximation on [0, lmax] of graph_matrix's bound, and the device
    # must approximate on the same interval.  Graph has no setter for a given bound - estimate_lmax computes its own -
    # so the test writes the attribute, as tests/test_gpu_s_reduction.py and test_gpu_f_learning.py do.
    G._lmax = lmax
    kernels = orc.mexican_hat_kernels(lmax, 9)
    f = filters.Filter(G, kernels)
    x = bh.signals("hub3001")[:, :6]
    ref = orc.filter_chebyshev(L, lmax, kernels, x, K)
    assert ref.shape == (3001, 6, 9)
    ref_back = orc.filter_chebyshev(L, lmax, kernels, ref, K)
    planes = np.moveaxis(ref, 2, 0)
    at = ("hub3001", dt.name)
    y = f.filter(x, order=K)
    assert y.shape == (3001, 6, 9) and y.dtype == np.float64
    hold("F Filter.filter, host arrays", dtype, np.moveaxis(y, 2, 0), planes, at + ("analysis",))
    back = f.filter(y, order=K)  # (the synthesis of that analysis)
    assert back.shape == (3001, 6)
    hold("F Filter.filter, host arrays", dtype, back, ref_back, at + ("synthesis",))
    d = f.filter(G.to_device(x), order=K)
    assert isinstance(d, engine.DeviceArray) and tuple(d.shape) == (3001, 6, 9)
    hold("F Filter.filter, device arrays", dtype, np.moveaxis(np.asarray(d), 2, 0), planes, at + ("analysis",))
    dback = f.filter(d, order=K)  # (the chain stays on the device)
    assert isinstance(dback, engine.DeviceArray) and tuple(dback.shape) == (3001, 6)
    hold("F Filter.filter, device arrays", dtype, np.asarray(dback), ref_back, at + ("synthesis",))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", ["hub3001", "sensor4097"])
def test_pipelined_host_call_of_nine_filters(ctx, graph, dtype):
    """A 9-filter bank over 24 columns, forced through the pipelined host form in three batches of 8: the bytes of the
    one-shot call."""
    c = bh.synthesis_case(graph, 9, K)
    dt = np.dtype(dtype)
    dev = device_graph(ctx, graph, dtype, "host")
    at = (graph, dt.name)
    with options(ctx, host_pipeline=0):
        y1 = analysis(ctx, dev, c, 24, tile(K), "F one-shot host call", at)
        s1 = synthesis(ctx, dev, c, 24, tile(K + 1), "F one-shot host call", at)
        assert ctx.last_host_timing() is None
    with options(ctx, host_pipeline=2, host_batch=8):
        y3 = analysis(ctx, dev, c, 24, tile(3 * K), "F pipelined host call", at)
        assert ctx.last_host_timing()["batches"] == 3, at
        s3 = synthesis(ctx, dev, c, 24, tile(3 * (K + 1)), "F pipelined host call", at)
        assert ctx.last_host_timing()["batches"] == 3, at
    assert np.array_equal(y1, y3), at
    assert np.array_equal(s1, s3), at


@pytest.mark.parametrize("dtype", DTYPES)
def test_replayed_call_of_seventeen_filters(ctx, dtype):
    """graph_launch = 1: the second identical call is recorded - K steps and three combine passes -, the third and
    fourth are replayed; the bits of the eager call."""
    c = bh.case("sensor4097", 17, K)
    dt = np.dtype(dtype)
    dev = device_graph(ctx, "sensor4097", dtype, "device")
    w = 8
    at = ("sensor4097", dt.name)
    eager = analysis(ctx, dev, c, w, tile(K), "F replay", at + ("eager",))
    with options(ctx, graph_launch=1):
        for call in (1, 2, 3, 4):
            again = analysis(ctx, dev, c, w, tile(K), "F replay", at + ("call %d" % call,), ref=False)
            assert np.array_equal(eager, again), (at, call)
        t = ctx.last_timing()
        assert t["total_ms"] == t["steps_ms"] > 0, (at, t)  # (a replayed call reports one time)
    assert np.array_equal(eager, analysis(ctx, dev, c, w, tile(K), "F replay", at + ("eager again",), ref=False))
