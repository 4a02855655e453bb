"""The Chebyshev recurrence (gspx_cheby_filter: the three-term recurrence with the fused flush, filter banks with the
deferred combine, synthesis by the Clenshaw recurrence and by the per-filter loop) on the LDS-staged tile kernel
k_step_tile, at small shapes: every flavour launch_step_tile tells apart (0 plain, 1 step 2 of a fused input, 2 extra
input panels) on every tile build (1- / 2- / 4- / 8- / 16-lane, the regrouped 3- / 5- / 10-piece builds, NCOL 1 / 2 / 0),
on graphs of 2, 10, 47 and 65 blocks with and without slow blocks and on two band graphs whose every block is staged;
the silent boundaries between tile and plain kernels and between direct and padded work panels
(Context.last_step_kinds() tells which kernels ran, every count an equality); options that must not change a bit;
other builds for the same rows; tiles on and off; replay.  Every column is compared with the oracle's recurrence.
`-m gpu`.  The whole matrix runs with graph_launch = 0 - every call eager, counting its own launches - but section F.

Bar: gpu_helpers.TOL * 10 = 1e-10 (float64) / 2e-4 (float32) of max |reference|, as test_tile_gather_kernel and the
programs module hold this path to.  The same steps in numpy in the compute dtype stay within 6.7e-15 / 2.2e-6 of the
oracle (tests/test_recurrence_host.py), 90 times and more inside the bar.

An order-m filter has m + 1 coefficients and runs K = m steps: Heat(20) at orders 1, 2, 3, 7, 30 is K = 1, 2, 3, 7, 30
launches, the bank of 3 at order 12 K = 12, its Clenshaw synthesis K + 1 = 13, its per-filter synthesis 3 K = 36.

Which test is the deterministic runner of which kernel choice:
    flavour 2 on the 8-lane and on the 16-lane NCOL 1 / 2 / 0 builds    A  test_every_flavour_on_every_tile_build, rows of
                                                                           128 and of 256, 272 / 512, 528 / 768 bytes
    flavour 2 on the regrouped 3- / 5- / 10-piece builds, both dtypes   A  rows of 48 / 80 / 160 bytes
    flavour 2 with a slow block (plain gather inside the kernel)        A  the hub graphs, sensor4097+hub
    synthesis = 1 on tiles (acc_existing / final_to_y)                  A  "per-filter synthesis", every row size; padded: B
    flavour 1 on the 1- / 2- / 4- / 8-lane builds, NCOL 1 / 2 / 0       A  the band graphs, rows of 16 / 32 / 64 / 128 bytes
                                                                           and wider, both dtypes, both builders; the
                                                                           gt_s1nat mapping: band4097-shuffled
    regrouped build (steps 1, 3, ...) mixed with flavour 1 (step 2)     A  the band graphs, rows of 48 / 80 / 160 bytes
    step 2 of a fused input that is also the last flush into y          A  heat20/2 on the band graphs
    deferred combine on tiles beyond width 8                            A  "bank on tiles", every row size; padded: B
    combine = 1 with several filters goes to the plain kernels          B  test_a_fused_flush_of_several_filters_...
    k_permute_in_pad / k_permute_out_pad, final = 0, combine with ldw   B  test_off_piece_widths_take_the_padded_route,
                                                                           test_pad_columns_change_no_bit,
                                                                           test_unaligned_output_takes_the_padded_route
    the fused-input gate: x aliasing y, ldx != ld, fuse_input = 0       B  test_an_in_place_call_takes_the_copy_route,
                                                                           test_column_batches_choose_their_kernel; A
    tile_regroup = 0, tile_lg for flavours 0, 1 and 2                   D  test_other_builds_for_the_same_rows
    recorded fused-input call (gt_s1nat at capture time)                F  test_replayed_calls_repeat_bits_and_kinds

Whether the fused route ran cannot be observed from outside: the copy-in phase of Context.last_timing() is the time
between two events, over three runs 0.004 ... 0.040 ms with the input fused and 0.006 ... 0.022 ms with it copied (the
report prints both) - no line between them, and nothing was added to the library for it.  The gate's seven
conditions (run_batch) were checked from the code for the band graphs' calls in section A instead: the rows are whole
16-byte pieces and y is a 16-byte aligned buffer of
the same pitch (tile_direct), one filter (not deferred), fuse_input = 1, no slow block (asserted with the tiles),
one column batch (ldx == ld), x a buffer of its own (aligned, apart from y), and band4097 has no internal order while
band4097-shuffled has tile lists (gt_ns1 > 0) and runs eagerly.  On those graphs the fused and the copied call must
agree in every bit.

Worst figures on an MI355X, of max |reference| (the module's report prints them at the end of a run with -s; the
run's output is profiles/recurrence_on_tiles_pytest_gpu.log), float64 / float32:
    A  single filter on tiles 3.1e-15 / 1.4e-6 (plain kernels the same), bank 5.2e-15 / 3.9e-6, Clenshaw synthesis
       8.0e-15 / 4.1e-6, per-filter synthesis 8.1e-15 / 4.2e-6
    B  combine = 1 and 2 4.7e-15 / 3.4e-6, off-piece widths 6.1e-15 / 3.9e-6, padded against direct 8.0e-15 / 4.1e-6,
       unaligned y 5.9e-15, x aliasing y 1.2e-15 / 8.2e-7, column batches 5.7e-15 / 3.7e-6, pipelined host call
       3.3e-15 / 2.7e-6
    C  default options 7.7e-15 / 4.1e-6 (every other setting: the same bits);  D  other builds 5.9e-15 / 3.9e-6
    E  tiles on and off 1.4e-15 / 5.3e-7;  F  replay 1.1e-15 / 6.7e-7
The module takes 13 s (455 tests, 0.3 s the slowest).

A value-only mutation, run once on a scratch build and never committed - GSPX_CL handing out the flavour-0 kernel of
the same LG_ / CL_ / NT_ when flavour == 2, so that the regrouped builds ignore the extra input panels of a synthesis;
no address, index or launch shape changes: this module fails on the 48-, 80- and 160-byte rows of every graph
(section A, the Clenshaw synthesis of bank3, deviation 1.0 of max |reference|) and passes on every other row size.
test_gpu_2_kernels.py does not pass it either: test_tile_gather_kernel[float64] fails at its padded width 5 (48-byte
rows) and test_host_pipeline_equals_one_shot_call[float32] at 24 columns - both on the 3-piece build; nothing there
runs a synthesis on the 5- and 10-piece builds, so on the 80- and 160-byte rows this module is the only one to fail."""
import numpy as np
import pytest

import tile_helpers
from gpu_helpers import ctx  # noqa: F401 (ctx is a fixture)
from pygsp_amd import _capi, engine
from recurrence_helpers import POLYNOMIALS, SINGLE, steps, synthesis_inputs, synthesis_reference
from tile_helpers import (BAND_GRAPHS, DTYPES, F64, GRAPHS, MAXW, OFF_PIECE, OPTIONS, ROW_BYTES, columns,
                          expected_kinds_recurrence, hold)

pytestmark = pytest.mark.gpu

ALL_GRAPHS = GRAPHS + BAND_GRAPHS
BASE = dict(OPTIONS, graph_launch=0)  # every call eager: last_step_kinds() counts the call's own launches
_COPY_IN = {}  # (fuse_input, dtype name) -> [least, greatest] copy-in phase (ms) of the band graphs' single-filter calls


def options(ctx, **kw):
    return tile_helpers.options(ctx, base=BASE, **kw)


def case(name):
    """tile_helpers.case with the polynomials of the recurrence tests, and on top of the oracle's analysis of the 192
    columns (c["ana"][name]: (Nf, N, 192)) the synthesis inputs of the banks and their reference (c["s"], c["syn"])."""
    c = tile_helpers.case(name, POLYNOMIALS)
    if "ana" not in c:
        c["ana"] = {k: r.reshape(-1, c["n"], MAXW) for k, r in c["ref"].items()}
        c["s"] = {k: synthesis_inputs(c["x"], c["polys"][k].shape[0]) for k in ("bank3", "bank2")}
        c["syn"] = {k: synthesis_reference(c["ana"][k]) for k in ("bank3", "bank2")}
        for a in list(c["s"].values()) + list(c["syn"].values()):
            a.setflags(write=False)
    return c


def device_graph(ctx, name, dtype, builder):
    return tile_helpers.device_graph(ctx, name, dtype, builder, POLYNOMIALS)


@pytest.fixture(scope="module", autouse=True)
def report(ctx):
    """Eager calls for the whole module.  After it: the device's worst deviation per test and dtype and the copy-in
    phases seen with and without a fused input; the device graphs go."""
    ctx.set_option("graph_launch", 0)
    yield
    for (fuse, dt), (lo, hi) in sorted(_COPY_IN.items()):
        print("\ncopy-in phase, band graphs, fuse_input = {} {:<8s} {:.4f} ... {:.4f} ms".format(fuse, dt, lo, hi), end="")
    tile_helpers.finish()


def panels(c, name, w, mode):
    """(input, oracle's result) of polynomial `name` on the first w columns: analysis (N, w) -> (Nf, N, w), synthesis
    (Nf, N, w) -> (N, w)."""
    if mode == "analysis":
        return columns(c, w), c["ana"][name][:, :, :w]
    return np.ascontiguousarray(c["s"][name][:, :, :w]), c["syn"][name][:, :w]


def run(ctx, dev, c, name, w, mode, kinds, test, where):
    """One host-array call: its launches must be exactly `kinds`, its result within the bar of the oracle's."""
    x, ref = panels(c, name, w, mode)
    y, _ = dev.cheby_filter(c["polys"][name], x, c["lmax"], _capi.ANALYSIS if mode == "analysis" else _capi.SYNTHESIS)
    where = (where, "w=%d" % w, name, mode)
    assert ctx.last_step_kinds() == kinds, (where, ctx.last_step_kinds(), kinds)
    hold(test, dev.dtype, y, ref, where)
    return y


def tile(n):
    return {"tile": n, "plain": 0}


def plain(n):
    return {"tile": 0, "plain": n}


def note_copy_in(ctx, fuse, dtype):
    ms = ctx.last_timing()["permute_ms"]
    lo, hi = _COPY_IN.get((fuse, np.dtype(dtype).name), (ms, ms))
    _COPY_IN[(fuse, np.dtype(dtype).name)] = (min(lo, ms), max(hi, ms))


# ---- A: every flavour on every build -------------------------------------------------------------------------------
@pytest.mark.parametrize("row_bytes", ROW_BYTES)
@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", ALL_GRAPHS)
def test_every_flavour_on_every_tile_build(ctx, graph, dtype, builder, row_bytes):
    c = case(graph)
    dev = device_graph(ctx, graph, dtype, builder)
    w = row_bytes // np.dtype(dtype).itemsize
    at = (graph, np.dtype(dtype).name, builder)
    for name in SINGLE:  # flavour 0, and 1 in step 2 where the input is fused (the band graphs)
        K = steps(c["polys"][name])
        y1 = run(ctx, dev, c, name, w, "analysis", tile(K), "A single filter on tiles", at)
        if graph in BAND_GRAPHS:
            note_copy_in(ctx, 1, dtype)
            with options(ctx, fuse_input=0):
                y0 = run(ctx, dev, c, name, w, "analysis", tile(K), "A single filter on tiles", at + ("copied in",))
                note_copy_in(ctx, 0, dtype)
            assert np.array_equal(y0, y1), (at, w, name, "fused against copied input")
        with options(ctx, tile_gather=0):
            run(ctx, dev, c, name, w, "analysis", plain(K), "A single filter on plain kernels", at)
    for name in ("bank3", "bank2"):  # the deferred combine
        K = steps(c["polys"][name])
        run(ctx, dev, c, name, w, "analysis", tile(K), "A bank on tiles", at)
        with options(ctx, tile_gather=0):
            run(ctx, dev, c, name, w, "analysis", plain(K), "A bank on plain kernels", at)
    K = steps(c["polys"]["bank3"])  # flavour 2: the Clenshaw recurrence; the per-filter loop (flavours 0 and 1)
    run(ctx, dev, c, "bank3", w, "synthesis", tile(K + 1), "A synthesis on tiles", at)
    with options(ctx, tile_gather=0):
        run(ctx, dev, c, "bank3", w, "synthesis", plain(K + 1), "A synthesis on plain kernels", at)
    with options(ctx, synthesis=1):
        run(ctx, dev, c, "bank3", w, "synthesis", tile(3 * K), "A per-filter synthesis on tiles", at)
        with options(ctx, tile_gather=0):
            run(ctx, dev, c, "bank3", w, "synthesis", plain(3 * K), "A per-filter synthesis on plain kernels", at)


# ---- B: the silent boundaries --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", ["sensor4097", "hub3001", "band4097"])
def test_a_fused_flush_of_several_filters_runs_on_the_plain_kernels(ctx, graph, dtype):
    """combine = 1: the accumulators of all filters are flushed inside the steps, which only the plain kernels do for
    two filters and more (work_panels(..., deferred || nf == 1, ...)); one filter, and combine = 2, stay on the tiles."""
    c = case(graph)
    dev = device_graph(ctx, graph, dtype, "host")
    at = (graph, np.dtype(dtype).name)
    for row_bytes in (16, 64, 80, 272):
        w = row_bytes // np.dtype(dtype).itemsize
        for name in ("bank3", "bank2"):
            K = steps(c["polys"][name])
            with options(ctx, combine=1):
                run(ctx, dev, c, name, w, "analysis", plain(K), "B combine = 1", at)
                assert rule(dev, c, name, "analysis", 0, w, combine=1) == plain(K), (at, w, name)
            with options(ctx, combine=2):
                run(ctx, dev, c, name, w, "analysis", tile(K), "B combine = 2", at)
        with options(ctx, combine=1):
            run(ctx, dev, c, "heat20/30", w, "analysis", tile(30), "B combine = 1", at)


CALLS = [(name, "analysis", 0) for name in SINGLE] + [("bank3", "analysis", 0), ("bank3", "synthesis", 0),
                                                      ("bank3", "synthesis", 1)]


def rule(dev, c, name, mode, synthesis, w, **kw):
    nf = c["polys"][name].shape[0]
    return expected_kinds_recurrence(w, dev.dtype.itemsize, nf, steps(c["polys"][name]), mode, synthesis=synthesis, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", ["sensor4097", "hub3001", "rand577", "band4097-shuffled"])
def test_off_piece_widths_take_the_padded_route(ctx, graph, dtype):
    """Rows that are not whole 16-byte pieces: tile_pad = 2 the tile kernels on padded work panels (k_permute_in_pad,
    final = 0, k_permute_out_pad or the combine with the padded pitch), 0 the plain kernels, 1 the tile kernels but for a
    single column, which the sub-wave kernel serves faster on graphs this small."""
    c = case(graph)
    dev = device_graph(ctx, graph, dtype, "device")
    at = (graph, np.dtype(dtype).name)
    for w in OFF_PIECE[np.dtype(dtype)]:
        for pad in (2, 0, 1):
            on_tiles = pad == 2 or (pad == 1 and w > 1)
            for name, mode, synthesis in CALLS:
                K = steps(c["polys"][name])
                n = K if mode == "analysis" else (3 * K if synthesis else K + 1)
                kinds = tile(n) if on_tiles else plain(n)
                assert rule(dev, c, name, mode, synthesis, w, tile_pad=pad) == kinds, (w, pad, name, mode, synthesis)
                with options(ctx, tile_pad=pad, synthesis=synthesis):
                    run(ctx, dev, c, name, w, mode, kinds, "B off-piece widths, tile_pad = %d" % pad, at + (synthesis,))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", ["sensor4097+hub", "hub3001", "band4097-shuffled"])
def test_pad_columns_change_no_bit(ctx, graph, dtype):
    """An off-piece width w on work panels padded up to ldp columns against the direct call of width ldp on the same
    columns followed by zero columns: the same build, the same order of operations - its first w columns are the padded
    call's bits, its other columns exactly zero."""
    c = case(graph)
    dt = np.dtype(dtype)
    dev = device_graph(ctx, graph, dtype, "host")
    per = 16 // dt.itemsize
    for w in OFF_PIECE[dt]:
        ldp = (w + per - 1) // per * per
        for name, mode, synthesis in [("heat20/2", "analysis", 0), ("heat20/30", "analysis", 0), ("bank3", "analysis", 0),
                                      ("bank3", "synthesis", 0), ("bank3", "synthesis", 1)]:
            at = (graph, dt.name, "w=%d" % w, name, mode, synthesis)
            K = steps(c["polys"][name])
            n = K if mode == "analysis" else (3 * K if synthesis else K + 1)
            x, ref = panels(c, name, w, mode)
            wide = np.zeros(x.shape[:-1] + (ldp,))
            wide[..., :w] = x
            code = _capi.ANALYSIS if mode == "analysis" else _capi.SYNTHESIS
            with options(ctx, tile_pad=2, synthesis=synthesis):
                yp, _ = dev.cheby_filter(c["polys"][name], x, c["lmax"], code)
                assert ctx.last_step_kinds() == tile(n), at
            with options(ctx, fuse_input=0, synthesis=synthesis):
                yd, _ = dev.cheby_filter(c["polys"][name], wide, c["lmax"], code)
                assert ctx.last_step_kinds() == tile(n), at
            hold("B padded against direct", dtype, yp, ref, at)
            assert np.array_equal(yd[..., :w], yp), (at, "pad columns changed the result")
            assert not np.any(yd[..., w:]), (at, "pad columns are not zero")


@pytest.mark.parametrize("graph", ["sensor4097", "hub3001", "band4097"])
def test_unaligned_output_takes_the_padded_route(ctx, graph):
    """y 8 bytes into a buffer (float64, width 8): no 16-byte stores into it, so the last flush stays in the work
    panels and leaves through the copy - the tile kernels all the same, unlike a program - and only the panel is
    written."""
    c = case(graph)
    dev = device_graph(ctx, graph, np.float64, "host")
    w, fill = 8, 7.5
    for name, mode, synthesis in [("heat20/2", "analysis", 0), ("heat20/30", "analysis", 0), ("bank3", "analysis", 0),
                                  ("bank3", "synthesis", 0), ("bank3", "synthesis", 1)]:
        at = (graph, "float64", "w=8", name, mode, synthesis)
        x, ref = panels(c, name, w, mode)
        K = steps(c["polys"][name])
        count = K if mode == "analysis" else (3 * K if synthesis else K + 1)
        assert rule(dev, c, name, mode, synthesis, w, y_offset=8) == tile(count)
        ybuf = np.full(ref.size + 4, fill)
        bx, by = ctx.take(x.nbytes), ctx.take(ybuf.nbytes)
        try:
            bx.upload(x)
            by.upload(ybuf)
            code = _capi.ANALYSIS if mode == "analysis" else _capi.SYNTHESIS
            with options(ctx, synthesis=synthesis):
                dev.cheby_filter_dev(c["polys"][name], bx.ptr, by.ptr + 8, w, c["lmax"], code)
            assert ctx.last_step_kinds() == tile(count), at
            back = by.download(ybuf.shape, np.float64)
            assert back[0] == fill and np.all(back[1 + ref.size:] == fill), (at, "the buffer around the panel was written")
            hold("B unaligned y", np.float64, back[1:1 + ref.size].reshape(ref.shape), ref, at)
        finally:
            ctx.give(bx)
            ctx.give(by)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", BAND_GRAPHS)
def test_an_in_place_call_takes_the_copy_route(ctx, graph, dtype):
    """x aliasing y: the input cannot be read in place while y is written, so it is copied into the internal order as
    with fuse_input = 0 - the same bits."""
    c = case(graph)
    dt = np.dtype(dtype)
    dev = device_graph(ctx, graph, dtype, "device")
    for row_bytes in (32, 48, 64, 272):
        w = row_bytes // dt.itemsize
        x = columns(c, w).astype(dt)
        bx, by, bz = ctx.take(x.nbytes), ctx.take(x.nbytes), ctx.take(x.nbytes)
        try:
            bx.upload(x)
            for name in ("heat20/1", "heat20/2", "heat20/3", "heat20/30"):
                at = (graph, dt.name, "w=%d" % w, name)
                K = steps(c["polys"][name])
                with options(ctx, fuse_input=0):
                    dev.cheby_filter_dev(c["polys"][name], bx.ptr, by.ptr, w, c["lmax"])
                    assert ctx.last_step_kinds() == tile(K), at
                y0 = by.download(x.shape, dt)
                bz.upload(x)
                dev.cheby_filter_dev(c["polys"][name], bz.ptr, bz.ptr, w, c["lmax"])
                assert ctx.last_step_kinds() == tile(K), at
                yz = bz.download(x.shape, dt)
                hold("B x aliasing y", dtype, yz, c["ana"][name][0][:, :w], at)
                assert np.array_equal(yz, y0), at
                assert np.array_equal(bx.download(x.shape, dt), x), (at, "the input panel was written")
        finally:
            for b in (bx, by, bz):
                ctx.give(b)


@pytest.mark.parametrize("max_batch", [2, 8, 20])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", ["sensor4097", "hub3001", "band4097-shuffled"])
def test_column_batches_choose_their_kernel(ctx, graph, dtype, max_batch):
    c = case(graph)
    dt = np.dtype(dtype)
    dev = device_graph(ctx, graph, dtype, "device")
    w = 20 if dt == F64 else 40
    at = (graph, dt.name, "max_batch=%d" % max_batch)
    for name, mode, synthesis in [("heat20/2", "analysis", 0), ("heat20/30", "analysis", 0), ("bank3", "analysis", 0),
                                  ("bank3", "synthesis", 0), ("bank3", "synthesis", 1)]:
        kinds = rule(dev, c, name, mode, synthesis, w, max_batch=max_batch)
        assert kinds["plain"] == 0 and kinds["tile"] > 0  # (8-byte batches too: padded)
        with options(ctx, max_batch=max_batch, synthesis=synthesis):
            run(ctx, dev, c, name, w, mode, kinds, "B column batches", at + (synthesis,))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", ["sensor4097+hub", "band4097-shuffled"])
def test_pipelined_host_call_sums_its_batches(ctx, graph, dtype):
    """A host-array call forced through the pipelined form in three column batches of 64-byte rows: the counts are
    those of all its batches."""
    c = case(graph)
    dt = np.dtype(dtype)
    dev = device_graph(ctx, graph, dtype, "host")
    per = 64 // dt.itemsize
    with options(ctx, host_pipeline=2, host_batch=per):
        for name in ("heat20/30", "bank3"):
            K = steps(c["polys"][name])
            run(ctx, dev, c, name, 3 * per, "analysis", tile(3 * K), "B pipelined host call", (graph, dt.name))
            assert ctx.last_host_timing()["batches"] == 3, (graph, dt.name, name)


# ---- C: options that must not change a bit -------------------------------------------------------------------------
SAME_BITS = ([{"tile_nt": v} for v in (0, 1, 4, 5, 8, 15)] + [{"tile_workgroups": v} for v in (8, 64, 4096)] +
             [{"alternate_sweep": 0}, {"xcd_remap": 0}])


@pytest.mark.parametrize("dtype,width", [(np.float64, 16), (np.float64, 64), (np.float32, 32), (np.float32, 128)])
@pytest.mark.parametrize("graph", ["band4097", "sensor4097+hub", "hub3001"])
def test_cache_hints_and_block_walks_keep_every_bit(ctx, graph, dtype, width):
    """Non-temporal accesses, the number of persistent workgroups, the sweep direction and the XCD mapping change who
    walks which block and how the caches are asked - never the arithmetic of a row."""
    c = case(graph)
    dev = device_graph(ctx, graph, dtype, "device")
    at = (graph, np.dtype(dtype).name)
    for name, mode in (("heat20/30", "analysis"), ("bank3", "analysis"), ("bank3", "synthesis")):
        K = steps(c["polys"][name])
        kinds = tile(K if mode == "analysis" else K + 1)
        y0 = run(ctx, dev, c, name, width, mode, kinds, "C default options", at)
        for opts in SAME_BITS:
            with options(ctx, **opts):
                y1 = run(ctx, dev, c, name, width, mode, kinds, "C other options", at + (str(opts),))
            assert np.array_equal(y0, y1), (at, width, name, mode, opts)


# ---- D: other builds for the same rows -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", ["band4097-shuffled", "band4097", "hub3001"])
def test_other_builds_for_the_same_rows(ctx, graph, dtype):
    """tile_regroup = 0: 48- / 80- / 160-byte rows on the power-of-two builds; tile_lg: 16- / 32-byte rows on the 2- / 4- /
    8-lane builds - every flavour (on the band graphs the single filter's input is fused).  Other builds need not give
    the same bits: held to the oracle."""
    c = case(graph)
    dt = np.dtype(dtype)
    dev = device_graph(ctx, graph, dtype, "host")
    per = 16 // dt.itemsize
    runs = [({"tile_regroup": 0}, pieces * per) for pieces in (3, 5, 10)]
    runs += [({"tile_lg": lg}, pieces * per) for lg in (2, 4, 8) for pieces in (1, 2)]
    for opts, w in runs:
        at = (graph, dt.name, str(opts))
        with options(ctx, **opts):
            for name in ("heat20/2", "heat20/3", "heat20/30"):
                run(ctx, dev, c, name, w, "analysis", tile(steps(c["polys"][name])), "D other builds", at)
            run(ctx, dev, c, "bank3", w, "analysis", tile(12), "D other builds", at)
            run(ctx, dev, c, "bank3", w, "synthesis", tile(13), "D other builds", at)
            with options(ctx, synthesis=1):
                run(ctx, dev, c, "bank3", w, "synthesis", tile(36), "D other builds", at)


# ---- E: tiles on and off -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_without_tiles_the_recurrence_runs_on_the_plain_kernels(ctx, dtype):
    c = case("rand577")
    dt = np.dtype(dtype)
    dev = engine.DeviceGraph.from_w(c["W"], c["lap"], dtype=dtype, perm=c["perm"], ctx=ctx)
    w = 128 // dt.itemsize
    try:
        for state, kinds in (("never had tiles", plain), ("tiles", tile), ("disabled", plain)):
            if state == "tiles":
                dev.build_gather_tiles()
            if state == "disabled":
                dev.disable_gather_tiles()
            at = ("rand577", dt.name, state)
            run(ctx, dev, c, "heat20/30", w, "analysis", kinds(30), "E tiles on and off", at)
            run(ctx, dev, c, "bank3", w, "synthesis", kinds(13), "E tiles on and off", at)
    finally:
        dev.destroy()


# ---- F: replay -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_replayed_calls_repeat_bits_and_kinds(ctx, dtype):
    """graph_launch = 1 on a graph that has not filtered yet: the first fused-input call makes the tile lists in the
    caller's row order (gt_s1nat), the second sees every address settled, the third is recorded - its steps 1 and 2 read
    the caller's panel - and replayed, the fourth is replayed.  Then the same for the bank's deferred combine."""
    c = case("band4097-shuffled")
    dt = np.dtype(dtype)
    dev = engine.DeviceGraph.from_w(c["W"], c["lap"], dtype=dtype, perm=c["perm"], ctx=ctx)
    w = 128 // dt.itemsize
    try:
        st = dev.build_gather_tiles()
        assert st["slow_blocks"] == 0 and st["nb"] == 65, st
        with options(ctx, graph_launch=1):
            for name in ("heat20/30", "bank3"):
                K = steps(c["polys"][name])
                at = ("band4097-shuffled", dt.name)
                first = run(ctx, dev, c, name, w, "analysis", tile(K), "F replay", at + ("call 1",))
                for call in (2, 3, 4):
                    again = run(ctx, dev, c, name, w, "analysis", tile(K), "F replay", at + ("call %d" % call,))
                    assert np.array_equal(first, again), (at, w, name, call)
                t = ctx.last_timing()
                assert t["total_ms"] == t["steps_ms"] > 0, (at, name, t)  # (a replayed call reports one time)
        run(ctx, dev, c, "heat20/30", w, "analysis", tile(30), "F replay", at + ("eager again",))
        t = ctx.last_timing()
        assert t["total_ms"] != t["steps_ms"], t
    finally:
        dev.destroy()
