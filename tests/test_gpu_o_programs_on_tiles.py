"""Product-form and Newton programs (gspx_poly_program) on the LDS-staged tile kernel k_step_tile, at small shapes: every
program shape of program_helpers.POLYNOMIALS (S = 1, two-pass and in-place three-pass steps, a first step that reads x, a
last step of either kind stored into y through perm) on every tile build (1- / 2- / 4- / 8- / 16-lane, the regrouped 3- /
5- / 10-piece builds, NCOL 1 / 2 / 0), on graphs of 2, 10, 47 and 65 blocks with and without slow blocks; the silent
boundary between tile and plain kernels (Context.last_step_kinds() tells which ran); options that must not change a bit;
repeats, replay neighbours and the filter API.  Every column is compared with the oracle's recurrence.  `-m gpu`.

Bar: gpu_helpers.TOL * 10 = 1e-10 (float64) / 2e-4 (float32) of max |reference|, as test_tile_gather_kernel holds the
recurrence and the Newton form to.  The same steps in numpy in the compute dtype stay within 1.2e-13 / 2.5e-6 of the
oracle (tests/test_program_host.py), 80 times and more inside the bar.

Worst figures on an MI355X, of max |reference| (the module's report prints them at the end of a run with -s; the
run's output is profiles/programs_on_tiles_pytest_gpu.log), float64 / float32:
    A  product form on tiles 8.0e-14 / 4.5e-6, on the plain kernels 8.0e-14 / 4.5e-6, Newton form on tiles 1.8e-15 / 9.0e-7
    B  off-piece widths 8.0e-14 / 2.9e-6, column batches 1.5e-14 / 1.5e-6, pipelined host call 2.2e-14 / 4.1e-7,
       unaligned y 1.5e-14
    C  default options 1.5e-14 / 1.9e-6 (every other setting: the same bits), other builds 1.6e-14 / 1.7e-6
    D  repeats 6.9e-14 / 1.1e-6, without tiles 1.5e-15;  E  filter API 3.3e-14
The module takes 10 s (331 tests, 0.3 s the slowest)."""
import numpy as np
import pytest

import tile_helpers
from gpu_helpers import ctx  # noqa: F401 (ctx is a fixture)
from oracle import cheby_oracle as orc
from program_helpers import POLYNOMIALS, shapes_for
from pygsp_amd import engine, filters, graphs
from tile_helpers import DTYPES, F64, GRAPHS, OFF_PIECE, ROW_BYTES, columns, expected_kinds, hold, options

pytestmark = pytest.mark.gpu


def case(name):
    """tile_helpers.case with the polynomials of the program tests."""
    return tile_helpers.case(name, POLYNOMIALS)


def device_graph(ctx, name, dtype, builder):
    return tile_helpers.device_graph(ctx, name, dtype, builder, POLYNOMIALS)


@pytest.fixture(scope="module", autouse=True)
def report():
    """After the module: the device's worst deviation per test and dtype; the device graphs go."""
    yield
    tile_helpers.finish()


def product_program(name, c, dtype):
    """The product-form program of polynomial `name`; its guard must hold (asserted, not filtered)."""
    ok, m = filters.product_guard(c, dtype)
    assert ok, (name, m)
    prog = filters.cheb_to_product(c, dtype)
    assert prog.shape[0] == shapes_for(dtype)[name][0]
    return prog


# ---- A: every program shape on every build -------------------------------------------------------------------------
@pytest.mark.parametrize("row_bytes", ROW_BYTES)
@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", GRAPHS)
def test_every_program_shape_on_every_tile_build(ctx, graph, dtype, builder, row_bytes):
    c = case(graph)
    dev = device_graph(ctx, graph, dtype, builder)
    w = row_bytes // np.dtype(dtype).itemsize
    x = columns(c, w)
    for name, coef in c["polys"].items():
        prog = product_program(name, coef, dtype)
        S = prog.shape[0]
        y, _ = dev.program_filter(prog, x, c["lmax"])
        assert ctx.last_step_kinds() == {"tile": S, "plain": 0}, (graph, w, name)
        hold("A product on tiles", dtype, y, c["ref"][name][:, :w], (graph, builder, w, name))
        with options(ctx, tile_gather=0):
            y, _ = dev.program_filter(prog, x, c["lmax"])
            assert ctx.last_step_kinds() == {"tile": 0, "plain": S}, (graph, w, name)
        hold("A product on plain kernels", dtype, y, c["ref"][name][:, :w], (graph, builder, w, name))
    for name in ("heat7/25", "heat5/2"):  # the Newton program: every step reads x
        prog = filters.newton_program(*filters.cheb_to_newton(c["polys"][name]))
        y, _ = dev.program_filter(prog, x, c["lmax"], old_is_x=True)
        assert ctx.last_step_kinds() == {"tile": prog.shape[0], "plain": 0}, (graph, w, name)
        hold("A newton on tiles", dtype, y, c["ref"][name][:, :w], (graph, builder, w, name))


# ---- B: the silent boundary ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", ["sensor4097", "hub3001", "rand577"])
def test_off_piece_widths_run_on_the_plain_kernels(ctx, graph, dtype):
    """Rows that are not whole 16-byte pieces: a program has no padded work panels, so every step is a plain launch."""
    c = case(graph)
    dev = device_graph(ctx, graph, dtype, "host")
    for w in OFF_PIECE[np.dtype(dtype)]:
        for name, coef in c["polys"].items():
            prog = product_program(name, coef, dtype)
            y, _ = dev.program_filter(prog, columns(c, w), c["lmax"])
            assert ctx.last_step_kinds() == {"tile": 0, "plain": prog.shape[0]}, (graph, w, name)
            hold("B off-piece widths", dtype, y, c["ref"][name][:, :w], (graph, w, name))


def test_the_restated_rule():
    assert expected_kinds(20, 8, 2, 3) == {"tile": 30, "plain": 0}      # ten 16-byte batches
    assert expected_kinds(40, 4, 2, 3) == {"tile": 0, "plain": 60}      # twenty 8-byte batches
    assert expected_kinds(20, 8, 8, 3) == {"tile": 9, "plain": 0}       # 8 + 8 + 4
    assert expected_kinds(40, 4, 8, 3) == {"tile": 15, "plain": 0}
    assert expected_kinds(20, 8, 20, 3) == {"tile": 3, "plain": 0}
    assert expected_kinds(40, 4, 20, 3) == {"tile": 6, "plain": 0}
    assert expected_kinds(33, 8, 0, 3) == {"tile": 0, "plain": 3}


@pytest.mark.parametrize("max_batch", [2, 8, 20])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", ["sensor4097", "hub3001"])
def test_column_batches_choose_their_kernel(ctx, graph, dtype, max_batch):
    c = case(graph)
    dt = np.dtype(dtype)
    dev = device_graph(ctx, graph, dtype, "device")
    w = 20 if dt == F64 else 40
    with options(ctx, max_batch=max_batch):
        for name in ("heat40/30", "pairs3", "heat5/1", "heat5/3"):
            prog = product_program(name, c["polys"][name], dtype)
            y, _ = dev.program_filter(prog, columns(c, w), c["lmax"])
            assert ctx.last_step_kinds() == expected_kinds(w, dt.itemsize, max_batch, prog.shape[0]), (graph, name)
            hold("B column batches", dtype, y, c["ref"][name][:, :w], (graph, max_batch, name))


@pytest.mark.parametrize("dtype", DTYPES)
def test_pipelined_host_call_sums_its_batches(ctx, dtype):
    """A host-array call forced through the pipelined form in three column batches of 64-byte rows: the counts are
    those of all its batches."""
    c = case("sensor4097+hub")
    dt = np.dtype(dtype)
    dev = device_graph(ctx, "sensor4097+hub", dtype, "host")
    per = 64 // dt.itemsize
    with options(ctx, host_pipeline=2, host_batch=per):
        for name in ("heat7/25", "heat5/1"):
            prog = product_program(name, c["polys"][name], dtype)
            y, _ = dev.program_filter(prog, columns(c, 3 * per), c["lmax"])
            assert ctx.last_host_timing()["batches"] == 3
            assert ctx.last_step_kinds() == {"tile": 3 * prog.shape[0], "plain": 0}, name
            hold("B pipelined host call", dtype, y, c["ref"][name][:, :3 * per], name)


@pytest.mark.parametrize("graph", ["sensor4097", "hub3001"])
def test_unaligned_output_runs_on_the_plain_kernels(ctx, graph):
    """y 8 bytes into a buffer: no 16-byte stores into it, so the plain kernels run - and write the panel only."""
    c = case(graph)
    dev = device_graph(ctx, graph, np.float64, "host")
    n, w, fill = c["n"], 8, 7.5
    x = columns(c, w)
    ybuf = np.full(n * w + 4, fill)
    bx, by = ctx.take(x.nbytes), ctx.take(ybuf.nbytes)
    try:
        bx.upload(x)
        for name in ("heat40/30", "pairs3"):
            prog = product_program(name, c["polys"][name], np.float64)
            by.upload(ybuf)
            dev.program_filter_dev(prog, bx.ptr, by.ptr + 8, w, c["lmax"])
            assert ctx.last_step_kinds() == {"tile": 0, "plain": prog.shape[0]}, name
            back = by.download(ybuf.shape, np.float64)
            assert back[0] == fill and np.all(back[1 + n * w:] == fill), "the buffer around the panel was written"
            hold("B unaligned y", np.float64, back[1:1 + n * w].reshape(n, w), c["ref"][name][:, :w], (graph, name))
            # the same call into the aligned buffer: the tile kernel, the same panel and nothing else
            by.upload(ybuf)
            dev.program_filter_dev(prog, bx.ptr, by.ptr, w, c["lmax"])
            assert ctx.last_step_kinds() == {"tile": prog.shape[0], "plain": 0}, name
            back = by.download(ybuf.shape, np.float64)
            assert np.all(back[n * w:] == fill)
            hold("B unaligned y", np.float64, back[:n * w].reshape(n, w), c["ref"][name][:, :w], (graph, name, "aligned"))
    finally:
        ctx.give(bx)
        ctx.give(by)


# ---- C: options that must not change a bit -------------------------------------------------------------------------
SAME_BITS = ([{"tile_nt": v} for v in (0, 1, 4, 5, 8, 15)] + [{"tile_workgroups": v} for v in (8, 64, 4096)] +
             [{"alternate_sweep": 0}, {"xcd_remap": 0}])


@pytest.mark.parametrize("dtype,width", [(np.float64, 16), (np.float64, 64), (np.float32, 32), (np.float32, 128)])
@pytest.mark.parametrize("graph", ["sensor4097", "sensor4097+hub", "hub3001"])
def test_cache_hints_and_block_walks_keep_every_bit(ctx, graph, dtype, width):
    """Non-temporal accesses (tile_nt: entries, T_{k-2} loads, accumulator, the out store), the number of persistent
    workgroups, the sweep direction and the XCD mapping change who walks which block and how the caches are asked -
    never the arithmetic of a row."""
    c = case(graph)
    dev = device_graph(ctx, graph, dtype, "device")
    x = columns(c, width)
    for name in ("heat40/30", "pairs3"):
        prog = product_program(name, c["polys"][name], dtype)
        y0, _ = dev.program_filter(prog, x, c["lmax"])
        assert ctx.last_step_kinds() == {"tile": prog.shape[0], "plain": 0}
        hold("C default options", dtype, y0, c["ref"][name][:, :width], (graph, width, name))
        for opts in SAME_BITS:
            with options(ctx, **opts):
                y1, _ = dev.program_filter(prog, x, c["lmax"])
                assert ctx.last_step_kinds() == {"tile": prog.shape[0], "plain": 0}, opts
            assert np.array_equal(y0, y1), (graph, width, name, opts, rel_err(y1, y0))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", ["sensor4097", "hub3001"])
def test_other_builds_for_the_same_rows(ctx, graph, dtype):
    """tile_regroup = 0: 48- / 80- / 160-byte rows on the power-of-two builds; tile_lg: 16- / 32-byte rows on the 2- / 4- /
    8-lane builds.  Other builds sum a row's products in the same order but need not give the same bits: held to the
    oracle."""
    c = case(graph)
    dt = np.dtype(dtype)
    dev = device_graph(ctx, graph, dtype, "host")
    per = 16 // dt.itemsize
    runs = [({"tile_regroup": 0}, pieces * per) for pieces in (3, 5, 10)]
    runs += [({"tile_lg": lg}, pieces * per) for lg in (2, 4, 8) for pieces in (1, 2)]
    for opts, w in runs:
        for name in ("heat40/30", "pairs3", "heat5/3"):
            prog = product_program(name, c["polys"][name], dtype)
            with options(ctx, **opts):
                y, _ = dev.program_filter(prog, columns(c, w), c["lmax"])
                assert ctx.last_step_kinds() == {"tile": prog.shape[0], "plain": 0}, (opts, w)
            hold("C other builds", dtype, y, c["ref"][name][:, :w], (graph, opts, w, name))


# ---- D: repeats and neighbours -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_repeats_and_replayed_neighbours(ctx, dtype):
    c = case("sensor4097")
    dt = np.dtype(dtype)
    dev = device_graph(ctx, "sensor4097", dtype, "device")
    w = 16 if dt == F64 else 32
    x = columns(c, w)
    prog = product_program("heat7/25", c["polys"]["heat7/25"], dtype)
    ya, _ = dev.program_filter(prog, x, c["lmax"])
    yb, _ = dev.program_filter(prog, x, c["lmax"])
    assert np.array_equal(ya, yb)
    hold("D repeats", dtype, ya, c["ref"]["heat7/25"][:, :w], "product")
    # a recurrence call that replays its recorded launches, a program between it and its next call
    coef = c["polys"]["heat40/30"]
    with options(ctx, graph_launch=2):
        r1, _ = dev.cheby_filter(coef, x, c["lmax"])
        kinds = ctx.last_step_kinds()
        assert kinds["tile"] > 0 and kinds["plain"] == 0, kinds
        dev.cheby_filter(coef, x, c["lmax"])  # (the first call may have grown a workspace: the addresses settle here)
        r2, _ = dev.cheby_filter(coef, x, c["lmax"])  # an identical call: recorded and replayed, or replayed
        t = ctx.last_timing()
        assert t["total_ms"] == t["steps_ms"] > 0, t  # (a replayed call reports one time)
        assert ctx.last_step_kinds() == kinds  # ... and the counts stored with its recording
        yc, _ = dev.program_filter(prog, x, c["lmax"])
        assert ctx.last_step_kinds() == {"tile": prog.shape[0], "plain": 0}
        r3, _ = dev.cheby_filter(coef, x, c["lmax"])
        assert ctx.last_step_kinds() == kinds
    assert np.array_equal(r1, r2) and np.array_equal(r1, r3) and np.array_equal(ya, yc)
    hold("D repeats", dtype, r1[0], c["ref"]["heat40/30"][:, :w], "recurrence")


def test_without_tiles_a_program_runs_on_the_plain_kernels(ctx):
    c = case("rand577")
    dev = engine.DeviceGraph.from_w(c["W"], c["lap"], dtype=np.float64, perm=c["perm"], ctx=ctx)
    try:
        x = columns(c, 16)
        prog = product_program("pairs3+real", c["polys"]["pairs3+real"], np.float64)
        S = prog.shape[0]
        dev.program_filter(prog, x, c["lmax"])
        assert ctx.last_step_kinds() == {"tile": 0, "plain": S}  # never had tiles
        dev.build_gather_tiles()
        y1, _ = dev.program_filter(prog, x, c["lmax"])
        assert ctx.last_step_kinds() == {"tile": S, "plain": 0}
        dev.disable_gather_tiles()
        y0, _ = dev.program_filter(prog, x, c["lmax"])
        assert ctx.last_step_kinds() == {"tile": 0, "plain": S}
        hold("D without tiles", np.float64, y1, c["ref"]["pairs3+real"][:, :16], "tiles")
        hold("D without tiles", np.float64, y0, c["ref"]["pairs3+real"][:, :16], "disabled")
    finally:
        dev.destroy()


# ---- E: through the filter API -------------------------------------------------------------------------------------
def test_product_form_through_the_filter_api(ctx):
    c = case("sensor4097")
    W, coords = graphs.sensor_weights(4097, k=8, seed=31)
    G = graphs.Graph(W, coords=coords, reorder="hilbert", tiles=True, ctx=ctx)
    G.estimate_lmax("bounds")
    assert G.device_graph().ctx is ctx and G.tile_stats["nb"] == 65, G.tile_stats
    x = c["x"][:, :64]
    y = filters.Heat(G, 10).filter(x, order=30, evaluation="product")
    assert G._gspx_last_evaluation == "product"
    S = filters.cheb_to_product(filters.compute_cheby_coeff(filters.Heat(G, 10), m=30), np.float64).shape[0]
    assert ctx.last_step_kinds() == {"tile": S, "plain": 0}
    ref = orc.filter_chebyshev(c["L"], G.lmax, [orc.heat_kernel(10, G.lmax)], x, 30)
    hold("E filter API", np.float64, y, ref, "Heat(10), order 30")
