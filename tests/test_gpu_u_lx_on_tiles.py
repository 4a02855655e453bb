"""y = L x and x^T L x (gspx_laplacian_apply_dev / gspx_dirichlet_energy_dev; lap_apply_t and dirichlet_t of
gspx_ops.hip.h) on small graphs that carry gather tiles - the product every solver of the package runs.

lap_apply_t has three routes, and tile_helpers.expected_kinds_lx restates which one a call takes and which kernel
each of its launches is:
- fused: ONE launch of the tile kernel gathers from the caller's panel (the tile lists mapped through the vertex
  order) and writes y in the caller's order.  Needs the panel in one batch, fuse_input, no slow block (the band graphs
  here), x 16-byte aligned and apart from y, rows of whole 16-byte pieces;
- one batch through the workspace (permute-in, then the tile or the plain kernel writing y);
- column batches (max_batch) that write y + c0 with ldy = Nsig: the tile kernel only where y + c0 is 16-byte aligned
  and the batch's rows and y's rows are whole pieces.
The launch counters are not zeroed by the operators and every launcher counts, so each call is held to the DIFFERENCE
of Context.last_step_kinds() around it.  Fused and unfused calls both run the tile kernel on the same lists in the
same order, one through row indices of the caller's panel and one on the permuted copy: they must agree bit for bit,
and test_fused_route_and_its_ways_out asserts it.

Bar: gpu_helpers.TOL * 10 of max |reference| for L x against the oracle's L @ X (tile_helpers.hold), and what
test_dirichlet_shared_gram holds the energy to (test_gpu_4_ops.TOL * 10 = 1e-11 / 3e-4)."""
import numpy as np
import pytest

import tile_helpers
from conftest import rel_err
from gpu_helpers import ctx  # noqa: F401 (ctx: fixture)
from operator_pins_helpers import no_polynomials
from oracle import ops_oracle as ops
from tile_helpers import DTYPES, F64, OFF_PIECE, OPTIONS, ROW_BYTES, columns, expected_kinds_lx, hold

pytestmark = pytest.mark.gpu

GRAPHS = ["sensor4097", "sensor4097+hub", "hub3001-normalized", "rand65", "band4097", "band4097-shuffled"]
ENERGY_TOL = {np.dtype(np.float64): 1e-11, np.dtype(np.float32): 3e-4}  # test_dirichlet_shared_gram's
BASE = dict(OPTIONS, graph_launch=0)
_REF, _SLOW = {}, {}


def options(ctx, **kw):
    return tile_helpers.options(ctx, base=BASE, **kw)


@pytest.fixture(scope="module", autouse=True)
def report(ctx):
    ctx.set_option("graph_launch", 0)
    yield
    tile_helpers.finish()


def case(graph):
    """The graph's case with the oracle's L @ X of its 192 columns."""
    c = tile_helpers.case(graph, no_polynomials)
    if graph not in _REF:
        _REF[graph] = c["L"].dot(c["x"])
        _REF[graph].setflags(write=False)
    return c, _REF[graph]


def device_graph(ctx, graph, dtype, builder):
    """The cached device graph with `builder`'s tiles and its number of slow blocks."""
    dev = tile_helpers.device_graph(ctx, graph, dtype, builder, no_polynomials)
    key = (graph, np.dtype(dtype), builder)
    if key not in _SLOW:  # (the same builder once more: the same tiles, and their statistics)
        _SLOW[key] = (dev.enable_gather_tiles() if builder == "host" else dev.build_gather_tiles())["slow_blocks"]
    return dev, _SLOW[key]


def widths(dtype):
    dt = np.dtype(dtype)
    return sorted(set([b // dt.itemsize for b in ROW_BYTES] + OFF_PIECE[dt]))


def counted(ctx, call):
    """call() and the launches it made: the counters' difference."""
    before = ctx.last_step_kinds()
    out = call()
    after = ctx.last_step_kinds()
    return out, {k: after[k] - before[k] for k in after}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("graph", GRAPHS)
def test_lx_routes_and_values(ctx, graph, builder, dtype):
    c, ref = case(graph)
    dev, slow = device_graph(ctx, graph, dtype, builder)
    elt = np.dtype(dtype).itemsize
    if graph.startswith("band4097"):
        assert slow == 0  # the fused route is open here
    batched = on_tiles = 0
    for w in widths(dtype):
        x = columns(c, w)
        for fuse in (1, 0):
            for tg in (1, 0):
                for mb in (0, 3, 4, 8):
                    with options(ctx, fuse_input=fuse, tile_gather=tg, max_batch=mb):
                        y, kinds = counted(ctx, lambda: dev.laplacian_apply(x))
                    want = expected_kinds_lx(w, elt, max_batch=mb, fuse_input=fuse, tile_gather=tg, slow_blocks=slow)
                    where = (graph, builder, "w=%d" % w, "fuse=%d tiles=%d max_batch=%d" % (fuse, tg, mb))
                    assert kinds == want, (where, kinds, want)
                    hold("L x", dtype, y, ref[:, :w], where)
                    batched += sum(want.values()) > 1
                    on_tiles += want["tile"] > 0
    assert batched > 0 and on_tiles > 0, (batched, on_tiles)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", ["band4097", "band4097-shuffled", "sensor4097+hub"])
def test_fused_route_and_its_ways_out(ctx, graph, dtype):
    """On the band graphs the default call is fused.  The same call with fuse_input = 0, in place (y_ptr == x_ptr) and -
    float64 - with x at an 8-byte offset into its buffer must step off the fused route, still take the tile kernel for
    its one batch, and return the fused call's bits: the tile kernel sums every row over the same list in the same
    order on either route.  On the graph with a slow block no call fuses; the same calls are held to the oracle."""
    c, ref = case(graph)
    dev, slow = device_graph(ctx, graph, dtype, "device")
    dt = np.dtype(dtype)
    one_tile = {"tile": 1, "plain": 0}
    for w in (16 // dt.itemsize, 64 // dt.itemsize, 64, 96):
        x = columns(c, w).astype(dtype)
        where = (graph, dt.name, "w=%d" % w)
        y, kinds = counted(ctx, lambda: dev.laplacian_apply(x))
        assert kinds == one_tile == expected_kinds_lx(w, dt.itemsize, slow_blocks=slow), (where, kinds)
        hold("L x fused" if slow == 0 else "L x, a slow block", dtype, y, ref[:, :w], where)
        with options(ctx, fuse_input=0):
            y0, kinds = counted(ctx, lambda: dev.laplacian_apply(x))
        assert kinds == one_tile, (where, kinds)
        assert y0.tobytes() == y.tobytes(), (where, "fused and unfused differ")
        # in place, and x at an 8-byte offset: through the device pointers
        pad = 8 // dt.itemsize
        buf = ctx.alloc((x.size + pad) * dt.itemsize)
        out = ctx.alloc(x.size * dt.itemsize)
        try:
            buf.upload(np.concatenate([x.ravel(), np.zeros(pad, dtype=dtype)]))
            _, kinds = counted(ctx, lambda: dev.laplacian_apply_dev(buf.ptr, buf.ptr, w))
            want = expected_kinds_lx(w, dt.itemsize, slow_blocks=slow, in_place=True)
            assert kinds == one_tile == want, (where, kinds)
            yi = buf.download((x.size + pad,), dtype)[:x.size].reshape(x.shape)
            assert yi.tobytes() == y.tobytes(), (where, "in place")
            if dt == F64:
                buf.upload(np.concatenate([np.zeros(1), x.ravel()]))
                _, kinds = counted(ctx, lambda: dev.laplacian_apply_dev(buf.ptr + 8, out.ptr, w))
                assert kinds == one_tile == expected_kinds_lx(w, 8, slow_blocks=slow, x_offset=8), (where, kinds)
                yo = out.download(x.shape, dtype)
                assert yo.tobytes() == y.tobytes(), (where, "x at an 8-byte offset")
        finally:
            buf.free()
            out.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("graph", GRAPHS)
def test_dirichlet_energy_on_tile_graphs(ctx, graph, builder, dtype):
    c, _ = case(graph)
    dev, _ = device_graph(ctx, graph, dtype, builder)
    tol = ENERGY_TOL[np.dtype(dtype)]
    for w in (1, 2, 15, 16, 64, 65):
        x = columns(c, w)
        want = ops.dirichlet_energy(c["L"], x)
        for tg in (1, 0):
            with options(ctx, tile_gather=tg):
                gram, kinds = counted(ctx, lambda: dev.dirichlet_energy(x))
                again = dev.dirichlet_energy(x)
            where = (graph, builder, "w=%d" % w, "tiles=%d" % tg)
            tile = tg and (w * np.dtype(dtype).itemsize) % 16 == 0  # (one batch into the workspace: no y to align)
            assert kinds == ({"tile": 1, "plain": 0} if tile else {"tile": 0, "plain": 1}), (where, kinds)
            assert gram.shape == (w, w) and gram.tobytes() == again.tobytes(), where
            err = rel_err(gram, want)
            key = ("Dirichlet energy", np.dtype(dtype).name)
            if err >= tile_helpers._WORST.get(key, (-1.0, None))[0]:
                tile_helpers._WORST[key] = (err, where)
            assert err < tol, (where, err)
            assert rel_err(gram.T, gram) <= tol, (where, "symmetry")
