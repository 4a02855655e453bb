"""The flush-free builds of k_step_tile (gspx_tile_kernels.hip.h, ACC = false; option tile_acc_builds) at small shapes.

A step without a flush - every step of a Newton or product program, and the steps of a single filter's recurrence
between two flushes - runs a build that carries no accumulator rows, forms no flush, and spells the row formula's three
roundings out (left to the compiler's contraction, the Newton form's last bit moved).  One of the six - float32, two
chunks per row: rows of 272 and 512 bytes - also requests the NEXT pass's T_{k-2} rows right after the first barrier of
a pass, into a second register set (TileSchedule::EARLY_OLD).  tile_acc_builds = 0 sends every step to the general
build.  The two must leave the same bits, issue the same launches, and stay within the bar of the oracle.

What a flush-free build and the early request add to a workgroup's walk, and which case runs it:
    the request from chunk c to chunk c + 1 of a block               rows of 272 / 512 bytes (NCOL = 2), 528 / 768 (NCOL = 0)
    a partly filled last chunk (lanes beyond the row switched off)    rows of 272 and 528 bytes
    the request from a block's last chunk into the NEXT block,
      the two register sets swapping across the block boundary,
      and the end of the walk (the last pass requests nothing)        tile_workgroups = 8: 8 blocks and more per workgroup
                                                                      (the default grid gives every workgroup ONE block)
    an odd number of chunks per block (the sets' parity differs       rows of 528 / 768 bytes (3 chunks), 8 workgroups
      from block to block)
    a last block of a single row (rows beyond N poisoned)             sensor4097, band4097 (4097 = 64 * 64 + 1)
    slow (plain-gather) blocks between staged ones                    sensor4097+hub, hub3001
    gamma = 0: no T_{k-2} request at all, both sets stay zero         order 1 (step 1 alone), the product program's
                                                                      two-pass steps
    every kind of launch in one call                                  order 7 (steps 1, 2, flush-free, flushes, the last)
    the walk backwards / forwards                                     alternate_sweep 1 / 0
    a recorded and replayed call                                      graph_launch 1 (the third identical call replays)
    steps 1 and 2 on the caller's panel (gt_s1nat, OLDNAT) or not     fuse_input 1 / 0 on the band graphs
"""
import numpy as np
import pytest

import tile_helpers
from gpu_helpers import ctx  # noqa: F401 (ctx is a fixture)
from program_helpers import POLYNOMIALS as PROGRAM_POLYNOMIALS
from pygsp_amd import _capi, filters
from recurrence_helpers import POLYNOMIALS as RECURRENCE_POLYNOMIALS
from recurrence_helpers import SINGLE, steps
from tile_helpers import BAND_GRAPHS, DTYPES, MAXW, OPTIONS, columns, hold

pytestmark = pytest.mark.gpu

GRAPHS = ["sensor4097", "sensor4097+hub", "hub3001", "band4097", "band4097-shuffled"]
ROW_BYTES = [256, 272, 512, 528, 768]
NEWTON, PRODUCT = "heat7/25", "heat40/30"
BASE = dict(OPTIONS, tile_acc_builds=1)


def POLYS(lmax):
    """Heat(20) at orders 1, 2, 3, 7 and 30 (recurrence_helpers) and the polynomials of the Newton and the product
    program (program_helpers)."""
    rec, prog = RECURRENCE_POLYNOMIALS(lmax), PROGRAM_POLYNOMIALS(lmax)
    polys = {name: rec[name] for name in SINGLE}
    polys[NEWTON], polys[PRODUCT] = prog[NEWTON], prog[PRODUCT]
    return polys


def options(ctx, **kw):
    return tile_helpers.options(ctx, base=BASE, **kw)


@pytest.fixture(scope="module", autouse=True)
def report(ctx):
    yield
    ctx.set_option("tile_acc_builds", 1)
    tile_helpers.finish()


def both_builds(ctx, call, calls=1):
    """{tile_acc_builds: (result, last_step_kinds)} of `call`, made `calls` times in a row (the last one counts)."""
    out = {}
    for acc in (1, 0):
        with options(ctx, tile_acc_builds=acc):
            for _ in range(calls):
                y = call()
            out[acc] = (y, ctx.last_step_kinds())
    return out


def same(out, where):
    (y1, k1), (y0, k0) = out[1], out[0]
    assert k1 == k0, (where, k1, k0)
    assert np.array_equal(y1, y0), (where, "flush-free against general build",
                                    float(np.max(np.abs(y1.astype(np.float64) - y0.astype(np.float64)))))
    return y1, k1


@pytest.mark.parametrize("row_bytes", ROW_BYTES)
@pytest.mark.parametrize("workgroups", [0, 8])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", GRAPHS)
def test_flushfree_builds_keep_every_bit_of_the_recurrence(ctx, graph, dtype, workgroups, row_bytes):
    c = tile_helpers.case(graph, POLYS)
    dev = tile_helpers.device_graph(ctx, graph, dtype, "device", POLYS)
    w = row_bytes // np.dtype(dtype).itemsize
    x = columns(c, w)
    for sweep in (1, 0):
        for launch in (0, 1):
            for fuse in ((1, 0) if graph in BAND_GRAPHS else (1,)):
                with options(ctx, tile_workgroups=workgroups, alternate_sweep=sweep, graph_launch=launch, fuse_input=fuse):
                    for name in SINGLE:
                        where = (graph, np.dtype(dtype).name, "w=%d" % w, name, "workgroups=%d" % workgroups,
                                 "sweep=%d launch=%d fuse=%d" % (sweep, launch, fuse))
                        out = both_builds(ctx, lambda: dev.cheby_filter(c["polys"][name], x, c["lmax"], _capi.ANALYSIS)[0],
                                          calls=3 if launch else 1)
                        y, kinds = same(out, where)
                        K = steps(c["polys"][name])
                        assert kinds == {"tile": K, "plain": 0}, (where, kinds)
                        hold("recurrence", dtype, y, c["ref"][name].reshape(-1, c["n"], MAXW)[:, :, :w], where)


@pytest.mark.parametrize("row_bytes", ROW_BYTES)
@pytest.mark.parametrize("workgroups", [0, 8])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", GRAPHS)
def test_flushfree_builds_keep_every_bit_of_the_programs(ctx, graph, dtype, workgroups, row_bytes):
    """Every step of a program is flush-free: the Newton form (every step reads x as its third panel, the last one
    stores y) and the product form (two-pass steps with gamma = 0, three-pass steps that overwrite h_{s-1} in place)."""
    c = tile_helpers.case(graph, POLYS)
    dev = tile_helpers.device_graph(ctx, graph, dtype, "device", POLYS)
    w = row_bytes // np.dtype(dtype).itemsize
    x = columns(c, w)
    ok, m = filters.product_guard(c["polys"][PRODUCT], dtype)
    assert ok, m
    programs = {"newton": (filters.newton_program(*filters.cheb_to_newton(c["polys"][NEWTON])), True, NEWTON),
                "product": (filters.cheb_to_product(c["polys"][PRODUCT], dtype), False, PRODUCT)}
    assert np.any(programs["product"][0][1:, 2] == 0) and np.any(programs["product"][0][1:, 2] != 0)
    for sweep in (1, 0):
        with options(ctx, tile_workgroups=workgroups, alternate_sweep=sweep):
            for form, (prog, old_is_x, name) in programs.items():
                where = (graph, np.dtype(dtype).name, "w=%d" % w, form, "workgroups=%d" % workgroups, "sweep=%d" % sweep)
                out = both_builds(ctx, lambda: dev.program_filter(prog, x, c["lmax"], old_is_x=old_is_x)[0])
                y, kinds = same(out, where)
                assert kinds == {"tile": prog.shape[0], "plain": 0}, (where, kinds)
                hold(form, dtype, y, c["ref"][name].reshape(-1, c["n"], MAXW)[0][:, :w], where)
