"""gspx_cheby_sqnorms_dev (k_combine_sqnorm<T, FB> and k_sqnorm_reduce; sqnorms_dev_t of gspx_poly.hip.h) at small
shapes, against the oracle as test_gpu_e_features has it (cheby_op, then the sum of squares in float64) on the input
rounded to the compute dtype.

- graphs of 1 (an isolated vertex), 63, 65 and 257 vertices - below one tile of rows, one row over it, several
  workgroups - at widths 1 ... 130: every cwl (tile columns 1 ... 64), one and three column blocks, a last block with
  one and two live columns; both dtypes;
- bank sizes 1 ... 257: every build (FB = 2 up to 8 filters of a pass, 8 up to 32, 32 up to 128) and one, two and
  three passes, the last of one filter (129, 257), in both dtypes;
- M = 2 ... 256 coefficients with 1, 9 and 100 filters: from M = 129 on the M x 512 bytes of LDS need
  hipFuncSetAttribute, once per build and dtype, up to 128 KiB at M = 256; 257 is refused with the library's message
  and the library goes on working;
- tile and plain steps side by side on three graphs with gather tiles;
- column batches with a ragged last batch.

Bars: gpu_helpers.TOL (1e-11 / 2e-5) wherever M <= 31, as the existing tests.  For M >= 128 float64 keeps it - the
oracle's own error against a longdouble recurrence is 7e-16 ... 1.7e-14 there, so nothing had to move.  float32 has
no project figure at such orders: operator_pins_helpers.sqnorms_bar measures a float32 numpy recurrence against the
oracle on the very inputs and gives the device max(TOL, 4 x that figure).  The figures measured on the CPU (N = 257,
w = 5; tests/test_operator_pins_host.py prints them; 4 x covers another summation order in a row and FMA contraction):

    Nf   M=128    M=129    M=200    M=256
      1  1.78e-05 8.07e-06 5.77e-07 3.35e-05      bars 7.12e-05 3.23e-05 2.00e-05 1.34e-04
      9  1.42e-05 1.90e-06 2.85e-05 2.31e-05           5.69e-05 2.00e-05 1.14e-04 9.24e-05
    100  1.63e-05 1.87e-05 4.04e-05 4.83e-05           6.51e-05 7.48e-05 1.61e-04 1.93e-04

The device measured 4.79e-05 at worst there (Nf 100, M 256), and 7.4e-15 in float64; every case prints its device
figure, the CPU figure and the bar (profiles/operator_pins_pytest_gpu.log).

The launches of the recurrence steps are held to tile_helpers.expected_kinds_recurrence with combine = 2 (the call
always defers).  The library's rule for this entry differs from the helper's in one point: it has no y, so
work_panels sees y = null and ldy = ld - a batch is DIRECT on the tile kernels iff its own rows are whole 16-byte
pieces of at least tile_min_row bytes, whatever the call's width and the batch's first column are, where the helper
also asks for Nsig to be whole pieces and y + c0 to be aligned and otherwise pads.  Direct and padded batches both count
as tile launches, and padding is on here (tile_pad = 1, every batch of two columns or more), so the two rules give the
same counts in every case of this module; sqnorm_kinds restates the library's own."""
import numpy as np
import pytest
from scipy import sparse

import tile_helpers
from conftest import rel_err
from gpu_helpers import TOL, ctx, random_graph, upper_lmax  # noqa: F401 (ctx: fixture)
from operator_pins_helpers import (LONG_M, LONG_NF, bank_coefficients, long_case, no_polynomials, oracle_sqnorms,
                                   sqnorms_bar)
from oracle import cheby_oracle as orc
from pygsp_amd import engine
from tile_helpers import DTYPES, OPTIONS, batch_columns, expected_kinds_recurrence

pytestmark = pytest.mark.gpu

BASE = dict(OPTIONS, graph_launch=0)  # every call eager: last_step_kinds() counts the call's own launches
_SMALL, _DEVS, _WORST = {}, {}, tile_helpers._WORST


def options(ctx, **kw):
    return tile_helpers.options(ctx, base=BASE, **kw)


@pytest.fixture(scope="module", autouse=True)
def report(ctx):
    ctx.set_option("graph_launch", 0)
    yield
    while _DEVS:
        _DEVS.popitem()[1].destroy()
    tile_helpers.finish()


def small(N):
    """(W, L, lmax) of the graphs of test_moments_small_shapes."""
    if N not in _SMALL:
        W = random_graph(N, 4, seed=N) if N > 1 else sparse.csr_matrix((1, 1))
        _SMALL[N] = (W, orc.laplacian(W), upper_lmax(W) if N > 1 else 1.0)  # (one isolated vertex: L = 0, any lmax)
    return _SMALL[N]


def device(ctx, N, dtype):
    key = (N, np.dtype(dtype))
    if key not in _DEVS:
        _DEVS[key] = engine.DeviceGraph.from_w(small(N)[0], dtype=dtype, ctx=ctx)
    return _DEVS[key]


def sqnorms(dev, C, x, lmax):
    """Two device calls on x in the graph's dtype: the result, the same bytes the second time."""
    d = engine.DeviceArray.from_host(dev.ctx, x, dev.dtype)
    try:
        s, _ = dev.cheby_sqnorms_dev(C, d.ptr, x.shape[1], lmax)
        kinds = dev.ctx.last_step_kinds()
        s2, _ = dev.cheby_sqnorms_dev(C, d.ptr, x.shape[1], lmax)
    finally:
        d.free()
    assert s.shape == (C.shape[0], x.shape[1]) and s.dtype == np.float64 and np.all(np.isfinite(s))
    assert s.tobytes() == s2.tobytes()
    return s, kinds


def hold(test, dtype, s, ref, bar, where):
    err = rel_err(s, ref)
    key = (test, np.dtype(dtype).name)
    if err >= _WORST.get(key, (-1.0, None))[0]:
        _WORST[key] = (err, where)
    assert err < bar, (where, err, bar)
    return err


def rounded(x, dtype):
    return np.asarray(x).astype(dtype).astype(np.float64)


def sqnorm_kinds(nsig, elt, K, max_batch=0, tile_gather=1, tiles=True, tile_pad=1, tile_min_row=16):
    """sqnorms_dev_t's own rule (see the module docstring): K steps per column batch; direct iff the batch's rows are
    whole pieces of at least tile_min_row bytes, else padded iff tile_pad is on, the batch has two columns or more and
    the padded rows have tile_min_row bytes; else plain."""
    tvec = 16 // elt
    kinds = {"tile": 0, "plain": 0}
    for _, ld in batch_columns(nsig, max_batch):
        ldp = (ld + tvec - 1) // tvec * tvec
        direct = ld % tvec == 0 and ld * elt >= tile_min_row
        padded = not direct and bool(tile_pad) and (tile_pad == 2 or ld >= 2) and ldp * elt >= tile_min_row
        kinds["tile" if tiles and tile_gather and (direct or padded) else "plain"] += K
    return kinds


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 63, 65, 257])
def test_small_graphs_and_every_width(ctx, N, dtype):
    W, L, lmax = small(N)
    dev = device(ctx, N, dtype)
    C = bank_coefficients(9, 12, seed=N)
    x = rounded(np.random.default_rng(N).standard_normal((N, 130)), dtype)
    ref = oracle_sqnorms(L, lmax, C, x)
    for w in (1, 2, 3, 5, 33, 64, 65, 130):
        s, kinds = sqnorms(dev, C, np.ascontiguousarray(x[:, :w]), lmax)
        assert kinds == {"tile": 0, "plain": 11}, (N, w, kinds)  # (no gather tiles on these graphs)
        hold("small graphs, widths", dtype, s, ref[:, :w], TOL[np.dtype(dtype)], (N, w))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nf", [1, 8, 9, 32, 33, 128, 129, 257])
def test_bank_sizes_and_passes(ctx, nf, dtype):
    W, L, lmax = small(257)
    dev = device(ctx, 257, dtype)
    C = bank_coefficients(nf, 12, seed=nf)
    x = rounded(np.random.default_rng(nf).standard_normal((257, 64)), dtype)
    ref = oracle_sqnorms(L, lmax, C, x)
    for w in (5, 64):
        s, _ = sqnorms(dev, C, np.ascontiguousarray(x[:, :w]), lmax)
        hold("bank sizes", dtype, s, ref[:, :w], TOL[np.dtype(dtype)], (nf, w))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nf", [1, 9, 100])
def test_short_recurrences(ctx, nf, dtype):
    W, L, lmax = small(257)
    dev = device(ctx, 257, dtype)
    x = rounded(np.random.default_rng(nf).standard_normal((257, 5)), dtype)
    for M in (2, 3, 31):
        C = bank_coefficients(nf, M, seed=1000 * nf + M)
        s, kinds = sqnorms(dev, C, x, lmax)
        assert kinds == {"tile": 0, "plain": M - 1}, (nf, M, kinds)
        hold("M <= 31", dtype, s, oracle_sqnorms(L, lmax, C, x), TOL[np.dtype(dtype)], (nf, M))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", LONG_M)
@pytest.mark.parametrize("nf", LONG_NF)
def test_long_recurrences(ctx, nf, M, dtype):
    """M = 128 still fits the default 64 KiB of LDS; 129, 200 and 256 ask for more, once per build (nf 1 -> FB 2, 9 ->
    FB 8, 100 -> FB 32) and dtype.  The bar: the module docstring."""
    W, L, lmax, C, x, ref = long_case(nf, M, dtype)
    bar, figure = sqnorms_bar(L, lmax, C, x, dtype, ref, TOL[np.dtype(dtype)])
    if np.dtype(dtype) == np.float64:
        assert bar == TOL[np.dtype(dtype)], (figure, "the oracle itself misses the float64 bar")
    s, kinds = sqnorms(device(ctx, 257, dtype), C, x, lmax)
    assert kinds == {"tile": 0, "plain": M - 1}, (nf, M, kinds)
    err = hold("M >= 128", dtype, s, ref, bar, (nf, M))
    print("sqnorms Nf {:3d} M {:3d} {:<8s} device {:.2e} cpu figure {:.2e} bar {:.2e}".format(
        nf, M, np.dtype(dtype).name, err, figure, bar))


def test_more_than_256_coefficients_are_refused(ctx):
    W, L, lmax = small(257)
    x = np.random.default_rng(5).standard_normal((257, 5))
    for dtype in DTYPES:
        dev = device(ctx, 257, dtype)
        d = engine.DeviceArray.from_host(ctx, x, dtype)
        try:
            with pytest.raises(ValueError, match="at most 256 coefficients per filter"):
                dev.cheby_sqnorms_dev(bank_coefficients(9, 257, seed=0), d.ptr, 5, lmax)
        finally:
            d.free()
        # ... and the library goes on working: one earlier case again
        _, _, _, C, xl, ref = long_case(9, 129, dtype)
        bar, _ = sqnorms_bar(L, lmax, C, xl, dtype, ref, TOL[np.dtype(dtype)])
        s, _ = sqnorms(dev, C, xl, lmax)
        hold("after the refusal", dtype, s, ref, bar, (9, 129))


TILE_GRAPHS = ["sensor4097", "hub3001", "rand65"]
_TILE_REF = {}


def tile_case(graph):
    """The graph's case and the oracle's squared norms of 9 filters of 12 coefficients on its first 96 columns."""
    c = tile_helpers.case(graph, no_polynomials)
    if graph not in _TILE_REF:
        C = bank_coefficients(9, 12, seed=len(graph))
        _TILE_REF[graph] = (C, oracle_sqnorms(c["L"], c["lmax"], C, c["x"][:, :96]))
    return (c,) + _TILE_REF[graph]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("graph", TILE_GRAPHS)
def test_tile_and_plain_steps_side_by_side(ctx, graph, builder, dtype):
    c, C, ref = tile_case(graph)
    dev = tile_helpers.device_graph(ctx, graph, dtype, builder, no_polynomials)
    elt = np.dtype(dtype).itemsize
    for w in (4, 5, 64, 96):
        x = tile_helpers.columns(c, w)
        for tg in (1, 0):
            with options(ctx, tile_gather=tg):
                s, kinds = sqnorms(dev, C, x, c["lmax"])
            want = expected_kinds_recurrence(w, elt, 9, 11, combine=2, tile_gather=tg)
            assert want == sqnorm_kinds(w, elt, 11, tile_gather=tg) == ({"tile": 11, "plain": 0} if tg else
                                                                        {"tile": 0, "plain": 11})
            assert kinds == want, (graph, builder, w, tg, kinds, want)
            hold("tile steps" if tg else "plain steps on a tile graph", dtype, s, ref[:, :w], TOL[np.dtype(dtype)],
                 (graph, builder, w))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("max_batch", [3, 8])
def test_column_batches(ctx, max_batch, dtype):
    """20 columns in batches of 3 (seven, the last of two) and of 8 (8, 8, 4): odd batch starts, partials sized by the
    first and the last batch; on a graph without tiles and on one with."""
    elt = np.dtype(dtype).itemsize
    W, L, lmax = small(257)
    C = bank_coefficients(9, 12, seed=20)
    x = rounded(np.random.default_rng(20).standard_normal((257, 20)), dtype)
    ref = oracle_sqnorms(L, lmax, C, x)
    batches = len(list(batch_columns(20, max_batch)))
    assert batches == {3: 7, 8: 3}[max_batch]
    with options(ctx, max_batch=max_batch):
        s, kinds = sqnorms(device(ctx, 257, dtype), C, x, lmax)
    assert kinds == {"tile": 0, "plain": 11 * batches}, kinds
    hold("column batches", dtype, s, ref, TOL[np.dtype(dtype)], (257, max_batch))
    one, _ = sqnorms(device(ctx, 257, dtype), C, x, lmax)
    assert rel_err(s, one) < TOL[np.dtype(dtype)]
    c, Ct, tref = tile_case("rand65")
    dev = tile_helpers.device_graph(ctx, "rand65", dtype, "device", no_polynomials)
    with options(ctx, max_batch=max_batch):
        s, kinds = sqnorms(dev, Ct, tile_helpers.columns(c, 20), c["lmax"])
    want = expected_kinds_recurrence(20, elt, 9, 11, combine=2, max_batch=max_batch)
    assert want == sqnorm_kinds(20, elt, 11, max_batch=max_batch) == {"tile": 11 * batches, "plain": 0}
    assert kinds == want, (max_batch, kinds, want)
    hold("column batches on tiles", dtype, s, tref[:, :20], TOL[np.dtype(dtype)], ("rand65", max_batch))
