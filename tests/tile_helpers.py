"""What the modules that pin k_step_tile at small shapes share (tests/test_gpu_o_programs_on_tiles.py: polynomial
programs; tests/test_gpu_p_recurrence_on_tiles.py: the recurrence, filter banks and synthesis; the squared norms and
L x of tests/test_gpu_u_sqnorms_small.py and tests/test_gpu_u_lx_on_tiles.py use them too): one cached case per
graph, cached device graphs with gather tiles from both builders, option scopes, the comparison with the oracle that
keeps the worst figures, and the restated rules of which launches take the tile kernel."""
import contextlib

import numpy as np
from scipy import sparse

from conftest import rel_err
from gpu_helpers import DEFAULT_OPTIONS, TOL, upper_lmax
from oracle import cheby_oracle as orc
from program_helpers import random_case
from pygsp_amd import engine, graphs
from recurrence_helpers import band_weights, shuffled

F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
DTYPES = [np.float64, np.float32]
# one row size (bytes) per tile build: 1-lane, 2-lane, 4-lane regrouped to 3 pieces, 4-lane, 8-lane regrouped to 5,
# 8-lane, 16-lane regrouped to 10, NCOL = 1, NCOL = 2 twice, NCOL = 0 twice: float64 widths 2 ... 96, float32 4 ... 192
ROW_BYTES = [16, 32, 48, 64, 80, 128, 160, 256, 272, 512, 528, 768]
OFF_PIECE = {F64: [1, 3, 5, 33], F32: [1, 2, 6, 66]}
# (sensor4097+hub: the sensor graph with a hub of 300 neighbours added - staged blocks and the hub's plain-gather block
# in one launch; the random graphs have no locality, so nearly all of their blocks gather from global memory)
GRAPHS = ["sensor4097", "sensor4097+hub", "hub3001", "hub3001-normalized", "rand577", "rand65"]
# (a ring whose every block is staged - what a fused input needs -, in its natural order without an internal order and
# relabelled at random with the internal order that restores the band)
BAND_GRAPHS = ["band4097", "band4097-shuffled"]
BLOCKS = {"sensor4097": 65, "sensor4097+hub": 65, "hub3001": 47, "hub3001-normalized": 47, "rand577": 10, "rand65": 2,
          "band4097": 65, "band4097-shuffled": 65}
MAXW = 192
OPTIONS = dict(DEFAULT_OPTIONS, tile_regroup=1, tile_lg=0, tile_pad=1, tile_min_row=16)

_GRAPHS, _CASES, _DEVS, _WORST = {}, {}, {}, {}


def graph_matrix(name):
    """(W, Laplacian type, L, an upper bound of the spectrum, coordinates or None, a given internal order or None) of
    one of GRAPHS + BAND_GRAPHS.  Host only."""
    if name in _GRAPHS:
        return _GRAPHS[name]
    coords = order = None
    if name.startswith("sensor4097"):
        W, coords = graphs.sensor_weights(4097, k=8, seed=31)
        if name.endswith("+hub"):
            rng = np.random.default_rng(32)
            to = rng.choice(4096, size=300, replace=False) + 1
            A = sparse.coo_matrix((rng.uniform(0.1, 1.0, 300), (np.zeros(300, dtype=np.int64), to)), shape=W.shape)
            W = sparse.csr_matrix(W + A + A.T)
            W.sum_duplicates()
            W.sort_indices()
        lap = "combinatorial"
        L, lmax = orc.laplacian(W), upper_lmax(W)
    elif name.startswith("band4097"):
        W = band_weights(4097, 4)
        if name.endswith("-shuffled"):
            W, order = shuffled(W)
        lap = "combinatorial"
        L, lmax = orc.laplacian(W), upper_lmax(W)
    else:
        lap = "normalized" if name.endswith("-normalized") else "combinatorial"
        W, L, lmax = random_case(name.split("-")[0], lap)
    _GRAPHS[name] = (W, lap, L, lmax, coords, order)
    return _GRAPHS[name]


def case(name, polynomials):
    """The graph, its Laplacian, an upper bound of its spectrum, 192 signals whose values are exact in both compute
    dtypes (one oracle call per polynomial serves every test) and the oracle's result for every polynomial of
    `polynomials(lmax)` (name -> coefficients)."""
    key = (name, polynomials)
    if key in _CASES:
        return _CASES[key]
    W, lap, L, lmax, coords, order = graph_matrix(name)
    if name.startswith("band4097"):
        perm = order  # (the natural order of the ring is the band: no internal order at all)
    else:
        perm = engine.locality_order(W, coords)
    n = W.shape[0]
    seed = (GRAPHS + BAND_GRAPHS).index(name)
    x = np.random.default_rng(seed).standard_normal((n, MAXW)).astype(np.float32).astype(np.float64)
    polys = polynomials(lmax)
    ref = {k: orc.cheby_op(L, lmax, c, x) for k, c in polys.items()}
    for r in ref.values():
        r.setflags(write=False)
    _CASES[key] = dict(W=W, lap=lap, L=L, lmax=lmax, perm=perm, n=n, x=x, polys=polys, ref=ref)
    return _CASES[key]


def device_graph(ctx, name, dtype, builder, polynomials):
    """The case's graph on the device in its locality order with gather tiles: built in numpy and uploaded
    (enable_gather_tiles) and built on the device (build_gather_tiles) - the two must agree -, `builder`'s left on."""
    key = (name, np.dtype(dtype), builder)
    if key in _DEVS:
        return _DEVS[key]
    c = case(name, polynomials)
    dev = engine.DeviceGraph.from_w(c["W"], c["lap"], dtype=dtype, perm=c["perm"], ctx=ctx)
    host = dev.enable_gather_tiles()
    device = dev.build_gather_tiles()
    assert host["nb"] == device["nb"] == BLOCKS[name], (host, device)
    assert host["slow_blocks"] == device["slow_blocks"] and host["lds_bytes"] == device["lds_bytes"], (host, device)
    if host["slow_blocks"] == 0:  # (the device build sums the gather sets of the staged blocks only)
        assert abs(host["mean_n1"] - device["mean_n1"]) < 1e-9, (host, device)
    if name.startswith("sensor4097"):
        assert host["slow_blocks"] * 20 < host["nb"], host
    if "hub" in name:  # the hub's block takes the plain-gather branch inside the tile kernel
        assert host["slow_blocks"] >= 1, host
    if name.startswith("band4097"):  # every block staged: a single filter's input can be fused
        assert host["slow_blocks"] == 0 and host["nb"] == 65, host
    if builder == "host":
        dev.enable_gather_tiles()
    print("{} {} tiles: {}".format(name, np.dtype(dtype).name, host))
    _DEVS[key] = dev
    return dev


def finish():
    """After a module: the device's worst deviation per test and dtype; the device graphs and the cases go."""
    for (test, dt), (err, where) in sorted(_WORST.items()):
        print("\nworst {:<34s} {:<8s} {:.2e} of max |ref| at {}".format(test, dt, err, where), end="")
    print()
    _WORST.clear()
    while _DEVS:
        _DEVS.popitem()[1].destroy()
    _CASES.clear()


@contextlib.contextmanager
def options(ctx, base=OPTIONS, **kw):
    """The options kw for the block, then back to their values in `base`."""
    try:
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in kw:
            ctx.set_option(k, base[k])


def columns(c, w):
    return np.ascontiguousarray(c["x"][:, :w])


def hold(test, dtype, y, ref, where):
    """y against the oracle, every column, at the bar; keeps the worst figure for the report."""
    assert y.shape == ref.shape and np.all(np.isfinite(y)), where
    err = rel_err(y.astype(np.float64), ref)
    key = (test, np.dtype(dtype).name)
    if err >= _WORST.get(key, (-1.0, None))[0]:
        _WORST[key] = (err, where)
    assert err < TOL[np.dtype(dtype)] * 10, (where, err)


def batch_columns(nsig, max_batch):
    """batch_width of gspx_poly.hip.h for graphs this small: column batches of max_batch signals, a multiple of 4 when
    there are several and max_batch >= 4.  Yields (first column, columns) of every batch."""
    width = nsig if max_batch <= 0 else min(max_batch, nsig)
    if width < nsig and width >= 4:
        width &= ~3
    for c0 in range(0, nsig, width):
        yield c0, min(width, nsig - c0)


def expected_kinds(nsig, elt, max_batch, S, tile_min_row=16):
    """The rule of gspx_poly.hip.h for a program restated: column batches of max_batch signals (a multiple of 4 when
    there are several and max_batch >= 4); a batch of ld columns starting at column c0 takes the tile kernel iff its
    rows and the rows of y are whole 16-byte pieces, its rows have at least tile_min_row bytes and y + c0 is 16-byte
    aligned (the buffers themselves are)."""
    kinds = {"tile": 0, "plain": 0}
    for c0, ld in batch_columns(nsig, max_batch):
        tile = ((ld * elt) % 16 == 0 and (nsig * elt) % 16 == 0 and ld * elt >= tile_min_row and (c0 * elt) % 16 == 0)
        kinds["tile" if tile else "plain"] += S
    return kinds


def expected_kinds_lx(nsig, elt, max_batch=0, fuse_input=1, tile_gather=1, tiles=True, slow_blocks=0, x_offset=0,
                      in_place=False, tile_min_row=16):
    """The rule of gspx_ops.hip.h for y = L x (lap_apply_t) restated, for nsig signals of elt bytes; one launch per
    batch, counted like a filter's steps.
    - Fused: ONE tile launch that gathers from the caller's panel, iff the panel fits one batch (ops_max_ld: max_batch
      columns, a multiple of 4 from 4 on), fuse_input is on, every block of the graph is staged (slow_blocks = 0), x is
      16-byte aligned (x_offset: bytes of x into its aligned buffer), x and y do not overlap, and the tile kernel can
      take the whole panel: rows of whole 16-byte pieces of at least tile_min_row bytes (y's buffer is aligned).
    - Else column batches through the workspace: a batch of ld columns starting at c0 takes the tile kernel iff its
      rows and the rows of y are whole 16-byte pieces, its rows have at least tile_min_row bytes and y + c0 is 16-byte
      aligned - expected_kinds' rule with one step -, else the plain kernel.
    (The 2 GiB windows and the workspace budget bind on no graph this small.)"""
    tvec = 16 // elt
    on = tiles and bool(tile_gather)

    def usable(ld, c0):
        return on and ld * elt >= tile_min_row and ld % tvec == 0 and nsig % tvec == 0 and (c0 * elt) % 16 == 0

    width = max_batch if max_batch > 0 else 1 << 30
    if width >= 4:
        width &= ~3
    if (nsig <= width and fuse_input and slow_blocks == 0 and x_offset % 16 == 0 and not in_place
            and usable(nsig, 0)):
        return {"tile": 1, "plain": 0}
    kinds = {"tile": 0, "plain": 0}
    for c0 in range(0, nsig, width):
        kinds["tile" if usable(min(width, nsig - c0), c0) else "plain"] += 1
    return kinds


def expected_kinds_recurrence(nsig, elt, nf, K, mode="analysis", max_batch=0, combine=0, synthesis=0, tile_gather=1,
                              tile_pad=1, tile_min_row=16, y_offset=0, tiles=True, big_matrix=False):
    """The rule of gspx_poly.hip.h for a recurrence call (filter_dev_t, work_panels) restated, for nf filters of K
    steps on nsig signals of elt bytes.

    Steps per column batch: K for an analysis (fused flush or deferred combine alike), K + 1 for a synthesis by the
    Clenshaw recurrence (synthesis = 0), nf K for the per-filter loop (synthesis = 1).  An analysis of two and more
    filters keeps every T_k and combines afterwards (deferred) with combine = 0 or 2; with combine = 1 it flushes inside
    the steps, which only the plain kernels do for several filters.  A batch of ld columns whose first is c0 runs
    - direct on the tile kernels iff its rows and the rows of y are whole 16-byte pieces of at least tile_min_row bytes
      and y + c0 is 16-byte aligned (y_offset: bytes of y into its aligned buffer),
    - else on the tile kernels with rows padded up to whole pieces iff tile_pad is on, the padded rows have tile_min_row
      bytes, and padding pays: tile_pad = 2, two columns or more, or a matrix of 20 MB and more (big_matrix),
    - else on the plain kernels.
    (The 2 GiB windows and the workspace budget of the library's rule bind on no graph this small.)"""
    tvec = 16 // elt
    analysis = mode == "analysis"
    deferred = analysis and (combine == 2 or (combine == 0 and nf >= 2))
    allowed = tiles and bool(tile_gather) and (not analysis or deferred or nf == 1)
    per_batch = K if analysis else (nf * K if synthesis == 1 else K + 1)

    def geometry(ld):
        return ld * elt >= tile_min_row and ld % tvec == 0

    kinds = {"tile": 0, "plain": 0}
    for c0, ld in batch_columns(nsig, max_batch):
        direct = allowed and geometry(ld) and nsig % tvec == 0 and (y_offset + c0 * elt) % 16 == 0
        ldp = (ld + tvec - 1) // tvec * tvec
        pad_pays = tile_pad == 2 or ld >= 2 or big_matrix
        padded = not direct and allowed and bool(tile_pad) and pad_pays and geometry(ldp)
        kinds["tile" if direct or padded else "plain"] += per_batch
    return kinds
