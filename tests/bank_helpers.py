"""What the wide-bank tests share (tests/test_bank_host.py, tests/test_gpu_t_wide_banks.py): filter banks of 7 to 40
filters that do not depend on the graph, one cached case per (graph, bank) with 48 signal columns and the oracle's
analysis, synthesis inputs of up to 40 panels whose every panel keeps a weight of at least 1/2, and the comparison
with the oracle that holds every filter plane on its own.  numpy, scipy and the oracle only: nothing of the library
takes part in what this module computes."""
import numpy as np

import tile_helpers
from gpu_helpers import TOL
from oracle import cheby_oracle as orc

GRAPHS = ["rand65", "hub3001", "sensor4097"]
NCOL = 48
ROTATE = 5
WEIGHTS = 2  # panel f of a synthesis weighs 2^-(f mod WEIGHTS)
# (filters, order) of every bank the GPU module runs: order 12 is K = 12 recurrence steps, order 30 K = 30
BANKS = [(7, 12), (8, 12), (9, 12), (16, 12), (17, 12), (33, 12), (40, 30)]

_CASES, _WORST = {}, {}


def bank(nf, order):
    """(nf, order + 1) Chebyshev coefficients: normal draws that decay like 0.75^k, every row of unit absolute sum -
    every filter differs from every other in every coefficient, and every |p_f| <= 1 on the spectrum."""
    c = np.random.default_rng(7 + nf).standard_normal((nf, order + 1)) * 0.75 ** np.arange(order + 1)
    return c / np.abs(c).sum(axis=1, keepdims=True)


def NO_POLYNOMIALS(lmax):
    """For tile_helpers.device_graph: the device graphs of this module's cases carry no polynomial of their own."""
    return {}


def signals(name):
    """(N, 48) signals of graph `name` whose values are exact in both compute dtypes."""
    n = tile_helpers.graph_matrix(name)[0].shape[0]
    seed = tile_helpers.GRAPHS.index(name)
    x = np.random.default_rng(seed).standard_normal((n, tile_helpers.MAXW))[:, :NCOL]
    return np.ascontiguousarray(x.astype(np.float32).astype(np.float64))


def case(name, nf, order):
    """The graph's Laplacian, an upper bound of its spectrum, the 48 signals, the bank and the oracle's analysis of all
    48 columns, (nf, N, 48) in float64, computed once."""
    key = (name, nf, order)
    if key not in _CASES:
        W, lap, L, lmax, _, _ = tile_helpers.graph_matrix(name)
        n = W.shape[0]
        x = signals(name)
        c = bank(nf, order)
        ana = orc.cheby_op(L, lmax, c, x).reshape(nf, n, NCOL)
        for a in (x, c, ana):
            a.setflags(write=False)
        _CASES[key] = dict(W=W, lap=lap, L=L, lmax=lmax, n=n, x=x, coeffs=c, ana=ana, K=order)
    return _CASES[key]


def wide_synthesis_inputs(x, nf):
    """(nf, N, 48) input panels of a synthesis: panel f holds 2^-(f mod 2) times x's columns rotated by 5 f (5 and 48
    are coprime: no two panels of a bank of up to 48 are rotated alike), so every value stays exact in float32 and no
    panel weighs less than 1/2.  The weights were first 2^-(f mod 4), 1/8 the least: of 33 panels summed on hub3001
    the lightest then moved the result by 64 float32 bars only (2^-(f mod 3): 99.9 on sensor4097), short of the 100
    that tests/test_bank_host.py asks of every dropped panel; with two weights the least is 154."""
    return np.stack([np.ldexp(np.roll(x, -ROTATE * f, axis=1), -(f % WEIGHTS)) for f in range(nf)])


def wide_synthesis_reference(analysis, drop=()):
    """The oracle's synthesis of wide_synthesis_inputs(x, nf) from its analysis of x, (nf, N, 48): the filters act on
    every column alone, so  sum_f p_f(L) s_f  is the same sum over the rotated, scaled columns of p_f(L) x.  `drop`:
    panels left out of the sum (the sensitivity checks)."""
    return sum(np.ldexp(np.roll(a, -ROTATE * f, axis=1), -(f % WEIGHTS))
               for f, a in enumerate(analysis) if f not in drop)


def synthesis_case(name, nf, order):
    """case() with the synthesis inputs (c["s"], (nf, N, 48)) and their reference (c["syn"], (N, 48)) on top."""
    c = case(name, nf, order)
    if "s" not in c:
        c["s"] = wide_synthesis_inputs(c["x"], nf)
        c["syn"] = wide_synthesis_reference(c["ana"])
        c["s"].setflags(write=False)
        c["syn"].setflags(write=False)
    return c


def plane_errors(y, ref):
    """max |y_f - ref_f| / max |ref_f| of every filter plane f of (nf, N, w) arrays."""
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert y.shape == ref.shape and y.ndim == 3, (y.shape, ref.shape)
    scale = np.abs(ref).max(axis=(1, 2))
    assert np.all(scale > 0)
    return np.abs(y - ref).max(axis=(1, 2)) / scale


def hold_per_filter(test, dtype, y, ref, where, inside=1.0):
    """y (nf, N, w) - or one plane (N, w) - against the oracle: every filter plane on its own under the bar
    gpu_helpers.TOL * 10 (divided by `inside`), relative to that plane's own max |reference|; keeps the worst figure
    for the report.  Returns the worst figure of this call."""
    dt = np.dtype(dtype)
    if np.ndim(ref) == 2:
        y, ref = np.asarray(y)[None], np.asarray(ref)[None]
    assert y.shape == ref.shape and np.all(np.isfinite(y)), (where, y.shape, ref.shape)
    errs = plane_errors(y, ref)
    f = int(np.argmax(errs))
    record(test, dt, errs[f], (where, "filter %d of %d" % (f, len(errs))))
    bad = np.flatnonzero(~(errs < TOL[dt] * 10 / inside))
    assert bad.size == 0, (where, "filters", bad.tolist(), errs[bad].tolist())
    return float(errs[f])


def record(test, dtype, err, where, metric="of the plane's max |ref|"):
    """Keeps the worst figure of `test` and dtype for the report.  A test that holds its figures under a bar of its own
    names their metric."""
    key = (test, np.dtype(dtype).name)
    if err >= _WORST.get(key, (-1.0, None, None))[0]:
        _WORST[key] = (float(err), where, metric)


def report():
    """After a module: the worst per-filter deviation per test and dtype; the cases go."""
    for (test, dt), (err, where, metric) in sorted(_WORST.items()):
        print("\nworst {:<40s} {:<8s} {:.2e} {} at {}".format(test, dt, err, metric, where), end="")
    print()
    _WORST.clear()
    _CASES.clear()


# ---- the rule of the column batches -------------------------------------------------------------------------------
def batch_width(n, elt, panels, nsig, max_batch=0, ws_limit_mb=65536):
    """batch_width of gspx_poly.hip.h restated: the signals per column batch of a device call on n vertices of elt
    bytes - below the 2 GiB buffer window, within the workspace budget of `panels` work columns per signal (M for a
    deferred call, 2 + Nf for a fused one), at most max_batch, and a multiple of 4 when the call has several batches
    of 4 and more."""
    rowb = n * elt
    width = ((1 << 31) - 65536) // rowb
    assert width >= 1
    budget = max(ws_limit_mb, 1) << 20
    width = min(width, max(1, budget // (rowb * panels)))
    if max_batch > 0:
        width = min(width, max_batch)
    if width < nsig and width >= 4:
        width &= ~3
    return width


def batches(n, elt, panels, nsig, **kw):
    """The column counts of the batches of such a call."""
    width = batch_width(n, elt, panels, nsig, **kw)
    return [min(width, nsig - c0) for c0 in range(0, nsig, width)]


def plain_kernel(ld, elt, kernel=0):
    """choose_shape of gspx_poly.hip.h restated: which plain step kernel a batch of ld columns of elt bytes runs under
    the option `kernel` - "narrow" (k_step_narrow), "panel" (k_step_panel) or "lds" (k_step_lds)."""
    name = "narrow" if ld <= 4 else "panel"
    if kernel == 2 and ld <= 64:
        name = "narrow"
    if kernel == 1 and ld > 4:
        name = "panel"
    if kernel == 5 and ld > 4:
        name = "lds"
    if kernel == 0 and name == "panel" and (elt == 4 or ld <= 32):
        name = "lds"
    return name


def combine_vec(ld, elt, padded, vec=0):
    """The lane vector of the deferred combine (k_combine<T, VEC>) of a batch of ld columns into rows of y that are
    aligned for it: 1 on padded work panels, else choose_shape's - the widest of 16 bytes that divides ld and leaves 16
    lanes per row, or the option `vec` where it divides ld; up to 4 columns the call is shaped for the narrow kernel,
    which has no lane vector."""
    if padded or ld <= 4:
        return 1
    maxvec = 16 // elt
    v = next(v for v in (4, 2, 1) if v <= maxvec and ld % v == 0)
    while v > 1 and ld // v < 16:
        v //= 2
    if vec and vec <= maxvec and ld % vec == 0:
        v = vec
    return v
