"""Lanczos filtering without a device: the driver of pygsp_amd.lanczos on the numpy backend of
tests/lanczos_helpers.py against the reference's fixtures and dense filtering, the argument checks of
filters.lanczos_op and of the C-ABI entry points, and the opt-in plugin seam."""
import ctypes
import os
import types

import numpy as np
import pytest

from lanczos_helpers import (complete, csr_from, exact_filter, host_filter, laplacian, rel_err, ring, run_numpy, star,
                             upper_bound)
from pygsp_amd import _capi, filters, lanczos, plugin

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", ["sensor123", "logo"])
@pytest.mark.parametrize("lap_type", ["combinatorial", "normalized"])
def test_driver_matches_reference_fixtures(name, lap_type):
    g = np.load(os.path.join(GOLDEN, "lanczos_{}.npz".format(name)))
    W = csr_from(g, "W")
    L, b = laplacian(W, lap_type), upper_bound(W, lap_type)
    for kind, key in (("heat10", "heat10"), ("mexicanhat", "mexicanhat6"), ("heat50", "heat50")):
        f = host_filter(kind, g["lmax_" + lap_type])
        k = "{}_{}".format(lap_type, key)
        order = int(g[k + "_order"])
        y1, _, _ = run_numpy(L, f, g["x1"], order, b)
        y5, _, _ = run_numpy(L, f, g["x5"], order, b)
        assert rel_err(y1, g[k + "_y1"]) <= 1e-11, k
        assert rel_err(y5, g[k + "_y5"]) <= 1e-11, k


@pytest.mark.parametrize("nf", [1, 6])
def test_shapes_and_filter_major_rows(nf):
    W = ring(50)
    L, b = laplacian(W, "combinatorial"), upper_bound(W, "combinatorial")
    f = host_filter("heat10" if nf == 1 else "mexicanhat", 4.0)
    x = np.random.default_rng(0).standard_normal((50, 3))
    y2, _, _ = run_numpy(L, f, x, 40, b)
    y1, _, _ = run_numpy(L, f, x[:, 1], 40, b)
    assert y2.shape == (50 * nf, 3) and y1.shape == (50 * nf,)
    assert rel_err(y1, y2[:, 1]) <= 1e-13  # (eigh of one H alone or in a batch: the last bits may differ)
    exact = exact_filter(L, f, x)
    for i in range(nf):  # row i N + n: filter i at vertex n
        assert rel_err(y2[i * 50:(i + 1) * 50], exact[i * 50:(i + 1) * 50]) <= 1e-12


@pytest.mark.parametrize("W,x,expected", [
    (ring(64), np.random.default_rng(0).standard_normal(64), 33),
    (complete(64), np.random.default_rng(1).standard_normal(64), 2),
    (star(30), np.random.default_rng(2).standard_normal(30), 3),
    (ring(64), np.ones(64), 1),
])
def test_breakdown_stops_at_the_touched_eigenvalues(W, x, expected):
    L, b = laplacian(W, "combinatorial"), upper_bound(W, "combinatorial")
    f = host_filter("mexicanhat", np.linalg.eigvalsh(L.toarray())[-1])
    y, _, stats = run_numpy(L, f, x, 60, b)
    assert stats["steps"][0] == expected
    assert rel_err(y, exact_filter(L, f, x)) <= 1e-12


def test_order_one_is_f_of_alpha0_times_x():
    W = ring(30)
    L, b = laplacian(W, "combinatorial"), upper_bound(W, "combinatorial")
    f = host_filter("mexicanhat", 4.0)
    x = np.random.default_rng(3).standard_normal(30)
    y, _, _ = run_numpy(L, f, x, 1, b)
    a0 = max(x @ (L @ x) / (x @ x), 0.0)
    expected = np.concatenate([fe * x for fe in f.evaluate(np.array([a0]))[:, 0]])
    np.testing.assert_allclose(y, expected, rtol=1e-13, atol=1e-15)


def test_zero_column_gives_zeros_and_batches_split_columns():
    W = ring(40)
    L, b = laplacian(W, "combinatorial"), upper_bound(W, "combinatorial")
    f = host_filter("heat10", 4.0)
    x = np.random.default_rng(4).standard_normal((40, 7))
    x[:, 2] = 0
    y, be, stats = run_numpy(L, f, x, 20, b, width=3)
    assert np.all(y[:, 2] == 0) and stats["steps"][2] == 0 and np.isfinite(y).all()
    assert be.batches == [(0, 3), (3, 6), (6, 7)]
    whole, _, _ = run_numpy(L, f, x, 20, b)
    assert rel_err(y, whole) <= 1e-13


def test_evaluate_is_called_once_per_batch():
    W = ring(40)
    L, b = laplacian(W, "combinatorial"), upper_bound(W, "combinatorial")
    calls = []
    inner = host_filter("mexicanhat", 4.0)
    f = types.SimpleNamespace(Nf=6, evaluate=lambda e: (calls.append(np.shape(e)), inner.evaluate(e))[1])
    x = np.random.default_rng(5).standard_normal((40, 5))
    run_numpy(L, f, x, 12, b)
    assert len(calls) == 1 and calls[0] == (5 * 12,)


def test_batch_width_rule():
    assert lanczos.max_batch_width(1000, 30, 65536) == 256
    assert lanczos.max_batch_width(1_000_000, 100, 65536) == 80  # 64 GiB / (103 panels x 8 MB), multiple of 4
    assert lanczos.max_batch_width(1_000_000, 30, 1) == 1
    assert lanczos.max_batch_width(1000, 30, 65536, max_batch=7) == 4
    assert lanczos.max_batch_width(300_000_000, 2, 65536) == 1  # one column over 2 GiB: refused by the library


def test_lanczos_op_argument_errors():
    G = types.SimpleNamespace(N=10, lmax=2.0)
    f = filters.Heat(G, scale=10)
    with pytest.raises(ValueError):
        filters.lanczos_op(f, np.zeros(10), order=0)
    with pytest.raises(TypeError):
        filters.lanczos_op(f, np.zeros(10, dtype=complex))
    with pytest.raises(ValueError):
        filters.lanczos_op(f, np.zeros(9))
    with pytest.raises(ValueError):
        filters.lanczos_op(f, np.zeros((10, 2, 2)))
    with pytest.raises(ValueError):
        filters.lanczos_op(f, np.zeros(()))


def test_filter_method_lanczos_still_refused():
    G = types.SimpleNamespace(N=10, lmax=2.0, _check_signal=lambda s: np.asarray(s))
    f = filters.Heat(G, scale=10)
    with pytest.raises(ValueError):
        f.filter(np.zeros(10), method="lanczos")
    with pytest.raises(NotImplementedError):
        f.filter(np.zeros(10), method="exact")


def _standin():
    """A pygsp-shaped module: filters (with approximations, cheby_op, lanczos_op and the aliases), graphs.Graph."""
    approx = types.ModuleType("approximations")
    approx.cheby_op = lambda *a, **k: "ref cheby"
    approx.lanczos_op = lambda *a, **k: "ref lanczos"
    approx.compute_cheby_coeff = lambda *a, **k: None
    fmod = types.ModuleType("filters")
    fmod.approximations = approx
    fmod.cheby_op, fmod.lanczos_op = approx.cheby_op, approx.lanczos_op

    class Filter:
        def filter(self, *a, **k):
            return "ref filter"

        def compute_frame(self, *a, **k):
            return "ref frame"

    fmod.Filter = Filter
    gmod = types.ModuleType("graphs")

    class Graph:
        def estimate_lmax(self, method="lanczos"):
            return None

        def compute_fourier_basis(self, n_eigenvectors=None):
            return None

    gmod.Graph = Graph
    mod = types.ModuleType("pygsp")
    mod.filters, mod.graphs = fmod, gmod
    return mod


def test_plugin_lanczos_seam_is_opt_in():
    mod = _standin()
    ref_op = mod.filters.approximations.lanczos_op
    try:
        plugin.install(mod)
        assert mod.filters.approximations.lanczos_op is ref_op and mod.filters.lanczos_op is ref_op
        plugin.install(mod, lanczos=True)
        assert mod.filters.approximations.lanczos_op is filters.lanczos_op
        assert mod.filters.lanczos_op is filters.lanczos_op
        plugin.install(mod, lanczos=False)  # asked for no more: restored
        assert mod.filters.approximations.lanczos_op is ref_op and mod.filters.lanczos_op is ref_op
        plugin.install(mod, lanczos=True)
    finally:
        plugin.uninstall(mod)
    assert mod.filters.approximations.lanczos_op is ref_op and mod.filters.lanczos_op is ref_op
    assert mod.filters.approximations.cheby_op() == "ref cheby"


def test_lanczos_entry_points_refuse_bad_arguments_without_a_device():
    lib = _capi.load()
    a = np.zeros((4, 4))
    s = np.zeros(4, dtype=np.int32)
    w = np.zeros((2, 4, 4))
    fake = ctypes.c_void_p(1 << 20)  # a non-null address: never dereferenced, the checks fail first

    def refused(rc, words):
        with pytest.raises(ValueError):
            _capi.check(rc)
        assert words in _capi.last_error(), _capi.last_error()

    kry, comb = lib.gspx_lanczos_krylov_dev, lib.gspx_lanczos_combine_dev
    P = _capi.ptr
    refused(kry(None, 4, 4, fake, 4, 0.0, fake, P(a), P(a), P(a), P(s), None, None), "null graph")
    refused(kry(None, 0, 4, fake, 4, 0.0, fake, P(a), P(a), P(a), P(s), None, None), "order")
    refused(kry(None, 4, -1, fake, 4, 0.0, fake, P(a), P(a), P(a), P(s), None, None), "number of signals")
    refused(kry(None, 4, 257, fake, 300, 0.0, fake, P(a), P(a), P(a), P(s), None, None), "number of signals")
    refused(kry(None, 4, 4, fake, 3, 0.0, fake, P(a), P(a), P(a), P(s), None, None), "leading dimension")
    refused(kry(None, 4, 4, fake, 4, -1.0, fake, P(a), P(a), P(a), P(s), None, None), "breakdown")
    refused(kry(None, 4, 4, fake, 4, float("nan"), fake, P(a), P(a), P(a), P(s), None, None), "breakdown")
    refused(kry(None, 4, 4, fake, 4, 0.0, fake, None, P(a), P(a), P(s), None, None), "null host output")
    refused(kry(None, 4, 4, fake, 4, 0.0, fake, P(a), P(a), P(a), None, None, None), "null host output")
    refused(comb(None, 4, 4, fake, 2, P(w), fake, 4, None), "null graph")
    refused(comb(None, 0, 4, fake, 2, P(w), fake, 4, None), "order")
    refused(comb(None, 4, -1, fake, 2, P(w), fake, 4, None), "number of signals")
    refused(comb(None, 4, 4, fake, 0, P(w), fake, 4, None), "Nf")
    refused(comb(None, 4, 4, fake, 2, P(w), fake, 3, None), "leading dimension")
    refused(comb(None, 4, 4, fake, 2, None, fake, 4, None), "null weights")
