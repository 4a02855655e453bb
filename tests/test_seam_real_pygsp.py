"""The drop-in seam checked against what the real reference computed, with nothing
from outside the repository: `pygsp_amd.plugin.install()` is applied to a pygsp-shaped stand-in - a module with the
names install() patches (`filters.approximations.cheby_op`, the alias `filters.cheby_op`, `filters.Filter.filter` /
`compute_frame`, `graphs.Graph.estimate_lmax`), whose own code is written here on the oracle - and the device object
is replaced by an oracle-backed one (no GPU in the build container).  What runs is the product's host side of the
seam: the `c` contract, the shape rules of analysis and synthesis, synthesis as one call, the frame by panels, and
the originals put back.  The results are compared with the outputs the real pygsp gave for the fixtures of its own
`pygsp/tests/test_filters.py` and for the doctest of `Filter.filter` (tests/golden/, gen_golden.py).  The real
pygsp itself runs through the seam on the device in tests/test_gpu_b_real_pygsp.py wherever one is importable."""
import types

import numpy as np
import pytest
from conftest import csr_from, load_golden, rel_err

from oracle import cheby_oracle as orc
from pygsp_amd import filters as product_filters
from pygsp_amd import plugin

TOL = 1e-12


class OracleDevice:
    """Stands in for engine.DeviceGraph: the call contract of cheby_filter, arithmetic by the oracle."""

    def __init__(self, G, calls):
        self.L, self.N, self.dtype, self.calls = G.L, G.N, np.dtype(np.float64), calls

    def cheby_filter(self, coeffs, x, lmax, mode=0):
        c = np.atleast_2d(np.asarray(coeffs, dtype=np.float64))
        x = np.ascontiguousarray(x, dtype=np.float64)
        self.calls["cheby_op"] += 1
        self.calls["synthesis_device_calls"] += int(mode == 1)
        if mode == 0:
            return orc.cheby_op(self.L, lmax, c, x).reshape(c.shape[0], self.N, -1), 0.0
        return sum(orc.cheby_op(self.L, lmax, c[f], x[f]) for f in range(c.shape[0])), 0.0


def bounds_lmax(W, dw):
    """The smallest of the four classical upper bounds of lambda_max of a combinatorial Laplacian."""
    ends = W.tocoo()
    with np.errstate(divide="ignore", invalid="ignore"):
        return min(W.shape[0] * W.max(), 2 * dw.max(), (dw[ends.row] + dw[ends.col]).max(),
                   np.max(dw + W.dot(dw) / dw))


def standin_pygsp():
    """A fresh pygsp-shaped module whose originals compute with the oracle (per-filter loops, dense identity)."""
    calls = {"original_cheby_op": 0, "original_filter": 0, "original_frame": 0, "original_lmax": 0,
             "cheby_op": 0, "synthesis_device_calls": 0, "synthesis_filters": 0, "device_graphs": 0}

    class Graph:
        def __init__(self, W, lmax=None):
            self.W, self.N, self.lap_type = W, W.shape[0], "combinatorial"
            self.L = orc.laplacian(W)
            self.dw = np.ravel(np.asarray(W.sum(axis=1), dtype=np.float64))
            self._lmax, self._lmax_method = lmax, None if lmax is None else "fourier"

        @property
        def lmax(self):
            return self._lmax

        def is_directed(self):
            return False

        def _check_signal(self, s):
            s = np.asanyarray(s)
            if s.shape[0] != self.N:
                raise ValueError("First dimension must be the number of vertices G.N = {}, got {}.".format(self.N,
                                                                                                          s.shape))
            return s

        def estimate_lmax(self, method="lanczos"):
            calls["original_lmax"] += 1
            if method != "bounds":
                raise NotImplementedError(method)
            self._lmax, self._lmax_method = bounds_lmax(self.W, self.dw), method

    def cheby_op(G, c, s, **kwargs):
        calls["original_cheby_op"] += 1
        return orc.cheby_op(G.L, G.lmax, c, s)

    def compute_cheby_coeff(f, m=30, N=None, **kwargs):
        return np.array([orc.compute_cheby_coeff(k, f.G.lmax, m, N) for k in f._kernels])

    class Filter:
        def __init__(self, G, kernels):
            self.G, self._kernels, self.Nf = G, list(kernels), len(kernels)

        def filter(self, s, method="chebyshev", order=30):
            calls["original_filter"] += 1
            c = approximations.compute_cheby_coeff(self, m=order)
            s = np.asarray(s, dtype=np.float64)
            if self.Nf > 1 and s.ndim >= 2 and s.shape[-1] == self.Nf:  # synthesis: one call per filter
                return sum(approximations.cheby_op(self.G, c[f], s[..., f]) for f in range(self.Nf))
            x = s.reshape(self.G.N, -1)
            y = approximations.cheby_op(self.G, c, x).reshape(self.Nf, self.G.N, x.shape[1]).transpose(1, 2, 0)
            if s.ndim == 1:
                y = y[:, 0, :]
            return y[..., 0] if self.Nf == 1 else y

        def compute_frame(self, method="chebyshev", order=30):
            calls["original_frame"] += 1
            c = approximations.compute_cheby_coeff(self, m=order)
            return approximations.cheby_op(self.G, c, np.identity(self.G.N))

    mod = types.ModuleType("pygsp")
    mod.graphs = types.ModuleType("pygsp.graphs")
    mod.graphs.Graph = Graph
    mod.filters = types.ModuleType("pygsp.filters")
    approximations = mod.filters.approximations = types.ModuleType("pygsp.filters.approximations")
    approximations.cheby_op = mod.filters.cheby_op = cheby_op
    approximations.compute_cheby_coeff = compute_cheby_coeff
    mod.filters.Filter = Filter
    return mod, calls


@pytest.fixture
def seam(monkeypatch):
    """(stand-in module, call counts); the device object of a graph is the oracle-backed one, and the originals are
    checked to be back in place once the test has uninstalled the seam."""
    mod, calls = standin_pygsp()

    def device_graph_for(G, ctx=None, dtype=None):
        cached = getattr(G, "_gspx_dev", None)
        if cached is not None and cached[0] is G.L:
            return cached[1]
        calls["device_graphs"] += 1
        G._gspx_dev = (G.L, OracleDevice(G, calls))
        return G._gspx_dev[1]

    monkeypatch.setattr(plugin, "device_graph_for", device_graph_for)
    originals = (mod.filters.approximations.cheby_op, mod.filters.cheby_op, mod.filters.Filter.filter,
                 mod.filters.Filter.compute_frame, mod.graphs.Graph.estimate_lmax)
    yield mod, calls
    plugin.uninstall(mod)
    assert (mod.filters.approximations.cheby_op, mod.filters.cheby_op, mod.filters.Filter.filter,
            mod.filters.Filter.compute_frame, mod.graphs.Graph.estimate_lmax) == originals


def _test_filters_cases(mod, calls):
    """The cases of pygsp/tests/test_filters.py on its own fixture (Sensor(123, seed=42), exact lmax): Heat(10) on
    one and five signals, low orders, the two-scale Heat frame, MexicanHat(Nf=6) analysis and synthesis of one and
    five signals - each against the real reference's output."""
    g = load_golden("sensor123.npz")
    lmax = float(g["lmax"])
    G = mod.graphs.Graph(csr_from(g, "W"), lmax)
    assert abs(G.L - csr_from(g, "Lcomb")).max() < 1e-14
    heat = mod.filters.Filter(G, [orc.heat_kernel(10, lmax)])
    mh = mod.filters.Filter(G, orc.mexican_hat_kernels(lmax, 6))
    assert rel_err(mod.filters.approximations.compute_cheby_coeff(mh, m=40), g["mh6_c"]) < TOL
    checks = [
        (heat.filter(g["signal"], method="chebyshev", order=30), g["heat10_y"]),
        (heat.filter(g["signals5"], method="chebyshev", order=30), g["heat10_y5"]),
        (heat.filter(g["signal"], method="chebyshev", order=1), g["heat10_order1"]),
        (heat.filter(g["signal"], method="chebyshev", order=2), g["heat10_order2"]),
        (mod.filters.Filter(G, [orc.heat_kernel(8, lmax), orc.heat_kernel(9, lmax)]).compute_frame(
            method="chebyshev", order=30), g["heat89_frame"]),
    ]
    a5 = mh.filter(g["signals5"], method="chebyshev", order=40)
    a1 = mh.filter(g["signal"], method="chebyshev", order=40)
    checks += [(a5, g["mh6_analysis"]), (a1, g["mh6_analysis1"]),
               (mh.filter(a5, method="chebyshev", order=40), g["mh6_synthesis"]),
               (mh.filter(a1, method="chebyshev", order=40), g["mh6_synthesis1"])]
    calls["synthesis_filters"] += 2
    for i, (y, ref) in enumerate(checks):
        assert np.shape(y) == ref.shape, (i, np.shape(y), ref.shape)
        assert rel_err(y, ref) < TOL, (i, rel_err(y, ref))
    with pytest.raises(ValueError):
        heat.filter(g["signal"][:-1])


def test_reference_test_filters_passes_through_the_patched_seam(seam):
    """install(): cheby_op, Filter.filter and compute_frame are the product's; every case gives the reference's
    output, no original runs, and every synthesis is ONE device call instead of Nf cheby_op calls."""
    mod, calls = seam
    plugin.install(mod)
    assert mod.filters.approximations.cheby_op is product_filters.cheby_op is mod.filters.cheby_op
    assert mod.filters.Filter.filter.__module__ == mod.filters.Filter.compute_frame.__module__ == "pygsp_amd.plugin"
    _test_filters_cases(mod, calls)
    assert calls["original_filter"] == calls["original_cheby_op"] == calls["original_frame"] == 0
    assert calls["cheby_op"] >= 9 and calls["device_graphs"] == 1
    assert calls["synthesis_device_calls"] == calls["synthesis_filters"] == 2


def test_reference_test_filters_passes_with_the_primary_seam_alone(seam):
    """install(wrap_filter=False): cheby_op is the only patched name; the stand-in's own Filter.filter and synthesis
    loop call it (once per filter) and no fused synthesis call is made."""
    mod, calls = seam
    original_filter, original_frame = mod.filters.Filter.filter, mod.filters.Filter.compute_frame
    plugin.install(mod, wrap_filter=False)
    assert mod.filters.approximations.cheby_op is product_filters.cheby_op
    assert mod.filters.Filter.filter is original_filter and mod.filters.Filter.compute_frame is original_frame
    _test_filters_cases(mod, calls)
    assert calls["original_cheby_op"] == 0 and calls["original_filter"] == 9 and calls["original_frame"] == 1
    assert calls["cheby_op"] == 7 + 2 * 6 and calls["synthesis_device_calls"] == 0


def test_reference_doctest_value_through_the_seam(seam):
    """filter.py:255-256 (the doctest of Filter.filter): Sensor(30, seed=42), a delta through Heat(3), MexicanHat x 4
    analysis then synthesis, ||s1 - s3|| = 0.27649 - through the patched seam, each stage equal to the reference's."""
    mod, calls = seam
    g = load_golden("doctest_sensor30.npz")
    lmax = float(g["lmax"])
    plugin.install(mod)
    G = mod.graphs.Graph(csr_from(g, "W"), lmax)
    s = np.zeros(G.N)
    s[13] = 1
    s1 = mod.filters.Filter(G, [orc.heat_kernel(3, lmax)]).filter(s)
    bank = mod.filters.Filter(G, orc.mexican_hat_kernels(lmax, 4))
    s2 = bank.filter(s1)
    assert s2.shape == (30, 4)
    s3 = bank.filter(s2)
    assert s3.shape == (30,)
    assert "{:.5f}".format(np.linalg.norm(s1 - s3)) == "0.27649"
    assert rel_err(s1, g["s1"]) < TOL and rel_err(s2, g["s2"]) < TOL and rel_err(s3, g["s3"]) < TOL
    assert calls["cheby_op"] >= 3 and calls["original_cheby_op"] == 0


def test_estimate_lmax_seam_on_the_real_graph_class(seam):
    """plugin.install(pygsp, lmax='device') replaces ``Graph.estimate_lmax`` and uninstall() / a default install()
    put the original back; with the seam in place the 'bounds' method is still the original code, and on the Logo
    graph it gives the reference's 18.583333333333332 (the 'lanczos' branch itself runs in `-m gpu`,
    test_plugin_estimate_lmax_seam)."""
    mod, calls = seam
    g = load_golden("logo_heat50.npz")
    orig = mod.graphs.Graph.estimate_lmax
    plugin.install(mod, lmax="device")
    assert mod.graphs.Graph.estimate_lmax is not orig
    G = mod.graphs.Graph(csr_from(g, "W"))
    assert rel_err(G.dw, g["dw"]) < 1e-15
    G.estimate_lmax("bounds")
    assert calls["original_lmax"] == 1 and G._lmax_method == "bounds"
    assert abs(G.lmax - 18.583333333333332) < 1e-12 and abs(G.lmax - float(g["lmax_bounds"])) < 1e-12
    plugin.install(mod)
    assert mod.graphs.Graph.estimate_lmax is orig
    plugin.install(mod, lmax="device")
    plugin.uninstall(mod)
    assert mod.graphs.Graph.estimate_lmax is orig
