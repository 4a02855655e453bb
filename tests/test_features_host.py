"""pygsp_amd.features (compute_tig / compute_norm_tig / compute_spectrogram) without a GPU: the device call replaced by
the oracle (a stand-in device object driving filters.frame_norms' host branch), checked against fixtures generated
from the reference's own pygsp.features (tests/golden/gen_features_golden.py); the plugin seam on a pygsp-shaped
module; argument checks of gspx_cheby_sqnorms_dev."""
import ctypes
import types

import numpy as np
import pytest

from conftest import csr_from, load_golden, rel_err
from oracle import cheby_oracle as orc
from pygsp_amd import _capi, features, filters, plugin


class StubGraph:
    """What the feature code reads from a Graph: N, L, lmax (and it stores spectr)."""

    def __init__(self, L, lmax):
        self.L, self.N, self.lmax = L, L.shape[0], lmax


class StubDev:
    """The oracle behind filters.frame_norms' stand-in branch (cheby_filter on host arrays)."""

    def __init__(self, L):
        self.L, self.calls = L, 0

    def cheby_filter(self, c, x, lm, mode=0):
        self.calls += 1
        return orc.cheby_op(self.L, lm, c, x).reshape(c.shape[0], self.L.shape[0], -1), 0.0


@pytest.fixture
def sensor(monkeypatch):
    g = load_golden("features_sensor123.npz")

    def make(lap="combinatorial"):
        G = StubGraph(csr_from(g, "L_" + lap), float(g["lmax_" + lap]))
        dev = StubDev(G.L)
        monkeypatch.setattr(filters, "_device_graph_of", lambda G_: dev)
        return G, dev
    return g, make


@pytest.mark.parametrize("lap", ["combinatorial", "normalized"])
def test_norm_tig_of_one_filter_matches_reference(sensor, lap):
    g, make = sensor
    G, _ = make(lap)
    n = features.compute_norm_tig(filters.Heat(G, scale=10))
    assert isinstance(n, np.ndarray) and n.shape == (G.N,)
    assert rel_err(n, g["heat10_norm_tig_" + lap]) < 1e-12


def test_norm_tig_of_a_bank_is_the_reference_list(sensor):
    """Nf > 1: a list of Nf identical (Nf N,) arrays (filterbank_handler over compute_tig, which ignores i); i=...
    gives one of them."""
    g, make = sensor
    G, dev = make()
    mh = filters.MexicanHat(G, Nf=6)
    out = features.compute_norm_tig(mh)
    assert isinstance(out, list) and len(out) == int(g["mh6_list_len"]) == 6 and bool(g["mh6_all_equal"])
    for a in out:
        assert a.shape == (6 * G.N,) and rel_err(a, g["mh6_norm_tig"]) < 1e-12
        assert np.array_equal(a, out[0])
    assert out[0] is not out[1]
    assert dev.calls == 1  # one bank evaluation, not one frame per list entry
    one = features.compute_norm_tig(mh, i=2)
    assert isinstance(one, np.ndarray) and one.shape == (6 * G.N,) and np.array_equal(one, out[0])


def test_kwargs_are_ignored(sensor):
    """The reference's compute_tig drops **kwargs: always Chebyshev, order 30."""
    g, make = sensor
    G, _ = make()
    h = filters.Heat(G, scale=10)
    a = features.compute_norm_tig(h)
    b = features.compute_norm_tig(h, order=5, method="exact")
    assert np.array_equal(a, b)
    s = features.compute_spectrogram(G, M=7, order=3)
    assert np.array_equal(s, features.compute_spectrogram(G, M=7))


def test_spectrogram_matches_reference_sensor(sensor):
    g, make = sensor
    G, dev = make()
    s = features.compute_spectrogram(G)
    assert s.shape == (G.N, 100) and G.spectr is s
    assert rel_err(s, g["spectrogram_M100"]) < 1e-12
    assert dev.calls == 1  # ONE bank of M kernels


def test_spectrogram_matches_reference_logo(monkeypatch):
    g = load_golden("features_logo.npz")
    G = StubGraph(csr_from(g, "L_combinatorial"), float(g["lmax_combinatorial"]))
    monkeypatch.setattr(filters, "_device_graph_of", lambda G_: StubDev(G.L))
    s = features.compute_spectrogram(G, M=30)
    assert s.shape == (G.N, 30) and G.spectr is s
    assert rel_err(s, g["spectrogram_M30"]) < 1e-12


def test_compute_tig_is_the_frame(sensor):
    g, make = sensor
    G, _ = make()
    h = filters.Heat(G, scale=10)
    F = features.compute_tig(h)
    assert F.shape == (G.N, G.N)
    assert rel_err(np.linalg.norm(F, axis=1), g["heat10_norm_tig_combinatorial"]) < 1e-12
    mh = filters.MexicanHat(G, Nf=3)
    Fl = features.compute_tig(mh)
    assert isinstance(Fl, list) and len(Fl) == 3 and all(f.shape == (3 * G.N, G.N) for f in Fl)


def test_spectrogram_kernels_are_distinct_shifts():
    """Each kernel keeps its own shift (no late-binding closure): kernel m peaks at linspace(0, lmax, M)[m]."""
    G = StubGraph(np.zeros((3, 3)), 8.0)
    M = 9
    ks = features.spectrogram_kernels(G, None, M)
    shifts = np.linspace(0, 8.0, M)
    x = np.linspace(0, 8.0, 801)
    vals = np.array([k(x) for k in ks])
    assert len({v.tobytes() for v in vals}) == M
    np.testing.assert_allclose(x[np.argmax(vals, axis=1)], shifts, atol=0.01)
    for m in range(M):
        assert ks[m](shifts[m]) == 1.0
        np.testing.assert_allclose(ks[m](x), np.exp(-M * ((x - shifts[m]) / 8.0) ** 2))
    custom = features.spectrogram_kernels(G, lambda y: y ** 2, 3)
    assert [k(4.0) for k in custom] == [16.0, 0.0, 16.0]


def _standin(with_features=True):
    approx = types.ModuleType("approximations")
    approx.cheby_op = lambda *a, **k: "ref cheby"
    approx.compute_cheby_coeff = lambda *a, **k: None
    fmod = types.ModuleType("filters")
    fmod.approximations = approx
    fmod.cheby_op = approx.cheby_op

    class Filter:
        def __init__(self, G=None, kernels=()):
            self.G, self._kernels = G, list(kernels)

        def filter(self, *a, **k):
            return "ref filter"

        def compute_frame(self, *a, **k):
            return "ref frame"
    fmod.Filter = Filter
    mod = types.ModuleType("pygsp")
    mod.filters = fmod
    if with_features:
        feats = types.ModuleType("features")
        feats.compute_tig = lambda g, **k: "ref tig"
        feats.compute_norm_tig = lambda g, **k: "ref norm tig"
        feats.compute_spectrogram = lambda G, atom=None, M=100, **k: "ref spectrogram"
        mod.features = feats
    return mod


def test_plugin_features_seam_is_opt_in():
    mod = _standin()
    feats = mod.features
    own = (feats.compute_tig, feats.compute_norm_tig, feats.compute_spectrogram)
    try:
        plugin.install(mod)
        assert (feats.compute_tig, feats.compute_norm_tig, feats.compute_spectrogram) == own
        plugin.install(mod, features=True)
        assert feats.compute_norm_tig is not own[1] and feats.compute_spectrogram is not own[2]
        assert feats.compute_tig is own[0]  # reaches the device through the wrapped compute_frame
        plugin.install(mod, features=True)  # again: the saved originals are still the package's own
        plugin.install(mod, features=False)
        assert (feats.compute_tig, feats.compute_norm_tig, feats.compute_spectrogram) == own
        plugin.install(mod, features=True)
        # a graph whose size collides with the shape rules calls the saved original
        G1 = types.SimpleNamespace(N=1)
        assert feats.compute_spectrogram(G1) == "ref spectrogram"
        assert feats.compute_norm_tig(types.SimpleNamespace(G=G1, Nf=1)) == "ref norm tig"
    finally:
        plugin.uninstall(mod)
    assert (feats.compute_tig, feats.compute_norm_tig, feats.compute_spectrogram) == own
    assert not hasattr(feats, plugin._SAVED)
    bare = _standin(with_features=False)
    with pytest.raises(ValueError):
        plugin.install(bare, features=True)
    plugin.uninstall(bare)


def test_plugin_features_run_the_patched_package_on_the_oracle(monkeypatch):
    """The patched compute_spectrogram builds ONE bank of the package's own Filter class, with its own coefficients."""
    g = load_golden("features_sensor123.npz")
    G = StubGraph(csr_from(g, "L_combinatorial"), float(g["lmax_combinatorial"]))
    monkeypatch.setattr(filters, "_device_graph_of", lambda G_: StubDev(G.L))
    mod = _standin()
    seen = []

    def coeff(bank, m=30):
        seen.append((type(bank), len(bank._kernels), m))
        return [filters.compute_cheby_coeff(filters.Filter(bank.G, [k]), m=m) for k in bank._kernels]
    mod.filters.approximations.compute_cheby_coeff = coeff
    mod.filters.Filter.Nf = property(lambda self: len(self._kernels))
    try:
        plugin.install(mod, features=True)
        s = mod.features.compute_spectrogram(G)
        assert rel_err(s, g["spectrogram_M100"]) < 1e-12 and G.spectr is s
        assert seen == [(mod.filters.Filter, 100, 30)]
    finally:
        plugin.uninstall(mod)


def test_sqnorms_entry_point_refuses_bad_arguments_without_a_device():
    lib = _capi.load()
    c = np.ones((2, 5))
    out = np.zeros((2, 4))
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: the checks fail first
    f = lib.gspx_cheby_sqnorms_dev
    with pytest.raises(ValueError, match="null graph"):
        _capi.check(f(None, 2.0, 2, 5, _capi.ptr(c), 4, fake, _capi.ptr(out), None))
