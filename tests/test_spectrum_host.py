"""pygsp_amd.spectrum without a GPU: the doubling identity behind gspx_cheby_moments_dev, the density / cdf / count /
quantile formulas on spectra known in closed form, the argument checks of the entry point, and
estimate_spectral_density over a stand-in device object whose cheby_moments is the numpy restatement."""
import ctypes

import numpy as np
import pytest

from conftest import rel_err
from gpu_helpers import random_graph, upper_lmax
from oracle import cheby_oracle as orc
from pygsp_amd import _capi, filters, graphs, spectrum
from spectrum_helpers import exact_moments, moments_direct, moments_doubling


@pytest.mark.parametrize("M", [64, 65])
def test_doubling_identity(M):
    W = random_graph(2000, 8, seed=1, hub=True, isolated=2)
    L, lmax = orc.laplacian(W), upper_lmax(W)
    z = spectrum.probes(2000, 32, 0)
    ref = moments_direct(L, lmax, z, M)
    err = rel_err(moments_doubling(L, lmax, z, M), ref)
    print("doubling against direct, M = {}: {:.2e}".format(M, err))
    assert ref.shape == (M, 32) and err < 1e-12


def ring_density(M, damping="jackson"):
    n, lmax = 240, 4.04
    e = 2.0 - 2.0 * np.cos(2.0 * np.pi * np.arange(n) / n)
    return e, lmax, spectrum.SpectralDensity(n * exact_moments(e, lmax, M)[:, None], lmax, n, damping)


@pytest.mark.parametrize("M", [64, 128])
def test_ring_of_240_vertices(M):
    e, lmax, sd = ring_density(M)
    assert sd.order == M - 1 and sd.n_vertices == 240 and sd.lmax == lmax
    lam = np.linspace(0, lmax, 41)
    exact = (e[None, :] <= lam[:, None]).mean(1)
    err = np.max(np.abs(sd.cdf(lam) - exact))
    steps = np.diff(sd.cdf(np.linspace(0, lmax, 2001)))
    print("ring, M = {}: cdf error {:.2e}, smallest cdf step {:.2e}".format(M, err, steps.min()))
    assert err <= 0.02
    assert steps.min() >= -1e-12
    assert abs(sd.cdf(0.0)) <= 1e-15 and abs(sd.cdf(-1.0)) <= 1e-15
    assert abs(sd.cdf(lmax) - 1) <= 1e-14 and abs(sd.cdf(lmax + 1) - 1) <= 1e-14
    pts = np.linspace(0.05, 0.95, 37) * lmax
    h = 1e-5 * lmax
    pdf = sd.pdf(pts)
    slope = (sd.cdf(pts + h) - sd.cdf(pts - h)) / (2 * h)
    d = np.max(np.abs(slope - pdf) / np.abs(pdf))
    print("ring, M = {}: central difference of cdf against pdf {:.2e}".format(M, d))
    assert d < 1e-6
    assert np.all(sd.pdf(np.linspace(-0.5, lmax + 0.5, 1001)) >= 0)
    assert sd.pdf(0.0) == 0 and sd.pdf(lmax) == 0 and sd.pdf(-1.0) == 0 and sd.pdf(lmax + 1) == 0
    for q in (0.1, 0.5, 0.9):
        assert abs(sd.cdf(sd.quantile(q)) - q) < 1e-12, q
    qs = sd.quantile(np.array([0.1, 0.5, 0.9]))
    assert qs.shape == (3,) and np.all(np.diff(qs) > 0) and qs[1] == sd.quantile(0.5)


def test_quantile_needs_jackson_damping():
    _, _, sd = ring_density(64, damping=None)
    assert sd.damping is None
    with pytest.raises(ValueError):
        sd.quantile(0.5)
    with pytest.raises(ValueError):
        spectrum.SpectralDensity(np.ones((4, 1)), 2.0, 4, damping="lorentz")


def test_two_clusters():
    e = np.concatenate([np.zeros(6), np.full(114, 20.0)])
    lmax = 20.2
    sd = spectrum.SpectralDensity(120 * exact_moments(e, lmax, 64)[:, None], lmax, 120)
    err = abs(120 * sd.cdf(lmax / 2) - 6)
    print("two clusters: count error {:.2e}".format(err))
    assert err < 0.01
    assert abs(sd.count(-1.0, lmax / 2) - 6) < 0.01 and abs(sd.count(lmax / 2, lmax) - 114) < 0.01


def test_jackson_damping_values():
    g = spectrum.jackson_damping(5)
    k = np.arange(5)
    ref = ((5 - k + 1) * np.cos(np.pi * k / 6) + np.sin(np.pi * k / 6) / np.tan(np.pi / 6)) / 6
    assert g.shape == (5,) and g[0] == 1 and np.allclose(g, ref, rtol=0, atol=1e-15) and np.all(np.diff(g) < 0)
    assert np.array_equal(spectrum.probes(7, 3, 5), np.random.default_rng(5).integers(0, 2, size=(7, 3)) * 2.0 - 1.0)


def test_moments_entry_point_refuses_bad_arguments_without_a_device():
    lib = _capi.load()
    out = np.zeros((5, 4))
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: the checks fail first
    f = lib.gspx_cheby_moments_dev
    with pytest.raises(ValueError, match="null graph"):
        _capi.check(f(None, 2.0, 5, 4, fake, _capi.ptr(out), None))


def test_density_statistics_of_a_hand_made_table():
    m = np.array([[4.0, 4.0], [1.0, 3.0], [0.0, 2.0]])
    sd = spectrum.SpectralDensity(m, 2.0, 4, damping=None)
    assert sd.moments.shape == (3, 2) and sd.order == 2
    assert np.array_equal(sd.mu, [1.0, 0.5, 0.25])
    assert np.allclose(sd.mu_stderr, [0.0, 0.25, 0.25], rtol=0, atol=1e-16)

    def cdf(mu, lam):  # the formula, written out for three moments
        th = np.arccos(np.clip(2 * lam / 2.0 - 1, -1, 1))
        return mu[0] * (1 - th / np.pi) - (2 / np.pi) * (mu[1] * np.sin(th) + mu[2] * np.sin(2 * th) / 2)

    lo, hi = 0.3, 1.4
    per = np.array([4 * (cdf(m[:, p] / 4, hi) - cdf(m[:, p] / 4, lo)) for p in range(2)])
    n, err = sd.count(lo, hi, return_stderr=True)
    assert abs(n - per.mean()) < 1e-14 and abs(n - sd.count(lo, hi)) == 0
    assert abs(err - per.std(ddof=1) / np.sqrt(2)) < 1e-14 and err > 0
    one = spectrum.SpectralDensity(m[:, :1], 2.0, 4)
    assert np.array_equal(one.mu_stderr, np.zeros(3)) and one.count(lo, hi, return_stderr=True)[1] == 0


class StubGraph:
    """What the spectrum code reads from a Graph: N, L, lmax; the two methods under test are Graph's own."""
    estimate_spectral_density = graphs.Graph.estimate_spectral_density
    count_eigenvalues = graphs.Graph.count_eigenvalues

    def __init__(self, L, lmax):
        self.L, self.N, self.lmax = L, L.shape[0], lmax


class StubDev:
    """The numpy restatement behind spectrum.cheby_moments' host branch."""

    def __init__(self, L):
        self.L, self.calls, self.dtype = L, 0, np.float64

    def cheby_moments(self, x, lmax, M):
        self.calls += 1
        return moments_direct(self.L, lmax, x, M), 0.25


def test_estimate_spectral_density_over_a_stand_in_device(monkeypatch):
    W = random_graph(300, 6, seed=4, isolated=1)
    L = orc.laplacian(W)
    G, dev = StubGraph(L, upper_lmax(W)), StubDev(L)
    monkeypatch.setattr(filters, "_device_graph_of", lambda G_: dev)
    sd = G.estimate_spectral_density(order=40, n_vectors=8, seed=3)
    z = spectrum.probes(300, 8, 3)
    assert dev.calls == 1 and G._gspx_last_kernel_ms == 0.25
    assert isinstance(sd, spectrum.SpectralDensity) and sd.damping == "jackson" and sd.lmax == G.lmax
    assert sd.moments.shape == (41, 8) and np.array_equal(sd.moments, moments_direct(L, G.lmax, z, 41))
    assert sd.mu[0] == 1 and sd.n_vertices == 300
    e = np.linalg.eigvalsh(L.toarray())
    lam = float(np.quantile(e, 0.5))
    n, err = sd.count(-1.0, lam, return_stderr=True)
    assert abs(n - np.sum(e <= lam)) <= 0.1 * 300 and err > 0
    assert G.count_eigenvalues(-1.0, lam, order=40, n_vectors=8, seed=3) == n
    m1 = spectrum.cheby_moments(G, z[:, 0], order=5)
    assert m1.shape == (6,) and np.array_equal(m1, moments_direct(L, G.lmax, z[:, :1], 6)[:, 0])
    with pytest.raises(ValueError):
        spectrum.cheby_moments(G, np.zeros((299, 2)))
