"""Chebyshev self-moments and the spectral density on the device (gspx_cheby_moments_dev / k_slot_dots,
pygsp_amd.spectrum, Graph.estimate_spectral_density): every width and parity against the numpy restatement, tiny
shapes, column batches, tile and plain steps, input types, eigenvalue counts against eigvalsh, and a 1M-vertex
graph."""
import numpy as np
import pytest

from conftest import rel_err
from gpu_helpers import TOL, ctx, random_graph, upper_lmax  # noqa: F401 (ctx: fixture)
from oracle import cheby_oracle as orc
from pygsp_amd import graphs, spectrum
from scipy import sparse
from spectrum_helpers import moments_direct

pytestmark = pytest.mark.gpu


def graph_of(W, dtype=np.float64):
    G = graphs.Graph(W, compute_dtype=dtype)
    G._lmax = upper_lmax(W)
    return G


def device_moments(G, x, M, dtype=np.float64):
    """One gspx_cheby_moments_dev call on x uploaded in `dtype`, and the reference on x rounded to it."""
    m, ms = G.device_graph(dtype).cheby_moments(x, G.lmax, M)
    ref = moments_direct(orc.laplacian(G.W), G.lmax, np.asarray(x).astype(dtype).astype(np.float64), M)
    return m, ref, ms


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nsig", [1, 3, 5, 67, 130])
def test_moments_widths_and_parities(dtype, nsig):
    W = random_graph(3000, 8, seed=nsig, hub=True, isolated=2)
    G = graph_of(W, dtype)
    x = np.random.default_rng(nsig).standard_normal((G.N, nsig))
    for M in (13, 14):
        m, ref, _ = device_moments(G, x, M, dtype)
        m2, _, _ = device_moments(G, x, M, dtype)
        err = rel_err(m, ref)
        print("moments {} nsig {} M {}: {:.2e}".format(np.dtype(dtype).name, nsig, M, err))
        assert m.shape == (M, nsig) and m.dtype == np.float64 and err < TOL[np.dtype(dtype)]
        assert np.array_equal(m, m2)  # identical calls, identical bits


@pytest.mark.parametrize("N", [1, 63, 65, 257])
@pytest.mark.parametrize("nsig", [1, 4])
def test_moments_small_shapes(N, nsig):
    W = random_graph(N, 4, seed=N) if N > 1 else sparse.csr_matrix((1, 1))
    G = graphs.Graph(W, compute_dtype=np.float64)
    G._lmax = upper_lmax(W) if N > 1 else 1.0  # (one isolated vertex: L = 0, any positive lmax)
    x = np.random.default_rng(N).standard_normal((N, nsig))
    for M in (2, 3, 4):
        m, ref, _ = device_moments(G, x, M)
        assert m.shape == (M, nsig) and rel_err(m, ref) < TOL[np.dtype(np.float64)], M


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_moments_around_the_chunks_of_slots(dtype):
    """k_slot_dots walks the kept slots in chunks of 16 (of 8 for fp32 panels of an even width), the last slot's
    square riding with the chunk before it: slot counts 8 .. 10 and 16 .. 19, an even and an odd width."""
    W = random_graph(700, 6, seed=11, isolated=1)
    G = graph_of(W, dtype)
    for nsig in (5, 6):
        x = np.random.default_rng(nsig).standard_normal((G.N, nsig))
        for M in (14, 15, 16, 17, 18, 19, 30, 31, 32, 33, 34, 35, 36, 37):
            m, ref, _ = device_moments(G, x, M, dtype)
            assert rel_err(m, ref) < TOL[np.dtype(dtype)], (nsig, M)


def test_moments_column_batches(ctx):
    W = random_graph(5000, 6, seed=7, isolated=1)
    G = graph_of(W)
    x = np.random.default_rng(7).standard_normal((G.N, 20))
    m, ref, _ = device_moments(G, x, 21)
    ctx.set_option("max_batch", 8)  # three column batches
    m3, _, _ = device_moments(G, x, 21)
    ctx.set_option("max_batch", 0)
    assert G.device_graph(np.float64).ctx is ctx
    assert rel_err(m, ref) < TOL[np.dtype(np.float64)] and rel_err(m3, ref) < TOL[np.dtype(np.float64)]


def test_moments_tile_and_plain_steps(ctx):
    G = graphs.Sensor(40_000, seed=3)
    G.estimate_lmax("bounds")
    x = np.random.default_rng(3).standard_normal((G.N, 16))
    m, ref, _ = device_moments(G, x, 32)
    tiled = ctx.last_step_kinds()
    ctx.set_option("tile_gather", 0)
    mp, _, _ = device_moments(G, x, 32)
    plain = ctx.last_step_kinds()
    ctx.set_option("tile_gather", 1)
    assert G.device_graph(np.float64).ctx is ctx
    assert rel_err(m, ref) < TOL[np.dtype(np.float64)] and rel_err(mp, ref) < TOL[np.dtype(np.float64)]
    # 32 moments from 16 recurrence steps: on the gather tiles the graph carries, then on the plain kernels
    assert tiled == {"tile": 16, "plain": 0} and plain == {"tile": 0, "plain": 16}


def test_moments_input_types():
    W = random_graph(1000, 6, seed=2)
    G = graph_of(W)
    x = np.random.default_rng(2).standard_normal((G.N, 5))
    host = spectrum.cheby_moments(G, x, order=9)
    d = G.to_device(x)
    try:
        dev = spectrum.cheby_moments(G, d, order=9)
    finally:
        d.free()
    assert host.shape == (10, 5) and np.array_equal(host, dev)
    one = spectrum.cheby_moments(G, x[:, 2], order=9)
    assert one.shape == (10,) and rel_err(one, host[:, 2]) < TOL[np.dtype(np.float64)]
    assert rel_err(host, moments_direct(orc.laplacian(W), G.lmax, x, 10)) < TOL[np.dtype(np.float64)]


def test_spectral_density_end_to_end():
    W = random_graph(2000, 8, seed=1, isolated=2)
    G = graph_of(W)
    sd = G.estimate_spectral_density(order=127, n_vectors=32, seed=0)
    L = orc.laplacian(W)
    ref = moments_direct(L, G.lmax, spectrum.probes(2000, 32, 0), 128)
    assert sd.moments.shape == (128, 32) and rel_err(sd.moments, ref) < TOL[np.dtype(np.float64)]
    assert sd.mu[0] == 1
    e = np.linalg.eigvalsh(L.toarray())
    for q in (0.1, 0.25, 0.5, 0.75, 0.9):
        lam = float(np.quantile(e, q))
        n = sd.count(-1.0, lam)
        print("count below the {} quantile: {:.1f} against {}".format(q, n, int(np.sum(e <= lam))))
        assert abs(n - np.sum(e <= lam)) <= 40, q
        assert n == G.count_eigenvalues(-1.0, lam, order=127, n_vectors=32, seed=0)


def test_moments_of_a_million_vertices():
    G = graphs.Sensor(1_000_000, seed=0)
    G.estimate_lmax("bounds")
    z = spectrum.probes(G.N, 8, 0)
    m = spectrum.cheby_moments(G, z, order=63)
    ref = moments_direct(orc.laplacian(G.W), G.lmax, z, 64)
    err = rel_err(m, ref)
    print("moments at 1M vertices: {:.2e}".format(err))
    assert m.shape == (64, 8) and err < TOL[np.dtype(np.float64)]
    assert np.array_equal(m[0], np.full(8, float(G.N)))
    sd = spectrum.SpectralDensity(m, G.lmax, G.N)
    assert np.all(np.diff(sd.cdf(np.linspace(0, G.lmax, 513))) >= 0)
