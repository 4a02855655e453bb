"""Localised-atom norms and spectrograms on the device (pygsp_amd.features, filters.frame_norms,
gspx_cheby_sqnorms_dev / k_combine_sqnorm): the reference's fixtures in fp64 and fp32, sampled deltas of a 1M-vertex
graph against the oracle, a full spectrogram against narrow panels, determinism, odd widths and bank sizes around the
one-pass cap."""
import numpy as np
import pytest
from scipy import sparse
from scipy.sparse import csgraph

from conftest import csr_from, load_golden, rel_err
from gpu_helpers import TOL, ctx, random_graph  # noqa: F401 (ctx: fixture)
from oracle import cheby_oracle as orc
from pygsp_amd import engine, features, filters, graphs

pytestmark = pytest.mark.gpu


def golden_graph(g, lap, dtype):
    G = graphs.Graph(csr_from(g, "W"), lap_type=lap, compute_dtype=dtype)
    G._lmax = float(g["lmax_" + lap])
    return G


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_features_against_reference_fixtures(dtype):
    tol = TOL[np.dtype(dtype)]
    g = load_golden("features_sensor123.npz")
    for lap in ("combinatorial", "normalized"):
        G = golden_graph(g, lap, dtype)
        n = features.compute_norm_tig(filters.Heat(G, scale=10))
        assert n.shape == (G.N,) and rel_err(n, g["heat10_norm_tig_" + lap]) < tol, lap
    G = golden_graph(g, "combinatorial", dtype)
    mh = features.compute_norm_tig(filters.MexicanHat(G, Nf=6))
    assert isinstance(mh, list) and len(mh) == 6
    for a in mh:
        assert a.shape == (6 * G.N,) and rel_err(a, g["mh6_norm_tig"]) < tol
    s = features.compute_spectrogram(G)
    assert s.shape == (G.N, 100) and G.spectr is s and rel_err(s, g["spectrogram_M100"]) < tol
    lg = load_golden("features_logo.npz")
    G = golden_graph(lg, "combinatorial", dtype)
    s = features.compute_spectrogram(G, M=30)
    assert s.shape == (G.N, 30) and rel_err(s, lg["spectrogram_M30"]) < tol


def atoms(lmax, M, order=30):
    G = type("G", (), {"lmax": lmax})()
    return filters._as_coeff_matrix(filters.compute_cheby_coeff(filters.Filter(G, features.spectrogram_kernels(G, None, M)),
                                                                m=order))


def oracle_sqnorms(L, lmax, C, x):
    y = orc.cheby_op(L, lmax, C, x).reshape(C.shape[0], L.shape[0], -1)
    return np.einsum("fnw,fnw->fw", y, y)


def test_sqnorms_on_sampled_deltas_of_a_million_vertices():
    """64 deltas of a 1M-vertex sensor graph (first, last, highest-degree and an isolated vertex among them), 100
    atoms: each delta against the oracle's cheby_op on the 31-hop ball around it - T_k delta_j for k <= 30 lives
    inside it and every vertex it reaches keeps all its neighbours there, so the numbers are the full graph's."""
    S = graphs.Sensor(1_000_000, seed=0)
    W = S.W.tocsr()
    iso = 123_457
    mask = np.ones(W.shape[0])
    mask[iso] = 0
    D = sparse.diags(mask)
    W = sparse.csr_matrix(D @ W @ D)
    W.eliminate_zeros()
    G = graphs.Graph(W, coords=S.coords)
    G.estimate_lmax("bounds")
    deg = np.diff(W.indptr)
    rng = np.random.default_rng(1)
    forced = [0, G.N - 1, int(np.argmax(deg)), iso]
    rest = rng.choice(np.setdiff1d(np.arange(G.N), forced), 64 - len(forced), replace=False)
    cols = np.sort(np.concatenate([forced, rest]))
    assert cols.size == 64 and iso in cols and 0 in cols and G.N - 1 in cols and deg[iso] == 0
    C = atoms(G.lmax, 100)
    dev = G.device_graph(np.float64)
    X = np.zeros((G.N, 64))
    X[cols, np.arange(64)] = 1
    d = engine.DeviceArray.from_host(dev.ctx, X, np.float64)
    try:
        s, _ = dev.cheby_sqnorms_dev(C, d.ptr, 64, G.lmax)
        s2, _ = dev.cheby_sqnorms_dev(C, d.ptr, 64, G.lmax)
    finally:
        d.free()
    assert s.shape == (100, 64) and np.array_equal(s, s2)
    L = orc.laplacian(W)
    for j, v in enumerate(cols):
        dist = csgraph.dijkstra(W, indices=int(v), unweighted=True, limit=31.5)
        ball = np.flatnonzero(np.isfinite(dist))
        Lb = L[ball][:, ball]
        x = (ball == v).astype(np.float64)[:, None]
        ref = oracle_sqnorms(Lb, G.lmax, C, x)[:, 0]
        assert rel_err(s[:, j], ref) < TOL[np.dtype(np.float64)], (j, v)


def test_full_spectrogram_against_narrow_panels():
    G = graphs.Sensor(20_000, seed=3)
    G.estimate_lmax("bounds")
    s = features.compute_spectrogram(G)
    bank = filters.Filter(G, features.spectrogram_kernels(G, None, 100))
    ref = filters.frame_norms(bank, 30, panel=64).T
    assert s.shape == (G.N, 100) and rel_err(s, ref) < TOL[np.dtype(np.float64)]
    assert np.array_equal(s, features.compute_spectrogram(G))  # identical calls, identical bits


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nsig", [1, 3, 5, 67, 130])
def test_sqnorms_odd_widths(dtype, nsig):
    W = random_graph(3000, 8, seed=nsig, hub=True, isolated=2)
    G = graphs.Graph(W, compute_dtype=dtype)
    G.estimate_lmax("bounds")
    C = atoms(G.lmax, 12)
    x = np.random.default_rng(nsig).standard_normal((G.N, nsig))
    dev = G.device_graph(dtype)
    d = engine.DeviceArray.from_host(dev.ctx, x, dtype)
    try:
        s, _ = dev.cheby_sqnorms_dev(C, d.ptr, nsig, G.lmax)
    finally:
        d.free()
    ref = oracle_sqnorms(orc.laplacian(W), G.lmax, C, x.astype(dtype).astype(np.float64))
    assert s.shape == (12, nsig) and rel_err(s, ref) < TOL[np.dtype(dtype)]


@pytest.mark.parametrize("nf", [1, 8, 9, 129])
def test_sqnorms_bank_sizes_around_the_one_pass_cap(ctx, nf):
    W = random_graph(5000, 6, seed=nf, isolated=1)
    G = graphs.Graph(W, compute_dtype=np.float64)
    G.estimate_lmax("bounds")
    C = atoms(G.lmax, nf, order=20)
    x = np.random.default_rng(nf).standard_normal((G.N, 20))
    dev = G.device_graph(np.float64)
    d = engine.DeviceArray.from_host(dev.ctx, x, np.float64)
    try:
        s, _ = dev.cheby_sqnorms_dev(C, d.ptr, 20, G.lmax)
        ctx.set_option("max_batch", 8)  # three column batches
        s3, _ = dev.cheby_sqnorms_dev(C, d.ptr, 20, G.lmax)
        ctx.set_option("max_batch", 0)
        t = dev.ctx.last_timing()
    finally:
        d.free()
    ref = oracle_sqnorms(orc.laplacian(W), G.lmax, C, x)
    assert s.shape == (nf, 20) and rel_err(s, ref) < TOL[np.dtype(np.float64)]
    assert rel_err(s3, ref) < TOL[np.dtype(np.float64)]
    assert t["total_ms"] > 0
