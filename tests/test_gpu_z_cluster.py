"""k-means and spectral clustering on the device (csrc/gspx_cluster.hip.h, pygsp_amd.clustering).

Lloyd's iteration from a given init, k-means++ seeding and row normalisation equal the numpy restatement
(clustering.kmeans_host, seed_host, rows_normalize_host) EXACTLY: labels, centre bits, inertia bits, iteration count,
convergence flag, chosen rows.  End to end: planted block models are recovered from both feature kinds with the panel
on the device throughout, and on a sensor graph the device labels equal kmeans_host on the downloaded device
features."""
import numpy as np
import pytest

import cluster_helpers as ch
from pygsp_amd import clustering, engine, graphs

pytestmark = pytest.mark.gpu

R = clustering.update_rows()
NS = (1, 63, 64, 65, 257, 1000, 2 * R + 1)
DS = (1, 2, 3, 25, 64, 65, 128)
CS = (1, 2, 7, 64)


def lloyd_cases():
    cases = [(n, 3, min(2, n)) for n in NS] + [(n, 65, min(7, n)) for n in NS]
    cases += [(1000, d, 7) for d in DS] + [(257, d, min(64, 8192 // d)) for d in DS]
    cases += [(1000, 25, c) for c in CS] + [(2 * R + 1, 33, 64), (4 * R + 77, 2, 64), (300, 8, 300)]
    return sorted(set(cases))


def data(n, d, seed):
    """Clumped rows (so that Lloyd moves for a few iterations) with a few exact duplicates."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)) + 3.0 * rng.integers(0, 3, (n, 1)) * rng.standard_normal((1, d))
    if n > 4:
        X[n // 2] = X[0]
        X[n - 1] = X[1]
    return np.ascontiguousarray(X)


def same(dev, host):
    """Bitwise equality of two results."""
    assert np.array_equal(dev.labels, host.labels)
    assert dev.labels.dtype == np.int32
    assert dev.centers.tobytes() == host.centers.tobytes()
    assert np.float64(dev.inertia).tobytes() == np.float64(host.inertia).tobytes(), (dev.inertia, host.inertia)
    assert (dev.n_iter, dev.converged) == (host.n_iter, host.converged)


@pytest.mark.parametrize("n,d,c", lloyd_cases())
def test_lloyd_equals_the_restatement(n, d, c):
    X = data(n, d, seed=n + 7 * d + c)
    init = X[np.random.default_rng(c).permutation(n)[:c]]
    dev = clustering.kmeans(X, c, init=init, max_iter=6)
    same(dev, clustering.kmeans_host(X, c, init=init, max_iter=6))


def test_hand_cases_equal_the_restatement():
    lattice = ch.lattice(5)
    ties = np.array([[1.0, 1.0], [1.0, 3.0], [3.0, 1.0], [3.0, 3.0]])
    dev = clustering.kmeans(lattice, 4, init=ties, max_iter=0)
    grid = dev.labels.reshape(5, 5)
    assert grid[2, 0] == 0 and grid[0, 2] == 0 and grid[2, 2] == 0 and grid[2, 3] == 1 and grid[3, 2] == 2
    same(dev, clustering.kmeans_host(lattice, 4, init=ties, max_iter=0))
    same(clustering.kmeans(lattice, 4, init=ties), clustering.kmeans_host(lattice, 4, init=ties))
    P = np.repeat(np.array([[0.0, 0.0], [5.0, 5.0]]), 4, axis=0)
    twice = np.array([[0.0, 0.0], [0.0, 0.0], [5.0, 5.0]])
    dev = clustering.kmeans(P, 3, init=twice)
    assert dev.labels.tolist() == [0, 0, 0, 0, 2, 2, 2, 2]
    same(dev, clustering.kmeans_host(P, 3, init=twice))
    # a centre that attracts nothing is kept
    X, z, _ = ch.blobs(300, 2, 2, 3)
    init = np.vstack([X[0], X[1], [1e3, 1e3]])
    dev = clustering.kmeans(X, 3, init=init)
    assert np.array_equal(dev.centers[2], [1e3, 1e3]) and not np.any(dev.labels == 2)
    same(dev, clustering.kmeans_host(X, 3, init=init))
    # an init that is a fixed point; max_iter reached
    X, z, _ = ch.blobs(500, 3, 4, 5)
    fixed = clustering.kmeans_host(X, 4, init=X[:4]).centers
    dev = clustering.kmeans(X, 4, init=fixed)
    assert dev.n_iter == 1 and dev.converged and np.array_equal(dev.labels, z)
    same(dev, clustering.kmeans_host(X, 4, init=fixed))
    Y = np.random.default_rng(6).standard_normal((600, 2))
    dev = clustering.kmeans(Y, 5, init=Y[:5], max_iter=2)
    assert dev.n_iter == 2 and not dev.converged
    same(dev, clustering.kmeans_host(Y, 5, init=Y[:5], max_iter=2))
    same(clustering.kmeans(Y, 5, init=Y[:5]), clustering.kmeans_host(Y, 5, init=Y[:5]))


@pytest.mark.parametrize("d,c", [(25, 7), (65, 3)])
def test_a_slice_of_a_wider_panel_and_twice_the_same_bits(d, c):
    wide = data(1500, d + 15, seed=d)
    X = np.ascontiguousarray(wide[:, 3:3 + d])
    ctx = engine.default_context()
    panel = engine.DeviceArray.from_host(ctx, wide)
    init = X[:c]
    first = clustering.kmeans_dev(ctx, panel.ptr + 8 * 3, 1500, d, d + 15, c, init=init, max_iter=5)
    again = clustering.kmeans_dev(ctx, panel.ptr + 8 * 3, 1500, d, d + 15, c, init=init, max_iter=5)
    same(first, again)
    same(first, clustering.kmeans_host(X, c, init=init, max_iter=5))
    assert np.array_equal(np.asarray(panel), wide)  # (the panel is only read)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_seeding_equals_the_restatement(seed):
    for n, d, c in ((2 * R + 300, 4, 6), (700, 65, 9), (5, 2, 5)):
        X = data(n, d, seed=seed + n)
        dev = clustering.kmeans(X, c, seed=seed, max_iter=3)
        host = clustering.kmeans_host(X, c, seed=seed, max_iter=3)
        assert np.array_equal(dev.seeds, host.seeds), (n, d, c)
        same(dev, host)
    best = clustering.kmeans(X, c, seed=seed, n_init=3, max_iter=3)
    same(best, clustering.kmeans_host(X, c, seed=seed, n_init=3, max_iter=3))
    # fewer distinct rows than centres: the first rows not chosen yet
    equal = np.ones((40, 3))
    dev = clustering.kmeans(equal, 4, seed=seed, max_iter=0)
    assert np.array_equal(dev.seeds, clustering.kmeans_host(equal, 4, seed=seed, max_iter=0).seeds)
    assert len(set(dev.seeds.tolist())) == 4 and set(dev.seeds[1:].tolist()) <= {0, 1, 2, 3}
    two = np.vstack([np.zeros((5, 2)), np.ones((5, 2))])
    dev = clustering.kmeans(two, 3, seed=seed)
    same(dev, clustering.kmeans_host(two, 3, seed=seed))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_row_normalisation_equals_the_restatement(seed):
    ctx = engine.default_context()
    for n, d in ((1, 1), (300, 3), (257, 25), (1000, 130)):
        X = data(n, d, seed=seed + d) * 10.0 ** np.random.default_rng(seed).integers(-3, 4, (n, 1))
        X[n // 3] = 0.0
        dev = engine.DeviceArray.from_host(ctx, X)
        clustering.rows_normalize_dev(ctx, dev.ptr, n, d)
        out = np.asarray(dev).reshape(n, d)
        assert out.tobytes() == clustering.rows_normalize_host(X).tobytes(), (n, d)
        assert not out[n // 3].any()
    wide = data(500, 12, seed=seed)
    dev = engine.DeviceArray.from_host(ctx, wide)
    clustering.rows_normalize_dev(ctx, dev.ptr + 8 * 2, 500, 7, ld=12)
    ref = wide.copy()
    ref[:, 2:9] = clustering.rows_normalize_host(wide[:, 2:9])
    assert np.asarray(dev).tobytes() == ref.tobytes()
    res = clustering.kmeans(wide, 3, init=wide[:3], normalize_rows=True)
    same(res, clustering.kmeans_host(wide, 3, init=wide[:3], normalize_rows=True))


@pytest.mark.parametrize("kind", ["fourier", "compressive"])
@pytest.mark.parametrize("seed", ch.SBM_SEEDS)
@pytest.mark.parametrize("name", sorted(ch.SBM_CASES))
def test_planted_partitions_are_recovered_on_the_device(name, seed, kind):
    """The low-pass of the compressive features cuts in the middle of the gap, read off eigvalsh of the downloaded
    Laplacian: the default estimate of lambda_k can sit at the gap's upper end (tests/test_cluster_host.py)."""
    N, k, p, q = ch.SBM_CASES[name]
    G = graphs.StochasticBlockModel(N, k=k, p=p, q=q, seed=seed)
    G.estimate_lmax()
    e = np.linalg.eigvalsh(G.L.toarray())
    kw = {"lambda_k": 0.5 * (e[k - 1] + e[k]), "order": ch.ORDER} if kind == "compressive" else {}
    res = clustering.spectral_clustering(G, k, features=kind, seed=0, **kw)
    print(name, seed, kind, "gap", e[k - 1], e[k], "sizes", np.bincount(res.labels), "n_iter", res.n_iter)
    assert res.features == kind and res.converged
    assert ch.same_partition(res.labels, G.z)


def test_sensor_labels_equal_the_restatement_on_the_device_features():
    G = graphs.Sensor(1000, seed=3)
    G.estimate_lmax()
    for kind in ("compressive", "fourier"):
        F = clustering.spectral_embedding(G, 8, kind, seed=0)
        assert isinstance(F, engine.DeviceArray) and F.kind == kind
        host = np.asarray(F).reshape(F.shape)
        if kind == "compressive":
            d = clustering.default_n_features(1000)
            assert host.shape == (1000, d) and d == 28
            sd = G.estimate_spectral_density(100, 32, 0)
            assert F.lambda_k == clustering.lambda_k_of(sd, 8) and 0.0 < F.lambda_k < G.lmax
        else:
            assert host.shape == (1000, 8) and np.array_equal(host, G.U[:, :8]) and F.lambda_k is None
        dev = clustering.kmeans(F, 8, seed=0, normalize_rows=True)
        assert np.array_equal(np.asarray(F).reshape(F.shape), host)  # (normalised in a copy)
        same(dev, clustering.kmeans_host(host, 8, seed=0, normalize_rows=True))
    e_before, U_before = G.e.copy(), G.U.copy()
    res = clustering.spectral_clustering(G, 8)  # 'auto': the basis is there
    assert res.features == "fourier" and res.lambda_k is None
    assert np.array_equal(G.e, e_before) and np.array_equal(G.U, U_before)
    same(res, clustering.kmeans_host(U_before[:, :8], 8, seed=0, normalize_rows=True))
    res = clustering.spectral_clustering(G, 8, features="compressive")
    assert res.features == "compressive" and res.lambda_k == clustering.lambda_k_of(G.estimate_spectral_density(), 8)


def test_a_device_array_is_clustered_where_it_lies(monkeypatch):
    X, z, _ = ch.blobs(5000, 16, 5, 9)
    ctx = engine.default_context()
    panel = engine.DeviceArray.from_host(ctx, X)
    seen = []
    download = engine.DeviceBuffer.download

    def counted(self, shape, dtype):
        seen.append(int(np.prod(shape)) * np.dtype(dtype).itemsize)
        return download(self, shape, dtype)

    monkeypatch.setattr(engine.DeviceBuffer, "download", counted)
    res = clustering.kmeans(panel, 5, seed=1)
    monkeypatch.undo()
    assert sorted(seen) == [5 * 16 * 8, 5000 * 4]  # the labels and the centres, nothing of the panel's size
    assert isinstance(res.labels, np.ndarray) and res.labels.dtype == np.int32 and res.labels.shape == (5000,)
    same(res, clustering.kmeans_host(X, 5, seed=1))
    assert ch.same_partition(res.labels, z)
    with pytest.raises(ValueError, match="128"):
        clustering.kmeans(engine.DeviceArray.from_host(ctx, np.zeros((4, 129))), 2)
