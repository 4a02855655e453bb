"""Shared by tests/test_cluster_host.py and tests/test_gpu_z_cluster.py: inputs with exact ties, an independent naive
Lloyd, host-computed spectral features of planted block models."""
import numpy as np
from scipy import sparse

from pygsp_amd import clustering, graphs, spectrum

# (N, k, p, q) of the planted partitions both suites must recover, three graph seeds each
SBM_CASES = {"sbm512": (512, 4, 0.5, 0.02), "sbm300": (300, 3, 0.3, 0.02)}
SBM_SEEDS = (0, 1, 2)
ORDER = 50
# the density estimate behind the default lambda_k in these suites: the default order, and 512 probes instead of the
# default 32, with which the estimate misses the gap on two of the six graphs (test_default_lambda_k_lies_in_the_gap)
DENSITY_ORDER, N_VECTORS = 100, 512


def blobs(n, d, k, seed, spread=0.05):
    """k well-separated Gaussian blobs (centres on a lattice of spacing 4) and their labels."""
    rng = np.random.default_rng(seed)
    centres = rng.permutation(4 ** min(d, 6))[:k]
    C = np.zeros((k, d))
    for j in range(min(d, 6)):
        C[:, j] = 4.0 * ((centres // 4 ** j) % 4)
    z = rng.integers(0, k, n)
    z[:k] = np.arange(k)
    return C[z] + spread * rng.standard_normal((n, d)), z, C


def naive_lloyd(X, centers, max_iter=100):
    """argmin of a broadcast distance, np.mean per cluster: independent of clustering.kmeans_host."""
    centers = np.array(centers, dtype=np.float64)
    labels = None
    for _ in range(max_iter + 1):
        new = np.argmin(((X[:, None, :] - centers[None, :, :]) ** 2).sum(-1), axis=1)
        if labels is not None and np.array_equal(new, labels):
            break
        labels = new
        for c in range(centers.shape[0]):
            if np.any(labels == c):
                centers[c] = X[labels == c].mean(0)
    return labels, centers


def lattice(side=5):
    """The integer lattice side x side: distances are small integers, so ties are exact."""
    g = np.arange(side, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)


def same_partition(a, b):
    """Two labelings describe one partition (equal up to renaming)."""
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def sbm_host(name, seed):
    """(z, W, L dense) of a planted block model from the numpy sampler."""
    N, k, p, q = SBM_CASES[name]
    z = np.sort(np.random.default_rng(seed).integers(0, k, N))
    W = sparse.csr_matrix(graphs.sbm_weights(N, k, z=z, p=p, q=q, seed=seed)[0], dtype=np.float64)
    L = (sparse.diags(np.asarray(W.sum(1)).ravel()) - W).toarray()
    return z, W, L


def cheby_apply_host(L, lmax, c, x):
    """sum_k c_k T_k(Lt) x with c_0 halved, Lt = (2 / lmax) L - I: the recurrence of cheby_op in numpy."""
    a = lmax / 2.0
    t0, t1 = x, (L @ x - a * x) / a
    y = 0.5 * c[0] * t0 + c[1] * t1
    for k in range(2, len(c)):
        t0, t1 = t1, (2.0 / a) * (L @ t1 - a * t1) - t0
        y = y + c[k] * t1
    return y


def density_host(L, lmax, seed=0, order=DENSITY_ORDER, n_vectors=N_VECTORS):
    """spectrum.estimate_spectral_density with the moments taken in numpy (same probes, same estimator)."""
    z = spectrum.probes(L.shape[0], n_vectors, seed)
    a = lmax / 2.0
    t0, t1 = z, (L @ z - a * z) / a
    m = [np.sum(z * t0, 0), np.sum(z * t1, 0)]
    for _ in range(2, order + 1):
        t0, t1 = t1, (2.0 / a) * (L @ t1 - a * t1) - t0
        m.append(np.sum(z * t1, 0))
    return spectrum.SpectralDensity(np.array(m), lmax, L.shape[0])


def features_host(L, k, kind, lmax, lambda_k, seed=0):
    """The embedding of clustering.spectral_embedding computed in numpy."""
    N = L.shape[0]
    if kind == "fourier":
        return np.linalg.eigh(L)[1][:, :k]
    d = clustering.default_n_features(N)
    c = clustering.lowpass_coefficients(lambda_k, lmax, ORDER)
    return cheby_apply_host(L, lmax, c, clustering.random_signals(N, d, seed))
