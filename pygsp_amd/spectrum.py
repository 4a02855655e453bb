"""Where a graph's eigenvalues lie, without a Fourier basis: the kernel polynomial method (KPM).

The Chebyshev moments m_k = z^T T_k(Lt) z of a few random +-1 vectors z (Lt = (L - a I) / a, a = lmax / 2, the scaled
operator of approximations.py:93-99) estimate mu_k = tr T_k(Lt) / N, the moments of the density of states.  From them:
the density, its cumulative distribution (the "spectrum cdf approximation" behind spectrum-adapted filter banks),
eigenvalue counts of an interval and quantiles - at the cost of order / 2 recurrence steps on the device
(gspx_cheby_moments_dev) instead of an eigendecomposition.  Everything but that one call is plain numpy.

The device graph comes from filters._device_graph_of(G), so the functions also serve a real pygsp graph after
plugin.install(); pygsp has no counterpart to replace, hence no patch-table entry."""
import numpy as np

from . import engine, filters


def cheby_moments(G, x, order=30):
    """x_j^T T_k(Lt) x_j for k <= order: float64 (order + 1,) for x of shape (N,), (order + 1, Nsig) for (N, Nsig).
    `x`: a host array, or an engine.DeviceArray with one feature (nothing is uploaded then).  Uses G.lmax."""
    dev = filters._device_graph_of(G)
    M = int(order) + 1
    if isinstance(x, engine.DeviceArray):
        n, nsig, nfeat = x.cube
        if nfeat != 1 or n != G.N:
            raise ValueError("cheby_moments takes (N,) or (N, Nsig) signals, got a device array of cube {}"
                             .format(x.cube))
        if np.dtype(x.dtype) != np.dtype(dev.dtype):
            raise TypeError("the device array holds {}, the graph computes in {}".format(x.dtype, np.dtype(dev.dtype)))
        one = len(x.shape) == 1
        m, ms = dev.cheby_moments_dev(x.ptr, nsig, G.lmax, M)
    else:
        x = np.asarray(x)
        if x.ndim not in (1, 2) or x.shape[0] != G.N:
            raise ValueError("cheby_moments takes (N,) or (N, Nsig) signals, got {}".format(x.shape))
        one = x.ndim == 1
        m, ms = dev.cheby_moments(x.reshape(G.N, -1), G.lmax, M)
    filters._record_timing(G, ms)
    m = np.asarray(m, dtype=np.float64)
    return m[:, 0] if one else m


def cheby_cross_moments(G, x, z, order=30):
    """sum_n z_f[n, j] (T_k(Lt) x)[n, j] for k <= order: the recurrence on `x` dotted with the foreign panels `z`
    (gspx_cheby_cross_moments_dev; the coefficient gradient of filters.cheby_op_vjp).  `x`: (N,) or (N, Nsig); `z`:
    (N,), (N, Nsig) or (Nf, N, Nsig), N and Nsig those of `x`.  Both host arrays, or both engine.DeviceArrays of the
    graph's compute dtype - a device `z` of Nf planes is one with Nf features, cube (N, Nsig, Nf).  Returns float64
    (Nf, order + 1, Nsig), without the Nf axis for a `z` of fewer than three dimensions and without the Nsig axis
    for a 1-D `x`.  Uses G.lmax."""
    dev = filters._device_graph_of(G)
    M = int(order) + 1
    on_device = [isinstance(a, engine.DeviceArray) for a in (x, z)]
    if any(on_device):
        if not all(on_device):
            raise TypeError("x and z must both be host arrays or both be DeviceArrays")
        n, nsig, nfeat = x.cube
        if nfeat != 1 or n != G.N:
            raise ValueError("cheby_cross_moments takes (N,) or (N, Nsig) signals, got a device array of cube {}"
                             .format(x.cube))
        if z.cube[:2] != (n, nsig):
            raise ValueError("z of cube {} does not match x of cube {}".format(z.cube, x.cube))
        for a in (x, z):
            if np.dtype(a.dtype) != np.dtype(dev.dtype):
                raise TypeError("the device array holds {}, the graph computes in {}".format(a.dtype,
                                                                                            np.dtype(dev.dtype)))
        one, bank = len(x.shape) == 1, z.cube[2] != 1 or len(z.shape) == 3
        m, ms = dev.cheby_cross_moments_dev(x.ptr, z.ptr, nsig, z.cube[2], G.lmax, M)
    else:
        x, z = np.asarray(x), np.asarray(z)
        if x.ndim not in (1, 2) or x.shape[0] != G.N:
            raise ValueError("cheby_cross_moments takes (N,) or (N, Nsig) signals, got {}".format(x.shape))
        one, bank = x.ndim == 1, z.ndim == 3
        x2 = x.reshape(G.N, -1)
        if z.ndim not in (1, 2, 3) or (z.shape[1:] if bank else z.shape[:1] + (z.size // max(G.N, 1),)) != x2.shape:
            raise ValueError("z must be (N,), (N, Nsig) or (Nf, N, Nsig) for x {}, got {}".format(x.shape, z.shape))
        m, ms = dev.cheby_cross_moments(x2, z.reshape((-1,) + x2.shape), G.lmax, M)
    filters._record_timing(G, ms)
    m = np.asarray(m, dtype=np.float64)
    if one:
        m = m[:, :, 0]
    return m if bank else m[0]


def probes(n_vertices, n_vectors, seed):
    """The random +-1 (Rademacher) probe vectors of the trace estimate, (n_vertices, n_vectors) float64."""
    return np.random.default_rng(seed).integers(0, 2, size=(n_vertices, n_vectors)) * 2.0 - 1.0


def jackson_damping(M):
    """The Jackson factors g_k, k < M, that make a truncated Chebyshev density non-negative (and its cdf monotone)."""
    k = np.arange(M)
    a = np.pi / (M + 1)
    return ((M - k + 1) * np.cos(a * k) + np.sin(a * k) / np.tan(a)) / (M + 1)


class SpectralDensity:
    """The density of states of a graph Laplacian from Chebyshev moments.

    `moments`: (M, n_vectors), column p the moments z_p^T T_k(Lt) z_p of probe p (cheby_moments); exact moments
    N mean_i T_k(2 e_i / lmax - 1) as one column work the same way.  `damping`: "jackson" or None.
    With theta = arccos(clip(2 lam / lmax - 1, -1, 1)) and c_k = g_k mu_k:
        cdf(lam) = c_0 (1 - theta / pi) - (2 / pi) sum_{k>=1} c_k sin(k theta) / k
        pdf(lam) = (2 / lmax) (c_0 + 2 sum_{k>=1} c_k cos(k theta)) / (pi sin(theta))"""

    def __init__(self, moments, lmax, n_vertices, damping="jackson"):
        m = np.asarray(moments, dtype=np.float64)
        if m.ndim == 1:
            m = m[:, None]
        if m.ndim != 2 or m.shape[0] < 2 or m.shape[1] < 1:
            raise ValueError("moments must be (M >= 2, n_vectors >= 1), got {}".format(m.shape))
        if damping not in ("jackson", None):
            raise ValueError("damping must be 'jackson' or None, got {!r}".format(damping))
        if not lmax > 0:
            raise ValueError("lmax must be positive, got {}".format(lmax))
        self.moments, self.lmax, self.n_vertices, self.damping = m, float(lmax), int(n_vertices), damping
        self.order = m.shape[0] - 1
        nv = m.shape[1]
        self.mu = m.mean(1) / self.n_vertices
        self.mu_stderr = m.std(1, ddof=1) / np.sqrt(nv) / self.n_vertices if nv > 1 else np.zeros(m.shape[0])
        self._g = jackson_damping(m.shape[0]) if damping == "jackson" else np.ones(m.shape[0])

    def _angles(self, lam):
        x = 2.0 * np.asarray(lam, dtype=np.float64) / self.lmax - 1.0
        return x, np.arccos(np.clip(x, -1.0, 1.0))

    def _cdf(self, lam, mu):
        """cdf at lam (any shape) for the columns of mu (M, P): lam.shape + (P,)"""
        x, theta = self._angles(lam)
        c = self._g[:, None] * mu
        k = np.arange(1, c.shape[0])
        series = (np.sin(theta[..., None] * k) / k) @ c[1:]
        out = c[0] * (1.0 - theta[..., None] / np.pi) - (2.0 / np.pi) * series
        return np.where((x <= -1.0)[..., None], 0.0, np.where((x >= 1.0)[..., None], c[0], out))

    def cdf(self, lam):
        """The estimated fraction of eigenvalues <= lam: 0 at and below 0, mu_0 at and above lmax."""
        out = self._cdf(lam, self.mu[:, None])[..., 0]
        return float(out) if out.ndim == 0 else out

    def pdf(self, lam):
        """The estimated density of eigenvalues per unit of lam (integrates to mu_0); 0 outside (0, lmax)."""
        x, theta = self._angles(lam)
        c = self._g * self.mu
        k = np.arange(1, c.shape[0])
        inside = (x > -1.0) & (x < 1.0)
        s = np.where(inside, np.sin(theta), 1.0)
        out = (2.0 / self.lmax) * (c[0] + 2.0 * (np.cos(theta[..., None] * k) @ c[1:])) / (np.pi * s)
        out = np.where(inside, out, 0.0)
        return float(out) if out.ndim == 0 else out

    def count(self, lo, hi, return_stderr=False):
        """The estimated number of eigenvalues in (lo, hi]: N (cdf(hi) - cdf(lo)); with return_stderr also the
        standard error across probes of the same expression evaluated per probe (0 for one probe)."""
        n = self.n_vertices * (self.cdf(hi) - self.cdf(lo))
        if not return_stderr:
            return n
        per = self._cdf(hi, self.moments / self.n_vertices) - self._cdf(lo, self.moments / self.n_vertices)
        nv = per.shape[-1]
        err = self.n_vertices * per.std(-1, ddof=1) / np.sqrt(nv) if nv > 1 else np.zeros(per.shape[:-1])
        return n, (float(err) if np.ndim(err) == 0 else err)

    def quantile(self, q):
        """The lam at which cdf(lam) = q, by bisection on [0, lmax].  Needs Jackson damping: only then is the cdf
        monotone."""
        if self.damping != "jackson":
            raise ValueError("quantile needs damping='jackson': an undamped cdf is not monotone")
        q = np.asarray(q, dtype=np.float64)
        lo, hi = np.zeros(q.shape), np.full(q.shape, self.lmax)
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            below = self._cdf(mid, self.mu[:, None])[..., 0] < q
            lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
        out = 0.5 * (lo + hi)
        return float(out) if out.ndim == 0 else out


def estimate_spectral_density(G, order=100, n_vectors=32, seed=0, damping="jackson"):
    """SpectralDensity of G's Laplacian from `n_vectors` probes and order + 1 moments: the probes are built on the
    host and uploaded once in the graph's compute dtype, then one cheby_moments call."""
    z = probes(G.N, int(n_vectors), seed)
    return SpectralDensity(cheby_moments(G, z, order), G.lmax, G.N, damping)
