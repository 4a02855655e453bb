"""Clustering on the device: k-means on a row-major fp64 panel, spectral embeddings, spectral clustering.

``kmeans`` runs Lloyd's iteration and k-means++ seeding in the kernels of csrc/gspx_cluster.hip.h: no atomics, every
sum in one fixed order, the same bits on every call.  ``kmeans_host`` is the numpy restatement of both device
algorithms, sum for sum and tie for tie (as reduction.coarsen_host restates the coarsening): the GPU tests compare the
two exactly.  ``spectral_embedding`` gives the rows to cluster - the first k Fourier modes, or low-pass-filtered random
signals (compressive spectral clustering: Tremblay, Puy, Gribonval, Vandergheynst, ICML 2016) - and
``spectral_clustering`` chains embedding, row normalisation and k-means without the panel leaving the device.

The orders of summation:
  distance   acc = acc + (x_j - c_j) * (x_j - c_j), j = 0 .. d - 1, no FMA; argmin over c with strict <, so ties go
             to the smaller index
  inertia    per workgroup of assign_rows(d) rows the halving tree v[i] += v[i + h], then the workgroup partials by
             64 lanes (lane l adds partials l, l + 64, ... in order) and the halving tree over the lanes
  update     part[b][c] = the members of cluster c among rows [b R, (b + 1) R), R = update_rows(), added in
             increasing row from +0; the centroid = (the parts added in increasing b) / count; an empty cluster keeps
             its centroid
  seeding    D2 = min(D2, distance to the new centre); block sums of R values by the halving tree; the host walks the
             block sums, then the chosen block's rows, sequentially (seed_host states the rule)

A real pygsp graph works through filters._device_graph_of / the plugin's float64 device graph, as elsewhere; there is
no plugin.install flag, because the reference has no clustering function to patch.

Out of scope: the vertex-subsampling and Tikhonov-interpolation stage of the compressive paper (k-means on all N rows
is cheap here); fp32; a matrix-core distance ||x||^2 - 2 x.c + ||c||^2, which cannot be restated bit for bit; k-means
with n_clusters * d > 8192 (the limit the kernels' LDS images are sized for); a Graph method."""
import ctypes

import numpy as np

from . import _capi, engine

MAX_D, MAX_C, MAX_CD = 128, 1024, 8192


UPDATE_ROWS = 1024  # KM_ROWS of csrc/gspx_cluster.hip.h


def update_rows():
    """Rows per block of the update's and the seeding's partial sums: a constant of the library
    (gspx_kmeans_block_rows reports the same number; tests/test_cluster_host.py holds the two together)."""
    return UPDATE_ROWS


def assign_rows(d):
    """Rows per workgroup of the assignment kernel (its partial inertia is summed per workgroup): 256 over the lanes
    per row, 1, 2 or 4 for d <= 32, <= 64, <= 128 - a function of d alone, as gspx_kmeans_block_rows reports it."""
    return 256 // (1 if d <= 32 else 2 if d <= 64 else 4)


def library_block_rows(d):
    """(update rows, assignment rows) as the library states them (gspx_kmeans_block_rows; needs no device)."""
    up, asg = ctypes.c_int(0), ctypes.c_int(0)
    _capi.check(_capi.load().gspx_kmeans_block_rows(int(d), ctypes.byref(up), ctypes.byref(asg)))
    return up.value, asg.value


class KMeansResult:
    """labels (int32, N), centers (float64, C x d), inertia (the sum of the rows' squared distances to their
    centres), n_iter (updates made), converged (no label changed in the last assignment), seeds (the rows k-means++
    chose, or None for a given init), kernel_ms (device time of the run kept)."""

    def __init__(self, labels, centers, inertia, n_iter, converged, seeds=None, kernel_ms=0.0):
        self.labels, self.centers, self.inertia = labels, centers, float(inertia)
        self.n_iter, self.converged, self.seeds, self.kernel_ms = int(n_iter), bool(converged), seeds, float(kernel_ms)

    def __repr__(self):
        return "KMeansResult(n_clusters={}, inertia={!r}, n_iter={}, converged={})".format(
            len(self.centers), self.inertia, self.n_iter, self.converged)


def _check(N, d, C, init):
    """The limits of the library, checked before anything is uploaded; returns the init array or the seeding's name."""
    if N < 1:
        raise ValueError("kmeans: needs at least one row, got N = {}".format(N))
    if not 1 <= d <= MAX_D:
        raise ValueError("kmeans: 1 <= d <= {} columns, got {}".format(MAX_D, d))
    if not 1 <= C <= min(N, MAX_C):
        raise ValueError("kmeans: 1 <= n_clusters <= min(N, {}), got {} (N = {})".format(MAX_C, C, N))
    if C * d > MAX_CD:
        raise ValueError("kmeans: n_clusters * d <= {} (64 KiB of centroids), got {} * {}"
                         .format(MAX_CD, C, d))
    if isinstance(init, str):
        if init != "k-means++":
            raise ValueError("kmeans: init must be 'k-means++' or a (n_clusters, d) array, got {!r}".format(init))
        return init
    init = np.ascontiguousarray(init, dtype=np.float64)
    if init.shape != (C, d):
        raise ValueError("kmeans: init must have shape ({}, {}), got {}".format(C, d, init.shape))
    return init


# ---- the numpy restatement ----------------------------------------------------------------------------------------
def _tree(v):
    """The halving tree v[i] += v[i + h], h = n / 2 ... 1, along the last axis (a power of two long)."""
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = v[..., :h] + v[..., h:]
    return v[..., 0]


def _blocks(v, rows):
    """v cut into blocks of `rows`, zeros after the end."""
    nb = -(-v.size // rows)
    out = np.zeros(nb * rows)
    out[:v.size] = v
    return out.reshape(nb, rows)


def _sqdist(X, c):
    acc = np.zeros(X.shape[0])
    for j in range(X.shape[1]):
        t = X[:, j] - c[j]
        acc = acc + t * t
    return acc


def assign_host(X, centers):
    """(labels int32, each row's squared distance to its centre, inertia): the assignment kernel and its sums."""
    N, d = X.shape
    best, labels = np.full(N, np.inf), np.zeros(N, dtype=np.int32)
    for c in range(centers.shape[0]):
        dist = _sqdist(X, centers[c])
        closer = dist < best
        best[closer], labels[closer] = dist[closer], c
    partials = _tree(_blocks(best, assign_rows(d)))
    lanes = np.zeros(64)
    for chunk in _blocks(partials, 64):
        lanes = lanes + chunk
    return labels, best, float(_tree(lanes))


def update_host(X, labels, centers):
    """The centroids after one update: the update kernels' partial sums and their second pass."""
    N, d = X.shape
    C, R = centers.shape[0], update_rows()
    nb = -(-N // R)
    part = np.zeros((nb, C, d))
    np.add.at(part, (np.arange(N) // R, labels), X)  # (unbuffered: in increasing row)
    total = np.zeros((C, d))
    for b in range(nb):
        total = total + part[b]
    count = np.bincount(labels, minlength=C)
    out = centers.copy()
    has = count > 0
    out[has] = total[has] / count[has, None]
    return out


def lloyd_host(X, centers, max_iter=100):
    """Lloyd's iteration as gspx_kmeans_dev runs it: assign; converged when no label changed (the first assignment
    counts every row); unconverged when max_iter updates have been made; else update and repeat."""
    centers = np.array(centers, dtype=np.float64)
    labels, n_iter = None, 0
    while True:
        new, _, inertia = assign_host(X, centers)
        changed = X.shape[0] if labels is None else int(np.count_nonzero(new != labels))
        labels = new
        if changed == 0 or n_iter == max_iter:
            return KMeansResult(labels, centers, inertia, n_iter, changed == 0)
        centers = update_host(X, labels, centers)
        n_iter += 1


def seed_host(X, n_clusters, u):
    """k-means++ from the draws u (n_clusters of them in [0, 1)): the chosen rows, as gspx_kmeans_seed_dev picks them.

    Centre 0 is row floor(u_0 N).  For centre c >= 1, with D2 the squared distance to the nearest centre so far and
    s_b the block sums of D2 (blocks of update_rows() rows, halving tree): run = 0, run += s_b in increasing b, total
    the final run.  total == 0: the smallest row index not chosen yet.  Otherwise target = u_c total; the block is the
    first whose run exceeds target or, if rounding lets none exceed it, the last with s_b > 0; t = target - (the run
    before that block); inside the block run = 0, run += D2[i] in increasing i, and the row is the first whose run
    exceeds t or, if none does, the block's last row with D2 > 0."""
    N, R = X.shape[0], update_rows()
    chosen, D2 = [], None
    for c in range(n_clusters):
        if c == 0:
            pick = min(N - 1, int(u[0] * float(N)))
        else:
            dist = _sqdist(X, X[chosen[-1]])
            D2 = dist if D2 is None else np.where(dist < D2, dist, D2)
            sums = _tree(_blocks(D2, R))
            run = np.zeros(sums.size + 1)
            for b in range(sums.size):
                run[b + 1] = run[b] + sums[b]
            total = run[-1]
            if not total > 0.0:
                pick = next(i for i in range(N) if i not in chosen)
            else:
                target = u[c] * total
                over = np.nonzero(run[1:] > target)[0]
                blk = int(over[0]) if over.size else int(np.nonzero(sums > 0.0)[0][-1])
                t = target - run[blk]
                rows = D2[blk * R:(blk + 1) * R]
                inner = np.zeros(rows.size + 1)
                for i in range(rows.size):
                    inner[i + 1] = inner[i] + rows[i]
                over = np.nonzero(inner[1:] > t)[0]
                pick = blk * R + (int(over[0]) if over.size else int(np.nonzero(rows > 0.0)[0][-1]))
        chosen.append(pick)
    return np.array(chosen, dtype=np.int64)


def rows_normalize_host(X):
    """Each row divided by the square root of acc = acc + x_j * x_j; a zero row stays."""
    X = np.asarray(X, dtype=np.float64)
    acc = np.zeros(X.shape[0])
    for j in range(X.shape[1]):
        acc = acc + X[:, j] * X[:, j]
    nrm = np.sqrt(acc)
    out = X.copy()
    has = nrm > 0.0
    out[has] = X[has] / nrm[has, None]
    return out


def _runs(C, init, n_init, seed):
    """The draws of every run: one run without draws for a given init, else n_init runs of C draws each."""
    if not isinstance(init, str):
        return [None]
    if n_init < 1:
        raise ValueError("kmeans: n_init must be at least 1")
    rng = np.random.default_rng(seed)
    return [rng.random(C) for _ in range(int(n_init))]


def kmeans_host(X, n_clusters, *, init="k-means++", n_init=1, max_iter=100, seed=0, normalize_rows=False):
    """kmeans in numpy: the restatement of the device algorithms (same arguments, same result, bit for bit)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("kmeans: X must be (N, d), got {}".format(X.shape))
    C = int(n_clusters)
    init = _check(X.shape[0], X.shape[1], C, init)
    if normalize_rows:
        X = rows_normalize_host(X)
    best = None
    for u in _runs(C, init, n_init, seed):
        seeds = None if u is None else seed_host(X, C, u)
        res = lloyd_host(X, init if u is None else X[seeds], max_iter)
        res.seeds = seeds
        if best is None or res.inertia < best.inertia:
            best = res
    return best


# ---- the device ---------------------------------------------------------------------------------------------------
def rows_normalize_dev(ctx, ptr, N, d, ld=None):
    """gspx_rows_normalize_dev on a device pointer, in place.  Returns the kernel ms."""
    ms = ctypes.c_double(0)
    ctx.call(_capi.load().gspx_rows_normalize_dev, ctx._h, int(N), int(d), ctypes.c_void_p(ptr),
             int(d if ld is None else ld), ctypes.byref(ms))
    return ms.value


def _panel_of(X, ctx, n_clusters, init):
    """(ctx, device pointer, N, d, pitch, owner to keep alive, whether the memory is ours to overwrite) of X: an
    engine.DeviceArray (N, d), or a host array, uploaded."""
    if isinstance(X, engine.DeviceArray):
        N, d, F = X.cube
        if F != 1 or len(X.shape) > 2:
            raise ValueError("kmeans: a device array must be (N, d), got cube {}".format(X.cube))
        if X.dtype != np.float64:
            raise TypeError("kmeans computes in float64, the device array holds {}".format(X.dtype))
        if ctx is not None and ctx is not X.ctx:
            raise ValueError("kmeans: the device array lives on another context")
        _check(N, d, n_clusters, init)
        return X.ctx, X.ptr, N, d, d, X, False
    A = np.ascontiguousarray(X, dtype=np.float64)
    if A.ndim != 2:
        raise ValueError("kmeans: X must be (N, d), got {}".format(A.shape))
    _check(A.shape[0], A.shape[1], n_clusters, init)  # (before a context is made and anything is uploaded)
    ctx = ctx or engine.default_context()
    dev = engine.DeviceArray.from_host(ctx, A)
    return ctx, dev.ptr, A.shape[0], A.shape[1], A.shape[1], dev, True


def kmeans_dev(ctx, ptr, N, d, ld, n_clusters, *, init="k-means++", n_init=1, max_iter=100, seed=0):
    """kmeans on a device pointer (row-major N x d doubles, pitch ld): labels and centres are the only downloads."""
    lib, C = _capi.load(), int(n_clusters)
    init = _check(N, d, C, init)
    best = None
    with ctx._temporaries() as t:
        cent = t.alloc(C * d * 8)
        labels = [t.alloc(N * 4), t.alloc(N * 4)]
        for u in _runs(C, init, n_init, seed):
            seeds, ms0 = None, ctypes.c_double(0)
            if u is None:
                cent.upload(init)
            else:
                seeds = np.zeros(C, dtype=np.int64)
                ctx.call(lib.gspx_kmeans_seed_dev, ctx._h, N, d, C, ctypes.c_void_p(ptr), ld,
                         _capi.ptr(np.ascontiguousarray(u, dtype=np.float64)), ctypes.c_void_p(cent.ptr),
                         _capi.ptr(seeds), ctypes.byref(ms0))
            inertia, n_iter, conv, ms = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_double(0)
            ctx.call(lib.gspx_kmeans_dev, ctx._h, N, d, C, ctypes.c_void_p(ptr), ld, ctypes.c_void_p(cent.ptr),
                     int(max_iter), ctypes.c_void_p(labels[0].ptr), None, ctypes.byref(inertia), ctypes.byref(n_iter),
                     ctypes.byref(conv), ctypes.byref(ms))
            if best is None or inertia.value < best.inertia:
                best = KMeansResult(None, cent.download((C, d), np.float64), inertia.value, n_iter.value, conv.value,
                                    seeds, ms0.value + ms.value)
                labels.reverse()  # (the kept run's labels stay in labels[1])
        best.labels = labels[1].download((N,), np.int32)
    return best


def kmeans(X, n_clusters, *, init="k-means++", n_init=1, max_iter=100, seed=0, normalize_rows=False, ctx=None):
    """k-means of the rows of X into n_clusters clusters, on the device.

    X: a numpy array or an engine.DeviceArray, (N, d) - a device array is clustered where it lies, and only the
    labels and the centres come back.  init: 'k-means++' (draws from np.random.default_rng(seed), n_clusters per run)
    or a (n_clusters, d) array.  n_init runs are made and the one of lowest inertia is returned, ties to the earlier
    run.  normalize_rows: the rows are divided by their norms first (a device array is copied for that, not changed).
    Limits: d <= 128, n_clusters <= min(N, 1024), n_clusters * d <= 8192; ValueError otherwise.
    Returns a KMeansResult."""
    ctx, ptr, N, d, ld, keep, ours = _panel_of(X, ctx, int(n_clusters), init)
    try:
        if normalize_rows:
            if not ours:
                from . import fourier
                copy = engine.DeviceArray.empty(ctx, (N, d, 1), np.float64)
                fourier.panel_copy(ctx, N, ptr, ld, d, copy.ptr, d)
                keep, ptr, ld, ours = copy, copy.ptr, d, True
            rows_normalize_dev(ctx, ptr, N, d, ld)
        return kmeans_dev(ctx, ptr, N, d, ld, n_clusters, init=init, n_init=n_init, max_iter=max_iter, seed=seed)
    finally:
        if ours:  # (the upload or the normalised copy; the caller's own array stays)
            keep.free()


# ---- spectral embeddings ------------------------------------------------------------------------------------------
def default_n_features(n_vertices):
    """Columns of the compressive embedding: min(128, ceil(4 ln N))."""
    return int(min(MAX_D, max(1, np.ceil(4.0 * np.log(n_vertices)))))


def random_signals(n_vertices, n_features, seed=0):
    """The compressive embedding's input: (N, d) Gaussian columns / sqrt(d) from np.random.default_rng(seed)."""
    return np.random.default_rng(seed).standard_normal((int(n_vertices), int(n_features))) / np.sqrt(n_features)


def lambda_k_of(density, n_clusters):
    """The cut of the low-pass from a spectrum.SpectralDensity: half way between the k / N and (k + 1) / N quantiles."""
    N, k = density.n_vertices, int(n_clusters)
    return 0.5 * (density.quantile(k / N) + density.quantile((k + 1) / N))


def lowpass_coefficients(lambda_k, lmax, order=50):
    """Jackson-Chebyshev coefficients of the ideal low-pass [0, lambda_k] on [0, lmax] (order + 1 of them)."""
    from . import filters
    return filters.compute_jackson_cheby_coeff([0.0, float(lambda_k)], [0.0, float(lmax)], int(order))[1]


def spectral_embedding(G, n_clusters, features="fourier", *, n_features=None, order=50, lambda_k=None, seed=0,
                       density_order=100, n_vectors=32):
    """The rows spectral clustering clusters: an engine.DeviceArray (N, d) on G's float64 device graph's context,
    with attributes `kind` and `lambda_k`.

    'fourier': d = n_clusters, a copy of the first n_clusters columns of G's partial Fourier basis on the device -
    computed (G.compute_fourier_basis(n_clusters)) if G has none that wide, left as it is otherwise.
    'compressive': d = n_features (None: min(128, ceil(4 ln N))) Gaussian columns / sqrt(d) from
    np.random.default_rng(seed), filtered on the device by the Jackson-Chebyshev low-pass [0, lambda_k] of `order`.
    lambda_k None: 0.5 (q(k / N) + q((k + 1) / N)), q the quantile of G.estimate_spectral_density(density_order,
    n_vectors, seed)."""
    from . import filters, fourier, spectrum
    k = int(n_clusters)
    dev = engine._float64_device_graph(G)
    N, ctx = dev.N, dev.ctx
    if not 1 <= k <= N:
        raise ValueError("n_clusters must be in 1..{}, got {}".format(N, n_clusters))
    if features == "fourier":
        if getattr(G, "_U", None) is None or G._U.shape[1] < k:
            G.compute_fourier_basis(n_eigenvectors=k)
        if hasattr(G, "_basis_on_device"):
            _, panel = G._basis_on_device()
            out = engine.DeviceArray.empty(ctx, (N, k, 1), np.float64)
            fourier.panel_copy(ctx, N, panel.ptr, panel.ld, k, out.ptr, k)
        else:  # a reference graph keeps its basis on the host
            out = engine.DeviceArray.from_host(ctx, np.ascontiguousarray(G.U[:, :k]))
        out.shape = (N, k)
        out.kind, out.lambda_k = "fourier", None
        return out
    if features != "compressive":
        raise ValueError("features must be 'fourier' or 'compressive', got {!r}".format(features))
    d = default_n_features(N) if n_features is None else int(n_features)
    if not 1 <= d <= MAX_D:
        raise ValueError("n_features must be in 1..{}, got {}".format(MAX_D, d))
    if lambda_k is None:
        lambda_k = lambda_k_of(spectrum.estimate_spectral_density(G, density_order, n_vectors, seed), k)
    coeffs = lowpass_coefficients(lambda_k, G.lmax, order)
    x = engine.DeviceArray.from_host(ctx, random_signals(N, d, seed))
    out = engine.DeviceArray.empty(ctx, (N, d, 1), np.float64)
    try:
        ms = dev.cheby_filter_dev(coeffs[np.newaxis, :], x.ptr, out.ptr, d, G.lmax, _capi.ANALYSIS)
    finally:
        x.free()
    filters._record_timing(G, ms)
    out.shape = (N, d)
    out.kind, out.lambda_k = "compressive", float(lambda_k)
    return out


def choose_features(G, n_clusters):
    """The rule of spectral_clustering(features='auto')."""
    from . import fourier
    k, N = int(n_clusters), G.N
    have = getattr(G, "_U", None)
    if have is not None and have.shape[1] >= k:
        return "fourier"
    if k * k > MAX_CD:
        return "compressive"
    if N < fourier.AUTO_MIN_VERTICES or fourier.use_device(N, k):
        return "fourier"
    return "compressive"


_EMBEDDING_KEYS = ("n_features", "order", "lambda_k", "density_order", "n_vectors")


def spectral_clustering(G, n_clusters, features="auto", **kw):
    """Spectral clustering of G's vertices: spectral_embedding, row normalisation and kmeans, the panel on the device
    throughout.  Keywords: those of spectral_embedding and of kmeans (`seed` serves both).  Returns the KMeansResult
    with `features` (the kind used) and `lambda_k` (None for 'fourier') attached.

    features='auto' is 'fourier' when G already holds a basis of at least n_clusters columns; otherwise
    'compressive' when n_clusters^2 > 8192 (k-means could not take the Fourier rows); otherwise 'fourier' when
    N < 2048 (the dense host solver is cheap) or fourier.use_device(N, n_clusters) (the device solver takes it);
    otherwise 'compressive'."""
    engine._refuse_unknown_keywords("spectral_clustering", kw, _EMBEDDING_KEYS + ("init", "n_init", "max_iter", "seed"))
    kind = choose_features(G, n_clusters) if features == "auto" else features
    emb = {key: kw[key] for key in _EMBEDDING_KEYS if key in kw}
    F = spectral_embedding(G, n_clusters, kind, seed=kw.get("seed", 0), **emb)
    try:
        N, d = F.shape
        rows_normalize_dev(F.ctx, F.ptr, N, d)
        out = kmeans(F, n_clusters, **{key: kw[key] for key in ("init", "n_init", "max_iter", "seed") if key in kw})
        out.features, out.lambda_k = kind, F.lambda_k
        return out
    finally:
        F.free()
