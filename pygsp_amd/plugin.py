"""Drop-in for the real pygsp: route ``Filter.filter(method='chebyshev')`` through libgspx.

PyGSP has no plugin / FFI interface; the seam is Python attribute lookup:
``pygsp/filters/filter.py:309,319`` call ``approximations.cheby_op`` looked up on the module at
call time, and ``pygsp/filters/__init__.py:115`` re-exports it at import time.  ``install()``
replaces both with ``pygsp_amd.filters.cheby_op``; ``uninstall()`` restores the originals.

    import pygsp, pygsp_amd.plugin
    pygsp_amd.plugin.install()                  # from here on Chebyshev filtering runs on MI355X
    g = pygsp.filters.Heat(G, 50); y = g.filter(s, method='chebyshev', order=30)
"""
import numpy as np
from scipy import sparse

from . import engine, filters as _filters

import threading

# The originals of everything install() replaces are kept ON the patched object itself (attribute _gspx_saved of
# every module and class in _targets(): name -> the package's own attribute), so that two pygsp-shaped modules can be
# patched and restored independently (one global table restored the first module's functions into the
# second).
_SAVED = "_gspx_saved"
_MISSING = object()  # saved for a name the package does not have (an alias, lanczos_op): nothing to put back
_installed = {}  # id(module) -> module, in installation order (uninstall() without an argument: the last one)
_config = {"laplacian": "device", "dtype": np.float64, "device": 0, "reorder": "auto", "tiles": "auto",
           "devices": None, "evaluation": None}
_cache_lock = threading.RLock()


def _finite_coords(G):
    try:
        coords = np.asarray(getattr(G, "coords", None), dtype=np.float64)
    except (TypeError, ValueError):
        return None
    if not engine._curve_coords(coords, G.N) or not np.isfinite(coords).all():
        return None  # plotting layouts may hold NaN / inf, a 1-D cloud has no curve: the pattern-based order
    return coords


def device_graph_for(G, ctx=None, dtype=None):
    """libgspx graph attached to a reference ``pygsp.graphs.Graph``: cached on the object next to the
    very ``G.L`` (and ``G.W``) it was built from, and rebuilt when ``G.compute_laplacian`` replaced
    them, mirroring graph.py:602-609.  The cache entry holds the matrices themselves and compares with
    ``is`` - an ``id()`` alone could be recycled by a later matrix.  One entry per context (`ctx`: the
    context of the configured device unless given - the replicas of a device list, pygsp_amd.multi).
    A stale entry is dropped, not destroyed: whoever still holds the old DeviceGraph (another thread in the
    middle of a filter call, a caller that kept the return value) keeps a live handle, and the device memory
    goes when the last reference does (DeviceGraph.__del__)."""
    dtype = np.dtype(dtype or _config["dtype"])
    conf = (G.lap_type, dtype.str, _config["laplacian"], _config["reorder"], bool(_config.get("tiles", "auto")))
    ctx = ctx or engine.default_context(_config["device"])
    key = (id(ctx), dtype.str)
    with _cache_lock:
        cache = G.__dict__.setdefault("_gspx_dev", {})
        cached = cache.get(key)
        if (cached is not None and cached[0] is G.L and cached[1] is G.W and cached[2] == conf
                and cached[4] is ctx and getattr(cached[3], "_h", None)):
            return cached[3]
        dev = None
        coords = _finite_coords(G)
        order = _config["reorder"]
        if order == "auto" and coords is None and G.N >= 4096 and sparse.isspmatrix_csr(G.W) and engine.expander_like(G.W):
            order = "none"  # a random-like graph (ER / SBM): no order helps, skip reverse Cuthill-McKee
        one_call = (_config["laplacian"] == "device" and sparse.isspmatrix_csr(G.W) and order in ("auto", "none", None, False)
                    and not (order == "auto" and coords is None and G.N >= 4096))  # (no coordinates: RCM is host work)
        if one_call:
            # checks, directedness, (W + W.T) / 2 of a directed graph, vertex order and Laplacian in one device call on
            # the uploaded G.W (gspx_graph_setup)
            try:
                dev, _ = engine.DeviceGraph.setup(G.W, G.lap_type, dtype, coords, order, ctx=ctx)
            except ValueError:
                dev = None
        if dev is None:
            perm = None
            if order == "auto" and G.N >= 4096:
                perm = engine.auto_order(G.W, coords, ctx=ctx)
            elif order == "rcm":
                perm = engine.locality_order(G.W, None)
            if _config["laplacian"] == "device":
                W = G.W if not G.is_directed() else sparse.csr_matrix((G.W + G.W.T) / 2)
                dev = engine.DeviceGraph.from_w(W, G.lap_type, dtype=dtype, perm=perm, ctx=ctx)
            else:  # bit-parity mode: upload the Laplacian the reference built
                dev = engine.DeviceGraph.from_l(G.L, dtype=dtype, perm=perm, ctx=ctx)
        if _config.get("tiles", "auto"):
            dev.auto_gather_tiles()
        cache[key] = (G.L, G.W, conf, dev, ctx)
        return dev


def _estimate_lmax_on_device(self, method="lanczos"):
    """``Graph.estimate_lmax`` of the reference (graph.py:858-931) with its 'lanczos' branch on the device: the
    ARPACK call of graph.py:911-917 (3.3 s at N = 1M, random start vector) becomes gspx_lanczos_lmax on the
    graph's device Laplacian (milliseconds, deterministic).  Same contract - a Ritz value from below, checked
    against the upper bound, increased by 1 % (graph.py:919-920), ValueError when it does not converge - and the
    same caching through ``_lmax_method``; every other method is the reference's own code."""
    if method != "lanczos":
        return _saved_on(type(self))["estimate_lmax"](self, method)
    if method == self._lmax_method:
        return
    ritz = _lanczos_ritz(device_graph_for(self, dtype=np.float64))
    if not ritz <= self._get_upper_bound() * (1 + 1e-6) + 1e-12:  # graph.py:919 (an assert there)
        raise ValueError("The Lanczos estimate {} exceeds the upper bound of lambda_max.".format(ritz))
    self._lmax_method = method
    self._lmax = ritz * 1.01


def _lanczos_ritz(dev):
    """Largest Ritz value of the float64 device Laplacian; a second, longer run before giving up (the
    reference's ARPACK call stops at tol 5e-3, graph.py:911-917: where it succeeds this must not fail)."""
    try:
        return dev.lanczos_lmax(max_iter=80, tol=5e-4)[0]
    except ValueError:
        return dev.lanczos_lmax(max_iter=400, tol=5e-3)[0]


def to_device(G, s):
    """Upload a signal of a reference ``pygsp.graphs.Graph`` once and keep it on the device (engine.DeviceArray):
    with install(wrap_filter=True) the real ``Filter.filter`` / ``analyze`` / ``synthesize`` take it and return
    one, so a chain of filters costs one upload and one download (``np.asarray(result)``)."""
    arr = G._check_signal(s)
    dev = device_graph_for(G)
    return engine.DeviceArray.from_host(dev.ctx, arr, dev.dtype)


def tune_placement(bank, n_signals, order=30, candidates=32, stride_mb=8000):
    """Placement tuning (filters.tune_placement) for a real ``pygsp.filters.Filter`` of one kernel after install():
    its own compute_cheby_coeff, the graph's device Laplacian on the configured context."""
    return _filters.tune_placement(bank, n_signals, order, candidates, _reference_coefficients, stride_mb)


def _saved_on(cls):
    """The originals saved on the patched class `cls` derives from (or is)."""
    for k in cls.__mro__:
        saved = k.__dict__.get(_SAVED)
        if saved is not None:
            return saved
    raise RuntimeError("pygsp_amd.plugin: {} is not a patched class".format(cls.__name__))


def _reference_coefficients(bank, m):
    # the coefficients of the bank's own package (approximations.py:9-55): its own code, its own kernels
    for mod in list(_installed.values()):  # (the patched package whose wrapped Filter class the bank derives from)
        filter_cls = getattr(mod.filters, "Filter", None)
        if filter_cls in type(bank).__mro__ and _SAVED in vars(filter_cls):
            return mod.filters.approximations.compute_cheby_coeff(bank, m=m)
    raise RuntimeError("pygsp_amd.plugin: {} is not a patched class".format(type(bank).__name__))


def basis_on_device_for(G):
    """(float64 DeviceGraph, fourier.DevicePanel of U) attached to a reference ``pygsp.graphs.Graph``: U uploaded once
    and cached on the object next to the very ``G.U`` it was copied from (compared with ``is``, as device_graph_for
    does for L), so a recomputed basis is uploaded again."""
    from . import fourier
    dev = device_graph_for(G, dtype=np.float64)
    with _cache_lock:
        held = G.__dict__.get("_gspx_basis")
        if held is not None and held[0] is G.U and held[1] is dev and held[2].buf is not None:
            return dev, held[2]
        if held is not None and held[2].buf is not None:
            held[2].buf.free()
        panel = fourier.DeviceBackend(dev, 1.0).from_host(np.ascontiguousarray(G.U, dtype=np.float64))
        G.__dict__["_gspx_basis"] = (G.U, dev, panel)
        return dev, panel


def _filter_exact_on_device(self, s, method="chebyshev", order=30):
    """What install(exact=True) puts in place of ``Filter.filter``: _filter_on_device whose method='exact' branch
    (filter.py:292-301) also runs on the device (filters.filter_signals: one Gram, one spectral apply against the
    device copy of ``G.U``).  ``Gabor.filter`` calls this through ``super()`` and follows."""
    if method == "exact":
        return _filters.filter_signals(self, s, method, order, None, _reference_coefficients)
    return _filter_on_device(self, s, method, order)


def _modulation_on_device(self, s, method="exact", order=None):
    """``Modulation.filter`` (modulation.py:164-177) on the device: modulation first is the exact path of the wrapped
    ``Filter.filter``; localisation first, the reference's loop over the vertices, is filters.modulation_localized
    (identity-panel Chebyshev filter, then one Gram per panel)."""
    if self._modulation_first:
        return _filters.filter_signals(self, s, "exact", order, None, _reference_coefficients)
    return _filters.modulation_localized(self, s, coefficients=_reference_coefficients)


def _filter_on_device(self, s, method="chebyshev", order=30):
    """``pygsp.filters.Filter.filter`` (filter.py:146-328) with its Chebyshev branch in one device call: the shape
    rules are the reference's (filters._cube_shape restates filter.py:267-290), analysis is the call the
    reference makes, synthesis is ONE vector-coefficient recurrence on the device instead of the loop of
    filter.py:318-321 (Nf cheby_op calls, each with its own host round trip), and a DeviceArray stays on the
    device.  Everything else (method='exact', unknown methods) is the reference's own code."""
    if method != "chebyshev":
        return _saved_on(type(self))["filter"](self, s, method=method, order=order)
    return _filters.filter_signals(self, s, method, order, None, _reference_coefficients)


def _compute_frame_on_device(self, **kwargs):
    """``Filter.compute_frame`` (filter.py:506-600) without its N x N host identity: the deltas are written on
    the device panel by panel (filters.frame_panels); same (Nf N, N) result.  Other methods, and graphs whose
    size collides with the shape rules (N in {1, Nf}: the identity then reads as a synthesis input,
    filter.py:270), run the reference's own code."""
    extra = set(kwargs) - {"method", "order"}
    if kwargs.get("method", "chebyshev") != "chebyshev" or extra or self.G.N in (1, self.Nf):
        return _saved_on(type(self))["compute_frame"](self, **kwargs)
    if self.G.N > 2000:  # filter.py:593-596
        _filters_logger(self).warning("Creating a big matrix. You should prefer the filter method.")
    return _filters.frame_panels(self, kwargs.get("order", 30), coefficients=_reference_coefficients)


def _filters_logger(bank):
    import logging
    return logging.getLogger(type(bank).__module__)


# install(full_basis=True): full requests of graphs this large go to the device.  The measured crossover against the
# host's eigh (profiles/eigh.md: host / device 0.73 at 1024 vertices, 1.57 at 2048)
FULL_BASIS_MIN_VERTICES = 2048


def _compute_full_basis_on_device(self, n_eigenvectors=None):
    """What install(fourier=True, full_basis=True) puts in place of ``Graph.compute_fourier_basis``: a request for
    all N vectors of a graph of at least FULL_BASIS_MIN_VERTICES vertices runs block Jacobi on the float64 device
    Laplacian (pygsp_amd.fourier.device_full_basis) instead of scipy's eigh, with the reference's bookkeeping
    (fourier.py:156-195: a cached basis is kept, ``_e``, ``_U``, e[0] checked and set to zero, ``_lmax`` = e[-1]).  The
    solver's N x N panel is cached where basis_on_device_for looks, so ``filter(method='exact')`` under
    install(exact=True) uploads nothing.  Partial requests follow install(fourier=True); smaller graphs run the
    package's own code."""
    from . import fourier
    n = self.n_vertices if n_eigenvectors is None else int(n_eigenvectors)
    if n != self.n_vertices or n < FULL_BASIS_MIN_VERTICES:
        return _compute_fourier_basis_on_device(self, n_eigenvectors)
    if self._U is not None and n <= len(self._e):
        return
    dev = device_graph_for(self, dtype=np.float64)
    e, U, U_dev, _ = fourier.device_full_basis(dev)
    fourier.finish_partial(e, U)  # (e[0] within 1e-5 of zero, then zero; the signs are set already)
    self._e, self._U = e, U
    self._lmax, self._lmax_method = e[-1], "fourier"
    self._coherence = np.max(np.abs(U))
    with _cache_lock:
        held = self.__dict__.get("_gspx_basis")
        if held is not None and held[2].buf is not None:
            held[2].buf.free()
        self.__dict__["_gspx_basis"] = (U, dev, U_dev)


def _compute_fourier_basis_on_device(self, n_eigenvectors=None):
    """``Graph.compute_fourier_basis`` of the reference (fourier.py:97-195) with its partial branch on the device: a
    request for k < N vectors that pygsp_amd.fourier.use_device sends there (N >= 2048, a block of at most N / 4) runs
    Chebyshev-filtered subspace iteration on the graph's float64 device Laplacian instead of ARPACK
    (eigsh(L, k, which='SM'), fourier.py:174-175) and is stored in ``_e`` / ``_U``; a cached basis of at least k
    vectors is kept (fourier.py:156).  Everything else - full bases, small graphs - is the reference's own code."""
    from . import fourier
    n = self.n_vertices if n_eigenvectors is None else int(n_eigenvectors)
    if 1 <= n < self.n_vertices and fourier.use_device(self.n_vertices, n):
        if self._U is not None and n <= len(self._e):
            return
        e, U, U_dev, _ = fourier.device_partial_basis(device_graph_for(self, dtype=np.float64), n,
                                                      self._get_upper_bound())
        U_dev.buf.free()  # (the real Graph keeps host arrays only)
        self._e, self._U = e, U
        return
    return _saved_on(type(self))["compute_fourier_basis"](self, n_eigenvectors)


_FEATURES = ("compute_norm_tig", "compute_spectrogram")


def _feature_functions(pygsp_module, saved):
    """compute_norm_tig and compute_spectrogram of `pygsp_module`'s features module on the device (pygsp_amd.features):
    its own Filter class and compute_cheby_coeff, the graph's device Laplacian.  Graphs whose size collides with the
    shape rules (N in {1, Nf}: the identity then reads as a synthesis input, filter.py:270) call the saved originals."""
    from . import features

    approx = pygsp_module.filters.approximations

    def norms(bank):
        return _filters.frame_norms(bank, features.ORDER,
                                    coefficients=lambda b, m: approx.compute_cheby_coeff(b, m=m))

    def compute_norm_tig(g, **kwargs):
        if g.G.N in (1, g.Nf):
            return saved["compute_norm_tig"](g, **kwargs)
        return features._norm_tig(g, norms, **kwargs)

    def compute_spectrogram(G, atom=None, M=100, **kwargs):
        if G.N == 1:  # (each of the reference's atoms is a bank of one: only N = 1 collides)
            return saved["compute_spectrogram"](G, atom, M, **kwargs)
        bank = pygsp_module.filters.Filter(G, features.spectrogram_kernels(G, atom, M))
        return features._spectrogram(G, bank, norms)

    compute_norm_tig.__doc__ = features.compute_norm_tig.__doc__
    compute_spectrogram.__doc__ = features.compute_spectrogram.__doc__
    return {"compute_norm_tig": compute_norm_tig, "compute_spectrogram": compute_spectrogram}


_LEARNING = ("classification_tikhonov_simplex", "regression_tikhonov")


def _learning_functions(saved, harmonic=False):
    """classification_tikhonov_simplex on the device (pygsp_amd.learning, no pyunlocbox) and regression_tikhonov whose
    tau > 0 branch with a sparse L runs the device conjugate gradients and, with `harmonic`, whose tau = 0 branch
    runs them on L_uu (DeviceGraph.dirichlet_cg at its default rtol); tau < 0, a dense L and, without `harmonic`,
    tau = 0 call the saved original.  classification_tikhonov looks regression_tikhonov up at call time and follows."""
    from . import learning

    def regression_tikhonov(G, y, M, tau=0):
        on_device = tau > 0 or (harmonic and tau == 0)
        if not (on_device and sparse.issparse(G.L)):
            return saved["regression_tikhonov"](G, y, M, tau)
        keep = np.asarray(M).reshape(-1).astype(bool)
        y = np.array(y, dtype=np.float64, copy=True)
        y[~keep] = 0  # (learning.py:326: NaN may sit at unmeasured vertices)
        if tau > 0:
            # the reference's cg with scipy's defaults: rtol 1e-5, atol 0, maxiter 10 N (learning.py:328-335)
            solution, _, _ = device_graph_for(G).tikhonov_cg(tau, keep, y)
        else:
            solution, _, _ = device_graph_for(G).dirichlet_cg(keep, y)
        return np.asarray(solution, dtype=np.float64)

    def classification_tikhonov_simplex(G, y, M, tau=0.1, **kwargs):
        return learning.classification_tikhonov_simplex(G, y, M, tau, **kwargs)

    regression_tikhonov.__doc__ = saved["regression_tikhonov"].__doc__
    classification_tikhonov_simplex.__doc__ = learning.classification_tikhonov_simplex.__doc__
    return {"classification_tikhonov_simplex": classification_tikhonov_simplex,
            "regression_tikhonov": regression_tikhonov}


_OPTIMIZATION = ("prox_tv",)


def _optimization_functions(saved):
    """prox_tv on the device (pygsp_amd.optimization): the package's own function cannot run as shipped."""
    from . import optimization

    def prox_tv(x, gamma, G, A=None, At=None, nu=1, tol=10e-4, maxit=200, use_matrix=True, **kwargs):
        return optimization.prox_tv(x, gamma, G, A, At, nu, tol, maxit, use_matrix, **kwargs)

    prox_tv.__doc__ = optimization.prox_tv.__doc__
    return {"prox_tv": prox_tv}


_REDUCTION = ("kron_reduction", "interpolate")


def _reduction_functions(pygsp_module, saved):
    """kron_reduction and interpolate of pygsp.reduction on the device (pygsp_amd.reduction: conjugate gradients where
    the package solves directly) for the inputs that qualify - an undirected graph with a sparse combinatorial
    Laplacian, or a sparse matrix of the form Lap(W) + sigma I, and a valid vertex list; everything else calls the
    saved original.  Results keep the package's types and shapes: a graph of its own Graph class, a CSR matrix, and
    the interpolated columns one below the other, (N Nv, 1).  graph_multiresolution and the pyramid functions look
    both names up at call time and follow."""
    from . import reduction
    graph_cls = pygsp_module.graphs.Graph

    def kept(ind, n):
        try:
            return engine.check_kept(ind, n)
        except ValueError:
            return None

    def kron_reduction(G, ind):
        if isinstance(G, graph_cls):
            keep = kept(ind, G.N)
            if keep is None or G.lap_type != "combinatorial" or not sparse.issparse(G.L) or G.is_directed():
                return saved["kron_reduction"](G, ind)
            W = device_graph_for(G, dtype=np.float64).kron(keep, dense=False, adjacency=True)[1].download()
            coords = G.coords[keep, :] if len(G.coords.shape) else np.ndarray(None)
            return graph_cls(W, coords=coords, lap_type=G.lap_type, plotting=G.plotting)
        if sparse.issparse(G) and kept(ind, G.shape[0]) is not None and reduction.split_laplacian(G) is not None:
            return reduction.kron_reduction(G, ind)
        return saved["kron_reduction"](G, ind)

    def interpolate(G, f_subsampled, keep_inds, order=100, reg_eps=0.005, **kwargs):
        keep = kept(keep_inds, G.N)
        shape = np.shape(f_subsampled)
        if (keep is None or not sparse.issparse(G.L) or len(shape) not in (1, 2) or shape[0] != keep.size or
                not reg_eps > 0 or set(kwargs) - {"method"} or kwargs.get("method", "chebyshev") not in ("chebyshev", "exact")):
            return saved["interpolate"](G, f_subsampled, keep_inds, order=order, reg_eps=reg_eps, **kwargs)
        out = reduction.interpolate(G, np.asarray(f_subsampled, dtype=np.float64), keep, order, reg_eps, **kwargs)
        return out.reshape(-1, 1, order="F")  # (the package's legacy analysis stacks the columns)

    kron_reduction.__doc__ = saved["kron_reduction"].__doc__
    interpolate.__doc__ = saved["interpolate"].__doc__
    return {"kron_reduction": kron_reduction, "interpolate": interpolate}


_TOPOLOGY = ("is_connected", "extract_components")


def _labels_on_device(G):
    """Whether the device labels G: an undirected graph with vertices whose device Laplacian has W's pattern (a
    normalized Laplacian with negative weights may have lost edges of W, graph.py:621-628)."""
    if G.N == 0 or G.is_directed():
        return False
    return not (G.lap_type == "normalized" and G.W.nnz and G.W.data.min() < 0)


def _is_connected_on_device(self):
    """``Graph.is_connected`` of the reference (graph.py:294-366: a Python depth-first search that slices one sparse
    row per vertex) answered by the device's component count (gspx_graph_components) for undirected graphs; cached
    in the reference's own ``_connected``.  Directed graphs run the reference's code."""
    if not _labels_on_device(self):
        return _saved_on(type(self))["is_connected"](self)
    if self._connected is None:
        self._connected = device_graph_for(self).components(labels=False)[0] == 1
    return self._connected


def _extract_components_on_device(self):
    """``Graph.extract_components`` of the reference (graph.py:444-508) with the vertex lists taken from the device
    labels (one stable sort); the children are built by the reference's own ``subgraph``, so they are graphs of
    the patched package, in order of smallest vertex, with ``info = {'orig_idx': ...}``.  Directed graphs run the
    reference's code (NotImplementedError there)."""
    if not _labels_on_device(self):
        return _saved_on(type(self))["extract_components"](self)
    n, labels, _ = device_graph_for(self).components()
    by_label = np.argsort(labels, kind="stable")
    starts = np.searchsorted(labels[by_label], np.arange(n + 1))
    parts = []
    for c in range(n):
        members = by_label[starts[c]:starts[c + 1]].tolist()
        part = self.subgraph(members)
        part.info = {"orig_idx": members}
        parts.append(part)
    return parts


_LAYOUT = ("_fruchterman_reingold",)


def _fruchterman_reingold_on_device(self, dim=2, k=None, pos=None, fixed=[], iterations=50, scale=1.0, center=None,
                                    seed=None):
    """``Graph._fruchterman_reingold`` of the reference (_layout.py:121-219: the spring layout behind
    ``set_coordinates('spring')``, an O(N^2) Python loop per iteration) with the iterations in one device call
    (gspx_layout_spring_dev) and the host bookkeeping of pygsp_amd.layout around them; the call's report is left in
    ``G.layout_report``.  A directed graph, a negative weight and dim outside {2, 3} run the reference's code."""
    from . import layout
    if self.N == 0 or layout.device_route(self, dim) is not None:
        return _saved_on(type(self))["_fruchterman_reingold"](self, dim, k, pos, fixed, iterations, scale, center, seed)
    out, self.layout_report = layout.fruchterman_reingold(self, layout.device_iterate(device_graph_for(self)), dim, k,
                                                          pos, fixed, iterations, scale, center, seed)
    return out


def _linegraph_on_device(graph):
    """Whether the device builds the line graph of a reference graph: an undirected graph with edges, a sparse W
    without self-loops or negative weights, and a device graph that is built from W (laplacian='device')."""
    if _config["laplacian"] != "device" or not sparse.issparse(graph.W) or graph.n_edges == 0 or graph.is_directed():
        return False
    return not (graph.W.diagonal().any() or graph.W.data.min() < 0)


def _linegraph_init(linegraph_cls):
    """What install(linegraph=True) puts in place of ``LineGraph.__init__`` (linegraph.py:34-53): the adjacency of an
    undirected graph without self-loops comes from the device (engine.line_graph on device_graph_for(graph), in
    ``get_edge_list`` order) instead of the host's sparse product B^T B - I; it is downloaded and handed to the
    package's own ``Graph.__init__`` with the reference's arguments - integer unit weights, midpoint coordinates,
    the graph's plotting settings.  Directed graphs and graphs with self-loops run the package's own code."""
    def __init__(self, graph, **kwargs):
        if not _linegraph_on_device(graph):
            return _saved_on(linegraph_cls)["__init__"](self, graph, **kwargs)
        if graph.is_weighted():
            import logging
            logging.getLogger(linegraph_cls.__module__).warning(
                "Your graph is weighted, and is considered unweighted to build a binary line graph.")
        dev = device_graph_for(graph)
        adjacency, _ = engine.line_graph(dev, keep_on_device=False)
        adjacency = adjacency.astype(int)
        points, coords = getattr(graph, "coords", None), None
        if points is not None:  # the midpoint of every edge
            sources, targets, _ = dev.edge_list()
            coords = (points[sources] + points[targets]) / 2
        super(linegraph_cls, self).__init__(adjacency, coords=coords, plotting=graph.plotting, **kwargs)

    return __init__


def install(pygsp_module=None, laplacian="device", dtype=np.float64, device=0, reorder="auto",
            tiles="auto", devices=None, lmax="reference", wrap_filter=True, evaluation=None, fourier=False,
            lanczos=False, features=False, learning=False, topology=False, optimization=False, harmonic=False,
            layout=False, exact=False, full_basis=False, linegraph=False, reduction=False):
    """Patch the real pygsp in place.  `laplacian`: 'device' (L assembled by HIP kernels from
    G.W) or 'host' (upload the reference's G.L).  `devices` (a list of GPU ids, optional): every
    ``Filter.filter(method='chebyshev')`` splits its signal columns over these GPUs - the graph is replicated
    once per GPU, the outputs are gathered by RCCL inside libgspx (pygsp_amd.multi.filter_columns).
    `lmax`: 'device' also replaces ``Graph.estimate_lmax`` so that its default 'lanczos' method runs on the device
    (the step right before the path); 'reference' (default) leaves ARPACK in place.
    `wrap_filter` (default True; the secondary seam of SURVEY 8(b)): also replace ``Filter.filter`` and
    ``Filter.compute_frame`` (filter.py:146, 506) - fused synthesis, device-built identity panels,
    device-resident arrays; False patches ``cheby_op`` alone, and the reference's own loops call it.
    `evaluation`: how the polynomial of a SINGLE filter is evaluated in analysis calls - 'recurrence' (the
    reference's three-term recurrence, approximations.py:99-112), 'newton' (the same polynomial in Newton form:
    fewer panel passes per order) or 'auto' (Newton where it is faster and filters.newton_guard() clears the
    polynomial for the compute dtype, the recurrence otherwise); None (default): pygsp_amd.filters.EVALUATION,
    which is 'recurrence' unless filters.set_evaluation() changed it.
    `fourier` (default False): also replace ``Graph.compute_fourier_basis`` so that partial requests on large graphs
    run on the device (pygsp_amd.fourier); full bases and small graphs keep the reference's code.
    `full_basis` (default False; needs ``fourier=True``): requests for the full basis of graphs of at least
    FULL_BASIS_MIN_VERTICES vertices also run on the device (block Jacobi, pygsp_amd.fourier.device_full_basis), and the
    N x N panel stays there for ``exact=True``.
    `lanczos` (default False): also replace ``approximations.lanczos_op`` and the ``pygsp.filters.lanczos_op`` alias
    with pygsp_amd.filters.lanczos_op (Lanczos filtering on the device, pygsp_amd.lanczos).
    `features` (default False): also replace ``pygsp.features.compute_norm_tig`` and ``compute_spectrogram`` with
    their device forms (pygsp_amd.features: squared column norms of identity panels, no dense frame);
    ``compute_tig`` already reaches the device through the wrapped ``Filter.compute_frame``.
    `learning` (default False): also replace ``pygsp.learning.classification_tikhonov_simplex`` (on the device, without
    pyunlocbox) and ``regression_tikhonov`` (tau > 0 with a sparse L: the device conjugate gradients; otherwise the
    original); ``classification_tikhonov`` looks ``regression_tikhonov`` up at call time and follows.
    `harmonic` (default False; needs ``learning=True``): the wrapped ``regression_tikhonov`` also serves tau = 0, the
    reference's default, with a sparse L on the device: conjugate gradients on L_uu (gspx_dirichlet_cg_dev, rtol 1e-10
    on a float64 graph, 1e-5 on a float32 one) where the reference calls spsolve.  An iterative answer in place of a
    direct one, hence its own flag; a component without a measured vertex gets zeros where spsolve fails.
    `topology` (default False): also replace ``Graph.is_connected`` and ``Graph.extract_components`` so that undirected
    graphs are labelled on the device (gspx_graph_components); directed graphs keep the reference's code.
    `optimization` (default False): also replace ``pygsp.optimization.prox_tv`` with pygsp_amd.optimization.prox_tv (the
    graph total-variation proximal operator on the device, without pyunlocbox).
    `layout` (default False): also replace ``Graph._fruchterman_reingold``, the spring layout behind
    ``Graph.set_coordinates('spring')``, so that undirected graphs without negative weights are laid out on the device
    in 2 or 3 dimensions (gspx_layout_spring_dev); other graphs keep the reference's code.  The eigenmap kinds follow
    ``fourier=True``.
    `linegraph` (default False): also replace ``graphs.LineGraph.__init__`` so that the line graph of an undirected
    graph without self-loops is built on the device (gspx_linegraph_build) and handed to the package's own
    ``Graph.__init__``; directed graphs and graphs with self-loops keep the reference's code.
    `exact` (default False; needs ``wrap_filter=True``): ``Filter.filter(method='exact')`` and ``Modulation.filter``
    also run on the device, against a device copy of the full ``G.U`` (float64 signals; the basis is the reference's
    own eigh, uploaded once, or the device's under ``full_basis=True``); ``Gabor`` follows through ``Filter.filter``.
    Off, the package's own code answers ``method='exact'``.
    `reduction` (default False): also replace ``pygsp.reduction.kron_reduction`` and ``interpolate`` with their device
    forms (pygsp_amd.reduction) for the inputs that qualify; the rest calls the original.  Iterative where the package
    is direct (conjugate gradients at rtol 1e-10 in place of spsolve), hence opt-in."""
    if evaluation is not None and evaluation not in _filters.EVALUATIONS:
        raise ValueError("evaluation must be 'recurrence', 'newton', 'product' or 'auto'")
    if laplacian not in ("device", "host"):
        raise ValueError("laplacian must be 'device' or 'host'")
    if lmax not in ("device", "reference"):
        raise ValueError("lmax must be 'device' or 'reference'")
    if harmonic and not learning:
        raise ValueError("harmonic=True needs learning=True")
    if exact and not wrap_filter:
        raise ValueError("exact=True needs wrap_filter=True")
    if full_basis and not fourier:
        raise ValueError("full_basis=True needs fourier=True")
    if pygsp_module is None:
        import pygsp as pygsp_module
    if devices is not None:
        devices = [int(d) for d in devices]
        if not devices:
            raise ValueError("devices must name at least one GPU")
        device = devices[0]
    _config.update(laplacian=laplacian, dtype=np.dtype(dtype), device=int(device), reorder=reorder,
                   tiles=tiles, devices=devices, evaluation=evaluation)
    on = _targets(pygsp_module)
    _installed.pop(id(pygsp_module), None)
    _installed[id(pygsp_module)] = pygsp_module
    ops = {"cheby_op": _filters.cheby_op}
    if lanczos:
        ops["lanczos_op"] = _filters.lanczos_op
    _apply(on["approximations"], ops)
    _apply(on["filters"], ops)  # (the aliases of pygsp/filters/__init__.py)
    if on["Filter"] is not None:
        wrap = wrap_filter and hasattr(on["approximations"], "compute_cheby_coeff")
        if exact and not wrap:
            raise ValueError("exact=True: {} has no compute_cheby_coeff to wrap Filter with".format(pygsp_module.__name__))
        _apply(on["Filter"], {"filter": _filter_exact_on_device if exact else _filter_on_device,
                              "compute_frame": _compute_frame_on_device} if wrap else {})
    elif exact:
        raise ValueError("exact=True: {} has no filters.Filter".format(pygsp_module.__name__))
    if on["Modulation"] is not None:
        _apply(on["Modulation"], {"filter": _modulation_on_device} if exact else {})
    for name, asked in (("topology", topology), ("layout", layout)):
        if asked and on["Graph"] is None:
            raise ValueError("{}=True: {} has no graphs.Graph".format(name, pygsp_module.__name__))
    if on["Graph"] is not None:
        methods = {}
        if lmax == "device":
            methods["estimate_lmax"] = _estimate_lmax_on_device
        if fourier:
            methods["compute_fourier_basis"] = (_compute_full_basis_on_device if full_basis
                                                else _compute_fourier_basis_on_device)
        if topology:
            methods.update(zip(_TOPOLOGY, (_is_connected_on_device, _extract_components_on_device)))
        if layout:
            methods.update(zip(_LAYOUT, (_fruchterman_reingold_on_device,)))
        _apply(on["Graph"], methods)
    if on["LineGraph"] is not None:
        _apply(on["LineGraph"], {"__init__": _linegraph_init(on["LineGraph"])} if linegraph else {})
    elif linegraph:
        raise ValueError("linegraph=True: {} has no graphs.LineGraph".format(pygsp_module.__name__))
    for name, asked, names, replacements in (
            ("features", features, _FEATURES, lambda saved: _feature_functions(pygsp_module, saved)),
            ("learning", learning, _LEARNING, lambda saved: _learning_functions(saved, harmonic)),
            ("optimization", optimization, _OPTIMIZATION, _optimization_functions),
            ("reduction", reduction, _REDUCTION, lambda saved: _reduction_functions(pygsp_module, saved))):
        if on[name] is not None:
            _apply(on[name], replacements(_originals(on[name], names)) if asked else {})
        elif asked:
            raise ValueError("{0}=True: {1} has no {0} module".format(name, pygsp_module.__name__))
    return pygsp_module


def _targets(pygsp_module):
    """The modules and classes of `pygsp_module` that install() patches, by role; None where the package has none."""
    filters = pygsp_module.filters
    return {"approximations": filters.approximations, "filters": filters, "Filter": getattr(filters, "Filter", None),
            "Modulation": getattr(filters, "Modulation", None),
            "Graph": getattr(getattr(pygsp_module, "graphs", None), "Graph", None),
            "LineGraph": getattr(getattr(pygsp_module, "graphs", None), "LineGraph", None),
            "features": getattr(pygsp_module, "features", None), "learning": getattr(pygsp_module, "learning", None),
            "optimization": getattr(pygsp_module, "optimization", None),
            "reduction": getattr(pygsp_module, "reduction", None)}


def _apply(obj, wanted):
    """Make `obj` (a module or a class) carry exactly the replacements `wanted` (name -> replacement): names patched
    before and not wanted now get their saved original back, the originals of newly patched names are saved in the
    table on `obj`, and an empty table is dropped."""
    saved = obj.__dict__.get(_SAVED, {})
    for n in [n for n in saved if n not in wanted]:
        original = saved.pop(n)
        if original is not _MISSING:
            setattr(obj, n, original)
    for n, replacement in wanted.items():
        saved.setdefault(n, getattr(obj, n, _MISSING))
        setattr(obj, n, replacement)
    if saved:
        setattr(obj, _SAVED, saved)
    elif _SAVED in obj.__dict__:
        delattr(obj, _SAVED)


def _restore(obj):
    """Put back every original saved on `obj` and drop the table; no-op when there is none."""
    _apply(obj, {})


def _originals(obj, names):
    """The package's own obj.name for each of `names`, whether or not it is patched at the moment."""
    saved = obj.__dict__.get(_SAVED, {})
    return {n: saved[n] if n in saved else getattr(obj, n) for n in names}


def uninstall(pygsp_module=None):
    """Restore what install() replaced in `pygsp_module` (default: the module patched last; the importable pygsp
    when nothing is recorded).  Other patched modules stay patched."""
    if pygsp_module is None:
        if _installed:
            pygsp_module = list(_installed.values())[-1]
        else:
            try:
                import pygsp as pygsp_module
            except ImportError:
                return
    _installed.pop(id(pygsp_module), None)
    if not _installed:
        _config["evaluation"] = None
    for obj in _targets(pygsp_module).values():
        if obj is not None:
            _restore(obj)


def use_backend(name, pygsp_module=None, **install_options):
    """Select who evaluates ``Filter.filter(method='chebyshev')`` of the real pygsp: 'gspx' (this
    engine, = install()) or 'reference' (scipy on the host, = uninstall())."""
    if name == "gspx":
        return install(pygsp_module, **install_options)
    if name == "reference":
        return uninstall(pygsp_module)
    raise ValueError("backend must be 'gspx' or 'reference', got {!r}".format(name))


def _backend_from_env():
    """PYGSP_AMD_BACKEND=gspx in the environment installs the seam as soon as this module is imported
    (e.g. from a sitecustomize / conftest line ``import pygsp_amd.plugin``); anything else: no-op."""
    import os
    if os.environ.get("PYGSP_AMD_BACKEND", "").strip().lower() == "gspx":
        try:
            import pygsp
        except ImportError:
            return
        install(pygsp)


_backend_from_env()
