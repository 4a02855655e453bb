"""pygsp.graphs.Graph surface for the Chebyshev-filtering hot path, backed by libgspx.

Mirrors (same names, argument meaning and exceptions) the parts of
``pygsp/graphs/graph.py`` the path touches:

* ``Graph.__init__``              graph.py:98-176   (validation, n_vertices/N, n_edges/Ne)
* ``Graph.compute_laplacian``     graph.py:510-630  -> built ON DEVICE (gspx_graph_create_from_w)
* ``Graph.dw``                    graph.py:783-838  -> device column sums
* ``Graph.lmax / estimate_lmax``  graph.py:840-960  (host, scipy: a read-only input of the path)
* ``Graph._check_signal``         graph.py:632-640
* ``Graph.is_directed``           graph.py:357-405
* ``Graph.is_connected``          graph.py:294-366  -> component labels ON DEVICE (gspx_graph_components)
* ``Graph.extract_components``    graph.py:444-508  -> the same labels, one ``subgraph`` per component
* ``Graph.subgraph / is_weighted / has_loops``      graph.py:218-292, 407-442
* ``Graph.set_coordinates``       _layout.py:5-233  -> 'spring' iterated ON DEVICE (gspx_layout_spring_dev)

Everything else of the reference's Graph (plotting, I/O, ...) is out of scope; use
the real pygsp together with ``pygsp_amd.plugin.install()`` for those.

NNGraph / ImgPatches / Grid2d / Grid2dImgPatches (nngraphs/, grid2d.py) build their W here: the neighbour search on
the device (1 to 4096 dimensions), patches and grid on the host.

The synthetic generators at the bottom (Sensor, ErdosRenyi, StochasticBlockModel) are vectorised
samplers of the same distributions as the reference's constructors (the reference's ER/SBM
constructors are O(N^2) Python loops, stochasticblockmodel.py:125-139, unusable at N >= 1e5).
"""
import logging

import numpy as np
from scipy import sparse, spatial
from scipy.sparse import linalg as splinalg

from . import engine

_logger = logging.getLogger(__name__)


def _checked_adjacency(adjacency, log):
    """The weight matrix as canonical-ready CSR, after the reference's checks (graph.py:98-134): square,
    finite; self-loops and negative weights only warn."""
    dense = None if sparse.issparse(adjacency) else np.asanyarray(adjacency)
    shape = adjacency.shape if dense is None else dense.shape
    if len(shape) != 2 or shape[0] != shape[1]:
        raise ValueError("Adjacency: must be a square matrix.")
    W = sparse.csr_matrix(adjacency if dense is None else dense, copy=False)
    mass = W.sum()
    if np.isnan(mass):
        raise ValueError("Adjacency: there is a Not a Number (NaN).")
    if np.isinf(mass):
        raise ValueError("Adjacency: there is an infinite value.")
    if np.any(W.diagonal() != 0):
        log.warning("Adjacency: there are self-loops (non-zeros on the diagonal). "
                    "The Laplacian will not see them.")
    if W.nnz and W.data.min() < 0:
        log.warning("Adjacency: there are negative edge weights.")
    W.eliminate_zeros()
    return W


class Graph:
    """A weighted graph whose Laplacian lives on the GPU.  Same constructor contract as
    pygsp.graphs.Graph for the path (adjacency, lap_type, coords, plotting); the keyword-only arguments
    are this engine's: compute dtype, device, internal vertex order, gather tiles."""

    def __init__(self, adjacency, lap_type="combinatorial", coords=None, plotting={}, *,
                 compute_dtype=np.float64, device=0, reorder="auto", tiles="auto", ctx=None):
        self.logger = _logger
        # engine-side configuration and state
        # (ctx: a specific libgspx context instead of the default one of `device` - one per driver thread
        # when a process runs several GPUs, pygsp_amd.multi)
        self._ctx = ctx
        self.compute_dtype, self.device = np.dtype(compute_dtype), int(ctx.device if ctx is not None else device)
        self.reorder = reorder
        self.tiles = tiles  # "auto" | True | False: gather tiles of the LDS-staged recurrence step
        self.tile_stats = None
        self._perm, self._perm_done = None, False
        self._dev = {}     # compute dtype -> engine.DeviceGraph
        self._adj_host = self._adj_dev = None  # W: the scipy matrix / a builder's result still on the device
        self._L = self._dw = self._A = self._d = None
        self._flags = {}   # lazily computed facts about W ("directed")
        self._forget_spectrum()
        if lap_type not in ("combinatorial", "normalized"):
            raise ValueError("Unknown Laplacian type {}".format(lap_type))
        self.lap_type = lap_type
        if coords is not None:
            self.coords = np.asanyarray(coords)
        self.plotting, self.signals = dict(plotting), {}
        if isinstance(adjacency, engine.DeviceAdjacency) and not self._setup_from_device_adjacency(adjacency):
            adjacency = adjacency.download()  # (a directed symmetrisation type: the host route below)
        if self._adj_dev is None and not self._setup_on_device(adjacency):
            # the host route (dense input, a directed graph, explicit zeros, ...): the reference's steps one by one
            self._adjacency = _checked_adjacency(adjacency, self.logger)
            self.n_vertices = self.N = self._adjacency.shape[0]
            # stored entries of a directed graph; unordered pairs (+ self-loops) of an undirected one
            loops = int(np.count_nonzero(self._adjacency.diagonal()))
            stored = self._adjacency.nnz
            self.n_edges = self.Ne = stored if self.is_directed() else (stored - loops) // 2 + loops
            self.compute_laplacian(lap_type)

    def _setup_on_device(self, adjacency):
        """Fast route for a scipy CSR matrix: ONE device call (engine.DeviceGraph.setup -> gspx_graph_setup) does the
        checks of graph.py:98-134, the directedness test of graph.py:357-405, the internal vertex order and the
        Laplacian of graph.py:510-630 on the uploaded matrix - no host pass over the stored entries.  False when
        the host route has to take over."""
        if not sparse.isspmatrix_csr(adjacency) or adjacency.shape[0] != adjacency.shape[1]:
            return False
        order = self.reorder
        if isinstance(order, str) and order == "rcm":
            return False
        coords = self._curve_coords(adjacency.shape[0])
        if order == "auto" and coords is None and adjacency.shape[0] >= 4096:
            # no coordinates: the candidate order is reverse Cuthill-McKee, a host (scipy) algorithm - unless the graph
            # is random-like (ER / SBM: balls grow by the mean degree per hop), where no order helps
            if not engine.expander_like(adjacency):
                return False
            order = "none"
        if order in ("morton", "hilbert") and adjacency.shape[0] < 4096:
            return False  # an explicitly requested curve on a small graph: the numpy curves of engine.locality_order
        try:
            dev, rep = engine.DeviceGraph.setup(adjacency, self.lap_type, self.compute_dtype, coords, order,
                                                ctx=self.context)
        except ValueError as e:
            if "canonical" in str(e):
                return False  # duplicates / unsorted indices: the host route sums and sorts them
            raise
        if dev is None:  # (a directed graph whose union pattern would not fit 32-bit indices)
            return False
        if rep["self_loops"]:
            self.logger.warning("Adjacency: there are self-loops (non-zeros on the diagonal). "
                                "The Laplacian will not see them.")
        if rep["negative"]:
            self.logger.warning("Adjacency: there are negative edge weights.")
        if rep["zeros"]:  # graph.py:126-128: W keeps no edge of weight 0 (in place, like the reference; the device
            adjacency.eliminate_zeros()  # Laplacian was built without them)
        self._adjacency = adjacency
        self._adopt_device_graph(dev, rep, adjacency)
        return True

    def _setup_from_device_adjacency(self, adjacency):
        """A generator class hands over the W its device builder produced (engine.DeviceAdjacency): checks, vertex
        order and Laplacian run on it where it lies (gspx_graph_setup_from_knn); the host copy behind G.W is made
        when somebody asks for it.  False when the host route has to take over."""
        order = self.reorder
        if isinstance(order, str) and order == "rcm":
            return False
        coords = self._curve_coords(adjacency.shape[0])
        if order == "auto" and coords is None:
            if getattr(self, "coords", None) is not None and adjacency.shape[0] >= 4096:
                return False  # coordinates no curve can use (a 1-D point cloud): the host route tries RCM
            order = "none"  # a sampled block model: no coordinates, and no order helps a random graph
        if order in ("morton", "hilbert") and adjacency.shape[0] < 4096:
            return False
        dev, rep = engine.DeviceGraph.setup_from(adjacency, self.lap_type, self.compute_dtype, coords, order)
        if dev is None or rep["zeros"]:  # (explicit zeros: W itself has to lose them - the host route)
            if dev is not None:
                dev.destroy()
            return False
        if rep["self_loops"]:
            self.logger.warning("Adjacency: there are self-loops (non-zeros on the diagonal). "
                                "The Laplacian will not see them.")
        self._adj_dev = adjacency
        self._adopt_device_graph(dev, rep, adjacency)
        return True

    def _adopt_device_graph(self, dev, rep, adjacency):
        """What both device set-up routes leave behind: the sizes of `adjacency` (a scipy matrix or a DeviceAdjacency),
        the facts of the set-up report, the device graph `dev` (with its gather tiles) as the one of the compute dtype."""
        self.n_vertices = self.N = adjacency.shape[0]
        # directed (W - W.T has a nonzero, counted on the device: also a 'tril' / 'triu' neighbour graph, a directed
        # block model): the Laplacian was built from (W + W.T) / 2 in the same device call (graph.py:613-616);
        # n_edges: stored entries, or unordered pairs + self-loops (graph.py:135-140)
        directed = self._flags["directed"] = rep["asymmetric"] > 0
        stored, loops = adjacency.nnz, rep["self_loops"]
        self.n_edges = self.Ne = stored if directed else (stored - loops) // 2 + loops
        self._perm_done, self._perm_lazy = True, dev if rep["reordered"] else None
        self.setup_report = rep
        self._apply_tiles(dev)
        self._dev[self.compute_dtype] = dev

    def _apply_tiles(self, dev):
        """Gather tiles of the LDS-staged recurrence step on `dev`, as `tiles` asks: "auto" (when the order is local)
        or a truth value."""
        if self.tiles == "auto":
            self.tile_stats = dev.auto_gather_tiles()
        elif self.tiles:
            self.tile_stats = dev.enable_gather_tiles()

    def _curve_coords(self, n_vertices):
        """The coordinates a space-filling curve can order (engine._curve_coords: one row per vertex, at least two
        columns), else None - a 1-D point cloud or a layout of another size then takes the same route as a graph
        without coordinates (random-like: no order; otherwise reverse Cuthill-McKee on the host) instead of silently
        keeping the graph's own order."""
        coords = getattr(self, "coords", None)
        return coords if engine._curve_coords(coords, n_vertices) else None

    @property
    def _adjacency(self):
        if self._adj_host is None and self._adj_dev is not None:
            self._adj_host, self._adj_dev = self._adj_dev.download(), None
        return self._adj_host

    @_adjacency.setter
    def _adjacency(self, W):
        self._adj_host, self._adj_dev = W, None
        self._A = self._d = None  # (the unweighted view follows W)

    def _forget_spectrum(self):
        """Everything derived from the Laplacian's spectrum (graph.py:602-609)."""
        self._release_basis_dev()
        self._lmax = self._lmax_method = self._e = self._U = None
        self.fourier_stats = None

    # ---- adjacency -----------------------------------------------------------------------------
    @property
    def W(self):
        return self._adjacency

    @property
    def A(self):
        """graph.py:717-727: the binary adjacency matrix ``W > 0`` (host; computed once)."""
        if self._A is None:
            self._A = self.W > 0
        return self._A

    @property
    def d(self):
        """graph.py:729-781: the number of neighbours of every vertex - the stored entries per row of W, or the mean
        of in- and out-degree for a directed graph (host; computed once)."""
        if self._d is None:
            if not self.is_directed():
                self._d = self.W.getnnz(axis=1)
            else:
                self._d = (self.W.getnnz(axis=0) + self.W.getnnz(axis=1)) / 2
        return self._d

    def is_directed(self):
        """True when W differs from its transpose (graph.py:357-405); computed once."""
        if "directed" not in self._flags:
            W = self._adjacency
            self._flags["directed"] = bool((W - W.T).count_nonzero())
        return self._flags["directed"]

    @property
    def _directed(self):
        return self._flags.get("directed")

    def is_weighted(self):
        """graph.py:257-292: some stored weight differs from one."""
        return not np.all(self.W.data == 1)

    def has_loops(self):
        """graph.py:407-442: some diagonal entry of W is not zero."""
        return bool(np.any(self.W.diagonal() != 0))

    def _labels_need_w(self):
        """True when the device Laplacian's pattern is not W's: with the normalized Laplacian and negative weights, a
        vertex whose weights cancel (dw == 0) has lost its row of L (graph.py:621-628) while W still connects it."""
        if self.lap_type != "normalized":
            return False
        report = getattr(self, "setup_report", None)
        if report is not None:
            return report["negative"] > 0
        return bool(self.W.nnz and self.W.data.min() < 0)

    def connected_components(self):
        """(n_components, labels): labels is an int32 array with the component 0 .. n - 1 of every vertex, components
        numbered by their smallest vertex; computed once.  An undirected graph is labelled on the device, on the
        pattern of its device Laplacian (engine.DeviceGraph.components): W is not read, a W that lies on the device
        stays there.  Two cases take the host route, scipy's csgraph on W: a normalized Laplacian with negative
        weights (its pattern may have lost edges of W), and a directed graph, whose labels are its STRONGLY
        connected components in scipy's numbering - the device Laplacian of a directed graph is built from
        (W + W.T) / 2, the direction is gone; labelling directed graphs on the device is out of scope."""
        if "components" not in self._flags:
            if self.n_vertices == 0:
                n, labels = 0, np.empty(0, dtype=np.int32)
            elif self.is_directed() or self._labels_need_w():
                from scipy.sparse import csgraph
                n, labels = csgraph.connected_components(self.W, directed=self.is_directed(), connection="strong",
                                                         return_labels=True)
            else:
                n, labels, self.components_report = self.device_graph().components()
            self._flags["components"] = (int(n), np.asarray(labels, dtype=np.int32))
            self._flags["connected"] = n <= 1
        return self._flags["components"]

    def is_connected(self):
        """graph.py:303-355: every vertex reachable from every other one - for a directed graph along the
        edges AND against them (strongly connected).  An undirected graph is answered by the device's component
        count (nothing but the count comes back, W is not read); a directed one by scipy's csgraph on W.  Computed
        once."""
        if "connected" not in self._flags:
            if self.n_vertices == 0:
                self._flags["connected"] = True
            elif self.is_directed() or self._labels_need_w():
                from scipy.sparse import csgraph
                n, _ = csgraph.connected_components(self.W, directed=self.is_directed(), connection="strong",
                                                    return_labels=True)
                self._flags["connected"] = bool(n == 1)
            else:
                n, _, self.components_report = self.device_graph().components(labels=False)
                self._flags["connected"] = n == 1
        return self._flags["connected"]

    def subgraph(self, vertices):
        """graph.py:218-255: the graph induced by `vertices` (a list of indices, in the order given, or a boolean
        indicator): adjacency W[vertices, :][:, vertices] (sliced on the host, O(nnz)), coords[vertices] if there are
        coordinates, the same lap_type and plotting, the signals sliced.  The child is set up on the device like any
        graph, with this graph's engine settings (compute dtype, device / context, reorder mode, tiles)."""
        vertices = np.asarray(vertices)
        if vertices.size == 0:
            vertices = vertices.astype(np.int64)
        adjacency = sparse.csr_matrix(self.W[vertices, :][:, vertices])
        adjacency.sort_indices()
        coords = getattr(self, "coords", None)
        # (an explicit permutation is one of this graph's vertices: the child chooses its own order)
        reorder = self.reorder if isinstance(self.reorder, str) or self.reorder in (None, False) else "auto"
        child = Graph(adjacency, self.lap_type, None if coords is None else coords[vertices], self.plotting,
                      compute_dtype=self.compute_dtype, device=self.device, reorder=reorder, tiles=self.tiles,
                      ctx=self._ctx)
        for name, signal in self.signals.items():
            child.signals[name] = child._check_signal(np.asanyarray(signal)[vertices])
        return child

    def extract_components(self):
        """graph.py:444-508: one ``subgraph`` per connected component, in order of smallest vertex, each with
        ``info = {'orig_idx': <its vertices, sorted>}``.  The vertex lists come from the device labels by one
        stable sort.  Directed graphs raise NotImplementedError, as in the reference."""
        if self.is_directed():
            raise NotImplementedError("Directed graphs not supported yet.")
        n, labels = self.connected_components()
        by_label = np.argsort(labels, kind="stable")
        starts = np.searchsorted(labels[by_label], np.arange(n + 1))
        parts = []
        for c in range(n):
            members = by_label[starts[c]:starts[c + 1]]
            self.logger.info("Constructing subgraph for component of size {}.".format(members.size))
            part = self.subgraph(members)
            part.info = {"orig_idx": members.tolist()}
            parts.append(part)
        return parts

    # ---- coordinates (pygsp/graphs/_layout.py; pygsp_amd/layout.py) ---------------------------------
    def set_coordinates(self, kind="spring", seed=None, **kwargs):
        """_layout.py:5-119: set ``G.coords`` from an array (N, N x 2 or N x 3) or by a named layout: 'line1D',
        'line2D', 'ring2D', 'random2D', 'random3D' (host; the reference's ``default_rng(seed)`` draws, the same bits),
        'spring' (default; ``_fruchterman_reingold(seed=seed, **kwargs)``, iterated on the device),
        'laplacian_eigenmap2D' / '3D' (``compute_fourier_basis`` of 3 / 4 vectors, then U[:, 1:3] / U[:, 1:4]).
        'community2D' raises NotImplementedError (no Community graphs here), any other string the reference's
        ValueError.  Coordinates set on a graph that is already set up do NOT re-derive the engine's internal vertex
        order: that order was chosen when the device graph was built and stays."""
        from . import layout
        layout.set_coordinates(self, kind, seed, **kwargs)

    def _fruchterman_reingold(self, dim=2, k=None, pos=None, fixed=[], iterations=50, scale=1.0, center=None,
                              seed=None):
        """_layout.py:121-219, Fruchterman-Reingold positions (N x dim): start positions from
        ``default_rng(seed).uniform`` (or `pos`, with `fixed` vertices kept where they are), optimal distance k
        (default sqrt(1 / N)), `iterations` steps cooling linearly from t = 0.1, then - when nothing is fixed - centred,
        rescaled to `scale` and moved to `center`.  The iterations are ONE device call (engine.DeviceGraph.layout_spring,
        report in ``G.layout_report``); the bookkeeping around them is host numpy (pygsp_amd.layout).
        A directed graph, a negative weight or dim outside {2, 3} raise NotImplementedError (pygsp_amd.layout).  The
        engine's internal vertex order is not touched."""
        from . import layout
        why = layout.device_route(self, dim)
        if why is not None:
            raise NotImplementedError(why + " (pygsp_amd.layout); use the real pygsp for this graph")
        out, self.layout_report = layout.fruchterman_reingold(self, layout.device_iterate(self.device_graph()), dim, k,
                                                              pos, fixed, iterations, scale, center, seed)
        return out

    def _symmetric_w(self):
        """W itself if undirected, else (W + W.T)/2 (utils.symmetrize 'average', graph.py:613-616)."""
        return sparse.csr_matrix((self.W + self.W.T) / 2) if self.is_directed() else self.W

    @property
    def context(self):
        """The libgspx context (device + stream) this graph's device state lives on."""
        return self._ctx if self._ctx is not None else engine.default_context(self.device)

    # ---- Laplacian (device) --------------------------------------------------------------------
    def _internal_order(self):
        lazy = getattr(self, "_perm_lazy", None)
        if lazy is not None:  # chosen on the device (gspx_graph_setup): downloaded when somebody asks
            self._perm_lazy = None
            if getattr(lazy, "_h", None):
                self._perm = lazy.download_perm()
            else:
                self._perm_done = False
        if not self._perm_done:
            self._perm_done = True
            mode = self.reorder
            if mode in (None, False, "none"):
                self._perm = None
            elif mode == "auto":
                # large graphs: Hilbert / Morton order of the coordinates if there are any, else reverse
                # Cuthill-McKee on the pattern (0.25 s at N = 1M; within 6 % of Morton on kNN
                # graphs) - kept only if it improves locality over the graph's own order
                big = self.n_vertices >= 4096
                self._perm = engine.auto_order(self.W, getattr(self, "coords", None), ctx=self.context) if big else None
            elif mode in ("morton", "hilbert"):
                self._perm = engine.locality_order(self.W, getattr(self, "coords", None), curve=mode,
                                                   ctx=self.context)
            elif mode == "rcm":
                self._perm = engine.locality_order(self.W, None)
            else:
                self._perm = np.asarray(mode, dtype=np.int32)
        return self._perm

    def device_graph(self, dtype=None):
        """The device-resident Laplacian in `dtype` (built on first use, cached)."""
        dt = np.dtype(dtype or self.compute_dtype)
        g = self._dev.get(dt)
        if g is None:
            perm = self._internal_order()
            if self.is_directed() and sparse.isspmatrix_csr(self.W):
                # (W + W.T) / 2 on the device, in the same call as the Laplacian (gspx_graph_setup)
                try:
                    g, _ = engine.DeviceGraph.setup(self.W, self.lap_type, dt, None, perm if perm is not None else "none",
                                                    ctx=self.context)
                except ValueError:
                    g = None
            if g is None:
                g = engine.DeviceGraph.from_w(self._symmetric_w(), self.lap_type, dtype=dt, perm=perm, ctx=self.context)
            self._apply_tiles(g)
            self._dev[dt] = g
        return g

    def compute_laplacian(self, lap_type="combinatorial"):
        """graph.py:510-630.  The Laplacian is assembled by HIP kernels from W; ``G.L`` is the
        scipy CSR copy downloaded from the device on first access."""
        if lap_type not in ("combinatorial", "normalized"):
            raise ValueError("Unknown Laplacian type {}".format(lap_type))
        if lap_type != self.lap_type:
            self._forget_spectrum()
        self.lap_type = lap_type
        self._L = None
        self._internal_order()  # (an order chosen on the device is fetched before its graph goes)
        while self._dev:
            self._dev.popitem()[1].destroy()
        self.device_graph()  # build now: errors surface here, like in the reference

    @property
    def L(self):
        # the reference's L is float64 for normalized and for integer W, and follows W's dtype for
        # combinatorial; the device copy is in the compute dtype
        if self._L is None:
            self._L = self.device_graph().download_l()
        return self._L

    @property
    def dw(self):
        """Weighted degrees (graph.py:783-838), summed on the device while the Laplacian is built."""
        if self._dw is None:
            self._dw = self.device_graph().download_dw()
        return self._dw

    def _check_signal(self, s):
        """graph.py:632-640: anything array-like whose first axis runs over the vertices."""
        arr = np.asanyarray(s)
        if arr.ndim == 0 or arr.shape[0] != self.n_vertices:
            raise ValueError("First dimension must be the number of vertices "
                             "G.N = {}, got {}.".format(self.N, arr.shape))
        return arr

    def to_device(self, s, dtype=None):
        """Upload a signal ((N,), (N, Nsig) or (N, Nsig, Nfeat)) once and keep it on this graph's device: an
        engine.DeviceArray that Filter.filter / analyze / synthesize take and return, so that a chain of filters
        costs one upload and one download (np.asarray(result))."""
        arr = self._check_signal(s)
        return engine.DeviceArray.from_host(self.context, arr, np.dtype(dtype or self.compute_dtype))

    # ---- operators on the device CSR ----------------------------------------
    def dirichlet_energy(self, x):
        """x^T L x (graph.py:642-702), computed on the device: one sparse product and one reduction."""
        return self.device_graph().dirichlet_energy(self._check_signal(x))

    def get_edge_list(self):
        """(sources, targets, weights), graph.py:934-1029: all stored entries of a directed graph,
        the upper triangle (row-major) of an undirected one."""
        C = self.W.tocoo() if self.is_directed() else sparse.triu(self.W, format="coo")
        assert self.n_edges == C.row.size
        return C.row, C.col, C.data

    def _device_differential(self):
        """The device graph with the edge list grad / div / D work on.  An undirected graph without self-loops
        reads its edges off its own device Laplacian; a directed graph (all stored entries, D / sqrt(2),
        difference.py:160-161) or one with self-loops (diagonal entries are edges whose two D values cancel,
        difference.py:166) hands over Graph.get_edge_list, and the D values are formed on the device."""
        dev = self.device_graph()
        if (self.is_directed() or self.W.diagonal().any()) and getattr(self, "_edges_given_to", None) is not dev:
            sources, targets, weights = self.get_edge_list()
            dev.set_edge_list(sources, targets, weights, directed=self.is_directed())
            self._edges_given_to = dev
        return dev

    def compute_differential_operator(self):
        """difference.py:26-166.  D is assembled on the device (edge enumeration, sqrt of the
        weights) and cached there; ``G.D`` is the scipy csc copy."""
        self._D = self._device_differential().differential_operator()
        self._D_lap_type = self.lap_type

    @property
    def D(self):
        """Differential operator (difference.py:15-24), N x n_edges, L = D D^T."""
        stale = getattr(self, "_D", None) is None or getattr(self, "_D_lap_type", None) != self.lap_type
        if stale:
            self.logger.warning("The differential operator G.D is not available, we need to compute "
                                "it. Explicitly call G.compute_differential_operator() once "
                                "beforehand to suppress the warning.")
            self.compute_differential_operator()
        return self._D

    def grad(self, x):
        """Gradient D^T x of a vertex signal (difference.py:168-244), on the device."""
        return self._device_differential().grad(self._check_signal(x))

    def div(self, y):
        """Divergence D y of an edge signal (difference.py:246-331), on the device."""
        edge_signal = np.asanyarray(y)
        if edge_signal.shape[0] != self.Ne:
            raise ValueError("First dimension must be the number of edges "
                             "G.Ne = {}, got {}.".format(self.Ne, edge_signal.shape))
        return self._device_differential().div(edge_signal)

    # ---- spectrum bounds (read-only input of the hot path) ----------------------------------------
    @property
    def lmax(self):
        if self._lmax is None:
            self.logger.warning("The largest eigenvalue G.lmax is not available, we need to "
                                "estimate it. Explicitly call G.estimate_lmax() or "
                                "G.compute_fourier_basis() once beforehand to suppress the warning.")
            self.estimate_lmax()
        return self._lmax

    def _lmax_lanczos_device(self):
        # Lanczos on the device (the reference calls ARPACK eigsh(tol=5e-3) on the host, graph.py:911-917,
        # with a random start vector: 3.3 s at N = 1M and not reproducible).  Same contract: an estimate
        # from below, increased by 1 % (graph.py:920); non-convergence is a ValueError (engine).
        ritz, _ = self.device_graph().lanczos_lmax(max_iter=80, tol=5e-4)
        if not ritz <= self._get_upper_bound() * (1 + 1e-6) + 1e-12:  # graph.py:919 (an assert there)
            raise ValueError("The Lanczos estimate {} exceeds the upper bound of lambda_max.".format(ritz))
        return ritz * 1.01

    def _lmax_lanczos_host(self):
        try:
            ritz = splinalg.eigsh(self.L.astype(np.float64), k=1, tol=5e-3, ncv=min(self.N, 10),
                                  return_eigenvectors=False)[0]
        except splinalg.ArpackNoConvergence:
            raise ValueError("The Lanczos method did not converge. Try to use bounds.")
        assert ritz <= self._get_upper_bound() + 1e-12
        return ritz * 1.01  # 1 % safety margin, as the reference

    def estimate_lmax(self, method="lanczos"):
        """graph.py:858-931: 'lanczos' (device), 'lanczos-host' (ARPACK, the reference's own call) or
        'bounds'; a repeated call with the method already used is a no-op."""
        if method == self._lmax_method:
            return
        estimators = {"lanczos": self._lmax_lanczos_device, "lanczos-host": self._lmax_lanczos_host,
                      "bounds": self._get_upper_bound}
        if method not in estimators:
            raise ValueError("Unknown method {}".format(method))
        self._lmax_method = method
        self._lmax = estimators[method]()

    def _get_upper_bound(self):
        """The smallest of four classical upper bounds of lambda_max (graph.py:933-960)."""
        if self.lap_type != "combinatorial":
            return 2  # normalized Laplacian
        w_dtype = self._adj_dev.weights if self._adj_dev is not None else self.W.dtype
        if not self.is_directed() and w_dtype in (np.float64, np.int64):
            # the same four candidates from one device pass over W (gspx_graph_lmax_bounds), same operation order
            on_device = self.device_graph().lmax_bounds() if self.compute_dtype == np.float64 else None
            if on_device is not None:
                candidates = [self.n_vertices * on_device[0], 2 * on_device[1]]
                if self.n_edges:
                    candidates.append(on_device[2])
                candidates.append(on_device[3])  # (NaN with isolated vertices: never the minimum, as in the reference)
                return float(min(candidates))
        W, deg = self._symmetric_w(), np.asarray(self.dw, dtype=np.float64)
        # (the first candidate on W AS STORED, graph.py:941 - for a directed graph max W_ij, not max (W + W.T) / 2,
        # which would give a smaller bound than the reference's where this candidate is the minimum: ADVICE r5)
        candidates = [self.n_vertices * self.W.max(), 2 * deg.max()]
        if self.n_edges:
            ends = self.W.tocoo()  # max over edges: both triangles give the same maximum
            candidates.append((deg[ends.row] + deg[ends.col]).max())
        with np.errstate(divide="ignore", invalid="ignore"):
            candidates.append(np.max(deg + W.dot(deg) / deg))
        return min(candidates)

    # ---- where the eigenvalues lie, without a basis (spectrum.py) ---------------------------------
    def estimate_spectral_density(self, order=100, n_vectors=32, seed=0, damping="jackson"):
        """The density of states of L by the kernel polynomial method: a spectrum.SpectralDensity (cdf, pdf, count,
        quantile) from the order + 1 Chebyshev moments of `n_vectors` random +-1 vectors - order / 2 recurrence steps
        on the device, no eigendecomposition.  Uses G.lmax."""
        from . import spectrum
        return spectrum.estimate_spectral_density(self, order, n_vectors, seed, damping)

    def count_eigenvalues(self, lo, hi, **kwargs):
        """The estimated number of eigenvalues of L in (lo, hi]; kwargs: those of estimate_spectral_density."""
        return self.estimate_spectral_density(**kwargs).count(lo, hi)

    def compute_fourier_basis(self, n_eigenvectors=None, *, method="auto", tol=None, maxiter=None, seed=0,
                              degree=(10, 300)):
        """The (partial) Fourier basis of L (fourier.py:97-195), cached in ``G.e`` / ``G.U``.

        ``n_eigenvectors=None`` or ``N``: the dense host eigendecomposition, sets ``lmax`` (method 'fourier').
        A partial request (k < N) keeps a cached basis of at least k vectors; otherwise `method` picks the solver:
        'device' - Chebyshev-filtered subspace iteration on the float64 device graph (pygsp_amd.fourier), residuals
        ||L u_i - e_i u_i|| <= tol * b with b the rigorous upper bound of lambda_max, ValueError after `maxiter`
        iterations, filter degree per iteration within `degree`, start block from `seed`; 'dense' - host eigh,
        sliced; 'auto' - 'device' when N >= 2048 and the block (k plus guard vectors) is at most N / 4.
        `tol` and `maxiter` default to 1e-10 and 100 there.
        A partial basis leaves ``lmax`` alone; e[0] is checked to be within 1e-5 of zero and set to zero, and each
        column's largest-magnitude entry is made positive.

        ``method='jacobi'`` (opt-in, for the full basis and for partial requests alike): all N eigenpairs by block
        Jacobi on the float64 device graph (fourier.device_full_basis; `tol` 1e-13 on off(L) / ||L||_F, ValueError
        after `maxiter` sweeps, 30 by default).  The N x N panel stays on the device, so a following
        ``filter(method='exact')``, ``gft`` or ``igft`` of a device array uploads no basis.  k < N keeps the first k
        columns under the partial-result rules, as 'dense' does."""
        N = self.n_vertices
        k = N if n_eigenvectors is None else int(n_eigenvectors)
        if method == "jacobi":
            return self._fourier_basis_jacobi(k, n_eigenvectors, tol, maxiter)
        tol = 1e-10 if tol is None else tol
        maxiter = 100 if maxiter is None else maxiter
        if k == N:
            if self._U is None or self._U.shape[1] < N:
                self._release_basis_dev()
                lam, vec = np.linalg.eigh(self.L.toarray().astype(np.float64))
                if abs(lam[0]) < 1e-9:
                    lam[0] = 0
                self._e, self._U = lam, vec
                self._lmax, self._lmax_method = lam[-1], "fourier"
            return
        if not 1 <= k < N:
            raise ValueError("n_eigenvectors must be in 1..{}, got {}".format(N, n_eigenvectors))
        if method not in ("auto", "device", "dense"):
            raise ValueError("method must be 'auto', 'device', 'dense' or 'jacobi', got {!r}".format(method))
        if self._U is not None and k <= len(self._e):
            return
        from . import fourier
        if method == "device" or (method == "auto" and fourier.use_device(N, k)):
            dev = self.device_graph(np.float64)
            e, U, U_dev, stats = fourier.device_partial_basis(dev, k, self._get_upper_bound(), tol=tol,
                                                              maxiter=maxiter, seed=seed, degree=degree)
            self._release_basis_dev()
            self._e, self._U, self._U_dev, self.fourier_stats = e, U, (dev, U_dev), stats
            return
        lam, vec = np.linalg.eigh(self.L.toarray().astype(np.float64))
        e, U = np.array(lam[:k]), np.array(vec[:, :k])
        fourier.finish_partial(e, U)
        self._release_basis_dev()
        self._e, self._U, self.fourier_stats = e, U, None

    def _fourier_basis_jacobi(self, k, asked, tol, maxiter):
        from . import fourier
        N = self.n_vertices
        if not 1 <= k <= N:
            raise ValueError("n_eigenvectors must be in 1..{}, got {}".format(N, asked))
        if self._U is not None and k <= len(self._e):
            return
        dev = self.device_graph(np.float64)
        e, U, U_dev, stats = fourier.device_full_basis(dev, tol=fourier.FULL_TOL if tol is None else tol,
                                                       max_sweeps=fourier.FULL_MAX_SWEEPS if maxiter is None else maxiter)
        self._release_basis_dev()
        if k == N:
            self._e, self._U, self._U_dev, self.fourier_stats = e, U, (dev, U_dev), stats
            self._lmax, self._lmax_method = e[-1], "fourier"
            return
        if U_dev.buf is not None:  # (the N x N panel is not kept for a slice: U[:, :k] is uploaded when first needed)
            dev.ctx.give(U_dev.buf)
            U_dev.buf = None
        e, U = np.array(e[:k]), np.array(U[:, :k])
        fourier.finish_partial(e, U)  # (the signs are already the rule's: this checks e[0] and sets it to zero)
        self._e, self._U, self.fourier_stats = e, U, stats

    def _release_basis_dev(self):
        """Drop the device copy of U: (float64 DeviceGraph, fourier.DevicePanel) or None."""
        held = getattr(self, "_U_dev", None)
        self._U_dev = None
        if held is not None:
            dev, panel = held
            if panel.buf is not None:
                dev.ctx.give(panel.buf)
                panel.buf = None

    def _basis_on_device(self):
        """(float64 DeviceGraph, DevicePanel N x n of U): the solver's copy, or U uploaded once."""
        if self._U_dev is None:
            from . import fourier
            dev = self.device_graph(np.float64)
            be = fourier.DeviceBackend(dev, 1.0)
            self._U_dev = (dev, be.from_host(self.U))
        return self._U_dev

    def gft(self, s):
        """Graph Fourier transform U^T s (fourier.py:197-230): numpy input on the host, exactly the reference's
        arithmetic.  A float64 engine.DeviceArray is read on the device against the device copy of U, for a basis of
        any width n, and the result is a DeviceArray of shape (n, ...) whose coefficients never leave the device
        (gspx_panel_gram_to_dev: the Gram kernel, written into the result's planes).  Bases of at most 512 vectors
        take this same call rather than the older Gram-to-the-host: it is the same kernel with the same row chunks,
        so up to 512 signal columns give the bits they gave before, and one path serves every width."""
        if isinstance(s, engine.DeviceArray):
            return self._transform_device(s, inverse=False)
        s = self._check_signal(s)
        U = np.conjugate(self.U)  # True Hermitian. (Although U is often real.)
        return np.tensordot(U, s, ([0], [0]))

    def igft(self, s_hat):
        """Inverse transform U s_hat (fourier.py:232-264).  The first axis of s_hat runs over the basis vectors
        (N of them for a full basis, as in the reference).  A float64 DeviceArray gives a DeviceArray: the n x Nsig
        coefficients are read where they lie (gspx_spectral_apply_dev in plain mode) and the N x Nsig product is
        formed on the device, for a basis of any width.  The product kernel is the one gspx_panel_combine_dev
        launches, tile for tile, so narrow bases keep their bits here too."""
        if isinstance(s_hat, engine.DeviceArray):
            return self._transform_device(s_hat, inverse=True)
        n = self.U.shape[1]
        arr = np.asanyarray(s_hat)
        if arr.ndim == 0 or arr.shape[0] != n:
            raise ValueError("First dimension must be the number of basis vectors "
                             "{}, got {}.".format(n, arr.shape))
        return np.tensordot(self.U, arr, ([1], [0]))

    def _transform_device(self, a, inverse):
        from . import fourier
        if a.dtype != np.float64:
            raise TypeError("gft / igft of a device array need float64 signals (got {}); fp32 is not "
                            "supported".format(a.dtype))
        n = self.U.shape[1]
        rows_in, rows_out = (n, self.N) if inverse else (self.N, n)
        if a.cube[0] != rows_in:
            raise ValueError("First dimension must be {}, got {}.".format(rows_in, a.shape))
        dev, U = self._basis_on_device()
        ctx = dev.ctx
        if a.ctx is not ctx:
            raise ValueError("the device array lives on another context than the graph's Fourier basis")
        _, S, F = a.cube
        shape = (rows_out,) + tuple(a.shape[1:])
        out = engine.DeviceArray.empty(ctx, (rows_out, S, F), np.float64)
        for f in range(F):  # planes [feature][row][signal] on both sides
            src, dst = a.ptr + 8 * f * rows_in * S, out.ptr + 8 * f * rows_out * S
            if inverse:
                fourier.spectral_apply(ctx, self.N, U.ptr, U.ld, n, src, S, S, dst, S)
            else:
                fourier.panel_gram_to(ctx, self.N, U.ptr, U.ld, n, src, S, S, dst, S)
        out.shape = shape
        return out

    @property
    def coherence(self):
        """max |U_ik| over the full Fourier basis (fourier.py:38-95): between 1 / sqrt(N) (every eigenvector spread
        over all vertices) and 1 (one of them is a delta).  Computed on the host from ``G.U``; a cached partial basis
        is replaced by the full one first, as the definition runs over all N vectors."""
        if self.U.shape[1] < self.N:
            self.compute_fourier_basis()
        return float(np.abs(self.U).max())

    @property
    def e(self):
        if self._U is None:  # (a cached partial basis is returned as it is, fourier.py:156)
            self.compute_fourier_basis()
        return self._e

    @property
    def U(self):
        if self._U is None:
            self.compute_fourier_basis()
        return self._U

    def __repr__(self):
        return "{}(n_vertices={}, n_edges={}, lap_type={})".format(
            type(self).__name__, self.n_vertices, self.n_edges, self.lap_type)


# ------------------------------------------------------------------------------------------------
# synthetic graph generators (vectorised restatements of the reference's models)
# ------------------------------------------------------------------------------------------------
def _sensor_points(N, seed, distributed=False):
    """Coordinates of ``graphs.Sensor`` (nngraphs/sensor.py:56-70), drawn from the same numpy stream as
    the reference so that the same seed gives the same graph: uniform in the unit square, or one jittered
    point per cell of a sqrt(N) x sqrt(N) grid."""
    stream = np.random.default_rng(seed)
    if not distributed:
        return stream.uniform(0, 1, (N, 2))
    side = np.sqrt(N)
    if side != np.floor(side):
        raise ValueError("The number of vertices must be a perfect square if they are to be "
                         "distributed on a grid.")
    cells = np.mgrid[0:1:1 / side, 0:1:1 / side].reshape(2, -1).T
    return cells + stream.uniform(0, 1 / side, (N, 2))


def sensor_weights(N, k=6, seed=None, return_coords=True):
    """W of ``graphs.Sensor(N, k, seed=seed)`` built on the HOST with a KD-tree (nngraphs/sensor.py:50-75,
    nngraph.py:213-297): k nearest neighbours of uniform points, weights exp(-d^2 / sigma) with sigma the
    mean neighbour distance, symmetrised by averaging.  The reference construction the device k-NN path is
    compared with."""
    coords = _sensor_points(N, seed)
    dist, nbr = spatial.cKDTree(coords).query(coords, k=k + 1, workers=-1)
    dist, nbr = dist[:, 1:], nbr[:, 1:]  # column 0 is the point itself
    sigma = float(dist.mean())
    directed = sparse.csc_matrix((np.exp(-np.square(dist.ravel()) / sigma),
                                  (np.repeat(np.arange(N), k), nbr.ravel())), shape=(N, N))
    W = sparse.csr_matrix((directed + directed.T) / 2)
    return (W, coords) if return_coords else W


_MINKOWSKI = {1: "manhattan", 2: "euclidean", np.inf: "max_dist"}


class NNGraph(Graph):
    """Nearest-neighbour graph from a point cloud (nngraphs/nngraph.py:13-313), built on the device
    (NNtype='knn', the KD-tree query, and NNtype='radius', the ball query: 1 to 4096 dimensions, k up to 64), dist_type
    'euclidean' / 'manhattan' / 'max_dist', every symmetrize_type of utils.symmetrize.  Other settings
    raise NotImplementedError (no host fallback)."""

    def __init__(self, Xin, NNtype="knn", use_flann=False, center=True, rescale=True, k=10, sigma=None,
                 epsilon=0.01, plotting={}, symmetrize_type="average", dist_type="euclidean", order=0,
                 **kwargs):
        self.Xin = np.asanyarray(Xin)
        self.NNtype, self.use_flann, self.center, self.rescale = NNtype, use_flann, center, rescale
        self.k, self.sigma, self.epsilon = k, sigma, epsilon
        self.symmetrize_type, self.dist_type, self.order = symmetrize_type, dist_type, order
        n_points, dim = self.Xin.shape
        if n_points <= k:
            raise ValueError("The number of neighbors (k={}) must be smaller "
                             "than the number of nodes ({}).".format(k, n_points))
        if NNtype not in ("knn", "radius"):
            raise ValueError("Unknown NNtype {}".format(NNtype))
        # nngraph.py:139-145: 'minkowski' is the p-norm of the given order
        metric = _MINKOWSKI.get(order) if dist_type == "minkowski" else (
            dist_type if dist_type in engine.METRICS else None)
        if metric is None:
            raise NotImplementedError("the device builder covers dist_type 'euclidean', 'manhattan', 'max_dist' "
                                      "(and 'minkowski' of order 1, 2, inf)")
        if symmetrize_type not in engine.SYMMETRIZE:
            raise ValueError("Unknown symmetrization method {}.".format(symmetrize_type))  # utils.py:277
        points = self.Xin
        if center:  # nngraph.py:129-130: the cloud's centroid moves to the origin
            points = points - points.mean(axis=0)[np.newaxis, :]
        if rescale:  # nngraph.py:132-137: N^(1/min(d,3)) / 10 over half the bounding-box diagonal
            half_diagonal = 0.5 * np.linalg.norm(points.max(axis=0) - points.min(axis=0), 2)
            points = points * (np.power(n_points, 1.0 / float(min(dim, 3))) / 10.0 / half_diagonal)
        ctx = kwargs.get("ctx") or engine.default_context(int(kwargs.get("device", 0)))
        if NNtype == "knn":
            W, self.sigma, info = engine.knn_graph(points, k, sigma, ctx=ctx, metric=metric,
                                                   symmetrize=symmetrize_type, keep_on_device=True)
        else:  # nngraph.py:228-287; a symmetric relation: (W + W.T) / 2 = W
            W, self.sigma, info = engine.radius_graph(points, epsilon, sigma, ctx=ctx, metric=metric,
                                                      keep_on_device=True)
        self.knn_build_ms = info["build_ms"]
        Graph.__init__(self, W, plotting=plotting, coords=points, **kwargs)


def image_patches(img, patch_shape):
    """Feature matrix of ``graphs.ImgPatches`` (nngraphs/imgpatches.py:52-99), on the host and without scikit-image:
    one row per pixel (raster order), holding the r x c window around it - all channels of a colour image, channel
    fastest - cut from the image padded symmetrically by ((r - 1) // 2, r // 2) rows and ((c - 1) // 2, c // 2)
    columns.  patch_shape: (r, c), or (r,) for a square window.  Returns (h * w, r * c * channels)."""
    pixels = np.asanyarray(img)
    if pixels.ndim not in (2, 3):
        raise ValueError("Image should be at least a 2D array.")
    window = tuple(patch_shape) if len(patch_shape) == 2 else (patch_shape[0], patch_shape[0])
    margins = [((side - 1) // 2, side // 2) for side in window]
    if pixels.ndim == 3:  # the window spans every channel
        margins.append((0, 0))
        window += (pixels.shape[2],)
    padded = np.pad(pixels, margins, mode="symmetric")
    views = np.lib.stride_tricks.sliding_window_view(padded, window)
    return views.reshape(pixels.shape[0] * pixels.shape[1], -1)


class ImgPatches(NNGraph):
    """Nearest-neighbour graph between the patches of an image (nngraphs/imgpatches.py:8-105): one vertex per pixel,
    its feature vector (``Xin``) the patch around it (``image_patches``); the neighbour search runs on the device -
    5 x 5 patches of an RGB image are a 75-dimensional cloud.  kwargs go to NNGraph."""

    def __init__(self, img, patch_shape=(3, 3), **kwargs):
        self.img, self.patch_shape = img, patch_shape
        NNGraph.__init__(self, image_patches(img, patch_shape), **kwargs)


def grid2d_weights(N1, N2=None, diagonal=0.0):
    """W and coordinates of ``graphs.Grid2d`` (grid2d.py:37-86), on the host: vertex a * N2 + b sits in row a, column
    b of an N1 x N2 grid; unit edges to the right and downward neighbour, edges of weight `diagonal` to the two
    downward diagonal ones (when there are two rows and columns at least); coordinates (b / N2, (N1 - 1 - a) / N1)."""
    N2 = N1 if N2 is None else N2
    a, b = np.divmod(np.arange(N1 * N2), N2)
    steps = [(b < N2 - 1, 1, 1.0), (a < N1 - 1, N2, 1.0)]
    if diagonal != 0.0 and N1 > 1 and N2 > 1:
        steps += [((a < N1 - 1) & (b < N2 - 1), N2 + 1, diagonal), ((a < N1 - 1) & (b > 0), N2 - 1, diagonal)]
    src = np.concatenate([np.flatnonzero(ok) for ok, _, _ in steps])
    dst = np.concatenate([np.flatnonzero(ok) + jump for ok, jump, _ in steps])
    wgt = np.concatenate([np.full(np.count_nonzero(ok), value) for ok, _, value in steps])
    half = sparse.coo_matrix((wgt, (src, dst)), shape=(N1 * N2, N1 * N2))
    coords = np.column_stack((b / float(N2), (N1 - 1 - a) / float(N1)))
    return sparse.csr_matrix(half + half.T), coords


class Grid2d(Graph):
    """2-D grid graph (grid2d.py:9-89); ``grid2d_weights`` builds W and the coordinates."""

    def __init__(self, N1=16, N2=None, diagonal=0.0, **kwargs):
        self.N1, self.N2 = N1, N1 if N2 is None else N2
        W, coords = grid2d_weights(self.N1, self.N2, diagonal)
        limits = np.array([-1.0 / self.N2, 1 + 1.0 / self.N2, 1.0 / self.N1, 1 + 1.0 / self.N1])
        Graph.__init__(self, W, coords=coords, plotting={"limits": limits}, **kwargs)


class Grid2dImgPatches(Graph):
    """Union of the patch graph of an image with the grid graph of its pixels (nngraphs/grid2dimgpatches.py:9-51):
    W = aggregate(Wp, Wg), the grid's coordinates.  kwargs go to ImgPatches."""

    def __init__(self, img, aggregate=lambda Wp, Wg: Wp + Wg, **kwargs):
        self.Gg, self.Gp = Grid2d(*np.shape(img)[:2]), ImgPatches(img, **kwargs)
        Graph.__init__(self, aggregate(self.Gp.W, self.Gg.W), coords=self.Gg.coords, plotting=self.Gg.plotting)


class Sensor(NNGraph):
    """Random sensor graph (nngraphs/sensor.py:11-78): uniform points in the unit square, k nearest
    neighbours; the neighbour search runs on the device.  ``sensor_weights`` is the host (KD-tree)
    construction of the same matrix."""

    def __init__(self, N=64, k=6, distributed=False, seed=None, **kwargs):
        self.distributed, self.seed = distributed, seed
        NNGraph.__init__(self, Xin=_sensor_points(N, seed, distributed), k=k, rescale=False, center=False,
                         plotting={"limits": np.array([0, 1, 0, 1])}, **kwargs)


def line_graph_host(sources, targets, n_vertices):
    """Adjacency of the line graph from an edge list, on the host with scipy - what linegraph.py:41-46 computes through
    the differential operator.  An edges x vertices indicator marks the endpoints of every edge; a self-loop marks
    none, because its column of D is empty (its two values cancel, difference.py:166).  Two edges are joined when
    their rows meet - the product is a boolean one, so an antiparallel pair of a directed graph, which shares both
    endpoints, still gets the value 1 - and the identity is subtracted: 0 on the diagonal of an ordinary edge
    (dropped), -1 on that of a self-loop.  Returns (adjacency csr int64, indicator csr float64)."""
    sources, targets = np.asarray(sources), np.asarray(targets)
    n_edges = sources.size
    ordinary = np.flatnonzero(sources != targets)
    touches = sparse.csr_matrix((np.ones(2 * ordinary.size), (np.concatenate([ordinary, ordinary]),
                                 np.concatenate([sources[ordinary], targets[ordinary]]))), shape=(n_edges, n_vertices))
    meet = sparse.csr_matrix(touches.dot(touches.T))
    meet.data = np.ones(meet.nnz, dtype=np.int64)
    adjacency = sparse.csr_matrix(meet - sparse.identity(n_edges, dtype=np.int64, format="csr"))
    adjacency.eliminate_zeros()
    adjacency.sort_indices()
    return adjacency, touches


class LineGraph(Graph):
    """Line graph of a graph (linegraph.py:11-53): one vertex per edge of ``graph.get_edge_list()``, two of them joined
    when the edges share an endpoint; unit weights (a weighted graph is read as unweighted, with the reference's
    warning), coordinates at the edges' midpoints when the graph has coordinates, the graph's plotting settings.
    kwargs go to Graph (lap_type and the engine's keyword-only arguments).

    An undirected graph without self-loops or negative weights is served on the device: the adjacency is built from
    the edge tables of its device graph (engine.line_graph) and stays there - checks, vertex order, Laplacian and
    gather tiles run on it where it lies, ``LG.W`` is downloaded when somebody reads it.  Every other graph takes the
    host route (``line_graph_host``), which keeps the reference's results for directed graphs and self-loops."""

    def __init__(self, graph, **kwargs):
        if graph.is_weighted():
            _logger.warning("Your graph is weighted, and is considered "
                            "unweighted to build a binary line graph.")
        points = getattr(graph, "coords", None)
        self.line_graph_info = None
        if self._on_device(graph):
            adjacency, self.line_graph_info = engine.line_graph(graph.device_graph())
            coords = None
            if points is not None:
                sources, targets, _ = graph.device_graph().edge_list()
                coords = (points[sources] + points[targets]) / 2
        else:
            sources, targets, _ = graph.get_edge_list()
            adjacency, touches = line_graph_host(sources, targets, graph.n_vertices)
            coords = None if points is None else touches.dot(points) / 2
        Graph.__init__(self, adjacency, coords=coords, plotting=graph.plotting, **kwargs)

    @staticmethod
    def _on_device(graph):
        """The device builder reads the pattern of the device Laplacian as the graph's simple undirected edge set:
        that holds for an undirected graph with edges, without self-loops and without negative weights (whose
        normalized Laplacian may have lost rows, graph.py:621-628)."""
        if graph.n_edges == 0 or graph.is_directed():
            return False
        report = getattr(graph, "setup_report", None)
        if report is not None and graph._adj_dev is not None:  # (W still lies on the device: the set-up's own counts)
            return not (report["self_loops"] or report["negative"])
        W = graph.W
        return not (W.diagonal().any() or (W.nnz and W.data.min() < 0))


def _sample_pairs_within(rng, n, p):
    """m ~ Binomial(n(n-1)/2, p) distinct unordered pairs (r > c) among n vertices."""
    total = n * (n - 1) // 2
    m = rng.binomial(total, p) if total > 0 else 0
    if m == 0:
        return np.empty(0, np.int64), np.empty(0, np.int64)
    got = np.empty(0, dtype=np.int64)
    while got.size < m:
        cand = rng.integers(0, total, size=int((m - got.size) * 1.1) + 16)
        got = np.unique(np.concatenate([got, cand]))
    got = rng.permutation(got)[:m]
    # linear index -> (r, c) with r > c :  idx = r(r-1)/2 + c
    r = np.floor((1 + np.sqrt(1 + 8 * got.astype(np.float64))) / 2).astype(np.int64)
    r = np.where(r * (r - 1) // 2 > got, r - 1, r)
    r = np.where((r + 1) * r // 2 <= got, r + 1, r)
    c = got - r * (r - 1) // 2
    return r, c


def _sample_pairs_between(rng, na, nb, p):
    total = na * nb
    m = rng.binomial(total, p) if total > 0 else 0
    if m == 0:
        return np.empty(0, np.int64), np.empty(0, np.int64)
    got = np.empty(0, dtype=np.int64)
    while got.size < m:
        cand = rng.integers(0, total, size=int((m - got.size) * 1.1) + 16)
        got = np.unique(np.concatenate([got, cand]))
    got = rng.permutation(got)[:m]
    return got // nb, got % nb


def _block_probabilities(k, p, q):
    """The k x k matrix of edge probabilities from the within-block probabilities p (scalar or length-k
    vector) and the between-block ones q (scalar or k x k matrix; default 0.3 / k), as
    stochasticblockmodel.py:91-116 assembles it."""
    within = np.asanyarray(p, dtype=np.float64)
    if within.size == 1:
        within = np.full(k, within.reshape(-1)[0])
    if within.shape != (k,):
        raise ValueError("Optional parameter p is neither a scalar nor a vector of length k.")
    between = np.asanyarray(0.3 / k if q is None else q, dtype=np.float64)
    if between.size == 1:
        between = np.full((k, k), float(between.reshape(-1)[0]))
    if between.shape != (k, k):
        raise ValueError("Optional parameter q is neither a scalar nor a matrix of size k x k.")
    M = np.array(between, dtype=np.float64)
    np.fill_diagonal(M, within)
    return M


def sbm_weights(N, k=5, z=None, p=0.7, q=None, seed=None):
    """W with the distribution of ``graphs.StochasticBlockModel(N, k, z, p=p, q=q,
    directed=False, self_loops=False)`` (stochasticblockmodel.py:61-144): every unordered pair
    is an edge independently with probability p (same block) or q (different blocks); unit
    weights (int64, as the reference).  O(nnz) instead of the reference's O(N^2) loop.  Host / numpy
    sampler; the product's generators use the device sampler (engine.sbm_graph)."""
    stream = np.random.default_rng(seed)
    labels = np.sort(stream.integers(0, k, N)) if z is None else np.asarray(z)
    between = 0.3 / k if q is None else q
    by_block = np.argsort(labels, kind="stable")
    starts = np.searchsorted(labels[by_block], np.arange(k + 1))
    members = [by_block[starts[b]:starts[b + 1]] for b in range(k)]
    heads, tails = [], []
    for a in range(k):
        r, c = _sample_pairs_within(stream, members[a].size, p)
        heads.append(members[a][r])
        tails.append(members[a][c])
        for b in range(a):
            r, c = _sample_pairs_between(stream, members[a].size, members[b].size, between)
            heads.append(members[a][r])
            tails.append(members[b][c])
    heads = np.concatenate(heads) if heads else np.empty(0, np.int64)
    tails = np.concatenate(tails) if tails else np.empty(0, np.int64)
    W = sparse.csr_matrix((np.ones(2 * heads.size, dtype=np.int64),
                           (np.concatenate([heads, tails]), np.concatenate([tails, heads]))), shape=(N, N))
    return W, labels


class StochasticBlockModel(Graph):
    """stochasticblockmodel.py:12-181: labels z (sorted random labels from the same numpy stream as the
    reference when not given), probabilities M (or p on the diagonal and q elsewhere), edges sampled on the
    device in O(edges) (engine.sbm_graph) - equal in distribution to the reference's N^2 loop, not bit-equal.
    directed / self_loops / connected (n_try fresh samples until one is connected) as the reference.
    ``sbm_weights`` is the numpy sampler of the undirected, loop-free distribution."""

    def __init__(self, N=1024, k=5, z=None, M=None, p=0.7, q=None, directed=False, self_loops=False,
                 connected=False, n_try=10, seed=None, **kwargs):
        self.k, self.directed, self.self_loops, self.connected = k, directed, self_loops, connected
        self.n_try, self.seed = n_try, seed
        stream = np.random.default_rng(seed)
        # labels first, then the device sampler's seed: the reference draws z first too
        # (stochasticblockmodel.py:84-87), so a given seed yields the reference's blocks
        self.z = np.sort(stream.integers(0, k, N)) if z is None else np.asarray(z)
        if M is None:
            self.p, self.q = p, (0.3 / k if q is None else q)
            M = _block_probabilities(k, p, q)
        self.M = np.asarray(M, dtype=np.float64)
        if self.M.min() < 0 or self.M.max() > 1:
            raise ValueError("Probabilities should be in [0, 1].")
        ctx = kwargs.get("ctx") or engine.default_context(int(kwargs.get("device", 0)))
        tries, self.sampler_ms = n_try, 0.0
        while True:  # stochasticblockmodel.py:122-157: sample until connected, at most n_try times (None: for ever)
            device_seed = int(stream.integers(0, 2 ** 63))
            # (W stays on the device until somebody reads G.W: unit int64 weights then, like the reference's W)
            W, ms = engine.sbm_graph(self.z, self.M, seed=device_seed, ctx=ctx, keep_on_device=True,
                                     directed=directed, self_loops=self_loops)
            self.sampler_ms += ms
            if not connected:
                break
            trial = Graph(W, reorder="none", tiles=False, ctx=ctx)
            if trial.is_connected():
                W = trial.W  # (downloaded now, for the one trial that is kept: the device handle goes with it)
                break
            if tries is not None:
                tries -= 1
                if tries <= 0:
                    raise ValueError("The graph could not be connected after {} trials. Increase the connection "
                                     "probability or the number of trials.".format(self.n_try))
        self.info = {"node_com": self.z, "comm_sizes": np.bincount(self.z), "world_rad": np.sqrt(N)}
        Graph.__init__(self, W, **kwargs)


class ErdosRenyi(StochasticBlockModel):
    """erdosrenyi.py:49-61: the one-block stochastic block model."""

    def __init__(self, N=100, p=0.1, directed=False, self_loops=False, connected=False, n_try=10,
                 seed=None, **kwargs):
        StochasticBlockModel.__init__(self, N=N, k=1, p=p, directed=directed, self_loops=self_loops,
                                      connected=connected, n_try=n_try, seed=seed, **kwargs)


def __getattr__(name):
    """``graphs.LearnedGraph`` lives in pygsp_amd/graph_learning.py, which builds on this module: resolved on first use."""
    if name == "LearnedGraph":
        from .graph_learning import LearnedGraph
        return LearnedGraph
    raise AttributeError("module {!r} has no attribute {!r}".format(__name__, name))
