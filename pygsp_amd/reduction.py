"""Mirror of the deterministic part of pygsp.reduction: Kron reduction, interpolation and graph pyramids on the device.

Every function takes the kept vertices as an input; nothing is sampled.  With kept set k, eliminated set u and
A = L + sigma I the Schur complement A_kk - A_ku A_uu^-1 A_uk equals rows k of A X, where X extends the indicator
columns of the kept vertices by A_uu X_u = -A_uk - a harmonic extension at a shift.  The reference solves A_uu directly
(spsolve, reduction.py:350-358); here the batched conjugate-gradient loop of the harmonic learners solves it on the
device (gspx_schur_cg_dev, gspx_kron_build; DESIGN.md "Graph reduction").

``interpolate`` needs no dense K_reg: K_reg f is rows k of A x with x the shifted extension of f - one solve per signal
column - and with an exact Green's kernel the interpolated signal is x itself (``method='exact'``).

``coarsen`` - an extension, the reference has no counterpart - is multilevel coarsening by heavy-edge matching (the
Graclus / METIS family) for pooling layers: handshake rounds on the device (gspx_match_heavy_edges), the coarse graphs
P^T W P assembled on the device (gspx_coarsen_build) and the vertex-to-cluster maps through which ``Coarsening.pool`` /
``unpool`` and ``pygsp_amd.nn.GraphPool`` move signals (gspx_segment_pool_dev; DESIGN.md "Coarsening and pooling").
``heavy_edge_matching_host`` and ``coarsen_host`` restate the two device algorithms in numpy, round for round and sum
for sum.

Not provided: graph_sparsify (and so ``graph_multiresolution(sparsify=True)``), tree_multiresolution, least-squares
pyramid synthesis.
"""
import numpy as np
from scipy import sparse
from scipy.sparse import linalg as splinalg

from . import engine, filters, graphs

SPARSIFY_MESSAGE = ("graph_sparsify is not provided (spectral sparsification samples edges at random); call "
                    "graph_multiresolution(..., sparsify=False)")


def split_laplacian(M):
    """(W, sigma) when the sparse matrix M is Lap(W) + sigma I - symmetric, non-positive off-diagonals, one constant
    non-negative row sum (to 1e-12 of its largest entry) - else None."""
    M = sparse.csr_matrix(M, dtype=np.float64)
    if M.shape[0] != M.shape[1] or abs(M - M.T).max() != 0:
        return None
    off = M - sparse.diags(M.diagonal())
    off.eliminate_zeros()
    if off.nnz and off.data.max() > 0:
        return None
    rows = np.asarray(M.sum(axis=1)).ravel()
    sigma = float(np.median(rows)) if rows.size else 0.0
    scale = max(float(abs(M).max()), 1.0)
    if sigma < -1e-12 * scale or np.abs(rows - sigma).max() > 1e-12 * scale * max(M.shape[0], 1) ** 0.5:
        return None
    return sparse.csr_matrix(-off), max(sigma, 0.0)


def kron_reduction_host(L, ind):
    """The reference's formula (reduction.py:350-362) with scipy, for matrices the device route does not take."""
    L = sparse.csr_matrix(L)
    N = L.shape[0]
    comp = np.setdiff1d(np.arange(N, dtype=int), ind)
    Lnew = L[np.ix_(ind, ind)]
    if comp.size:
        inner = splinalg.spsolve(L[np.ix_(comp, comp)].tocsc(), L[np.ix_(comp, ind)].tocsc())
        inner = sparse.csc_matrix(inner.reshape(comp.size, len(ind)) if not sparse.issparse(inner) else inner)
        Lnew = Lnew - L[np.ix_(ind, comp)].dot(inner)
    if np.abs(Lnew - Lnew.T).sum() < np.spacing(1) * np.abs(Lnew).sum():
        Lnew = (Lnew + Lnew.T) / 2.0
    return Lnew


def _is_graph(G):
    return hasattr(G, "lap_type") and hasattr(G, "is_directed")


def kron_reduction(G, ind, rtol=1e-10, maxiter=None):
    """Kron reduction of a graph or a sparse matrix onto the vertices `ind` (reduction.py:309-381): the Schur complement
    of the Laplacian with respect to the eliminated vertices.  Vertex ind[c] becomes vertex c.

    A Graph (combinatorial Laplacian, undirected; otherwise the reference's NotImplementedError) gives a Graph whose
    adjacency W = max(0, -offdiag(Lnew)) was built on the device and stays there until somebody reads ``.W``;
    ``coords`` and ``plotting`` are carried over.  The diagonal of W is always empty: the reference's self-loop branch
    (``norm(Snew) >= spacing(1000)``) triggers on rounding alone and its result is then "removed for stability".

    A sparse matrix of the form Lap(W) + sigma I (``split_laplacian``) is reduced on the device at that shift and comes
    back as a CSR matrix of its non-zeros, like the reference's; any other matrix takes
    ``kron_reduction_host``.

    The eliminated block is solved by conjugate gradients (`rtol`, default 1e-10; `maxiter`, default 10 N) where the
    reference solves directly.  After m iterations the solve has reached m hops: entries of the result whose two
    vertices lie further apart are exact zeros here, where a direct solve leaves values below the tolerance, and every
    entry dropped that way is smaller than the tolerance.  Empty, repeated or out-of-range `ind` is a ValueError."""
    if _is_graph(G):
        if G.lap_type != "combinatorial":
            raise NotImplementedError("Unknown reduction for {} Laplacian.".format(G.lap_type))
        if G.is_directed():
            raise NotImplementedError("This method only work for undirected graphs.")
        ind = engine.check_kept(ind, G.N)
        _, W, iters, info = engine._float64_device_graph(G).kron(ind, 0.0, rtol, maxiter, dense=False, adjacency=True)
        if W.nnz == 0:
            W = W.download()
        coords = getattr(G, "coords", None)
        coords = np.asarray(coords)[ind] if coords is not None and np.ndim(coords) else None
        kwargs = {"compute_dtype": G.compute_dtype} if hasattr(G, "compute_dtype") else {}
        Gnew = graphs.Graph(W, coords=coords, lap_type=G.lap_type, plotting=G.plotting, **kwargs)
        Gnew.kron_info = dict(info, iterations=iters)
        return Gnew
    if not sparse.issparse(G):
        raise TypeError("kron_reduction takes a Graph or a scipy sparse matrix")
    ind = engine.check_kept(ind, G.shape[0])
    parts = split_laplacian(G)
    if parts is None:
        return kron_reduction_host(G, ind)
    dev = engine.DeviceGraph.from_w(parts[0], dtype=np.float64)
    try:
        Lnew = dev.kron(ind, parts[1], rtol, maxiter)[0]
    finally:
        dev.destroy()
    return sparse.csr_matrix(Lnew)


def interpolate(G, f_subsampled, keep_inds, order=100, reg_eps=0.005, method="chebyshev", **kwargs):
    """Interpolate a signal known on `keep_inds` to every vertex of G (reduction.py:150-193; Pesenson's variational
    splines).  Works on any graph: ``G.mr`` is not needed and no dense K_reg is formed.

    alpha = K_reg f is rows keep_inds of (L + reg_eps I) x, with x the extension of f that solves the eliminated rows
    (DeviceGraph.schur_cg at shift reg_eps, conjugate gradients; keywords ``rtol`` / ``maxiter``).  ``'chebyshev'``:
    the zero-filled alpha goes through the Green's kernel 1 / (reg_eps + lambda) as a Chebyshev filter of `order` on
    the device, without visiting the host in between; other keywords go to ``Filter.filter``.  ``'exact'``: with the
    exact kernel the result is x itself - no Fourier basis, no filter.

    f_subsampled: (nk,) or (nk, Nv), numpy or engine.DeviceArray; the result is (N, Nv) - (N, 1) for a 1-D input, as
    the reference's - of the same kind (a DeviceArray's nk rows pass through the host once, for the scatter to N rows;
    alpha and the result do not)."""
    keep = engine.check_kept(keep_inds, G.N)
    on_device = isinstance(f_subsampled, engine.DeviceArray)
    f = np.asarray(f_subsampled, dtype=np.float64)
    if f.ndim not in (1, 2) or f.shape[0] != keep.size:
        raise ValueError("f_subsampled must be ({0},) or ({0}, Nv), got {1}".format(keep.size, f.shape))
    if method not in ("chebyshev", "exact"):
        raise ValueError("Unknown method {}.".format(method))
    rtol, maxiter = kwargs.pop("rtol", None), kwargs.pop("maxiter", None)
    f2 = f.reshape(keep.size, -1)
    nv = f2.shape[1]
    dev = filters._device_graph_of(G)
    full = np.zeros((G.N, nv), dtype=dev.dtype)
    full[keep] = f2
    mask = np.zeros(G.N, dtype=dev.dtype)
    mask[keep] = 1
    out = engine.DeviceArray.empty(dev.ctx, (G.N, nv, 1), dev.dtype)
    exact = method == "exact"
    with dev.ctx._temporaries() as t:
        bm, bf = t.upload(mask), t.upload(full)
        if nv:
            dev.schur_cg_dev(reg_eps, bm.ptr, bf.ptr, out.ptr if exact else None, None if exact else out.ptr, nv,
                             rtol=rtol, maxiter=maxiter)
    if not exact and nv:
        green = filters.Filter(G, lambda x: 1.0 / (reg_eps + x))
        out = filters.filter_signals(green, out, "chebyshev", order, **kwargs)
    out.shape = (G.N, nv)
    return out if on_device else np.asarray(out).reshape(G.N, nv)


def _largest_eigenvector_set(G):
    """The polarity set of the eigenvector of the largest eigenvalue (reduction.py:271-278), made positive at vertex 0."""
    if getattr(G, "_U", None) is not None:
        V = np.array(G.U[:, -1], dtype=np.float64)
    elif G.N < 3:
        V = np.linalg.eigh(G.L.toarray())[1][:, -1]
    else:
        V = splinalg.eigsh(G.L.asfptype() if hasattr(G.L, "asfptype") else G.L, 1, which="LA")[1][:, 0]
    V = V * (np.sign(V[0]) or 1.0)
    return np.nonzero(V >= 0)[0]


def graph_multiresolution(G, levels, sparsify=True, sparsify_eps=None, downsampling_method="largest_eigenvector",
                          reduction_method="kron", compute_full_eigen=False, reg_eps=0.005):
    """A pyramid of graphs by repeated downsampling and Kron reduction (reduction.py:196-306), the reference's
    signature.  ``sparsify=True`` - the default - raises NotImplementedError: graph_sparsify is not provided (the
    reference's own fails on a current SciPy).  `downsampling_method`: 'largest_eigenvector' (``U[:, -1]`` when a
    basis is present, else ``eigsh(L, 1, which='LA')`` on the host) or - an extension - a callable
    ``(G, level) -> ind`` that fixes the kept vertices.  Every graph gets ``mr`` with ``idx``, ``orig_idx``, ``level``
    (from level 1 on) and ``green_kernel`` (all but the last); the dense ``K_reg`` is not stored - nothing reads it."""
    if sparsify:
        raise NotImplementedError(SPARSIFY_MESSAGE)
    if not callable(downsampling_method) and downsampling_method != "largest_eigenvector":
        raise NotImplementedError("Unknown graph downsampling method.")
    if reduction_method != "kron":
        raise NotImplementedError("Unknown graph reduction method.")

    def spectrum(g):
        if compute_full_eigen:
            g.compute_fourier_basis()
        else:
            g.estimate_lmax()

    spectrum(G)
    Gs = [G]
    G.mr = {"idx": np.arange(G.N), "orig_idx": np.arange(G.N)}
    for i in range(levels):
        if callable(downsampling_method):
            ind = np.asarray(downsampling_method(Gs[i], i))
        else:
            ind = _largest_eigenvector_set(Gs[i])
        Gs.append(kron_reduction(Gs[i], ind))
        spectrum(Gs[i + 1])
        Gs[i + 1].mr = {"idx": ind, "orig_idx": Gs[i].mr["orig_idx"][ind], "level": i}
        Gs[i].mr["green_kernel"] = filters.Filter(Gs[i], lambda x: 1.0 / (reg_eps + x))
    return Gs


def _as_columns(f, n):
    f = np.asarray(f, dtype=np.float64)
    if f.ndim == 1:
        f = f[:, None]
    if f.ndim != 2 or f.shape[0] != n:
        raise ValueError("the signal must be ({0},) or ({0}, Nv), got {1}".format(n, f.shape))
    return f


def pyramid_analysis(Gs, f, **kwargs):
    """Graph pyramid transform (reduction.py:384-449): per level the low-passed signal on the kept vertices and the
    error of predicting the finer signal from it by ``interpolate``.  Returns (ca, pe).  ``h_filters``: one kernel or
    one per level, default 1 / (2x + 1); other keywords go to the filter and to ``interpolate``, as in the reference.
    A 1-D `f` is treated as (N, 1): the reference broadcasts its (N,) signal against the (N, 1) prediction into an
    N x N "prediction error"."""
    if np.shape(f)[0] != Gs[0].N:
        raise ValueError("PYRAMID ANALYSIS: The signal to analyze should have the same dimension as the first graph.")
    levels = len(Gs) - 1
    h_filters = kwargs.pop("h_filters", lambda x: 1.0 / (2 * x + 1))
    if not isinstance(h_filters, list):
        if not callable(h_filters):
            raise ValueError("Filters must be a list of functions.")
        h_filters = [h_filters]
    if len(h_filters) == 1:
        h_filters = h_filters * levels
    elif len(h_filters) != levels:
        raise ValueError("The number of filters must be one or equal to {}.".format(levels))
    solver = {k: kwargs.pop(k) for k in ("rtol", "maxiter", "reg_eps") if k in kwargs}
    ca, pe = [_as_columns(f, Gs[0].N)], []
    for i in range(levels):
        idx = Gs[i + 1].mr["idx"]
        s_low = np.asarray(filters.Filter(Gs[i], h_filters[i]).filter(ca[i], **kwargs)).reshape(ca[i].shape)
        ca.append(s_low[idx])
        pe.append(ca[i] - interpolate(Gs[i], ca[i + 1], idx, **solver, **kwargs))
    return ca, pe


def pyramid_synthesis(Gs, cap, pe, order=30, **kwargs):
    """Synthesis from the coarsest approximation and the prediction errors (reduction.py:452-531): level by level
    ``interpolate(...) + pe``.  Returns (reconstruction, ca).  The signal comes back exactly only when `order` is the
    one the analysis interpolated with - the defaults are the reference's, 100 there and 30 here.  ``least_squares=True`` raises NotImplementedError (the
    reference's raises NameError); ``use_landweber`` and ``h_filters`` belong to it and are ignored."""
    if bool(kwargs.pop("least_squares", False)):
        raise NotImplementedError("least-squares pyramid synthesis is not provided")
    kwargs.pop("use_landweber", None)
    kwargs.pop("h_filters", None)
    reg_eps = float(kwargs.pop("reg_eps", 0.005))
    levels = len(Gs) - 1
    if len(pe) != levels:
        raise ValueError("Gs and pe have different shapes.")
    ca = [_as_columns(cap, Gs[levels].N)]
    for i in range(levels):
        fine = Gs[levels - i - 1]
        s_pred = interpolate(fine, ca[i], Gs[levels - i].mr["idx"], order=order, reg_eps=reg_eps, **kwargs)
        ca.append(s_pred + _as_columns(pe[levels - i - 1], fine.N))
    ca.reverse()
    return ca[0], ca


# ---- multilevel coarsening by heavy-edge matching -------------------------------------------------------------------
MATCH_METRICS = ("normalized_cut", "weight")


def _undirected_csr(W):
    W = sparse.csr_matrix(W, dtype=np.float64)
    if W.shape[0] != W.shape[1]:
        raise ValueError("the adjacency must be square")
    if (W != W.T).nnz:
        raise ValueError("coarsening needs an undirected graph (a symmetric adjacency)")
    W.sum_duplicates()
    W.sort_indices()
    return W


def heavy_edge_matching_host(W, d=None, metric="normalized_cut", max_rounds=None):
    """The device matching (gspx_match_heavy_edges) restated in numpy: the same rounds, the same scores and the same
    tie-break.  W: symmetric sparse adjacency (its diagonal is ignored: a self-loop is no candidate); d: the weighted
    degrees the scores use (default: the row sums of W without its diagonal; hand over ``download_dw()`` to score the
    device's own bits).  score(i, j) = w_ij (1 / d_i + 1 / d_j) for 'normalized_cut', w_ij for 'weight'.  Per round every
    unmatched vertex proposes to its unmatched neighbour of largest score, ties to the smaller index, and mutual
    proposals are matched; the loop ends at the first round that matches nothing or after `max_rounds` rounds.  A path
    with monotone weights matches one pair per round: N / 2 rounds.
    Returns (mate int32 with mate[i] == i for a singleton, rounds that matched something, pairs)."""
    if metric not in MATCH_METRICS:
        raise ValueError("Unknown metric {!r}: 'normalized_cut' or 'weight'".format(metric))
    if max_rounds is not None and int(max_rounds) < 0:
        raise ValueError("max_rounds must be None or non-negative")
    W = _undirected_csr(W)
    N = W.shape[0]
    C = W.tocoo()
    off = C.row != C.col
    rows, cols, w = C.row[off], C.col[off], C.data[off]
    if d is None:
        d = np.bincount(rows, weights=w, minlength=N)
    d = np.asarray(d, dtype=np.float64)
    if d.shape != (N,):
        raise ValueError("d must hold one degree per vertex")
    with np.errstate(divide="ignore"):
        inv = 1.0 / d
    score = w if metric == "weight" else w * (inv[rows] + inv[cols])
    mate = np.full(N, -1, dtype=np.int64)
    rounds = 0
    while max_rounds is None or rounds < int(max_rounds):
        live = (mate[rows] < 0) & (mate[cols] < 0)
        r, c, s = rows[live], cols[live], score[live]
        order = np.lexsort((c, -s, r))  # per row: largest score first, then the smaller column
        r, c = r[order], c[order]
        first = np.ones(r.size, dtype=bool)
        first[1:] = r[1:] != r[:-1]
        prop = np.full(N, -1, dtype=np.int64)
        prop[r[first]] = c[first]
        i = np.flatnonzero(prop >= 0)
        i = i[prop[prop[i]] == i]
        if i.size == 0:
            break
        mate[i] = prop[i]
        rounds += 1
    single = mate < 0
    mate[single] = np.flatnonzero(single)
    return mate.astype(np.int32), rounds, int(np.count_nonzero(mate > np.arange(N)))


def parent_of(mate):
    """(parent int32, n_clusters) of a matching: cluster c is the rank of its smaller member among all cluster
    representatives in ascending order, so `parent` is monotone in the representative."""
    mate = np.asarray(mate)
    rep = np.minimum(mate, np.arange(mate.size))
    is_rep = rep == np.arange(mate.size)
    rank = np.cumsum(is_rep) - 1
    return rank[rep].astype(np.int32), int(np.count_nonzero(is_rep))


def coarsen_host(W, parent):
    """The device build (gspx_coarsen_build) restated in numpy: Wc = P^T W P without its diagonal, P the N x Nc cluster
    indicator of `parent` (Nc = max(parent) + 1, every cluster non-empty).  An entry above the diagonal is the sum of
    its fine entries in ascending (fine row, fine column) order, one term at a time; the entry below the diagonal is
    its copy, so the result equals its transpose bit for bit.  Returns a canonical CSR matrix (float64)."""
    W = _undirected_csr(W)
    N = W.shape[0]
    parent = np.asarray(parent)
    if parent.ndim != 1 or parent.size != N:
        raise ValueError("parent must hold one cluster per vertex ({}), got shape {}".format(N, parent.shape))
    nc = int(parent.max()) + 1 if N else 0
    parent = engine.check_parent(parent, N, nc).astype(np.int64)
    C = W.tocoo()  # (canonical CSR: row-major, columns ascending)
    cr, cd = parent[C.row], parent[C.col]
    up = cr < cd
    cr, cd, v = cr[up], cd[up], C.data[up]
    order = np.lexsort((np.arange(v.size), cd, cr))  # stable: (fine row, fine column) order survives inside a group
    cr, cd, v = cr[order], cd[order], v[order]
    head = np.ones(v.size, dtype=bool)
    head[1:] = (cr[1:] != cr[:-1]) | (cd[1:] != cd[:-1])
    group = np.cumsum(head) - 1
    start = np.flatnonzero(head)
    place = np.arange(v.size) - start[group] if v.size else np.zeros(0, dtype=np.int64)
    acc = np.zeros(start.size)
    for t in range(int(place.max()) + 1 if v.size else 0):  # term t of every group: one addition each, in order
        sel = place == t
        acc[group[sel]] = acc[group[sel]] + v[sel] if t else v[sel]
    U = sparse.coo_matrix((acc, (cr[head], cd[head])), shape=(nc, nc))
    Wc = sparse.csr_matrix(U + U.T)
    Wc.sort_indices()
    return Wc


class Coarsening:
    """What ``coarsen`` returns: ``graphs`` [G_0 = G, ..., G_levels], ``parents`` (per level the int32 map of a
    vertex of G_l to its cluster in G_{l+1}) and ``info`` (per level 'rounds', 'pairs', 'singletons', 'kernel_ms' of
    the matching and 'build_kernel_ms' of the coarse graph).  ``segments(lo, hi)`` is the composed partition of the
    vertices of G_lo into those of G_hi as an engine.Segments, uploaded once and cached; ``pool`` / ``unpool`` move
    signals through it on the device."""

    def __init__(self, graphs_, parents, info):
        self.graphs, self.parents, self.info = list(graphs_), list(parents), list(info)
        self._segments = {}

    @property
    def levels(self):
        return len(self.parents)

    def _span(self, lo, hi):
        hi = self.levels if hi is None else int(hi)
        lo = int(lo)
        if not 0 <= lo < hi <= self.levels:
            raise ValueError("need 0 <= lo < hi <= {}, got lo = {}, hi = {}".format(self.levels, lo, hi))
        return lo, hi

    def parent(self, lo=0, hi=None):
        """The composed cluster map from level `lo` to level `hi` (host)."""
        lo, hi = self._span(lo, hi)
        p = self.parents[lo]
        for level in range(lo + 1, hi):
            p = self.parents[level][p]
        return p

    def segments(self, lo=0, hi=None):
        lo, hi = self._span(lo, hi)
        if (lo, hi) not in self._segments:
            # (the coarse graphs are this package's own and live on the context that coarsened G_0)
            self._segments[lo, hi] = engine.Segments.from_parent(self.graphs[-1].context, self.parent(lo, hi),
                                                                 self.graphs[hi].N)
        return self._segments[lo, hi]

    def pool(self, x, lo=0, hi=None, mode="max"):
        """`x` on the vertices of G_lo ((N_lo, ...) numpy array or engine.DeviceArray) pooled to those of G_hi (default:
        the coarsest): 'max', 'mean' or 'sum' over every cluster, members in ascending order.  Returns the same kind."""
        seg = self.segments(lo, hi)
        return engine.segment_pool(seg.ctx, seg, x, mode)

    def pool_vjp(self, g, x=None, lo=0, hi=None, mode="max"):
        """The vector-Jacobian product of ``pool`` (engine.segment_pool_vjp): `g` on G_hi back to G_lo."""
        seg = self.segments(lo, hi)
        return engine.segment_pool_vjp(seg.ctx, seg, g, x, mode)

    def unpool(self, y, lo=0, hi=None):
        """`y` on the vertices of G_hi copied to every member on G_lo (the 'sum' vjp).  Returns the same kind."""
        seg = self.segments(lo, hi)
        return engine.segment_unpool(seg.ctx, seg, y)


def _matching_device_graph(G):
    """The float64 device graph the matching and the build read: G's own when its Laplacian is combinatorial (the
    weights are its off-diagonals), else a combinatorial one made from G.W for the call.  Returns (dev, temporary)."""
    if G.lap_type == "combinatorial":
        return engine._float64_device_graph(G), False
    return engine.DeviceGraph.from_w(G.W, "combinatorial", dtype=np.float64, ctx=getattr(G, "context", None)), True


def coarsen(G, levels=1, metric="normalized_cut", max_rounds=None):
    """Multilevel coarsening of G by heavy-edge matching: per level a maximal matching by handshake rounds
    (engine.DeviceGraph.match_heavy_edges; `metric` 'normalized_cut' - Graclus' w_ij (1 / d_i + 1 / d_j) - or
    'weight'; `max_rounds` None runs to maximality, and a path with monotone weights needs N / 2 rounds), matched pairs
    merged, and the coarse graph Wc = P^T W P without its diagonal assembled on the device
    (engine.DeviceGraph.coarsen) and set up there without a host round trip.  Cluster c is the rank of its smaller
    member among the representatives, so a local vertex order stays local.  ``lap_type``, ``compute_dtype`` and
    ``plotting`` are carried over; ``coords`` are the mean of the members' coordinates when G has them.  A level that
    matches nothing (no edges left) returns the same graph one level up.  Returns a ``Coarsening``.
    ValueError for a directed graph."""
    if not _is_graph(G):
        raise TypeError("coarsen takes a Graph")
    if G.is_directed():
        raise ValueError("coarsening needs an undirected graph")
    if metric not in MATCH_METRICS:
        raise ValueError("Unknown metric {!r}: 'normalized_cut' or 'weight'".format(metric))
    if int(levels) < 1:
        raise ValueError("levels must be at least 1")
    Gs, parents, infos = [G], [], []
    for _ in range(int(levels)):
        fine = Gs[-1]
        dev, temporary = _matching_device_graph(fine)
        try:
            mate, info = dev.match_heavy_edges(metric, max_rounds)
            parent, nc = parent_of(mate)
            W, build = dev.coarsen(parent, nc)
        finally:
            if temporary:
                dev.destroy()
        if W.nnz == 0:
            W = W.download()
        coords = getattr(fine, "coords", None)
        if coords is not None and np.ndim(coords) == 2 and np.shape(coords)[0] == fine.N:
            sums = np.zeros((nc, np.shape(coords)[1]))
            np.add.at(sums, parent, np.asarray(coords, dtype=np.float64))
            coords = sums / np.bincount(parent, minlength=nc)[:, None]
        else:
            coords = None
        kwargs = {"compute_dtype": fine.compute_dtype} if hasattr(fine, "compute_dtype") else {}
        if getattr(fine, "_ctx", None) is not None:
            kwargs["ctx"] = fine._ctx
        Gs.append(graphs.Graph(W, coords=coords, lap_type=fine.lap_type, plotting=fine.plotting, **kwargs))
        parents.append(parent)
        infos.append(dict(info, build_kernel_ms=build["kernel_ms"], build_ms=build["build_ms"]))
    return Coarsening(Gs, parents, infos)
