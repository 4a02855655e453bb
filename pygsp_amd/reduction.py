"""Mirror of the deterministic part of pygsp.reduction: Kron reduction, interpolation and graph pyramids on the device.

Every function takes the kept vertices as an input; nothing is sampled.  With kept set k, eliminated set u and
A = L + sigma I the Schur complement A_kk - A_ku A_uu^-1 A_uk equals rows k of A X, where X extends the indicator
columns of the kept vertices by A_uu X_u = -A_uk - a harmonic extension at a shift.  The reference solves A_uu directly
(spsolve, reduction.py:350-358); here the batched conjugate-gradient loop of the harmonic learners solves it on the
device (gspx_schur_cg_dev, gspx_kron_build; DESIGN.md "Graph reduction").

``interpolate`` needs no dense K_reg: K_reg f is rows k of A x with x the shifted extension of f - one solve per signal
column - and with an exact Green's kernel the interpolated signal is x itself (``method='exact'``).

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
