"""Learning a graph from smooth signals, on the device.

The log-degree model of Kalofolias, "How to learn a graph from smooth signals" (2016): over symmetric non-negative W with
an empty diagonal, minimise ``||W o Z||_1 - a 1^T log(W 1) + (b / 2) ||W||_F^2``, Z the pairwise squared distances of
the observations.  It is made scalable as in Kalofolias & Perraudin, "Large scale graph learning from smooth signals"
(2019): the support is restricted to a k-nearest-neighbour candidate pattern, and the one remaining parameter theta
(which multiplies Z, with a = b = 1) is taken from the sorted neighbour distances so that every vertex keeps about k
edges.  The reference library has no counterpart (GSPBox ships it as ``gsp_learn_graph_log_degrees``): the algorithm -
forward-backward-forward primal-dual iterations with a fixed step, DESIGN.md "Graph learning" - is pinned by this
project's own numpy restatement (tests/graphlearn_helpers.py).  Float64 and undirected patterns only; the l2-degree
model is not covered.
"""
import numpy as np

from . import engine
from .graphs import Graph

MAX_CANDIDATES = 64  # the device neighbour search returns at most 64 neighbours


def _theta_rows(D, k):
    D = np.asarray(D, dtype=np.float64)
    k = int(k)
    if D.ndim != 2 or not 2 <= k < D.shape[1]:
        raise ValueError("theta_bounds: D must be (N, m) sorted neighbour distances with m > k >= 2, got {} and k = {}"
                         .format(D.shape, k))
    Z = D * D
    bk = Z[:, :k].sum(axis=1)
    lo = k * Z[:, k] ** 2 - bk * Z[:, k]
    hi = k * Z[:, k - 1] ** 2 - bk * Z[:, k - 1]
    ok = (lo > 0) & (hi > 0)
    return lo[ok], hi[ok]


def theta_bounds(D, k):
    """The interval of theta in which a vertex keeps exactly k edges, averaged over the vertices (host).  D: (N, m)
    neighbour distances, every row ascending, the point itself not among them, m > k >= 2.  Per row, with Z = D^2 and
    b_k the sum of its k smallest entries, lo = 1 / sqrt(k Z_{k+1}^2 - b_k Z_{k+1}) and hi = 1 / sqrt(k Z_k^2 - b_k
    Z_k) (1-based).  Returns the geometric means (lo, hi) over the rows whose radicands are positive; ValueError if
    there is none.  ``sqrt(lo * hi)`` is the default theta of LearnedGraph."""
    lo, hi = _theta_rows(D, k)
    if lo.size == 0:
        raise ValueError("theta_bounds: no row has a positive radicand (all neighbour distances of a row are equal)")
    return float(np.exp(-0.5 * np.mean(np.log(lo)))), float(np.exp(-0.5 * np.mean(np.log(hi))))


def _check_model(a, b, step):
    a, b, step = float(a), float(b), float(step)
    if not (a > 0 and np.isfinite(a)):
        raise ValueError("a must be positive and finite")
    if not (b >= 0 and np.isfinite(b)):
        raise ValueError("b must be non-negative and finite")
    if not 0 < step < 1:
        raise ValueError("step must lie in (0, 1)")
    return a, b, step


def _learn(G, X, Z, a, b, theta, step, tol, maxit, w0, adjacency, dev=None, dmax=None):
    """What learn_weights and LearnedGraph share.  dev, dmax: the device graph and the largest degree of the pattern
    when the caller knows them (a pattern that still lies on the device)."""
    a, b, step = _check_model(a, b, step)
    if (X is None) == (Z is None):
        raise ValueError("exactly one of X (signals) and Z (squared distances per edge) must be given")
    theta = 1.0 if theta is None else float(theta)
    if not (theta > 0 and np.isfinite(theta)):
        raise ValueError("theta must be positive and finite")
    if dev is None:
        if G.compute_dtype != np.float64:
            raise ValueError("graph learning needs a float64 graph (compute_dtype)")
        if G.is_directed():
            raise ValueError("weights are learned on undirected patterns; the graph is directed")
        dev = G._device_differential()  # (hands a graph with self-loops its own edge list: refused by the library)
    if X is not None:
        # theta z_e = ||sqrt(theta) (x_s - x_t)||^2: the scale goes into the one upload of X, z never leaves the device
        X = np.asarray(X, dtype=np.float64)
        if X.ndim not in (1, 2) or X.shape[0] != G.n_vertices:
            raise ValueError("X should be of shape (G.n_vertices[, features]), got {}".format(X.shape))
        X = X.reshape(X.shape[0], -1)
        Z = dev.edge_sqdist(engine.DeviceArray.from_host(G.context, X if theta == 1.0 else X * np.sqrt(theta)))
    else:
        Z = np.asarray(Z, dtype=np.float64)
        if Z.shape != (G.n_edges,):
            raise ValueError("Z should hold one squared distance per edge, ({},), got {}".format(G.n_edges, Z.shape))
        if Z.size and not (Z.min() >= 0):  # (also NaN)
            raise ValueError("Z holds a negative or NaN entry")
        if theta != 1.0:
            Z = Z * theta
    if dmax is None:
        dmax = int(np.max(G.d)) if G.n_vertices else 0
    gamma = step / (2.0 * b + np.sqrt(2.0 * dmax)) if dmax > 0 or b > 0 else step
    return dev.learn_log_degrees(Z, a, b, gamma, tol=tol, maxit=maxit, w0=w0, adjacency=adjacency)


def learn_weights(G, X=None, *, Z=None, a=1.0, b=1.0, theta=None, step=0.5, tol=1e-5, maxit=10000, w0=None):
    """Weights of the log-degree model on the pattern of the undirected graph G (its weights are not read): argmin over
    w >= 0 of ``2 z^T w - a sum_i log (S w)_i + b ||w||^2``, (S w)_i the sum of w over the edges at vertex i.  Exactly
    one of ``X`` ((N, F) signals or features, 1 <= F <= 4096: z_e = ||X_s - X_t||^2 on the device) and ``Z`` (one squared
    distance per edge, ``G.get_edge_list`` order) is given, as numpy arrays; ``theta`` (default 1) multiplies z (for X it
    scales the signals by sqrt(theta) before they are uploaded).  Primal-dual iterations
    with the fixed step ``gamma = step / (2 b + sqrt(2 max(G.d)))``, 0 < step < 1, from ``w0`` (zeros), stopped when both
    relative residuals are <= tol (None: off) or after maxit iterations.  Returns (w, info): w in edge order,
    non-negative with exact zeros, float64; info = {'niter', 'crit' ('TOL' or 'MAXIT'), 'history', 'ms', 'w_last'} -
    'w_last' is the last (only approximately feasible) iterate, the warm start of a continued run.  ValueError for a
    float32 or directed graph, a graph with self-loops, a <= 0, b < 0, step outside (0, 1), bad Z."""
    P, w, _, info = _learn(G, X, Z, a, b, theta, step, tol, maxit, w0, False)
    info["w_last"] = np.asarray(w)
    return np.asarray(P), info


class LearnedGraph(Graph):
    """A graph learned from the rows of X ((N, F), 1 <= F <= 4096) by the log-degree model with about k neighbours per
    vertex.  The candidate pattern is the symmetrised (``'maximum'``) k-NN graph of X with ``candidates`` neighbours
    (default min(3 k, 64); k < candidates <= 64), built on the device; only its pattern is used.  z is the squared
    distance along every candidate edge, theta (unless given) ``sqrt(lo * hi)`` of ``theta_bounds`` on the builder's
    sorted distances, and the weights solve ``learn_weights`` with z theta, a and b.  The learned adjacency is
    assembled on the device and handed to ``Graph.__init__`` where it lies - nothing of W crosses PCIe until ``G.W`` is
    read - with the leading (up to three) columns of X as coordinates, as NNGraph does.  Attributes: ``theta``,
    ``learn_info`` (niter, crit, history, ms), ``candidate_edges``.  kwargs go to Graph."""

    def __init__(self, X, k=10, candidates=None, theta=None, a=1.0, b=1.0, tol=1e-5, maxit=10000, **kwargs):
        self.Xin = X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("X must be (N, F)")
        k = int(k)
        candidates = min(3 * k, MAX_CANDIDATES) if candidates is None else int(candidates)
        if k < 2:
            raise ValueError("k must be at least 2")
        if candidates <= k:
            raise ValueError("candidates ({}) must exceed k ({})".format(candidates, k))
        if candidates > MAX_CANDIDATES:
            raise ValueError("candidates must be at most {} (the device neighbour search)".format(MAX_CANDIDATES))
        if X.shape[0] <= candidates:
            raise ValueError("The number of candidates ({}) must be smaller than the number of nodes ({})."
                             .format(candidates, X.shape[0]))
        _check_model(a, b, 0.5)
        self.k, self.candidates, self.a, self.b = k, candidates, float(a), float(b)
        ctx = kwargs.get("ctx") or engine.default_context(int(kwargs.get("device", 0)))
        pattern, _, found = engine.knn_graph(X, candidates, ctx=ctx, neighbors=True, symmetrize="maximum",
                                             keep_on_device=True)
        self.theta = float(np.sqrt(np.prod(theta_bounds(found["D"], k)))) if theta is None else float(theta)
        base = Graph(pattern, compute_dtype=np.float64, reorder="none", tiles=False, ctx=ctx)
        self.candidate_edges = base.n_edges
        dev = base.device_graph()
        if base.n_edges:  # the degrees of the pattern from its edge list: the pattern itself stays on the device
            src, dst, _ = dev.edge_list()
            dmax = int((np.bincount(src, minlength=base.N) + np.bincount(dst, minlength=base.N)).max())
        else:
            dmax = 0
        _, _, W, self.learn_info = _learn(base, X, None, a, b, self.theta, 0.5, tol, maxit, None, True, dev=dev,
                                          dmax=dmax)
        Graph.__init__(self, W, coords=X[:, :3], **kwargs)
