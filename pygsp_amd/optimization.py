"""Mirror of pygsp.optimization: the proximal operator of the graph total variation, on the device.

The reference's ``prox_tv`` (pygsp/optimization.py:24-103) cannot run as shipped: it names an undefined ``D`` and an
undefined ``verbose``, hands the problem to a pyunlocbox ``norm_l1`` prox that has no non-tight branch, and returns
nothing.  There is therefore no reference behaviour to reproduce: the algorithm here - FISTA on the dual problem
(Beck & Teboulle 2009), DESIGN.md "Graph total-variation prox" - is this project's choice, and what pins it is the
project's own numpy restatement (tests/prox_tv_helpers.py), not the reference.
"""
import numpy as np

from . import engine

TV_OPTIONS = ("atol", "dtol", "xtol", "verbosity")
TV_MAX_WIDTH = 256


def tv_step(G, nu=1):
    """The fixed dual step 1 / (2 G.lmax nu): the reference's bound on the operator norm is l1_nu = 2 * G.lmax * nu
    (optimization.py:82), twice lambda_max(D D^T), which stays safe when lmax is an estimate from below."""
    return 1.0 / (2.0 * G.lmax * nu)


def _tv_device_graph(G):
    """The float64 device graph holding G's edge list: its own upper triangle, or Graph.get_edge_list handed over
    for a directed graph or one with self-loops (as Graph.grad / Graph.div do for the graph's compute dtype)."""
    dev = engine._float64_device_graph(G)
    if G.is_directed() or G.W.diagonal().any():
        if getattr(G, "_edges_given_to", None) is not dev and getattr(dev, "_tv_edges_from", None) is not G.W:
            sources, targets, weights = G.get_edge_list()
            dev.set_edge_list(sources, targets, weights, directed=G.is_directed())
            dev._tv_edges_from = G.W
    return dev


def prox_tv(x, gamma, G, A=None, At=None, nu=1, tol=10e-4, maxit=200, use_matrix=True, **kwargs):
    """Total-variation proximal operator on the graph G: argmin_z 1/2 ||x - z||_2^2 + gamma ||grad_G z||_1, the
    gradient being ``G.grad`` (D^T z).  x: (N,) or (N, Nsig), a numpy array or an engine.DeviceArray; the result has
    the same shape and kind, float64.

    The reference's function of this name cannot run as shipped (undefined names, no return value, a pyunlocbox prox
    without the branch it asks for), so nothing here claims parity with it: the algorithm is this project's choice,
    pinned by its own numpy restatement.  It is FISTA on the dual problem min_{|u| <= gamma} 1/2 ||x - D u||^2 with
    the fixed step ``tv_step(G, nu)`` = 1 / (2 G.lmax nu), started at u = 0, on the float64 device graph (also for a
    float32 graph), z_k = x - D u_k.  It stops on the first of these that holds for the primal objective obj_k of z_k:
    ``atol`` (obj_k < atol), ``dtol`` (|obj_k - obj_{k-1}| < dtol), ``tol`` (the reference's name for rtol: the same
    difference relative to obj_k; default 10e-4 = 1e-3), ``xtol`` (||z_k - z_{k-1}||_F / sqrt(N Nsig) < xtol) and
    ``maxit`` (default 200).  atol, dtol and xtol come as keywords and default to None (off); ``verbosity`` is
    accepted and ignored, as is ``use_matrix``; any other keyword is a TypeError.  One objective serves all columns of
    a device call, so they stop together; more than 256 columns go in batches of 256, and BATCHES STOP
    INDEPENDENTLY (prox_tv_solve then returns one info per batch).  ``A`` / ``At`` raise NotImplementedError: host
    lambdas cannot run inside the device loop.  A negative or non-finite gamma is a ValueError."""
    z, _ = prox_tv_solve(x, gamma, G, A, At, nu, tol, maxit, use_matrix, **kwargs)
    return z


def prox_tv_solve(x, gamma, G, A=None, At=None, nu=1, tol=10e-4, maxit=200, use_matrix=True, **kwargs):
    """prox_tv that also returns the solver's info dict (niter, crit, objective, ms): one dict for up to 256 columns,
    a list of dicts, one per batch of 256 columns, beyond."""
    engine._refuse_unknown_keywords("prox_tv", kwargs, TV_OPTIONS)
    if A is not None or At is not None:
        raise NotImplementedError("prox_tv: A / At are host functions and cannot run inside the device loop")
    gamma = float(gamma)
    if not (gamma >= 0 and np.isfinite(gamma)):
        raise ValueError("gamma should be finite and >= 0")
    opts = {k: kwargs[k] for k in ("atol", "dtol", "xtol") if k in kwargs}
    opts.update(rtol=tol, maxit=maxit)
    step = tv_step(G, nu)
    dev = _tv_device_graph(G)
    if isinstance(x, engine.DeviceArray):
        if x.cube[1] > TV_MAX_WIDTH:
            raise ValueError("prox_tv: a device signal holds at most {} columns per call".format(TV_MAX_WIDTH))
        return dev.prox_tv(x, gamma, step, **opts)
    x = np.asarray(x, dtype=np.float64)
    if x.ndim not in (1, 2) or x.shape[0] != G.n_vertices:
        raise ValueError("x should be of shape (G.n_vertices,) or (G.n_vertices, Nsig), got {}".format(x.shape))
    if x.ndim == 1 or x.shape[1] <= TV_MAX_WIDTH:
        return dev.prox_tv(x, gamma, step, **opts)
    z, infos = np.empty_like(x), []
    for c0 in range(0, x.shape[1], TV_MAX_WIDTH):
        z[:, c0:c0 + TV_MAX_WIDTH], info = dev.prox_tv(x[:, c0:c0 + TV_MAX_WIDTH], gamma, step, **opts)
        infos.append(info)
    return z, infos
