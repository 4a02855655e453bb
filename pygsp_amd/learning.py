"""Mirror of pygsp.learning for the solver loops that run on the device.

regression_tikhonov / classification_tikhonov with tau > 0 solve (diag(M) + tau L) x = M y by
conjugate gradients (pygsp/learning.py:324-337, one scipy.sparse.linalg.cg call per column); here
all columns advance together on the GPU with the same recurrence and stopping rule
(gspx_tikhonov_cg_dev).

tau = 0, the reference's default, is harmonic interpolation: x = y on the measured vertices and L_uu x_u = -L_ul y_l
on the others, which the reference hands to a direct sparse solve (spsolve, learning.py:349-367).  L_uu is symmetric
positive definite on every component that holds a measured vertex, so the same conjugate-gradient loop solves it on
the device (gspx_dirichlet_cg_dev, DESIGN.md "Harmonic extension").  It is an iterative answer where the reference
gives a direct one, so it is opt-in: ``solver="cg"``; without it tau = 0 raises as before.

classification_tikhonov_simplex (learning.py:111-180) keeps every row of the solution on the probability simplex.
The reference hands it to pyunlocbox's accelerated forward-backward solver; here the same iteration runs on the
device (gspx_tikhonov_simplex_dev, DESIGN.md "Simplex-constrained classification") and pyunlocbox is not needed.
"""
import numpy as np

from . import engine


def _one_hot(labels):
    """Integer class labels -> (N, classes) indicator matrix (what learning.py:36-39 calls logits)."""
    labels = np.asarray(labels, dtype=np.int64)
    return (labels[:, np.newaxis] == np.arange(labels.max() + 1)[np.newaxis, :]).astype(np.float64)


def _measured_only(y, mask):
    """A float copy of y with every unmeasured vertex set to zero (learning.py:325-326)."""
    keep = np.asarray(mask).reshape(-1).astype(bool)
    out = np.array(y, copy=True)
    out[~keep] = 0
    return out, keep


def regression_tikhonov(G, y, M, tau=0, rtol=None, atol=0.0, maxiter=None, solver=None):
    """argmin_x ||M x - y||^2 + tau x^T L x for tau > 0 (learning.py:254-337); for tau = 0 and ``solver="cg"``
    argmin_x x^T L x subject to x = y on the measured vertices (learning.py:349-367).

    y: (N,) or (N, Nsig) measurements, M: boolean mask of the measured vertices.  rtol / atol /
    maxiter are scipy.sparse.linalg.cg's; rtol None is 1e-5 for tau > 0 (the reference uses scipy's defaults) and,
    for tau = 0, 1e-10 on a float64 graph and 1e-5 on a float32 one (the reference solves that branch directly).
    solver: None or "cg".  tau = 0 runs on the device with "cg" only and raises NotImplementedError without it; on
    a component without a measured vertex the "cg" answer is zero (the reference's spsolve fails there).
    """
    if np.size(M) != G.n_vertices:
        raise ValueError("M should be of size [G.n_vertices,]")
    if solver not in (None, "cg"):
        raise ValueError("solver must be None or 'cg', got {!r}".format(solver))
    rhs, keep = _measured_only(y, M)
    if tau > 0:
        solution, _, _ = G.device_graph().tikhonov_cg(tau, keep, rhs, rtol=1e-5 if rtol is None else rtol, atol=atol,
                                                      maxiter=maxiter)
    elif tau == 0 and solver == "cg":
        solution, _, _ = G.device_graph().dirichlet_cg(keep, rhs, rtol=rtol, atol=atol, maxiter=maxiter)
    else:
        raise NotImplementedError("tau = 0 is a direct sparse solve in the reference (learning.py:342-367); pass "
                                  "solver=\"cg\" for conjugate gradients on the device, or use tau > 0")
    return solution


def classification_tikhonov(G, y, M, tau=0, **kwargs):
    """Tikhonov regression of the one-hot encoded labels (learning.py:170-251); the keywords are
    regression_tikhonov's (tau = 0 needs ``solver="cg"``)."""
    labels, _ = _measured_only(y, M)
    return regression_tikhonov(G, _one_hot(labels), M, tau, **kwargs)


SIMPLEX_OPTIONS = ("rtol", "atol", "dtol", "xtol", "maxit", "verbosity")
SIMPLEX_MAX_CLASSES = 256


def simplex_labels(y, M):
    """(labels, n_classes) of the simplex solver: y copied, zeroed where unmeasured and cast to int (NaN may sit at
    unmeasured vertices), n_classes = max + 1 of those, labels = the class where measured and -1 elsewhere (learning.py:
    120-123).  A negative or NaN measured label is a ValueError: the reference would index the last column with it."""
    keep = np.asarray(M).reshape(-1).astype(bool)
    yz = np.array(y, dtype=np.float64, copy=True).reshape(-1)
    yz[~keep] = 0
    if not np.isfinite(yz).all():
        raise ValueError("measured labels must be finite")
    yi = yz.astype(int)
    if (yi < 0).any():
        raise ValueError("labels must be >= 0 at measured vertices")
    n_classes = int(yi.max()) + 1 if yi.size else 1
    if n_classes > SIMPLEX_MAX_CLASSES:
        raise ValueError("at most {} classes are supported, got {}".format(SIMPLEX_MAX_CLASSES, n_classes))
    return np.where(keep, yi, -1).astype(np.int32), n_classes


def simplex_step(G, tau):
    """The reference's fixed step 0.5 / (1 + tau lambda_max) (G.lmax warns and estimates when unset)."""
    return 0.5 / (1 + tau * G.lmax)


def classification_tikhonov_simplex(G, y, M, tau=0.1, **kwargs):
    """Classification on the graph by Tikhonov minimisation, every row of the result on the probability simplex
    (learning.py:111-180): argmin_X tau tr(X^T L X) + sum_i m_i ||X_i - Y_i||^2 subject to X >= 0 and X 1 = 1, Y the
    one-hot labels (zero rows where unmeasured).  Returns X, (N, n_classes) float64.

    The solver is FISTA with the reference's step 0.5 / (1 + tau G.lmax), started at Y, on the float64 device graph,
    and stops on the first of these criteria that holds for obj_k = f(X_k): ``atol`` (obj_k < atol), ``dtol``
    (|obj_k - obj_{k-1}| < dtol), ``rtol`` (the same difference relative to obj_k; default 1e-3), ``xtol``
    (||X_k - X_{k-1}||_F / sqrt(N n_classes) < xtol) and ``maxit`` (default 200).  atol, dtol and xtol default to
    None (off); ``verbosity`` is accepted and ignored; any other keyword is a TypeError.  This is meant to be the
    iteration of pyunlocbox's forward_backward with its default acceleration, driven by solvers.solve; bit parity
    with pyunlocbox is not claimed and has not been checked.  Unlike the reference, a negative label at a measured
    vertex is a ValueError (the reference would silently put it in the last class), as are more than 256 classes."""
    X, _ = simplex_solve(G, y, M, tau, **kwargs)
    return X


def simplex_solve(G, y, M, tau=0.1, **kwargs):
    """classification_tikhonov_simplex that also returns the solver's info dict (niter, crit, objective, ms)."""
    engine._refuse_unknown_keywords("classification_tikhonov_simplex", kwargs, SIMPLEX_OPTIONS)
    if tau <= 0:
        raise ValueError("Tau should be greater than 0.")
    if np.size(M) != G.n_vertices:
        raise ValueError("M should be of size [G.n_vertices,]")
    labels, n_classes = simplex_labels(y, M)
    opts = {k: kwargs[k] for k in ("rtol", "atol", "dtol", "xtol", "maxit") if k in kwargs}
    step = simplex_step(G, tau)
    return engine._float64_device_graph(G).tikhonov_simplex(tau, step, labels, n_classes, **opts)
