"""A numpy restatement of the simplex-constrained Tikhonov classifier (pygsp_amd.learning.classification_tikhonov_simplex,
DESIGN.md "Simplex-constrained classification"), written from the math; the CPU and GPU tests compare against it.

    f(X) = tau sum(X * L X) + sum_i m_i ||X_i - Y_i||^2,   grad f(X) = 2 (m (X - Y) + tau L X)
    X_k = P(V_{k-1} - step grad f(V_{k-1})),   V_k = X_k + b_k (X_k - X_{k-1}),   b_k = (t_{k-1} - 1) / t_k
    t_0 = 1, t_k = (1 + sqrt(1 + 4 t_{k-1}^2)) / 2,   X_0 = V_0 = Y

P is the row-wise Euclidean projection onto {x >= 0, sum x = 1}.  L V is formed as (1 + b) L X_k - b L X_{k-1}, as on
the device: one product per iteration.
"""
import math

import numpy as np

from fista_helpers import CRITERIA, assert_rule_is_decisive, momentum, stopping_rule, threshold_between  # noqa: F401


def project_simplex(Z):
    """Row-wise projection onto the probability simplex by the active-set pass: theta = (sum of the active entries -
    1) / their count, entries <= theta leave the active set, repeated until none leaves; x = max(z - theta, 0)."""
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    act = np.ones(Z.shape, dtype=bool)
    while True:
        theta = (np.where(act, Z, 0.0).sum(axis=1) - 1.0) / act.sum(axis=1)
        keep = act & (Z > theta[:, None])
        if (keep == act).all():
            return np.maximum(Z - theta[:, None], 0.0)
        act = keep


def one_hot(labels, n_classes):
    """Y: one-hot rows for labels >= 0, zero rows for -1."""
    labels = np.asarray(labels)
    return (labels[:, None] == np.arange(n_classes)[None, :]).astype(np.float64)


def objective(L, X, m, Y, tau, LX=None):
    LX = L @ X if LX is None else LX
    return tau * np.sum(X * LX) + np.sum(m[:, None] * (X - Y) ** 2)


def gradient(L, X, m, Y, tau):
    return 2.0 * (m[:, None] * (X - Y) + tau * (L @ X))


def fixed_point_residual(L, X, labels, n_classes, tau, step):
    """||X - P(X - step grad f(X))|| / ||X||: zero exactly at the minimiser."""
    m = (np.asarray(labels) >= 0).astype(np.float64)
    Y = one_hot(labels, n_classes)
    return np.linalg.norm(X - project_simplex(X - step * gradient(L, X, m, Y, tau))) / np.linalg.norm(X)


def solve(L, labels, n_classes, tau, step, rtol=1e-3, atol=None, dtol=None, xtol=None, maxit=200):
    """The iteration and its stopping rule.  Returns (X, info): info has niter, crit, objective (obj_0 .. obj_niter)
    and dx (||X_k - X_{k-1}||_F / sqrt(N C) for k = 1 .. niter)."""
    labels = np.asarray(labels)
    N = labels.size
    m = (labels >= 0).astype(np.float64)
    Y = one_hot(labels, n_classes)
    X = Y.copy()
    LX = L @ X
    Xp, LXp = X, LX
    t, b = 1.0, 0.0
    obj = [objective(L, X, m, Y, tau, LX)]
    dxs = []
    k = 0
    while True:
        k += 1
        V = X + b * (X - Xp)
        LV = (1.0 + b) * LX - b * LXp
        G = 2.0 * (m[:, None] * (V - Y) + tau * LV)
        Xn = project_simplex(V - step * G)
        LXn = L @ Xn
        o = objective(L, Xn, m, Y, tau, LXn)
        prev = obj[-1]
        obj.append(o)
        dx = np.linalg.norm(Xn - X) / math.sqrt(N * n_classes)
        dxs.append(dx)
        crit = stopping_rule(o, prev, dx, k, rtol, atol, dtol, xtol, maxit)
        if crit:
            return Xn, {"niter": k, "crit": crit, "objective": np.array(obj), "dx": np.array(dxs)}
        t, b = momentum(t)
        Xp, LXp, X, LX = X, LX, Xn, LXn


def golden_problem(g):
    """W, labels (int32, -1 where unmeasured) and n_classes of the ops_sensor123 fixture."""
    from conftest import csr_from
    W = csr_from(g, "W")
    keep = g["mask"].astype(bool)
    labels = np.where(keep, g["labels"], -1).astype(np.int32)
    return W, labels, int(g["labels"][keep].max()) + 1


def laplacian(W):
    from scipy import sparse
    W = sparse.csr_matrix(W, dtype=np.float64)
    return (sparse.diags(np.asarray(W.sum(axis=1)).ravel()) - W).tocsr()
