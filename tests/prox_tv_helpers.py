"""A numpy / scipy restatement of the graph total-variation prox (pygsp_amd.optimization.prox_tv, DESIGN.md "Graph
total-variation prox"), written from the math; the CPU and GPU tests compare against it.

    z* = argmin_z 1/2 ||x - z||^2 + gamma ||D^T z||_1        dual: min_{|u| <= gamma} 1/2 ||x - D u||^2, z = x - D u

FISTA on the dual with a fixed step.  State u_k (edges), a_k = D u_k, g_k = D^T (x - a_k); u_0 = 0, t_0 = 1, b_0 = 0:

    v   = u_{k-1} + b_{k-1} (u_{k-1} - u_{k-2})
    gv  = g_{k-1} + b_{k-1} (g_{k-1} - g_{k-2})        (D^T is linear: no product at v, as on the device)
    u_k = clip(v + step gv, -gamma, gamma),   a_k = D u_k,   g_k = D^T (x - a_k)
    obj_k = 1/2 ||a_k||^2 + gamma ||g_k||_1,   t_k = (1 + sqrt(1 + 4 t_{k-1}^2)) / 2,   b_k = (t_{k-1} - 1) / t_k
"""
import math

import numpy as np
from scipy import sparse

from fista_helpers import assert_rule_is_decisive, momentum, stopping_rule, threshold_between  # noqa: F401


def incidence(W):
    """D (N x n_edges, csc) of an undirected graph without self-loops, combinatorial Laplacian: the upper triangle of
    W in row-major order, -sqrt(w) at the source and +sqrt(w) at the target (L = D D^T)."""
    C = sparse.triu(sparse.csr_matrix(W, dtype=np.float64), k=1, format="coo")
    E = C.row.size
    r = np.sqrt(C.data)
    rows, cols = np.concatenate([C.row, C.col]), np.concatenate([np.arange(E), np.arange(E)])
    return sparse.csc_matrix((np.concatenate([-r, r]), (rows, cols)), shape=(W.shape[0], E))


def primal_objective(x, z, gamma, D):
    return 0.5 * np.sum((x - z) ** 2) + gamma * np.abs(D.T @ z).sum()


def duality_gap(x, z, gamma, D):
    """Primal objective at z minus the dual value 1/2 ||x||^2 - 1/2 ||z||^2 of the u with z = x - D u: >= 0 for
    feasible u, zero exactly at the solution."""
    return primal_objective(x, z, gamma, D) - (0.5 * np.sum(x ** 2) - 0.5 * np.sum(z ** 2))


def solve(D, x, gamma, step, rtol=1e-3, atol=None, dtol=None, xtol=None, maxit=200):
    """The iteration and its stopping rule.  Returns (z, info): info has niter, crit, objective (obj_0 .. obj_niter),
    dx (||a_k - a_{k-1}||_F / sqrt(N Nsig) for k = 1 .. niter) and the dual iterate u."""
    Dm = sparse.csr_matrix(D, dtype=np.float64)
    Dt = Dm.T.tocsr()
    x = np.asarray(x, dtype=np.float64)
    x2 = x.reshape(x.shape[0], -1)
    N, S = x2.shape
    u = np.zeros((Dm.shape[1], S))
    a = np.zeros((N, S))
    g = Dt @ x2
    up, gp = u, g
    t, b = 1.0, 0.0
    obj = [gamma * np.abs(g).sum()]
    dxs = []
    k = 0
    while True:
        k += 1
        v = u + b * (u - up)
        gv = g + b * (g - gp)
        un = np.clip(v + step * gv, -gamma, gamma)
        an = Dm @ un
        gn = Dt @ (x2 - an)
        o = 0.5 * np.sum(an * an) + gamma * np.abs(gn).sum()
        prev = obj[-1]
        obj.append(o)
        dx = np.linalg.norm(an - a) / math.sqrt(N * S)
        dxs.append(dx)
        crit = stopping_rule(o, prev, dx, k, rtol, atol, dtol, xtol, maxit)
        if crit:
            z = (x2 - an).reshape(x.shape)
            return z, {"niter": k, "crit": crit, "objective": np.array(obj), "dx": np.array(dxs), "u": un}
        t, b = momentum(t)
        up, gp, u, g, a = u, g, un, gn, an
