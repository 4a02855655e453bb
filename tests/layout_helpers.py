"""The numpy restatement of the spring layout (pygsp/graphs/_layout.py:121-233) that pins gspx_layout_spring_dev, the
named cases of tests/golden/layout_spring.npz (written by tests/golden/gen_layout_golden.py from the real reference), and
the two tolerances of the device tests.

``step`` is one Fruchterman-Reingold iteration, dense and vectorised; ``run`` repeats it with the reference's cooling
(``t -= dt`` in float64).  A mode picks the arithmetic: 'reference' sums over j as the reference's ``.sum(axis=1)`` does,
'permuted' sums the j in a shuffled order in chunks of 37 (partial sums added one after the other - the shape of the
device's split partials), 'longdouble' does everything in numpy's longdouble.

The iteration is chaotic: summed in another order it differs from the reference by up to 5.4e-14 after 5 iterations and
by 1e-3 .. 4e-2 after 50, so no test compares a free run of 50.  ONE step from given positions is benign: the modes agree
to 1.2e-15 at every one of the 50 steps of a run (tests/test_layout_host.py measures both figures again and asserts that
the constants below cover them).  The device is allowed MARGIN times that spread, in absolute position units (positions
are O(1)): it takes a reciprocal with two Newton steps for the division, fused multiply-adds, and max(d^2, 1e-4) for the
reference's sqrt-clamp-square - each a few ulp per term of the same sum.
"""
import os

import numpy as np
from scipy import sparse

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layout_spring.npz")

SPREAD_STEP = 1.2e-15   # fp64 permuted order against longdouble, one step from the same positions (and one free iteration)
SPREAD_FIVE = 5.4e-14   # the same after a free run of five iterations
MARGIN = 100
DEV_STEP_TOL = MARGIN * SPREAD_STEP
DEV_FIVE_TOL = MARGIN * SPREAD_FIVE

MAIN = ("sensor300", "er200", "sensor64")
EDGE = ("single", "coincident", "subclamp", "ring257", "fixed300")
MODES = ("reference", "permuted", "longdouble")
T0, RUN = 0.1, 50


def temperatures(iterations, t0=T0, dt=None):
    """t of every iteration, by the reference's repeated subtraction (_layout.py:190-217)."""
    dt = t0 / float(iterations + 1) if dt is None else dt
    out, t = [], t0
    for _ in range(iterations):
        out.append(t)
        t -= dt
    return out


def step(A, pos, k, t, fixed=(), mode="reference", info=None):
    """Positions after one iteration at temperature t.  A: dense 0 / 1 adjacency (N x N); fixed: vertex indices.
    info (a dict): takes 'pair_gap' and 'len_gap', the smallest relative distance of a pair distance (i != j) and of a
    displacement length from 0.01, 'short', how many displacements were shorter than 0.01, and 'clamped', how many
    ordered pairs were closer than 0.01 - smallest / summed over the calls that share the dict - and 'length', the
    displacement lengths of this call."""
    dtype = np.longdouble if mode == "longdouble" else np.float64
    P = np.asarray(pos, dtype=dtype)
    N = P.shape[0]
    A = np.asarray(A, dtype=dtype)
    k = dtype(k)
    delta = P[:, None, :] - P[None, :, :]                      # delta[i, j] = pos_i - pos_j
    raw = np.sqrt((delta ** 2).sum(axis=2))
    dist = np.where(raw < 0.01, dtype(0.01), raw)
    terms = delta * (k * k / dist ** 2 - A * dist / k)[:, :, None]
    terms = np.ascontiguousarray(terms.transpose(0, 2, 1))     # (i, axis, j): j contiguous, as in the reference
    if mode == "permuted":
        order = np.random.default_rng(N).permutation(N)
        disp = np.zeros(terms.shape[:2], dtype=dtype)
        for c0 in range(0, N, 37):
            disp = disp + np.ascontiguousarray(terms[:, :, order[c0:c0 + 37]]).sum(axis=2)
    else:
        disp = terms.sum(axis=2)
    if len(fixed):
        disp[np.asarray(fixed, dtype=np.int64)] = 0
    length = np.sqrt((disp ** 2).sum(axis=1))
    short = length < 0.01
    if info is not None:
        off = raw[~np.eye(N, dtype=bool)]
        free = np.setdiff1d(np.arange(N), np.asarray(fixed, dtype=np.int64))
        info["pair_gap"] = min(info.get("pair_gap", np.inf), float(np.abs(off / 0.01 - 1).min(initial=np.inf)))
        info["len_gap"] = min(info.get("len_gap", np.inf), float(np.abs(length[free] / 0.01 - 1).min(initial=np.inf)))
        info["short"] = info.get("short", 0) + int(short[free].sum())
        info["clamped"] = info.get("clamped", 0) + int((off < 0.01).sum())
        info["length"] = np.asarray(length, dtype=np.float64)  # of this call, before the rule
    length = np.where(short, dtype(0.1), length)
    return P + disp * dtype(t) / length[:, None]


def run(A, pos, k, iterations, t0=T0, dt=None, fixed=(), mode="reference", info=None):
    """Positions after 1, 2, ... `iterations` iterations (float64 arrays; longdouble is carried between the steps)."""
    out, P = [], pos
    for t in temperatures(iterations, t0, dt):
        P = step(A, P, k, t, fixed, mode, info)
        out.append(np.asarray(P, dtype=np.float64))
    return out


def iterate(A, mode="reference"):
    """`iterate` of pygsp_amd.layout.fruchterman_reingold on the restatement: (positions, report)."""
    def go(pos, k, fixed, iterations, t0, dt):
        out = run(A, pos, k, iterations, t0, dt, fixed, mode)[-1] if iterations else np.array(pos)
        return out, {"iterations": iterations}
    return go


class Case:
    """One case of the golden file: W (scipy CSR), A (dense 0 / 1), pos0, k, fixed, dim, pos1 / pos5 (the reference
    after free runs of 1 and 5 iterations) and, for MAIN, traj: (RUN + 1, N, dim), the reference's positions before
    iteration 0 .. RUN - 1 of one run of RUN iterations and after the last."""

    def __init__(self, npz, name):
        self.name = name
        shape = tuple(int(v) for v in npz[name + "_W_shape"])
        self.W = sparse.csr_matrix((npz[name + "_W_data"], npz[name + "_W_indices"], npz[name + "_W_indptr"]), shape=shape)
        self.A = (self.W > 0).toarray().astype(np.float64)
        self.N = shape[0]
        self.pos0, self.k = npz[name + "_pos0"], float(npz[name + "_k"])
        self.fixed = [int(v) for v in npz[name + "_fixed"]]
        self.dim = self.pos0.shape[1]
        self.pos1, self.pos5 = npz[name + "_pos1"], npz[name + "_pos5"]
        self.traj = npz[name + "_traj"] if name + "_traj" in npz.files else None
        # a vertex order for the permuted device graphs: a fixed shuffle
        self.perm = np.random.default_rng(self.N + 1).permutation(self.N).astype(np.int32)


_cache = {}


def golden():
    if "npz" not in _cache:
        _cache["npz"] = np.load(GOLDEN)
    return _cache["npz"]


def case(name):
    if name not in _cache:
        _cache[name] = Case(golden(), name)
    return _cache[name]


def dev(a, b):
    """Largest absolute deviation of two position arrays."""
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max(initial=0.0))
