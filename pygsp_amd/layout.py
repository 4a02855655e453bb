"""Vertex coordinates: pygsp.graphs.Graph.set_coordinates (pygsp/graphs/_layout.py), with the one kind that costs
anything - 'spring', Fruchterman-Reingold - iterated on the device.

The reference's `_sparse_fruchterman_reingold` (_layout.py:169-219) loops over the rows in Python, makes one lil row
dense per vertex and forms N x dim temporaries per row, `iterations` times: O(N^2) interpreted work, 1.4 s at N = 300.
Here the iterations are one call of engine.DeviceGraph.layout_spring (gspx_layout_spring_dev: the exact all-pairs sum in
float64, a fixed summation order).  Everything around them - center, pos, dom_size, k with fixed vertices, the rescaling
with its mean-then-lim statement order (_layout.py:136-166, 222-233) - is O(N dim) numpy on the host, written to
give the reference's results (the goldens of tests/golden/layout_spring.npz pin them); the start positions come from the same ``default_rng(seed).uniform`` draw, so a seed starts
from the reference's bits.  The iteration itself is chaotic: 50 free iterations in another summation order differ from
the reference by 1e-3 .. 4e-2 while one step from the same positions agrees to 1e-15 (profiles/layout.md) - a layout is
as good as the reference's, it is not the same picture.

A_ij = (W_ij > 0) is read off the pattern of the device Laplacian, so the cases whose pattern does not show A stay off
the device, as for connected components: a directed graph (the device Laplacian is that of (W + W.T) / 2), any
negative weight (A drops the entry, the pattern keeps it), and dim outside {2, 3}.  `device_route` names the reason;
the mirror raises NotImplementedError, the plugin calls the reference's own code.
"""
import numpy as np

import collections

Layout = collections.namedtuple("Layout", "coords report")  # positions (N x dim) and what the iterations reported


def device_route(G, dim):
    """None when the spring iterations of `G` can run on the device, else the reason they cannot."""
    if dim not in (2, 3):
        return "the device layout covers 2 and 3 dimensions, not {}".format(dim)
    if G.is_directed():
        return "the device layout covers undirected graphs"
    report = getattr(G, "setup_report", None)
    negative = report["negative"] > 0 if report is not None else bool(G.W.nnz and G.W.data.min() < 0)
    if negative:
        return "the device layout covers graphs without negative weights"
    return None


def rescale_layout(pos, scale=1):
    """The reference's `_rescale_layout` (_layout.py:222-233) as array expressions: every axis loses its mean, `lim` is
    the largest SIGNED coordinate of the centred array (never below 0; the other side is not looked at), and everything
    is multiplied by scale / lim.  The means are taken over contiguous columns, which sums them as the reference's
    per-axis slices are summed.  Returns a new array."""
    pos = np.asarray(pos, dtype=np.float64)
    centred = pos - np.ascontiguousarray(pos.T).mean(axis=1)
    lim = centred.max(initial=0.0)
    return centred * (scale / lim)


def _start(G, dim, pos, center, seed):
    """(start positions, extent of the domain): uniform draws of ``default_rng(seed)`` in the unit box when the caller
    gives no positions - the reference's draw, so the same seed starts from the same bits - else the caller's, one row
    per vertex (an array or anything indexed by vertex), with the largest coordinate given as the extent."""
    if pos is None:
        return np.random.default_rng(seed).uniform(size=(G.N, dim)), 1
    rows = np.array([np.asanyarray(pos[v]) for v in range(G.N)], dtype=np.float64).reshape(G.N, dim)
    return rows, np.max(pos)


def fruchterman_reingold(G, iterate, dim=2, k=None, pos=None, fixed=[], iterations=50, scale=1.0, center=None,
                         seed=None):
    """The spring layout with the argument meaning of the reference's `_fruchterman_reingold` (_layout.py:121-219)
    around `iterate(start, k, fixed, iterations, t0, dt)`, which returns (positions after the iterations, report) - the
    device call, or a restatement in the tests.  k defaults to sqrt(1 / N), times the extent of the given positions
    when vertices are fixed; the temperature falls from 0.1 by 0.1 / (iterations + 1) per iteration; a layout without
    fixed vertices is centred, rescaled to `scale` and moved to `center`, one with fixed vertices is returned as
    iterated.  Returns Layout(coords, report)."""
    shift = np.zeros((1, dim)) if center is None else center
    if np.shape(shift)[1] != dim:
        G.logger.error("Spring coordinates: center has wrong size.")
        shift = np.zeros((1, dim))
    start, extent = _start(G, dim, pos, shift, seed)
    anchored = len(fixed) > 0
    if k is None:
        k = extent / np.sqrt(G.N) if anchored else np.sqrt(1.0 / G.N)
    t0 = 0.1
    moved, report = iterate(start, float(k), fixed, int(iterations), t0, t0 / float(iterations + 1))
    moved = np.asarray(moved, dtype=np.float64)
    return Layout(moved if anchored else rescale_layout(moved, scale) + shift, report)


def device_iterate(dev):
    """`iterate` of fruchterman_reingold on the engine.DeviceGraph `dev`."""
    def iterate(start, k, fixed, iterations, t0, dt):
        return dev.layout_spring(start, k, fixed, iterations, t0, dt)
    return iterate


def _from_array(G, given):
    coords = np.squeeze(np.asanyarray(given))
    shape = coords.shape
    fits = (len(shape) == 1 and shape[0] == G.N) or (len(shape) == 2 and shape[0] == G.N and shape[1] in (2, 3))
    if not fits:
        raise ValueError("Expecting coordinates to be of size N, Nx2, or Nx3.")
    return coords


def _ring(G):
    turn = 2 * np.arange(G.N) * np.pi / G.N
    return np.column_stack([np.cos(turn), np.sin(turn)])


def _eigenmap(G, dim):
    G.compute_fourier_basis(n_eigenvectors=dim + 1)
    return G.U[:, 1:dim + 1]


def _community(G):
    raise NotImplementedError("community2D needs the reference's Community graphs: use the real pygsp (with "
                              "pygsp_amd.plugin.install() its own code keeps running)")


# kind -> (G, seed, kwargs) -> coordinates; the names are the reference's (_layout.py:10-16)
KINDS = {
    "line1D": lambda G, seed, kw: np.arange(G.N),
    "line2D": lambda G, seed, kw: np.column_stack([np.arange(G.N), np.zeros(G.N)]),
    "ring2D": lambda G, seed, kw: _ring(G),
    "random2D": lambda G, seed, kw: np.random.default_rng(seed).uniform(size=(G.N, 2)),
    "random3D": lambda G, seed, kw: np.random.default_rng(seed).uniform(size=(G.N, 3)),
    "spring": lambda G, seed, kw: G._fruchterman_reingold(seed=seed, **kw),
    "laplacian_eigenmap2D": lambda G, seed, kw: _eigenmap(G, 2),
    "laplacian_eigenmap3D": lambda G, seed, kw: _eigenmap(G, 3),
    "community2D": lambda G, seed, kw: _community(G),
}


def set_coordinates(G, kind="spring", seed=None, **kwargs):
    """``G.coords`` from an array (N, N x 2 or N x 3, after squeezing) or from one of KINDS; the keyword arguments go
    to the spring layout.  Messages and random draws are the reference's (_layout.py:5-119)."""
    if not isinstance(kind, str):
        G.coords = _from_array(G, kind)
    elif kind in KINDS:
        G.coords = KINDS[kind](G, seed, kwargs)
    else:
        raise ValueError("Unexpected argument kind={}.".format(kind))
