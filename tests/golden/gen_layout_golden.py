#!/usr/bin/env python3
"""Generate tests/golden/layout_spring.npz by running the REAL reference (pygsp v0.6.1, the checkout named by
$PYGSP_PATH): the spring layout of pygsp/graphs/_layout.py on small graphs.

    PYGSP_PATH=path/to/reference python tests/golden/gen_layout_golden.py

Per case <c>: <c>_W_* (the adjacency as CSR parts), <c>_pos0 (start positions), <c>_k, <c>_fixed (vertex indices),
<c>_pos1 / <c>_pos5 (_sparse_fruchterman_reingold after free runs of 1 and of 5 iterations) and, for the MAIN cases,
<c>_traj: (51, N, dim), the positions before every one of the 50 iterations of ONE run of 50 and after the last.  The
reference keeps no history; it asks ``i in fixed`` for every vertex of every iteration, so the `fixed` handed to it here
is an empty list that copies the position array whenever it is asked about vertex 0.  `full_a`, `full_b`: complete
``set_coordinates('spring', seed=3, iterations=5)`` results on `sensor64`, the second with scale=2, center=[[1, -1]].
`cases` lists the names.  The fixture is committed; tests read it, never the reference.
"""
import os
import sys

import numpy as np
from scipy import sparse

sys.path.insert(0, os.environ["PYGSP_PATH"])
os.environ.setdefault("MPLBACKEND", "agg")
from pygsp import graphs  # noqa: E402
from pygsp.graphs import _layout  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def csr_parts(M, prefix):
    M = sparse.csr_matrix(M)
    M.sort_indices()
    return {prefix + "_indptr": M.indptr.astype(np.int32), prefix + "_indices": M.indices.astype(np.int32),
            prefix + "_data": M.data.astype(np.float64), prefix + "_shape": np.array(M.shape)}


class Watching(list):
    """A `fixed` list that records `pos` at the start of every iteration (the reference asks about vertex 0 first)."""

    def __init__(self, members, pos):
        list.__init__(self, members)
        self.pos, self.seen = pos, []

    def __contains__(self, i):
        if i == 0:
            self.seen.append(self.pos.copy())
        return list.__contains__(self, i)


def reference_run(W, dim, k, pos0, fixed, iterations, watch=False):
    A = sparse.csr_matrix(W) > 0  # graph.py:718-726
    pos = np.array(pos0, dtype=np.float64)
    members = Watching(fixed, pos) if watch else list(fixed)
    out = _layout._sparse_fruchterman_reingold(A, dim, k, pos, members, iterations, None)
    assert out is pos
    return (out, np.array(members.seen + [out])) if watch else out


def record(out, name, W, pos0, k=None, fixed=(), traj=False):
    W = sparse.csr_matrix(W, dtype=np.float64)
    N, dim = pos0.shape
    k = float(np.sqrt(1.0 / N)) if k is None else float(k)
    out.update(csr_parts(W, name + "_W"))
    out[name + "_pos0"], out[name + "_k"], out[name + "_fixed"] = pos0, np.float64(k), np.array(fixed, dtype=np.int64)
    out[name + "_pos1"] = reference_run(W, dim, k, pos0, fixed, 1)
    out[name + "_pos5"] = reference_run(W, dim, k, pos0, fixed, 5)
    if traj:
        _, seen = reference_run(W, dim, k, pos0, fixed, 50, watch=True)
        assert seen.shape == (51, N, dim) and np.array_equal(seen[0], pos0)
        out[name + "_traj"] = seen


def main():
    out, names = {}, []

    def case(name, *args, **kwargs):
        names.append(name)
        record(out, name, *args, **kwargs)

    start = lambda N, dim: np.random.default_rng(7).uniform(size=(N, dim))  # noqa: E731
    sensor300 = graphs.Sensor(300, seed=2).W
    case("sensor300", sensor300, start(300, 2), traj=True)
    case("er200", graphs.ErdosRenyi(200, p=0.05, seed=3).W, start(200, 3), traj=True)
    case("sensor64", graphs.Sensor(64, seed=1).W, start(64, 2), traj=True)
    case("single", sparse.csr_matrix((1, 1)), np.array([[0.25, 0.75]]))
    case("coincident", np.array([[0., 1.], [1., 0.]]), np.array([[0.3, 0.4], [0.3, 0.4]]))
    case("subclamp", np.array([[0., 1., 0.], [1., 0., 1.], [0., 1., 0.]]),
         np.array([[0.2, 0.2], [0.203, 0.2], [0.7, 0.5]]))
    ring = sparse.lil_matrix((260, 260))
    for i in range(257):
        ring[i, (i + 1) % 257] = ring[(i + 1) % 257, i] = 1.0
    case("ring257", ring.tocsr(), start(260, 3))
    user = 2.0 * np.random.default_rng(11).uniform(size=(300, 2))
    case("fixed300", sensor300, user, k=user.max() / np.sqrt(300), fixed=[0, 17, 299])
    G = graphs.Sensor(64, seed=1)
    G.set_coordinates("spring", seed=3, iterations=5)
    out["full_a"] = np.array(G.coords)
    G.set_coordinates("spring", seed=3, iterations=5, scale=2, center=[[1, -1]])
    out["full_b"] = np.array(G.coords)
    out["cases"] = np.array(names)
    path = os.path.join(OUT, "layout_spring.npz")
    np.savez_compressed(path, **out)
    print("layout_spring.npz: {} cases, {} arrays, {} bytes".format(len(names), len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
