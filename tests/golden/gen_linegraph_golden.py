#!/usr/bin/env python3
"""Generate tests/golden/linegraph.npz by running the REAL reference (pygsp v0.6.1, the checkout named by
$PYGSP_PATH): graphs.LineGraph on small graphs.

    PYGSP_PATH=path/to/reference python tests/golden/gen_linegraph_golden.py

Per case <c>: <c>_W_* (the graph's adjacency as CSR parts), <c>_lap_type, <c>_coords when the graph has coordinates,
and what the reference's line graph holds: <c>_LG_* (its W as canonical CSR parts, int64 data as the reference's),
<c>_LG_coords (when there are coordinates), <c>_n_edges, <c>_directed, <c>_loops.  `cases` lists the names.  Arrays
only; the fixture is committed, tests read it, never the reference.
"""
import os
import sys

import numpy as np
from scipy import sparse

sys.path.insert(0, os.environ["PYGSP_PATH"])
os.environ.setdefault("MPLBACKEND", "agg")
from pygsp import graphs  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def csr_parts(M, prefix, dtype):
    M = sparse.csr_matrix(M)
    M.sum_duplicates()
    M.sort_indices()
    return {prefix + "_indptr": M.indptr.astype(np.int32), prefix + "_indices": M.indices.astype(np.int32),
            prefix + "_data": M.data.astype(dtype), prefix + "_shape": np.array(M.shape)}


def undirected(n, edges, weights=None):
    W = np.zeros((n, n))
    for k, (i, j) in enumerate(edges):
        W[i, j] = W[j, i] = 1.0 if weights is None else weights[k]
    return sparse.csr_matrix(W)


def record(out, name, W, lap_type="combinatorial", coords=None):
    G = graphs.Graph(W, lap_type=lap_type, coords=coords)
    LG = graphs.LineGraph(G, lap_type=lap_type)
    out.update(csr_parts(G.W, name + "_W", np.float64))
    out[name + "_lap_type"] = np.array(lap_type)
    out[name + "_directed"] = np.bool_(G.is_directed())
    out[name + "_loops"] = np.bool_(G.has_loops())
    out[name + "_n_edges"] = np.int64(G.n_edges)
    assert LG.n_vertices == G.n_edges
    out.update(csr_parts(LG.W, name + "_LG", np.int64))
    out[name + "_LG_n_edges"] = np.int64(LG.n_edges)
    if coords is not None:
        out[name + "_coords"] = np.asarray(coords)
        out[name + "_LG_coords"] = np.asarray(LG.coords)


def main():
    out, names = {}, []

    def case(name, W, **kwargs):
        names.append(name)
        record(out, name, W, **kwargs)

    case("path4", undirected(4, [(0, 1), (1, 2), (2, 3)]))
    case("triangle", undirected(3, [(0, 1), (1, 2), (0, 2)]))
    case("star6", undirected(7, [(0, k) for k in range(1, 7)]))  # its line graph is K6
    case("two_parts_isolated", undirected(8, [(0, 1), (1, 2), (0, 2), (2, 3), (5, 6), (6, 7)]))  # (vertex 4 is alone)
    case("single_edge", undirected(2, [(0, 1)]))
    case("weighted", undirected(5, [(0, 1), (0, 3), (1, 2), (1, 4), (2, 3), (3, 4)], [0.5, 2.0, 1.0, 3.5, 0.25, 1.5]))
    sensor = graphs.Sensor(30, seed=42)
    case("sensor30", sensor.W, coords=sensor.coords)
    case("sensor30_normalized", sensor.W, lap_type="normalized", coords=sensor.coords)
    # 0 -> 1 and 1 -> 0 with different weights (an antiparallel pair of a directed graph), and 1 -> 2
    case("directed_antiparallel", sparse.csr_matrix(np.array([[0., 1., 0.], [1.5, 0., 1.], [0., 0., 0.]])))
    loop = undirected(4, [(0, 1), (1, 2), (2, 3), (0, 3)]).tolil()
    loop[2, 2] = 1.0
    case("self_loop", loop.tocsr())
    out["cases"] = np.array(names)
    path = os.path.join(OUT, "linegraph.npz")
    np.savez_compressed(path, **out)
    print("linegraph.npz: {} cases, {} arrays, {} bytes".format(len(names), len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
