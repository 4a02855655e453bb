#!/usr/bin/env python3
"""Generate tests/golden/components.npz by running the REAL reference (pygsp v0.6.1, the checkout named by
$PYGSP_PATH): Graph.is_connected, Graph.extract_components and Graph.subgraph on small adjacencies.

    PYGSP_PATH=path/to/reference python tests/golden/gen_components_golden.py

Per case <c>: <c>_W_* (the adjacency as CSR parts), <c>_directed, <c>_connected, and for an undirected graph
<c>_n (number of components) and per component i <c>_k<i>_idx (info['orig_idx']) and <c>_k<i>_W_* (its adjacency);
cases with coordinates also carry <c>_coords and <c>_k<i>_coords.  `cases` lists the names.  The fixture is
committed; tests read it, never the reference.
"""
import os
import sys

import numpy as np
from scipy import sparse

sys.path.insert(0, os.environ["PYGSP_PATH"])
os.environ.setdefault("MPLBACKEND", "agg")
from pygsp import graphs  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def csr_parts(M, prefix):
    M = sparse.csr_matrix(M)
    M.sort_indices()
    return {prefix + "_indptr": M.indptr.astype(np.int32), prefix + "_indices": M.indices.astype(np.int32),
            prefix + "_data": M.data.astype(np.float64), prefix + "_shape": np.array(M.shape)}


def shuffled_union(sizes, seed):
    """Block-diagonal union of Sensor graphs of the given sizes, vertices shuffled: (W, coords)."""
    parts = [graphs.Sensor(n, seed=seed + i) for i, n in enumerate(sizes)]
    W = sparse.block_diag([g.W for g in parts], format="csr")
    coords = np.concatenate([g.coords + 2.0 * i for i, g in enumerate(parts)])
    order = np.random.default_rng(seed).permutation(W.shape[0])
    return W[order, :][:, order], coords[order]


def record(out, name, W, coords=None):
    G = graphs.Graph(W, coords=coords)
    out.update(csr_parts(G.W, name + "_W"))
    out[name + "_directed"] = np.bool_(G.is_directed())
    out[name + "_connected"] = np.bool_(G.is_connected())
    if coords is not None:
        out[name + "_coords"] = np.asarray(coords)
    if G.is_directed():
        return
    parts = G.extract_components()
    out[name + "_n"] = np.int64(len(parts))
    for i, part in enumerate(parts):
        out["{}_k{}_idx".format(name, i)] = np.asarray(part.info["orig_idx"], dtype=np.int64)
        out.update(csr_parts(part.W, "{}_k{}_W".format(name, i)))
        if coords is not None:
            out["{}_k{}_coords".format(name, i)] = np.asarray(part.coords)


def main():
    out, names = {}, []

    def case(name, W, coords=None):
        names.append(name)
        record(out, name, W, coords)

    case("union3", *shuffled_union([40, 25, 60], seed=1))
    case("union4", *shuffled_union([30, 30, 45, 20], seed=2))
    case("union5", *shuffled_union([20, 35, 50, 28, 33], seed=3))
    # isolated vertices: a sensor graph with empty rows and columns spliced in (first, last and in between)
    g = graphs.Sensor(30, seed=4)
    keep = np.setdiff1d(np.arange(36), [0, 7, 8, 20, 35])[:30]
    W = sparse.lil_matrix((36, 36))
    W[np.ix_(keep, keep)] = g.W.toarray()
    case("isolated", W.tocsr())
    case("loops_only", sparse.diags([1.0, 2.0, 3.0, 0.5, 4.0]).tocsr())
    # the doctest graphs of Graph.is_connected (graph.py:316-336): the second one is directed
    doc_connected = np.array([[0., 3., 0., 0.], [3., 0., 4., 0.], [0., 4., 0., 2.], [0., 0., 2., 0.]])
    doc_directed = np.array([[0., 3., 0., 0.], [3., 0., 4., 0.], [0., 0., 0., 2.], [0., 0., 2., 0.]])
    case("doctest_connected", doc_connected)
    case("doctest_directed", doc_directed)
    # the doctest of Graph.subgraph (graph.py:234-244), with a signal carried over
    G = graphs.Graph(doc_connected)
    G.set_signal(np.array([10., 11., 12., 13.]), "s")
    sub = G.subgraph([0, 2, 1])
    out.update(csr_parts(sub.W, "doctest_subgraph_W"))
    out["doctest_subgraph_signal"] = sub.signals["s"]
    out["cases"] = np.array(names)
    np.savez_compressed(os.path.join(OUT, "components.npz"), **out)
    print("components.npz: {} cases, {} arrays".format(len(names), len(out)))


if __name__ == "__main__":
    main()
