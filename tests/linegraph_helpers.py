"""A numpy / scipy restatement of the line graph for the tests of graphs.LineGraph (tests/test_linegraph_host.py,
tests/test_gpu_n_linegraph.py).  It reads W alone: the upper-triangle edge list, then every pair of edges that
share an endpoint.  It does not go through the differential operator D, as the reference and the host route of
graphs.LineGraph do, nor through per-vertex sorted lists, as the device builder does."""
import numpy as np
from scipy import sparse


def edge_list(W):
    """(sources, targets) of the upper triangle of W in row-major order: Graph.get_edge_list of an undirected graph
    without self-loops."""
    upper = sparse.triu(sparse.csr_matrix(W), k=1, format="coo")
    order = np.lexsort((upper.col, upper.row))
    return upper.row[order].astype(np.int64), upper.col[order].astype(np.int64)


def line_graph(W, coords=None):
    """(adjacency csr float64 with sorted columns and unit values, coords or None) of the line graph of the simple
    undirected graph W: edges i != j are joined when they share an endpoint."""
    W = sparse.csr_matrix(W)
    sources, targets = edge_list(W)
    n_edges, n_vertices = sources.size, W.shape[0]
    ends = np.concatenate([sources, targets])
    ids = np.concatenate([np.arange(n_edges), np.arange(n_edges)])
    by_vertex = np.argsort(ends, kind="stable")
    ends, ids = ends[by_vertex], ids[by_vertex]
    starts = np.searchsorted(ends, np.arange(n_vertices + 1))
    rows, cols = [np.empty(0, dtype=np.int64)], [np.empty(0, dtype=np.int64)]
    for v in range(n_vertices):
        incident = ids[starts[v]:starts[v + 1]]
        if incident.size > 1:
            a, b = np.meshgrid(incident, incident, indexing="ij")
            rows.append(a[a != b])
            cols.append(b[a != b])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    A = sparse.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(n_edges, n_edges))
    A.sum_duplicates()
    assert A.nnz == rows.size  # (two edges of a simple graph share at most one endpoint)
    A.sort_indices()
    midpoints = None if coords is None else (np.asarray(coords)[sources] + np.asarray(coords)[targets]) / 2
    return A, midpoints


def same_csr(A, B):
    """Exact equality of two canonical CSR matrices: shape, indptr, indices and data."""
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(A.data, B.data))


def star(n_vertices, tail=0):
    """A star whose hub is vertex 0, with a path of `tail` further vertices attached to its last leaf."""
    n = n_vertices + tail
    src = np.concatenate([np.zeros(n_vertices - 1, dtype=np.int64), np.arange(n_vertices - 1, n - 1)])
    dst = np.concatenate([np.arange(1, n_vertices), np.arange(n_vertices, n)])
    half = sparse.coo_matrix((np.ones(src.size), (src, dst)), shape=(n, n))
    W = sparse.csr_matrix(half + half.T)
    W.sort_indices()
    return W


def random_simple(n_vertices, density, seed):
    """A random simple undirected graph with weights in (0.1, 1): every pair is an edge with probability `density`."""
    rng = np.random.default_rng(seed)
    upper = np.triu(rng.random((n_vertices, n_vertices)) < density, k=1)
    weights = np.where(upper, rng.uniform(0.1, 1.0, upper.shape), 0.0)
    W = sparse.csr_matrix(weights + weights.T)
    W.sort_indices()
    return W


def with_edge_count(n_edges, seed):
    """A random simple undirected graph on 40 vertices with exactly `n_edges` edges (unit weights)."""
    rng = np.random.default_rng(seed)
    i, j = np.triu_indices(40, k=1)
    pick = rng.choice(i.size, size=n_edges, replace=False)
    half = sparse.coo_matrix((np.ones(n_edges), (i[pick], j[pick])), shape=(40, 40))
    W = sparse.csr_matrix(half + half.T)
    W.sort_indices()
    return W
