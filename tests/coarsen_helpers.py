"""Shared by tests/test_coarsen_host.py and tests/test_gpu_z_coarsen.py: the hand-worked graphs of the matching tests,
the property checks of a matching and of a coarse graph, and the numpy restatement of segment pooling and its vjp - the
same order of operations as the kernels (members in ascending order, one operation per member), so the device is
compared with it exactly."""
import numpy as np
from scipy import sparse

from pygsp_amd import reduction


def from_edges(n, edges):
    """Symmetric CSR adjacency of the weighted edges [(i, j, w), ...] on n vertices."""
    if not edges:
        return sparse.csr_matrix((n, n), dtype=np.float64)
    i, j, w = (np.array(v) for v in zip(*edges))
    W = sparse.coo_matrix((np.r_[w, w].astype(np.float64), (np.r_[i, j], np.r_[j, i])), shape=(n, n)).tocsr()
    W.sort_indices()
    return W


def path(n, weights=None):
    w = np.ones(n - 1) if weights is None else np.asarray(weights, dtype=np.float64)
    return from_edges(n, [(k, k + 1, w[k]) for k in range(n - 1)])


def increasing_path(n=64):
    """Strictly increasing weights along the path: with metric='weight' one pair per round, from the far end."""
    return path(n, 1.0 + np.arange(n - 1) / 8.0)


def triangle():
    return from_edges(3, [(0, 1, 1.0), (0, 2, 1.0), (1, 2, 1.0)])


def star(leaves, seed=None):
    """Hub 0 and `leaves` leaves; equal weights, or random ones with a seed."""
    w = np.ones(leaves) if seed is None else np.random.default_rng(seed).uniform(0.5, 1.5, leaves)
    return from_edges(leaves + 1, [(0, k + 1, w[k]) for k in range(leaves)])


def ring(n=7):
    return from_edges(n, [(k, (k + 1) % n, 1.0) for k in range(n)])


def with_isolated():
    """Nine vertices: a weighted path 1-2-4-5, an edge 7-8, and 0, 3, 6 isolated."""
    return from_edges(9, [(1, 2, 0.5), (2, 4, 2.0), (4, 5, 1.0), (7, 8, 0.25)])


def two_hubs(leaves=600, seed=5):
    """Hubs 0 and 1 joined to every leaf by light random weights, the leaves joined in heavy pairs: the leaves match
    each other, so every entry of the two long coarse rows is a sum of two fine entries."""
    rng = np.random.default_rng(seed)
    edges = [(h, 2 + k, w) for h in (0, 1) for k, w in enumerate(rng.uniform(0.01, 0.02, leaves))]
    edges += [(2 + k, 3 + k, w) for k, w in zip(range(0, leaves - 1, 2), rng.uniform(5.0, 6.0, leaves // 2))]
    return from_edges(leaves + 2, edges)


def random_simple(n, avg_deg, seed):
    """A random simple graph with random weights (no two equal, almost surely)."""
    rng = np.random.default_rng(seed)
    m = n * avg_deg // 2
    i, j = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = i != j
    lo, hi = np.minimum(i, j)[keep], np.maximum(i, j)[keep]
    _, first = np.unique(lo * n + hi, return_index=True)
    lo, hi = lo[first], hi[first]
    w = rng.uniform(0.1, 1.0, lo.size)
    W = sparse.coo_matrix((np.r_[w, w], (np.r_[lo, hi], np.r_[hi, lo])), shape=(n, n)).tocsr()
    W.sort_indices()
    return W


HAND_CASES = {
    "path2": lambda: path(2),
    "path3": lambda: path(3),
    "triangle": triangle,
    "star5": lambda: star(5),
    "ring7": ring,
    "increasing_path64": increasing_path,
    "isolated": with_isolated,
}


def check_matching(W, mate, pairs=None):
    """`mate` is an involution, its pairs are edges of W, and no edge joins two singletons (maximal)."""
    W = sparse.csr_matrix(W)
    n = W.shape[0]
    mate = np.asarray(mate)
    assert mate.dtype == np.int32 and mate.shape == (n,)
    assert np.array_equal(mate[mate], np.arange(n))
    i = np.flatnonzero(mate != np.arange(n))
    assert i.size == 0 or np.all(np.asarray(W[i, mate[i]]).ravel() != 0)
    if pairs is not None:
        assert 2 * pairs == i.size


def check_maximal(W, mate):
    C = sparse.csr_matrix(W).tocoo()
    single = np.asarray(mate) == np.arange(C.shape[0])
    off = C.row != C.col
    assert not np.any(single[C.row[off]] & single[C.col[off]])


def check_parent(mate, parent, nc):
    """Cluster c is the rank of its smaller member among the representatives: monotone in the representative."""
    n = len(mate)
    rep = np.minimum(mate, np.arange(n))
    reps = np.unique(rep)
    assert nc == reps.size and np.array_equal(parent[reps], np.arange(nc))
    assert np.array_equal(parent, parent[rep])
    assert np.all(np.diff(parent[reps]) > 0)


def scipy_coarse(W, parent):
    """P^T W P without its diagonal, by scipy's sparse products."""
    n, nc = W.shape[0], int(parent.max()) + 1
    P = sparse.csr_matrix((np.ones(n), (np.arange(n), parent)), shape=(n, nc))
    Wc = sparse.csr_matrix(P.T @ sparse.csr_matrix(W, dtype=np.float64) @ P)
    Wc.setdiag(0)
    Wc.eliminate_zeros()
    Wc.sort_indices()
    return Wc


def check_coarse(Wc, W, parent):
    """Canonical, no diagonal, no stored zero, exactly symmetric, and scipy's P^T W P to 1e-15 relative per entry (at
    most four positive terms in another order: both sides within 3 * 2^-53 of the exact sum)."""
    assert sparse.isspmatrix_csr(Wc) and Wc.has_sorted_indices
    assert not Wc.diagonal().any() and (Wc.nnz == 0 or np.all(Wc.data != 0))
    assert (Wc != Wc.T).nnz == 0
    ref = scipy_coarse(W, parent)
    assert np.array_equal(Wc.indptr, ref.indptr) and np.array_equal(Wc.indices, ref.indices)
    if ref.nnz:
        assert np.max(np.abs(Wc.data - ref.data) / ref.data) <= 1e-15


def host_levels(W, levels, metric="normalized_cut", d=None):
    """`levels` levels of the two restatements: [(mate, rounds, pairs, parent, nc, Wc), ...]; d: the degrees of level 0
    (deeper levels use the row sums of the restated coarse graph)."""
    out = []
    for _ in range(levels):
        mate, rounds, pairs = reduction.heavy_edge_matching_host(W, d, metric)
        parent, nc = reduction.parent_of(mate)
        Wc = reduction.coarsen_host(W, parent)
        out.append((mate, rounds, pairs, parent, nc, Wc))
        W, d = Wc, None
    return out


# ---- pooling --------------------------------------------------------------------------------------------------------
def mixed_partition(n_coarse, seed):
    """(ptr, idx, parent): segments of sizes 1, 2, 3 and 4 mixed, members scattered and ascending inside a segment."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 5, n_coarse)
    sizes[:4] = [1, 2, 3, 4][:min(4, n_coarse)]
    n = int(sizes.sum())
    parent = np.repeat(np.arange(n_coarse), sizes)[rng.permutation(n)].astype(np.int32)
    return partition_of(parent, n_coarse) + (parent,)


def partition_of(parent, n_coarse):
    idx = np.argsort(parent, kind="stable").astype(np.int32)
    ptr = np.r_[0, np.cumsum(np.bincount(parent, minlength=n_coarse))].astype(np.int32)
    return ptr, idx


def pool_host(ptr, idx, x, mode):
    """y[c] = reduce of x[idx[m]] over the segment, members in order: max keeps the larger by ``v > acc``, sum and mean
    add one member at a time, mean divides the sum by the size - in x's dtype throughout."""
    x = np.asarray(x)
    sizes = np.diff(ptr)
    acc = x[idx[ptr[:-1]]].copy()
    for t in range(1, int(sizes.max())):
        sel = np.flatnonzero(sizes > t)
        v = x[idx[ptr[sel] + t]]
        acc[sel] = np.where(v > acc[sel], v, acc[sel]) if mode == "max" else acc[sel] + v
    if mode == "mean":
        acc = acc / sizes.astype(x.dtype).reshape((-1,) + (1,) * (x.ndim - 1))
    return acc.astype(x.dtype)


def pool_vjp_host(ptr, idx, g, x, mode):
    """gx[idx[m]] from g[c]: sum - a copy, mean - g / size, max - g at the first member attaining the maximum, else 0."""
    g = np.asarray(g)
    sizes = np.diff(ptr)
    seg_of = np.repeat(np.arange(sizes.size), sizes)  # segment of idx[m]
    gx = np.empty((idx.size,) + g.shape[1:], dtype=g.dtype)
    if mode == "sum":
        gx[idx] = g[seg_of]
    elif mode == "mean":
        gx[idx] = (g / sizes.astype(g.dtype).reshape((-1,) + (1,) * (g.ndim - 1)))[seg_of]
    else:
        x = np.asarray(x)
        best, arg = x[idx[ptr[:-1]]].copy(), np.zeros((sizes.size,) + g.shape[1:], dtype=np.int64)
        for t in range(1, int(sizes.max())):
            sel = np.flatnonzero(sizes > t)
            v = x[idx[ptr[sel] + t]]
            better = v > best[sel]
            best[sel] = np.where(better, v, best[sel])
            arg[sel] = np.where(better, t, arg[sel])
        place = np.arange(idx.size) - ptr[:-1][seg_of]  # position of idx[m] inside its segment
        hit = arg[seg_of] == place.reshape((-1,) + (1,) * (g.ndim - 1))
        gx[idx] = np.where(hit, g[seg_of], np.zeros((), dtype=g.dtype))
    return gx
