#!/usr/bin/env python3
"""Generate tests/golden/knn_wide.npz by running the REAL reference (the checkout named by $PYGSP_PATH): patch
features, Grid2d, and NN graphs of clouds with more than 64 columns.

    PYGSP_PATH=path/to/reference python tests/golden/gen_knn_wide_golden.py

The reference's ImgPatches cuts its windows with skimage.util.view_as_windows; where scikit-image is missing, a
stand-in module with that one function (numpy's sliding window: the same windows) is registered before the reference
runs, so the reference's own padding, window shape and reshape are what gets recorded.  Images and clouds come from
default_rng seeds that the tests repeat (cases() below is the list both sides follow); the file keeps only features,
W, sigma and coordinates.
"""
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.environ["PYGSP_PATH"])
os.environ.setdefault("MPLBACKEND", "agg")
try:
    import skimage.util  # noqa: F401
except ImportError:
    _util = types.ModuleType("skimage.util")
    _util.view_as_windows = lambda arr_in, window_shape: np.lib.stride_tricks.sliding_window_view(arr_in, window_shape)
    _pkg = types.ModuleType("skimage")
    _pkg.util = _util
    sys.modules["skimage"], sys.modules["skimage.util"] = _pkg, _util
from pygsp import graphs  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def csr_parts(M, prefix):
    M = M.tocsr()
    M.sort_indices()
    M.eliminate_zeros()
    return {prefix + "_indptr": M.indptr.astype(np.int32), prefix + "_indices": M.indices.astype(np.int32),
            prefix + "_data": M.data, prefix + "_shape": np.array(M.shape)}


def image(seed, shape):
    """Whole-numbered grey levels on a ramp (patches of neighbouring pixels resemble each other; the features
    compress well)."""
    rng = np.random.default_rng(seed)
    ramp = 4.0 * np.add.outer(np.arange(shape[0]), np.arange(shape[1]))
    return (ramp.reshape(ramp.shape + (1,) * (len(shape) - 2)) + rng.integers(0, 64, shape)).astype(np.float64)


# the small images of the host test: (tag, seed, image shape, patch_shape)
PATCH_CASES = (("g33", 1, (6, 7), (3, 3)), ("g4", 2, (5, 6), (4,)), ("g25", 3, (7, 5), (2, 5)),
               ("c32", 4, (5, 4, 3), (3, 2)), ("c5", 5, (6, 6, 2), (5,)), ("g1", 6, (4, 3), (1,)))
GRID_CASES = (("grid_7x5", 7, 5, 0.0), ("grid_4x6d", 4, 6, 0.25), ("grid_5", 5, None, 0.0), ("grid_1x6d", 1, 6, 0.5))


def main():
    out = {}
    for tag, seed, shape, patch in PATCH_CASES:
        G = graphs.ImgPatches(image(seed, shape), patch_shape=patch, k=3)
        out["feat_" + tag] = G.Xin
    for tag, n1, n2, diagonal in GRID_CASES:
        G = graphs.Grid2d(n1, n2, diagonal=diagonal)
        out.update(csr_parts(G.W, "W_" + tag))
        out["coords_" + tag] = G.coords
    # NN graphs beyond 64 dimensions
    rgb = image(21, (20, 24, 3))
    G = graphs.ImgPatches(rgb, patch_shape=(5, 5), k=10)  # 75-D
    out["feat_rgb"] = G.Xin
    out.update(csr_parts(G.W, "W_rgb"))
    out["sigma_rgb"] = np.float64(G.sigma)
    grey = image(22, (18, 22))
    G = graphs.ImgPatches(grey, patch_shape=(9,), k=8)  # 81-D
    out["feat_grey"] = G.Xin
    out.update(csr_parts(G.W, "W_grey"))
    out["sigma_grey"] = np.float64(G.sigma)
    out["coords_grey"] = G.coords
    G = graphs.Grid2dImgPatches(rgb, patch_shape=(5, 5), k=10)
    out.update(csr_parts(G.W, "W_gridrgb"))
    X300 = np.random.default_rng(23).standard_normal((600, 300))
    G = graphs.NNGraph(X300, k=9, dist_type="minkowski", order=1)
    out.update(csr_parts(G.W, "W_x300"))
    out["sigma_x300"] = np.float64(G.sigma)
    X96 = np.random.default_rng(24).standard_normal((500, 96))
    G = graphs.NNGraph(X96, NNtype="radius", epsilon=0.3)
    out.update(csr_parts(G.W, "W_r96"))
    out["sigma_r96"] = np.float64(G.sigma)
    out["nnz_r96"] = np.int64(G.W.nnz)
    path = os.path.join(OUT, "knn_wide.npz")
    np.savez_compressed(path, **out)
    print("knn_wide.npz", os.path.getsize(path), "bytes; radius graph nnz", G.W.nnz)


if __name__ == "__main__":
    main()
