"""Host halves of graphs.ImgPatches / Grid2d (CPU only): the patch feature matrices and the grid's W and coordinates
against what the reference recorded (tests/golden/knn_wide.npz, gen_knn_wide_golden.py)."""
import numpy as np
import pytest

from conftest import csr_from, load_golden
from pygsp_amd import graphs


def image(seed, shape):
    """The generator's image(): whole-numbered grey levels on a ramp."""
    rng = np.random.default_rng(seed)
    ramp = 4.0 * np.add.outer(np.arange(shape[0]), np.arange(shape[1]))
    return (ramp.reshape(ramp.shape + (1,) * (len(shape) - 2)) + rng.integers(0, 64, shape)).astype(np.float64)


@pytest.fixture(scope="module")
def golden():
    return load_golden("knn_wide.npz")


# grey and colour, (r, c) and (r,), even and odd sides, a 1 x 1 window; the two images of the GPU goldens
@pytest.mark.parametrize("tag,seed,shape,patch", [
    ("g33", 1, (6, 7), (3, 3)), ("g4", 2, (5, 6), (4,)), ("g25", 3, (7, 5), (2, 5)), ("c32", 4, (5, 4, 3), (3, 2)),
    ("c5", 5, (6, 6, 2), (5,)), ("g1", 6, (4, 3), (1,)), ("rgb", 21, (20, 24, 3), (5, 5)), ("grey", 22, (18, 22), (9,))])
def test_image_patches_match_reference(golden, tag, seed, shape, patch):
    img = image(seed, shape)
    X = graphs.image_patches(img, patch)
    ref = golden["feat_" + tag]
    side = patch if len(patch) == 2 else patch * 2
    assert X.shape == ref.shape == (shape[0] * shape[1], side[0] * side[1] * (shape[2] if len(shape) == 3 else 1))
    np.testing.assert_array_equal(X, ref)  # bit for bit
    # the pixel itself sits at window position ((r - 1) // 2, (c - 1) // 2)
    centre = ((side[0] - 1) // 2 * side[1] + (side[1] - 1) // 2) * (shape[2] if len(shape) == 3 else 1)
    np.testing.assert_array_equal(X[:, centre], img.reshape(shape[0] * shape[1], -1)[:, 0])
    assert graphs.image_patches(img.tolist(), list(patch)).shape == ref.shape  # array-likes


@pytest.mark.parametrize("tag,n1,n2,diagonal", [("grid_7x5", 7, 5, 0.0), ("grid_4x6d", 4, 6, 0.25),
                                                ("grid_5", 5, None, 0.0), ("grid_1x6d", 1, 6, 0.5)])
def test_grid2d_weights_match_reference(golden, tag, n1, n2, diagonal):
    W, coords = graphs.grid2d_weights(n1, n2, diagonal)
    Wref = csr_from(golden, "W_" + tag)
    W.sort_indices()
    assert W.shape == Wref.shape and W.nnz == Wref.nnz
    np.testing.assert_array_equal(W.indptr, Wref.indptr)
    np.testing.assert_array_equal(W.indices, Wref.indices)
    np.testing.assert_array_equal(W.data, Wref.data)
    np.testing.assert_array_equal(coords, golden["coords_" + tag])
    if diagonal:
        assert (W.data == diagonal).any() == (min(n1, n2 or n1) > 1)


def test_one_dimensional_image_raises():
    with pytest.raises(ValueError, match="at least a 2D array"):
        graphs.image_patches(np.arange(12.0), (3, 3))
    with pytest.raises(ValueError):
        graphs.image_patches(np.zeros((2, 2, 2, 2)), (3,))
