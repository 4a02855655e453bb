"""Partial Fourier bases on the MI355X: the four panel primitives against numpy (values, edge shapes, bit-identical
repeats), compute_fourier_basis(method='device') against dense eigh, the solver at 200k vertices against scipy's
shift-invert eigsh and at 1M vertices on its own bars, and gft / igft of device arrays."""
import numpy as np
import pytest
from scipy import sparse
from scipy.sparse import linalg as splinalg

from conftest import csr_from, rel_err
from fourier_helpers import check_against_dense, laplacian
from pygsp_amd import engine, fourier, graphs

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 1000, 100_003]
WIDTHS = [1, 17, 64, 96, 200, 512]
PAIRS = [(1, 1), (17, 64), (64, 17), (96, 96), (200, 512), (512, 200), (512, 512), (1, 512)]


def _upload(ctx, a):
    buf = ctx.take(max(a.nbytes, 16))
    if a.size:
        buf.upload(np.ascontiguousarray(a))
    return buf


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context(0)


@pytest.mark.parametrize("N", SIZES)
def test_panel_gram_against_numpy(ctx, N):
    rng = np.random.default_rng(N)
    for na, nb in PAIRS:
        lda, ldb = na + 3, nb + 5  # unequal leading dimensions, columns taken from the middle of wider panels
        A = rng.standard_normal((N, lda))
        B = rng.standard_normal((N, ldb))
        ba, bb = _upload(ctx, A), _upload(ctx, B)
        try:
            C1, _ = fourier.panel_gram(ctx, N, ba.ptr + 8, lda, na, bb.ptr + 16, ldb, nb)
            C2, _ = fourier.panel_gram(ctx, N, ba.ptr + 8, lda, na, bb.ptr + 16, ldb, nb)
        finally:
            ctx.give(ba)
            ctx.give(bb)
        ref = A[:, 1:1 + na].T @ B[:, 2:2 + nb]
        assert C1.shape == (na, nb)
        assert rel_err(C1, ref) < 1e-13, (N, na, nb, rel_err(C1, ref))
        assert np.array_equal(C1, C2)


@pytest.mark.parametrize("N", SIZES)
def test_panel_combine_against_numpy(ctx, N):
    rng = np.random.default_rng(N + 1)
    for p, q in PAIRS:
        ldx, ldy = p + 2, q + 7
        X = rng.standard_normal((N, ldx))
        Q = rng.standard_normal((p, q))
        Y0 = rng.standard_normal((N, ldy))
        bx, by = _upload(ctx, X), _upload(ctx, Y0)
        try:
            fourier.panel_combine(ctx, N, bx.ptr + 16, ldx, p, Q, by.ptr + 8, ldy)
            Y1 = by.download((N, ldy), np.float64) if N else np.zeros((0, ldy))
            fourier.panel_combine(ctx, N, bx.ptr + 16, ldx, p, Q, by.ptr + 8, ldy)
            Y2 = by.download((N, ldy), np.float64) if N else np.zeros((0, ldy))
        finally:
            ctx.give(bx)
            ctx.give(by)
        ref = X[:, 2:2 + p] @ Q
        assert rel_err(Y1[:, 1:1 + q], ref) < 1e-13, (N, p, q)
        # columns outside the view untouched
        assert np.array_equal(Y1[:, :1], Y0[:, :1]) and np.array_equal(Y1[:, 1 + q:], Y0[:, 1 + q:])
        assert np.array_equal(Y1, Y2)


@pytest.mark.parametrize("N", SIZES)
def test_panel_copy_against_numpy(ctx, N):
    """A column block out of a wider panel and back into another one: exact, columns outside the view untouched."""
    rng = np.random.default_rng(N + 3)
    for w in WIDTHS:
        ldx, ldy = w + 5, w + 2
        X = rng.standard_normal((N, ldx))
        Y0 = rng.standard_normal((N, ldy))
        bx, by = _upload(ctx, X), _upload(ctx, Y0)
        try:
            fourier.panel_copy(ctx, N, bx.ptr + 24, ldx, w, by.ptr + 8, ldy)
            Y = by.download((N, ldy), np.float64) if N else np.zeros((0, ldy))
        finally:
            ctx.give(bx)
            ctx.give(by)
        assert np.array_equal(Y[:, 1:1 + w], X[:, 3:3 + w])
        assert np.array_equal(Y[:, :1], Y0[:, :1]) and np.array_equal(Y[:, 1 + w:], Y0[:, 1 + w:])


@pytest.mark.parametrize("N", SIZES)
def test_panel_residual_norms_against_numpy(ctx, N):
    rng = np.random.default_rng(N + 2)
    for p in WIDTHS:
        ld = p + 3
        # (1) independent panels; (2) LX = theta X + 1e-9 noise, the small residuals where ||LX||^2 - theta^2 would
        # cancel - X and theta with few significant bits, so theta X and LX - theta X are exact in either arithmetic
        # (fused or not) and the comparison sees only the summation
        X = rng.standard_normal((N, ld))
        theta = rng.uniform(0, 2, p)
        Xs = rng.integers(-1024, 1024, (N, ld)) / 1024.0
        ths = rng.integers(0, 16, p) / 8.0
        LXs = Xs.copy()
        LXs[:, :p] = Xs[:, :p] * ths + 1e-9 * rng.standard_normal((N, p))
        for X_, LX_, th in ((X, rng.standard_normal((N, ld)), theta), (Xs, LXs, ths)):
            bx, bl = _upload(ctx, X_), _upload(ctx, LX_)
            try:
                r1, _ = fourier.panel_residual_norms(ctx, N, bx.ptr, bl.ptr, ld, p, th)
                r2, _ = fourier.panel_residual_norms(ctx, N, bx.ptr, bl.ptr, ld, p, th)
            finally:
                ctx.give(bx)
                ctx.give(bl)
            ref = np.linalg.norm(LX_[:, :p] - X_[:, :p] * th, axis=0)
            assert r1.shape == (p,)
            assert np.all(np.abs(r1 - ref) <= 1e-13 * ref), (N, p, np.max(np.abs(r1 - ref) / np.maximum(ref, 1e-300)))
            assert np.array_equal(r1, r2)


def _sensor_w(N, seed):
    from oracle import knn_oracle as knn
    return sparse.csr_matrix(knn.knn_weights(knn.sensor_coords(N, seed=seed), 6)[0])


def _cases(golden_logo):
    W1 = _sensor_w(2000, 0)
    Wd = sparse.csr_matrix(sparse.block_diag([_sensor_w(700, 1), _sensor_w(900, 2)]))
    return {"sensor2000": W1, "logo": csr_from(golden_logo, "W"), "disconnected": Wd}


@pytest.mark.parametrize("lap_type", ["combinatorial", "normalized"])
@pytest.mark.parametrize("name", ["sensor2000", "logo", "disconnected"])
def test_device_basis_against_dense_eigh(golden_logo, name, lap_type):
    W = _cases(golden_logo)[name]
    G = graphs.Graph(W, lap_type=lap_type)
    k = 12
    G.compute_fourier_basis(n_eigenvectors=k, method="device")
    b = G._get_upper_bound()
    L = laplacian(W, lap_type)
    assert G.U.shape == (W.shape[0], k) and G._lmax is None and G.e[0] == 0
    assert G.fourier_stats["worst_residual"] <= 1e-10 * b
    e = G.e.copy()
    lam = np.linalg.eigh(L.toarray())[0]
    e[0] = lam[0]  # (set to zero by the partial-result rule)
    check_against_dense(L, b, e, G.U)
    idx = np.argmax(np.abs(G.U), axis=0)
    assert np.all(G.U[idx, np.arange(k)] > 0)
    if name == "disconnected":
        assert abs(G.e[1]) <= 1e-10 * b


def test_device_basis_with_close_ritz_values():
    """Two nearly equal grids and a ring: clusters of close eigenvalues, where locked columns can lose their
    residual in Rayleigh-Ritz - every returned pair must still meet the tolerance."""
    from fourier_helpers import grid, ring
    W = sparse.csr_matrix(sparse.block_diag([grid(20), grid(20) * (1 + 1e-6), ring(60)]))
    G = graphs.Graph(W)
    k = 16
    G.compute_fourier_basis(n_eigenvectors=k, method="device")
    b = G._get_upper_bound()
    L = laplacian(W, "combinatorial")
    e = G.e.copy()
    e[0] = G.fourier_stats["theta0"]
    assert np.linalg.norm(L @ G.U - G.U * e, axis=0).max() <= 1e-10 * b * (1 + 1e-6)
    check_against_dense(L, b, e, G.U)


def test_device_basis_of_an_fp32_graph():
    """The solver runs on the float64 device graph whatever the compute dtype."""
    W = _sensor_w(2000, 4)
    G = graphs.Graph(W, compute_dtype=np.float32)
    G.compute_fourier_basis(n_eigenvectors=10, method="device")
    L = laplacian(W, "combinatorial")
    e = G.e.copy()
    e[0] = np.linalg.eigh(L.toarray())[0][0]
    check_against_dense(L, G._get_upper_bound(), e, G.U)
    assert np.float64 in [np.dtype(k).type for k in G._dev]


def test_device_basis_at_200k_against_shift_invert():
    G = graphs.Sensor(200_000, seed=0)
    k = 32
    G.compute_fourier_basis(n_eigenvectors=k)  # 'auto': the device
    assert G.fourier_stats is not None
    b = G._get_upper_bound()
    L = G.device_graph(np.float64).download_l().astype(np.float64)
    U, e = G.U, G.e
    res = np.linalg.norm(L @ U - U * e, axis=0)
    assert res[1:].max() <= 1e-10 * b * (1 + 1e-6) and res[0] <= 1e-9 * b
    assert np.max(np.abs(U.T @ U - np.eye(k))) <= 1e-12
    ref = np.sort(splinalg.eigsh(sparse.csc_matrix(L), k, sigma=-1e-3, which="LM", return_eigenvectors=False))
    ref[0] = 0
    assert np.max(np.abs(e - ref)) <= 1e-8 * b


def test_device_basis_at_1m():
    G = graphs.Sensor(1_000_000, seed=0)
    k = 64
    G.compute_fourier_basis(n_eigenvectors=k)
    b = G._get_upper_bound()
    assert G.fourier_stats["worst_residual"] <= 1e-10 * b
    U = G.U
    assert np.max(np.abs(U.T @ U - np.eye(k))) <= 1e-12
    L = G.device_graph(np.float64).download_l().astype(np.float64)
    e = G.e.copy()
    e[0] = G.fourier_stats["theta0"]
    assert np.linalg.norm(L @ U - U * e, axis=0).max() <= 1e-10 * b * (1 + 1e-6)


def test_gft_igft_on_device_arrays():
    G = graphs.Sensor(3000, seed=1)
    G.compute_fourier_basis(n_eigenvectors=20, method="device")
    rng = np.random.default_rng(0)
    for shape in [(3000,), (3000, 5), (3000, 4, 3)]:
        s = rng.standard_normal(shape)
        d = G.to_device(s, np.float64)
        s_hat = G.gft(d)
        assert isinstance(s_hat, engine.DeviceArray) and s_hat.shape == (20,) + shape[1:]
        ref = np.tensordot(G.U, s, ([0], [0]))
        assert rel_err(np.asarray(s_hat), ref) < 1e-13
        back = G.igft(s_hat)
        assert isinstance(back, engine.DeviceArray) and back.shape == shape
        ref2 = np.tensordot(G.U, ref, ([1], [0]))
        assert rel_err(np.asarray(back), ref2) < 1e-13
        assert np.array_equal(G.gft(s), ref)  # numpy input: the host arithmetic of the reference
    with pytest.raises(TypeError):
        G.gft(G.to_device(rng.standard_normal(3000), np.float32))
