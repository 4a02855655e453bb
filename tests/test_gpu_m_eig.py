"""The full Fourier basis on the MI355X: the block Jacobi eigensolver (gspx_sym_eig_dev) on dense symmetric matrices
and degenerate spectra, its non-convergence code, Graph.compute_fourier_basis(method='jacobi') on the golden sensor
graph and on Sensor(600), device residency of the solver's panel, and the plugin's full-basis seam when a pygsp is
importable.  Every case is judged by invariants (eigenvalues against eigvalsh, residual, orthonormality), never by
comparing eigenvectors column by column.  The bars: with s = max(lambda_max, 1), eigenvalues within 1e-13 s, max |A U -
U diag(e)| <= 1e-13 s, max |U^T U - I| <= 1e-13."""
import subprocess
import sys

import numpy as np
import pytest

import eig_helpers as eh
from conftest import csr_from
from pygsp_amd import engine, filters, fourier, graphs
from test_gpu_b_real_pygsp import _env, needs_pygsp

pytestmark = pytest.mark.gpu

BAR = 1e-13


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context(0)


def _solve(ctx, A, pad=(3, 5), fill=7.5, **kw):
    """sym_eig of the host matrix A through strided views at an offset into wider buffers.  Returns (e, U, stats, the
    whole V buffer as it came back with its untouched entries masked out of U)."""
    n = A.shape[0]
    lda, ldv = n + pad[0], n + pad[1]
    Abuf = np.full(n * lda + 2, -3.25)
    Vbuf = np.full(n * ldv + 3, fill)
    for r in range(n):
        Abuf[2 + r * lda:2 + r * lda + n] = A[r]
    ba, bv = ctx.take(max(Abuf.nbytes, 16)), ctx.take(max(Vbuf.nbytes, 16))
    try:
        ba.upload(Abuf)
        bv.upload(Vbuf)
        e, stats = fourier.sym_eig(ctx, n, ba.ptr + 16, lda, bv.ptr + 24, ldv, **kw)
        back = bv.download(Vbuf.shape, np.float64)
    finally:
        ctx.give(ba)
        ctx.give(bv)
    U = np.zeros((n, n))
    mask = np.ones(Vbuf.shape, dtype=bool)
    for r in range(n):
        U[r] = back[3 + r * ldv:3 + r * ldv + n]
        mask[3 + r * ldv:3 + r * ldv + n] = False
    assert np.all(back[mask] == fill), "the padding of the V buffer was written"
    return e, U, stats, back


def _check_bars(A, e, U, what):
    de, res, orth = eh.bars(A, e, U)
    print("{}: eigenvalues {:.2e}, residual {:.2e}, orthonormality {:.2e}".format(what, de, res, orth))
    assert de <= BAR and res <= BAR and orth <= BAR, (what, de, res, orth)
    assert np.all(np.diff(e) >= 0), what


def _random_symmetric(n):
    R = np.random.default_rng(1000 + n).standard_normal((n, n))
    return (R + R.T) / 2


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 200])
def test_sym_eig_on_dense_indefinite_matrices(ctx, n):
    A = _random_symmetric(n)
    e, U, stats, back = _solve(ctx, A)
    assert e.shape == (n,) and stats["pad_mass"] == 0.0
    _check_bars(A, e, U, "random symmetric, n = {} ({} sweeps)".format(n, stats["sweeps"]))
    e2, U2, stats2, back2 = _solve(ctx, A)
    assert np.array_equal(e, e2) and np.array_equal(back, back2) and stats2["sweeps"] == stats["sweeps"]
    if n > 1:
        assert stats["sweeps"] >= 1 and stats["pairs_rotated"] >= 1 and stats["off_rel"] <= 1e-13
        assert len(stats["skipped_per_sweep"]) == stats["sweeps"]


def _two_components():
    """Two path-like components of 30 and 25 vertices plus two isolated vertices: a null space of dimension 4."""
    n = 57
    W = np.zeros((n, n))
    rng = np.random.default_rng(5)
    for lo, hi in ((0, 30), (30, 55)):
        for i in range(lo, hi - 1):
            W[i, i + 1] = W[i + 1, i] = rng.uniform(0.5, 1.5)
        W[lo, hi - 1] = W[hi - 1, lo] = 0.7
    return np.diag(W.sum(1)) - W


def _ring(n):
    eye = np.eye(n)
    return 2 * eye - np.roll(eye, 1, 0) - np.roll(eye, -1, 0)


@pytest.mark.parametrize("name", ["zero", "identity", "diagonal", "ring", "components"])
def test_sym_eig_on_degenerate_spectra(ctx, name):
    A, components, zero_sweeps = {
        "zero": (np.zeros((70, 70)), None, True),
        "identity": (2.5 * np.eye(70), None, True),
        "diagonal": (np.diag(np.random.default_rng(2).standard_normal(70)), None, True),
        "ring": (_ring(256), 1, False),
        "components": (_two_components(), 4, False),
    }[name]
    e, U, stats, _ = _solve(ctx, A)
    _check_bars(A, e, U, "{} ({} sweeps)".format(name, stats["sweeps"]))
    if zero_sweeps:
        assert stats["sweeps"] == 0 and stats["pairs_rotated"] == 0
        assert np.array_equal(e, np.sort(np.diag(A)))
        assert np.array_equal(np.abs(U).sum(0), np.ones(70)) and np.array_equal(np.abs(U).sum(1), np.ones(70))
    if name in ("zero", "identity"):
        assert np.array_equal(U, np.eye(70))
    if components is not None:
        s = max(float(e[-1]), 1.0)
        assert int(np.sum(np.abs(e) <= 1e-13 * s)) == components


def test_non_convergence_is_an_error_and_the_library_goes_on(ctx):
    A = _random_symmetric(200)
    with pytest.raises(ValueError, match="no convergence in 1 sweeps"):
        _solve(ctx, A, max_sweeps=1)
    e, U, stats, _ = _solve(ctx, A)
    _check_bars(A, e, U, "after the refused call")


@pytest.fixture(scope="module")
def golden_basis(golden_sensor123):
    g = golden_sensor123
    G = graphs.Graph(csr_from(g, "W"), reorder="none", tiles=False)
    G.compute_fourier_basis(method="jacobi")
    return G, csr_from(g, "Lcomb").toarray()


def test_graph_path_on_the_golden_sensor_graph(golden_basis):
    G, L = golden_basis
    assert G.U.dtype == np.float64 and G.U.shape == (123, 123) and G.e.shape == (123,)
    _check_bars(L, G.e, G.U, "sensor123 ({} sweeps)".format(G.fourier_stats["sweeps"]))
    assert G.e[0] == 0 and abs(G.fourier_stats["theta0"]) < 1e-13 * G.e[-1]
    idx = np.argmax(np.abs(G.U), axis=0)
    assert np.all(G.U[idx, np.arange(123)] > 0)
    assert G._lmax == G.e[-1] and G._lmax_method == "fourier"
    assert G.fourier_stats["pad_mass"] == 0.0
    _, _, model = eh.sym_eig(L)
    assert abs(G.fourier_stats["sweeps"] - model["sweeps"]) <= 1, (G.fourier_stats["sweeps"], model["sweeps"])
    # the device copy carries the same signs as the host copy
    dev, panel = G._basis_on_device()
    assert np.array_equal(panel.buf.download((123, 123), np.float64), G.U)


def test_sensor_600(ctx):
    G = graphs.Sensor(600, k=8, seed=0)
    G.compute_fourier_basis(method="jacobi")
    sweeps = G.fourier_stats["sweeps"]
    _check_bars(G.L.toarray(), G.e, G.U, "Sensor(600) ({} sweeps)".format(sweeps))
    assert sweeps <= 14, "Sensor(600, k=8) took {} sweeps (the numpy restatement needs 11)".format(sweeps)
    G._forget_spectrum()
    assert G._U_dev is None and G._U is None


def test_the_solvers_panel_serves_exact_filtering(golden_sensor123):
    W = csr_from(golden_sensor123, "W")
    G = graphs.Graph(W, reorder="none", tiles=False)
    G.compute_fourier_basis(method="jacobi")
    held = G._U_dev
    assert held is not None and G._basis_on_device() is held and G._basis_on_device()[1] is held[1]
    H = graphs.Graph(W, reorder="none", tiles=False)
    H.compute_fourier_basis()  # host eigh
    assert H.fourier_stats is None
    x = np.random.default_rng(9).standard_normal((123, 4))
    ref = filters.Heat(H, 10).filter(x, method="exact")
    out = filters.Heat(G, 10).filter(x, method="exact")
    assert out.shape == ref.shape and np.max(np.abs(out - ref)) <= 1e-12 * np.max(np.abs(ref))
    out_dev = filters.Heat(G, 10).filter(G.to_device(x), method="exact")
    assert isinstance(out_dev, engine.DeviceArray)
    assert np.max(np.abs(np.asarray(out_dev) - ref)) <= 1e-12 * np.max(np.abs(ref))
    assert G._U_dev is held  # nothing was uploaded in its place
    # a slice of the full solve follows the partial-result rules and leaves lmax alone
    P = graphs.Graph(W, reorder="none", tiles=False)
    P.compute_fourier_basis(n_eigenvectors=9, method="jacobi")
    assert P.U.shape == (123, 9) and P.e[0] == 0 and P._lmax is None
    assert np.max(np.abs(P.e - G.e[:9])) <= 1e-13 * G.e[-1]


@needs_pygsp
def test_plugin_sends_full_bases_to_the_device(tmp_path):
    code = (
        "import numpy as np, pygsp\n"
        "from pygsp import graphs, filters\n"
        "from pygsp_amd import plugin\n"
        "plugin.FULL_BASIS_MIN_VERTICES = 1024  # (the measured crossover is higher: this test stays small)\n"
        "plugin.install(pygsp, fourier=True, full_basis=True, exact=True)\n"
        "G = graphs.Sensor(1024, seed=42)\n"
        "G.compute_fourier_basis()\n"
        "L = G.L.toarray()\n"
        "ref = np.linalg.eigvalsh(L)\n"
        "s = max(ref[-1], 1.0)\n"
        "assert G.U.shape == (1024, 1024) and G.e[0] == 0 and G.lmax == G.e[-1]\n"
        "assert np.max(np.abs(G.e - ref)) <= 1e-13 * s\n"
        "assert np.max(np.abs(L @ G.U - G.U * G.e[None, :])) <= 1e-13 * s\n"
        "assert np.max(np.abs(G.U.T @ G.U - np.eye(1024))) <= 1e-13\n"
        "held = G.__dict__['_gspx_basis']\n"
        "assert held[0] is G.U\n"
        "x = np.random.default_rng(3).standard_normal((G.N, 3))\n"
        "y = filters.Heat(G, 10).filter(x, method='exact')\n"
        "assert G.__dict__['_gspx_basis'] is held and plugin.basis_on_device_for(G)[1] is held[2]\n"
        "plugin.uninstall(pygsp)\n"
        "ref_y = filters.Heat(G, 10).filter(x, method='exact')\n"
        "assert np.max(np.abs(y - ref_y)) <= 1e-12 * np.max(np.abs(ref_y))\n"
        "print('full basis through the plugin ok')\n")
    res = subprocess.run([sys.executable, "-c", code], env=_env(tmp_path), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "full basis through the plugin ok" in res.stdout, res.stdout[-1500:] + res.stderr[-1500:]
