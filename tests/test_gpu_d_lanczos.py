"""Lanczos filtering on the device (pygsp_amd.filters.lanczos_op, gspx_lanczos_krylov_dev / _combine_dev):
the reference's fixtures, the numpy restatement of tests/lanczos_helpers.py, orthogonality, breakdown, determinism,
column batches, device arrays, fp32 graphs and the large sizes."""
import numpy as np
import pytest
from scipy import sparse

from gpu_helpers import random_graph
from lanczos_helpers import (complete, csr_from, exact_filter, laplacian, rel_err, ring, run_numpy, star)
from pygsp_amd import engine, filters, graphs

pytestmark = pytest.mark.gpu
GOLDEN = {}


def golden(name):
    if name not in GOLDEN:
        import os
        GOLDEN[name] = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "lanczos_{}.npz".format(name))))
    return GOLDEN[name]


def bank(G, kind):
    return filters.Heat(G, scale=float(kind[4:])) if kind.startswith("heat") else filters.MexicanHat(G, Nf=6)


@pytest.mark.parametrize("name", ["sensor123", "logo"])
@pytest.mark.parametrize("lap_type", ["combinatorial", "normalized"])
def test_lanczos_op_against_reference_fixtures(name, lap_type):
    g = golden(name)
    G = graphs.Graph(csr_from(g, "W"), lap_type=lap_type, compute_dtype=np.float64)
    G._lmax = float(g["lmax_" + lap_type])
    for kind, key in (("heat10", "heat10"), ("mexicanhat", "mexicanhat6"), ("heat50", "heat50")):
        f = bank(G, kind)
        k = "{}_{}".format(lap_type, key)
        order = int(g[k + "_order"])
        y1 = filters.lanczos_op(f, g["x1"], order=order)
        y5 = filters.lanczos_op(f, g["x5"], order=order)
        assert y1.shape == (G.N * f.Nf,) and y5.shape == (G.N * f.Nf, 5)
        assert rel_err(y1, g[k + "_y1"]) <= 1e-10, k
        assert rel_err(y5, g[k + "_y5"]) <= 1e-10, k


CASES = [(2000, 1, 1, 1), (2000, 3, 2, 6), (20_000, 64, 30, 1), (5000, 300, 30, 6), (100_000, 3, 100, 1),
         (100_000, 1, 30, 6)]


@pytest.mark.parametrize("N,nv,order,nf", CASES)
def test_lanczos_op_against_numpy_restatement(N, nv, order, nf):
    W = random_graph(N, 8, seed=N + nv, hub=True, isolated=3)
    G = graphs.Graph(W, compute_dtype=np.float64)
    G.estimate_lmax("bounds")
    f = filters.Heat(G, scale=10) if nf == 1 else filters.MexicanHat(G, Nf=6)
    x = np.random.default_rng(order).standard_normal((N, nv))
    if nv > 2:
        x[:, 1] = 0  # a zero column
    y = filters.lanczos_op(f, x[:, 0] if nv == 1 else x, order=order)
    ref, _, _ = run_numpy(laplacian(W, "combinatorial"), f, x[:, 0] if nv == 1 else x, order, G._get_upper_bound())
    assert y.shape == ref.shape
    assert rel_err(y, ref) <= 1e-10
    if nv > 2:
        assert np.all(y[:, 1] == 0)


@pytest.mark.parametrize("lap_type", ["combinatorial", "normalized"])
def test_basis_is_orthonormal(lap_type):
    W = random_graph(30_000, 8, seed=5, hub=True, isolated=2)
    dev = graphs.Graph(W, lap_type=lap_type, compute_dtype=np.float64).device_graph(np.float64)
    x = np.random.default_rng(1).standard_normal((W.shape[0], 7))
    order = 60
    V, alpha, beta, steps = dev.lanczos_basis(x, order)
    assert V.shape == (W.shape[0], order, 7) and np.all(steps == order)
    for c in range(7):
        Q = V[:, :, c]
        assert np.max(np.abs(Q.T @ Q - np.eye(order))) <= 1e-12
    np.testing.assert_allclose(V[:, 0, :], x / np.linalg.norm(x, axis=0), rtol=0, atol=1e-15)
    np.testing.assert_allclose(beta[0], np.linalg.norm(x, axis=0), rtol=1e-13)


@pytest.mark.parametrize("W,x,expected", [
    (ring(64), np.random.default_rng(0).standard_normal(64), 33),
    (complete(64), np.random.default_rng(1).standard_normal(64), 2),
    (star(30), np.random.default_rng(2).standard_normal(30), 3),
    (ring(64), np.ones(64), 1),
])
def test_breakdown_steps_and_exactness(W, x, expected):
    G = graphs.Graph(W, compute_dtype=np.float64)
    G.estimate_lmax("bounds")
    b = G._get_upper_bound()
    _, _, _, steps = G.device_graph(np.float64).lanczos_basis(x, 60, 64 * np.finfo(float).eps * b)
    assert steps == expected
    f = filters.MexicanHat(G, Nf=6)
    y = filters.lanczos_op(f, x, order=60)
    assert rel_err(y, exact_filter(laplacian(W, "combinatorial"), f, x)) <= 1e-12


SMALL_GRAPHS = {}


@pytest.mark.parametrize("order", [8, 20])
@pytest.mark.parametrize("width", [1, 3, 17, 64, 65, 255, 256])
@pytest.mark.parametrize("N", [70, 257])
def test_shared_thread_map_at_small_n(N, width, order):
    """The column kernels' thread map (gspx_reduce.hip.h) under Lanczos where it changes behaviour: fewer rows than one
    workgroup takes and a ragged last row group, ldp = 1 .. 256 (rstep = 1 at 255 and 256: k_lz_update's four-row tail
    is ragged at both sizes), and at width 256 the dot pass of step 16 (16 x 256 = 4096 entries) switches sum_parts
    from k_colsum to k_panel_sum_parts inside one order-20 run.  Against the numpy backend's basis."""
    from lanczos_helpers import NumpyBackend
    if N not in SMALL_GRAPHS:
        W = random_graph(N, 4, seed=N)
        SMALL_GRAPHS[N] = (W, laplacian(W, "combinatorial"))
    W, L = SMALL_GRAPHS[N]
    rng = np.random.default_rng(1000 * N + 10 * width + order)
    x = rng.standard_normal((N, width))
    if width > 2:
        x[:, 1] = 0  # a zero column
    Vr, ar, br, _, sr = NumpyBackend(L).krylov(x, 0, width, order, 0.0)
    live = x.any(axis=0)
    assert np.array_equal(sr, np.where(live, order, 0))
    for perm in (rng.permutation(N).astype(np.int32), None):
        dev = engine.DeviceGraph.from_w(W, dtype=np.float64, perm=perm)
        V, alpha, beta, steps = dev.lanczos_basis(x, order)
        again = dev.lanczos_basis(x, order)
        dev.destroy()
        assert V.shape == (N, order, width) and np.array_equal(steps, sr)
        for c in np.flatnonzero(live):
            assert rel_err(alpha[:, c], ar[:, c]) <= 1e-10 and rel_err(beta[:, c], br[:, c]) <= 1e-10, (c, perm is None)
            Q = V[:, :, c]
            assert np.max(np.abs(Q.T @ Q - np.eye(order))) <= 1e-12, (c, perm is None)
        assert rel_err(V, np.moveaxis(Vr, 0, 1)) <= 1e-10
        assert not V[:, :, ~live].any() and not alpha[:, ~live].any() and not beta[:, ~live].any()
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip((V, alpha, beta, steps), again))


def test_repeated_calls_give_identical_bits():
    W = random_graph(50_000, 8, seed=9, hub=True)
    G = graphs.Graph(W, compute_dtype=np.float64)
    f = filters.MexicanHat(G, Nf=6)
    x = np.random.default_rng(3).standard_normal((W.shape[0], 16))
    a = filters.lanczos_op(f, x, order=40)
    b = filters.lanczos_op(f, x, order=40)
    assert np.array_equal(a, b)


def test_column_batches_agree_with_one_batch():
    W = random_graph(40_000, 8, seed=11)
    G = graphs.Graph(W, compute_dtype=np.float64)
    f = filters.Heat(G, scale=10)
    x = np.random.default_rng(4).standard_normal((W.shape[0], 40))
    one = filters.lanczos_op(f, x, order=30)
    ctx = G.device_graph(np.float64).ctx
    old = ctx.get_option("ws_limit_mb")
    try:
        ctx.set_option("ws_limit_mb", 100)  # 33 panels of 40k x 8 columns: ~84 MB
        from pygsp_amd import lanczos
        assert lanczos.max_batch_width(W.shape[0], 30, 100) < 40
        many = filters.lanczos_op(f, x, order=30)
    finally:
        ctx.set_option("ws_limit_mb", old)
    assert rel_err(many, one) <= 1e-12


def test_device_array_in_device_array_out():
    W = random_graph(30_000, 8, seed=13, hub=True)
    G = graphs.Graph(W, compute_dtype=np.float64)
    f = filters.MexicanHat(G, Nf=6)
    x = np.random.default_rng(5).standard_normal((W.shape[0], 5))
    host = filters.lanczos_op(f, x, order=30)
    d = G.to_device(x) if hasattr(G, "to_device") else engine.DeviceArray.from_host(G.device_graph(np.float64).ctx, x)
    out = filters.lanczos_op(f, d, order=30)
    assert isinstance(out, engine.DeviceArray) and out.shape == host.shape
    assert np.array_equal(out.numpy(), host)
    d1 = engine.DeviceArray.from_host(G.device_graph(np.float64).ctx, x[:, 2])
    out1 = filters.lanczos_op(f, d1, order=30)
    assert out1.shape == (W.shape[0] * 6,)
    assert np.array_equal(out1.numpy(), filters.lanczos_op(f, x[:, 2], order=30))
    d32 = engine.DeviceArray.from_host(G.device_graph(np.float64).ctx, x, np.float32)
    with pytest.raises(ValueError):
        filters.lanczos_op(f, d32, order=30)


def test_fp32_graph_gives_fp64_results():
    W = random_graph(20_000, 8, seed=17)
    G32 = graphs.Graph(W, compute_dtype=np.float32)
    G64 = graphs.Graph(W, compute_dtype=np.float64)
    G64.estimate_lmax("bounds")
    G32._lmax = G64.lmax  # (the same kernel on both: only the graph's compute dtype differs)
    x = np.random.default_rng(6).standard_normal((W.shape[0], 3))
    y32 = filters.lanczos_op(filters.Heat(G32, scale=10), x, order=30)
    y64 = filters.lanczos_op(filters.Heat(G64, scale=10), x, order=30)
    assert y32.dtype == np.float64
    assert rel_err(y32, y64) <= 1e-12


def test_fp32_graph_is_refused_by_the_entry_points():
    import ctypes

    from pygsp_amd import _capi
    W = random_graph(1000, 6, seed=1)
    dev = graphs.Graph(W, compute_dtype=np.float32).device_graph(np.float32)
    z = np.zeros((4, 1))
    s = np.zeros(1, dtype=np.int32)
    buf = dev.ctx.alloc(1000 * 8 * 4)
    rc = _capi.load().gspx_lanczos_krylov_dev(dev._h, 4, 1, ctypes.c_void_p(buf.ptr), 1, 0.0, ctypes.c_void_p(buf.ptr),
                                              _capi.ptr(z), _capi.ptr(z), _capi.ptr(z), _capi.ptr(s), None, None)
    with pytest.raises(ValueError):
        _capi.check(rc)
    assert "float32" in _capi.last_error()
    buf.free()


def test_low_frequency_signals_sensor2000():
    G = graphs.Sensor(2000, seed=0, compute_dtype=np.float64)
    G.estimate_lmax("bounds")
    L = laplacian(G.W, "combinatorial")
    e, U = np.linalg.eigh(L.toarray())
    x = U[:, :20] @ np.random.default_rng(8).standard_normal((20, 4))
    f = filters.Heat(G, scale=200)
    y = filters.lanczos_op(f, x, order=30)
    assert rel_err(y, exact_filter(L, f, x)) <= 1e-8


def test_sensor_1m_against_chebyshev_order60():
    G = graphs.Sensor(1_000_000, seed=0, compute_dtype=np.float64)
    f = filters.Heat(G, scale=10)
    x = np.random.default_rng(9).standard_normal((G.N, 64))
    y = filters.lanczos_op(f, x, order=30)
    ref = f.filter(x, method="chebyshev", order=60)
    assert rel_err(y, ref) <= 1e-10
