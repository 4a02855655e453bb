"""Chebyshev cross-moments and the vector-Jacobian product on the device (gspx_cheby_cross_moments_dev /
k_slot_cross_dots, spectrum.cheby_cross_moments, filters.cheby_op_vjp, Filter.filter_vjp): every width, parity, plane
pass and chunk of slots against the numpy restatement with z drawn independently of x, tiny shapes, column batches, an
internal vertex order, tile and plain steps, aliased and swapped arguments, input types, and the linearity identities of
the vjp with the device's own forward."""
import ctypes

import numpy as np
import pytest

from autograd_helpers import cross_moments_direct, vjp_direct
from conftest import rel_err
from gpu_helpers import TOL, ctx, random_graph, upper_lmax  # noqa: F401 (ctx: fixture)
from oracle import cheby_oracle as orc
from pygsp_amd import filters, graphs, spectrum
from scipy import sparse

pytestmark = pytest.mark.gpu

F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
# k_slot_cross_dots (CROSS_PASS, CROSS_FEW, cross_cs of csrc/gspx_poly.hip.h): at most PASS planes per pass; a pass of
# more than FEW planes walks the slots in chunks of 8, a pass of one or two in chunks of 16 - half that for fp32 panels
# of an even width
PASS, FEW = 8, 2


def graph_of(W, dtype=np.float64):
    G = graphs.Graph(W, compute_dtype=dtype)
    G._lmax = upper_lmax(W)
    return G


def device_cross(G, x, z, M, dtype=np.float64):
    """One gspx_cheby_cross_moments_dev call on x, z uploaded in `dtype`, and the reference on both rounded to it."""
    m, ms = G.device_graph(dtype).cheby_cross_moments(x, z, G.lmax, M)
    r = (lambda a: np.asarray(a).astype(dtype).astype(np.float64))
    return m, cross_moments_direct(orc.laplacian(G.W), G.lmax, r(x), r(z), M), ms


@pytest.fixture(scope="module")
def hub_graphs():
    W = random_graph(3000, 8, seed=5, hub=True, isolated=2)
    return {F64: graph_of(W, np.float64), F32: graph_of(W, np.float32)}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nsig", [1, 3, 5, 6, 67, 130])
def test_cross_moments_widths_and_parities(hub_graphs, dtype, nsig):
    G = hub_graphs[np.dtype(dtype)]
    rng = np.random.default_rng(nsig)
    x = rng.standard_normal((G.N, nsig))
    for M, nf in ((13, 1), (14, 1), (13, 2), (14, 2), (13, FEW + 1), (14, FEW + 1)):
        z = rng.standard_normal((nf, G.N, nsig))
        m, ref, _ = device_cross(G, x, z, M, dtype)
        m2, _, _ = device_cross(G, x, z, M, dtype)
        err = rel_err(m, ref)
        print("cross-moments {} nsig {} M {} Nf {}: {:.2e}".format(np.dtype(dtype).name, nsig, M, nf, err))
        assert m.shape == (nf, M, nsig) and m.dtype == np.float64 and err < TOL[np.dtype(dtype)]
        assert np.array_equal(m, m2)  # identical calls, identical bits


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nf", [PASS - 1, PASS, PASS + 1])
def test_cross_moments_around_the_plane_pass(hub_graphs, dtype, nf):
    G = hub_graphs[np.dtype(dtype)]
    rng = np.random.default_rng(nf)
    for nsig, M in ((5, 13), (6, 14)):
        x, z = rng.standard_normal((G.N, nsig)), rng.standard_normal((nf, G.N, nsig))
        m, ref, _ = device_cross(G, x, z, M, dtype)
        m2, _, _ = device_cross(G, x, z, M, dtype)
        err = rel_err(m, ref)
        print("cross-moments {} Nf {} nsig {}: {:.2e}".format(np.dtype(dtype).name, nf, nsig, err))
        assert m.shape == (nf, M, nsig) and err < TOL[np.dtype(dtype)] and np.array_equal(m, m2)
        for f in range(nf):  # plane by plane: a plane that met another plane's slots would pass the max-norm above
            assert rel_err(m[f], ref[f]) < TOL[np.dtype(dtype)], f


@pytest.mark.parametrize("N", [1, 63, 65, 257])
@pytest.mark.parametrize("nsig", [1, 4])
def test_cross_moments_small_shapes(N, nsig):
    W = random_graph(N, 4, seed=N) if N > 1 else sparse.csr_matrix((1, 1))
    G = graphs.Graph(W, compute_dtype=np.float64)
    G._lmax = upper_lmax(W) if N > 1 else 1.0  # (one isolated vertex: L = 0, any positive lmax)
    rng = np.random.default_rng(N)
    x = rng.standard_normal((N, nsig))
    for nf in (1, 3):
        z = rng.standard_normal((nf, N, nsig))
        for M in (2, 3, 4):
            m, ref, _ = device_cross(G, x, z, M)
            assert m.shape == (nf, M, nsig) and rel_err(m, ref) < TOL[F64], (nf, M)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_cross_moments_around_the_chunks_of_slots(dtype):
    """The chunks of slots are 4, 8 or 16 long (see PASS, FEW above): slot counts one below, at and one above every
    multiple of each up to two chunks and one, an even and an odd width, a pass on either side of FEW."""
    W = random_graph(700, 6, seed=11, isolated=1)
    G = graph_of(W, dtype)
    rng = np.random.default_rng(11)
    for nsig in (5, 6):
        x = rng.standard_normal((G.N, nsig))
        for nf in (FEW, FEW + 1):
            z = rng.standard_normal((nf, G.N, nsig))
            for M in (3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33):
                m, ref, _ = device_cross(G, x, z, M, dtype)
                assert m.shape == (nf, M, nsig) and rel_err(m, ref) < TOL[np.dtype(dtype)], (nsig, nf, M)


def test_cross_moments_column_batches(ctx):
    W = random_graph(5000, 6, seed=7, isolated=1)
    G = graph_of(W)
    rng = np.random.default_rng(7)
    x, z = rng.standard_normal((G.N, 20)), rng.standard_normal((3, G.N, 20))
    m, ref, _ = device_cross(G, x, z, 21)
    ctx.set_option("max_batch", 8)  # three column batches
    try:
        m3, _, _ = device_cross(G, x, z, 21)
    finally:
        ctx.set_option("max_batch", 0)
    assert G.device_graph(np.float64).ctx is ctx
    assert rel_err(m, ref) < TOL[F64] and rel_err(m3, ref) < TOL[F64]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_cross_moments_in_an_internal_vertex_order(dtype):
    """The kept slots are in the graph's internal order and z is not: only a z read through the permutation meets them
    row for row."""
    G = graphs.Sensor(5000, seed=0, tiles=True, reorder="morton", compute_dtype=dtype)
    G.estimate_lmax("bounds")
    dev = G.device_graph(dtype)
    perm = dev.download_perm()
    assert perm is not None and not np.array_equal(perm, np.arange(G.N))
    rng = np.random.default_rng(0)
    for nsig in (4, 5):
        x, z = rng.standard_normal((G.N, nsig)), rng.standard_normal((2, G.N, nsig))
        m, ref, _ = device_cross(G, x, z, 12, dtype)
        err = rel_err(m, ref)
        print("internal order {} nsig {}: {:.2e}".format(np.dtype(dtype).name, nsig, err))
        assert err < TOL[np.dtype(dtype)]


def test_cross_moments_tile_and_plain_steps(ctx):
    G = graphs.Sensor(40_000, seed=3)
    G.estimate_lmax("bounds")
    rng = np.random.default_rng(3)
    x, z = rng.standard_normal((G.N, 16)), rng.standard_normal((2, G.N, 16))
    m, ref, _ = device_cross(G, x, z, 32)
    tiled = ctx.last_step_kinds()
    ctx.set_option("tile_gather", 0)
    try:
        mp, _, _ = device_cross(G, x, z, 32)
        plain = ctx.last_step_kinds()
    finally:
        ctx.set_option("tile_gather", 1)
    assert G.device_graph(np.float64).ctx is ctx
    assert rel_err(m, ref) < TOL[F64] and rel_err(mp, ref) < TOL[F64]
    # 32 orders from 31 recurrence steps: on the gather tiles the graph carries, then on the plain kernels
    assert tiled == {"tile": 31, "plain": 0} and plain == {"tile": 0, "plain": 31}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_cross_moments_aliased_and_swapped(hub_graphs, dtype):
    G = hub_graphs[np.dtype(dtype)]
    dev = G.device_graph(dtype)
    rng = np.random.default_rng(4)
    x, z = rng.standard_normal((G.N, 6)), rng.standard_normal((G.N, 6))
    d = G.to_device(x, dtype)
    try:
        own, _ = dev.cheby_cross_moments_dev(d.ptr, d.ptr, 6, 1, G.lmax, 14)  # z IS x: the same pointer
        self_moments, _ = dev.cheby_moments_dev(d.ptr, 6, G.lmax, 14)
    finally:
        d.free()
    assert own.shape == (1, 14, 6) and rel_err(own[0], self_moments) < TOL[np.dtype(dtype)]
    a, _ = dev.cheby_cross_moments(x, z[None], G.lmax, 14)
    b, _ = dev.cheby_cross_moments(z, x[None], G.lmax, 14)
    err = rel_err(a, b)
    print("roles swapped {}: {:.2e}".format(np.dtype(dtype).name, err))
    assert err < TOL[np.dtype(dtype)]


def test_spectrum_cross_moments_input_types():
    W = random_graph(1000, 6, seed=2)
    G = graph_of(W)
    rng = np.random.default_rng(2)
    x, z = rng.standard_normal((G.N, 5)), rng.standard_normal((3, G.N, 5))
    host = spectrum.cheby_cross_moments(G, x, z, order=9)
    dx, dz = G.to_device(x), G.to_device(np.moveaxis(z, 0, 2))  # planes [f][n][s] are the cube (N, Nsig, Nf)
    try:
        dev = spectrum.cheby_cross_moments(G, dx, dz, order=9)
    finally:
        dx.free()
        dz.free()
    assert host.shape == (3, 10, 5) and np.array_equal(host, dev)
    assert rel_err(host, cross_moments_direct(orc.laplacian(W), G.lmax, x, z, 10)) < TOL[F64]
    one = spectrum.cheby_cross_moments(G, x, z[1], order=9)
    assert one.shape == (10, 5) and rel_err(one, host[1]) < TOL[F64]
    vec = spectrum.cheby_cross_moments(G, x[:, 2], z[1, :, 2], order=9)
    assert vec.shape == (10,) and rel_err(vec, host[1, :, 2]) < TOL[F64]


def test_ptr_device_knows_the_library_s_own_buffers(ctx):
    from pygsp_amd import _capi
    lib, dev = _capi.load(), ctypes.c_int(-1)
    buf = ctx.alloc(4096)
    try:
        assert lib.gspx_ptr_device(ctypes.c_void_p(buf.ptr), ctypes.byref(dev)) == _capi.OK and dev.value == ctx.device
        assert lib.gspx_ptr_device(ctypes.c_void_p(buf.ptr + 1000), ctypes.byref(dev)) == _capi.OK
        host = np.zeros(16)
        assert lib.gspx_ptr_device(_capi.ptr(host), ctypes.byref(dev)) == _capi.ERR_INVALID and dev.value == -1
        ctx.sync()  # the refused query left no sticky error behind: the next call on the context succeeds
        buf.upload(host)
    finally:
        buf.free()


# ---- the vector-Jacobian product ---------------------------------------------------------------------------------------
def dot(a, b):
    return float(np.vdot(np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()))


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, TOL[F32])])
@pytest.mark.parametrize("Nf", [1, 3])
def test_cheby_op_vjp_linearity_with_the_device_forward(hub_graphs, Nf, dtype, tol):
    """<cot, y> is linear in c and in x: <grad_c, dc> = <cot, cheby_op(dc, x)>, <grad_x, dx> = <cot, cheby_op(c, dx)>,
    forward and backward both on the device."""
    G = hub_graphs[np.dtype(dtype)]
    rng = np.random.default_rng(Nf)
    decay = 0.8 ** np.arange(21)
    c, dc = rng.standard_normal((Nf, 21)) * decay, rng.standard_normal((Nf, 21)) * decay
    x, dx = rng.standard_normal((G.N, 4)), rng.standard_normal((G.N, 4))
    cot = rng.standard_normal((Nf * G.N, 4))
    gx, gc = filters.cheby_op_vjp(G, c, x, cot)
    assert gx.shape == x.shape and gc.shape == c.shape and gc.dtype == np.float64
    rhs_c, rhs_x = dot(cot, filters.cheby_op(G, dc, x)), dot(cot, filters.cheby_op(G, c, dx))
    ec, ex = abs(dot(gc, dc) - rhs_c) / abs(rhs_c), abs(dot(gx, dx) - rhs_x) / abs(rhs_x)
    print("cancellation: |rhs| / (|g| |d|) = {:.2e} (coefficients), {:.2e} (signal)".format(
        abs(rhs_c) / (np.linalg.norm(gc) * np.linalg.norm(dc)), abs(rhs_x) / (np.linalg.norm(gx) * np.linalg.norm(dx))))
    print("vjp linearity {} Nf {}: coefficients {:.2e}, signal {:.2e}".format(np.dtype(dtype).name, Nf, ec, ex))
    assert ec < tol and ex < tol
    r = (lambda a: np.asarray(a).astype(dtype).astype(np.float64))
    _, ref_c = vjp_direct(orc.laplacian(G.W), G.lmax, c, r(x), r(cot).reshape(Nf, G.N, 4))
    err = rel_err(gc, ref_c)
    print("grad_c against the restatement: {:.2e}".format(err))
    assert err < TOL[np.dtype(dtype)]


@pytest.mark.parametrize("synthesis", [False, True])
def test_filter_vjp_of_a_mexican_hat_bank(hub_graphs, synthesis):
    G = hub_graphs[F64]
    bank = filters.MexicanHat(G, Nf=3)
    rng = np.random.default_rng(6)
    s = rng.standard_normal((G.N, 4, 3) if synthesis else (G.N, 4))
    cot = rng.standard_normal((G.N, 4) if synthesis else (G.N, 4, 3))
    gs, gc = bank.filter_vjp(s, cot, order=20)
    c = filters._as_coeff_matrix(filters.compute_cheby_coeff(bank, m=20))
    planes = (lambda a: np.ascontiguousarray(np.moveaxis(a, 2, 0)))
    L = orc.laplacian(G.W)
    if synthesis:
        rx, rc = vjp_direct(L, G.lmax, c, planes(s), cot, True)
        rx = np.moveaxis(rx, 0, 2)
    else:
        rx, rc = vjp_direct(L, G.lmax, c, s, planes(cot), False)
    ex, ec = rel_err(gs, rx), rel_err(gc, rc)
    print("filter_vjp synthesis {}: grad_s {:.2e}, grad_c {:.2e}".format(synthesis, ex, ec))
    assert gs.shape == s.shape and gc.shape == (3, 21) and ex < TOL[F64] and ec < TOL[F64]
    ds = rng.standard_normal(s.shape)
    lhs, rhs = dot(gs, ds), dot(cot, bank.filter(ds, order=20))
    assert abs(lhs - rhs) / abs(rhs) < 1e-10
    # DeviceArrays in, a DeviceArray out, the bits of the host-array call
    d_s, d_cot = G.to_device(s), G.to_device(cot)
    try:
        d_gs, d_gc = bank.filter_vjp(d_s, d_cot, order=20)
        from pygsp_amd import engine
        assert isinstance(d_gs, engine.DeviceArray) and d_gs.shape == s.shape
        assert np.array_equal(np.asarray(d_gs), gs) and np.array_equal(d_gc, gc)
        d_gs.free()
    finally:
        d_s.free()
        d_cot.free()
