"""Differentiable Chebyshev filtering without a GPU: the numpy restatement of the cross-moments and of the
vector-Jacobian product (autograd_helpers) against the self-moments and the linearity of the filter, filters.cheby_op_vjp
/ Filter.filter_vjp and the torch layer (pygsp_amd.nn) over a stand-in device object that computes with the oracle,
torch.autograd.gradcheck, the ChebyshevFilter module, and the argument checks of the two new entry points."""
import ctypes

import numpy as np
import pytest

from autograd_helpers import (OracleGraph, analysis_direct, cross_moments_direct, synthesis_direct, vjp_direct)
from conftest import rel_err
from gpu_helpers import random_graph, upper_lmax
from oracle import cheby_oracle as orc
from pygsp_amd import _capi, filters, spectrum
from spectrum_helpers import moments_direct


def small_graph(n=40, seed=3):
    W = random_graph(n, 5, seed=seed, isolated=1)
    return W, orc.laplacian(W), upper_lmax(W)


def test_cross_moments_of_a_signal_with_itself_are_its_moments():
    W, L, lmax = small_graph(300)
    x = np.random.default_rng(0).standard_normal((300, 5))
    m = cross_moments_direct(L, lmax, x, x, 12)
    assert m.shape == (1, 12, 5) and np.array_equal(m[0], moments_direct(L, lmax, x, 12))


def test_cross_moments_are_symmetric_in_their_arguments():
    """<z, T_k x> = <x, T_k z> for a symmetric L."""
    W, L, lmax = small_graph(300)
    rng = np.random.default_rng(1)
    x, z = rng.standard_normal((300, 4)), rng.standard_normal((300, 4))
    a, b = cross_moments_direct(L, lmax, x, z, 20), cross_moments_direct(L, lmax, z, x, 20)
    err = rel_err(a, b)
    print("roles swapped: {:.2e}".format(err))
    assert a.shape == (1, 20, 4) and err < 1e-12


def dot(a, b):
    return float(np.vdot(np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()))


def linearity_errors(L, lmax, c, x, cot, grad_x, grad_c, synthesis, seed):
    """The loss <cot, y> is linear in c and in x: <grad_c, dc> = <cot, y(dc, x)> and <grad_x, dx> = <cot, y(c, dx)>.
    Returns the two relative deviations (the factor 1/2 on c_0 is what the first one catches)."""
    rng = np.random.default_rng(seed)
    dc, dx = rng.standard_normal(np.shape(c)), rng.standard_normal(np.shape(x))
    forward = synthesis_direct if synthesis else analysis_direct
    lhs_c, rhs_c = dot(grad_c, dc), dot(cot, forward(L, lmax, dc, x))
    lhs_x, rhs_x = dot(grad_x, dx), dot(cot, forward(L, lmax, c, dx))
    return abs(lhs_c - rhs_c) / abs(rhs_c), abs(lhs_x - rhs_x) / abs(rhs_x)


@pytest.mark.parametrize("synthesis", [False, True])
@pytest.mark.parametrize("Nf", [1, 3])
def test_vjp_direct_satisfies_both_linearity_identities(Nf, synthesis):
    W, L, lmax = small_graph()
    rng = np.random.default_rng(Nf)
    c = rng.standard_normal((Nf, 9))
    x = rng.standard_normal((Nf, 40, 4) if synthesis else (40, 4))
    cot = rng.standard_normal((40, 4) if synthesis else (Nf, 40, 4))
    gx, gc = vjp_direct(L, lmax, c, x, cot, synthesis)
    ec, ex = linearity_errors(L, lmax, c, x, cot, gx, gc, synthesis, seed=7)
    print("Nf {} synthesis {}: coefficients {:.2e}, signal {:.2e}".format(Nf, synthesis, ec, ex))
    assert gx.shape == x.shape and gc.shape == c.shape and ec < 1e-12 and ex < 1e-12


@pytest.mark.parametrize("Nf", [1, 3])
def test_cheby_op_vjp_over_a_stand_in_device(Nf):
    W, L, lmax = small_graph()
    G = OracleGraph(W, lmax)
    rng = np.random.default_rng(10 + Nf)
    c, x, cot = rng.standard_normal((Nf, 7)), rng.standard_normal((40, 3)), rng.standard_normal((Nf * 40, 3))
    gx, gc = filters.cheby_op_vjp(G, c, x, cot)
    rx, rc = vjp_direct(L, lmax, c, x, cot.reshape(Nf, 40, 3))
    assert gx.shape == x.shape and gc.shape == c.shape and gc.dtype == np.float64
    assert np.array_equal(gx, rx) and np.array_equal(gc, rc)
    assert G.dev.calls == ["synthesis", "cross_moments"]
    ec, ex = linearity_errors(L, lmax, c, x, cot.reshape(Nf, 40, 3), gx, gc, False, seed=8)
    assert ec < 1e-12 and ex < 1e-12
    # one vector of coefficients, one signal vector: the shapes of the arguments come back
    g1, c1 = filters.cheby_op_vjp(G, c[0], x[:, 0], cot[:40, 0])
    assert g1.shape == (40,) and c1.shape == (7,)
    assert rel_err(c1, vjp_direct(L, lmax, c[:1], x[:, :1], cot[:40, :1].reshape(1, 40, 1))[1][0]) < 1e-13


def test_cheby_op_vjp_refuses_other_evaluations_and_device_lists():
    W, L, lmax = small_graph()
    G = OracleGraph(W, lmax)
    c, x, cot = np.ones((1, 4)), np.ones((40, 2)), np.ones((40, 2))
    for how in ("product", "newton", "auto"):
        with pytest.raises(ValueError, match="recurrence"):
            filters.cheby_op_vjp(G, c, x, cot, evaluation=how)
    with pytest.raises(ValueError, match="device list"):
        filters.cheby_op_vjp(G, c, x, cot, devices=[0, 1])
    with pytest.raises(ValueError, match="cotangent"):
        filters.cheby_op_vjp(G, c, x, np.ones((41, 2)))
    assert G.dev.calls == []
    gx, gc = filters.cheby_op_vjp(G, c, x, cot, evaluation="recurrence")
    assert gx.shape == (40, 2) and gc.shape == (1, 4)


@pytest.mark.parametrize("synthesis", [False, True])
def test_filter_vjp_over_a_stand_in_device(synthesis):
    W, L, lmax = small_graph()
    G = OracleGraph(W, lmax)
    bank = filters.MexicanHat(G, Nf=3)
    rng = np.random.default_rng(5)
    s = rng.standard_normal((40, 4, 3) if synthesis else (40, 4))
    cot = rng.standard_normal((40, 4) if synthesis else (40, 4, 3))
    gs, gc = bank.filter_vjp(s, cot, order=8)
    c = filters._as_coeff_matrix(filters.compute_cheby_coeff(bank, m=8))
    planes = (lambda a: np.ascontiguousarray(np.moveaxis(a, 2, 0)))
    if synthesis:
        rx, rc = vjp_direct(L, lmax, c, planes(s), cot, True)
        rx = np.moveaxis(rx, 0, 2)
    else:
        rx, rc = vjp_direct(L, lmax, c, s, planes(cot), False)
    assert gs.shape == s.shape and gc.shape == (3, 9)
    assert np.array_equal(gs, rx) and np.array_equal(gc, rc)
    # against the forward the reference defines (oracle.filter_chebyshev): <cot, filter(ds)> = <grad_s, ds>
    ds = rng.standard_normal(s.shape)
    kernels = [bank._kernels[i] for i in range(3)]
    y = orc.filter_chebyshev(L, lmax, kernels, ds, order=8)
    assert abs(dot(cot, y) - dot(gs, ds)) / abs(dot(cot, y)) < 1e-12


def test_spectrum_cross_moments_over_a_stand_in_device(monkeypatch):
    W, L, lmax = small_graph()
    G = OracleGraph(W, lmax)
    monkeypatch.setattr(filters, "_device_graph_of", lambda G_: G.dev)
    rng = np.random.default_rng(2)
    x, z = rng.standard_normal((40, 3)), rng.standard_normal((2, 40, 3))
    m = spectrum.cheby_cross_moments(G, x, z, order=6)
    assert m.shape == (2, 7, 3) and np.array_equal(m, cross_moments_direct(L, lmax, x, z, 7))
    one = spectrum.cheby_cross_moments(G, x, z[0], order=6)
    assert one.shape == (7, 3) and np.array_equal(one, m[0])
    vec = spectrum.cheby_cross_moments(G, x[:, 1], z[1, :, 1], order=6)
    assert vec.shape == (7,) and np.array_equal(vec, cross_moments_direct(L, lmax, x[:, 1:2], z[1, :, 1:2], 7)[0, :, 0])
    with pytest.raises(ValueError):
        spectrum.cheby_cross_moments(G, x, z[:, :, :2])
    with pytest.raises(ValueError):
        spectrum.cheby_cross_moments(G, np.zeros((39, 3)), z)


def test_entry_points_refuse_bad_arguments_without_a_device():
    lib = _capi.load()
    out = np.zeros((2, 5, 4))
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: the checks fail first

    def refused(rc, words):
        assert rc == _capi.ERR_INVALID
        with pytest.raises(ValueError):
            _capi.check(rc)
        assert words in _capi.last_error(), _capi.last_error()

    f = lib.gspx_cheby_cross_moments_dev
    refused(f(None, 2.0, 5, 4, fake, 2, fake, _capi.ptr(out), None), "null graph")
    refused(f(None, 2.0, 1, 4, fake, 2, fake, _capi.ptr(out), None), "2 to 256")
    refused(f(None, 2.0, 257, 4, fake, 2, fake, _capi.ptr(out), None), "2 to 256")
    refused(f(None, 2.0, 5, 4, fake, 0, fake, _capi.ptr(out), None), "Nf must be")
    refused(f(None, 2.0, 5, -1, fake, 2, fake, _capi.ptr(out), None), "negative number of signals")
    for lmax in (0.0, -1.0, float("nan"), float("inf")):
        refused(f(None, lmax, 5, 4, fake, 2, fake, _capi.ptr(out), None), "lmax must be positive")
    dev = ctypes.c_int(7)
    refused(lib.gspx_ptr_device(None, ctypes.byref(dev)), "null argument")
    refused(lib.gspx_ptr_device(fake, None), "null argument")
    assert dev.value == 7


# ---- the torch layer -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_nn():
    """(torch, pygsp_amd.nn), imported when the first test asks - and after libgspx has loaded AND initialised its HIP
    runtime (device_count does; it answers 0 without a GPU): a process that also runs the GPU tests must keep the
    runtime libgspx links against.  Seen on the card: with torch imported between the load and the first HIP call of
    libgspx, torch's bundled runtime claimed the GPU and every later gspx_ctx_create found no device.  torch only ever
    computes on the CPU here."""
    _capi.load()
    _capi.device_count()
    torch = pytest.importorskip("torch")
    from pygsp_amd import nn
    return torch, nn


def tiny_graph():
    W = random_graph(12, 4, seed=9)
    return OracleGraph(W, upper_lmax(W))


@pytest.mark.parametrize("which", ["both", "coeffs", "x"])
@pytest.mark.parametrize("Nf", [1, 2])
def test_gradcheck(torch_nn, Nf, which):
    torch, nn = torch_nn
    G = tiny_graph()
    gen = torch.Generator().manual_seed(Nf)
    coeffs = torch.randn((Nf, 4), dtype=torch.float64, generator=gen, requires_grad=which in ("both", "coeffs"))
    x = torch.randn((12, 3), dtype=torch.float64, generator=gen, requires_grad=which in ("both", "x"))
    assert torch.autograd.gradcheck(lambda c, s: nn.cheby_filter(G, c, s), (coeffs, x), eps=1e-6, atol=1e-7, rtol=1e-6)
    # needs_input_grad decides which device calls the backward pass makes
    G.dev.calls.clear()
    y = nn.cheby_filter(G, coeffs, x)
    assert y.shape == (12, 3, Nf) and y.dtype == torch.float64
    y.sum().backward()
    assert G.dev.calls == ["analysis"] + {"both": ["synthesis", "cross_moments"], "coeffs": ["cross_moments"],
                                          "x": ["synthesis"]}[which]


def test_cheby_filter_shapes_and_dtypes(torch_nn):
    torch, nn = torch_nn
    G = tiny_graph()
    c = torch.tensor([2.0, 0.5, -0.25], dtype=torch.float32, requires_grad=True)
    x = torch.arange(12, dtype=torch.float64, requires_grad=True)
    y = nn.cheby_filter(G, c, x)
    ref = analysis_direct(G.L, G.lmax, c.detach().numpy().astype(np.float64), x.detach().numpy()[:, None])
    assert y.shape == (12, 1, 1) and np.array_equal(y.detach().numpy()[:, :, 0], ref[0])
    y.sum().backward()
    assert c.grad.shape == (3,) and c.grad.dtype == torch.float32 and x.grad.shape == (12,) and x.grad.dtype == torch.float64
    twice = nn.cheby_filter(G, c, x, lmax=2 * G.lmax)
    assert not np.array_equal(twice.detach().numpy(), y.detach().numpy())
    with pytest.raises(TypeError):
        nn.cheby_filter(G, c, x.to(torch.float16))
    with pytest.raises(ValueError):
        nn.cheby_filter(G, c, x.reshape(12, 1, 1))


def test_chebyshev_filter_module(torch_nn):
    torch, nn = torch_nn
    G = tiny_graph()
    layer = nn.ChebyshevFilter(G, n_filters=2, order=5)
    params = list(layer.parameters())
    assert len(params) == 1 and params[0] is layer.coeffs and layer.coeffs.shape == (2, 6) and layer.n_filters == 2
    x = torch.randn((12, 3), dtype=torch.float64)
    y = layer.double()(x)
    assert y.shape == (12, 3, 2)
    for f in range(2):  # the identity start
        assert rel_err(y.detach().numpy()[:, :, f], x.numpy()) < 1e-14
    bank = filters.Heat(G, scale=[5, 20])
    heat = nn.ChebyshevFilter(G, n_filters=2, order=7, init=bank).double()
    assert np.array_equal(heat.coeffs.detach().numpy(),
                          filters._as_coeff_matrix(filters.compute_cheby_coeff(bank, m=7)))
    with pytest.raises(ValueError):
        nn.ChebyshevFilter(G, n_filters=3, order=7, init=bank)
    loss = (heat(x) ** 2).sum()
    loss.backward()
    assert heat.coeffs.grad.shape == (2, 8) and torch.isfinite(heat.coeffs.grad).all()
