"""The Chebyshev graph convolution without a GPU: the numpy restatement (chebconv_helpers) against its own identities
and the oracle's cheby_op, filters.cheby_conv / cheby_conv_vjp and the torch layer (pygsp_amd.nn.cheby_conv, ChebConv)
over a stand-in device object that computes with the restatement, torch.autograd.gradcheck, and the argument checks of
gspx_cheby_conv_dev and gspx_cheby_cross_grams_dev."""
import ctypes

import numpy as np
import pytest

from chebconv_helpers import OracleGraph, bridge_theta, conv_direct, conv_vjp_direct
from conftest import rel_err
from gpu_helpers import random_graph, upper_lmax
from oracle import cheby_oracle as orc
from pygsp_amd import _capi, engine, filters


def small_graph(n=40, seed=3):
    W = random_graph(n, 5, seed=seed, isolated=1)
    return W, orc.laplacian(W), upper_lmax(W)


def dot(a, b):
    return float(np.vdot(np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()))


def test_restatement_satisfies_both_adjoint_identities():
    """<cot, conv(X, theta)> is linear in X and in theta: <grad_X, dX> = <cot, conv(dX, theta)> and
    <grad_theta, dtheta> = <cot, conv(X, dtheta)>."""
    W, L, lmax = small_graph()
    rng = np.random.default_rng(0)
    theta, X, cot = rng.standard_normal((6, 3, 2)), rng.standard_normal((40, 2, 3)), rng.standard_normal((40, 2, 2))
    gx, gt = conv_vjp_direct(L, lmax, X, theta, cot)
    dX, dT = rng.standard_normal(X.shape), rng.standard_normal(theta.shape)
    ex = abs(dot(gx, dX) - dot(cot, conv_direct(L, lmax, dX, theta))) / abs(dot(gx, dX))
    et = abs(dot(gt, dT) - dot(cot, conv_direct(L, lmax, X, dT))) / abs(dot(gt, dT))
    print("signal {:.2e}, theta {:.2e}".format(ex, et))
    assert gx.shape == X.shape and gt.shape == theta.shape and ex < 1e-12 and et < 1e-12


def test_bridge_to_cheby_op():
    """theta[k] = c_k I with theta[0] halved is the scalar filter c: the convolution's sum is plain, pygsp's is not."""
    W, L, lmax = small_graph()
    G = OracleGraph(W, lmax)
    rng = np.random.default_rng(1)
    c, x = rng.standard_normal(7), rng.standard_normal((40, 4))
    y = filters.cheby_conv(G, bridge_theta(c, 4), x)
    ref = orc.cheby_op(L, lmax, c, x)
    err = rel_err(y, ref)
    print("bridge: {:.2e}".format(err))
    assert y.shape == (40, 4) and err < 1e-13
    unhalved = filters.cheby_conv(G, c[:, None, None] * np.eye(4)[None], x)
    assert rel_err(unhalved - 0.5 * c[0] * x, ref) < 1e-13


@pytest.mark.parametrize("batched", [False, True])
def test_filters_cheby_conv_and_vjp_over_a_stand_in_device(batched):
    W, L, lmax = small_graph()
    G = OracleGraph(W, lmax)
    rng = np.random.default_rng(2)
    theta = rng.standard_normal((5, 3, 2))
    x = rng.standard_normal((40, 2, 3) if batched else (40, 3))
    cot = rng.standard_normal((40, 2, 2) if batched else (40, 2))
    y = filters.cheby_conv(G, theta, x)
    assert y.shape == cot.shape and y.dtype == np.float64
    assert np.array_equal(y, conv_direct(L, lmax, x, theta).reshape(cot.shape))
    assert G.dev.calls == ["conv"]
    gx, gt = filters.cheby_conv_vjp(G, theta, x, cot)
    rx, rt = conv_vjp_direct(L, lmax, x, theta, cot)
    assert gx.shape == x.shape and gt.shape == theta.shape and gt.dtype == np.float64
    assert np.array_equal(gx, rx.reshape(x.shape)) and np.array_equal(gt, rt)
    assert G.dev.calls == ["conv", "conv", "cross_grams"]


def test_filters_cheby_conv_refuses_what_it_cannot_take():
    W, L, lmax = small_graph()
    G = OracleGraph(W, lmax)
    theta, x = np.ones((3, 3, 2)), np.ones((40, 3))
    with pytest.raises(ValueError, match="theta must be"):
        filters.cheby_conv(G, np.ones((3, 3)), x)
    with pytest.raises(TypeError, match="invalid shape"):
        filters.cheby_conv(G, theta[:1], x)
    with pytest.raises(ValueError):
        filters.cheby_conv(G, theta, np.ones((39, 3)))
    with pytest.raises(ValueError, match="Fin = 3"):
        filters.cheby_conv(G, theta, np.ones((40, 4)))
    with pytest.raises(ValueError, match="Fin = 3"):
        filters.cheby_conv(G, theta, np.ones((40, 1, 1, 3)))
    with pytest.raises(TypeError, match="complex"):
        filters.cheby_conv(G, theta, x.astype(complex))
    with pytest.raises(ValueError, match="cotangent"):
        filters.cheby_conv_vjp(G, theta, x, np.ones((40, 3)))
    with pytest.raises(TypeError, match=r"\[feature\]\[vertex\]\[signal\]"):
        filters.cheby_conv(G, theta, engine.DeviceArray.__new__(engine.DeviceArray))
    assert G.dev.calls == []


def test_entry_points_refuse_bad_arguments_without_a_device():
    lib = _capi.load()
    theta, out = np.ones((5, 3, 2)), np.zeros((5, 3, 2))
    fake, other = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)  # never dereferenced: the checks fail first

    def refused(rc, words, code=_capi.ERR_INVALID, error=ValueError):
        assert rc == code
        with pytest.raises(error):
            _capi.check(rc)
        assert words in _capi.last_error(), _capi.last_error()

    def conv(lmax=2.0, M=5, fin=3, fout=2, B=4):
        return lib.gspx_cheby_conv_dev(None, lmax, M, fin, fout, _capi.ptr(theta), B, fake, other, None)

    def grams(lmax=2.0, M=5, fin=3, fout=2, B=4):
        return lib.gspx_cheby_cross_grams_dev(None, lmax, M, fin, fout, B, fake, other, _capi.ptr(out), None)

    for f in (conv, grams):
        refused(f(), "null graph")
        refused(f(M=1), "invalid shape", _capi.ERR_COEFF, TypeError)
        refused(f(M=257), "2 to 256")
        for bad in (0, 129, -1):
            refused(f(fin=bad), "1 to 128 features")
            refused(f(fout=bad), "1 to 128 features")
        refused(f(B=-1), "negative number of samples")
        for lmax in (0.0, -1.0, float("nan"), float("inf")):
            refused(f(lmax=lmax), "lmax must be positive")


# ---- the torch layer -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_nn():
    """(torch, pygsp_amd.nn), imported when the first test asks - and after libgspx has loaded AND initialised its HIP
    runtime, as tests/test_autograd_host.py does and for its reason.  torch only ever computes on the CPU here."""
    _capi.load()
    _capi.device_count()
    torch = pytest.importorskip("torch")
    from pygsp_amd import nn
    return torch, nn


def tiny_graph(n=20):
    W = random_graph(n, 4, seed=9)
    return OracleGraph(W, upper_lmax(W))


@pytest.mark.parametrize("which", ["both", "theta", "x"])
def test_gradcheck(torch_nn, which):
    torch, nn = torch_nn
    G = tiny_graph()
    gen = torch.Generator().manual_seed(3)
    theta = torch.randn((4, 3, 2), dtype=torch.float64, generator=gen, requires_grad=which in ("both", "theta"))
    x = torch.randn((20, 2, 3), dtype=torch.float64, generator=gen, requires_grad=which in ("both", "x"))
    assert torch.autograd.gradcheck(lambda t, s: nn.cheby_conv(G, t, s), (theta, x), eps=1e-6, atol=1e-7, rtol=1e-6)
    # needs_input_grad decides which device calls the backward pass makes
    G.dev.calls.clear()
    y = nn.cheby_conv(G, theta, x)
    assert y.shape == (20, 2, 2) and y.dtype == torch.float64 and nn.last_path == "staged"
    y.sum().backward()
    assert G.dev.calls == ["conv"] + {"both": ["conv", "cross_grams"], "theta": ["cross_grams"], "x": ["conv"]}[which]
    assert nn.last_path == "staged"


def test_cheby_conv_shapes_dtypes_and_values(torch_nn):
    torch, nn = torch_nn
    G = tiny_graph()
    gen = torch.Generator().manual_seed(4)
    theta = torch.randn((3, 3, 2), dtype=torch.float32, generator=gen, requires_grad=True)
    x = torch.randn((20, 3), dtype=torch.float64, generator=gen, requires_grad=True)
    y = nn.cheby_conv(G, theta, x)
    ref = conv_direct(G.L, G.lmax, x.detach().numpy(), theta.detach().numpy().astype(np.float64))
    assert y.shape == (20, 2) and np.array_equal(y.detach().numpy(), ref[:, 0, :])
    cot = torch.randn((20, 2), dtype=torch.float64, generator=gen)
    (y * cot).sum().backward()
    rx, rt = conv_vjp_direct(G.L, G.lmax, x.detach().numpy(), theta.detach().numpy().astype(np.float64), cot.numpy())
    assert theta.grad.shape == (3, 3, 2) and theta.grad.dtype == torch.float32
    assert x.grad.shape == (20, 3) and x.grad.dtype == torch.float64
    assert np.array_equal(x.grad.numpy(), rx[:, 0, :]) and rel_err(theta.grad.numpy(), rt) < 1e-6
    twice = nn.cheby_conv(G, theta, x, lmax=2 * G.lmax)
    assert not np.array_equal(twice.detach().numpy(), y.detach().numpy())
    with pytest.raises(TypeError):
        nn.cheby_conv(G, theta, x.to(torch.float16))
    with pytest.raises(ValueError):
        nn.cheby_conv(G, theta, x.reshape(20, 1, 1, 3))
    with pytest.raises(ValueError):
        nn.cheby_conv(G, theta[0], x)
    with pytest.raises(ValueError):
        nn.cheby_conv(G, theta, x[:, :2])


def test_chebconv_module(torch_nn):
    torch, nn = torch_nn
    G = tiny_graph()
    torch.manual_seed(0)
    layer = nn.ChebConv(G, 3, 5, order=4)
    names = dict(layer.named_parameters())
    assert sorted(names) == ["bias", "theta"]
    assert layer.theta.shape == (5, 3, 5) and layer.theta.dtype == torch.float64
    assert layer.bias.shape == (5,) and not layer.bias.detach().numpy().any()
    bound = np.sqrt(6.0 / (5 * 3 + 5))  # Glorot-uniform over a fan-in of (order + 1) Fin
    assert float(layer.theta.detach().abs().max()) <= bound and float(layer.theta.detach().abs().max()) > 0.5 * bound
    assert "in_features=3, out_features=5, order=4, bias=True" in repr(layer)
    x2, x3 = torch.randn((20, 3), dtype=torch.float64), torch.randn((20, 2, 3), dtype=torch.float32)
    y2, y3 = layer(x2), layer(x3)
    assert y2.shape == (20, 5) and y2.dtype == torch.float64 and y3.shape == (20, 2, 5) and y3.dtype == torch.float32
    with torch.no_grad():
        layer.bias += 1.5
    ref = conv_direct(G.L, G.lmax, x2.numpy(), layer.theta.detach().numpy())[:, 0, :] + 1.5
    assert rel_err(layer(x2).detach().numpy(), ref) < 1e-14
    plain = nn.ChebConv(G, 3, 5, order=1, bias=False)
    assert plain.bias is None and [n for n, _ in plain.named_parameters()] == ["theta"]
    assert "bias=False" in repr(plain) and plain(x2).shape == (20, 5)
    for order in (0, -1):
        with pytest.raises(ValueError, match="order"):
            nn.ChebConv(G, 3, 5, order=order)
    loss = (layer(x3) ** 2).sum()
    loss.backward()
    assert layer.theta.grad.shape == (5, 3, 5) and torch.isfinite(layer.theta.grad).all()
    assert layer.bias.grad.shape == (5,)
