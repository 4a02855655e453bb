"""The edge-weight gradient of Chebyshev filters without a GPU: the numpy restatement (wgrad_helpers) against dense
torch autograd and central differences, filters.cheby_op_vjp_laplacian / cheby_op_vjp_weights / Filter.filter_vjp_weights
and the torch layer (pygsp_amd.nn.WeightedGraph, nn.cheby_filter) over a stand-in device object that computes with the
restatement, torch.autograd.gradcheck, and the argument checks of gspx_cheby_laplacian_grad_dev."""
import ctypes

import numpy as np
import pytest
from scipy import sparse

from conftest import rel_err
from gpu_helpers import random_graph, upper_lmax
from oracle import cheby_oracle as orc
from pygsp_amd import _capi, filters
from wgrad_helpers import WgradGraph, adjacency_of, laplacian_grad_direct, torch_filter_dense, weights_grad_direct


def pattern_of(W, extra, seed):
    """(pairs (2, P), weights (P,)): the upper-triangle edges of W, then `extra` pairs that are no edges (weight 0),
    some of them the other way round."""
    rng = np.random.default_rng(seed)
    C = sparse.triu(W, format="coo")
    N, have, more = W.shape[0], set(zip(C.row.tolist(), C.col.tolist())), []
    while len(more) < extra:
        s, t = sorted(rng.integers(0, N, 2).tolist())
        if s != t and (s, t) not in have:
            have.add((s, t))
            more.append((s, t) if len(more) % 2 else (t, s))
    pairs = np.concatenate([np.stack([C.row, C.col]), np.array(more, dtype=np.int64).reshape(-1, 2).T], axis=1)
    return pairs, np.concatenate([C.data, np.zeros(extra)])


def lmax_of(W, lap_type):
    return upper_lmax(W) if lap_type == "combinatorial" else 2.0


@pytest.fixture(scope="module")
def torch_nn():
    """(torch, pygsp_amd.nn), imported when the first test asks - and after libgspx has loaded AND initialised its HIP
    runtime, as tests/test_chebconv_host.py does and for its reason.  torch only ever computes on the CPU here."""
    _capi.load()
    _capi.device_count()
    torch = pytest.importorskip("torch")
    from pygsp_amd import nn
    return torch, nn


# ---- the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lap_type", ["combinatorial", "normalized"])
@pytest.mark.parametrize("M", [2, 3, 9, 31])
@pytest.mark.parametrize("Nf", [1, 3])
def test_restatement_against_dense_torch_autograd(torch_nn, lap_type, M, Nf):
    torch, _ = torch_nn
    W = random_graph(30, 4, seed=M, isolated=1)
    lmax = lmax_of(W, lap_type)
    pairs, w0 = pattern_of(W, 12, seed=M)
    rng = np.random.default_rng(100 * M + Nf)
    for nsig in (1, 4):
        c, x = rng.standard_normal((Nf, M)), rng.standard_normal((30, nsig))
        cot = rng.standard_normal((Nf, 30, nsig))
        w = torch.tensor(w0, requires_grad=True)
        y = torch_filter_dense(torch, 30, pairs, w, lap_type, lmax, torch.from_numpy(c), torch.from_numpy(x))
        (y * torch.from_numpy(cot)).sum().backward()
        grad = weights_grad_direct(W, lap_type, lmax, c, x, cot, pairs)
        err = rel_err(grad, w.grad.numpy())
        print("{} M {} Nf {} nsig {}: {:.2e}".format(lap_type, M, Nf, nsig, err))
        assert grad.shape == w0.shape and np.abs(grad[w0 == 0]).max() > 0 and err < 1e-12


@pytest.mark.parametrize("lap_type", ["combinatorial", "normalized"])
def test_restatement_against_central_differences(lap_type):
    W = random_graph(30, 4, seed=1)
    lmax = lmax_of(W, lap_type)
    pairs, w0 = pattern_of(W, 4, seed=1)
    rng = np.random.default_rng(1)
    c, x, cot = rng.standard_normal((2, 9)) * 0.8 ** np.arange(9), rng.standard_normal((30, 3)), rng.standard_normal((60, 3))
    grad = weights_grad_direct(W, lap_type, lmax, c, x, cot.reshape(2, 30, 3), pairs)

    def loss(w):
        return float((cot * orc.cheby_op(orc.laplacian(adjacency_of(30, pairs, w), lap_type), lmax, c, x)).sum())

    h = 1e-5
    for p in (0, 7, w0.size - 1):  # two edges and a pair that is none (its weight goes to +-h: the formula is smooth there)
        e = np.zeros_like(w0)
        e[p] = h
        fd = (loss(w0 + e) - loss(w0 - e)) / (2 * h)
        print("{} pair {}: {:.3e} against {:.3e}".format(lap_type, p, grad[p], fd))
        assert abs(fd - grad[p]) < 1e-6 * np.abs(grad).max()


# ---- the Python layer over a stand-in device --------------------------------------------------------------------------
@pytest.mark.parametrize("lap_type", ["combinatorial", "normalized"])
def test_python_layer_shapes_and_values(lap_type):
    W = random_graph(40, 5, seed=3)
    lmax = lmax_of(W, lap_type)
    G = WgradGraph(W, lmax, lap_type)
    pairs, _ = pattern_of(W, 6, seed=3)
    extra = pairs[:, -6:]
    E = sparse.triu(W).nnz
    rng = np.random.default_rng(3)
    c, x, cot = rng.standard_normal((2, 6)), rng.standard_normal((40, 3)), rng.standard_normal((80, 3))
    gdiag, goff = filters.cheby_op_vjp_laplacian(G, c, x, cot)
    rd, ro = laplacian_grad_direct(G.dev.L, lmax, c, x, cot.reshape(2, 40, 3), pairs[:, :E])
    assert gdiag.shape == (40,) and goff.shape == (E,) and gdiag.dtype == goff.dtype == np.float64
    assert np.array_equal(gdiag, rd) and np.array_equal(goff, ro)
    gd2, go2 = filters.cheby_op_vjp_laplacian(G, c, x, cot, pairs=extra)
    assert go2.shape == (6,) and np.array_equal(gd2, rd)
    own = filters.cheby_op_vjp_weights(G, c, x, cot)
    ref = weights_grad_direct(W, lap_type, lmax, c, x, cot.reshape(2, 40, 3), pairs)
    assert own.shape == (E,) and own.dtype == np.float64 and rel_err(own, ref[:E]) < 1e-13
    G.dev.calls.clear()
    G.dev.pair_counts.clear()
    more = filters.cheby_op_vjp_weights(G, c, x, cot, pairs=extra)
    assert more.shape == (6,) and rel_err(more, ref[E:]) < 1e-13
    # ONE device call: normalized on the graph's own edges and the pairs together
    assert G.dev.calls == ["laplacian_grad"]
    assert G.dev.pair_counts == [E + 6 if lap_type == "normalized" else 6]
    # a 1-D signal and a single coefficient vector
    one = filters.cheby_op_vjp_weights(G, c[0], x[:, 0], cot[:40, 0])
    assert one.shape == (E,)
    assert rel_err(one, weights_grad_direct(W, lap_type, lmax, c[0], x[:, :1], cot[None, :40, :1], pairs[:, :E])) < 1e-13
    assert filters.cheby_op_vjp_weights(G, c, x, cot, pairs=np.zeros((2, 0), dtype=np.int64)).shape == (0,)


@pytest.mark.parametrize("lap_type", ["combinatorial", "normalized"])
def test_filter_vjp_weights_analysis_and_the_synthesis_swap(lap_type):
    W = random_graph(40, 5, seed=4)
    lmax = lmax_of(W, lap_type)
    G = WgradGraph(W, lmax, lap_type)
    bank = filters.MexicanHat(G, Nf=3)
    c = filters._as_coeff_matrix(filters.compute_cheby_coeff(bank, m=8))
    rng = np.random.default_rng(4)
    s, cot = rng.standard_normal((40, 4)), rng.standard_normal((40, 4, 3))
    planes = np.ascontiguousarray(np.moveaxis(cot, 2, 0))
    pairs, _ = pattern_of(W, 5, seed=4)
    ana = bank.filter_vjp_weights(s, cot, order=8, pairs=pairs)
    assert ana.shape == (pairs.shape[1],)
    assert np.array_equal(ana, filters.cheby_op_vjp_weights(G, c, s, planes.reshape(120, 4), pairs=pairs))
    assert rel_err(ana, weights_grad_direct(W, lap_type, lmax, c, s, planes, pairs)) < 1e-13
    # synthesis y = sum_f p_f(L) s_f with cotangent g: the analysis call with signal g and cotangent planes s_f
    syn = bank.filter_vjp_weights(cot, s, order=8, pairs=pairs)
    assert np.array_equal(syn, ana)
    own = bank.filter_vjp_weights(s, cot, order=8)
    assert own.shape == (sparse.triu(W).nnz,)
    with pytest.raises(ValueError, match="cotangent"):
        bank.filter_vjp_weights(s, cot[:, :3], order=8)


def test_python_layer_refuses_before_the_device():
    W = random_graph(40, 5, seed=5, isolated=1)
    lmax = upper_lmax(W)
    G = WgradGraph(W, lmax)
    c, x, cot = np.ones((2, 4)), np.ones((40, 3)), np.ones((80, 3))
    iso = int(np.flatnonzero(np.ravel(W.sum(axis=1)) == 0)[0])
    other = (iso + 1) % 40
    for f in (filters.cheby_op_vjp_laplacian, filters.cheby_op_vjp_weights):
        with pytest.raises(ValueError, match="evaluation"):
            f(G, c, x, cot, evaluation="newton")
        with pytest.raises(ValueError, match="device list"):
            f(G, c, x, cot, devices=[0, 1])
        with pytest.raises(ValueError, match="cotangent"):
            f(G, c, x, cot[:40])
        with pytest.raises(ValueError, match="number of vertices"):
            f(G, c, x[:39], cot)
        with pytest.raises(TypeError, match="complex"):
            f(G, c, x.astype(complex), cot)
        with pytest.raises(TypeError, match="invalid shape"):
            f(G, np.ones((2, 1)), x, cot)
        with pytest.raises(ValueError, match="must be"):
            f(G, c, x, cot, pairs=np.zeros((3, 2), dtype=np.int64))
        with pytest.raises(TypeError, match="integer"):
            f(G, c, x, cot, pairs=np.zeros((2, 2)))
        with pytest.raises(ValueError, match="outside"):
            f(G, c, x, cot, pairs=np.array([[0], [40]]))
        with pytest.raises(ValueError, match="outside"):
            f(G, c, x, cot, pairs=np.array([[-1], [3]]))
        with pytest.raises(ValueError, match="different"):
            f(G, c, x, cot, pairs=np.array([[3], [3]]))
    with pytest.raises(ValueError, match="undirected"):
        filters.cheby_op_vjp_weights(WgradGraph(W, lmax, directed=True), c, x, cot)
    loops = sparse.csr_matrix(W + sparse.diags(np.r_[1.0, np.zeros(39)]))
    with pytest.raises(ValueError, match="self-loops"):
        filters.cheby_op_vjp_weights(WgradGraph(loops, lmax), c, x, cot)
    GL = WgradGraph(loops, lmax)
    assert filters.cheby_op_vjp_weights(GL, c, x, cot, pairs=np.array([[1], [2]])).shape == (1,)  # (L = D - W has none)
    GN = WgradGraph(W, 2.0, "normalized")
    with pytest.raises(ValueError, match="positive degree"):
        filters.cheby_op_vjp_weights(GN, c, x, cot, pairs=np.array([[iso], [other]]))
    with pytest.raises(ValueError, match="self-loops"):
        filters.cheby_op_vjp_weights(WgradGraph(loops, 2.0, "normalized"), c, x, cot, pairs=np.array([[1], [2]]))
    assert G.dev.calls == [] and GN.dev.calls == []


# ---- the torch layer -------------------------------------------------------------------------------------------------
def stand_in(nn, builds):
    class StandIn(nn.WeightedGraph):
        """A WeightedGraph whose graphs are WgradGraphs (no device); `builds` counts the rebuilds."""

        def _build(self, W):
            builds.append(W)
            return WgradGraph(W, self.G.lmax, self.G.lap_type)
    return StandIn


def module_on(cls, G, pairs, w):
    """A module whose ``weight`` IS the tensor w (gradcheck perturbs its inputs, not a module's Parameter)."""
    m = cls(G, pairs)
    del m.weight
    m.weight = w
    return m


@pytest.mark.parametrize("lap_type", ["combinatorial", "normalized"])
def test_gradcheck_in_the_weights_and_in_all_three_inputs(torch_nn, lap_type):
    torch, nn = torch_nn
    W = random_graph(14, 4, seed=8)
    G = WgradGraph(W, lmax_of(W, lap_type), lap_type)
    pairs, _ = pattern_of(W, 4, seed=8)
    cls = stand_in(nn, [])
    gen = torch.Generator().manual_seed(8)
    w = (0.2 + torch.rand(pairs.shape[1], dtype=torch.float64, generator=gen)).requires_grad_(True)
    c = torch.randn((2, 5), dtype=torch.float64, generator=gen)
    x = torch.randn((14, 3), dtype=torch.float64, generator=gen)
    lmax = 2.0 if lap_type == "normalized" else 4.0 * float(w.detach().sum())  # bounds every perturbed iterate
    f = (lambda w_, c_, x_: nn.cheby_filter(module_on(cls, G, pairs, w_), c_, x_, lmax=lmax))
    assert torch.autograd.gradcheck(f, (w, c, x), eps=1e-6, atol=1e-7, rtol=1e-6)
    c.requires_grad_(True)
    x.requires_grad_(True)
    assert torch.autograd.gradcheck(f, (w, c, x), eps=1e-6, atol=1e-7, rtol=1e-6)


def test_weighted_graph_module(torch_nn):
    torch, nn = torch_nn
    W = random_graph(20, 4, seed=9)
    G = WgradGraph(W, upper_lmax(W))
    builds = []
    cls = stand_in(nn, builds)
    C = sparse.triu(W, format="coo")
    m = cls(G)
    assert [n for n, _ in m.named_parameters()] == ["weight"]
    assert m.weight.dtype == torch.float64 and np.array_equal(m.weight.detach().numpy(), C.data)
    assert np.array_equal(m.pairs, np.stack([C.row, C.col]))
    g1 = m.graph()
    assert m.graph() is g1 and len(builds) == 1 and abs(g1.W - W).max() == 0 and g1.lap_type == G.lap_type
    with torch.no_grad():
        m.weight[0] = 0.0  # a zero weight leaves W; the pattern keeps the pair
    g2 = m.graph()
    assert g2 is not g1 and len(builds) == 2 and g2.W.nnz == W.nnz - 2 and m.graph() is g2 and len(builds) == 2
    assert g2.W[C.row[0], C.col[0]] == 0 and m.pairs.shape[1] == C.row.size
    with torch.no_grad():
        m.weight[1] = -0.5
    with pytest.raises(ValueError, match="negative"):
        m.graph()
    with torch.no_grad():
        m.weight[1] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        m.graph()
    # a given pattern: weights from G, 0 where a pair is no edge; the pairs must be unique as unordered pairs
    pairs, w0 = pattern_of(W, 3, seed=9)
    p = cls(G, pairs)
    assert np.array_equal(p.weight.detach().numpy(), w0) and abs(p.graph().W - W).max() == 0
    with pytest.raises(ValueError, match="unique"):
        cls(G, np.array([[0, 1], [1, 0]]))
    with pytest.raises(ValueError, match="different"):
        cls(G, np.array([[2], [2]]))
    with pytest.raises(ValueError, match="undirected"):
        cls(WgradGraph(W, 1.0, directed=True))
    assert "pairs={}".format(C.row.size) in repr(m)


def test_backward_runs_the_weight_call_only_when_asked(torch_nn):
    torch, nn = torch_nn
    W = random_graph(20, 4, seed=10)
    G = WgradGraph(W, upper_lmax(W))
    pairs, w0 = pattern_of(W, 3, seed=10)
    made = []
    m = stand_in(nn, made)(G, pairs)
    gen = torch.Generator().manual_seed(10)
    c = torch.randn((2, 6), dtype=torch.float64, generator=gen, requires_grad=True)
    x = torch.randn((20, 3), dtype=torch.float64, generator=gen, requires_grad=True)
    cot = torch.randn((20, 3, 2), dtype=torch.float64, generator=gen)
    lmax = 1.5 * G.lmax
    y = nn.cheby_filter(m, c, x, lmax=lmax)
    dev = m.graph().dev
    assert y.shape == (20, 3, 2) and dev.calls == ["analysis"] and nn.last_path == "staged"
    (y * cot).sum().backward()
    assert dev.calls == ["analysis", "laplacian_grad", "synthesis", "cross_moments"] and dev.pair_counts == [w0.size]
    ref = weights_grad_direct(W, "combinatorial", lmax, c.detach().numpy(), x.detach().numpy(),
                              np.ascontiguousarray(cot.numpy().transpose(2, 0, 1)), pairs)
    assert m.weight.grad.shape == (w0.size,) and m.weight.grad.dtype == torch.float64
    assert rel_err(m.weight.grad.numpy(), ref) < 1e-13 and np.abs(ref[w0 == 0]).max() > 0  # (weight 0: a gradient too)
    m.weight.requires_grad_(False)
    dev.calls.clear()
    (nn.cheby_filter(m, c, x, lmax=lmax) * cot).sum().backward()
    assert dev.calls == ["analysis", "synthesis", "cross_moments"]
    # a plain graph goes the way it always went
    plain = m.graph()
    plain.dev.calls.clear()
    nn.cheby_filter(plain, c, x, lmax=lmax).sum().backward()
    assert plain.dev.calls == ["analysis", "synthesis", "cross_moments"]


# ---- the entry point ---------------------------------------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments_without_a_device():
    lib = _capi.load()
    c = np.ones((2, 5))
    fake, other = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)  # never dereferenced: the checks fail first
    idx = ctypes.c_void_p(1 << 22)

    def refused(rc, words):
        assert rc == _capi.ERR_INVALID
        with pytest.raises(ValueError):
            _capi.check(rc)
        assert words in _capi.last_error(), _capi.last_error()

    def grad(lmax=2.0, Nf=2, M=5, coeffs=c, nsig=4, n=3, src=idx, dst=idx):
        return lib.gspx_cheby_laplacian_grad_dev(None, lmax, Nf, M, _capi.ptr(coeffs) if coeffs is not None else None,
                                                 nsig, fake, other, n, src, dst, fake, other, None)

    refused(grad(), "null graph")
    refused(grad(src=None, dst=None), "null graph")
    for M in (1, 0, 257):
        refused(grad(M=M), "2 to 256")
    refused(grad(Nf=0), "Nf must be")
    refused(grad(nsig=-1), "negative number of signals")
    for lmax in (0.0, -1.0, float("nan"), float("inf")):
        refused(grad(lmax=lmax), "lmax must be positive")
    refused(grad(dst=None), "come together")
    refused(grad(src=None), "come together")
    refused(grad(n=-1), "vertex couples")
    refused(grad(coeffs=None), "null coefficients")
    bad = c.copy()
    bad[1, 2] = np.inf
    refused(grad(coeffs=bad), "non-finite coefficient")
    refused(grad(nsig=1 << 27), "too many signals")


def test_an_empty_pattern_asks_the_device_for_nothing(torch_nn):
    torch, nn = torch_nn
    W = random_graph(12, 3, seed=11)
    G = WgradGraph(W, upper_lmax(W))
    m = stand_in(nn, [])(G, np.zeros((2, 0), dtype=np.int64))
    c, x = torch.ones((1, 3), dtype=torch.float64), torch.ones((12, 2), dtype=torch.float64)
    y = nn.cheby_filter(m, c, x, lmax=1.0)
    y.sum().backward()
    assert m.graph().W.nnz == 0 and m.weight.grad.shape == (0,) and m.graph().dev.calls == ["analysis"]
