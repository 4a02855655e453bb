"""The process behind tests/test_gpu_y_wgrad_torch.py: nn.WeightedGraph and nn.cheby_filter with torch and libgspx on
the same GPU, torch loaded FIRST (what ``import pygsp_amd.nn`` is for), in float64.  Prints one JSON line and exits 0
when everything held; an assertion that fails ends the process with a traceback and a non-zero status.  Run by its test
only, in a fresh process."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import pygsp_amd.nn as nn  # noqa: E402 (imports torch before anything loads libgspx)
import numpy as np  # noqa: E402
import torch  # noqa: E402

LR, STEPS = 200.0, 3  # (the mean-square loss is of the order 1e-3: at this rate the dense restatement falls by a tenth a step)


def rel(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return float((a - b).abs().max() / b.abs().max())


def fit_problem():
    """(W, pattern (2, P), start weights, target weights, lmax, heat coefficients (1, M), signals): a graph, a copy with
    perturbed weights whose heat-filtered signals are the observations, and an lmax above every iterate's."""
    from gpu_helpers import random_graph, upper_lmax
    from pygsp_amd import filters
    from scipy import sparse
    W = random_graph(300, 6, seed=1)
    C = sparse.triu(W, format="coo")
    rng = np.random.default_rng(1)
    pairs, w0 = np.stack([C.row, C.col]), C.data.copy()
    target = w0 * (1.0 + 0.4 * rng.uniform(-1.0, 1.0, w0.size))
    lmax = 2.0 * upper_lmax(W)  # (twice the start's bound; main() checks it against every iterate's)

    class Scaled:  # what compute_cheby_coeff reads of a graph
        pass
    S = Scaled()
    S.lmax = lmax
    heat = filters.Heat(S, scale=4.0)
    c = filters._as_coeff_matrix(filters.compute_cheby_coeff(heat, m=12))
    return W, pairs, w0, target, lmax, c, rng.standard_normal((300, 6))


def dense_losses(W, pairs, w0, target, lmax, c, x):
    """The losses of STEPS projected SGD steps in dense CPU torch (wgrad_helpers.torch_filter_dense)."""
    from wgrad_helpers import torch_filter_dense
    N, ct, xt = W.shape[0], torch.from_numpy(c), torch.from_numpy(x)
    want = torch_filter_dense(torch, N, pairs, torch.from_numpy(target), "combinatorial", lmax, ct, xt)
    w = torch.from_numpy(w0.copy()).requires_grad_()
    losses = []
    for step in range(STEPS + 1):
        loss = ((torch_filter_dense(torch, N, pairs, w, "combinatorial", lmax, ct, xt) - want) ** 2).mean()
        losses.append(float(loss.detach()))
        if step < STEPS:
            (g,) = torch.autograd.grad(loss, w)
            with torch.no_grad():
                w -= LR * g
                w.clamp_(min=0)
    return losses, want.permute(1, 2, 0).contiguous()


def main():
    if not torch.cuda.is_available():
        print(json.dumps({"skip": "torch.cuda.is_available() is false in the child process"}))
        return 0
    from gpu_helpers import random_graph, upper_lmax
    from pygsp_amd import graphs
    from scipy import sparse
    from wgrad_helpers import torch_filter_dense

    # 1. forward and backward on GPU tensors against dense torch on the CPU with the weights as a leaf, for both
    # Laplacians, on a pattern of the graph's edges and twenty pairs that are none
    errs, paths = {}, set()
    for lap_type in ("combinatorial", "normalized"):
        W = random_graph(300, 6, seed=1)
        G = graphs.Graph(W, lap_type=lap_type, compute_dtype=np.float64)
        lmax = 1.5 * upper_lmax(W) if lap_type == "combinatorial" else 2.0
        C = sparse.triu(W, format="coo")
        rng = np.random.default_rng(2)
        more = [(s, t) for s, t in rng.integers(0, 300, (200, 2)).tolist() if s != t and W[s, t] == 0]
        more = sorted({(min(s, t), max(s, t)) for s, t in more})[:20]
        pairs = np.concatenate([np.stack([C.row, C.col]), np.array(more).T], axis=1)
        module = nn.WeightedGraph(G, pairs)
        gen = torch.Generator().manual_seed(0)
        c0 = torch.randn((2, 8), dtype=torch.float64, generator=gen) * 0.7 ** torch.arange(8, dtype=torch.float64)
        x0 = torch.randn((300, 5), dtype=torch.float64, generator=gen)
        cot = torch.randn((300, 5, 2), dtype=torch.float64, generator=gen)
        w_ref, c_ref, x_ref = (t.clone().requires_grad_() for t in (module.weight.detach(), c0, x0))
        y_ref = torch_filter_dense(torch, 300, pairs, w_ref, lap_type, lmax, c_ref, x_ref).permute(1, 2, 0)
        (y_ref * cot).sum().backward()
        c_gpu, x_gpu = c0.cuda().requires_grad_(), x0.cuda().requires_grad_()
        y = nn.cheby_filter(module, c_gpu, x_gpu, lmax=lmax)
        paths.add(nn.last_path)
        (y * cot.cuda()).sum().backward()
        paths.add(nn.last_path)
        errs[lap_type] = {"y": rel(y, y_ref), "weight_grad": rel(module.weight.grad, w_ref.grad),
                          "x_grad": rel(x_gpu.grad, x_ref.grad), "coeffs_grad": rel(c_gpu.grad, c_ref.grad)}
        assert module.weight.grad.shape == (pairs.shape[1],) and float(module.weight.grad[-20:].abs().max()) > 0
        assert all(e < 1e-10 for e in errs[lap_type].values()), errs
    assert len(paths) == 1, paths

    # 2. three projected SGD steps of a WeightedGraph towards the heat-filtered outputs of a perturbed copy of the graph;
    # the learning rate is one at which the dense CPU restatement falls too, checked first
    W, pairs, w0, target, lmax, c, x = fit_problem()
    dense, want = dense_losses(W, pairs, w0, target, lmax, c, x)
    assert all(b < a for a, b in zip(dense, dense[1:])), dense
    G = graphs.Graph(W, compute_dtype=np.float64)
    module = nn.WeightedGraph(G)
    assert np.array_equal(module.pairs, pairs) and np.array_equal(module.weight.detach().numpy(), w0)
    ct, xt, want = torch.from_numpy(c), torch.from_numpy(x).cuda(), want.cuda()
    losses = []
    for step in range(STEPS + 1):
        assert upper_lmax(module.graph().W) <= lmax
        loss = ((nn.cheby_filter(module, ct, xt, lmax=lmax) - want) ** 2).mean()
        losses.append(float(loss.detach()))
        if step < STEPS:
            module.weight.grad = None
            loss.backward()
            with torch.no_grad():
                module.weight -= LR * module.weight.grad
                module.weight.clamp_(min=0)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert max(abs(a - b) / b for a, b in zip(losses, dense)) < 1e-9, (losses, dense)

    print(json.dumps({"path": paths.pop(), "errors": errs, "losses": losses, "dense_losses": dense,
                      "torch": torch.__version__}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
