"""The process behind the torch test of tests/test_gpu_z_coarsen.py: torch and libgspx on the same GPU, torch loaded
FIRST (what ``import pygsp_amd.nn`` is for), in float64.  Prints one JSON line and exits 0 when everything held; an
assertion that fails ends the process with a traceback and a non-zero status.  Run by its test only, in a fresh
process."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import pygsp_amd.nn as nn  # noqa: E402 (imports torch before anything loads libgspx)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def rel(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return float((a - b).abs().max() / b.abs().max())


def torch_pool(parent, n_coarse, x, mode):
    """The same pooling composed from torch.index_select and amax / sum over a padded (cluster, member) table."""
    parent = np.asarray(parent)
    order = np.argsort(parent, kind="stable")
    sizes = np.bincount(parent, minlength=n_coarse)
    start = np.r_[0, np.cumsum(sizes)[:-1]]
    width = int(sizes.max())
    slot = np.minimum(np.arange(width)[None, :], sizes[:, None] - 1)  # short clusters repeat their last member
    table = torch.from_numpy(order[start[:, None] + slot].reshape(-1)).to(x.device)
    members = torch.index_select(x, 0, table).reshape((n_coarse, width) + tuple(x.shape[1:]))
    if mode == "max":
        return members.amax(dim=1)
    live = torch.from_numpy((np.arange(width)[None, :] < sizes[:, None])).to(x.device, x.dtype)
    total = (members * live.reshape(live.shape + (1,) * (x.dim() - 1))).sum(dim=1)
    if mode == "sum":
        return total
    return total / torch.from_numpy(sizes).to(x.device, x.dtype).reshape((-1,) + (1,) * (x.dim() - 1))


def main():
    if not torch.cuda.is_available():
        print(json.dumps({"skip": "torch.cuda.is_available() is false in the child process"}))
        return 0
    from gpu_helpers import random_graph, upper_lmax
    from pygsp_amd import graphs, reduction

    gen = torch.Generator().manual_seed(0)
    paths, checks, same, network = {}, {}, {}, {}

    # 1. gradcheck on a 40-vertex graph, F = 3, B = 2, one and two levels; max on distinct values
    G40 = graphs.Graph(random_graph(40, 4, seed=2), compute_dtype=np.float64)
    C40 = reduction.coarsen(G40, levels=2)
    distinct = torch.randperm(40 * 2 * 3, generator=gen).to(torch.float64).reshape(40, 2, 3) / 7.0
    for mode in ("mean", "sum", "max"):
        for hi in (1, 2):
            x = (distinct if mode == "max" else torch.randn((40, 2, 3), dtype=torch.float64, generator=gen))
            x = x.cuda().requires_grad_()
            checks["%s_%d" % (mode, hi)] = bool(torch.autograd.gradcheck(
                lambda t: nn.graph_pool(C40, t, 0, hi, mode), (x,), eps=1e-6, atol=1e-7, rtol=1e-7))
            paths["gradcheck_%s_%d" % (mode, hi)] = nn.last_path
    y = torch.randn((C40.graphs[2].N, 2, 3), dtype=torch.float64, generator=gen).cuda().requires_grad_()
    checks["unpool"] = bool(torch.autograd.gradcheck(lambda t: nn.graph_unpool(C40, t, 0, 2), (y,), eps=1e-6,
                                                      atol=1e-7, rtol=1e-7))
    paths["gradcheck_unpool"] = nn.last_path

    # 2. GPU tensors by pointer, CPU tensors through host arrays: equal values, forward and backward, both dtypes
    for dtype in (torch.float64, torch.float32):
        for mode in ("max", "mean", "sum"):
            x0 = torch.randn((40, 5), dtype=dtype, generator=gen)
            w = torch.randn((C40.graphs[2].N, 5), dtype=dtype, generator=gen)
            xg, xc = x0.cuda().requires_grad_(), x0.clone().requires_grad_()
            yg = nn.graph_pool(C40, xg, mode=mode)
            paths["forward_%s_%s" % (mode, dtype)] = nn.last_path
            (yg * w.cuda()).sum().backward()
            paths["backward_%s_%s" % (mode, dtype)] = nn.last_path
            yc = nn.graph_pool(C40, xc, mode=mode)
            assert nn.last_path == "staged" and not yc.is_cuda and yg.is_cuda and yg.dtype == dtype
            (yc * w).sum().backward()
            assert yg.shape == (C40.graphs[2].N, 5) and xg.grad.is_cuda
            same["y_%s_%s" % (mode, dtype)] = float((yg.detach().cpu() - yc.detach()).abs().max())
            same["grad_%s_%s" % (mode, dtype)] = float((xg.grad.cpu() - xc.grad).abs().max())
            ref = torch_pool(C40.parent(0, 2), C40.graphs[2].N, x0, mode)
            assert rel(yc, ref) < (1e-14 if dtype == torch.float64 else 1e-6), (mode, dtype)

    # 3. ChebConv -> GraphPool -> ChebConv, forward and backward, against the same network with the pooling composed
    # from torch.index_select and amax
    W = random_graph(300, 6, seed=1, isolated=1)
    G = graphs.Graph(W, compute_dtype=np.float64)
    G._lmax = upper_lmax(W)
    C = reduction.coarsen(G, levels=2)
    G2 = C.graphs[2]
    G2._lmax = upper_lmax(G2.W)
    torch.manual_seed(3)
    conv1, conv2 = nn.ChebConv(G, 4, 6, order=3).cuda(), nn.ChebConv(G2, 6, 2, order=3).cuda()
    pool = nn.GraphPool(C, 0, 2, mode="max")
    x = torch.randn((300, 2, 4), dtype=torch.float64, generator=gen).cuda()
    w = torch.randn((G2.N, 2, 2), dtype=torch.float64, generator=gen).cuda()
    params = list(conv1.parameters()) + list(conv2.parameters())
    grads = []
    for composed in (False, True):
        for p in params:
            p.grad = None
        h = torch.tanh(conv1(x))  # (no ties: amax splits a tied maximum's gradient, the layer gives it to the first)
        h = torch_pool(C.parent(0, 2), G2.N, h, "max") if composed else pool(h)
        if not composed:
            paths["network_pool"] = nn.last_path
        out = conv2(h)
        (out * w).sum().backward()
        grads.append([out.detach().clone()] + [p.grad.detach().clone() for p in params])
    assert grads[0][0].shape == (G2.N, 2, 2) and len(params) == 4
    for k, (a, b) in enumerate(zip(*grads)):
        assert torch.isfinite(a).all() and a.is_cuda
        network["output" if k == 0 else "param_%d" % (k - 1)] = rel(a, b)
    assert "GraphPool" in repr(pool) and "mode=max" in repr(pool) and "lo=0" in repr(nn.GraphUnpool(C, 0, 1))

    print(json.dumps({"paths": paths, "gradcheck": checks, "cpu_equals_gpu": same, "network": network,
                      "torch": torch.__version__}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
