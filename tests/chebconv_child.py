"""The process behind tests/test_gpu_w_chebconv_torch.py: torch and libgspx on the same GPU, torch loaded FIRST (what
``import pygsp_amd.nn`` is for), in float64.  Prints one JSON line and exits 0 when everything held; an assertion that
fails ends the process with a traceback and a non-zero status.  Run by its test only, in a fresh process."""
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


def dense_conv(L, lmax, theta, x):
    """The same layer in dense torch ops: x (N, B, Fin) -> (N, B, Fout), a plain sum over the orders."""
    a = lmax / 2.0
    Lt = (L - a * torch.eye(L.shape[0], dtype=L.dtype)) / a
    T = [x, torch.einsum("nm,mbi->nbi", Lt, x)]
    for _ in range(2, theta.shape[0]):
        T.append(2.0 * torch.einsum("nm,mbi->nbi", Lt, T[-1]) - T[-2])
    return sum(torch.einsum("nbi,io->nbo", T[k], theta[k]) for k in range(theta.shape[0]))


def main():
    if not torch.cuda.is_available():
        print(json.dumps({"skip": "torch.cuda.is_available() is false in the child process"}))
        return 0
    from gpu_helpers import random_graph, upper_lmax
    from oracle import cheby_oracle as orc
    from pygsp_amd import _capi, graphs

    W = random_graph(300, 6, seed=1, isolated=1)
    G = graphs.Graph(W, compute_dtype=np.float64)
    G._lmax = upper_lmax(W)
    found = nn.ptr_device(torch.empty(1024, dtype=torch.float64, device="cuda:0").data_ptr())

    # 1. forward and backward on GPU tensors against dense torch ops on the CPU
    gen = torch.Generator().manual_seed(0)
    t0 = torch.randn((8, 5, 3), dtype=torch.float64, generator=gen) / 5 ** 0.5
    x0 = torch.randn((300, 2, 5), dtype=torch.float64, generator=gen)
    w = torch.randn((300, 2, 3), dtype=torch.float64, generator=gen)
    t_ref, x_ref = t0.clone().requires_grad_(), x0.clone().requires_grad_()
    y_ref = dense_conv(torch.from_numpy(orc.laplacian(W).toarray()), G.lmax, t_ref, x_ref)
    (y_ref * w).sum().backward()
    t_gpu, x_gpu = t0.cuda().requires_grad_(), x0.cuda().requires_grad_()
    y = nn.cheby_conv(G, t_gpu, x_gpu)
    forward_path = nn.last_path
    (y * w.cuda()).sum().backward()
    backward_path = nn.last_path
    errs = {"y": rel(y, y_ref), "x_grad": rel(x_gpu.grad, x_ref.grad), "theta_grad": rel(t_gpu.grad, t_ref.grad)}
    assert y.shape == (300, 2, 3) and y.is_cuda and x_gpu.grad.is_cuda and t_gpu.grad.is_cuda
    assert all(e < 1e-10 for e in errs.values()), errs
    assert forward_path == backward_path, (forward_path, backward_path)

    # 2. three SGD steps of a ChebConv towards a fixed random target layer: the loss falls every step
    torch.manual_seed(1)
    target = nn.ChebConv(G, 5, 3, order=4).cuda()
    with torch.no_grad():
        want = target(x_gpu.detach())
    layer = nn.ChebConv(G, 5, 3, order=4).cuda()
    opt = torch.optim.SGD(layer.parameters(), lr=0.05)
    losses = []
    for step in range(4):
        opt.zero_grad()
        out = layer(x_gpu.detach())
        loss = ((out - want) ** 2).mean()
        losses.append(float(loss.detach()))
        if step < 3:
            loss.backward()
            opt.step()
    assert out.shape == (300, 2, 3) and out.dtype == torch.float64 and out.is_cuda
    assert all(b < a for a, b in zip(losses, losses[1:])), losses

    print(json.dumps({"path": forward_path, "ptr_found": found == 0, "errors": errs, "losses": losses,
                      "torch": torch.__version__, "gspx": _capi.load().gspx_version().decode()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
