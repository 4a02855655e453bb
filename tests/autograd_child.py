"""The process behind tests/test_gpu_v_autograd.py: torch and libgspx on the same GPU, torch loaded FIRST (what
``import pygsp_amd.nn`` is for), in float64.  Prints one JSON line and exits 0 when everything held; an assertion that
fails ends the process with a traceback and a non-zero status.  Run by its test only, in a fresh process."""
import ctypes
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


def dense_filter(L, lmax, coeffs, x):
    """The same polynomial in dense torch ops: (N, Nsig, Nf)."""
    a = lmax / 2.0
    Lt = (L - a * torch.eye(L.shape[0], dtype=L.dtype)) / a
    T = [x, Lt @ x]
    for _ in range(2, coeffs.shape[1]):
        T.append(2.0 * (Lt @ T[-1]) - T[-2])
    return torch.stack([0.5 * c[0] * T[0] + sum(c[k] * T[k] for k in range(1, len(T))) for c in coeffs], dim=2)


def main():
    if not torch.cuda.is_available():
        print(json.dumps({"skip": "torch.cuda.is_available() is false in the child process"}))
        return 0
    from gpu_helpers import random_graph, upper_lmax
    from oracle import cheby_oracle as orc
    from pygsp_amd import _capi, filters, graphs

    W = random_graph(300, 6, seed=1, isolated=1)
    G = graphs.Graph(W, compute_dtype=np.float64)
    G._lmax = upper_lmax(W)
    lib = _capi.load()

    # 1. the gate: a tensor of torch's is device memory of GPU 0 to libgspx's runtime; host memory is refused
    t = torch.empty(1024, dtype=torch.float64, device="cuda:0")
    found = nn.ptr_device(t.data_ptr())
    host, dev = np.zeros(16), ctypes.c_int(5)
    rc = lib.gspx_ptr_device(_capi.ptr(host), ctypes.byref(dev))
    assert rc == _capi.ERR_INVALID and dev.value == -1, (rc, dev.value)
    assert found == 0, "libgspx's HIP runtime does not know torch's tensor: {!r} ({})".format(found, _capi.last_error())

    # 2. forward and backward on GPU tensors against dense torch ops on the CPU
    gen = torch.Generator().manual_seed(0)
    c0 = torch.randn((2, 8), dtype=torch.float64, generator=gen) * 0.7 ** torch.arange(8, dtype=torch.float64)
    x0 = torch.randn((300, 5), dtype=torch.float64, generator=gen)
    w = torch.randn((300, 5, 2), dtype=torch.float64, generator=gen)
    c_ref, x_ref = c0.clone().requires_grad_(), x0.clone().requires_grad_()
    y_ref = dense_filter(torch.from_numpy(orc.laplacian(W).toarray()), G.lmax, c_ref, x_ref)
    (y_ref * w).sum().backward()
    c_gpu, x_gpu = c0.cuda().requires_grad_(), x0.cuda().requires_grad_()
    y = nn.cheby_filter(G, c_gpu, x_gpu)
    forward_path = nn.last_path
    (y * w.cuda()).sum().backward()
    backward_path = nn.last_path
    errs = {"y": rel(y, y_ref), "x_grad": rel(x_gpu.grad, x_ref.grad), "coeffs_grad": rel(c_gpu.grad, c_ref.grad)}
    assert y.shape == (300, 5, 2) and y.is_cuda and x_gpu.grad.is_cuda and c_gpu.grad.is_cuda
    assert all(e < 1e-10 for e in errs.values()), errs
    assert forward_path == backward_path, (forward_path, backward_path)

    # 3. three SGD steps of a ChebyshevFilter towards a heat kernel: the loss falls every step
    target = nn.ChebyshevFilter(G, 1, order=7, init=filters.Heat(G, scale=10)).cuda()
    with torch.no_grad():
        want = target(x_gpu.detach())
    layer = nn.ChebyshevFilter(G, 1, order=7).cuda()
    opt = torch.optim.SGD(layer.parameters(), lr=0.05)
    losses = []
    for step in range(4):
        opt.zero_grad()
        loss = ((layer(x_gpu.detach()) - want) ** 2).mean()
        losses.append(float(loss.detach()))
        if step < 3:
            loss.backward()
            opt.step()
    assert all(b < a for a, b in zip(losses, losses[1:])), losses

    # 4. the record: the path taken, the versions, and every HIP runtime file mapped into this process (one, if the
    # import order did its work)
    with open("/proc/self/maps") as maps:
        runtimes = sorted({line.split()[-1] for line in maps if "libamdhip64" in line})
    print(json.dumps({"path": forward_path, "ptr_found": found == 0, "errors": errs, "losses": losses,
                      "torch": torch.__version__, "torch_hip": torch.version.hip, "hip_runtimes": runtimes,
                      "gspx": lib.gspx_version().decode()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
