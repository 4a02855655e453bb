"""k_lz_combine<FB> and the projection V^T x of the Lanczos entry points at the shapes where they change behaviour
(gspx_lanczos_combine_dev / gspx_lanczos_krylov_dev, gspx_lanczos.hip.h).

The combine runs on SYNTHETIC stacks and weights - random numbers in a pool buffer, not a Krylov basis - through
pygsp_amd.lanczos.DeviceBackend.combine, against a longdouble einsum within (order + 1) eps (|w| . |V|): every build
(FB = 1, 2, 4, 8), partial groups fb < FB, two and three workgroup groups with a ragged last one (Nf 9, 16, 17), fewer
rows than one workgroup takes (N 1, 3), the two-rows-per-thread tail on and off, ldp 1 ... 256, with and without a
vertex permutation, full width and into a column window of a wider y whose other entries must keep their sentinel.
The projection is DeviceBackend.krylov's proj against sum_i V[j, i, c] x[perm[i], c] of the stack it returns, within
(N + 2) eps (|V|^T |x|), with exact zeros where a column never started or stopped.  filters.lanczos_op then runs banks
of 2, 3, 4, 9 and 17 filters end to end against the numpy backend."""
import numpy as np
import pytest
from scipy import sparse

from gpu_helpers import ctx, random_graph  # noqa: F401 (ctx: fixture)
from lanczos_helpers import laplacian, rel_err, run_numpy
from operator_pins_helpers import (LD, caller_rows, combine_reference, path_graph, projection_reference,
                                   shuffled_order)
from pygsp_amd import engine, filters, graphs, lanczos

pytestmark = pytest.mark.gpu

SENTINEL = -1.2345e300
WIDTHS = [1, 3, 17, 64, 65, 256]
ORDERS = [1, 8, 20]
_DEVS, _STACKS, _WORST = {}, {}, {}


def small_w(N):
    if N == 1:
        return sparse.csr_matrix((1, 1))
    if N == 3:
        return path_graph(3)
    return random_graph(N, 4, seed=N)  # (70 and 257: the graphs of test_shared_thread_map_at_small_n)


def device(ctx, N, permuted):
    """One float64 device graph per (N, permuted), for the module."""
    key = (N, permuted)
    if key not in _DEVS:
        perm = shuffled_order(np.random.default_rng(7 * N + 1), N) if permuted else None
        _DEVS[key] = engine.DeviceGraph.from_w(small_w(N), dtype=np.float64, perm=perm, ctx=ctx)
    return _DEVS[key]


def stack(N, n, order):
    """A synthetic (order, N, n) stack in the internal order, shared by every bank size and both vertex orders."""
    key = (N, n, order)
    if key not in _STACKS:
        V = np.random.default_rng(100_000 * order + 300 * N + n).standard_normal((order, N, n))
        V.setflags(write=False)
        _STACKS[key] = V
    return _STACKS[key]


def note(test, err, where):
    if err >= _WORST.get(test, (-1.0, None))[0]:
        _WORST[test] = (err, where)


def teardown_module(module):
    for test, (err, where) in sorted(_WORST.items()):
        print("\nworst {:<28s} float64  {:.3f} of the bound at {}".format(test, err, where), end="")
    print()
    _WORST.clear()
    _STACKS.clear()
    while _DEVS:
        _DEVS.popitem()[1].destroy()


@pytest.mark.parametrize("N", [1, 3, 70, 257])
@pytest.mark.parametrize("Nf", [1, 2, 3, 4, 5, 8, 9, 16, 17])
def test_combine_on_synthetic_stacks(ctx, Nf, N):
    """Builds launched: Nf 1 -> k_lz_combine<1>, 2 -> <2>, 3 and 4 -> <4>, 5 and 8 -> <8> in one group, 9 and 16 -> <8>
    in two groups (a last group of one filter at 9), 17 -> <8> in three groups with a last group of one."""
    rng = np.random.default_rng(1000 * Nf + N)
    for n in WIDTHS:
        for order in ORDERS:
            V = stack(N, n, order)
            w = rng.standard_normal((Nf, order, n))
            ref, bound = combine_reference(V, w)
            buf = ctx.take(order * N * n * 8)
            buf.upload(V)
            try:
                for permuted in (True, False):
                    dev = device(ctx, N, permuted)
                    perm = dev.download_perm()
                    assert (perm is not None) == (permuted and N > 1)  # (one vertex: the identity, dropped)
                    be = lanczos.DeviceBackend(dev)
                    want, lim = caller_rows(ref, perm, 1), caller_rows(bound, perm, 1)
                    # full width, then a window [c0, c0 + n) of a wider y: c0 odd and even
                    for c0, ldy in ((0, n), (1, n + 3), (2, n + 2)):
                        host = np.full((Nf * N, ldy), SENTINEL)
                        y = ctx.upload(host)
                        try:
                            be.combine((buf, order, n), w, (y.ptr, ldy), c0, c0 + n)
                            got = y.download(host.shape, np.float64)
                            be.combine((buf, order, n), w, (y.ptr, ldy), c0, c0 + n)
                            again = y.download(host.shape, np.float64)
                        finally:
                            y.free()
                        where = (Nf, N, n, order, permuted, c0, ldy)
                        assert got.tobytes() == again.tobytes(), where
                        outside = np.ones(ldy, dtype=bool)
                        outside[c0:c0 + n] = False
                        assert np.all(got[:, outside] == SENTINEL), where
                        view = got[:, c0:c0 + n].reshape(Nf, N, n)
                        assert np.all(np.isfinite(view)), where
                        err = np.abs(view.astype(LD) - want)
                        assert np.all(err <= lim), (where, float(np.max(err - lim)))
                        note("combine", float(np.max(err[lim > 0] / lim[lim > 0])), where)
            finally:
                ctx.give(buf)


@pytest.mark.parametrize("order", [8, 20])
@pytest.mark.parametrize("width", [1, 17, 65, 256])
@pytest.mark.parametrize("N", [70, 257])
def test_projection_of_the_krylov_call(ctx, N, width, order):
    """proj = V^T x (the last k_lz_dots launch, alpha == nullptr) against the stack the same call returns; order 20
    at width 256 crosses the 4096 entries at which sum_parts switches kernels.  Column 1 is zero (never starts) and
    column 2 constant (L 1 = 0: it stops after its first vector) where the width allows."""
    W = small_w(N)
    rng = np.random.default_rng(1000 * N + 10 * width + order)
    x = rng.standard_normal((N, width))
    if width > 2:
        x[:, 1] = 0
        x[:, 2] = 1.5
    thr = lanczos.breakdown_threshold(2.0 * float(np.ravel(W.sum(axis=0)).max()))
    for permuted in (True, False):
        dev = device(ctx, N, permuted)
        perm = dev.download_perm()
        be = lanczos.DeviceBackend(dev)
        bx = ctx.upload(x)
        try:
            V, alpha, beta, proj, steps = be.krylov((bx.ptr, width), 0, width, order, thr)
            try:
                S = V[0].download((order, N, width), np.float64)
            finally:
                be.free(V)
            V2, _, _, proj2, steps2 = be.krylov((bx.ptr, width), 0, width, order, thr)
            be.free(V2)
        finally:
            bx.free()
        where = (N, width, order, permuted)
        assert proj.tobytes() == proj2.tobytes() and np.array_equal(steps, steps2), where
        xi = x if perm is None else x[perm]  # internal row i is the caller's row perm[i]
        ref, bound = projection_reference(S, xi)
        err = np.abs(proj.astype(LD) - ref)
        assert np.all(err <= bound), (where, float(np.max(err - bound)))
        live = bound > 0
        if live.any():
            note("projection", float(np.max(err[live] / bound[live])), where)
        assert np.all(steps >= 0) and np.all(steps <= order)
        if width > 2:
            assert steps[1] == 0 and steps[2] == 1, (where, steps[:3])
        assert np.all(steps[np.abs(x).sum(axis=0) > 0] >= 1), where
        for c in range(width):  # exact zeros beyond the Krylov dimension of every column
            assert not proj[steps[c]:, c].any() and not S[steps[c]:, :, c].any(), (where, c)
        first = np.flatnonzero(steps >= 1)  # q_0 = x / ||x||: proj[0] = ||x||
        assert rel_err(proj[0, first], np.linalg.norm(x[:, first], axis=0)) <= 1e-13, where


class _Scaled:
    """g(x) = a exp(-t x / lmax): one kernel of a hand-made Filter bank."""

    def __init__(self, a, t, lmax):
        self.a, self.t, self.lmax = a, t, lmax

    def __call__(self, x):
        return self.a * np.exp(-self.t * np.asarray(x) / self.lmax)


@pytest.mark.parametrize("N", [70, 257])
@pytest.mark.parametrize("Nf", [2, 3, 4, 9, 17])
def test_lanczos_op_bank_sizes_end_to_end(Nf, N):
    W = small_w(N)
    G = graphs.Graph(W, compute_dtype=np.float64)
    G.estimate_lmax("bounds")
    banks = [filters.MexicanHat(G, Nf=Nf),
             filters.Filter(G, [_Scaled(1.0 + 0.1 * i, 0.5 + 1.5 * i, G.lmax) for i in range(Nf)])]
    x = np.random.default_rng(N + Nf).standard_normal((N, 5))
    L = laplacian(W, "combinatorial")
    for f in banks:
        assert int(f.Nf) == Nf
        y = filters.lanczos_op(f, x, order=20)
        ref, _, _ = run_numpy(L, f, x, 20, G._get_upper_bound())
        assert y.shape == ref.shape == (Nf * N, 5)
        err = rel_err(y, ref)
        note("lanczos_op (of 1e-10)", err / 1e-10, (Nf, N, type(f).__name__))
        assert err <= 1e-10, (Nf, N, type(f).__name__, err)
        assert np.array_equal(y, filters.lanczos_op(f, x, order=20))
