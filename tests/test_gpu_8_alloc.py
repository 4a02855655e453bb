"""Allocator regression tests for the context workspaces (libgspx DevMem, pygsp_amd/csrc/gspx_mem.hip.h).

Round 1 ended red on hardware because a workspace of 32 MB and more - assembled from 2 MB physical
chunks through the HIP virtual-memory API - was re-grown by unmap / address-free / re-reserve / re-map
without synchronisation, and the next filter read stale translations (fuzz case 42: 4e-2 error in
fp64).  These tests walk exactly that life cycle, deterministically: first use, growth in place,
growth beyond the reservation, reuse at a smaller size, teardown and re-creation of the context, many
times over, with parity against the oracle (cheby_op, approximations.py:58-114) after every step.
Needs a real MI355X: `-m gpu`."""
import numpy as np
import pytest

from oracle import cheby_oracle as orc
from pygsp_amd import engine, graphs
from conftest import rel_err
from gpu_helpers import upper_lmax

pytestmark = pytest.mark.gpu

MB = 1 << 20


def _bank(lmax, nf, order):
    kernels = [orc.heat_kernel(15.0, lmax)] if nf == 1 else orc.mexican_hat_kernels(lmax, nf)
    return np.stack([orc.compute_cheby_coeff(k, lmax, order) for k in kernels])


def _check(dev, L, lmax, rng, nsig, order, nf, tol=1e-11):
    # one-shot host calls: the whole panel is one device batch, so the workspaces reach the sizes these tests are
    # about (the pipelined host path would cut the call into 16-column batches with megabyte-sized workspaces)
    dev.ctx.set_option("host_pipeline", 0)
    c = _bank(lmax, nf, order)
    x = rng.standard_normal((dev.N, nsig))
    y, _ = dev.cheby_filter(c, x, lmax)
    ref = orc.cheby_op(L, lmax, c, x).reshape(nf, dev.N, nsig)
    err = float(np.max(np.abs(y - ref)) / np.max(np.abs(ref)))
    assert err < tol, dict(nsig=nsig, order=order, nf=nf, err=err)


def test_deferred_workspace_grows_and_is_recreated():
    """Filterbank calls keep K+1 panels: 15586 x 16 fp64 = 2 MB per panel, so orders 20 / 43 / 59 ask
    for 42 / 88 / 120 MB - the sizes of the failing fuzz stream - on one context; then the context is
    destroyed and the sequence repeats on a new one (20 cycles)."""
    W, coords = graphs.sensor_weights(15586, k=7, seed=3)
    L = orc.laplacian(W, "normalized")
    rng = np.random.default_rng(0)
    for cycle in range(20):
        ctx = engine.Context(0)
        ctx.set_option("streamed_alloc", 1)  # (a second context on a device gets plain workspaces by default)
        dev = engine.DeviceGraph.from_w(W, "normalized", dtype=np.float64, perm=engine.locality_order(W, coords), ctx=ctx)
        try:
            for order in (20, 43, 12, 59, 43):  # first use, grow, smaller, grow again, reuse
                _check(dev, L, 2.0, rng, 16, order, 4)
            _check(dev, L, 2.0, rng, 16, 30, 1)  # the fused path on the same context
        finally:
            dev.destroy()
            ctx.close()


def test_fused_workspace_growth_beyond_reservation():
    """Single-filter calls use two T_k panels + one accumulator panel.  130k x {32, 64, 130, 64} fp64
    signals: 67 -> 133 -> 270 MB of slots, i.e. growth inside the first reservation and then past it
    (a reservation is max(2 x request, 1 GiB) only when the request is small: the 600 MB request of
    the last graph below forces a second reservation on the same context)."""
    ctx = engine.Context(0)
    ctx.set_option("streamed_alloc", 1)
    rng = np.random.default_rng(1)
    try:
        W, coords = graphs.sensor_weights(130000, k=8, seed=11)
        L = orc.laplacian(W)
        lmax = upper_lmax(W)
        dev = engine.DeviceGraph.from_w(W, dtype=np.float64, perm=engine.locality_order(W, coords), ctx=ctx)
        dev.build_gather_tiles()
        for nsig in (32, 64, 130, 64, 16):
            _check(dev, L, lmax, rng, nsig, 9, 1)
        dev.destroy()
        # a larger graph on the same context: 450k x 168 fp64 = 605 MB per panel, 1.2 GB of slots
        W, coords = graphs.sensor_weights(450000, k=8, seed=12)
        L = orc.laplacian(W)
        lmax = upper_lmax(W)
        dev = engine.DeviceGraph.from_w(W, dtype=np.float64, perm=engine.locality_order(W, coords), ctx=ctx)
        dev.build_gather_tiles()
        c = _bank(lmax, 1, 6)
        x = rng.standard_normal((dev.N, 168))
        ctx.set_option("host_pipeline", 0)
        y, _ = dev.cheby_filter(c, x, lmax)
        cols = [0, 77, 167]
        ref = orc.cheby_op(L, lmax, c, x[:, cols]).reshape(dev.N, len(cols))
        assert np.max(np.abs(y[0][:, cols] - ref)) / np.max(np.abs(ref)) < 1e-11
        # back to a small request on the grown workspace
        _check(dev, L, lmax, rng, 8, 5, 1)
        dev.destroy()
    finally:
        ctx.close()


def test_two_contexts_interleaved():
    """Two live contexts with chunk-mapped workspaces, growing alternately."""
    W, coords = graphs.sensor_weights(60000, k=6, seed=5)
    L = orc.laplacian(W)
    lmax = upper_lmax(W)
    rng = np.random.default_rng(2)
    ctxs = [engine.Context(0), engine.Context(0)]
    # (a further context on a device that already has one gets plain workspaces by default - no retired address
    # space per tenant; this test is about the chunked mode, so it asks for it)
    assert [c.get_option("streamed_alloc") for c in ctxs][1] == 0
    for c in ctxs:
        c.set_option("streamed_alloc", 1)
    devs = [engine.DeviceGraph.from_w(W, dtype=np.float64, ctx=c) for c in ctxs]
    try:
        for nsig in (70, 100, 140, 200):  # 34 .. 96 MB panels
            for dev in devs:
                _check(dev, L, lmax, rng, nsig, 7, 1)
    finally:
        for dev in devs:
            dev.destroy()
        for c in ctxs:
            c.close()


def test_plain_allocation_switch_and_retired_address_space():
    """The safe mode of the workspaces: option "streamed_alloc" = 0 - or GSPX_STREAMED_ALLOC=0
    before the context exists - makes them plain hipMalloc allocations; switching it off on a live context
    drops a chunk-mapped workspace; results are the same either way; "retired_va_mb" counts the address space
    the chunked mode has retired in this process."""
    import os
    W, coords = graphs.sensor_weights(60000, k=6, seed=6)
    L = orc.laplacian(W)
    lmax = upper_lmax(W)
    rng = np.random.default_rng(4)
    ctx = engine.Context(0)
    # the process-wide default context of this device exists already (other tests): a further context starts plain
    assert ctx.get_option("streamed_alloc") == (0 if engine._default_ctx.get(0) is not None else 1)
    ctx.set_option("streamed_alloc", 1)
    dev = engine.DeviceGraph.from_w(W, dtype=np.float64, ctx=ctx)
    try:
        assert ctx.get_option("streamed_alloc") == 1
        before = ctx.get_option("retired_va_mb")
        _check(dev, L, lmax, rng, 100, 7, 1)  # 48 MB panels: chunk-mapped
        ctx.set_option("streamed_alloc", 0)  # drops (retires) the mapped ranges
        assert ctx.get_option("retired_va_mb") >= before + 2048  # two ranges of at least 1 GiB each
        mid = ctx.get_option("retired_va_mb")
        for nsig in (100, 200, 64):
            _check(dev, L, lmax, rng, nsig, 7, 1)
        assert ctx.get_option("retired_va_mb") == mid  # plain allocations retire nothing, also when they grow
        ctx.set_option("streamed_alloc", 1)
        _check(dev, L, lmax, rng, 100, 7, 1)
    finally:
        dev.destroy()
        ctx.close()
    os.environ["GSPX_STREAMED_ALLOC"] = "0"
    try:
        ctx = engine.Context(0)
        assert ctx.get_option("streamed_alloc") == 0
        dev = engine.DeviceGraph.from_w(W, dtype=np.float64, ctx=ctx)
        mid = ctx.get_option("retired_va_mb")
        _check(dev, L, lmax, rng, 150, 7, 1)
        dev.destroy()
        ctx.close()
        assert engine.default_context(0).get_option("retired_va_mb") == mid
    finally:
        del os.environ["GSPX_STREAMED_ALLOC"]
    # several contexts on one device (a multi-tenant process): the first owns the chunked mode, the others start
    # plain - unless the environment says 1
    engine.default_context(0)
    extra = engine.Context(0)
    assert extra.get_option("streamed_alloc") == 0
    extra.close()
    os.environ["GSPX_STREAMED_ALLOC"] = "1"
    try:
        extra = engine.Context(0)
        assert extra.get_option("streamed_alloc") == 1
        extra.close()
    finally:
        del os.environ["GSPX_STREAMED_ALLOC"]


def test_staged_copies_of_large_buffers():
    """gspx_buf_download from 32 MB on (and gspx_buf_upload with option staged_copy = 2) goes through pinned 16 MB chunks
    drained / filled by host threads while the DMA engine ships the next ones: the same bytes as the plain pageable
    copy, sizes that are not a multiple of the chunk (or of anything), several thread counts; smaller buffers keep the
    plain copy.  (Downloads into fresh memory: 46 against 11.7 GB/s; uploads: the runtime's own staging is as fast.)"""
    import time
    ctx = engine.Context(0)
    rng = np.random.default_rng(9)
    try:
        for nbytes in (16 << 20, (32 << 20) + 1, (100 << 20) + 12345, 3 * (16 << 20)):
            src = rng.integers(0, 256, nbytes, dtype=np.uint8)
            for threads in (0, 1, 3):
                ctx.set_option("copy_threads", threads)
                ctx.set_option("staged_copy", 2)  # both directions staged
                buf = ctx.alloc(nbytes)
                buf.upload(src)
                back = buf.download((nbytes,), np.uint8)
                assert np.array_equal(back, src), (nbytes, threads)
                ctx.set_option("staged_copy", 0)  # the plain copy sees what the staged one wrote, and the other way round
                assert np.array_equal(buf.download((nbytes,), np.uint8), src)
                buf.upload(src[::-1].copy())
                ctx.set_option("staged_copy", 2)
                assert np.array_equal(buf.download((nbytes,), np.uint8), src[::-1])
                buf.free()
        ctx.set_option("copy_threads", 0)
        # a device-resident array of 256 MB: to_device / np.asarray ride on it
        x = rng.standard_normal((1 << 20, 32))
        rates = {}
        for mode in (2, 0):
            ctx.set_option("staged_copy", mode)
            buf = ctx.alloc(x.nbytes)
            buf.upload(x)
            t0 = time.perf_counter()
            buf.upload(x)
            t1 = time.perf_counter()
            y = buf.download(x.shape, np.float64)
            t2 = time.perf_counter()
            assert np.array_equal(x, y)
            rates[mode] = (x.nbytes / (t1 - t0) / 1e9, x.nbytes / (t2 - t1) / 1e9)
            buf.free()
        print("GB/s (upload, download): staged {} plain {}".format(rates[2], rates[0]))
    finally:
        ctx.close()


def test_placement_tuning_keeps_the_fastest_backing_and_the_same_bits():
    """gspx_ctx_tune_placement (round 6): several physical backings of the streamed workspaces are drawn, timed with a
    short call and the fastest kept.  The result of a filter call is bit-identical before and after (only WHERE the
    work panels lie changes), the reported candidate kept is the fastest, the context stays usable (growth, other
    widths, another tuning), and bad arguments are refused."""
    ctx = engine.Context(0)
    try:
        G = graphs.Sensor(200000, k=8, seed=5, ctx=ctx)
        G.estimate_lmax("bounds")
        dev = G.device_graph()
        x = np.random.default_rng(3).standard_normal((G.N, 64))
        c = orc.compute_cheby_coeff(orc.heat_kernel(20, G.lmax), G.lmax, 30)
        y0, _ = dev.cheby_filter(c, x, G.lmax)
        bx, by = ctx.upload(x), ctx.alloc(x.nbytes)
        rep = dev.tune_placement(c, bx.ptr, by.ptr, 64, G.lmax, candidates=5)
        assert np.array_equal(by.download(x.shape, np.float64), y0[0])  # the tuned call's own result
        assert len(rep["launch_ms"]) == 5 and all(v > 0 for v in rep["launch_ms"])
        assert rep["launch_ms"][rep["kept"]] == min(rep["launch_ms"])
        y1, _ = dev.cheby_filter(c, x, G.lmax)
        assert np.array_equal(y0, y1)
        ref = orc.cheby_op(orc.laplacian(G.W), G.lmax, c, x[:, :2])
        assert rel_err(y1[0][:, :2], ref) < 1e-11
        # wider than tuned for (the workspaces grow), narrower, a bank, then tuning again for another width
        x2 = np.random.default_rng(4).standard_normal((G.N, 96))
        y2, _ = dev.cheby_filter(c, x2, G.lmax)
        assert rel_err(y2[0][:, :2], orc.cheby_op(orc.laplacian(G.W), G.lmax, c, x2[:, :2])) < 1e-11
        rep2 = dev.tune_placement(c, bx.ptr, by.ptr, 32, G.lmax, candidates=2)
        assert rep2["kept"] in (0, 1)
        # a strided search: a held pad between the draws (candidates that no longer fit would read 0)
        rep2 = dev.tune_placement(c, bx.ptr, by.ptr, 64, G.lmax, candidates=3, stride_mb=512)
        assert rep2["kept"] in (0, 1, 2) and all(v > 0 for v in rep2["launch_ms"])
        with pytest.raises(ValueError):
            dev.tune_placement(c, bx.ptr, by.ptr, 64, G.lmax, candidates=2, stride_mb=-1)
        y3, _ = dev.cheby_filter(c, x, G.lmax)
        assert np.array_equal(y0, y3)
        with pytest.raises(ValueError):
            dev.tune_placement(c, bx.ptr, by.ptr, 64, G.lmax, candidates=0)
        with pytest.raises(TypeError):
            dev.tune_placement(c[:1], bx.ptr, by.ptr, 64, G.lmax, candidates=2)
        bx.free()
        by.free()
        # the one-liner of the drop-in layer: scratch panels, the bank's own coefficients
        from pygsp_amd import filters
        rep3 = filters.Heat(G, 20).tune_placement(64, order=30, candidates=2)
        assert len(rep3["launch_ms"]) == 2 and rep3["kept"] in (0, 1)
        with pytest.raises(ValueError, match="single-filter"):
            filters.MexicanHat(G, Nf=3).tune_placement(64)
        y4, _ = dev.cheby_filter(c, x, G.lmax)
        assert np.array_equal(y0, y4)
        dev.destroy()
    finally:
        ctx.close()
