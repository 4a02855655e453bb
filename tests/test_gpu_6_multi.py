"""the path's one collective.  gspx_gather across contexts in one process (peer copies and
the RCCL form), the one-process-per-GPU communicator (gspx_comm_*: RCCL inside the library), and two
ranks under torch.distributed.run sharing this box's one GPU (bench.py's N > 1 code path with libgspx
outputs; RCCL refuses two ranks on one device, so that launch gathers over gloo).  `-m gpu`."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_err
from gpu_helpers import BAR, TOL, ctx, random_graph, upper_lmax  # noqa: F401 (ctx is a fixture)
from oracle import cheby_oracle as orc
from pygsp_amd import _capi, engine, filters, graphs

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _flush_c_stdio():
    """RCCL prints a version banner through printf when a communicator is created; flush it inside the test
    that caused it (pytest captures it there) instead of at process exit, after pytest's summary line."""
    yield
    import ctypes
    ctypes.CDLL(None).fflush(None)


def _torchrun_bench(nproc, bench_args, env, timeout=900):
    """bench.py under torch.distributed.run on a free local port; a port that was taken between probing and
    binding (EADDRINUSE: other sockets of this very test session) is retried on another one."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = None
    for _ in range(4):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py")] + bench_args
        res = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=timeout)
        if res.returncode == 0 or "EADDRINUSE" not in res.stderr:
            break
    return res


def test_gather_and_batch_across_contexts(ctx):
    """gspx_gather: buffers of several contexts concatenated on the root (single-process form of the
    final gather; two contexts on this box's one GPU), and engine.filter_batch on top of it."""
    ctx2 = engine.Context(ctx.device)
    try:
        rng = np.random.default_rng(31)
        a = rng.standard_normal(1000)
        b = rng.standard_normal(333).astype(np.float32)
        pa, pb, pc = ctx.upload(a), ctx2.upload(b), ctx2.alloc(0)
        root = ctx.alloc(a.nbytes + b.nbytes + 16)
        engine.gather([pa, pc, pb], root)
        flat = root.download((a.nbytes + b.nbytes + 16,), np.uint8)
        assert np.array_equal(flat[:a.nbytes].view(np.float64), a)
        assert np.array_equal(flat[a.nbytes:a.nbytes + b.nbytes].view(np.float32), b)
        small = ctx.alloc(8)
        with pytest.raises(ValueError):
            engine.gather([pa, pb], small)
        with pytest.raises(ValueError):
            engine.gather([root], root)
        jobs, refs = [], []
        for i, c_ in enumerate((ctx, ctx2, ctx)):
            W, coords = graphs.sensor_weights(3000 + 500 * i, k=6, seed=40 + i)
            lmax = upper_lmax(W)
            dev = engine.DeviceGraph.from_w(W, dtype=np.float64, perm=engine.locality_order(W, coords), ctx=c_)
            c = orc.compute_cheby_coeff(orc.heat_kernel(10, lmax), lmax, 12)
            x = rng.standard_normal((W.shape[0], 5 + i))
            jobs.append((dev, c, x, lmax))
            refs.append(orc.cheby_op(orc.laplacian(W), lmax, c, x))
        outs = engine.filter_batch(jobs, root_ctx=ctx)
        for o, r in zip(outs, refs):
            assert o.shape == (1,) + r.shape and rel_err(o[0], r) < 1e-12
        for d, _, _, _ in jobs:
            d.destroy()
        for buf in (pa, pb, pc, root, small):  # a context must outlive its buffers
            buf.free()
    finally:
        ctx2.close()


def test_gather_through_rccl_in_the_library(ctx):
    """Option gather_rccl = 2 routes every block of gspx_gather through RCCL (ncclCommInitAll over the
    parts' devices, grouped ncclSend / ncclRecv) - on this one-GPU box as self send / recv, which still
    runs RCCL's communicator set-up, group launch and copy kernels on hardware."""
    if not engine.comm_available():
        pytest.skip("RCCL cannot be loaded on this box")
    ctx2 = engine.Context(ctx.device)
    try:
        rng = np.random.default_rng(5)
        a, b = rng.standard_normal(70000), rng.standard_normal(12345).astype(np.float32)
        pa, pb = ctx.upload(a), ctx2.upload(b)
        root = ctx.alloc(a.nbytes + b.nbytes)
        ctx.set_option("gather_rccl", 2)
        try:
            engine.gather([pa, pb], root)
        finally:
            ctx.set_option("gather_rccl", 1)
        flat = root.download((a.nbytes + b.nbytes,), np.uint8)
        assert np.array_equal(flat[:a.nbytes].view(np.float64), a)
        assert np.array_equal(flat[a.nbytes:].view(np.float32), b)
        for buf in (pa, pb, root):
            buf.free()
    finally:
        ctx2.close()


def test_comm_gather_one_rank(ctx):
    """gspx_comm_*: unique id -> ncclCommInitRank -> grouped send / recv.  One rank here (one GPU): the
    block of a filter output travels to the root buffer through RCCL and arrives bit for bit."""
    if not engine.comm_available():
        pytest.skip("RCCL cannot be loaded on this box")
    W, coords = graphs.sensor_weights(40000, k=6, seed=9)
    lmax = upper_lmax(W)
    dev = engine.DeviceGraph.from_w(W, dtype=np.float64, perm=engine.locality_order(W, coords), ctx=ctx)
    c = orc.compute_cheby_coeff(orc.heat_kernel(10, lmax), lmax, 20)
    x = np.random.default_rng(3).standard_normal((W.shape[0], 16))
    bx, by, broot = ctx.upload(x), ctx.alloc(x.nbytes), ctx.alloc(x.nbytes)
    comm = engine.Comm(ctx, 1, 0, engine.comm_unique_id())
    try:
        dev.cheby_filter_dev(c, bx.ptr, by.ptr, 16, lmax)
        ms = comm.gather(by.ptr, [x.nbytes], 0, broot.ptr)
        assert ms >= 0
        y = broot.download(x.shape, np.float64)
        assert np.array_equal(y, by.download(x.shape, np.float64))
        assert rel_err(y, orc.cheby_op(orc.laplacian(W), lmax, c, x)) < 1e-12
        with pytest.raises(ValueError):
            comm.gather(by.ptr, [x.nbytes, 0], 0, broot.ptr)
    finally:
        comm.close()
        dev.destroy()
        for b in (bx, by, broot):
            b.free()


def test_comm_outlives_its_context_safely():
    """A communicator whose context is destroyed first (use-after-free at the C-ABI): the context
    takes the RCCL communicator down with it, the handle stays a valid empty shell - gather reports an error,
    close() just frees it."""
    if not engine.comm_available():
        pytest.skip("RCCL cannot be loaded on this box")
    ctx2 = engine.Context(0)
    comm = engine.Comm(ctx2, 1, 0, engine.comm_unique_id())
    buf = ctx2.alloc(64)
    ptr = buf.ptr
    buf.free()
    ctx2.close()
    with pytest.raises(ValueError, match="context was destroyed"):
        comm.gather(ptr, [64], 0, ptr)
    comm.close()
    comm.close()  # idempotent
    with engine.Comm(engine.default_context(0), 1, 0, engine.comm_unique_id()) as c2:
        assert c2.nranks == 1


def test_two_ranks_on_this_gpu_through_bench():
    """bench.py --gpus 2 under torch.distributed.run, both ranks on device 0 (gloo process group): the
    N > 1 path - independent graph per rank, barrier-bracketed timing, MAX over ranks, final gather - runs
    end to end with libgspx outputs; rank 0 prints one JSON line with n_gpus = 2 and a gather time."""
    pytest.importorskip("torch")
    # GSPX_BENCH_LIB_GATHER=force: the in-library RCCL gather is attempted although RCCL must refuse two ranks
    # on one device - the attempt (id exchange, communicator creation under the watchdog), the agreement of the
    # ranks on its failure and the fall-back to the launcher's gather all run
    env = dict(os.environ, GSPX_ALL_RANKS_DEVICE0="1", HSA_ENABLE_IPC_MODE_LEGACY="0", GSPX_BENCH_LIB_GATHER="force")
    res = _torchrun_bench(2, ["--full", "--gpus", "2", "--steps", "2", "--warmup", "1", "--vertices", "100000", "--nsig", "16",
                              "--backend", "gloo", "--no-newton"], env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["value"] > 0
    assert out["gather_ms"] is not None and out["gather_ms"] > 0 and "torch.distributed (gloo)" in out["gather_impl"]
    assert out["config"]["N"] == 100000 and out["roofline"]["frac"] > 0
    assert out["parity_vs_oracle"]["ranks"] == 2 and out["parity_vs_oracle"]["max_rel_err"] < 1e-11
    b5 = out["batch_config4"]  # BASELINE configs[4]: 8 graphs sharded 4 + 4
    assert b5["n_gpus"] == 2 and b5["n_graphs"] == 8 and b5["value"] > 0 and "4/4" in b5["workload"]
    assert b5["parity_vs_oracle"]["max_rel_err"] < 1e-11
    # VERDICT r5 "Next 5": the N > 1 line is as checkable as the N = 1 line - the same keys
    check_multi_line_keys(out, wide=False)


def check_multi_line_keys(out, wide):
    """What BENCH_rNN's `parsed` holds at N = 1 is in the N > 1 line too: whole-call fraction, traffic (null away from
    the headline workload), this run's copy rate, the mix ceiling (wide panels), a CPU baseline with its cores."""
    rf = out["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic", "frac_whole_call", "copy_GBps_this_run",
                "algorithmic_bytes_per_launch", "avg_launch_ms", "launches_timed", "parity_max_rel_err"):
        assert key in rf, key
    assert 0 < rf["frac_whole_call"] <= rf["frac"] * 1.05 and rf["copy_GBps_this_run"] > 1000
    if wide:
        assert 0.5 < rf["frac_of_mix_ceiling"] < 1.3
    cb = out["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["value"] > 0 and "reference itself" in cb["note"]
    assert "real_pygsp_on_device" in out["config"]


def test_multi_gpu_lines_carry_the_single_gpu_keys():
    """The same check on a wide panel (64 fp64 signals: the wide LDS-staged step, so the mix ceiling is measured) for
    the launcher-free form, per device."""
    res = _run_bench(["--full", "--gpus", "2", "--devices", "0,0", "--steps", "2", "--warmup", "1", "--vertices", "100000",
                      "--nsig", "64", "--no-configs", "--cpu-cols", "4"])
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    check_multi_line_keys(out, wide=True)
    assert len(out["roofline"]["copy_GBps_per_device"]) == 2 and len(out["roofline"]["frac_of_mix_ceiling_per_device"]) == 2
    assert all(0.5 < p["frac_of_mix_ceiling"] < 1.3 and p["copy_GBps"] > 1000 for p in out["per_device"])


# ---- one process, several contexts / GPUs: bench.py --gpus N without a launcher, signal-parallel filtering ----
def _run_bench(args, timeout=900):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    return subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args, cwd=root, env=env,
                          capture_output=True, text=True, timeout=timeout)


def test_bench_refuses_more_gpus_than_visible():
    """`python bench.py --gpus N` with fewer than N devices: non-zero exit and a one-line reason, never a silent
    single-GPU line."""
    n = _capi.device_count()
    res = _run_bench(["--gpus", str(n + 1), "--steps", "1", "--warmup", "0"], timeout=300)
    assert res.returncode != 0
    assert "refusing" in res.stderr and not [ln for ln in res.stdout.splitlines() if ln.startswith("{")]


def test_bench_plain_run_is_the_headline_alone(tmp_path):
    """A plain `bench.py --gpus 1`: the timed steps, the dumped output and the headline keys; nothing that --full adds."""
    res = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--vertices", "100000", "--nsig", "16",
                      "--dump-outputs", str(tmp_path)], timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["unit"] == "vertex*signal*order/s" and out["metric"] and (out["steps"], out["warmup"]) == (2, 1)
    assert out["value"] == pytest.approx(100000 * 16 * 30 * 1e3 / out["ms_per_step"], rel=1e-9)
    for key in ("configs", "cpu_baseline", "headline_f32", "end_to_end_host_arrays", "chain3", "parity_vs_oracle",
                "batch_config4"):
        assert key not in out, key
    assert out["newton_form"] is None and out["product_form"] is None and out["gather_ms"] is None
    assert out["roofline"]["frac"] > 0 and out["roofline"]["copy_GBps_this_run"] is None
    assert np.load(tmp_path / "y.npy").shape == (100000, 16)


def test_bench_threads_two_contexts_on_this_gpu():
    """The launcher-free N > 1 path of bench.py on this box's one GPU: two contexts, two driver threads
    (`--devices 0,0`), barrier-bracketed timing, gspx_gather, parity of BOTH ranks, the strong-scaling batch."""
    res = _run_bench(["--full", "--gpus", "2", "--devices", "0,0", "--steps", "2", "--warmup", "1", "--vertices", "100000",
                      "--nsig", "16"])
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["value"] > 0 and out["devices"] == [0, 0]
    assert out["gather_ms"] > 0 and "gspx_gather" in out["gather_impl"] and out["rccl_ranks"] == 0
    assert len(out["per_device"]) == 2 and all(p["frac"] > 0 for p in out["per_device"])
    assert out["parity_vs_oracle"]["ranks"] == 2 and out["parity_vs_oracle"]["max_rel_err"] < 1e-11
    b5 = out["batch_config4"]
    assert b5["n_gpus"] == 2 and b5["n_graphs"] == 8 and "4/4" in b5["workload"] and b5["value"] > 0
    assert b5["parity_vs_oracle"]["max_rel_err"] < 1e-11 and b5["parity_vs_oracle"]["graphs_checked"] == 2
    sp = out["signal_parallel"]  # one graph, its 16 signals split 8 / 8 over the two contexts
    assert sp["n_gpus"] == 2 and "8/8" in sp["workload"] and sp["value"] > 0 and sp["gather_ms"] > 0
    assert sp["parity_vs_oracle"]["max_rel_err"] < 1e-11
    check_multi_line_keys(out, wide=False)


def test_bench_threads_eight_contexts_on_this_gpu():
    """The 8-way form the driver's 8-GPU node would run, dry on this box's one GPU (`--gpus 8 --devices 0,0,0,0,0,0,0,0`):
    eight contexts and driver threads, the weak line, the 64 signals of one graph split 8 x 8 (signal_parallel), the
    batch of BASELINE configs[4] one graph per context, gspx_gather of eight parts - parity on all eight."""
    res = _run_bench(["--full", "--gpus", "8", "--devices", "0,0,0,0,0,0,0,0", "--steps", "2", "--warmup", "1", "--vertices", "100000"],
                     timeout=1200)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == 8 and out["scaling"] == "weak" and out["value"] > 0 and out["devices"] == [0] * 8
    assert len(out["per_device"]) == 8 and all(p["frac"] > 0 for p in out["per_device"])
    assert out["driver_thread_cores"] == [None] * 8  # one physical GPU: nothing to pin apart
    assert out["gather_ms"] > 0 and "gspx_gather" in out["gather_impl"] and out["rccl_ranks"] == 0
    assert out["parity_vs_oracle"]["ranks"] == 8 and out["parity_vs_oracle"]["max_rel_err"] < 1e-11
    sp = out["signal_parallel"]
    assert sp["n_gpus"] == 8 and "8/8/8/8/8/8/8/8" in sp["workload"] and sp["value"] > 0
    assert sp["parity_vs_oracle"]["max_rel_err"] < 1e-11
    b5 = out["batch_config4"]
    assert b5["n_gpus"] == 8 and b5["n_graphs"] == 8 and "1/1/1/1/1/1/1/1" in b5["workload"] and b5["value"] > 0
    assert b5["parity_vs_oracle"]["max_rel_err"] < 1e-11 and b5["parity_vs_oracle"]["graphs_checked"] == 8


def test_device_pci_address_and_numa_lookup():
    """gspx_device_pci_bus_id names this GPU's PCI function; the NUMA lookup built on it never raises (the cores of
    the GPU's node, or None when the platform does not say)."""
    import ctypes

    from pygsp_amd import multi
    buf = ctypes.create_string_buffer(64)
    _capi.check(_capi.load().gspx_device_pci_bus_id(0, buf, 64))
    address = buf.value.decode()
    assert len(address.split(":")) == 3 and "." in address, address
    with pytest.raises(ValueError):
        _capi.check(_capi.load().gspx_device_pci_bus_id(_capi.device_count(), buf, 64))
    cpus = multi.numa_cpus_of(0)
    assert cpus is None or (isinstance(cpus, set) and cpus)
    before = os.sched_getaffinity(0)
    try:
        pinned = multi.pin_thread_near(0)
        assert pinned is None or pinned == os.sched_getaffinity(0)
    finally:
        os.sched_setaffinity(0, before)


def test_bench_all_visible_gpus_through_rccl():
    """On a box with >= 2 GPUs: bench.py --gpus <all> drives them from one process and gathers through the
    library's RCCL communicators (ncclCommInitAll) with real peers."""
    n = _capi.device_count()
    if n < 2:
        pytest.skip("one GPU visible: cross-device gspx_gather cannot run here")
    res = _run_bench(["--full", "--gpus", str(n), "--steps", "2", "--warmup", "1", "--vertices", "200000", "--nsig", "16"])
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == n and out["rccl_ranks"] == n and "RCCL" in out["gather_impl"]
    assert out["parity_vs_oracle"]["ranks"] == n and out["parity_vs_oracle"]["max_rel_err"] < 1e-11
    assert out["batch_config4"]["parity_vs_oracle"]["max_rel_err"] < 1e-11


def test_comm_gather_real_peers():
    """gspx_comm_* (one process per GPU) with real peers, on a box with >= 2 GPUs: bench.py under
    torch.distributed.run, backend nccl, the in-library gather must succeed on every rank."""
    n = _capi.device_count()
    if n < 2:
        pytest.skip("one GPU visible")
    pytest.importorskip("torch")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = _torchrun_bench(n, ["--full", "--gpus", str(n), "--steps", "2", "--warmup", "1", "--vertices", "200000", "--nsig", "16",
                              "--no-newton"], env, timeout=1200)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == n and "gspx_comm_gather" in out["gather_impl"]
    assert out["parity_vs_oracle"]["max_rel_err"] < 1e-11


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_filter_columns_split_over_two_contexts(ctx, dtype):
    """ONE graph replicated on every context of the device list, the signal columns split,
    one gather - through Filter.filter(..., devices=[...]).  Two contexts on this box's GPU; columns come back
    in the caller's order and equal the single-device result bit for bit (same kernels, same panel widths are
    not guaranteed - so: equal to the oracle within the bar, and to the one-device call within rounding)."""
    from pygsp_amd import multi
    G = graphs.Sensor(6000, seed=3, compute_dtype=dtype)
    G.estimate_lmax("bounds")
    rng = np.random.default_rng(8)
    L = orc.laplacian(G.W)
    tol = TOL[np.dtype(dtype)] * 10
    for bank, kernels in ((filters.Heat(G, 10), [orc.heat_kernel(10, G.lmax)]),
                          (filters.MexicanHat(G, Nf=4), orc.mexican_hat_kernels(G.lmax, 4))):
        for nsig in (1, 5, 16):
            x = rng.standard_normal((G.N, nsig))
            one = bank.filter(x, order=20)
            two = bank.filter(x, order=20, devices=[0, 0])
            assert two.shape == one.shape
            ref = orc.filter_chebyshev(L, G.lmax, kernels, x.astype(dtype).astype(np.float64), 20)
            assert rel_err(two, np.squeeze(ref)) < tol and rel_err(two, one) < tol
    # synthesis: (N, Nsig, Nf) -> (N, Nsig), columns split the same way
    bank = filters.MexicanHat(G, Nf=4)
    s = rng.standard_normal((G.N, 6, 4))
    assert rel_err(bank.filter(s, order=12, devices=[0, 0]), bank.filter(s, order=12)) < tol
    # three "devices", fewer columns than devices: the empty shard is skipped
    x = rng.standard_normal((G.N, 2))
    tm = {}
    y, _ = multi.filter_columns(G, filters.compute_cheby_coeff(filters.Heat(G, 10), m=10), x, [0, 0, 0], timings=tm)
    assert tm["columns"] == [1, 1, 0] and y.shape == (1, G.N, 2)
    assert rel_err(y[0], orc.filter_chebyshev(L, G.lmax, [orc.heat_kernel(10, G.lmax)],
                                              x.astype(dtype).astype(np.float64), 10)) < tol
    # every GPU shipping its own columns to the host (no collective) gives the same panel
    yh, _ = multi.filter_columns(G, filters.compute_cheby_coeff(filters.Heat(G, 10), m=10), x, [0, 0, 0], collect="host")
    assert np.array_equal(yh, y)
    # the replicas are cached on the graph: a second call builds nothing
    reps = dict(G._gspx_replicas)
    bank.filter(s, order=12, devices=[0, 0])
    assert {k: v[1] for k, v in G._gspx_replicas.items()} == {k: v[1] for k, v in reps.items()}
    with pytest.raises(ValueError):
        bank.filter(x, devices=[0, _capi.device_count()])


def test_plugin_install_with_a_device_list(ctx):
    """plugin.install(devices=[...]): a reference-shaped graph is replicated per context and every
    cheby_op call splits its columns (here over two contexts of this GPU)."""
    import types

    from pygsp_amd import plugin
    W = random_graph(5000, 6, 21)

    class RefGraph:
        def __init__(self):
            self.W, self.N, self.lap_type = W, W.shape[0], "combinatorial"
            self.L = orc.laplacian(W)
            self.lmax = upper_lmax(W)

        def is_directed(self):
            return False

    fake = types.ModuleType("pygsp")
    fake.filters = types.ModuleType("pygsp.filters")
    fake.filters.approximations = types.ModuleType("pygsp.filters.approximations")
    orig = lambda G, c, s, **kw: orc.cheby_op(G.L, G.lmax, c, s)  # noqa: E731
    fake.filters.approximations.cheby_op = orig
    fake.filters.cheby_op = orig
    G = RefGraph()
    c = orc.compute_cheby_coeff(orc.heat_kernel(4, G.lmax), G.lmax, 15)
    s = np.random.default_rng(3).standard_normal((G.N, 7))
    plugin.install(fake, devices=[0, 0])
    try:
        y = fake.filters.approximations.cheby_op(G, c, s)
        assert y.shape == (G.N, 7) and rel_err(y, orig(G, c, s)) < 1e-12
        assert len(G._gspx_dev) == 2  # one device graph per context
        assert fake.filters.cheby_op(G, c, s[:, 0]).shape == (G.N,)
    finally:
        plugin.uninstall(fake)
        plugin.install(fake)  # back to the single-device configuration for the tests that follow
        plugin.uninstall(fake)
