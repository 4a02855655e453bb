"""Thin object layer over the libgspx C-ABI: Context, DeviceBuffer, DeviceArray, Comm, DeviceGraph, DeviceAdjacency
and the device graph builders (knn_graph, radius_graph, sbm_graph).

Nothing here computes: every numeric result comes out of the HIP kernels in
pygsp_amd/csrc.  Vertex reordering (a graph-setup step, like building the Laplacian) is the
only host-side preparation, see ``locality_order``.
"""
import ctypes
import sys
import threading

import numpy as np
from scipy import sparse

from . import _capi


class Context:
    """One device + one HIP stream (gspx_ctx).  Calls on one Context must be serialised."""

    def __init__(self, device=0):
        lib = _capi.load()
        h = ctypes.c_void_p()
        _capi.check(lib.gspx_ctx_create(int(device), ctypes.byref(h)))
        self._h = h
        self.device = int(device)
        self._init_pool()

    def _init_pool(self):
        """The recycled-buffer pool and its lock (also called by host-only tests that build a Context without a
        device)."""
        self._pool, self._pooled, self._pool_lock = {}, 0, threading.RLock()

    def close(self):
        """Explicit teardown.  (No __del__: graphs and buffers hold a pointer to their context, so
        a context must outlive them; default contexts simply live until the process exits.)"""
        if getattr(self, "_h", None):
            self.clear_pool()
            _capi.load().gspx_ctx_destroy(self._h)
            self._h = None

    def set_option(self, key, value):
        _capi.check(_capi.load().gspx_ctx_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key):
        v = ctypes.c_int64(0)
        _capi.check(_capi.load().gspx_ctx_get_option(self._h, key.encode(), ctypes.byref(v)))
        return v.value

    def sync(self):
        _capi.check(_capi.load().gspx_ctx_sync(self._h))

    def last_timing(self):
        """dict of HIP-event timings (ms) of the last filter call on this context."""
        out = (ctypes.c_double * 5)()
        _capi.check(_capi.load().gspx_last_timing(self._h, out))
        return {"total_ms": out[0], "steps_ms": out[1], "step_launches": int(out[2]),
                "permute_ms": out[3], "combine_ms": out[4]}

    def last_step_kinds(self):
        """{"tile": launches of the LDS-staged tile kernel, "plain": launches of the plain step kernels} of the last
        filter, Newton or program call on this context (gspx_last_step_kinds; counted on the host)."""
        out = (ctypes.c_int64 * 2)()
        _capi.check(_capi.load().gspx_last_step_kinds(self._h, out))
        return {"tile": int(out[0]), "plain": int(out[1])}

    def last_host_timing(self):
        """Stage times (ms) of the last host-array filter call on this context (gspx_last_host_timing); None
        when that call was not pipelined."""
        out = (ctypes.c_double * 9)()
        _capi.check(_capi.load().gspx_last_host_timing(self._h, out))
        if out[6] == 0:
            return None
        return {"wall_ms": out[0], "pack_ms": out[1], "h2d_ms": out[2], "kernel_ms": out[3], "d2h_ms": out[4],
                "unpack_ms": out[5], "batches": int(out[6]), "signals_per_batch": int(out[7]),
                "host_threads_per_direction": int(out[8])}

    def last_host_timeline(self):
        """(batches, 6) array: host clock (ms since the call began) at which every batch of the last pipelined
        host-array call was packed, had its H2D issued, began / finished its kernels, finished its D2H, was unpacked."""
        n = ctypes.c_int(0)
        _capi.check(_capi.load().gspx_last_host_timeline(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros((max(n.value, 0), 6))
        if n.value > 0:
            _capi.check(_capi.load().gspx_last_host_timeline(self._h, _capi.ptr(out), out.size, ctypes.byref(n)))
        return out

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    # Buffers of device-resident arrays (DeviceArray) are recycled: a chain of filters allocates and drops a few
    # panels of the same sizes per call, and hipMalloc / hipFree of gigabyte buffers cost milliseconds each (and a
    # device synchronisation).  Exact-size matches only, a bounded amount kept (POOL_BYTES; the pool never holds more
    # than that, and less as soon as device memory is short: every library call that may allocate goes through
    # call(), which empties the pool and retries once when the allocation fails); clear_pool() frees it.  The pool is
    # touched from DeviceArray.__del__ (any thread the collector runs on) and from user threads: one lock.
    POOL_BYTES = 8 << 30

    def pooled_bytes(self):
        with self._pool_lock:
            return self._pooled

    def take(self, nbytes):
        nbytes = max(int(nbytes), 16)
        with self._pool_lock:
            stack = self._pool.get(nbytes)
            if stack:
                self._pooled -= nbytes
                return stack.pop()
        return DeviceBuffer(self, nbytes)  # (through call(): trims the pool and retries if the device is full)

    def give(self, buf):
        with self._pool_lock:
            if not getattr(buf, "_h", None) or buf.ctx is not self or self._pooled + buf.nbytes > self.POOL_BYTES:
                buf.free()
                return
            self._pool.setdefault(buf.nbytes, []).append(buf)
            self._pooled += buf.nbytes

    def clear_pool(self):
        with self._pool_lock:
            stacks, self._pool, self._pooled = list(self._pool.values()), {}, 0
        for stack in stacks:
            for buf in stack:
                buf.free()

    def call(self, fn, *args):
        """rc = fn(*args) for a libgspx entry point that may allocate device memory (buffers, workspaces, graph
        builds), mapped to the reference's exception types.  An ALLOCATION failure (GSPX_ERR_OOM: nothing has been
        launched or written by then - every entry point allocates its workspaces before its first kernel) while the
        pool holds recycled buffers empties the pool and runs the call once more: memory kept for reuse must never be
        the reason a call fails that would have succeeded without the pool.  Any other failure surfaces at
        once: a call that failed midway is never repeated on inputs it may have overwritten (workspaces
        are grow-only and sized by a call's first batch, so an allocation can only fail before the first kernel)."""
        rc = fn(*args)
        if rc == _capi.ERR_OOM and self.pooled_bytes() > 0:
            self.clear_pool()
            rc = fn(*args)
        _capi.check(rc)

    def bench_copy(self, nbytes=1 << 30, iters=10):
        """Measured read+write GB/s of the engine's streaming copy kernel (HBM ceiling)."""
        v = ctypes.c_double(0)
        _capi.check(_capi.load().gspx_bench_copy(self._h, int(nbytes), int(iters), ctypes.byref(v)))
        return v.value

    def bench_read(self, nbytes, passes=50):
        """Read-only GB/s of an nbytes buffer streamed `passes` times in one launch."""
        v = ctypes.c_double(0)
        _capi.check(_capi.load().gspx_bench_read(self._h, int(nbytes), int(passes), ctypes.byref(v)))
        return v.value

    def bench_streams(self, bytes_per_stream, n_read, n_write, nt=0, workgroups_per_cu=8, iters=5):
        """Total GB/s of n_read read streams + n_write write streams walked together (gspx_bench_streams)."""
        v = ctypes.c_double(0)
        _capi.check(_capi.load().gspx_bench_streams(self._h, int(bytes_per_stream), int(n_read), int(n_write), int(nt),
                                                    int(workgroups_per_cu), int(iters), ctypes.byref(v)))
        return v.value

    def bench_gather(self, panel_rows, row_bytes, n_gathers, in_flight=8, blocks=1, p_intra=0.0, workgroups_per_cu=8,
                     iters=5):
        """Rate of random row gathers on this device (gspx_bench_gather): (ms per launch, GB/s of row bytes)."""
        ms, gb = ctypes.c_double(0), ctypes.c_double(0)
        _capi.check(_capi.load().gspx_bench_gather(self._h, int(panel_rows), int(row_bytes), int(n_gathers),
                                                   int(in_flight), int(blocks), float(p_intra), int(workgroups_per_cu),
                                                   int(iters), ctypes.byref(ms), ctypes.byref(gb)))
        return ms.value, gb.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        buf = DeviceBuffer(self, arr.nbytes)
        buf.upload(arr)
        return buf

    def _temporaries(self):
        """``with ctx._temporaries() as t``: the device buffers of one host-array call (_Temporaries)."""
        return _Temporaries(self)

    def identity_panel(self, buf, N, j0, w, dtype):
        """Write columns [j0, j0 + w) of the N x N identity into `buf` (row-major N x w, on the device)."""
        _capi.check(_capi.load().gspx_identity_panel_dev(self._h, _capi.dtype_code(dtype), int(N), int(j0), int(w),
                                                        ctypes.c_void_p(buf.ptr)))


_default_ctx = {}
_default_lock = threading.Lock()


def default_context(device=0):
    with _default_lock:
        ctx = _default_ctx.get(device)
        if ctx is None:
            ctx = Context(device)
            _default_ctx[device] = ctx
        return ctx


class DeviceBuffer:
    """Device memory owned by libgspx (gspx_buf)."""

    def __init__(self, ctx, nbytes):
        h = ctypes.c_void_p()
        ctx.call(_capi.load().gspx_buf_alloc, ctx._h, int(nbytes), ctypes.byref(h))
        self._h = h
        self.ctx = ctx
        self.nbytes = int(nbytes)

    def free(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):  # a closed context took the device state with it:
                _capi.load().gspx_buf_free(self._h)  # never hand libgspx a dangling context
            self._h = None

    def __del__(self):
        if sys.is_finalizing():  # the HIP runtime may already be gone; the OS reclaims the memory
            return
        try:
            self.free()
        except Exception:
            pass

    @property
    def ptr(self):
        p = ctypes.c_void_p()
        _capi.check(_capi.load().gspx_buf_ptr(self._h, ctypes.byref(p)))
        return p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        _capi.check(_capi.load().gspx_buf_upload(self._h, _capi.ptr(arr), arr.nbytes))

    def download(self, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        _capi.check(_capi.load().gspx_buf_download(self._h, _capi.ptr(out), out.nbytes))
        return out


class _Temporaries:
    """The DeviceBuffers of one call (Context._temporaries): upload() and alloc() hand them out, and every one of
    them is freed, in the order they were made, when the ``with`` block ends - also when an exception passes through."""

    def __init__(self, ctx):
        self.ctx, self._bufs = ctx, []

    def add(self, buf):
        self._bufs.append(buf)
        return buf

    def upload(self, arr):
        return self.add(self.ctx.upload(arr))

    def alloc(self, nbytes):
        return self.add(self.ctx.alloc(max(int(nbytes), 16)))  # (a zero-size output still gets a valid pointer)

    def keep(self, buf):
        """`buf` outlives the block: the caller owns it from here on."""
        self._bufs.remove(buf)
        return buf

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for buf in self._bufs:
            buf.free()


class DeviceArray:
    """A signal tensor that lives on the device between calls: what ``Filter.filter`` / ``analyze`` /
    ``synthesize`` return when they are given one, so that a chain of filters (the doctest of filter.py:232-256:
    heat -> analysis -> synthesis) costs one upload and one download instead of a PCIe round trip per call.

    `shape` is the shape the reference's call would have returned (the squeezed (vertices, signals, features)
    cube of filter.py:328); the memory is the engine's layout - `n_features` planes [feature][vertex][signal] in
    the compute dtype, exactly what gspx_cheby_filter_dev reads and writes, so chaining moves nothing.
    ``np.asarray(a)`` / ``a.numpy()`` download it as the float64 array the reference would have returned."""

    __array_priority__ = 100

    def __init__(self, buf, cube, dtype):
        self._buf, self.ctx = buf, buf.ctx
        self.cube = tuple(int(d) for d in cube)  # (vertices, signals, features)
        self.dtype = np.dtype(dtype)
        self.shape = tuple(d for d in self.cube if d != 1)

    @classmethod
    def from_host(cls, ctx, array, dtype=np.float64):
        """Upload a host signal: (N,), (N, Nsig) or (N, Nsig, Nfeat) of any real dtype / memory order."""
        a = np.asanyarray(array)
        if np.iscomplexobj(a):
            raise TypeError("complex signals are not supported by the Chebyshev path")
        if a.ndim < 1 or a.ndim > 3:
            raise ValueError("At most 3 dimensions: #nodes x #signals x #features.")
        cube = a.reshape(a.shape + (1,) * (3 - a.ndim))
        planes = np.ascontiguousarray(np.moveaxis(cube, 2, 0), dtype=dtype)
        buf = ctx.take(max(planes.nbytes, 16))
        if planes.nbytes:
            buf.upload(planes)
        out = cls(buf, cube.shape, dtype)
        out.shape = tuple(a.shape)  # as given (not squeezed): the caller's own shape rules apply to it
        return out

    @classmethod
    def empty(cls, ctx, cube, dtype):
        n = int(np.prod(cube)) * np.dtype(dtype).itemsize
        return cls(ctx.take(max(n, 16)), cube, dtype)

    @property
    def ndim(self):
        return len(self.shape)

    @property
    def size(self):
        return int(np.prod(self.cube))

    @property
    def nbytes(self):
        return self.size * self.dtype.itemsize

    @property
    def ptr(self):
        if self._buf is None:
            raise ValueError("the device array has been freed")
        return self._buf.ptr

    def planes(self, signals, features):
        """Device pointer (+ the object keeping it alive) of this tensor as `features` planes of (N, signals):
        itself when that is how it is stored, else a repacked copy (gspx_planes_pack_dev) - the per-vertex
        elements are re-read in row-major order, as ``reshape`` of the host array would."""
        N, S0, F0 = self.cube
        if S0 * F0 != signals * features:
            raise ValueError("cannot view {} signals x {} features as {} x {}".format(S0, F0, signals, features))
        if (S0, F0) == (signals, features) or self.size == 0:
            return self.ptr, self
        lib, code, cur = _capi.load(), _capi.dtype_code(self.dtype), self
        if F0 != 1:  # planes -> the row-major cube (N, S0 * F0)
            flat = DeviceArray.empty(self.ctx, (N, S0 * F0, 1), self.dtype)
            _capi.check(lib.gspx_planes_pack_dev(self.ctx._h, code, N, S0, F0, ctypes.c_void_p(self.ptr),
                                                 ctypes.c_void_p(flat.ptr), 0))
            cur = flat
        if features != 1:  # the cube (N, signals, features) -> planes
            out = DeviceArray.empty(self.ctx, (N, signals, features), self.dtype)
            _capi.check(lib.gspx_planes_pack_dev(self.ctx._h, code, N, signals, features, ctypes.c_void_p(cur.ptr),
                                                 ctypes.c_void_p(out.ptr), 1))
            cur = out
        return cur.ptr, cur

    def numpy(self):
        """The float64 host array the reference would have returned (shape `self.shape`)."""
        N, S, F = self.cube
        if self.size == 0:
            return np.zeros(self.shape)
        planes = self._buf_download((F, N, S))
        return np.asarray(np.moveaxis(planes, 0, 2), dtype=np.float64).reshape(self.shape)

    def _buf_download(self, shape):
        if self._buf is None:
            raise ValueError("the device array has been freed")
        return self._buf.download(shape, self.dtype)

    def __array__(self, dtype=None, copy=None):
        out = self.numpy()
        return out if dtype is None else out.astype(dtype, copy=False)

    def __len__(self):
        if not self.shape:
            raise TypeError("len() of unsized object")
        return self.shape[0]

    def __repr__(self):
        return "DeviceArray(shape={}, dtype={}, device={})".format(self.shape, self.dtype, self.ctx.device)

    def free(self):
        """Give the memory back (to the context's pool of recycled buffers: Context.give)."""
        if self._buf is not None:
            buf, self._buf = self._buf, None
            if getattr(self.ctx, "_h", None):
                self.ctx.sync()  # (nothing queued on the stream may still read or write it when it is handed out again)
                self.ctx.give(buf)
            else:
                buf.free()

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.free()
        except Exception:
            pass


def gather(parts, root_out):
    """Concatenate device buffers living on (possibly) different contexts / GPUs into `root_out`:
    the single-process form of the path's one collective (gspx_gather; peer copies over xGMI)."""
    n = len(parts)
    arr = (ctypes.c_void_p * max(n, 1))(*[b._h for b in parts])
    _capi.check(_capi.load().gspx_gather(None, n, arr, root_out._h))
    return root_out


COMM_ID_BYTES = 128


def comm_available():
    """True when RCCL could be loaded by libgspx (gspx_comm_available)."""
    return bool(_capi.load().gspx_comm_available())


def comm_unique_id():
    """A fresh RCCL unique id (bytes): made on rank 0, handed to the other ranks by the launcher."""
    buf = (ctypes.c_ubyte * COMM_ID_BYTES)()
    _capi.check(_capi.load().gspx_comm_unique_id(buf))
    return bytes(buf)


def comm_info(comm=None):
    """{"rccl_version", "nranks", "rank"} as RCCL reports them (gspx_comm_info): of `comm`, or - without one - of the
    device set this process's last RCCL gspx_gather ran on (nranks 0: none has run).  Version 0: RCCL is unavailable."""
    out = np.zeros(3, dtype=np.int64)
    _capi.check(_capi.load().gspx_comm_info(comm._h if comm is not None else None, _capi.ptr(out)))
    return {"rccl_version": int(out[0]), "nranks": int(out[1]), "rank": int(out[2])}


class Comm:
    """RCCL communicator of one rank (gspx_comm): the one-process-per-GPU form of the path's only
    collective, the gather of the ranks' output blocks to a root over xGMI."""

    def __init__(self, ctx, nranks, rank, unique_id):
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("unique_id must be {} bytes".format(COMM_ID_BYTES))
        buf = (ctypes.c_ubyte * COMM_ID_BYTES).from_buffer_copy(unique_id)
        h = ctypes.c_void_p()
        _capi.check(_capi.load().gspx_comm_create(ctx._h, int(nranks), int(rank), buf, ctypes.byref(h)))
        self._h, self.ctx, self.nranks, self.rank = h, ctx, int(nranks), int(rank)

    def gather(self, part_ptr, nbytes_per_rank, root=0, root_out_ptr=None):
        """Collective: this rank's block (device pointer, nbytes_per_rank[rank] bytes) lands in the root's
        buffer at the offset of its rank.  Returns the device milliseconds of the exchange on this rank."""
        table = np.ascontiguousarray(nbytes_per_rank, dtype=np.int64)
        if table.shape != (self.nranks,):
            raise ValueError("nbytes_per_rank must have one entry per rank")
        ms = ctypes.c_double(0)
        _capi.check(_capi.load().gspx_comm_gather(
            self._h, ctypes.c_void_p(part_ptr), _capi.ptr(table), int(root),
            ctypes.c_void_p(root_out_ptr) if root_out_ptr else None, ctypes.byref(ms)))
        return ms.value

    def info(self):
        """What RCCL itself reports about this communicator (gspx_comm_info): version code, ranks, own rank."""
        return comm_info(self)

    def close(self):
        # (after its context is gone the handle is an empty shell inside libgspx - gspx_ctx_destroy took the RCCL
        # communicator down with the stream - and gspx_comm_destroy only frees it)
        if getattr(self, "_h", None):
            _capi.load().gspx_comm_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


def filter_batch(jobs, root_ctx=None):
    """Independent (graph, coefficients, signals, lmax) jobs, one driver thread per context: job i
    runs on the context its DeviceGraph lives on (ctypes releases the GIL inside libgspx), the
    outputs are gathered onto `root_ctx` and returned as one list of host arrays.

    jobs: list of (DeviceGraph, c (Nf, K+1) or (K+1,), x (N, Nsig) host array, lmax).
    This is the single-process counterpart of `bench.py --gpus N` (one process per GPU there)."""
    import threading as _th
    root_ctx = root_ctx or jobs[0][0].ctx
    outs = [None] * len(jobs)
    errs = []

    def work(i):
        try:
            dev, c, x, lmax = jobs[i]
            c2 = _coeff_matrix(c)
            x = np.ascontiguousarray(x, dtype=dev.dtype)
            with dev.ctx._temporaries() as t:
                bx = t.upload(x)
                by = t.add(dev.ctx.alloc(x.nbytes * c2.shape[0]))  # (exactly the bytes gather() concatenates)
                dev.cheby_filter_dev(c2, bx.ptr, by.ptr, x.shape[1], lmax)
                outs[i] = (t.keep(by), (c2.shape[0],) + x.shape, dev.dtype)  # owned by outs from here on
        except Exception as e:  # surfaced on the caller's thread
            errs.append(e)

    by_ctx = {}
    for i, j in enumerate(jobs):
        by_ctx.setdefault(id(j[0].ctx), []).append(i)
    threads = [_th.Thread(target=lambda idx=idx: [work(i) for i in idx]) for idx in by_ctx.values()]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    root = None
    try:
        if errs:
            raise errs[0]
        total = sum(b.nbytes for b, _, _ in outs)
        root = root_ctx.alloc(total)
        gather([b for b, _, _ in outs], root)
        flat = root.download((total,), np.uint8)
        res, off = [], 0
        for b, shape, dt in outs:
            res.append(flat[off:off + b.nbytes].view(dt).reshape(shape))
            off += b.nbytes
        return res
    finally:  # every device buffer of the batch is released, also when a job failed
        for o in outs:
            if o is not None:
                o[0].free()
        if root is not None:
            root.free()


def _int32_csr(M):
    """(indptr, indices) of the scipy CSR matrix M as int32 arrays: its own when they are already."""
    indptr, indices = M.indptr, M.indices
    if indptr.dtype != np.int32 or indices.dtype != np.int32:
        if M.shape[0] >= 2 ** 31 - 1 or M.nnz >= 2 ** 31 - 1:
            raise ValueError("graph too large for int32 CSR indices")
        indptr, indices = indptr.astype(np.int32), indices.astype(np.int32)
    return indptr, indices


def _canonical_csr(M):
    M = sparse.csr_matrix(M)
    if not M.has_canonical_format:
        M = M.copy()
        M.sum_duplicates()
    indptr, indices = _int32_csr(M)
    if indptr is not M.indptr:
        M = sparse.csr_matrix((M.data, indices, indptr), shape=M.shape)
    return M


def _lap_code(lap_type):
    if lap_type not in ("combinatorial", "normalized"):
        raise ValueError("Unknown Laplacian type {}".format(lap_type))
    return _capi.LAP_COMBINATORIAL if lap_type == "combinatorial" else _capi.LAP_NORMALIZED


def _theta_stack(theta):
    """(M, Fin, Fout) float64, contiguous: the matrix coefficients of a Chebyshev graph convolution."""
    th = np.ascontiguousarray(theta, dtype=np.float64)
    if th.ndim != 3:
        raise ValueError("theta must be (M, Fin, Fout), got {}".format(th.shape))
    return th


def _coeff_matrix(coeffs):
    """Chebyshev coefficients as the contiguous float64 (Nf, M) matrix libgspx reads; a vector is one filter."""
    return np.ascontiguousarray(np.atleast_2d(np.asarray(coeffs, dtype=np.float64)))


def _program_columns(program):
    """(S, scale, beta, gamma): the rows (scale, beta, gamma) of a polynomial program as three contiguous columns."""
    prog = np.ascontiguousarray(program, dtype=np.float64).reshape(-1, 3)
    return (prog.shape[0],) + tuple(np.ascontiguousarray(prog[:, k]) for k in range(3))


def _curve_coords(coords, n_vertices):
    """True when a space-filling curve can order the vertices by `coords`: one row per vertex, at least two columns."""
    return (coords is not None and np.ndim(coords) == 2 and np.shape(coords)[0] == n_vertices
            and np.shape(coords)[1] >= 2)


def hilbert_order(coords, bits=16):
    """Vertex order along a 2-D Hilbert curve (no long jumps, unlike the Z-curve)."""
    c = np.asarray(coords, dtype=np.float64)[:, :2]
    lo = c.min(axis=0)
    span = c.max(axis=0) - lo
    span[span == 0] = 1.0
    q = np.minimum(((c - lo) / span * (1 << bits)).astype(np.int64), (1 << bits) - 1)
    x, y = q[:, 0].copy(), q[:, 1].copy()
    d = np.zeros(len(x), dtype=np.int64)
    s = 1 << (bits - 1)
    while s > 0:
        rx = ((x & s) > 0).astype(np.int64)
        ry = ((y & s) > 0).astype(np.int64)
        d += s * s * ((3 * rx) ^ ry)
        flip = (ry == 0) & (rx == 1)
        x = np.where(flip, s - 1 - x, x)
        y = np.where(flip, s - 1 - y, y)
        swap = ry == 0
        x, y = np.where(swap, y, x), np.where(swap, x, y)
        s >>= 1
    return np.argsort(d, kind="stable").astype(np.int32)


def locality_order(W, coords=None, curve="auto", device=0, ctx=None):
    """Vertex order used INSIDE the engine (perm[new] = old) so that neighbour gathers hit cache.

    * with coordinates (NN graphs such as Sensor): a space-filling curve through the first two /
      three coordinates - median |i-j| over stored entries drops from ~N/4 to a handful.
      curve="auto": Hilbert in 2-D (no long jumps: a 64-row block of the k=8 sensor graph gathers
      117 distinct rows instead of 123 under the Z-curve, and the LDS-staged step kernel runs 5-8 %
      faster), Morton (Z-order) in 3-D; "morton" / "hilbert" force one;
    * otherwise reverse Cuthill-McKee on the pattern of W.
    The order is invisible to callers: inputs/outputs stay in the graph's own vertex order.
    """
    N = W.shape[0]
    if N < 2:
        return None
    has_coords = _curve_coords(coords, N)
    if has_coords and N >= 4096 and _capi.device_count() > 0:
        # curve keys and their stable argsort (a radix sort) on the device: gspx_curve_order
        hil = curve == "hilbert" or (curve == "auto" and coords.shape[1] == 2)
        c = np.ascontiguousarray(coords, dtype=np.float64)
        perm = np.empty(N, dtype=np.int32)
        _capi.check(_capi.load().gspx_curve_order((ctx or default_context(device))._h, N, c.shape[1], _capi.ptr(c),
                                                  1 if hil else 0, _capi.ptr(perm)))
        return perm
    if has_coords and (curve == "hilbert" or (curve == "auto" and coords.shape[1] == 2)):
        return hilbert_order(coords)
    if has_coords:
        c = np.asarray(coords, dtype=np.float64)[:, :3]
        lo = c.min(axis=0)
        span = c.max(axis=0) - lo
        span[span == 0] = 1.0
        d = c.shape[1]
        bits = 21 if d == 3 else 31
        q = np.minimum(((c - lo) / span * (2 ** bits - 1)).astype(np.uint64), 2 ** bits - 1)
        code = np.zeros(N, dtype=np.uint64)
        for b in range(bits):
            for k in range(d):
                code |= ((q[:, k] >> np.uint64(b)) & np.uint64(1)) << np.uint64(b * d + k)
        return np.argsort(code, kind="stable").astype(np.int32)
    from scipy.sparse.csgraph import reverse_cuthill_mckee
    pattern = sparse.csr_matrix((np.ones(W.nnz, dtype=np.int8), W.indices, W.indptr), shape=W.shape)
    return np.asarray(reverse_cuthill_mckee(pattern, symmetric_mode=True), dtype=np.int32)


def locality_score(W, perm=None, reach=None, sample=None):
    """Fraction of stored entries whose two vertices are at most `reach` positions apart in the
    given order (perm[new] = old; None = the graph's own order): a proxy for how many neighbour
    gathers find their row in the L2 of the XCD that sweeps that index range."""
    W = sparse.csr_matrix(W)
    if W.nnz == 0:
        return 1.0
    if reach is None:
        reach = min(8192, max(64, W.shape[0] // 64))  # ~ rows of a 64-signal panel one L2 holds
    if sample is not None and W.nnz > sample:  # every stride-th stored entry
        pos = np.arange(0, W.nnz, W.nnz // sample, dtype=np.int64)
        rows = np.searchsorted(W.indptr, pos, side="right") - 1
        cols = W.indices[pos]
    else:
        coo = W.tocoo()
        rows, cols = coo.row, coo.col
    if perm is None:
        r, c = rows, cols
    else:
        inv = np.empty(W.shape[0], dtype=np.int64)
        inv[np.asarray(perm, dtype=np.int64)] = np.arange(W.shape[0])
        r, c = inv[rows], inv[cols]
    return float(np.mean(np.abs(r.astype(np.int64) - c.astype(np.int64)) <= reach))


def expander_like(W, seeds=12):
    """True when balls around sample vertices grow like in a random graph: the number of NEW vertices at distance 3
    is about (mean degree) x the number at distance 2 - Erdos-Renyi, block models, small-world graphs - instead of
    the r^(d-1) of a graph embedded in a few dimensions (k-NN graphs, meshes: a ratio of 1.5-2.5).  No vertex order
    gives such a graph locality, so reverse Cuthill-McKee (a host algorithm, ~1 s at 10M entries) is not worth
    running on it.  Looks at a few hundred rows of the CSR arrays only; `W` need not be validated."""
    W = W if sparse.isspmatrix_csr(W) else sparse.csr_matrix(W)
    N = W.shape[0]
    if N < 64 or W.nnz == 0:
        return False
    indptr, indices = W.indptr, W.indices
    mean_deg = W.nnz / N
    ratios = []
    for s in np.linspace(0, N - 1, seeds).astype(np.int64):
        ball = frontier = np.array([s], dtype=np.int64)
        sizes = []
        for _ in range(3):
            if frontier.size == 0 or frontier.size > 20000:
                break
            nbrs = np.unique(np.concatenate([indices[indptr[v]:indptr[v + 1]] for v in frontier]).astype(np.int64))
            nbrs = nbrs[(nbrs >= 0) & (nbrs < N)]
            new = np.setdiff1d(nbrs, ball, assume_unique=True)
            ball = np.union1d(ball, new)
            frontier = new
            sizes.append(new.size)
        if len(sizes) == 3 and sizes[1] > 0:
            ratios.append(sizes[2] / sizes[1])
    if len(ratios) < max(3, seeds // 3):
        return False
    return mean_deg >= 4 and float(np.median(ratios)) > 0.5 * mean_deg


def auto_order(W, coords=None, device=0, ctx=None):
    """The internal order `reorder='auto'` picks: Morton order when coordinates exist, otherwise
    reverse Cuthill-McKee - but only if it beats the graph's own order on `locality_score`
    (block-structured graphs such as a sorted SBM are already local; RCM would scramble them)."""
    has_coords = _curve_coords(coords, W.shape[0])
    if not has_coords and expander_like(W):
        return None  # a random-like graph: no order helps, skip the reverse Cuthill-McKee pass
    perm = locality_order(W, coords, device=device, ctx=ctx)
    if perm is None:
        return None
    # (scored on a sample of the entries: coordinates may be a plotting layout unrelated to the edges)
    if locality_score(W, perm, sample=200000) < locality_score(W, None, sample=200000) + 0.05:
        return None
    return perm


class _SolverRun:
    """The stopping rule going into, and the outputs coming out of, one call of a FISTA solver entry point
    (gspx_tikhonov_simplex_dev, gspx_prox_tv_dev): `rule` = rtol, atol, dtol, xtol (None -> -1.0, off) and maxit,
    `outputs` = niter, crit, the objective sequence and the device time, in the order both entry points take them."""
    CRITERIA = {1: "ATOL", 2: "DTOL", 3: "RTOL", 4: "XTOL", 5: "MAXIT"}

    def __init__(self, rtol, atol, dtol, xtol, maxit):
        maxit = int(maxit)
        self.rule = tuple(-1.0 if v is None else float(v) for v in (rtol, atol, dtol, xtol)) + (maxit,)
        self.obj = np.zeros(max(maxit, 0) + 1, dtype=np.float64)
        self.niter, self.crit, self.ms = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_double(0)
        self.outputs = (ctypes.byref(self.niter), ctypes.byref(self.crit), _capi.ptr(self.obj), ctypes.byref(self.ms))

    def info(self):
        n = int(self.niter.value)
        return {"niter": n, "crit": self.CRITERIA.get(self.crit.value), "objective": self.obj[:n + 1].copy(),
                "ms": self.ms.value}


def _float64_device_graph(G):
    """The float64 device graph of G: a pygsp_amd graph's own, or the plugin's for a reference pygsp graph."""
    if hasattr(G, "device_graph"):
        return G.device_graph(np.float64)
    from . import plugin
    return plugin.device_graph_for(G, dtype=np.float64)


def _refuse_unknown_keywords(function, kwargs, known):
    unknown = sorted(set(kwargs) - set(known))
    if unknown:
        raise TypeError("{}() got unexpected keyword argument(s) {}".format(
            function, ", ".join(repr(k) for k in unknown)))


class DeviceGraph:
    """Device-resident Laplacian (gspx_graph): built on the GPU from W, or uploaded as L."""

    def __init__(self, handle, ctx, N, dtype):
        self._h = handle
        self.ctx = ctx
        self.N = int(N)
        self.dtype = np.dtype(dtype)

    # ---- construction --------------------------------------------------------------------------
    @classmethod
    def from_w(cls, W, lap_type="combinatorial", dtype=np.float64, perm=None, ctx=None):
        """graph.py:510-630 on device.  W must be symmetric (undirected)."""
        ctx = ctx or default_context()
        lap = _lap_code(lap_type)
        W = _canonical_csr(W)
        data = W.data
        if data.dtype not in (np.float32, np.float64):
            data = data.astype(np.float64)  # int64 adjacency (ER/SBM) -> float64, as scipy does
        data = np.ascontiguousarray(data)
        p = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
        h = ctypes.c_void_p()
        ctx.call(_capi.load().gspx_graph_create_from_w,
            ctx._h, W.shape[0], W.nnz, _capi.ptr(W.indptr), _capi.ptr(W.indices), _capi.ptr(data),
            _capi.dtype_code(data.dtype), lap, _capi.dtype_code(dtype), _capi.ptr(p),
            ctypes.byref(h))
        return cls(h, ctx, W.shape[0], dtype)

    ORDER_MODES = {"none": 0, None: 0, False: 0, "auto": 1, "morton": 2, "hilbert": 3}

    @classmethod
    def setup(cls, W, lap_type="combinatorial", dtype=np.float64, coords=None, order="auto", ctx=None):
        """Graph set-up in one device call (gspx_graph_setup): W - a scipy CSR matrix, NOT checked on the host - is
        uploaded once, validated, inspected (NaN / inf / negative / zero / diagonal entries, symmetry), given its
        internal vertex order (curve order of `coords`: 'auto' / 'morton' / 'hilbert' / 'none', or a permutation
        array) and turned into the device Laplacian.  Returns (DeviceGraph or None, report): None when the graph
        is directed or stores explicit zeros - the caller prepares W on the host (graph.py:613-616) and uses
        from_w.  Raises ValueError for NaN / inf entries (the reference's messages) and for a non-canonical CSR."""
        ctx = ctx or default_context()
        lap = _lap_code(lap_type)
        if not sparse.isspmatrix_csr(W):
            W = sparse.csr_matrix(W)
        N, data = W.shape[0], W.data
        indptr, indices = _int32_csr(W)
        if data.dtype == np.float32:
            code = _capi.F32
        elif data.dtype == np.float64:
            code = _capi.F64
        elif data.dtype == np.int64:
            code = 2  # int64 adjacency (ER / SBM): converted on the device
        else:
            data, code = data.astype(np.float64), _capi.F64
        c = np.ascontiguousarray
        mode, xy, d, perm_in = cls._order_args(N, coords, order)
        report = np.zeros(12, dtype=np.int64)
        h = ctypes.c_void_p()
        ctx.call(_capi.load().gspx_graph_setup,
            ctx._h, N, W.nnz, _capi.ptr(c(indptr)), _capi.ptr(c(indices)), _capi.ptr(c(data)), code, lap,
            _capi.dtype_code(dtype), _capi.ptr(xy), d, mode, _capi.ptr(perm_in), _capi.ptr(report), ctypes.byref(h))
        return (cls(h, ctx, N, dtype) if h.value else None), cls._setup_report(report)

    @classmethod
    def _order_args(cls, N, coords, order):
        """(order_mode, coordinates or None, their dimension, permutation or None) of the set-up calls."""
        perm_in, xy, d = None, None, 0
        if isinstance(order, np.ndarray) or isinstance(order, (list, tuple)):
            perm_in, mode = np.ascontiguousarray(order, dtype=np.int32), 4
        else:
            mode = cls.ORDER_MODES[order]
        if mode in (1, 2, 3):
            if _curve_coords(coords, N) and N >= 4096:
                xy = np.asarray(coords)
                if xy.shape[1] > 64:  # the set-up takes up to 64 columns; a curve reads the first two or three
                    xy = xy[:, :3]
                xy = np.ascontiguousarray(xy, dtype=np.float64)
                d = xy.shape[1]
            else:
                mode = 0
        return mode, xy, d, perm_in

    @staticmethod
    def _setup_report(report):
        return {"nan": int(report[0]), "inf": int(report[1]), "negative": int(report[2]), "zeros": int(report[3]),
                "self_loops": int(report[4]), "asymmetric": int(report[5]), "reordered": bool(report[7]),
                "locality_own": report[8] / 1e9, "locality_curve": report[9] / 1e9, "built": report[10] == 0,
                "setup_ms": report[11] / 1e3}

    @classmethod
    def setup_from(cls, adjacency, lap_type="combinatorial", dtype=np.float64, coords=None, order="auto"):
        """The same set-up for a DeviceAdjacency - the W a device builder (knn_graph / radius_graph / sbm_graph with
        keep_on_device=True) left on the device: nothing is downloaded or uploaded (gspx_graph_setup_from_knn)."""
        lap = _lap_code(lap_type)
        N = adjacency.shape[0]
        mode, xy, d, perm_in = cls._order_args(N, coords, order)
        report = np.zeros(12, dtype=np.int64)
        h = ctypes.c_void_p()
        adjacency.ctx.call(_capi.load().gspx_graph_setup_from_knn,
            adjacency._h, lap, _capi.dtype_code(dtype), _capi.ptr(xy), d, mode, _capi.ptr(perm_in), _capi.ptr(report),
            ctypes.byref(h))
        return (cls(h, adjacency.ctx, N, dtype) if h.value else None), cls._setup_report(report)

    def lmax_bounds(self):
        """(max W, max dw, max (dw_i + dw_j) over entries, max (dw_i + (W dw)_i / dw_i)) taken on the device while W
        was there (gspx_graph_lmax_bounds), or None when the graph carries none."""
        out = np.zeros(4)
        try:
            _capi.check(_capi.load().gspx_graph_lmax_bounds(self._h, _capi.ptr(out)))
        except ValueError:
            return None
        return out

    def components(self, labels=True):
        """Connected components of the graph's undirected pattern, labelled on the device (gspx_graph_components):
        (n, labels or None, report).  labels: int32, one per vertex in the caller's order, components numbered
        0 .. n - 1 by their smallest vertex - the numbering of scipy's connected_components(W, directed=False);
        labels=False asks for the count alone and moves nothing but it.  report: {'rounds' (hook rounds run),
        'round_cap' (the library's own bound for this N, never exceeded), 'kernel_ms' (device time)}."""
        lib = _capi.load()
        n, rounds, cap, ms = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_double(0)
        out = np.empty(self.N, dtype=np.int32) if labels else None
        self.ctx.call(lib.gspx_graph_components, self._h, _capi.ptr(out), ctypes.byref(n), ctypes.byref(rounds),
                      ctypes.byref(ms))
        _capi.check(lib.gspx_components_round_cap(self.N, ctypes.byref(cap)))
        return int(n.value), out, {"rounds": rounds.value, "round_cap": cap.value, "kernel_ms": ms.value}

    def download_perm(self):
        """The internal vertex order (perm[new] = old), or None when the graph keeps its own order."""
        perm = np.empty(self.N, dtype=np.int32)
        try:
            _capi.check(_capi.load().gspx_graph_download_perm(self._h, _capi.ptr(perm)))
        except ValueError:
            return None
        return perm

    @classmethod
    def from_l(cls, L, dtype=np.float64, perm=None, ctx=None):
        ctx = ctx or default_context()
        L = _canonical_csr(L)
        data = L.data
        if data.dtype not in (np.float32, np.float64):
            data = data.astype(np.float64)
        data = np.ascontiguousarray(data)
        p = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
        h = ctypes.c_void_p()
        ctx.call(_capi.load().gspx_graph_create_from_l,
            ctx._h, L.shape[0], L.nnz, _capi.ptr(L.indptr), _capi.ptr(L.indices), _capi.ptr(data),
            _capi.dtype_code(data.dtype), _capi.dtype_code(dtype), _capi.ptr(p), ctypes.byref(h))
        return cls(h, ctx, L.shape[0], dtype)

    def destroy(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):
                _capi.load().gspx_graph_destroy(self._h)
            self._h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.destroy()
        except Exception:
            pass

    def _i64(self, fn):
        v = ctypes.c_int64(0)
        _capi.check(fn(self._h, ctypes.byref(v)))
        return v.value

    @property
    def nnz_l(self):
        return self._i64(_capi.load().gspx_graph_nnz_l)

    @property
    def nnz_internal(self):
        return self._i64(_capi.load().gspx_graph_nnz_internal)

    @property
    def build_ms(self):
        v = ctypes.c_double(0)
        _capi.check(_capi.load().gspx_graph_build_ms(self._h, ctypes.byref(v)))
        return v.value

    def download_l(self):
        """Canonical Laplacian as scipy CSR in the graph's own vertex order."""
        nnz = self.nnz_l
        indptr = np.empty(self.N + 1, dtype=np.int32)
        indices = np.empty(nnz, dtype=np.int32)
        data = np.empty(nnz, dtype=self.dtype)
        _capi.check(_capi.load().gspx_graph_download_l(self._h, _capi.ptr(indptr),
                                                       _capi.ptr(indices), _capi.ptr(data)))
        return sparse.csr_matrix((data, indices, indptr), shape=(self.N, self.N))

    def download_dw(self):
        dw = np.empty(self.N, dtype=self.dtype)
        _capi.check(_capi.load().gspx_graph_download_dw(self._h, _capi.ptr(dw)))
        return dw

    def lanczos_lmax(self, max_iter=60, tol=5e-4):
        """Largest Ritz value of L after a device Lanczos run: (value, iterations).  Raises ValueError
        when the step budget runs out before the residual criterion is met, as Graph.estimate_lmax
        does on ArpackNoConvergence (graph.py:918-919): a value from below lambda_max would put part of
        the spectrum outside [-1, 1], where the Chebyshev recurrence diverges."""
        v = ctypes.c_double(0)
        it = ctypes.c_int(0)
        ok = ctypes.c_int(0)
        self.ctx.call(_capi.load().gspx_lanczos_lmax, self._h, int(max_iter), float(tol), ctypes.byref(v),
                                                   ctypes.byref(it), ctypes.byref(ok))
        if not ok.value:
            raise ValueError("The Lanczos method did not converge. Try to use bounds.")
        return v.value, it.value

    # ---- the hot path -------------------------------------------------------------------------
    def cheby_filter(self, coeffs, x, lmax, mode=_capi.ANALYSIS):
        """Host arrays in / out.  coeffs: (Nf, M) float64.
        analysis:  x (N, Nsig)      -> (Nf, N, Nsig)
        synthesis: x (Nf, N, Nsig)  -> (N, Nsig)
        Returns (y, kernel_ms)."""
        c = _coeff_matrix(coeffs)
        Nf, M = c.shape
        x = np.ascontiguousarray(x, dtype=self.dtype)
        if mode == _capi.ANALYSIS:
            if x.ndim != 2 or x.shape[0] != self.N:
                raise ValueError("analysis input must be (N, Nsig), got {}".format(x.shape))
            nsig = x.shape[1]
            y = np.empty((Nf, self.N, nsig), dtype=self.dtype)
        else:
            if x.ndim != 3 or x.shape[0] != Nf or x.shape[1] != self.N:
                raise ValueError("synthesis input must be (Nf, N, Nsig), got {}".format(x.shape))
            nsig = x.shape[2]
            y = np.empty((self.N, nsig), dtype=self.dtype)
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_cheby_filter,
            self._h, float(lmax), Nf, M, _capi.ptr(c), nsig, _capi.ptr(x), _capi.ptr(y), mode,
            ctypes.byref(ms))
        return y, ms.value

    def cheby_filter_dev(self, coeffs, x_ptr, y_ptr, nsig, lmax, mode=_capi.ANALYSIS):
        """Device pointers in / out (ints).  Returns device milliseconds of the whole call."""
        c = _coeff_matrix(coeffs)
        Nf, M = c.shape
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_cheby_filter_dev,
            self._h, float(lmax), Nf, M, _capi.ptr(c), int(nsig), ctypes.c_void_p(x_ptr),
            ctypes.c_void_p(y_ptr), mode, ctypes.byref(ms))
        return ms.value

    def cheby_sqnorms_dev(self, coeffs, x_ptr, nsig, lmax):
        """Squared column norms of the bank `coeffs` (Nf, M) applied to the device signals at x_ptr (N x nsig):
        ((Nf, nsig) float64 host array of ||p_f(L) x_j||^2, device milliseconds of the call), without the filtered
        outputs (gspx_cheby_sqnorms_dev)."""
        c = _coeff_matrix(coeffs)
        Nf, M = c.shape
        out = np.zeros((Nf, int(nsig)))
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_cheby_sqnorms_dev, self._h, float(lmax), Nf, M, _capi.ptr(c), int(nsig),
                      ctypes.c_void_p(x_ptr), _capi.ptr(out), ctypes.byref(ms))
        return out, ms.value

    def cheby_moments_dev(self, x_ptr, nsig, lmax, M):
        """Chebyshev self-moments of the device signals at x_ptr (N x nsig): ((M, nsig) float64 host array of
        x_j^T T_k(Lt) x_j for k < M, device milliseconds of the call) from M // 2 recurrence steps
        (gspx_cheby_moments_dev)."""
        out = np.zeros((int(M), int(nsig)))
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_cheby_moments_dev, self._h, float(lmax), int(M), int(nsig),
                      ctypes.c_void_p(x_ptr), _capi.ptr(out), ctypes.byref(ms))
        return out, ms.value

    def cheby_moments(self, x, lmax, M):
        """cheby_moments_dev of a host array (N, nsig): uploaded in the graph's dtype, freed afterwards."""
        x = self._signals(x)
        with self.ctx._temporaries() as t:
            bx = t.alloc(x.nbytes)
            if x.nbytes:
                bx.upload(x)
            return self.cheby_moments_dev(bx.ptr, x.shape[1], lmax, M)

    def cheby_cross_moments_dev(self, x_ptr, z_ptr, nsig, nf, lmax, M):
        """Chebyshev cross-moments of the device signals at x_ptr (N x nsig) with the nf planes at z_ptr
        (nf x N x nsig): ((nf, M, nsig) float64 host array of sum_n z[f][n][j] (T_k(Lt) x)[n][j] for k < M, device
        milliseconds of the call) from M - 1 recurrence steps (gspx_cheby_cross_moments_dev)."""
        out = np.zeros((int(nf), int(M), int(nsig)))
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_cheby_cross_moments_dev, self._h, float(lmax), int(M), int(nsig),
                      ctypes.c_void_p(x_ptr), int(nf), ctypes.c_void_p(z_ptr), _capi.ptr(out), ctypes.byref(ms))
        return out, ms.value

    def cheby_cross_moments(self, x, z, lmax, M):
        """cheby_cross_moments_dev of host arrays x (N, nsig) and z (nf, N, nsig): uploaded in the graph's dtype,
        freed afterwards."""
        x = self._signals(x)
        z = np.ascontiguousarray(z, dtype=self.dtype)
        if z.ndim != 3 or z.shape[0] < 1 or z.shape[1:] != x.shape:
            raise ValueError("z must be (Nf, N, Nsig) with x's N and Nsig, got {} for x {}".format(z.shape, x.shape))
        with self.ctx._temporaries() as t:
            bx, bz = t.alloc(x.nbytes), t.alloc(z.nbytes)
            if x.nbytes:
                bx.upload(x)
                bz.upload(z)
            return self.cheby_cross_moments_dev(bx.ptr, bz.ptr, x.shape[1], z.shape[0], lmax, M)

    def cheby_conv_dev(self, theta, x_ptr, y_ptr, batch, lmax):
        """The Chebyshev graph convolution y[n, b, :] = sum_k (T_k(Lt) x)[n, b, :] theta[k] of the device signals at
        x_ptr (N x batch*Fin) into y_ptr (N x batch*Fout), theta (M, Fin, Fout) float64 on the host, a plain sum
        (gspx_cheby_conv_dev).  Returns device milliseconds of the call."""
        th = _theta_stack(theta)
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_cheby_conv_dev, self._h, float(lmax), th.shape[0], th.shape[1], th.shape[2],
                      _capi.ptr(th), int(batch), ctypes.c_void_p(x_ptr), ctypes.c_void_p(y_ptr), ctypes.byref(ms))
        return ms.value

    def cheby_conv(self, theta, x, lmax):
        """cheby_conv_dev of a host array x (N, B, Fin): ((N, B, Fout) array in the graph's dtype, device
        milliseconds); uploaded in the graph's dtype, freed afterwards."""
        th = _theta_stack(theta)
        x = self._samples(x, th.shape[1])
        y = np.zeros((self.N, x.shape[1], th.shape[2]), dtype=self.dtype)
        with self.ctx._temporaries() as t:
            bx, by = t.alloc(x.nbytes), t.alloc(y.nbytes)
            if x.nbytes:
                bx.upload(x)
            ms = self.cheby_conv_dev(th, bx.ptr, by.ptr, x.shape[1], lmax)
            if y.nbytes:
                y = by.download(y.shape, self.dtype)
        return y, ms

    def cheby_cross_grams_dev(self, x_ptr, z_ptr, batch, fin, fout, lmax, M):
        """The cross-Grams of the recurrence on the device signals at x_ptr (N x batch*fin) with those at z_ptr
        (N x batch*fout): ((M, fin, fout) float64 host array of sum_{n, b} (T_k(Lt) x)[n, b, i] z[n, b, o], device
        milliseconds of the call) from M - 1 recurrence steps (gspx_cheby_cross_grams_dev)."""
        out = np.zeros((max(int(M), 0), max(int(fin), 0), max(int(fout), 0)))
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_cheby_cross_grams_dev, self._h, float(lmax), int(M), int(fin), int(fout),
                      int(batch), ctypes.c_void_p(x_ptr), ctypes.c_void_p(z_ptr), _capi.ptr(out), ctypes.byref(ms))
        return out, ms.value

    def cheby_cross_grams(self, x, z, lmax, M):
        """cheby_cross_grams_dev of host arrays x (N, B, Fin) and z (N, B, Fout): uploaded in the graph's dtype, freed
        afterwards."""
        x = self._samples(x)
        z = self._samples(z)
        if z.shape[1] != x.shape[1]:
            raise ValueError("x and z must hold the same samples, got {} and {}".format(x.shape, z.shape))
        with self.ctx._temporaries() as t:
            bx, bz = t.alloc(x.nbytes), t.alloc(z.nbytes)
            if x.nbytes:
                bx.upload(x)
                bz.upload(z)
            return self.cheby_cross_grams_dev(bx.ptr, bz.ptr, x.shape[1], x.shape[2], z.shape[2], lmax, M)

    def cheby_laplacian_grad_dev(self, coeffs, x_ptr, z_ptr, nsig, lmax, src_ptr=None, dst_ptr=None, n_pairs=0,
                                 gdiag_ptr=None, goff_ptr=None):
        """The derivative of a Chebyshev filter's output with respect to the Laplacian's entries, on device pointers
        (gspx_cheby_laplacian_grad_dev): coeffs (Nf, M) float64 on the host, the signals at x_ptr (N x nsig), the Nf
        cotangent planes at z_ptr (Nf x N x nsig); src_ptr / dst_ptr: device int32 arrays of n_pairs vertices, None
        for the graph's own edge list; gdiag_ptr (N doubles) and goff_ptr (one double per pair) are device buffers that
        are overwritten, either may be None.  Returns device milliseconds of the call."""
        c = _coeff_matrix(coeffs)
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_cheby_laplacian_grad_dev, self._h, float(lmax), c.shape[0], c.shape[1],
                      _capi.ptr(c), int(nsig), ctypes.c_void_p(x_ptr), ctypes.c_void_p(z_ptr), int(n_pairs),
                      ctypes.c_void_p(src_ptr), ctypes.c_void_p(dst_ptr), ctypes.c_void_p(gdiag_ptr),
                      ctypes.c_void_p(goff_ptr), ctypes.byref(ms))
        return ms.value

    def cheby_laplacian_grad(self, coeffs, x, z, lmax, pairs=None, need_diag=True):
        """cheby_laplacian_grad_dev of host arrays x (N, nsig) and z (Nf, N, nsig), uploaded in the graph's dtype and
        freed afterwards.  pairs: a (2, P) integer array of vertex pairs, or None for the graph's own edge list.
        Returns (gdiag (N,) float64 or None without need_diag, goff (P,) float64, device milliseconds)."""
        c = _coeff_matrix(coeffs)
        x = self._signals(x)
        z = np.ascontiguousarray(z, dtype=self.dtype)
        if z.ndim != 3 or z.shape[0] != c.shape[0] or z.shape[1:] != x.shape:
            raise ValueError("z must be (Nf, N, Nsig) with the coefficients' Nf and x's N and Nsig, got {} for x {}"
                             .format(z.shape, x.shape))
        if pairs is not None:
            pairs = np.ascontiguousarray(pairs, dtype=np.int32)
            if pairs.ndim != 2 or pairs.shape[0] != 2:
                raise ValueError("pairs must be (2, P), got {}".format(pairs.shape))
        P = self.n_edges() if pairs is None else pairs.shape[1]
        with self.ctx._temporaries() as t:
            bx, bz = t.alloc(x.nbytes), t.alloc(z.nbytes)
            if x.nbytes:
                bx.upload(x)
                bz.upload(z)
            bp = t.upload(pairs) if pairs is not None and P else None
            bd = t.alloc(8 * self.N) if need_diag else None
            bo = t.alloc(8 * P)
            ms = self.cheby_laplacian_grad_dev(
                c, bx.ptr, bz.ptr, x.shape[1], lmax, None if pairs is None else (bp.ptr if bp else bo.ptr),
                None if pairs is None else (bp.ptr + 4 * P if bp else bo.ptr), P, bd.ptr if bd else None, bo.ptr)
            gdiag = bd.download((self.N,), np.float64) if need_diag and self.N else (np.zeros(0) if need_diag else None)
            goff = bo.download((P,), np.float64) if P else np.zeros(0)
        return gdiag, goff, ms

    def _samples(self, x, features=None):
        x = np.ascontiguousarray(x, dtype=self.dtype)
        if x.ndim != 3 or x.shape[0] != self.N or (features is not None and x.shape[2] != features):
            raise ValueError("input must be (N, B, {}), got {}".format("F" if features is None else features, x.shape))
        return x

    def tune_placement(self, coeffs, x_ptr, y_ptr, nsig, lmax, candidates=6, stride_mb=0):
        """Draw `candidates` physical backings for the context's streamed workspaces and keep the one on which THIS call
        (the arguments of cheby_filter_dev, one filter) runs fastest (gspx_ctx_tune_placement; on MI355X the same call
        runs 0.54-0.60 of 8 TB/s depending on which pages back the work panels).  Returns {"launch_ms": [per
        candidate], "kept": index}; y holds the call's result.  Results are bit-identical whichever backing is kept.
        stride_mb > 0: a pad of that size is held before every further draw, so the candidates sample the card's
        memory at that stride (fast and slow pages come in zones of tens of GB); candidates that no longer fit read 0."""
        c = np.ascontiguousarray(np.asarray(coeffs, dtype=np.float64).ravel())
        out = np.zeros(int(candidates) + 1)
        self.ctx.call(_capi.load().gspx_ctx_tune_placement, self._h, float(lmax), int(c.size), _capi.ptr(c), int(nsig),
                      ctypes.c_void_p(x_ptr), ctypes.c_void_p(y_ptr), int(candidates), int(stride_mb), _capi.ptr(out))
        return {"launch_ms": [float(v) for v in out[:-1]], "kept": int(out[-1])}

    def bench_step_mix(self, coeffs, x_ptr, y_ptr, nsig, lmax, mode=1):
        """CALIBRATION, not a filter: the launches cheby_filter_dev(coeffs, ...) would make with the row products
        removed from every wide k_step_tile launch (gspx_bench_step_mix; mode 2: the barriers of a pass too).  y
        receives numbers without meaning.  Returns ctx.last_timing() of that call."""
        c = np.ascontiguousarray(np.asarray(coeffs, dtype=np.float64).ravel())
        self.ctx.call(_capi.load().gspx_bench_step_mix, self._h, float(lmax), int(c.size), _capi.ptr(c), int(nsig),
                      ctypes.c_void_p(x_ptr), ctypes.c_void_p(y_ptr), int(mode))
        return self.ctx.last_timing()

    # ---- polynomial programs (Newton and product forms of one filter) -----------------------------
    def _signals(self, x):
        x = np.ascontiguousarray(x, dtype=self.dtype)
        if x.ndim != 2 or x.shape[0] != self.N:
            raise ValueError("input must be (N, Nsig), got {}".format(x.shape))
        return x

    def newton_filter(self, nodes, dcoef, x, lmax):
        """Newton-form evaluation (single filter): host arrays in/out, x (N, Nsig) -> (N, Nsig)."""
        nodes = np.ascontiguousarray(nodes, dtype=np.float64)
        dcoef = np.ascontiguousarray(dcoef, dtype=np.float64)
        if dcoef.size != nodes.size + 1:
            raise ValueError("need K nodes and K+1 coefficients")
        x = self._signals(x)
        y = np.empty_like(x)
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_newton_filter,
            self._h, float(lmax), int(nodes.size), _capi.ptr(nodes), _capi.ptr(dcoef), x.shape[1],
            _capi.ptr(x), _capi.ptr(y), ctypes.byref(ms))
        return y, ms.value

    def newton_filter_dev(self, nodes, dcoef, x_ptr, y_ptr, nsig, lmax):
        nodes = np.ascontiguousarray(nodes, dtype=np.float64)
        dcoef = np.ascontiguousarray(dcoef, dtype=np.float64)
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_newton_filter_dev,
            self._h, float(lmax), int(nodes.size), _capi.ptr(nodes), _capi.ptr(dcoef), int(nsig),
            ctypes.c_void_p(x_ptr), ctypes.c_void_p(y_ptr), ctypes.byref(ms))
        return ms.value

    def program_filter(self, program, x, lmax, old_is_x=False):
        """A polynomial program (gspx_poly_program; filters.cheb_to_product builds the product form's): host arrays in /
        out, x (N, Nsig) -> (N, Nsig).  program: (S, 3) rows of (scale, beta, gamma)."""
        S, scale, beta, gamma = _program_columns(program)
        x = self._signals(x)
        y = np.empty_like(x)
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_poly_program, self._h, float(lmax), S, _capi.ptr(scale), _capi.ptr(beta),
                      _capi.ptr(gamma), int(bool(old_is_x)), x.shape[1], _capi.ptr(x), _capi.ptr(y), ctypes.byref(ms))
        return y, ms.value

    def program_filter_dev(self, program, x_ptr, y_ptr, nsig, lmax, old_is_x=False):
        S, scale, beta, gamma = _program_columns(program)
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_poly_program_dev, self._h, float(lmax), S, _capi.ptr(scale), _capi.ptr(beta),
                      _capi.ptr(gamma), int(bool(old_is_x)), int(nsig), ctypes.c_void_p(x_ptr), ctypes.c_void_p(y_ptr),
                      ctypes.byref(ms))
        return ms.value

    # ---- gather tiles (the LDS-staged recurrence step, k_step_tile) --------------------------------
    def download_internal(self):
        """(rowptr, col) of the engine's internal padded CSR (internal vertex order)."""
        rp = np.empty(self.N + 1, dtype=np.int32)
        col = np.empty(self.nnz_internal, dtype=np.int32)
        _capi.check(_capi.load().gspx_graph_download_internal(self._h, _capi.ptr(rp), _capi.ptr(col)))
        return rp, col

    def enable_gather_tiles(self):
        """Build (numpy) and upload the one-level row tiles of the LDS-staged recurrence step
        (k_step_tile): per 64-row block the distinct rows it gathers, per entry a 16-bit position in
        that list.  With them (and option "tile_gather" = 1, the default) single-filter Chebyshev
        filtering stages the gathered panel in LDS.  Returns tile statistics."""
        from . import tiling
        rp, col = self.download_internal()
        t = tiling.build_tiles(rp, col, self.N, 64)
        lidx = t["lidx1"].copy()
        lidx[lidx == tiling.PAD] = 0  # pads carry the value 0: any valid position will do
        c = np.ascontiguousarray
        stats = np.zeros(3, dtype=np.int64)
        _capi.check(_capi.load().gspx_graph_set_gather_tiles(
            self._h, 64, t["nb"], _capi.ptr(c(t["s1ptr"])), _capi.ptr(c(t["s1rows"])), _capi.ptr(c(lidx)),
            _capi.ptr(stats)))
        return {"nb": t["nb"], "max_n1": t["max_n1"], "mean_n1": t["mean_n1"],
                "slow_blocks": int(stats[1]), "lds_bytes": int(stats[2])}

    def build_gather_tiles(self):
        """The same tiles as enable_gather_tiles(), computed on the device (gspx_graph_build_gather_tiles):
        milliseconds instead of half a second of numpy at N = 1M."""
        stats = np.zeros(4, dtype=np.int64)
        self.ctx.call(_capi.load().gspx_graph_build_gather_tiles, self._h, _capi.ptr(stats))
        nb = int(stats[0])
        return {"nb": nb, "mean_n1": float(stats[3]) / max(nb, 1), "slow_blocks": int(stats[1]),
                "lds_bytes": int(stats[2])}

    def auto_gather_tiles(self, min_vertices=32768):
        """enable_gather_tiles() when it pays: a large graph whose internal order is local (nearly
        every 64-row block's gather set fits its LDS tile).  Returns the statistics (with
        "enabled") or None when the graph is too small to bother."""
        if self.N < min_vertices:
            return None
        st = self.build_gather_tiles()  # on the device: cheap enough to just try
        st["enabled"] = st["slow_blocks"] * 50 <= st["nb"]
        if not st["enabled"]:
            self.disable_gather_tiles()
        return st

    def disable_gather_tiles(self):
        _capi.check(_capi.load().gspx_graph_set_gather_tiles(self._h, 0, 0, None, None, None, None))

    # ---- operators that reuse the device CSR (include/gspx_ext.h) ----------------
    # Host arrays in / out; the *_dev variants take device pointers.
    def _panel(self, x, rows, what):
        x = np.asarray(x)
        one_d = x.ndim == 1
        # (the columns spelled out: reshape(0, -1) cannot infer them for the empty edge signal of an edgeless graph)
        x2 = np.ascontiguousarray(x.reshape(x.shape[0], int(np.prod(x.shape[1:]))), dtype=self.dtype)
        if x2.shape[0] != rows:
            raise ValueError("{}: first dimension must be {}, got {}".format(what, rows, x.shape))
        return x2, one_d

    def _panel_op(self, x, rows_in, rows_out, fn, what):
        """fn(x_ptr, y_ptr, nsig) on the uploaded panel x, (rows_in[, Nsig]) -> (rows_out[, Nsig])."""
        x2, one_d = self._panel(x, rows_in, what)
        with self.ctx._temporaries() as t:
            bx, by = t.upload(x2), t.alloc(rows_out * x2.shape[1] * self.dtype.itemsize)
            fn(bx.ptr, by.ptr, x2.shape[1])
            y = by.download((rows_out, x2.shape[1]), self.dtype)
        return y[:, 0] if one_d else y

    def laplacian_apply_dev(self, x_ptr, y_ptr, nsig):
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_laplacian_apply_dev,
            self._h, int(nsig), ctypes.c_void_p(x_ptr), ctypes.c_void_p(y_ptr), ctypes.byref(ms))
        return ms.value

    def laplacian_apply(self, x):
        """L x for x of shape (N,) or (N, Nsig)."""
        return self._panel_op(x, self.N, self.N, self.laplacian_apply_dev, "laplacian_apply")

    def dirichlet_energy_dev(self, x_ptr, nsig):
        gram = np.zeros((int(nsig), int(nsig)), dtype=np.float64)
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_dirichlet_energy_dev,
            self._h, int(nsig), ctypes.c_void_p(x_ptr), _capi.ptr(gram), ctypes.byref(ms))
        return gram, ms.value

    def dirichlet_energy(self, x):
        """x^T L x: a float for one signal, the (Nsig, Nsig) matrix x.T @ (L @ x) for a panel
        (what Graph.dirichlet_energy returns for 2-D input, graph.py:701-702)."""
        x2, one_d = self._panel(x, self.N, "dirichlet_energy")
        with self.ctx._temporaries() as t:
            gram, _ = self.dirichlet_energy_dev(t.upload(x2).ptr, x2.shape[1])
        return float(gram[0, 0]) if one_d else gram

    def lanczos_basis(self, x, order, breakdown=0.0):
        """The Krylov stacks of gspx_lanczos_krylov_dev for x (N,) or (N, n), n <= 256, on this float64 graph,
        downloaded: (V (N, order[, n]) in the caller's vertex order, alpha (order[, n]), beta (order[, n]: row 0 is
        ||x||, row k beta_k), steps (Krylov dimension per column; an int for 1-D x)).  A column stops at step k when
        beta_k <= `breakdown`.  For tests at small N."""
        from . import lanczos
        x2, one_d = self._panel(x, self.N, "lanczos_basis")
        V, alpha, beta, steps = lanczos.device_basis(self, x2, order, breakdown)
        if one_d:
            return V[:, :, 0], alpha[:, 0], beta[:, 0], int(steps[0])
        return V, alpha, beta, steps

    # ---- learning (Tikhonov regression and classification) ------------------------------------------
    def tikhonov_cg_dev(self, tau, mask_ptr, y_ptr, x_ptr, nsig, rtol=1e-5, atol=0.0, maxiter=None):
        maxiter = 10 * self.N if maxiter is None else int(maxiter)
        iters = np.zeros(max(int(nsig), 1), dtype=np.int32)
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_tikhonov_cg_dev,
            self._h, float(tau), ctypes.c_void_p(mask_ptr), int(nsig), ctypes.c_void_p(y_ptr),
            ctypes.c_void_p(x_ptr), float(rtol), float(atol), maxiter, _capi.ptr(iters), ctypes.byref(ms))
        return iters[:int(nsig)], ms.value

    def tikhonov_cg(self, tau, mask, y, rtol=1e-5, atol=0.0, maxiter=None):
        """Solve (diag(mask) + tau L) x = mask * y per column by conjugate gradients (scipy's cg
        recurrence and stopping rule).  Returns (x, iterations per column, device ms)."""
        y2, one_d = self._panel(y, self.N, "tikhonov_cg")
        m = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=self.dtype)
        if m.size != self.N:
            raise ValueError("M should be of size [G.n_vertices,]")
        with self.ctx._temporaries() as t:
            bm, by, bx = t.upload(m), t.upload(y2), t.alloc(y2.nbytes)
            iters, ms = self.tikhonov_cg_dev(tau, bm.ptr, by.ptr, bx.ptr, y2.shape[1], rtol, atol, maxiter)
            x = bx.download(y2.shape, self.dtype)
        return (x[:, 0] if one_d else x), iters, ms

    def dirichlet_cg_dev(self, mask_ptr, y_ptr, x_ptr, nsig, rtol=None, atol=0.0, maxiter=None):
        rtol = (1e-10 if self.dtype == np.float64 else 1e-5) if rtol is None else float(rtol)
        maxiter = 10 * self.N if maxiter is None else int(maxiter)
        iters = np.zeros(max(int(nsig), 1), dtype=np.int32)
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_dirichlet_cg_dev,
            self._h, ctypes.c_void_p(mask_ptr), int(nsig), ctypes.c_void_p(y_ptr), ctypes.c_void_p(x_ptr), rtol,
            float(atol), maxiter, _capi.ptr(iters), ctypes.byref(ms))
        return iters[:int(nsig)], ms.value

    def dirichlet_cg(self, mask, y, rtol=None, atol=0.0, maxiter=None):
        """Harmonic extension: x = y on the measured vertices (mask != 0) and L_uu x_u = -L_ul y_l on the others,
        per column by conjugate gradients (gspx_dirichlet_cg_dev); y is read at measured vertices only.  rtol None:
        1e-10 on a float64 graph, 1e-5 on a float32 one; maxiter None: 10 N.  Returns (x, iterations per column,
        device ms)."""
        y2, one_d = self._panel(y, self.N, "dirichlet_cg")
        m = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=self.dtype)
        if m.size != self.N:
            raise ValueError("M should be of size [G.n_vertices,]")
        with self.ctx._temporaries() as t:
            bm, by, bx = t.upload(m), t.upload(y2), t.alloc(y2.nbytes)
            iters, ms = self.dirichlet_cg_dev(bm.ptr, by.ptr, bx.ptr, y2.shape[1], rtol, atol, maxiter)
            x = bx.download(y2.shape, self.dtype)
        return (x[:, 0] if one_d else x), iters, ms

    # ---- reduction (Schur complements of L + shift I) -------------------------------------------------
    def schur_cg_dev(self, shift, mask_ptr, f_ptr, x_ptr, alpha_ptr, nsig, rtol=None, atol=0.0, maxiter=None):
        """gspx_schur_cg_dev on device pointers (x_ptr / alpha_ptr may be None); returns (iterations, device ms)."""
        rtol = (1e-10 if self.dtype == np.float64 else 1e-5) if rtol is None else float(rtol)
        maxiter = 10 * self.N if maxiter is None else int(maxiter)
        iters = np.zeros(max(int(nsig), 1), dtype=np.int32)
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_schur_cg_dev,
            self._h, float(shift), ctypes.c_void_p(mask_ptr), int(nsig), ctypes.c_void_p(f_ptr),
            ctypes.c_void_p(x_ptr), ctypes.c_void_p(alpha_ptr), rtol, float(atol), maxiter, _capi.ptr(iters),
            ctypes.byref(ms))
        return iters[:int(nsig)], ms.value

    def schur_cg(self, shift, mask, f, rtol=None, atol=0.0, maxiter=None):
        """The harmonic extension at a shift: with A = L + shift I, x = f on the kept vertices (mask != 0) and
        A_uu x_u = -A_uk f_k on the others, per column by conjugate gradients (gspx_schur_cg_dev; shift = 0 is
        dirichlet_cg, byte for byte); alpha = A x on the kept rows - the Schur complement applied to f_k - and exact
        zeros elsewhere.  f (N,) or (N, Nsig) is read at kept vertices only.  Defaults as dirichlet_cg.  Returns
        (x, alpha, iterations per column, device ms)."""
        f2, one_d = self._panel(f, self.N, "schur_cg")
        m = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=self.dtype)
        if m.size != self.N:
            raise ValueError("the mask should be of size [G.n_vertices,]")
        with self.ctx._temporaries() as t:
            bm, bf, bx, ba = t.upload(m), t.upload(f2), t.alloc(f2.nbytes), t.alloc(f2.nbytes)
            iters, ms = self.schur_cg_dev(shift, bm.ptr, bf.ptr, bx.ptr, ba.ptr, f2.shape[1], rtol, atol, maxiter)
            x, alpha = bx.download(f2.shape, self.dtype), ba.download(f2.shape, self.dtype)
        return (x[:, 0] if one_d else x), (alpha[:, 0] if one_d else alpha), iters, ms

    def kron(self, ind, shift=0.0, rtol=1e-10, maxiter=None, dense=True, adjacency=False):
        """Kron reduction of A = L + shift I onto the vertices `ind` (gspx_kron_build, float64 graphs): vertex ind[c]
        becomes vertex c.  Returns (Lnew, W, iterations, info): Lnew the dense symmetrised (nk, nk) Schur complement
        (None unless `dense`), W = max(0, -offdiag) as a DeviceAdjacency (None unless `adjacency`), the iteration
        count of every kept vertex's solve, info = {"kernel_ms", "solve_ms", "rows_ms", "finalise_ms"}.  Entries the iteration never reaches are exact
        zeros.  ValueError for an empty, repeated or out-of-range `ind` and when the dense result exceeds the
        context's ws_limit_mb."""
        if self.dtype != np.float64:
            raise ValueError("kron runs on the float64 device graph")
        ind = check_kept(ind, self.N)
        nk = ind.size
        maxiter = 10 * self.N if maxiter is None else int(maxiter)
        iters = np.zeros(nk, dtype=np.int32)
        h, ms = ctypes.c_void_p(), ctypes.c_double(0)
        lnew = W = None
        with self.ctx._temporaries() as t:
            bl = t.alloc(nk * nk * 8) if dense else None
            self.ctx.call(_capi.load().gspx_kron_build, self._h, float(shift), _capi.ptr(ind), nk, float(rtol), maxiter,
                          ctypes.c_void_p(bl.ptr if dense else None), ctypes.byref(h) if adjacency else None,
                          _capi.ptr(iters), ctypes.byref(ms))
            if adjacency:
                W, _, _ = _adjacency(h, self.ctx, nk, True)
            if dense:
                lnew = bl.download((nk, nk), np.float64)
        parts = (ctypes.c_double * 5)()  # (gspx_kron_build leaves its phases where gspx_last_timing reads)
        _capi.check(_capi.load().gspx_last_timing(self.ctx._h, parts))
        return lnew, W, iters, {"kernel_ms": ms.value, "solve_ms": parts[0], "rows_ms": parts[1], "finalise_ms": parts[2]}

    MATCH_METRICS = {"normalized_cut": 0, "weight": 1}

    def match_heavy_edges(self, metric="normalized_cut", max_rounds=None):
        """A maximal matching of heavy edges by handshake rounds on the device (gspx_match_heavy_edges; float64 graphs
        with the combinatorial Laplacian).  Every unmatched vertex proposes to its unmatched neighbour of largest score
        - 'normalized_cut': w_ij (1 / d_i + 1 / d_j), 'weight': w_ij - ties to the smaller vertex index (the caller's
        indices: the internal order plays no part), and mutual proposals are matched.  `max_rounds`: None runs until a
        round matches nothing (a path with monotone weights needs N / 2 rounds); otherwise at most that many rounds,
        the rest stay singletons.  Returns (mate, info): mate int32 (N,), mate[i] == i for a singleton; info =
        {'rounds' (the rounds that matched something), 'pairs', 'singletons', 'kernel_ms'}."""
        if self.dtype != np.float64:
            raise ValueError("match_heavy_edges runs on the float64 device graph")
        if metric not in self.MATCH_METRICS:
            raise ValueError("Unknown metric {!r}: 'normalized_cut' or 'weight'".format(metric))
        if max_rounds is not None and int(max_rounds) < 0:
            raise ValueError("max_rounds must be None or non-negative")
        mate = np.empty(self.N, dtype=np.int32)
        rounds, pairs, ms = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_match_heavy_edges, self._h, self.MATCH_METRICS[metric],
                      -1 if max_rounds is None else int(max_rounds), _capi.ptr(mate), ctypes.byref(rounds),
                      ctypes.byref(pairs), ctypes.byref(ms))
        return mate, {"rounds": int(rounds.value), "pairs": int(pairs.value),
                      "singletons": self.N - 2 * int(pairs.value), "kernel_ms": ms.value}

    def coarsen(self, parent, n_clusters):
        """The coarse adjacency P^T W P without its diagonal for the cluster map `parent` (N ints in [0, n_clusters),
        every cluster non-empty), assembled on the device (gspx_coarsen_build).  Returns (W, info): W a
        DeviceAdjacency under gspx_kron_build's contract (canonical CSR, sorted columns, no diagonal, its transpose
        bit for bit), info = {'kernel_ms', 'build_ms'}.  ValueError for a `parent` of wrong length or out of range."""
        if self.dtype != np.float64:
            raise ValueError("coarsen runs on the float64 device graph")
        parent, n_clusters = check_parent(parent, self.N, n_clusters), int(n_clusters)
        h, ms = ctypes.c_void_p(), ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_coarsen_build, self._h, _capi.ptr(parent), n_clusters, ctypes.byref(h),
                      ctypes.byref(ms))
        W, _, build_ms = _adjacency(h, self.ctx, n_clusters, True)
        return W, {"kernel_ms": ms.value, "build_ms": build_ms}

    def tikhonov_simplex(self, tau, step, labels, n_classes, rtol=1e-3, atol=None, dtol=None, xtol=None, maxit=200):
        """FISTA on the simplex-constrained Tikhonov problem of learning.classification_tikhonov_simplex
        (gspx_tikhonov_simplex_dev), on this float64 graph.  labels: N ints in the graph's vertex order, the class
        0..n_classes-1 of a measured vertex, -1 for an unmeasured one; a tolerance of None is off.  Returns (X (N,
        n_classes) float64, info) with info = {'niter', 'crit' ('ATOL', 'DTOL', 'RTOL', 'XTOL' or 'MAXIT'),
        'objective' (obj_0 .. obj_niter), 'ms' (device time)}."""
        if self.dtype != np.float64:
            raise ValueError("tikhonov_simplex runs on the float64 device graph")
        lab = np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int32)
        if lab.size != self.N:
            raise ValueError("labels must hold one entry per vertex")
        n_classes, run = int(n_classes), _SolverRun(rtol, atol, dtol, xtol, maxit)
        with self.ctx._temporaries() as t:
            bl, bx = t.upload(lab), t.alloc(self.N * max(n_classes, 1) * 8)
            self.ctx.call(_capi.load().gspx_tikhonov_simplex_dev,
                self._h, float(tau), float(step), ctypes.c_void_p(bl.ptr), n_classes, *run.rule,
                ctypes.c_void_p(bx.ptr), *run.outputs)
            X = bx.download((self.N, n_classes), np.float64)
        return X, run.info()

    # ---- optimization (proximal operators) ----------------------------------------------------------
    def prox_tv_dev(self, x_ptr, z_ptr, nsig, gamma, step, rtol=1e-3, atol=None, dtol=None, xtol=None, maxit=200):
        """gspx_prox_tv_dev on device pointers (N x nsig float64 panels, caller's vertex order); returns info."""
        run = _SolverRun(rtol, atol, dtol, xtol, maxit)
        self.ctx.call(_capi.load().gspx_prox_tv_dev,
            self._h, float(gamma), float(step), int(nsig), ctypes.c_void_p(x_ptr), ctypes.c_void_p(z_ptr), *run.rule,
            *run.outputs)
        return run.info()

    def prox_tv(self, x, gamma, step, rtol=1e-3, atol=None, dtol=None, xtol=None, maxit=200):
        """argmin_z 1/2 ||x - z||^2 + gamma ||D^T z||_1 for x (N,) or (N, Nsig), Nsig <= 256, by FISTA on the dual
        (gspx_prox_tv_dev), on this float64 graph and the edge list it holds; a tolerance of None is off, one
        objective for the whole panel.  x: a numpy array or a float64 DeviceArray of this context; z comes back as
        the same kind.  Returns (z, info) with info = {'niter', 'crit' ('ATOL', 'DTOL', 'RTOL', 'XTOL' or 'MAXIT'),
        'objective' (obj_0 .. obj_niter), 'ms' (device time)}."""
        if self.dtype != np.float64:
            raise ValueError("prox_tv runs on the float64 device graph")
        opts = dict(rtol=rtol, atol=atol, dtol=dtol, xtol=xtol, maxit=maxit)
        if isinstance(x, DeviceArray):
            if x.dtype != np.float64 or x.ctx is not self.ctx or x.cube[0] != self.N or x.cube[2] != 1:
                raise ValueError("prox_tv: a device signal must be (N[, Nsig]) float64 on the graph's context")
            z = DeviceArray.empty(self.ctx, x.cube, np.float64)
            z.shape = x.shape
            return z, self.prox_tv_dev(x.ptr, z.ptr, x.cube[1], gamma, step, **opts)
        x2, one_d = self._panel(x, self.N, "prox_tv")
        with self.ctx._temporaries() as t:
            bx, bz = t.upload(x2), t.alloc(max(x2.nbytes, 16))
            info = self.prox_tv_dev(bx.ptr, bz.ptr, x2.shape[1], gamma, step, **opts)
            z = bz.download(x2.shape, np.float64)
        return (z[:, 0] if one_d else z), info

    # ---- graph learning (pygsp_amd/graph_learning.py) -----------------------------------------------
    def _device_panel(self, x, rows, what, temporaries):
        """Device pointer and column count of a (rows[, cols]) float64 panel: a DeviceArray of this context as it lies,
        a host array uploaded into `temporaries`."""
        if isinstance(x, DeviceArray):
            if x.dtype != np.float64 or x.ctx is not self.ctx or x.cube[0] != rows or x.cube[2] != 1:
                raise ValueError("{}: a device array must be ({}[, columns]) float64 on the graph's context".format(
                    what, rows))
            return x.ptr, x.cube[1]
        x2 = np.asarray(x, dtype=np.float64)
        if x2.ndim not in (1, 2) or x2.shape[0] != rows:
            raise ValueError("{}: first dimension must be {}, got {}".format(what, rows, x2.shape))
        x2 = np.ascontiguousarray(x2.reshape(rows, 1) if x2.ndim == 1 else x2)
        return (temporaries.upload(x2).ptr if x2.size else None), x2.shape[1]

    def edge_sqdist(self, X):
        """z_e = ||X_s - X_t||^2 for every edge (s, t) of this float64 graph's default edge list, in
        Graph.get_edge_list order (gspx_edge_sqdist_dev).  X: (N, F) or (N,), 1 <= F <= 4096, a numpy array or a
        float64 DeviceArray of this context; z comes back as the same kind, (n_edges,)."""
        E, ms = self.n_edges(), ctypes.c_double(0)
        z = DeviceArray.empty(self.ctx, (E, 1, 1), np.float64)
        z.shape = (E,)  # (also for E = 1)
        with self.ctx._temporaries() as t:
            x_ptr, F = self._device_panel(X, self.N, "edge_sqdist", t)
            self.ctx.call(_capi.load().gspx_edge_sqdist_dev, self._h, F, ctypes.c_void_p(x_ptr), ctypes.c_void_p(z.ptr),
                          ctypes.byref(ms))
        return z if isinstance(X, DeviceArray) else z.numpy()

    def learn_log_degrees(self, z, a, b, gamma, tol=1e-5, maxit=10000, w0=None, adjacency=False):
        """Weights of the log-degree model on this float64 graph's pattern (gspx_learn_log_degrees_dev): argmin over
        w >= 0 of 2 z^T w - a sum log(S w) + b ||w||^2 by primal-dual iterations with the fixed step `gamma`, stopped
        when both relative residuals are <= tol (None or negative: off) or after maxit iterations.  z, w0: (n_edges,)
        in Graph.get_edge_list order, numpy arrays or float64 DeviceArrays of this context.  Returns (P, w, W, info): P the
        result (non-negative, exact zeros) and w the last iterate (for warm starts), of the kind z is; W the adjacency
        of P as a DeviceAdjacency (None unless `adjacency`); info = {'niter', 'crit' ('TOL' or 'MAXIT'), 'history'
        (niter, 4): ||dw||, ||w||, ||dv||, ||v||, 'ms' (device time of the iterations)}."""
        E, maxit = self.n_edges(), int(maxit)
        hist = np.zeros((max(maxit, 1), 4), dtype=np.float64)
        niter, crit, ms, h = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_double(0), ctypes.c_void_p()
        P, w = (DeviceArray.empty(self.ctx, (E, 1, 1), np.float64) for _ in range(2))
        P.shape = w.shape = (E,)  # (also for E = 1)
        with self.ctx._temporaries() as t:
            z_ptr, cols = self._device_panel(z, E, "learn_log_degrees: z", t)
            w0_ptr = None
            if w0 is not None:
                w0_ptr, c0 = self._device_panel(w0, E, "learn_log_degrees: w0", t)
                cols = max(cols, c0)
            if cols != 1:
                raise ValueError("learn_log_degrees: z and w0 hold one value per edge")
            self.ctx.call(_capi.load().gspx_learn_log_degrees_dev, self._h, ctypes.c_void_p(z_ptr), float(a), float(b),
                          float(gamma), -1.0 if tol is None else float(tol), maxit, ctypes.c_void_p(w0_ptr),
                          ctypes.c_void_p(P.ptr), ctypes.c_void_p(w.ptr), ctypes.byref(h) if adjacency else None,
                          ctypes.byref(niter), ctypes.byref(crit), _capi.ptr(hist), ctypes.byref(ms))
        W = _adjacency(h, self.ctx, self.N, True)[0] if adjacency else None
        n = int(niter.value)
        info = {"niter": n, "crit": {1: "TOL", 5: "MAXIT"}.get(crit.value), "history": hist[:n].copy(), "ms": ms.value}
        if not isinstance(z, DeviceArray):
            P, w = P.numpy(), w.numpy()
        return P, w, W, info

    # ---- layout (Graph.set_coordinates('spring')) ---------------------------------------------------
    def layout_splits(self):
        """Ways gspx_layout_spring_dev splits the all-pairs sum for this graph (from N and the CU count, or the
        context option 'layout_splits')."""
        return self._i64(_capi.load().gspx_layout_splits)

    def layout_spring_dev(self, pos_ptr, dim, k, fixed_ptr=None, iterations=50, t0=0.1, dt=None):
        """gspx_layout_spring_dev on device pointers (N x dim float64 positions, in place; N uint8 fixed flags or
        None), caller's vertex order; returns the report of layout_spring."""
        iterations = int(iterations)
        if dt is None:  # (a negative count is the library's to refuse)
            dt = float(t0) / float(iterations + 1) if iterations >= 0 else 0.0
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_layout_spring_dev,
            self._h, int(dim), float(k), ctypes.c_void_p(fixed_ptr), iterations, float(t0), dt,
            ctypes.c_void_p(pos_ptr), ctypes.byref(ms))
        return {"kernel_ms": ms.value, "splits": self.layout_splits(), "iterations": iterations}

    def layout_spring(self, pos, k, fixed=None, iterations=50, t0=0.1, dt=None):
        """`iterations` Fruchterman-Reingold steps (pygsp/graphs/_layout.py:169-219) from the positions `pos` (N x 2
        or N x 3), on the pattern of this graph's Laplacian (fp32 and fp64 graphs alike; positions are float64):
        step it runs at temperature t0 - it * dt, formed by repeated subtraction as the reference does; dt None:
        t0 / (iterations + 1), the reference's cooling.  fixed: indices (or a boolean indicator of length N) of the
        vertices that never move.  One step at a given temperature (iterations=1, t0=t) and the continuation of a
        longer run (t0 where it stopped, the same dt) are ordinary calls.  pos: a numpy array or a float64
        DeviceArray of this context (left unchanged); the result comes back as the same kind.  Returns (pos, report)
        with report = {'kernel_ms', 'splits' (ways the all-pairs sum was split), 'iterations'}."""
        mask = None
        if fixed is not None and np.size(fixed):
            fixed = np.asarray(fixed)
            if fixed.dtype == np.bool_ and fixed.shape == (self.N,):
                mask = fixed.astype(np.uint8)
            else:
                mask = np.zeros(self.N, dtype=np.uint8)
                mask[fixed.astype(np.int64)] = 1
            if not mask.any():
                mask = None
        if isinstance(pos, DeviceArray):
            if pos.dtype != np.float64 or pos.ctx is not self.ctx or pos.cube[0] != self.N or pos.cube[2] != 1:
                raise ValueError("layout_spring: device positions must be (N, dim) float64 on the graph's context")
            dim = pos.cube[1]
            out = DeviceArray.empty(self.ctx, pos.cube, np.float64)
            out.shape = pos.shape
            if self.N:
                from . import fourier
                fourier.panel_copy(self.ctx, self.N, pos.ptr, dim, dim, out.ptr, dim)
            with self.ctx._temporaries() as t:
                bm = None if mask is None else t.upload(mask)
                report = self.layout_spring_dev(out.ptr, dim, k, None if bm is None else bm.ptr, iterations, t0, dt)
            return out, report
        p = np.ascontiguousarray(pos, dtype=np.float64)
        if p.ndim != 2 or p.shape[0] != self.N:
            raise ValueError("layout_spring: positions must be (N, dim), got {}".format(np.shape(pos)))
        with self.ctx._temporaries() as t:
            bp = t.upload(p) if p.size else t.alloc(16)
            bm = None if mask is None else t.upload(mask)
            report = self.layout_spring_dev(bp.ptr, p.shape[1], k, None if bm is None else bm.ptr, iterations, t0, dt)
            out = bp.download(p.shape, np.float64) if p.size else p.copy()
        return out, report

    # ---- edges: the differential operator D, grad = D^T x, div = D y ---------------------------------
    def n_edges(self):
        return self._i64(_capi.load().gspx_graph_n_edges)

    def edge_list(self, with_d=False):
        """(sources, targets, weights) in Graph.get_edge_list order; with_d adds D's two values per edge."""
        E = self.n_edges()
        src, dst = np.empty(E, dtype=np.int32), np.empty(E, dtype=np.int32)
        w, ds, dt = (np.empty(E, dtype=self.dtype) for _ in range(3))
        _capi.check(_capi.load().gspx_graph_download_edges(
            self._h, _capi.ptr(src), _capi.ptr(dst), _capi.ptr(w), _capi.ptr(ds), _capi.ptr(dt)))
        return (src, dst, w, ds, dt) if with_d else (src, dst, w)

    def differential_operator(self):
        """D as scipy csc (N x n_edges), assembled on the host from the device edge arrays."""
        src, dst, _, ds, dt = self.edge_list(with_d=True)
        E = src.size
        rows = np.concatenate([src, dst])
        cols = np.concatenate([np.arange(E), np.arange(E)])
        D = sparse.csc_matrix((np.concatenate([ds, dt]), (rows, cols)), shape=(self.N, E))
        D.eliminate_zeros()  # the two values of a self-loop cancel (difference.py:166)
        return D

    def set_edge_list(self, sources, targets, weights, directed):
        """Replace the edge list of grad / div / D by the caller's (gspx_graph_set_edge_list): the edges of a
        directed graph or of a graph with self-loops, in Graph.get_edge_list order (sources non-decreasing)."""
        src = np.ascontiguousarray(sources, dtype=np.int32)
        dst = np.ascontiguousarray(targets, dtype=np.int32)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if not (src.shape == dst.shape == w.shape and src.ndim == 1):
            raise ValueError("sources, targets and weights must be vectors of one length")
        _capi.check(_capi.load().gspx_graph_set_edge_list(self._h, src.size, _capi.ptr(src), _capi.ptr(dst),
                                                          _capi.ptr(w), 1 if directed else 0))

    def grad_dev(self, x_ptr, y_ptr, nsig):
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_grad_dev, self._h, int(nsig), ctypes.c_void_p(x_ptr),
                                               ctypes.c_void_p(y_ptr), ctypes.byref(ms))
        return ms.value

    def div_dev(self, y_ptr, z_ptr, nsig):
        ms = ctypes.c_double(0)
        self.ctx.call(_capi.load().gspx_div_dev, self._h, int(nsig), ctypes.c_void_p(y_ptr),
                                              ctypes.c_void_p(z_ptr), ctypes.byref(ms))
        return ms.value

    def grad(self, x):
        """D^T x: (N,) or (N, Nsig) -> (n_edges,) or (n_edges, Nsig)."""
        return self._panel_op(x, self.N, self.n_edges(), self.grad_dev, "grad")

    def div(self, y):
        """D y: (n_edges,) or (n_edges, Nsig) -> (N,) or (N, Nsig)."""
        return self._panel_op(y, self.n_edges(), self.N, self.div_dev, "div")


METRICS = {"euclidean": 0, "manhattan": 1, "max_dist": 2}
SYMMETRIZE = {"average": 0, "maximum": 1, "fill": 1, "tril": 2, "triu": 3}


class DeviceAdjacency:
    """The weight matrix a device builder produced, still on the device (a gspx_knn handle).  Graph() takes it in
    place of a scipy matrix (DeviceGraph.setup_from): the host copy is made by download(), once, when somebody
    reads G.W.  `weights`: dtype of the host copy (the block-model samplers hand out int64 ones like the
    reference)."""

    def __init__(self, handle, ctx, N, nnz, weights=np.float64):
        self._h, self.ctx, self.shape, self.nnz, self.weights = handle, ctx, (int(N), int(N)), int(nnz), np.dtype(weights)
        self._host = None

    def download(self):
        if self._host is None:
            if not self._h:
                raise RuntimeError("the device adjacency has been released")
            N = self.shape[0]
            indptr = np.empty(N + 1, dtype=np.int32)
            indices = np.empty(self.nnz, dtype=np.int32)
            data = np.empty(self.nnz, dtype=np.float64)
            _capi.check(_capi.load().gspx_knn_download_w(self._h, _capi.ptr(indptr), _capi.ptr(indices), _capi.ptr(data)))
            if self.weights != np.float64:
                data = np.ones(self.nnz, dtype=self.weights) if self.weights.kind in "iu" else data.astype(self.weights)
            self._host = sparse.csr_matrix((data, indices, indptr), shape=self.shape)
            self.close()
        return self._host

    def close(self):
        h, self._h = self._h, None
        if h:
            _capi.load().gspx_knn_destroy(h)

    def __del__(self):
        if sys.is_finalizing():  # the HIP runtime may already be gone; the OS reclaims the memory
            return
        try:
            self.close()
        except Exception:
            pass


def _adjacency(h, ctx, N, keep_on_device, weights=np.float64, neighbors=None):
    """The common end of the device builders: the gspx_knn handle `h` becomes a DeviceAdjacency (destroyed instead
    when anything fails before that), downloaded unless it is to stay on the device.  neighbors: (NN, D) arrays to
    fill with the k-NN query's result while the handle is there.  Returns (W, sigma, build_ms)."""
    lib = _capi.load()
    try:
        nnz, sg, ms = ctypes.c_int64(0), ctypes.c_double(0), ctypes.c_double(0)
        _capi.check(lib.gspx_knn_info(h, ctypes.byref(nnz), ctypes.byref(sg), ctypes.byref(ms)))
        if neighbors is not None:
            _capi.check(lib.gspx_knn_download_neighbors(h, _capi.ptr(neighbors[0]), _capi.ptr(neighbors[1])))
        W = DeviceAdjacency(h, ctx, N, nnz.value, weights)
        h = None
    finally:
        if h:
            lib.gspx_knn_destroy(h)
    return (W if keep_on_device else W.download()), sg.value, ms.value


def knn_graph(coords, k, sigma=None, ctx=None, neighbors=False, metric="euclidean", symmetrize="average",
              keep_on_device=False):
    """k-nearest-neighbour weights on the device (gspx_knn_build): the KD-tree query, Gaussian weights
    and symmetrisation of NNGraph (nngraph.py:213-226, 289-297) in 1 to 4096 dimensions, 1 <= k <= 64 (a uniform grid
    in 1-3-D; beyond that a tiled brute force whose pair distances run on the matrix cores - from 65 dimensions on with
    a run-time dimension loop, same results).  coords: (N, d), already centred / rescaled.  Returns (W csr float64, sigma, info)
    where info = {"build_ms": ...} plus "NN", "D" (N x k, nearest first) when neighbors=True.  keep_on_device: W is
    returned as a DeviceAdjacency (not downloaded)."""
    ctx = ctx or default_context()
    X = np.ascontiguousarray(coords, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("coords must be (N, d)")
    N, d = X.shape
    h = ctypes.c_void_p()
    _capi.check(_capi.load().gspx_knn_build(ctx._h, N, d, _capi.ptr(X), int(k), float(sigma or 0.0), METRICS[metric],
                                            SYMMETRIZE[symmetrize], ctypes.byref(h)))
    nn = (np.empty((N, int(k)), dtype=np.int32), np.empty((N, int(k)), dtype=np.float64)) if neighbors else None
    W, sg, ms = _adjacency(h, ctx, N, keep_on_device, neighbors=nn)
    info = {"build_ms": ms}
    if neighbors:
        info["NN"], info["D"] = nn
    return W, sg, info


def radius_graph(coords, epsilon, sigma=None, ctx=None, metric="euclidean", keep_on_device=False):
    """Radius-graph weights on the device (gspx_radius_build): NNtype='radius' of NNGraph
    (nngraph.py:228-287) in 1 to 4096 dimensions (a grid of epsilon-sized cells up to 3-D; beyond that the candidates of
    an MFMA distance sweep, tested in the KD-tree's arithmetic).  Returns (W csr float64, sigma, info)."""
    ctx = ctx or default_context()
    X = np.ascontiguousarray(coords, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("coords must be (N, d)")
    N, d = X.shape
    h = ctypes.c_void_p()
    _capi.check(_capi.load().gspx_radius_build(ctx._h, N, d, _capi.ptr(X), float(epsilon), float(sigma or 0.0),
                                               METRICS[metric], ctypes.byref(h)))
    W, sg, ms = _adjacency(h, ctx, N, keep_on_device)
    return W, sg, {"build_ms": ms}


def sbm_graph(z, M, seed=None, ctx=None, keep_on_device=False, directed=False, self_loops=False):
    """Stochastic-block-model adjacency sampled on the device (gspx_sbm_build_ex): every unordered pair
    of distinct vertices (r, c) is an edge with probability M[z[r], z[c]], unit weights
    (stochasticblockmodel.py:125-144; one block = Erdos-Renyi).  directed: every ORDERED pair is an entry
    W[r, c] on its own (M need not be symmetric); self_loops: the pairs r == c take part.
    z: (N,) block labels in 0..k-1, M: (k, k).  Returns (W csr float64, build_ms)."""
    ctx = ctx or default_context()
    z = np.asarray(z)
    M = np.ascontiguousarray(M, dtype=np.float64)
    k = M.shape[0]
    if M.shape != (k, k) or z.ndim != 1 or (z.size and (z.min() < 0 or z.max() >= k)):
        raise ValueError("z must hold labels 0..k-1 and M must be k x k")
    N = z.size
    order = np.ascontiguousarray(np.argsort(z, kind="stable"), dtype=np.int32)
    bounds = np.ascontiguousarray(np.searchsorted(z[order], np.arange(k + 1)), dtype=np.int64)
    if seed is None:
        seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])
    h = ctypes.c_void_p()
    flags = (1 if directed else 0) | (2 if self_loops else 0)
    _capi.check(_capi.load().gspx_sbm_build_ex(ctx._h, N, k, _capi.ptr(order), _capi.ptr(bounds), _capi.ptr(M),
                                               ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), flags, ctypes.byref(h)))
    # (keep_on_device: unit int64 weights in the host copy, like the reference's W)
    W, _, ms = _adjacency(h, ctx, N, keep_on_device, weights=np.int64 if keep_on_device else np.float64)
    return W, ms


def check_kept(ind, n_vertices):
    """The kept vertices of a reduction as a contiguous int32 array: ValueError when `ind` is empty, not
    one-dimensional integers, out of range or holds a vertex twice (host only)."""
    a = np.asarray(ind)
    if a.ndim != 1 or a.size == 0:
        raise ValueError("ind must be a non-empty one-dimensional list of vertices")
    if a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("ind must hold integer vertex indices, got {}".format(a.dtype))
    if a.min() < 0 or a.max() >= n_vertices:
        raise ValueError("ind must lie in [0, {}), got {} .. {}".format(n_vertices, a.min(), a.max()))
    if np.unique(a).size != a.size:
        raise ValueError("ind holds a vertex more than once")
    return np.ascontiguousarray(a, dtype=np.int32)


def check_parent(parent, n_vertices, n_clusters):
    """A cluster map as a contiguous int32 array: ValueError unless `parent` holds one integer in [0, n_clusters) per
    vertex and every cluster has a member (host only)."""
    a = np.asarray(parent)
    if a.ndim != 1 or a.size != n_vertices:
        raise ValueError("parent must hold one cluster per vertex ({}), got shape {}".format(n_vertices, a.shape))
    if a.dtype == bool or (a.size and not np.issubdtype(a.dtype, np.integer)):
        raise ValueError("parent must hold integer cluster indices, got {}".format(a.dtype))
    n_clusters = int(n_clusters)
    if n_clusters < 0 or (a.size and (a.min() < 0 or a.max() >= n_clusters)):
        raise ValueError("parent must lie in [0, {})".format(n_clusters))
    if np.unique(a).size != n_clusters:
        raise ValueError("every one of the {} clusters needs a member".format(n_clusters))
    return np.ascontiguousarray(a, dtype=np.int32)


POOL_MODES = {"max": 0, "mean": 1, "sum": 2}


class Segments:
    """A partition of N fine rows into Nc segments as CSR (ptr (Nc + 1,), idx (N,)), checked on the host and uploaded
    once: every row in exactly one segment, no empty segment, members ascending inside a segment - what the pooling
    kernels rely on for their bounds and their summation order.  ``from_parent`` builds it from a cluster map."""

    def __init__(self, ctx, ptr, idx):
        ptr, idx = np.asarray(ptr), np.asarray(idx)
        if ptr.ndim != 1 or idx.ndim != 1 or ptr.size < 1 or ptr[0] != 0 or ptr[-1] != idx.size:
            raise ValueError("segments: ptr must run from 0 to len(idx)")
        if np.any(np.diff(ptr) < 1):
            raise ValueError("segments: every segment needs a member")
        if idx.size and not np.array_equal(np.sort(idx), np.arange(idx.size)):
            raise ValueError("segments: idx must hold every fine row exactly once")
        inner = np.ones(idx.size, dtype=bool)
        inner[ptr[:-1][ptr[:-1] < idx.size]] = False
        if np.any(np.diff(idx)[inner[1:]] <= 0):
            raise ValueError("segments: members must ascend inside a segment")
        self.ctx, self.n_fine, self.n_coarse = ctx, int(idx.size), int(ptr.size - 1)
        self.ptr = np.ascontiguousarray(ptr, dtype=np.int32)
        self.idx = np.ascontiguousarray(idx, dtype=np.int32)
        self._ptr_dev, self._idx_dev = ctx.upload(self.ptr), ctx.upload(self.idx if idx.size else np.zeros(1, np.int32))

    @classmethod
    def from_parent(cls, ctx, parent, n_clusters):
        parent = check_parent(parent, np.size(parent), n_clusters)
        idx = np.argsort(parent, kind="stable")
        ptr = np.concatenate([[0], np.cumsum(np.bincount(parent, minlength=int(n_clusters)))])
        return cls(ctx, ptr, idx)

    @property
    def sizes(self):
        return np.diff(self.ptr)


def _pool_call(ctx, seg, mode, dtype, width, x_ptr, g_ptr, out_ptr, vjp):
    lib, ms = _capi.load(), ctypes.c_double(0)
    head = (ctx._h, _capi.dtype_code(dtype), POOL_MODES[mode], seg.n_fine, seg.n_coarse, int(width),
            ctypes.c_void_p(seg._ptr_dev.ptr), ctypes.c_void_p(seg._idx_dev.ptr), ctypes.c_void_p(x_ptr))
    if vjp:
        ctx.call(lib.gspx_segment_pool_vjp_dev, *head, ctypes.c_void_p(g_ptr), ctypes.c_void_p(out_ptr), ctypes.byref(ms))
    else:
        ctx.call(lib.gspx_segment_pool_dev, *head, ctypes.c_void_p(out_ptr), ctypes.byref(ms))
    return ms.value


def segment_pool_dev(ctx, seg, mode, dtype, width, x_ptr, y_ptr):
    """gspx_segment_pool_dev on device pointers: the row-major (n_fine, width) panel at x_ptr pooled over the Segments
    `seg` into the (n_coarse, width) panel at y_ptr.  Returns kernel_ms."""
    return _pool_call(ctx, seg, mode, dtype, width, x_ptr, None, y_ptr, False)


def segment_pool_vjp_dev(ctx, seg, mode, dtype, width, x_ptr, g_ptr, gx_ptr):
    """gspx_segment_pool_vjp_dev on device pointers: the (n_coarse, width) cotangent at g_ptr spread to the (n_fine,
    width) panel at gx_ptr; x_ptr (the pooled input) is read for 'max' only and may be None otherwise."""
    return _pool_call(ctx, seg, mode, dtype, width, x_ptr, g_ptr, gx_ptr, True)


def _pool_any(ctx, seg, mode, a, x, rows_in, rows_out, vjp):
    """The shared frame of segment_pool and segment_pool_vjp: `a` ((rows_in, ...), numpy or DeviceArray) is the panel
    that sets kind, dtype and trailing shape; `x` the pooled input of a 'max' vjp (same kind) or None."""
    if mode not in POOL_MODES:
        raise ValueError("Unknown pooling mode {!r}: 'max', 'mean' or 'sum'".format(mode))
    need_x = vjp and mode == "max"
    if need_x and x is None:
        raise ValueError("the vjp of 'max' pooling needs the pooled input x")
    if isinstance(a, DeviceArray):
        if a.cube[0] != rows_in:
            raise ValueError("expected {} rows, got {}".format(rows_in, a.cube[0]))
        _, S, F = a.cube
        if need_x and (not isinstance(x, DeviceArray) or x.cube != (rows_out, S, F) or x.dtype != a.dtype):
            raise ValueError("x must be a DeviceArray like the cotangent, with {} rows".format(rows_out))
        out = DeviceArray.empty(ctx, (rows_out, S, F), a.dtype)
        out.shape = (rows_out,) + tuple(a.shape[1:])
        item = a.dtype.itemsize
        for f in range(F if S else 0):  # one (rows, S) row-major panel per feature plane
            xp = x.ptr + f * rows_out * S * item if need_x else None
            if vjp:
                segment_pool_vjp_dev(ctx, seg, mode, a.dtype, S, xp, a.ptr + f * rows_in * S * item,
                                     out.ptr + f * rows_out * S * item)
            else:
                segment_pool_dev(ctx, seg, mode, a.dtype, S, a.ptr + f * rows_in * S * item,
                                 out.ptr + f * rows_out * S * item)
        return out
    a = np.asarray(a)
    if a.ndim < 1 or a.shape[0] != rows_in:
        raise ValueError("expected {} rows, got shape {}".format(rows_in, a.shape))
    dtype = np.dtype(np.float32 if a.dtype == np.float32 else np.float64)
    panel = np.ascontiguousarray(a.reshape(rows_in, -1), dtype=dtype)
    width, shape = panel.shape[1], (rows_out,) + a.shape[1:]
    if width == 0 or rows_in == 0:
        return np.zeros(shape, dtype=dtype)
    with ctx._temporaries() as t:
        ba, bo, bx = t.upload(panel), t.alloc(rows_out * width * dtype.itemsize), None
        if need_x:
            xh = np.asarray(x)
            if xh.shape != (rows_out,) + a.shape[1:]:
                raise ValueError("x must have shape {}, got {}".format((rows_out,) + a.shape[1:], xh.shape))
            bx = t.upload(np.ascontiguousarray(xh.reshape(rows_out, -1), dtype=dtype))
        if vjp:
            segment_pool_vjp_dev(ctx, seg, mode, dtype, width, bx.ptr if need_x else None, ba.ptr, bo.ptr)
        else:
            segment_pool_dev(ctx, seg, mode, dtype, width, ba.ptr, bo.ptr)
        return bo.download((rows_out, width), dtype).reshape(shape)


def segment_pool(ctx, seg, x, mode="max"):
    """Pool the vertex signal `x` ((n_fine, ...) numpy array, or a DeviceArray) over the Segments `seg`: 'max', 'mean'
    (the ascending-order sum divided by the size) or 'sum' of every segment's rows.  Returns the same kind with
    n_coarse rows; float32 stays float32, anything else computes in float64.  No atomics: bit-reproducible."""
    return _pool_any(ctx, seg, mode, x, None, seg.n_fine, seg.n_coarse, False)


def segment_pool_vjp(ctx, seg, g, x=None, mode="max"):
    """The vector-Jacobian product of segment_pool: `g` ((n_coarse, ...)) spread to the fine rows - 'sum': a copy of
    the segment's row (unpooling), 'mean': g / size, 'max': g at the first member that attains the maximum of `x`
    (the pooled input, needed for 'max' only), zero at the others."""
    return _pool_any(ctx, seg, mode, g, x, seg.n_coarse, seg.n_fine, True)


def segment_unpool(ctx, seg, y):
    """Copy every segment's row of `y` ((n_coarse, ...)) to all of its members: the 'sum' vjp under its other name."""
    return segment_pool_vjp(ctx, seg, y, None, "sum")


def line_graph_size(dev):
    """(vertices, stored entries) of the line graph of the DeviceGraph `dev` (gspx_linegraph_size): its edge count
    and a 64-bit sum of the row lengths, which may exceed what the builder's 32-bit indices hold."""
    n, nnz = ctypes.c_int64(0), ctypes.c_int64(0)
    _capi.check(_capi.load().gspx_linegraph_size(dev._h, ctypes.byref(n), ctypes.byref(nnz)))
    return n.value, nnz.value


def line_graph(dev, keep_on_device=True):
    """Adjacency of the line graph of the DeviceGraph `dev` (gspx_linegraph_build; linegraph.py:34-46): one vertex per
    edge of Graph.get_edge_list, two of them joined when the edges share an endpoint, unit weights.  `dev` is an
    undirected graph without self-loops that was built from W.  Returns (W, info): W a DeviceAdjacency (or the
    scipy CSR matrix, float64, with keep_on_device=False), info = {"kernel_ms", "build_ms"}.  ValueError when the
    vertex or entry count exceeds 32-bit indices - nothing is allocated by then."""
    h, kernel_ms = ctypes.c_void_p(), ctypes.c_double(0)
    dev.ctx.call(_capi.load().gspx_linegraph_build, dev._h, ctypes.byref(h), ctypes.byref(kernel_ms))
    W, _, build_ms = _adjacency(h, dev.ctx, dev.n_edges(), keep_on_device)
    return W, {"kernel_ms": kernel_ms.value, "build_ms": build_ms}


def plan_describe(coeffs, ctx=None):
    """The engine's step schedule for these coefficients (host-only; for schedule tests)."""
    c = _coeff_matrix(coeffs)
    Nf, M = c.shape
    if M < 2:
        _capi.check(_capi.load().gspx_plan_describe(None, Nf, M, _capi.ptr(c), None))
    plan = np.zeros((M - 1, 4 + 3 * Nf), dtype=np.float64)
    _capi.check(_capi.load().gspx_plan_describe(ctx._h if ctx else None, Nf, M, _capi.ptr(c),
                                                _capi.ptr(plan)))
    return plan
