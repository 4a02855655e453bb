// gspx_ctx.hip.h - the handles of the C-ABI and what belongs to a context rather than to a subject: Options (and the
// one table of their keys), gspx_ctx, gspx_buf, gspx_graph; replay_reset, finish_timed, pool_event, elt_size; device
// count / PCI id, context create / destroy / sync, gspx_ctx_set_option / gspx_ctx_get_option, the gspx_buf_* entry
// points with the staged copy of large buffers, and the gspx_last_*timing* getters.
// After gspx_mem.hip.h (DevMem, PinMem, CopyStage, HostPipe are members of the handles).
#pragma once

// ------------------------------------------------------------------------------------------------
// handles
// ------------------------------------------------------------------------------------------------
struct Options {
  int64_t kernel = 0;         // 0 auto, 1 panel, 2 narrow
  int64_t vec = 0;            // 0 auto
  int64_t rows_per_wave = 0;  // 0 = auto (4 for the scalar-metadata kernel, 16 for the LDS kernel)
  int64_t narrow_g_log2 = -1;  // -1 = auto (4 lanes per row in total)
  int64_t waves_per_block = 4;  // panel kernel (kernel 1): 4, 8 or 16
  int64_t calib_mix = 0;        // NOT a user option (no key): set for the duration of gspx_bench_step_mix - the wide
                                // k_step_tile launches run their calibration build (arithmetic removed; 2: barriers too)
  int64_t graph_launch = 2;     // replay a repeated identical call as one hipGraph: 0 never, 1 always, 2 when the panel is small (launch-bound)
  int64_t tile_gather = 1;      // recurrence steps stage the gathered panel in LDS when the graph carries gather tiles
  int64_t tile_workgroups = 0;  // persistent workgroups of that kernel (0: two per CU; what fits for the small builds)
  int64_t knn_f32 = 1;          // neighbour sweep beyond three dimensions on the fp32 matrix cores: 1 when its rounding
                                // margin is small against the bounds, 0 never, 2 always (the selection stays exact)
  int64_t tile_pad = 1;         // 1: panels whose rows are not made of 16-byte pieces take the tile kernels with padded rows
                                // (a single signal only on graphs beyond the L2s); 2: always; 0: never
  int64_t tile_min_row = 16;    // narrowest rows (bytes) the tile kernel takes; below: the sub-wave kernel
  int64_t staged_copy = 1;        // large gspx_buf_download (1) and also gspx_buf_upload (2) through pinned chunks and host threads
  int64_t staged_copy_min_mb = 32;  // ... from that many MB on
  int64_t copy_threads = 0;       // host threads of a staged copy (0: 8)
  int64_t tile_regroup = 1;     // 1: rows of 3 / 5 / 6 / 7 / 10 / 12 / 14 sixteen-byte pieces run the builds whose compute
                                // phases regroup the lanes by pieces (k_step_tile<..., CL>); 0: the power-of-two builds
  int64_t tile_acc_builds = 1;  // 1: steps without a flush run the flush-free builds of k_step_tile (ACC = false: no
                                // accumulator registers or loads, no flush formed; the same bits); 0: the general build
  int64_t tile_lg = 0;          // lanes per row of the narrow builds: 0 by row size (1 / 2 / 4 / 8); 2, 4 or 8: at least that
  int64_t edge_vertex_walk = 1; // grad / div walk the vertices in the internal order (k_grad_v / k_div_v); 0: edge order
  int64_t fuse_input = 1;       // 1: k_step_tile reads the caller's panel directly in steps 1-2 (no permute-in copy)
  int64_t tile_nt = -1;         // k_step_tile non-temporal accesses: bit 0 matrix entries, bit 2 T_{k-2} loads (each
                                // -1 % on panels beyond the 256 MB Infinity Cache, +5 % each on panels that fit in
                                // it); bit 1 accumulator, bit 3 T_k stores (no effect).  -1: 5 for panels >= 192 MiB
  int64_t synthesis = 0;        // 0 vector-coefficient Clenshaw (K products), 1 per-filter loop
  int64_t alternate_sweep = 1;  // 1: odd steps sweep the rows backwards (Infinity-Cache reuse, -3..5 %)
  int64_t xcd_remap = 1;
  int64_t combine = 0;        // 0 auto, 1 fused flush, 2 deferred
  int64_t ws_limit_mb = 65536;  // workspace budget per filter call
  int64_t max_batch = 0;        // 0 = no extra cap on signals per batch
  int64_t gather_rccl = 1;      // gspx_gather: 0 peer copies, 1 RCCL between devices (peer copies if it fails), 2 RCCL for every block
  int64_t lds_pad_kb = 0;       // k_step_lds: unused dynamic LDS per workgroup (0..40 KB), caps the occupancy
  int64_t host_pipeline = 1;    // gspx_cheby_filter (host pointers): 1 column batches pipelined over pinned staging when the
                                // call is large enough, 2 always, 0 one pageable copy in, the kernels, one out
  int64_t host_batch = 0;       // signals per pipelined batch (0: auto = 128-byte rows; > 0: uniform batches of that width)
  int64_t host_edge = 0;        // width of the first and the last batch (0: auto = half a batch in auto mode)
  int64_t host_threads = 0;     // host threads packing / unpacking, per direction (0: auto, a quarter of the cores, at most 16)
  int64_t streamed_alloc = 1;   // 1: the two streamed workspaces are assembled from scrambled 2 MB chunks (HIP
                                // virtual-memory API; +2..8 % bandwidth); 0: plain hipMalloc (the safe mode on an
                                // untested ROCm: no address range is ever reserved or retired)
  int64_t layout_splits = 0;    // gspx_layout_spring_dev: ways the all-pairs j range is split over grid.y (0: from N and
                                // the CU count, gspx_layout.hip.h)
};

struct gspx_ctx {
  int device = 0;
  int cu_count = 256;
  hipStream_t stream = nullptr;
  Options opt;
  // workspace (grow-only, reused across calls)
  DevMem ws_t;      // T_k panels
  DevMem ws_r;      // accumulators
  DevMem ws_w;      // per-step flush weights / combine coefficients
  DevMem io_x, io_y;  // staging for the host-pointer entry point
  DevMem ws_spec;     // small matrices and Gram partials of the panel primitives (gspx_spectral.hip.h, gspx_reduce.hip.h)
  DevMem ws_sq, ws_sqp;  // column norms: coefficients and norms | workgroup partials (gspx_cheby_sqnorms_dev)
  HostPipe* pipe = nullptr;  // its pipelined form (created on first use)
  CopyStage* copy = nullptr; // staged transfers of large buffers (created on first use)
  bool counted = false;      // this context is in g_live_ctx
  // live RCCL communicators made on this context (gspx_comm_create): invalidated when the context goes
  std::mutex comms_mu;
  std::vector<struct gspx_comm*> comms;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  std::vector<hipEvent_t> ev_pool;
  double timing[5] = {0, 0, 0, 0, 0};  // what gspx_last_timing reports (run_batches fills it)
  // step launches of the last filter / Newton / program call (gspx_last_step_kinds): k_step_tile | the plain step
  // kernels.  Counted on the host where they are issued (launch_step_tile, launch_step), zeroed with `timing`.
  int64_t step_kinds[2] = {0, 0};
  // hipGraph replay of a repeated identical filter call (launch-bound small graphs)
  bool capturing = false;     // run_batch is being recorded: no copies, syncs or events inside
  // identity of a call = the full tuple of everything the recorded launches depend on, compared
  // byte for byte (not a hash of it: a collision would replay the wrong graph silently)
  std::vector<unsigned char> seen_key;   // key of the last eager call (empty: none)
  std::vector<unsigned char> graph_key;  // key the instantiated graph was captured for
  hipGraphExec_t graph_exec = nullptr;
  int64_t graph_kinds[2] = {0, 0};  // step_kinds of the recorded launches: what a replay reports
};

static std::atomic<int> g_live_ctx[64];  // live contexts per device (zero-initialised)

// any other work on the context invalidates a recorded replay (it may have rewritten the weights,
// the cached gather offsets or the workspace the graph refers to)
static void replay_reset(gspx_ctx* ctx) {
  if (!ctx) return;
  ctx->seen_key.clear();
  ctx->graph_key.clear();
  if (ctx->graph_exec) {
    (void)hipGraphExecDestroy(ctx->graph_exec);
    ctx->graph_exec = nullptr;
  }
}

// end of a timed entry point: kernel_ms = the time between ctx->ev[0] and ctx->ev[1], which the caller has recorded
// on ctx->stream - where it records them (around its small host copies or inside them) is what its kernel_ms means
static int finish_timed(gspx_ctx* ctx, double* kernel_ms) {
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float f = 0;
  HIPCHK(hipEventElapsedTime(&f, ctx->ev[0], ctx->ev[1]));
  if (kernel_ms) *kernel_ms = f;
  return GSPX_OK;
}

struct gspx_buf {
  gspx_ctx* ctx = nullptr;
  DevMem mem;
  int64_t bytes = 0;
};

static std::atomic<uint64_t> g_generation{1};  // handles are told apart by birth number, not by address

struct gspx_graph {
  gspx_ctx* ctx = nullptr;
  const uint64_t generation = g_generation.fetch_add(1);
  int64_t N = 0;
  int dtype = GSPX_F64;
  bool from_w = false;
  // canonical Laplacian, caller's vertex order
  int64_t nnz_l = 0;
  DevMem lptr, lcol, lval, dw;
  // internal padded CSR, engine vertex order
  int64_t nnz_int = 0;
  DevMem rptr, rcol, rval, fval, coff;
  unsigned coff_ldb = 0;  // panel row bytes the cached byte offsets were built for
  DevMem perm, iperm;
  bool has_perm = false;
  double fval_lmax = -1.0;
  double build_ms = 0.0;
  // ingredients of Graph._get_upper_bound (graph.py:933-960), taken while W is on the device (fp64 graphs built
  // from W): max W_ij, max dw, max (dw_i + dw_j) over entries, max (dw_i + (W dw)_i / dw_i) or NaN
  bool has_bounds = false;
  double bounds[4] = {0, 0, 0, 0};
  // one-level row tiles of the LDS-staged recurrence step (optional; gspx_tile_kernels.hip.h)
  DevMem gt_hdr, gt_s1rows, gt_lidx;
  DevMem gt_s1nat;   // gt_s1rows mapped through perm: the same lists as rows of the caller's (unpermuted) panel
  int gt_ns1 = 0;
  int gt_rows = 0, gt_nb = 0, gt_slow = 0;
  size_t gt_lds = 0;
  int gt_entmax = 0;  // most stored entries of a staged block (sizes the LDS of the narrow builds)
  // differential operator (built on first use; gspx_ops.hip.h)
  int lap_type = GSPX_LAP_COMBINATORIAL;
  bool edges_built = false;
  bool edges_custom = false;  // the edge list is a caller's (gspx_graph_set_edge_list), not the Laplacian's own
  int64_t n_edges = 0;
  DevMem e_off, e_toff, e_src, e_dst, e_tedge, e_cs, e_ct, e_w;
};

static size_t elt_size(int dtype) { return dtype == GSPX_F32 ? 4 : 8; }

static hipEvent_t pool_event(gspx_ctx* ctx, size_t& i_ref) {
  // at most 1024 timing events per call: calls split into more batches than that (huge panels)
  // reuse the last quadruple - their per-phase timings are then only a lower bound
  size_t i = i_ref - 1;
  if (i >= 1024) {
    i = 1020 + (i & 3);
    i_ref = i + 1;
  }
  while (ctx->ev_pool.size() <= i) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    ctx->ev_pool.push_back(e);
  }
  return ctx->ev_pool[i];
}

// ------------------------------------------------------------------------------------------------
// devices / contexts
// ------------------------------------------------------------------------------------------------
extern "C" int gspx_device_count(int* n) {
  if (!n) return set_err(GSPX_ERR_INVALID, "gspx_device_count: null output");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *n = 0;
    (void)hipGetLastError();
    return set_err(GSPX_ERR_NODEVICE, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
  }
  *n = c;
  return GSPX_OK;
}

extern "C" int gspx_device_pci_bus_id(int device, char* out, int capacity) {
  if (!out || capacity < 16) return set_err(GSPX_ERR_INVALID, "gspx_device_pci_bus_id: need a buffer of >= 16 chars");
  out[0] = 0;
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(GSPX_ERR_NODEVICE, "no HIP device visible (libgspx has no CPU fallback)");
  }
  if (device < 0 || device >= c) return set_err(GSPX_ERR_INVALID, "device %d of %d", device, c);
  HIPCHK(hipDeviceGetPCIBusId(out, capacity, device));
  return GSPX_OK;
}

extern "C" int gspx_ctx_create(int device, gspx_ctx** out) {
  if (!out) return set_err(GSPX_ERR_INVALID, "gspx_ctx_create: null output");
  *out = nullptr;
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess || c <= 0) {
    (void)hipGetLastError();
    return set_err(GSPX_ERR_NODEVICE, "no HIP device visible (libgspx has no CPU fallback)");
  }
  if (device < 0 || device >= c)
    return set_err(GSPX_ERR_INVALID, "device %d out of range (%d visible)", device, c);
  HIPCHK(hipSetDevice(device));
  gspx_ctx* ctx = new gspx_ctx();
  ctx->device = device;
  {  // the two workspaces the recurrence streams every step (GSPX_STREAMED_ALLOC=0: plain hipMalloc).  The chunked
     // mapping retires address space whenever a workspace is re-created (see DevMem): worth 2-8 % to the one
     // context that owns a GPU, not worth an address-space leak per context to a process that keeps several
     // contexts on one device (a multi-tenant server) - those get plain allocations unless GSPX_STREAMED_ALLOC=1
     // (or the option, per context) asks otherwise
    const char* env = getenv("GSPX_STREAMED_ALLOC");
    const int others = g_live_ctx[device & 63].fetch_add(1);
    ctx->counted = true;
    if (env && (env[0] == '0' || env[0] == '1')) ctx->opt.streamed_alloc = env[0] == '1';
    else ctx->opt.streamed_alloc = others == 0 ? 1 : 0;
    ctx->ws_t.streamed = ctx->ws_r.streamed = ctx->opt.streamed_alloc != 0;
  }
  if (hipDeviceGetAttribute(&ctx->cu_count, hipDeviceAttributeMultiprocessorCount, device) !=
          hipSuccess ||
      ctx->cu_count < 1)
    ctx->cu_count = 256;
  hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete ctx;
    return set_err(GSPX_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
  }
  for (int i = 0; i < 4; ++i) {
    e = hipEventCreate(&ctx->ev[i]);
    if (e != hipSuccess) {
      delete ctx;
      return set_err(GSPX_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(e));
    }
  }
  *out = ctx;
  return GSPX_OK;
}

// (the one prototype of the library: gspx_comm.hip.h needs gspx_ctx and gspx_buf complete and comes after this header)
static void comm_invalidate_all(gspx_ctx* ctx);

extern "C" int gspx_ctx_destroy(gspx_ctx* ctx) {
  replay_reset(ctx);
  if (!ctx) return GSPX_OK;
  if (ctx->counted) g_live_ctx[ctx->device & 63].fetch_sub(1);
  comm_invalidate_all(ctx);
  if (ctx->graph_exec) {
    (void)hipGraphExecDestroy(ctx->graph_exec);
    ctx->graph_exec = nullptr;
  }
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (int i = 0; i < 4; ++i)
    if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
  for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
  ctx->ws_t.release();
  ctx->ws_r.release();
  ctx->ws_w.release();
  ctx->io_x.release();
  ctx->io_y.release();
  ctx->ws_spec.release();
  ctx->ws_sq.release();
  ctx->ws_sqp.release();
  if (ctx->pipe) {
    ctx->pipe->destroy();
    delete ctx->pipe;
    ctx->pipe = nullptr;
  }
  if (ctx->copy) {
    ctx->copy->destroy();
    delete ctx->copy;
    ctx->copy = nullptr;
  }
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return GSPX_OK;
}

extern "C" int gspx_ctx_sync(gspx_ctx* ctx) {
  if (!ctx) return set_err(GSPX_ERR_INVALID, "null ctx");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return GSPX_OK;
}

// Every option once: its key, its member of Options, the values it takes (ok == nullptr: any) and the text of the
// error a refused value gets.  gspx_ctx_set_option and gspx_ctx_get_option scan this table and nothing else; calib_mix
// has no key, and the read-only "retired_va_mb" of gspx_ctx_get_option is not a member of Options.
struct OptionDef {
  const char* key;
  int64_t Options::*slot;
  bool (*ok)(int64_t);
  const char* refusal;
};
static const OptionDef OPTION_TABLE[] = {
    {"kernel", &Options::kernel, [](int64_t v) { return v == 0 || v == 1 || v == 2 || v == 5; },
     "kernel must be 0 (auto), 1 (panel), 2 (narrow) or 5 (LDS-staged)"},
    {"vec", &Options::vec, [](int64_t v) { return v == 0 || v == 1 || v == 2 || v == 4; }, "vec must be 0, 1, 2 or 4"},
    {"rows_per_wave", &Options::rows_per_wave, [](int64_t v) { return v >= 0 && v <= 1024; },
     "rows_per_wave must be in [0, 1024] (0 = auto)"},
    {"narrow_g_log2", &Options::narrow_g_log2, [](int64_t v) { return v >= -1 && v <= 6; },
     "narrow_g_log2 must be in [-1, 6] (-1 = auto)"},
    {"waves_per_block", &Options::waves_per_block, [](int64_t v) { return v == 4 || v == 8 || v == 16; },
     "waves_per_block must be 4, 8 or 16"},
    {"alternate_sweep", &Options::alternate_sweep, nullptr, nullptr},
    {"synthesis", &Options::synthesis, nullptr, nullptr},
    {"tile_gather", &Options::tile_gather, nullptr, nullptr},
    {"graph_launch", &Options::graph_launch, nullptr, nullptr},
    {"tile_workgroups", &Options::tile_workgroups, nullptr, nullptr},
    {"tile_lg", &Options::tile_lg, nullptr, nullptr},
    {"tile_regroup", &Options::tile_regroup, nullptr, nullptr},
    {"tile_acc_builds", &Options::tile_acc_builds, nullptr, nullptr},
    {"staged_copy", &Options::staged_copy, nullptr, nullptr},
    {"staged_copy_min_mb", &Options::staged_copy_min_mb, nullptr, nullptr},
    {"copy_threads", &Options::copy_threads, nullptr, nullptr},
    {"tile_min_row", &Options::tile_min_row, nullptr, nullptr},
    {"tile_pad", &Options::tile_pad, nullptr, nullptr},
    {"knn_f32", &Options::knn_f32, nullptr, nullptr},
    {"tile_nt", &Options::tile_nt, nullptr, nullptr},
    {"fuse_input", &Options::fuse_input, nullptr, nullptr},
    {"edge_vertex_walk", &Options::edge_vertex_walk, nullptr, nullptr},
    {"xcd_remap", &Options::xcd_remap, nullptr, nullptr},
    {"combine", &Options::combine, nullptr, nullptr},
    {"ws_limit_mb", &Options::ws_limit_mb, nullptr, nullptr},
    {"max_batch", &Options::max_batch, nullptr, nullptr},
    {"gather_rccl", &Options::gather_rccl, nullptr, nullptr},
    {"lds_pad_kb", &Options::lds_pad_kb, nullptr, nullptr},
    {"host_pipeline", &Options::host_pipeline, nullptr, nullptr},
    {"host_batch", &Options::host_batch, nullptr, nullptr},
    {"host_edge", &Options::host_edge, nullptr, nullptr},
    {"host_threads", &Options::host_threads, nullptr, nullptr},
    {"streamed_alloc", &Options::streamed_alloc, nullptr, nullptr},
    {"layout_splits", &Options::layout_splits, [](int64_t v) { return v >= 0 && v <= 65535; },
     "layout_splits must be in [0, 65535] (0 = automatic)"},
};

static const OptionDef* find_option(const char* key) {
  if (key)
    for (const OptionDef& d : OPTION_TABLE)
      if (!strcmp(key, d.key)) return &d;
  set_err(GSPX_ERR_INVALID, "unknown option '%s'", key ? key : "(null)");
  return nullptr;
}

extern "C" int gspx_ctx_set_option(gspx_ctx* ctx, const char* key, int64_t value) {
  replay_reset(ctx);
  if (!ctx) return set_err(GSPX_ERR_INVALID, "null ctx");
  const OptionDef* d = find_option(key);
  if (!d) return GSPX_ERR_INVALID;
  if (d->ok && !d->ok(value)) return set_err(GSPX_ERR_INVALID, "%s", d->refusal);
  ctx->opt.*d->slot = value;
  if (d->slot == &Options::streamed_alloc) {
    const bool on = value != 0;
    (void)hipSetDevice(ctx->device);
    for (DevMem* m : {&ctx->ws_t, &ctx->ws_r}) {
      if (!on && m->va_size) {  // currently chunked: drop it, the next call allocates plainly
        (void)hipStreamSynchronize(ctx->stream);
        m->release();
      }
      m->streamed = on;
    }
  }
  return GSPX_OK;
}

extern "C" int gspx_ctx_get_option(gspx_ctx* ctx, const char* key, int64_t* value) {
  if (!ctx || !value) return set_err(GSPX_ERR_INVALID, "null argument");
  if (key && !strcmp(key, "retired_va_mb")) {  // read-only: address space of retired workspace ranges, whole process
    *value = (int64_t)(g_retired_va_bytes.load() >> 20);
    return GSPX_OK;
  }
  const OptionDef* d = find_option(key);
  if (!d) return GSPX_ERR_INVALID;
  *value = ctx->opt.*d->slot;
  return GSPX_OK;
}

// ------------------------------------------------------------------------------------------------
// buffers
// ------------------------------------------------------------------------------------------------
extern "C" int gspx_buf_alloc(gspx_ctx* ctx, int64_t bytes, gspx_buf** out) {
  if (!ctx || !out || bytes < 0) return set_err(GSPX_ERR_INVALID, "gspx_buf_alloc: bad argument");
  *out = nullptr;
  HIPCHK(hipSetDevice(ctx->device));
  gspx_buf* b = new gspx_buf();
  b->ctx = ctx;
  b->bytes = bytes;
  int rc = b->mem.alloc((size_t)bytes);  // caller-visible memory: one plain allocation (peer copies, interop)
  if (rc != GSPX_OK) {
    delete b;
    return rc;
  }
  *out = b;
  return GSPX_OK;
}

extern "C" int gspx_buf_free(gspx_buf* b) {
  if (!b) return GSPX_OK;
  (void)hipSetDevice(b->ctx->device);
  (void)hipStreamSynchronize(b->ctx->stream);
  delete b;
  return GSPX_OK;
}

// one direction of a staged transfer; GSPX_OK, or an error with nothing guaranteed about the destination
static int staged_copy(gspx_ctx* ctx, unsigned char* dev, unsigned char* host, size_t bytes, bool to_device) {
  if (!ctx->copy) ctx->copy = new CopyStage();
  CopyStage& cs = *ctx->copy;
  CHK(cs.init());
  constexpr int NS = CopyStage::NS;
  const size_t chunk = CopyStage::CHUNK;
  const int nchunks = (int)((bytes + chunk - 1) / chunk);
  const int P = (int)std::max<int64_t>(1, std::min<int64_t>(ctx->opt.copy_threads > 0 ? ctx->opt.copy_threads : 8,
                                                             (int64_t)std::thread::hardware_concurrency()));
  if (!to_device) {  // a result array fresh from the allocator: huge pages before the threads fault it in
    const uintptr_t lo = ((uintptr_t)host + ((size_t)2 << 20) - 1) & ~(((uintptr_t)2 << 20) - 1);
    const uintptr_t hi = ((uintptr_t)host + bytes) & ~(((uintptr_t)2 << 20) - 1);
    if (hi > lo) (void)madvise((void*)lo, hi - lo, MADV_HUGEPAGE);
  }
  // chunk c may be touched by the host threads once `released` > c; they report a finished chunk in done[c]
  std::atomic<int> released{to_device ? std::min(NS, nchunks) : 0};
  std::vector<std::atomic<int>> done((size_t)nchunks);
  for (auto& d : done) d.store(0);
  std::atomic<bool> failed{false};
  auto worker = [&](int t) {
    for (int c = 0; c < nchunks; ++c) {
      while (released.load(std::memory_order_acquire) <= c) {
        if (failed.load()) return;
        std::this_thread::yield();
      }
      if (failed.load(std::memory_order_acquire)) return;  // a failed transfer releases everything: copy nothing stale
      const size_t off = (size_t)c * chunk, len = std::min(chunk, bytes - off);
      const size_t per = ((len + P - 1) / P + 63) & ~(size_t)63;
      const size_t lo = std::min(len, per * (size_t)t), hi = std::min(len, lo + per);
      if (hi > lo) {
        unsigned char* pinned = (unsigned char*)cs.pin[c % NS].p;
        if (to_device) memcpy(pinned + lo, host + off + lo, hi - lo);
        else memcpy(host + off + lo, pinned + lo, hi - lo);
      }
      done[(size_t)c].fetch_add(1, std::memory_order_release);
    }
  };
  // (nothing may throw across the C boundary: a thread that cannot be created ends the staged attempt - the ones
  // already running are told to stop and joined - and the caller falls back to the plain copy)
  std::vector<std::thread> pool;
  try {
    pool.reserve((size_t)P);
    for (int t = 0; t < P; ++t) pool.emplace_back(worker, t);
  } catch (...) {
    failed.store(true, std::memory_order_release);
    released.store(nchunks, std::memory_order_release);
    for (auto& th : pool)
      if (th.joinable()) th.join();
    return set_err(GSPX_ERR_HIP, "staged copy: could not start %d host threads", P);
  }
  auto wait_done = [&](int c) {
    while (done[(size_t)c].load(std::memory_order_acquire) < P) std::this_thread::yield();
  };
  hipError_t err = hipSuccess;
  for (int c = 0; c < nchunks && err == hipSuccess; ++c) {
    const size_t off = (size_t)c * chunk, len = std::min(chunk, bytes - off);
    void* pinned = cs.pin[c % NS].p;
    if (to_device) {
      wait_done(c);  // the chunk sits in its pinned slot
      err = hipMemcpyAsync(dev + off, pinned, len, hipMemcpyHostToDevice, cs.st);
      if (err == hipSuccess) err = hipStreamSynchronize(cs.st);  // (the threads are filling the next slots meanwhile)
      released.store(std::min(nchunks, c + NS + 1), std::memory_order_release);  // this slot is free again
    } else {
      if (c >= NS) wait_done(c - NS);  // the slot's previous chunk has been copied out
      err = hipMemcpyAsync(pinned, dev + off, len, hipMemcpyDeviceToHost, cs.st);
      if (err == hipSuccess) err = hipStreamSynchronize(cs.st);
      released.store(c + 1, std::memory_order_release);
    }
  }
  if (err != hipSuccess) {
    failed.store(true, std::memory_order_release);  // before the release: no worker copies a chunk that never arrived
    released.store(nchunks, std::memory_order_release);
  }
  for (auto& th : pool) th.join();
  if (err != hipSuccess) return set_err(GSPX_ERR_HIP, "staged copy: %s", hipGetErrorString(err));
  return GSPX_OK;
}

extern "C" int gspx_buf_upload(gspx_buf* b, const void* host, int64_t bytes) {
  if (!b || (!host && bytes > 0) || bytes < 0 || bytes > b->bytes)
    return set_err(GSPX_ERR_INVALID, "gspx_buf_upload: bad argument");
  HIPCHK(hipSetDevice(b->ctx->device));
  if (bytes == 0) return GSPX_OK;
  // (measured, 256 MB: the runtime's own pageable upload runs at 56 GB/s, the staged one at 51 - uploads stay plain
  // unless the option asks for 2; downloads into fresh memory: 11.7 GB/s plain, 46 GB/s staged)
  if (b->ctx->opt.staged_copy >= 2 && (size_t)bytes >= ((size_t)b->ctx->opt.staged_copy_min_mb << 20)) {
    HIPCHK(hipStreamSynchronize(b->ctx->stream));  // whoever still reads the buffer's old contents is done
    if (staged_copy(b->ctx, (unsigned char*)b->mem.p, (unsigned char*)const_cast<void*>(host), (size_t)bytes, true) == GSPX_OK)
      return GSPX_OK;
    (void)hipGetLastError();  // no staging memory: the plain copy below
  }
  HIPCHK(hipMemcpyAsync(b->mem.p, host, (size_t)bytes, hipMemcpyHostToDevice, b->ctx->stream));
  HIPCHK(hipStreamSynchronize(b->ctx->stream));
  return GSPX_OK;
}

extern "C" int gspx_buf_download(gspx_buf* b, void* host, int64_t bytes) {
  if (!b || (!host && bytes > 0) || bytes < 0 || bytes > b->bytes)
    return set_err(GSPX_ERR_INVALID, "gspx_buf_download: bad argument");
  HIPCHK(hipSetDevice(b->ctx->device));
  if (bytes == 0) return GSPX_OK;
  if (b->ctx->opt.staged_copy && (size_t)bytes >= ((size_t)b->ctx->opt.staged_copy_min_mb << 20)) {
    HIPCHK(hipStreamSynchronize(b->ctx->stream));  // the kernels that produce the buffer are done
    if (staged_copy(b->ctx, (unsigned char*)b->mem.p, (unsigned char*)host, (size_t)bytes, false) == GSPX_OK) return GSPX_OK;
    (void)hipGetLastError();
  }
  HIPCHK(hipMemcpyAsync(host, b->mem.p, (size_t)bytes, hipMemcpyDeviceToHost, b->ctx->stream));
  HIPCHK(hipStreamSynchronize(b->ctx->stream));
  return GSPX_OK;
}

extern "C" int gspx_buf_ptr(gspx_buf* b, void** p) {
  if (!b || !p) return set_err(GSPX_ERR_INVALID, "gspx_buf_ptr: null argument");
  *p = b->mem.p;
  return GSPX_OK;
}

// Which device a pointer belongs to, as THIS library's HIP runtime sees it: the gate for pointers another library
// allocated (pygsp_amd.nn).  A process can hold two HIP runtimes, and a pointer of the other one means nothing here.
// No kernel, no memory access; a failed query leaves no sticky error behind.
extern "C" int gspx_ptr_device(const void* p, int* device) {
  if (!p || !device) return set_err(GSPX_ERR_INVALID, "gspx_ptr_device: null argument");
  *device = -1;
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof(a));
  const hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return set_err(GSPX_ERR_INVALID, "gspx_ptr_device: not a pointer this HIP runtime knows (%s)", hipGetErrorName(e));
  }
  if (a.type != hipMemoryTypeDevice)
    return set_err(GSPX_ERR_INVALID, "gspx_ptr_device: not device memory of this HIP runtime (memory type %d)",
                   (int)a.type);
  *device = a.device;
  return GSPX_OK;
}

extern "C" int gspx_buf_bytes(gspx_buf* b, int64_t* bytes) {
  if (!b || !bytes) return set_err(GSPX_ERR_INVALID, "gspx_buf_bytes: null argument");
  *bytes = b->bytes;
  return GSPX_OK;
}

extern "C" int gspx_last_host_timing(gspx_ctx* ctx, double out[9]) {
  if (!ctx || !out) return set_err(GSPX_ERR_INVALID, "null argument");
  for (int i = 0; i < 9; ++i) out[i] = ctx->pipe ? ctx->pipe->timing[i] : 0.0;
  return GSPX_OK;
}

extern "C" int gspx_last_host_timeline(gspx_ctx* ctx, double* out, int capacity, int* batches) {
  if (!ctx || !batches) return set_err(GSPX_ERR_INVALID, "null argument");
  const std::vector<double> empty;
  const std::vector<double>& t = ctx->pipe ? ctx->pipe->timeline : empty;
  *batches = (int)(t.size() / 6);
  if (out)
    for (int i = 0; i < capacity && i < (int)t.size(); ++i) out[i] = t[(size_t)i];
  return GSPX_OK;
}

extern "C" int gspx_last_timing(gspx_ctx* ctx, double out[5]) {
  if (!ctx || !out) return set_err(GSPX_ERR_INVALID, "null argument");
  for (int i = 0; i < 5; ++i) out[i] = ctx->timing[i];
  return GSPX_OK;
}

extern "C" int gspx_last_step_kinds(gspx_ctx* ctx, int64_t out[2]) {
  if (!ctx || !out) return set_err(GSPX_ERR_INVALID, "null argument");
  out[0] = ctx->step_kinds[0];
  out[1] = ctx->step_kinds[1];
  return GSPX_OK;
}
