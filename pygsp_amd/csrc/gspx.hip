// gspx.hip — host side of libgspx (C-ABI in include/gspx.h) for MI355X / gfx950.
//
// Replaces, for ONE hot path of epfl-lts2/pygsp:
//   pygsp/filters/approximations.py:58-114  cheby_op           -> gspx_cheby_filter[_dev]
//   pygsp/filters/filter.py:313-322         synthesis loop     -> mode GSPX_SYNTHESIS
//   pygsp/graphs/graph.py:510-630, 830-838  compute_laplacian  -> gspx_graph_create_from_w
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC gspx.hip -o libgspx.so
#include "gspx_kernels.hip.h"
#include "gspx_tile_kernels.hip.h"
// (The kernels that measured slower than what runs by default - two recurrence orders per launch, the fused Newton
// pair, the small pair kernel, 128-row blocks - were retired in round 6; their counter-backed records are
// profiles/r04_pair_experiment.md, profiles/r05_pair_experiment.md and profiles/r05_narrow_rows.md.)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <numeric>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <sys/mman.h>

#include "../../include/gspx.h"
#include "../../include/gspx_ext.h"

using namespace gspx;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;

static int set_err(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return set_err(GSPX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                     __FILE__, __LINE__);                                                   \
  } while (0)

#define CHK(expr)               \
  do {                          \
    int rc_ = (expr);           \
    if (rc_ != GSPX_OK) return rc_; \
  } while (0)

extern "C" const char* gspx_last_error(void) { return g_err.c_str(); }
extern "C" const char* gspx_version(void) { return "gspx 0.1 (gfx950)"; }

// ------------------------------------------------------------------------------------------------
// small RAII device allocation
// ------------------------------------------------------------------------------------------------
// Plain buffers are one hipMalloc.  The two streamed workspaces of a context (T_k slots, accumulators)
// are "streamed" buffers: from 32 MB on they are assembled from 2 MB physical chunks (hipMemCreate)
// mapped in a scrambled order into one reserved address range.  On MI355X the physical placement of a
// streamed buffer moves its bandwidth by several percent - a plain copy of 2 x 1 GiB runs at
// 5.3-5.4 TB/s from hipMalloc memory and 5.7-6.0 from scrambled 2 MB chunks - and the recurrence
// follows it.
// Safety rules of the mapping.  Round 1 shipped a version that, on growth, unmapped the chunks, gave the
// address range back (hipMemAddressFree), reserved a larger one and mapped recycled chunks into it; on
// ROCm 7.0 the next kernels then read through stale translations (fp64 error 4e-2 in the fuzz test).
// The bisect of round 2 (profiles/r02_vmm_bisect.log: same test, five allocator policies) showed that a
// device synchronisation before the unmap does NOT cure it and that never handing an address range back
// does.  Hence:
//   * a range GROWS IN PLACE: the reservation is larger than the first request (address space only) and
//     later requests map more chunks behind the ones already there; nothing is unmapped while the buffer
//     lives;
//   * release() synchronises the device, unmaps and frees the physical chunks, and RETIRES the address
//     range: it stays reserved for the life of the process, so no later mapping can ever alias it
//     (costs address space only: at most max(2 x size, 1 GiB) of the 2^47-byte space per retired buffer);
//   * a request beyond the reservation retires the range that way and starts a new one.
static std::atomic<size_t> g_retired_va_bytes{0};  // address space of retired ranges (never handed back)

struct DevMem {
  void* p = nullptr;
  size_t bytes = 0;     // usable bytes
  bool streamed = false;  // eligible for the chunked mapping (set once by the owner)
  // chunked mapping
  size_t va_size = 0;   // > 0: p is a reserved address range of that many bytes
  size_t mapped = 0;    // bytes mapped from its start (a multiple of chunk)
  size_t chunk = 0;
  struct Piece { hipMemGenericAllocationHandle_t h; size_t off; };
  std::vector<Piece> pieces;
  DevMem() = default;
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  ~DevMem() { release(); }
  void release() {
    if (p && va_size) {
      (void)hipDeviceSynchronize();  // nothing in flight may still translate through the range
      for (const Piece& pc : pieces) {
        (void)hipMemUnmap((char*)p + pc.off, chunk);
        (void)hipMemRelease(pc.h);
      }
      pieces.clear();
      (void)hipGetLastError();  // the range itself is retired, never freed (see above)
      g_retired_va_bytes += va_size;
    } else if (p) {
      (void)hipFree(p);
    }
    p = nullptr;
    bytes = 0;
    va_size = 0;
    mapped = 0;
  }
  // map chunks so that [0, n) of the range is backed; false on any failure (the range stays consistent:
  // what was mapped before the call is still mapped)
  bool map_up_to(size_t n) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = dev;
    const size_t want = (n + chunk - 1) / chunk * chunk;
    if (want <= mapped) return true;
    if (want > va_size) return false;
    const size_t base = mapped, cnt = (want - mapped) / chunk;
    size_t mult = 257;  // coprime with the piece count: a scrambled, fixed order that visits every slot once
    while (cnt > 1 && std::gcd(mult, cnt) != 1) mult += 2;
    const size_t first = pieces.size();
    bool ok = true;
    for (size_t i = 0; i < cnt && ok; ++i) {
      hipMemGenericAllocationHandle_t h;
      ok = hipMemCreate(&h, chunk, &prop, 0) == hipSuccess;
      if (!ok) break;
      const size_t off = base + ((i * mult) % cnt) * chunk;
      if (hipMemMap((char*)p + off, chunk, 0, h, 0) != hipSuccess) {
        (void)hipMemRelease(h);
        ok = false;
        break;
      }
      pieces.push_back({h, off});
    }
    if (ok) {
      hipMemAccessDesc acc = {};
      acc.location = prop.location;
      acc.flags = hipMemAccessFlagsProtReadWrite;
      ok = hipMemSetAccess((char*)p + base, want - base, &acc, 1) == hipSuccess;
    }
    if (!ok) {  // undo this call's pieces only
      (void)hipDeviceSynchronize();
      while (pieces.size() > first) {
        (void)hipMemUnmap((char*)p + pieces.back().off, chunk);
        (void)hipMemRelease(pieces.back().h);
        pieces.pop_back();
      }
      (void)hipGetLastError();
      return false;
    }
    mapped = want;
    return true;
  }
  bool alloc_chunked(size_t n) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = dev;
    size_t gran = 0;
    if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || !gran)
      return false;
    size_t c = (size_t)2 << 20;
    c = (c + gran - 1) / gran * gran;
    const size_t need = (n + c - 1) / c * c;
    // room to grow in place: twice the request, at least 1 GiB (address space only)
    const size_t reserve = std::max<size_t>(2 * need, (size_t)1 << 30);
    void* va = nullptr;
    if (hipMemAddressReserve(&va, reserve, 0, nullptr, 0) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    p = va;
    va_size = reserve;
    chunk = c;
    mapped = 0;
    pieces.clear();
    if (!map_up_to(n)) {  // nothing was ever mapped into this range: safe to hand back
      (void)hipMemAddressFree(va, reserve);
      (void)hipGetLastError();
      p = nullptr;
      va_size = 0;
      return false;
    }
    bytes = n;
    return true;
  }
  int alloc(size_t n) {
    release();
    if (n == 0) n = 16;
    if (streamed && n >= ((size_t)32 << 20) && alloc_chunked(n)) return GSPX_OK;
    (void)hipGetLastError();
    hipError_t e = hipMalloc(&p, n);
    if (e != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();  // an allocation failure is not sticky: the caller may free memory and try again
      return set_err(e == hipErrorOutOfMemory ? GSPX_ERR_OOM : GSPX_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", n,
                     hipGetErrorString(e));
    }
    bytes = n;
    return GSPX_OK;
  }
  int ensure(size_t n) {  // grow-only
    if (n <= bytes && p) return GSPX_OK;
    if (p && va_size && n <= va_size && map_up_to(n)) {  // grow in place
      bytes = n;
      return GSPX_OK;
    }
    return alloc(n);
  }
  template <typename T> T* as() const { return (T*)p; }
  void swap(DevMem& o) {  // exchange the backing of two buffers (placement tuning: candidates against the live workspace)
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
    std::swap(streamed, o.streamed);
    std::swap(va_size, o.va_size);
    std::swap(mapped, o.mapped);
    std::swap(chunk, o.chunk);
    pieces.swap(o.pieces);
  }
};

// pinned host memory and the per-context state of the pipelined host-pointer entry point
// (gspx_hostpipe.hip.h): two staging panels per direction, two device panels per direction, a stream per
// copy direction
struct PinMem {
  void* p = nullptr;
  size_t bytes = 0;
  PinMem() = default;
  PinMem(const PinMem&) = delete;
  PinMem& operator=(const PinMem&) = delete;
  ~PinMem() { release(); }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
  }
  int ensure(size_t n) {
    if (p && n <= bytes) return GSPX_OK;
    release();
    hipError_t e = hipHostMalloc(&p, n, hipHostMallocDefault);
    if (e != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();
      return set_err(GSPX_ERR_HIP, "hipHostMalloc(%zu bytes) failed: %s", n, hipGetErrorString(e));
    }
    bytes = n;
    return GSPX_OK;
  }
};

// Large transfers between pageable host memory and a device buffer (gspx_buf_upload / gspx_buf_download: what
// engine.DeviceArray and Context.upload move): a pageable hipMemcpy is staged by the runtime on one thread at
// ~25 GB/s.  Here the buffer is cut into 16 MB chunks that a few host threads copy into / out of three pinned
// staging chunks while the DMA engine ships the previous ones - the link's rate instead of a single core's.
struct CopyStage {
  static constexpr int NS = 3;
  static constexpr size_t CHUNK = (size_t)16 << 20;
  PinMem pin[NS];
  hipEvent_t ev[NS] = {nullptr, nullptr, nullptr};
  hipStream_t st = nullptr;
  bool ready = false;
  int init() {
    if (ready) return GSPX_OK;
    for (auto& pm : pin) CHK(pm.ensure(CHUNK));
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (auto& e : ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ready = true;
    return GSPX_OK;
  }
  void destroy() {
    if (st) (void)hipStreamDestroy(st);
    st = nullptr;
    for (auto& e : ev) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
    for (auto& pm : pin) pm.release();
    ready = false;
  }
};

struct HostPipe {
  static constexpr int NIN = 3;  // input slots: batch b is packed and shipped while batches b-1 and b-2 compute
  hipStream_t stream_in = nullptr, stream_out = nullptr;
  hipEvent_t h2d_ev[NIN] = {nullptr, nullptr, nullptr};
  hipEvent_t t_in[NIN][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};  // per slot: H2D start / stop
  hipEvent_t t_out[2] = {nullptr, nullptr};                          // D2H start / stop (the shipper waits for each)
  PinMem pin_in[NIN], pin_out[2];
  DevMem dx[NIN], dy[2];
  // timings of the last pipelined call (ms): wall, pack (busiest worker), H2D (sum of DMA times), kernels
  // (sum of device times), D2H, unpack (busiest worker), batches, batch width, host threads per direction
  double timing[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  // host clock (ms since the call began) per batch of the last pipelined call: packed, H2D issued, kernels begun,
  // kernels done, D2H done, unpacked
  std::vector<double> timeline;
  bool ready = false;
  int init() {
    if (ready) return GSPX_OK;
    HIPCHK(hipStreamCreateWithFlags(&stream_in, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&stream_out, hipStreamNonBlocking));
    for (auto& e : h2d_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& sl : t_in)
      for (auto& e : sl) HIPCHK(hipEventCreate(&e));
    for (auto& e : t_out) HIPCHK(hipEventCreate(&e));
    ready = true;
    return GSPX_OK;
  }
  void destroy() {
    if (stream_in) (void)hipStreamDestroy(stream_in);
    if (stream_out) (void)hipStreamDestroy(stream_out);
    for (auto& e : h2d_ev)
      if (e) (void)hipEventDestroy(e);
    for (auto& sl : t_in)
      for (auto& e : sl) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
      }
    for (auto& e : t_out) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
    stream_in = stream_out = nullptr;
    for (auto& e : h2d_ev) e = nullptr;
    for (int i = 0; i < NIN; ++i) {
      pin_in[i].release();
      dx[i].release();
    }
    for (int i = 0; i < 2; ++i) {
      pin_out[i].release();
      dy[i].release();
    }
    ready = false;
  }
};

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
  double timing[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // [5], [6]: LDS bytes / resident workgroups of the last pair-filter call
  // hipGraph replay of a repeated identical filter call (launch-bound small graphs)
  bool capturing = false;     // run_batch is being recorded: no copies, syncs or events inside
  // identity of a call = the full tuple of everything the recorded launches depend on, compared
  // byte for byte (not a hash of it: a collision would replay the wrong graph silently)
  std::vector<unsigned char> seen_key;   // key of the last eager call (empty: none)
  std::vector<unsigned char> graph_key;  // key the instantiated graph was captured for
  hipGraphExec_t graph_exec = nullptr;
};

// any other work on the context invalidates a recorded replay (it may have rewritten the weights,
// the cached gather offsets or the workspace the graph refers to)
static std::atomic<int> g_live_ctx[64];  // live contexts per device (zero-initialised)

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
  int64_t n_edges = 0;
  DevMem e_off, e_toff, e_src, e_dst, e_tedge, e_cs, e_ct, e_w;
};

static size_t elt_size(int dtype) { return dtype == GSPX_F32 ? 4 : 8; }

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

static void comm_invalidate_all(gspx_ctx* ctx);  // gspx_comm.hip.h

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

static int64_t* option_slot(Options& o, const char* key) {
  if (!key) return nullptr;
  if (!strcmp(key, "kernel")) return &o.kernel;
  if (!strcmp(key, "vec")) return &o.vec;
  if (!strcmp(key, "rows_per_wave")) return &o.rows_per_wave;
  if (!strcmp(key, "narrow_g_log2")) return &o.narrow_g_log2;
  if (!strcmp(key, "waves_per_block")) return &o.waves_per_block;
  if (!strcmp(key, "alternate_sweep")) return &o.alternate_sweep;
  if (!strcmp(key, "synthesis")) return &o.synthesis;
  if (!strcmp(key, "tile_gather")) return &o.tile_gather;
  if (!strcmp(key, "graph_launch")) return &o.graph_launch;
  if (!strcmp(key, "tile_workgroups")) return &o.tile_workgroups;
  if (!strcmp(key, "tile_lg")) return &o.tile_lg;
  if (!strcmp(key, "tile_regroup")) return &o.tile_regroup;
  if (!strcmp(key, "staged_copy")) return &o.staged_copy;
  if (!strcmp(key, "staged_copy_min_mb")) return &o.staged_copy_min_mb;
  if (!strcmp(key, "copy_threads")) return &o.copy_threads;
  if (!strcmp(key, "tile_min_row")) return &o.tile_min_row;
  if (!strcmp(key, "tile_pad")) return &o.tile_pad;
  if (!strcmp(key, "knn_f32")) return &o.knn_f32;
  if (!strcmp(key, "tile_nt")) return &o.tile_nt;
  if (!strcmp(key, "fuse_input")) return &o.fuse_input;
  if (!strcmp(key, "edge_vertex_walk")) return &o.edge_vertex_walk;
  if (!strcmp(key, "xcd_remap")) return &o.xcd_remap;
  if (!strcmp(key, "combine")) return &o.combine;
  if (!strcmp(key, "ws_limit_mb")) return &o.ws_limit_mb;
  if (!strcmp(key, "max_batch")) return &o.max_batch;
  if (!strcmp(key, "gather_rccl")) return &o.gather_rccl;
  if (!strcmp(key, "lds_pad_kb")) return &o.lds_pad_kb;
  if (!strcmp(key, "host_pipeline")) return &o.host_pipeline;
  if (!strcmp(key, "host_batch")) return &o.host_batch;
  if (!strcmp(key, "host_edge")) return &o.host_edge;
  if (!strcmp(key, "host_threads")) return &o.host_threads;
  if (!strcmp(key, "streamed_alloc")) return &o.streamed_alloc;
  return nullptr;
}

extern "C" int gspx_ctx_set_option(gspx_ctx* ctx, const char* key, int64_t value) {
  replay_reset(ctx);
  if (!ctx) return set_err(GSPX_ERR_INVALID, "null ctx");
  int64_t* s = option_slot(ctx->opt, key);
  if (!s) return set_err(GSPX_ERR_INVALID, "unknown option '%s'", key ? key : "(null)");
  if (!strcmp(key, "rows_per_wave") && (value < 0 || value > 1024))
    return set_err(GSPX_ERR_INVALID, "rows_per_wave must be in [0, 1024] (0 = auto)");
  if (!strcmp(key, "narrow_g_log2") && (value < -1 || value > 6))
    return set_err(GSPX_ERR_INVALID, "narrow_g_log2 must be in [-1, 6] (-1 = auto)");
  if (!strcmp(key, "waves_per_block") && !(value == 4 || value == 8 || value == 16))
    return set_err(GSPX_ERR_INVALID, "waves_per_block must be 4, 8 or 16");
  if (!strcmp(key, "kernel") && !(value == 0 || value == 1 || value == 2 || value == 5))
    return set_err(GSPX_ERR_INVALID, "kernel must be 0 (auto), 1 (panel), 2 (narrow) or 5 (LDS-staged)");
  if (!strcmp(key, "vec") && !(value == 0 || value == 1 || value == 2 || value == 4))
    return set_err(GSPX_ERR_INVALID, "vec must be 0, 1, 2 or 4");
  *s = value;
  if (!strcmp(key, "streamed_alloc")) {
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
  int64_t* s = option_slot(ctx->opt, key);
  if (!s) return set_err(GSPX_ERR_INVALID, "unknown option '%s'", key ? key : "(null)");
  *value = *s;
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

#include "gspx_comm.hip.h"

// The path's one collective in single-process form: every part (a buffer on its own context /
// device) lands in root_out, one after the other in argument order.  Between devices the blocks travel
// as grouped RCCL send / recv pairs (gather_rccl, gspx_comm.hip.h), each over its own xGMI link.  If RCCL
// cannot be loaded or refuses the device set, the same gather is done with peer copies: each queued on
// the SOURCE context's stream (hipMemcpyPeerAsync, DMA engines); same-device parts are device copies.
extern "C" int gspx_gather(gspx_ctx** ctxs, int n, gspx_buf** parts, gspx_buf* root_out) {
  if (n < 0 || (n > 0 && !parts) || !root_out)
    return set_err(GSPX_ERR_INVALID, "gspx_gather: bad argument");
  int64_t total = 0;
  for (int i = 0; i < n; ++i) {
    if (!parts[i]) return set_err(GSPX_ERR_INVALID, "gspx_gather: null part");
    if (ctxs && ctxs[i] && ctxs[i] != parts[i]->ctx)
      return set_err(GSPX_ERR_INVALID, "gspx_gather: part %d does not belong to context %d", i, i);
    if (parts[i] == root_out) return set_err(GSPX_ERR_INVALID, "gspx_gather: a part aliases the output");
    total += parts[i]->bytes;
  }
  if (total > root_out->bytes)
    return set_err(GSPX_ERR_INVALID, "gspx_gather: output holds %lld bytes, parts add up to %lld",
                   (long long)root_out->bytes, (long long)total);
  gspx_ctx* root = root_out->ctx;
  if (root->opt.gather_rccl > 0) {
    bool multi = false;
    for (int i = 0; i < n; ++i) multi |= parts[i]->ctx->device != root->device;
    if (multi || root->opt.gather_rccl == 2) {
      if (gather_rccl(n, parts, root_out, root->opt.gather_rccl == 2) == GSPX_OK) return GSPX_OK;
      if (root->opt.gather_rccl == 2) return GSPX_ERR_HIP;  // asked for RCCL explicitly: report why not
      (void)hipGetLastError();  // otherwise: peer copies below
    }
  }
  HIPCHK(hipSetDevice(root->device));
  HIPCHK(hipStreamSynchronize(root->stream));  // earlier work on the output buffer
  int64_t off = 0;
  for (int i = 0; i < n; ++i) {
    gspx_ctx* src = parts[i]->ctx;
    const size_t nb = (size_t)parts[i]->bytes;
    if (nb) {
      HIPCHK(hipSetDevice(src->device));
      unsigned char* dst = (unsigned char*)root_out->mem.p + off;
      if (src->device == root->device) {
        HIPCHK(hipMemcpyAsync(dst, parts[i]->mem.p, nb, hipMemcpyDeviceToDevice, src->stream));
      } else {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, src->device, root->device) == hipSuccess && can) {
          const hipError_t e = hipDeviceEnablePeerAccess(root->device, 0);
          if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
            return set_err(GSPX_ERR_HIP, "hipDeviceEnablePeerAccess: %s", hipGetErrorString(e));
          (void)hipGetLastError();
        }
        HIPCHK(hipMemcpyPeerAsync(dst, root->device, parts[i]->mem.p, src->device, nb, src->stream));
      }
    }
    off += parts[i]->bytes;
  }
  for (int i = 0; i < n; ++i) {
    HIPCHK(hipSetDevice(parts[i]->ctx->device));
    HIPCHK(hipStreamSynchronize(parts[i]->ctx->stream));
  }
  HIPCHK(hipSetDevice(root->device));
  return GSPX_OK;
}

extern "C" int gspx_buf_ptr(gspx_buf* b, void** p) {
  if (!b || !p) return set_err(GSPX_ERR_INVALID, "gspx_buf_ptr: null argument");
  *p = b->mem.p;
  return GSPX_OK;
}

extern "C" int gspx_buf_bytes(gspx_buf* b, int64_t* bytes) {
  if (!b || !bytes) return set_err(GSPX_ERR_INVALID, "gspx_buf_bytes: null argument");
  *bytes = b->bytes;
  return GSPX_OK;
}

// ------------------------------------------------------------------------------------------------
// device exclusive scan of n int32 (in-place safe: out may equal in)
// ------------------------------------------------------------------------------------------------
static int scan_exclusive(gspx_ctx* ctx, const int* in, int* out, int n) {
  if (n <= 0) return GSPX_OK;
  const int ntiles = (n + GSPX_SCAN_TILE - 1) / GSPX_SCAN_TILE;
  DevMem sums;
  CHK(sums.alloc((size_t)ntiles * sizeof(int)));
  hipLaunchKernelGGL(k_scan_tiles, dim3(ntiles), dim3(256), 0, ctx->stream, in, n, out,
                     sums.as<int>());
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(256), 0, ctx->stream, sums.as<int>(), ntiles);
  hipLaunchKernelGGL(k_scan_add, dim3(ntiles), dim3(256), 0, ctx->stream, out, n, sums.as<int>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return GSPX_OK;
}

// ------------------------------------------------------------------------------------------------
// graph construction
// ------------------------------------------------------------------------------------------------
static int validate_csr(int64_t N, int64_t nnz, const int32_t* indptr, const int32_t* indices) {
  if (N < 0 || nnz < 0) return set_err(GSPX_ERR_INVALID, "negative N or nnz");
  if (N >= (int64_t)1 << 30) return set_err(GSPX_ERR_INVALID, "N too large (%lld)", (long long)N);
  if (nnz >= ((int64_t)1 << 31) - 8 * N - 64)
    return set_err(GSPX_ERR_INVALID, "nnz too large for int32 indexing (%lld)", (long long)nnz);
  if (!indptr || (nnz > 0 && !indices)) return set_err(GSPX_ERR_INVALID, "null CSR arrays");
  if (indptr[0] != 0 || indptr[N] != nnz)
    return set_err(GSPX_ERR_INVALID, "indptr[0] must be 0 and indptr[N] must equal nnz");
  for (int64_t i = 0; i < N; ++i) {
    const int32_t s = indptr[i], e = indptr[i + 1];
    if (e < s) return set_err(GSPX_ERR_INVALID, "indptr not monotone at row %lld", (long long)i);
    for (int32_t j = s; j < e; ++j) {
      const int32_t c = indices[j];
      if (c < 0 || c >= N)
        return set_err(GSPX_ERR_INVALID, "column index %d out of range in row %lld", c,
                       (long long)i);
      if (j > s && indices[j - 1] >= c)
        return set_err(GSPX_ERR_INVALID,
                       "row %lld is not canonical (indices must be strictly ascending)",
                       (long long)i);
    }
  }
  return GSPX_OK;
}

template <typename T>
static void convert_values(const void* data, int data_dtype, int64_t n, std::vector<T>& out) {
  out.resize((size_t)n);
  if (data_dtype == GSPX_F32) {
    const float* p = (const float*)data;
    for (int64_t i = 0; i < n; ++i) out[(size_t)i] = (T)p[i];
  } else {
    const double* p = (const double*)data;
    for (int64_t i = 0; i < n; ++i) out[(size_t)i] = (T)p[i];
  }
}

static int upload_perm(gspx_graph* g, const int32_t* perm) {
  const int64_t N = g->N;
  g->has_perm = false;
  if (!perm || N == 0) return GSPX_OK;
  std::vector<char> seen((size_t)N, 0);
  bool identity = true;
  for (int64_t i = 0; i < N; ++i) {
    const int32_t p = perm[i];
    if (p < 0 || p >= N || seen[(size_t)p])
      return set_err(GSPX_ERR_INVALID, "perm is not a permutation of 0..N-1");
    seen[(size_t)p] = 1;
    if (p != i) identity = false;
  }
  if (identity) return GSPX_OK;
  gspx_ctx* ctx = g->ctx;
  CHK(g->perm.alloc((size_t)N * sizeof(int)));
  CHK(g->iperm.alloc((size_t)N * sizeof(int)));
  HIPCHK(hipMemcpyAsync(g->perm.p, perm, (size_t)N * sizeof(int), hipMemcpyHostToDevice,
                        ctx->stream));
  const int nb = (int)((N + 255) / 256);
  hipLaunchKernelGGL(k_inverse_perm, dim3(nb), dim3(256), 0, ctx->stream, g->perm.as<int>(),
                     (int)N, g->iperm.as<int>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));
  g->has_perm = true;
  return GSPX_OK;
}

// canonical L (device) -> internal padded CSR
template <typename T> static int build_internal(gspx_graph* g) {
  gspx_ctx* ctx = g->ctx;
  const int N = (int)g->N;
  const int nb = std::max(1, (N + 255) / 256);
  const int* perm = g->has_perm ? g->perm.as<int>() : nullptr;
  const int* iperm = g->has_perm ? g->iperm.as<int>() : nullptr;
  DevMem cnt;
  CHK(cnt.alloc((size_t)(N + 1) * sizeof(int)));
  HIPCHK(hipMemsetAsync(cnt.p, 0, (size_t)(N + 1) * sizeof(int), ctx->stream));
  CHK(g->rptr.alloc((size_t)(N + 1 + 16) * sizeof(int)));
  if (N > 0) {
    hipLaunchKernelGGL((k_internal_build<T, false>), dim3(nb), dim3(256), 0, ctx->stream,
                       g->lptr.as<int>(), g->lcol.as<int>(), g->lval.as<T>(), N, perm, iperm,
                       cnt.as<int>(), (int*)nullptr, (int*)nullptr, (T*)nullptr);
    HIPCHK(hipGetLastError());
  }
  CHK(scan_exclusive(ctx, cnt.as<int>(), g->rptr.as<int>(), N + 1));
  int total = 0;
  HIPCHK(hipMemcpy(&total, g->rptr.as<int>() + N, sizeof(int), hipMemcpyDeviceToHost));
  g->nnz_int = total;
  // rows past N read as empty: rowptr[N+1 .. N+16] = total
  hipLaunchKernelGGL((k_fill<int>), dim3(1), dim3(64), 0, ctx->stream, g->rptr.as<int>() + N + 1,
                     (size_t)16, total);
  const size_t cap = (size_t)total + 64;
  CHK(g->rcol.alloc(cap * sizeof(int)));
  CHK(g->rval.alloc(cap * sizeof(T)));
  CHK(g->fval.alloc(cap * sizeof(T)));
  // tail padding (never used by the kernels; keeps any over-read inside the allocation)
  hipLaunchKernelGGL((k_fill<int>), dim3(1), dim3(64), 0, ctx->stream, g->rcol.as<int>() + total,
                     (size_t)64, N);
  hipLaunchKernelGGL((k_fill<T>), dim3(1), dim3(64), 0, ctx->stream, g->rval.as<T>() + total,
                     (size_t)64, T(0));
  hipLaunchKernelGGL((k_fill<T>), dim3(1), dim3(64), 0, ctx->stream, g->fval.as<T>() + total,
                     (size_t)64, T(0));
  if (N > 0) {
    hipLaunchKernelGGL((k_internal_build<T, true>), dim3(nb), dim3(256), 0, ctx->stream,
                       g->lptr.as<int>(), g->lcol.as<int>(), g->lval.as<T>(), N, perm, iperm,
                       (int*)nullptr, g->rptr.as<int>(), g->rcol.as<int>(), g->rval.as<T>());
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));
  g->fval_lmax = -1.0;
  g->coff_ldb = 0;
  return GSPX_OK;
}

// W already on the device (canonical CSR, values in the compute dtype): degrees, Laplacian, internal layout
template <typename T>
static int create_from_w_dev(gspx_graph* g, int64_t nnz, const int* wptr, const int* wcol, const T* wval) {
  gspx_ctx* ctx = g->ctx;
  const int N = (int)g->N;
  const int lap_type = g->lap_type;
  DevMem cnt;
  CHK(g->dw.alloc((size_t)std::max(N, 1) * sizeof(T)));
  const auto t0 = std::chrono::steady_clock::now();
  const int nb = std::max(1, (N + 255) / 256);
  CHK(cnt.alloc((size_t)(N + 1) * sizeof(int)));
  HIPCHK(hipMemsetAsync(cnt.p, 0, (size_t)(N + 1) * sizeof(int), ctx->stream));
  CHK(g->lptr.alloc((size_t)(N + 1) * sizeof(int)));
  if (N > 0) {
    hipLaunchKernelGGL((k_degree<T>), dim3(nb), dim3(256), 0, ctx->stream, wptr, wval, N, g->dw.as<T>());
    hipLaunchKernelGGL((k_lap_build<T, false>), dim3(nb), dim3(256), 0, ctx->stream, wptr, wcol, wval,
                       g->dw.as<T>(), N, lap_type, cnt.as<int>(), (int*)nullptr, (int*)nullptr, (T*)nullptr);
    HIPCHK(hipGetLastError());
  }
  CHK(scan_exclusive(ctx, cnt.as<int>(), g->lptr.as<int>(), N + 1));
  int total = 0;
  HIPCHK(hipMemcpy(&total, g->lptr.as<int>() + N, sizeof(int), hipMemcpyDeviceToHost));
  g->nnz_l = total;
  CHK(g->lcol.alloc((size_t)total * sizeof(int)));
  CHK(g->lval.alloc((size_t)total * sizeof(T)));
  if (N > 0) {
    hipLaunchKernelGGL((k_lap_build<T, true>), dim3(nb), dim3(256), 0, ctx->stream, wptr, wcol, wval,
                       g->dw.as<T>(), N, lap_type, (int*)nullptr, g->lptr.as<int>(), g->lcol.as<int>(),
                       g->lval.as<T>());
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if constexpr (std::is_same<T, double>::value) {
    if (N > 0) {
      DevMem part;
      CHK(part.alloc((size_t)nb * 4 * sizeof(double)));
      hipLaunchKernelGGL(k_lmax_bounds, dim3(nb), dim3(256), 0, ctx->stream, wptr, wcol, wval, g->dw.as<double>(), N,
                         part.as<double>());
      std::vector<double> hp((size_t)nb * 4);
      HIPCHK(hipMemcpyAsync(hp.data(), part.p, hp.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      std::vector<double> hd((size_t)N);
      HIPCHK(hipMemcpyAsync(hd.data(), g->dw.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      double wmax = 0.0 /* a sparse matrix's maximum sees its implicit zeros */, emax = -1e300, mmax = -1e300, zeros = 0;
      if ((int64_t)N * N == nnz) wmax = -1e300;  // (a full matrix has none)
      for (int b = 0; b < nb; ++b) {
        wmax = std::max(wmax, hp[(size_t)b * 4 + 0]);
        emax = std::max(emax, hp[(size_t)b * 4 + 1]);
        mmax = std::max(mmax, hp[(size_t)b * 4 + 2]);
        zeros += hp[(size_t)b * 4 + 3];
      }
      double dmax = hd[0];
      for (double v : hd) dmax = std::max(dmax, v);
      g->bounds[0] = wmax;
      g->bounds[1] = dmax;
      g->bounds[2] = emax;
      g->bounds[3] = zeros > 0 ? std::nan("") : mmax;
      g->has_bounds = true;
    }
  }
  CHK(build_internal<T>(g));
  g->build_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return GSPX_OK;
}

template <typename T>
static int create_from_w_t(gspx_graph* g, int64_t nnz, const int32_t* indptr,
                           const int32_t* indices, const void* data, int data_dtype,
                           int lap_type) {
  const int N = (int)g->N;
  std::vector<T> vals;
  convert_values<T>(data, data_dtype, nnz, vals);
  DevMem wptr, wcol, wval;
  CHK(wptr.alloc((size_t)(N + 1) * sizeof(int)));
  CHK(wcol.alloc((size_t)nnz * sizeof(int)));
  CHK(wval.alloc((size_t)nnz * sizeof(T)));
  HIPCHK(hipMemcpy(wptr.p, indptr, (size_t)(N + 1) * sizeof(int), hipMemcpyHostToDevice));
  if (nnz > 0) {
    HIPCHK(hipMemcpy(wcol.p, indices, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(wval.p, vals.data(), (size_t)nnz * sizeof(T), hipMemcpyHostToDevice));
  }
  return create_from_w_dev<T>(g, nnz, wptr.as<int>(), wcol.as<int>(), wval.as<T>());
}

template <typename T>
static int create_from_l_t(gspx_graph* g, int64_t nnz, const int32_t* indptr,
                           const int32_t* indices, const void* data, int data_dtype) {
  const int N = (int)g->N;
  std::vector<T> vals;
  convert_values<T>(data, data_dtype, nnz, vals);
  CHK(g->lptr.alloc((size_t)(N + 1) * sizeof(int)));
  CHK(g->lcol.alloc((size_t)nnz * sizeof(int)));
  CHK(g->lval.alloc((size_t)nnz * sizeof(T)));
  HIPCHK(hipMemcpy(g->lptr.p, indptr, (size_t)(N + 1) * sizeof(int), hipMemcpyHostToDevice));
  if (nnz > 0) {
    HIPCHK(hipMemcpy(g->lcol.p, indices, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(g->lval.p, vals.data(), (size_t)nnz * sizeof(T), hipMemcpyHostToDevice));
  }
  g->nnz_l = nnz;
  const auto t0 = std::chrono::steady_clock::now();
  CHK(build_internal<T>(g));
  g->build_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return GSPX_OK;
}

static int graph_create_common(gspx_ctx* ctx, int64_t N, int64_t nnz, const int32_t* indptr,
                               const int32_t* indices, const void* data, int data_dtype,
                               int lap_type, int compute_dtype, const int32_t* perm, bool from_w,
                               gspx_graph** out) {
  if (!ctx || !out) return set_err(GSPX_ERR_INVALID, "null ctx or output");
  *out = nullptr;
  if (data_dtype != GSPX_F32 && data_dtype != GSPX_F64)
    return set_err(GSPX_ERR_INVALID, "data_dtype must be GSPX_F32 or GSPX_F64");
  if (compute_dtype != GSPX_F32 && compute_dtype != GSPX_F64)
    return set_err(GSPX_ERR_INVALID, "compute_dtype must be GSPX_F32 or GSPX_F64");
  if (from_w && lap_type != GSPX_LAP_COMBINATORIAL && lap_type != GSPX_LAP_NORMALIZED)
    return set_err(GSPX_ERR_INVALID, "Unknown Laplacian type %d", lap_type);
  if (nnz > 0 && !data) return set_err(GSPX_ERR_INVALID, "null data");
  CHK(validate_csr(N, nnz, indptr, indices));
  HIPCHK(hipSetDevice(ctx->device));
  gspx_graph* g = new gspx_graph();
  g->ctx = ctx;
  g->N = N;
  g->dtype = compute_dtype;
  g->from_w = from_w;
  g->lap_type = lap_type;
  int rc = upload_perm(g, perm);
  if (rc == GSPX_OK) {
    if (from_w) {
      rc = compute_dtype == GSPX_F32
               ? create_from_w_t<float>(g, nnz, indptr, indices, data, data_dtype, lap_type)
               : create_from_w_t<double>(g, nnz, indptr, indices, data, data_dtype, lap_type);
    } else {
      rc = compute_dtype == GSPX_F32
               ? create_from_l_t<float>(g, nnz, indptr, indices, data, data_dtype)
               : create_from_l_t<double>(g, nnz, indptr, indices, data, data_dtype);
    }
  }
  if (rc != GSPX_OK) {
    delete g;
    return rc;
  }
  *out = g;
  return GSPX_OK;
}

extern "C" int gspx_graph_create_from_w(gspx_ctx* ctx, int64_t N, int64_t nnz,
                                        const int32_t* indptr, const int32_t* indices,
                                        const void* data, int data_dtype, int lap_type,
                                        int compute_dtype, const int32_t* perm,
                                        gspx_graph** out) {
  return graph_create_common(ctx, N, nnz, indptr, indices, data, data_dtype, lap_type,
                             compute_dtype, perm, true, out);
}

extern "C" int gspx_graph_create_from_l(gspx_ctx* ctx, int64_t N, int64_t nnz,
                                        const int32_t* indptr, const int32_t* indices,
                                        const void* data, int data_dtype, int compute_dtype,
                                        const int32_t* perm, gspx_graph** out) {
  return graph_create_common(ctx, N, nnz, indptr, indices, data, data_dtype, 0, compute_dtype,
                             perm, false, out);
}

extern "C" int gspx_graph_destroy(gspx_graph* g) {
  if (g) replay_reset(g->ctx);
  if (!g) return GSPX_OK;
  (void)hipSetDevice(g->ctx->device);
  (void)hipStreamSynchronize(g->ctx->stream);
  delete g;
  return GSPX_OK;
}

extern "C" int gspx_graph_n(gspx_graph* g, int64_t* N) {
  if (!g || !N) return set_err(GSPX_ERR_INVALID, "null argument");
  *N = g->N;
  return GSPX_OK;
}
extern "C" int gspx_graph_nnz_l(gspx_graph* g, int64_t* nnz) {
  if (!g || !nnz) return set_err(GSPX_ERR_INVALID, "null argument");
  *nnz = g->nnz_l;
  return GSPX_OK;
}
extern "C" int gspx_graph_nnz_internal(gspx_graph* g, int64_t* nnz) {
  if (!g || !nnz) return set_err(GSPX_ERR_INVALID, "null argument");
  *nnz = g->nnz_int;
  return GSPX_OK;
}
extern "C" int gspx_graph_build_ms(gspx_graph* g, double* ms) {
  if (!g || !ms) return set_err(GSPX_ERR_INVALID, "null argument");
  *ms = g->build_ms;
  return GSPX_OK;
}

extern "C" int gspx_graph_download_l(gspx_graph* g, int32_t* indptr, int32_t* indices,
                                     void* data) {
  if (!g || !indptr) return set_err(GSPX_ERR_INVALID, "null argument");
  if (g->nnz_l > 0 && (!indices || !data)) return set_err(GSPX_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(g->ctx->device));
  HIPCHK(hipMemcpy(indptr, g->lptr.p, (size_t)(g->N + 1) * sizeof(int), hipMemcpyDeviceToHost));
  if (g->nnz_l > 0) {
    HIPCHK(hipMemcpy(indices, g->lcol.p, (size_t)g->nnz_l * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(data, g->lval.p, (size_t)g->nnz_l * elt_size(g->dtype),
                     hipMemcpyDeviceToHost));
  }
  return GSPX_OK;
}

extern "C" int gspx_graph_download_dw(gspx_graph* g, void* dw) {
  if (!g || (!dw && g->N > 0)) return set_err(GSPX_ERR_INVALID, "null argument");
  if (!g->from_w) return set_err(GSPX_ERR_INVALID, "graph was created from L: no degree vector");
  HIPCHK(hipSetDevice(g->ctx->device));
  if (g->N > 0)
    HIPCHK(hipMemcpy(dw, g->dw.p, (size_t)g->N * elt_size(g->dtype), hipMemcpyDeviceToHost));
  return GSPX_OK;
}

extern "C" int gspx_graph_lmax_bounds(gspx_graph* g, double out[4]) {
  if (!g || !out) return set_err(GSPX_ERR_INVALID, "null argument");
  if (!g->has_bounds)
    return set_err(GSPX_ERR_INVALID, "no bound ingredients: the graph was not built from W in float64, or is empty");
  for (int i = 0; i < 4; ++i) out[i] = g->bounds[i];
  return GSPX_OK;
}

extern "C" int gspx_graph_download_internal(gspx_graph* g, int32_t* rowptr, int32_t* col) {
  if (!g || !rowptr) return set_err(GSPX_ERR_INVALID, "null argument");
  if (g->nnz_int > 0 && !col) return set_err(GSPX_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(g->ctx->device));
  HIPCHK(hipMemcpy(rowptr, g->rptr.p, (size_t)(g->N + 1) * sizeof(int), hipMemcpyDeviceToHost));
  if (g->nnz_int > 0)
    HIPCHK(hipMemcpy(col, g->rcol.p, (size_t)g->nnz_int * sizeof(int), hipMemcpyDeviceToHost));
  return GSPX_OK;
}


extern "C" int gspx_graph_set_gather_tiles(gspx_graph* g, int block_rows, int nb, const int32_t* s1ptr,
                                           const int32_t* s1rows, const uint16_t* lidx, int64_t* stats) {
  if (g) replay_reset(g->ctx);
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (block_rows == 0) {  // drop the tiles
    g->gt_rows = 0;
    return GSPX_OK;
  }
  if (block_rows != GSPX_TILE_BR)
    return set_err(GSPX_ERR_INVALID, "gather tiles must use %d-row blocks", GSPX_TILE_BR);
  if (!s1ptr || !s1rows || !lidx || nb < 1 || nb != (int)((g->N + block_rows - 1) / block_rows))
    return set_err(GSPX_ERR_INVALID, "gspx_graph_set_gather_tiles: bad argument");
  HIPCHK(hipSetDevice(g->ctx->device));
  std::vector<int> rp((size_t)g->N + 1);
  HIPCHK(hipMemcpy(rp.data(), g->rptr.p, ((size_t)g->N + 1) * sizeof(int), hipMemcpyDeviceToHost));
  for (auto& r : rp) r &= ~3;
  // three workgroups per CU: 52 KB each (h tile + the block's slice of entries)
  const size_t lds = (size_t)52 * 1024;
  const size_t esz = elt_size(g->dtype);
  std::vector<int> hdr((size_t)nb * 4);
  int slow = 0, entmax = 0;
  for (int b = 0; b < nb; ++b) {
    const int lo = s1ptr[b], n1 = s1ptr[b + 1] - lo;
    const int r0 = b * block_rows, r1 = (int)std::min<int64_t>((int64_t)r0 + block_rows, g->N);
    const int ent = rp[r1] - rp[r0];
    if (n1 < 0 || lo < 0) return set_err(GSPX_ERR_INVALID, "gspx_graph_set_gather_tiles: bad s1ptr");
    for (int o = lo; o < lo + n1; ++o)
      if (s1rows[o] < 0 || s1rows[o] >= g->N)
        return set_err(GSPX_ERR_INVALID, "gspx_graph_set_gather_tiles: bad S1 row");
    const size_t need = (size_t)n1 * 256 + (((size_t)ent * esz + 15) & ~(size_t)15) +
                        (((size_t)ent * 2 + 15) & ~(size_t)15) + 32;
    const bool fast = n1 <= GSPX_TILE_MAXN1 && n1 < 65535 && need <= lds;
    slow += !fast;
    if (fast) entmax = std::max(entmax, ent);
    hdr[(size_t)b * 4 + 0] = lo;
    hdr[(size_t)b * 4 + 1] = fast ? n1 : -1;
    hdr[(size_t)b * 4 + 2] = rp[r0];
    hdr[(size_t)b * 4 + 3] = ent;
  }
  const int n_s1 = s1ptr[nb];
  CHK(g->gt_hdr.alloc(hdr.size() * 4 + 64));
  CHK(g->gt_s1rows.alloc((size_t)std::max(n_s1, 1) * 4 + 64));
  CHK(g->gt_lidx.alloc((size_t)g->nnz_int + 128));
  HIPCHK(hipMemcpy(g->gt_hdr.p, hdr.data(), hdr.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(g->gt_s1rows.p, s1rows, (size_t)n_s1 * 4, hipMemcpyHostToDevice));
  {  // the device keeps 8-bit positions (only staged blocks use them: n1 <= GSPX_TILE_MAXN1 < 256)
    std::vector<unsigned char> l8((size_t)g->nnz_int);
    for (int b = 0; b < nb; ++b) {
      const bool fast = hdr[(size_t)b * 4 + 1] >= 0;
      const int e0 = hdr[(size_t)b * 4 + 2], e1 = e0 + hdr[(size_t)b * 4 + 3];
      for (int e = e0; e < e1; ++e) {
        if (fast && lidx[e] >= 256) return set_err(GSPX_ERR_INVALID, "gspx_graph_set_gather_tiles: tile position out of range");
        l8[(size_t)e] = fast ? (unsigned char)lidx[e] : 0;
      }
    }
    HIPCHK(hipMemcpy(g->gt_lidx.p, l8.data(), l8.size(), hipMemcpyHostToDevice));
  }
  g->gt_rows = block_rows;
  g->gt_nb = nb;
  g->gt_ns1 = n_s1;
  g->gt_s1nat.release();
  g->gt_slow = slow;
  g->gt_lds = lds;
  g->gt_entmax = entmax;
  if (stats) {
    stats[0] = nb;
    stats[1] = slow;
    stats[2] = (int64_t)lds;
  }
  return GSPX_OK;
}

// the same tiles, computed on the device from the internal CSR (no host arrays):
// the gather tiles of the 64-row blocks (k_tiles_unique / k_tiles_fill): lists, positions, headers
static int build_tiles_dev(gspx_graph* g, size_t lds, DevMem& hdr, DevMem& s1rows, DevMem& lidx, int* out_nb, int* out_ns1,
                           int* out_slow, int* out_entmax) {
  gspx_ctx* ctx = g->ctx;
  hipStream_t st = ctx->stream;
  const int N = (int)g->N;
  constexpr int BR = GSPX_TILE_BR;
  const int nb = (N + BR - 1) / BR;
  DevMem tmp, n1, keep, s1lo, nslow;
  CHK(tmp.alloc((size_t)nb * GSPX_TILE_TMPCAP * sizeof(int)));
  CHK(n1.alloc(((size_t)nb + 1) * sizeof(int)));
  CHK(keep.alloc(((size_t)nb + 1) * sizeof(int)));
  CHK(s1lo.alloc(((size_t)nb + 1) * sizeof(int)));
  CHK(nslow.alloc(sizeof(int)));
  HIPCHK(hipMemsetAsync(nslow.p, 0, sizeof(int), st));
  hipLaunchKernelGGL(k_tiles_unique, dim3(nb), dim3(256), 0, st, g->rptr.as<int>(), g->rcol.as<int>(), N, nb,
                     tmp.as<int>(), n1.as<int>());
  hipLaunchKernelGGL(k_tiles_keep, dim3((nb + 1 + 255) / 256), dim3(256), 0, st, n1.as<int>(), nb,
                     keep.as<int>());
  CHK(scan_exclusive(ctx, keep.as<int>(), s1lo.as<int>(), nb + 1));
  int n_s1 = 0;
  HIPCHK(hipMemcpyAsync(&n_s1, s1lo.as<int>() + nb, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  CHK(hdr.alloc((size_t)nb * 4 * sizeof(int) + 64));
  CHK(s1rows.alloc((size_t)std::max(n_s1, 1) * 4 + 64));
  CHK(lidx.alloc((size_t)g->nnz_int + 128));
  hipLaunchKernelGGL(k_tiles_fill, dim3(nb), dim3(256), 0, st, g->rptr.as<int>(), g->rcol.as<int>(), N, nb,
                     tmp.as<int>(), n1.as<int>(), s1lo.as<int>(), (int)elt_size(g->dtype), (int)lds,
                     s1rows.as<int>(), lidx.as<unsigned char>(), hdr.as<int>(), nslow.as<int>());
  int slow = 0, entmax = 0;
  HIPCHK(hipMemcpyAsync(&slow, nslow.p, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemsetAsync(nslow.p, 0, sizeof(int), st));
  hipLaunchKernelGGL(k_tiles_entmax, dim3((nb + 255) / 256), dim3(256), 0, st, hdr.as<int>(), nb, nslow.as<int>());
  HIPCHK(hipMemcpyAsync(&entmax, nslow.p, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  *out_nb = nb;
  *out_ns1 = n_s1;
  *out_slow = slow;
  *out_entmax = entmax;
  return GSPX_OK;
}

extern "C" int gspx_graph_build_gather_tiles(gspx_graph* g, int64_t* stats) {
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  replay_reset(g->ctx);
  HIPCHK(hipSetDevice(g->ctx->device));
  if (g->N < 1) return set_err(GSPX_ERR_INVALID, "empty graph");
  const size_t lds = (size_t)52 * 1024;
  int nb = 0, n_s1 = 0, slow = 0, entmax = 0;
  CHK(build_tiles_dev(g, lds, g->gt_hdr, g->gt_s1rows, g->gt_lidx, &nb, &n_s1, &slow, &entmax));
  g->gt_rows = GSPX_TILE_BR;
  g->gt_nb = nb;
  g->gt_ns1 = n_s1;
  g->gt_s1nat.release();
  g->gt_slow = slow;
  g->gt_lds = lds;
  g->gt_entmax = entmax;
  if (stats) {
    stats[0] = nb;
    stats[1] = slow;
    stats[2] = (int64_t)lds;
    stats[3] = n_s1;
  }
  return GSPX_OK;
}

// ------------------------------------------------------------------------------------------------
// step schedule ("plan")
// ------------------------------------------------------------------------------------------------
struct PlanStep {
  double scale = 1.0, gamma = -1.0;
  int flush = 0;   // 0 none, 1 write, 2 accumulate
  int final = 0;
  std::vector<double> w;  // nf*3: w_new, w_cur, w_old
};

// Fused-flush schedule.  T_k overwrites T_{k-2} in place, so a term must be folded into the
// accumulators no later than the step that overwrites it; folding happens every third step
// (when T_k, T_{k-1}, T_{k-2} are all in registers), i.e. 2/3 of an accumulator pass per step
// instead of the reference's one read-modify-write per step per filter
// (approximations.py:108-109).
//   cp: nf x M coefficients with c[.,0] already halved (approximations.py:103)
static void make_plan_fused(int nf, int M, const std::vector<double>& cp, bool acc_existing,
                            bool final_to_y, std::vector<PlanStep>& plan) {
  const int K = M - 1;
  plan.assign((size_t)K, PlanStep());
  int covered = -1;  // T_0..T_covered are already folded
  bool first = !acc_existing;
  for (int k = 1; k <= K; ++k) {
    PlanStep& st = plan[(size_t)k - 1];
    st.scale = (k == 1) ? 0.5 : 1.0;
    st.gamma = (k == 1) ? 0.0 : -1.0;
    st.w.assign((size_t)nf * 3, 0.0);
    const bool must = (k == K) || (k >= 2 && (k - 2) > covered);
    if (!must) continue;
    st.flush = first ? 1 : 2;
    first = false;
    st.final = (k == K && final_to_y) ? 1 : 0;
    for (int f = 0; f < nf; ++f) {
      const double* c = &cp[(size_t)f * M];
      if (k > covered) st.w[(size_t)f * 3 + 0] = c[k];
      if (k - 1 > covered) st.w[(size_t)f * 3 + 1] = c[k - 1];
      if (k >= 2 && k - 2 > covered) st.w[(size_t)f * 3 + 2] = c[k - 2];
    }
    covered = k;
  }
}

// Deferred schedule: every T_k is kept, no flush inside the steps.
static void make_plan_deferred(int nf, int M, std::vector<PlanStep>& plan) {
  const int K = M - 1;
  plan.assign((size_t)K, PlanStep());
  for (int k = 1; k <= K; ++k) {
    PlanStep& st = plan[(size_t)k - 1];
    st.scale = (k == 1) ? 0.5 : 1.0;
    st.gamma = (k == 1) ? 0.0 : -1.0;
    st.w.assign((size_t)nf * 3, 0.0);
  }
}

static void halve_c0(int nf, int M, const double* coeffs, std::vector<double>& cp) {
  cp.assign(coeffs, coeffs + (size_t)nf * M);
  for (int f = 0; f < nf; ++f) cp[(size_t)f * M] *= 0.5;
}

extern "C" int gspx_plan_describe(gspx_ctx* ctx, int Nf, int M, const double* coeffs,
                                  double* plan_out) {
  if (M < 2) return set_err(GSPX_ERR_COEFF, "The coefficients have an invalid shape");
  if (Nf < 1 || !coeffs || !plan_out) return set_err(GSPX_ERR_INVALID, "bad argument");
  Options opt;
  if (ctx) opt = ctx->opt;
  std::vector<double> cp;
  halve_c0(Nf, M, coeffs, cp);
  std::vector<PlanStep> plan;
  const bool deferred = opt.combine == 2 || (opt.combine == 0 && Nf >= 2);
  if (deferred)
    make_plan_deferred(Nf, M, plan);
  else
    make_plan_fused(Nf, M, cp, false, true, plan);
  const size_t stride = 4 + 3 * (size_t)Nf;
  for (size_t k = 0; k < plan.size(); ++k) {
    double* o = plan_out + k * stride;
    o[0] = plan[k].scale;
    o[1] = plan[k].gamma;
    o[2] = plan[k].flush;
    o[3] = plan[k].final;
    for (size_t j = 0; j < 3 * (size_t)Nf; ++j) o[4 + j] = plan[k].w[j];
  }
  return GSPX_OK;
}

// ------------------------------------------------------------------------------------------------
// kernel dispatch
// ------------------------------------------------------------------------------------------------
struct Shape {
  int kernel;  // 1 panel (lane groups), 2 narrow, 3 wave-row
  int vec;
  int wlog2;
  int glog2;   // narrow only
  int gridy;   // panel only
};

static Shape choose_shape(const Options& opt, size_t elt, int64_t ld, int veccap) {
  Shape s{};
  const int maxvec = std::min((int)(16 / elt), veccap);
  int vec = 1;
  for (int v = maxvec; v >= 1; v /= 2)
    if (ld % v == 0) { vec = v; break; }
  while (vec > 1 && ld / vec < 16) vec /= 2;
  if (opt.vec != 0 && opt.vec <= maxvec && ld % opt.vec == 0) vec = (int)opt.vec;
  int kernel = (ld <= 4) ? 2 : 1;
  if (opt.kernel == 2 && ld <= 64) kernel = 2;
  if (opt.kernel == 1 && ld > 4) kernel = 1;
  if (opt.kernel == 5 && ld > 4) kernel = 5;
  // auto: fp32 panels and fp64 panels of up to 32 signals -> LDS-staged kernel; wide fp64 panels ->
  // scalar-metadata lane-group kernel.  Measured (round 1, headline graph):
  // fp32 the LDS kernel is 25 % faster; fp64 x 8 / 16 / 32 signals 0.18 / 0.21 / 0.26 ms per order
  // against 0.28 / 0.31 / 0.37 (many rows per row set make the scalar blends expensive); fp64 x 64
  // the scalar-metadata kernel wins by 4 %.
  if (opt.kernel == 0 && kernel == 1 && (elt == 4 || ld <= 32)) kernel = 5;
  s.kernel = kernel;
  if (kernel == 1 || kernel == 5) {
    s.vec = vec;
    const int64_t lanes = ld / vec;
    s.wlog2 = lanes <= 16 ? 4 : (lanes <= 32 ? 5 : 6);
    s.gridy = (int)((lanes + 63) / 64);
    s.glog2 = 0;
  } else {
    s.vec = 1;
    int wl = 0;
    while ((1 << wl) < ld) ++wl;
    s.wlog2 = wl;
    // auto: 4 lanes per row in total (measured best on the cache-resident config 1)
    const int64_t gl = opt.narrow_g_log2 >= 0 ? opt.narrow_g_log2 : std::max(0, 2 - wl);
    s.glog2 = (int)std::min<int64_t>(gl, 6 - wl);
    s.gridy = 1;
  }
  return s;
}

template <typename T, int VEC, int MODE>
static void launch_panel_w(const StepArgs<T>& a, int wlog2, dim3 grid, hipStream_t st) {
#define GSPX_LP(WL)                                                                     \
  hipLaunchKernelGGL((k_step_panel<T, VEC, WL, MODE>), grid, dim3(64 * a.wpb), 0, st, a.rowptr, \
                     a.col, a.val, a.cur, a.wts, a.perm, a)
  switch (wlog2) {
    case 4: GSPX_LP(4); break;
    case 5: GSPX_LP(5); break;
    default: GSPX_LP(6); break;
  }
#undef GSPX_LP
}

template <typename T, int MODE>
static void launch_panel(const StepArgs<T>& a, const Shape& s, dim3 grid, hipStream_t st) {
  if constexpr (sizeof(T) == 4) {
    if (s.vec == 4) return launch_panel_w<T, 4, MODE>(a, s.wlog2, grid, st);
  }
  if (s.vec == 2) return launch_panel_w<T, 2, MODE>(a, s.wlog2, grid, st);
  return launch_panel_w<T, 1, MODE>(a, s.wlog2, grid, st);
}

template <typename T, int VEC, int MODE>
static void launch_lds_w(const StepArgs<T>& a, const unsigned* coff, int wlog2, dim3 grid,
                         hipStream_t st) {
  // (a.lds_pad: unused dynamic LDS that only lowers the workgroups resident per CU - an experiment knob for
  // graphs without locality, where fewer gathers in flight per L2 can mean more hits)
#define GSPX_LL(WL)                                                                          \
  hipLaunchKernelGGL((k_step_lds<T, VEC, WL, MODE>), grid, dim3(256), (size_t)a.lds_pad, st, a.rowptr, coff, \
                     a.val, a.cur, a.wts, a.perm, a)
  switch (wlog2) {
    case 4: GSPX_LL(4); break;
    case 5: GSPX_LL(5); break;
    default: GSPX_LL(6); break;
  }
#undef GSPX_LL
}

template <typename T, int MODE>
static void launch_lds(const StepArgs<T>& a, const unsigned* coff, const Shape& s, dim3 grid,
                       hipStream_t st) {
  if constexpr (sizeof(T) == 4) {
    if (s.vec == 4) return launch_lds_w<T, 4, MODE>(a, coff, s.wlog2, grid, st);
  }
  if (s.vec == 2) return launch_lds_w<T, 2, MODE>(a, coff, s.wlog2, grid, st);
  return launch_lds_w<T, 1, MODE>(a, coff, s.wlog2, grid, st);
}

template <typename T>
static void launch_step(StepArgs<T> a, const Shape& s, const Options& opt, hipStream_t st,
                        const unsigned* coff) {
  int rpw = (int)opt.rows_per_wave;
  if (rpw <= 0)
    rpw = (s.kernel == 5) ? (sizeof(T) == 4 ? 16 : 8) : (s.kernel == 2 ? 1 : 4);
  if (s.kernel == 1 || s.kernel == 5) {
    const int R = 64 >> s.wlog2;  // rows per row set
    rpw = ((rpw + R - 1) / R) * R;
    if (s.kernel == 5 && rpw > 32) rpw = 32;
  }
  a.rows_per_wave = rpw;
  int rows_per_chunk;
  a.lds_pad = (int)std::min<int64_t>(std::max<int64_t>(opt.lds_pad_kb, 0), 40) * 1024;
  a.wpb = (s.kernel == 1) ? (int)opt.waves_per_block : 4;
  if (s.kernel == 1 || s.kernel == 5)
    rows_per_chunk = a.wpb * rpw;
  else
    rows_per_chunk = rpw * (4 << (6 - s.wlog2 - s.glog2));
  a.nchunks = (a.N + rows_per_chunk - 1) / rows_per_chunk;
  int gx = a.nchunks;
  a.cpx = 0;
  if (opt.xcd_remap) {
    a.cpx = (a.nchunks + 7) / 8;
    gx = a.cpx * 8;
  }
  dim3 grid((unsigned)gx, (unsigned)s.gridy, 1);
  const int mode = a.flush ? 1 : ((a.beta != T(0) || a.nin > 0 || a.final) ? 2 : 0);
  if (s.kernel == 5) {
    if (mode == 1) launch_lds<T, 1>(a, coff, s, grid, st);
    else if (mode == 2) launch_lds<T, 2>(a, coff, s, grid, st);
    else launch_lds<T, 0>(a, coff, s, grid, st);
  } else if (s.kernel == 1) {
    if (mode == 1) launch_panel<T, 1>(a, s, grid, st);
    else if (mode == 2) launch_panel<T, 2>(a, s, grid, st);
    else launch_panel<T, 0>(a, s, grid, st);
  } else {
    if (a.flush)
      hipLaunchKernelGGL((k_step_narrow<T, true>), grid, dim3(256), 0, st, a, s.wlog2, s.glog2);
    else
      hipLaunchKernelGGL((k_step_narrow<T, false>), grid, dim3(256), 0, st, a, s.wlog2, s.glog2);
  }
}

template <typename T>
static void launch_permute_in(const T* x, unsigned ldx, T* out, unsigned ld, int N,
                              const int* perm, int vec, hipStream_t st) {
  const size_t total = (size_t)N * (ld / vec);
  const unsigned nb = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
  if (nb == 0) return;
  if constexpr (sizeof(T) == 4) {
    if (vec == 4) {
      hipLaunchKernelGGL((k_permute_in<T, 4>), dim3(nb), dim3(256), 0, st, x, ldx, out, ld, N, perm);
      return;
    }
  }
  if (vec == 2)
    hipLaunchKernelGGL((k_permute_in<T, 2>), dim3(nb), dim3(256), 0, st, x, ldx, out, ld, N, perm);
  else
    hipLaunchKernelGGL((k_permute_in<T, 1>), dim3(nb), dim3(256), 0, st, x, ldx, out, ld, N, perm);
}

template <typename T, int VEC>
static void launch_combine_v(const T* slots, int nslots, size_t slot_stride, const T* cf, int M,
                             int nf, int N, unsigned ld, T* y, unsigned ldy, size_t plane_y,
                             const int* perm, hipStream_t st, unsigned pitch) {
  const size_t total = (size_t)N * (ld / VEC);
  const unsigned nb = (unsigned)std::min<size_t>((total + 255) / 256, 16384);
  if (nb == 0) return;
  constexpr int NFB = 8;
  for (int f0 = 0; f0 < nf; f0 += NFB) {
    const int here = std::min(NFB, nf - f0);
    hipLaunchKernelGGL((k_combine<T, VEC, NFB>), dim3(nb), dim3(256), 0, st, slots, nslots,
                       slot_stride, cf, M, f0, here, N, ld, y, ldy, plane_y, perm, 0, pitch);
  }
}

template <typename T>
static void launch_combine(const T* slots, int nslots, size_t slot_stride, const T* cf, int M,
                           int nf, int N, unsigned ld, T* y, unsigned ldy, size_t plane_y,
                           const int* perm, int vec, hipStream_t st, unsigned pitch = 0) {
  if (!pitch) pitch = ld;
  if constexpr (sizeof(T) == 4) {
    if (vec == 4)
      return launch_combine_v<T, 4>(slots, nslots, slot_stride, cf, M, nf, N, ld, y, ldy, plane_y,
                                    perm, st, pitch);
  }
  if (vec == 2)
    return launch_combine_v<T, 2>(slots, nslots, slot_stride, cf, M, nf, N, ld, y, ldy, plane_y,
                                  perm, st, pitch);
  return launch_combine_v<T, 1>(slots, nslots, slot_stride, cf, M, nf, N, ld, y, ldy, plane_y,
                                perm, st, pitch);
}

// The squared column norms of a deferred batch instead of its outputs (gspx_cheby_sqnorms_dev): cf [k][ldc] fp64
// coefficients (c'_f0 halved, zero beyond Nf), out [Nf][ldo] fp64 at the batch's first column, part the workgroup
// partials (sqnorm_parts doubles at the call's widest batch).
struct SqNorms {
  const double* cf;
  int ldc, nf;
  double* out;
  size_t ldo;
  double* part;
};
static const int SQ_PASS = 128;  // filters per pass over the stack
static int sqnorm_cwl(unsigned w) {  // log2 of the columns of a tile: the batch width up to 64, a power of two
  int l = 0;
  while (l < 6 && (1u << l) < w) ++l;
  return l;
}
static int sqnorm_gx(const gspx_ctx* ctx, int N, unsigned w) {  // workgroups along the rows
  const int cwl = sqnorm_cwl(w);
  const int64_t tiles = ((int64_t)N + (64 >> cwl) - 1) / (64 >> cwl);
  const int64_t gy = ((int64_t)w + (1 << cwl) - 1) >> cwl;
  return (int)std::max<int64_t>(1, std::min<int64_t>(tiles, (4 * (int64_t)ctx->cu_count + gy - 1) / gy));
}
static size_t sqnorm_parts(const gspx_ctx* ctx, int N, unsigned w) {
  return (size_t)sqnorm_gx(ctx, N, w) * SQ_PASS * w;
}

template <typename T>
static int launch_combine_sqnorm(gspx_ctx* ctx, const T* slots, int nslots, size_t slot_stride, unsigned pitch, int N,
                                 unsigned w, const SqNorms& sq, hipStream_t st) {
  const size_t lds = (size_t)nslots * 64 * sizeof(double);
  const int cwl = sqnorm_cwl(w);
  const dim3 grid((unsigned)sqnorm_gx(ctx, N, w), (w + (1u << cwl) - 1) >> cwl);
  for (int f0 = 0; f0 < sq.nf; f0 += SQ_PASS) {
    const int here = std::min(SQ_PASS, sq.nf - f0);
    const int fb = here <= 8 ? 2 : here <= 32 ? 8 : 32;  // filters per wave: 4 waves cover the pass
    typedef void (*kern_t)(const T*, int, size_t, u32, int, int, int, const double*, int, double*);
    const kern_t kern = fb == 2 ? k_combine_sqnorm<T, 2> : fb == 8 ? k_combine_sqnorm<T, 8> : k_combine_sqnorm<T, 32>;
    if (lds > ((size_t)64 << 10))
      HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, slots, nslots, slot_stride, (u32)pitch, N, (int)w, cwl,
                       sq.cf + f0, sq.ldc, sq.part);
    const int64_t n = (int64_t)here * w;
    hipLaunchKernelGGL(k_sqnorm_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, sq.part, (int)grid.x,
                       4 * fb, here, (int)w, sq.out + (size_t)f0 * sq.ldo, sq.ldo);
  }
  return GSPX_OK;
}

// ------------------------------------------------------------------------------------------------
// the filter
// ------------------------------------------------------------------------------------------------
template <typename T> static int ensure_factor(gspx_graph* g, double lmax) {
  if (g->fval_lmax == lmax) return GSPX_OK;
  gspx_ctx* ctx = g->ctx;
  const int N = (int)g->N;
  // a1 = a2 = lmax/2 (approximations.py:93-96); the reference's arithmetic dtype follows L
  const T a1 = (T)(lmax / 2.0), a2 = (T)(lmax / 2.0);
  const T two_over_a1 = T(2) / a1;
  const int nb = std::max(1, (N + 255) / 256);
  if (N > 0)
    hipLaunchKernelGGL((k_factor<T>), dim3(nb), dim3(256), 0, ctx->stream, g->rptr.as<int>(),
                       g->rcol.as<int>(), g->rval.as<T>(), N, two_over_a1, a2, g->fval.as<T>());
  HIPCHK(hipGetLastError());
  g->fval_lmax = lmax;
  return GSPX_OK;
}

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

// One (sub)problem: nf filters applied to one batch of `ld` signals whose first column is
// x/y column c0.  x: [N][ldx] (+c0), y: [nf][N][ldy] (+c0).
// LDS-staged gather step (gspx_tile_kernels.hip.h): usable when the graph carries gather tiles and
// every panel the kernel touches is made of 16-byte lane pieces
// the gather lists as rows of an unpermuted panel: nat[i] = perm[s1rows[i]]
__global__ void k_s1nat(const int* __restrict__ s1, const int* __restrict__ perm, int n, int* __restrict__ nat) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) nat[i] = perm[s1[i]];
}
static int ensure_s1nat(gspx_graph* g, hipStream_t st) {
  if (g->gt_s1nat.p || !g->has_perm) return GSPX_OK;
  CHK(g->gt_s1nat.alloc((size_t)std::max(g->gt_ns1, 1) * 4 + 64));
  if (g->gt_ns1 > 0)
    hipLaunchKernelGGL(k_s1nat, dim3((g->gt_ns1 + 255) / 256), dim3(256), 0, st, g->gt_s1rows.as<int>(),
                       g->perm.as<int>(), g->gt_ns1, g->gt_s1nat.as<int>());
  return GSPX_OK;
}

// a work panel of row pitch ld can take the tile kernels
template <typename T> static bool tile_geometry(const gspx_graph* g, const Options& opt, unsigned ld) {
  constexpr int TVEC = 16 / (int)sizeof(T);
  const size_t U = (size_t)g->N * ld;
  return opt.tile_gather && g->gt_rows == GSPX_TILE_BR && (size_t)ld * sizeof(T) >= (size_t)opt.tile_min_row &&
         (ld % TVEC) == 0 && U * sizeof(T) < ((size_t)1 << 31) && (size_t)g->nnz_int * sizeof(T) < ((size_t)1 << 31);
}
// ... and the final flush can store 16-byte pieces straight into y
template <typename T>
static bool tile_usable(const gspx_graph* g, const Options& opt, unsigned ld, const T* y, unsigned ldy) {
  constexpr int TVEC = 16 / (int)sizeof(T);
  return tile_geometry<T>(g, opt, ld) && (ldy % TVEC) == 0 && (((uintptr_t)y / sizeof(T)) % TVEC) == 0;
}
// fills the graph / geometry fields of t and launches; the caller sets cur, old, out, racc, y,
// ldy, perm, scale, gamma, beta, flush, final, wn, wc, wo
template <typename T>
static int launch_step_tile(gspx_graph* g, const Options& opt, TileArgs<T> t, unsigned ld, hipStream_t st,
                            const T* vals = nullptr) {
  // narrow panels (rows of at most 128 bytes): 8- / 4- / 2- / 1-lane row groups in workgroups of 512 / 256 / 128 / 64
  // threads - every lane holds a piece of a row, and the smaller workgroups keep more blocks in flight per CU
  const size_t rowb = (size_t)ld * sizeof(T);
  int lg = rowb <= 16 ? 1 : rowb <= 32 ? 2 : rowb <= 64 ? 4 : rowb <= 128 ? 8 : 16;
  if (opt.tile_lg == 8 || opt.tile_lg == 4 || opt.tile_lg == 2) lg = rowb <= 128 ? std::max(lg, (int)opt.tile_lg) : 16;  // (tuning)
  // (the 8-lane build in 256-thread workgroups with two rows per group - four resident workgroups instead of two -
  // measured within 3 % of the 512-thread build on 80- to 128-byte rows: those passes are not latency bound.)
  // (several column chunks per block with the small builds lose to the 16-lane build: 96- / 192-byte rows 4.1 / 6.7 ms
  // against 2.7 / 4.9 ms on the headline graph - a pass per chunk costs more than the idle lanes of a last chunk)
  const bool narrow = lg < 16;
  const int ncol = narrow ? 1 : (int)((rowb + 255) / 256);
  const int flavour = t.old_rows ? 1 : t.nin > 0 ? 2 : 0;  // plain | T_{k-2} from the caller's unpermuted panel
                                                           // (step 2 of a fused-input filter) | extra input panels
                                                           // (synthesis); never both
  typedef void (*kern_t)(const TileArgs<T>);
  static const kern_t wide[3][3] = {
      {k_step_tile<T, 0>, k_step_tile<T, 1>, k_step_tile<T, 2>},
      {k_step_tile<T, 0, 16, true>, k_step_tile<T, 1, 16, true>, k_step_tile<T, 2, 16, true>},
      {k_step_tile<T, 0, 16, false, true>, k_step_tile<T, 1, 16, false, true>, k_step_tile<T, 2, 16, false, true>}};
  static const kern_t slim[3][4] = {
      {k_step_tile<T, 1, 1, false, false, 64>, k_step_tile<T, 1, 2, false, false, 128>,
       k_step_tile<T, 1, 4, false, false, 256>, k_step_tile<T, 1, 8>},
      {k_step_tile<T, 1, 1, true, false, 64>, k_step_tile<T, 1, 2, true, false, 128>,
       k_step_tile<T, 1, 4, true, false, 256>, k_step_tile<T, 1, 8, true>},
      {k_step_tile<T, 1, 1, false, true, 64>, k_step_tile<T, 1, 2, false, true, 128>,
       k_step_tile<T, 1, 4, false, true, 256>, k_step_tile<T, 1, 8, false, true>}};
  kern_t kern = narrow ? slim[flavour][lg == 1 ? 0 : lg == 2 ? 1 : lg == 4 ? 2 : 3] : wide[flavour][ncol <= 2 ? ncol : 0];
  unsigned threads = narrow ? 64u * (unsigned)lg : 512u;
  // calibration (gspx_bench_step_mix): the same launch with the row products removed (gspx_tile_kernels.hip.h, MIX)
  bool mix = false;
  if (opt.calib_mix && !narrow && flavour == 0) {
    static const kern_t mixk[2][3] = {
        {k_step_tile<T, 0, 16, false, false, 512, 16, 1>, k_step_tile<T, 1, 16, false, false, 512, 16, 1>,
         k_step_tile<T, 2, 16, false, false, 512, 16, 1>},
        {k_step_tile<T, 0, 16, false, false, 512, 16, 2>, k_step_tile<T, 1, 16, false, false, 512, 16, 2>,
         k_step_tile<T, 2, 16, false, false, 512, 16, 2>}};
    kern = mixk[opt.calib_mix == 2 ? 1 : 0][ncol <= 2 ? ncol : 0];
    mix = true;
  }
  // rows of fewer 16-byte pieces than the lanes they are staged with: the builds whose compute phases regroup the
  // threads by pieces (template parameter CL), in workgroups of 64 x pieces (one row per group) or 32 x pieces (two
  // rows) threads.  Measured per piece count, A/B on one box (profiles/r04_regroup_ab*.json): 3 pieces (48-byte rows:
  // 5 / 6 fp64, 10 / 12 fp32 signals) +6...8 %, 5 pieces (80 bytes: 10 fp64) +2.5 %, 10 pieces (160 bytes: 20 fp64)
  // +6 %; 6, 7, 12 and 14 pieces -2...0 % (idle compute lanes are not what bounds those passes) - they keep the
  // power-of-two builds.
  const int pieces = (int)(rowb / 16);
  if (opt.tile_regroup && ncol == 1 && flavour != 1 && pieces < lg && !mix) {
#define GSPX_CL(LG_, CL_, NT_) \
  (flavour == 2 ? (kern_t)k_step_tile<T, 1, LG_, false, true, NT_, CL_> : (kern_t)k_step_tile<T, 1, LG_, false, false, NT_, CL_>)
    kern_t k2 = nullptr;
    unsigned nt2 = 0;
    if (lg == 4 && pieces == 3) k2 = GSPX_CL(4, 3, 192), nt2 = 192;
    else if (lg == 8 && pieces == 5) k2 = GSPX_CL(8, 5, 320), nt2 = 320;
    else if (lg == 16 && pieces == 10) k2 = GSPX_CL(16, 10, 320), nt2 = 320;
#undef GSPX_CL
    if (k2) kern = k2, threads = nt2;
  }
  // dynamic LDS: the wide builds take the tile budget the blocks were classified with; a narrow build's tile
  // rows are 16 lg bytes, so the largest staged block needs far less - and more workgroups fit a CU
  size_t lds = g->gt_lds;
  if (lg < 8)
    lds = std::min(lds, (size_t)GSPX_TILE_MAXN1 * 16 * lg + (((size_t)g->gt_entmax * sizeof(T) + 15) & ~(size_t)15) +
                            (((size_t)g->gt_entmax + 15) & ~(size_t)15) + 64);
  if (lg < 8) lds = (lds + 2047) & ~(size_t)2047;  // (graphs differ in their largest block: few distinct sizes)
  int per_cu = 2;
  {  // once per kernel build, device and LDS size (a driver call per launch would cost microseconds each)
    struct Known { size_t attr = 0; std::map<size_t, int> fit; };
    static std::map<std::pair<const void*, int>, Known> known;
    static std::mutex lds_mu;
    std::lock_guard<std::mutex> lock(lds_mu);
    Known& k = known[std::make_pair((const void*)kern, g->ctx->device)];
    if (k.attr < lds) {  // the limit only ever grows
      HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      k.attr = lds;
    }
    if (lg < 8) {  // resident workgroups of the small builds: what registers and LDS allow
      auto it = k.fit.find(lds);
      if (it == k.fit.end()) {
        int fit = 2;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, (const void*)kern, (int)threads, lds));
        it = k.fit.emplace(lds, std::max(2, std::min(fit, 16))).first;
      }
      per_cu = it->second;
    }
  }
  t.rowptr = g->rptr.as<int>();
  t.col = g->rcol.as<int>();
  t.val = vals ? vals : g->fval.as<T>();  // any values array on the internal pattern
  t.hdr = g->gt_hdr.as<int>();
  if (!t.s1rows) t.s1rows = g->gt_s1rows.as<int>();  // (the caller may pass the lists in its panel's row order)
  t.lidx = g->gt_lidx.as<unsigned char>();
  t.N = (int)g->N;
  t.ld = ld;
  t.panel_bytes = (unsigned)((size_t)g->N * ld * sizeof(T));
  t.val_bytes = (unsigned)((size_t)g->nnz_int * sizeof(T));
  t.lidx_bytes = (unsigned)((size_t)g->nnz_int);
  t.nb = g->gt_nb;
  t.ncol = ncol;
  t.per_xcd = (t.nb + 7) / 8;
  t.lds_bytes = (int)lds;
  unsigned nwg = (unsigned)std::max<int64_t>(8, ((int64_t)per_cu * g->ctx->cu_count) / 8 * 8);
  if (opt.tile_workgroups > 0)
    nwg = (unsigned)std::max<int64_t>(8, std::min<int64_t>(opt.tile_workgroups, 1 << 20) / 8 * 8);
  nwg = std::min(nwg, 8u * (unsigned)std::max(t.per_xcd, 1));  // (workgroups beyond an XCD's blocks would exit at once)
  t.nt = opt.tile_nt >= 0 ? (int)opt.tile_nt : ((size_t)g->N * ld * sizeof(T) >= ((size_t)192 << 20) ? 5 : 0);
  hipLaunchKernelGGL(kern, dim3(nwg), dim3(threads), lds, st, t);
  return GSPX_OK;
}

// byte offsets col*ld*sizeof(T) of the stored entries for this panel width (cached on the graph; the
// LDS-staged plain kernel reads them)
template <typename T>
static int prepare_coff(gspx_graph* g, const Shape& shape, unsigned ld, hipStream_t st) {
  if (shape.kernel == 5 && g->coff_ldb != ld * (unsigned)sizeof(T)) {
    CHK(g->coff.ensure(((size_t)g->nnz_int + 64) * sizeof(unsigned)));
    const int nb = std::max(1, (int)((g->N + 255) / 256));
    hipLaunchKernelGGL((k_coff<T>), dim3(nb), dim3(256), 0, st, g->rptr.as<int>(), g->rcol.as<int>(), (int)g->N,
                       ld * (unsigned)sizeof(T), g->coff.as<unsigned>());
    g->coff_ldb = ld * (unsigned)sizeof(T);
  }
  return GSPX_OK;
}

// the widest lane vector, at most v, whose accesses to rows of pitch ld starting at p stay aligned
template <typename T> static int vec_cap(int v, unsigned ld, const T* p) {
  while (v > 1 && ((ld % v) != 0 || (((uintptr_t)p / sizeof(T)) % v) != 0)) v /= 2;
  return v;
}

// The work panels of a batch of ld signals.  tile_direct: the tile kernels on panels of pitch ld, the last step storing
// into y.  padded: rows that are not made of 16-byte pieces (or a y the final flush cannot store such pieces into) get
// work panels of pitch ldw, rounded up to whole pieces, so that the tile kernels take them all the same - zero columns
// cost little next to kernels that are several times faster - and the result leaves through a copy.  `tiles`: the
// caller's steps may take the tile kernels at all; `planes`: the panels one tile launch spans (its buffer window stays
// below 2 GiB).
struct WorkPanels {
  bool tile_direct, padded;
  unsigned ldw;
};
template <typename T>
static WorkPanels work_panels(const gspx_graph* g, const Options& opt, bool tiles, size_t planes, unsigned ld,
                              const T* y, unsigned ldy) {
  constexpr unsigned TVEC = 16 / (unsigned)sizeof(T);
  const unsigned ldp = (ld + TVEC - 1) / TVEC * TVEC;
  auto window = [&](unsigned w) { return planes * (size_t)g->N * w * sizeof(T) < ((size_t)1 << 31); };
  // (a single signal on a graph whose matrix stays in the L2s: the sub-wave kernel is the faster one there, 0.125
  // against 0.150 ms for 30 orders at N = 50k; from ~20 MB of matrix on the padded tile path wins, 0.86 against
  // 1.19 ms at N = 1M.  Two signals and more: the tile path at every size - 0.15 against 0.18 ms for two fp32
  // signals at N = 100k.)
  const bool pad_pays = opt.tile_pad == 2 || ld >= 2 ||
                        (size_t)g->nnz_int * (sizeof(T) + 4) >= ((size_t)20 << 20);
  WorkPanels p;
  p.tile_direct = tiles && tile_usable<T>(g, opt, ld, y, ldy) && window(ld);
  p.padded = !p.tile_direct && tiles && opt.tile_pad && pad_pays && tile_geometry<T>(g, opt, ldp) && window(ldp);
  p.ldw = p.padded ? ldp : ld;
  return p;
}

// what every plain step (StepArgs) of a batch shares: the graph, the panel geometry and the final store into y
template <typename T>
static StepArgs<T> step_base(const gspx_graph* g, unsigned ld, T* y, unsigned ldy) {
  StepArgs<T> a{};
  a.rowptr = g->rptr.as<int>();
  a.col = g->rcol.as<int>();
  a.val = g->fval.as<T>();
  a.N = (int)g->N;
  a.ld = ld;
  a.curbytes = (u32)((size_t)g->N * ld * sizeof(T));
  a.y = y;
  a.ldy = ldy;
  a.perm = g->has_perm ? g->perm.as<int>() : nullptr;
  return a;
}

// the four pool events of a batch, the first recorded at once: copy in | steps | combine or copy out between them
// (run_batches sums each phase over the batches)
static int batch_events(gspx_ctx* ctx, size_t& ev_idx, hipEvent_t ev[4]) {
  for (int i = 0; i < 4; ++i) ev[i] = pool_event(ctx, ++ev_idx);
  if (!ev[0] || !ev[1] || !ev[2] || !ev[3]) return set_err(GSPX_ERR_HIP, "hipEventCreate failed");
  HIPCHK(hipEventRecord(ev[0], ctx->stream));
  return GSPX_OK;
}

template <typename T>
static int run_batch(gspx_graph* g, int nf, int M, const std::vector<double>& cp, const T* x,
                     unsigned ldx, T* y, unsigned ldy, unsigned ld, bool deferred,
                     bool acc_existing, bool final_to_y, size_t& ev_idx, const SqNorms* sq = nullptr) {
  gspx_ctx* ctx = g->ctx;
  const Options& opt = ctx->opt;
  hipStream_t st = ctx->stream;
  const int N = (int)g->N;
  const int K = M - 1;
  const WorkPanels wp = work_panels<T>(g, opt, deferred || nf == 1, 1, ld, y, ldy);
  const bool tile_direct = wp.tile_direct, padded = wp.padded;
  const unsigned ldw = wp.ldw;
  const size_t U = (size_t)N * ldw;  // elements per panel
  // vector stores into y need aligned rows: cap the lane vector width accordingly
  const Shape shape = choose_shape(opt, sizeof(T), ld, vec_cap(4, ldy, y));
  const int* perm = g->has_perm ? g->perm.as<int>() : nullptr;

  std::vector<PlanStep> plan;
  if (deferred)
    make_plan_deferred(nf, M, plan);
  else
    make_plan_fused(nf, M, cp, acc_existing, final_to_y, plan);

  // device-side weights / coefficients
  std::vector<T> hw;
  if (deferred) {
    hw.resize((size_t)nf * M);
    for (size_t i = 0; i < hw.size(); ++i) hw[i] = (T)cp[i];
  } else {
    hw.resize((size_t)K * nf * 3);
    for (int k = 0; k < K; ++k)
      for (int j = 0; j < nf * 3; ++j) hw[(size_t)k * nf * 3 + j] = (T)plan[(size_t)k].w[(size_t)j];
  }
  const bool cap = ctx->capturing;  // replay recording: the previous eager call left the same weights
  if (!cap) {                       // and workspace in place
    CHK(ctx->ws_w.ensure(hw.size() * sizeof(T) + 64));
    HIPCHK(hipMemcpyAsync(ctx->ws_w.p, hw.data(), hw.size() * sizeof(T), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // hw is a stack-owned staging buffer
  }

  const size_t nslots = deferred ? (size_t)M : 2;
  // (Shifting slot 1 or the accumulator against slot 0 by 256 B ... 16 MB changes nothing: the placement effect of
  // profiles/r06_placement.md is not stream-against-stream channel aliasing - tools/skew_sweep.py's record.)
  const size_t SU = U;  // slot pitch
  CHK(ctx->ws_t.ensure(nslots * SU * sizeof(T) + 256));
  if (!deferred) CHK(ctx->ws_r.ensure((size_t)nf * U * sizeof(T) + 256));
  T* slots = ctx->ws_t.as<T>();
  T* racc = ctx->ws_r.as<T>();

  hipEvent_t ev[4] = {};
  if (!cap) CHK(batch_events(ctx, ev_idx, ev));
  // LDS-staged gather: one filter with the fused flush
  // (or a filterbank's deferred combine, whose steps are plain recurrence steps into kept slots)
  const bool tile_ok = tile_direct || padded;
  // Fused input: step 1 gathers straight from the caller's panel (the tile lists mapped through the
  // vertex order) and step 2 reads T_0 from it, so the copy into the internal order never happens.
  // Needs every block on the LDS path, the panel in the internal row pitch, and x not aliasing y
  // (the copy used to make in-place calls safe).
  const unsigned char* xb = (const unsigned char*)x;
  const unsigned char* yb = (const unsigned char*)y;
  const size_t xbytes = (size_t)N * ldx * sizeof(T), ybytes = (size_t)nf * N * ldy * sizeof(T);
  const bool fuse_in = tile_direct && !deferred && opt.fuse_input && g->gt_slow == 0 && ldx == ld &&
                       ((uintptr_t)x % 16) == 0 && (xb + xbytes <= yb || yb + ybytes <= xb) &&
                       (!g->has_perm || (g->gt_ns1 > 0 && (!cap || g->gt_s1nat.p)));
  if (fuse_in) {
    CHK(ensure_s1nat(g, st));
  } else if (padded) {
    const unsigned nb = (unsigned)std::min<size_t>((U + 255) / 256, 65536);
    hipLaunchKernelGGL((k_permute_in_pad<T>), dim3(nb), dim3(256), 0, st, x, ldx, slots, ldw, ld, N, perm);
  } else {  // (permute-in vector width: x rows must be aligned too)
    launch_permute_in<T>(x, ldx, slots, ld, N, perm, vec_cap(shape.vec, ldx, x), st);
  }
  if (!cap) HIPCHK(hipEventRecord(ev[1], st));

  CHK(prepare_coff<T>(g, shape, ld, st));
  StepArgs<T> a = step_base<T>(g, ld, y, ldy);
  a.nf = nf;
  a.racc = racc;
  for (int k = 1; k <= K; ++k) {
    const PlanStep& ps = plan[(size_t)k - 1];
    if (tile_ok) {
      TileArgs<T> t{};
      if (deferred) {
        t.cur = slots + (size_t)(k - 1) * SU;
        t.old = (k >= 2 && ps.gamma != 0.0) ? slots + (size_t)(k - 2) * SU : t.cur;
        t.out = slots + (size_t)k * SU;
      } else {
        t.cur = slots + (size_t)((k - 1) & 1) * SU;
        t.old = ps.gamma == 0.0 ? t.cur : slots + (size_t)(k & 1) * SU;
        t.out = slots + (size_t)(k & 1) * SU;
        if (fuse_in && k == 1) {  // T_0 is the caller's panel
          t.cur = x;
          t.old = x;
          t.s1rows = g->has_perm ? g->gt_s1nat.as<int>() : nullptr;
        } else if (fuse_in && k == 2) {
          t.old = x;
          t.old_rows = perm;  // null without an internal order: plain rows
        }
      }
      t.racc = racc;
      t.y = y;
      t.ldy = ldy;
      t.perm = perm;
      t.scale = (T)ps.scale;
      t.gamma = (T)ps.gamma;
      t.beta = T(0);
      t.flush = ps.flush;
      t.final = padded ? 0 : ps.final;  // padded rows: the last flush stays in the accumulator panel, copied out below
      t.reverse = (opt.alternate_sweep && (k & 1)) ? 1 : 0;
      if (ps.flush) {
        t.wn = (T)ps.w[0];
        t.wc = (T)ps.w[1];
        t.wo = (T)ps.w[2];
      }
      CHK(launch_step_tile<T>(g, opt, t, ldw, st));
      continue;
    }
    if (deferred) {
      a.cur = slots + (size_t)(k - 1) * SU;
      a.old = k >= 2 ? slots + (size_t)(k - 2) * SU : slots;
      a.out = slots + (size_t)k * SU;
    } else {
      a.cur = slots + (size_t)((k - 1) & 1) * SU;
      a.old = slots + (size_t)(k & 1) * SU;
      a.out = slots + (size_t)(k & 1) * SU;
    }
    if (ps.gamma == 0.0) a.old = a.cur;  // never read for its value; keeps the kernel branch-free
    a.scale = (T)ps.scale;
    a.gamma = (T)ps.gamma;
    a.flush = ps.flush;
    a.final = ps.final;
    a.reverse = (opt.alternate_sweep && (k & 1)) ? 1 : 0;
    a.wts = ctx->ws_w.as<T>() + (size_t)(k - 1) * nf * 3;
    launch_step<T>(a, shape, opt, st, g->coff.as<unsigned>());
  }
  if (!cap) HIPCHK(hipEventRecord(ev[2], st));
  if (deferred && sq) {  // the squared column norms in place of the outputs (rows in any order: no perm)
    CHK(launch_combine_sqnorm<T>(ctx, slots, M, SU, ldw, N, ld, *sq, st));
  } else if (deferred) {
    launch_combine<T>(slots, M, SU, ctx->ws_w.as<T>(), M, nf, N, ld, y, ldy, (size_t)N * ldy, perm,
                      padded ? 1 : vec_cap(shape.vec, ldy, y), st, ldw);
  } else if (padded && final_to_y) {
    const unsigned nb = (unsigned)std::min<size_t>(((size_t)N * ld + 255) / 256, 65536);
    hipLaunchKernelGGL((k_permute_out_pad<T>), dim3(nb), dim3(256), 0, st, racc, ldw, y, ldy, ld, N, perm);
  }
  if (!cap) {
    HIPCHK(hipEventRecord(ev[3], st));
    HIPCHK(hipGetLastError());
  }
  return GSPX_OK;
}

template <typename T>
static int run_synthesis_batch(gspx_graph* g, int nf, int M, const std::vector<double>& cp,
                               const T* x, size_t plane_x, unsigned ldx, T* y, unsigned ldy,
                               unsigned ld, size_t& ev_idx);

// Signals per column batch of a device call: bounded by the 2 GiB buffer-descriptor window, by the workspace budget
// (`panels` workspace columns of N elements per signal) and by max_batch.  A call of several batches gets widths that
// are multiples of 4: batch starts stay 16-byte friendly.
static int batch_width(const gspx_graph* g, size_t elt, size_t panels, int64_t Nsig, int64_t* width) {
  const Options& opt = g->ctx->opt;
  const size_t rowb = (size_t)g->N * elt;
  int64_t max_ld = (int64_t)((((size_t)1 << 31) - 65536) / rowb);
  if (max_ld < 1)
    return set_err(GSPX_ERR_INVALID, "graph too large: one signal column exceeds 2 GiB");
  const size_t budget = (size_t)std::max<int64_t>(opt.ws_limit_mb, 1) << 20;
  max_ld = std::min<int64_t>(max_ld, std::max<int64_t>(1, (int64_t)(budget / (rowb * panels))));
  if (opt.max_batch > 0) max_ld = std::min<int64_t>(max_ld, opt.max_batch);
  if (max_ld < Nsig && max_ld >= 4) max_ld &= ~(int64_t)3;
  *width = max_ld;
  return GSPX_OK;
}

// The column batches of a device call: batch(c0, ld, ev_idx) runs signals [c0, c0 + ld) and takes its pool events
// from batch_events.  Then the call's device time, the per-phase sums and the steps run (`steps` per batch) go to
// ctx->timing[0..4].
template <typename Batch>
static int run_batches(gspx_graph* g, int64_t Nsig, int64_t width, int steps, const Batch& batch) {
  gspx_ctx* ctx = g->ctx;
  size_t ev_idx = 0;
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  for (int64_t c0 = 0; c0 < Nsig; c0 += width)
    CHK(batch(c0, (unsigned)std::min<int64_t>(width, Nsig - c0), ev_idx));
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
  ctx->timing[0] = ms;
  double phase[3] = {0, 0, 0};  // copy in, steps, combine / copy out
  for (size_t i = 0; i + 3 < ev_idx; i += 4)
    for (size_t j = 0; j < 3; ++j) {
      float t = 0;
      HIPCHK(hipEventElapsedTime(&t, ctx->ev_pool[i + j], ctx->ev_pool[i + j + 1]));
      phase[j] += t;
    }
  ctx->timing[1] = phase[1];
  ctx->timing[2] = (double)(ev_idx / 4) * steps;
  ctx->timing[3] = phase[0];
  ctx->timing[4] = phase[2];
  return GSPX_OK;
}

template <typename T>
static int filter_dev_t(gspx_graph* g, double lmax, int Nf, int M, const double* coeffs,
                        int64_t Nsig, const T* x, T* y, int mode) {
  gspx_ctx* ctx = g->ctx;
  const Options& opt = ctx->opt;
  const int64_t N = g->N;
  for (int i = 0; i < 5; ++i) ctx->timing[i] = 0;
  if (N == 0 || Nsig == 0) return GSPX_OK;
  CHK(ensure_factor<T>(g, lmax));
  std::vector<double> cp;
  halve_c0(Nf, M, coeffs, cp);

  // final-flush / combine stores use the panel's vector width on y rows of Nsig elements
  const int K = M - 1;
  const bool analysis = mode == GSPX_ANALYSIS;
  bool deferred = analysis && (opt.combine == 2 || (opt.combine == 0 && Nf >= 2));
  // workspace per signal: M kept panels (deferred combine) or two panels and Nf accumulators
  const size_t budget = (size_t)std::max<int64_t>(opt.ws_limit_mb, 1) << 20;
  if (deferred && (size_t)N * sizeof(T) * M * (size_t)std::min<int64_t>(Nsig, 4) > budget) deferred = false;
  int64_t max_ld = 0;
  CHK(batch_width(g, sizeof(T), deferred ? (size_t)M : (size_t)(2 + Nf), Nsig, &max_ld));

  // ---- hipGraph replay: an analysis call that repeats the previous one exactly (same graph, lmax,
  // coefficients, pointers, options) is recorded once and replayed as one graph launch - K + 1
  // kernel launches cost ~5 us each, which is the whole call on cache-resident graphs
  std::vector<unsigned char> key;
  const bool graph_mode =
      analysis && Nsig <= max_ld &&
      (opt.graph_launch == 1 || (opt.graph_launch == 2 && (size_t)N * Nsig * sizeof(T) <= ((size_t)32 << 20)));
  if (graph_mode) {
    auto put = [&](const void* p, size_t n) {
      const unsigned char* b = (const unsigned char*)p;
      key.insert(key.end(), b, b + n);
    };
    // the graph by birth number (a destroyed graph's address may be handed out again), every device
    // address the launches carry, the scalars and options they were shaped by
    put(&g->generation, sizeof(g->generation));
    const void* ptrs[] = {x, y, ctx->ws_t.p, ctx->ws_r.p, ctx->ws_w.p, g->coff.p, g->gt_hdr.p, g->gt_s1nat.p,
                          g->fval.p, g->perm.p};
    put(ptrs, sizeof(ptrs));
    put(&lmax, sizeof(lmax));
    put(&g->fval_lmax, sizeof(g->fval_lmax));
    put(&Nf, sizeof(Nf));
    put(&M, sizeof(M));
    put(&Nsig, sizeof(Nsig));
    put(cp.data(), cp.size() * sizeof(double));
    put(&opt, sizeof(opt));
    put(&g->gt_rows, sizeof(g->gt_rows));
    put(&g->gt_slow, sizeof(g->gt_slow));
    if (ctx->graph_exec && !key.empty() && ctx->graph_key == key) {
      HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
      HIPCHK(hipGraphLaunch(ctx->graph_exec, ctx->stream));
      HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      float gms = 0;
      HIPCHK(hipEventElapsedTime(&gms, ctx->ev[0], ctx->ev[1]));
      ctx->timing[0] = gms;
      ctx->timing[1] = gms;  // one graph: no per-phase split
      ctx->timing[2] = (double)K;
      return GSPX_OK;
    }
    if (!key.empty() && ctx->seen_key == key) {  // second identical call: record it
      if (ctx->graph_exec) {
        (void)hipGraphExecDestroy(ctx->graph_exec);
        ctx->graph_exec = nullptr;
      }
      hipGraph_t graph = nullptr;
      size_t dummy = 0;
      HIPCHK(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
      ctx->capturing = true;
      const int rc = run_batch<T>(g, Nf, M, cp, x, (unsigned)Nsig, y, (unsigned)Nsig, (unsigned)Nsig,
                                  deferred, false, true, dummy);
      ctx->capturing = false;
      const hipError_t ce = hipStreamEndCapture(ctx->stream, &graph);
      if (rc != GSPX_OK || ce != hipSuccess || !graph) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        ctx->seen_key.clear();  // fall through to the eager path below
      } else {
        const hipError_t ie = hipGraphInstantiate(&ctx->graph_exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ie == hipSuccess) {
          ctx->graph_key = key;
          return filter_dev_t<T>(g, lmax, Nf, M, coeffs, Nsig, x, y, mode);  // replays
        }
        ctx->graph_exec = nullptr;
        (void)hipGetLastError();
      }
    }
  }
  if (ctx->graph_exec && ctx->graph_key != key) replay_reset(ctx);
  ctx->seen_key = key;  // empty when graph mode is off

  const size_t plane_x = (size_t)N * Nsig;  // synthesis: x is [Nf][N][Nsig]
  return run_batches(g, Nsig, max_ld, K, [&](int64_t c0, unsigned ld, size_t& ev_idx) -> int {
    if (analysis)
      return run_batch<T>(g, Nf, M, cp, x + c0, (unsigned)Nsig, y + c0, (unsigned)Nsig, ld, deferred, false, true,
                          ev_idx);
    // out = sum_f p_f(L) s_f  (filter.py:317-321)
    if (opt.synthesis != 1)
      return run_synthesis_batch<T>(g, Nf, M, cp, x + c0, plane_x, (unsigned)Nsig, y + c0, (unsigned)Nsig, ld, ev_idx);
    // the reference's scheme: one single-filter recurrence per feature, accumulated on
    // device; only the last one writes y (K*Nf sparse products)
    for (int f = 0; f < Nf; ++f) {
      std::vector<double> cf(cp.begin() + (size_t)f * M, cp.begin() + (size_t)(f + 1) * M);
      CHK(run_batch<T>(g, 1, M, cf, x + (size_t)f * plane_x + c0, (unsigned)Nsig, y + c0, (unsigned)Nsig, ld, false,
                       f > 0, f == Nf - 1, ev_idx));
    }
    return GSPX_OK;
  });
}

// ------------------------------------------------------------------------------------------------
// Synthesis  out = sum_f p_f(L) s_f  (filter.py:313-322) by a vector-coefficient Clenshaw
// recurrence.  By linearity  sum_f sum_k c'_fk T_k(Lt) s_f = sum_k T_k(Lt) u_k  with
// u_k = sum_f c'_fk s_f, and Clenshaw evaluates that with ONE recurrence:
//     b_K = u_K,   b_k = u_k + F b_{k+1} - b_{k+2}  (k = K-1..1),   out = u_0 + (F/2) b_1 - b_2
// K sparse products instead of the reference's K*Nf (it runs cheby_op once per filter); each
// step reads the Nf input panels at its own row, (Nf+3) panel passes per order instead of
// Nf*(3 2/3).  Same polynomial, different summation order: agrees to rounding.
// ------------------------------------------------------------------------------------------------
template <typename T>
static int run_synthesis_batch(gspx_graph* g, int nf, int M, const std::vector<double>& cp,
                               const T* x, size_t plane_x, unsigned ldx, T* y, unsigned ldy,
                               unsigned ld, size_t& ev_idx) {
  gspx_ctx* ctx = g->ctx;
  Options opt = ctx->opt;
  hipStream_t st = ctx->stream;
  const int N = (int)g->N;
  const int K = M - 1;
  // (padded work panels as in run_batch; the tile launches span all nf input panels)
  const WorkPanels wp = work_panels<T>(g, opt, true, (size_t)nf, ld, y, ldy);
  const bool padded = wp.padded;
  const unsigned ldw = wp.ldw;
  const size_t U = (size_t)N * ldw;
  const Shape shape = choose_shape(opt, sizeof(T), ld, vec_cap(4, ldy, y));
  const int* perm = g->has_perm ? g->perm.as<int>() : nullptr;

  // weights [K+1][nf]: w[k][f] = c'_fk  (c'_f0 already halved)
  std::vector<T> hw((size_t)M * nf);
  for (int k = 0; k < M; ++k)
    for (int f = 0; f < nf; ++f) hw[(size_t)k * nf + f] = (T)cp[(size_t)f * M + k];
  CHK(ctx->ws_w.ensure(hw.size() * sizeof(T) + 64));
  HIPCHK(hipMemcpyAsync(ctx->ws_w.p, hw.data(), hw.size() * sizeof(T), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  CHK(ctx->ws_r.ensure((size_t)nf * U * sizeof(T) + 256));  // the nf input panels, internal order
  CHK(ctx->ws_t.ensure(2 * U * sizeof(T) + 256));
  T* S = ctx->ws_r.as<T>();
  T* B[2] = {ctx->ws_t.as<T>(), ctx->ws_t.as<T>() + U};

  hipEvent_t ev[4];
  CHK(batch_events(ctx, ev_idx, ev));
  for (int f = 0; f < nf; ++f) {
    const T* xf = x + (size_t)f * plane_x;
    if (padded) {
      const unsigned nbp = (unsigned)std::min<size_t>((U + 255) / 256, 65536);
      hipLaunchKernelGGL((k_permute_in_pad<T>), dim3(nbp), dim3(256), 0, st, xf, ldx, S + (size_t)f * U, ldw, ld, N, perm);
      continue;
    }
    launch_permute_in<T>(xf, ldx, S + (size_t)f * U, ld, N, perm, vec_cap(shape.vec, ldx, xf), st);
  }
  HIPCHK(hipEventRecord(ev[1], st));

  CHK(prepare_coff<T>(g, shape, ld, st));
  StepArgs<T> a = step_base<T>(g, ld, y, ldy);
  a.nf = 1;
  a.nin = nf;
  a.racc = S;
  // (nf input panels: the buffer window of the tile kernel spans all of them)
  const bool tile_ok = wp.tile_direct || padded;
  for (int k = K; k >= 0; --k) {
    if (tile_ok) {
      TileArgs<T> t{};
      const bool has_b2 = (k + 2 <= K);
      t.cur = (k == K) ? S : B[(k + 1) & 1];
      t.old = (k < K && has_b2) ? B[k & 1] : t.cur;
      t.out = B[k & 1];
      t.racc = B[0];  // unused (flush == 0)
      t.y = y;
      t.ldy = ldy;
      t.perm = perm;
      t.scale = (k == K) ? T(0) : (k == 0 ? T(0.5) : T(1));
      t.gamma = (k < K && has_b2) ? T(-1) : T(0);
      t.beta = T(0);
      t.inp = S;
      t.wts = ctx->ws_w.as<T>() + (size_t)k * nf;
      t.nin = nf;
      t.flush = 0;
      t.final = (k == 0 && !padded) ? 1 : 0;  // padded rows: b_0 stays in B[0] and is copied out below
      t.reverse = (opt.alternate_sweep && (k & 1)) ? 1 : 0;
      CHK(launch_step_tile<T>(g, opt, t, ldw, st));
      continue;
    }
    a.wts = ctx->ws_w.as<T>() + (size_t)k * nf;
    a.final = (k == 0) ? 1 : 0;
    a.flush = 0;
    if (k == K) {  // b_K = u_K : no product needed (scale 0 on any valid panel)
      a.cur = S;
      a.old = S;
      a.out = B[k & 1];
      a.scale = T(0);
      a.gamma = T(0);
    } else {
      a.cur = B[(k + 1) & 1];
      a.out = B[k & 1];
      const bool has_b2 = (k + 2 <= K);
      a.old = has_b2 ? B[k & 1] : a.cur;
      a.gamma = has_b2 ? T(-1) : T(0);
      a.scale = (k == 0) ? T(0.5) : T(1);
    }
    a.reverse = (opt.alternate_sweep && (k & 1)) ? 1 : 0;
    launch_step<T>(a, shape, opt, st, g->coff.as<unsigned>());
  }
  HIPCHK(hipEventRecord(ev[2], st));
  if (padded) {
    const unsigned nbp = (unsigned)std::min<size_t>(((size_t)N * ld + 255) / 256, 65536);
    hipLaunchKernelGGL((k_permute_out_pad<T>), dim3(nbp), dim3(256), 0, st, B[0], ldw, y, ldy, ld, N, perm);
  }
  HIPCHK(hipEventRecord(ev[3], st));
  HIPCHK(hipGetLastError());
  return GSPX_OK;
}

// ------------------------------------------------------------------------------------------------
// Newton-form evaluation of the SAME polynomial (single filter, analysis):
//     p(Lt) x = sum_j d_j prod_{i<j} (Lt - r_i I) x,   Lt = (L - a2 I)/a1 = F/2
// by Horner:  h_K = d_K x,  h_j = (Lt - r_j I) h_{j+1} + d_j x,  y = h_0.
// A two-term recurrence: per order it gathers h, reads x and writes h (3 panels) and needs NO
// accumulator, where the three-term Chebyshev recurrence moves 3 + 2/3.  Nodes (Leja-ordered
// Chebyshev points) and divided differences are computed by the caller in exact arithmetic from
// the reference's Chebyshev coefficients (pygsp_amd/filters.py::cheb_to_newton), so the polynomial
// is identical; results agree with the reference to ~1e-14 (fp64).
// ------------------------------------------------------------------------------------------------
// A polynomial PROGRAM on one batch of columns: h_0 = x (copied into the internal order), then S steps
//     h_{s+1} = scale_s * (F h_s) + beta_s * h_s + gamma_s * o_s,
// o_s = x for every step (old_is_x: the Newton form's Horner recurrence) or o_s = h_{s-1} (the product form's quadratic
// factors; h_{s+1} then overwrites h_{s-1} in place, as the three-term recurrence does); the last step stores y.
// F = (2/a1)(L - a2 I) has its spectrum in [-2, 2]: a factor (t - r) of a polynomial in t = F/2 is scale 1/2, beta -r.
// A step whose gamma is 0 reads no third panel at all: gather h_s, write h_{s+1} - two panel passes.
template <typename T>
static int run_program_batch(gspx_graph* g, int S, const double* sc, const double* be, const double* ga, bool old_is_x,
                             const T* x, unsigned ldx, T* y, unsigned ldy, unsigned ld, size_t& ev_idx) {
  gspx_ctx* ctx = g->ctx;
  Options opt = ctx->opt;
  hipStream_t st = ctx->stream;
  const int N = (int)g->N;
  const size_t U = (size_t)N * ld;
  const Shape shape = choose_shape(opt, sizeof(T), ld, vec_cap(4, ldy, y));
  const int* perm = g->has_perm ? g->perm.as<int>() : nullptr;

  const T hw[3] = {T(1), T(0), T(0)};  // final step of the plain kernels: y = 1 * h
  CHK(ctx->ws_w.ensure(sizeof(hw) + 64));
  HIPCHK(hipMemcpyAsync(ctx->ws_w.p, hw, sizeof(hw), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  // panels: X (h_0; kept for the whole call when every step reads it) and one or two more
  CHK(ctx->ws_t.ensure((old_is_x ? 3 : 2) * U * sizeof(T) + 256));
  T* X = ctx->ws_t.as<T>();
  T* H[2] = {X + U, old_is_x ? X + 2 * U : X};  // product form: ping-pong between the second panel and X itself

  hipEvent_t ev[4];
  CHK(batch_events(ctx, ev_idx, ev));
  launch_permute_in<T>(x, ldx, X, ld, N, perm, vec_cap(shape.vec, ldx, x), st);
  HIPCHK(hipEventRecord(ev[1], st));

  CHK(prepare_coff<T>(g, shape, ld, st));
  StepArgs<T> a = step_base<T>(g, ld, y, ldy);
  a.nf = 1;
  a.racc = H[0];  // never read (flush == 1) - any valid panel
  a.wts = ctx->ws_w.as<T>();
  const bool tile_ok = tile_usable<T>(g, opt, ld, y, ldy);
  for (int s = 0; s < S; ++s) {
    const bool last = s == S - 1;
    const T* cur = (s == 0) ? X : H[(s - 1) & 1];
    T* out = H[s & 1];
    // o_s: x, or h_{s-1} - which lives in the panel this step writes (s >= 1: H[(s - 2) & 1] == H[s & 1]; s == 0 has none)
    const T* old = old_is_x ? X : (const T*)out;
    const double gam = (!old_is_x && s == 0) ? 0.0 : ga[s];
    if (tile_ok) {
      TileArgs<T> t{};
      t.cur = cur;
      t.old = gam == 0.0 ? cur : old;
      t.out = out;
      t.racc = H[0];  // never read or written (flush == 0)
      t.y = y;
      t.ldy = ldy;
      t.perm = perm;
      t.scale = (T)sc[s];
      t.beta = (T)be[s];
      t.gamma = (T)gam;
      t.flush = 0;
      t.final = last ? 1 : 0;
      t.reverse = (opt.alternate_sweep && (s & 1)) ? 1 : 0;
      CHK(launch_step_tile<T>(g, opt, t, ld, st));
      continue;
    }
    a.cur = cur;
    a.old = gam == 0.0 ? cur : old;
    a.out = out;
    a.scale = (T)sc[s];
    a.beta = (T)be[s];
    a.gamma = (T)gam;
    a.flush = last ? 1 : 0;
    a.final = last ? 1 : 0;
    a.reverse = (opt.alternate_sweep && (s & 1)) ? 1 : 0;
    launch_step<T>(a, shape, opt, st, g->coff.as<unsigned>());
  }
  HIPCHK(hipEventRecord(ev[2], st));
  HIPCHK(hipEventRecord(ev[3], st));
  HIPCHK(hipGetLastError());
  return GSPX_OK;
}

template <typename T>
static int program_dev_t(gspx_graph* g, double lmax, int S, const double* sc, const double* be, const double* ga,
                         bool old_is_x, int64_t Nsig, const T* x, T* y) {
  gspx_ctx* ctx = g->ctx;
  replay_reset(ctx);  // (a program rewrites the weights and panels a recorded filter call replays from)
  for (int i = 0; i < 5; ++i) ctx->timing[i] = 0;
  if (g->N == 0 || Nsig == 0) return GSPX_OK;
  CHK(ensure_factor<T>(g, lmax));
  int64_t max_ld = 0;
  CHK(batch_width(g, sizeof(T), 3, Nsig, &max_ld));
  CHK(run_batches(g, Nsig, max_ld, S, [&](int64_t c0, unsigned ld, size_t& ev_idx) {
    return run_program_batch<T>(g, S, sc, be, ga, old_is_x, x + c0, (unsigned)Nsig, y + c0, (unsigned)Nsig, ld, ev_idx);
  }));
  ctx->timing[4] = 0;  // no combine: the last step stores y
  return GSPX_OK;
}

// the Newton form p(t) = sum_j d_j prod_{i<j} (t - r_i) by Horner, as a program with o_s = x (old_is_x):
// h <- (t - r_j) h + d_j x, j = K-1 .. 0
static void horner_program(int K, const double* nodes, const double* dc, std::vector<double>& sc,
                           std::vector<double>& be, std::vector<double>& ga) {
  sc.assign((size_t)K, 0.0);
  be.assign((size_t)K, 0.0);
  ga.assign((size_t)K, 0.0);
  for (int s = 0; s < K; ++s) {
    const int j = K - 1 - s;
    if (s == 0) {  // h_1 = d_K (t - r_{K-1}) x + d_{K-1} x
      sc[0] = 0.5 * dc[K];
      be[0] = 0.0;
      ga[0] = dc[j] - dc[K] * nodes[j];
    } else {
      sc[(size_t)s] = 0.5;
      be[(size_t)s] = -nodes[j];
      ga[(size_t)s] = dc[j];
    }
  }
}

// a device call on the graph's element type: run(x, y, Nsig) with x, y typed; kernel_ms: its device time
template <typename Run>
static int device_call(gspx_graph* g, int64_t Nsig, const void* x, void* y, double* kernel_ms, const Run& run) {
  HIPCHK(hipSetDevice(g->ctx->device));
  const int rc = g->dtype == GSPX_F32 ? run((const float*)x, (float*)y, Nsig) : run((const double*)x, (double*)y, Nsig);
  if (rc == GSPX_OK && kernel_ms) *kernel_ms = g->ctx->timing[0];
  return rc;
}

static int check_program_args(gspx_graph* g, double lmax, int S, const double* scale, const double* beta,
                              const double* gamma, int64_t Nsig, const void* x, void* y) {
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (S < 1) return set_err(GSPX_ERR_COEFF, "The coefficients have an invalid shape");
  if (!scale || !beta || !gamma) return set_err(GSPX_ERR_INVALID, "null program");
  if (Nsig < 0) return set_err(GSPX_ERR_INVALID, "negative number of signals");
  if (!(lmax > 0.0) || !std::isfinite(lmax))
    return set_err(GSPX_ERR_INVALID, "lmax must be positive and finite (got %g)", lmax);
  if (Nsig > 0 && g->N > 0 && (!x || !y)) return set_err(GSPX_ERR_INVALID, "null signal pointer");
  for (int i = 0; i < S; ++i)
    if (!std::isfinite(scale[i]) || !std::isfinite(beta[i]) || !std::isfinite(gamma[i]))
      return set_err(GSPX_ERR_INVALID, "non-finite program coefficient");
  if (Nsig >= ((int64_t)1 << 31) / 16) return set_err(GSPX_ERR_INVALID, "too many signals");
  return GSPX_OK;
}

// A polynomial of the scaled operator t = (2 / lmax) L - I evaluated as a PROGRAM of S steps on device panels
// (see run_program_batch): h_0 = x; h_{s+1} = scale_s (2 t) h_s + beta_s h_s + gamma_s o_s; y = h_S.  old_is_x != 0: o_s = x
// (the Newton form); 0: o_s = h_{s-1}, gamma_0 ignored (the PRODUCT form: a real root r of the polynomial is one step
// with scale sigma / 2, beta -sigma r, gamma 0 - two panel passes -, a conjugate pair a +- ib two steps, the second with
// gamma sigma^2 b^2 - three passes).  pygsp_amd.filters.cheb_to_product builds such programs from Chebyshev coefficients.
extern "C" int gspx_poly_program_dev(gspx_graph* g, double lmax, int S, const double* scale, const double* beta,
                                     const double* gamma, int old_is_x, int64_t Nsig, const void* x_dev, void* y_dev,
                                     double* kernel_ms) {
  if (g) replay_reset(g->ctx);
  CHK(check_program_args(g, lmax, S, scale, beta, gamma, Nsig, x_dev, y_dev));
  return device_call(g, Nsig, x_dev, y_dev, kernel_ms, [&](auto x, auto y, int64_t n) {
    return program_dev_t(g, lmax, S, scale, beta, gamma, old_is_x != 0, n, x, y);
  });
}

static int check_newton_args(gspx_graph* g, double lmax, int K, const double* nodes, const double* dcoef,
                             int64_t Nsig, const void* x, void* y) {
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (K < 1) return set_err(GSPX_ERR_COEFF, "The coefficients have an invalid shape");
  if (!nodes || !dcoef) return set_err(GSPX_ERR_INVALID, "null nodes / coefficients");
  if (Nsig < 0) return set_err(GSPX_ERR_INVALID, "negative number of signals");
  if (!(lmax > 0.0) || !std::isfinite(lmax))
    return set_err(GSPX_ERR_INVALID, "lmax must be positive and finite (got %g)", lmax);
  if (Nsig > 0 && g->N > 0 && (!x || !y))
    return set_err(GSPX_ERR_INVALID, "null signal pointer");
  for (int i = 0; i < K; ++i)
    if (!std::isfinite(nodes[i])) return set_err(GSPX_ERR_INVALID, "non-finite node");
  for (int i = 0; i <= K; ++i)
    if (!std::isfinite(dcoef[i])) return set_err(GSPX_ERR_INVALID, "non-finite coefficient");
  if (Nsig >= ((int64_t)1 << 31) / 16) return set_err(GSPX_ERR_INVALID, "too many signals");
  return GSPX_OK;
}

extern "C" int gspx_newton_filter_dev(gspx_graph* g, double lmax, int K, const double* nodes,
                                      const double* dcoef, int64_t Nsig, const void* x_dev,
                                      void* y_dev, double* kernel_ms) {
  if (g) replay_reset(g->ctx);
  CHK(check_newton_args(g, lmax, K, nodes, dcoef, Nsig, x_dev, y_dev));
  std::vector<double> sc, be, ga;
  horner_program(K, nodes, dcoef, sc, be, ga);
  return device_call(g, Nsig, x_dev, y_dev, kernel_ms, [&](auto x, auto y, int64_t n) {
    return program_dev_t(g, lmax, K, sc.data(), be.data(), ga.data(), true, n, x, y);
  });
}

#include "gspx_hostpipe.hip.h"

// What the host-array entry points share, after the checks the caller makes up front.  An empty call does nothing;
// `prepare` (the checks that come after the empty-call test, and any setup) runs next.  A large call is pipelined in
// column batches (gspx_hostpipe.hip.h); any other - or one the pipeline steps aside for - is one copy in through io_x,
// run(x, y, Nsig) on the device copies, one copy out through io_y.  x / y hold in_planes / out_planes [N][Nsig] planes.
template <typename Prepare, typename Run>
static int host_call(gspx_graph* g, int64_t Nsig, int in_planes, int out_planes, const void* x_host, void* y_host,
                     double* kernel_ms, const Prepare& prepare, const Run& run) {
  gspx_ctx* ctx = g->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  if (g->N == 0 || Nsig <= 0) {
    if (kernel_ms) *kernel_ms = 0;
    return GSPX_OK;
  }
  CHK(prepare());
  const size_t e = elt_size(g->dtype);
  std::vector<int64_t> widths;
  int threads = 1;
  host_pipeline_shape(ctx->opt, e, g->N, Nsig, in_planes + out_planes, &widths, &threads);
  if (widths.size() >= 2) {
    if (!ctx->pipe) ctx->pipe = new HostPipe();
    replay_reset(ctx);
    const int rc = g->dtype == GSPX_F32
                       ? filter_host_pipelined<float>(g, Nsig, in_planes, out_planes, (const float*)x_host,
                                                      (float*)y_host, widths, threads, kernel_ms, run)
                       : filter_host_pipelined<double>(g, Nsig, in_planes, out_planes, (const double*)x_host,
                                                       (double*)y_host, widths, threads, kernel_ms, run);
    if (rc != GSPX_HOSTPIPE_UNAVAILABLE) return rc;
    // an in-place call, or no pinned / device staging memory to be had: the one-shot form below
  }
  if (ctx->pipe) {  // this host call is not pipelined: no stage times, no timeline of an earlier call
    ctx->pipe->timing[6] = 0;
    ctx->pipe->timeline.clear();
  }
  const size_t n_in = (size_t)in_planes * g->N * Nsig * e, n_out = (size_t)out_planes * g->N * Nsig * e;
  CHK(ctx->io_x.ensure(n_in));
  CHK(ctx->io_y.ensure(n_out));
  HIPCHK(hipMemcpyAsync(ctx->io_x.p, x_host, n_in, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  CHK(device_call(g, Nsig, ctx->io_x.p, ctx->io_y.p, kernel_ms, run));
  HIPCHK(hipMemcpyAsync(y_host, ctx->io_y.p, n_out, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return GSPX_OK;
}

// gspx_newton_filter_dev with host arrays
extern "C" int gspx_newton_filter(gspx_graph* g, double lmax, int K, const double* nodes,
                                  const double* dcoef, int64_t Nsig, const void* x_host,
                                  void* y_host, double* kernel_ms) {
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (Nsig > 0 && g->N > 0 && (!x_host || !y_host))
    return set_err(GSPX_ERR_INVALID, "null signal pointer");
  if (K < 1) return set_err(GSPX_ERR_COEFF, "The coefficients have an invalid shape");
  std::vector<double> sc, be, ga;
  auto prepare = [&]() -> int {
    CHK(check_newton_args(g, lmax, K, nodes, dcoef, Nsig, x_host, y_host));
    horner_program(K, nodes, dcoef, sc, be, ga);
    return GSPX_OK;
  };
  return host_call(g, Nsig, 1, 1, x_host, y_host, kernel_ms, prepare, [&](auto x, auto y, int64_t n) {
    return program_dev_t(g, lmax, K, sc.data(), be.data(), ga.data(), true, n, x, y);
  });
}

static int check_filter_args(gspx_graph* g, double lmax, int Nf, int M, const double* coeffs,
                             int64_t Nsig, const void* x, void* y, int mode) {
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (M < 2) return set_err(GSPX_ERR_COEFF, "The coefficients have an invalid shape");
  if (Nf < 1) return set_err(GSPX_ERR_INVALID, "Nf must be >= 1");
  if (!coeffs) return set_err(GSPX_ERR_INVALID, "null coefficients");
  if (Nsig < 0) return set_err(GSPX_ERR_INVALID, "negative number of signals");
  if (mode != GSPX_ANALYSIS && mode != GSPX_SYNTHESIS)
    return set_err(GSPX_ERR_INVALID, "unknown mode %d", mode);
  if (!(lmax > 0.0) || !std::isfinite(lmax))
    return set_err(GSPX_ERR_INVALID, "lmax must be positive and finite (got %g)", lmax);
  if (Nsig > 0 && g->N > 0 && (!x || !y)) return set_err(GSPX_ERR_INVALID, "null signal pointer");
  for (int64_t i = 0; i < (int64_t)Nf * M; ++i)
    if (!std::isfinite(coeffs[i])) return set_err(GSPX_ERR_INVALID, "non-finite coefficient");
  if (Nsig >= ((int64_t)1 << 31) / 16) return set_err(GSPX_ERR_INVALID, "too many signals");
  return GSPX_OK;
}

extern "C" int gspx_cheby_filter_dev(gspx_graph* g, double lmax, int Nf, int M,
                                     const double* coeffs, int64_t Nsig, const void* x_dev,
                                     void* y_dev, int mode, double* kernel_ms) {
  CHK(check_filter_args(g, lmax, Nf, M, coeffs, Nsig, x_dev, y_dev, mode));
  return device_call(g, Nsig, x_dev, y_dev, kernel_ms, [&](auto x, auto y, int64_t n) {
    return filter_dev_t(g, lmax, Nf, M, coeffs, n, x, y, mode);
  });
}

extern "C" int gspx_cheby_filter(gspx_graph* g, double lmax, int Nf, int M, const double* coeffs,
                                 int64_t Nsig, const void* x_host, void* y_host, int mode,
                                 double* kernel_ms) {
  CHK(check_filter_args(g, lmax, Nf, M, coeffs, Nsig, x_host, y_host, mode));
  const bool analysis = mode == GSPX_ANALYSIS;
  return host_call(g, Nsig, analysis ? 1 : Nf, analysis ? Nf : 1, x_host, y_host, kernel_ms,
                   [] { return (int)GSPX_OK; }, [&](auto x, auto y, int64_t n) {
                     return filter_dev_t(g, lmax, Nf, M, coeffs, n, x, y, mode);
                   });
}

// ------------------------------------------------------------------------------------------------
// Squared column norms of a filterbank applied to device signals (features.compute_norm_tig / compute_spectrogram):
// the deferred plan for every Nf, Nf = 1 included, and per column batch k_combine_sqnorm over the kept slots in place
// of k_combine.  Nothing of size Nf x N x w exists: the workspaces are the M slots, the coefficient table, the Nf x Nsig
// norms and the workgroup partials.  out: HOST, Nf x Nsig.
// ------------------------------------------------------------------------------------------------
template <typename T>
static int sqnorms_dev_t(gspx_graph* g, double lmax, int Nf, int M, const double* coeffs, int64_t Nsig, const T* x,
                         double* out) {
  gspx_ctx* ctx = g->ctx;
  const int64_t N = g->N;
  for (int i = 0; i < 5; ++i) ctx->timing[i] = 0;
  if (Nsig == 0) return GSPX_OK;
  if (N == 0) {
    std::fill(out, out + (size_t)Nf * Nsig, 0.0);
    return GSPX_OK;
  }
  int64_t width = 0;
  CHK(batch_width(g, sizeof(T), (size_t)M, Nsig, &width));
  std::vector<double> cp;
  halve_c0(Nf, M, coeffs, cp);
  const int ldc = (Nf + SQ_PASS - 1) / SQ_PASS * SQ_PASS;  // [k][ldc], zero beyond Nf: a pass never reads past it
  std::vector<double> hc((size_t)M * ldc, 0.0);
  for (int f = 0; f < Nf; ++f)
    for (int k = 0; k < M; ++k) hc[(size_t)k * ldc + f] = cp[(size_t)f * M + k];
  const size_t cbytes = (hc.size() * sizeof(double) + 255) / 256 * 256, obytes = (size_t)Nf * Nsig * sizeof(double);
  const int64_t first = std::min<int64_t>(width, Nsig), last = Nsig - (Nsig - 1) / width * width;
  const size_t parts = std::max(sqnorm_parts(ctx, (int)N, (unsigned)first), sqnorm_parts(ctx, (int)N, (unsigned)last));
  CHK(ctx->ws_sq.ensure(cbytes + obytes + 256));
  CHK(ctx->ws_sqp.ensure(parts * sizeof(double) + 256));
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(ctx->ws_sq.p, hc.data(), hc.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));  // hc is a stack-owned staging buffer
  CHK(ensure_factor<T>(g, lmax));
  double* outd = (double*)((char*)ctx->ws_sq.p + cbytes);
  const SqNorms sq{ctx->ws_sq.as<double>(), ldc, Nf, outd, (size_t)Nsig, ctx->ws_sqp.as<double>()};
  CHK(run_batches(g, Nsig, width, M - 1, [&](int64_t c0, unsigned ld, size_t& ev_idx) -> int {
    SqNorms b = sq;
    b.out = outd + c0;
    return run_batch<T>(g, Nf, M, cp, x + c0, (unsigned)Nsig, (T*)nullptr, ld, ld, true, false, false, ev_idx, &b);
  }));
  HIPCHK(hipMemcpyAsync(out, outd, obytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return GSPX_OK;
}

extern "C" int gspx_cheby_sqnorms_dev(gspx_graph* g, double lmax, int Nf, int M, const double* coeffs, int64_t Nsig,
                                      const void* x_dev, double* out, double* kernel_ms) {
  if (g) replay_reset(g->ctx);
  CHK(check_filter_args(g, lmax, Nf, M, coeffs, Nsig, x_dev, out, GSPX_ANALYSIS));
  if (M > 256) return set_err(GSPX_ERR_INVALID, "gspx_cheby_sqnorms_dev: at most 256 coefficients per filter");
  if (Nsig > 0 && !out) return set_err(GSPX_ERR_INVALID, "gspx_cheby_sqnorms_dev: null output");
  return device_call(g, Nsig, x_dev, out, kernel_ms, [&](auto x, auto, int64_t n) {
    return sqnorms_dev_t(g, lmax, Nf, M, coeffs, n, x, out);
  });
}

// gspx_poly_program_dev with host arrays
extern "C" int gspx_poly_program(gspx_graph* g, double lmax, int S, const double* scale, const double* beta,
                                 const double* gamma, int old_is_x, int64_t Nsig, const void* x_host, void* y_host,
                                 double* kernel_ms) {
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (Nsig > 0 && g->N > 0 && (!x_host || !y_host)) return set_err(GSPX_ERR_INVALID, "null signal pointer");
  if (S < 1) return set_err(GSPX_ERR_COEFF, "The coefficients have an invalid shape");
  auto prepare = [&] { return check_program_args(g, lmax, S, scale, beta, gamma, Nsig, x_host, y_host); };
  return host_call(g, Nsig, 1, 1, x_host, y_host, kernel_ms, prepare, [&](auto x, auto y, int64_t n) {
    return program_dev_t(g, lmax, S, scale, beta, gamma, old_is_x != 0, n, x, y);
  });
}

// host-only: the column batches and thread count the pipelined host-pointer call would use (for schedule tests)
extern "C" int gspx_host_pipeline_describe(int mode, int64_t host_batch, int64_t host_edge, int64_t host_threads,
                                           int dtype, int64_t N, int64_t Nsig, int planes_total, int64_t* widths,
                                           int capacity, int* n_batches, int* threads) {
  if (!n_batches || N < 0 || Nsig < 0 || planes_total < 1 || (dtype != GSPX_F32 && dtype != GSPX_F64))
    return set_err(GSPX_ERR_INVALID, "bad argument");
  Options opt;
  opt.host_pipeline = mode;
  opt.host_batch = host_batch;
  opt.host_edge = host_edge;
  opt.host_threads = host_threads;
  std::vector<int64_t> w;
  int t = 1;
  host_pipeline_shape(opt, elt_size(dtype), N, Nsig, planes_total, &w, &t);
  if (w.size() < 2) w.clear();  // (a single batch is the one-shot form)
  *n_batches = (int)w.size();
  if (threads) *threads = t;
  if (widths)
    for (int i = 0; i < capacity && i < (int)w.size(); ++i) widths[i] = w[(size_t)i];
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

// ------------------------------------------------------------------------------------------------
// lambda_max by Lanczos ON DEVICE (replaces the ARPACK call of
// graph.py:911-917, 3.3 s on the host at N = 1M).  Plain three-term Lanczos on L with a fixed
// start vector (deterministic, unlike ARPACK's random start); the largest Ritz value of the
// tridiagonal matrix is found by bisection on the host.  Stops when the residual of the Ritz pair,
// beta_j |s_j|, is below `tol` * theta (an eigenvalue of L lies within that distance) or after
// max_iter steps.  Returns the Ritz value itself (<= lambda_max); the caller
// applies the reference's 1 % safety factor (graph.py:920).
// ------------------------------------------------------------------------------------------------
static double tridiag_max_eig(const std::vector<double>& al, const std::vector<double>& be) {
  // Gershgorin bracket + Sturm-sequence bisection for the largest eigenvalue
  const int m = (int)al.size();
  double lo = al[0], hi = al[0];
  for (int i = 0; i < m; ++i) {
    const double r = (i > 0 ? std::fabs(be[i - 1]) : 0.0) + (i + 1 < m ? std::fabs(be[i]) : 0.0);
    lo = std::min(lo, al[i] - r);
    hi = std::max(hi, al[i] + r);
  }
  auto count_below = [&](double x) {  // eigenvalues < x
    int cnt = 0;
    double q = al[0] - x;
    if (q < 0) ++cnt;
    for (int i = 1; i < m; ++i) {
      const double d = (q == 0.0) ? 1e-300 : q;
      q = al[i] - x - be[i - 1] * be[i - 1] / d;
      if (q < 0) ++cnt;
    }
    return cnt;
  };
  for (int it = 0; it < 200 && hi - lo > 1e-14 * std::max(1.0, std::fabs(hi)); ++it) {
    const double mid = 0.5 * (lo + hi);
    if (count_below(mid) >= m) hi = mid; else lo = mid;
  }
  return 0.5 * (lo + hi);
}

template <typename T>
static int lanczos_t(gspx_graph* g, int max_iter, double tol, double* out, int* iters, int* converged) {
  gspx_ctx* ctx = g->ctx;
  hipStream_t st = ctx->stream;
  const int N = (int)g->N;
  *out = 0.0;
  if (iters) *iters = 0;
  if (converged) *converged = 1;
  if (N == 0) return GSPX_OK;
  // L v = 0.5 * F v + v  with F = 2 (L - I), i.e. the factor matrix for lmax = 2
  CHK(ensure_factor<T>(g, 2.0));
  Options opt = ctx->opt;
  opt.kernel = 2;  // one signal: narrow kernel
  const Shape shape = choose_shape(opt, sizeof(T), 1, 1);
  DevMem vbuf, partial, scal;
  CHK(vbuf.alloc((size_t)3 * N * sizeof(T)));
  const int nb = std::min(1024, std::max(1, (N + 255) / 256));
  CHK(partial.alloc((size_t)nb * sizeof(double)));
  CHK(scal.alloc(sizeof(double)));
  T* v[3] = {vbuf.as<T>(), vbuf.as<T>() + N, vbuf.as<T>() + 2 * (size_t)N};
  auto dot = [&](const T* x, const T* y, double* res) -> int {
    hipLaunchKernelGGL((k_dot_partial<T>), dim3(nb), dim3(256), 0, st, x, y, (size_t)N,
                       partial.as<double>());
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, st, partial.as<double>(), nb,
                       scal.as<double>());
    HIPCHK(hipMemcpyAsync(res, scal.p, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GSPX_OK;
  };
  hipLaunchKernelGGL((k_start_vector<T>), dim3(nb), dim3(256), 0, st, v[0], (size_t)N);
  double nrm2 = 0;
  CHK(dot(v[0], v[0], &nrm2));
  if (!(nrm2 > 0)) return GSPX_OK;
  hipLaunchKernelGGL((k_axpby<T>), dim3(nb), dim3(256), 0, st, T(0), v[0], (T)(1.0 / std::sqrt(nrm2)),
                     v[0], (size_t)N);
  StepArgs<T> a{};
  a.rowptr = g->rptr.as<int>();
  a.col = g->rcol.as<int>();
  a.val = g->fval.as<T>();
  a.N = N;
  a.ld = 1;
  a.curbytes = (u32)((size_t)N * sizeof(T));
  a.scale = T(0.5);
  a.gamma = T(0);
  a.beta = T(1);
  std::vector<double> al, be;
  double theta = 0, beta_prev = 0;
  bool met = false;  // the residual criterion was met (or the Krylov space became invariant: theta is exact)
  int cur = 0, prev = 2;
  for (int j = 0; j < max_iter && j < N; ++j) {
    const int nxt = 3 - cur - prev;  // the third buffer
    a.cur = v[cur];
    a.old = v[cur];
    a.out = v[nxt];
    launch_step<T>(a, shape, opt, st, nullptr);  // w = L v_j
    if (j > 0)
      hipLaunchKernelGGL((k_axpby<T>), dim3(nb), dim3(256), 0, st, (T)(-beta_prev), v[prev], T(1),
                         v[nxt], (size_t)N);
    double alpha = 0;
    CHK(dot(v[nxt], v[cur], &alpha));
    hipLaunchKernelGGL((k_axpby<T>), dim3(nb), dim3(256), 0, st, (T)(-alpha), v[cur], T(1), v[nxt],
                       (size_t)N);
    double b2 = 0;
    CHK(dot(v[nxt], v[nxt], &b2));
    al.push_back(alpha);
    theta = tridiag_max_eig(al, be);
    if (iters) *iters = j + 1;
    const double beta = std::sqrt(std::max(b2, 0.0));
    if (!(beta > 1e-300 * std::max(1.0, std::fabs(theta)))) {  // invariant subspace
      met = true;
      break;
    }
    // residual of the Ritz pair: ||L y - theta y|| = beta_j |s_j|, s = unit eigenvector of the
    // tridiagonal matrix for theta; its components come from the backward recurrence (the stable
    // direction for the extreme eigenvalue).  There is an eigenvalue of L within that distance of
    // theta - a bound, unlike "theta stopped moving", which stalls on plateaus.
    {
      const int m = (int)al.size();
      double w_next = 0.0, w_cur = 1.0, w_last = 1.0, nrm2w = 1.0;  // w_m = 1
      for (int i = m - 1; i >= 1; --i) {
        // row i (0-based) of (T - theta) w = 0:  be[i-1] w_{i-1} + (al[i] - theta) w_i + be[i] w_{i+1} = 0
        const double up = (i < m - 1) ? be[(size_t)i] * w_next : 0.0;
        const double w_prev = ((theta - al[(size_t)i]) * w_cur - up) / be[(size_t)i - 1];
        w_next = w_cur;
        w_cur = w_prev;
        nrm2w += w_cur * w_cur;
        if (nrm2w > 1e200) {  // rescale everything, the last component included
          w_next *= 1e-100;
          w_cur *= 1e-100;
          w_last *= 1e-100;
          nrm2w *= 1e-200;
        }
      }
      const double s_last = w_last / std::sqrt(nrm2w);
      if (j >= 2 && beta * std::fabs(s_last) <= tol * std::fabs(theta)) {
        met = true;
        break;
      }
    }
    be.push_back(beta);
    hipLaunchKernelGGL((k_axpby<T>), dim3(nb), dim3(256), 0, st, T(0), v[nxt], (T)(1.0 / beta),
                       v[nxt], (size_t)N);
    beta_prev = beta;
    prev = cur;
    cur = nxt;
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  *out = theta;
  if (converged) *converged = (met || (int)al.size() >= N) ? 1 : 0;  // N steps span the whole space
  return GSPX_OK;
}

extern "C" int gspx_lanczos_lmax(gspx_graph* g, int max_iter, double tol, double* lmax,
                                 int* iterations, int* converged) {
  if (g) replay_reset(g->ctx);
  if (!g || !lmax) return set_err(GSPX_ERR_INVALID, "null argument");
  if (max_iter < 1 || !(tol > 0)) return set_err(GSPX_ERR_INVALID, "max_iter >= 1 and tol > 0");
  HIPCHK(hipSetDevice(g->ctx->device));
  return g->dtype == GSPX_F32 ? lanczos_t<float>(g, max_iter, tol, lmax, iterations, converged)
                              : lanczos_t<double>(g, max_iter, tol, lmax, iterations, converged);
}

// ------------------------------------------------------------------------------------------------
// calibration: streaming copy with the engine's own 16-byte-per-lane copy kernel (k_permute_in
// without a permutation) - the measured HBM ceiling quoted beside every roofline fraction.
// ------------------------------------------------------------------------------------------------
// Columns [j0, j0 + w) of the N x N identity as a row-major N x w panel, written on the device: the
// input of Filter.compute_frame (filter.py:593-600 filters np.identity(N)) without an N x N host array or
// its trip over PCIe.
template <typename T> __global__ void k_identity_panel(T* __restrict__ out, int N, int j0, int w) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)N * w) return;
  const int row = (int)(i / w), col = (int)(i % w);
  out[i] = row == j0 + col ? T(1) : T(0);
}

extern "C" int gspx_identity_panel_dev(gspx_ctx* ctx, int dtype, int64_t N, int64_t j0, int64_t w, void* out_dev) {
  if (!ctx || N < 0 || j0 < 0 || w < 0 || j0 + w > N || (dtype != GSPX_F32 && dtype != GSPX_F64))
    return set_err(GSPX_ERR_INVALID, "gspx_identity_panel_dev: bad argument");
  if (N * w == 0) return GSPX_OK;
  if (!out_dev) return set_err(GSPX_ERR_INVALID, "gspx_identity_panel_dev: null output");
  if (N >= ((int64_t)1 << 31) || w >= ((int64_t)1 << 31))
    return set_err(GSPX_ERR_INVALID, "gspx_identity_panel_dev: panel too large");
  HIPCHK(hipSetDevice(ctx->device));
  const size_t total = (size_t)N * (size_t)w;
  const unsigned nb = (unsigned)((total + 255) / 256);
  if (dtype == GSPX_F32)
    hipLaunchKernelGGL((k_identity_panel<float>), dim3(nb), dim3(256), 0, ctx->stream, (float*)out_dev, (int)N,
                       (int)j0, (int)w);
  else
    hipLaunchKernelGGL((k_identity_panel<double>), dim3(nb), dim3(256), 0, ctx->stream, (double*)out_dev, (int)N,
                       (int)j0, (int)w);
  HIPCHK(hipGetLastError());
  return GSPX_OK;
}

// (vertex, signal, feature) tensor <-> feature planes [feature][vertex][signal]: the two layouts a signal cube
// has on either side of Filter.filter (filter.py:310-311, 315-316) - for device-resident arrays that arrive in
// the "wrong" one (an (N, Nf) panel of Nf signals read as one signal with Nf features, filter.py:270-278).
// One thread per element of the planes side, whose accesses are the coalesced ones; the cube side of a vertex
// is S * F contiguous elements, so its lines are shared by neighbouring lanes.
template <typename T>
__global__ void k_planes_pack(const T* __restrict__ src, T* __restrict__ dst, int64_t N, int S, int F, int to_planes) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // index in [f][n][s]
  if (i >= N * S * F) return;
  const int s = (int)(i % S);
  const int64_t n = (i / S) % N;
  const int f = (int)(i / ((int64_t)S * N));
  const int64_t cube = (n * S + s) * F + f;
  if (to_planes) dst[i] = src[cube];
  else dst[cube] = src[i];
}

extern "C" int gspx_planes_pack_dev(gspx_ctx* ctx, int dtype, int64_t N, int64_t S, int64_t F, const void* src_dev,
                                    void* dst_dev, int to_planes) {
  if (!ctx || N < 0 || S < 0 || F < 0 || (dtype != GSPX_F32 && dtype != GSPX_F64))
    return set_err(GSPX_ERR_INVALID, "gspx_planes_pack_dev: bad argument");
  if (N * S * F == 0) return GSPX_OK;
  if (!src_dev || !dst_dev || src_dev == dst_dev)
    return set_err(GSPX_ERR_INVALID, "gspx_planes_pack_dev: null or aliased buffers");
  if (S >= ((int64_t)1 << 31) || F >= ((int64_t)1 << 31) || N * S * F >= ((int64_t)1 << 40))
    return set_err(GSPX_ERR_INVALID, "gspx_planes_pack_dev: tensor too large");
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t total = N * S * F;
  const unsigned nb = (unsigned)((total + 255) / 256);
  if (dtype == GSPX_F32)
    hipLaunchKernelGGL((k_planes_pack<float>), dim3(nb), dim3(256), 0, ctx->stream, (const float*)src_dev,
                       (float*)dst_dev, N, (int)S, (int)F, to_planes);
  else
    hipLaunchKernelGGL((k_planes_pack<double>), dim3(nb), dim3(256), 0, ctx->stream, (const double*)src_dev,
                       (double*)dst_dev, N, (int)S, (int)F, to_planes);
  HIPCHK(hipGetLastError());
  return GSPX_OK;
}

extern "C" int gspx_bench_copy(gspx_ctx* ctx, int64_t bytes, int iters, double* gbps) {
  if (!ctx || !gbps || bytes < 4096 || iters < 1)
    return set_err(GSPX_ERR_INVALID, "gspx_bench_copy: bad argument");
  HIPCHK(hipSetDevice(ctx->device));
  DevMem a, b;
  CHK(a.alloc((size_t)bytes));
  CHK(b.alloc((size_t)bytes));
  const unsigned ld = 1024;  // floats per row
  const int rows = (int)(bytes / (ld * sizeof(float)));
  hipLaunchKernelGGL((k_fill<float>), dim3(4096), dim3(256), 0, ctx->stream, a.as<float>(),
                     (size_t)rows * ld, 1.0f);
  launch_permute_in<float>(a.as<float>(), ld, b.as<float>(), ld, rows, nullptr, 4, ctx->stream);
  HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
  for (int i = 0; i < iters; ++i)
    launch_permute_in<float>(a.as<float>(), ld, b.as<float>(), ld, rows, nullptr, 4, ctx->stream);
  HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipGetLastError());
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]));
  *gbps = 2.0 * (double)rows * ld * sizeof(float) * iters / (ms * 1e-3) / 1e9;
  return GSPX_OK;
}

// calibration: read-only bandwidth of a `bytes`-sized buffer streamed `passes` times inside one
// launch (cache-level bandwidth as seen by the CUs)
extern "C" int gspx_bench_read(gspx_ctx* ctx, int64_t bytes, int passes, double* gbps) {
  if (!ctx || !gbps || bytes < 4096 || passes < 1)
    return set_err(GSPX_ERR_INVALID, "gspx_bench_read: bad argument");
  HIPCHK(hipSetDevice(ctx->device));
  DevMem a, sink;
  CHK(a.alloc((size_t)bytes));
  CHK(sink.alloc(64));
  const size_t n4 = (size_t)bytes / 16;
  hipLaunchKernelGGL((k_fill<float>), dim3(4096), dim3(256), 0, ctx->stream, a.as<float>(), n4 * 4,
                     1.0f);
  const unsigned nb = (unsigned)std::min<size_t>((n4 + 255) / 256, 4096);
  hipLaunchKernelGGL(k_read_loop, dim3(nb), dim3(256), 0, ctx->stream, (const float4*)a.p, n4, 1,
                     sink.as<float>());
  HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
  hipLaunchKernelGGL(k_read_loop, dim3(nb), dim3(256), 0, ctx->stream, (const float4*)a.p, n4,
                     passes, sink.as<float>());
  HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipGetLastError());
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]));
  *gbps = (double)n4 * 16.0 * passes / (ms * 1e-3) / 1e9;
  return GSPX_OK;
}

// Calibration: the call gspx_cheby_filter_dev(g, lmax, 1, M, coeffs, Nsig, x, y, analysis) would make - the same
// plan, the same K launches over the same buffers with the same flushes, sweeps and cache bits - with the row products
// removed from every wide k_step_tile launch (mode 1; mode 2: the two barriers of a pass too).  y receives numbers
// without meaning.  Times through gspx_last_timing like any filter call.  The mix ceiling of bench.py's roofline.
extern "C" int gspx_bench_step_mix(gspx_graph* g, double lmax, int M, const double* coeffs, int64_t Nsig,
                                   const void* x_dev, void* y_dev, int mode) {
  if (!g || !g->ctx) return set_err(GSPX_ERR_INVALID, "gspx_bench_step_mix: null graph");
  if (mode != 1 && mode != 2) return set_err(GSPX_ERR_INVALID, "gspx_bench_step_mix: mode must be 1 or 2");
  gspx_ctx* ctx = g->ctx;
  const bool wide = Nsig > 0 && Nsig < (1 << 20) && (size_t)Nsig * elt_size(g->dtype) > 128 &&
                    (g->dtype == GSPX_F32 ? tile_geometry<float>(g, ctx->opt, (unsigned)Nsig)
                                          : tile_geometry<double>(g, ctx->opt, (unsigned)Nsig));
  if (!wide)
    return set_err(GSPX_ERR_INVALID, "gspx_bench_step_mix: this call would not run the wide LDS-staged step "
                                     "(gather tiles, rows of more than 128 bytes made of 16-byte pieces)");
  replay_reset(ctx);
  ctx->opt.calib_mix = mode;
  const int rc = gspx_cheby_filter_dev(g, lmax, 1, M, coeffs, Nsig, x_dev, y_dev, GSPX_ANALYSIS, nullptr);
  ctx->opt.calib_mix = 0;
  replay_reset(ctx);
  return rc;
}

// Placement tuning (round 6, profiles/r06_placement.md).  On MI355X the speed of the recurrence on panels beyond the
// Infinity Cache depends on WHICH physical pages back the streamed workspaces: the same call, in one process on one GPU,
// runs anywhere between 0.54 and 0.60 of 8 TB/s as the allocator hands out different pages - the "slow boxes" of rounds
// 2 to 5 were partly boxes whose first allocation drew badly (and partly cards that are slow whatever they draw).
// Relative shifts of the panels inside one allocation change nothing (256 B ... 16 MB, measured), so this is not
// stream-against-stream channel aliasing that a layout rule could avoid; the remedy is to draw several times and keep
// the best.  For `candidates` fresh backings of the two workspaces (the previous ones held meanwhile, so every draw
// gets other pages) the caller's OWN call runs three times (a 7-launch stand-in on scratch panels ranked the candidates
// wrongly: its spread was 2 %, the full call's 8 %); the fastest backing stays in the context, the others are
// released.  out[i]: milliseconds per recurrence launch with candidate i (candidate 0 = the backing the context had,
// or its first own draw; 0 for candidates never drawn because memory ran out), out[candidates] = index kept.
// stride_mb > 0: a pad of that size is allocated and held before every further draw, so that the candidates sample the
// card's memory at that stride - the speed classes come in zones of tens of GB in allocation order (tools/zone_map.py:
// 0 - 60 GB mixed, 60 - 130 GB slow, 130 - 200 GB medium, 200 - 270 GB fast on one card), and a card whose first 12 GB
// are slow may have its fast zone 200 GB in.  The pads are released with the losing candidates.
extern "C" int gspx_ctx_tune_placement(gspx_graph* g, double lmax, int M, const double* coeffs, int64_t Nsig,
                                       const void* x_dev, void* y_dev, int candidates, int64_t stride_mb, double* out) {
  if (!g || !g->ctx || !out) return set_err(GSPX_ERR_INVALID, "gspx_ctx_tune_placement: null argument");
  if (candidates < 1 || candidates > 32) return set_err(GSPX_ERR_INVALID, "gspx_ctx_tune_placement: 1 to 32 candidates");
  if (stride_mb < 0 || stride_mb > ((int64_t)1 << 20))
    return set_err(GSPX_ERR_INVALID, "gspx_ctx_tune_placement: stride_mb out of range");
  CHK(check_filter_args(g, lmax, 1, M, coeffs, Nsig, x_dev, y_dev, GSPX_ANALYSIS));
  for (int i = 0; i <= candidates; ++i) out[i] = 0.0;
  gspx_ctx* ctx = g->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  replay_reset(ctx);
  std::vector<std::unique_ptr<DevMem>> held;  // losing candidates stay allocated until the end: no page is drawn twice
  struct Pads {  // physical memory held without a mapping (hipMemCreate): occupies pages, costs no page-table work
    std::vector<hipMemGenericAllocationHandle_t> h;
    bool hold(size_t bytes, int device) {
      hipMemAllocationProp prop = {};
      prop.type = hipMemAllocationTypePinned;
      prop.location.type = hipMemLocationTypeDevice;
      prop.location.id = device;
      size_t gran = 0;
      if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || !gran) {
        (void)hipGetLastError();
        return false;
      }
      hipMemGenericAllocationHandle_t one;
      if (hipMemCreate(&one, (bytes + gran - 1) / gran * gran, &prop, 0) != hipSuccess) {
        (void)hipGetLastError();
        return false;
      }
      h.push_back(one);
      return true;
    }
    ~Pads() {
      for (auto& one : h) (void)hipMemRelease(one);
    }
  } pads;
  DevMem best_t, best_r;
  double best_ms = 0;
  int best = -1;
  for (int i = 0; i < candidates; ++i) {
    if (i > 0) {  // candidate 0 is what the context has (or draws now); later ones start from empty workspaces
      DevMem t, r;
      t.streamed = ctx->ws_t.streamed;
      r.streamed = ctx->ws_r.streamed;
      ctx->ws_t.swap(t);
      ctx->ws_r.swap(r);
      if (best == i - 1) {  // the previous candidate is the best so far: keep it aside
        best_t.swap(t);
        best_r.swap(r);
      }
      held.emplace_back(new DevMem());
      held.back()->swap(t);  // (what best_t held before, or the loser itself)
      held.emplace_back(new DevMem());
      held.back()->swap(r);
      if (stride_mb > 0) {  // a held pad moves the next draw `stride_mb` further along the allocator's order: the speed
        bool ok = pads.hold((size_t)stride_mb << 20, ctx->device);  // classes come in zones of tens of GB
        if (!ok) {  // (physical memory without a mapping is all a pad needs; a plain allocation if that API refuses)
          held.emplace_back(new DevMem());
          ok = held.back()->alloc((size_t)stride_mb << 20) == GSPX_OK;
          if (!ok) held.pop_back();
        }
        if (!ok) {  // memory exhausted: the search ends here
          ctx->ws_t.swap(best_t);  // (the live workspaces are empty at this point: the best so far goes back in)
          ctx->ws_r.swap(best_r);
          out[candidates] = (double)best;
          replay_reset(ctx);
          return GSPX_OK;
        }
      }
    }
    {  // room for a third panel in the candidate's T workspace, drawn from the same place: the Newton evaluation of the
       // same call (evaluation='auto') keeps three panels there and would otherwise grow the winner by one panel from
       // wherever the allocator stands after the search
      const size_t panel = (size_t)g->N * (size_t)Nsig * elt_size(g->dtype);
      if (panel < ((size_t)1 << 31) && ctx->ws_t.ensure(3 * panel + 256) != GSPX_OK && best >= 0) {
        ctx->ws_t.swap(best_t);  // memory exhausted: the search ends here with the best so far
        ctx->ws_r.swap(best_r);
        out[candidates] = (double)best;
        replay_reset(ctx);
        return gspx_cheby_filter_dev(g, lmax, 1, M, coeffs, Nsig, x_dev, y_dev, GSPX_ANALYSIS, nullptr);
      }
    }
    double ms = 0;
    for (int rep = 0; rep < 3; ++rep) {  // the caller's own call: the first run allocates, the best of the next two counts
      const int rc = gspx_cheby_filter_dev(g, lmax, 1, M, coeffs, Nsig, x_dev, y_dev, GSPX_ANALYSIS, nullptr);
      if (rc != GSPX_OK) {
        if (best >= 0 && best != i) {  // put the best backing found so far in place
          ctx->ws_t.swap(best_t);
          ctx->ws_r.swap(best_r);
        }
        if (rc == GSPX_ERR_OOM && best >= 0) {  // a deep candidate that did not fit: the search ends, not the call
          out[candidates] = (double)best;
          replay_reset(ctx);
          return gspx_cheby_filter_dev(g, lmax, 1, M, coeffs, Nsig, x_dev, y_dev, GSPX_ANALYSIS, nullptr);
        }
        return rc;
      }
      const double t = ctx->timing[1] / std::max(ctx->timing[2], 1.0);
      if (rep == 1 || (rep == 2 && t < ms)) ms = t;
      replay_reset(ctx);
    }
    out[i] = ms;
    if (best < 0 || ms < best_ms) best_ms = ms, best = i;
  }
  if (best != candidates - 1) {  // the live workspaces hold the last candidate: exchange it for the best
    ctx->ws_t.swap(best_t);
    ctx->ws_r.swap(best_r);
  }
  out[candidates] = (double)best;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return GSPX_OK;  // (held and best_t / best_r - now the losers - are released here; y holds the call's result)
}

#include "gspx_calib.hip.h"
#include "gspx_ops.hip.h"
#include "gspx_knn.hip.h"
#include "gspx_setup.hip.h"
#include "gspx_components.hip.h"
#include "gspx_spectral.hip.h"
#include "gspx_lanczos.hip.h"
#include "gspx_learning.hip.h"
