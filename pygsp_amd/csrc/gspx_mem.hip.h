// gspx_mem.hip.h - memory owners of libgspx: DevMem (device allocations; the streamed workspaces assembled from
// scrambled 2 MB chunks, and the rules under which their address ranges are retired), PinMem (pinned host memory),
// CopyStage (the pinned chunks, stream and events of a staged gspx_buf_upload / gspx_buf_download) and HostPipe (the
// staging state of the pipelined host-pointer calls, gspx_hostpipe.hip.h).  A context owns one of each of the last two,
// created on first use.  Needs only gspx.hip's set_err / CHK / HIPCHK.
#pragma once

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
