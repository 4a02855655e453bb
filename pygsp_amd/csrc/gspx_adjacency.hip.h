// gspx_adjacency.hip.h - what every device builder of a weight matrix shares: the int32 exclusive scan that turns row
// lengths into row offsets (and hands back their total), the handle gspx_knn such a builder leaves behind with its
// destroy / info / download entry points, and the frame of a builder: adjacency_open, adjacency_offsets,
// adjacency_close ("The adjacency frame").  After gspx_ctx.hip.h; needs nothing else.  The scan also serves
// gspx_graph / gspx_ops / gspx_setup / gspx_components, which build no handle.
#pragma once

namespace gspx {

// ---------------------------------------------------------------------------------------------
// exclusive scan of int32 (three small kernels; tile = 1024 elements)
// ---------------------------------------------------------------------------------------------
#define GSPX_SCAN_TILE 1024
// (in and out may be the same array - radix_argsort scans its histogram in place: every thread reads its four
// inputs before it writes its four outputs, and no thread touches another's - so neither is __restrict__)
__global__ __launch_bounds__(256) void k_scan_tiles(const int* in, int n, int* out, int* __restrict__ tile_sums) {
  __shared__ int wsum[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int base = blockIdx.x * GSPX_SCAN_TILE + t * 4;
  int v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = (base + k < n) ? in[base + k] : 0;
  const int mine = v[0] + v[1] + v[2] + v[3];
  int incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off);
    if (lane >= off) incl += o;
  }
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  int wbase = 0;
  for (int k = 0; k < wv; ++k) wbase += wsum[k];
  int run = wbase + incl - mine;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (base + k < n) out[base + k] = run;
    run += v[k];
  }
  if (t == 255) tile_sums[blockIdx.x] = wbase + incl;
}

__global__ __launch_bounds__(256) void k_scan_sums(int* tile_sums, int ntiles) {
  // single workgroup: serial over 256-element strips with a carry
  __shared__ int wsum[4];
  __shared__ int carry_s;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < ntiles; base += 256) {
    const int i = base + t;
    const int mine = i < ntiles ? tile_sums[i] : 0;
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off);
      if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int wbase = carry_s;
    for (int k = 0; k < wv; ++k) wbase += wsum[k];
    if (i < ntiles) tile_sums[i] = wbase + incl - mine;
    __syncthreads();
    if (t == 255) carry_s = wbase + incl;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_scan_add(int* __restrict__ out, int n,
                                                  const int* __restrict__ tile_sums) {
  const int add = tile_sums[blockIdx.x];
  const int base = blockIdx.x * GSPX_SCAN_TILE + threadIdx.x * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (base + k < n) out[base + k] += add;
}

}  // namespace gspx

// ------------------------------------------------------------------------------------------------
// device exclusive scan of n int32 (in-place safe: out may equal in).  Waits for the stream.  With total, *total =
// out[n - 1], the sum of in[0 .. n-2]: callers pass n = rows + 1 lengths with a zero in the last slot, so that is the
// sum of all of them (0 when n <= 0).
// ------------------------------------------------------------------------------------------------
static int scan_exclusive(gspx_ctx* ctx, const int* in, int* out, int n, int* total = nullptr) {
  if (total) *total = 0;
  if (n <= 0) return GSPX_OK;
  const int ntiles = (n + GSPX_SCAN_TILE - 1) / GSPX_SCAN_TILE;
  DevMem sums;
  CHK(sums.alloc((size_t)ntiles * sizeof(int)));
  hipLaunchKernelGGL(k_scan_tiles, dim3(ntiles), dim3(256), 0, ctx->stream, in, n, out,
                     sums.as<int>());
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(256), 0, ctx->stream, sums.as<int>(), ntiles);
  hipLaunchKernelGGL(k_scan_add, dim3(ntiles), dim3(256), 0, ctx->stream, out, n, sums.as<int>());
  HIPCHK(hipGetLastError());
  if (total) HIPCHK(hipMemcpyAsync(total, out + n - 1, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return GSPX_OK;
}

// ------------------------------------------------------------------------------------------------
// the adjacency handle: the weight matrix (N x N, CSR: rowptr / col / val, nnz entries) any device builder leaves on
// the device - neighbour graphs, the block-model sampler, line graphs, Kron reduction, learned graphs, coarse graphs.
// Only the neighbour builders fill nn, dist, d, k, sigma and search_stats.  (The name is the public typedef of
// include/gspx_ext.h and older than the other builders.)
// ------------------------------------------------------------------------------------------------
struct gspx_knn {
  gspx_ctx* ctx = nullptr;
  int64_t N = 0;
  int d = 0, k = 0;
  double sigma = 0.0;
  int64_t nnz = 0;
  double build_ms = 0.0;
  double search_stats[4] = {0, 0, 0, 0};  // brute-force search (d > 3): sample, capacity, mean candidates, exact scans
  DevMem nn, dist, rowptr, col, val;
};

extern "C" int gspx_knn_destroy(gspx_knn* h) {
  if (!h) return GSPX_OK;
  (void)hipSetDevice(h->ctx->device);
  delete h;
  return GSPX_OK;
}

extern "C" int gspx_knn_info(gspx_knn* h, int64_t* nnz, double* sigma, double* build_ms) {
  if (!h) return set_err(GSPX_ERR_INVALID, "null handle");
  if (nnz) *nnz = h->nnz;
  if (sigma) *sigma = h->sigma;
  if (build_ms) *build_ms = h->build_ms;
  return GSPX_OK;
}

extern "C" int gspx_knn_download_w(gspx_knn* h, int32_t* indptr, int32_t* indices, double* data) {
  if (!h || !indptr) return set_err(GSPX_ERR_INVALID, "null argument");
  if (h->nnz > 0 && (!indices || !data)) return set_err(GSPX_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->ctx->device));
  HIPCHK(hipMemcpy(indptr, h->rowptr.p, ((size_t)h->N + 1) * sizeof(int), hipMemcpyDeviceToHost));
  if (h->nnz > 0) {
    HIPCHK(hipMemcpy(indices, h->col.p, (size_t)h->nnz * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(data, h->val.p, (size_t)h->nnz * sizeof(double), hipMemcpyDeviceToHost));
  }
  return GSPX_OK;
}

// ---- the frame of a builder --------------------------------------------------------------------------------------
// A fresh handle of N rows with rowptr allocated and cleared on the stream; a builder that fails drops it.
static int adjacency_open(gspx_ctx* ctx, int64_t N, std::unique_ptr<gspx_knn>& h) {
  h.reset(new gspx_knn());
  h->ctx = ctx;
  h->N = N;
  CHK(h->rowptr.alloc(((size_t)N + 1) * sizeof(int)));
  HIPCHK(hipMemsetAsync(h->rowptr.p, 0, ((size_t)N + 1) * sizeof(int), ctx->stream));
  return GSPX_OK;
}

// N + 1 row lengths on the device (len; h->rowptr itself when the builder counted in place) -> offsets in h->rowptr,
// their total in h->nnz, col and val allocated for it (DevMem::alloc covers zero).  Waits for the stream.
static int adjacency_offsets(gspx_knn* h, const int* len, const char* who) {
  int total = 0;
  CHK(scan_exclusive(h->ctx, len, h->rowptr.as<int>(), (int)h->N + 1, &total));
  if (total < 0) return set_err(GSPX_ERR_INVALID, "%s: more than 2^31 entries", who);
  h->nnz = total;
  CHK(h->col.alloc((size_t)total * sizeof(int)));
  CHK(h->val.alloc((size_t)total * sizeof(double)));
  return GSPX_OK;
}

static void adjacency_close(std::unique_ptr<gspx_knn>& h, std::chrono::steady_clock::time_point t0, gspx_knn** out) {
  h->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out = h.release();
}
