// gspx_reduce.hip.h - the reductions every operator next to the Chebyshev path shares: one in-workgroup column sum,
// one in-workgroup total, one second pass over workgroup partials, one Gram kernel on the matrix cores.  Every reduction is per
// workgroup (or per wave) into partials, then a fixed-order second pass: no atomics, the same bits on every call -
// for all callers, because there is one definition of each piece.  gfx950 only.
// Included by gspx_ops.hip.h (the host helpers use gspx_ctx, DevMem, HIPCHK, CHK).
//
// The shared thread map of the column kernels (k_coldot_partial, k_cg_xr_dot, k_lz_three, k_lz_dots, k_lz_update):
// a 256-thread workgroup over a row-major N x ld panel, ldp = ld rounded up to a power of two (col_pow2, <= 256),
// rstep = 256 / ldp.  Thread t takes column t % ldp and rows blockIdx.x * rstep + t / ldp + s * gridDim.x * rstep,
// s = 0, 1, ...  Lanes of one row read neighbouring elements; for ld = 1 neighbouring rows.
#pragma once

namespace gspx {

// ---- in-workgroup column sum ------------------------------------------------------------------------------------
// One value per thread, summed over the rstep row lanes of each column in a fixed order in LDS (ws: 256 doubles):
// out[c] = sum over k = 0..rstep-1 of the value of thread k * ldp + c, for c < ld.  All 256 threads call it; the
// closing barrier lets the next call reuse ws.
__device__ inline void block_colsum(double* ws, double v, int ld, int ldp, int rstep, double* out) {
  ws[threadIdx.x] = v;
  __syncthreads();
  if ((int)threadIdx.x < ld) {
    double s = 0;
    for (int k = 0; k < rstep; ++k) s += ws[k * ldp + threadIdx.x];
    out[threadIdx.x] = s;
  }
  __syncthreads();
}

// ---- in-workgroup totals of Q per-thread sums --------------------------------------------------------------------
// A 256-thread workgroup: wave shuffles, then the four waves in the order (w0 + w1) + (w2 + w3); thread q < Q writes
// out[q * stride].  All 256 threads call it, once per kernel (ws is not guarded for a second call).
template <int Q>
__device__ inline void block_sums(const double (&s)[Q], double* out, size_t stride) {
  __shared__ double ws[Q][4];
  double v[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    v[q] = s[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_down(v[q], off);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < Q; ++q) ws[q][threadIdx.x >> 6] = v[q];
  }
  __syncthreads();
  if ((int)threadIdx.x < Q) {
    const int q = threadIdx.x;
    out[(size_t)q * stride] = (ws[q][0] + ws[q][1]) + (ws[q][2] + ws[q][3]);
  }
}

// ---- second pass: out[c] = sum over b of partial[b * count + c] (sum_parts below picks the kernel) ---------------
// one 64-lane wave per entry, fixed summation tree: the narrow sums (fewer than 4096 entries)
__global__ __launch_bounds__(64) void k_colsum(const double* __restrict__ partial, int nb, int ld,
                                               double* __restrict__ out) {
  const int c = blockIdx.x;
  if (c >= ld) return;
  double s = 0;
  for (int b = threadIdx.x; b < nb; b += 64) s += partial[(size_t)b * ld + c];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
  if (threadIdx.x == 0) out[c] = s;
}
// one thread per entry, b in order, so neighbouring threads read neighbouring entries: the wide sums
__global__ __launch_bounds__(256) void k_panel_sum_parts(const double* __restrict__ partial, int nparts, int64_t count,
                                                         double* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= count) return;
  double s = 0;
  int b = 0;
  for (; b + 4 <= nparts; b += 4) {
    const double v0 = partial[(size_t)b * count + c], v1 = partial[(size_t)(b + 1) * count + c];
    const double v2 = partial[(size_t)(b + 2) * count + c], v3 = partial[(size_t)(b + 3) * count + c];
    s += v0;
    s += v1;
    s += v2;
    s += v3;
  }
  for (; b < nparts; ++b) s += partial[(size_t)b * count + c];
  out[c] = s;
}

// ---- C = A^T B: per wave a 64 x 64 tile of C over a slice of rows ------------------------------------------
// grid.x = tile (ta * ntb + tb), grid.y = row chunk of `rpc` rows (a multiple of 16).  Wave w of the workgroup takes
// the 4-row groups w, w + 4, ... of its chunk.  v_mfma_f64_16x16x4f64 with A-operand = A^T (lane l: column l % 16 of
// the tile, row l / 16 of the group) and B-operand = B (the same lane map): coalesced row segments, no LDS.  fp32
// panels are converted on load: the sums are double either way.
// D layout of the f64 instruction: lane l holds rows (l / 16) + 4 e, column l % 16.
// ROWSCALE: C = A^T diag(rs) B, the A element scaled by rs[row] on load (rs: N doubles); without it rs is not read
// and the arithmetic is the unscaled kernel's.
// The four waves' tiles are summed in LDS in a fixed order (((w0 + w1) + w2) + w3) and wave 0 writes the workgroup's
// partial[chunk * na * nb + a * nb + c]: every entry of every chunk's slot is written (zeros where the slice has no
// rows), so the second pass needs no initialisation.
template <typename T, bool ROWSCALE>
__global__ __launch_bounds__(256) void k_panel_gram(const T* __restrict__ A, int64_t lda, int na,
                                                    const T* __restrict__ B, int64_t ldb, int nb, int64_t N,
                                                    int64_t rpc, const double* __restrict__ rs,
                                                    double* __restrict__ partial) {
  typedef double d4 __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int kq = lane >> 4, cq = lane & 15;
  const int ntb = (nb + 63) / 64;
  const int a0 = (int)(blockIdx.x / ntb) * 64, b0 = (int)(blockIdx.x % ntb) * 64;
  const int nta = min(4, (na - a0 + 15) / 16), ntc = min(4, (nb - b0 + 15) / 16);  // 16-wide sub-tiles in use
  const int64_t r_begin = (int64_t)blockIdx.y * rpc;
  const int64_t r_end = min(N, r_begin + rpc);
  d4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0;
  for (int64_t r = r_begin + 4 * w; r < r_end; r += 16) {
    const int64_t row = r + kq;
    const bool rok = row < r_end;
    double xa[4], yb[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int ca = a0 + t * 16 + cq, cb = b0 + t * 16 + cq;
      xa[t] = (rok && ca < na) ? (double)A[row * lda + ca] : 0.0;
      yb[t] = (rok && cb < nb) ? (double)B[row * ldb + cb] : 0.0;
    }
    if constexpr (ROWSCALE) {
      const double sc = rok ? rs[row] : 0.0;
#pragma unroll
      for (int t = 0; t < 4; ++t) xa[t] *= sc;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nta)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < ntc) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[i], yb[j], acc[i][j], 0, 0, 0);
  }
  __shared__ double red[16 * 4 * 64];  // one wave's 4 x 4 tiles, lane-major (no bank conflicts)
  for (int src = 1; src < 4; ++src) {
    if (w == src)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) red[((i * 4 + j) * 4 + e) * 64 + lane] = acc[i][j][e];
    __syncthreads();
    if (w == 0)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][j][e] += red[((i * 4 + j) * 4 + e) * 64 + lane];
    __syncthreads();
  }
  if (w != 0) return;
  double* out = partial + (size_t)blockIdx.y * (size_t)na * nb;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int aa = a0 + i * 16 + kq + 4 * e, cc = b0 + j * 16 + cq;
        if (aa < na && cc < nb) out[(size_t)aa * nb + cc] = acc[i][j][e];
      }
}

}  // namespace gspx

// ---- host side --------------------------------------------------------------------------------------------------
// ldp of the shared thread map: the column count rounded up to a power of two
static int col_pow2(int ld) {
  int p = 1;
  while (p < ld) p <<= 1;
  return p;
}

// sum of `nparts` partial slabs of `count` entries, in a fixed order
static void sum_parts(const double* partial, int nparts, int64_t count, double* out, hipStream_t st) {
  if (count >= 4096)
    hipLaunchKernelGGL(gspx::k_panel_sum_parts, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, partial,
                       nparts, count, out);
  else
    hipLaunchKernelGGL(gspx::k_colsum, dim3((unsigned)count), dim3(64), 0, st, partial, nparts, (int)count, out);
}

// C = A^T B (na x nb, row-major doubles) of two N-row device panels, N > 0, left on the device in ctx->ws_spec
// (*out_dev, valid until the next use of that workspace): records no events, copies nothing to the host.
// rs (N doubles on the device, or null): C = A^T diag(rs) B.
template <typename T>
static int launch_panel_gram(gspx_ctx* ctx, const T* A, int64_t lda, int na, const T* B, int64_t ldb, int nb, int64_t N,
                             double** out_dev, const double* rs = nullptr) {
  const size_t count = (size_t)na * nb;
  const int ntiles = ((na + 63) / 64) * ((nb + 63) / 64);
  // about eight workgroups per CU in all; at least 16 rows per wave; at most 256 MiB of partials
  int64_t nchunk = std::max<int64_t>(1, ((int64_t)8 * ctx->cu_count + ntiles - 1) / ntiles);
  nchunk = std::min<int64_t>(nchunk, (N + 63) / 64);
  nchunk = std::min<int64_t>(nchunk, std::max<int64_t>(1, ((int64_t)256 << 20) / (int64_t)(count * sizeof(double))));
  nchunk = std::min<int64_t>(nchunk, 65535);
  const int64_t rpc = ((N + nchunk - 1) / nchunk + 15) / 16 * 16;
  nchunk = (N + rpc - 1) / rpc;
  const size_t nparts = (size_t)nchunk;
  CHK(ctx->ws_spec.ensure((nparts + 1) * count * sizeof(double)));
  double* partial = ctx->ws_spec.as<double>();
  *out_dev = partial + nparts * count;
  if (rs)
    hipLaunchKernelGGL((gspx::k_panel_gram<T, true>), dim3(ntiles, (unsigned)nchunk), dim3(256), 0, ctx->stream, A, lda,
                       na, B, ldb, nb, N, rpc, rs, partial);
  else
    hipLaunchKernelGGL((gspx::k_panel_gram<T, false>), dim3(ntiles, (unsigned)nchunk), dim3(256), 0, ctx->stream, A, lda,
                       na, B, ldb, nb, N, rpc, rs, partial);
  sum_parts(partial, (int)nparts, (int64_t)count, *out_dev, ctx->stream);
  return GSPX_OK;
}
