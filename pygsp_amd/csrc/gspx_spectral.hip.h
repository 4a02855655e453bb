// gspx_spectral.hip.h - dense primitives on tall-skinny fp64 panels for the partial Fourier basis
// (pygsp_amd/fourier.py: Chebyshev-filtered subspace iteration).  The polynomial of L is the existing program
// path (gspx_poly_program_dev); these are the three dense pieces around it:
//   C = A^T B                 gspx_panel_gram_dev            (na x nb, to the host)
//   Y = X Q                   gspx_panel_combine_dev         (Q p x q from the host, staged in LDS)
//   r_i = ||LX_i - th_i X_i|| gspx_panel_residual_norms_dev  (one read of both panels)
//   Y = X (strided)           gspx_panel_copy_dev            (a column block out of / into a wider panel)
// Panels are row-major device arrays with an explicit leading dimension (elements), any N >= 0, widths 1..512.
// Gram and combine run on the matrix cores (v_mfma_f64_16x16x4f64).  The Gram kernel and the second pass of every
// reduction are gspx_reduce.hip.h's (launch_panel_gram, sum_parts): no atomics, the same bits on every call.
// After gspx_ops.hip.h (which brings gspx_reduce.hip.h).
#pragma once

namespace gspx {

typedef double spec_d4 __attribute__((ext_vector_type(4)));

// ---- Y = X Q: a workgroup owns 64 rows x 64 columns of Y ---------------------------------------------------
// The contraction runs in chunks of SPEC_KC columns of X: the X chunk (64 rows) and the matching SPEC_KC x 64 tile of
// Q are staged in LDS (33.8 KiB per workgroup, four workgroups per CU within 160 KiB), then wave w forms rows
// 16 w .. 16 w + 15 against the four 16-column sub-tiles: A-operand X[row l % 16][k l / 16], B-operand Q[k l / 16]
// [column l % 16].  Row stride SPEC_KC + 1 (X) and 64 + 4 (Q) doubles keep the fragment reads off one bank.
// Tiles are numbered column tile fastest, so the column tiles of one row block run side by side and share X in L2.
constexpr int SPEC_KC = 32;
constexpr int SPEC_XS = SPEC_KC + 1;
constexpr int SPEC_QS = 64 + 4;
__global__ __launch_bounds__(256) void k_panel_combine(const double* __restrict__ X, int64_t ldx, int p,
                                                       const double* __restrict__ Q, int q, double* __restrict__ Y,
                                                       int64_t ldy, int64_t N) {
  __shared__ double xs[64 * SPEC_XS];
  __shared__ double qs[SPEC_KC * SPEC_QS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kq = lane >> 4, cq = lane & 15;
  const int nct = (q + 63) / 64;
  const int64_t ntiles = (N + 63) / 64 * nct;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile / nct * 64;
    const int c0 = (int)(tile % nct) * 64;
    const int ntc = min(4, (q - c0 + 15) / 16);
    spec_d4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = 0;
    for (int k0 = 0; k0 < p; k0 += SPEC_KC) {
      __syncthreads();  // (the previous chunk's fragments have been read)
      for (int idx = tid; idx < 64 * SPEC_KC; idx += 256) {
        const int r = idx / SPEC_KC, k = idx % SPEC_KC;
        const int64_t row = r0 + r;
        xs[r * SPEC_XS + k] = (row < N && k0 + k < p) ? X[row * ldx + k0 + k] : 0.0;
      }
      for (int idx = tid; idx < SPEC_KC * 64; idx += 256) {
        const int k = idx / 64, c = idx % 64;
        qs[k * SPEC_QS + c] = (k0 + k < p && c0 + c < q) ? Q[(size_t)(k0 + k) * q + c0 + c] : 0.0;
      }
      __syncthreads();
      const int kend = min(SPEC_KC, p - k0);
      for (int kk = 0; kk < kend; kk += 4) {
        const double a = xs[(w * 16 + cq) * SPEC_XS + kk + kq];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < ntc)
            acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, qs[(kk + kq) * SPEC_QS + j * 16 + cq], acc[j], 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t row = r0 + w * 16 + kq + 4 * e;
        const int col = c0 + j * 16 + cq;
        if (row < N && col < q) Y[row * ldy + col] = acc[j][e];
      }
  }
}

// ---- residual norms: partial[b][c] = sum over the block's rows of (LX[i][c] - theta[c] X[i][c])^2 ----------
// grid.x = row blocks, grid.y = 64-column groups; thread t: column 64 y + t % 64, rows 4 b + t / 64 + k * 4 grid.x.
// The four row lanes of a column are summed in a fixed order in LDS.
__global__ __launch_bounds__(256) void k_panel_residual(const double* __restrict__ X, const double* __restrict__ LX,
                                                        int64_t ld, int p, const double* __restrict__ theta, int64_t N,
                                                        double* __restrict__ partial) {
  __shared__ double ws[256];
  const int c = blockIdx.y * 64 + (threadIdx.x & 63);
  const int r0 = threadIdx.x >> 6;
  double s = 0;
  if (c < p) {
    const double th = theta[c];
    const int64_t stride = (int64_t)gridDim.x * 4;
    double s0 = 0, s1 = 0;
    int64_t i = (int64_t)blockIdx.x * 4 + r0;
    for (; i + stride < N; i += 2 * stride) {
      const double d0 = LX[i * ld + c] - th * X[i * ld + c];
      const double d1 = LX[(i + stride) * ld + c] - th * X[(i + stride) * ld + c];
      s0 += d0 * d0;
      s1 += d1 * d1;
    }
    if (i < N) {
      const double d0 = LX[i * ld + c] - th * X[i * ld + c];
      s0 += d0 * d0;
    }
    s = s0 + s1;
  }
  ws[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < 64 && c < p)
    partial[(size_t)blockIdx.x * p + c] = (ws[threadIdx.x] + ws[threadIdx.x + 64]) + (ws[threadIdx.x + 128] + ws[threadIdx.x + 192]);
}

}  // namespace gspx

// ---- host side: argument checks first (they need no context, so no device), then the null context -----------------------------------------------------------------------------------------------
static constexpr int SPEC_MAX_WIDTH = 512;

static bool spec_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + bbytes && pb < pa + abytes;
}

// bytes a panel of N rows spans in memory
static size_t spec_span(int64_t N, int64_t ld, int width) {
  return N > 0 ? ((size_t)(N - 1) * (size_t)ld + (size_t)width) * sizeof(double) : 0;
}

// kernel_ms covers the kernels only: ev[0] is recorded after the small host-to-device copies (Q, theta) and ev[1]
// before the device-to-host copy of the result
extern "C" int gspx_panel_gram_dev(gspx_ctx* ctx, int64_t N, const double* A, int64_t lda, int na, const double* B,
                                   int64_t ldb, int nb, double* C_host, double* kernel_ms) {
  if (N < 0) return set_err(GSPX_ERR_INVALID, "panel_gram: negative number of rows");
  if (na < 1 || na > SPEC_MAX_WIDTH || nb < 1 || nb > SPEC_MAX_WIDTH)
    return set_err(GSPX_ERR_INVALID, "panel_gram: widths must be 1..%d (got %d, %d)", SPEC_MAX_WIDTH, na, nb);
  if (lda < na || ldb < nb) return set_err(GSPX_ERR_INVALID, "panel_gram: leading dimension below the width");
  if (!C_host) return set_err(GSPX_ERR_INVALID, "panel_gram: null output");
  if (N > 0 && (!A || !B)) return set_err(GSPX_ERR_INVALID, "panel_gram: null panel");
  if (!ctx) return set_err(GSPX_ERR_INVALID, "null context");
  replay_reset(ctx);
  if (kernel_ms) *kernel_ms = 0;
  const size_t count = (size_t)na * nb;
  if (N == 0) {
    for (size_t i = 0; i < count; ++i) C_host[i] = 0.0;
    return GSPX_OK;
  }
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  double* csum = nullptr;
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  CHK(launch_panel_gram<double>(ctx, A, lda, na, B, ldb, nb, N, &csum));
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  HIPCHK(hipMemcpyAsync(C_host, csum, count * sizeof(double), hipMemcpyDeviceToHost, st));
  return finish_timed(ctx, kernel_ms);
}

extern "C" int gspx_panel_combine_dev(gspx_ctx* ctx, int64_t N, const double* X, int64_t ldx, int p,
                                      const double* Q_host, int q, double* Y, int64_t ldy, double* kernel_ms) {
  if (N < 0) return set_err(GSPX_ERR_INVALID, "panel_combine: negative number of rows");
  if (p < 1 || p > SPEC_MAX_WIDTH || q < 1 || q > SPEC_MAX_WIDTH)
    return set_err(GSPX_ERR_INVALID, "panel_combine: widths must be 1..%d (got %d, %d)", SPEC_MAX_WIDTH, p, q);
  if (ldx < p || ldy < q) return set_err(GSPX_ERR_INVALID, "panel_combine: leading dimension below the width");
  if (!Q_host) return set_err(GSPX_ERR_INVALID, "panel_combine: null Q");
  if (N > 0 && (!X || !Y)) return set_err(GSPX_ERR_INVALID, "panel_combine: null panel");
  if (N > 0 && spec_overlap(X, spec_span(N, ldx, p), Y, spec_span(N, ldy, q)))
    return set_err(GSPX_ERR_INVALID, "panel_combine: Y must not alias X");
  if (!ctx) return set_err(GSPX_ERR_INVALID, "null context");
  replay_reset(ctx);
  if (kernel_ms) *kernel_ms = 0;
  if (N == 0) return GSPX_OK;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t qbytes = (size_t)p * q * sizeof(double);
  CHK(ctx->ws_spec.ensure(qbytes));
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(ctx->ws_spec.p, Q_host, qbytes, hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  const int64_t ntiles = (N + 63) / 64 * ((q + 63) / 64);
  const unsigned grid = (unsigned)std::min<int64_t>(ntiles, (int64_t)1 << 20);
  hipLaunchKernelGGL(gspx::k_panel_combine, dim3(grid), dim3(256), 0, st, X, ldx, p, ctx->ws_spec.as<double>(), q, Y,
                     ldy, N);
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  return finish_timed(ctx, kernel_ms);
}

extern "C" int gspx_panel_residual_norms_dev(gspx_ctx* ctx, int64_t N, const double* X, const double* LX, int64_t ld,
                                             int p, const double* theta_host, double* out_host, double* kernel_ms) {
  if (N < 0) return set_err(GSPX_ERR_INVALID, "panel_residual_norms: negative number of rows");
  if (p < 1 || p > SPEC_MAX_WIDTH)
    return set_err(GSPX_ERR_INVALID, "panel_residual_norms: width must be 1..%d (got %d)", SPEC_MAX_WIDTH, p);
  if (ld < p) return set_err(GSPX_ERR_INVALID, "panel_residual_norms: leading dimension below the width");
  if (!theta_host || !out_host) return set_err(GSPX_ERR_INVALID, "panel_residual_norms: null theta / output");
  if (N > 0 && (!X || !LX)) return set_err(GSPX_ERR_INVALID, "panel_residual_norms: null panel");
  if (!ctx) return set_err(GSPX_ERR_INVALID, "null context");
  replay_reset(ctx);
  if (kernel_ms) *kernel_ms = 0;
  if (N == 0) {
    for (int i = 0; i < p; ++i) out_host[i] = 0.0;
    return GSPX_OK;
  }
  HIPCHK(hipSetDevice(ctx->device));
  const int nbk = (int)std::min<int64_t>(1024, (N + 63) / 64);
  const size_t nthe = ((size_t)p + 31) / 32 * 32;  // theta, then the partials, then the column sums
  CHK(ctx->ws_spec.ensure((nthe + (size_t)(nbk + 1) * p) * sizeof(double)));
  double* th = ctx->ws_spec.as<double>();
  double* partial = th + nthe;
  double* sums = partial + (size_t)nbk * p;
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(th, theta_host, (size_t)p * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL(gspx::k_panel_residual, dim3(nbk, (p + 63) / 64), dim3(256), 0, st, X, LX, ld, p, th, N, partial);
  sum_parts(partial, nbk, p, sums, st);
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  HIPCHK(hipMemcpyAsync(out_host, sums, (size_t)p * sizeof(double), hipMemcpyDeviceToHost, st));
  CHK(finish_timed(ctx, kernel_ms));
  for (int i = 0; i < p; ++i) out_host[i] = std::sqrt(out_host[i]);
  return GSPX_OK;
}

extern "C" int gspx_panel_copy_dev(gspx_ctx* ctx, int64_t N, const double* X, int64_t ldx, int w, double* Y, int64_t ldy,
                                   double* kernel_ms) {
  if (N < 0) return set_err(GSPX_ERR_INVALID, "panel_copy: negative number of rows");
  if (w < 1 || w > SPEC_MAX_WIDTH)
    return set_err(GSPX_ERR_INVALID, "panel_copy: width must be 1..%d (got %d)", SPEC_MAX_WIDTH, w);
  if (ldx < w || ldy < w) return set_err(GSPX_ERR_INVALID, "panel_copy: leading dimension below the width");
  if (N > 0 && (!X || !Y)) return set_err(GSPX_ERR_INVALID, "panel_copy: null panel");
  if (N > 0 && spec_overlap(X, spec_span(N, ldx, w), Y, spec_span(N, ldy, w)))
    return set_err(GSPX_ERR_INVALID, "panel_copy: Y must not alias X");
  if (!ctx) return set_err(GSPX_ERR_INVALID, "null context");
  replay_reset(ctx);
  if (kernel_ms) *kernel_ms = 0;
  if (N == 0) return GSPX_OK;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  HIPCHK(hipMemcpy2DAsync(Y, (size_t)ldy * sizeof(double), X, (size_t)ldx * sizeof(double), (size_t)w * sizeof(double),
                          (size_t)N, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  return finish_timed(ctx, kernel_ms);
}
