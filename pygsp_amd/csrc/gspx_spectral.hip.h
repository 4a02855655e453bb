// gspx_spectral.hip.h - dense primitives on fp64 panels for the Fourier basis: the partial basis
// (pygsp_amd/fourier.py: Chebyshev-filtered subspace iteration) and exact Fourier filtering against a full one
// (filters.filter_signals(method='exact'), Graph.gft / igft of device arrays, filters.Modulation).  The polynomial of
// L is the existing program path (gspx_poly_program_dev); these are the dense pieces around it:
//   C = A^T B                       gspx_panel_gram_dev            (na x nb <= 512, to the host)
//   C = alpha A^T diag(r) B         gspx_panel_gram_to_dev         (any na x nb, to a device buffer; r optional)
//   Y = X Q                         gspx_panel_combine_dev         (Q p x q <= 512 from the host, staged in LDS)
//   Y_g = U (diag(h_g) S)           gspx_spectral_apply_dev        (S, h on the device; analysis, synthesis or plain;
//                                                                   any contraction length, any width)
//   r_i = ||LX_i - th_i X_i||       gspx_panel_residual_norms_dev  (one read of both panels)
//   Y = X (strided)                 gspx_panel_copy_dev            (a column block out of / into a wider panel)
// Panels are row-major device arrays with an explicit leading dimension (elements), any N >= 0.
// Gram and the X Q products run on the matrix cores (v_mfma_f64_16x16x4f64); combine and spectral apply are one
// kernel (k_spectral_apply) that differs only in how the Q tile is staged.  The Gram kernel and the second pass of every
// reduction are gspx_reduce.hip.h's (launch_panel_gram, sum_parts): no atomics, the same bits on every call.
// After gspx_ops.hip.h (which brings gspx_reduce.hip.h).
#pragma once

namespace gspx {

typedef double spec_d4 __attribute__((ext_vector_type(4)));

// ---- Y = X Q: a workgroup owns 64 rows x 64 columns of Y ---------------------------------------------------
// The contraction runs in chunks of SPEC_KC columns of X, in order, for any length p: the X chunk (64 rows) and the
// matching SPEC_KC x 64 tile of Q are staged in LDS (33.8 KiB per workgroup, four workgroups per CU within 160 KiB),
// then wave w forms rows 16 w .. 16 w + 15 against the four 16-column sub-tiles: A-operand X[row l % 16][k l / 16],
// B-operand Q[k l / 16][column l % 16].  Row stride SPEC_KC + 1 (X) and 64 + 4 (Q) doubles keep the fragment reads off
// one bank.  STAGE says what the Q tile is, formed while it is staged and never written to memory:
//   SPEC_PLAIN      Q[k][c]                                 (one plane: combine, igft)
//   SPEC_ANALYSIS   H[g][k] Q[k][c] for output plane g      (nf output planes N x q, plane stride N ldy)
//   SPEC_SYNTHESIS  sum_f H[f][k] Q_f[k][c], f in order     (nf input planes p x q, plane stride p ldq; one output)
// H is nf x p, row-major.  Tiles are numbered column tile fastest, then output plane, then row block, so the tiles
// that read one row block of X run side by side and share it in L2.
constexpr int SPEC_KC = 32;
constexpr int SPEC_XS = SPEC_KC + 1;
constexpr int SPEC_QS = 64 + 4;
enum { SPEC_PLAIN = 0, SPEC_ANALYSIS = 1, SPEC_SYNTHESIS = 2 };
template <int STAGE>
__global__ __launch_bounds__(256) void k_spectral_apply(const double* __restrict__ X, int64_t ldx, int p,
                                                        const double* __restrict__ Q, int64_t ldq, int q,
                                                        const double* __restrict__ H, int nf, double* __restrict__ Y,
                                                        int64_t ldy, int64_t N) {
  __shared__ double xs[64 * SPEC_XS];
  __shared__ double qs[SPEC_KC * SPEC_QS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kq = lane >> 4, cq = lane & 15;
  const int nct = (q + 63) / 64;
  const int nplanes = STAGE == SPEC_ANALYSIS ? nf : 1;
  const int64_t ntiles = (N + 63) / 64 * nplanes * nct;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile / ((int64_t)nct * nplanes) * 64;
    const int g = (int)(tile / nct % nplanes);
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
        double v = 0.0;
        if (k0 + k < p && c0 + c < q) {
          const size_t at = (size_t)(k0 + k) * ldq + c0 + c;
          if constexpr (STAGE == SPEC_PLAIN) v = Q[at];
          if constexpr (STAGE == SPEC_ANALYSIS) v = H[(size_t)g * p + k0 + k] * Q[at];
          if constexpr (STAGE == SPEC_SYNTHESIS)
            for (int f = 0; f < nf; ++f) v += H[(size_t)f * p + k0 + k] * Q[(size_t)f * p * ldq + at];
        }
        qs[k * SPEC_QS + c] = v;
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
    double* Yg = Y + (size_t)g * (size_t)N * ldy;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t row = r0 + w * 16 + kq + 4 * e;
        const int col = c0 + j * 16 + cq;
        if (row < N && col < q) Yg[row * ldy + col] = acc[j][e];
      }
  }
}

// ---- C[a][c] = alpha * sum[a][c]: the Gram's summed tile into the caller's (strided) device matrix -----------
__global__ __launch_bounds__(256) void k_gram_store(const double* __restrict__ sum, int na, int nb, double alpha,
                                                    double* __restrict__ C, int64_t ldc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)na * nb) return;
  C[i / nb * ldc + i % nb] = alpha * sum[i];
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
  hipLaunchKernelGGL(gspx::k_spectral_apply<gspx::SPEC_PLAIN>, dim3(grid), dim3(256), 0, st, X, ldx, p,
                     ctx->ws_spec.as<double>(), (int64_t)q, q, (const double*)nullptr, 1, Y, ldy, N);
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  return finish_timed(ctx, kernel_ms);
}

// C (na x nb, leading dimension ldc, DEVICE) = alpha A^T diag(r) B for any widths: the output is formed in blocks of at
// most SPEC_GRAM_BLOCK x SPEC_GRAM_BLOCK entries (32 MiB, so that launch_panel_gram keeps several row chunks within its
// 256 MiB of partials), each block summed by sum_parts and scaled into C by k_gram_store.  N == 0 or an empty width:
// nothing is launched and C is left as it is.  (A later block may grow the workspace after earlier blocks were written;
// if that allocation fails the call can be repeated as it is: the inputs are untouched and every entry of C is rewritten.)
static constexpr int SPEC_GRAM_BLOCK = 2048;
extern "C" int gspx_panel_gram_to_dev(gspx_ctx* ctx, int64_t N, const double* A, int64_t lda, int na, const double* B,
                                      int64_t ldb, int nb, const double* rowscale, double alpha, double* C, int64_t ldc,
                                      double* kernel_ms) {
  if (N < 0) return set_err(GSPX_ERR_INVALID, "panel_gram_to: negative number of rows");
  if (na < 0 || nb < 0) return set_err(GSPX_ERR_INVALID, "panel_gram_to: negative width (got %d, %d)", na, nb);
  if (lda < na || ldb < nb || ldc < nb)
    return set_err(GSPX_ERR_INVALID, "panel_gram_to: leading dimension below the width");
  const bool work = N > 0 && na > 0 && nb > 0;
  if (work && (!A || !B || !C)) return set_err(GSPX_ERR_INVALID, "panel_gram_to: null panel");
  if (work) {
    const size_t cbytes = spec_span(na, ldc, nb);
    if (spec_overlap(C, cbytes, A, spec_span(N, lda, na)) || spec_overlap(C, cbytes, B, spec_span(N, ldb, nb)) ||
        (rowscale && spec_overlap(C, cbytes, rowscale, (size_t)N * sizeof(double))))
      return set_err(GSPX_ERR_INVALID, "panel_gram_to: C must not alias A, B or the row scale");
  }
  if (!ctx) return set_err(GSPX_ERR_INVALID, "null context");
  replay_reset(ctx);
  if (kernel_ms) *kernel_ms = 0;
  if (!work) return GSPX_OK;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  for (int a0 = 0; a0 < na; a0 += SPEC_GRAM_BLOCK)
    for (int b0 = 0; b0 < nb; b0 += SPEC_GRAM_BLOCK) {
      const int aw = std::min(SPEC_GRAM_BLOCK, na - a0), bw = std::min(SPEC_GRAM_BLOCK, nb - b0);
      double* csum = nullptr;
      CHK(launch_panel_gram<double>(ctx, A + a0, lda, aw, B + b0, ldb, bw, N, &csum, rowscale));
      const int64_t count = (int64_t)aw * bw;
      hipLaunchKernelGGL(gspx::k_gram_store, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, csum, aw, bw, alpha,
                         C + (size_t)a0 * ldc + b0, ldc);
    }
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  return finish_timed(ctx, kernel_ms);
}

// Y_g = U Q_g with Q_g formed from S (and H) while it is staged (k_spectral_apply): mode 0 plain (Y = U S, H unused,
// nf = 1), 1 analysis (S one n x w panel, nf output planes), 2 synthesis (nf panels of S, plane stride n lds, one
// output plane).  N == 0 or w == 0: nothing is launched.
extern "C" int gspx_spectral_apply_dev(gspx_ctx* ctx, int64_t N, const double* U, int64_t ldu, int n, const double* S,
                                       int64_t lds, int w, int mode, int nf, const double* H, double* Y, int64_t ldy,
                                       double* kernel_ms) {
  if (N < 0) return set_err(GSPX_ERR_INVALID, "spectral_apply: negative number of rows");
  if (n < 1) return set_err(GSPX_ERR_INVALID, "spectral_apply: the contraction length must be at least 1 (got %d)", n);
  if (w < 0) return set_err(GSPX_ERR_INVALID, "spectral_apply: negative width (got %d)", w);
  if (mode < gspx::SPEC_PLAIN || mode > gspx::SPEC_SYNTHESIS)
    return set_err(GSPX_ERR_INVALID, "spectral_apply: mode must be 0 (plain), 1 (analysis) or 2 (synthesis), got %d", mode);
  if (nf < 1 || (mode == gspx::SPEC_PLAIN && nf != 1))
    return set_err(GSPX_ERR_INVALID, "spectral_apply: the number of filters must be at least 1 (1 in plain mode), got %d", nf);
  if (ldu < n || lds < w || ldy < w) return set_err(GSPX_ERR_INVALID, "spectral_apply: leading dimension below the width");
  const bool work = N > 0 && w > 0;
  if (work && (!U || !S || !Y || (mode != gspx::SPEC_PLAIN && !H)))
    return set_err(GSPX_ERR_INVALID, "spectral_apply: null panel");
  if (work) {
    const int planes_in = mode == gspx::SPEC_SYNTHESIS ? nf : 1, planes_out = mode == gspx::SPEC_ANALYSIS ? nf : 1;
    const size_t ybytes = (size_t)(planes_out - 1) * (size_t)N * ldy * sizeof(double) + spec_span(N, ldy, w);
    const size_t sbytes = (size_t)(planes_in - 1) * (size_t)n * lds * sizeof(double) + spec_span(n, lds, w);
    if (spec_overlap(Y, ybytes, U, spec_span(N, ldu, n)) || spec_overlap(Y, ybytes, S, sbytes) ||
        (H && spec_overlap(Y, ybytes, H, (size_t)nf * n * sizeof(double))))
      return set_err(GSPX_ERR_INVALID, "spectral_apply: Y must not alias U, the coefficients or the multipliers");
  }
  if (!ctx) return set_err(GSPX_ERR_INVALID, "null context");
  replay_reset(ctx);
  if (kernel_ms) *kernel_ms = 0;
  if (!work) return GSPX_OK;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  const int64_t ntiles = (N + 63) / 64 * ((w + 63) / 64) * (mode == gspx::SPEC_ANALYSIS ? nf : 1);
  const dim3 grid((unsigned)std::min<int64_t>(ntiles, (int64_t)1 << 20)), block(256);
  if (mode == gspx::SPEC_PLAIN)
    hipLaunchKernelGGL(gspx::k_spectral_apply<gspx::SPEC_PLAIN>, grid, block, 0, st, U, ldu, n, S, lds, w, H, nf, Y, ldy, N);
  else if (mode == gspx::SPEC_ANALYSIS)
    hipLaunchKernelGGL(gspx::k_spectral_apply<gspx::SPEC_ANALYSIS>, grid, block, 0, st, U, ldu, n, S, lds, w, H, nf, Y, ldy,
                       N);
  else
    hipLaunchKernelGGL(gspx::k_spectral_apply<gspx::SPEC_SYNTHESIS>, grid, block, 0, st, U, ldu, n, S, lds, w, H, nf, Y,
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
