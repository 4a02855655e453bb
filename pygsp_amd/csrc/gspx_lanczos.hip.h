// gspx_lanczos.hip.h - Lanczos filtering on the graph Laplacian (pygsp_amd/lanczos.py; the reference's
// approximations.lanczos / lanczos_op): one Krylov basis per signal column, full reorthogonalisation against it.
//   gspx_lanczos_krylov_dev   the Krylov stack V (order fp64 panels of N x Nsig, internal vertex order), the
//                             tridiagonal H (alpha, beta), V^T x and the Krylov dimension of every column
//   gspx_lanczos_combine_dev  y_f = sum_j W[f][j] V_j for all Nf filters, one pass over the stack, written in the
//                             caller's vertex order
// The host eigen-step (eigh of H, f.evaluate at the Ritz values) sits between the two calls.
//
// Step k of a column (r = the unnormalised residual, beta_k = ||r||; r = x, beta_0 = ||x|| at k = 0):
//   W = L r                                     spmm_internal (the engine's product, internal order)
//   q_k = r / beta_k,  w = W / beta_k - beta_k q_{k-1},  alpha_k = q_k . w              k_lz_three
//   h_j = q_j . (w - alpha_k q_k), j = 0..k                                              k_lz_dots
//   r = w - alpha_k q_k - sum_j h_j q_j,  ||r||^2                                        k_lz_update
//   beta_{k+1} = ||r||; the column stops when beta_{k+1} <= breakdown                    k_lz_next
// that is the reference's three-term step followed by ONE classical Gram-Schmidt pass against q_0..q_k (DESIGN.md,
// "Lanczos filtering": why one pass is enough after the three-term subtraction).  alpha, beta, the dots and the
// per-column active flags stay on the device: the loop does not synchronise with the host until it ends.
// Every reduction is per workgroup into partials (block_colsum), then a fixed-order second pass (sum_parts), both
// from gspx_reduce.hip.h: no atomics, the same bits on every call.  After gspx_poly.hip.h (and
// gspx_ops.hip.h, which brings gspx_reduce.hip.h).
#pragma once

namespace gspx {

// Column kernels use the shared thread map of gspx_reduce.hip.h (column t % ldp, row lanes t / ldp).
constexpr int LZ_JB = 16;  // stack panels per workgroup of the dot kernel
constexpr int LZ_MAX_WIDTH = 256;

struct LzScalars {  // device resident
  double* alpha;    // [order][ld]
  double* beta;     // [order + 1][ld]: beta[0] = ||x||, beta[k] = beta_k
  double* h;        // [order][ld]: the dots of the current step
  double* rr;       // [ld]: a column sum of squares
  int* active;      // [ld]
  int* steps;       // [ld]: Krylov vectors written so far (m)
};

// beta_0 = ||x||; a zero column never starts (its outputs stay zero)
__global__ void k_lz_start(LzScalars s, int ld) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ld) return;
  const double b = sqrt(s.rr[c]);
  s.beta[c] = b;
  const int act = b > 0 && isfinite(b);
  s.active[c] = act;
  s.steps[c] = act;
}

// after the update of step k: beta_{k+1} = ||r||, and the breakdown test of step k + 1
__global__ void k_lz_next(LzScalars s, int ld, int k, double breakdown) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ld || !s.active[c]) return;
  const double b = sqrt(s.rr[c]);
  s.beta[(size_t)(k + 1) * ld + c] = b;
  if (b <= breakdown)
    s.active[c] = 0;
  else
    s.steps[c] = k + 2;
}

// q_k = r / beta_k (zero for a stopped column), w = W / beta_k - beta_k q_{k-1} (in place), partial alpha_k = q_k . w
__global__ __launch_bounds__(256) void k_lz_three(double* __restrict__ V, size_t pstride, int k,
                                                  const double* __restrict__ r, double* __restrict__ W, LzScalars s,
                                                  int64_t N, int ld, int ldp, double* __restrict__ partial) {
  __shared__ double ws[256];
  const int c = threadIdx.x & (ldp - 1);
  const int rstep = 256 / ldp;
  double acc = 0;
  if (c < ld) {
    const bool on = s.active[c] != 0;
    const double bk = s.beta[(size_t)k * ld + c];
    double* __restrict__ qk = V + (size_t)k * pstride;
    const double* __restrict__ qp = k > 0 ? V + (size_t)(k - 1) * pstride : nullptr;
    const size_t stride = (size_t)gridDim.x * rstep;
    for (size_t i = (size_t)blockIdx.x * rstep + threadIdx.x / ldp; i < (size_t)N; i += stride) {
      const size_t e = i * ld + c;
      double q = 0, w = 0;
      if (on) {
        q = r[e] / bk;
        w = W[e] / bk;
        if (qp) w -= bk * qp[e];
      }
      qk[e] = q;
      W[e] = w;
      acc += q * w;
    }
  }
  block_colsum(ws, acc, ld, ldp, rstep, partial + (size_t)blockIdx.x * ld);
}

// partial h_j = q_j . (w - alpha_k q_k) for the LZ_JB stack panels j0 = blockIdx.y * LZ_JB .. of j = 0..nj-1
// (alpha == nullptr: plain q_j . w, i.e. V^T x with w = x).  partial[b][j][c], count = nj * ld per workgroup row b.
__global__ __launch_bounds__(256) void k_lz_dots(const double* __restrict__ V, size_t pstride, int nj,
                                                 const double* __restrict__ qk, const double* __restrict__ W,
                                                 const double* __restrict__ alpha, int64_t N, int ld, int ldp,
                                                 double* __restrict__ partial) {
  __shared__ double ws[256];
  const int c = threadIdx.x & (ldp - 1);
  const int rstep = 256 / ldp;
  const int j0 = blockIdx.y * LZ_JB;
  const int nb = min(LZ_JB, nj - j0);
  double acc[LZ_JB];
#pragma unroll
  for (int t = 0; t < LZ_JB; ++t) acc[t] = 0;
  if (c < ld) {
    const double al = alpha ? alpha[c] : 0.0;
    const double* __restrict__ V0 = V + (size_t)j0 * pstride;
    const size_t stride = (size_t)gridDim.x * rstep;
    for (size_t i = (size_t)blockIdx.x * rstep + threadIdx.x / ldp; i < (size_t)N; i += stride) {
      const size_t e = i * ld + c;
      double t = W[e];
      if (alpha) t -= al * qk[e];
#pragma unroll
      for (int jj = 0; jj < LZ_JB; ++jj)
        if (jj < nb) acc[jj] += V0[(size_t)jj * pstride + e] * t;
    }
  }
  double* out = partial + (size_t)blockIdx.x * nj * ld + (size_t)j0 * ld;
#pragma unroll
  for (int jj = 0; jj < LZ_JB; ++jj)
    if (jj < nb) block_colsum(ws, acc[jj], ld, ldp, rstep, out + (size_t)jj * ld);
}

// r = w - alpha_k q_k - sum_j h_j q_j (active columns; a stopped column keeps its r) and partial ||r||^2.
// Each thread carries four rows, so that one h_j load serves four stack reads.
__global__ __launch_bounds__(256) void k_lz_update(const double* __restrict__ V, size_t pstride, int k,
                                                   const double* __restrict__ W, double* __restrict__ r, LzScalars s,
                                                   int64_t N, int ld, int ldp, double* __restrict__ partial) {
  __shared__ double ws[256];
  const int c = threadIdx.x & (ldp - 1);
  const int rstep = 256 / ldp;
  double acc = 0;
  if (c < ld) {
    const bool on = s.active[c] != 0;
    const double al = s.alpha[(size_t)k * ld + c];
    const double* __restrict__ qk = V + (size_t)k * pstride;
    const size_t stride = (size_t)gridDim.x * rstep;
    double a[4] = {0, 0, 0, 0};
    for (size_t i = (size_t)blockIdx.x * rstep + threadIdx.x / ldp; i < (size_t)N; i += 4 * stride) {
      double t[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const size_t row = i + u * stride;
        ok[u] = row < (size_t)N;
        const size_t e = row * ld + c;
        t[u] = ok[u] ? W[e] - al * qk[e] : 0.0;
      }
      if (on) {
        for (int j = 0; j <= k; ++j) {
          const double hj = s.h[(size_t)j * ld + c];
          const double* __restrict__ qj = V + (size_t)j * pstride;
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (ok[u]) t[u] -= hj * qj[(i + u * stride) * ld + c];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (ok[u]) r[(i + u * stride) * ld + c] = t[u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] += t[u] * t[u];
    }
    acc = (a[0] + a[1]) + (a[2] + a[3]);
  }
  block_colsum(ws, acc, ld, ldp, rstep, partial + (size_t)blockIdx.x * ld);
}

// y[(f0 + f) N + perm[i]][c] = sum_j Wt[f0 + f][j][c] V_j[i][c] for FB filters; two rows per thread, so that
// one weight load serves two stack reads.
template <int FB>
__global__ __launch_bounds__(256) void k_lz_combine(const double* __restrict__ V, size_t pstride, int order,
                                                    const double* __restrict__ Wt, int nf, int64_t N, int ld, int ldp,
                                                    const int* __restrict__ perm, double* __restrict__ y,
                                                    int64_t ldy) {
  const int c = threadIdx.x & (ldp - 1);
  if (c >= ld) return;
  const int rstep = 256 / ldp;
  const int f0 = blockIdx.y * FB;
  const int fb = min(FB, nf - f0);
  const size_t stride = (size_t)gridDim.x * rstep;
  for (size_t i = (size_t)blockIdx.x * rstep + threadIdx.x / ldp; i < (size_t)N; i += 2 * stride) {
    const size_t i1 = i + stride;
    const bool ok1 = i1 < (size_t)N;
    double acc0[FB], acc1[FB];
#pragma unroll
    for (int f = 0; f < FB; ++f) acc0[f] = acc1[f] = 0;
    for (int j = 0; j < order; ++j) {
      const double* __restrict__ qj = V + (size_t)j * pstride;
      const double v0 = qj[i * ld + c];
      const double v1 = ok1 ? qj[i1 * ld + c] : 0.0;
#pragma unroll
      for (int f = 0; f < FB; ++f)
        if (f < fb) {
          const double w = Wt[((size_t)(f0 + f) * order + j) * ld + c];
          acc0[f] += w * v0;
          acc1[f] += w * v1;
        }
    }
    const size_t o0 = perm ? (size_t)perm[i] : i;
    const size_t o1 = ok1 ? (perm ? (size_t)perm[i1] : i1) : 0;
#pragma unroll
    for (int f = 0; f < FB; ++f)
      if (f < fb) {
        y[((size_t)(f0 + f) * N + o0) * ldy + c] = acc0[f];
        if (ok1) y[((size_t)(f0 + f) * N + o1) * ldy + c] = acc1[f];
      }
  }
}

}  // namespace gspx

// ---- host side ---------------------------------------------------------------------------------------------------
// workgroups along the rows: about 2048 in all (eight per CU) over `groups` workgroup columns, and no more than
// the rows need
static int lz_rows_grid(int64_t N, int ldp, int groups) {
  const int64_t rstep = 256 / ldp;
  const int64_t need = (N + rstep - 1) / rstep;
  const int64_t want = std::max<int64_t>(64, 2048 / std::max(groups, 1));
  return (int)std::max<int64_t>(1, std::min(need, want));
}

// per-phase event timing (only when the caller asks for phase times): one event pair per launch group
struct LzTimer {
  std::vector<hipEvent_t> ev;
  std::vector<int> phase;
  bool on = false;
  int mark(hipStream_t st, int ph) {
    if (!on) return GSPX_OK;
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    ev.push_back(e);
    phase.push_back(ph);
    HIPCHK(hipEventRecord(e, st));
    return GSPX_OK;
  }
  // phase ph of the pair (ev[i], ev[i + 1]) is that of ev[i + 1]: the time since the previous mark
  int sum(double* out, int nphase) {
    for (int p = 0; p < nphase; ++p) out[p] = 0;
    for (size_t i = 1; i < ev.size(); ++i) {
      float f = 0;
      HIPCHK(hipEventElapsedTime(&f, ev[i - 1], ev[i]));
      if (phase[i] >= 0 && phase[i] < nphase) out[phase[i]] += f;
    }
    return GSPX_OK;
  }
  ~LzTimer() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
};

// the same batch bound as the Python driver (pygsp_amd/lanczos.py, max_batch_width): `order` stack panels plus three
// work panels within ws_limit_mb, one panel below 2 GiB, at most LZ_MAX_WIDTH columns
static int64_t lz_max_width(gspx_graph* g, int order) {
  return std::min<int64_t>(ops_max_ld(g, sizeof(double), order + 3), gspx::LZ_MAX_WIDTH);
}

enum { LZ_PH_PERMUTE = 0, LZ_PH_SPMM, LZ_PH_THREE, LZ_PH_DOTS, LZ_PH_UPDATE, LZ_PH_PROJ, LZ_NPHASE };

extern "C" int gspx_lanczos_krylov_dev(gspx_graph* g, int order, int64_t Nsig, const void* x_dev, int64_t ldx,
                                       double breakdown, void* V_dev, double* alpha_host, double* beta_host,
                                       double* proj_host, int32_t* steps_host, double* phase_ms, double* kernel_ms) {
  if (order < 1) return set_err(GSPX_ERR_INVALID, "lanczos_krylov: order must be >= 1 (got %d)", order);
  if (Nsig < 0 || Nsig > gspx::LZ_MAX_WIDTH)
    return set_err(GSPX_ERR_INVALID, "lanczos_krylov: number of signals must be 0..%d (got %lld)", gspx::LZ_MAX_WIDTH,
                   (long long)Nsig);
  if (ldx < Nsig) return set_err(GSPX_ERR_INVALID, "lanczos_krylov: leading dimension below the number of signals");
  if (!(breakdown >= 0) || !std::isfinite(breakdown))
    return set_err(GSPX_ERR_INVALID, "lanczos_krylov: breakdown threshold must be finite and >= 0");
  if (Nsig > 0 && (!alpha_host || !beta_host || !proj_host || !steps_host))
    return set_err(GSPX_ERR_INVALID, "lanczos_krylov: null host output");
  if (g) replay_reset(g->ctx);
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (Nsig > 0 && g->N > 0 && (!x_dev || !V_dev)) return set_err(GSPX_ERR_INVALID, "lanczos_krylov: null signal pointer");
  if (g->dtype != GSPX_F64)
    return set_err(GSPX_ERR_INVALID, "lanczos_krylov: the graph computes in float32; Lanczos needs the float64 graph");
  if (kernel_ms) *kernel_ms = 0;
  if (phase_ms)
    for (int p = 0; p < LZ_NPHASE; ++p) phase_ms[p] = 0;
  const int64_t N = g->N;
  const int ld = (int)Nsig;
  if (Nsig == 0) return GSPX_OK;
  if (N == 0) {
    for (int64_t i = 0; i < (int64_t)order * ld; ++i) alpha_host[i] = beta_host[i] = proj_host[i] = 0.0;
    for (int c = 0; c < ld; ++c) steps_host[c] = 0;
    return GSPX_OK;
  }
  if (Nsig > lz_max_width(g, order))
    return set_err(GSPX_ERR_INVALID, "lanczos_krylov: %lld signals x order %d do not fit the workspace (at most %lld "
                   "columns; raise ws_limit_mb)", (long long)Nsig, order, (long long)lz_max_width(g, order));
  gspx_ctx* ctx = g->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int ldp = col_pow2(ld);
  const size_t U = (size_t)N * ld;
  const int* perm = g->has_perm ? g->perm.as<int>() : nullptr;
  // work panels: x (internal order), r, W; scalars; reduction partials (sized for the widest launch: the projection)
  CHK(ctx->ws_t.ensure(3 * U * sizeof(double) + 256));
  double* X = ctx->ws_t.as<double>();
  double* R = X + U;
  double* W = R + U;
  const int nred1 = lz_rows_grid(N, ldp, 1);
  int64_t part_max = (int64_t)nred1 * ld;
  for (int nj = 1; nj <= order; ++nj) {
    const int gy = (nj + gspx::LZ_JB - 1) / gspx::LZ_JB;
    part_max = std::max<int64_t>(part_max, (int64_t)lz_rows_grid(N, ldp, gy) * nj * ld);
  }
  DevMem scal, partial;
  const size_t nsc = (size_t)ld * (3 * (size_t)order + 2) + (size_t)ld;
  CHK(scal.alloc(nsc * sizeof(double) + 2 * (size_t)ld * sizeof(int) + 64));
  CHK(partial.alloc((size_t)part_max * sizeof(double)));
  gspx::LzScalars s;
  double* d = scal.as<double>();
  s.alpha = d;
  s.beta = s.alpha + (size_t)order * ld;
  s.h = s.beta + (size_t)(order + 1) * ld;
  s.rr = s.h + (size_t)order * ld;
  s.active = (int*)(s.rr + ld);
  s.steps = s.active + ld;
  double* proj = s.h;  // (the last step computes no dots: h holds V^T x at the end)
  HIPCHK(hipMemsetAsync(scal.p, 0, nsc * sizeof(double), st));
  double* V = (double*)V_dev;
  const size_t ps = U;
  const unsigned nsm = (unsigned)((ld + 63) / 64);
  LzTimer tm;
  tm.on = phase_ms != nullptr;
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  CHK(tm.mark(st, -1));
  CHK(permute_panel<double>(g, (const double*)x_dev, (unsigned)ldx, X, (unsigned)ld, perm));
  HIPCHK(hipMemcpyAsync(R, X, U * sizeof(double), hipMemcpyDeviceToDevice, st));
  CHK(tm.mark(st, LZ_PH_PERMUTE));
  hipLaunchKernelGGL((gspx::k_coldot_partial<double>), dim3(nred1), dim3(256), 0, st, X, X, (int)N, ld, ldp,
                     partial.as<double>());
  sum_parts(partial.as<double>(), nred1, ld, s.rr, st);
  hipLaunchKernelGGL(gspx::k_lz_start, dim3(nsm), dim3(64), 0, st, s, ld);
  CHK(tm.mark(st, LZ_PH_UPDATE));
  for (int k = 0; k < order; ++k) {
    CHK(spmm_internal<double>(g, g->rval.as<double>(), 1.0, 0.0, R, W, (unsigned)ld, nullptr, 0));
    CHK(tm.mark(st, LZ_PH_SPMM));
    hipLaunchKernelGGL(gspx::k_lz_three, dim3(nred1), dim3(256), 0, st, V, ps, k, R, W, s, N, ld, ldp,
                       partial.as<double>());
    sum_parts(partial.as<double>(), nred1, ld, s.alpha + (size_t)k * ld, st);
    CHK(tm.mark(st, LZ_PH_THREE));
    if (k + 1 == order) break;  // (beta_order is not needed)
    const int nj = k + 1, gy = (nj + gspx::LZ_JB - 1) / gspx::LZ_JB;
    const int nr = lz_rows_grid(N, ldp, gy);
    hipLaunchKernelGGL(gspx::k_lz_dots, dim3(nr, gy), dim3(256), 0, st, V, ps, nj, V + (size_t)k * ps, W,
                       s.alpha + (size_t)k * ld, N, ld, ldp, partial.as<double>());
    sum_parts(partial.as<double>(), nr, (int64_t)nj * ld, s.h, st);
    CHK(tm.mark(st, LZ_PH_DOTS));
    hipLaunchKernelGGL(gspx::k_lz_update, dim3(nred1), dim3(256), 0, st, V, ps, k, W, R, s, N, ld, ldp,
                       partial.as<double>());
    sum_parts(partial.as<double>(), nred1, ld, s.rr, st);
    hipLaunchKernelGGL(gspx::k_lz_next, dim3(nsm), dim3(64), 0, st, s, ld, k, breakdown);
    CHK(tm.mark(st, LZ_PH_UPDATE));
  }
  {  // V^T x, explicitly (the reference's np.dot(V.T, s))
    const int gy = (order + gspx::LZ_JB - 1) / gspx::LZ_JB;
    const int nr = lz_rows_grid(N, ldp, gy);
    hipLaunchKernelGGL(gspx::k_lz_dots, dim3(nr, gy), dim3(256), 0, st, V, ps, order, (const double*)nullptr, X,
                       (const double*)nullptr, N, ld, ldp, partial.as<double>());
    sum_parts(partial.as<double>(), nr, (int64_t)order * ld, proj, st);
    CHK(tm.mark(st, LZ_PH_PROJ));
  }
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  const size_t ob = (size_t)order * ld * sizeof(double);
  HIPCHK(hipMemcpyAsync(alpha_host, s.alpha, ob, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(beta_host, s.beta, ob, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(proj_host, proj, ob, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(steps_host, s.steps, (size_t)ld * sizeof(int), hipMemcpyDeviceToHost, st));
  CHK(finish_timed(ctx, kernel_ms));
  if (phase_ms) CHK(tm.sum(phase_ms, LZ_NPHASE));
  return GSPX_OK;
}

extern "C" int gspx_lanczos_combine_dev(gspx_graph* g, int order, int64_t Nsig, const void* V_dev, int Nf,
                                        const double* weights_host, void* y_dev, int64_t ldy, double* kernel_ms) {
  if (order < 1) return set_err(GSPX_ERR_INVALID, "lanczos_combine: order must be >= 1 (got %d)", order);
  if (Nsig < 0 || Nsig > gspx::LZ_MAX_WIDTH)
    return set_err(GSPX_ERR_INVALID, "lanczos_combine: number of signals must be 0..%d (got %lld)", gspx::LZ_MAX_WIDTH,
                   (long long)Nsig);
  if (Nf < 1) return set_err(GSPX_ERR_INVALID, "lanczos_combine: Nf must be >= 1 (got %d)", Nf);
  if (ldy < Nsig) return set_err(GSPX_ERR_INVALID, "lanczos_combine: leading dimension below the number of signals");
  if (Nsig > 0 && !weights_host) return set_err(GSPX_ERR_INVALID, "lanczos_combine: null weights");
  if (g) replay_reset(g->ctx);
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (Nsig > 0 && g->N > 0 && (!V_dev || !y_dev)) return set_err(GSPX_ERR_INVALID, "lanczos_combine: null signal pointer");
  if (g->dtype != GSPX_F64)
    return set_err(GSPX_ERR_INVALID, "lanczos_combine: the graph computes in float32; Lanczos needs the float64 graph");
  if (kernel_ms) *kernel_ms = 0;
  const int64_t N = g->N;
  const int ld = (int)Nsig;
  if (Nsig == 0 || N == 0) return GSPX_OK;
  gspx_ctx* ctx = g->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t wbytes = (size_t)Nf * order * ld * sizeof(double);
  CHK(ctx->ws_spec.ensure(wbytes));
  HIPCHK(hipMemcpyAsync(ctx->ws_spec.p, weights_host, wbytes, hipMemcpyHostToDevice, st));
  const int ldp = col_pow2(ld);
  const int* perm = g->has_perm ? g->perm.as<int>() : nullptr;
  const double* V = (const double*)V_dev;
  const size_t ps = (size_t)N * ld;
  // filters per launch: the smallest FB >= Nf among 1, 2, 4, 8 (Nf > 8: one pass over the stack per 8 filters)
  const int fb = Nf <= 1 ? 1 : Nf <= 2 ? 2 : Nf <= 4 ? 4 : 8;
  const int gy = (Nf + fb - 1) / fb;
  const int nr = (int)std::max<int64_t>(1, std::min<int64_t>((N + 2 * (256 / ldp) - 1) / (2 * (256 / ldp)),
                                                             std::max(64, 2048 / gy)));
  HIPCHK(hipEventRecord(ctx->ev[0], st));
#define LZ_COMBINE(FB)                                                                                          \
  hipLaunchKernelGGL((gspx::k_lz_combine<FB>), dim3(nr, gy), dim3(256), 0, st, V, ps, order,                   \
                     ctx->ws_spec.as<double>(), Nf, N, ld, ldp, perm, (double*)y_dev, ldy)
  switch (fb) {
    case 1: LZ_COMBINE(1); break;
    case 2: LZ_COMBINE(2); break;
    case 4: LZ_COMBINE(4); break;
    default: LZ_COMBINE(8); break;
  }
#undef LZ_COMBINE
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  return finish_timed(ctx, kernel_ms);
}
