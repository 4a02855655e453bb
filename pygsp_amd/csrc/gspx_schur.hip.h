// gspx_schur.hip.h - Schur complements of A = L + shift I on the device: the harmonic extension at a shift with the kept
// rows of A x (gspx_schur_cg_dev), and the Kron reduction built from it (gspx_kron_build; pygsp/reduction.py:309-381
// solves A_uu directly with spsolve).  gfx950 only.  Included by gspx.hip after gspx_linegraph.hip.h (uses the
// harmonic frame of gspx_ops.hip.h, the adjacency frame of gspx_adjacency.hip.h, DevMem, HIPCHK, CHK).
//
// With kept set k and eliminated set u the Schur complement A_kk - A_ku A_uu^-1 A_uk is rows k of A X, where X holds the
// indicator columns of the kept vertices extended by A_uu X_u = -A_uk: the solve gspx_dirichlet_cg_dev runs for
// shift = 0.  Applied to a signal f on the kept vertices the same rows are K_reg f of reduction.interpolate, one solve
// per column and no dense nk x nk matrix.
//
// Kron reduction, per batch of <= 256 kept vertices: an indicator panel made on the device, the solve, the kept rows
// written in `ind` order into columns [c0, c0 + w) of a dense nk x nk buffer.  Then (S + S^T) / 2 tile by tile through
// LDS, and W = max(0, -offdiag) as CSR by count, scan, fill: one wavefront per row, places from ballots - no atomics,
// the same bits on every call.
#pragma once

namespace gspx {

// out[orow[i]][0 .. ld) = sum_j L[i][j] X[j][:] + shift X[i][:] for the measured internal rows i (m[i] != 0); an
// unmeasured row is skipped - not computed - and, with zero_fill, its output row is set to zero.  orow null: row i.
// One group of gs lanes per row, VEC elements (16 bytes when the pitches allow) per lane, four neighbour rows in
// flight; X is an internal-order panel of pitch ld, out has pitch ldo.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void k_schur_rows(const int* __restrict__ rptr, const int* __restrict__ rcol,
                                                    const T* __restrict__ rval, const T* __restrict__ m,
                                                    const int* __restrict__ orow, const T* __restrict__ X,
                                                    T* __restrict__ out, int N, int ld, size_t ldo, T shift, int gs,
                                                    int zero_fill) {
  typedef typename VT<T, VEC>::t V;
  const int lane = threadIdx.x % gs, grp = threadIdx.x / gs, gpb = 256 / gs, cpr = ld / VEC;
  for (int i = blockIdx.x * gpb + grp; i < N; i += gridDim.x * gpb) {
    const bool kept = m[i] != T(0);
    if (!kept && !zero_fill) continue;
    const int r = orow ? orow[i] : i;
    T* __restrict__ o = out + (size_t)r * ldo;
    if (!kept) {
      for (int c = lane; c < cpr; c += gs) *(V*)(o + (size_t)c * VEC) = V(0);
      continue;
    }
    const int j0 = rptr[i] & ~3, j1 = rptr[i + 1] & ~3;  // (every row length is a multiple of 4; pads have col == N)
    for (int c = lane; c < cpr; c += gs) {
      V acc = shift * *(const V*)(X + (size_t)i * ld + (size_t)c * VEC);
      for (int j = j0; j < j1; j += 4) {
        int cc[4];
        T vv[4];
        V xv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          cc[q] = rcol[j + q];
          vv[q] = cc[q] == N ? T(0) : rval[j + q];
          if (cc[q] == N) cc[q] = i;  // a pad: a row that is there, times zero
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) xv[q] = *(const V*)(X + (size_t)cc[q] * ld + (size_t)c * VEC);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc += vv[q] * xv[q];
      }
      *(V*)(o + (size_t)c * VEC) = acc;
    }
  }
}

// Kron reduction: the internal-order tables of a kept set.  rank: N ints in the caller's vertex order, the place of a
// kept vertex in `ind`, -1 for an eliminated one.  orow[i] = rank of internal row i, m[i] = 1 where kept.
__global__ void k_kron_rows(const int* __restrict__ rank, const int* __restrict__ perm, int N, int* __restrict__ orow,
                            double* __restrict__ m) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int r = rank[perm ? perm[i] : i];
  orow[i] = r;
  m[i] = r >= 0 ? 1.0 : 0.0;
}
// the indicator panel of kept vertices c0 .. c0 + ld - 1: B[i][c] = 1 where orow[i] == c0 + c
__global__ void k_kron_indicator(const int* __restrict__ orow, double* __restrict__ B, size_t total, int ld, int c0) {
  const unsigned n = (unsigned)total, step = gridDim.x * blockDim.x;
  for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += step)
    B[e] = orow[e / (unsigned)ld] == c0 + (int)(e % (unsigned)ld) ? 1.0 : 0.0;
}

// out = (S + S^T) / 2 for the n x n row-major S, 32 x 32 tiles: workgroup (bx, by), bx <= by, stages tile (by, bx) and
// tile (bx, by) in LDS (rows padded to 33 doubles: the transposed reads walk a column) and writes both halves of the
// pair, rows coalesced.  a + b and b + a round alike, so out equals its transpose bit for bit.  out may be S.
__global__ __launch_bounds__(256) void k_kron_symmetrize(const double* S, double* out, int n) {
  if (blockIdx.x > blockIdx.y) return;
  __shared__ double A[32][33], B[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 columns x 8 rows per pass
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  for (int k = ty; k < 32; k += 8) {
    const int ra = r0 + k, ca = c0 + tx, rb = c0 + k, cb = r0 + tx;
    A[k][tx] = (ra < n && ca < n) ? S[(size_t)ra * n + ca] : 0.0;  // tile (by, bx)
    B[k][tx] = (rb < n && cb < n) ? S[(size_t)rb * n + cb] : 0.0;  // tile (bx, by)
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int ra = r0 + k, ca = c0 + tx, rb = c0 + k, cb = r0 + tx;
    if (ra < n && ca < n) out[(size_t)ra * n + ca] = (A[k][tx] + B[tx][k]) * 0.5;
    if (blockIdx.x != blockIdx.y && rb < n && cb < n) out[(size_t)rb * n + cb] = (B[k][tx] + A[tx][k]) * 0.5;
  }
}

// W = max(0, -offdiag(S)): the stored entries of row r are the columns c != r with S[r][c] < 0.  One wavefront per row,
// 64 columns per pass; a lane's place is the row's running count plus the kept lanes below it (ballot).  rowptr null:
// count only (len[r]); else fill col / val from rowptr[r].
__global__ __launch_bounds__(256) void k_kron_w(const double* __restrict__ S, int n, int* __restrict__ len,
                                                const int* __restrict__ rowptr, int* __restrict__ col,
                                                double* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;  // (whole wavefronts leave together)
  const double* __restrict__ row = S + (size_t)r * n;
  int base = rowptr ? rowptr[r] : 0;
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int c = c0 + lane;
    const double v = c < n ? row[c] : 0.0;
    const bool keep = c < n && c != r && v < 0.0;
    const unsigned long long b = __ballot(keep);
    if (rowptr && keep) {
      const int pos = base + __popcll(b & ((1ull << lane) - 1ull));
      col[pos] = c;
      val[pos] = -v;
    }
    base += __popcll(b);
  }
  if (!rowptr && lane == 0) len[r] = base;
}

}  // namespace gspx

template <typename T>
static int schur_kept_rows(gspx_graph* g, T shift, const T* m, const T* X, unsigned ld, const int* orow, bool zero_fill,
                           T* out, size_t ldo) {
  constexpr int W = 16 / (int)sizeof(T);
  const bool wide = ld % W == 0 && ldo % W == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)X % 16) == 0;
  const int cpr = wide ? (int)ld / W : (int)ld;
  int gs = 1;
  while (gs < 64 && gs < cpr) gs *= 2;
  const int gpb = 256 / gs;
  const unsigned nb = (unsigned)std::min<int64_t>((g->N + gpb - 1) / gpb, 65536);
  hipStream_t st = g->ctx->stream;
  if (wide)
    hipLaunchKernelGGL((gspx::k_schur_rows<T, W>), dim3(nb), dim3(256), 0, st, g->rptr.as<int>(), g->rcol.as<int>(),
                       g->rval.as<T>(), m, orow, X, out, (int)g->N, (int)ld, ldo, shift, gs, zero_fill ? 1 : 0);
  else
    hipLaunchKernelGGL((gspx::k_schur_rows<T, 1>), dim3(nb), dim3(256), 0, st, g->rptr.as<int>(), g->rcol.as<int>(),
                       g->rval.as<T>(), m, orow, X, out, (int)g->N, (int)ld, ldo, shift, gs, zero_fill ? 1 : 0);
  HIPCHK(hipGetLastError());
  return GSPX_OK;
}

extern "C" int gspx_schur_cg_dev(gspx_graph* g, double shift, const void* mask_dev, int64_t Nsig, const void* f_dev,
                                 void* x_dev, void* alpha_dev, double rtol, double atol, int64_t maxiter,
                                 int32_t* iterations, double* kernel_ms) {
  if (g) replay_reset(g->ctx);
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (!(shift >= 0) || !std::isfinite(shift))
    return set_err(GSPX_ERR_INVALID, "schur_cg: shift must be non-negative and finite");
  if (Nsig < 0 || maxiter < 0 || !(rtol >= 0) || !(atol >= 0)) return set_err(GSPX_ERR_INVALID, "schur_cg: bad argument");
  if (Nsig > 0 && g->N > 0 && (!mask_dev || !f_dev)) return set_err(GSPX_ERR_INVALID, "null pointer");
  HIPCHK(hipSetDevice(g->ctx->device));
  return g->dtype == GSPX_F32
             ? dirichlet_cg_t<float>(g, (float)shift, (const float*)mask_dev, Nsig, (const float*)f_dev, (float*)x_dev,
                                     (float*)alpha_dev, rtol, atol, maxiter, iterations, kernel_ms)
             : dirichlet_cg_t<double>(g, shift, (const double*)mask_dev, Nsig, (const double*)f_dev, (double*)x_dev,
                                      (double*)alpha_dev, rtol, atol, maxiter, iterations, kernel_ms);
}

extern "C" int gspx_kron_build(gspx_graph* g, double shift, const int32_t* ind_host, int64_t nk, double rtol,
                               int64_t maxiter, double* lnew_dev, gspx_knn** w_out, int32_t* iterations,
                               double* kernel_ms) {
  if (w_out) *w_out = nullptr;
  if (kernel_ms) *kernel_ms = 0;
  if (g) replay_reset(g->ctx);
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (g->dtype != GSPX_F64) return set_err(GSPX_ERR_INVALID, "kron_build: float64 graphs only");
  if (!(shift >= 0) || !std::isfinite(shift))
    return set_err(GSPX_ERR_INVALID, "kron_build: shift must be non-negative and finite");
  if (maxiter < 0 || !(rtol >= 0)) return set_err(GSPX_ERR_INVALID, "kron_build: bad argument");
  const int64_t N = g->N;
  if (nk < 1 || nk > N || !ind_host)
    return set_err(GSPX_ERR_INVALID, "kron_build: 1 <= nk <= N vertices to keep, got %lld of %lld", (long long)nk,
                   (long long)N);
  std::vector<int> rank((size_t)N, -1);
  for (int64_t c = 0; c < nk; ++c) {
    const int64_t v = ind_host[c];
    if (v < 0 || v >= N || rank[(size_t)v] >= 0)
      return set_err(GSPX_ERR_INVALID, "kron_build: ind[%lld] = %lld is out of range or repeated", (long long)c,
                     (long long)v);
    rank[(size_t)v] = (int)c;
  }
  gspx_ctx* ctx = g->ctx;
  hipStream_t st = ctx->stream;
  HIPCHK(hipSetDevice(ctx->device));
  // the dense result next to the five work panels of one batch: within the context's workspace limit
  const int64_t max_ld = std::min<int64_t>(cg_max_ld(g, sizeof(double)), nk);
  const size_t dense = (size_t)nk * (size_t)nk * sizeof(double);
  const size_t panels = 5 * (size_t)N * (size_t)std::max<int64_t>(max_ld, 1) * sizeof(double);
  const size_t budget = (size_t)std::max<int64_t>(ctx->opt.ws_limit_mb, 1) << 20;
  if (max_ld < 1 || dense + panels > budget)
    return set_err(GSPX_ERR_INVALID,
                   "kron_build: the dense %lld x %lld result (%.1f MiB) and the work panels (%.1f MiB) exceed "
                   "ws_limit_mb = %lld", (long long)nk, (long long)nk, dense / 1048576.0, panels / 1048576.0,
                   (long long)ctx->opt.ws_limit_mb);
  const auto t0 = std::chrono::steady_clock::now();
  DevMem rank_d, orow, sbuf;
  CHK(rank_d.alloc((size_t)N * sizeof(int)));
  CHK(orow.alloc((size_t)N * sizeof(int)));
  CHK(sbuf.alloc(dense));
  HarmonicSystem<double> hs;
  CHK(harmonic_alloc<double>(g, shift, hs));
  HIPCHK(hipMemcpyAsync(rank_d.p, rank.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  const int nbN = std::max(1, (int)((N + 255) / 256));
  hipLaunchKernelGGL(gspx::k_kron_rows, dim3(nbN), dim3(256), 0, st, rank_d.as<int>(),
                     g->has_perm ? g->perm.as<int>() : nullptr, (int)N, orow.as<int>(), hs.mint.as<double>());
  CHK(harmonic_values<double>(g, hs));
  double* S = sbuf.as<double>();
  // per-phase device time (solves, row products, finalise), left in the context for gspx_last_timing: three marks per
  // batch, read once the batch is done (its solve has synchronised the stream many times by then)
  struct Marks {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    ~Marks() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  } mk;
  for (hipEvent_t& x : mk.e) HIPCHK(hipEventCreate(&x));
  double phase[3] = {0, 0, 0};
  auto lap = [&](hipEvent_t a, hipEvent_t b, double* acc) {
    float f = 0;
    if (hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&f, a, b) == hipSuccess) *acc += f;
  };
  for (int64_t c0 = 0; c0 < nk; c0 += max_ld) {
    const unsigned ld = (unsigned)std::min<int64_t>(max_ld, nk - c0);
    const size_t U = (size_t)N * ld;
    CgPanels<double> w;
    CHK(cg_panels<double>(g, ld, &w));
    const unsigned nbU = (unsigned)std::min<size_t>((U + 255) / 256, 65536);
    HIPCHK(hipEventRecord(mk.e[0], st));
    hipLaunchKernelGGL(gspx::k_kron_indicator, dim3(nbU), dim3(256), 0, st, orow.as<int>(), w.B, U, (int)ld, (int)c0);
    CHK(harmonic_solve<double>(g, hs, w, ld, rtol, 0.0, maxiter, iterations ? iterations + c0 : nullptr));
    HIPCHK(hipEventRecord(mk.e[1], st));
    CHK(schur_kept_rows<double>(g, shift, hs.mint.as<double>(), w.X, ld, orow.as<int>(), false, S + c0, (size_t)nk));
    HIPCHK(hipEventRecord(mk.e[2], st));
    lap(mk.e[0], mk.e[1], &phase[0]);
    lap(mk.e[1], mk.e[2], &phase[1]);
  }
  HIPCHK(hipEventRecord(mk.e[0], st));  // the finalising pass begins
  // finalise: symmetrise (into the caller's buffer when there is one), then W from the symmetric matrix
  const unsigned nt = (unsigned)((nk + 31) / 32);
  double* L = lnew_dev ? lnew_dev : S;
  hipLaunchKernelGGL(gspx::k_kron_symmetrize, dim3(nt, nt), dim3(256), 0, st, S, L, (int)nk);
  HIPCHK(hipGetLastError());
  std::unique_ptr<gspx_knn> h;
  if (w_out) {
    CHK(adjacency_open(ctx, nk, h));
    const unsigned nbw = (unsigned)((nk + 3) / 4);
    hipLaunchKernelGGL(gspx::k_kron_w, dim3(nbw), dim3(256), 0, st, L, (int)nk, h->rowptr.as<int>(),
                       (const int*)nullptr, (int*)nullptr, (double*)nullptr);
    CHK(adjacency_offsets(h.get(), h->rowptr.as<int>(), "kron_build"));  // lengths -> offsets, in place
    if (h->nnz > 0) {
      hipLaunchKernelGGL(gspx::k_kron_w, dim3(nbw), dim3(256), 0, st, L, (int)nk, (int*)nullptr,
                         (const int*)h->rowptr.as<int>(), h->col.as<int>(), h->val.as<double>());
      HIPCHK(hipGetLastError());
    }
  }
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  CHK(finish_timed(ctx, kernel_ms));
  lap(mk.e[0], ctx->ev[1], &phase[2]);
  for (int i = 0; i < 5; ++i) ctx->timing[i] = i < 3 ? phase[i] : 0.0;
  if (h) adjacency_close(h, t0, w_out);
  return GSPX_OK;
}
