// gspx_graph.hip.h - building a gspx_graph (replaces graph.py:510-630, 830-838): CSR validation, the Laplacian from W
// (or L as given), the internal padded CSR in the engine's vertex order, the gather tiles of the LDS-staged step, the
// download entry points, and what is derived from a built graph on first use: the
// scaled operator F of a given lmax (ensure_factor) and the gather lists as rows of an unpermuted panel (ensure_s1nat).
// The kernels only these use come first.  After gspx_adjacency.hip.h (scan_exclusive) and the kernel headers (k_fill,
// gspx_tile_kernels.hip.h's tile builders); gspx_setup uses k_inverse_perm from here.
#pragma once

namespace gspx {

// ---------------------------------------------------------------------------------------------
// graph build kernels (replace graph.py:618-628, 830-838)
// ---------------------------------------------------------------------------------------------
// dw[i] = sum_j W_ij, sequential in ascending column order: for an exactly symmetric W this is
// the same addition order as scipy's column sums W.sum(axis=0) (graph.py:833).
template <typename T>
__global__ void k_degree(const int* __restrict__ ptr, const T* __restrict__ val, int N,
                         T* __restrict__ dw) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  T s = 0;
  for (int j = ptr[i]; j < ptr[i + 1]; ++j) s += val[j];
  dw[i] = s;
}

// The ingredients of Graph._get_upper_bound (graph.py:933-960) in one pass over W, per 256-row block:
// part[4 b + 0..3] = max W_ij, max (dw_i + dw_j) over stored entries, max (dw_i + (W dw)_i / dw_i), number of
// zero-degree rows (their 0 / 0 makes numpy's maximum NaN: the host layer then drops that candidate, as
// Python's min() does).  The row sums run in column order without fused multiply-add, like scipy's W.dot(dw).
__global__ __launch_bounds__(256) void k_lmax_bounds(const int* __restrict__ ptr, const int* __restrict__ col,
                                                     const double* __restrict__ val, const double* __restrict__ dw,
                                                     int N, double* __restrict__ part) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  double wmax = -1e300, emax = -1e300, mmax = -1e300, zero = 0;
  if (i < N) {
    const double di = dw[i];
    double s = 0;
    for (int j = ptr[i]; j < ptr[i + 1]; ++j) {
      const double w = val[j], dj = dw[col[j]];
      const double p = w * dj;
      s = s + p;
      wmax = fmax(wmax, w);
      emax = fmax(emax, di + dj);
    }
    if (di == 0.0) zero = 1;
    else mmax = di + s / di;
  }
  __shared__ double sh[4][4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    wmax = fmax(wmax, __shfl_down(wmax, off));
    emax = fmax(emax, __shfl_down(emax, off));
    mmax = fmax(mmax, __shfl_down(mmax, off));
    zero += __shfl_down(zero, off);
  }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sh[wv][0] = wmax;
    sh[wv][1] = emax;
    sh[wv][2] = mmax;
    sh[wv][3] = zero;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = part + (size_t)blockIdx.x * 4;
    o[0] = fmax(fmax(sh[0][0], sh[1][0]), fmax(sh[2][0], sh[3][0]));
    o[1] = fmax(fmax(sh[0][1], sh[1][1]), fmax(sh[2][1], sh[3][1]));
    o[2] = fmax(fmax(sh[0][2], sh[1][2]), fmax(sh[2][2], sh[3][2]));
    o[3] = sh[0][3] + sh[1][3] + sh[2][3] + sh[3][3];
  }
}

// d^{-1/2} with the reference's isolated-vertex rule (graph.py:622-624)
template <typename T> __device__ __forceinline__ T inv_sqrt_deg(T dw) {
  return dw == T(0) ? T(0) : T(1) / sqrt(dw);
}

// value of L_ij for an off-diagonal stored W_ij
template <typename T>
__device__ __forceinline__ T lap_offdiag(int lap_type, T w, T di, T dj) {
  if (lap_type == 0) return -w;
  return -((di * w) * dj);  // (D*W)*D, graph.py:626
}
// value of L_ii given dw_i and the (possibly absent) self-loop weight
template <typename T> __device__ __forceinline__ T lap_diag(int lap_type, T dw, T wii, T di) {
  if (lap_type == 0) return dw - wii;
  if (dw == T(0)) return T(0);   // L[disconnected, disconnected] = 0, graph.py:627
  return T(1) - (di * wii) * di;
}

// pass 1 (count) / pass 2 (fill) of canonical L = D - W  or  I - D^-1/2 W D^-1/2, zeros dropped
template <typename T, bool FILL>
__global__ void k_lap_build(const int* __restrict__ wptr, const int* __restrict__ wcol,
                            const T* __restrict__ wval, const T* __restrict__ dw, int N,
                            int lap_type, int* __restrict__ cnt, const int* __restrict__ lptr,
                            int* __restrict__ lcol, T* __restrict__ lval) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const T dwi = dw[i];
  const T di = lap_type == 1 ? inv_sqrt_deg(dwi) : T(0);
  // self loop weight
  T wii = 0;
  for (int j = wptr[i]; j < wptr[i + 1]; ++j)
    if (wcol[j] == i) wii = wval[j];
  const T dval = lap_diag(lap_type, dwi, wii, di);
  int n = 0;
  int o = FILL ? lptr[i] : 0;
  bool diag_done = false;
  for (int j = wptr[i]; j < wptr[i + 1]; ++j) {
    const int c = wcol[j];
    if (c == i) continue;
    if (!diag_done && c > i) {
      diag_done = true;
      if (dval != T(0)) {
        if (FILL) { lcol[o] = i; lval[o] = dval; ++o; }
        ++n;
      }
    }
    const T dj = lap_type == 1 ? inv_sqrt_deg(dw[c]) : T(0);
    const T v = lap_offdiag(lap_type, wval[j], di, dj);
    if (v != T(0)) {
      if (FILL) { lcol[o] = c; lval[o] = v; ++o; }
      ++n;
    }
  }
  if (!diag_done && dval != T(0)) {
    if (FILL) { lcol[o] = i; lval[o] = dval; ++o; }
    ++n;
  }
  if (!FILL) cnt[i] = n;
}

__global__ void k_inverse_perm(const int* __restrict__ perm, int N, int* __restrict__ iperm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) iperm[perm[i]] = i;
}

// canonical L -> internal padded CSR.  pass 1: padded row lengths; pass 2: fill.
template <typename T, bool FILL>
__global__ void k_internal_build(const int* __restrict__ lptr, const int* __restrict__ lcol,
                                 const T* __restrict__ lval, int N,
                                 const int* __restrict__ perm, const int* __restrict__ iperm,
                                 int* __restrict__ cnt, int* __restrict__ rptr,
                                 int* __restrict__ rcol, T* __restrict__ rval) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // internal row
  if (i >= N) return;
  const int old = perm ? perm[i] : i;
  const int s = lptr[old], e = lptr[old + 1];
  bool has_diag = false;
  for (int j = s; j < e; ++j)
    if (lcol[j] == old) { has_diag = true; break; }
  const int n = (e - s) + (has_diag ? 0 : 1);
  const int npad = (n + 3) & ~3;
  if (!FILL) {
    cnt[i] = npad;
    return;
  }
  const int o = rptr[i];  // multiple of 4 (every row length is)
  rptr[i] = o | (npad - n);  // low 2 bits: number of pad entries closing this row
  // Rows of at most CAP entries (all but hubs): read once into registers, every entry's final position - the
  // diagonal first, the others by ascending internal column - is its rank among the row's entries (CAP^2 predicated
  // compares on registers), written once.  (The insertion sort in global memory below cost 5.2 GB of traffic for
  // 130 MB of matrix at N = 1M: profiles/r04_setup_hostpipe_rocprofv3_summary.txt.)
  constexpr int CAP = sizeof(T) == 8 ? 24 : 32;  // (32 doubles + 32 columns would spill at the default register bound)
  if (n <= CAP) {
    int cc[CAP];
    T vv[CAP];
    const int len = e - s;
#pragma unroll
    for (int p = 0; p < CAP; ++p) {
      const bool in = p < len;
      const int c = in ? lcol[s + p] : 0;
      cc[p] = in ? (iperm ? iperm[c] : c) : (p == len && !has_diag ? i : 0x7FFFFFFF);
      vv[p] = in ? lval[s + p] : T(0);
    }
#pragma unroll
    for (int p = 0; p < CAP; ++p) {
      if (p < n) {
        int pos = 0;
        if (cc[p] != i) {
          pos = 1;
#pragma unroll
          for (int q = 0; q < CAP; ++q) pos += (q < n && cc[q] != i && cc[q] < cc[p]) ? 1 : 0;
        }
        rcol[o + pos] = cc[p];
        rval[o + pos] = vv[p];
      }
    }
    for (int m2 = n; m2 < npad; ++m2) {
      rcol[o + m2] = N;  // out-of-range sentinel: the gather's bounds check returns 0
      rval[o + m2] = T(0);
    }
    return;
  }
  int m = 0;
  for (int j = s; j < e; ++j) {
    rcol[o + m] = iperm ? iperm[lcol[j]] : lcol[j];
    rval[o + m] = lval[j];
    ++m;
  }
  if (!has_diag) {
    rcol[o + m] = i;
    rval[o + m] = T(0);
    ++m;
  }
  // keep short rows sorted by (internal) column: neighbouring gathers stay adjacent
  if ((perm || !has_diag) && m <= 128) {
    for (int p = 1; p < m; ++p) {
      const int c = rcol[o + p];
      const T v = rval[o + p];
      int q = p - 1;
      while (q >= 0 && rcol[o + q] > c) {
        rcol[o + q + 1] = rcol[o + q];
        rval[o + q + 1] = rval[o + q];
        --q;
      }
      rcol[o + q + 1] = c;
      rval[o + q + 1] = v;
    }
  }
  // the diagonal slot becomes entry 0 of the row: the step kernels take T_{k-1}[row] from that
  // gather instead of loading it again (flush and Newton-form steps)
  {
    int p = 0;
    while (p < m && rcol[o + p] != i) ++p;
    const T dv = rval[o + p];
    if (m <= 128) {
      for (int q = p; q > 0; --q) {  // keep the rest sorted
        rcol[o + q] = rcol[o + q - 1];
        rval[o + q] = rval[o + q - 1];
      }
    } else {
      rcol[o + p] = rcol[o];
      rval[o + p] = rval[o];
    }
    rcol[o] = i;
    rval[o] = dv;
  }
  for (; m < npad; ++m) {
    rcol[o + m] = N;  // out-of-range sentinel: the gather's bounds check returns 0
    rval[o + m] = T(0);
  }
}

// F = (2/a1) * (L - a2 I) on the internal layout (approximations.py:105)
template <typename T>
__global__ void k_factor(const int* __restrict__ rptr, const int* __restrict__ rcol,
                         const T* __restrict__ rval, int N, T two_over_a1, T a2,
                         T* __restrict__ fval) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  for (int j = rptr[i] & ~3; j < (rptr[i + 1] & ~3); ++j) {
    const int c = rcol[j];
    T v = rval[j];
    if (c == i) v -= a2;
    fval[j] = (c == N) ? T(0) : two_over_a1 * v;
  }
}

}  // namespace gspx

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
  int total = 0;
  CHK(scan_exclusive(ctx, cnt.as<int>(), g->rptr.as<int>(), N + 1, &total));
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
  int total = 0;
  CHK(scan_exclusive(ctx, cnt.as<int>(), g->lptr.as<int>(), N + 1, &total));
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
  int n_s1 = 0;
  CHK(scan_exclusive(ctx, keep.as<int>(), s1lo.as<int>(), nb + 1, &n_s1));
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
// derived from a built graph on first use
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
