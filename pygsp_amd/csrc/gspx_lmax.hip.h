// gspx_lmax.hip.h - lambda_max by Lanczos on the device (gspx_lanczos_lmax; replaces the ARPACK call of
// graph.py:907-920) and its four vector kernels.  The reductions are its own, not gspx_reduce.hip.h's: the order of
// summation decides the last bits of the Ritz value, and with them every coefficient scaled by lambda_max.
// After gspx_poly.hip.h (choose_shape, launch_step: the product L v is one recurrence-step launch).
#pragma once

namespace gspx {

// ---------------------------------------------------------------------------------------------
// small vector kernels for the device Lanczos estimate of lambda_max (graph.py:907-920)
// ---------------------------------------------------------------------------------------------
// partial[b] = sum over the block's grid-stride elements of x*y (double accumulation)
template <typename T>
__global__ __launch_bounds__(256) void k_dot_partial(const T* __restrict__ x, const T* __restrict__ y,
                                                     size_t n, double* __restrict__ partial) {
  __shared__ double ws[4];
  double acc = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    acc += (double)x[i] * (double)y[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
// out[0] = sum(partial[0..n)) in a fixed order (deterministic)
__global__ __launch_bounds__(256) void k_sum_partials(const double* __restrict__ partial, int n,
                                                      double* __restrict__ out) {
  __shared__ double ws[4];
  double acc = 0;
  for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = ws[0] + ws[1] + ws[2] + ws[3];
}
// y = a*x + b*y
template <typename T>
__global__ void k_axpby(T a, const T* __restrict__ x, T b, T* __restrict__ y, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x)
    y[i] = a * x[i] + b * y[i];
}
// deterministic start vector: a fixed hash of the index mapped to [-1, 1)
template <typename T> __global__ void k_start_vector(T* v, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    unsigned h = (unsigned)i * 2654435761u;
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    v[i] = (T)((double)h / 2147483648.0 - 1.0);
  }
}

}  // namespace gspx

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
    launch_step<T>(g->ctx, a, shape, opt, st, nullptr);  // w = L v_j
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
