// gspx_learning.hip.h - classification_tikhonov_simplex on the device (pygsp_amd/learning.py; the reference's
// learning.classification_tikhonov_simplex, which drives pyunlocbox's accelerated forward-backward solver).
//   gspx_tikhonov_simplex_dev   argmin_X tau tr(X^T L X) + sum_i m_i ||X_i - Y_i||^2, every row of X on the
//                               probability simplex, by FISTA with a fixed step; X is N x C, C = number of classes
//
// With f(X) = tau sum(X * LX) + sum_i m_i ||X_i - Y_i||^2, grad f(X) = 2 (m (X - Y) + tau LX) and P the row-wise
// Euclidean projection onto {x >= 0, sum x = 1}, iteration k (X_0 = V_0 = Y, t_0 = 1) is
//   X_k = P(V_{k-1} - step grad f(V_{k-1}))
//   t_k = (1 + sqrt(1 + 4 t_{k-1}^2)) / 2,   b_k = (t_{k-1} - 1) / t_k,   V_k = X_k + b_k (X_k - X_{k-1})
// and stops on the first of atol / dtol / rtol / xtol / maxit that holds for obj_k = f(X_k) (DESIGN.md,
// "Simplex-constrained classification").  L is linear, so L V_{k-1} = (1 + b) L X_{k-1} - b L X_{k-2}: one product
// per iteration, on X_k.  The b_k do not depend on the data and come from the host as launch arguments.
//
// Launch k of the loop (all panels N x C fp64 in the graph's INTERNAL vertex order):
//   k_spx_step_*   X_k from X_{k-1}, X_{k-2}, L X_{k-1}, L X_{k-2} and the labels, row-local; partial sums of
//                  sum m ||X_k - Y||^2 and ||X_k - X_{k-1}||^2, and of sum X_{k-1} * L X_{k-1} (both read anyway):
//                  obj_{k-1} is complete only after launch k, so three X buffers rotate and the rule fires on
//                  X_{k-1} while X_k sits in the third
//   k_spx_rule     one workgroup: forms obj_{k-1} from the summed partials and hands iteration k - 1 to the shared
//                  rule (fista_totals, fista_judge)
//   spmm_internal  L X_k, the engine's product
// The loop around them - momentum, stopping rule, done flag, poll, finish - is gspx_fista.hip.h's.  Partial sums have
// one order for a given N and C: the same inputs give the same bits on every call.  After gspx_fista.hip.h.
#pragma once

namespace gspx {

constexpr int SPX_MAX_CLASSES = 256;
constexpr int SPX_BLOCKS = 2048;  // fixed grid of the step kernels (grid-stride over rows): one summation order

struct SpxState {     // device resident
  double data_prev;   // sum m ||X_{k-1} - Y||^2 of the last iterate the rule has not judged yet
  double dx_prev;     // ||X_{k-1} - X_{k-2}||^2
  FistaState f;
  int bad_label;      // a label outside -1..C-1 was seen by k_spx_init
};

struct SpxStep {
  const double* A;    // X_{k-1}
  const double* B;    // X_{k-2} (= A for k = 1)
  const double* LA;   // L X_{k-1}
  const double* LB;   // L X_{k-2}
  const int* lab;     // class per internal row, -1 = unmeasured
  double* X;          // X_k
  double* partial;    // [3][gridDim.x]: data term, ||X_k - X_{k-1}||^2, sum X_{k-1} * L X_{k-1}
  const SpxState* state;
  int N, C;
  double b, step, tau;
  int write;          // 0 on the launch after maxit: only the last objective's dot product is wanted
};

// labels in the internal order, X_0 = one-hot rows (zero rows for unmeasured vertices)
__global__ void k_spx_init(const int* __restrict__ labels, const int* __restrict__ perm, int N, int C,
                           int* __restrict__ lab, double* __restrict__ X0, SpxState* state) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  int l = labels[perm ? perm[i] : i];
  if (l < -1 || l >= C) {
    state->bad_label = 1;  // (a plain store of the same value from every offender)
    l = -1;
  }
  lab[i] = l;
  for (int c = 0; c < C; ++c) X0[(size_t)i * C + c] = c == l ? 1.0 : 0.0;
}

// the three per-thread sums -> partial[q * gridDim.x + blockIdx.x] (gspx_reduce.hip.h's block_sums)
__device__ inline void spx_block_sums(double s0, double s1, double s2, double* partial) {
  const double v[3] = {s0, s1, s2};
  block_sums<3>(v, partial + blockIdx.x, gridDim.x);
}

// z = V - step grad f(V) for one entry (y = [c == label], m = [label >= 0])
__device__ inline double spx_point(const SpxStep& a, double av, double bv, double la, double lb, double m, double y) {
  const double v = av + a.b * (av - bv);
  const double lv = (1.0 + a.b) * la - a.b * lb;
  const double g = 2.0 * (m * (v - y) + a.tau * lv);
  return v - a.step * g;
}

// Rows of at most CMAX classes: one row per thread, the row in registers; the projection is Michelot's active-set
// pass (theta = (sum of the active entries - 1) / their count; drop the entries <= theta; repeat until none drops),
// exact and sort-free, at most C passes and usually two or three.
template <int CMAX>
__global__ __launch_bounds__(256) void k_spx_step_row(SpxStep a) {
  if (a.state->f.done) return;
  const int C = a.C;
  double sd = 0, sx = 0, ss = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < a.N; i += gridDim.x * 256) {
    const size_t o = (size_t)i * C;
    const int l = a.lab[i];
    const double m = l >= 0 ? 1.0 : 0.0;
    double z[CMAX], xa[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      if (c < C) {
        xa[c] = a.A[o + c];
        ss += xa[c] * a.LA[o + c];
        if (a.write) z[c] = spx_point(a, xa[c], a.B[o + c], a.LA[o + c], a.LB[o + c], m, c == l ? 1.0 : 0.0);
      }
    }
    if (!a.write) continue;
    unsigned act = (C >= 32) ? ~0u : ((1u << C) - 1u);
    double theta = 0;
    for (int pass = 0; pass < CMAX; ++pass) {
      double s = 0;
      int n = 0;
#pragma unroll
      for (int c = 0; c < CMAX; ++c)
        if ((act >> c) & 1u) {
          s += z[c];
          ++n;
        }
      theta = (s - 1.0) / n;
      unsigned keep = act;
#pragma unroll
      for (int c = 0; c < CMAX; ++c)
        if (((act >> c) & 1u) && z[c] <= theta) keep &= ~(1u << c);
      if (keep == act) break;
      act = keep;
    }
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      if (c < C) {
        const double x = fmax(z[c] - theta, 0.0);
        a.X[o + c] = x;
        const double e = x - (c == l ? 1.0 : 0.0);
        sd += m * (e * e);
        const double d = x - xa[c];
        sx += d * d;
      }
    }
  }
  spx_block_sums(sd, sx, ss, a.partial);
}

__device__ inline double spx_wave_sum(double v) {  // butterfly: every lane ends with the same bits
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Rows of 17..64 VPL classes: one row per wave, lane l holds classes l + 64 j (j < VPL); the same Michelot pass with
// wave sums.
template <int VPL>
__global__ __launch_bounds__(256) void k_spx_step_wave(SpxStep a) {
  if (a.state->f.done) return;
  const int C = a.C;
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  double sd = 0, sx = 0, ss = 0;
  for (int i = wave; i < a.N; i += gridDim.x * 4) {
    const size_t o = (size_t)i * C;
    const int l = a.lab[i];
    const double m = l >= 0 ? 1.0 : 0.0;
    double z[VPL], xa[VPL];
    bool act[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      const int c = lane + 64 * j;
      act[j] = c < C;
      z[j] = 0;
      xa[j] = 0;
      if (c < C) {
        xa[j] = a.A[o + c];
        ss += xa[j] * a.LA[o + c];
        if (a.write) z[j] = spx_point(a, xa[j], a.B[o + c], a.LA[o + c], a.LB[o + c], m, c == l ? 1.0 : 0.0);
      }
    }
    if (!a.write) continue;
    double theta = 0;
    for (int pass = 0; pass < 64 * VPL; ++pass) {
      double s = 0, n = 0;
#pragma unroll
      for (int j = 0; j < VPL; ++j)
        if (act[j]) {
          s += z[j];
          n += 1.0;
        }
      s = spx_wave_sum(s);
      n = spx_wave_sum(n);
      theta = (s - 1.0) / n;
      bool drop = false;
#pragma unroll
      for (int j = 0; j < VPL; ++j)
        if (act[j] && z[j] <= theta) {
          act[j] = false;
          drop = true;
        }
      if (!__any(drop)) break;
    }
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      const int c = lane + 64 * j;
      if (c < C) {
        const double x = fmax(z[j] - theta, 0.0);
        a.X[o + c] = x;
        const double e = x - (c == l ? 1.0 : 0.0);
        sd += m * (e * e);
        const double d = x - xa[j];
        sx += d * d;
      }
    }
  }
  spx_block_sums(sd, sx, ss, a.partial);
}

// After launch k: obj_{k-1} = tau sum(X_{k-1} L X_{k-1}) + data_{k-1}, judged as iteration k - 1 with the distance that
// waited in the state beside data_{k-1}; unless the rule fires, the sums of X_k wait there for the next launch.
__global__ __launch_bounds__(256) void k_spx_rule(SpxState* state, const double* __restrict__ partial, int nb,
                                                  long long k, double tau, FistaTol tol, double nc,
                                                  double* __restrict__ obj) {
  if (state->f.done) return;
  __shared__ double tot[3];
  fista_totals<3>(partial, nb, tot);
  if (threadIdx.x != 0) return;
  const double cur = tau * tot[2] + state->data_prev;
  if (fista_judge(&state->f, obj, k - 1, cur, state->dx_prev, nc, tol)) return;
  state->data_prev = tot[0];
  state->dx_prev = tot[1];
}

}  // namespace gspx

using gspx::SpxState;
using gspx::SpxStep;

static int spx_launch_step(const SpxStep& a, int nb, hipStream_t st) {
  const int C = a.C;
  if (C <= 2) hipLaunchKernelGGL((gspx::k_spx_step_row<2>), dim3(nb), dim3(256), 0, st, a);
  else if (C <= 4) hipLaunchKernelGGL((gspx::k_spx_step_row<4>), dim3(nb), dim3(256), 0, st, a);
  else if (C <= 8) hipLaunchKernelGGL((gspx::k_spx_step_row<8>), dim3(nb), dim3(256), 0, st, a);
  else if (C <= 16) hipLaunchKernelGGL((gspx::k_spx_step_row<16>), dim3(nb), dim3(256), 0, st, a);
  else if (C <= 64) hipLaunchKernelGGL((gspx::k_spx_step_wave<1>), dim3(nb), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((gspx::k_spx_step_wave<4>), dim3(nb), dim3(256), 0, st, a);
  return GSPX_OK;
}

static int spx_blocks(int64_t N, int C) {  // a function of N and C alone: the partial sums keep one order
  const int64_t rows_per_block = C <= 16 ? 256 : 4;
  return (int)std::max<int64_t>(1, std::min<int64_t>(gspx::SPX_BLOCKS, (N + rows_per_block - 1) / rows_per_block));
}

static int tikhonov_simplex_t(gspx_graph* g, double tau, double step, const int32_t* labels, int C, const FistaTol& tol,
                              double* x, int64_t* niter, int32_t* crit, double* objective, double* ms) {
  gspx_ctx* ctx = g->ctx;
  hipStream_t st = ctx->stream;
  const int64_t N = g->N, maxit = tol.maxit;
  const size_t U = (size_t)N * C;
  const int* perm = g->has_perm ? g->perm.as<int>() : nullptr;
  const int* iperm = g->has_perm ? g->iperm.as<int>() : nullptr;
  const int nb = spx_blocks(N, C);
  FistaLoop loop;
  CHK(loop.init(g, "tikhonov_simplex", tol, sizeof(SpxState), offsetof(SpxState, f)));
  DevMem panels, lab, part;
  // panels 256-byte aligned, with room for the product kernels' vector reads past a panel's end
  const size_t pitch = (U * sizeof(double) + 511) & ~(size_t)255;
  const size_t pad = 256;
  CHK(panels.alloc(5 * pitch));
  CHK(lab.alloc((size_t)N * sizeof(int) + pad));
  CHK(part.alloc((size_t)3 * nb * sizeof(double)));
  double* X[3];
  double* LX[2];
  for (int j = 0; j < 5; ++j) {
    double* p = (double*)((char*)panels.p + j * pitch);
    if (j < 3) X[j] = p;
    else LX[j - 3] = p;
  }
  CHK(loop.start());
  SpxState* sd = loop.state.as<SpxState>();
  hipLaunchKernelGGL(gspx::k_spx_init, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, labels, perm, (int)N, C,
                     lab.as<int>(), X[0], sd);
  SpxState hs{};
  HIPCHK(hipMemcpyAsync(&hs, sd, sizeof(SpxState), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (hs.bad_label) return set_err(GSPX_ERR_INVALID, "tikhonov_simplex: a label lies outside -1..n_classes-1");
  CHK(spmm_internal<double>(g, g->rval.as<double>(), 1.0, 0.0, X[0], LX[0], (unsigned)C, nullptr, 0));
  SpxStep a{};
  a.lab = lab.as<int>();
  a.partial = part.as<double>();
  a.state = sd;
  a.N = (int)N;
  a.C = C;
  a.step = step;
  a.tau = tau;
  for (int64_t k = 1; k <= maxit + 1; ++k) {  // loop.b is b_{k-1} at launch k
    a.A = X[(k - 1) % 3];
    a.B = k >= 2 ? X[(k - 2) % 3] : a.A;
    a.LA = LX[(k - 1) % 2];
    a.LB = k >= 2 ? LX[(k - 2) % 2] : a.LA;
    a.X = X[k % 3];
    a.b = loop.b;
    a.write = k <= maxit;
    CHK(spx_launch_step(a, nb, st));
    hipLaunchKernelGGL(gspx::k_spx_rule, dim3(1), dim3(256), 0, st, sd, part.as<double>(), nb, (long long)k, tau, tol,
                       (double)U, loop.obj.as<double>());
    if (k <= maxit) CHK(spmm_internal<double>(g, g->rval.as<double>(), 1.0, 0.0, X[k % 3], LX[k % 2], (unsigned)C,
                                              nullptr, 0));
    loop.advance();
    if (k % gspx::FISTA_POLL == 0 && k <= maxit) {
      bool done = false;
      CHK(loop.poll(&done));
      if (done) break;
    }
  }
  return loop.finish(
      [&](int64_t n_it) { return permute_panel<double>(g, X[n_it % 3], (unsigned)C, x, (unsigned)C, iperm); }, objective,
      niter, crit, ms);
}

extern "C" int gspx_tikhonov_simplex_dev(gspx_graph* g, double tau, double step, const int32_t* labels_dev,
                                         int n_classes, double rtol, double atol, double dtol, double xtol,
                                         int64_t maxit, void* x_dev, int64_t* niter, int32_t* crit,
                                         double* objective_host, double* kernel_ms) {
  if (!(tau > 0) || !std::isfinite(tau)) return set_err(GSPX_ERR_INVALID, "tikhonov_simplex: tau must be positive and finite");
  const FistaTol tol{rtol, atol, dtol, xtol, (long long)maxit};
  CHK(fista_check("tikhonov_simplex", g, step, tol, "n_classes", n_classes, gspx::SPX_MAX_CLASSES, labels_dev, x_dev,
                  niter, crit, objective_host));
  if (fista_panel_too_large(g->N, n_classes))
    return set_err(GSPX_ERR_INVALID, "tikhonov_simplex: an N x n_classes panel exceeds 2 GiB");
  if (kernel_ms) *kernel_ms = 0;
  if (g->N == 0) {
    *niter = 0;
    *crit = 0;
    return GSPX_OK;
  }
  return tikhonov_simplex_t(g, tau, step, labels_dev, n_classes, tol, (double*)x_dev, niter, crit, objective_host,
                            kernel_ms);
}
