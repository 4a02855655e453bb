// gspx_optim.hip.h - the proximal operator of the graph total variation on the device (pygsp_amd/optimization.py; the
// reference's optimization.prox_tv, pygsp/optimization.py:25-103, cannot run as shipped: it names an undefined D and
// an undefined verbose and returns nothing, so the algorithm below is this project's choice).
//   gspx_prox_tv_dev   argmin_z 1/2 ||x - z||^2 + gamma ||D^T z||_1 for an N x Nsig panel x, by FISTA on the dual
//
// With grad y = D^T y (edge panel) and div u = D u (vertex panel), the dual is min over |u| <= gamma of
// 1/2 ||x - D u||^2 and the primal point of u is z = x - D u.  State: u_k, a_k = D u_k, g_k = D^T (x - a_k); u_0 = 0,
// t_0 = 1, b_0 = 0, and for k = 0, 1, ...
//   u_{k+1} = clip(u_k + b_k (u_k - u_{k-1}) + step (g_k + b_k (g_k - g_{k-1})), -gamma, +gamma)
//   obj_k   = 1/2 ||a_k||^2 + gamma ||g_k||_1              (the primal objective at z_k = x - a_k)
//   t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2,  b_{k+1} = (t_k - 1) / t_{k+1}
// D^T is linear, so the gradient at the extrapolated point is the extrapolation of the gradients: one D and one D^T
// product per iteration, both on u_k itself, and g_k is recomputed from a_k every time (nothing drifts).  The rule is
// the shared one on obj_k and ||a_k - a_{k-1}||_F / sqrt(N Nsig), one objective for the panel.
//
// Launches of iteration k (vertex panels N x Nsig and edge panels n_edges x Nsig, fp64, caller's vertex order; the
// vertices are WALKED in the internal order: gspx_ops_kernels.hip.h's VertexWalk, as in k_div_v / k_grad_v):
//   k_tv_div        a_k = D u_k (the old a is read first), zt = x - a_k; partial sums of ||a_k||^2, ||a_k - a_{k-1}||^2
//   k_tv_grad_step  per source vertex: g_k = cs zt[src] + ct zt[dst] over g_{k-1} in place, partial sums of |g_k|, and
//                   u_{k+1} over u_{k-1} in place (the two u panels swap roles every iteration): three edge panels
//   k_tv_rule       one workgroup: forms obj_k from the summed partials and hands iteration k to the shared rule
// The loop around them - momentum, stopping rule, done flag, poll, finish - is gspx_fista.hip.h's.  The rule of
// iteration k runs before k_tv_div of iteration k + 1, so the accepted a_k and zt = z_k are never overwritten: the
// result is a copy of zt.  The grid is a function of N and Nsig alone and every sum has one order: the same inputs
// give the same bits on every call.  After gspx_fista.hip.h; nothing here needs gspx_learning.hip.h.
#pragma once

namespace gspx {

constexpr int TV_MAX_WIDTH = 256;
constexpr int TV_XCD_BLOCKS = 1024;  // most workgroups per XCD range (grid-stride beyond)

typedef VertexWalk<double> TvWalk;

typedef double tv_d2 __attribute__((ext_vector_type(2)));
__device__ inline double tv_sq(double v) { return v * v; }
__device__ inline double tv_sq(tv_d2 v) { return v.x * v.x + v.y * v.y; }
__device__ inline double tv_l1(double v) { return fabs(v); }
__device__ inline double tv_l1(tv_d2 v) { return fabs(v.x) + fabs(v.y); }
__device__ inline double tv_clip(double v, double g) { return fmin(fmax(v, -g), g); }
__device__ inline tv_d2 tv_clip(tv_d2 v, double g) {
  tv_d2 r;
  r.x = fmin(fmax(v.x, -g), g);
  r.y = fmin(fmax(v.y, -g), g);
  return r;
}

// partial[q * gridDim.x + blockIdx.x], q = 0: ||a_k||^2, q = 1: ||a_k - a_{k-1}||^2
template <int VEC>
__global__ __launch_bounds__(256) void k_tv_div(TvWalk w, const FistaState* state, const double* __restrict__ x,
                                                const double* __restrict__ u, double* __restrict__ a,
                                                double* __restrict__ zt, double* __restrict__ partial) {
  if (state->done) return;
  typedef typename VT<double, VEC>::t V;
  const WalkSpan sp = walk_span(w, VEC);
  const int ld = w.ld, gs = w.gs, lane = sp.lane, cpr = sp.cpr;
  double s[2] = {0, 0};
  for (int i = sp.lo; i < sp.hi; i += sp.stride) {
    const int v = w.perm ? w.perm[i] : i;
    const int e0 = w.eoff[v], e1 = w.eoff[v + 1], t0 = w.toff[v], t1 = w.toff[v + 1];
    for (int c = lane; c < cpr; c += gs) {
      const size_t o = (size_t)v * ld + (size_t)c * VEC;
      const V old = *(const V*)(a + o), xv = *(const V*)(x + o);
      V acc = 0;  // k_div_v's order: the vertex's own edges, then the edges pointing at it
      for (int k = e0; k < e1; k += 4) {  // four edge rows in flight per lane
        V uv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) uv[j] = *(const V*)(u + (size_t)(k + j < e1 ? k + j : e1 - 1) * ld + (size_t)c * VEC);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k + j < e1) acc += w.cs[k + j] * uv[j];
      }
      for (int m = t0; m < t1; m += 4) {
        int kk[4];
        V uv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) kk[j] = w.tedge[m + j < t1 ? m + j : t1 - 1];
#pragma unroll
        for (int j = 0; j < 4; ++j) uv[j] = *(const V*)(u + (size_t)kk[j] * ld + (size_t)c * VEC);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (m + j < t1) acc += w.ct[kk[j]] * uv[j];
      }
      *(V*)(a + o) = acc;
      *(V*)(zt + o) = xv - acc;
      s[0] += tv_sq(acc);
      s[1] += tv_sq(acc - old);
    }
  }
  block_sums<2>(s, partial + blockIdx.x, gridDim.x);
}

// partial[blockIdx.x] = sum |g_k| over the workgroup's edges.  g holds g_{k-1} and receives g_k; un holds u_{k-1} and
// receives u_{k+1}; every edge belongs to one source vertex, so one lane reads and writes each entry.
template <int VEC>
__global__ __launch_bounds__(256) void k_tv_grad_step(TvWalk w, const FistaState* state, const double* __restrict__ zt,
                                                      const double* __restrict__ u, double* __restrict__ un,
                                                      double* __restrict__ g, double b, double step, double gamma,
                                                      double* __restrict__ partial) {
  if (state->done) return;
  typedef typename VT<double, VEC>::t V;
  const WalkSpan sp = walk_span(w, VEC);
  const int ld = w.ld, gs = w.gs, lane = sp.lane, cpr = sp.cpr;
  double s[1] = {0};
  for (int i = sp.lo; i < sp.hi; i += sp.stride) {
    const int v = w.perm ? w.perm[i] : i;
    const int e0 = w.eoff[v], e1 = w.eoff[v + 1];
    for (int c = lane; c < cpr; c += gs) {
      const V xv = *(const V*)(zt + (size_t)v * ld + (size_t)c * VEC);
      for (int k = e0; k < e1; k += 4) {  // four edges in flight per lane
        size_t o[4];
        V xd[4], gp[4], uc[4], up[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int kk = k + j < e1 ? k + j : e1 - 1;
          o[j] = (size_t)kk * ld + (size_t)c * VEC;
          xd[j] = *(const V*)(zt + (size_t)w.edst[kk] * ld + (size_t)c * VEC);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          gp[j] = *(const V*)(g + o[j]);
          uc[j] = *(const V*)(u + o[j]);
          up[j] = *(const V*)(un + o[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k + j < e1) {
            const V gn = w.cs[k + j] * xv + w.ct[k + j] * xd[j];
            s[0] += tv_l1(gn);
            *(V*)(g + o[j]) = gn;
            const V p = uc[j] + b * (uc[j] - up[j]) + step * (gn + b * (gn - gp[j]));
            *(V*)(un + o[j]) = tv_clip(p, gamma);
          }
      }
    }
  }
  block_sums<1>(s, partial + blockIdx.x, gridDim.x);
}

// After the two panel launches of iteration k: obj_k = 1/2 ||a_k||^2 + gamma ||g_k||_1, judged as iteration k.
// partial: [3][nb], the two slabs of k_tv_div then the one of k_tv_grad_step.
__global__ __launch_bounds__(256) void k_tv_rule(FistaState* state, const double* __restrict__ partial, int nb,
                                                 long long k, double gamma, FistaTol tol, double nc,
                                                 double* __restrict__ obj) {
  if (state->done) return;
  __shared__ double tot[3];
  fista_totals<3>(partial, nb, tot);
  if (threadIdx.x != 0) return;
  fista_judge(state, obj, k, 0.5 * tot[0] + gamma * tot[2], tot[1], nc, tol);
}

}  // namespace gspx

using gspx::TvWalk;

template <int VEC>
static void tv_launch_iteration(const TvWalk& w, int nb, hipStream_t st, FistaState* sd, const double* x, const double* u,
                                double* un, double* a, double* zt, double* g, double b, double step, double gamma,
                                double* partial) {
  hipLaunchKernelGGL((gspx::k_tv_div<VEC>), dim3(nb), dim3(256), 0, st, w, sd, x, u, a, zt, partial);
  hipLaunchKernelGGL((gspx::k_tv_grad_step<VEC>), dim3(nb), dim3(256), 0, st, w, sd, zt, u, un, g, b, step, gamma,
                     partial + (size_t)2 * nb);
}

static int prox_tv_t(gspx_graph* g, double gamma, double step, int ld, const double* x, double* z, const FistaTol& tol,
                     int64_t* niter, int32_t* crit, double* objective, double* ms) {
  gspx_ctx* ctx = g->ctx;
  hipStream_t st = ctx->stream;
  const int64_t N = g->N, E = g->n_edges, maxit = tol.maxit;
  const size_t VU = (size_t)N * ld;
  // panels 256-byte aligned: a, zt | u (two, swapping roles) and g; an edge panel of an edgeless graph holds one row
  const size_t pv = (VU * sizeof(double) + 255) & ~(size_t)255;
  const size_t pe = ((size_t)std::max<int64_t>(E, 1) * ld * sizeof(double) + 255) & ~(size_t)255;
  const size_t total = 2 * pv + 3 * pe;
  if (total > ((size_t)std::max<int64_t>(ctx->opt.ws_limit_mb, 1) << 20))
    return set_err(GSPX_ERR_INVALID, "prox_tv: %lld signals need %zu MiB of workspace (raise ws_limit_mb)", (long long)ld,
                   total >> 20);
  FistaLoop loop;
  CHK(loop.init(g, "prox_tv", tol));
  CHK(ctx->ws_t.ensure(total));
  char* base = ctx->ws_t.as<char>();
  double* a = (double*)base;
  double* zt = (double*)(base + pv);
  double* U[2] = {(double*)(base + 2 * pv), (double*)(base + 2 * pv + pe)};
  double* G = (double*)(base + 2 * pv + 2 * pe);
  const int vec = (ld % 2 == 0 && ((uintptr_t)x % 16) == 0) ? 2 : 1;  // 16-byte lanes where the rows allow them
  TvWalk w{};
  // a function of N and Nsig alone (and of the alignment of x): the partial sums keep one order
  const int nb = (int)vertex_walk<double>(g, ld, vec, gspx::TV_XCD_BLOCKS, &w);
  DevMem part;
  CHK(part.alloc((size_t)3 * nb * sizeof(double)));
  CHK(loop.start());
  HIPCHK(hipMemsetAsync(base, 0, total, st));  // u_0 = u_{-1} = 0, a_{-1} = 0, g_{-1} = 0 (b_0 = 0 multiplies it)
  for (int64_t k = 0; k <= maxit; ++k) {  // loop.b is b_k at iteration k
    double* u = U[k % 2];
    double* un = U[(k + 1) % 2];
    if (vec == 2) tv_launch_iteration<2>(w, nb, st, loop.flags, x, u, un, a, zt, G, loop.b, step, gamma, part.as<double>());
    else tv_launch_iteration<1>(w, nb, st, loop.flags, x, u, un, a, zt, G, loop.b, step, gamma, part.as<double>());
    hipLaunchKernelGGL(gspx::k_tv_rule, dim3(1), dim3(256), 0, st, loop.flags, part.as<double>(), nb, (long long)k, gamma,
                       tol, (double)VU, loop.obj.as<double>());
    loop.advance();
    if (k > 0 && k % gspx::FISTA_POLL == 0 && k < maxit) {
      bool done = false;
      CHK(loop.poll(&done));
      if (done) break;
    }
  }
  return loop.finish(  // z_niter = x - a_niter
      [&](int64_t) -> int {
        HIPCHK(hipMemcpyAsync(z, zt, VU * sizeof(double), hipMemcpyDeviceToDevice, st));
        return GSPX_OK;
      },
      objective, niter, crit, ms);
}

extern "C" int gspx_prox_tv_dev(gspx_graph* g, double gamma, double step, int64_t Nsig, const void* x_dev, void* z_dev,
                                double rtol, double atol, double dtol, double xtol, int64_t maxit, int64_t* niter,
                                int32_t* crit, double* objective_host, double* kernel_ms) {
  if (!(gamma >= 0) || !std::isfinite(gamma)) return set_err(GSPX_ERR_INVALID, "prox_tv: gamma must be finite and >= 0");
  const FistaTol tol{rtol, atol, dtol, xtol, (long long)maxit};
  CHK(fista_check("prox_tv", g, step, tol, "number of signals", Nsig, gspx::TV_MAX_WIDTH, x_dev, z_dev, niter, crit,
                  objective_host));
  if (kernel_ms) *kernel_ms = 0;
  if (g->N == 0) {
    *niter = 0;
    *crit = 0;
    return GSPX_OK;
  }
  CHK(edges_for(g));
  if (fista_panel_too_large(g->N, Nsig) || fista_panel_too_large(g->n_edges, Nsig))
    return set_err(GSPX_ERR_INVALID, "prox_tv: an N x Nsig or n_edges x Nsig panel exceeds 2 GiB");
  return prox_tv_t(g, gamma, step, (int)Nsig, (const double*)x_dev, (double*)z_dev, tol, niter, crit, objective_host,
                   kernel_ms);
}
