// gspx_graphlearn.hip.h - learning the weights of a graph from smooth signals on the device: the log-degree model of
// Kalofolias, "How to learn a graph from smooth signals" (2016), on a fixed candidate pattern as in Kalofolias &
// Perraudin, "Large scale graph learning from smooth signals" (2019) (pygsp_amd/graph_learning.py; DESIGN.md "Graph
// learning").  The reference has no counterpart: the definition is the numpy restatement tests/graphlearn_helpers.py.
//   gspx_edge_sqdist_dev        z_e = ||x_s - x_t||^2 over the graph's default edge list
//   gspx_learn_log_degrees_dev  argmin over w >= 0 of 2 z^T w - a sum_i log (S w)_i + b ||w||^2
// with (S w)_i = the sum of w over the edges at vertex i and (S^T v)_e = v_s + v_t.  Edge e = (s, t), s < t, is edge e
// of Graph.get_edge_list; the edge tables are gspx_ops.hip.h's (ensure_edges), in the caller's vertex order: I(i), the
// edges at vertex i, is tedge[toff[i] .. toff[i + 1]) (the edges that end in i, ascending) followed by the block
// eoff[i] .. eoff[i + 1] - 1 (the edges that start in i).
//
// Forward-backward-forward primal-dual with the fixed step g (the caller's step / (2 b + sqrt(2 dmax)), ||S||^2 <= 2 dmax),
// from w_0 (zeros unless given) and v_0 = S w_0; for k = 1, 2, ...
//   Y = w - g (2 b w + S^T v)        y = v + g S w
//   P = max(0, Y - 2 g z)            p = prox(y) = (y - r) / 2 for y <= 0, -2 a g / (y + r) for y > 0, r = sqrt(y^2 + 4 a g)
//   Q = P - g (2 b P + S^T p)        q = p + g S P
//   w <- (w - Y) + Q                 v <- (v - y) + q
// A vertex without edges takes no part: its v and p stay 0 (the log of its degree is not in the objective).
// Stop after iteration k when ||w_k - w_{k-1}|| <= tol ||w_k|| and ||v_k - v_{k-1}|| <= tol ||v_k|| (crit 1; compared as
// written, no division; a negative tol: off) or k >= maxit (crit SPX_MAXIT).  The result is P of the last iteration.
//
// Two passes per iteration, each one launch, and a one-workgroup rule kernel:
//   k_gl_vertex  V_k: finishes iteration k - 1, v <- d + (p + g S P) with d = v - y kept from before, sums ||v - v_old||^2
//                and ||v||^2 per workgroup, then opens iteration k: y = v + g S w, p = prox(y), d = v - y.  S P and S w
//                are formed together, reading the pair (w, P) of every edge of I(i) once.  V_1 forms v_0 = S w_0 instead.
//   k_gl_edge    E_k: Y, P, Q and the new w of every edge from (v, p) of its two endpoints; sums ||w - w_old||^2, ||w||^2.
//   k_gl_rule    R_k, after V_{k+1}: the four totals in a fixed order, the history row of iteration k, the stopping rule.
// Launch order V_1 E_1 | V_2 R_1 E_2 | V_3 R_2 E_3 | ... : three launches per iteration.  Once R_k has set the done flag
// every later launch returns at once; V_{k+1} ran before it and has left v_k (and an unused y, p), E_{k+1} never runs, so
// (w, P) are those of iteration k.  The update formulas are compiled without contraction into fused multiply-adds, so
// that they are the restatement's operations one by one (only the order of the sums differs).  The host reads the flag every FISTA_POLL iterations (gspx_fista.hip.h, whose
// FistaState, fista_totals and block_sums are reused; its objective-based FistaLoop is not).
// Layout: edges hold the pair wP[e] = (w, P) and vertices the pair vp[i] = (v, p), 16 bytes each, so that the gathers of
// both passes are one 16-byte load per neighbour; z (E) and d (N) are plain arrays.
// Vertex pass thread map: 8 lanes per vertex, lane j taking entries j, j + 8, ... of I(i) in order, combined by a
// fixed shuffle tree; a vertex with more than GL_HEAVY edges is left to the whole workgroup afterwards (256 threads
// stride its list, one fixed LDS tree), so a star centre costs one workgroup, not one lane.  No atomics anywhere, every
// grid is a function of N and E alone: the same inputs give the same bits on every call.
// The adjacency (w_out): count, scan, fill - one wavefront per vertex walks I(i) 64 entries at a time and keeps the
// edges with P > 0 in place by ballot; tedge sources ascend and lie below i, the eoff targets ascend above it, so the
// row is sorted as written, and both (s, t) and (t, s) carry the same P_e.
// After gspx_fista.hip.h (FistaState, fista_totals; block_sums, finish_timed, edges_for, the adjacency frame of
// gspx_adjacency.hip.h).
#pragma once

namespace gspx {

constexpr int GL_GROUP = 8;          // lanes per vertex in the vertex pass
constexpr int GL_HEAVY = 256;        // more edges than this at a vertex: the whole workgroup sums them
constexpr int GL_MAX_BLOCKS = 2048;  // workgroups per pass (grid-stride beyond): bounds the rule kernel's sums (it
                                     // took 26 us of a 590 us iteration with 8192 partials per sum)
constexpr int GL_MAX_F = 4096;

typedef double gl_d2 __attribute__((ext_vector_type(2)));

struct GlTables {
  const int* eoff;
  const int* toff;
  const int* tedge;
  const int* esrc;
  const int* edst;
  int N, E;
};

// the proximal step of -a log at step g, in the form that does not cancel
__device__ inline double gl_prox(double y, double ag4) {
#pragma clang fp contract(off)
  const double r = sqrt(y * y + ag4);
  return y <= 0.0 ? (y - r) / 2.0 : -(ag4 / 2.0) / (y + r);
}

// z_e = sum over columns of (x_s - x_t)^2: G lanes per edge (a power of two <= 64), lane j takes chunks j, j + G, ...
// of VEC columns in ascending order; the lanes are combined by a fixed shuffle tree
template <int VEC>
__global__ __launch_bounds__(256) void k_gl_sqdist(const int* __restrict__ esrc, const int* __restrict__ edst, int E,
                                                   int F, int G, const double* __restrict__ x, double* __restrict__ z) {
  typedef typename VT<double, VEC>::t V;
  const int lane = threadIdx.x & (G - 1), epb = 256 / G, cpr = F / VEC;
  // (the lanes of a group share e, so they stay in the loop together and the shuffles read live lanes only)
  for (int64_t e = (int64_t)blockIdx.x * epb + threadIdx.x / G; e < E; e += (int64_t)gridDim.x * epb) {
    const double* __restrict__ xs = x + (size_t)esrc[e] * F;
    const double* __restrict__ xt = x + (size_t)edst[e] * F;
    double acc = 0;
    for (int c = lane; c < cpr; c += G) {
      const V a = *(const V*)(xs + (size_t)c * VEC), b = *(const V*)(xt + (size_t)c * VEC);
      if constexpr (VEC == 2) {
        const double d0 = a.x - b.x, d1 = a.y - b.y;
        acc += d0 * d0;
        acc += d1 * d1;
      } else {
        const double d0 = a - b;
        acc += d0 * d0;
      }
    }
    for (int off = G >> 1; off > 0; off >>= 1) acc += __shfl_down(acc, off, G);
    if (lane == 0) z[e] = acc;
  }
}

// flag[0] = 1 when an entry of z is negative or NaN (every writer stores the same value)
__global__ __launch_bounds__(256) void k_gl_check_z(const double* __restrict__ z, int E, int* __restrict__ flag) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < E; e += (int64_t)gridDim.x * 256)
    if (!(z[e] >= 0.0)) flag[0] = 1;
}

// wP[e] = (w0[e] or 0, 0)
__global__ __launch_bounds__(256) void k_gl_init(const double* __restrict__ w0, int E, gl_d2* __restrict__ wP) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < E; e += (int64_t)gridDim.x * 256) {
    gl_d2 r;
    r.x = w0 ? w0[e] : 0.0;
    r.y = 0.0;
    wP[e] = r;
  }
}

// the pairs apart: P and (nullable) w
__global__ __launch_bounds__(256) void k_gl_split(const gl_d2* __restrict__ wP, int E, double* __restrict__ P,
                                                  double* __restrict__ w) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < E; e += (int64_t)gridDim.x * 256) {
    const gl_d2 r = wP[e];
    P[e] = r.y;
    if (w) w[e] = r.x;
  }
}

// what the lane that owns vertex i does with (S w)_i and (S P)_i; s: its partial sums (||dv||^2, ||v||^2)
__device__ inline void gl_vertex_finish(int i, bool isolated, double sw, double sp, int first, double g, double ag4,
                                        gl_d2* __restrict__ vp, double* __restrict__ d, double (&s)[2]) {
#pragma clang fp contract(off)
  if (isolated) {  // takes no part: v = p = 0 for good
    if (first) {
      gl_d2 zero;
      zero.x = zero.y = 0.0;
      vp[i] = zero;
      d[i] = 0.0;
    }
    return;
  }
  double v;
  if (first) {
    v = sw;  // v_0 = S w_0
  } else {
    const gl_d2 old = vp[i];
    v = d[i] + (old.y + g * sp);
    const double dv = v - old.x;
    s[0] += dv * dv;
    s[1] += v * v;
  }
  const double y = v + g * sw;
  gl_d2 nw;
  nw.x = v;
  nw.y = gl_prox(y, ag4);
  vp[i] = nw;
  d[i] = v - y;
}

// entry m of I(i): the pair (w, P) of that edge
__device__ inline gl_d2 gl_incident(const GlTables& t, const gl_d2* __restrict__ wP, int t0, int nt, int e0, int m) {
  return wP[m < nt ? t.tedge[t0 + m] : e0 + (m - nt)];
}

// partial[q * gridDim.x + blockIdx.x], q = 0: ||v_k - v_{k-1}||^2, q = 1: ||v_k||^2 (zeros from V_1)
__global__ __launch_bounds__(256) void k_gl_vertex(GlTables t, const FistaState* state, const gl_d2* __restrict__ wP,
                                                   gl_d2* __restrict__ vp, double* __restrict__ d, int first, double g,
                                                   double ag4, double* __restrict__ partial) {
  if (state->done) return;
  constexpr int VPB = 256 / GL_GROUP;  // vertices per workgroup and sweep
  __shared__ int heavy[VPB];
  __shared__ double red[2][4];
  const int lane = threadIdx.x & (GL_GROUP - 1), grp = threadIdx.x / GL_GROUP;
  double s[2] = {0, 0};
  for (int64_t base = (int64_t)blockIdx.x * VPB; base < t.N; base += (int64_t)gridDim.x * VPB) {
    const int64_t i64 = base + grp;
    const bool live = i64 < t.N;
    const int i = live ? (int)i64 : 0;
    int t0 = 0, nt = 0, e0 = 0, deg = 0;
    if (live) {
      t0 = t.toff[i];
      nt = t.toff[i + 1] - t0;
      e0 = t.eoff[i];
      deg = nt + (t.eoff[i + 1] - e0);
    }
    const bool big = deg > GL_HEAVY;
    double sw = 0, sp = 0;
    if (!big)
      for (int m = lane; m < deg; m += GL_GROUP) {
        const gl_d2 r = gl_incident(t, wP, t0, nt, e0, m);
        sw += r.x;
        sp += r.y;
      }
#pragma unroll
    for (int off = GL_GROUP >> 1; off > 0; off >>= 1) {
      sw += __shfl_down(sw, off, GL_GROUP);
      sp += __shfl_down(sp, off, GL_GROUP);
    }
    if (lane == 0) heavy[grp] = live && big ? 1 : 0;
    if (live && !big && lane == 0) gl_vertex_finish(i, deg == 0, sw, sp, first, g, ag4, vp, d, s);
    __syncthreads();
    for (int j = 0; j < VPB; ++j) {
      if (!heavy[j]) continue;  // (the same for every thread)
      const int h = (int)(base + j);
      const int ht0 = t.toff[h], hnt = t.toff[h + 1] - ht0, he0 = t.eoff[h], hdeg = hnt + (t.eoff[h + 1] - he0);
      double hw = 0, hp = 0;
      for (int m = threadIdx.x; m < hdeg; m += 256) {
        const gl_d2 r = gl_incident(t, wP, ht0, hnt, he0, m);
        hw += r.x;
        hp += r.y;
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        hw += __shfl_down(hw, off);
        hp += __shfl_down(hp, off);
      }
      if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = hw;
        red[1][threadIdx.x >> 6] = hp;
      }
      __syncthreads();
      if (threadIdx.x == 0)
        gl_vertex_finish(h, false, (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]),
                         (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]), first, g, ag4, vp, d, s);
      __syncthreads();
    }
    __syncthreads();  // heavy[] is rewritten by the next sweep
  }
  block_sums<2>(s, partial + blockIdx.x, gridDim.x);
}

// partial[q * gridDim.x + blockIdx.x], q = 0: ||w_k - w_{k-1}||^2, q = 1: ||w_k||^2
__global__ __launch_bounds__(256) void k_gl_edge(GlTables t, const FistaState* state, const double* __restrict__ z,
                                                 const gl_d2* __restrict__ vp, gl_d2* __restrict__ wP, double g,
                                                 double b2, double* __restrict__ partial) {
#pragma clang fp contract(off)
  if (state->done) return;
  double s[2] = {0, 0};
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < t.E; e += (int64_t)gridDim.x * 256) {
    const gl_d2 a = vp[t.esrc[e]], c = vp[t.edst[e]];
    const double w = wP[e].x;
    const double Y = w - g * (b2 * w + (a.x + c.x));
    const double P = fmax(0.0, Y - 2.0 * g * z[e]);
    const double Q = P - g * (b2 * P + (a.y + c.y));
    const double wn = (w - Y) + Q;
    const double dw = wn - w;
    s[0] += dw * dw;
    s[1] += wn * wn;
    gl_d2 r;
    r.x = wn;
    r.y = P;
    wP[e] = r;
  }
  block_sums<2>(s, partial + blockIdx.x, gridDim.x);
}

// R_k: pe = the two slabs of E_k (nbe workgroups), pv = those of V_{k+1} (nbv).  hist[4 (k - 1) ..] = ||dw||, ||w||,
// ||dv||, ||v||.
__global__ __launch_bounds__(256) void k_gl_rule(FistaState* state, const double* __restrict__ pe, int nbe,
                                                 const double* __restrict__ pv, int nbv, long long k, double tol,
                                                 long long maxit, double* __restrict__ hist) {
  if (state->done) return;
  __shared__ double tot[4];
  fista_totals<2>(pe, nbe, tot);
  fista_totals<2>(pv, nbv, tot + 2);
  if (threadIdx.x != 0) return;
  const double dw = sqrt(tot[0]), nw = sqrt(tot[1]), dv = sqrt(tot[2]), nv = sqrt(tot[3]);
  double* h = hist + 4 * (size_t)(k - 1);
  h[0] = dw;
  h[1] = nw;
  h[2] = dv;
  h[3] = nv;
  int crit = 0;
  if (tol >= 0 && dw <= tol * nw && dv <= tol * nv) crit = 1;
  else if (k >= maxit) crit = SPX_MAXIT;
  if (!crit) return;
  state->crit = crit;
  state->niter = k;
  state->done = 1;
}

// one wavefront per vertex over I(i), 64 entries a pass: the edges with P > 0.  rowptr null: count (len[i]); else fill.
__global__ __launch_bounds__(256) void k_gl_adjacency(GlTables t, const gl_d2* __restrict__ wP, int* __restrict__ len,
                                                      const int* __restrict__ rowptr, int* __restrict__ col,
                                                      double* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  const int64_t i64 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i64 >= t.N) return;  // (whole wavefronts leave together)
  const int i = (int)i64;
  const int t0 = t.toff[i], nt = t.toff[i + 1] - t0, e0 = t.eoff[i], deg = nt + (t.eoff[i + 1] - e0);
  int base = rowptr ? rowptr[i] : 0;
  for (int m0 = 0; m0 < deg; m0 += 64) {
    const int m = m0 + lane;
    int e = 0;
    double P = 0.0;
    if (m < deg) {
      e = m < nt ? t.tedge[t0 + m] : e0 + (m - nt);
      P = wP[e].y;
    }
    const bool keep = m < deg && P > 0.0;
    const unsigned long long bal = __ballot(keep);
    if (rowptr && keep) {
      const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
      col[pos] = m < nt ? t.esrc[e] : t.edst[e];
      val[pos] = P;
    }
    base += __popcll(bal);
  }
  if (!rowptr && lane == 0) len[i] = base;
}

}  // namespace gspx

// the graph's default edge tables, or the reason why the graph learner does not serve this graph
static int graphlearn_tables(gspx_graph* g, const char* who, gspx::GlTables* t) {
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (g->dtype != GSPX_F64)
    return set_err(GSPX_ERR_INVALID, "%s: the graph computes in float32; graph learning needs the float64 graph", who);
  if (!g->from_w)
    return set_err(GSPX_ERR_INVALID, "%s: the graph was created from L; graph learning needs a graph created from W", who);
  CHK(edges_for(g));
  if (g->edges_custom)
    return set_err(GSPX_ERR_INVALID,
                   "%s: the graph carries a caller's edge list (a directed graph or one with self-loops); weights are "
                   "learned on undirected patterns without self-loops", who);
  if (g->n_edges >= ((int64_t)1 << 31)) return set_err(GSPX_ERR_INVALID, "%s: %lld edges", who, (long long)g->n_edges);
  t->eoff = g->e_off.as<int>();
  t->toff = g->e_toff.as<int>();
  t->tedge = g->e_tedge.as<int>();
  t->esrc = g->e_src.as<int>();
  t->edst = g->e_dst.as<int>();
  t->N = (int)g->N;
  t->E = (int)g->n_edges;
  return GSPX_OK;
}

static unsigned graphlearn_blocks(int64_t items, int per_block) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, gspx::GL_MAX_BLOCKS));
}

extern "C" int gspx_edge_sqdist_dev(gspx_graph* g, int64_t F, const void* x_dev, void* z_dev, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  if (g) replay_reset(g->ctx);
  if (F < 1 || F > gspx::GL_MAX_F)
    return set_err(GSPX_ERR_INVALID, "edge_sqdist: the number of features must be 1..%d (got %lld)", gspx::GL_MAX_F,
                   (long long)F);
  gspx::GlTables t{};
  CHK(graphlearn_tables(g, "edge_sqdist", &t));
  if (t.E == 0) return GSPX_OK;
  if (!x_dev || !z_dev) return set_err(GSPX_ERR_INVALID, "edge_sqdist: null device pointer");
  gspx_ctx* ctx = g->ctx;
  hipStream_t st = ctx->stream;
  const int vec = (F % 2 == 0 && ((uintptr_t)x_dev % 16) == 0) ? 2 : 1;  // 16-byte loads where the rows allow them
  int G = 1;
  while (G < 64 && G < (int)F / vec) G <<= 1;
  const unsigned nb = graphlearn_blocks(t.E, 256 / G);
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  if (vec == 2)
    hipLaunchKernelGGL((gspx::k_gl_sqdist<2>), dim3(nb), dim3(256), 0, st, t.esrc, t.edst, t.E, (int)F, G,
                       (const double*)x_dev, (double*)z_dev);
  else
    hipLaunchKernelGGL((gspx::k_gl_sqdist<1>), dim3(nb), dim3(256), 0, st, t.esrc, t.edst, t.E, (int)F, G,
                       (const double*)x_dev, (double*)z_dev);
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  return finish_timed(ctx, kernel_ms);
}

// P as a symmetric adjacency in a fresh handle: count, scan, fill (the handle dies with any failure)
static int graphlearn_adjacency(gspx_graph* g, const gspx::GlTables& t, const gspx::gl_d2* wP, gspx_knn** out) {
  gspx_ctx* ctx = g->ctx;
  hipStream_t st = ctx->stream;
  const int64_t N = g->N;
  const auto t0 = std::chrono::steady_clock::now();
  std::unique_ptr<gspx_knn> h;
  CHK(adjacency_open(ctx, N, h));
  if (N > 0 && t.E > 0) {
    const unsigned nbw = (unsigned)((N + 3) / 4);
    hipLaunchKernelGGL(gspx::k_gl_adjacency, dim3(nbw), dim3(256), 0, st, t, wP, h->rowptr.as<int>(), (const int*)nullptr,
                       (int*)nullptr, (double*)nullptr);
    CHK(adjacency_offsets(h.get(), h->rowptr.as<int>(), "learn_log_degrees"));  // lengths -> offsets, in place
    if (h->nnz > 0) {
      hipLaunchKernelGGL(gspx::k_gl_adjacency, dim3(nbw), dim3(256), 0, st, t, wP, (int*)nullptr,
                         (const int*)h->rowptr.as<int>(), h->col.as<int>(), h->val.as<double>());
      HIPCHK(hipGetLastError());
    }
  }
  HIPCHK(hipStreamSynchronize(st));  // wP is the caller's to free after this
  adjacency_close(h, t0, out);
  return GSPX_OK;
}

extern "C" int gspx_learn_log_degrees_dev(gspx_graph* g, const void* z_dev, double a, double b, double step_gamma,
                                          double tol, int64_t maxit, const void* w0_dev, void* p_dev, void* w_dev,
                                          gspx_knn** w_out, int64_t* niter, int32_t* crit, double* history_host,
                                          double* kernel_ms) {
  const char* who = "learn_log_degrees";
  if (w_out) *w_out = nullptr;
  if (kernel_ms) *kernel_ms = 0;
  if (g) replay_reset(g->ctx);
  if (!(a > 0) || !std::isfinite(a)) return set_err(GSPX_ERR_INVALID, "%s: a must be positive and finite", who);
  if (!(b >= 0) || !std::isfinite(b)) return set_err(GSPX_ERR_INVALID, "%s: b must be non-negative and finite", who);
  if (!(step_gamma > 0) || !std::isfinite(step_gamma))
    return set_err(GSPX_ERR_INVALID, "%s: the step gamma must be positive and finite", who);
  if (maxit < 1 || maxit > gspx::FISTA_MAXIT_LIMIT)
    return set_err(GSPX_ERR_INVALID, "%s: maxit must be 1..%lld (got %lld)", who, gspx::FISTA_MAXIT_LIMIT,
                   (long long)maxit);
  if (std::isnan(tol)) return set_err(GSPX_ERR_INVALID, "%s: tol is NaN (a negative one disables the criterion)", who);
  if (!niter || !crit || !history_host) return set_err(GSPX_ERR_INVALID, "%s: null host output", who);
  *niter = 0;
  *crit = 0;
  gspx::GlTables t{};
  CHK(graphlearn_tables(g, who, &t));
  gspx_ctx* ctx = g->ctx;
  hipStream_t st = ctx->stream;
  const int64_t N = g->N, E = t.E;
  if (E == 0) {  // nothing to learn; the adjacency of no edges is an empty one
    if (w_out) CHK(graphlearn_adjacency(g, t, nullptr, w_out));
    return GSPX_OK;
  }
  if (!z_dev || !p_dev) return set_err(GSPX_ERR_INVALID, "%s: null device pointer", who);
  if (w_out && 2 * E > (int64_t)0x7fffffff)
    return set_err(GSPX_ERR_INVALID, "%s: the adjacency of %lld edges exceeds 32-bit indices", who, (long long)E);
  const double* z = (const double*)z_dev;
  const unsigned nbe = graphlearn_blocks(E, 256), nbv = graphlearn_blocks(N, 256 / gspx::GL_GROUP);
  // everything the loop touches is allocated here
  DevMem wPm, vpm, dm, part, hist, state, bad;
  CHK(wPm.alloc((size_t)E * sizeof(gspx::gl_d2)));
  CHK(vpm.alloc((size_t)N * sizeof(gspx::gl_d2)));
  CHK(dm.alloc((size_t)N * sizeof(double)));
  CHK(part.alloc((size_t)2 * (nbe + nbv) * sizeof(double)));
  CHK(hist.alloc((size_t)4 * (size_t)maxit * sizeof(double)));
  CHK(state.alloc(sizeof(FistaState)));
  CHK(bad.alloc(sizeof(int)));
  gspx::gl_d2* wP = wPm.as<gspx::gl_d2>();
  gspx::gl_d2* vp = vpm.as<gspx::gl_d2>();
  double* d = dm.as<double>();
  double* pe = part.as<double>();
  double* pv = pe + (size_t)2 * nbe;
  FistaState* sd = state.as<FistaState>();
  HIPCHK(hipMemsetAsync(bad.p, 0, sizeof(int), st));
  hipLaunchKernelGGL(gspx::k_gl_check_z, dim3(nbe), dim3(256), 0, st, z, (int)E, bad.as<int>());
  int hbad = 0;
  HIPCHK(hipMemcpyAsync(&hbad, bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (hbad) return set_err(GSPX_ERR_INVALID, "%s: z holds a negative or NaN entry", who);
  const double gm = step_gamma, ag4 = 4.0 * a * gm, b2 = 2.0 * b;
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  HIPCHK(hipMemsetAsync(sd, 0, sizeof(FistaState), st));
  hipLaunchKernelGGL(gspx::k_gl_init, dim3(nbe), dim3(256), 0, st, (const double*)w0_dev, (int)E, wP);
  hipLaunchKernelGGL(gspx::k_gl_vertex, dim3(nbv), dim3(256), 0, st, t, sd, wP, vp, d, 1, gm, ag4, pv);
  for (int64_t k = 1; k <= maxit; ++k) {
    hipLaunchKernelGGL(gspx::k_gl_edge, dim3(nbe), dim3(256), 0, st, t, sd, z, vp, wP, gm, b2, pe);
    hipLaunchKernelGGL(gspx::k_gl_vertex, dim3(nbv), dim3(256), 0, st, t, sd, wP, vp, d, 0, gm, ag4, pv);
    hipLaunchKernelGGL(gspx::k_gl_rule, dim3(1), dim3(256), 0, st, sd, pe, (int)nbe, pv, (int)nbv, (long long)k, tol,
                       (long long)maxit, hist.as<double>());
    if (k % gspx::FISTA_POLL == 0 && k < maxit) {  // a 4-byte read of the flag and a sync
      int done = 0;
      HIPCHK(hipMemcpyAsync(&done, &sd->done, sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (done) break;
    }
  }
  FistaState hs{};
  HIPCHK(hipMemcpyAsync(&hs, sd, sizeof(FistaState), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (!hs.done) return set_err(GSPX_ERR_HIP, "%s: the stopping rule did not fire", who);
  hipLaunchKernelGGL(gspx::k_gl_split, dim3(nbe), dim3(256), 0, st, wP, (int)E, (double*)p_dev, (double*)w_dev);
  HIPCHK(hipMemcpyAsync(history_host, hist.p, (size_t)4 * (size_t)hs.niter * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  CHK(finish_timed(ctx, kernel_ms));
  if (w_out) CHK(graphlearn_adjacency(g, t, wP, w_out));
  *niter = hs.niter;
  *crit = hs.crit;
  return GSPX_OK;
}
