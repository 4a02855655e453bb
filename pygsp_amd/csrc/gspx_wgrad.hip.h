// gspx_wgrad.hip.h - the derivative of a Chebyshev filter's output with respect to the Laplacian's entries
// (gspx_cheby_laplacian_grad_dev; pygsp_amd.filters.cheby_op_vjp_weights, pygsp_amd.nn.WeightedGraph).
// With y_f = c_f0/2 x + sum_{k>=1} c_fk T_k(Lt) x, Lt = (2/lmax) L - I, t_k = T_k(Lt) x and cotangent planes g_f, the
// adjoint states are the Clenshaw sequence of the cotangent,
//     b_k = u_k + 2 Lt b_{k+1} - b_{k+2},  u_k = sum_f c_fk g_f,  k = M-1 .. 1,  b_M = b_{M+1} = 0,
// and, at fixed lmax and with the entries of L taken as independent,
//     dl/dL = (2/lmax) sum_{k=1}^{M-1} phi_k b_k t_{k-1}^T,   phi_1 = 1, phi_k = 2 otherwise.
// Two restrictions of that matrix leave the device, both summed over the signal columns: its diagonal (k_row_cross)
// and the symmetric sums over a list of vertex pairs (k_pair_cross).  Per column batch the deferred plan of one filter
// keeps t_0 .. t_{M-2} (run_batch with a SlotsUse hook, as the cross-Grams of gspx_conv.hip.h); the hook brings the
// cotangent planes into the internal order, runs clenshaw_step for k = M-1 .. 1 and after each step the two kernels on
// (b_k, t_{k-1}).  Step 0 (the gradient of x) stays with the synthesis call.  No step kernel is touched.  gfx950 only.
// After gspx_poly.hip.h (run_batch, clenshaw_step, run_batches) and gspx_ops.hip.h (edges_for).
#pragma once

namespace gspx {

// The pairs of a call into the internal vertex order, checked on the way: flag[0] = 1 when a pair has a vertex outside
// [0, N) or names one vertex twice (every writer stores the same value; such a pair is mapped to (0, 0)).
__global__ __launch_bounds__(256) void k_wgrad_map(const int* __restrict__ src, const int* __restrict__ dst, int64_t P,
                                                   int N, const int* __restrict__ iperm, int* __restrict__ ms,
                                                   int* __restrict__ md, int* __restrict__ flag) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    const int s = src[p], t = dst[p];
    const bool ok = s >= 0 && s < N && t >= 0 && t < N && s != t;
    if (!ok) flag[0] = 1;
    ms[p] = ok ? (iperm ? iperm[s] : s) : 0;
    md[p] = ok ? (iperm ? iperm[t] : t) : 0;
  }
}

// sum_c (b[s, c] t[t, c] + b[t, c] t[s, c]) over the columns one lane of a group of G takes: pieces of V elements
// (16 bytes where V > 1) at lane, lane + G, ..., then the w % V columns no piece holds, one per lane.  fp64 products
// and sums for both panel dtypes.  s == t (k_row_cross): one product per column.
template <typename T, int V, bool SAME>
__device__ __forceinline__ double wgrad_lane_sum(const T* __restrict__ bs, const T* __restrict__ bt,
                                                 const T* __restrict__ ts, const T* __restrict__ tt, int w, int lane,
                                                 int G) {
  typedef typename VT<T, V>::t vec_t;
  double acc = 0.0;
  const int nv = w / V;
  for (int c = lane; c < nv; c += G) {
    if constexpr (V == 1) {
      if constexpr (SAME) {
        acc += (double)bs[c] * (double)ts[c];
      } else {
        acc += (double)bs[c] * (double)tt[c];
        acc += (double)bt[c] * (double)ts[c];
      }
    } else {
      const vec_t vbs = *(const vec_t*)(bs + (size_t)c * V), vts = *(const vec_t*)(ts + (size_t)c * V);
      if constexpr (SAME) {
#pragma unroll
        for (int e = 0; e < V; ++e) acc += (double)vbs[e] * (double)vts[e];
      } else {
        const vec_t vbt = *(const vec_t*)(bt + (size_t)c * V), vtt = *(const vec_t*)(tt + (size_t)c * V);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          acc += (double)vbs[e] * (double)vtt[e];
          acc += (double)vbt[e] * (double)vts[e];
        }
      }
    }
  }
  if constexpr (V > 1) {
    for (int c = nv * V + lane; c < w; c += G) {
      if constexpr (SAME) {
        acc += (double)bs[c] * (double)ts[c];
      } else {
        acc += (double)bs[c] * (double)tt[c];
        acc += (double)bt[c] * (double)ts[c];
      }
    }
  }
  return acc;
}

// ---------------------------------------------------------------------------------------------
// goff[p] += phi * sum_c (b[s_p, c] t[t_p, c] + b[t_p, c] t[s_p, c])  over the w columns of a batch.
// b (pitch pb) and t (pitch pt): panels in the internal vertex order; ps / pd: the pairs in that order (k_wgrad_map).
// A group of G = 2^gl lanes (1 .. 64, inside one wave) owns a pair: its lanes run across the columns, V elements per
// load, rows wider than a group looped over; the group's sums meet by shuffles in a fixed order and lane 0 adds the
// total to goff[p].  A pair belongs to one group of one launch and the launches of a call follow each other on one
// stream, so the read-modify-write is race-free and there are no atomics: identical calls give identical bits.
// grid: groups walk the pairs with stride gridDim.x * (256 >> gl).
// ---------------------------------------------------------------------------------------------
template <typename T, int V>
__global__ __launch_bounds__(256) void k_pair_cross(const T* __restrict__ b, size_t pb, const T* __restrict__ t,
                                                    size_t pt, int w, const int* __restrict__ ps,
                                                    const int* __restrict__ pd, int64_t P, int gl, double phi,
                                                    double* __restrict__ goff) {
  const int G = 1 << gl;
  const int lane = threadIdx.x & (G - 1);
  const int64_t gpb = 256 >> gl;
  for (int64_t p = (int64_t)blockIdx.x * gpb + (threadIdx.x >> gl); p < P; p += (int64_t)gridDim.x * gpb) {
    const size_t s = (size_t)ps[p], d = (size_t)pd[p];
    double acc = wgrad_lane_sum<T, V, false>(b + s * pb, b + d * pb, t + s * pt, t + d * pt, w, lane, G);
    for (int off = G >> 1; off > 0; off >>= 1) acc += __shfl_down(acc, off, G);
    if (lane == 0) goff[p] += phi * acc;
  }
}

// ---------------------------------------------------------------------------------------------
// gdiag[perm(row)] += phi * sum_c b[row, c] t[row, c]: both panels streamed once, a group of 2^gl lanes per row as
// above; perm: the internal row -> the caller's row (null: the same).  A row belongs to one group: no atomics.
// ---------------------------------------------------------------------------------------------
template <typename T, int V>
__global__ __launch_bounds__(256) void k_row_cross(const T* __restrict__ b, size_t pb, const T* __restrict__ t,
                                                   size_t pt, int w, int N, const int* __restrict__ perm, int gl,
                                                   double phi, double* __restrict__ gdiag) {
  const int G = 1 << gl;
  const int lane = threadIdx.x & (G - 1);
  const int64_t gpb = 256 >> gl;
  for (int64_t r = (int64_t)blockIdx.x * gpb + (threadIdx.x >> gl); r < N; r += (int64_t)gridDim.x * gpb) {
    const T* __restrict__ br = b + (size_t)r * pb;
    const T* __restrict__ tr = t + (size_t)r * pt;
    double acc = wgrad_lane_sum<T, V, true>(br, br, tr, tr, w, lane, G);
    for (int off = G >> 1; off > 0; off >>= 1) acc += __shfl_down(acc, off, G);
    if (lane == 0) gdiag[perm ? perm[r] : (int)r] += phi * acc;
  }
}

}  // namespace gspx

// ---- host side --------------------------------------------------------------------------------------------------
// What the hook of a batch needs beside the kept slots.
struct LapGrad {
  gspx_graph* g;
  const void* z;  // the cotangent planes at the batch's first column, the caller's vertex order
  unsigned ldz;
  size_t zplane;
  int nf, M;             // M: the orders of the call (the batch keeps M - 1 slots)
  const double* coeffs;  // HOST, nf x M
  const int* ps;         // the pairs in the internal order
  const int* pd;
  int64_t P;
  double scale;  // 2 / lmax
  double* gdiag;  // null: not wanted
  double* goff;
};

// (b_k, t_{k-1}) of one batch into the two outputs
template <typename T>
static void launch_wgrad_cross(const gspx_ctx* ctx, const T* b, size_t pb, const T* t, size_t pt, int N, unsigned w,
                               const int* perm, const LapGrad& lg, double phi, hipStream_t st) {
  constexpr unsigned VM = 16 / (unsigned)sizeof(T);
  const bool vec = w >= VM && pb % VM == 0 && pt % VM == 0 && ((uintptr_t)b % 16) == 0 && ((uintptr_t)t % 16) == 0;
  const unsigned pieces = vec ? w / VM : w;
  int gl = 0;
  while ((1u << gl) < pieces && gl < 6) ++gl;
  const int64_t gpb = 256 >> gl, most = (int64_t)32 * std::max(ctx->cu_count, 1);
  if (lg.goff && lg.P > 0) {
    const unsigned nb = (unsigned)std::min<int64_t>((lg.P + gpb - 1) / gpb, most);
    typedef void (*kern_t)(const T*, size_t, const T*, size_t, int, const int*, const int*, int64_t, int, double, double*);
    const kern_t kern = vec ? k_pair_cross<T, (int)VM> : k_pair_cross<T, 1>;
    hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, st, b, pb, t, pt, (int)w, lg.ps, lg.pd, lg.P, gl, phi, lg.goff);
  }
  if (lg.gdiag) {
    const unsigned nb = (unsigned)std::min<int64_t>(((int64_t)N + gpb - 1) / gpb, most);
    typedef void (*kern_t)(const T*, size_t, const T*, size_t, int, int, const int*, int, double, double*);
    const kern_t kern = vec ? k_row_cross<T, (int)VM> : k_row_cross<T, 1>;
    hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, st, b, pb, t, pt, (int)w, N, perm, gl, phi, lg.gdiag);
  }
}

// where the two Clenshaw panels of a batch start: behind its kept slots, on a 256-byte boundary
template <typename T> static T* wgrad_panels(const void* slots, int nslots, size_t slot_stride) {
  const size_t off = ((size_t)nslots * slot_stride * sizeof(T) + 255) & ~(size_t)255;
  return (T*)((unsigned char*)const_cast<void*>(slots) + off);
}

// The SlotsUse hook: slots t_0 .. t_{M-2} of pitch `pitch` in ctx->ws_t, which the caller sized for the two Clenshaw
// panels behind them; the cotangent planes go to ctx->ws_r (idle in a deferred batch) in the geometry work_panels
// gives nf input panels - the routing (tile_direct / padded / plain) is run_synthesis_batch's, the same clenshaw_step.
template <typename T>
static int lap_grad_use(gspx_ctx* ctx, const void* slots_v, int nslots, size_t slot_stride, unsigned pitch, int N,
                        unsigned ld, const int* perm, const void* arg, hipStream_t st) {
  const LapGrad& lg = *(const LapGrad*)arg;
  gspx_graph* g = lg.g;
  const Options opt = ctx->opt;
  const int nf = lg.nf, M = lg.M, K = M - 1;
  const T* slots = (const T*)slots_v;
  const WorkPanels wp = work_panels<T>(g, opt, true, (size_t)nf, ld, (const T*)nullptr, ld);
  const unsigned ldw = wp.ldw;
  const size_t U = (size_t)N * ldw;
  const Shape shape = choose_shape(opt, sizeof(T), ld, vec_cap(4, ld, (const T*)nullptr));

  // weights [M][nf]: w[k][f] = c_fk (row 0 is never read: step 0 does not run)
  std::vector<T> hw((size_t)M * nf);
  for (int k = 0; k < M; ++k)
    for (int f = 0; f < nf; ++f) hw[(size_t)k * nf + f] = (T)lg.coeffs[(size_t)f * M + k];
  CHK(ctx->ws_w.ensure(hw.size() * sizeof(T) + 64));
  HIPCHK(hipMemcpyAsync(ctx->ws_w.p, hw.data(), hw.size() * sizeof(T), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));  // hw is a stack-owned staging buffer
  CHK(ctx->ws_r.ensure((size_t)nf * U * sizeof(T) + 256));
  T* S = ctx->ws_r.as<T>();
  T* B0 = wgrad_panels<T>(slots_v, nslots, slot_stride);
  T* B[2] = {B0, B0 + U};

  const T* z = (const T*)lg.z;
  for (int f = 0; f < nf; ++f) {
    const T* zf = z + (size_t)f * lg.zplane;
    if (wp.padded) {
      const unsigned nbp = (unsigned)std::min<size_t>((U + 255) / 256, 65536);
      hipLaunchKernelGGL((k_permute_in_pad<T>), dim3(nbp), dim3(256), 0, st, zf, lg.ldz, S + (size_t)f * U, ldw, ld, N, perm);
      continue;
    }
    launch_permute_in<T>(zf, lg.ldz, S + (size_t)f * U, ld, N, perm, vec_cap(shape.vec, lg.ldz, zf), st);
  }
  CHK(prepare_coff<T>(g, shape, ld, st));
  StepArgs<T> a = step_base<T>(g, ld, (T*)nullptr, ld);
  for (int k = K; k >= 1; --k) {
    CHK(clenshaw_step<T>(g, opt, wp, shape, a, k, K, S, ctx->ws_w.as<T>() + (size_t)k * nf, nf, S, B, (T*)nullptr, ld, st));
    launch_wgrad_cross<T>(ctx, B[k & 1], ldw, slots + (size_t)(k - 1) * slot_stride, pitch, N, ld, perm, lg,
                          (k == 1 ? 1.0 : 2.0) * lg.scale, st);
  }
  return GSPX_OK;
}

template <typename T>
static int laplacian_grad_dev_t(gspx_graph* g, double lmax, int Nf, int M, const double* coeffs, int64_t Nsig, const T* x,
                                const T* z, int64_t P, const int* ps, const int* pd, double* gdiag, double* goff) {
  gspx_ctx* ctx = g->ctx;
  const int64_t N = g->N;
  hipStream_t st = ctx->stream;
  for (int i = 0; i < 5; ++i) ctx->timing[i] = 0;
  ctx->step_kinds[0] = ctx->step_kinds[1] = 0;
  if (gdiag && N > 0) HIPCHK(hipMemsetAsync(gdiag, 0, (size_t)N * sizeof(double), st));
  if (goff && P > 0) HIPCHK(hipMemsetAsync(goff, 0, (size_t)P * sizeof(double), st));
  const bool wanted = (gdiag && N > 0) || (goff && P > 0);
  if (Nsig == 0 || N == 0 || !wanted) {
    HIPCHK(hipStreamSynchronize(st));
    return GSPX_OK;
  }
  // per signal: the M - 1 kept slots, the Nf cotangent planes in the internal order and the two Clenshaw panels
  int64_t width = 0;
  CHK(batch_width(g, sizeof(T), (size_t)(M - 1) + (size_t)Nf + 2, Nsig, &width));
  constexpr int64_t TVEC = 16 / (int64_t)sizeof(T);
  const int64_t widest = (std::min<int64_t>(width, Nsig) + TVEC - 1) / TVEC * TVEC;  // (a padded batch's pitch)
  CHK(ctx->ws_t.ensure((size_t)(M + 1) * (size_t)N * (size_t)widest * sizeof(T) + 1024));
  CHK(ctx->ws_w.ensure((size_t)M * Nf * sizeof(T) + 64));
  const std::vector<double> cp((size_t)M, 0.0);  // (the deferred plan uploads its filter's coefficients; none are read)
  CHK(ensure_factor<T>(g, lmax));
  return run_batches(g, Nsig, width, M - 1, [&](int64_t c0, unsigned ld, size_t& ev_idx) -> int {
    const LapGrad lg{g, z + c0, (unsigned)Nsig, (size_t)N * (size_t)Nsig, Nf, M, coeffs, ps, pd, P, 2.0 / lmax, gdiag, goff};
    const SlotsUse use{lap_grad_use<T>, &lg};
    return run_batch<T>(g, 1, M - 1, cp, x + c0, (unsigned)Nsig, (T*)nullptr, ld, ld, true, false, false, ev_idx, nullptr,
                        nullptr, nullptr, &use);
  });
}

extern "C" int gspx_cheby_laplacian_grad_dev(gspx_graph* g, double lmax, int Nf, int M, const double* coeffs,
                                             int64_t Nsig, const void* x_dev, const void* z_dev, int64_t n_pairs,
                                             const int32_t* src_dev, const int32_t* dst_dev, double* gdiag_dev,
                                             double* goff_dev, double* kernel_ms) {
  static const char* who = "gspx_cheby_laplacian_grad_dev";
  // (the scalar checks first: they need no graph, and so no device, to be exercised)
  if (M < 2 || M > 256) return set_err(GSPX_ERR_INVALID, "%s: 2 to 256 orders (got %d)", who, M);
  if (Nf < 1) return set_err(GSPX_ERR_INVALID, "Nf must be >= 1");
  if (Nsig < 0) return set_err(GSPX_ERR_INVALID, "negative number of signals");
  if (!(lmax > 0.0) || !std::isfinite(lmax))
    return set_err(GSPX_ERR_INVALID, "lmax must be positive and finite (got %g)", lmax);
  if ((src_dev == nullptr) != (dst_dev == nullptr))
    return set_err(GSPX_ERR_INVALID, "%s: sources and targets come together (both null: the graph's own edges)", who);
  if (src_dev && (n_pairs < 0 || n_pairs >= ((int64_t)1 << 31)))
    return set_err(GSPX_ERR_INVALID, "%s: 0 to 2^31 - 1 vertex couples (got %lld)", who, (long long)n_pairs);
  if (!coeffs) return set_err(GSPX_ERR_INVALID, "null coefficients");
  if (Nsig >= ((int64_t)1 << 31) / 16) return set_err(GSPX_ERR_INVALID, "too many signals");
  for (size_t i = 0; i < (size_t)Nf * M; ++i)
    if (!std::isfinite(coeffs[i])) return set_err(GSPX_ERR_INVALID, "non-finite coefficient");
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (Nsig > 0 && g->N > 0 && (!x_dev || !z_dev)) return set_err(GSPX_ERR_INVALID, "null signal pointer");
  gspx_ctx* ctx = g->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int* src = src_dev;
  const int* dst = dst_dev;
  int64_t P = n_pairs;
  if (!src_dev) {  // the graph's own list, the order of Graph.get_edge_list
    CHK(edges_for(g));
    P = g->n_edges;
    src = g->e_src.as<int>();
    dst = g->e_dst.as<int>();
  }
  // one pass over the list before any work: every vertex in range, no vertex twice; the internal order on the way
  // (in the context's grow-only partials workspace, which no kernel of this call uses: the flag, then the two lists -
  // no allocation per call in a training loop's backward pass)
  const int* ps = nullptr;
  const int* pd = nullptr;
  if (P > 0) {
    CHK(ctx->ws_sqp.ensure(256 + (size_t)2 * (size_t)P * sizeof(int)));
    int* flag = ctx->ws_sqp.as<int>();
    int* mapped = flag + 64;
    HIPCHK(hipMemsetAsync(flag, 0, sizeof(int), st));
    const unsigned nb = (unsigned)std::min<int64_t>((P + 255) / 256, 65536);
    hipLaunchKernelGGL(gspx::k_wgrad_map, dim3(nb), dim3(256), 0, st, src, dst, P, (int)g->N,
                       g->has_perm ? g->iperm.as<int>() : (const int*)nullptr, mapped, mapped + P, flag);
    int hbad = 0;
    HIPCHK(hipMemcpyAsync(&hbad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (hbad)
      return set_err(GSPX_ERR_INVALID, "%s: a vertex couple lies outside [0, N) or names one vertex twice", who);
    ps = mapped;
    pd = ps + P;
  }
  replay_reset(ctx);  // (the kept slots overwrite the panels a recorded filter call replays from)
  return device_call(g, Nsig, x_dev, nullptr, kernel_ms, [&](auto x, auto, int64_t n) {
    return laplacian_grad_dev_t(g, lmax, Nf, M, coeffs, n, x, (decltype(x))z_dev, P, ps, pd, gdiag_dev, goff_dev);
  });
}
