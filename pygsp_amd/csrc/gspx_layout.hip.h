// gspx_layout.hip.h - the spring layout (Fruchterman-Reingold) of a gspx_graph on the device.  After gspx_ops.hip.h
// (permute_panel) and gspx_graph.hip.h.
//
// What Graph.set_coordinates('spring') of the reference iterates on the host (pygsp/graphs/_layout.py:169-219,
// _sparse_fruchterman_reingold: a Python loop over the rows, one dense row of A and N x dim numpy temporaries per
// vertex, `iterations` times over), with A = (W > 0) read off the pattern that already lies on the device: the
// off-diagonal stored entries of the internal padded CSR (rptr / rcol, engine vertex order).  The values are never
// read, so fp32 and fp64 graphs run the same code; positions are fp64 either way.  Per iteration, with temperature t,
//   delta_j = pos_i - pos_j,  d_j = max(||delta_j||, 0.01)                                   (all j; j = i gives 0)
//   disp_i  = sum_j delta_j (k^2 / d_j^2 - A_ij d_j / k)      (i not fixed; fixed vertices keep disp = 0)
//   len_i   = ||disp_i||, replaced by 0.1 where < 0.01;  pos_i += disp_i t / len_i
// and every position is updated after all displacements are formed: positions are read from one buffer and written
// to the other (ping-pong), both in the internal vertex order (permuted in once, out once).
//
// Two launches per iteration, no grid barrier:
//   k_fr_repulse         all pairs: part[s][i][:] = sum over the j of split s of delta_j k^2 / max(|delta_j|^2, 1e-4)
//                        - no square root per pair, one reciprocal (v_rcp_f64 and two Newton steps: d^2 lies in
//                        [1e-4, O(1)], nothing to scale or fix up) and a dozen fp64 operations.  A 256-thread
//                        workgroup owns FR_IPT x 256 vertices i in registers and walks its j range in tiles of 256
//                        positions staged in LDS; every lane reads the same j, so the LDS reads are broadcasts (one
//                        ds_read per j and wave against 13 or 16 fp64 instructions per owned vertex: the LDS is idle
//                        next to the vector units, and unlike wave-uniform scalar loads the tile costs no SGPRs and does
//                        not depend on the compiler proving the index uniform).  grid.y splits the j range so that small
//                        N still fills the chip; every thread sums its j in ascending order.
//   k_fr_attract_update  one thread per vertex: the split partials in ascending split order, then the vertex's CSR
//                        row (diagonal, pads and out-of-range columns skipped; the one square root per stored entry,
//                        clamped at 0.01), the length rule and the step.  A fixed vertex copies its position.
// Every sum has one order, a function of N, the split count and the vertex order alone: no atomics, the same bits on
// every call.  The split count is a function of N and the CU count (layout_split_count), or the "layout_splits" option.
// There is no approximate repulsion (grid, Barnes-Hut): the contract is the reference's exact sum.
#pragma once

namespace gspx {

constexpr int FR_TILE = 256;  // j positions staged per pass (one per thread)
constexpr int FR_IPT = 2;     // vertices i a thread owns

// split s of grid.y takes j in [s * jlen, min(N, (s + 1) * jlen)); vertex i = blockIdx.x * FR_IPT * 256 + q * 256 + t
template <int DIM>
__global__ __launch_bounds__(256) void k_fr_repulse(const double* __restrict__ pos, int N, int jlen, double k2,
                                                    double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double tile[FR_TILE * DIM];
  const int t = threadIdx.x;
  const int i0 = blockIdx.x * (FR_IPT * 256) + t;
  double pi[FR_IPT][DIM], acc[FR_IPT][DIM];
#pragma unroll
  for (int q = 0; q < FR_IPT; ++q) {
    const int i = min(i0 + q * 256, N - 1);  // (a lane past the end works on the last vertex and stores nothing)
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      pi[q][c] = pos[(size_t)i * DIM + c];
      acc[q][c] = 0.0;
    }
  }
  const int jb = min((int)blockIdx.y * jlen, N), je = min(jb + jlen, N);
  for (int j0 = jb; j0 < je; j0 += FR_TILE) {
    const int cnt = min(FR_TILE, je - j0);
    __syncthreads();  // the previous tile has been read
    for (int e = t; e < cnt * DIM; e += 256) tile[e] = pos[(size_t)j0 * DIM + e];
    __syncthreads();
#pragma unroll 4
    for (int jj = 0; jj < cnt; ++jj) {
      double pj[DIM];
#pragma unroll
      for (int c = 0; c < DIM; ++c) pj[c] = tile[jj * DIM + c];
#pragma unroll
      for (int q = 0; q < FR_IPT; ++q) {
        double d[DIM], d2 = 0.0;
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
          d[c] = pi[q][c] - pj[c];
          d2 = fma(d[c], d[c], d2);
        }
        d2 = fmax(d2, 1e-4);
        double r = __builtin_amdgcn_rcp(d2);
        r = fma(fma(-d2, r, 1.0), r, r);
        r = fma(fma(-d2, r, 1.0), r, r);
        const double w = k2 * r;
#pragma unroll
        for (int c = 0; c < DIM; ++c) acc[q][c] = fma(d[c], w, acc[q][c]);
      }
    }
  }
  double* out = part + (size_t)blockIdx.y * N * DIM;
#pragma unroll
  for (int q = 0; q < FR_IPT; ++q) {
    const int i = i0 + q * 256;
    if (i < N)
#pragma unroll
      for (int c = 0; c < DIM; ++c) out[(size_t)i * DIM + c] = acc[q][c];
  }
}

// fixed: N uint8 in the caller's vertex order, or null
template <int DIM>
__global__ __launch_bounds__(256) void k_fr_attract_update(const int* __restrict__ rptr, const int* __restrict__ rcol,
                                                           const int* __restrict__ perm,
                                                           const unsigned char* __restrict__ fixed,
                                                           const double* __restrict__ part, int splits,
                                                           const double* __restrict__ pos, int N, double inv_k, double t,
                                                           double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double pi[DIM], disp[DIM];
#pragma unroll
  for (int c = 0; c < DIM; ++c) pi[c] = pos[(size_t)i * DIM + c];
  if (fixed && fixed[perm ? perm[i] : i]) {
#pragma unroll
    for (int c = 0; c < DIM; ++c) out[(size_t)i * DIM + c] = pi[c];
    return;
  }
#pragma unroll
  for (int c = 0; c < DIM; ++c) disp[c] = 0.0;
  for (int s = 0; s < splits; ++s)
#pragma unroll
    for (int c = 0; c < DIM; ++c) disp[c] += part[((size_t)s * N + i) * DIM + c];
  for (int e = rptr[i] & ~3, e1 = rptr[i + 1] & ~3; e < e1; ++e) {
    const int j = rcol[e];
    if (j == i || (unsigned)j >= (unsigned)N) continue;  // the diagonal slot, the pads closing the row
    double d[DIM], d2 = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      d[c] = pi[c] - pos[(size_t)j * DIM + c];
      d2 = fma(d[c], d[c], d2);
    }
    const double w = fmax(sqrt(d2), 0.01) * inv_k;
#pragma unroll
    for (int c = 0; c < DIM; ++c) disp[c] = fma(-d[c], w, disp[c]);
  }
  double l2 = 0.0;
#pragma unroll
  for (int c = 0; c < DIM; ++c) l2 = fma(disp[c], disp[c], l2);
  double len = sqrt(l2);
  if (len < 0.01) len = 0.1;
  const double f = t / len;
#pragma unroll
  for (int c = 0; c < DIM; ++c) out[(size_t)i * DIM + c] = fma(disp[c], f, pi[c]);
}

}  // namespace gspx

// how many ways the j range is split: about four workgroups per CU in all (four waves per SIMD: enough to keep the
// vector units issuing, profiles/layout.md; the 52 / 60 registers of the kernel would admit eight), at least 64 j per
// split, at most grid.y's 65535; the option forces it (clamped to 1 .. N)
static int layout_split_count(const gspx_ctx* ctx, int64_t N) {
  if (N <= 0) return 1;
  const int64_t cap = std::min<int64_t>(N, 65535);
  if (ctx->opt.layout_splits > 0) return (int)std::min<int64_t>(ctx->opt.layout_splits, cap);
  const int64_t nbx = (N + gspx::FR_IPT * 256 - 1) / (gspx::FR_IPT * 256);
  const int64_t want = ((int64_t)4 * ctx->cu_count + nbx - 1) / nbx;
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, (N + 63) / 64), cap));
}

extern "C" int gspx_layout_splits(gspx_graph* g, int64_t* splits) {
  if (!g || !splits) return set_err(GSPX_ERR_INVALID, "null graph or null output");
  *splits = layout_split_count(g->ctx, g->N);
  return GSPX_OK;
}

template <int DIM>
static void layout_launch_iteration(gspx_graph* g, const int* perm, const unsigned char* fixed, int splits, int jlen,
                                    double k, double t, const double* in, double* out, double* part) {
  const int N = (int)g->N;
  hipStream_t st = g->ctx->stream;
  const unsigned nbx = (unsigned)((N + gspx::FR_IPT * 256 - 1) / (gspx::FR_IPT * 256));
  hipLaunchKernelGGL((gspx::k_fr_repulse<DIM>), dim3(nbx, (unsigned)splits), dim3(256), 0, st, in, N, jlen, k * k, part);
  hipLaunchKernelGGL((gspx::k_fr_attract_update<DIM>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st,
                     g->rptr.as<int>(), g->rcol.as<int>(), perm, fixed, part, splits, in, N, 1.0 / k, t, out);
}

extern "C" int gspx_layout_spring_dev(gspx_graph* g, int dim, double k, const void* fixed_dev, int64_t iterations,
                                      double t0, double dt, void* pos_dev, double* kernel_ms) {
  if (g) replay_reset(g->ctx);
  if (kernel_ms) *kernel_ms = 0;
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (dim != 2 && dim != 3) return set_err(GSPX_ERR_INVALID, "layout_spring: dim must be 2 or 3, got %d", dim);
  if (!(k > 0) || !std::isfinite(k)) return set_err(GSPX_ERR_INVALID, "layout_spring: k must be positive and finite");
  if (iterations < 0) return set_err(GSPX_ERR_INVALID, "layout_spring: negative number of iterations");
  if (!std::isfinite(t0) || !std::isfinite(dt)) return set_err(GSPX_ERR_INVALID, "layout_spring: t0 and dt must be finite");
  const int64_t N = g->N;
  if (N == 0 || iterations == 0) return GSPX_OK;
  if (N > ((int64_t)1 << 29)) return set_err(GSPX_ERR_INVALID, "layout_spring: more than 2^29 vertices");
  if (!pos_dev) return set_err(GSPX_ERR_INVALID, "layout_spring: null positions");
  gspx_ctx* ctx = g->ctx;
  hipStream_t st = ctx->stream;
  HIPCHK(hipSetDevice(ctx->device));
  const int splits = layout_split_count(ctx, N);
  const int jlen = (int)((N + splits - 1) / splits);
  // two position buffers and the split partials, 256-byte aligned, in the context's workspace
  const size_t pb = ((size_t)N * dim * sizeof(double) + 255) & ~(size_t)255;
  const size_t total = (2 + (size_t)splits) * pb;
  if (total > ((size_t)std::max<int64_t>(ctx->opt.ws_limit_mb, 1) << 20))
    return set_err(GSPX_ERR_INVALID, "layout_spring: %d splits of %lld vertices need %zu MiB of workspace (raise "
                   "ws_limit_mb or set layout_splits)", splits, (long long)N, total >> 20);
  CHK(ctx->ws_t.ensure(total));
  char* base = ctx->ws_t.as<char>();
  double* P[2] = {(double*)base, (double*)(base + pb)};
  double* part = (double*)(base + 2 * pb);  // [splits][N][dim], contiguous
  const int* perm = g->has_perm ? g->perm.as<int>() : nullptr;
  const int* iperm = g->has_perm ? g->iperm.as<int>() : nullptr;
  const unsigned char* fixed = (const unsigned char*)fixed_dev;
  double* pos = (double*)pos_dev;
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  CHK(permute_panel<double>(g, pos, (unsigned)dim, P[0], (unsigned)dim, perm));
  double t = t0;
  for (int64_t it = 0; it < iterations; ++it) {
    if (dim == 2) layout_launch_iteration<2>(g, perm, fixed, splits, jlen, k, t, P[it & 1], P[(it + 1) & 1], part);
    else layout_launch_iteration<3>(g, perm, fixed, splits, jlen, k, t, P[it & 1], P[(it + 1) & 1], part);
    t -= dt;  // the reference's own arithmetic (_layout.py:217), not t0 - it * dt
  }
  HIPCHK(hipGetLastError());
  CHK(permute_panel<double>(g, P[iterations & 1], (unsigned)dim, pos, (unsigned)dim, iperm));
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  return finish_timed(ctx, kernel_ms);
}
