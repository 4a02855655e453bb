// gspx_knn_bf.hip.h - k nearest neighbours in MORE than three dimensions (NNGraph on feature / patch clouds,
// pygsp/graphs/nngraphs/nngraph.py:213-226, nngraphs/imgpatches.py): tiled brute force with the pair
// distances on the matrix cores.  Included by gspx_knn.hip.h (uses its KD-tree arithmetic helpers).
//
// A uniform grid stops paying beyond three dimensions (a KD-tree degrades the same way), while all pair
// distances of a point block are ONE dense contraction,  |x - y|^2 = |x|^2 + |y|^2 - 2 x.y  - the one place
// of the path's surroundings where a dense panel product is the natural formulation, so it runs on MFMA
// (v_mfma_f64_16x16x4f64: a 16 x 16 tile of dot products per instruction, fp64 because the selection below
// must not lose a true neighbour to rounding).  Four stages:
//   1. k_bf_prepare   points -> MFMA operand order (per 16-point tile and 4 dimensions: one coalesced 512-byte
//                     line, lane l = point l % 16, dimension l / 16), squared norms
//   2. k_bf_exact<0>  per query an UPPER BOUND tau of its k-th neighbour distance: the exact k-th smallest
//                     squared distance to a strided sample of M points (a subset's order statistics bound the
//                     full set's from above)
//   3. k_bf_collect   MFMA sweep of every 64-query block over the points: every pair whose approximate squared
//                     distance is <= tau (+ a rounding margin) is appended to the query's candidate list.  Two
//                     sweeps: a strided subset of sqrt(N M) points, then - after k_bf_exact<1> tightened every bound to the
//                     exact k-th smallest of the candidates so far - the rest: k (N1 / M + N / N1) entries per query
//   4. k_bf_exact<2>  candidates re-evaluated in the KD-tree's own arithmetic (knn_sqdist: per-dimension
//                     differences, no fused multiply-add; correctly rounded square root) and the k smallest by
//                     (distance, index) kept - so neighbours and distances equal scipy's bit for bit, exactly
//                     like the grid search in 1-3 dimensions.  A query whose list overflowed (heavy ties /
//                     duplicates) scans all points exactly instead.
// Other metrics (manhattan, max_dist) have no product form: every query takes the exact scan of stage 4.
//
// Up to 64 dimensions the query lives in registers (stages 2 and 4: q[4 DT] per thread; stage 3: the operands of a
// wave's 64 queries), DT a template constant in {4, 8, 16}.  From 65 to 4096 dimensions (learned embeddings, 5 x 5 RGB
// patches) the same plan runs on a second set of kernels, chosen by d > 64 alone: k_bf_collect_wide loops over the
// dimension at run time with the accumulators in registers, k_bf_exact_wide / k_bf_radius_wide serve one query per
// wave with its row in LDS.  No wide kernel holds a row in a per-thread array (see knn_sqdist_reg for why).
#pragma once

namespace gspx {

typedef double bf_d4 __attribute__((ext_vector_type(4)));

// knn_sqdist / knn_key (the KD-tree's arithmetic, gspx_knn.hip.h) with the query in REGISTERS: q is indexed with
// compile-time constants only (4 DT >= d values, fully unrolled, the real dimension d guards each block), so it
// never goes to scratch memory - the runtime-indexed q[64] of the first version did, and a scratch read per
// multiply made these kernels several times slower than their arithmetic.
template <int DT>
__device__ __forceinline__ double knn_sqdist_reg(const double (&q)[4 * DT], const double* __restrict__ p, int d) {
#pragma clang fp contract(off)
  double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
  for (int b = 0; b < DT; ++b)
    if (4 * b + 4 <= d) {
      const double d0 = q[4 * b] - p[4 * b], d1 = q[4 * b + 1] - p[4 * b + 1], d2 = q[4 * b + 2] - p[4 * b + 2],
                   d3 = q[4 * b + 3] - p[4 * b + 3];
      const double s0 = d0 * d0, s1 = d1 * d1, s2 = d2 * d2, s3 = d3 * d3;
      a0 = a0 + s0;
      a1 = a1 + s1;
      a2 = a2 + s2;
      a3 = a3 + s3;
    }
  double s = ((a0 + a1) + a2) + a3;
#pragma unroll
  for (int b = 0; b < DT; ++b)
    if (4 * b < d && 4 * b + 4 > d) {  // the block that holds the last d % 4 dimensions
#pragma unroll
      for (int r = 0; r < 3; ++r)
        if (4 * b + r < d) {
          const double df = q[4 * b + r] - p[4 * b + r];
          const double sq = df * df;
          s = s + sq;
        }
    }
  return s;
}
template <int DT>
__device__ __forceinline__ double knn_key_reg(const double (&q)[4 * DT], const double* __restrict__ p, int d, int metric) {
  if (metric == 0) return knn_sqdist_reg<DT>(q, p, d);
  double s = 0;
#pragma unroll
  for (int j = 0; j < 4 * DT; ++j)
    if (j < d) {
      const double a = fabs(q[j] - p[j]);
      s = metric == 1 ? s + a : fmax(s, a);
    }
  return s;
}
template <int DT> __device__ __forceinline__ void bf_load_query(double (&q)[4 * DT], const double* __restrict__ row, int d) {
#pragma unroll
  for (int j = 0; j < 4 * DT; ++j) q[j] = j < d ? row[j] : 0.0;
}

// X (N x d, row major) -> Xop[tile][t][lane] = X[16 tile + (lane & 15)][4 t + (lane >> 4)] (zero beyond N / d),
// norm[i] = sum_j x_ij^2 (padded to whole tiles with 1e300)
__global__ void k_bf_prepare(const double* __restrict__ x, int N, int d, int DT, double* __restrict__ xop,
                             double* __restrict__ norm, float* __restrict__ xop32) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)((N + 15) / 16) * DT * 64;
  if (gid < total) {
    const int lane = (int)(gid & 63);
    const long long tt = gid >> 6;
    const int t = (int)(tt % DT);
    const long long tile = tt / DT;
    const long long p = tile * 16 + (lane & 15);
    const int j = 4 * t + (lane >> 4);
    const double v = (p < N && j < d) ? x[p * d + j] : 0.0;
    xop[gid] = v;
    if (xop32) xop32[gid] = (float)v;  // operands of the fp32 sweep (the bound's margin covers their rounding)
  }
  if (gid < N) {
    double s = 0;
    for (int j = 0; j < d; ++j) s += x[gid * d + j] * x[gid * d + j];
    norm[gid] = s;
  } else if (gid < (long long)((N + 15) / 16) * 16) {
    norm[gid] = 1e300;  // the padding points of the last tile are infinitely far away
  }
}

// The three exact stages of the plan up to 64 dimensions, one thread per query with the query and its list of the
// KMAX best (knn_best_*, gspx_knn.hip.h) in registers.  All of them evaluate candidates in the KD-tree's arithmetic:
//   WHAT 0  tau[i] = the k-th smallest key (squared euclidean distance) from point i to the sample {0, stride,
//           2 stride, ...} without i itself: an upper bound of its k-th neighbour's key
//   WHAT 1  between the two sweeps: the exact k-th smallest key among the query's candidates so far (all from the first
//           point range) is a tighter bound than the sample gave; tau[i] only ever goes down
//   WHAT 2  the candidates (or every point, when the list overflowed / holds fewer than k / no list was made)
//           evaluated in the caller's metric and the k smallest by (key, index) written, nearest first
// Stages 0 and 1 keep keys alone and are euclidean only (knn_sqdist_reg); stage 2 keeps indices and goes through
// knn_key_reg.  A stage reads only its own arguments: 0 - stride, tau; 1 - cap, cnt, buf, tau; 2 - metric, cap, cnt
// (nullable), buf, nn, dist, n_scans.  k_bf_exact_wide<WHAT> is the same beyond 64 dimensions.
template <int WHAT, int KMAX, int DT>
__global__ __launch_bounds__(128) void k_bf_exact(const double* __restrict__ x, int N, int d, int k, int metric,
                                                  int stride, int cap, const int* __restrict__ cnt,
                                                  const int* __restrict__ buf, double* __restrict__ tau,
                                                  int* __restrict__ nn, double* __restrict__ dist,
                                                  int* __restrict__ n_scans) {
  const int i = blockIdx.x * 128 + threadIdx.x;
  if (i >= N) return;
  double q[4 * DT];
  bf_load_query<DT>(q, x + (size_t)i * d, d);
  constexpr bool IDX = WHAT == 2;
  double bd[KMAX];
  int bi[IDX ? KMAX : 1];  // (stages 0 and 1 carry no indices: never touched)
  if constexpr (IDX) knn_best_init<KMAX>(bd, bi);
  else knn_best_init<KMAX>(bd);
  // the candidates: a = 0, inc, 2 inc, ... below n, each either a point itself or a slot of the query's list
  bool scan = false;
  int n = N, inc = 1;
  if constexpr (WHAT == 0) {
    inc = stride;
  } else if constexpr (WHAT == 1) {
    n = min(cnt[i], cap);
  } else {
    const int have = cnt ? cnt[i] : -1;
    scan = have < 0 || have > cap || have < k;
    n = scan ? N : have;
    if (scan && cnt) atomicAdd(n_scans, 1);
  }
  for (int a = 0; a < n; a += inc) {
    const int idx = (WHAT == 0 || scan) ? a : buf[(size_t)i * cap + a];
    if (idx == i) continue;
    const double* p = x + (size_t)idx * d;
    if constexpr (IDX) knn_best_insert<KMAX>(bd, bi, knn_key_reg<DT>(q, p, d, metric), idx);
    else knn_best_insert<KMAX>(bd, knn_sqdist_reg<DT>(q, p, d));
  }
  if constexpr (IDX) {
#pragma unroll
    for (int t = 0; t < KMAX; ++t)
      if (t < k) {
        nn[(size_t)i * k + t] = bi[t];
        dist[(size_t)i * k + t] = metric == 0 ? knn_sqrt(bd[t]) : bd[t];
      }
  } else {
    const double kth = knn_best_kth<KMAX>(bd, k);
    if (WHAT == 0 || kth < tau[i]) tau[i] = kth;
  }
}

// candidate lists: either N fixed-capacity rows (off == null; cap == 0: count only), or rows of their own lengths
// (off[q] .. off[q + 1], from a counting sweep: the radius search, whose neighbourhoods have no common bound)
__device__ __forceinline__ void bf_append(const int* __restrict__ off, int cap, int q, int slot, int c,
                                          int* __restrict__ buf) {
  if (off) {
    const int lo = off[q];
    if (slot < off[q + 1] - lo) buf[(size_t)lo + slot] = c;
  } else if (slot < cap) {
    buf[(size_t)q * cap + slot] = c;
  }
}

// ---- what the narrow (d <= 64) and the wide (d > 64) sweep share ---------------------------------------------------
// F = double: v_mfma_f64_16x16x4f64.  F = float: v_mfma_f32_16x16x4f32 at twice the rate - the sweep only has to
// admit a SUPERSET of the true neighbours (the exact stage decides in the KD-tree's arithmetic), so single precision
// does when its rounding margin, (4 DT + 8) 2^-24 (|x|^2 + |y|^2), is small against the bounds (the caller checks);
// the bound is rounded up and the point's norm down, towards admitting.
typedef float bf_f4 __attribute__((ext_vector_type(4)));
template <typename F> struct bf_mfma {
  static constexpr bool F32 = sizeof(F) == 4;
  typedef typename std::conditional<F32, bf_f4, bf_d4>::type acc_t;
  static __device__ __forceinline__ acc_t mac(F a, F b, acc_t c) {
    if constexpr (F32) return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
};
// the query behind element e of this lane's result of query tile qt: rows kq + 4 e of the tile in the fp64 product's
// result layout, rows 4 kq + e in the fp32 one's
template <typename F> __device__ __forceinline__ int bf_query_of(int q0, int kq, int qt, int e) {
  return q0 + 16 * qt + (bf_mfma<F>::F32 ? 4 * kq + e : kq + 4 * e);
}
// this lane's 16 bounds: tau minus the query's own norm (what is compared is |y|^2 - 2 x.y), with the rounding
// margin of the product form; queries beyond N admit nothing
template <typename F>
__device__ __forceinline__ void bf_limits(F (&lim)[4][4], const double* __restrict__ norm, const double* __restrict__ tau,
                                          int N, int q0, int kq, double margin_scale, double norm_max) {
  constexpr bool F32 = bf_mfma<F>::F32;
#pragma unroll
  for (int qt = 0; qt < 4; ++qt)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = bf_query_of<F>(q0, kq, qt, e);
      if (q < N) {
        const double nq = norm[q];
        const double l = tau[q] - nq + margin_scale * (nq + norm_max);
        if constexpr (F32) lim[qt][e] = __double2float_ru(l);
        else lim[qt][e] = l;
      } else {
        lim[qt][e] = F32 ? F(-3e38) : F(-1e300);
      }
    }
}
// a point's norm as the sweep compares it (the padding points' 1e300 stays "infinitely far" in single precision)
template <typename F> __device__ __forceinline__ F bf_norm_of(const double* __restrict__ norm, int i) {
  const double v = norm[i];
  if constexpr (bf_mfma<F>::F32) return v > 3e38 ? 3e38f : __double2float_rd(v);
  else return v;
}
// the j-th point tile of a sweep: phase 0 takes every step-th tile (a strided subset of the cloud: a fair sample
// whatever order the points come in), phase 1 the tiles in between
__device__ __forceinline__ int bf_tile_of(int phase, int step, int j) {
  return phase == 0 ? j * step : (j / (step - 1)) * step + 1 + j % (step - 1);
}
// The 16 (query, point) tests of a lane for one point tile (acc: the four query tiles' products with it, nc: the
// point's norm), folded into one mask: a single wave-wide branch per tile guards the rare appends.  (The point itself
// is not filtered here: the exact stages skip it.)  Hits are parked in the wave's LDS queue ((query << 32) | point, 128
// slots) and appended 64 at a time: an append is an atomic (whose return the wave must wait for) plus a scattered
// store, and about 60 % of the tiles hit something - appending on the spot stalled the wave a memory round trip per
// tile.  queued is wave-uniform.
template <typename F>
__device__ __forceinline__ void bf_test_tile(const typename bf_mfma<F>::acc_t (&acc)[4], F nc, const F (&lim)[4][4], int ct,
                                             int q0, int lane, unsigned long long lt_mask,
                                             volatile unsigned long long* queue, int& queued, const int* __restrict__ off, int cap, int* __restrict__ cnt,
                                             int* __restrict__ buf) {
  const int kq = lane >> 4, cq = lane & 15;
  // D layout: lane (kq, cq) holds query rows kq + 4 e (fp64) / 4 kq + e (fp32), point column cq
  // (the tests are folded with a scalar OR of the compare masks: two vector instructions per pair)
  bool any = false;
#pragma unroll
  for (int qt = 0; qt < 4; ++qt)
#pragma unroll
    for (int e = 0; e < 4; ++e) any |= nc - F(2) * acc[qt][e] <= lim[qt][e];
  if (__builtin_amdgcn_ballot_w64(any) != 0) {
    const int c = ct * 16 + cq;
#pragma unroll
    for (int qt = 0; qt < 4; ++qt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool hit = nc - F(2) * acc[qt][e] <= lim[qt][e];
        const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
        if (m != 0) {
          if (hit) {
            const int pos = queued + __popcll(m & lt_mask);
            queue[pos] = ((unsigned long long)(unsigned)bf_query_of<F>(q0, kq, qt, e) << 32) | (unsigned)c;
          }
          queued += __popcll(m);
          if (queued >= 64) {  // at most 127 parked: room for one more round of 64
            __builtin_amdgcn_wave_barrier();
            const unsigned long long it = queue[lane];
            const int iq = (int)(it >> 32), ic = (int)(unsigned)it;
            const int slot = atomicAdd(&cnt[iq], 1);
            bf_append(off, cap, iq, slot, ic, buf);
            const int rest = queued - 64;
            unsigned long long mv = 0;
            if (lane < rest) mv = queue[64 + lane];
            __builtin_amdgcn_wave_barrier();
            if (lane < rest) queue[lane] = mv;
            __builtin_amdgcn_wave_barrier();
            queued = rest;
          }
        }
      }
  }
}
// what is still parked when the sweep ends
__device__ __forceinline__ void bf_flush(int lane, volatile unsigned long long* queue, int queued,
                                         const int* __restrict__ off, int cap, int* __restrict__ cnt,
                                         int* __restrict__ buf) {
  __builtin_amdgcn_wave_barrier();
  if (lane < queued) {
    const unsigned long long it = queue[lane];
    const int iq = (int)(it >> 32), ic = (int)(unsigned)it;
    const int slot = atomicAdd(&cnt[iq], 1);
    bf_append(off, cap, iq, slot, ic, buf);
  }
}

// One wave = 64 queries (four 16-query tiles, their operands in registers), sweeping all point tiles: 4 x DT
// MFMAs per point tile, then 16 (query, point) pairs per lane are tested against the query's bound.
template <int DT, typename F>
__global__ __launch_bounds__(256) void k_bf_collect(const F* __restrict__ xop, const double* __restrict__ norm,
                                                    const double* __restrict__ tau, int N, int phase, int step,
                                                    int count, double margin_scale, double norm_max, int cap,
                                                    const int* __restrict__ off, int* __restrict__ cnt,
                                                    int* __restrict__ buf) {
  const int lane = threadIdx.x & 63, kq = lane >> 4, cq = lane & 15;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int q0 = wave * 64;
  if (q0 >= N) return;
  typedef typename bf_mfma<F>::acc_t acc_t;
  const int ntiles = (N + 15) / 16;
  F a[4][DT];
#pragma unroll
  for (int qt = 0; qt < 4; ++qt) {
    const long long tile = (long long)(q0 / 16 + qt);
#pragma unroll
    for (int t = 0; t < DT; ++t) a[qt][t] = tile < ntiles ? xop[(tile * DT + t) * 64 + lane] : F(0);
  }
  F lim[4][4];
  bf_limits<F>(lim, norm, tau, N, q0, kq, margin_scale, norm_max);
  // Software pipeline: a tile's operands AND its norms are loaded one tile ahead, so no load issued in an
  // iteration is waited for in that iteration (the first version loaded the norm at the top of the tile and
  // paid an L2 round trip per tile: the matrix cores idled two thirds of the time).  The four query tiles'
  // product chains are interleaved (four independent accumulators in flight, no stall on a chain's own result).
  __shared__ unsigned long long queue_all[4][128];
  volatile unsigned long long* queue = queue_all[threadIdx.x >> 6];
  const unsigned long long lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));  // the lanes before this one
  int queued = 0;  // wave-uniform
  F b[DT], b_next[DT], n_next;
  int ct_next = bf_tile_of(phase, step, 0);
  {
    n_next = bf_norm_of<F>(norm, ct_next * 16 + cq);
#pragma unroll
    for (int t = 0; t < DT; ++t) b_next[t] = xop[((long long)ct_next * DT + t) * 64 + lane];
  }
  for (int j = 0; j < count; ++j) {
    const int ct = ct_next;
    const F nc = n_next;
#pragma unroll
    for (int t = 0; t < DT; ++t) b[t] = b_next[t];
    if (j + 1 < count) {
      ct_next = bf_tile_of(phase, step, j + 1);
      n_next = bf_norm_of<F>(norm, ct_next * 16 + cq);  // (padded: no bounds test between the load and its use a tile later)
#pragma unroll
      for (int t = 0; t < DT; ++t) b_next[t] = xop[((long long)ct_next * DT + t) * 64 + lane];
    }
    acc_t acc[4];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) acc[qt] = acc_t{0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int qt = 0; qt < 4; ++qt) acc[qt] = bf_mfma<F>::mac(a[qt][t], b[t], acc[qt]);
    bf_test_tile<F>(acc, nc, lim, ct, q0, lane, lt_mask, queue, queued, off, cap, cnt, buf);
  }
  bf_flush(lane, queue, queued, off, cap, cnt, buf);
}

// The sweep in more than 64 dimensions: the dimension is a run-time loop over 4-column MFMA steps (DT = ceil(d / 4)
// of them), so neither the 64 queries' operands nor a point tile's fit in registers.  A wave keeps the ACCUMULATORS
// there instead - 4 query tiles x 4 point tiles, 16 independent product chains across the whole dimension loop -, so
// every operand it reads feeds four MFMAs.  The four waves of a workgroup (256 queries) sweep the same four point tiles:
// their operands go through LDS, BF_WS steps at a time (each wave loads one tile's share, double buffered: one
// barrier per 16 BF_WS MFMAs of a wave); the queries' operands stream from xop for every group (already in operand
// order: one coalesced line per load; from the L2 while the array fits it, profiles/knn_wide.md).  Bounds, tests, hit
// queue, norm pipelining (a group ahead) and tile order are the narrow kernel's.
constexpr int BF_WS = 4;
template <typename F>
__global__ __launch_bounds__(256) void k_bf_collect_wide(const F* __restrict__ xop, const double* __restrict__ norm,
                                                         const double* __restrict__ tau, int N, int DT, int phase,
                                                         int step, int count, double margin_scale, double norm_max,
                                                         int cap, const int* __restrict__ off, int* __restrict__ cnt,
                                                         int* __restrict__ buf) {
  if (count <= 0) return;
  const int lane = threadIdx.x & 63, kq = lane >> 4, cq = lane & 15, w = threadIdx.x >> 6;
  const int q0 = (blockIdx.x * 4 + w) * 64;  // (a wave beyond N stays for the barriers: its bounds admit nothing)
  typedef typename bf_mfma<F>::acc_t acc_t;
  const int ntiles = (N + 15) / 16;
  const F* ap[4];
#pragma unroll
  for (int qt = 0; qt < 4; ++qt) ap[qt] = xop + (long long)min(q0 / 16 + qt, ntiles - 1) * DT * 64 + lane;
  F lim[4][4];
  bf_limits<F>(lim, norm, tau, N, q0, kq, margin_scale, norm_max);
  __shared__ unsigned long long queue_all[4][128];
  __shared__ F bs[2][4][BF_WS][64];
  volatile unsigned long long* queue = queue_all[w];
  const unsigned long long lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  int queued = 0;  // wave-uniform
  const int nchunks = (DT + BF_WS - 1) / BF_WS, ngroups = (count + 3) / 4;
  // this wave's share of a chunk's point operands: tile 4 g + w of the sweep (the last group repeats the last
  // tile: finite operands, and a norm that admits nothing), steps BF_WS c .. + BF_WS (zero beyond DT)
  auto stage = [&](int g, int c, F (&r)[BF_WS]) {
    const F* bp = xop + (long long)bf_tile_of(phase, step, min(4 * g + w, count - 1)) * DT * 64 + lane;
#pragma unroll
    for (int s = 0; s < BF_WS; ++s) r[s] = BF_WS * c + s < DT ? bp[(long long)(BF_WS * c + s) * 64] : F(0);
  };
  auto norms = [&](int g, F (&n)[4]) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
      n[p] = 4 * g + p < count ? bf_norm_of<F>(norm, bf_tile_of(phase, step, 4 * g + p) * 16 + cq)
                               : (bf_mfma<F>::F32 ? F(3e38) : F(1e300));
  };
  F r[BF_WS], nc[4], n_next[4];
  stage(0, 0, r);
  norms(0, n_next);
#pragma unroll
  for (int s = 0; s < BF_WS; ++s) bs[0][w][s][lane] = r[s];
  __syncthreads();
  acc_t acc[4][4];  // [point tile][query tile]
  int it = 0;
  for (int g = 0; g < ngroups; ++g) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      nc[p] = n_next[p];
#pragma unroll
      for (int qt = 0; qt < 4; ++qt) acc[p][qt] = acc_t{0, 0, 0, 0};
    }
    if (g + 1 < ngroups) norms(g + 1, n_next);  // a group ahead: not waited for in this group
    for (int c = 0; c < nchunks; ++c, ++it) {
      const bool more = c + 1 < nchunks || g + 1 < ngroups;
      if (more) stage(c + 1 < nchunks ? g : g + 1, c + 1 < nchunks ? c + 1 : 0, r);
      const int cur = it & 1;
#pragma unroll
      for (int s = 0; s < BF_WS; ++s) {
        const long long t = min(BF_WS * c + s, DT - 1);  // (beyond DT the point operands are zero)
        F a[4], b[4];
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) a[qt] = ap[qt][t * 64];
#pragma unroll
        for (int p = 0; p < 4; ++p) b[p] = bs[cur][p][s][lane];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int qt = 0; qt < 4; ++qt) acc[p][qt] = bf_mfma<F>::mac(a[qt], b[p], acc[p][qt]);
      }
      if (more) {
#pragma unroll
        for (int s = 0; s < BF_WS; ++s) bs[cur ^ 1][w][s][lane] = r[s];
      }
      __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
      bf_test_tile<F>(acc[p], nc[p], lim, bf_tile_of(phase, step, min(4 * g + p, count - 1)), q0, lane, lt_mask, queue, queued,
                      off, cap, cnt, buf);
  }
  bf_flush(lane, queue, queued, off, cap, cnt, buf);
}

// ---- exact evaluation in more than 64 dimensions --------------------------------------------------------------
// A query row of that width in a per-thread array would live in scratch memory (see knn_sqdist_reg), so here ONE WAVE
// serves a query: the row is staged once in LDS (d doubles; every lane reads the same word: a broadcast), the lanes take
// different candidates - each key is still computed by one thread, in the KD-tree's order (knn_key) - and the best 64
// by (key, index) are kept sorted ACROSS the wave, lane t holding the t-th: no per-thread list either, and one build
// for every k <= 64.
struct bf_best {
  double d;
  int i;
};
// the wave's candidates of one round (cd / ci per lane, live: this lane has one) merged into the sorted list: only
// those below the k-th entry (rare once the list has settled) are inserted, one at a time, by a shift across lanes
__device__ __forceinline__ void bf_wave_merge(bf_best& best, double cd, int ci, bool live, int k, int lane) {
  const double td = __shfl(best.d, k - 1);
  const int ti = __shfl(best.i, k - 1);
  unsigned long long m = __builtin_amdgcn_ballot_w64(live && (cd < td || (cd == td && ci < ti)));
  while (m != 0) {  // wave-uniform
    const int src = __builtin_ctzll(m);
    m &= m - 1;
    const double vd = __shfl(cd, src);
    const int vi = __shfl(ci, src);
    const unsigned long long after = __builtin_amdgcn_ballot_w64(vd < best.d || (vd == best.d && vi < best.i));
    const double pd = __shfl_up(best.d, 1);
    const int pi = __shfl_up(best.i, 1);
    if (after != 0) {  // the entries from the first larger one on move up a lane (the 64th drops out)
      const int pos = __builtin_ctzll(after);
      if (lane > pos) best.d = pd, best.i = pi;
      else if (lane == pos) best.d = vd, best.i = vi;
    }
  }
}
__device__ __forceinline__ void bf_stage_query(double* qs, const double* __restrict__ row, int d, int lane) {
  for (int j = lane; j < d; j += 64) qs[j] = row[j];
  __syncthreads();  // (a one-wave workgroup)
}
// WHAT as in k_bf_exact - 0: the sample bounds (candidates: the strided sample), 1: their refinement (the candidates
// so far), 2: the selection (the candidates, or every point).  One 64-thread workgroup per query; dynamic LDS: d
// doubles.
template <int WHAT>
__global__ __launch_bounds__(64) void k_bf_exact_wide(const double* __restrict__ x, int N, int d, int k, int metric,
                                                      int stride, int cap, const int* __restrict__ cnt,
                                                      const int* __restrict__ buf, double* __restrict__ tau,
                                                      int* __restrict__ nn, double* __restrict__ dist,
                                                      int* __restrict__ n_scans) {
  extern __shared__ double bf_qs[];
  const int i = blockIdx.x, lane = threadIdx.x;
  bf_stage_query(bf_qs, x + (size_t)i * d, d, lane);
  bf_best best{1e300, 0x7fffffff};
  bool scan = false;
  int n;
  if (WHAT == 0) {
    n = (N + stride - 1) / stride;
  } else if (WHAT == 1) {
    n = min(cnt[i], cap);
  } else {
    const int have = cnt ? cnt[i] : -1;
    scan = have < 0 || have > cap || have < k;
    n = scan ? N : have;
    if (scan && cnt && lane == 0) atomicAdd(n_scans, 1);
  }
  for (int base = 0; base < n; base += 64) {
    const int a = base + lane;
    int idx = 0x7fffffff;
    if (a < n) idx = WHAT == 0 ? a * stride : (scan ? a : buf[(size_t)i * cap + a]);
    const bool live = a < n && idx != i;
    double cd = 1e300;
    if (live) cd = knn_key(bf_qs, x + (size_t)idx * d, d, WHAT == 2 ? metric : 0);
    bf_wave_merge(best, cd, idx, live, k, lane);
  }
  if (WHAT == 2) {
    if (lane < k) {
      nn[(size_t)i * k + lane] = best.i;
      dist[(size_t)i * k + lane] = metric == 0 ? knn_sqrt(best.d) : best.d;
    }
  } else if (lane == k - 1) {
    if (WHAT == 0 || best.d < tau[i]) tau[i] = best.d;
  }
}

}  // namespace gspx

// The exact stage WHAT (0 the sample bounds, 1 their refinement between the sweeps, 2 the selection): up to 64
// dimensions the build of k_bf_exact for k <= 8 / 16 / 32 / 64 and d <= 16 / 32 / 64 (36 builds), one thread per query;
// beyond, k_bf_exact_wide, one wave per query with its row in LDS and one build for every k.  The kernels share one
// argument list (what a stage does not read may be null / 0).
template <int WHAT, int KMAX> static auto bf_exact_kernel(int d) {
  return d <= 16 ? gspx::k_bf_exact<WHAT, KMAX, 4>
                 : (d <= 32 ? gspx::k_bf_exact<WHAT, KMAX, 8> : gspx::k_bf_exact<WHAT, KMAX, 16>);
}
template <int WHAT>
static void launch_bf(gspx_ctx* ctx, const double* x, int N, int d, int k, int metric, int stride, double* tau, int cap,
                      const int* cnt, const int* buf, int* nn, double* dist, int* n_scans) {
  auto kernel = gspx::k_bf_exact_wide<WHAT>;
  dim3 grid((unsigned)N), block(64);
  size_t lds = (size_t)d * sizeof(double);
  if (d <= 64) {
    kernel = k <= 8 ? bf_exact_kernel<WHAT, 8>(d)
                    : (k <= 16 ? bf_exact_kernel<WHAT, 16>(d)
                               : (k <= 32 ? bf_exact_kernel<WHAT, 32>(d) : bf_exact_kernel<WHAT, 64>(d)));
    grid = dim3((unsigned)((N + 127) / 128));
    block = dim3(128);
    lds = 0;
  }
  hipLaunchKernelGGL(kernel, grid, block, lds, ctx->stream, x, N, d, k, metric, stride, cap, cnt, buf, tau, nn, dist,
                     n_scans);
}

// 4-column MFMA steps of the sweep: the narrow builds' template constant up to 64 dimensions, ceil(d / 4) beyond
static int bf_steps(int d) { return d <= 16 ? 4 : (d <= 32 ? 8 : (d <= 64 ? 16 : (d + 3) / 4)); }

// What a sweep multiplies: the cloud in MFMA operand order (fp64, and fp32 on request), the squared norms and their
// maximum, and the rounding margin of the fp64 product form.  prepare() queues k_bf_prepare; norm_max() downloads the
// norms and waits for the stream - whatever the caller queued in between runs meanwhile.
struct BfOperands {
  DevMem xop, xop32, norm;
  int N = 0, d = 0, DT = 0, ntiles = 0;
  double nmax = 0;
  // |fl(|y|^2 - 2 x.y) + |x|^2 - |x - y|^2| <= (4 DT + 8) u (|x|^2 + |y|^2) with u = 2^-53; ten times that
  // (DT = ceil(d / 4) steps beyond 64 dimensions: the bound grows with the length of the dot product)
  double margin64 = 0;
  int prepare(gspx_ctx* ctx, const double* x, int N_, int d_, bool with32) {
    N = N_, d = d_, DT = bf_steps(d), ntiles = (N + 15) / 16;
    margin64 = 10.0 * (4.0 * DT + 8.0) * 1.1102230246251565e-16;
    CHK(xop.alloc((size_t)ntiles * DT * 64 * sizeof(double)));
    if (with32) CHK(xop32.alloc((size_t)ntiles * DT * 64 * sizeof(float)));
    CHK(norm.alloc((size_t)ntiles * 16 * sizeof(double)));
    const long long total = (long long)ntiles * DT * 64;
    hipLaunchKernelGGL(gspx::k_bf_prepare, dim3((unsigned)((std::max<long long>(total, N) + 255) / 256)), dim3(256), 0,
                       ctx->stream, x, N, d, DT, xop.as<double>(), norm.as<double>(),
                       with32 ? xop32.as<float>() : (float*)nullptr);
    return GSPX_OK;
  }
  int norm_max(gspx_ctx* ctx) {
    std::vector<double> hn((size_t)N);
    HIPCHK(hipMemcpyAsync(hn.data(), norm.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    nmax = 0;
    for (double v : hn) nmax = std::max(nmax, v);
    return GSPX_OK;
  }
};

// One sweep of the 64-query blocks over `count` point tiles (phase / step: bf_tile_of) on the fp32 or the fp64 matrix
// cores: k_bf_collect<4 | 8 | 16> up to 64 dimensions, k_bf_collect_wide beyond.  Every pair within the query's bound
// tau (+ margin (|x|^2 + nmax)) is counted in cnt and appended to buf: fixed-capacity rows (cap), or rows off[q] ..
// off[q + 1] (bf_append).
template <typename F>
static void launch_bf_collect_as(hipStream_t st, const BfOperands& op, const F* xop, const double* tau, int phase, int step,
                                 int count, double margin, int cap, const int* off, int* cnt, int* buf) {
  const dim3 grid((unsigned)((op.N + 255) / 256)), block(256);
  if (op.d > 64) {
    hipLaunchKernelGGL(gspx::k_bf_collect_wide<F>, grid, block, 0, st, xop, op.norm.as<double>(), tau, op.N, op.DT, phase,
                       step, count, margin, op.nmax, cap, off, cnt, buf);
    return;
  }
  const auto kernel =
      op.DT == 4 ? gspx::k_bf_collect<4, F> : (op.DT == 8 ? gspx::k_bf_collect<8, F> : gspx::k_bf_collect<16, F>);
  hipLaunchKernelGGL(kernel, grid, block, 0, st, xop, op.norm.as<double>(), tau, op.N, phase, step, count, margin, op.nmax,
                     cap, off, cnt, buf);
}
static void launch_bf_collect(hipStream_t st, bool f32, const BfOperands& op, const double* tau, int phase, int step,
                              int count, double margin, int cap, const int* off, int* cnt, int* buf) {
  if (f32) launch_bf_collect_as<float>(st, op, op.xop32.as<float>(), tau, phase, step, count, margin, cap, off, cnt, buf);
  else launch_bf_collect_as<double>(st, op, op.xop.as<double>(), tau, phase, step, count, margin, cap, off, cnt, buf);
}

// x: N x d doubles on the device; nn / dist: N x k outputs (nearest first, the point itself excluded).
// stats (nullable, 4 values): sample size, candidate capacity per query, mean candidates per query, queries that
// fell back to the exact scan
static int knn_bruteforce(gspx_ctx* ctx, const double* x, int N, int d, int k, int metric, int* nn, double* dist,
                          double* stats) {
  hipStream_t st = ctx->stream;
  DevMem n_scans;
  CHK(n_scans.alloc(64));
  HIPCHK(hipMemsetAsync(n_scans.p, 0, 64, st));
  if (metric != 0 || N <= 4 * k + 64) {  // no product form (or too few points to bother): exact scan for everybody
    launch_bf<2>(ctx, x, N, d, k, metric, 1, nullptr, 0, nullptr, nullptr, nn, dist, n_scans.as<int>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    if (stats) stats[0] = 0, stats[1] = 0, stats[2] = (double)N, stats[3] = (double)N;
    return GSPX_OK;
  }
  const int ntiles = (N + 15) / 16;
  // sample: about max(2048, N / 128) points (at least 4 k + 1), strided through the cloud
  const int want = std::max(std::max(2048, N / 128), 4 * k + 1);
  const int stride = std::max(1, N / want);
  const int M = (N + stride - 1) / stride;
  // Two sweeps.  The sample's bound admits about k N / M points per query; sweeping only N1 points (every step-th
  // tile of the cloud) with it (k N1 / M candidates), tightening every bound to the exact k-th smallest of those (the k-th neighbour among
  // N1 points: admits about k N / N1 of all points), then sweeping the rest, appends k (N1 / M + N / N1) candidates
  // per query - least at N1 = sqrt(N M), a fifth of the single sweep's at N = 200k.  (The appends, one atomic and
  // one scattered store each, were what the single sweep spent its time on, not the products.)
  int step = (int)std::floor((double)ntiles / std::max(1.0, std::ceil(std::sqrt((double)N * (double)M) / 16.0)));
  if (step < 2) step = 1;                        // small clouds: one sweep over every tile
  const int t1 = (ntiles + step - 1) / step;     // tiles 0, step, 2 step, ...: the first sweep
  const double n1 = std::min<double>((double)t1 * 16.0, (double)N);
  const double expect = (double)k * (n1 / std::max(M - 1, 1) + (step > 1 ? (double)N / n1 : 0.0));
  // room for four times the expectation (clustered clouds), at least 8 k (+ 1: the point itself passes its own bound)
  const int cap = (int)std::min<int64_t>(std::max<int64_t>((int64_t)(4.0 * expect), 8 * k) + 1, N);
  const bool try32 = ctx->opt.knn_f32 != 0;
  BfOperands op;
  DevMem tau, cnt, buf;
  CHK(tau.alloc((size_t)N * sizeof(double)));
  CHK(cnt.alloc((size_t)N * sizeof(int)));
  CHK(buf.alloc((size_t)N * cap * sizeof(int)));
  HIPCHK(hipMemsetAsync(cnt.p, 0, (size_t)N * sizeof(int), st));
  CHK(op.prepare(ctx, x, N, d, try32));
  launch_bf<0>(ctx, x, N, d, k, metric, stride, tau.as<double>(), 0, nullptr, nullptr, nullptr, nullptr, nullptr);
  std::vector<double> ht((size_t)N);
  if (try32) HIPCHK(hipMemcpyAsync(ht.data(), tau.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
  CHK(op.norm_max(ctx));
  // The same bound as op.margin64 with u = 2^-24 for the single-precision sweep: used when it widens a typical bound
  // (the median over a sample of the queries) by at most half a percent - clouds far from the origin (|x|^2 >> the
  // neighbour distances) keep the fp64 sweep.
  const double margin32 = 10.0 * (4.0 * op.DT + 8.0) * 5.9604644775390625e-08;
  bool use32 = false;
  if (try32 && op.nmax < 1e30) {
    std::vector<double> sample;
    for (size_t i = 0; i < (size_t)N; i += std::max<size_t>(1, (size_t)N / 2048)) sample.push_back(ht[i]);
    std::nth_element(sample.begin(), sample.begin() + sample.size() / 2, sample.end());
    const double tmed = sample[sample.size() / 2];
    use32 = ctx->opt.knn_f32 == 2 || margin32 * 2.0 * op.nmax <= 0.005 * tmed;
  }
  const double margin = use32 ? margin32 : op.margin64;
  launch_bf_collect(st, use32, op, tau.as<double>(), 0, step, t1, margin, cap, nullptr, cnt.as<int>(), buf.as<int>());
  if (step > 1) {
    launch_bf<1>(ctx, x, N, d, k, metric, stride, tau.as<double>(), cap, cnt.as<int>(), buf.as<int>(), nullptr, nullptr,
                 nullptr);
    launch_bf_collect(st, use32, op, tau.as<double>(), 1, step, ntiles - t1, margin, cap, nullptr, cnt.as<int>(),
                      buf.as<int>());
  }
  launch_bf<2>(ctx, x, N, d, k, metric, stride, nullptr, cap, cnt.as<int>(), buf.as<int>(), nn, dist, n_scans.as<int>());
  HIPCHK(hipGetLastError());
  int scans = 0;
  HIPCHK(hipMemcpyAsync(&scans, n_scans.p, sizeof(int), hipMemcpyDeviceToHost, st));
  std::vector<int> hc;
  if (stats) {
    hc.resize((size_t)N);
    HIPCHK(hipMemcpyAsync(hc.data(), cnt.p, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  if (stats) {
    double s = 0;
    for (int v : hc) s += v;
    stats[0] = M;
    stats[1] = cap;
    stats[2] = s / N;
    stats[3] = scans;
  }
  return GSPX_OK;
}

// ---- radius search in more than three dimensions (NNtype='radius', nngraph.py:228-287) -------------------------
namespace gspx {

// PASS 0: count the points within the radius (key <= eps2, the KD-tree's ball-query criterion in its own
// arithmetic), PASS 1: write them at rowptr[i].  Candidates from the MFMA sweep (off / buf), or every point.
template <int PASS, int DT>
__global__ __launch_bounds__(128) void k_bf_radius(const double* __restrict__ x, int N, int d, int metric, double eps2,
                                                   const int* __restrict__ off, const int* __restrict__ buf,
                                                   int* __restrict__ cnt, const int* __restrict__ rowptr,
                                                   int* __restrict__ col, double* __restrict__ dist) {
  const int i = blockIdx.x * 128 + threadIdx.x;
  if (i >= N) return;
  double q[4 * DT];
  bf_load_query<DT>(q, x + (size_t)i * d, d);
  const int lo = off ? off[i] : 0, n = off ? off[i + 1] - lo : N;
  const int o = PASS ? rowptr[i] : 0;
  int m = 0;
  for (int a = 0; a < n; ++a) {
    const int idx = off ? buf[(size_t)lo + a] : a;
    if (idx == i) continue;
    const double key = knn_key_reg<DT>(q, x + (size_t)idx * d, d, metric);
    if (key <= eps2) {
      if (PASS) {
        col[o + m] = idx;
        dist[o + m] = metric == 0 ? knn_sqrt(key) : key;
      }
      ++m;
    }
  }
  if (!PASS) cnt[i] = m;
}

// the same two passes in more than 64 dimensions: one wave per query, its row in LDS, the lanes on different
// candidates (k_bf_exact_wide); a round's members keep their candidate order (k_knn_row_sort orders the row later)
template <int PASS>
__global__ __launch_bounds__(64) void k_bf_radius_wide(const double* __restrict__ x, int N, int d, int metric, double eps2,
                                                       const int* __restrict__ off, const int* __restrict__ buf,
                                                       int* __restrict__ cnt, const int* __restrict__ rowptr,
                                                       int* __restrict__ col, double* __restrict__ dist) {
  extern __shared__ double bf_qs[];
  const int i = blockIdx.x, lane = threadIdx.x;
  bf_stage_query(bf_qs, x + (size_t)i * d, d, lane);
  const int lo = off ? off[i] : 0, n = off ? off[i + 1] - lo : N;
  const int o = PASS ? rowptr[i] : 0;
  const unsigned long long lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  int m = 0;  // wave-uniform
  for (int base = 0; base < n; base += 64) {
    const int a = base + lane;
    const int idx = a < n ? (off ? buf[(size_t)lo + a] : a) : i;
    double key = 1e300;
    if (idx != i) key = knn_key(bf_qs, x + (size_t)idx * d, d, metric);
    const bool in = idx != i && key <= eps2;
    const unsigned long long hits = __builtin_amdgcn_ballot_w64(in);
    if (PASS && in) {
      const int at = o + m + __popcll(hits & lt_mask);
      col[at] = idx;
      dist[at] = metric == 0 ? knn_sqrt(key) : key;
    }
    m += __popcll(hits);
  }
  if (!PASS && lane == 0) cnt[i] = m;
}

}  // namespace gspx

template <int PASS>
static void launch_bf_radius(gspx_ctx* ctx, const double* x, int N, int d, int metric, double eps2, const int* off,
                             const int* buf, int* cnt, const int* rowptr, int* col, double* dist) {
  const dim3 grid((unsigned)((N + 127) / 128));
#define GSPX_BR(D_)                                                                                                   \
  hipLaunchKernelGGL((gspx::k_bf_radius<PASS, D_>), grid, dim3(128), 0, ctx->stream, x, N, d, metric, eps2, off, buf, cnt, \
                     rowptr, col, dist)
  if (d > 64)
    hipLaunchKernelGGL((gspx::k_bf_radius_wide<PASS>), dim3((unsigned)N), dim3(64), (size_t)d * sizeof(double), ctx->stream,
                       x, N, d, metric, eps2, off, buf, cnt, rowptr, col, dist);
  else if (d <= 16) GSPX_BR(4);
  else if (d <= 32) GSPX_BR(8);
  else GSPX_BR(16);
#undef GSPX_BR
}

// Candidate lists of the radius search: per query every point whose product-form squared distance is within
// eps2 (+ the rounding margin).  Two sweeps with the same bound: one counts, one fills rows of exactly those lengths.
// Leaves off (N + 1) and buf; euclidean only (the other metrics scan every point in k_bf_radius).
static int radius_candidates(gspx_ctx* ctx, const double* x, int N, int d, double eps2, DevMem& off, DevMem& buf) {
  hipStream_t st = ctx->stream;
  BfOperands op;
  DevMem tau, cnt;
  CHK(tau.alloc((size_t)N * sizeof(double)));
  CHK(cnt.alloc(((size_t)N + 1) * sizeof(int)));
  CHK(off.alloc(((size_t)N + 1) * sizeof(int)));
  HIPCHK(hipMemsetAsync(cnt.p, 0, ((size_t)N + 1) * sizeof(int), st));
  CHK(op.prepare(ctx, x, N, d, false));
  hipLaunchKernelGGL((k_fill<double>), dim3(1024), dim3(256), 0, st, tau.as<double>(), (size_t)N, eps2);
  CHK(op.norm_max(ctx));
  auto sweep = [&](const int* offp, int* bufp) {  // every tile, on the fp64 matrix cores
    launch_bf_collect(st, false, op, tau.as<double>(), 0, 1, op.ntiles, op.margin64, 0, offp, cnt.as<int>(), bufp);
  };
  sweep(nullptr, nullptr);  // count only
  {  // the total in 64 bits BEFORE the 32-bit scan: a sum beyond 2^32 would wrap back to a plausible positive value
    std::vector<int> hc((size_t)N);
    HIPCHK(hipMemcpyAsync(hc.data(), cnt.p, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int64_t total64 = 0;
    for (int v : hc) total64 += v;
    if (total64 >= ((int64_t)1 << 31))
      return set_err(GSPX_ERR_INVALID, "gspx_radius_build: %lld candidate pairs, more than 2^31 (epsilon too large)",
                     (long long)total64);
  }
  int total_c = 0;
  CHK(scan_exclusive(ctx, cnt.as<int>(), off.as<int>(), N + 1, &total_c));
  if (total_c < 0) return set_err(GSPX_ERR_INVALID, "gspx_radius_build: more than 2^31 candidate pairs (epsilon too large)");
  CHK(buf.alloc((size_t)std::max(total_c, 1) * sizeof(int)));
  HIPCHK(hipMemsetAsync(cnt.p, 0, ((size_t)N + 1) * sizeof(int), st));
  sweep(off.as<int>(), buf.as<int>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  return GSPX_OK;
}
