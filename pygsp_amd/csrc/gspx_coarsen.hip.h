// gspx_coarsen.hip.h - multilevel coarsening and pooling on the device: heavy-edge matching by handshake rounds
// (gspx_match_heavy_edges), the coarse graph Wc = P^T W P without its diagonal (gspx_coarsen_build) and segment
// pooling of row-major panels with its vector-Jacobian product (gspx_segment_pool_dev, gspx_segment_pool_vjp_dev).
// gfx950 only.  Included by gspx.hip last (uses the adjacency frame and scan_exclusive of gspx_adjacency.hip.h, DevMem,
// finish_timed, HIPCHK, CHK).
//
// Everything reads the graph's canonical Laplacian (lptr / lcol / lval, the CALLER's vertex order) and its weighted
// degrees dw: for the combinatorial Laplacian w_ij = -L_ij off the diagonal, the bits of W.  The internal (curve)
// order is never looked at, so no result depends on it.
//
// MATCHING.  score(i, j) = w_ij (1 / d_i + 1 / d_j) (normalized cut) or w_ij (weight), fp64, 1 / d once per vertex;
// the sum is commutative and w_ij == w_ji, so both endpoints see the same bits.  A round is two kernels.  k_match_propose:
// a group of lanes per unmatched vertex scans its row and proposes to the unmatched neighbour of largest score, ties to
// the smaller index (lanes walk ascending columns and keep the first maximum; the group combines by a shuffle tree
// under the same rule).  k_match_accept: vertex i with prop[prop[i]] == i takes mate[i] = prop[i] - it writes its own
// slot only - and stores the round's number into a flag word (every writer stores the same value: a plain store).
// Among the edges between two unmatched vertices take those of largest score and of them the one with the smallest
// lower endpoint i, then the smallest other endpoint j: i proposes to j (no neighbour scores higher, none of equal
// score has a smaller index) and j proposes to i (a neighbour k < i of equal score would be an edge of largest score
// with a smaller lower endpoint).  So a round matches a pair while such an edge exists, the loop ends at the first
// round that matches nothing, and the matching is then maximal.  A path with monotone weights matches one pair per
// round: N / 2 rounds.
//
// COARSE GRAPH.  parent[N] (cluster of a vertex) and the clusters' member lists (ascending) come from the host.  Row c
// of the result is made of the member rows laid end to end - (fine row, fine column) ascending - with columns
// relabelled by parent and the entries of the cluster itself dropped (k_co_relabel, into scratch at offsets from a
// scan of the summed row lengths).  k_co_heads marks the first entry of every coarse column and counts them; a scan
// gives the row offsets; k_co_fill places every head at the number of heads with a smaller column and, above the
// diagonal, sums the entries of its column in list order - ascending (fine row, fine column); k_co_mirror copies each
// value below the diagonal from its mirror entry, found by bisection in the sorted row: the result equals its
// transpose bit for bit (summing rows below the diagonal in their own list order would add the same terms in another
// order).  Rows are handled by groups of lanes sized to the mean row, whose pair loops are quadratic in the row; a scratch
// row of more than COARSEN_LONG_ROW entries (a hub) gets a workgroup of its own instead: k_co_long_sort sorts its keys
// (column << 32 | place in the list, so equal columns keep their list order) by a bitonic network in place and counts
// the heads, k_co_long_fill places them by ballots.  No atomics.
//
// POOLING.  A partition as CSR (ptr[Nc + 1], idx[N], members ascending).  One group of lanes per coarse row, lanes
// along the row, 16-byte accesses when the width and the pointers allow; members are visited in order, so `sum` and
// `mean` (the sum divided by the size) add ascending and `max` keeps the first maximum.  The vjp writes every fine row
// from its segment's cotangent row (disjoint writes); for `max` the argmax is recomputed from x.
#pragma once

#include <climits>

namespace gspx {

// ---- matching -------------------------------------------------------------------------------------------------
__global__ void k_match_init(const double* __restrict__ dw, int N, double* __restrict__ invd, int* __restrict__ mate) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  invd[i] = 1.0 / dw[i];
  mate[i] = -1;
}

__global__ __launch_bounds__(256) void k_match_propose(const int* __restrict__ lptr, const int* __restrict__ lcol,
                                                       const double* __restrict__ lval, const double* __restrict__ invd,
                                                       const int* __restrict__ mate, int N, int by_weight, int gs,
                                                       int* __restrict__ prop) {
  const int lane = threadIdx.x % gs, gpb = 256 / gs;
  const int i = blockIdx.x * gpb + threadIdx.x / gs;
  if (i >= N) return;  // (whole groups leave together; the shuffles below stay inside a group)
  if (mate[i] >= 0) {
    if (lane == 0) prop[i] = -1;
    return;
  }
  const double di = invd[i];
  double best = 0.0;
  int bc = -1;
  for (int j = lptr[i] + lane; j < lptr[i + 1]; j += gs) {
    const int c = lcol[j];
    if (c == i || mate[c] >= 0) continue;
    const double w = -lval[j];
    const double s = by_weight ? w : w * (di + invd[c]);
    if (bc < 0 || s > best) {  // (ascending columns: the first maximum has the smallest index)
      best = s;
      bc = c;
    }
  }
  for (int off = gs >> 1; off > 0; off >>= 1) {
    const double os = __shfl_xor(best, off);
    const int oc = __shfl_xor(bc, off);
    if (oc >= 0 && (bc < 0 || os > best || (os == best && oc < bc))) {
      best = os;
      bc = oc;
    }
  }
  if (lane == 0) prop[i] = bc;
}

__global__ void k_match_accept(const int* __restrict__ prop, int N, int round, int* __restrict__ mate,
                               int* __restrict__ flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int p = prop[i];
  if (p >= 0 && prop[p] == i) {  // (prop of a matched vertex is -1: both ends are unmatched)
    mate[i] = p;
    flag[0] = round;
  }
}

// singletons become their own mate; one partial count of pairs per workgroup
__global__ __launch_bounds__(256) void k_match_finish(int* __restrict__ mate, int N, int* __restrict__ partial) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  int n = 0;
  if (i < N) {
    const int m = mate[i];
    if (m < 0) mate[i] = i;
    n = m > i;
  }
  __shared__ int ws[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// ---- coarse graph ---------------------------------------------------------------------------------------------
// summed Laplacian row lengths of every cluster's members
// (and the longest of every workgroup's rows: pmax[blockIdx.x])
__global__ __launch_bounds__(256) void k_co_len(const int* __restrict__ lptr, const int* __restrict__ cptr,
                                                const int* __restrict__ cidx, int Nc, int* __restrict__ tlen,
                                                int* __restrict__ pmax) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  int n = 0;
  if (c < Nc) {
    for (int m = cptr[c]; m < cptr[c + 1]; ++m) {
      const int i = cidx[m];
      n += lptr[i + 1] - lptr[i];
    }
    tlen[c] = n;
  }
  __shared__ int ws[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n = max(n, __shfl_down(n, off));
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) pmax[blockIdx.x] = max(max(ws[0], ws[1]), max(ws[2], ws[3]));
}

// scratch row c = the member rows end to end: cc the coarse column (-1: inside the cluster), wv the weight
__global__ __launch_bounds__(256) void k_co_relabel(const int* __restrict__ lptr, const int* __restrict__ lcol,
                                                    const double* __restrict__ lval, const int* __restrict__ parent,
                                                    const int* __restrict__ cptr, const int* __restrict__ cidx,
                                                    const int* __restrict__ toff, int Nc, int gs,
                                                    int* __restrict__ cc, double* __restrict__ wv) {
  const int lane = threadIdx.x % gs, gpb = 256 / gs;
  const int c = blockIdx.x * gpb + threadIdx.x / gs;
  if (c >= Nc) return;
  int o = toff[c];
  for (int m = cptr[c]; m < cptr[c + 1]; ++m) {
    const int i = cidx[m], j0 = lptr[i], n = lptr[i + 1] - j0;
    for (int k = lane; k < n; k += gs) {
      const int p = parent[lcol[j0 + k]];
      cc[o + k] = p == c ? -1 : p;
      wv[o + k] = -lval[j0 + k];
    }
    o += n;
  }
}

// head[e] = 1 for the first entry of its coarse column in the scratch row; len[c] = the row's heads
__global__ __launch_bounds__(256) void k_co_heads(const int* __restrict__ toff, const int* __restrict__ cc, int Nc,
                                                  int gs, int long_row, unsigned char* __restrict__ head,
                                                  int* __restrict__ len) {
  const int lane = threadIdx.x % gs, gpb = 256 / gs;
  const int c = blockIdx.x * gpb + threadIdx.x / gs;
  if (c >= Nc) return;
  const int o = toff[c], n = toff[c + 1] - o;
  if (n > long_row) return;  // (k_co_long_sort counts it)
  int cnt = 0;
  for (int e = lane; e < n; e += gs) {
    const int d = cc[o + e];
    bool h = d >= 0;
    for (int f = 0; h && f < e; ++f) h = cc[o + f] != d;
    head[o + e] = h ? 1 : 0;
    cnt += h;
  }
  for (int off = gs >> 1; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if (lane == 0) len[c] = cnt;
}

// every head to its place: the number of heads with a smaller column; above the diagonal its value is the sum of the
// column's entries in list order
__global__ __launch_bounds__(256) void k_co_fill(const int* __restrict__ toff, const int* __restrict__ cc,
                                                 const double* __restrict__ wv, const unsigned char* __restrict__ head,
                                                 const int* __restrict__ rowptr, int Nc, int gs, int long_row,
                                                 int* __restrict__ col, double* __restrict__ val) {
  const int lane = threadIdx.x % gs, gpb = 256 / gs;
  const int c = blockIdx.x * gpb + threadIdx.x / gs;
  if (c >= Nc) return;
  const int o = toff[c], n = toff[c + 1] - o, r0 = rowptr[c], rn = rowptr[c + 1] - r0;
  if (n > long_row) return;  // (k_co_long_fill writes it)
  for (int e = lane; e < n; e += gs) {
    if (!head[o + e]) continue;
    const int d = cc[o + e];
    int pos = 0;
    for (int f = 0; f < n; ++f) pos += head[o + f] && cc[o + f] < d;
    if (pos >= rn) continue;  // (cannot happen: rn counts this row's heads)
    col[r0 + pos] = d;
    if (d > c) {
      double s = wv[o + e];
      for (int f = e + 1; f < n; ++f)
        if (cc[o + f] == d) s += wv[o + f];
      val[r0 + pos] = s;
    }
  }
}

// ---- long scratch rows (hubs): the pair loops above are quadratic in the row, these sort it ------------------------
// flag[c] = 1 for a scratch row of more than long_row entries (scanned into places in the list of long rows)
__global__ void k_co_long_flag(const int* __restrict__ toff, int Nc, int long_row, int* __restrict__ flag) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < Nc) flag[c] = toff[c + 1] - toff[c] > long_row;
}
__global__ void k_co_long_list(const int* __restrict__ toff, const int* __restrict__ place, int Nc, int long_row,
                               int* __restrict__ lrow, int* __restrict__ llen) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= Nc) return;
  const int n = toff[c + 1] - toff[c];
  if (n > long_row) {
    lrow[place[c]] = c;
    llen[place[c]] = n;
  }
}

#define GSPX_CO_NOKEY (~0ull)
// is sorted position p the first of its coarse column?  (keys: column << 32 | place in the list; dropped entries and
// the padding carry GSPX_CO_NOKEY and sort last)
__device__ __forceinline__ bool co_long_head(const unsigned long long* __restrict__ K, int p, int n) {
  if (p >= n) return false;
  const unsigned long long k = K[p];
  return k != GSPX_CO_NOKEY && (p == 0 || (K[p - 1] >> 32) != (k >> 32));
}

// one workgroup per long row: its keys into K[koff[b] .. koff[b + 1]) (a power of two), a bitonic sort in place - equal
// columns keep their list order, the place is part of the key - and the row's count of heads
__global__ __launch_bounds__(256) void k_co_long_sort(const int* __restrict__ toff, const int* __restrict__ cc,
                                                      const int* __restrict__ lrow, const int* __restrict__ koff,
                                                      unsigned long long* __restrict__ keys, int* __restrict__ len) {
  const int c = lrow[blockIdx.x], o = toff[c], n = toff[c + 1] - o;
  unsigned long long* K = keys + koff[blockIdx.x];
  const int P = koff[blockIdx.x + 1] - koff[blockIdx.x], t = threadIdx.x;
  for (int e = t; e < P; e += 256) {
    const int d = e < n ? cc[o + e] : -1;
    K[e] = d < 0 ? GSPX_CO_NOKEY : ((unsigned long long)(unsigned)d << 32) | (unsigned)e;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int e = t; e < P; e += 256) {
        const int f = e ^ j;
        if (f > e) {
          const unsigned long long a = K[e], b = K[f];
          if ((a > b) == ((e & k) == 0)) {
            K[e] = b;
            K[f] = a;
          }
        }
      }
      __syncthreads();
    }
  int cnt = 0;
  for (int p = t; p < n; p += 256) cnt += co_long_head(K, p, n);
  __shared__ int ws[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
  if ((t & 63) == 0) ws[t >> 6] = cnt;
  __syncthreads();
  if (t == 0) len[c] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// the sorted long row into the result: a head's place is the number of heads before it (ballots and a running base);
// above the diagonal it sums its column's entries, which follow it in list order
__global__ __launch_bounds__(256) void k_co_long_fill(const int* __restrict__ toff, const double* __restrict__ wv,
                                                      const int* __restrict__ lrow, const int* __restrict__ koff,
                                                      const unsigned long long* __restrict__ keys,
                                                      const int* __restrict__ rowptr, int* __restrict__ col,
                                                      double* __restrict__ val) {
  const int c = lrow[blockIdx.x], o = toff[c], n = toff[c + 1] - o;
  const unsigned long long* K = keys + koff[blockIdx.x];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r0 = rowptr[c], rn = rowptr[c + 1] - r0;
  __shared__ int ws[4];
  int base = 0;
  for (int p0 = 0; p0 < n; p0 += 256) {
    const int p = p0 + t;
    const bool h = co_long_head(K, p, n);
    const unsigned long long b = __ballot(h);
    if (lane == 0) ws[wave] = __popcll(b);
    __syncthreads();
    int pos = base + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += ws[w];
    base += (ws[0] + ws[1]) + (ws[2] + ws[3]);
    __syncthreads();  // (ws is rewritten by the next pass)
    if (h && pos < rn) {
      const unsigned long long k = K[p];
      const int d = (int)(k >> 32);
      col[r0 + pos] = d;
      if (d > c) {
        double s = wv[o + (int)(unsigned)k];
        for (int q = p + 1; q < n && (K[q] >> 32) == (k >> 32); ++q) s += wv[o + (int)(unsigned)K[q]];
        val[r0 + pos] = s;
      }
    }
  }
}

// below the diagonal: the value of the mirror entry (row d, column c), found by bisection
__global__ void k_co_mirror(const int* __restrict__ rowptr, const int* __restrict__ col, int Nc, int nnz,
                            double* __restrict__ val) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nnz) return;
  int lo = 0, hi = Nc;  // the row of entry k: rowptr[c] <= k < rowptr[c + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (rowptr[mid] <= k) lo = mid; else hi = mid;
  }
  const int c = lo, d = col[k];
  if (d >= c) return;
  int a = rowptr[d], b = rowptr[d + 1];
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (col[mid] < c) a = mid + 1; else b = mid;
  }
  if (a < rowptr[d + 1] && col[a] == c) val[k] = val[a];
}

// ---- pooling --------------------------------------------------------------------------------------------------
template <typename T, int VEC> struct alignas(sizeof(T) * VEC) PoolPack { T e[VEC]; };

enum { POOL_MAX = 0, POOL_MEAN = 1, POOL_SUM = 2 };

// y[c][:] = reduce of x[idx[m]][:] over ptr[c] <= m < ptr[c + 1]; cpr = width / VEC packs per row
template <typename T, int VEC>
__global__ __launch_bounds__(256) void k_segment_pool(const int* __restrict__ ptr, const int* __restrict__ idx,
                                                      const T* __restrict__ x, T* __restrict__ y, int Nc, int cpr,
                                                      int mode, int gs) {
  typedef PoolPack<T, VEC> V;
  const int lane = threadIdx.x % gs, gpb = 256 / gs;
  const size_t width = (size_t)cpr * VEC;
  for (int c = blockIdx.x * gpb + threadIdx.x / gs; c < Nc; c += gridDim.x * gpb) {
    const int m0 = ptr[c], m1 = ptr[c + 1];
    if (m1 <= m0) {  // (an empty segment - the host layer refuses them - reads nothing and pools to zero)
      for (int q = lane; q < cpr; q += gs) *(V*)(y + (size_t)c * width + (size_t)q * VEC) = V{};
      continue;
    }
    for (int q = lane; q < cpr; q += gs) {
      V acc = *(const V*)(x + (size_t)idx[m0] * width + (size_t)q * VEC);
      for (int m = m0 + 1; m < m1; ++m) {
        const V v = *(const V*)(x + (size_t)idx[m] * width + (size_t)q * VEC);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          if (mode == POOL_MAX) acc.e[k] = v.e[k] > acc.e[k] ? v.e[k] : acc.e[k];
          else acc.e[k] = acc.e[k] + v.e[k];
        }
      }
      if (mode == POOL_MEAN) {
        const T size = (T)(m1 - m0);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.e[k] = acc.e[k] / size;
      }
      *(V*)(y + (size_t)c * width + (size_t)q * VEC) = acc;
    }
  }
}

// gx[idx[m]][:] from g[c][:]: sum - a copy, mean - g / size, max - g at the first member that attains the maximum of
// x and zero at the others
template <typename T, int VEC>
__global__ __launch_bounds__(256) void k_segment_pool_vjp(const int* __restrict__ ptr, const int* __restrict__ idx,
                                                          const T* __restrict__ x, const T* __restrict__ g,
                                                          T* __restrict__ gx, int Nc, int cpr, int mode, int gs) {
  typedef PoolPack<T, VEC> V;
  const int lane = threadIdx.x % gs, gpb = 256 / gs;
  const size_t width = (size_t)cpr * VEC;
  for (int c = blockIdx.x * gpb + threadIdx.x / gs; c < Nc; c += gridDim.x * gpb) {
    const int m0 = ptr[c], m1 = ptr[c + 1];
    if (m1 <= m0) continue;
    for (int q = lane; q < cpr; q += gs) {
      V gv = *(const V*)(g + (size_t)c * width + (size_t)q * VEC);
      int arg[VEC];
      if (mode == POOL_MAX) {
        V best = *(const V*)(x + (size_t)idx[m0] * width + (size_t)q * VEC);
#pragma unroll
        for (int k = 0; k < VEC; ++k) arg[k] = m0;
        for (int m = m0 + 1; m < m1; ++m) {
          const V v = *(const V*)(x + (size_t)idx[m] * width + (size_t)q * VEC);
#pragma unroll
          for (int k = 0; k < VEC; ++k)
            if (v.e[k] > best.e[k]) {
              best.e[k] = v.e[k];
              arg[k] = m;
            }
        }
      } else if (mode == POOL_MEAN) {
        const T size = (T)(m1 - m0);
#pragma unroll
        for (int k = 0; k < VEC; ++k) gv.e[k] = gv.e[k] / size;
      }
      for (int m = m0; m < m1; ++m) {
        V o = gv;
        if (mode == POOL_MAX) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) o.e[k] = arg[k] == m ? gv.e[k] : T(0);
        }
        *(V*)(gx + (size_t)idx[m] * width + (size_t)q * VEC) = o;
      }
    }
  }
}

}  // namespace gspx

#define COARSEN_LONG_ROW 256  /* scratch rows longer than this are sorted by a workgroup of their own */

// lanes per row for rows of `mean` entries: a power of two in [4, 64]
static int coarsen_group(double mean) {
  int gs = 4;
  while (gs < 64 && gs < mean) gs *= 2;
  return gs;
}

static int coarsen_graph_check(gspx_graph* g, const char* who) {
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (g->dtype != GSPX_F64) return set_err(GSPX_ERR_INVALID, "%s: float64 graphs only", who);
  if (!g->from_w) return set_err(GSPX_ERR_INVALID, "%s needs a graph created from W (degrees)", who);
  if (g->lap_type != GSPX_LAP_COMBINATORIAL)
    return set_err(GSPX_ERR_INVALID, "%s reads the weights off the combinatorial Laplacian", who);
  return GSPX_OK;
}

extern "C" int gspx_match_heavy_edges(gspx_graph* g, int metric, int64_t max_rounds, int32_t* mate_host,
                                      int32_t* rounds, int64_t* pairs, double* kernel_ms) {
  if (rounds) *rounds = 0;
  if (pairs) *pairs = 0;
  if (kernel_ms) *kernel_ms = 0;
  CHK(coarsen_graph_check(g, "match_heavy_edges"));
  if (metric != 0 && metric != 1)
    return set_err(GSPX_ERR_INVALID, "match_heavy_edges: metric must be 0 (normalized cut) or 1 (weight)");
  const int64_t N = g->N;
  if (N > 0 && !mate_host) return set_err(GSPX_ERR_INVALID, "match_heavy_edges: null output");
  if (N == 0) return GSPX_OK;
  gspx_ctx* ctx = g->ctx;
  hipStream_t st = ctx->stream;
  replay_reset(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  const int nbN = (int)((N + 255) / 256);
  DevMem invd, mate, prop, flag, partial;
  CHK(invd.alloc((size_t)N * sizeof(double)));
  CHK(mate.alloc((size_t)N * sizeof(int)));
  CHK(prop.alloc((size_t)N * sizeof(int)));
  CHK(flag.alloc(sizeof(int)));
  CHK(partial.alloc((size_t)nbN * sizeof(int)));
  HIPCHK(hipMemsetAsync(flag.p, 0, sizeof(int), st));
  const int gs = coarsen_group((double)g->nnz_l / (double)N);
  const int gpb = 256 / gs;
  const unsigned nbr = (unsigned)((N + gpb - 1) / gpb);
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL(gspx::k_match_init, dim3(nbN), dim3(256), 0, st, g->dw.as<double>(), (int)N, invd.as<double>(),
                     mate.as<int>());
  int done = 0;
  while (max_rounds < 0 || done < max_rounds) {
    hipLaunchKernelGGL(gspx::k_match_propose, dim3(nbr), dim3(256), 0, st, g->lptr.as<int>(), g->lcol.as<int>(),
                       g->lval.as<double>(), invd.as<double>(), mate.as<int>(), (int)N, metric, gs, prop.as<int>());
    hipLaunchKernelGGL(gspx::k_match_accept, dim3(nbN), dim3(256), 0, st, prop.as<int>(), (int)N, done + 1,
                       mate.as<int>(), flag.as<int>());
    HIPCHK(hipGetLastError());
    int seen = 0;
    HIPCHK(hipMemcpyAsync(&seen, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (seen != done + 1) break;  // the round matched nothing
    ++done;
  }
  hipLaunchKernelGGL(gspx::k_match_finish, dim3(nbN), dim3(256), 0, st, mate.as<int>(), (int)N, partial.as<int>());
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  std::vector<int> hp((size_t)nbN);
  HIPCHK(hipMemcpyAsync(hp.data(), partial.p, (size_t)nbN * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(mate_host, mate.p, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, st));
  CHK(finish_timed(ctx, kernel_ms));
  int64_t np = 0;
  for (int v : hp) np += v;
  if (rounds) *rounds = done;
  if (pairs) *pairs = np;
  return GSPX_OK;
}

extern "C" int gspx_coarsen_build(gspx_graph* g, const int32_t* parent_host, int64_t n_clusters, gspx_knn** out,
                                  double* kernel_ms) {
  if (out) *out = nullptr;
  if (kernel_ms) *kernel_ms = 0;
  if (!out) return set_err(GSPX_ERR_INVALID, "coarsen_build: null output");
  CHK(coarsen_graph_check(g, "coarsen_build"));
  const int64_t N = g->N, Nc = n_clusters;
  if (Nc < 0 || Nc > N || (N > 0 && (!parent_host || Nc < 1)))
    return set_err(GSPX_ERR_INVALID, "coarsen_build: %lld clusters for %lld vertices", (long long)Nc, (long long)N);
  // the clusters' member lists, ascending (a counting sort of the vertices by parent); every cluster has a member
  std::vector<int> cptr((size_t)Nc + 1, 0), cidx((size_t)N);
  for (int64_t i = 0; i < N; ++i) {
    const int64_t p = parent_host[i];
    if (p < 0 || p >= Nc)
      return set_err(GSPX_ERR_INVALID, "coarsen_build: parent[%lld] = %lld is outside [0, %lld)", (long long)i,
                     (long long)p, (long long)Nc);
    ++cptr[(size_t)p + 1];
  }
  for (int64_t c = 0; c < Nc; ++c) {
    if (cptr[(size_t)c + 1] == 0)
      return set_err(GSPX_ERR_INVALID, "coarsen_build: cluster %lld has no member", (long long)c);
    cptr[(size_t)c + 1] += cptr[(size_t)c];
  }
  {
    std::vector<int> cur(cptr.begin(), cptr.end() - 1);
    for (int64_t i = 0; i < N; ++i) cidx[(size_t)cur[(size_t)parent_host[i]]++] = (int)i;
  }
  gspx_ctx* ctx = g->ctx;
  hipStream_t st = ctx->stream;
  replay_reset(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  std::unique_ptr<gspx_knn> h;
  CHK(adjacency_open(ctx, Nc, h));
  const int64_t total = g->nnz_l;  // every Laplacian entry lands in exactly one scratch row
  if (Nc > 0 && total > 0) {
    DevMem par, cp, ci, toff, cc, wv, head, pmax;
    CHK(par.alloc((size_t)N * sizeof(int)));
    CHK(cp.alloc(((size_t)Nc + 1) * sizeof(int)));
    CHK(ci.alloc((size_t)N * sizeof(int)));
    CHK(toff.alloc(((size_t)Nc + 1) * sizeof(int)));
    CHK(cc.alloc((size_t)total * sizeof(int)));
    CHK(wv.alloc((size_t)total * sizeof(double)));
    CHK(head.alloc((size_t)total));
    CHK(pmax.alloc((size_t)((Nc + 255) / 256) * sizeof(int)));
    HIPCHK(hipMemcpyAsync(par.p, parent_host, (size_t)N * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(cp.p, cptr.data(), ((size_t)Nc + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ci.p, cidx.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(toff.p, 0, ((size_t)Nc + 1) * sizeof(int), st));
    const int gs = coarsen_group((double)total / (double)Nc);
    const int gpb = 256 / gs;
    const unsigned nbc = (unsigned)((Nc + 255) / 256), nbr = (unsigned)((Nc + gpb - 1) / gpb);
    HIPCHK(hipEventRecord(ctx->ev[0], st));
    hipLaunchKernelGGL(gspx::k_co_len, dim3(nbc), dim3(256), 0, st, g->lptr.as<int>(), cp.as<int>(), ci.as<int>(),
                       (int)Nc, toff.as<int>(), pmax.as<int>());
    CHK(scan_exclusive(ctx, toff.as<int>(), toff.as<int>(), (int)Nc + 1));  // lengths -> offsets, in place
    // rows of more than COARSEN_LONG_ROW entries leave the pair loops for a sort of their own: their list, their padded
    // key ranges
    std::vector<int> hmax((size_t)nbc);
    HIPCHK(hipMemcpyAsync(hmax.data(), pmax.p, (size_t)nbc * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int long_row = INT_MAX, nlong = 0;
    DevMem lrow, koff, keys;
    if (*std::max_element(hmax.begin(), hmax.end()) > COARSEN_LONG_ROW) {
      long_row = COARSEN_LONG_ROW;
      DevMem place, llen;
      CHK(place.alloc(((size_t)Nc + 1) * sizeof(int)));
      HIPCHK(hipMemsetAsync(place.p, 0, ((size_t)Nc + 1) * sizeof(int), st));
      hipLaunchKernelGGL(gspx::k_co_long_flag, dim3(nbc), dim3(256), 0, st, toff.as<int>(), (int)Nc, long_row,
                         place.as<int>());
      CHK(scan_exclusive(ctx, place.as<int>(), place.as<int>(), (int)Nc + 1, &nlong));
      CHK(lrow.alloc((size_t)nlong * sizeof(int)));
      CHK(llen.alloc((size_t)nlong * sizeof(int)));
      CHK(koff.alloc(((size_t)nlong + 1) * sizeof(int)));
      hipLaunchKernelGGL(gspx::k_co_long_list, dim3(nbc), dim3(256), 0, st, toff.as<int>(), place.as<int>(), (int)Nc,
                         long_row, lrow.as<int>(), llen.as<int>());
      std::vector<int> hl((size_t)nlong), hk((size_t)nlong + 1, 0);
      HIPCHK(hipMemcpyAsync(hl.data(), llen.p, (size_t)nlong * sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      int64_t padded = 0;
      for (int k = 0; k < nlong; ++k) {
        int64_t P = 1;
        while (P < hl[(size_t)k]) P *= 2;
        padded += P;
        if (padded >= ((int64_t)1 << 31)) return set_err(GSPX_ERR_INVALID, "coarsen_build: the long rows' keys exceed 32-bit offsets");
        hk[(size_t)k + 1] = (int)padded;
      }
      CHK(keys.alloc((size_t)padded * sizeof(unsigned long long)));
      HIPCHK(hipMemcpyAsync(koff.p, hk.data(), ((size_t)nlong + 1) * sizeof(int), hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));  // (hk goes out of scope)
    }
    hipLaunchKernelGGL(gspx::k_co_relabel, dim3(nbr), dim3(256), 0, st, g->lptr.as<int>(), g->lcol.as<int>(),
                       g->lval.as<double>(), par.as<int>(), cp.as<int>(), ci.as<int>(), toff.as<int>(), (int)Nc, gs,
                       cc.as<int>(), wv.as<double>());
    hipLaunchKernelGGL(gspx::k_co_heads, dim3(nbr), dim3(256), 0, st, toff.as<int>(), cc.as<int>(), (int)Nc, gs,
                       long_row, head.as<unsigned char>(), h->rowptr.as<int>());
    if (nlong > 0)
      hipLaunchKernelGGL(gspx::k_co_long_sort, dim3((unsigned)nlong), dim3(256), 0, st, toff.as<int>(), cc.as<int>(),
                         lrow.as<int>(), koff.as<int>(), keys.as<unsigned long long>(), h->rowptr.as<int>());
    CHK(adjacency_offsets(h.get(), h->rowptr.as<int>(), "coarsen_build"));  // lengths -> offsets, in place
    const int nnz = (int)h->nnz;
    if (nnz > 0) {
      hipLaunchKernelGGL(gspx::k_co_fill, dim3(nbr), dim3(256), 0, st, toff.as<int>(), cc.as<int>(), wv.as<double>(),
                         head.as<unsigned char>(), h->rowptr.as<int>(), (int)Nc, gs, long_row, h->col.as<int>(),
                         h->val.as<double>());
      if (nlong > 0)
        hipLaunchKernelGGL(gspx::k_co_long_fill, dim3((unsigned)nlong), dim3(256), 0, st, toff.as<int>(),
                           wv.as<double>(), lrow.as<int>(), koff.as<int>(), keys.as<unsigned long long>(),
                           h->rowptr.as<int>(), h->col.as<int>(), h->val.as<double>());
      hipLaunchKernelGGL(gspx::k_co_mirror, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, h->rowptr.as<int>(),
                         h->col.as<int>(), (int)Nc, nnz, h->val.as<double>());
    }
    HIPCHK(hipEventRecord(ctx->ev[1], st));
    CHK(finish_timed(ctx, kernel_ms));  // (synchronises: the host vectors and the scratch are at rest)
  } else {
    HIPCHK(hipStreamSynchronize(st));
  }
  adjacency_close(h, t0, out);
  return GSPX_OK;
}

// ---- pooling entry points ---------------------------------------------------------------------------------------
static int pool_check(gspx_ctx* ctx, int dtype, int mode, int64_t N, int64_t Nc, int64_t width, const void* ptr,
                      const void* idx) {
  if (!ctx) return set_err(GSPX_ERR_INVALID, "null ctx");
  if (dtype != GSPX_F32 && dtype != GSPX_F64) return set_err(GSPX_ERR_INVALID, "segment_pool: dtype must be GSPX_F32 or GSPX_F64");
  if (mode < 0 || mode > 2) return set_err(GSPX_ERR_INVALID, "segment_pool: mode must be 0 (max), 1 (mean) or 2 (sum)");
  if (N < 0 || Nc < 0 || Nc > N || (N > 0 && Nc < 1) || N >= ((int64_t)1 << 31) || width < 1 ||
      width >= ((int64_t)1 << 24))
    return set_err(GSPX_ERR_INVALID, "segment_pool: bad sizes (N %lld, Nc %lld, width %lld)", (long long)N,
                   (long long)Nc, (long long)width);
  if (N > 0 && (!ptr || !idx)) return set_err(GSPX_ERR_INVALID, "segment_pool: null partition");
  return GSPX_OK;
}

template <typename T, bool VJP>
static int pool_launch(gspx_ctx* ctx, int mode, int64_t Nc, int64_t width, const int* ptr, const int* idx, const T* x,
                       const T* g, T* out, double* kernel_ms) {
  constexpr int W = 16 / (int)sizeof(T);
  const bool wide = width % W == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)out % 16) == 0;
  const int cpr = (int)(wide ? width / W : width);
  int gs = 1;
  while (gs < 64 && gs < cpr) gs *= 2;
  const int gpb = 256 / gs;
  const unsigned nb = (unsigned)std::min<int64_t>((Nc + gpb - 1) / gpb, (int64_t)ctx->cu_count * 32);
  hipStream_t st = ctx->stream;
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  if (VJP) {
    if (wide)
      hipLaunchKernelGGL((gspx::k_segment_pool_vjp<T, W>), dim3(nb), dim3(256), 0, st, ptr, idx, x, g, out, (int)Nc, cpr,
                         mode, gs);
    else
      hipLaunchKernelGGL((gspx::k_segment_pool_vjp<T, 1>), dim3(nb), dim3(256), 0, st, ptr, idx, x, g, out, (int)Nc, cpr,
                         mode, gs);
  } else {
    if (wide)
      hipLaunchKernelGGL((gspx::k_segment_pool<T, W>), dim3(nb), dim3(256), 0, st, ptr, idx, x, out, (int)Nc, cpr, mode,
                         gs);
    else
      hipLaunchKernelGGL((gspx::k_segment_pool<T, 1>), dim3(nb), dim3(256), 0, st, ptr, idx, x, out, (int)Nc, cpr, mode,
                         gs);
  }
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  return finish_timed(ctx, kernel_ms);
}

extern "C" int gspx_segment_pool_dev(gspx_ctx* ctx, int dtype, int mode, int64_t N, int64_t Nc, int64_t width,
                                     const int32_t* ptr_dev, const int32_t* idx_dev, const void* x_dev, void* y_dev,
                                     double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  CHK(pool_check(ctx, dtype, mode, N, Nc, width, ptr_dev, idx_dev));
  if (N == 0) return GSPX_OK;
  if (!x_dev || !y_dev) return set_err(GSPX_ERR_INVALID, "segment_pool: null panel");
  replay_reset(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  return dtype == GSPX_F32 ? pool_launch<float, false>(ctx, mode, Nc, width, ptr_dev, idx_dev, (const float*)x_dev,
                                                       (const float*)nullptr, (float*)y_dev, kernel_ms)
                           : pool_launch<double, false>(ctx, mode, Nc, width, ptr_dev, idx_dev, (const double*)x_dev,
                                                        (const double*)nullptr, (double*)y_dev, kernel_ms);
}

extern "C" int gspx_segment_pool_vjp_dev(gspx_ctx* ctx, int dtype, int mode, int64_t N, int64_t Nc, int64_t width,
                                         const int32_t* ptr_dev, const int32_t* idx_dev, const void* x_dev,
                                         const void* g_dev, void* gx_dev, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  CHK(pool_check(ctx, dtype, mode, N, Nc, width, ptr_dev, idx_dev));
  if (N == 0) return GSPX_OK;
  if (!g_dev || !gx_dev || (mode == 0 && !x_dev)) return set_err(GSPX_ERR_INVALID, "segment_pool_vjp: null panel");
  replay_reset(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  return dtype == GSPX_F32 ? pool_launch<float, true>(ctx, mode, Nc, width, ptr_dev, idx_dev, (const float*)x_dev,
                                                      (const float*)g_dev, (float*)gx_dev, kernel_ms)
                           : pool_launch<double, true>(ctx, mode, Nc, width, ptr_dev, idx_dev, (const double*)x_dev,
                                                       (const double*)g_dev, (double*)gx_dev, kernel_ms);
}
