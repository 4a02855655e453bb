// gspx_knn.hip.h - neighbour graphs on the device: k nearest neighbours and, at the end of the file, the radius
// search.  After gspx_adjacency.hip.h (the handle gspx_knn and the builder's frame,
// scan_exclusive).  gfx950 only.
//
// Replaces, for NNtype='knn' (1 <= d <= 3 by the grid search below; 4 <= d <= 4096 by the tiled brute force on the
// matrix cores of gspx_knn_bf.hip.h; the weights / symmetrisation / CSR stages are shared):
//   pygsp/graphs/nngraphs/nngraph.py:213-216  kdt = spatial.KDTree(Xout); D, NN = kdt.query(Xout, k + 1)
//   nngraph.py:218-226                        sigma = mean(D[:, 1:]);  w = exp(-D^2 / sigma)
//   nngraph.py:289-297                        W = csc((w, (i, j)));  W = (W + W.T) / 2
// Method: uniform grid (about 2.5 points per cell), counting sort of the points by cell, one thread
// per query walking the Chebyshev rings of cells around its own until the k-th best distance is
// below what any unvisited ring can offer.  Distances are formed exactly like the KD-tree's
// (sum of squared differences in dimension order, no fused multiply-add, one correctly rounded
// sqrt), so neighbour lists and distances equal scipy's bit for bit (ties, i.e. exactly equal
// distances, are ordered by vertex index).
#pragma once

namespace gspx {

struct KnnGrid {
  double lo[3];
  double inv_h[3];
  double h_min;
  int n[3];
  int d;
  int metric;  // 0 euclidean, 1 manhattan, 2 max_dist (the reference's dist_type, nngraph.py:139-145)
};

__device__ __forceinline__ int knn_cell_of(const KnnGrid& g, const double* __restrict__ p, int c[3]) {
  int id = 0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    c[j] = 0;
    if (j < g.d) {
      int v = (int)((p[j] - g.lo[j]) * g.inv_h[j]);
      v = v < 0 ? 0 : (v >= g.n[j] ? g.n[j] - 1 : v);
      c[j] = v;
    }
  }
  id = (c[2] * g.n[1] + c[1]) * g.n[0] + c[0];
  return id;
}

__global__ void k_knn_cell_count(const double* __restrict__ x, int N, KnnGrid g, int* __restrict__ cell,
                                 int* __restrict__ count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  int c[3];
  const int id = knn_cell_of(g, x + (size_t)i * g.d, c);
  cell[i] = id;
  atomicAdd(&count[id], 1);
}
__global__ void k_knn_scatter(const int* __restrict__ cell, int N, const int* __restrict__ start,
                              int* __restrict__ cursor, int* __restrict__ order) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int id = cell[i];
  order[start[id] + atomicAdd(&cursor[id], 1)] = i;
}
// the scatter's order inside a cell depends on atomics: sort every cell's points by index, and
// gather the coordinates in that order (sorted[s] = x[order[s]])
__global__ void k_knn_cell_sort(const int* __restrict__ start, int ncells, int* __restrict__ order,
                                const double* __restrict__ x, int d, double* __restrict__ sorted) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncells) return;
  const int lo = start[c], hi = start[c + 1];
  for (int a = lo + 1; a < hi; ++a) {
    const int v = order[a];
    int b = a - 1;
    while (b >= lo && order[b] > v) {
      order[b + 1] = order[b];
      --b;
    }
    order[b + 1] = v;
  }
  for (int a = lo; a < hi; ++a)
    for (int j = 0; j < d; ++j) sorted[(size_t)a * d + j] = x[(size_t)order[a] * d + j];
}

// KD-tree arithmetic (scipy ckdtree, distance_base.h: sqeuclidean_distance_double): four running sums over the
// dimensions taken four at a time - acc[j] += (u[i+j] - v[i+j])^2 -, then s = ((acc0 + acc1) + acc2) + acc3, then
// the remaining (at most three) dimensions added to s one by one; in 1-3 dimensions that is the plain sum in
// dimension order.  Every operation is rounded on its own - hipcc contracts a*b+c into an fma by default, which
// changes the last bit, so contraction is switched off here.  (Checked against scipy 1.15 in 4 to 64
// dimensions: tests/test_gpu_5_knn.py::test_highdim_oracle.)
__device__ __forceinline__ double knn_sqdist(const double* q, const double* __restrict__ p, int d) {
#pragma clang fp contract(off)
  double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  int j = 0;
  for (; j + 4 <= d; j += 4) {
    const double d0 = q[j] - p[j], d1 = q[j + 1] - p[j + 1], d2 = q[j + 2] - p[j + 2], d3 = q[j + 3] - p[j + 3];
    const double s0 = d0 * d0, s1 = d1 * d1, s2 = d2 * d2, s3 = d3 * d3;
    a0 = a0 + s0;
    a1 = a1 + s1;
    a2 = a2 + s2;
    a3 = a3 + s3;
  }
  double d2 = ((a0 + a1) + a2) + a3;
  for (; j < d; ++j) {
    const double df = q[j] - p[j];
    const double sq = df * df;
    d2 = d2 + sq;
  }
  return d2;
}
// the comparison key of a candidate: squared euclidean distance, or the manhattan / max distance itself
// (ckdtree's MinkowskiDistP1 / Pinf: a sum of |differences| in dimension order / their maximum - exact)
__device__ __forceinline__ double knn_key(const double* q, const double* __restrict__ p, int d, int metric) {
  if (metric == 0) return knn_sqdist(q, p, d);
  double s = 0;
  for (int j = 0; j < d; ++j) {
    const double a = fabs(q[j] - p[j]);
    s = metric == 1 ? s + a : fmax(s, a);
  }
  return s;
}
// correctly rounded square root: the hardware-assisted sqrt is within an ulp; one exact residual
// (fma) and a correction decide the last bit
__device__ __forceinline__ double knn_sqrt(double x) {
  if (!(x > 0.0)) return 0.0;
  const double s = sqrt(x);
  const double r = fma(-s, s, x);  // exact x - s*s
  return s + r / (2.0 * s);
}

// The KMAX best candidates of one thread's query, in registers: bd[] sorted ascending, kept so by a chain of
// conditional swaps.  Every element is indexed with compile-time constants only (fully unrolled loops) - no dynamic
// register indexing, so nothing goes to scratch memory.  Two forms: keys alone, compared with a strict < (for a bound:
// the k-th smallest key), and keys with the candidates' indices bi[], ordered by (key, index) - the KD-tree's answer
// for exactly equal distances.  (Plain arrays of the kernel, not members of a struct: with a struct the register
// allocator needed 14 to 30 more VGPRs at KMAX = 16 and two builds lost a wave of occupancy, profiles/knn_refactor.md.)
template <int KMAX> __device__ __forceinline__ void knn_best_init(double (&bd)[KMAX]) {
#pragma unroll
  for (int t = 0; t < KMAX; ++t) bd[t] = 1e300;
}
template <int KMAX> __device__ __forceinline__ void knn_best_init(double (&bd)[KMAX], int (&bi)[KMAX]) {
#pragma unroll
  for (int t = 0; t < KMAX; ++t) {
    bd[t] = 1e300;
    bi[t] = 0x7fffffff;
  }
}
// the cheap test against the last entry guards the chain: once the list has settled, few candidates pass it
template <int KMAX> __device__ __forceinline__ void knn_best_insert(double (&bd)[KMAX], double cd) {
  if (cd < bd[KMAX - 1]) {
#pragma unroll
    for (int t = 0; t < KMAX; ++t) {
      const bool lt = cd < bd[t];
      const double td = bd[t];
      bd[t] = lt ? cd : td;
      cd = lt ? td : cd;
    }
  }
}
template <int KMAX>
__device__ __forceinline__ void knn_best_insert(double (&bd)[KMAX], int (&bi)[KMAX], double cd, int ci) {
  if (cd < bd[KMAX - 1] || (cd == bd[KMAX - 1] && ci < bi[KMAX - 1])) {
#pragma unroll
    for (int t = 0; t < KMAX; ++t) {
      const bool lt = cd < bd[t] || (cd == bd[t] && ci < bi[t]);
      const double td = bd[t];
      const int ti = bi[t];
      bd[t] = lt ? cd : td;
      bi[t] = lt ? ci : ti;
      cd = lt ? td : cd;
      ci = lt ? ti : ci;
    }
  }
}
// the k-th entry (1 <= k <= KMAX, a run-time value) by a compile-time scan
template <int KMAX> __device__ __forceinline__ double knn_best_kth(const double (&bd)[KMAX], int k) {
  double kth = 1e300;
#pragma unroll
  for (int t = 0; t < KMAX; ++t)
    if (t == k - 1) kth = bd[t];
  return kth;
}

// one thread per query (in cell order: a wave's queries are neighbours in space)
template <int KMAX>
__global__ __launch_bounds__(128) void k_knn_query(const double* __restrict__ sorted,
                                                   const int* __restrict__ order,
                                                   const int* __restrict__ start, int N, KnnGrid g,
                                                   int k, int* __restrict__ nn,
                                                   double* __restrict__ dist) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= N) return;
  const int self = order[s];
  double q[3] = {0, 0, 0};
  for (int j = 0; j < g.d; ++j) q[j] = sorted[(size_t)s * g.d + j];
  int c[3];
  knn_cell_of(g, q, c);
  // distance from the query to the nearest wall of its own cell (>= 0 up to rounding)
  double m = 1e300;
  for (int j = 0; j < g.d; ++j) {
    const double h = 1.0 / g.inv_h[j];
    const double a = q[j] - (g.lo[j] + c[j] * h), b = (g.lo[j] + (c[j] + 1) * h) - q[j];
    m = fmin(m, fmin(a, b));
  }
  m = fmax(m, 0.0);
  double bd[KMAX];
  int bi[KMAX];
  knn_best_init<KMAX>(bd, bi);
  const int rmax = max(g.n[0], max(g.n[1], g.n[2]));
  const int r2 = g.d >= 2 ? 1 : 0, r3 = g.d >= 3 ? 1 : 0;
  for (int r = 0; r <= rmax; ++r) {
    for (int dz = -r * r3; dz <= r * r3; ++dz) {
      const int cz = c[2] + dz;
      if (cz < 0 || cz >= g.n[2]) continue;
      for (int dy = -r * r2; dy <= r * r2; ++dy) {
        const int cy = c[1] + dy;
        if (cy < 0 || cy >= g.n[1]) continue;
        const bool shell = (abs(dz) == r && r3) || (abs(dy) == r && r2);
        // on the shell every dx counts; inside it only the two end cells dx = -r, +r
        const int step = (shell || r == 0) ? 1 : 2 * r;
        for (int dx = -r; dx <= r; dx += step) {
          const int cx = c[0] + dx;
          if (cx < 0 || cx >= g.n[0]) continue;
          const int cid = (cz * g.n[1] + cy) * g.n[0] + cx;
          for (int a = start[cid]; a < start[cid + 1]; ++a) {
            const int idx = order[a];
            if (idx == self) continue;
            knn_best_insert<KMAX>(bd, bi, knn_key(q, sorted + (size_t)a * g.d, g.d, g.metric), idx);
          }
        }
      }
    }
    // every point not yet visited lies beyond r whole cells plus the way out of the own cell
    const double kth = knn_best_kth<KMAX>(bd, k);
    const double lb = (r * g.h_min + m) * (1.0 - 1e-12);
    if (kth < 1e300 && kth <= (g.metric == 0 ? lb * lb : lb)) break;  // every p-norm is >= the max norm
  }
#pragma unroll
  for (int t = 0; t < KMAX; ++t)
    if (t < k) {
      nn[(size_t)self * k + t] = bi[t];
      dist[(size_t)self * k + t] = g.metric == 0 ? knn_sqrt(bd[t]) : bd[t];
    }
}

// sum of all distances (double, fixed order): partial sums per block, then one block
__global__ __launch_bounds__(256) void k_knn_sum_partial(const double* __restrict__ v, size_t n,
                                                         double* __restrict__ partial) {
  __shared__ double ws[4];
  double acc = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) acc += v[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// w = exp(-d^2 / sigma) (nngraph.py:224-226: the distance is squared again after the sqrt); an edge
// i -> j is mutual when i is among j's neighbours; non-mutual edges add one entry to row j
// Symmetrisation of the directed k-NN matrix (utils.symmetrize, utils.py:247-275; the weights of a
// mutual pair are equal):  0 'average'  (W + W^T) / 2 - a mutual pair keeps w, a one-sided edge leaves
// w / 2 in both rows;  1 'maximum' / 'fill' - w in both rows either way;  2 'tril' / 3 'triu' - only
// the entries below / above the diagonal count: the pair {i, j} exists iff its larger (smaller) end
// chose the other.  Per directed edge i -> j: `self` = row i keeps (i, j), `other` = row j gets (j, i).
__device__ __forceinline__ void knn_sym_rule(int sym, int i, int j, bool mutual, bool& self, bool& other,
                                             double& scale) {
  scale = 1.0;
  if (sym <= 1) {
    self = true;
    other = !mutual;
    if (sym == 0 && !mutual) scale = 0.5;
  } else {
    self = other = (sym == 2) ? (j < i) : (j > i);
  }
}
// w = exp(-d^2 / sigma) (nngraph.py:224-226: the distance is squared again after the sqrt); an edge
// i -> j is mutual when i is among j's neighbours; row lengths are counted here
__global__ void k_knn_weights(const int* __restrict__ nn, const double* __restrict__ dist, int N, int k,
                              double sigma, int sym, double* __restrict__ w,
                              unsigned char* __restrict__ mutual, int* __restrict__ len) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)N * k) return;
  const int i = (int)(e / k);
  const int j = nn[e];
  const double d = dist[e];
  w[e] = exp(-(d * d) / sigma);
  bool mu = false;
  for (int t = 0; t < k; ++t) mu |= nn[(size_t)j * k + t] == i;
  mutual[e] = mu ? 1 : 0;
  bool self, other;
  double scale;
  knn_sym_rule(sym, i, j, mu, self, other, scale);
  if (self) atomicAdd(&len[i], 1);
  if (other) atomicAdd(&len[j], 1);
}
// The same result out of place, without dependent memory chains: every entry's final position is the number of
// smaller columns in its row (columns are distinct within a row), counted with independent, cache-resident loads.
// (The in-place insertion sort above shifts through global memory - a dependent load / store pair per shift: it
// was 15 % of a high-dimensional build.)
__global__ void k_knn_row_rank(const int* __restrict__ rowptr, int N, const int* __restrict__ col,
                               const double* __restrict__ val, int* __restrict__ col2, double* __restrict__ val2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int lo = rowptr[i], hi = rowptr[i + 1];
  if (hi - lo > 64) return;  // long rows (hubs - common in high dimensions): a whole wave each, below
  for (int a = lo; a < hi; ++a) {
    const int c = col[a];
    int rank = 0;
    for (int b = lo; b < hi; ++b) rank += col[b] < c;
    col2[lo + rank] = c;
    val2[lo + rank] = val[a];
  }
}
// rows longer than 64 entries: one wave per row, every lane ranks its share of the entries
__global__ __launch_bounds__(256) void k_knn_row_rank_long(const int* __restrict__ rowptr, int N,
                                                           const int* __restrict__ col, const double* __restrict__ val,
                                                           int* __restrict__ col2, double* __restrict__ val2) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= N) return;
  const int lo = rowptr[i], hi = rowptr[i + 1];
  if (hi - lo <= 64) return;
  for (int a = lo + lane; a < hi; a += 64) {
    const int c = col[a];
    int rank = 0;
    for (int b = lo; b < hi; ++b) rank += col[b] < c;
    col2[lo + rank] = c;
    val2[lo + rank] = val[a];
  }
}
__global__ void k_knn_fill(const int* __restrict__ nn, const double* __restrict__ w,
                           const unsigned char* __restrict__ mutual, int N, int k, int sym,
                           const int* __restrict__ rowptr, int* __restrict__ cursor,
                           int* __restrict__ col, double* __restrict__ val) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)N * k) return;
  const int i = (int)(e / k);
  const int j = nn[e];
  bool self, other;
  double scale;
  knn_sym_rule(sym, i, j, mutual[e] != 0, self, other, scale);
  const double v = w[e] * scale;
  if (self) {
    const int o = rowptr[i] + atomicAdd(&cursor[i], 1);
    col[o] = j;
    val[o] = v;
  }
  if (other) {
    const int o = rowptr[j] + atomicAdd(&cursor[j], 1);
    col[o] = i;
    val[o] = v;
  }
}
__global__ void k_knn_row_sort(const int* __restrict__ rowptr, int N, int* __restrict__ col,
                               double* __restrict__ val) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int lo = rowptr[i], hi = rowptr[i + 1];
  for (int a = lo + 1; a < hi; ++a) {
    const int c = col[a];
    const double v = val[a];
    int b = a - 1;
    while (b >= lo && col[b] > c) {
      col[b + 1] = col[b];
      val[b + 1] = val[b];
      --b;
    }
    col[b + 1] = c;
    val[b + 1] = v;
  }
}

}  // namespace gspx

#include "gspx_knn_bf.hip.h"

// ---- what gspx_knn_build and gspx_radius_build share ------------------------------------------------------------
// One pass over the host coordinates: every value must be finite (all d columns).  For the grid search (d <= 3;
// beyond it g.d = 0, no box is taken and the tiled brute force of gspx_knn_bf.hip.h does the search) it leaves the
// grid's defaults and the bounding box's lower corner in g and the box's extents in ext; the caller's rule for the
// cell size finishes g.
static int knn_scan_coords(int64_t N, int d, const double* coords, int metric, KnnGrid& g, double ext[3]) {
  g = KnnGrid{};
  g.d = d <= 3 ? d : 0;
  g.metric = metric;
  g.h_min = 1e300;
  double hi[3] = {0, 0, 0};
  for (int j = 0; j < 3; ++j) {
    g.lo[j] = 0;
    g.inv_h[j] = 1;
    g.n[j] = 1;
  }
  for (int j = 0; j < g.d; ++j) g.lo[j] = hi[j] = coords[j];
  for (int64_t i = 0; i < N; ++i)
    for (int j = 0; j < d; ++j) {
      const double v = coords[i * d + j];
      if (!std::isfinite(v)) return set_err(GSPX_ERR_INVALID, "non-finite coordinate");
      if (j < g.d) {
        g.lo[j] = std::min(g.lo[j], v);
        hi[j] = std::max(hi[j], v);
      }
    }
  for (int j = 0; j < 3; ++j) ext[j] = hi[j] - g.lo[j];
  return GSPX_OK;
}
// most cells per axis, whatever the rule for the cell size asks for
static int knn_axis_cap(int d) { return d == 1 ? (1 << 21) : (d == 2 ? 2048 : 128); }

// The grid index of a cloud on the device (d <= 3 only: the brute force allocates none of this): the points are
// counted into the cells of a finished KnnGrid, an exclusive scan of the counts gives every cell its range (start),
// the points are scattered into cell order and every cell's members sorted by index (order), and the coordinates
// gathered in that order (sorted).  The query kernels read those three.  alloc() and build() are two calls because a
// builder allocates all it needs for the search first, in one fixed order, and only then queues the upload of the
// cloud (profiles/knn_refactor.md: the 1M-point build in one dimension was timed with the index allocated after it).
struct KnnGridIndex {
  DevMem sorted, order, start;  // N x d doubles, N, ncells + 1
  DevMem cell, count, cursor;   // what the chain needs on the way
  int ncells = 0;
  size_t cell_bytes = 0;
  int alloc(int N, const KnnGrid& g) {
    ncells = g.n[0] * g.n[1] * g.n[2];  // (at most 2^22: knn_axis_cap)
    cell_bytes = ((size_t)ncells + 1) * sizeof(int);
    CHK(sorted.alloc((size_t)N * g.d * sizeof(double)));
    CHK(cell.alloc((size_t)N * sizeof(int)));
    CHK(count.alloc(cell_bytes));
    CHK(start.alloc(cell_bytes));
    CHK(cursor.alloc(cell_bytes));
    CHK(order.alloc((size_t)N * sizeof(int)));
    return GSPX_OK;
  }
  int build(gspx_ctx* ctx, const double* x, int N, const KnnGrid& g) {
    hipStream_t st = ctx->stream;
    HIPCHK(hipMemsetAsync(count.p, 0, cell_bytes, st));
    HIPCHK(hipMemsetAsync(cursor.p, 0, cell_bytes, st));
    const int nbN = (N + 255) / 256;
    hipLaunchKernelGGL(k_knn_cell_count, dim3(nbN), dim3(256), 0, st, x, N, g, cell.as<int>(), count.as<int>());
    CHK(scan_exclusive(ctx, count.as<int>(), start.as<int>(), ncells + 1));
    hipLaunchKernelGGL(k_knn_scatter, dim3(nbN), dim3(256), 0, st, cell.as<int>(), N, start.as<int>(),
                       cursor.as<int>(), order.as<int>());
    hipLaunchKernelGGL(k_knn_cell_sort, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, st, start.as<int>(),
                       ncells, order.as<int>(), x, g.d, sorted.as<double>());
    return GSPX_OK;
  }
};

// mean of n distances on the device (sigma when the caller gives none, nngraph.py:218-219 and 248-262): 1024 blocks'
// partial sums, added on the host in index order - sigma's last bits depend on both.  Waits for the stream.  (partial:
// the caller's, so that it is freed with the caller's other buffers, after build_ms is taken.)
static int knn_mean_dist(gspx_ctx* ctx, const double* dist, size_t n, DevMem& partial, double* mean) {
  const int nb = 1024;
  CHK(partial.alloc((size_t)nb * sizeof(double)));
  hipLaunchKernelGGL(k_knn_sum_partial, dim3(nb), dim3(256), 0, ctx->stream, dist, n, partial.as<double>());
  std::vector<double> hp(nb);
  HIPCHK(hipMemcpyAsync(hp.data(), partial.p, nb * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  double s = 0;
  for (double v : hp) s += v;
  *mean = s / (double)n;
  return GSPX_OK;
}

extern "C" int gspx_knn_build(gspx_ctx* ctx, int64_t N, int d, const double* coords, int k,
                              double sigma, int metric, int symmetrize, gspx_knn** out) {
  if (!ctx || !out) return set_err(GSPX_ERR_INVALID, "null ctx or output");
  *out = nullptr;
  if (metric < 0 || metric > 2) return set_err(GSPX_ERR_INVALID, "metric: 0 euclidean, 1 manhattan, 2 max_dist");
  if (symmetrize < 0 || symmetrize > 3)
    return set_err(GSPX_ERR_INVALID, "symmetrize: 0 average, 1 maximum / fill, 2 tril, 3 triu");
  if (N < 2 || N >= ((int64_t)1 << 31) / 64) return set_err(GSPX_ERR_INVALID, "gspx_knn_build: bad N");
  if (d < 1 || d > 4096)
    return set_err(GSPX_ERR_INVALID, "gspx_knn_build: the device k-NN search covers 1 to 4096 dimensions (got %d)", d);
  if (k < 1 || k > 64) return set_err(GSPX_ERR_INVALID, "gspx_knn_build: 1 <= k <= 64 (got %d)", k);
  if (k >= N)  // nngraph.py:123-127
    return set_err(GSPX_ERR_INVALID, "The number of neighbors (k=%d) must be smaller than the number of nodes (%lld).",
                   k, (long long)N);
  if (!coords) return set_err(GSPX_ERR_INVALID, "null coordinates");
  if (!(sigma >= 0) || !std::isfinite(sigma)) return set_err(GSPX_ERR_INVALID, "sigma must be >= 0 (0: mean distance)");
  KnnGrid g;
  double ext[3];
  CHK(knn_scan_coords(N, d, coords, metric, g, ext));
  const bool grid_search = g.d > 0;
  // about 2.5 points per cell over the bounding box; degenerate extents get one cell
  const int per_dim =
      std::max(1, std::min(knn_axis_cap(d), (int)std::floor(std::pow((double)N / 2.5, 1.0 / std::max(g.d, 1)))));
  for (int j = 0; j < g.d; ++j) {
    g.n[j] = ext[j] > 0 ? per_dim : 1;
    const double h = ext[j] > 0 ? ext[j] / g.n[j] : 1.0;
    g.inv_h[j] = 1.0 / h;
    if (ext[j] > 0) g.h_min = std::min(g.h_min, h);
  }
  if (g.h_min == 1e300) g.h_min = 1.0;  // all points coincide
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  auto t0 = std::chrono::steady_clock::now();
  std::unique_ptr<gspx_knn> h;
  CHK(adjacency_open(ctx, N, h));
  h->d = d;
  h->k = k;
  const int n = (int)N;
  const size_t nk = (size_t)N * k;
  DevMem x, w, mutual, len, partial;
  KnnGridIndex index;
  CHK(x.alloc((size_t)N * d * sizeof(double)));
  if (grid_search) CHK(index.alloc(n, g));
  CHK(h->nn.alloc(nk * sizeof(int)));
  CHK(h->dist.alloc(nk * sizeof(double)));
  HIPCHK(hipMemcpyAsync(x.p, coords, (size_t)N * d * sizeof(double), hipMemcpyHostToDevice, st));
  if (!grid_search) {
    HIPCHK(hipStreamSynchronize(st));
    CHK(knn_bruteforce(ctx, x.as<double>(), n, d, k, metric, h->nn.as<int>(), h->dist.as<double>(), h->search_stats));
  } else {
    CHK(index.build(ctx, x.as<double>(), n, g));
    const auto query =
        k <= 8 ? k_knn_query<8> : (k <= 16 ? k_knn_query<16> : (k <= 32 ? k_knn_query<32> : k_knn_query<64>));
    hipLaunchKernelGGL(query, dim3((n + 127) / 128), dim3(128), 0, st, index.sorted.as<double>(), index.order.as<int>(),
                       index.start.as<int>(), n, g, k, h->nn.as<int>(), h->dist.as<double>());
  }
  HIPCHK(hipGetLastError());
  if (sigma == 0.0) {  // the mean neighbour distance (nngraph.py:218-219) unless given
    CHK(knn_mean_dist(ctx, h->dist.as<double>(), nk, partial, &sigma));
    if (!(sigma > 0)) return set_err(GSPX_ERR_INVALID, "gspx_knn_build: all neighbour distances are zero");
  }
  h->sigma = sigma;
  CHK(w.alloc(nk * sizeof(double)));
  CHK(mutual.alloc(nk));
  CHK(len.alloc(((size_t)N + 1) * sizeof(int)));
  const int nbN = (n + 255) / 256;
  const unsigned nbE = (unsigned)((nk + 255) / 256);
  HIPCHK(hipMemsetAsync(len.p, 0, ((size_t)N + 1) * sizeof(int), st));
  hipLaunchKernelGGL(k_knn_weights, dim3(nbE), dim3(256), 0, st, h->nn.as<int>(), h->dist.as<double>(), n, k,
                     sigma, symmetrize, w.as<double>(), mutual.as<unsigned char>(), len.as<int>());
  CHK(adjacency_offsets(h.get(), len.as<int>(), "gspx_knn_build"));
  // (the row lengths are scanned: cleared again, their N + 1 counters are the rows' fill cursors)
  HIPCHK(hipMemsetAsync(len.p, 0, ((size_t)N + 1) * sizeof(int), st));
  hipLaunchKernelGGL(k_knn_fill, dim3(nbE), dim3(256), 0, st, h->nn.as<int>(), w.as<double>(),
                     mutual.as<unsigned char>(), n, k, symmetrize, h->rowptr.as<int>(), len.as<int>(), h->col.as<int>(),
                     h->val.as<double>());
  {
    DevMem col2, val2;
    CHK(col2.alloc((size_t)h->nnz * sizeof(int)));
    CHK(val2.alloc((size_t)h->nnz * sizeof(double)));
    hipLaunchKernelGGL(k_knn_row_rank, dim3(nbN), dim3(256), 0, st, h->rowptr.as<int>(), n, h->col.as<int>(),
                       h->val.as<double>(), col2.as<int>(), val2.as<double>());
    hipLaunchKernelGGL(k_knn_row_rank_long, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, h->rowptr.as<int>(), n,
                       h->col.as<int>(), h->val.as<double>(), col2.as<int>(), val2.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    std::swap(h->col.p, col2.p);      // the sorted arrays become the result; the unsorted ones go with col2 / val2
    std::swap(h->col.bytes, col2.bytes);
    std::swap(h->val.p, val2.p);
    std::swap(h->val.bytes, val2.bytes);
  }
  adjacency_close(h, t0, out);
  return GSPX_OK;
}

extern "C" int gspx_knn_search_stats(gspx_knn* h, double out[4]) {
  if (!h || !out) return set_err(GSPX_ERR_INVALID, "null argument");
  for (int i = 0; i < 4; ++i) out[i] = h->search_stats[i];
  return GSPX_OK;
}

extern "C" int gspx_knn_download_neighbors(gspx_knn* h, int32_t* nn, double* dist) {
  if (!h) return set_err(GSPX_ERR_INVALID, "null handle");
  if (h->k == 0) return set_err(GSPX_ERR_INVALID, "this handle was not built by gspx_knn_build");
  HIPCHK(hipSetDevice(h->ctx->device));
  const size_t nk = (size_t)h->N * h->k;
  if (nn) HIPCHK(hipMemcpy(nn, h->nn.p, nk * sizeof(int), hipMemcpyDeviceToHost));
  if (dist) HIPCHK(hipMemcpy(dist, h->dist.p, nk * sizeof(double), hipMemcpyDeviceToHost));
  return GSPX_OK;
}

// ------------------------------------------------------------------------------------------------
// Radius graphs (NNtype='radius' of NNGraph, nngraph.py:228-287): neighbours = the points within
// epsilon (squared distance <= epsilon^2, the KD-tree's ball query), weights exp(-d^2 / sigma) with
// sigma = mean neighbour distance unless given.  The relation is symmetric and so are the weights, so
// (W + W^T) / 2 = W.  Same grid as the k-NN search with cells of at least epsilon: 3^d cells per query;
// pass 1 counts, pass 2 fills, rows are then sorted by column.
// ------------------------------------------------------------------------------------------------
namespace gspx {

template <int PASS>
__global__ __launch_bounds__(128) void k_radius_query(const double* __restrict__ sorted,
                                                      const int* __restrict__ order,
                                                      const int* __restrict__ start, int N, KnnGrid g,
                                                      double eps2, int* __restrict__ cnt,
                                                      const int* __restrict__ rowptr, int* __restrict__ col,
                                                      double* __restrict__ dist) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= N) return;
  const int self = order[s];
  double q[3] = {0, 0, 0};
  for (int j = 0; j < g.d; ++j) q[j] = sorted[(size_t)s * g.d + j];
  int c[3];
  knn_cell_of(g, q, c);
  const int r2 = g.d >= 2 ? 1 : 0, r3 = g.d >= 3 ? 1 : 0;
  int n = 0;
  const int o = PASS ? rowptr[self] : 0;
  for (int dz = -r3; dz <= r3; ++dz) {
    const int cz = c[2] + dz;
    if (cz < 0 || cz >= g.n[2]) continue;
    for (int dy = -r2; dy <= r2; ++dy) {
      const int cy = c[1] + dy;
      if (cy < 0 || cy >= g.n[1]) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const int cx = c[0] + dx;
        if (cx < 0 || cx >= g.n[0]) continue;
        const int cid = (cz * g.n[1] + cy) * g.n[0] + cx;
        for (int a = start[cid]; a < start[cid + 1]; ++a) {
          const int idx = order[a];
          if (idx == self) continue;
          const double d2 = knn_key(q, sorted + (size_t)a * g.d, g.d, g.metric);
          if (d2 <= eps2) {
            if (PASS) {
              col[o + n] = idx;
              dist[o + n] = g.metric == 0 ? knn_sqrt(d2) : d2;
            }
            ++n;
          }
        }
      }
    }
  }
  if (!PASS) cnt[self] = n;
}
__global__ void k_radius_weights(const double* __restrict__ dist, size_t nnz, double sigma,
                                 double* __restrict__ val) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < nnz) {
    const double d = dist[e];
    val[e] = exp(-(d * d) / sigma);
  }
}

}  // namespace gspx

extern "C" int gspx_radius_build(gspx_ctx* ctx, int64_t N, int d, const double* coords, double epsilon,
                                 double sigma, int metric, gspx_knn** out) {
  if (!ctx || !out) return set_err(GSPX_ERR_INVALID, "null ctx or output");
  *out = nullptr;
  if (metric < 0 || metric > 2) return set_err(GSPX_ERR_INVALID, "metric: 0 euclidean, 1 manhattan, 2 max_dist");
  if (N < 1 || N >= ((int64_t)1 << 31) / 64) return set_err(GSPX_ERR_INVALID, "gspx_radius_build: bad N");
  if (d < 1 || d > 4096)
    return set_err(GSPX_ERR_INVALID, "gspx_radius_build: the device search covers 1 to 4096 dimensions (got %d)", d);
  if (!coords) return set_err(GSPX_ERR_INVALID, "null coordinates");
  if (!(epsilon > 0) || !std::isfinite(epsilon)) return set_err(GSPX_ERR_INVALID, "epsilon must be positive");
  if (!(sigma >= 0) || !std::isfinite(sigma)) return set_err(GSPX_ERR_INVALID, "sigma must be >= 0 (0: mean distance)");
  KnnGrid g;
  double ext[3];
  CHK(knn_scan_coords(N, d, coords, metric, g, ext));
  const bool grid_search = g.d > 0;  // beyond three dimensions: MFMA candidate sweep + exact test (gspx_knn_bf.hip.h)
  // cells of at least epsilon (a little more, against rounding at the walls), at most knn_axis_cap per axis
  for (int j = 0; j < g.d; ++j) {
    int n = ext[j] > 0 ? (int)std::min<double>((double)knn_axis_cap(d), std::floor(ext[j] / (epsilon * 1.0000001))) : 1;
    n = std::max(n, 1);
    const double h = ext[j] > 0 ? ext[j] / n : 1.0;
    g.n[j] = n;
    g.inv_h[j] = 1.0 / h;
    g.h_min = std::min(g.h_min, h);
  }
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  auto t0 = std::chrono::steady_clock::now();
  std::unique_ptr<gspx_knn> h;
  CHK(adjacency_open(ctx, N, h));
  h->d = d;
  const int n = (int)N;
  DevMem x, cnt, partial;
  KnnGridIndex index;
  DevMem c_off, c_buf;  // candidate lists of the brute-force search
  CHK(x.alloc((size_t)N * d * sizeof(double)));
  if (grid_search) CHK(index.alloc(n, g));
  CHK(cnt.alloc(((size_t)N + 1) * sizeof(int)));
  HIPCHK(hipMemcpyAsync(x.p, coords, (size_t)N * d * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(cnt.p, 0, ((size_t)N + 1) * sizeof(int), st));
  const double eps2 = metric == 0 ? epsilon * epsilon : epsilon;  // threshold on the comparison key
  const bool swept = !grid_search && metric == 0 && N > 256;
  const dim3 qgrid((n + 127) / 128), qblock(128);
  if (!grid_search) {
    HIPCHK(hipStreamSynchronize(st));
    if (swept) CHK(radius_candidates(ctx, x.as<double>(), n, d, eps2, c_off, c_buf));
    launch_bf_radius<0>(ctx, x.as<double>(), n, d, metric, eps2, swept ? c_off.as<int>() : nullptr,
                        swept ? c_buf.as<int>() : nullptr, cnt.as<int>(), nullptr, nullptr, nullptr);
  } else {
    CHK(index.build(ctx, x.as<double>(), n, g));
    hipLaunchKernelGGL((k_radius_query<0>), qgrid, qblock, 0, st, index.sorted.as<double>(), index.order.as<int>(),
                       index.start.as<int>(), n, g, eps2, cnt.as<int>(), (const int*)nullptr, (int*)nullptr,
                       (double*)nullptr);
  }
  CHK(adjacency_offsets(h.get(), cnt.as<int>(), "gspx_radius_build"));
  const int nnz = (int)h->nnz;
  CHK(h->dist.alloc((size_t)nnz * sizeof(double)));
  if (nnz > 0) {
    if (!grid_search)
      launch_bf_radius<1>(ctx, x.as<double>(), n, d, metric, eps2, swept ? c_off.as<int>() : nullptr,
                          swept ? c_buf.as<int>() : nullptr, nullptr, h->rowptr.as<int>(), h->col.as<int>(),
                          h->dist.as<double>());
    else
      hipLaunchKernelGGL((k_radius_query<1>), qgrid, qblock, 0, st, index.sorted.as<double>(), index.order.as<int>(),
                         index.start.as<int>(), n, g, eps2, (int*)nullptr, h->rowptr.as<int>(), h->col.as<int>(),
                         h->dist.as<double>());
    hipLaunchKernelGGL(k_knn_row_sort, dim3((n + 255) / 256), dim3(256), 0, st, h->rowptr.as<int>(), n, h->col.as<int>(),
                       h->dist.as<double>());
    if (sigma == 0.0) {  // mean neighbour distance (nngraph.py:248-262)
      CHK(knn_mean_dist(ctx, h->dist.as<double>(), (size_t)nnz, partial, &sigma));
      if (!(sigma > 0)) return set_err(GSPX_ERR_INVALID, "gspx_radius_build: all neighbour distances are zero");
    }
    hipLaunchKernelGGL(k_radius_weights, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st,
                       h->dist.as<double>(), (size_t)nnz, sigma, h->val.as<double>());
  } else if (sigma == 0.0) {
    return set_err(GSPX_ERR_INVALID, "No neighbors found");  // nngraph.py:263-264
  }
  h->sigma = sigma;
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  adjacency_close(h, t0, out);
  return GSPX_OK;
}
