// gspx_sbm.hip.h - stochastic block model / Erdos-Renyi sampler on the device (second half).
// Included by gspx.hip after gspx_knn.hip.h (k_knn_row_sort); the result is an adjacency handle, built on the frame of
// gspx_adjacency.hip.h (adjacency_open / _offsets / _close, scan_exclusive).
//
// The reference visits all N^2 ordered pairs in a Python loop and keeps pair (r > c) with probability
// M[z_r][z_c] (pygsp/graphs/stochasticblockmodel.py:125-144; erdosrenyi.py is the one-block case).
// Same distribution in O(edges): the candidates of every block pair (a, b <= a) - a triangle of
// n_a (n_a - 1) / 2 pairs for a == b, a rectangle of n_a n_b otherwise - are cut into chunks; one
// thread walks a chunk by geometric skips (the gap to the next kept pair of independent Bernoulli(p)
// trials is Geometric(p)), so every pair is kept independently with probability p, chunks are
// independent, and no duplicate can arise.  Counter-based random numbers (a hash of seed, chunk and
// draw number): pass 1 counts, pass 2 replays the same stream and emits.  The stream differs from
// numpy's, so graphs are equal in distribution to the reference's, not bit-equal.
#pragma once

namespace gspx {

struct SbmSeg {       // one block pair
  long long total;    // candidate pairs
  long long chunk;    // candidates per chunk
  long long first;    // global index of its first chunk
  double log1mp;      // log(1 - p)  (-inf for p == 1)
  int lo_a, n_a, lo_b, n_b;  // member ranges in `order`
  int kind;           // candidate index -> (r, c): 0 rectangle n_a x n_b, 1 triangle r > c, 2 triangle r >= c
                      // (self-loops allowed), 3 square n_a x n_a without its diagonal (directed, no self-loops)
};
constexpr int GSPX_SBM_DIRECTED = 1, GSPX_SBM_SELF_LOOPS = 2;

__device__ __forceinline__ unsigned long long sbm_hash(unsigned long long x) {  // splitmix64 finaliser
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// u in (0, 1]
__device__ __forceinline__ double sbm_uniform(unsigned long long seed, unsigned long long chunk, unsigned draw) {
  const unsigned long long h = sbm_hash(sbm_hash(seed ^ (chunk * 0xD1B54A32D192ED03ull)) + draw);
  return (double)((h >> 11) + 1) * (1.0 / 9007199254740992.0);
}

// PASS 0: count per chunk; PASS 1: emit (er[], ec[]) at off[chunk] and count degrees
template <int PASS>
__global__ void k_sbm_chunks(const SbmSeg* __restrict__ seg, int nseg, long long nchunks,
                             unsigned long long seed, const int* __restrict__ order,
                             int* __restrict__ cnt, const int* __restrict__ off, int* __restrict__ er,
                             int* __restrict__ ec, int* __restrict__ deg, int directed) {
  const long long ch = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= nchunks) return;
  int lo = 0, hi = nseg - 1;  // last segment whose first chunk is <= ch
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg[mid].first <= ch) lo = mid; else hi = mid - 1;
  }
  const SbmSeg s = seg[lo];
  const long long base = (ch - s.first) * s.chunk;
  const long long len = min(s.chunk, s.total - base);
  long long pos = 0;
  int n = 0;
  const int o = PASS ? off[ch] : 0;
  for (unsigned draw = 0;; ++draw) {
    const double u = sbm_uniform(seed, (unsigned long long)ch, draw);
    const double g = floor(log(u) / s.log1mp);  // failures before the next success
    if (!(g < (double)(len - pos))) break;
    pos += (long long)g;
    if (PASS) {
      const long long idx = base + pos;
      long long r, c;
      if (s.kind == 1) {  // idx = r (r - 1) / 2 + c, r > c
        r = (long long)floor((1.0 + sqrt(1.0 + 8.0 * (double)idx)) * 0.5);
        if (r * (r - 1) / 2 > idx) --r;
        if ((r + 1) * r / 2 <= idx) ++r;
        c = idx - r * (r - 1) / 2;
      } else if (s.kind == 2) {  // idx = r (r + 1) / 2 + c, r >= c
        r = (long long)floor((sqrt(1.0 + 8.0 * (double)idx) - 1.0) * 0.5);
        if (r * (r + 1) / 2 > idx) --r;
        if ((r + 1) * (r + 2) / 2 <= idx) ++r;
        c = idx - r * (r + 1) / 2;
      } else if (s.kind == 3) {  // row r holds its n_a - 1 off-diagonal columns
        r = idx / (s.n_a - 1);
        c = idx - r * (s.n_a - 1);
        if (c >= r) ++c;
      } else {
        r = idx / s.n_b;
        c = idx - r * s.n_b;
      }
      const int vr = order[s.lo_a + (int)r], vc = order[s.lo_b + (int)c];
      er[o + n] = vr;
      ec[o + n] = vc;
      atomicAdd(&deg[vr], 1);
      if (!directed && vr != vc) atomicAdd(&deg[vc], 1);  // (an undirected self-loop is one stored entry)
    }
    ++n;
    ++pos;
    if (pos >= len) break;
  }
  if (!PASS) cnt[ch] = n;
}
__global__ void k_sbm_fill(const int* __restrict__ er, const int* __restrict__ ec, long long m,
                           const int* __restrict__ rowptr, int* __restrict__ cursor, int* __restrict__ col,
                           double* __restrict__ val, int directed) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  const int r = er[e], c = ec[e];
  const int a = rowptr[r] + atomicAdd(&cursor[r], 1);
  col[a] = c;
  val[a] = 1.0;
  if (directed || r == c) return;  // W[r, c] alone / the one entry of a self-loop
  const int b = rowptr[c] + atomicAdd(&cursor[c], 1);
  col[b] = r;
  val[b] = 1.0;
}

}  // namespace gspx

extern "C" int gspx_sbm_build(gspx_ctx* ctx, int64_t N, int k, const int32_t* order, const int64_t* bounds,
                              const double* M, uint64_t seed, gspx_knn** out) {
  return gspx_sbm_build_ex(ctx, N, k, order, bounds, M, seed, 0, out);
}

extern "C" int gspx_sbm_build_ex(gspx_ctx* ctx, int64_t N, int k, const int32_t* order, const int64_t* bounds,
                                 const double* M, uint64_t seed, int flags, gspx_knn** out) {
  if (!ctx || !out) return set_err(GSPX_ERR_INVALID, "null ctx or output");
  *out = nullptr;
  if (N < 1 || N >= ((int64_t)1 << 31) - 1 || k < 1 || k > 4096 || !order || !bounds || !M ||
      (flags & ~(GSPX_SBM_DIRECTED | GSPX_SBM_SELF_LOOPS)))
    return set_err(GSPX_ERR_INVALID, "gspx_sbm_build: bad argument");
  const bool directed = (flags & GSPX_SBM_DIRECTED) != 0, loops = (flags & GSPX_SBM_SELF_LOOPS) != 0;
  if (bounds[0] != 0 || bounds[k] != N) return set_err(GSPX_ERR_INVALID, "gspx_sbm_build: bounds must span [0, N]");
  for (int a = 0; a < k; ++a) {
    if (bounds[a + 1] < bounds[a]) return set_err(GSPX_ERR_INVALID, "gspx_sbm_build: bounds must not decrease");
    for (int b = 0; b < k; ++b) {
      const double p = M[(size_t)a * k + b];
      if (!(p >= 0.0 && p <= 1.0)) return set_err(GSPX_ERR_INVALID, "Probabilities should be in [0, 1].");
      if (!directed && p != M[(size_t)b * k + a])
        return set_err(GSPX_ERR_INVALID, "gspx_sbm_build: M must be symmetric (undirected graphs)");
    }
  }
  std::vector<SbmSeg> segs;
  long long nchunks = 0;
  // undirected: the block pairs (a, b <= a), the reference's r >= c half (stochasticblockmodel.py:129, mirrored
  // by utils.symmetrize 'tril'); directed: all k^2 ordered block pairs, entry W[r, c] alone
  for (int a = 0; a < k; ++a)
    for (int b = 0; b <= (directed ? k - 1 : a); ++b) {
      const double p = M[(size_t)a * k + b];
      const long long na = bounds[a + 1] - bounds[a], nbk = bounds[b + 1] - bounds[b];
      int kind = 0;
      long long total = na * nbk;
      if (a == b && !directed) {
        kind = loops ? 2 : 1;
        total = loops ? na * (na + 1) / 2 : na * (na - 1) / 2;
      } else if (a == b && !loops) {
        kind = 3;
        total = na * (na - 1);
      }
      if (p <= 0.0 || total <= 0) continue;
      SbmSeg s{};
      s.total = total;
      s.kind = kind;
      long long c = 64;  // about 16 kept pairs per chunk
      while (c < ((long long)1 << 22) && (double)c * p < 16.0) c <<= 1;
      s.chunk = c;
      s.first = nchunks;
      s.log1mp = std::log1p(-p);
      s.lo_a = (int)bounds[a];
      s.n_a = (int)na;
      s.lo_b = (int)bounds[b];
      s.n_b = (int)nbk;
      nchunks += (total + c - 1) / c;
      segs.push_back(s);
    }
  if (nchunks >= ((long long)1 << 31)) return set_err(GSPX_ERR_INVALID, "gspx_sbm_build: too many candidate chunks");
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  auto t0 = std::chrono::steady_clock::now();
  std::unique_ptr<gspx_knn> h;
  CHK(adjacency_open(ctx, N, h));
  const int n = (int)N;
  DevMem dseg, dorder, cnt, off, er, ec, deg, cursor;
  CHK(deg.alloc(((size_t)N + 1) * sizeof(int)));
  HIPCHK(hipMemsetAsync(deg.p, 0, ((size_t)N + 1) * sizeof(int), st));
  long long m = 0;
  if (nchunks > 0) {
    CHK(dseg.alloc(segs.size() * sizeof(SbmSeg)));
    CHK(dorder.alloc((size_t)N * sizeof(int)));
    CHK(cnt.alloc(((size_t)nchunks + 1) * sizeof(int)));
    CHK(off.alloc(((size_t)nchunks + 1) * sizeof(int)));
    HIPCHK(hipMemcpyAsync(dseg.p, segs.data(), segs.size() * sizeof(SbmSeg), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dorder.p, order, (size_t)N * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(cnt.p, 0, ((size_t)nchunks + 1) * sizeof(int), st));
    const unsigned nbc = (unsigned)((nchunks + 255) / 256);
    hipLaunchKernelGGL((k_sbm_chunks<0>), dim3(nbc), dim3(256), 0, st, dseg.as<SbmSeg>(), (int)segs.size(), nchunks,
                       (unsigned long long)seed, dorder.as<int>(), cnt.as<int>(), (const int*)nullptr,
                       (int*)nullptr, (int*)nullptr, (int*)nullptr, directed ? 1 : 0);
    int mi = 0;
    CHK(scan_exclusive(ctx, cnt.as<int>(), off.as<int>(), (int)nchunks + 1, &mi));
    if (mi < 0 || (long long)mi * 2 >= ((long long)1 << 31))
      return set_err(GSPX_ERR_INVALID, "gspx_sbm_build: more than 2^30 edges");
    m = mi;
    CHK(er.alloc((size_t)std::max<long long>(m, 1) * sizeof(int)));
    CHK(ec.alloc((size_t)std::max<long long>(m, 1) * sizeof(int)));
    hipLaunchKernelGGL((k_sbm_chunks<1>), dim3(nbc), dim3(256), 0, st, dseg.as<SbmSeg>(), (int)segs.size(), nchunks,
                       (unsigned long long)seed, dorder.as<int>(), (int*)nullptr, off.as<int>(), er.as<int>(),
                       ec.as<int>(), deg.as<int>(), directed ? 1 : 0);
  }
  // (nnz: 2 m for an undirected graph without self-loops; fewer with them, m when directed)
  CHK(adjacency_offsets(h.get(), deg.as<int>(), "gspx_sbm_build"));
  if (m > 0) {
    CHK(cursor.alloc(((size_t)N + 1) * sizeof(int)));
    HIPCHK(hipMemsetAsync(cursor.p, 0, ((size_t)N + 1) * sizeof(int), st));
    hipLaunchKernelGGL(k_sbm_fill, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, er.as<int>(), ec.as<int>(),
                       m, h->rowptr.as<int>(), cursor.as<int>(), h->col.as<int>(), h->val.as<double>(), directed ? 1 : 0);
    hipLaunchKernelGGL(k_knn_row_sort, dim3((n + 255) / 256), dim3(256), 0, st, h->rowptr.as<int>(), n,
                       h->col.as<int>(), h->val.as<double>());
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  adjacency_close(h, t0, out);
  return GSPX_OK;
}
