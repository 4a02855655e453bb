// gspx_cluster.hip.h - k-means on a row-major fp64 panel: Lloyd's assignment and update, k-means++ seeding, row
// normalisation.  No atomics, the same bits on every call; every sum has one fixed order, which
// pygsp_amd/clustering.py restates in numpy (kmeans_host).  gfx950 only.
// After gspx_ops.hip.h (sum_parts of gspx_reduce.hip.h, finish_timed, DevMem, HIPCHK, CHK).
//
// X is N x d with pitch ldx >= d.  1 <= d <= 128, 1 <= C <= min(N, 1024), C * d <= 8192 (64 KiB of centroids; the
// assignment kernel's padded LDS image is at most 91 456 bytes, k_km_partial's LDS at most 79 872: km_lds_attr).  Squared distances are acc = acc + (x_j - c_j) * (x_j - c_j) for j = 0 .. d - 1 in that order, without FMA
// contraction.
//
// How rows reach the threads: k_stage8 brings eight columns of 256 "thread rows" into LDS with 64-byte row segments
// per eight lanes (pitch 9 doubles: the transposed read is conflict-free), and each thread picks up its own eight
// values.  No thread walks global memory at stride d.
#pragma once

namespace gspx {

constexpr int KM_ROWS = 1024;   // rows per block of the update and seeding sums: a constant of the library
constexpr int KM_MAX_D = 128, KM_MAX_C = 1024, KM_MAX_CD = 8192;
constexpr int KM_STAGE = 256 * 9;  // doubles of one staging tile

// lanes per row of the assignment kernel: a lane keeps at most 32 coordinates in registers
__host__ __device__ inline int km_lanes(int d) { return d <= 32 ? 1 : d <= 64 ? 2 : 4; }

// Stage columns [j0, j0 + 8) of every thread row's segment into sc[256][9] (zeros outside the panel).  P lanes per row,
// segments of S columns: thread row v (= the thread index that will read it) is wave v / 64, lane v % 64, segment
// g = lane / (64 / P), row row0 + wave * (64 / P) + lane % (64 / P); its column j is panel column g * S + j.
// P = 1, S = d: thread row v is row row0 + v.  The caller puts barriers around it.
template <int P>
__device__ inline void k_stage8(const double* __restrict__ X, int64_t ldx, int64_t N, int d, int S, int64_t row0, int j0,
                                double* __restrict__ sc) {
  constexpr int RWL = 64 / P;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int e = threadIdx.x + 256 * i, v = e >> 3, col = e & 7;
    const int vl = v & 63, g = vl / RWL;
    const int64_t r = row0 + (v >> 6) * RWL + vl % RWL;
    const int jj = j0 + col, gc = g * S + jj;
    sc[v * 9 + col] = (r < N && jj < S && gc < d) ? X[r * ldx + gc] : 0.0;
  }
}

// ---- assignment -------------------------------------------------------------------------------------------------
// A workgroup takes 256 / P rows, P = km_lanes(d) lanes per row, each lane S = ceil(d / P) <= 32 coordinates of its row
// in registers.  The centroids are staged in LDS after the rows have gone through the same LDS, segment by segment:
// centroid c at pitch P S4, S4 = S rounded up to four, segment g at g S4, zeros behind its columns.  A zero of x
// against a zero of c adds (0 - 0) (0 - 0) = +0, which changes no sum, so the inner loop runs in groups of four terms
// with one scalar branch per group and no per-lane test.  Every read of c_j is one address per lane group (an LDS
// broadcast).  For P > 1 the lane groups of a wave form a pipeline: in step s group g continues centroid s - g from
// the running sum group g - 1 handed over (one shuffle per centroid), so each distance is still one sequential sum
// over j.  The last group takes the argmin, ties to the smaller index (strict <, centroids in increasing order).
// Per workgroup: part[2 b] = the sum of its rows' minimum distances, part[2 b + 1] = the number of labels that
// changed (`first`: every row), both by the halving tree v[i] += v[i + h], h = 128 / P ... 1.
__host__ __device__ inline int km_pitch(int d) {  // doubles per centroid in the assignment kernel's LDS image
  const int P = km_lanes(d), S = (d + P - 1) / P;
  return P * ((S + 3) / 4 * 4);
}

template <int P>
__global__ __launch_bounds__(256) void k_km_assign(const double* __restrict__ X, int64_t ldx, int64_t N, int d, int C,
                                                   const double* __restrict__ cent, int first, int* __restrict__ label,
                                                   double* __restrict__ mind, double* __restrict__ part) {
#pragma clang fp contract(off)
  typedef double d2 __attribute__((ext_vector_type(2)));
  extern __shared__ __attribute__((aligned(16))) double km_lds[];
  constexpr int RWL = 64 / P, RB = 256 / P;
  const int S = (d + P - 1) / P, S4 = (S + 3) / 4 * 4, dp = P * S4;
  const int CP = C * dp;
  double* red = km_lds + (CP > KM_STAGE ? CP : KM_STAGE);  // [2][256]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int g = lane / RWL, rr = lane % RWL;
  const int64_t row0 = (int64_t)blockIdx.x * RB;
  const int64_t row = row0 + w * RWL + rr;
  double x[32];
#pragma unroll
  for (int j = 0; j < 32; ++j) x[j] = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (8 * q < S) {  // (the same in every thread)
      __syncthreads();
      k_stage8<P>(X, ldx, N, d, S, row0, 8 * q, km_lds);
      __syncthreads();
#pragma unroll
      for (int col = 0; col < 8; ++col) x[8 * q + col] = km_lds[t * 9 + col];
    }
  }
  __syncthreads();
  for (int i = t; i < CP; i += 256) {
    const int c = i / dp, r = i - c * dp;
    const int sg = r / S4, j = r - sg * S4, col = sg * S + j;
    km_lds[i] = (j < S && col < d) ? cent[c * d + col] : 0.0;
  }
  __syncthreads();
  double best = INFINITY, prev = 0.0;
  int bi = 0;
  for (int s = 0; s < C + P - 1; ++s) {
    const int c = s - g;
    const int cc = min(max(c, 0), C - 1);
    double acc = 0.0;
    if constexpr (P > 1) {
      const double in = __shfl(prev, (lane - RWL) & 63);
      acc = g == 0 ? 0.0 : in;
    }
    const d2* __restrict__ cp2 = (const d2*)(km_lds + cc * dp + g * S4);  // (dp and S4 are multiples of four)
    // (no `break` in the unrolled body: with one, the loop is not fully unrolled and x[] goes to scratch)
#pragma unroll
    for (int j4 = 0; j4 < 8; ++j4) {
      if (4 * j4 < S) {
        const d2 c01 = cp2[2 * j4], c23 = cp2[2 * j4 + 1];  // (16-byte aligned: one ds_read_b128 each)
        const double cv[4] = {c01.x, c01.y, c23.x, c23.y};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double df = x[4 * j4 + j] - cv[j];
          acc = acc + df * df;
        }
      }
    }
    prev = acc;
    if (g == P - 1 && c >= 0 && c < C && acc < best) {
      best = acc;
      bi = c;
    }
  }
  const int ri = w * RWL + rr;
  if (g == P - 1) {
    double md = 0.0, ch = 0.0;
    if (row < N) {
      ch = (first || label[row] != bi) ? 1.0 : 0.0;
      md = best;
      label[row] = bi;
      if (mind) mind[row] = best;
    }
    red[ri] = md;
    red[256 + ri] = ch;
  }
  __syncthreads();
  for (int h = RB / 2; h > 0; h >>= 1) {
    if (t < h) {
      red[t] = red[t] + red[t + h];
      red[256 + t] = red[256 + t] + red[256 + t + h];
    }
    __syncthreads();
  }
  if (t == 0) {
    part[2 * (size_t)blockIdx.x] = red[0];
    part[2 * (size_t)blockIdx.x + 1] = red[256];
  }
}

// ---- update: per-block partial sums -------------------------------------------------------------------------------
// Block b takes rows [b KM_ROWS, (b + 1) KM_ROWS) in four sub-tiles of 256.  Per sub-tile the rows are ordered by
// (label, row) with a counting sort in LDS - each thread counts, over the 256 labels, the rows that come before its
// own - and thread p, p + 256, ... < C d (p = c d + j: neighbouring lanes read neighbouring columns of one row) adds
// the members of cluster c in increasing row to its running sum in LDS.  So part[b][c][j] = the sum of x[i][j] over
// the rows i of block b with label c, in increasing i, starting from +0; cntp[b][c] their number.
// Every element of X is read once.
__global__ __launch_bounds__(256) void k_km_partial(const double* __restrict__ X, int64_t ldx, int64_t N, int d, int C,
                                                    const int* __restrict__ label, double* __restrict__ part,
                                                    int* __restrict__ cntp) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double km_lds[];
  const int CD = C * d, t = threadIdx.x;
  double* acc = km_lds;                      // [C d]
  int* lab = (int*)(km_lds + CD);            // [256]
  int* ord = lab + 256;                      // [256]
  int* cstart = ord + 256;                   // [C]
  int* ccnt = cstart + C;                    // [C]
  int* ctot = ccnt + C;                      // [C]
  const int64_t base = (int64_t)blockIdx.x * KM_ROWS;
  for (int i = t; i < CD; i += 256) acc[i] = 0.0;
  for (int i = t; i < C; i += 256) ctot[i] = 0;
  for (int sub = 0; sub < KM_ROWS / 256; ++sub) {
    const int64_t r0 = base + sub * 256;
    if (r0 >= N) break;
    __syncthreads();
    const int64_t row = r0 + t;
    const int l = row < N ? label[row] : 0x7fffffff;
    lab[t] = l;
    for (int i = t; i < C; i += 256) ccnt[i] = 0;
    __syncthreads();
    int pos = 0, rank = 0, tot = 0;
    for (int r = 0; r < 256; ++r) {
      const int l2 = lab[r];
      const int same = l2 == l, before = same & (r < t);
      pos += (l2 < l) | before;
      rank += before;
      tot += same;
    }
    if (row < N && (unsigned)l < (unsigned)C) {
      ord[pos] = t;
      if (rank == 0) {
        cstart[l] = pos;
        ccnt[l] = tot;
      }
    }
    __syncthreads();
    for (int p = t; p < CD; p += 256) {
      const int c = p / d, j = p - c * d;
      const int n = ccnt[c];
      if (n > 0) {
        const int s0 = cstart[c];
        double a = acc[p];
        for (int m = 0; m < n; ++m) a = a + X[(r0 + ord[s0 + m]) * ldx + j];
        acc[p] = a;
      }
    }
    for (int i = t; i < C; i += 256) ctot[i] += ccnt[i];
  }
  __syncthreads();
  double* out = part + (size_t)blockIdx.x * CD;
  for (int i = t; i < CD; i += 256) out[i] = acc[i];
  for (int i = t; i < C; i += 256) cntp[(size_t)blockIdx.x * C + i] = ctot[i];
}

// ---- update: centroids ------------------------------------------------------------------------------------------
// One thread per (c, j): the sum of part[b][c][j] over b = 0, 1, ... in that order, divided by the count; a cluster
// without members keeps its centroid.
__global__ __launch_bounds__(256) void k_km_finish(const double* __restrict__ part, const int* __restrict__ cntp, int nb,
                                                   int C, int d, double* __restrict__ cent) {
#pragma clang fp contract(off)
  const int CD = C * d;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= CD) return;
  const int c = p / d;
  int64_t n = 0;
  double s = 0.0;
  int b = 0;
  for (; b + 4 <= nb; b += 4) {
    const double v0 = part[(size_t)b * CD + p], v1 = part[(size_t)(b + 1) * CD + p];
    const double v2 = part[(size_t)(b + 2) * CD + p], v3 = part[(size_t)(b + 3) * CD + p];
    n += (int64_t)cntp[(size_t)b * C + c] + cntp[(size_t)(b + 1) * C + c] + cntp[(size_t)(b + 2) * C + c] +
         cntp[(size_t)(b + 3) * C + c];
    s = s + v0;
    s = s + v1;
    s = s + v2;
    s = s + v3;
  }
  for (; b < nb; ++b) {
    n += cntp[(size_t)b * C + c];
    s = s + part[(size_t)b * CD + p];
  }
  if (n > 0) cent[p] = s / (double)n;
}

// ---- seeding ----------------------------------------------------------------------------------------------------
// D2[i] = min(D2[i], dist(i, centre)) (`first`: = dist) over block b's rows, one thread per row, the row streamed
// through LDS eight columns at a time; bsum[b] = the sum of the block's KM_ROWS values (zeros past N) by the halving
// tree v[i] += v[i + h], h = 512 ... 1.
__global__ __launch_bounds__(256) void k_km_seed_step(const double* __restrict__ X, int64_t ldx, int64_t N, int d,
                                                      const double* __restrict__ centre, int first,
                                                      double* __restrict__ D2, double* __restrict__ bsum) {
#pragma clang fp contract(off)
  __shared__ double sc[KM_STAGE];
  __shared__ double cs[KM_MAX_D];
  __shared__ double dv[KM_ROWS];
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * KM_ROWS;
  if (t < d) cs[t] = centre[t];
  for (int sub = 0; sub < KM_ROWS / 256; ++sub) {
    const int64_t r0 = base + sub * 256, row = r0 + t;
    double v = 0.0;
    if (r0 < N) {  // (the same in every thread: the barriers below are met by all or by none)
      double acc = 0.0;
      for (int j0 = 0; j0 < d; j0 += 8) {
        __syncthreads();
        k_stage8<1>(X, ldx, N, d, d, r0, j0, sc);
        __syncthreads();
#pragma unroll
        for (int col = 0; col < 8; ++col)
          if (j0 + col < d) {
            const double df = sc[t * 9 + col] - cs[j0 + col];
            acc = acc + df * df;
          }
      }
      if (row < N) {
        const double old = first ? acc : D2[row];
        v = acc < old ? acc : old;
        D2[row] = v;
      }
    }
    dv[sub * 256 + t] = v;
  }
  __syncthreads();
  for (int h = KM_ROWS / 2; h > 0; h >>= 1) {
    for (int i = t; i < h; i += 256) dv[i] = dv[i] + dv[i + h];
    __syncthreads();
  }
  if (t == 0) bsum[blockIdx.x] = dv[0];
}

// ---- row normalisation --------------------------------------------------------------------------------------------
// In place: row i divided by sqrt of acc = acc + x_j * x_j, j = 0 .. d - 1; a row of zeros stays.  256 rows per
// workgroup, one thread per row, read and written through the staging tile.
__global__ __launch_bounds__(256) void k_km_rows_normalize(double* __restrict__ X, int64_t ldx, int64_t N, int d) {
#pragma clang fp contract(off)
  __shared__ double sc[KM_STAGE];
  const int t = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * 256;
  double acc = 0.0;
  for (int j0 = 0; j0 < d; j0 += 8) {
    __syncthreads();
    k_stage8<1>(X, ldx, N, d, d, r0, j0, sc);
    __syncthreads();
#pragma unroll
    for (int col = 0; col < 8; ++col) {
      const double xv = sc[t * 9 + col];  // (zeros past column d)
      acc = acc + xv * xv;
    }
  }
  const double nrm = sqrt(acc);
  for (int j0 = 0; j0 < d; j0 += 8) {
    __syncthreads();
    k_stage8<1>(X, ldx, N, d, d, r0, j0, sc);
    __syncthreads();
    if (nrm > 0.0)
#pragma unroll
      for (int col = 0; col < 8; ++col) sc[t * 9 + col] = sc[t * 9 + col] / nrm;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = t + 256 * i, v = e >> 3, col = e & 7;
      const int64_t r = r0 + v;
      if (r < N && j0 + col < d) X[r * ldx + j0 + col] = sc[v * 9 + col];
    }
  }
}

}  // namespace gspx

// ---- host side --------------------------------------------------------------------------------------------------
static int km_check(const char* who, gspx_ctx* ctx, int64_t N, int d, int C, const void* X, int64_t ldx) {
  if (!ctx || !X) return set_err(GSPX_ERR_INVALID, "%s: null argument", who);
  if (N < 1) return set_err(GSPX_ERR_INVALID, "%s: needs at least one row, got N = %lld", who, (long long)N);
  if (d < 1 || d > gspx::KM_MAX_D)
    return set_err(GSPX_ERR_INVALID, "%s: 1 <= d <= %d columns, got %d", who, gspx::KM_MAX_D, d);
  if (ldx < d) return set_err(GSPX_ERR_INVALID, "%s: pitch %lld is less than d = %d", who, (long long)ldx, d);
  if (C < 1 || C > gspx::KM_MAX_C || C > N)
    return set_err(GSPX_ERR_INVALID, "%s: 1 <= n_clusters <= min(N, %d), got %d (N = %lld)", who, gspx::KM_MAX_C, C,
                   (long long)N);
  if ((int64_t)C * d > gspx::KM_MAX_CD)
    return set_err(GSPX_ERR_INVALID, "%s: n_clusters * d <= %d (64 KiB of centroids), got %d * %d", who,
                   gspx::KM_MAX_CD, C, d);
  if ((N + 63) / 64 > 0x7fffffff) return set_err(GSPX_ERR_INVALID, "%s: N = %lld is too large", who, (long long)N);
  return GSPX_OK;
}

static int km_lds_attr(const void* kern, size_t lds) {
  if (lds > ((size_t)64 << 10))
    HIPCHK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return GSPX_OK;
}

extern "C" int gspx_kmeans_block_rows(int d, int* update_rows, int* assign_rows) {
  if (d < 1 || d > gspx::KM_MAX_D)
    return set_err(GSPX_ERR_INVALID, "kmeans_block_rows: 1 <= d <= %d columns, got %d", gspx::KM_MAX_D, d);
  if (update_rows) *update_rows = gspx::KM_ROWS;
  if (assign_rows) *assign_rows = 256 / gspx::km_lanes(d);
  return GSPX_OK;
}

extern "C" int gspx_kmeans_dev(gspx_ctx* ctx, int64_t N, int d, int C, const double* X, int64_t ldx, double* cent,
                               int64_t max_iter, int32_t* labels, double* mind, double* inertia, int64_t* n_iter,
                               int32_t* converged, double* kernel_ms) {
  if (inertia) *inertia = 0;
  if (n_iter) *n_iter = 0;
  if (converged) *converged = 0;
  if (kernel_ms) *kernel_ms = 0;
  CHK(km_check("kmeans", ctx, N, d, C, X, ldx));
  if (!cent || !labels) return set_err(GSPX_ERR_INVALID, "kmeans: null centroids or labels");
  if (max_iter < 0) return set_err(GSPX_ERR_INVALID, "kmeans: max_iter must not be negative");
  hipStream_t st = ctx->stream;
  replay_reset(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  const int P = gspx::km_lanes(d), CD = C * d;
  const unsigned nba = (unsigned)((N + 256 / P - 1) / (256 / P));
  const unsigned nbu = (unsigned)((N + gspx::KM_ROWS - 1) / gspx::KM_ROWS);
  DevMem apart, tot, part, cntp;
  CHK(apart.alloc((size_t)nba * 2 * sizeof(double)));
  CHK(tot.alloc(2 * sizeof(double)));
  CHK(part.alloc((size_t)nbu * CD * sizeof(double)));
  CHK(cntp.alloc((size_t)nbu * C * sizeof(int)));
  typedef void (*assign_t)(const double*, int64_t, int64_t, int, int, const double*, int, int*, double*, double*);
  const assign_t assign = P == 1 ? gspx::k_km_assign<1> : P == 2 ? gspx::k_km_assign<2> : gspx::k_km_assign<4>;
  const size_t lds_a = ((size_t)std::max(C * gspx::km_pitch(d), gspx::KM_STAGE) + 512) * sizeof(double);
  const size_t lds_u = (size_t)CD * sizeof(double) + (size_t)(512 + 3 * C) * sizeof(int);
  CHK(km_lds_attr((const void*)assign, lds_a));
  CHK(km_lds_attr((const void*)gspx::k_km_partial, lds_u));
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  int64_t done = 0;
  int conv = 0;
  double h[2] = {0, 0};
  for (;;) {
    hipLaunchKernelGGL(assign, dim3(nba), dim3(256), lds_a, st, X, ldx, N, d, C, (const double*)cent, done == 0 ? 1 : 0,
                       labels, mind, apart.as<double>());
    sum_parts(apart.as<double>(), (int)nba, 2, tot.as<double>(), st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, tot.p, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h[1] == 0.0) {
      conv = 1;
      break;
    }
    if (done == max_iter) break;
    hipLaunchKernelGGL(gspx::k_km_partial, dim3(nbu), dim3(256), lds_u, st, X, ldx, N, d, C, (const int*)labels,
                       part.as<double>(), cntp.as<int>());
    hipLaunchKernelGGL(gspx::k_km_finish, dim3((CD + 255) / 256), dim3(256), 0, st, part.as<double>(), cntp.as<int>(),
                       (int)nbu, C, d, cent);
    ++done;
  }
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  CHK(finish_timed(ctx, kernel_ms));
  if (inertia) *inertia = h[0];
  if (n_iter) *n_iter = done;
  if (converged) *converged = conv;
  return GSPX_OK;
}

// The k-means++ rule (restated by clustering.seed_host).  Centre 0 is row floor(u_0 N).  For centre c >= 1, with the
// block sums s_b of D2: run = 0; run += s_b in increasing b; total = the final run.  total == 0 (not > 0): the
// smallest row index not chosen yet.  Otherwise target = u_c total; block = the first b whose run exceeds target, or,
// if none does, the last b with s_b > 0; t = target - (run before that block); inside the block run = 0; run += D2[i]
// in increasing i and the row is the first whose run exceeds t, or, if none does, the block's last row with D2 > 0.
extern "C" int gspx_kmeans_seed_dev(gspx_ctx* ctx, int64_t N, int d, int C, const double* X, int64_t ldx,
                                    const double* u, double* cent, int64_t* chosen, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  CHK(km_check("kmeans_seed", ctx, N, d, C, X, ldx));
  if (!u || !cent || !chosen) return set_err(GSPX_ERR_INVALID, "kmeans_seed: null draws, centroids or output");
  for (int c = 0; c < C; ++c)
    if (!(u[c] >= 0.0 && u[c] < 1.0)) return set_err(GSPX_ERR_INVALID, "kmeans_seed: draw %d is not in [0, 1)", c);
  hipStream_t st = ctx->stream;
  replay_reset(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  const int nb = (int)((N + gspx::KM_ROWS - 1) / gspx::KM_ROWS);
  DevMem D2, bsum;
  CHK(D2.alloc((size_t)nb * gspx::KM_ROWS * sizeof(double)));
  CHK(bsum.alloc((size_t)nb * sizeof(double)));
  std::vector<double> hs((size_t)nb), hd((size_t)gspx::KM_ROWS);
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  for (int c = 0; c < C; ++c) {
    int64_t pick = -1;
    if (c == 0) {
      pick = std::min<int64_t>(N - 1, (int64_t)(u[0] * (double)N));
    } else {
      HIPCHK(hipMemcpyAsync(hs.data(), bsum.p, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      double total = 0.0;
      for (int b = 0; b < nb; ++b) total += hs[b];
      if (!(total > 0.0)) {
        for (int64_t i = 0; i < N && pick < 0; ++i)
          if (std::find(chosen, chosen + c, i) == chosen + c) pick = i;
      } else {
        const double target = u[c] * total;
        int blk = -1, lastpos = -1;
        double run = 0.0, before = 0.0;
        for (int b = 0; b < nb; ++b) {
          const double prev = run;
          run += hs[b];
          if (hs[b] > 0.0) lastpos = b;
          if (run > target) {
            blk = b;
            before = prev;
            break;
          }
        }
        if (blk < 0) {  // rounding left the target at the total: the last block that holds anything
          blk = lastpos;
          before = 0.0;
          for (int b = 0; b < blk; ++b) before += hs[b];
        }
        const int64_t i0 = (int64_t)blk * gspx::KM_ROWS;
        const int cnt = (int)std::min<int64_t>(gspx::KM_ROWS, N - i0);
        HIPCHK(hipMemcpyAsync(hd.data(), D2.as<double>() + i0, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const double t = target - before;
        int in = -1, lastrow = -1;
        double r2 = 0.0;
        for (int i = 0; i < cnt; ++i) {
          r2 += hd[i];
          if (hd[i] > 0.0) lastrow = i;
          if (r2 > t) {
            in = i;
            break;
          }
        }
        if (in < 0) in = lastrow;
        if (in < 0) return set_err(GSPX_ERR_INTERNAL, "kmeans_seed: block %d has no row with D2 > 0", blk);
        pick = i0 + in;
      }
    }
    chosen[c] = pick;
    HIPCHK(hipMemcpyAsync(cent + (size_t)c * d, X + pick * ldx, (size_t)d * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (c + 1 < C)
      hipLaunchKernelGGL(gspx::k_km_seed_step, dim3(nb), dim3(256), 0, st, X, ldx, N, d, (const double*)(cent + (size_t)c * d),
                         c == 0 ? 1 : 0, D2.as<double>(), bsum.as<double>());
  }
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  return finish_timed(ctx, kernel_ms);
}

extern "C" int gspx_rows_normalize_dev(gspx_ctx* ctx, int64_t N, int d, double* X, int64_t ldx, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  if (!ctx || !X) return set_err(GSPX_ERR_INVALID, "rows_normalize: null argument");
  if (N < 1 || d < 1 || ldx < d || (N + 255) / 256 > 0x7fffffff)
    return set_err(GSPX_ERR_INVALID, "rows_normalize: needs N >= 1 rows of 1 <= d <= pitch columns");
  hipStream_t st = ctx->stream;
  replay_reset(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL(gspx::k_km_rows_normalize, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, X, ldx, N, d);
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  return finish_timed(ctx, kernel_ms);
}
