// gspx_eig.hip.h - the full Fourier basis on the device: a dense symmetric fp64 eigensolver by two-sided cyclic block
// Jacobi.  What Graph.compute_fourier_basis(method='jacobi') runs (pygsp_amd/fourier.py:
// device_full_basis); tests/eig_helpers.py restates it in numpy.
//
// The matrix is copied into an npad x npad work matrix, npad = nb * JAC_B (nb >= 2 blocks), whose padding is zero with
// distinct diagonal entries above the Gershgorin bound of A: a scalar rotation is skipped where its off-diagonal entry
// is exactly zero, so the padding never mixes with A, sorts behind it, and the n kept columns have no mass outside the
// first n rows (reported as info[11]).  V starts as the identity.  A sweep visits every unordered block pair once, in
// the round-robin order of jac_round_pair (floor(nb / 2) disjoint pairs per round, an odd block count gets a bye); a
// round is three launches:
//   k_jac_sub   one workgroup per pair: S = sym(A[IJ, IJ]) in LDS, JAC_INNER parallel-order sweeps of scalar Jacobi
//               rotations (Q stays near the identity), Q to memory; or the skip flag when off(S)^2 <= thr2
//   k_jac_cols  A[:, IJ] <- A[:, IJ] Q and V[:, IJ] <- V[:, IJ] Q   (v_mfma_f64_16x16x4f64, each workgroup owns its rows)
//   k_jac_rows  A[IJ, :] <- Q^T A[IJ, :]                            (the same over column tiles)
// Once per sweep k_jac_off sums the squares of the off-diagonal entries of every row directly (not ||A||_F^2 -
// sum a_ii^2, which cancels) and the host adds the rows in order.  The loop stops when off(A) <= tol ||A||_F and no
// row's off-diagonal norm - the residual of that eigenpair - exceeds tol max |a_ii|: the first alone lets one column
// keep a residual of tol ||A||_F, far above tol lambda_max.  A pair is skipped below thr = tol min(||A||_F / nb,
// max |a_ii| / sqrt(nb)): every pair skipped means off(A)^2 <= nb (nb - 1) / 2 thr^2 and every row's nb blocks
// within thr each, so a matrix that only skips has converged.
// The finish gathers the columns in ascending order of diag(A), takes one Newton-Schulz step V <- V (3 I - V^T V) / 2
// (the Gram and X Q kernels of gspx_reduce / gspx_spectral), and recomputes the eigenvalues as Rayleigh quotients
// v_i^T (A v_i) against the caller's A, which is only read.  No atomics; every sum has a fixed order.
// After gspx_spectral.hip.h (k_spectral_apply, k_gram_store, launch_panel_gram, spec_overlap, spec_span).
#pragma once

namespace gspx {

constexpr int JAC_B = 32;            // block size: a pair is a 64 x 64 subproblem
constexpr int JAC_M = 2 * JAC_B;
constexpr int JAC_INNER = 2;         // scalar sweeps per subproblem
constexpr int JAC_KS = JAC_B + 1;    // LDS row strides of the two apply kernels, as k_spectral_apply's
constexpr int JAC_QS = JAC_M + 4;

// pair k (0 <= k < me / 2) of round r (0 <= r < me - 1) over an even field of me players: the circle method with
// player me - 1 fixed.  Used for the blocks of a sweep (host) and for the rows of a subproblem (device, me = 64).
__host__ __device__ inline void jac_round_pair(int me, int r, int k, int* a, int* b) {
  if (k == 0) {
    *a = me - 1;
    *b = r;
  } else {
    *a = (r + k) % (me - 1);
    *b = (r - k + (me - 1)) % (me - 1);
  }
}

// row / column of the work matrix behind index i (0..63) of the pair (bi, bj)
__device__ inline int jac_index(int2 pr, int i) { return (i < JAC_B ? pr.x : pr.y) * JAC_B + (i & (JAC_B - 1)); }

// ---- set-up: row sums, the padded copy ---------------------------------------------------------------------------
// one workgroup per row: out[row] = sum |a|, out[n + row] = sum a^2
__global__ __launch_bounds__(256) void k_jac_rowstats(const double* __restrict__ A, int64_t lda, int n,
                                                      double* __restrict__ out) {
  const int64_t row = blockIdx.x;
  double s[2] = {0, 0};
  for (int c = threadIdx.x; c < n; c += 256) {
    const double v = A[row * lda + c];
    s[0] += fabs(v);
    s[1] += v * v;
  }
  block_sums<2>(s, out + row, (size_t)n);
}

__global__ __launch_bounds__(256) void k_jac_init(const double* __restrict__ A, int64_t lda, int n, double padunit,
                                                  double* __restrict__ Ap, double* __restrict__ Vp, int npad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)npad * npad) return;
  const int r = (int)(i / npad), c = (int)(i % npad);
  double a = 0;
  if (r < n && c < n) a = A[(int64_t)r * lda + c];
  else if (r == c) a = (2.0 + (r - n)) * padunit;
  Ap[i] = a;
  Vp[i] = r == c ? 1.0 : 0.0;
}

// ---- the subproblem of one pair -------------------------------------------------------------------------------------
// S and Q^T are 64 x 64 in LDS (64 KiB).  A step of the parallel order holds 32 disjoint rotations (p_k, q_k): 32 threads
// form (c, s); S <- S J as a column operation (lanes over k, so the strided column reads spread over the banks) and
// Q^T <- J^T Q^T as a row operation; then S <- J^T S as a row operation, with the rotated entry set to zero.
__global__ __launch_bounds__(256) void k_jac_sub(const double* __restrict__ A, int64_t ld,
                                                 const int2* __restrict__ pairs, double thr2, double* __restrict__ Q,
                                                 int* __restrict__ skip) {
  __shared__ double S[JAC_M * JAC_M];
  __shared__ double Qt[JAC_M * JAC_M];
  __shared__ double red[256];
  __shared__ double cs[JAC_B], sn[JAC_B];
  __shared__ int pp[JAC_B], qq[JAC_B];
  const int tid = threadIdx.x;
  const int2 pr = pairs[blockIdx.x];
  for (int idx = tid; idx < JAC_M * JAC_M; idx += 256)
    Qt[idx] = A[(int64_t)jac_index(pr, idx >> 6) * ld + jac_index(pr, idx & 63)];
  __syncthreads();
  double v = 0;
  for (int idx = tid; idx < JAC_M * JAC_M; idx += 256) {
    const int r = idx >> 6, c = idx & 63;
    const double s = 0.5 * (Qt[idx] + Qt[c * JAC_M + r]);
    S[idx] = s;
    if (r != c) v += s * s;
  }
  red[tid] = v;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  const bool skipped = red[0] <= thr2;  // (the same value in every thread)
  if (tid == 0) skip[blockIdx.x] = skipped ? 1 : 0;
  if (skipped) return;
  for (int idx = tid; idx < JAC_M * JAC_M; idx += 256) Qt[idx] = (idx >> 6) == (idx & 63) ? 1.0 : 0.0;
  for (int sw = 0; sw < JAC_INNER; ++sw)
    for (int r = 0; r < JAC_M - 1; ++r) {
      __syncthreads();  // (the previous step's rows are written; Q^T is initialised)
      if (tid < JAC_B) {
        int a, b;
        jac_round_pair(JAC_M, r, tid, &a, &b);
        const int p = min(a, b), q = max(a, b);
        const double app = S[p * JAC_M + p], aqq = S[q * JAC_M + q], apq = S[p * JAC_M + q];
        double c = 1.0, s = 0.0;
        if (apq != 0.0) {
          const double tau = (aqq - app) / (2.0 * apq);
          const double t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
          c = 1.0 / sqrt(1.0 + t * t);
          s = t * c;
        }
        pp[tid] = p;
        qq[tid] = q;
        cs[tid] = c;
        sn[tid] = s;
      }
      __syncthreads();
      // (every phase loads its eight entry pairs before it stores any: the LDS latencies overlap)
      const int col = tid & 63, k0 = tid >> 6;
      int pk[8], qk[8];
      double ck[8], sk[8], xp[8], xq[8], yp[8], yq[8];
      {
        const int k = tid & (JAC_B - 1), p = pp[k], q = qq[k], row0 = tid >> 5;
        const double c = cs[k], s = sn[k];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          pk[i] = pp[k0 + 4 * i];
          qk[i] = qq[k0 + 4 * i];
          ck[i] = cs[k0 + 4 * i];
          sk[i] = sn[k0 + 4 * i];
          xp[i] = S[(row0 + 8 * i) * JAC_M + p];
          xq[i] = S[(row0 + 8 * i) * JAC_M + q];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          yp[i] = Qt[pk[i] * JAC_M + col];
          yq[i] = Qt[qk[i] * JAC_M + col];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          S[(row0 + 8 * i) * JAC_M + p] = c * xp[i] - s * xq[i];
          S[(row0 + 8 * i) * JAC_M + q] = s * xp[i] + c * xq[i];
          Qt[pk[i] * JAC_M + col] = ck[i] * yp[i] - sk[i] * yq[i];
          Qt[qk[i] * JAC_M + col] = sk[i] * yp[i] + ck[i] * yq[i];
        }
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        xp[i] = S[pk[i] * JAC_M + col];
        xq[i] = S[qk[i] * JAC_M + col];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        S[pk[i] * JAC_M + col] = col == qk[i] ? 0.0 : ck[i] * xp[i] - sk[i] * xq[i];
        S[qk[i] * JAC_M + col] = col == pk[i] ? 0.0 : sk[i] * xp[i] + ck[i] * xq[i];
      }
    }
  __syncthreads();
  double* Qp = Q + (size_t)blockIdx.x * (JAC_M * JAC_M);
  for (int idx = tid; idx < JAC_M * JAC_M; idx += 256) Qp[idx] = Qt[(idx & 63) * JAC_M + (idx >> 6)];
}

// ---- X[:, IJ] <- X[:, IJ] Q for X = A (blockIdx.z = 0) and X = V (1) -----------------------------------------------
// grid (row tiles of 64, pairs of the round, 2).  The two 32-column halves of the tile are staged one after the other
// with the matching 32 rows of Q; the tile is stored only after both have been read, and no other workgroup touches
// these rows and columns.  Operand maps as k_spectral_apply.
__global__ __launch_bounds__(256) void k_jac_cols(double* __restrict__ A, double* __restrict__ V, int64_t ld, int npad,
                                                  const int2* __restrict__ pairs, const double* __restrict__ Q,
                                                  const int* __restrict__ skip) {
  if (skip[blockIdx.y]) return;
  __shared__ double xs[JAC_M * JAC_KS];
  __shared__ double qs[JAC_B * JAC_QS];
  double* X = blockIdx.z ? V : A;
  const int2 pr = pairs[blockIdx.y];
  const double* Qp = Q + (size_t)blockIdx.y * (JAC_M * JAC_M);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kq = lane >> 4, cq = lane & 15;
  const int r0 = blockIdx.x * JAC_M;
  spec_d4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = 0;
  for (int h = 0; h < 2; ++h) {
    const int cb = (h ? pr.y : pr.x) * JAC_B;
    __syncthreads();
    for (int idx = tid; idx < JAC_M * JAC_B; idx += 256) {
      const int r = idx / JAC_B, k = idx % JAC_B;
      xs[r * JAC_KS + k] = r0 + r < npad ? X[(int64_t)(r0 + r) * ld + cb + k] : 0.0;
    }
    for (int idx = tid; idx < JAC_B * JAC_M; idx += 256) {
      const int k = idx / JAC_M, c = idx % JAC_M;
      qs[k * JAC_QS + c] = Qp[(h * JAC_B + k) * JAC_M + c];
    }
    __syncthreads();
    for (int kk = 0; kk < JAC_B; kk += 4) {
      const double a = xs[(w * 16 + cq) * JAC_KS + kk + kq];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, qs[(kk + kq) * JAC_QS + j * 16 + cq], acc[j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = r0 + w * 16 + kq + 4 * e;
      if (row < npad) X[(int64_t)row * ld + jac_index(pr, j * 16 + cq)] = acc[j][e];
    }
}

// ---- A[IJ, :] <- Q^T A[IJ, :] ------------------------------------------------------------------------------------------
// grid (column tiles of 64, pairs of the round).  A-operand Q^T[row l % 16][k l / 16] = Q[k][row], B-operand
// A[IJ[k]][column l % 16]; both staged with row stride JAC_QS.
__global__ __launch_bounds__(256) void k_jac_rows(double* __restrict__ A, int64_t ld, int npad,
                                                  const int2* __restrict__ pairs, const double* __restrict__ Q,
                                                  const int* __restrict__ skip) {
  if (skip[blockIdx.y]) return;
  __shared__ double qs[JAC_B * JAC_QS];
  __shared__ double xs[JAC_B * JAC_QS];
  const int2 pr = pairs[blockIdx.y];
  const double* Qp = Q + (size_t)blockIdx.y * (JAC_M * JAC_M);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kq = lane >> 4, cq = lane & 15;
  const int c0 = blockIdx.x * JAC_M;
  spec_d4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = 0;
  for (int h = 0; h < 2; ++h) {
    const int rb = (h ? pr.y : pr.x) * JAC_B;
    __syncthreads();
    for (int idx = tid; idx < JAC_B * JAC_M; idx += 256) {
      const int k = idx / JAC_M, c = idx % JAC_M;
      qs[k * JAC_QS + c] = Qp[(h * JAC_B + k) * JAC_M + c];
      xs[k * JAC_QS + c] = c0 + c < npad ? A[(int64_t)(rb + k) * ld + c0 + c] : 0.0;
    }
    __syncthreads();
    for (int kk = 0; kk < JAC_B; kk += 4) {
      const double a = qs[(kk + kq) * JAC_QS + w * 16 + cq];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xs[(kk + kq) * JAC_QS + j * 16 + cq], acc[j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = c0 + j * 16 + cq;
      if (col < npad) A[(int64_t)jac_index(pr, w * 16 + kq + 4 * e) * ld + col] = acc[j][e];
    }
}

// ---- off(A)^2 by rows, one workgroup per row: out[row] = sum over c != row of a^2, out[npad + row] = a[row][row] ------
__global__ __launch_bounds__(256) void k_jac_off(const double* __restrict__ A, int64_t ld, int npad,
                                                 double* __restrict__ out) {
  const int row = blockIdx.x;
  double s[1] = {0};
  for (int c = threadIdx.x; c < npad; c += 256) {
    const double v = A[(int64_t)row * ld + c];
    if (c != row) s[0] += v * v;
    else out[npad + row] = v;
  }
  block_sums<1>(s, out + row, 1);
}

// ---- the finish ------------------------------------------------------------------------------------------------------
// X[r][c] = V[r][perm[c]] for r, c < n (X contiguous)
__global__ __launch_bounds__(256) void k_jac_gather(const double* __restrict__ V, int64_t ld, const int* __restrict__ perm,
                                                    int n, double* __restrict__ X) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)n * n) return;
  X[i] = V[i / n * ld + perm[i % n]];
}

// out[0] = max |V[r][perm[c]]| over the padding rows r = n .. npad - 1 of the kept columns (one workgroup)
__global__ __launch_bounds__(256) void k_jac_padmass(const double* __restrict__ V, int64_t ld, const int* __restrict__ perm,
                                                     int n, int npad, double* __restrict__ out) {
  __shared__ double red[256];
  double m = 0;
  for (int64_t i = threadIdx.x; i < (int64_t)(npad - n) * n; i += 256)
    m = fmax(m, fabs(V[(n + i / n) * ld + perm[i % n]]));
  red[threadIdx.x] = m;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + h]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

__global__ __launch_bounds__(256) void k_jac_add_diag(double* __restrict__ G, int64_t ld, int n, double v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) G[(int64_t)i * ld + i] += v;
}

// partial[b][c] = sum over the rows of block b of X Y (theta null) or of (Y - theta[c] X)^2; the thread map of
// k_panel_residual: grid.x row blocks, grid.y groups of 64 columns.
__global__ __launch_bounds__(256) void k_jac_coldot(const double* __restrict__ X, int64_t ldx,
                                                    const double* __restrict__ Y, int64_t ldy, int n,
                                                    const double* __restrict__ theta, double* __restrict__ partial) {
  __shared__ double ws[256];
  const int c = blockIdx.y * 64 + (threadIdx.x & 63);
  double s = 0;
  if (c < n) {
    const double th = theta ? theta[c] : 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.x * 4) {
      const double x = X[i * ldx + c], y = Y[i * ldy + c];
      const double d = y - th * x;
      s += theta ? d * d : x * y;
    }
  }
  ws[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < 64 && c < n)
    partial[(size_t)blockIdx.x * n + c] =
        (ws[threadIdx.x] + ws[threadIdx.x + 64]) + (ws[threadIdx.x + 128] + ws[threadIdx.x + 192]);
}

// X[:, c] *= s[c]
__global__ __launch_bounds__(256) void k_scale_cols(double* __restrict__ X, int64_t ldx, int w, int64_t N,
                                                    const double* __restrict__ s) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * w) return;
  X[i / w * ldx + i % w] *= s[i % w];
}

}  // namespace gspx

// ---- host side --------------------------------------------------------------------------------------------------------
static constexpr int EIG_MAX_N = 32768;  // the work matrix, V and the caller's A and V are live together: four n^2 fp64

static int eig_blocks(int n) { return n > 0 ? std::max(2, (n + gspx::JAC_B - 1) / gspx::JAC_B) : 0; }
static int eig_rounds(int nb) { return nb > 0 ? (nb + 1) / 2 * 2 - 1 : 0; }

// the pairs (i < j) of every round of a sweep over nb blocks, round-major, nb / 2 per round
static std::vector<int> eig_schedule(int nb) {
  std::vector<int> out;
  const int me = nb + (nb & 1);
  for (int r = 0; r < eig_rounds(nb); ++r)
    for (int k = 0; k < me / 2; ++k) {
      int a, b;
      gspx::jac_round_pair(me, r, k, &a, &b);
      if (a >= nb || b >= nb) continue;  // the bye
      out.push_back(std::min(a, b));
      out.push_back(std::max(a, b));
    }
  return out;
}

extern "C" int gspx_sym_eig_schedule_describe(int n_blocks, int* pairs_out, int* n_rounds) {
  if (n_blocks < 1 || n_blocks > EIG_MAX_N / gspx::JAC_B)
    return set_err(GSPX_ERR_INVALID, "sym_eig_schedule: n_blocks must be 1..%d (got %d)", EIG_MAX_N / gspx::JAC_B,
                   n_blocks);
  if (!n_rounds) return set_err(GSPX_ERR_INVALID, "sym_eig_schedule: null output");
  *n_rounds = eig_rounds(n_blocks);
  if (pairs_out) {
    const std::vector<int> s = eig_schedule(n_blocks);
    std::copy(s.begin(), s.end(), pairs_out);
  }
  return GSPX_OK;
}

extern "C" int gspx_sym_eig_dev(gspx_ctx* ctx, int n, const double* A, int64_t lda, double* V, int64_t ldv, double* e_host,
                                double tol, int max_sweeps, double* info, int64_t* skipped_per_sweep) {
  if (n < 0) return set_err(GSPX_ERR_INVALID, "sym_eig: negative order");
  if (n > EIG_MAX_N) return set_err(GSPX_ERR_INVALID, "sym_eig: the order must be at most %d (got %d)", EIG_MAX_N, n);
  if (lda < n || ldv < n) return set_err(GSPX_ERR_INVALID, "sym_eig: leading dimension below the order");
  if (!(tol > 0) || !std::isfinite(tol)) return set_err(GSPX_ERR_INVALID, "sym_eig: tol must be positive and finite");
  if (max_sweeps < 1) return set_err(GSPX_ERR_INVALID, "sym_eig: max_sweeps must be at least 1 (got %d)", max_sweeps);
  if (n > 0 && (!A || !V || !e_host)) return set_err(GSPX_ERR_INVALID, "sym_eig: null matrix or output");
  if (n > 0 && spec_overlap(A, spec_span(n, lda, n), V, spec_span(n, ldv, n)))
    return set_err(GSPX_ERR_INVALID, "sym_eig: V must not alias A");
  if (!ctx) return set_err(GSPX_ERR_INVALID, "null context");
  replay_reset(ctx);
  if (info)
    for (int i = 0; i < 12; ++i) info[i] = 0;
  if (n == 0) return GSPX_OK;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const auto wall0 = std::chrono::steady_clock::now();
  const int nb = eig_blocks(n), npad = nb * gspx::JAC_B, nrounds = eig_rounds(nb), ppr = nb / 2;
  const int ntile = (npad + gspx::JAC_M - 1) / gspx::JAC_M;
  const std::vector<int> sched = eig_schedule(nb);
  const size_t npairs = (size_t)nrounds * ppr;
  if (sched.size() != 2 * npairs)
    return set_err(GSPX_ERR_INTERNAL, "sym_eig: the schedule has %zu entries, not %zu", sched.size(), 2 * npairs);

  // work buffers: the padded matrix, V, one Q per pair of a round | pairs, skip flags of a sweep | small vectors
  DevMem ap, vp, qbuf, ibuf, dbuf;
  const size_t nn = (size_t)npad * npad;
  CHK(ap.alloc(nn * sizeof(double)));
  CHK(vp.alloc(nn * sizeof(double)));
  CHK(qbuf.alloc((size_t)ppr * gspx::JAC_M * gspx::JAC_M * sizeof(double)));
  CHK(ibuf.alloc((3 * npairs + (size_t)npad) * sizeof(int)));
  const int nbk = std::min(1024, (n + 63) / 64);  // row blocks of k_jac_coldot
  CHK(dbuf.alloc(((size_t)2 * npad + 1 + (size_t)(nbk + 2) * n) * sizeof(double)));
  double* Ap = ap.as<double>();
  double* Vp = vp.as<double>();
  double* Q = qbuf.as<double>();
  int2* pairs = (int2*)ibuf.as<int>();
  int* skip = ibuf.as<int>() + 2 * npairs;
  int* perm = skip + npairs;
  double* rowstat = dbuf.as<double>();           // 2 npad: row sums, then the rows' off-norms (npad) and diag (npad)
  double* padmass = rowstat + 2 * (size_t)npad;  // 1
  double* evals = padmass + 1;                   // n
  double* resid = evals + n;                     // n
  double* colpart = resid + n;                   // nbk n

  // timing events: one chain per sweep (3 per round + 3), read after the sweep's sync
  const size_t nev = 3 * (size_t)nrounds + 4;
  while (ctx->ev_pool.size() < nev) {
    hipEvent_t e = nullptr;
    HIPCHK(hipEventCreate(&e));
    ctx->ev_pool.push_back(e);
  }
  double ms_stage[5] = {0, 0, 0, 0, 0};  // sub, cols, rows, off, finish
  auto elapsed = [&](size_t i, size_t j, double* into) -> int {
    float f = 0;
    HIPCHK(hipEventElapsedTime(&f, ctx->ev_pool[i], ctx->ev_pool[j]));
    *into += f;
    return GSPX_OK;
  };

  // ||A||_F, the Gershgorin bound, the padded copy
  std::vector<double> hrow(2 * (size_t)n);
  hipLaunchKernelGGL(gspx::k_jac_rowstats, dim3(n), dim3(256), 0, st, A, lda, n, rowstat);
  HIPCHK(hipMemcpyAsync(hrow.data(), rowstat, hrow.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(pairs, sched.data(), sched.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  double gersh = 0, norm2 = 0;
  for (int i = 0; i < n; ++i) {
    gersh = std::max(gersh, hrow[i]);
    norm2 += hrow[n + i];
  }
  if (!std::isfinite(norm2) || !std::isfinite(gersh))
    return set_err(GSPX_ERR_INVALID, "sym_eig: the matrix has non-finite entries");
  const double norm = std::sqrt(norm2);
  hipLaunchKernelGGL(gspx::k_jac_init, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, A, lda, n,
                     std::max(gersh, 1.0), Ap, Vp, npad);

  int sweeps = 0;
  int64_t skipped_total = 0;
  double off = 0;
  std::vector<int> hskip(npairs);
  std::vector<double> hoff(2 * (size_t)npad);  // the rows' squared off-norms, then the diagonal
  for (;;) {
    HIPCHK(hipEventRecord(ctx->ev_pool[0], st));
    hipLaunchKernelGGL(gspx::k_jac_off, dim3(npad), dim3(256), 0, st, Ap, (int64_t)npad, npad, rowstat);
    HIPCHK(hipEventRecord(ctx->ev_pool[1], st));
    HIPCHK(hipMemcpyAsync(hoff.data(), rowstat, hoff.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    CHK(elapsed(0, 1, &ms_stage[3]));
    double off2 = 0, worst2 = 0, rho = 0;
    for (int i = 0; i < npad; ++i) {
      off2 += hoff[i];
      worst2 = std::max(worst2, hoff[i]);
    }
    for (int i = 0; i < n; ++i) rho = std::max(rho, std::fabs(hoff[npad + i]));
    off = std::sqrt(off2);
    if (off <= tol * norm && std::sqrt(worst2) <= tol * rho) break;
    if (!(off == off)) return set_err(GSPX_ERR_INTERNAL, "sym_eig: the off-diagonal norm is not a number");
    const double thr = tol * std::min(norm / nb, rho / std::sqrt((double)nb)), thr2 = thr * thr;
    if (sweeps >= max_sweeps) {
      if (info) {
        info[0] = sweeps;
        info[1] = off / norm;
        info[2] = (double)((int64_t)npairs * sweeps - skipped_total);
        info[3] = (double)skipped_total;
      }
      return set_err(GSPX_ERR_NOCONV, "sym_eig: no convergence in %d sweeps: off(A) / ||A||_F = %.3e against tol = %.3e.  "
                     "Raise max_sweeps or tol.", max_sweeps, off / norm, tol);
    }
    size_t ev = 2;
    HIPCHK(hipEventRecord(ctx->ev_pool[ev], st));
    for (int r = 0; r < nrounds; ++r) {
      const int2* pr = pairs + (size_t)r * ppr;
      int* sk = skip + (size_t)r * ppr;
      hipLaunchKernelGGL(gspx::k_jac_sub, dim3(ppr), dim3(256), 0, st, Ap, (int64_t)npad, pr, thr2, Q, sk);
      HIPCHK(hipEventRecord(ctx->ev_pool[ev + 1], st));
      hipLaunchKernelGGL(gspx::k_jac_cols, dim3(ntile, ppr, 2), dim3(256), 0, st, Ap, Vp, (int64_t)npad, npad, pr, Q, sk);
      HIPCHK(hipEventRecord(ctx->ev_pool[ev + 2], st));
      hipLaunchKernelGGL(gspx::k_jac_rows, dim3(ntile, ppr), dim3(256), 0, st, Ap, (int64_t)npad, npad, pr, Q, sk);
      HIPCHK(hipEventRecord(ctx->ev_pool[ev + 3], st));
      ev += 3;
    }
    HIPCHK(hipMemcpyAsync(hskip.data(), skip, npairs * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    for (size_t i = 2; i < ev; i += 3) {
      CHK(elapsed(i, i + 1, &ms_stage[0]));
      CHK(elapsed(i + 1, i + 2, &ms_stage[1]));
      CHK(elapsed(i + 2, i + 3, &ms_stage[2]));
    }
    int64_t sk_now = 0;
    for (int v : hskip) sk_now += v != 0;
    if (skipped_per_sweep) skipped_per_sweep[sweeps] = sk_now;
    skipped_total += sk_now;
    ++sweeps;
  }

  // finish: order, Newton-Schulz, Rayleigh quotients and residual norms against the caller's A
  HIPCHK(hipEventRecord(ctx->ev_pool[0], st));
  const double* hdiag = hoff.data() + npad;  // (of the converged matrix: the last k_jac_off read it)
  std::vector<int> order(npad);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return hdiag[a] < hdiag[b]; });
  HIPCHK(hipMemcpyAsync(perm, order.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
  double* X = Ap;  // (the work matrix is spent: its diagonal is on the host)
  hipLaunchKernelGGL(gspx::k_jac_gather, dim3((unsigned)(((size_t)n * n + 255) / 256)), dim3(256), 0, st, Vp,
                     (int64_t)npad, perm, n, X);
  hipLaunchKernelGGL(gspx::k_jac_padmass, dim3(1), dim3(256), 0, st, Vp, (int64_t)npad, perm, n, npad, padmass);
  double hpad = 0;
  HIPCHK(hipMemcpyAsync(&hpad, padmass, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // (V's work copy becomes the Gram's target below)
  double* G = Vp;  // n x n: (3 I - X^T X) / 2, in blocks as gspx_panel_gram_to_dev forms them
  for (int a0 = 0; a0 < n; a0 += SPEC_GRAM_BLOCK)
    for (int b0 = 0; b0 < n; b0 += SPEC_GRAM_BLOCK) {
      const int aw = std::min(SPEC_GRAM_BLOCK, n - a0), bw = std::min(SPEC_GRAM_BLOCK, n - b0);
      double* csum = nullptr;
      CHK(launch_panel_gram<double>(ctx, X + a0, (int64_t)n, aw, X + b0, (int64_t)n, bw, (int64_t)n, &csum));
      const int64_t count = (int64_t)aw * bw;
      hipLaunchKernelGGL(gspx::k_gram_store, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, csum, aw, bw, -0.5,
                         G + (size_t)a0 * n + b0, (int64_t)n);
    }
  hipLaunchKernelGGL(gspx::k_jac_add_diag, dim3((n + 255) / 256), dim3(256), 0, st, G, (int64_t)n, n, 1.5);
  const int64_t ntiles = (int64_t)((n + 63) / 64) * ((n + 63) / 64);
  const dim3 agrid((unsigned)std::min<int64_t>(ntiles, (int64_t)1 << 20));
  hipLaunchKernelGGL(gspx::k_spectral_apply<gspx::SPEC_PLAIN>, agrid, dim3(256), 0, st, (const double*)X, (int64_t)n, n,
                     (const double*)G, (int64_t)n, n, (const double*)nullptr, 1, V, ldv, (int64_t)n);
  double* W = X;  // A V, over the gathered columns (read by the launch before, in stream order)
  hipLaunchKernelGGL(gspx::k_spectral_apply<gspx::SPEC_PLAIN>, agrid, dim3(256), 0, st, A, lda, n, (const double*)V, ldv,
                     n, (const double*)nullptr, 1, W, (int64_t)n, (int64_t)n);
  const dim3 cgrid(nbk, (n + 63) / 64);
  hipLaunchKernelGGL(gspx::k_jac_coldot, cgrid, dim3(256), 0, st, (const double*)V, ldv, (const double*)W, (int64_t)n, n,
                     (const double*)nullptr, colpart);
  sum_parts(colpart, nbk, n, evals, st);
  hipLaunchKernelGGL(gspx::k_jac_coldot, cgrid, dim3(256), 0, st, (const double*)V, ldv, (const double*)W, (int64_t)n, n,
                     (const double*)evals, colpart);
  sum_parts(colpart, nbk, n, resid, st);
  std::vector<double> hres(n);
  HIPCHK(hipMemcpyAsync(e_host, evals, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hres.data(), resid, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(ctx->ev_pool[1], st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  CHK(elapsed(0, 1, &ms_stage[4]));
  // ascending: Rayleigh quotients of a cluster may come out of order by a rounding error; each is raised to its
  // predecessor (a change below the error of either)
  for (int i = 1; i < n; ++i) e_host[i] = std::max(e_host[i], e_host[i - 1]);
  if (info) {
    double worst = 0;
    for (double r2 : hres) worst = std::max(worst, r2);
    info[0] = sweeps;
    info[1] = norm > 0 ? off / norm : 0.0;
    info[2] = (double)((int64_t)npairs * sweeps - skipped_total);
    info[3] = (double)skipped_total;
    for (int i = 0; i < 5; ++i) info[4 + i] = ms_stage[i];
    info[9] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    info[10] = std::sqrt(worst);
    info[11] = hpad;
  }
  return GSPX_OK;
}

extern "C" int gspx_panel_scale_cols_dev(gspx_ctx* ctx, int64_t N, double* X, int64_t ldx, int w, const double* s_host) {
  if (N < 0) return set_err(GSPX_ERR_INVALID, "panel_scale_cols: negative number of rows");
  if (w < 0 || w > EIG_MAX_N)
    return set_err(GSPX_ERR_INVALID, "panel_scale_cols: width must be 0..%d (got %d)", EIG_MAX_N, w);
  if (ldx < w) return set_err(GSPX_ERR_INVALID, "panel_scale_cols: leading dimension below the width");
  const bool work = N > 0 && w > 0;
  if (work && (!X || !s_host)) return set_err(GSPX_ERR_INVALID, "panel_scale_cols: null panel or scale");
  if (!ctx) return set_err(GSPX_ERR_INVALID, "null context");
  replay_reset(ctx);
  if (!work) return GSPX_OK;
  HIPCHK(hipSetDevice(ctx->device));
  CHK(ctx->ws_spec.ensure((size_t)w * sizeof(double)));
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(ctx->ws_spec.p, s_host, (size_t)w * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(gspx::k_scale_cols, dim3((unsigned)((N * w + 255) / 256)), dim3(256), 0, st, X, ldx, w, N,
                     ctx->ws_spec.as<double>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  return GSPX_OK;
}
