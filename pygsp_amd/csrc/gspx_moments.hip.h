// gspx_moments.hip.h - device code of the Chebyshev self-moments (gspx_cheby_moments_dev, pygsp_amd.spectrum): the
// inner products of neighbouring kept slots of a deferred batch - and of the cross-moments
// (gspx_cheby_cross_moments_dev, filters.cheby_op_vjp): the kept slots against foreign planes.  The recurrence steps
// that fill the slots are the ones every filter runs (gspx_kernels.hip.h, gspx_tile_kernels.hip.h); the drivers are in
// gspx_poly.hip.h.
#pragma once
#include "gspx_kernels.hip.h"

namespace gspx {

// ---------------------------------------------------------------------------------------------
// For the kept slots T_0 .. T_{nslots-1} (nslots >= 2) of a column batch (row pitch `pitch` >= w, slot pitch
// slot_stride):
//     a_i[j] = sum_rows T_i[row][j]^2                 (i < nslots)
//     b_i[j] = sum_rows T_{i+1}[row][j] T_i[row][j]   (i < nslots - 1)
// With T_i T_j = (T_{i+j} + T_{|i-j|}) / 2 and a symmetric L these are the moments x^T T_k x of 2 nslots - 1 orders.
// Every product and every sum is fp64, for fp32 slots too.  Rows in any order: a sum over rows does not care that the
// slots are in the internal vertex order.
// A lane owns VEC neighbouring columns at ONE position of a tile of 64 (64 >> cwl rows x 2^cwl column groups, as
// k_combine_sqnorm) and one chunk of CS slots (blockIdx.y: b_i for i in [CS y, CS y + CS), a_i likewise, and the a of
// the very last slot in the last chunk); per row it loads its elements of the chunk's slots and of the slot after
// them - CS + 1 independent loads, each 64 lanes wide over consecutive addresses - and its (2 CS + 1) VEC accumulators
// stay in registers over the whole row loop.  So a slot is read once, the first of every chunk but chunk 0 twice; no
// LDS staging.  VEC = 2 (fp32, w and pitch even) makes the loads 8 bytes per lane as fp64's are: 4-byte loads
// streamed at 1.5 TB/s against 5.5 (profiles/spectrum.md).  Pad columns (>= w) and rows >= N are never read.
// Rows of one column are then summed across the wave by a fixed butterfly, the four waves in wave order through LDS,
// and every workgroup writes its own partials part[blockIdx.x][2 nslots - 1][w] (a rows first, then b rows;
// k_dots_reduce sums them in a fixed order): no atomics, identical calls give identical bits.
// grid: (row groups, ceil((nslots - 1) / CS) chunks, blocks of 2^cwl column groups).
// ---------------------------------------------------------------------------------------------
template <int VEC, typename V> static __device__ __forceinline__ double dots_elem(const V& v, int j) {
  if constexpr (VEC == 1) return (double)v;
  else return (double)v[j];
}

template <typename T, int VEC, int CS>
__global__ __launch_bounds__(256) void k_slot_dots(const T* __restrict__ slots, int nslots, size_t slot_stride,
                                                   u32 pitch, int N, int w, int cwl, double* __restrict__ part) {
  typedef typename VT<T, VEC>::t V;
  __shared__ double red[2 * CS + 1][VEC][64];
  const int e = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int cw = 1 << cwl;
  const int rpt = 64 >> cwl;  // rows per tile
  const int col = (blockIdx.z * cw + (e & (cw - 1))) * VEC;
  const bool colok = col < w;  // (w is a multiple of VEC)
  const int i0 = blockIdx.y * CS;
  const int ns = min(CS + 1, nslots - i0);  // slots this chunk reads
  double a[CS + 1][VEC], b[CS][VEC];
#pragma unroll
  for (int s = 0; s <= CS; ++s)
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      a[s][j] = 0.0;
      if (s < CS) b[s][j] = 0.0;
    }
  const T* __restrict__ base = slots + (size_t)i0 * slot_stride + col;
  const int stride = (int)gridDim.x * 4 * rpt;
  for (int row = ((int)blockIdx.x * 4 + wave) * rpt + (e >> cwl); row < N; row += stride) {
    const T* __restrict__ p = base + (size_t)row * pitch;
    V v[CS + 1];
#pragma unroll
    for (int s = 0; s <= CS; ++s) v[s] = (s < ns && colok) ? *(const V*)(p + (size_t)s * slot_stride) : V(0);
#pragma unroll
    for (int s = 0; s <= CS; ++s)
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const double t = dots_elem<VEC>(v[s], j);
        a[s][j] = fma(t, t, a[s][j]);
        if (s < CS) b[s][j] = fma(dots_elem<VEC>(v[s + 1], j), t, b[s][j]);
      }
  }
  for (int off = cw; off < 64; off <<= 1) {
#pragma unroll
    for (int s = 0; s <= CS; ++s)
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        a[s][j] += __shfl_xor(a[s][j], off);
        if (s < CS) b[s][j] += __shfl_xor(b[s][j], off);
      }
  }
  // lanes e < 2^cwl hold their columns' sums over the wave's rows: waves 0..2 add theirs up in LDS, in wave order
  const bool owner = (e >> cwl) == 0;
  for (int q = 0; q < 3; ++q) {
    if (wave == q && owner) {
#pragma unroll
      for (int s = 0; s <= CS; ++s)
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          red[s][j][e] = q ? red[s][j][e] + a[s][j] : a[s][j];
          if (s < CS) red[CS + 1 + s][j][e] = q ? red[CS + 1 + s][j][e] + b[s][j] : b[s][j];
        }
    }
    __syncthreads();
  }
  if (wave == 3 && owner && colok) {
    double* __restrict__ pr = part + (size_t)blockIdx.x * (size_t)(2 * nslots - 1) * w + col;
#pragma unroll
    for (int s = 0; s <= CS; ++s) {
      const int i = i0 + s;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        if (s < CS ? i < nslots : i == nslots - 1) pr[(size_t)i * w + j] = red[s][j][e] + a[s][j];
        if (s < CS && i + 1 < nslots) pr[(size_t)(nslots + i) * w + j] = red[CS + 1 + s][j][e] + b[s][j];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Cross-moments (gspx_cheby_cross_moments_dev): the kept slots T_0 .. T_{nslots-1} of a column batch dotted against
// np <= P FOREIGN planes z_p (row pitch ldz, plane pitch zplane, the caller's vertex order):
//     c_{p,i}[j] = sum_rows z_p[rows(row)][j] T_i[row][j]      (p < np, i < nslots)
// The slots are in the internal vertex order and z is not, and a cross-moment does care: slot row `row` meets z row
// zrows[row] (zrows == null: the same row).  The row index is one 4-byte load per row and lane, 64 >> cwl distinct
// addresses per wave; the z rows themselves stay whole 2^cwl VEC-element pieces, so an internal order that keeps
// neighbours together keeps the z stream nearly sequential.
// Lane layout, row walk, fp64 products and sums, the wave butterfly, the LDS pass over the four waves in wave order
// and the per-workgroup partials are those of k_slot_dots above.  A lane owns VEC neighbouring columns, one chunk of
// CS slots (blockIdx.y) and the pass's planes; per row it loads its elements of the chunk's slots and of the np
// planes - CS + P independent loads - for CS P VEC fused multiply-adds, and the CS P VEC accumulators stay in
// registers over the row loop.  A slot is read once per pass, a plane once per chunk of slots.  Pad columns (>= w)
// and rows >= N are never read, of the slots or of z.
// part[blockIdx.x][p][i][w]: n = np nslots w doubles per workgroup row, summed by k_dots_reduce in a fixed order.
// grid: (row groups, ceil(nslots / CS) chunks, blocks of 2^cwl column groups).
// ---------------------------------------------------------------------------------------------
template <typename T, int VEC, int CS, int P>
__global__ __launch_bounds__(256) void k_slot_cross_dots(const T* __restrict__ slots, int nslots, size_t slot_stride,
                                                         u32 pitch, const T* __restrict__ z, int np, size_t zplane,
                                                         u32 ldz, const int* __restrict__ zrows, int N, int w, int cwl,
                                                         double* __restrict__ part) {
  typedef typename VT<T, VEC>::t V;
  __shared__ double red[CS * P][VEC][64];
  const int e = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int cw = 1 << cwl;
  const int rpt = 64 >> cwl;  // rows per tile
  const int col = (blockIdx.z * cw + (e & (cw - 1))) * VEC;
  const bool colok = col < w;  // (w is a multiple of VEC)
  const int i0 = blockIdx.y * CS;
  const int ns = min(CS, nslots - i0);  // slots this chunk reads
  double acc[CS][P][VEC];
#pragma unroll
  for (int s = 0; s < CS; ++s)
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[s][p][j] = 0.0;
  const T* __restrict__ base = slots + (size_t)i0 * slot_stride + col;
  const int stride = (int)gridDim.x * 4 * rpt;
  for (int row = ((int)blockIdx.x * 4 + wave) * rpt + (e >> cwl); row < N; row += stride) {
    const T* __restrict__ ps = base + (size_t)row * pitch;
    const size_t zr = zrows ? (size_t)zrows[row] : (size_t)row;
    const T* __restrict__ pz = z + zr * ldz + col;
    V v[CS], u[P];
#pragma unroll
    for (int s = 0; s < CS; ++s) v[s] = (s < ns && colok) ? *(const V*)(ps + (size_t)s * slot_stride) : V(0);
#pragma unroll
    for (int p = 0; p < P; ++p) u[p] = (p < np && colok) ? *(const V*)(pz + (size_t)p * zplane) : V(0);
#pragma unroll
    for (int s = 0; s < CS; ++s)
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          acc[s][p][j] = fma(dots_elem<VEC>(u[p], j), dots_elem<VEC>(v[s], j), acc[s][p][j]);
  }
  for (int off = cw; off < 64; off <<= 1) {
#pragma unroll
    for (int s = 0; s < CS; ++s)
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[s][p][j] += __shfl_xor(acc[s][p][j], off);
  }
  // lanes e < 2^cwl hold their columns' sums over the wave's rows: waves 0..2 add theirs up in LDS, in wave order
  const bool owner = (e >> cwl) == 0;
  for (int q = 0; q < 3; ++q) {
    if (wave == q && owner) {
#pragma unroll
      for (int s = 0; s < CS; ++s)
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
          for (int j = 0; j < VEC; ++j)
            red[s * P + p][j][e] = q ? red[s * P + p][j][e] + acc[s][p][j] : acc[s][p][j];
    }
    __syncthreads();
  }
  if (wave == 3 && owner && colok) {
    double* __restrict__ pr = part + (size_t)blockIdx.x * (size_t)np * (size_t)nslots * w + col;
#pragma unroll
    for (int s = 0; s < CS; ++s)
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          if (s < ns && p < np) pr[((size_t)p * nslots + (i0 + s)) * w + j] = red[s * P + p][j][e] + acc[s][p][j];
  }
}

// out[f][col] = the sum over the nparts workgroup partials part[b][i], i = f w + col < n, of k_slot_dots; out row
// pitch ldo.  Wave q of a workgroup takes the partials b with (b / 4) % 4 == q in four running sums (sixteen
// independent chains per output, so that the latency of a partial is paid nparts / 16 times); the sums meet in a
// fixed order.
__global__ __launch_bounds__(256) void k_dots_reduce(const double* __restrict__ part, int nparts, int64_t n, int w,
                                                     double* __restrict__ out, size_t ldo) {
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 64 + lane;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (i < n)
    for (int b = 4 * q; b < nparts; b += 16) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (b + u < nparts) s[u] += part[(size_t)(b + u) * (size_t)n + (size_t)i];
    }
  red[q][lane] = (s[0] + s[1]) + (s[2] + s[3]);
  __syncthreads();
  if (q == 0 && i < n) {
    const int64_t f = i / w;
    out[(size_t)f * ldo + (size_t)(i - f * w)] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
  }
}

}  // namespace gspx
