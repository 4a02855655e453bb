// gspx_moments.hip.h - device code of the Chebyshev self-moments (gspx_cheby_moments_dev, pygsp_amd.spectrum): the
// inner products of neighbouring kept slots of a deferred batch.  The recurrence steps that fill the slots are the
// ones every filter runs (gspx_kernels.hip.h, gspx_tile_kernels.hip.h); the driver is in gspx_poly.hip.h.
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
