// gspx_conv.hip.h - the Chebyshev graph convolution (ChebNet layer; gspx_cheby_conv_dev, gspx_cheby_cross_grams_dev,
// pygsp_amd.nn.ChebConv):
//     Y[n, b, :] = sum_{k < M} (T_k(Lt) X)[n, b, :] Theta_k,    Theta_k in R^{Fin x Fout}, plain sum (Theta_0 not halved).
// T_k(Lt) acts on the vertex index and Theta_k on the feature index, so Y = sum_k T_k(Lt) U_k with U_k = X Theta_k: the
// vector-coefficient Clenshaw recurrence of the synthesis call (clenshaw_step, gspx_poly.hip.h) with one input panel
// per order, made by the dense kernel k_group_mix.  L is symmetric, so the gradient with respect to X is the same
// operator with every Theta_k transposed; the gradient with respect to Theta_k is the cross-Gram
//     G_k[i][o] = sum_{n, b} (T_k(Lt) X)[n, b, i] cot[n, b, o]
// of the kept slots of a deferred batch with the cotangent (k_slot_cross_gram).  No step kernel is touched.  gfx950
// only.
// After gspx_poly.hip.h (run_batch, clenshaw_step, run_batches) and gspx_ops.hip.h (sum_parts of gspx_reduce.hip.h).
#pragma once

namespace gspx {

typedef double conv_d4 __attribute__((ext_vector_type(4)));
typedef float conv_f4 __attribute__((ext_vector_type(4)));
template <typename T> struct ConvAcc;
template <> struct ConvAcc<double> { typedef conv_d4 t; };
template <> struct ConvAcc<float> { typedef conv_f4 t; };
__device__ __forceinline__ conv_d4 conv_mfma(double a, double b, conv_d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ conv_f4 conv_mfma(float a, float b, conv_f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// row of a 16 x 16 result tile that element e of a lane's accumulator holds: the f64 instruction interleaves the four
// lane groups, the f32 one gives each group four neighbouring rows (the column is lane % 16 for both)
template <typename T> __device__ __forceinline__ int conv_drow(int lane, int e) {
  return sizeof(T) == 8 ? (lane >> 4) + 4 * e : (lane >> 4) * 4 + e;
}

// ---------------------------------------------------------------------------------------------
// out[n, b, :] = in[n, b, :] Theta      (Theta: Fin x Fout, row-major, the panel's dtype, on the device)
// in: N rows of pitch ld_in holding B groups of Fin elements; out: N rows of pitch ld_out holding B groups of Fout
// elements and, where ld_out > B Fout, ZEROS in the pad columns (the step kernels read whole padded rows).  Both in the
// internal vertex order: the kernel is row-local.  Pad columns of `in` and rows >= N are never read.
// The logical rows are the (n, b) pairs, r = n B + b.  A wave takes 16 of them at a time and all of Fout: the matrix
// cores' 16 x 16 x 4 product with A = the rows' elements (lane l: row l % 16, the element its lane group q = l / 16
// contributes to step s) and B = Theta (lane l: that element's row of Theta, column l % 16 of the wave's tile j), NT
// accumulator tiles per wave.  A product sums over its four elements in any order, so WHICH element group q brings
// to step s is free as long as Theta's rows follow: element (4 (s / V) + q) V + s % V.  A lane's elements of V
// consecutive steps are then V neighbours in memory - one 16-byte load (V = 2 fp64, 4 fp32) where Fin, the pitch and
// the base allow it, and the four groups of a row read 64 consecutive bytes; V = 1 (any Fin) is the natural order,
// element 4 s + q.  A lane loads its up to QM elements before the first product, so that many loads are in flight.
// Theta is staged once per workgroup in LDS in the order the steps read it (row 4 s + q of the image = Theta's row of
// step s, group q), zero-padded to 4 Q rows, Q = V ceil(Fin / 4 V), of pitch P >= 16 ceil(Fout / 16); the launcher
// picks P = 16 mod 32 elements, so that the two lane groups of a 32-lane half, which read neighbouring rows of the
// image, land on different banks.  Edge tiles are products with zeros: one path for every Fin, Fout <= 128.
// Arithmetic in the panel's dtype (the f32 instruction is an fp32 fma chain over k).
// grid: (workgroups); waves walk the 16-row tiles with stride 4 gridDim.x.  Dynamic LDS: 4 Q P sizeof(T).
// ---------------------------------------------------------------------------------------------
// Two waves per SIMD at least (another wave's loads and stores under this one's products), except for the three shapes
// the compiler does not fit into half the register file without scratch: those keep the whole file, and no build
// uses scratch.
template <typename T, int NT, int QM> constexpr int mix_min_waves() {
  return (sizeof(T) == 4 && NT == 8) || (sizeof(T) == 8 && NT == 4 && QM == 32) ? 1 : 2;
}
template <typename T, int NT, int QM, int V>
__global__ __launch_bounds__(256, (mix_min_waves<T, NT, QM>())) void k_group_mix(const T* __restrict__ in, size_t ld_in,
                                                      const T* __restrict__ theta, int Fin, int Fout, int B, int N,
                                                      T* __restrict__ out, size_t ld_out, int P) {
  typedef typename ConvAcc<T>::t acc_t;
  typedef typename VT<T, V>::t vec_t;
  static_assert(QM % V == 0, "whole vectors");
  extern __shared__ __attribute__((aligned(16))) unsigned char conv_lds[];
  T* th = (T*)conv_lds;
  const int Q = V * ((Fin + 4 * V - 1) / (4 * V));  // products along Fin
  const int nt = (Fout + 15) >> 4;                  // 16-wide tiles of Fout in use (<= NT)
  for (int idx = threadIdx.x; idx < 4 * Q * P; idx += 256) {
    const int row = idx / P, o = idx - row * P;
    const int s = row >> 2, q = row & 3;
    const int i = (4 * (s / V) + q) * V + s % V;
    th[idx] = (i < Fin && o < Fout) ? theta[(size_t)i * Fout + o] : T(0);
  }
  const int w = B * Fout, pad = (int)ld_out - w;
  if (pad > 0) {
    const size_t total = (size_t)N * pad;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
      const size_t n = idx / pad;
      out[n * ld_out + w + (idx - n * pad)] = T(0);
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, c = lane & 15;
  const int64_t R = (int64_t)N * B;
  for (int64_t t0 = ((int64_t)blockIdx.x * 4 + wave) * 16; t0 < R; t0 += (int64_t)gridDim.x * 64) {
    const int64_t r = t0 + c;
    const bool rok = r < R;
    const int64_t n = rok ? r / B : 0;
    const int b = rok ? (int)(r - n * B) : 0;
    const T* __restrict__ pin = in + (size_t)n * ld_in + (size_t)b * Fin + q * V;
    T a[QM];
#pragma unroll
    for (int g = 0; g < QM / V; ++g) {  // (V > 1: Fin is a multiple of V, so a vector is inside the row or outside)
      const bool ok = rok && (4 * g + q) * V < Fin;
      if constexpr (V == 1) {
        a[g] = ok ? pin[4 * g] : T(0);
      } else {
        const vec_t v = ok ? *(const vec_t*)(pin + 4 * g * V) : vec_t(0);
#pragma unroll
        for (int k = 0; k < V; ++k) a[g * V + k] = v[k];
      }
    }
    acc_t acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = 0;
#pragma unroll
    for (int s = 0; s < QM; ++s) {
      if (s < Q) {
        const T* pb = th + (4 * s + q) * P + c;
#pragma unroll
        for (int j = 0; j < NT; ++j)
          if (j < nt) acc[j] = conv_mfma(a[s], pb[16 * j], acc[j]);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t rr = t0 + conv_drow<T>(lane, e);
      if (rr < R) {
        const int64_t n2 = rr / B;
        T* __restrict__ po = out + (size_t)n2 * ld_out + (size_t)(rr - n2 * B) * Fout + c;
#pragma unroll
        for (int j = 0; j < NT; ++j)
          if (j < nt && 16 * j + c < Fout) po[16 * j] = acc[j][e];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The cross-Grams of the kept slots T_0 .. T_{nslots-1} of a column batch with the cotangent z:
//     part[chunk][k][i][o] = sum over the chunk's logical rows (row, b) of T_k[row, b, i] z[zrows[row], b, o].
// The slots are in the internal vertex order at pitch `pitch` (groups of Fin at b Fin); z is in the CALLER's order at
// pitch ldz (groups of Fout at b Fout): slot row `row` meets z row zrows[row] (null: the same row).
// The product is k_panel_gram's (gspx_reduce.hip.h): v_mfma_f64_16x16x4f64 with A-operand = the slot (lane l: column
// l % 16 of the tile, logical row l / 16 of the group of four) and B-operand = z under the same lane map, wave w taking
// the 4-row groups w, w + 4, ... of the chunk; every product and sum is fp64, fp32 panels are converted at the product.  A
// workgroup owns a tile of 16 TA x 16 TC entries (blockIdx.x), a chunk of `rpc` logical rows (blockIdx.y, rpc a
// multiple of 16) and CS = 16 / (TA TC) slots (blockIdx.z): z is read once per chunk of slots, a slot once per tile
// column - once, where Fout <= 64.  The CS TA loads of the slots and the TC loads of z of the NEXT group are issued
// before this group's products.  The four waves' sums meet in LDS in the fixed order ((w0 + w1) + w2) + w3; every
// entry of every chunk's slab is written (zeros for a chunk without rows), so the second pass (sum_parts) needs no
// initialisation and there are no atomics: identical calls give identical bits.
// ---------------------------------------------------------------------------------------------
template <typename T, int TA, int TC>
__global__ __launch_bounds__(256) void k_slot_cross_gram(const T* __restrict__ slots, int nslots, size_t slot_stride,
                                                         size_t pitch, const T* __restrict__ z, size_t ldz,
                                                         const int* __restrict__ zrows, int N, int B, int Fin, int Fout,
                                                         int64_t rpc, double* __restrict__ part) {
  constexpr int CS = 16 / (TA * TC);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int kq = lane >> 4, cq = lane & 15;
  const int ntb = (Fout + 16 * TC - 1) / (16 * TC);
  const int a0 = (int)(blockIdx.x / ntb) * 16 * TA, b0 = (int)(blockIdx.x % ntb) * 16 * TC;
  const int i0 = blockIdx.z * CS;
  const int ns = min(CS, nslots - i0);
  const int64_t R = (int64_t)N * B;
  const int64_t r_begin = (int64_t)blockIdx.y * rpc;
  const int64_t r_end = min(R, r_begin + rpc);
  conv_d4 acc[CS][TA][TC];
#pragma unroll
  for (int s = 0; s < CS; ++s)
#pragma unroll
    for (int i = 0; i < TA; ++i)
#pragma unroll
      for (int j = 0; j < TC; ++j) acc[s][i][j] = 0;
  const T* __restrict__ sbase = slots + (size_t)i0 * slot_stride;
  // the operands of the 4-row group at r (zeros, and no access, for rows beyond the chunk)
  auto load = [&](int64_t r, T (&xa)[CS][TA], T (&yb)[TC]) {
    const int64_t rr = r + kq;
    const bool rok = rr < r_end;
    const int64_t n = rok ? rr / B : 0;
    const int b = rok ? (int)(rr - n * B) : 0;
    const size_t zr = (rok && zrows) ? (size_t)zrows[n] : (size_t)n;
    const T* __restrict__ pz = z + zr * ldz + (size_t)b * Fout;
    const T* __restrict__ ps = sbase + (size_t)n * pitch + (size_t)b * Fin;
#pragma unroll
    for (int s = 0; s < CS; ++s)
#pragma unroll
      for (int t = 0; t < TA; ++t) {
        const int ca = a0 + t * 16 + cq;
        xa[s][t] = (rok && s < ns && ca < Fin) ? ps[(size_t)s * slot_stride + ca] : T(0);
      }
#pragma unroll
    for (int t = 0; t < TC; ++t) {
      const int cb = b0 + t * 16 + cq;
      yb[t] = (rok && cb < Fout) ? pz[cb] : T(0);
    }
  };
  // (converted where they are used, so that a load is awaited at its products and not when it is issued; a chunk's
  // missing slots cost no products)
  auto products = [&](const T (&xa)[CS][TA], const T (&yb)[TC]) {
#pragma unroll
    for (int s = 0; s < CS; ++s)
      if (s < ns)
#pragma unroll
        for (int i = 0; i < TA; ++i)
#pragma unroll
          for (int j = 0; j < TC; ++j)
            acc[s][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)xa[s][i], (double)yb[j], acc[s][i][j], 0, 0, 0);
  };
  // two register sets: the loads of the next group are in flight while this one's products run (a wave alone on its
  // SIMD - the accumulators fill the register file - would otherwise wait out every load)
  T xa0[CS][TA], yb0[TC], xa1[CS][TA], yb1[TC];
  int64_t r = r_begin + 4 * w;
  load(r, xa0, yb0);
  for (; r < r_end; r += 32) {
    load(r + 16, xa1, yb1);
    products(xa0, yb0);
    load(r + 32, xa0, yb0);
    products(xa1, yb1);
  }
  __shared__ double red[16 * 4 * 64];  // one wave's CS x TA x TC tiles, lane-major (no bank conflicts)
  for (int src = 1; src < 4; ++src) {
    if (w == src)
#pragma unroll
      for (int s = 0; s < CS; ++s)
#pragma unroll
        for (int i = 0; i < TA; ++i)
#pragma unroll
          for (int j = 0; j < TC; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[(((s * TA + i) * TC + j) * 4 + e) * 64 + lane] = acc[s][i][j][e];
    __syncthreads();
    if (w == 0)
#pragma unroll
      for (int s = 0; s < CS; ++s)
#pragma unroll
        for (int i = 0; i < TA; ++i)
#pragma unroll
          for (int j = 0; j < TC; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[s][i][j][e] += red[(((s * TA + i) * TC + j) * 4 + e) * 64 + lane];
    __syncthreads();
  }
  if (w != 0) return;
  const size_t FF = (size_t)Fin * Fout;
  double* __restrict__ po = part + (size_t)blockIdx.y * (size_t)nslots * FF + (size_t)i0 * FF;
#pragma unroll
  for (int s = 0; s < CS; ++s)
#pragma unroll
    for (int i = 0; i < TA; ++i)
#pragma unroll
      for (int j = 0; j < TC; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int aa = a0 + i * 16 + kq + 4 * e, cc = b0 + j * 16 + cq;
          if (s < ns && aa < Fin && cc < Fout) po[(size_t)s * FF + (size_t)aa * Fout + cc] = acc[s][i][j][e];
        }
}

}  // namespace gspx

// ---- host side --------------------------------------------------------------------------------------------------
static const int CONV_FMAX = 128;  // widest feature dimension: Theta_k fits the LDS of one workgroup

// LDS pitch of k_group_mix's image of Theta: whole 16-wide tiles, and 16 mod 32 elements (see the kernel)
static int mix_pitch(int Fout) {
  const int p = (Fout + 15) / 16 * 16;
  return p % 32 == 0 ? p + 16 : p;
}

template <typename T>
static int launch_group_mix(gspx_ctx* ctx, const T* in, size_t ld_in, const T* theta, int Fin, int Fout, int B, int N,
                            T* out, size_t ld_out, hipStream_t st) {
  typedef void (*kern_t)(const T*, size_t, const T*, int, int, int, int, T*, size_t, int);
  // builds: 1, 2, 4 or 8 tiles of Fout; 16-byte loads (V elements) and room for 8, 16 or 32 products along Fin where
  // rows split into such pieces, single elements and room for 8 or 32 otherwise
  constexpr int VM = 16 / (int)sizeof(T);
#define GSPX_MIX(QM_, V_) \
  {k_group_mix<T, 1, QM_, V_>, k_group_mix<T, 2, QM_, V_>, k_group_mix<T, 4, QM_, V_>, k_group_mix<T, 8, QM_, V_>}
  static const kern_t wide[3][4] = {GSPX_MIX(8, VM), GSPX_MIX(16, VM), GSPX_MIX(32, VM)};
  static const kern_t single[3][4] = {GSPX_MIX(8, 1), GSPX_MIX(32, 1), GSPX_MIX(32, 1)};
#undef GSPX_MIX
  const bool vec = Fin % VM == 0 && ld_in % VM == 0 && ((uintptr_t)in % 16) == 0;
  const int V = vec ? VM : 1;
  const int nt = (Fout + 15) / 16, Q = V * ((Fin + 4 * V - 1) / (4 * V));
  const kern_t kern = (vec ? wide : single)[Q <= 8 ? 0 : Q <= 16 ? 1 : 2][nt <= 1 ? 0 : nt <= 2 ? 1 : nt <= 4 ? 2 : 3];
  const int P = mix_pitch(Fout);
  const size_t lds = (size_t)4 * Q * P * sizeof(T);
  if (lds > ((size_t)64 << 10))
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // workgroups: what the LDS image lets a CU hold (at most eight), no more than there are tiles of four waves
  const int64_t tiles = ((int64_t)N * B + 63) / 64;
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(8, ((int64_t)160 << 10) / (int64_t)std::max<size_t>(lds, 1)));
  const int64_t nwg = std::max<int64_t>(1, std::min<int64_t>(tiles, per_cu * ctx->cu_count));
  hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(256), lds, st, in, ld_in, theta, Fin, Fout, B, N, out, ld_out, P);
  return GSPX_OK;
}

// The tile builds of k_slot_cross_gram: TA, TC = the 16-wide tiles of Fin and Fout a workgroup takes (1, 2 or 4: the
// smallest power of two that covers the dimension, at most 64 entries), CS = 16 / (TA TC) slots per chunk - sixteen
// accumulator tiles per wave whatever the shape, as cross_cs keeps the accumulators of k_slot_cross_dots constant.
static int gram_tiles(int F) { return F <= 16 ? 1 : F <= 32 ? 2 : 4; }
static int gram_cs(int Fin, int Fout) { return 16 / (gram_tiles(Fin) * gram_tiles(Fout)); }
static int gram_blocks(int Fin, int Fout, int M) {  // grid.x * grid.z
  const int ta = 16 * gram_tiles(Fin), tc = 16 * gram_tiles(Fout), cs = gram_cs(Fin, Fout);
  return ((Fin + ta - 1) / ta) * ((Fout + tc - 1) / tc) * ((M + cs - 1) / cs);
}
// row chunks of a call: about eight workgroups per CU in all, at least 64 logical rows per chunk, at most 64 MiB of
// partials.  One figure for every batch of a call (from its widest): the running total sits behind the partials.
static int gram_chunks(const gspx_ctx* ctx, int64_t R, int Fin, int Fout, int M) {
  const int64_t blocks = gram_blocks(Fin, Fout, M);
  int64_t n = std::max<int64_t>(1, ((int64_t)8 * ctx->cu_count + blocks - 1) / blocks);
  n = std::min<int64_t>(n, (R + 63) / 64);
  n = std::min<int64_t>(n, std::max<int64_t>(1, ((int64_t)64 << 20) / ((int64_t)M * Fin * Fout * (int64_t)sizeof(double))));
  return (int)std::max<int64_t>(1, std::min<int64_t>(n, 65535));
}

// The cross-Grams of one batch added to the call's running total.  ws: [total 0][nchunk partial slabs][total 1], slabs
// of M Fin Fout doubles; batch `index` sums (total 0, partials) into total 1 when even and (partials, total 1) into
// total 0 when odd - one fixed-order pass (sum_parts), the batches in order.
struct CrossGram {
  const void* z;  // the cotangent at the batch's first column, the caller's vertex order
  size_t ldz;
  int s, Fin, Fout;  // samples in the batch
  int nchunk, index;
  double* ws;
};

template <typename T>
static int cross_gram_use(gspx_ctx* ctx, const void* slots, int M, size_t slot_stride, unsigned pitch, int N, unsigned,
                          const int* perm, const void* arg, hipStream_t st) {
  const CrossGram& cg = *(const CrossGram*)arg;
  typedef void (*kern_t)(const T*, int, size_t, size_t, const T*, size_t, const int*, int, int, int, int, int64_t, double*);
  static const kern_t kerns[3][3] = {
      {k_slot_cross_gram<T, 1, 1>, k_slot_cross_gram<T, 1, 2>, k_slot_cross_gram<T, 1, 4>},
      {k_slot_cross_gram<T, 2, 1>, k_slot_cross_gram<T, 2, 2>, k_slot_cross_gram<T, 2, 4>},
      {k_slot_cross_gram<T, 4, 1>, k_slot_cross_gram<T, 4, 2>, k_slot_cross_gram<T, 4, 4>}};
  const int ta = gram_tiles(cg.Fin), tc = gram_tiles(cg.Fout), cs = gram_cs(cg.Fin, cg.Fout);
  const kern_t kern = kerns[ta == 1 ? 0 : ta == 2 ? 1 : 2][tc == 1 ? 0 : tc == 2 ? 1 : 2];
  const size_t count = (size_t)M * cg.Fin * cg.Fout;
  const int64_t R = (int64_t)N * cg.s;
  const int64_t rpc = ((R + cg.nchunk - 1) / cg.nchunk + 15) / 16 * 16;
  double* part = cg.ws + count;
  const dim3 grid((unsigned)(((cg.Fin + 16 * ta - 1) / (16 * ta)) * ((cg.Fout + 16 * tc - 1) / (16 * tc))),
                  (unsigned)cg.nchunk, (unsigned)((M + cs - 1) / cs));
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, (const T*)slots, M, slot_stride, (size_t)pitch, (const T*)cg.z, cg.ldz,
                     perm, N, cg.s, cg.Fin, cg.Fout, rpc, part);
  double* total1 = part + (size_t)cg.nchunk * count;
  if (cg.index % 2 == 0)
    sum_parts(cg.ws, cg.nchunk + 1, (int64_t)count, total1, st);
  else
    sum_parts(part, cg.nchunk + 1, (int64_t)count, cg.ws, st);
  return GSPX_OK;
}

// One batch of `s` whole samples of the convolution: x [N][ldx] at the batch's first input column (s Fin columns), y
// [N][ldy] at its first output column (s Fout columns); theta [M][Fin][Fout] and `one` (a 1.0) on the device.  X goes
// into the internal order once; per order k = K .. 0 k_group_mix makes U_k = X Theta_k in one work panel and the
// Clenshaw step of the synthesis call takes it as its single input panel with weight one.  Routing (tile_direct /
// padded / plain), scale, gamma, final, reverse and the copy out are run_synthesis_batch's: the same clenshaw_step.
template <typename T>
static int run_conv_batch(gspx_graph* g, int M, int Fin, int Fout, const T* theta, const T* one, const T* x, unsigned ldx,
                          T* y, unsigned ldy, unsigned s, size_t& ev_idx) {
  gspx_ctx* ctx = g->ctx;
  Options opt = ctx->opt;
  hipStream_t st = ctx->stream;
  const int N = (int)g->N;
  const int K = M - 1;
  const unsigned ld = s * (unsigned)Fout, ldi = s * (unsigned)Fin;
  const WorkPanels wp = work_panels<T>(g, opt, true, 1, ld, y, ldy);
  const unsigned ldw = wp.ldw;
  const size_t U = (size_t)N * ldw;
  const size_t XU = ((size_t)N * ldi + 63) & ~(size_t)63;  // (the U panel starts on a 256-byte boundary)
  const Shape shape = choose_shape(opt, sizeof(T), ld, vec_cap(4, ldy, y));
  const int* perm = g->has_perm ? g->perm.as<int>() : nullptr;

  CHK(ctx->ws_r.ensure((XU + U) * sizeof(T) + 256));  // X in the internal order | U_k
  CHK(ctx->ws_t.ensure(2 * U * sizeof(T) + 256));
  T* X = ctx->ws_r.as<T>();
  T* Uk = X + XU;
  T* B[2] = {ctx->ws_t.as<T>(), ctx->ws_t.as<T>() + U};

  hipEvent_t ev[4];
  CHK(batch_events(ctx, ev_idx, ev));
  launch_permute_in<T>(x, ldx, X, ldi, N, perm, vec_cap(vec_cap((int)(16 / sizeof(T)), ldi, X), ldx, x), st);
  HIPCHK(hipEventRecord(ev[1], st));

  CHK(prepare_coff<T>(g, shape, ld, st));
  StepArgs<T> a = step_base<T>(g, ld, y, ldy);
  for (int k = K; k >= 0; --k) {
    CHK(launch_group_mix<T>(ctx, X, ldi, theta + (size_t)k * Fin * Fout, Fin, Fout, (int)s, N, Uk, ldw, st));
    CHK(clenshaw_step<T>(g, opt, wp, shape, a, k, K, Uk, one, 1, Uk, B, y, ldy, st));
  }
  HIPCHK(hipEventRecord(ev[2], st));
  if (wp.padded) {
    const unsigned nbp = (unsigned)std::min<size_t>(((size_t)N * ld + 255) / 256, 65536);
    hipLaunchKernelGGL((k_permute_out_pad<T>), dim3(nbp), dim3(256), 0, st, B[0], ldw, y, ldy, ld, N, perm);
  }
  HIPCHK(hipEventRecord(ev[3], st));
  HIPCHK(hipGetLastError());
  return GSPX_OK;
}

// Samples per column batch: batches hold WHOLE samples, s Fin input and s Fout output columns.  From batch_width with
// the wider of the two panels and the `panels` panels of that width the call keeps; one sample where max_batch or the
// workspace budget allow less - unless one sample alone leaves the 2 GiB window of a panel.
static int conv_samples(const gspx_graph* g, size_t elt, size_t panels, int Fin, int Fout, int64_t B, int64_t* s) {
  const int64_t F = std::max(Fin, Fout);
  if ((size_t)g->N * (size_t)F * elt > ((size_t)1 << 31) - 65536)
    return set_err(GSPX_ERR_INVALID, "graph too large: one sample of %d features exceeds 2 GiB", (int)F);
  int64_t width = 0;
  CHK(batch_width(g, elt, panels, B * F, &width));
  *s = std::max<int64_t>(1, std::min<int64_t>(B, width / F));
  return GSPX_OK;
}

template <typename T>
static int conv_dev_t(gspx_graph* g, double lmax, int M, int Fin, int Fout, const double* theta, int64_t B, const T* x,
                      T* y) {
  gspx_ctx* ctx = g->ctx;
  for (int i = 0; i < 5; ++i) ctx->timing[i] = 0;
  ctx->step_kinds[0] = ctx->step_kinds[1] = 0;
  if (g->N == 0 || B == 0) return GSPX_OK;
  CHK(ensure_factor<T>(g, lmax));
  int64_t s = 0;
  CHK(conv_samples(g, sizeof(T), 4, Fin, Fout, B, &s));  // X, U_k and the two recurrence panels
  // the device copy of Theta in the panel's dtype, behind a 1.0 (the weight of the step's single input panel)
  const size_t nth = (size_t)M * Fin * Fout, off = 256 / sizeof(T);
  std::vector<T> hw(off + nth, T(0));
  hw[0] = T(1);
  for (size_t i = 0; i < nth; ++i) hw[off + i] = (T)theta[i];
  CHK(ctx->ws_w.ensure(hw.size() * sizeof(T) + 64));
  HIPCHK(hipMemcpyAsync(ctx->ws_w.p, hw.data(), hw.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));  // hw is a stack-owned staging buffer
  const T* one = ctx->ws_w.as<T>();
  const unsigned ldx = (unsigned)(B * Fin), ldy = (unsigned)(B * Fout);
  return run_batches(g, B, s, M - 1, [&](int64_t c0, unsigned here, size_t& ev_idx) -> int {
    return run_conv_batch<T>(g, M, Fin, Fout, one + off, one, x + c0 * Fin, ldx, y + c0 * Fout, ldy, here, ev_idx);
  });
}

// out (HOST, M x Fin x Fout): per batch the deferred plan of one filter with M kept slots on the batch's s Fin columns
// (M - 1 plain recurrence steps), then k_slot_cross_gram in place of the combine; the batches' Grams are summed on the
// device in batch order.
template <typename T>
static int cross_grams_dev_t(gspx_graph* g, double lmax, int M, int Fin, int Fout, int64_t B, const T* x, const T* z,
                             double* out) {
  gspx_ctx* ctx = g->ctx;
  const int64_t N = g->N;
  for (int i = 0; i < 5; ++i) ctx->timing[i] = 0;
  ctx->step_kinds[0] = ctx->step_kinds[1] = 0;
  if (B == 0) return GSPX_OK;
  const size_t count = (size_t)M * Fin * Fout;
  if (N == 0) {
    std::fill(out, out + count, 0.0);
    return GSPX_OK;
  }
  int64_t s = 0;
  CHK(conv_samples(g, sizeof(T), (size_t)M, Fin, Fout, B, &s));  // the M kept slots
  const std::vector<double> cp((size_t)M, 0.0);  // (the deferred plan uploads its filter's coefficients; none are read)
  const int nchunk = gram_chunks(ctx, N * s, Fin, Fout, M);
  CHK(ctx->ws_sqp.ensure(((size_t)nchunk + 2) * count * sizeof(double) + 256));
  double* ws = ctx->ws_sqp.as<double>();
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemsetAsync(ws, 0, count * sizeof(double), st));
  CHK(ensure_factor<T>(g, lmax));
  const unsigned ldx = (unsigned)(B * Fin);
  int index = 0;
  CHK(run_batches(g, B, s, M - 1, [&](int64_t c0, unsigned here, size_t& ev_idx) -> int {
    const CrossGram cg{z + c0 * Fout, (size_t)(B * Fout), (int)here, Fin, Fout, nchunk, index++, ws};
    const SlotsUse use{cross_gram_use<T>, &cg};
    const unsigned ld = here * (unsigned)Fin;
    return run_batch<T>(g, 1, M, cp, x + c0 * Fin, ldx, (T*)nullptr, ld, ld, true, false, false, ev_idx, nullptr, nullptr,
                        nullptr, &use);
  }));
  const double* total = index % 2 ? ws + ((size_t)nchunk + 1) * count : ws;
  HIPCHK(hipMemcpyAsync(out, total, count * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return GSPX_OK;
}

// the scalar checks of both entry points: they need no graph, and so no device, to be exercised
static int check_conv_args(const char* who, double lmax, int M, int Fin, int Fout, int64_t B) {
  if (M < 2) return set_err(GSPX_ERR_COEFF, "The coefficients have an invalid shape");
  if (M > 256) return set_err(GSPX_ERR_INVALID, "%s: 2 to 256 orders (got %d)", who, M);
  if (Fin < 1 || Fin > CONV_FMAX || Fout < 1 || Fout > CONV_FMAX)
    return set_err(GSPX_ERR_INVALID, "%s: 1 to %d features in and out (got %d and %d)", who, CONV_FMAX, Fin, Fout);
  if (B < 0) return set_err(GSPX_ERR_INVALID, "negative number of samples");
  if (!(lmax > 0.0) || !std::isfinite(lmax))
    return set_err(GSPX_ERR_INVALID, "lmax must be positive and finite (got %g)", lmax);
  return GSPX_OK;
}

extern "C" int gspx_cheby_conv_dev(gspx_graph* g, double lmax, int M, int Fin, int Fout, const double* theta, int64_t B,
                                   const void* x_dev, void* y_dev, double* kernel_ms) {
  CHK(check_conv_args("gspx_cheby_conv_dev", lmax, M, Fin, Fout, B));
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (!theta) return set_err(GSPX_ERR_INVALID, "null coefficients");
  if (B > 0 && g->N > 0 && (!x_dev || !y_dev)) return set_err(GSPX_ERR_INVALID, "null signal pointer");
  if (B > 0 && g->N > 0 && x_dev == (const void*)y_dev)
    return set_err(GSPX_ERR_INVALID, "gspx_cheby_conv_dev: x and y must not be the same buffer");
  if (B >= ((int64_t)1 << 31) / 16 / std::max(Fin, Fout)) return set_err(GSPX_ERR_INVALID, "too many signals");
  for (size_t i = 0; i < (size_t)M * Fin * Fout; ++i)
    if (!std::isfinite(theta[i])) return set_err(GSPX_ERR_INVALID, "non-finite coefficient");
  replay_reset(g->ctx);  // (the work panels overwrite what a recorded filter call replays from)
  return device_call(g, B, x_dev, y_dev, kernel_ms, [&](auto x, auto y, int64_t n) {
    return conv_dev_t(g, lmax, M, Fin, Fout, theta, n, x, y);
  });
}

extern "C" int gspx_cheby_cross_grams_dev(gspx_graph* g, double lmax, int M, int Fin, int Fout, int64_t B,
                                          const void* x_dev, const void* z_dev, double* out, double* kernel_ms) {
  CHK(check_conv_args("gspx_cheby_cross_grams_dev", lmax, M, Fin, Fout, B));
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (B > 0 && (!out || (g->N > 0 && (!x_dev || !z_dev)))) return set_err(GSPX_ERR_INVALID, "null signal pointer");
  if (B >= ((int64_t)1 << 31) / 16 / std::max(Fin, Fout)) return set_err(GSPX_ERR_INVALID, "too many signals");
  replay_reset(g->ctx);  // (the kept slots overwrite the panels a recorded filter call replays from)
  return device_call(g, B, x_dev, out, kernel_ms, [&](auto x, auto, int64_t n) {
    return cross_grams_dev_t(g, lmax, M, Fin, Fout, n, x, (decltype(x))z_dev, out);
  });
}
