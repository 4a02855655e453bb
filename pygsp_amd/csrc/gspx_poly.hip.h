// gspx_poly.hip.h - the polynomial-filter pipeline (replaces approximations.py:58-114 cheby_op and the synthesis loop of
// filter.py:313-322): step plans, launch shapes and the launch_* family, the work panels of a batch, the column-batch
// driver (batch_width, run_batches), the three batch runners (run_batch, run_synthesis_batch, run_program_batch) and the
// Clenshaw step the synthesis and the graph convolution (gspx_conv.hip.h) share (clenshaw_step),
// filter_dev_t / program_dev_t / sqnorms_dev_t / moments_dev_t, device_call / host_call and the gspx_cheby_* /
// gspx_newton_* / gspx_poly_program* entry points.
// After gspx_graph.hip.h (ensure_factor, ensure_s1nat) and gspx_hostpipe.hip.h (host_call hands large calls to it).
#pragma once

// ------------------------------------------------------------------------------------------------
// step schedule ("plan")
// ------------------------------------------------------------------------------------------------
struct PlanStep {
  double scale = 1.0, gamma = -1.0;
  int flush = 0;   // 0 none, 1 write, 2 accumulate
  int final = 0;
  std::vector<double> w;  // nf*3: w_new, w_cur, w_old
};

// Fused-flush schedule.  T_k overwrites T_{k-2} in place, so a term must be folded into the
// accumulators no later than the step that overwrites it; folding happens every third step
// (when T_k, T_{k-1}, T_{k-2} are all in registers), i.e. 2/3 of an accumulator pass per step
// instead of the reference's one read-modify-write per step per filter
// (approximations.py:108-109).
//   cp: nf x M coefficients with c[.,0] already halved (approximations.py:103)
static void make_plan_fused(int nf, int M, const std::vector<double>& cp, bool acc_existing,
                            bool final_to_y, std::vector<PlanStep>& plan) {
  const int K = M - 1;
  plan.assign((size_t)K, PlanStep());
  int covered = -1;  // T_0..T_covered are already folded
  bool first = !acc_existing;
  for (int k = 1; k <= K; ++k) {
    PlanStep& st = plan[(size_t)k - 1];
    st.scale = (k == 1) ? 0.5 : 1.0;
    st.gamma = (k == 1) ? 0.0 : -1.0;
    st.w.assign((size_t)nf * 3, 0.0);
    const bool must = (k == K) || (k >= 2 && (k - 2) > covered);
    if (!must) continue;
    st.flush = first ? 1 : 2;
    first = false;
    st.final = (k == K && final_to_y) ? 1 : 0;
    for (int f = 0; f < nf; ++f) {
      const double* c = &cp[(size_t)f * M];
      if (k > covered) st.w[(size_t)f * 3 + 0] = c[k];
      if (k - 1 > covered) st.w[(size_t)f * 3 + 1] = c[k - 1];
      if (k >= 2 && k - 2 > covered) st.w[(size_t)f * 3 + 2] = c[k - 2];
    }
    covered = k;
  }
}

// Deferred schedule: every T_k is kept, no flush inside the steps.
static void make_plan_deferred(int nf, int M, std::vector<PlanStep>& plan) {
  const int K = M - 1;
  plan.assign((size_t)K, PlanStep());
  for (int k = 1; k <= K; ++k) {
    PlanStep& st = plan[(size_t)k - 1];
    st.scale = (k == 1) ? 0.5 : 1.0;
    st.gamma = (k == 1) ? 0.0 : -1.0;
    st.w.assign((size_t)nf * 3, 0.0);
  }
}

static void halve_c0(int nf, int M, const double* coeffs, std::vector<double>& cp) {
  cp.assign(coeffs, coeffs + (size_t)nf * M);
  for (int f = 0; f < nf; ++f) cp[(size_t)f * M] *= 0.5;
}

extern "C" int gspx_plan_describe(gspx_ctx* ctx, int Nf, int M, const double* coeffs,
                                  double* plan_out) {
  if (M < 2) return set_err(GSPX_ERR_COEFF, "The coefficients have an invalid shape");
  if (Nf < 1 || !coeffs || !plan_out) return set_err(GSPX_ERR_INVALID, "bad argument");
  Options opt;
  if (ctx) opt = ctx->opt;
  std::vector<double> cp;
  halve_c0(Nf, M, coeffs, cp);
  std::vector<PlanStep> plan;
  const bool deferred = opt.combine == 2 || (opt.combine == 0 && Nf >= 2);
  if (deferred)
    make_plan_deferred(Nf, M, plan);
  else
    make_plan_fused(Nf, M, cp, false, true, plan);
  const size_t stride = 4 + 3 * (size_t)Nf;
  for (size_t k = 0; k < plan.size(); ++k) {
    double* o = plan_out + k * stride;
    o[0] = plan[k].scale;
    o[1] = plan[k].gamma;
    o[2] = plan[k].flush;
    o[3] = plan[k].final;
    for (size_t j = 0; j < 3 * (size_t)Nf; ++j) o[4 + j] = plan[k].w[j];
  }
  return GSPX_OK;
}

// ------------------------------------------------------------------------------------------------
// kernel dispatch
// ------------------------------------------------------------------------------------------------
struct Shape {
  int kernel;  // 1 panel (lane groups), 2 narrow, 3 wave-row
  int vec;
  int wlog2;
  int glog2;   // narrow only
  int gridy;   // panel only
};

static Shape choose_shape(const Options& opt, size_t elt, int64_t ld, int veccap) {
  Shape s{};
  const int maxvec = std::min((int)(16 / elt), veccap);
  int vec = 1;
  for (int v = maxvec; v >= 1; v /= 2)
    if (ld % v == 0) { vec = v; break; }
  while (vec > 1 && ld / vec < 16) vec /= 2;
  if (opt.vec != 0 && opt.vec <= maxvec && ld % opt.vec == 0) vec = (int)opt.vec;
  int kernel = (ld <= 4) ? 2 : 1;
  if (opt.kernel == 2 && ld <= 64) kernel = 2;
  if (opt.kernel == 1 && ld > 4) kernel = 1;
  if (opt.kernel == 5 && ld > 4) kernel = 5;
  // auto: fp32 panels and fp64 panels of up to 32 signals -> LDS-staged kernel; wide fp64 panels ->
  // scalar-metadata lane-group kernel.  Measured (round 1, headline graph):
  // fp32 the LDS kernel is 25 % faster; fp64 x 8 / 16 / 32 signals 0.18 / 0.21 / 0.26 ms per order
  // against 0.28 / 0.31 / 0.37 (many rows per row set make the scalar blends expensive); fp64 x 64
  // the scalar-metadata kernel wins by 4 %.
  if (opt.kernel == 0 && kernel == 1 && (elt == 4 || ld <= 32)) kernel = 5;
  s.kernel = kernel;
  if (kernel == 1 || kernel == 5) {
    s.vec = vec;
    const int64_t lanes = ld / vec;
    s.wlog2 = lanes <= 16 ? 4 : (lanes <= 32 ? 5 : 6);
    s.gridy = (int)((lanes + 63) / 64);
    s.glog2 = 0;
  } else {
    s.vec = 1;
    int wl = 0;
    while ((1 << wl) < ld) ++wl;
    s.wlog2 = wl;
    // auto: 4 lanes per row in total (measured best on the cache-resident config 1)
    const int64_t gl = opt.narrow_g_log2 >= 0 ? opt.narrow_g_log2 : std::max(0, 2 - wl);
    s.glog2 = (int)std::min<int64_t>(gl, 6 - wl);
    s.gridy = 1;
  }
  return s;
}

template <typename T, int VEC, int MODE>
static void launch_panel_w(const StepArgs<T>& a, int wlog2, dim3 grid, hipStream_t st) {
#define GSPX_LP(WL)                                                                     \
  hipLaunchKernelGGL((k_step_panel<T, VEC, WL, MODE>), grid, dim3(64 * a.wpb), 0, st, a.rowptr, \
                     a.col, a.val, a.cur, a.wts, a.perm, a)
  switch (wlog2) {
    case 4: GSPX_LP(4); break;
    case 5: GSPX_LP(5); break;
    default: GSPX_LP(6); break;
  }
#undef GSPX_LP
}

template <typename T, int MODE>
static void launch_panel(const StepArgs<T>& a, const Shape& s, dim3 grid, hipStream_t st) {
  if constexpr (sizeof(T) == 4) {
    if (s.vec == 4) return launch_panel_w<T, 4, MODE>(a, s.wlog2, grid, st);
  }
  if (s.vec == 2) return launch_panel_w<T, 2, MODE>(a, s.wlog2, grid, st);
  return launch_panel_w<T, 1, MODE>(a, s.wlog2, grid, st);
}

template <typename T, int VEC, int MODE>
static void launch_lds_w(const StepArgs<T>& a, const unsigned* coff, int wlog2, dim3 grid,
                         hipStream_t st) {
  // (a.lds_pad: unused dynamic LDS that only lowers the workgroups resident per CU - an experiment knob for
  // graphs without locality, where fewer gathers in flight per L2 can mean more hits)
#define GSPX_LL(WL)                                                                          \
  hipLaunchKernelGGL((k_step_lds<T, VEC, WL, MODE>), grid, dim3(256), (size_t)a.lds_pad, st, a.rowptr, coff, \
                     a.val, a.cur, a.wts, a.perm, a)
  switch (wlog2) {
    case 4: GSPX_LL(4); break;
    case 5: GSPX_LL(5); break;
    default: GSPX_LL(6); break;
  }
#undef GSPX_LL
}

template <typename T, int MODE>
static void launch_lds(const StepArgs<T>& a, const unsigned* coff, const Shape& s, dim3 grid,
                       hipStream_t st) {
  if constexpr (sizeof(T) == 4) {
    if (s.vec == 4) return launch_lds_w<T, 4, MODE>(a, coff, s.wlog2, grid, st);
  }
  if (s.vec == 2) return launch_lds_w<T, 2, MODE>(a, coff, s.wlog2, grid, st);
  return launch_lds_w<T, 1, MODE>(a, coff, s.wlog2, grid, st);
}

template <typename T>
static void launch_step(gspx_ctx* ctx, StepArgs<T> a, const Shape& s, const Options& opt, hipStream_t st,
                        const unsigned* coff) {
  ++ctx->step_kinds[1];
  int rpw = (int)opt.rows_per_wave;
  if (rpw <= 0)
    rpw = (s.kernel == 5) ? (sizeof(T) == 4 ? 16 : 8) : (s.kernel == 2 ? 1 : 4);
  if (s.kernel == 1 || s.kernel == 5) {
    const int R = 64 >> s.wlog2;  // rows per row set
    rpw = ((rpw + R - 1) / R) * R;
    if (s.kernel == 5 && rpw > 32) rpw = 32;
  }
  a.rows_per_wave = rpw;
  int rows_per_chunk;
  a.lds_pad = (int)std::min<int64_t>(std::max<int64_t>(opt.lds_pad_kb, 0), 40) * 1024;
  a.wpb = (s.kernel == 1) ? (int)opt.waves_per_block : 4;
  if (s.kernel == 1 || s.kernel == 5)
    rows_per_chunk = a.wpb * rpw;
  else
    rows_per_chunk = rpw * (4 << (6 - s.wlog2 - s.glog2));
  a.nchunks = (a.N + rows_per_chunk - 1) / rows_per_chunk;
  int gx = a.nchunks;
  a.cpx = 0;
  if (opt.xcd_remap) {
    a.cpx = (a.nchunks + 7) / 8;
    gx = a.cpx * 8;
  }
  dim3 grid((unsigned)gx, (unsigned)s.gridy, 1);
  const int mode = a.flush ? 1 : ((a.beta != T(0) || a.nin > 0 || a.final) ? 2 : 0);
  if (s.kernel == 5) {
    if (mode == 1) launch_lds<T, 1>(a, coff, s, grid, st);
    else if (mode == 2) launch_lds<T, 2>(a, coff, s, grid, st);
    else launch_lds<T, 0>(a, coff, s, grid, st);
  } else if (s.kernel == 1) {
    if (mode == 1) launch_panel<T, 1>(a, s, grid, st);
    else if (mode == 2) launch_panel<T, 2>(a, s, grid, st);
    else launch_panel<T, 0>(a, s, grid, st);
  } else {
    if (a.flush)
      hipLaunchKernelGGL((k_step_narrow<T, true>), grid, dim3(256), 0, st, a, s.wlog2, s.glog2);
    else
      hipLaunchKernelGGL((k_step_narrow<T, false>), grid, dim3(256), 0, st, a, s.wlog2, s.glog2);
  }
}

template <typename T>
static void launch_permute_in(const T* x, unsigned ldx, T* out, unsigned ld, int N,
                              const int* perm, int vec, hipStream_t st) {
  const size_t total = (size_t)N * (ld / vec);
  const unsigned nb = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
  if (nb == 0) return;
  if constexpr (sizeof(T) == 4) {
    if (vec == 4) {
      hipLaunchKernelGGL((k_permute_in<T, 4>), dim3(nb), dim3(256), 0, st, x, ldx, out, ld, N, perm);
      return;
    }
  }
  if (vec == 2)
    hipLaunchKernelGGL((k_permute_in<T, 2>), dim3(nb), dim3(256), 0, st, x, ldx, out, ld, N, perm);
  else
    hipLaunchKernelGGL((k_permute_in<T, 1>), dim3(nb), dim3(256), 0, st, x, ldx, out, ld, N, perm);
}

template <typename T, int VEC>
static void launch_combine_v(const T* slots, int nslots, size_t slot_stride, const T* cf, int M,
                             int nf, int N, unsigned ld, T* y, unsigned ldy, size_t plane_y,
                             const int* perm, hipStream_t st, unsigned pitch) {
  const size_t total = (size_t)N * (ld / VEC);
  const unsigned nb = (unsigned)std::min<size_t>((total + 255) / 256, 16384);
  if (nb == 0) return;
  constexpr int NFB = 8;
  for (int f0 = 0; f0 < nf; f0 += NFB) {
    const int here = std::min(NFB, nf - f0);
    hipLaunchKernelGGL((k_combine<T, VEC, NFB>), dim3(nb), dim3(256), 0, st, slots, nslots,
                       slot_stride, cf, M, f0, here, N, ld, y, ldy, plane_y, perm, 0, pitch);
  }
}

template <typename T>
static void launch_combine(const T* slots, int nslots, size_t slot_stride, const T* cf, int M,
                           int nf, int N, unsigned ld, T* y, unsigned ldy, size_t plane_y,
                           const int* perm, int vec, hipStream_t st, unsigned pitch = 0) {
  if (!pitch) pitch = ld;
  if constexpr (sizeof(T) == 4) {
    if (vec == 4)
      return launch_combine_v<T, 4>(slots, nslots, slot_stride, cf, M, nf, N, ld, y, ldy, plane_y,
                                    perm, st, pitch);
  }
  if (vec == 2)
    return launch_combine_v<T, 2>(slots, nslots, slot_stride, cf, M, nf, N, ld, y, ldy, plane_y,
                                  perm, st, pitch);
  return launch_combine_v<T, 1>(slots, nslots, slot_stride, cf, M, nf, N, ld, y, ldy, plane_y,
                                perm, st, pitch);
}

// The squared column norms of a deferred batch instead of its outputs (gspx_cheby_sqnorms_dev): cf [k][ldc] fp64
// coefficients (c'_f0 halved, zero beyond Nf), out [Nf][ldo] fp64 at the batch's first column, part the workgroup
// partials (sqnorm_parts doubles at the call's widest batch).
struct SqNorms {
  const double* cf;
  int ldc, nf;
  double* out;
  size_t ldo;
  double* part;
};
static const int SQ_PASS = 128;  // filters per pass over the stack
static int sqnorm_cwl(unsigned w) {  // log2 of the columns of a tile: the batch width up to 64, a power of two
  int l = 0;
  while (l < 6 && (1u << l) < w) ++l;
  return l;
}
static int sqnorm_gx(const gspx_ctx* ctx, int N, unsigned w) {  // workgroups along the rows
  const int cwl = sqnorm_cwl(w);
  const int64_t tiles = ((int64_t)N + (64 >> cwl) - 1) / (64 >> cwl);
  const int64_t gy = ((int64_t)w + (1 << cwl) - 1) >> cwl;
  return (int)std::max<int64_t>(1, std::min<int64_t>(tiles, (4 * (int64_t)ctx->cu_count + gy - 1) / gy));
}
static size_t sqnorm_parts(const gspx_ctx* ctx, int N, unsigned w) {
  return (size_t)sqnorm_gx(ctx, N, w) * SQ_PASS * w;
}

template <typename T>
static int launch_combine_sqnorm(gspx_ctx* ctx, const T* slots, int nslots, size_t slot_stride, unsigned pitch, int N,
                                 unsigned w, const SqNorms& sq, hipStream_t st) {
  const size_t lds = (size_t)nslots * 64 * sizeof(double);
  const int cwl = sqnorm_cwl(w);
  const dim3 grid((unsigned)sqnorm_gx(ctx, N, w), (w + (1u << cwl) - 1) >> cwl);
  for (int f0 = 0; f0 < sq.nf; f0 += SQ_PASS) {
    const int here = std::min(SQ_PASS, sq.nf - f0);
    const int fb = here <= 8 ? 2 : here <= 32 ? 8 : 32;  // filters per wave: 4 waves cover the pass
    typedef void (*kern_t)(const T*, int, size_t, u32, int, int, int, const double*, int, double*);
    const kern_t kern = fb == 2 ? k_combine_sqnorm<T, 2> : fb == 8 ? k_combine_sqnorm<T, 8> : k_combine_sqnorm<T, 32>;
    if (lds > ((size_t)64 << 10))
      HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, slots, nslots, slot_stride, (u32)pitch, N, (int)w, cwl,
                       sq.cf + f0, sq.ldc, sq.part);
    const int64_t n = (int64_t)here * w;
    hipLaunchKernelGGL(k_sqnorm_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, sq.part, (int)grid.x,
                       4 * fb, here, (int)w, sq.out + (size_t)f0 * sq.ldo, sq.ldo);
  }
  return GSPX_OK;
}

// The inner products of neighbouring kept slots of a deferred batch instead of its outputs (gspx_cheby_moments_dev):
// out [2 S - 1][ldo] fp64 at the batch's first column (a_0 .. a_{S-1}, then b_0 .. b_{S-2}: k_slot_dots,
// gspx_moments.hip.h), part the workgroup partials (dots_parts doubles at the call's widest batch).
struct SlotDots {
  double* out;
  size_t ldo;
  double* part;
};
// the two builds of k_slot_dots: one column per lane in chunks of 16 slots; two columns per lane in chunks of 8 (the
// same registers) for fp32 panels whose rows split into pairs
static const int DOTS_CS[2] = {16, 8};
template <typename T> static int dots_vec(unsigned w, unsigned pitch) {
  return sizeof(T) == 4 && w % 2 == 0 && pitch % 2 == 0 ? 2 : 1;
}
static int dots_chunks(int S, int vec) { return (S - 1 + DOTS_CS[vec - 1] - 1) / DOTS_CS[vec - 1]; }  // grid.y, S >= 2
// row groups of a k_slot_dots launch: about eight workgroups per CU over all chunks and column blocks, no more than
// there are tiles of four waves, and at most 64 MiB of partials.  A function of N, w, S, the build and the CU count.
static int dots_gx(const gspx_ctx* ctx, int N, unsigned w, int S, int vec) {
  const int cwl = sqnorm_cwl(w / vec);
  const int64_t rows = 4 * (int64_t)(64 >> cwl);
  const int64_t tiles = ((int64_t)N + rows - 1) / rows;
  const int64_t others = (((int64_t)(w / vec) + (1 << cwl) - 1) >> cwl) * dots_chunks(S, vec);
  const int64_t fit = ((int64_t)64 << 20) / ((int64_t)(2 * S - 1) * w * (int64_t)sizeof(double));
  const int64_t want = (8 * (int64_t)ctx->cu_count + others - 1) / others;
  return (int)std::max<int64_t>(1, std::min(std::min(tiles, want), fit));
}
static size_t dots_parts(const gspx_ctx* ctx, int N, unsigned w, int S) {  // (whichever build a batch takes)
  const int gx = std::max(dots_gx(ctx, N, w, S, 1), w % 2 == 0 ? dots_gx(ctx, N, w, S, 2) : 0);
  return (size_t)gx * (size_t)(2 * S - 1) * w;
}

template <typename T>
static int launch_slot_dots(gspx_ctx* ctx, const T* slots, int S, size_t slot_stride, unsigned pitch, int N, unsigned w,
                            const SlotDots& sd, hipStream_t st) {
  const int vec = dots_vec<T>(w, pitch);
  const int cwl = sqnorm_cwl(w / vec);
  const int gx = dots_gx(ctx, N, w, S, vec);
  const dim3 grid((unsigned)gx, (unsigned)dots_chunks(S, vec), (w / vec + (1u << cwl) - 1) >> cwl);
  typedef void (*kern_t)(const T*, int, size_t, u32, int, int, int, double*);
  kern_t kern = k_slot_dots<T, 1, 16>;
  if constexpr (sizeof(T) == 4) {
    if (vec == 2) kern = k_slot_dots<T, 2, 8>;
  }
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, slots, S, slot_stride, (u32)pitch, N, (int)w, cwl, sd.part);
  const int64_t n = (int64_t)(2 * S - 1) * w;
  hipLaunchKernelGGL(k_dots_reduce, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, sd.part, gx, n, (int)w, sd.out,
                     sd.ldo);
  return GSPX_OK;
}

// The inner products of the kept slots of a deferred batch with nf foreign planes z instead of its outputs
// (gspx_cheby_cross_moments_dev): z [nf][N][ldz] at the batch's first column, in the CALLER's vertex order
// (k_slot_cross_dots reads its rows through the graph's permutation); out [nf][M][ldo] fp64 at the batch's first column;
// part the workgroup partials (cross_parts doubles at the call's widest batch).
struct CrossDots {
  const void* z;
  unsigned ldz;
  size_t zplane;
  int nf;
  double* out;
  size_t ldo;
  double* part;
};
// The builds of k_slot_cross_dots.  A pass takes at most CROSS_PASS planes; a pass of more than CROSS_FEW planes runs
// the wide build - 8 planes x a chunk of 8 slots, 64 fp64 accumulators, two waves per SIMD - and a pass of one or two
// planes (the single filter whose coefficients are learnt) the narrow one - 2 planes x a chunk of 16 slots, 32
// accumulators, four waves per SIMD and 17 or 18 loads in flight per lane where the wide build with one plane has 9:
// the kernel is bound by the loads it keeps in flight (profiles/autograd.md).  fp32 panels whose rows split into pairs
// take two columns per lane and half the chunk: the same accumulators, 8-byte loads.
static const int CROSS_PASS = 8, CROSS_FEW = 2;
static int cross_cs(int here, int vec) { return (here <= CROSS_FEW ? 16 : 8) / vec; }  // slots per chunk
template <typename T> static int cross_vec(unsigned w, unsigned pitch, const T* z, unsigned ldz) {
  return dots_vec<T>(w, pitch) == 2 && ldz % 2 == 0 && ((uintptr_t)z % (2 * sizeof(T))) == 0 ? 2 : 1;
}
static int cross_chunks(int M, int here, int vec) { return (M + cross_cs(here, vec) - 1) / cross_cs(here, vec); }  // grid.y
// row groups of a k_slot_cross_dots launch of `here` planes: as dots_gx, with here M w doubles per row group
static int cross_gx(const gspx_ctx* ctx, int N, unsigned w, int M, int here, int vec) {
  const int cwl = sqnorm_cwl(w / vec);
  const int64_t rows = 4 * (int64_t)(64 >> cwl);
  const int64_t tiles = ((int64_t)N + rows - 1) / rows;
  const int64_t others = (((int64_t)(w / vec) + (1 << cwl) - 1) >> cwl) * cross_chunks(M, here, vec);
  const int64_t fit = ((int64_t)64 << 20) / ((int64_t)here * M * w * (int64_t)sizeof(double));
  const int64_t want = (8 * (int64_t)ctx->cu_count + others - 1) / others;
  return (int)std::max<int64_t>(1, std::min(std::min(tiles, want), fit));
}
static size_t cross_parts(const gspx_ctx* ctx, int N, unsigned w, int M, int nf) {  // (whichever build and pass)
  size_t most = 0;
  for (int here : {std::min(nf, CROSS_PASS), nf % CROSS_PASS})
    for (int vec = 1; here > 0 && vec <= (w % 2 == 0 ? 2 : 1); ++vec)
      most = std::max(most, (size_t)cross_gx(ctx, N, w, M, here, vec) * (size_t)here * M * w);
  return most;
}

template <typename T>
static int launch_slot_cross_dots(gspx_ctx* ctx, const T* slots, int M, size_t slot_stride, unsigned pitch, int N,
                                  unsigned w, const int* perm, const CrossDots& cd, hipStream_t st) {
  const T* z = (const T*)cd.z;
  const int vec = cross_vec<T>(w, pitch, z, cd.ldz);
  const int cwl = sqnorm_cwl(w / vec);
  typedef void (*kern_t)(const T*, int, size_t, u32, const T*, int, size_t, u32, const int*, int, int, int, double*);
  for (int f0 = 0; f0 < cd.nf; f0 += CROSS_PASS) {
    const int here = std::min(CROSS_PASS, cd.nf - f0);
    const bool few = here <= CROSS_FEW;
    kern_t kern = few ? k_slot_cross_dots<T, 1, 16, CROSS_FEW> : k_slot_cross_dots<T, 1, 8, CROSS_PASS>;
    if constexpr (sizeof(T) == 4) {
      if (vec == 2) kern = few ? k_slot_cross_dots<T, 2, 8, CROSS_FEW> : k_slot_cross_dots<T, 2, 4, CROSS_PASS>;
    }
    const int gx = cross_gx(ctx, N, w, M, here, vec);
    const dim3 grid((unsigned)gx, (unsigned)cross_chunks(M, here, vec), (w / vec + (1u << cwl) - 1) >> cwl);
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, slots, M, slot_stride, (u32)pitch, z + (size_t)f0 * cd.zplane, here,
                       cd.zplane, (u32)cd.ldz, perm, N, (int)w, cwl, cd.part);
    const int64_t n = (int64_t)here * M * w;
    hipLaunchKernelGGL(k_dots_reduce, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, cd.part, gx, n, (int)w,
                       cd.out + (size_t)f0 * M * cd.ldo, cd.ldo);
  }
  return GSPX_OK;
}

// What a header further down does with the kept slots of a deferred batch instead of its outputs (gspx_conv.hip.h: the
// cross-Grams): fn(ctx, slots, M, slot stride, slot pitch, N, batch width, the internal row -> caller's row map, arg,
// stream), launched where the combine would be.
struct SlotsUse {
  int (*fn)(gspx_ctx*, const void*, int, size_t, unsigned, int, unsigned, const int*, const void*, hipStream_t);
  const void* arg;
};

// ------------------------------------------------------------------------------------------------
// the filter
// ------------------------------------------------------------------------------------------------
// LDS-staged gather step (gspx_tile_kernels.hip.h): usable when the graph carries gather tiles and
// every panel the kernel touches is made of 16-byte lane pieces
// a work panel of row pitch ld can take the tile kernels
template <typename T> static bool tile_geometry(const gspx_graph* g, const Options& opt, unsigned ld) {
  constexpr int TVEC = 16 / (int)sizeof(T);
  const size_t U = (size_t)g->N * ld;
  return opt.tile_gather && g->gt_rows == GSPX_TILE_BR && (size_t)ld * sizeof(T) >= (size_t)opt.tile_min_row &&
         (ld % TVEC) == 0 && U * sizeof(T) < ((size_t)1 << 31) && (size_t)g->nnz_int * sizeof(T) < ((size_t)1 << 31);
}
// ... and the final flush can store 16-byte pieces straight into y
template <typename T>
static bool tile_usable(const gspx_graph* g, const Options& opt, unsigned ld, const T* y, unsigned ldy) {
  constexpr int TVEC = 16 / (int)sizeof(T);
  return tile_geometry<T>(g, opt, ld) && (ldy % TVEC) == 0 && (((uintptr_t)y / sizeof(T)) % TVEC) == 0;
}
// fills the graph / geometry fields of t and launches; the caller sets cur, old, out, racc, y,
// ldy, perm, scale, gamma, beta, flush, final, wn, wc, wo
template <typename T>
static int launch_step_tile(gspx_graph* g, const Options& opt, TileArgs<T> t, unsigned ld, hipStream_t st,
                            const T* vals = nullptr) {
  // narrow panels (rows of at most 128 bytes): 8- / 4- / 2- / 1-lane row groups in workgroups of 512 / 256 / 128 / 64
  // threads - every lane holds a piece of a row, and the smaller workgroups keep more blocks in flight per CU
  const size_t rowb = (size_t)ld * sizeof(T);
  int lg = rowb <= 16 ? 1 : rowb <= 32 ? 2 : rowb <= 64 ? 4 : rowb <= 128 ? 8 : 16;
  if (opt.tile_lg == 8 || opt.tile_lg == 4 || opt.tile_lg == 2) lg = rowb <= 128 ? std::max(lg, (int)opt.tile_lg) : 16;  // (tuning)
  // (the 8-lane build in 256-thread workgroups with two rows per group - four resident workgroups instead of two -
  // measured within 3 % of the 512-thread build on 80- to 128-byte rows: those passes are not latency bound.)
  // (several column chunks per block with the small builds lose to the 16-lane build: 96- / 192-byte rows 4.1 / 6.7 ms
  // against 2.7 / 4.9 ms on the headline graph - a pass per chunk costs more than the idle lanes of a last chunk)
  const bool narrow = lg < 16;
  const int ncol = narrow ? 1 : (int)((rowb + 255) / 256);
  const int flavour = t.old_rows ? 1 : t.nin > 0 ? 2 : 0;  // plain | T_{k-2} from the caller's unpermuted panel
                                                           // (step 2 of a fused-input filter) | extra input panels
                                                           // (synthesis); never both
  typedef void (*kern_t)(const TileArgs<T>);
  static const kern_t wide[3][3] = {
      {k_step_tile<T, 0>, k_step_tile<T, 1>, k_step_tile<T, 2>},
      {k_step_tile<T, 0, 16, true>, k_step_tile<T, 1, 16, true>, k_step_tile<T, 2, 16, true>},
      {k_step_tile<T, 0, 16, false, true>, k_step_tile<T, 1, 16, false, true>, k_step_tile<T, 2, 16, false, true>}};
  static const kern_t slim[3][4] = {
      {k_step_tile<T, 1, 1, false, false, 64>, k_step_tile<T, 1, 2, false, false, 128>,
       k_step_tile<T, 1, 4, false, false, 256>, k_step_tile<T, 1, 8>},
      {k_step_tile<T, 1, 1, true, false, 64>, k_step_tile<T, 1, 2, true, false, 128>,
       k_step_tile<T, 1, 4, true, false, 256>, k_step_tile<T, 1, 8, true>},
      {k_step_tile<T, 1, 1, false, true, 64>, k_step_tile<T, 1, 2, false, true, 128>,
       k_step_tile<T, 1, 4, false, true, 256>, k_step_tile<T, 1, 8, false, true>}};
  kern_t kern = narrow ? slim[flavour][lg == 1 ? 0 : lg == 2 ? 1 : lg == 4 ? 2 : 3] : wide[flavour][ncol <= 2 ? ncol : 0];
  unsigned threads = narrow ? 64u * (unsigned)lg : 512u;
  // a step without a flush (every step of a Newton or product program and of a deferred combine; 18 of the 30 steps of
  // the headline call): the flush-free builds of the wide plain flavour (gspx_tile_kernels.hip.h, ACC = false) - the
  // same T_k, bit for bit.  (Synthesis steps, the narrow and the regrouped builds have none: not measured.)
  const bool noacc = opt.tile_acc_builds && t.flush == 0 && !narrow && flavour == 0;
  if (noacc) {
    static const kern_t freek[3] = {k_step_tile<T, 0, 16, false, false, 512, 16, 0, false>,
                                    k_step_tile<T, 1, 16, false, false, 512, 16, 0, false>,
                                    k_step_tile<T, 2, 16, false, false, 512, 16, 0, false>};
    kern = freek[ncol <= 2 ? ncol : 0];
  }
  // calibration (gspx_bench_step_mix): the same launch with the row products removed (gspx_tile_kernels.hip.h, MIX)
  bool mix = false;
  if (opt.calib_mix && !narrow && flavour == 0) {
    static const kern_t mixk[2][3] = {
        {k_step_tile<T, 0, 16, false, false, 512, 16, 1>, k_step_tile<T, 1, 16, false, false, 512, 16, 1>,
         k_step_tile<T, 2, 16, false, false, 512, 16, 1>},
        {k_step_tile<T, 0, 16, false, false, 512, 16, 2>, k_step_tile<T, 1, 16, false, false, 512, 16, 2>,
         k_step_tile<T, 2, 16, false, false, 512, 16, 2>}};
    // (the same split as the real launches: a flush-free step is calibrated against its flush-free twin)
    static const kern_t mixfree[2][3] = {
        {k_step_tile<T, 0, 16, false, false, 512, 16, 1, false>, k_step_tile<T, 1, 16, false, false, 512, 16, 1, false>,
         k_step_tile<T, 2, 16, false, false, 512, 16, 1, false>},
        {k_step_tile<T, 0, 16, false, false, 512, 16, 2, false>, k_step_tile<T, 1, 16, false, false, 512, 16, 2, false>,
         k_step_tile<T, 2, 16, false, false, 512, 16, 2, false>}};
    kern = (noacc ? mixfree : mixk)[opt.calib_mix == 2 ? 1 : 0][ncol <= 2 ? ncol : 0];
    mix = true;
  }
  // rows of fewer 16-byte pieces than the lanes they are staged with: the builds whose compute phases regroup the
  // threads by pieces (template parameter CL), in workgroups of 64 x pieces (one row per group) or 32 x pieces (two
  // rows) threads.  Measured per piece count, A/B on one box (profiles/r04_regroup_ab*.json): 3 pieces (48-byte rows:
  // 5 / 6 fp64, 10 / 12 fp32 signals) +6...8 %, 5 pieces (80 bytes: 10 fp64) +2.5 %, 10 pieces (160 bytes: 20 fp64)
  // +6 %; 6, 7, 12 and 14 pieces -2...0 % (idle compute lanes are not what bounds those passes) - they keep the
  // power-of-two builds.
  const int pieces = (int)(rowb / 16);
  if (opt.tile_regroup && ncol == 1 && flavour != 1 && pieces < lg && !mix) {
#define GSPX_CL(LG_, CL_, NT_) \
  (flavour == 2 ? (kern_t)k_step_tile<T, 1, LG_, false, true, NT_, CL_> : (kern_t)k_step_tile<T, 1, LG_, false, false, NT_, CL_>)
    kern_t k2 = nullptr;
    unsigned nt2 = 0;
    if (lg == 4 && pieces == 3) k2 = GSPX_CL(4, 3, 192), nt2 = 192;
    else if (lg == 8 && pieces == 5) k2 = GSPX_CL(8, 5, 320), nt2 = 320;
    else if (lg == 16 && pieces == 10) k2 = GSPX_CL(16, 10, 320), nt2 = 320;
#undef GSPX_CL
    if (k2) kern = k2, threads = nt2;
  }
  // dynamic LDS: the wide builds take the tile budget the blocks were classified with; a narrow build's tile
  // rows are 16 lg bytes, so the largest staged block needs far less - and more workgroups fit a CU
  size_t lds = g->gt_lds;
  if (lg < 8)
    lds = std::min(lds, (size_t)GSPX_TILE_MAXN1 * 16 * lg + (((size_t)g->gt_entmax * sizeof(T) + 15) & ~(size_t)15) +
                            (((size_t)g->gt_entmax + 15) & ~(size_t)15) + 64);
  if (lg < 8) lds = (lds + 2047) & ~(size_t)2047;  // (graphs differ in their largest block: few distinct sizes)
  int per_cu = 2;
  {  // once per kernel build, device and LDS size (a driver call per launch would cost microseconds each)
    struct Known { size_t attr = 0; std::map<size_t, int> fit; };
    static std::map<std::pair<const void*, int>, Known> known;
    static std::mutex lds_mu;
    std::lock_guard<std::mutex> lock(lds_mu);
    Known& k = known[std::make_pair((const void*)kern, g->ctx->device)];
    if (k.attr < lds) {  // the limit only ever grows
      HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      k.attr = lds;
    }
    if (lg < 8) {  // resident workgroups of the small builds: what registers and LDS allow
      auto it = k.fit.find(lds);
      if (it == k.fit.end()) {
        int fit = 2;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, (const void*)kern, (int)threads, lds));
        it = k.fit.emplace(lds, std::max(2, std::min(fit, 16))).first;
      }
      per_cu = it->second;
    }
  }
  t.rowptr = g->rptr.as<int>();
  t.col = g->rcol.as<int>();
  t.val = vals ? vals : g->fval.as<T>();  // any values array on the internal pattern
  t.hdr = g->gt_hdr.as<int>();
  if (!t.s1rows) t.s1rows = g->gt_s1rows.as<int>();  // (the caller may pass the lists in its panel's row order)
  t.lidx = g->gt_lidx.as<unsigned char>();
  t.N = (int)g->N;
  t.ld = ld;
  t.panel_bytes = (unsigned)((size_t)g->N * ld * sizeof(T));
  t.val_bytes = (unsigned)((size_t)g->nnz_int * sizeof(T));
  t.lidx_bytes = (unsigned)((size_t)g->nnz_int);
  t.nb = g->gt_nb;
  t.ncol = ncol;
  t.per_xcd = (t.nb + 7) / 8;
  t.lds_bytes = (int)lds;
  unsigned nwg = (unsigned)std::max<int64_t>(8, ((int64_t)per_cu * g->ctx->cu_count) / 8 * 8);
  if (opt.tile_workgroups > 0)
    nwg = (unsigned)std::max<int64_t>(8, std::min<int64_t>(opt.tile_workgroups, 1 << 20) / 8 * 8);
  nwg = std::min(nwg, 8u * (unsigned)std::max(t.per_xcd, 1));  // (workgroups beyond an XCD's blocks would exit at once)
  t.nt = opt.tile_nt >= 0 ? (int)opt.tile_nt : ((size_t)g->N * ld * sizeof(T) >= ((size_t)192 << 20) ? 5 : 0);
  ++g->ctx->step_kinds[0];
  hipLaunchKernelGGL(kern, dim3(nwg), dim3(threads), lds, st, t);
  return GSPX_OK;
}

// byte offsets col*ld*sizeof(T) of the stored entries for this panel width (cached on the graph; the
// LDS-staged plain kernel reads them)
template <typename T>
static int prepare_coff(gspx_graph* g, const Shape& shape, unsigned ld, hipStream_t st) {
  if (shape.kernel == 5 && g->coff_ldb != ld * (unsigned)sizeof(T)) {
    CHK(g->coff.ensure(((size_t)g->nnz_int + 64) * sizeof(unsigned)));
    const int nb = std::max(1, (int)((g->N + 255) / 256));
    hipLaunchKernelGGL((k_coff<T>), dim3(nb), dim3(256), 0, st, g->rptr.as<int>(), g->rcol.as<int>(), (int)g->N,
                       ld * (unsigned)sizeof(T), g->coff.as<unsigned>());
    g->coff_ldb = ld * (unsigned)sizeof(T);
  }
  return GSPX_OK;
}

// the widest lane vector, at most v, whose accesses to rows of pitch ld starting at p stay aligned
template <typename T> static int vec_cap(int v, unsigned ld, const T* p) {
  while (v > 1 && ((ld % v) != 0 || (((uintptr_t)p / sizeof(T)) % v) != 0)) v /= 2;
  return v;
}

// The work panels of a batch of ld signals.  tile_direct: the tile kernels on panels of pitch ld, the last step storing
// into y.  padded: rows that are not made of 16-byte pieces (or a y the final flush cannot store such pieces into) get
// work panels of pitch ldw, rounded up to whole pieces, so that the tile kernels take them all the same - zero columns
// cost little next to kernels that are several times faster - and the result leaves through a copy.  `tiles`: the
// caller's steps may take the tile kernels at all; `planes`: the panels one tile launch spans (its buffer window stays
// below 2 GiB).
struct WorkPanels {
  bool tile_direct, padded;
  unsigned ldw;
};
template <typename T>
static WorkPanels work_panels(const gspx_graph* g, const Options& opt, bool tiles, size_t planes, unsigned ld,
                              const T* y, unsigned ldy) {
  constexpr unsigned TVEC = 16 / (unsigned)sizeof(T);
  const unsigned ldp = (ld + TVEC - 1) / TVEC * TVEC;
  auto window = [&](unsigned w) { return planes * (size_t)g->N * w * sizeof(T) < ((size_t)1 << 31); };
  // (a single signal on a graph whose matrix stays in the L2s: the sub-wave kernel is the faster one there, 0.125
  // against 0.150 ms for 30 orders at N = 50k; from ~20 MB of matrix on the padded tile path wins, 0.86 against
  // 1.19 ms at N = 1M.  Two signals and more: the tile path at every size - 0.15 against 0.18 ms for two fp32
  // signals at N = 100k.)
  const bool pad_pays = opt.tile_pad == 2 || ld >= 2 ||
                        (size_t)g->nnz_int * (sizeof(T) + 4) >= ((size_t)20 << 20);
  WorkPanels p;
  p.tile_direct = tiles && tile_usable<T>(g, opt, ld, y, ldy) && window(ld);
  p.padded = !p.tile_direct && tiles && opt.tile_pad && pad_pays && tile_geometry<T>(g, opt, ldp) && window(ldp);
  p.ldw = p.padded ? ldp : ld;
  return p;
}

// what every plain step (StepArgs) of a batch shares: the graph, the panel geometry and the final store into y
template <typename T>
static StepArgs<T> step_base(const gspx_graph* g, unsigned ld, T* y, unsigned ldy) {
  StepArgs<T> a{};
  a.rowptr = g->rptr.as<int>();
  a.col = g->rcol.as<int>();
  a.val = g->fval.as<T>();
  a.N = (int)g->N;
  a.ld = ld;
  a.curbytes = (u32)((size_t)g->N * ld * sizeof(T));
  a.y = y;
  a.ldy = ldy;
  a.perm = g->has_perm ? g->perm.as<int>() : nullptr;
  return a;
}

// the four pool events of a batch, the first recorded at once: copy in | steps | combine or copy out between them
// (run_batches sums each phase over the batches)
static int batch_events(gspx_ctx* ctx, size_t& ev_idx, hipEvent_t ev[4]) {
  for (int i = 0; i < 4; ++i) ev[i] = pool_event(ctx, ++ev_idx);
  if (!ev[0] || !ev[1] || !ev[2] || !ev[3]) return set_err(GSPX_ERR_HIP, "hipEventCreate failed");
  HIPCHK(hipEventRecord(ev[0], ctx->stream));
  return GSPX_OK;
}

// Signals per column batch of a device call: bounded by the 2 GiB buffer-descriptor window, by the workspace budget
// (`panels` workspace columns of N elements per signal) and by max_batch.  A call of several batches gets widths that
// are multiples of 4: batch starts stay 16-byte friendly.
static int batch_width(const gspx_graph* g, size_t elt, size_t panels, int64_t Nsig, int64_t* width) {
  const Options& opt = g->ctx->opt;
  const size_t rowb = (size_t)g->N * elt;
  int64_t max_ld = (int64_t)((((size_t)1 << 31) - 65536) / rowb);
  if (max_ld < 1)
    return set_err(GSPX_ERR_INVALID, "graph too large: one signal column exceeds 2 GiB");
  const size_t budget = (size_t)std::max<int64_t>(opt.ws_limit_mb, 1) << 20;
  max_ld = std::min<int64_t>(max_ld, std::max<int64_t>(1, (int64_t)(budget / (rowb * panels))));
  if (opt.max_batch > 0) max_ld = std::min<int64_t>(max_ld, opt.max_batch);
  if (max_ld < Nsig && max_ld >= 4) max_ld &= ~(int64_t)3;
  *width = max_ld;
  return GSPX_OK;
}

// The column batches of a device call: batch(c0, ld, ev_idx) runs signals [c0, c0 + ld) and takes its pool events
// from batch_events.  Then the call's device time, the per-phase sums and the steps run (`steps` per batch) go to
// ctx->timing[0..4].
template <typename Batch>
static int run_batches(gspx_graph* g, int64_t Nsig, int64_t width, int steps, const Batch& batch) {
  gspx_ctx* ctx = g->ctx;
  size_t ev_idx = 0;
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  for (int64_t c0 = 0; c0 < Nsig; c0 += width)
    CHK(batch(c0, (unsigned)std::min<int64_t>(width, Nsig - c0), ev_idx));
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
  ctx->timing[0] = ms;
  double phase[3] = {0, 0, 0};  // copy in, steps, combine / copy out
  for (size_t i = 0; i + 3 < ev_idx; i += 4)
    for (size_t j = 0; j < 3; ++j) {
      float t = 0;
      HIPCHK(hipEventElapsedTime(&t, ctx->ev_pool[i + j], ctx->ev_pool[i + j + 1]));
      phase[j] += t;
    }
  ctx->timing[1] = phase[1];
  ctx->timing[2] = (double)(ev_idx / 4) * steps;
  ctx->timing[3] = phase[0];
  ctx->timing[4] = phase[2];
  return GSPX_OK;
}

// One (sub)problem: nf filters applied to one batch of `ld` signals whose first column is
// x/y column c0.  x: [N][ldx] (+c0), y: [nf][N][ldy] (+c0).
template <typename T>
static int run_batch(gspx_graph* g, int nf, int M, const std::vector<double>& cp, const T* x,
                     unsigned ldx, T* y, unsigned ldy, unsigned ld, bool deferred,
                     bool acc_existing, bool final_to_y, size_t& ev_idx, const SqNorms* sq = nullptr,
                     const SlotDots* sd = nullptr, const CrossDots* cd = nullptr, const SlotsUse* use = nullptr) {
  gspx_ctx* ctx = g->ctx;
  const Options& opt = ctx->opt;
  hipStream_t st = ctx->stream;
  const int N = (int)g->N;
  const int K = M - 1;
  const WorkPanels wp = work_panels<T>(g, opt, deferred || nf == 1, 1, ld, y, ldy);
  const bool tile_direct = wp.tile_direct, padded = wp.padded;
  const unsigned ldw = wp.ldw;
  const size_t U = (size_t)N * ldw;  // elements per panel
  // vector stores into y need aligned rows: cap the lane vector width accordingly
  const Shape shape = choose_shape(opt, sizeof(T), ld, vec_cap(4, ldy, y));
  const int* perm = g->has_perm ? g->perm.as<int>() : nullptr;

  std::vector<PlanStep> plan;
  if (deferred)
    make_plan_deferred(nf, M, plan);
  else
    make_plan_fused(nf, M, cp, acc_existing, final_to_y, plan);

  // device-side weights / coefficients
  std::vector<T> hw;
  if (deferred) {
    hw.resize((size_t)nf * M);
    for (size_t i = 0; i < hw.size(); ++i) hw[i] = (T)cp[i];
  } else {
    hw.resize((size_t)K * nf * 3);
    for (int k = 0; k < K; ++k)
      for (int j = 0; j < nf * 3; ++j) hw[(size_t)k * nf * 3 + j] = (T)plan[(size_t)k].w[(size_t)j];
  }
  const bool cap = ctx->capturing;  // replay recording: the previous eager call left the same weights
  if (!cap) {                       // and workspace in place
    CHK(ctx->ws_w.ensure(hw.size() * sizeof(T) + 64));
    HIPCHK(hipMemcpyAsync(ctx->ws_w.p, hw.data(), hw.size() * sizeof(T), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // hw is a stack-owned staging buffer
  }

  const size_t nslots = deferred ? (size_t)M : 2;
  // (Shifting slot 1 or the accumulator against slot 0 by 256 B ... 16 MB changes nothing: the placement effect of
  // profiles/r06_placement.md is not stream-against-stream channel aliasing - tools/skew_sweep.py's record.)
  const size_t SU = U;  // slot pitch
  CHK(ctx->ws_t.ensure(nslots * SU * sizeof(T) + 256));
  if (!deferred) CHK(ctx->ws_r.ensure((size_t)nf * U * sizeof(T) + 256));
  T* slots = ctx->ws_t.as<T>();
  T* racc = ctx->ws_r.as<T>();

  hipEvent_t ev[4] = {};
  if (!cap) CHK(batch_events(ctx, ev_idx, ev));
  // LDS-staged gather: one filter with the fused flush
  // (or a filterbank's deferred combine, whose steps are plain recurrence steps into kept slots)
  const bool tile_ok = tile_direct || padded;
  // Fused input: step 1 gathers straight from the caller's panel (the tile lists mapped through the
  // vertex order) and step 2 reads T_0 from it, so the copy into the internal order never happens.
  // Needs every block on the LDS path, the panel in the internal row pitch, and x not aliasing y
  // (the copy used to make in-place calls safe).
  const unsigned char* xb = (const unsigned char*)x;
  const unsigned char* yb = (const unsigned char*)y;
  const size_t xbytes = (size_t)N * ldx * sizeof(T), ybytes = (size_t)nf * N * ldy * sizeof(T);
  const bool fuse_in = tile_direct && !deferred && opt.fuse_input && g->gt_slow == 0 && ldx == ld &&
                       ((uintptr_t)x % 16) == 0 && (xb + xbytes <= yb || yb + ybytes <= xb) &&
                       (!g->has_perm || (g->gt_ns1 > 0 && (!cap || g->gt_s1nat.p)));
  if (fuse_in) {
    CHK(ensure_s1nat(g, st));
  } else if (padded) {
    const unsigned nb = (unsigned)std::min<size_t>((U + 255) / 256, 65536);
    hipLaunchKernelGGL((k_permute_in_pad<T>), dim3(nb), dim3(256), 0, st, x, ldx, slots, ldw, ld, N, perm);
  } else {  // (permute-in vector width: x rows must be aligned too)
    launch_permute_in<T>(x, ldx, slots, ld, N, perm, vec_cap(shape.vec, ldx, x), st);
  }
  if (!cap) HIPCHK(hipEventRecord(ev[1], st));

  CHK(prepare_coff<T>(g, shape, ld, st));
  StepArgs<T> a = step_base<T>(g, ld, y, ldy);
  a.nf = nf;
  a.racc = racc;
  for (int k = 1; k <= K; ++k) {
    const PlanStep& ps = plan[(size_t)k - 1];
    if (tile_ok) {
      TileArgs<T> t{};
      if (deferred) {
        t.cur = slots + (size_t)(k - 1) * SU;
        t.old = (k >= 2 && ps.gamma != 0.0) ? slots + (size_t)(k - 2) * SU : t.cur;
        t.out = slots + (size_t)k * SU;
      } else {
        t.cur = slots + (size_t)((k - 1) & 1) * SU;
        t.old = ps.gamma == 0.0 ? t.cur : slots + (size_t)(k & 1) * SU;
        t.out = slots + (size_t)(k & 1) * SU;
        if (fuse_in && k == 1) {  // T_0 is the caller's panel
          t.cur = x;
          t.old = x;
          t.s1rows = g->has_perm ? g->gt_s1nat.as<int>() : nullptr;
        } else if (fuse_in && k == 2) {
          t.old = x;
          t.old_rows = perm;  // null without an internal order: plain rows
        }
      }
      t.racc = racc;
      t.y = y;
      t.ldy = ldy;
      t.perm = perm;
      t.scale = (T)ps.scale;
      t.gamma = (T)ps.gamma;
      t.beta = T(0);
      t.flush = ps.flush;
      t.final = padded ? 0 : ps.final;  // padded rows: the last flush stays in the accumulator panel, copied out below
      t.reverse = (opt.alternate_sweep && (k & 1)) ? 1 : 0;
      if (ps.flush) {
        t.wn = (T)ps.w[0];
        t.wc = (T)ps.w[1];
        t.wo = (T)ps.w[2];
      }
      CHK(launch_step_tile<T>(g, opt, t, ldw, st));
      continue;
    }
    if (deferred) {
      a.cur = slots + (size_t)(k - 1) * SU;
      a.old = k >= 2 ? slots + (size_t)(k - 2) * SU : slots;
      a.out = slots + (size_t)k * SU;
    } else {
      a.cur = slots + (size_t)((k - 1) & 1) * SU;
      a.old = slots + (size_t)(k & 1) * SU;
      a.out = slots + (size_t)(k & 1) * SU;
    }
    if (ps.gamma == 0.0) a.old = a.cur;  // never read for its value; keeps the kernel branch-free
    a.scale = (T)ps.scale;
    a.gamma = (T)ps.gamma;
    a.flush = ps.flush;
    a.final = ps.final;
    a.reverse = (opt.alternate_sweep && (k & 1)) ? 1 : 0;
    a.wts = ctx->ws_w.as<T>() + (size_t)(k - 1) * nf * 3;
    launch_step<T>(ctx, a, shape, opt, st, g->coff.as<unsigned>());
  }
  if (!cap) HIPCHK(hipEventRecord(ev[2], st));
  if (deferred && sq) {  // the squared column norms in place of the outputs (rows in any order: no perm)
    CHK(launch_combine_sqnorm<T>(ctx, slots, M, SU, ldw, N, ld, *sq, st));
  } else if (deferred && sd) {  // the slots' inner products in place of the outputs (likewise)
    CHK(launch_slot_dots<T>(ctx, slots, M, SU, ldw, N, ld, *sd, st));
  } else if (deferred && cd) {  // the slots' inner products with the caller's planes, read through the vertex order
    CHK(launch_slot_cross_dots<T>(ctx, slots, M, SU, ldw, N, ld, perm, *cd, st));
  } else if (deferred && use) {  // whatever the caller does with the kept slots
    CHK(use->fn(ctx, slots, M, SU, ldw, N, ld, perm, use->arg, st));
  } else if (deferred) {
    launch_combine<T>(slots, M, SU, ctx->ws_w.as<T>(), M, nf, N, ld, y, ldy, (size_t)N * ldy, perm,
                      padded ? 1 : vec_cap(shape.vec, ldy, y), st, ldw);
  } else if (padded && final_to_y) {
    const unsigned nb = (unsigned)std::min<size_t>(((size_t)N * ld + 255) / 256, 65536);
    hipLaunchKernelGGL((k_permute_out_pad<T>), dim3(nb), dim3(256), 0, st, racc, ldw, y, ldy, ld, N, perm);
  }
  if (!cap) {
    HIPCHK(hipEventRecord(ev[3], st));
    HIPCHK(hipGetLastError());
  }
  return GSPX_OK;
}

// One step of the vector-coefficient Clenshaw recurrence on a batch's work panels (run_synthesis_batch, and
// run_conv_batch of gspx_conv.hip.h):  b_k = u_k + F b_{k+1} - b_{k+2}, out = u_0 + (F/2) b_1 - b_2, with
// u_k = sum_f wts[f] inp[f] over nin input panels of the work panels' geometry.  `first` is the panel step K gathers
// from with scale 0 (b_K = u_K needs no product: any valid panel).  B: the two recurrence panels; step 0 stores into y
// on the tile_direct and plain routes and leaves b_0 in B[0] on the padded one.  a: step_base of the batch.
template <typename T>
static int clenshaw_step(gspx_graph* g, const Options& opt, const WorkPanels& wp, const Shape& shape, StepArgs<T>& a,
                         int k, int K, const T* inp, const T* wts, int nin, const T* first, T* const B[2], T* y,
                         unsigned ldy, hipStream_t st) {
  gspx_ctx* ctx = g->ctx;
  const bool has_b2 = (k + 2 <= K);
  if (wp.tile_direct || wp.padded) {
    TileArgs<T> t{};
    t.cur = (k == K) ? first : B[(k + 1) & 1];
    t.old = (k < K && has_b2) ? B[k & 1] : t.cur;
    t.out = B[k & 1];
    t.racc = B[0];  // unused (flush == 0)
    t.y = y;
    t.ldy = ldy;
    t.perm = a.perm;
    t.scale = (k == K) ? T(0) : (k == 0 ? T(0.5) : T(1));
    t.gamma = (k < K && has_b2) ? T(-1) : T(0);
    t.beta = T(0);
    t.inp = inp;
    t.wts = wts;
    t.nin = nin;
    t.flush = 0;
    t.final = (k == 0 && !wp.padded) ? 1 : 0;  // padded rows: b_0 stays in B[0] and is copied out by the caller
    t.reverse = (opt.alternate_sweep && (k & 1)) ? 1 : 0;
    return launch_step_tile<T>(g, opt, t, wp.ldw, st);
  }
  a.nf = 1;
  a.nin = nin;
  a.racc = const_cast<T*>(inp);
  a.wts = wts;
  a.final = (k == 0) ? 1 : 0;
  a.flush = 0;
  if (k == K) {  // b_K = u_K : no product needed (scale 0 on any valid panel)
    a.cur = first;
    a.old = first;
    a.out = B[k & 1];
    a.scale = T(0);
    a.gamma = T(0);
  } else {
    a.cur = B[(k + 1) & 1];
    a.out = B[k & 1];
    a.old = has_b2 ? B[k & 1] : a.cur;
    a.gamma = has_b2 ? T(-1) : T(0);
    a.scale = (k == 0) ? T(0.5) : T(1);
  }
  a.reverse = (opt.alternate_sweep && (k & 1)) ? 1 : 0;
  launch_step<T>(ctx, a, shape, opt, st, g->coff.as<unsigned>());
  return GSPX_OK;
}

// ------------------------------------------------------------------------------------------------
// Synthesis  out = sum_f p_f(L) s_f  (filter.py:313-322) by a vector-coefficient Clenshaw
// recurrence.  By linearity  sum_f sum_k c'_fk T_k(Lt) s_f = sum_k T_k(Lt) u_k  with
// u_k = sum_f c'_fk s_f, and Clenshaw evaluates that with ONE recurrence:
//     b_K = u_K,   b_k = u_k + F b_{k+1} - b_{k+2}  (k = K-1..1),   out = u_0 + (F/2) b_1 - b_2
// K sparse products instead of the reference's K*Nf (it runs cheby_op once per filter); each
// step reads the Nf input panels at its own row, (Nf+3) panel passes per order instead of
// Nf*(3 2/3).  Same polynomial, different summation order: agrees to rounding.
// ------------------------------------------------------------------------------------------------
template <typename T>
static int run_synthesis_batch(gspx_graph* g, int nf, int M, const std::vector<double>& cp,
                               const T* x, size_t plane_x, unsigned ldx, T* y, unsigned ldy,
                               unsigned ld, size_t& ev_idx) {
  gspx_ctx* ctx = g->ctx;
  Options opt = ctx->opt;
  hipStream_t st = ctx->stream;
  const int N = (int)g->N;
  const int K = M - 1;
  // (padded work panels as in run_batch; the tile launches span all nf input panels)
  const WorkPanels wp = work_panels<T>(g, opt, true, (size_t)nf, ld, y, ldy);
  const bool padded = wp.padded;
  const unsigned ldw = wp.ldw;
  const size_t U = (size_t)N * ldw;
  const Shape shape = choose_shape(opt, sizeof(T), ld, vec_cap(4, ldy, y));
  const int* perm = g->has_perm ? g->perm.as<int>() : nullptr;

  // weights [K+1][nf]: w[k][f] = c'_fk  (c'_f0 already halved)
  std::vector<T> hw((size_t)M * nf);
  for (int k = 0; k < M; ++k)
    for (int f = 0; f < nf; ++f) hw[(size_t)k * nf + f] = (T)cp[(size_t)f * M + k];
  CHK(ctx->ws_w.ensure(hw.size() * sizeof(T) + 64));
  HIPCHK(hipMemcpyAsync(ctx->ws_w.p, hw.data(), hw.size() * sizeof(T), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  CHK(ctx->ws_r.ensure((size_t)nf * U * sizeof(T) + 256));  // the nf input panels, internal order
  CHK(ctx->ws_t.ensure(2 * U * sizeof(T) + 256));
  T* S = ctx->ws_r.as<T>();
  T* B[2] = {ctx->ws_t.as<T>(), ctx->ws_t.as<T>() + U};

  hipEvent_t ev[4];
  CHK(batch_events(ctx, ev_idx, ev));
  for (int f = 0; f < nf; ++f) {
    const T* xf = x + (size_t)f * plane_x;
    if (padded) {
      const unsigned nbp = (unsigned)std::min<size_t>((U + 255) / 256, 65536);
      hipLaunchKernelGGL((k_permute_in_pad<T>), dim3(nbp), dim3(256), 0, st, xf, ldx, S + (size_t)f * U, ldw, ld, N, perm);
      continue;
    }
    launch_permute_in<T>(xf, ldx, S + (size_t)f * U, ld, N, perm, vec_cap(shape.vec, ldx, xf), st);
  }
  HIPCHK(hipEventRecord(ev[1], st));

  CHK(prepare_coff<T>(g, shape, ld, st));
  StepArgs<T> a = step_base<T>(g, ld, y, ldy);
  // (nf input panels: the buffer window of the tile kernel spans all of them)
  for (int k = K; k >= 0; --k)
    CHK(clenshaw_step<T>(g, opt, wp, shape, a, k, K, S, ctx->ws_w.as<T>() + (size_t)k * nf, nf, S, B, y, ldy, st));
  HIPCHK(hipEventRecord(ev[2], st));
  if (padded) {
    const unsigned nbp = (unsigned)std::min<size_t>(((size_t)N * ld + 255) / 256, 65536);
    hipLaunchKernelGGL((k_permute_out_pad<T>), dim3(nbp), dim3(256), 0, st, B[0], ldw, y, ldy, ld, N, perm);
  }
  HIPCHK(hipEventRecord(ev[3], st));
  HIPCHK(hipGetLastError());
  return GSPX_OK;
}

// ------------------------------------------------------------------------------------------------
// Newton-form evaluation of the SAME polynomial (single filter, analysis):
//     p(Lt) x = sum_j d_j prod_{i<j} (Lt - r_i I) x,   Lt = (L - a2 I)/a1 = F/2
// by Horner:  h_K = d_K x,  h_j = (Lt - r_j I) h_{j+1} + d_j x,  y = h_0.
// A two-term recurrence: per order it gathers h, reads x and writes h (3 panels) and needs NO
// accumulator, where the three-term Chebyshev recurrence moves 3 + 2/3.  Nodes (Leja-ordered
// Chebyshev points) and divided differences are computed by the caller in exact arithmetic from
// the reference's Chebyshev coefficients (pygsp_amd/filters.py::cheb_to_newton), so the polynomial
// is identical; results agree with the reference to ~1e-14 (fp64).
// ------------------------------------------------------------------------------------------------
// A polynomial PROGRAM on one batch of columns: h_0 = x (copied into the internal order), then S steps
//     h_{s+1} = scale_s * (F h_s) + beta_s * h_s + gamma_s * o_s,
// o_s = x for every step (old_is_x: the Newton form's Horner recurrence) or o_s = h_{s-1} (the product form's quadratic
// factors; h_{s+1} then overwrites h_{s-1} in place, as the three-term recurrence does); the last step stores y.
// F = (2/a1)(L - a2 I) has its spectrum in [-2, 2]: a factor (t - r) of a polynomial in t = F/2 is scale 1/2, beta -r.
// A step whose gamma is 0 reads no third panel at all: gather h_s, write h_{s+1} - two panel passes.
template <typename T>
static int run_program_batch(gspx_graph* g, int S, const double* sc, const double* be, const double* ga, bool old_is_x,
                             const T* x, unsigned ldx, T* y, unsigned ldy, unsigned ld, size_t& ev_idx) {
  gspx_ctx* ctx = g->ctx;
  Options opt = ctx->opt;
  hipStream_t st = ctx->stream;
  const int N = (int)g->N;
  const size_t U = (size_t)N * ld;
  const Shape shape = choose_shape(opt, sizeof(T), ld, vec_cap(4, ldy, y));
  const int* perm = g->has_perm ? g->perm.as<int>() : nullptr;

  const T hw[3] = {T(1), T(0), T(0)};  // final step of the plain kernels: y = 1 * h
  CHK(ctx->ws_w.ensure(sizeof(hw) + 64));
  HIPCHK(hipMemcpyAsync(ctx->ws_w.p, hw, sizeof(hw), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  // panels: X (h_0; kept for the whole call when every step reads it) and one or two more
  CHK(ctx->ws_t.ensure((old_is_x ? 3 : 2) * U * sizeof(T) + 256));
  T* X = ctx->ws_t.as<T>();
  T* H[2] = {X + U, old_is_x ? X + 2 * U : X};  // product form: ping-pong between the second panel and X itself

  hipEvent_t ev[4];
  CHK(batch_events(ctx, ev_idx, ev));
  launch_permute_in<T>(x, ldx, X, ld, N, perm, vec_cap(shape.vec, ldx, x), st);
  HIPCHK(hipEventRecord(ev[1], st));

  CHK(prepare_coff<T>(g, shape, ld, st));
  StepArgs<T> a = step_base<T>(g, ld, y, ldy);
  a.nf = 1;
  a.racc = H[0];  // never read (flush == 1) - any valid panel
  a.wts = ctx->ws_w.as<T>();
  const bool tile_ok = tile_usable<T>(g, opt, ld, y, ldy);
  for (int s = 0; s < S; ++s) {
    const bool last = s == S - 1;
    const T* cur = (s == 0) ? X : H[(s - 1) & 1];
    T* out = H[s & 1];
    // o_s: x, or h_{s-1} - which lives in the panel this step writes (s >= 1: H[(s - 2) & 1] == H[s & 1]; s == 0 has none)
    const T* old = old_is_x ? X : (const T*)out;
    const double gam = (!old_is_x && s == 0) ? 0.0 : ga[s];
    if (tile_ok) {
      TileArgs<T> t{};
      t.cur = cur;
      t.old = gam == 0.0 ? cur : old;
      t.out = out;
      t.racc = H[0];  // never read or written (flush == 0)
      t.y = y;
      t.ldy = ldy;
      t.perm = perm;
      t.scale = (T)sc[s];
      t.beta = (T)be[s];
      t.gamma = (T)gam;
      t.flush = 0;
      t.final = last ? 1 : 0;
      t.reverse = (opt.alternate_sweep && (s & 1)) ? 1 : 0;
      CHK(launch_step_tile<T>(g, opt, t, ld, st));
      continue;
    }
    a.cur = cur;
    a.old = gam == 0.0 ? cur : old;
    a.out = out;
    a.scale = (T)sc[s];
    a.beta = (T)be[s];
    a.gamma = (T)gam;
    a.flush = last ? 1 : 0;
    a.final = last ? 1 : 0;
    a.reverse = (opt.alternate_sweep && (s & 1)) ? 1 : 0;
    launch_step<T>(ctx, a, shape, opt, st, g->coff.as<unsigned>());
  }
  HIPCHK(hipEventRecord(ev[2], st));
  HIPCHK(hipEventRecord(ev[3], st));
  HIPCHK(hipGetLastError());
  return GSPX_OK;
}

template <typename T>
static int filter_dev_t(gspx_graph* g, double lmax, int Nf, int M, const double* coeffs,
                        int64_t Nsig, const T* x, T* y, int mode) {
  gspx_ctx* ctx = g->ctx;
  const Options& opt = ctx->opt;
  const int64_t N = g->N;
  for (int i = 0; i < 5; ++i) ctx->timing[i] = 0;
  ctx->step_kinds[0] = ctx->step_kinds[1] = 0;
  if (N == 0 || Nsig == 0) return GSPX_OK;
  CHK(ensure_factor<T>(g, lmax));
  std::vector<double> cp;
  halve_c0(Nf, M, coeffs, cp);

  // final-flush / combine stores use the panel's vector width on y rows of Nsig elements
  const int K = M - 1;
  const bool analysis = mode == GSPX_ANALYSIS;
  bool deferred = analysis && (opt.combine == 2 || (opt.combine == 0 && Nf >= 2));
  // workspace per signal: M kept panels (deferred combine) or two panels and Nf accumulators
  const size_t budget = (size_t)std::max<int64_t>(opt.ws_limit_mb, 1) << 20;
  if (deferred && (size_t)N * sizeof(T) * M * (size_t)std::min<int64_t>(Nsig, 4) > budget) deferred = false;
  int64_t max_ld = 0;
  CHK(batch_width(g, sizeof(T), deferred ? (size_t)M : (size_t)(2 + Nf), Nsig, &max_ld));

  // ---- hipGraph replay: an analysis call that repeats the previous one exactly (same graph, lmax,
  // coefficients, pointers, options) is recorded once and replayed as one graph launch - K + 1
  // kernel launches cost ~5 us each, which is the whole call on cache-resident graphs
  std::vector<unsigned char> key;
  const bool graph_mode =
      analysis && Nsig <= max_ld &&
      (opt.graph_launch == 1 || (opt.graph_launch == 2 && (size_t)N * Nsig * sizeof(T) <= ((size_t)32 << 20)));
  if (graph_mode) {
    auto put = [&](const void* p, size_t n) {
      const unsigned char* b = (const unsigned char*)p;
      key.insert(key.end(), b, b + n);
    };
    // the graph by birth number (a destroyed graph's address may be handed out again), every device
    // address the launches carry, the scalars and options they were shaped by
    put(&g->generation, sizeof(g->generation));
    const void* ptrs[] = {x, y, ctx->ws_t.p, ctx->ws_r.p, ctx->ws_w.p, g->coff.p, g->gt_hdr.p, g->gt_s1nat.p,
                          g->fval.p, g->perm.p};
    put(ptrs, sizeof(ptrs));
    put(&lmax, sizeof(lmax));
    put(&g->fval_lmax, sizeof(g->fval_lmax));
    put(&Nf, sizeof(Nf));
    put(&M, sizeof(M));
    put(&Nsig, sizeof(Nsig));
    put(cp.data(), cp.size() * sizeof(double));
    put(&opt, sizeof(opt));
    put(&g->gt_rows, sizeof(g->gt_rows));
    put(&g->gt_slow, sizeof(g->gt_slow));
    if (ctx->graph_exec && !key.empty() && ctx->graph_key == key) {
      HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
      HIPCHK(hipGraphLaunch(ctx->graph_exec, ctx->stream));
      HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      float gms = 0;
      HIPCHK(hipEventElapsedTime(&gms, ctx->ev[0], ctx->ev[1]));
      ctx->timing[0] = gms;
      ctx->timing[1] = gms;  // one graph: no per-phase split
      ctx->timing[2] = (double)K;
      ctx->step_kinds[0] = ctx->graph_kinds[0];  // no launch is issued: the counts of the recording
      ctx->step_kinds[1] = ctx->graph_kinds[1];
      return GSPX_OK;
    }
    if (!key.empty() && ctx->seen_key == key) {  // second identical call: record it
      if (ctx->graph_exec) {
        (void)hipGraphExecDestroy(ctx->graph_exec);
        ctx->graph_exec = nullptr;
      }
      hipGraph_t graph = nullptr;
      size_t dummy = 0;
      HIPCHK(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
      ctx->capturing = true;
      const int rc = run_batch<T>(g, Nf, M, cp, x, (unsigned)Nsig, y, (unsigned)Nsig, (unsigned)Nsig,
                                  deferred, false, true, dummy);
      ctx->capturing = false;
      const hipError_t ce = hipStreamEndCapture(ctx->stream, &graph);
      if (rc != GSPX_OK || ce != hipSuccess || !graph) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        ctx->seen_key.clear();  // fall through to the eager path below
      } else {
        const hipError_t ie = hipGraphInstantiate(&ctx->graph_exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ie == hipSuccess) {
          ctx->graph_key = key;
          ctx->graph_kinds[0] = ctx->step_kinds[0];
          ctx->graph_kinds[1] = ctx->step_kinds[1];
          return filter_dev_t<T>(g, lmax, Nf, M, coeffs, Nsig, x, y, mode);  // replays
        }
        ctx->graph_exec = nullptr;
        (void)hipGetLastError();
      }
    }
  }
  if (ctx->graph_exec && ctx->graph_key != key) replay_reset(ctx);
  ctx->seen_key = key;  // empty when graph mode is off

  const size_t plane_x = (size_t)N * Nsig;  // synthesis: x is [Nf][N][Nsig]
  return run_batches(g, Nsig, max_ld, K, [&](int64_t c0, unsigned ld, size_t& ev_idx) -> int {
    if (analysis)
      return run_batch<T>(g, Nf, M, cp, x + c0, (unsigned)Nsig, y + c0, (unsigned)Nsig, ld, deferred, false, true,
                          ev_idx);
    // out = sum_f p_f(L) s_f  (filter.py:317-321)
    if (opt.synthesis != 1)
      return run_synthesis_batch<T>(g, Nf, M, cp, x + c0, plane_x, (unsigned)Nsig, y + c0, (unsigned)Nsig, ld, ev_idx);
    // the reference's scheme: one single-filter recurrence per feature, accumulated on
    // device; only the last one writes y (K*Nf sparse products)
    for (int f = 0; f < Nf; ++f) {
      std::vector<double> cf(cp.begin() + (size_t)f * M, cp.begin() + (size_t)(f + 1) * M);
      CHK(run_batch<T>(g, 1, M, cf, x + (size_t)f * plane_x + c0, (unsigned)Nsig, y + c0, (unsigned)Nsig, ld, false,
                       f > 0, f == Nf - 1, ev_idx));
    }
    return GSPX_OK;
  });
}

template <typename T>
static int program_dev_t(gspx_graph* g, double lmax, int S, const double* sc, const double* be, const double* ga,
                         bool old_is_x, int64_t Nsig, const T* x, T* y) {
  gspx_ctx* ctx = g->ctx;
  replay_reset(ctx);  // (a program rewrites the weights and panels a recorded filter call replays from)
  for (int i = 0; i < 5; ++i) ctx->timing[i] = 0;
  ctx->step_kinds[0] = ctx->step_kinds[1] = 0;
  if (g->N == 0 || Nsig == 0) return GSPX_OK;
  CHK(ensure_factor<T>(g, lmax));
  int64_t max_ld = 0;
  CHK(batch_width(g, sizeof(T), 3, Nsig, &max_ld));
  CHK(run_batches(g, Nsig, max_ld, S, [&](int64_t c0, unsigned ld, size_t& ev_idx) {
    return run_program_batch<T>(g, S, sc, be, ga, old_is_x, x + c0, (unsigned)Nsig, y + c0, (unsigned)Nsig, ld, ev_idx);
  }));
  ctx->timing[4] = 0;  // no combine: the last step stores y
  return GSPX_OK;
}

// the Newton form p(t) = sum_j d_j prod_{i<j} (t - r_i) by Horner, as a program with o_s = x (old_is_x):
// h <- (t - r_j) h + d_j x, j = K-1 .. 0
static void horner_program(int K, const double* nodes, const double* dc, std::vector<double>& sc,
                           std::vector<double>& be, std::vector<double>& ga) {
  sc.assign((size_t)K, 0.0);
  be.assign((size_t)K, 0.0);
  ga.assign((size_t)K, 0.0);
  for (int s = 0; s < K; ++s) {
    const int j = K - 1 - s;
    if (s == 0) {  // h_1 = d_K (t - r_{K-1}) x + d_{K-1} x
      sc[0] = 0.5 * dc[K];
      be[0] = 0.0;
      ga[0] = dc[j] - dc[K] * nodes[j];
    } else {
      sc[(size_t)s] = 0.5;
      be[(size_t)s] = -nodes[j];
      ga[(size_t)s] = dc[j];
    }
  }
}

// a device call on the graph's element type: run(x, y, Nsig) with x, y typed; kernel_ms: its device time
template <typename Run>
static int device_call(gspx_graph* g, int64_t Nsig, const void* x, void* y, double* kernel_ms, const Run& run) {
  HIPCHK(hipSetDevice(g->ctx->device));
  const int rc = g->dtype == GSPX_F32 ? run((const float*)x, (float*)y, Nsig) : run((const double*)x, (double*)y, Nsig);
  if (rc == GSPX_OK && kernel_ms) *kernel_ms = g->ctx->timing[0];
  return rc;
}

static int check_program_args(gspx_graph* g, double lmax, int S, const double* scale, const double* beta,
                              const double* gamma, int64_t Nsig, const void* x, void* y) {
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (S < 1) return set_err(GSPX_ERR_COEFF, "The coefficients have an invalid shape");
  if (!scale || !beta || !gamma) return set_err(GSPX_ERR_INVALID, "null program");
  if (Nsig < 0) return set_err(GSPX_ERR_INVALID, "negative number of signals");
  if (!(lmax > 0.0) || !std::isfinite(lmax))
    return set_err(GSPX_ERR_INVALID, "lmax must be positive and finite (got %g)", lmax);
  if (Nsig > 0 && g->N > 0 && (!x || !y)) return set_err(GSPX_ERR_INVALID, "null signal pointer");
  for (int i = 0; i < S; ++i)
    if (!std::isfinite(scale[i]) || !std::isfinite(beta[i]) || !std::isfinite(gamma[i]))
      return set_err(GSPX_ERR_INVALID, "non-finite program coefficient");
  if (Nsig >= ((int64_t)1 << 31) / 16) return set_err(GSPX_ERR_INVALID, "too many signals");
  return GSPX_OK;
}

// A polynomial of the scaled operator t = (2 / lmax) L - I evaluated as a PROGRAM of S steps on device panels
// (see run_program_batch): h_0 = x; h_{s+1} = scale_s (2 t) h_s + beta_s h_s + gamma_s o_s; y = h_S.  old_is_x != 0: o_s = x
// (the Newton form); 0: o_s = h_{s-1}, gamma_0 ignored (the PRODUCT form: a real root r of the polynomial is one step
// with scale sigma / 2, beta -sigma r, gamma 0 - two panel passes -, a conjugate pair a +- ib two steps, the second with
// gamma sigma^2 b^2 - three passes).  pygsp_amd.filters.cheb_to_product builds such programs from Chebyshev coefficients.
extern "C" int gspx_poly_program_dev(gspx_graph* g, double lmax, int S, const double* scale, const double* beta,
                                     const double* gamma, int old_is_x, int64_t Nsig, const void* x_dev, void* y_dev,
                                     double* kernel_ms) {
  if (g) replay_reset(g->ctx);
  CHK(check_program_args(g, lmax, S, scale, beta, gamma, Nsig, x_dev, y_dev));
  return device_call(g, Nsig, x_dev, y_dev, kernel_ms, [&](auto x, auto y, int64_t n) {
    return program_dev_t(g, lmax, S, scale, beta, gamma, old_is_x != 0, n, x, y);
  });
}

static int check_newton_args(gspx_graph* g, double lmax, int K, const double* nodes, const double* dcoef,
                             int64_t Nsig, const void* x, void* y) {
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (K < 1) return set_err(GSPX_ERR_COEFF, "The coefficients have an invalid shape");
  if (!nodes || !dcoef) return set_err(GSPX_ERR_INVALID, "null nodes / coefficients");
  if (Nsig < 0) return set_err(GSPX_ERR_INVALID, "negative number of signals");
  if (!(lmax > 0.0) || !std::isfinite(lmax))
    return set_err(GSPX_ERR_INVALID, "lmax must be positive and finite (got %g)", lmax);
  if (Nsig > 0 && g->N > 0 && (!x || !y))
    return set_err(GSPX_ERR_INVALID, "null signal pointer");
  for (int i = 0; i < K; ++i)
    if (!std::isfinite(nodes[i])) return set_err(GSPX_ERR_INVALID, "non-finite node");
  for (int i = 0; i <= K; ++i)
    if (!std::isfinite(dcoef[i])) return set_err(GSPX_ERR_INVALID, "non-finite coefficient");
  if (Nsig >= ((int64_t)1 << 31) / 16) return set_err(GSPX_ERR_INVALID, "too many signals");
  return GSPX_OK;
}

extern "C" int gspx_newton_filter_dev(gspx_graph* g, double lmax, int K, const double* nodes,
                                      const double* dcoef, int64_t Nsig, const void* x_dev,
                                      void* y_dev, double* kernel_ms) {
  if (g) replay_reset(g->ctx);
  CHK(check_newton_args(g, lmax, K, nodes, dcoef, Nsig, x_dev, y_dev));
  std::vector<double> sc, be, ga;
  horner_program(K, nodes, dcoef, sc, be, ga);
  return device_call(g, Nsig, x_dev, y_dev, kernel_ms, [&](auto x, auto y, int64_t n) {
    return program_dev_t(g, lmax, K, sc.data(), be.data(), ga.data(), true, n, x, y);
  });
}

// What the host-array entry points share, after the checks the caller makes up front.  An empty call does nothing;
// `prepare` (the checks that come after the empty-call test, and any setup) runs next.  A large call is pipelined in
// column batches (gspx_hostpipe.hip.h); any other - or one the pipeline steps aside for - is one copy in through io_x,
// run(x, y, Nsig) on the device copies, one copy out through io_y.  x / y hold in_planes / out_planes [N][Nsig] planes.
template <typename Prepare, typename Run>
static int host_call(gspx_graph* g, int64_t Nsig, int in_planes, int out_planes, const void* x_host, void* y_host,
                     double* kernel_ms, const Prepare& prepare, const Run& run) {
  gspx_ctx* ctx = g->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  if (g->N == 0 || Nsig <= 0) {
    if (kernel_ms) *kernel_ms = 0;
    return GSPX_OK;
  }
  CHK(prepare());
  const size_t e = elt_size(g->dtype);
  std::vector<int64_t> widths;
  int threads = 1;
  host_pipeline_shape(ctx->opt, e, g->N, Nsig, in_planes + out_planes, &widths, &threads);
  if (widths.size() >= 2) {
    if (!ctx->pipe) ctx->pipe = new HostPipe();
    replay_reset(ctx);
    const int rc = g->dtype == GSPX_F32
                       ? filter_host_pipelined<float>(g, Nsig, in_planes, out_planes, (const float*)x_host,
                                                      (float*)y_host, widths, threads, kernel_ms, run)
                       : filter_host_pipelined<double>(g, Nsig, in_planes, out_planes, (const double*)x_host,
                                                       (double*)y_host, widths, threads, kernel_ms, run);
    if (rc != GSPX_HOSTPIPE_UNAVAILABLE) return rc;
    // an in-place call, or no pinned / device staging memory to be had: the one-shot form below
  }
  if (ctx->pipe) {  // this host call is not pipelined: no stage times, no timeline of an earlier call
    ctx->pipe->timing[6] = 0;
    ctx->pipe->timeline.clear();
  }
  const size_t n_in = (size_t)in_planes * g->N * Nsig * e, n_out = (size_t)out_planes * g->N * Nsig * e;
  CHK(ctx->io_x.ensure(n_in));
  CHK(ctx->io_y.ensure(n_out));
  HIPCHK(hipMemcpyAsync(ctx->io_x.p, x_host, n_in, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  CHK(device_call(g, Nsig, ctx->io_x.p, ctx->io_y.p, kernel_ms, run));
  HIPCHK(hipMemcpyAsync(y_host, ctx->io_y.p, n_out, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return GSPX_OK;
}

// gspx_newton_filter_dev with host arrays
extern "C" int gspx_newton_filter(gspx_graph* g, double lmax, int K, const double* nodes,
                                  const double* dcoef, int64_t Nsig, const void* x_host,
                                  void* y_host, double* kernel_ms) {
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (Nsig > 0 && g->N > 0 && (!x_host || !y_host))
    return set_err(GSPX_ERR_INVALID, "null signal pointer");
  if (K < 1) return set_err(GSPX_ERR_COEFF, "The coefficients have an invalid shape");
  std::vector<double> sc, be, ga;
  auto prepare = [&]() -> int {
    CHK(check_newton_args(g, lmax, K, nodes, dcoef, Nsig, x_host, y_host));
    horner_program(K, nodes, dcoef, sc, be, ga);
    return GSPX_OK;
  };
  return host_call(g, Nsig, 1, 1, x_host, y_host, kernel_ms, prepare, [&](auto x, auto y, int64_t n) {
    return program_dev_t(g, lmax, K, sc.data(), be.data(), ga.data(), true, n, x, y);
  });
}

static int check_filter_args(gspx_graph* g, double lmax, int Nf, int M, const double* coeffs,
                             int64_t Nsig, const void* x, void* y, int mode) {
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (M < 2) return set_err(GSPX_ERR_COEFF, "The coefficients have an invalid shape");
  if (Nf < 1) return set_err(GSPX_ERR_INVALID, "Nf must be >= 1");
  if (!coeffs) return set_err(GSPX_ERR_INVALID, "null coefficients");
  if (Nsig < 0) return set_err(GSPX_ERR_INVALID, "negative number of signals");
  if (mode != GSPX_ANALYSIS && mode != GSPX_SYNTHESIS)
    return set_err(GSPX_ERR_INVALID, "unknown mode %d", mode);
  if (!(lmax > 0.0) || !std::isfinite(lmax))
    return set_err(GSPX_ERR_INVALID, "lmax must be positive and finite (got %g)", lmax);
  if (Nsig > 0 && g->N > 0 && (!x || !y)) return set_err(GSPX_ERR_INVALID, "null signal pointer");
  for (int64_t i = 0; i < (int64_t)Nf * M; ++i)
    if (!std::isfinite(coeffs[i])) return set_err(GSPX_ERR_INVALID, "non-finite coefficient");
  if (Nsig >= ((int64_t)1 << 31) / 16) return set_err(GSPX_ERR_INVALID, "too many signals");
  return GSPX_OK;
}

extern "C" int gspx_cheby_filter_dev(gspx_graph* g, double lmax, int Nf, int M,
                                     const double* coeffs, int64_t Nsig, const void* x_dev,
                                     void* y_dev, int mode, double* kernel_ms) {
  CHK(check_filter_args(g, lmax, Nf, M, coeffs, Nsig, x_dev, y_dev, mode));
  return device_call(g, Nsig, x_dev, y_dev, kernel_ms, [&](auto x, auto y, int64_t n) {
    return filter_dev_t(g, lmax, Nf, M, coeffs, n, x, y, mode);
  });
}

extern "C" int gspx_cheby_filter(gspx_graph* g, double lmax, int Nf, int M, const double* coeffs,
                                 int64_t Nsig, const void* x_host, void* y_host, int mode,
                                 double* kernel_ms) {
  CHK(check_filter_args(g, lmax, Nf, M, coeffs, Nsig, x_host, y_host, mode));
  const bool analysis = mode == GSPX_ANALYSIS;
  return host_call(g, Nsig, analysis ? 1 : Nf, analysis ? Nf : 1, x_host, y_host, kernel_ms,
                   [] { return (int)GSPX_OK; }, [&](auto x, auto y, int64_t n) {
                     return filter_dev_t(g, lmax, Nf, M, coeffs, n, x, y, mode);
                   });
}

// ------------------------------------------------------------------------------------------------
// Squared column norms of a filterbank applied to device signals (features.compute_norm_tig / compute_spectrogram):
// the deferred plan for every Nf, Nf = 1 included, and per column batch k_combine_sqnorm over the kept slots in place
// of k_combine.  Nothing of size Nf x N x w exists: the workspaces are the M slots, the coefficient table, the Nf x Nsig
// norms and the workgroup partials.  out: HOST, Nf x Nsig.
// ------------------------------------------------------------------------------------------------
template <typename T>
static int sqnorms_dev_t(gspx_graph* g, double lmax, int Nf, int M, const double* coeffs, int64_t Nsig, const T* x,
                         double* out) {
  gspx_ctx* ctx = g->ctx;
  const int64_t N = g->N;
  for (int i = 0; i < 5; ++i) ctx->timing[i] = 0;
  ctx->step_kinds[0] = ctx->step_kinds[1] = 0;
  if (Nsig == 0) return GSPX_OK;
  if (N == 0) {
    std::fill(out, out + (size_t)Nf * Nsig, 0.0);
    return GSPX_OK;
  }
  int64_t width = 0;
  CHK(batch_width(g, sizeof(T), (size_t)M, Nsig, &width));
  std::vector<double> cp;
  halve_c0(Nf, M, coeffs, cp);
  const int ldc = (Nf + SQ_PASS - 1) / SQ_PASS * SQ_PASS;  // [k][ldc], zero beyond Nf: a pass never reads past it
  std::vector<double> hc((size_t)M * ldc, 0.0);
  for (int f = 0; f < Nf; ++f)
    for (int k = 0; k < M; ++k) hc[(size_t)k * ldc + f] = cp[(size_t)f * M + k];
  const size_t cbytes = (hc.size() * sizeof(double) + 255) / 256 * 256, obytes = (size_t)Nf * Nsig * sizeof(double);
  const int64_t first = std::min<int64_t>(width, Nsig), last = Nsig - (Nsig - 1) / width * width;
  const size_t parts = std::max(sqnorm_parts(ctx, (int)N, (unsigned)first), sqnorm_parts(ctx, (int)N, (unsigned)last));
  CHK(ctx->ws_sq.ensure(cbytes + obytes + 256));
  CHK(ctx->ws_sqp.ensure(parts * sizeof(double) + 256));
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(ctx->ws_sq.p, hc.data(), hc.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));  // hc is a stack-owned staging buffer
  CHK(ensure_factor<T>(g, lmax));
  double* outd = (double*)((char*)ctx->ws_sq.p + cbytes);
  const SqNorms sq{ctx->ws_sq.as<double>(), ldc, Nf, outd, (size_t)Nsig, ctx->ws_sqp.as<double>()};
  CHK(run_batches(g, Nsig, width, M - 1, [&](int64_t c0, unsigned ld, size_t& ev_idx) -> int {
    SqNorms b = sq;
    b.out = outd + c0;
    return run_batch<T>(g, Nf, M, cp, x + c0, (unsigned)Nsig, (T*)nullptr, ld, ld, true, false, false, ev_idx, &b);
  }));
  HIPCHK(hipMemcpyAsync(out, outd, obytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return GSPX_OK;
}

extern "C" int gspx_cheby_sqnorms_dev(gspx_graph* g, double lmax, int Nf, int M, const double* coeffs, int64_t Nsig,
                                      const void* x_dev, double* out, double* kernel_ms) {
  if (g) replay_reset(g->ctx);
  CHK(check_filter_args(g, lmax, Nf, M, coeffs, Nsig, x_dev, out, GSPX_ANALYSIS));
  if (M > 256) return set_err(GSPX_ERR_INVALID, "gspx_cheby_sqnorms_dev: at most 256 coefficients per filter");
  if (Nsig > 0 && !out) return set_err(GSPX_ERR_INVALID, "gspx_cheby_sqnorms_dev: null output");
  return device_call(g, Nsig, x_dev, out, kernel_ms, [&](auto x, auto, int64_t n) {
    return sqnorms_dev_t(g, lmax, Nf, M, coeffs, n, x, out);
  });
}

// ------------------------------------------------------------------------------------------------
// Chebyshev self-moments of device signals (pygsp_amd.spectrum: density of states, eigenvalue counts):
//     out[k][j] = x_j^T T_k(Lt) x_j,  k < M.
// L is symmetric, so T_i T_j = (T_{i+j} + T_{|i-j|}) / 2 gives  m_{2i} = 2 <T_i, T_i> - m_0  and
// m_{2i+1} = 2 <T_{i+1}, T_i> - m_1:  S = M / 2 + 1 kept slots, S - 1 recurrence steps instead of M - 1.  Per column
// batch the deferred plan of ONE filter with S slots, then k_slot_dots over the kept slots in place of k_combine; the
// 2 S - 1 dot rows come back in one download and the doubling is fp64 host arithmetic.  out: HOST, M x Nsig.
// ------------------------------------------------------------------------------------------------
template <typename T>
static int moments_dev_t(gspx_graph* g, double lmax, int M, int64_t Nsig, const T* x, double* out) {
  gspx_ctx* ctx = g->ctx;
  const int64_t N = g->N;
  for (int i = 0; i < 5; ++i) ctx->timing[i] = 0;
  ctx->step_kinds[0] = ctx->step_kinds[1] = 0;
  if (Nsig == 0) return GSPX_OK;
  if (N == 0) {
    std::fill(out, out + (size_t)M * Nsig, 0.0);
    return GSPX_OK;
  }
  const int S = M / 2 + 1, rows = 2 * S - 1;
  int64_t width = 0;
  CHK(batch_width(g, sizeof(T), (size_t)S, Nsig, &width));
  const std::vector<double> cp((size_t)S, 0.0);  // (the deferred plan uploads its filter's coefficients; none are read)
  const size_t obytes = (size_t)rows * Nsig * sizeof(double);
  const int64_t first = std::min<int64_t>(width, Nsig), last = Nsig - (Nsig - 1) / width * width;
  const size_t parts =
      std::max(dots_parts(ctx, (int)N, (unsigned)first, S), dots_parts(ctx, (int)N, (unsigned)last, S));
  CHK(ctx->ws_sq.ensure(obytes + 256));
  CHK(ctx->ws_sqp.ensure(parts * sizeof(double) + 256));
  hipStream_t st = ctx->stream;
  CHK(ensure_factor<T>(g, lmax));
  double* outd = ctx->ws_sq.as<double>();
  CHK(run_batches(g, Nsig, width, S - 1, [&](int64_t c0, unsigned ld, size_t& ev_idx) -> int {
    const SlotDots b{outd + c0, (size_t)Nsig, ctx->ws_sqp.as<double>()};
    return run_batch<T>(g, 1, S, cp, x + c0, (unsigned)Nsig, (T*)nullptr, ld, ld, true, false, false, ev_idx, nullptr,
                        &b);
  }));
  std::vector<double> d((size_t)rows * Nsig);
  HIPCHK(hipMemcpyAsync(d.data(), outd, obytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const double *a = d.data(), *b = d.data() + (size_t)S * Nsig;  // a_i = <T_i, T_i>, b_i = <T_{i+1}, T_i>
  for (int k = 0; k < M; ++k)
    for (int64_t j = 0; j < Nsig; ++j) {
      const double dot = (k & 1 ? b : a)[(size_t)(k / 2) * Nsig + j];
      out[(size_t)k * Nsig + j] = k < 2 ? dot : 2.0 * dot - (k & 1 ? b : a)[j];
    }
  return GSPX_OK;
}

extern "C" int gspx_cheby_moments_dev(gspx_graph* g, double lmax, int M, int64_t Nsig, const void* x_dev, double* out,
                                      double* kernel_ms) {
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (M < 2 || M > 2048) return set_err(GSPX_ERR_INVALID, "gspx_cheby_moments_dev: 2 to 2048 moments (got %d)", M);
  if (Nsig < 0) return set_err(GSPX_ERR_INVALID, "negative number of signals");
  if (!(lmax > 0.0) || !std::isfinite(lmax))
    return set_err(GSPX_ERR_INVALID, "lmax must be positive and finite (got %g)", lmax);
  if (Nsig > 0 && (!out || (g->N > 0 && !x_dev))) return set_err(GSPX_ERR_INVALID, "null signal pointer");
  if (Nsig >= ((int64_t)1 << 31) / 16) return set_err(GSPX_ERR_INVALID, "too many signals");
  replay_reset(g->ctx);  // (the kept slots overwrite the panels a recorded filter call replays from)
  return device_call(g, Nsig, x_dev, out, kernel_ms, [&](auto x, auto, int64_t n) {
    return moments_dev_t(g, lmax, M, n, x, out);
  });
}

// ------------------------------------------------------------------------------------------------
// Chebyshev cross-moments of device signals (the coefficient gradient of filters.cheby_op_vjp):
//     out[f][k][j] = sum_n z[f][n][j] (T_k(Lt) x)[n][j],  k < M.
// Per column batch the deferred plan of ONE filter with M kept slots - M - 1 plain recurrence steps; z is foreign, so
// the doubling of the self-moments does not apply - then k_slot_cross_dots over the kept slots in place of k_combine,
// CROSS_PASS planes per pass.  The workspaces are the M slots, the Nf x M x Nsig result and the workgroup partials.
// out: HOST, Nf x M x Nsig.
// ------------------------------------------------------------------------------------------------
template <typename T>
static int cross_moments_dev_t(gspx_graph* g, double lmax, int M, int64_t Nsig, const T* x, int Nf, const T* z,
                               double* out) {
  gspx_ctx* ctx = g->ctx;
  const int64_t N = g->N;
  for (int i = 0; i < 5; ++i) ctx->timing[i] = 0;
  ctx->step_kinds[0] = ctx->step_kinds[1] = 0;
  if (Nsig == 0) return GSPX_OK;
  if (N == 0) {
    std::fill(out, out + (size_t)Nf * M * Nsig, 0.0);
    return GSPX_OK;
  }
  int64_t width = 0;
  CHK(batch_width(g, sizeof(T), (size_t)M, Nsig, &width));
  const std::vector<double> cp((size_t)M, 0.0);  // (the deferred plan uploads its filter's coefficients; none are read)
  const size_t obytes = (size_t)Nf * M * Nsig * sizeof(double);
  const int64_t first = std::min<int64_t>(width, Nsig), last = Nsig - (Nsig - 1) / width * width;
  const size_t parts =
      std::max(cross_parts(ctx, (int)N, (unsigned)first, M, Nf), cross_parts(ctx, (int)N, (unsigned)last, M, Nf));
  CHK(ctx->ws_sq.ensure(obytes + 256));
  CHK(ctx->ws_sqp.ensure(parts * sizeof(double) + 256));
  hipStream_t st = ctx->stream;
  CHK(ensure_factor<T>(g, lmax));
  double* outd = ctx->ws_sq.as<double>();
  CHK(run_batches(g, Nsig, width, M - 1, [&](int64_t c0, unsigned ld, size_t& ev_idx) -> int {
    const CrossDots b{z + c0, (unsigned)Nsig, (size_t)N * (size_t)Nsig, Nf, outd + c0, (size_t)Nsig,
                      ctx->ws_sqp.as<double>()};
    return run_batch<T>(g, 1, M, cp, x + c0, (unsigned)Nsig, (T*)nullptr, ld, ld, true, false, false, ev_idx, nullptr,
                        nullptr, &b);
  }));
  HIPCHK(hipMemcpyAsync(out, outd, obytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return GSPX_OK;
}

extern "C" int gspx_cheby_cross_moments_dev(gspx_graph* g, double lmax, int M, int64_t Nsig, const void* x_dev, int Nf,
                                            const void* z_dev, double* out, double* kernel_ms) {
  // (the scalar checks first: they need no graph, and so no device, to be exercised)
  if (M < 2 || M > 256)
    return set_err(GSPX_ERR_INVALID, "gspx_cheby_cross_moments_dev: 2 to 256 orders (got %d)", M);
  if (Nf < 1) return set_err(GSPX_ERR_INVALID, "Nf must be >= 1");
  if (Nsig < 0) return set_err(GSPX_ERR_INVALID, "negative number of signals");
  if (!(lmax > 0.0) || !std::isfinite(lmax))
    return set_err(GSPX_ERR_INVALID, "lmax must be positive and finite (got %g)", lmax);
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (Nsig > 0 && (!out || (g->N > 0 && (!x_dev || !z_dev)))) return set_err(GSPX_ERR_INVALID, "null signal pointer");
  if (Nsig >= ((int64_t)1 << 31) / 16) return set_err(GSPX_ERR_INVALID, "too many signals");
  replay_reset(g->ctx);  // (the kept slots overwrite the panels a recorded filter call replays from)
  return device_call(g, Nsig, x_dev, out, kernel_ms, [&](auto x, auto, int64_t n) {
    return cross_moments_dev_t(g, lmax, M, n, x, Nf, (decltype(x))z_dev, out);
  });
}

// gspx_poly_program_dev with host arrays
extern "C" int gspx_poly_program(gspx_graph* g, double lmax, int S, const double* scale, const double* beta,
                                 const double* gamma, int old_is_x, int64_t Nsig, const void* x_host, void* y_host,
                                 double* kernel_ms) {
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (Nsig > 0 && g->N > 0 && (!x_host || !y_host)) return set_err(GSPX_ERR_INVALID, "null signal pointer");
  if (S < 1) return set_err(GSPX_ERR_COEFF, "The coefficients have an invalid shape");
  auto prepare = [&] { return check_program_args(g, lmax, S, scale, beta, gamma, Nsig, x_host, y_host); };
  return host_call(g, Nsig, 1, 1, x_host, y_host, kernel_ms, prepare, [&](auto x, auto y, int64_t n) {
    return program_dev_t(g, lmax, S, scale, beta, gamma, old_is_x != 0, n, x, y);
  });
}
