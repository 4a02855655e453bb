// gspx_fista.hip.h - the fixed-step FISTA loop that the proximal solvers share (gspx_learning.hip.h's simplex
// classifier, gspx_optim.hip.h's total-variation prox; DESIGN.md section 10, "The shared FISTA driver").  A solver
// brings its step kernels and a thin rule kernel that says how its objective `cur` and its squared iterate distance
// `dx2` arise from the step kernels' partial sums; everything else about stopping is here, once.
//
// Device: the criterion codes and fista_rule; FistaState (done, crit, niter); fista_totals, the fixed-order sum of Q
// slabs of workgroup partials in a one-workgroup rule kernel; fista_judge, which records obj[it], applies the rule
// for it >= 1 and sets the state.  Once `done` is set every step and rule launch returns at once, so what the host
// launches past the stop changes nothing.
// Host: FistaTol (the five stopping parameters, also the rule kernels' argument); fista_check, the refusals every
// solver entry point makes, under the solver's name; FistaLoop, which owns the momentum sequence t_k, b_k (they do not
// depend on the data: b is a launch argument), the objective and state buffers, the poll of the done flag every
// FISTA_POLL iterations and the finish.  Each solver keeps its own loop bounds and says when it polls.
// After gspx_ops.hip.h (block_sums, finish_timed, DevMem).
#pragma once

namespace gspx {

constexpr int FISTA_POLL = 4;                      // the host looks at the done flag every FISTA_POLL iterations
constexpr long long FISTA_MAXIT_LIMIT = 10000000;  // (the objective sequence is a device array of maxit + 1 doubles)

enum { SPX_ATOL = 1, SPX_DTOL = 2, SPX_RTOL = 3, SPX_XTOL = 4, SPX_MAXIT = 5 };

struct FistaTol {  // a negative tolerance disables its criterion
  double rtol, atol, dtol, xtol;
  long long maxit;
};

struct FistaState {  // device resident, zeroed before the first launch
  int done;
  int crit;
  long long niter;
};

// The stopping rule for iteration it >= 1: the first criterion that holds, in this order, or 0.
// dx2 = ||X_it - X_{it-1}||_F^2, nc = the number of entries of X.
__device__ inline int fista_rule(double cur, double prev, double dx2, double nc, long long it, double rtol, double atol,
                                 double dtol, double xtol, long long maxit) {
  const double diff = fabs(cur - prev);
  double den = cur;
  if (den == 0) den = prev;
  if (den == 0) den = 1.0;
  if (atol >= 0 && cur < atol) return SPX_ATOL;
  if (dtol >= 0 && diff < dtol) return SPX_DTOL;
  if (rtol >= 0 && diff / den < rtol) return SPX_RTOL;
  if (xtol >= 0 && sqrt(dx2) / sqrt(nc) < xtol) return SPX_XTOL;
  if (it >= maxit) return SPX_MAXIT;
  return 0;
}

// tot[q] = sum over b < nb of partial[q * nb + b].  One workgroup of 256 threads, all of which call it: thread t sums
// entries t, t + 256, ... in order, block_sums combines the threads; tot (shared memory) is readable on return.
template <int Q>
__device__ inline void fista_totals(const double* __restrict__ partial, int nb, double* tot) {
  double v[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) v[q] = 0;
  for (int b = threadIdx.x; b < nb; b += 256) {
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] += partial[(size_t)q * nb + b];
  }
  block_sums<Q>(v, tot, 1);
  __syncthreads();
}

// One thread: obj[it] = cur, then the rule on iteration it >= 1.  True when it fired (crit, niter and done are set).
__device__ inline bool fista_judge(FistaState* s, double* __restrict__ obj, long long it, double cur, double dx2,
                                   double nc, const FistaTol& tol) {
  obj[it] = cur;
  if (it < 1) return false;
  const int crit = fista_rule(cur, obj[it - 1], dx2, nc, it, tol.rtol, tol.atol, tol.dtol, tol.xtol, tol.maxit);
  if (!crit) return false;
  s->crit = crit;
  s->niter = it;
  s->done = 1;
  return true;
}

}  // namespace gspx

using gspx::FistaState;
using gspx::FistaTol;

// The refusals of a solver entry point that do not depend on the solver, under its name `who`; its own parameter
// (tau, gamma) is checked before the call, its panel sizes after.  `width` is the column count of the panel, called
// `width_name` in the message.
static int fista_check(const char* who, gspx_graph* g, double step, const FistaTol& tol, const char* width_name,
                       long long width, int width_max, const void* in_dev, const void* out_dev, const int64_t* niter,
                       const int32_t* crit, const double* objective_host) {
  if (!(step > 0) || !std::isfinite(step)) return set_err(GSPX_ERR_INVALID, "%s: step must be positive and finite", who);
  if (tol.maxit < 1 || tol.maxit > gspx::FISTA_MAXIT_LIMIT)
    return set_err(GSPX_ERR_INVALID, "%s: maxit must be 1..%lld (got %lld)", who, gspx::FISTA_MAXIT_LIMIT, tol.maxit);
  if (width < 1 || width > width_max)
    return set_err(GSPX_ERR_INVALID, "%s: %s must be 1..%d (got %lld)", who, width_name, width_max, width);
  if (std::isnan(tol.rtol) || std::isnan(tol.atol) || std::isnan(tol.dtol) || std::isnan(tol.xtol))
    return set_err(GSPX_ERR_INVALID, "%s: a tolerance is NaN (a negative one disables its criterion)", who);
  if (!niter || !crit || !objective_host) return set_err(GSPX_ERR_INVALID, "%s: null host output", who);
  if (g) replay_reset(g->ctx);
  if (!g) return set_err(GSPX_ERR_INVALID, "null graph");
  if (g->N > 0 && (!in_dev || !out_dev)) return set_err(GSPX_ERR_INVALID, "%s: null device pointer", who);
  if (g->dtype != GSPX_F64)
    return set_err(GSPX_ERR_INVALID, "%s: the graph computes in float32; the solver needs the float64 graph", who);
  return GSPX_OK;
}

// an N x width fp64 panel that the 32-bit offsets of the panel kernels cannot address
static bool fista_panel_too_large(int64_t rows, int64_t width) {
  return (double)rows * width * sizeof(double) > (double)(((size_t)1 << 31) - 65536);
}

struct FistaLoop {
  gspx_ctx* ctx = nullptr;
  const char* who = nullptr;
  FistaTol tol{};
  DevMem obj, state;           // obj_0 .. obj_maxit | the solver's device state, which holds a FistaState
  size_t state_bytes = 0, flags_at = 0;
  FistaState* flags = nullptr;  // that FistaState
  double t = 1.0, b = 0.0;     // t_k, and the b_k the next step launch takes (b_0 = 0: the first point is X_0 itself)

  // the shared preamble of a solver, before its own allocations.  A solver whose device state is more than a
  // FistaState gives its size and where the FistaState sits in it.
  int init(gspx_graph* g, const char* name, const FistaTol& tl, size_t state_size = sizeof(FistaState),
           size_t flags_offset = 0) {
    ctx = g->ctx;
    who = name;
    tol = tl;
    state_bytes = state_size;
    flags_at = flags_offset;
    HIPCHK(hipSetDevice(ctx->device));
    return GSPX_OK;
  }
  // after the solver's allocations: the objective and state buffers, then the timed span opens and the state is zeroed
  int start() {
    CHK(obj.alloc((size_t)(tol.maxit + 1) * sizeof(double)));
    CHK(state.alloc(state_bytes));
    flags = (FistaState*)(state.as<char>() + flags_at);
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    HIPCHK(hipMemsetAsync(state.p, 0, state_bytes, ctx->stream));
    return GSPX_OK;
  }
  void advance() {  // t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2,  b_{k+1} = (t_k - 1) / t_{k+1}
    const double tn = (1.0 + std::sqrt(1.0 + 4.0 * t * t)) / 2.0;
    b = (t - 1.0) / tn;
    t = tn;
  }
  int poll(bool* done) {  // a 4-byte read of the flag and a sync
    int d = 0;
    HIPCHK(hipMemcpyAsync(&d, &flags->done, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *done = d != 0;
    return GSPX_OK;
  }
  // After the loop: reads the state (an error if the rule never fired), lets the solver queue the copy of its result
  // for iteration niter (copy_result(niter) -> status), copies obj_0 .. obj_niter to the host and closes the timed span.
  template <class CopyResult>
  int finish(CopyResult copy_result, double* objective, int64_t* niter, int32_t* crit, double* ms) {
    FistaState hs{};
    HIPCHK(hipMemcpyAsync(&hs, flags, sizeof(FistaState), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (!hs.done) return set_err(GSPX_ERR_HIP, "%s: the stopping rule did not fire", who);
    CHK(copy_result((int64_t)hs.niter));
    HIPCHK(hipMemcpyAsync(objective, obj.p, (size_t)(hs.niter + 1) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    CHK(finish_timed(ctx, ms));
    *niter = hs.niter;
    *crit = hs.crit;
    return GSPX_OK;
  }
};
