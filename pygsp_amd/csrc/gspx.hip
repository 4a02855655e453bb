// gspx.hip - libgspx for MI355X / gfx950: the one translation unit behind the C-ABI of include/gspx.h and
// include/gspx_ext.h.  This file is the table of contents: the error state and the CHK / HIPCHK macros every header
// uses, then the subject headers in dependency order.  A header may use what the headers listed before it define and
// nothing below it.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC gspx.hip -o libgspx.so

// device code of the recurrence: step, combine and permute kernels, k_coff, k_fill | the LDS-staged step and its tile
// builders (on gspx_kernels.hip.h)
#include "gspx_kernels.hip.h"
#include "gspx_tile_kernels.hip.h"
// the inner products of kept slots: Chebyshev self-moments (on gspx_kernels.hip.h)
#include "gspx_moments.hip.h"
// (The kernels that measured slower than what runs by default - two recurrence orders per launch, the fused Newton
// pair, the small pair kernel, 128-row blocks - were retired in round 6; their counter-backed records are
// profiles/r04_pair_experiment.md, profiles/r05_pair_experiment.md and profiles/r05_narrow_rows.md.)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <numeric>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <sys/mman.h>

#include "../../include/gspx.h"
#include "../../include/gspx_ext.h"

using namespace gspx;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;

static int set_err(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return set_err(GSPX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                     __FILE__, __LINE__);                                                   \
  } while (0)

#define CHK(expr)               \
  do {                          \
    int rc_ = (expr);           \
    if (rc_ != GSPX_OK) return rc_; \
  } while (0)

extern "C" const char* gspx_last_error(void) { return g_err.c_str(); }
extern "C" const char* gspx_version(void) { return "gspx 0.1 (gfx950)"; }

#include "gspx_mem.hip.h"         // DevMem, PinMem, CopyStage, HostPipe                              (needs only the above)
#include "gspx_ctx.hip.h"         // Options and their table, the handles, contexts, buffers, timings (on mem)
#include "gspx_comm.hip.h"        // RCCL gather, gspx_comm_*, gspx_gather                            (on ctx)
#include "gspx_adjacency.hip.h"   // scan_exclusive, the gspx_knn handle of every device builder and its frame (on ctx)
#include "gspx_graph.hip.h"       // graph construction and its kernels, ensure_factor              (on ctx, adjacency)
#include "gspx_hostpipe.hip.h"    // host-pointer calls pipelined over column batches                 (on ctx)
#include "gspx_poly.hip.h"        // plans, launchers, batch runners, cheby / newton / program calls  (on graph, hostpipe)
#include "gspx_lmax.hip.h"        // lambda_max by Lanczos and its vector kernels                     (on poly)
#include "gspx_calib.hip.h"       // bandwidth / gather / mix calibrations, the placement tuner       (on poly)
#include "gspx_ops.hip.h"         // L x, Dirichlet energy, Tikhonov CG, grad / div, panel primitives; brings
                                  // gspx_reduce.hip.h and gspx_ops_kernels.hip.h                     (on poly)
#include "gspx_knn.hip.h"         // k-NN / radius graphs on the device; brings gspx_knn_bf.hip.h     (on adjacency)
#include "gspx_sbm.hip.h"         // stochastic block model / Erdos-Renyi sampler                     (on adjacency, knn's row sort)
#include "gspx_setup.hip.h"       // graph set-up in one call, curve keys and orders                  (on graph, adjacency)
#include "gspx_linegraph.hip.h"   // line graphs from the edge tables of grad / div                   (on ops, adjacency)
#include "gspx_schur.hip.h"       // Schur complements of L + shift I: schur_cg, Kron reduction     (on ops, adjacency)
#include "gspx_components.hip.h"  // connected components                                             (on graph)
#include "gspx_spectral.hip.h"    // panel Gram / combine / residual norms of the Fourier basis       (on ops)
#include "gspx_eig.hip.h"         // the full Fourier basis: dense symmetric eigensolver by block Jacobi   (on spectral)
#include "gspx_lanczos.hip.h"     // Lanczos filtering: Krylov stack and combine                      (on poly, ops)
#include "gspx_conv.hip.h"        // Chebyshev graph convolution: k_group_mix, k_slot_cross_gram      (on poly, ops)
#include "gspx_wgrad.hip.h"       // the filter's gradient in the Laplacian: k_pair_cross, k_row_cross (on poly, ops)
#include "gspx_fista.hip.h"       // the FISTA driver: stopping rule, argument check, host loop       (on ops)
#include "gspx_graphlearn.hip.h"  // graph learning: edge distances, the log-degree model, its adjacency (on ops, adjacency, fista)
#include "gspx_learning.hip.h"    // classification_tikhonov_simplex                                  (on ops, fista)
#include "gspx_optim.hip.h"       // prox_tv: the graph total-variation proximal operator             (on ops, fista)
#include "gspx_layout.hip.h"      // spring layout: all-pairs repulsion, attraction and update        (on ops)
#include "gspx_coarsen.hip.h"     // heavy-edge matching, coarse graphs, segment pooling and its vjp     (on graph, adjacency)
#include "gspx_cluster.hip.h"     // k-means: assignment, update, k-means++ seeding, row normalisation (on ops)
