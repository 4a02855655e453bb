// gspx_components.hip.h - connected components of a gspx_graph, labelled on the device.  After gspx_graph.hip.h.
//
// What Graph.is_connected / Graph.extract_components of the reference (pygsp/graphs/graph.py:294-366, 444-508: a
// Python depth-first search that slices one sparse row per vertex) and scipy.sparse.csgraph.connected_components
// answer on the host, answered on the pattern that already lies on the device: the off-diagonal stored entries of
// the canonical Laplacian (lptr / lcol, caller's vertex order), read in both directions.  Nothing is uploaded, one
// int32 per vertex comes back.
//
// Algorithm: hook to the smaller label, then shorten pointers.  Two arrays of N int32: lab[v], the label of v, and
// par[r], the parent of label r.  Between rounds every tree is a star: lab[v] is a root (par[lab[v]] == lab[v]) and
// the smallest vertex of the set it names.  One round is
//   k_cc_hook      for every stored entry (u, v) with lab[u] != lab[v]: atomicMin(&par[larger label], smaller label) -
//                  afterwards every root points at the smallest label among itself and the roots its set touches;
//                  lab is only read and par only takes atomicMin, so the result does not depend on the schedule.
//                  Any such entry raises the `changed` flag, which the host reads once per round.
//   k_cc_shorten   every vertex follows par from its label to the new root (each step goes to a strictly smaller
//                  index, so a walk ends after fewer than N steps whatever other threads do) and stores it in lab;
//                  on the way par[x] = par[par[x]] halves the chain for everybody else (a stale or overwritten value
//                  is still an ancestor of x: any of them is correct).
// A round whose hook finds no entry between two labels ends the loop: every set is closed under the edges and is
// named by its smallest vertex.  Then roots are marked, an exclusive scan numbers them and k_cc_rename rewrites the
// labels to 0 .. C-1 in order of smallest vertex - the numbering of scipy's connected_components(W, directed=False).
#pragma once

namespace gspx {

__global__ __launch_bounds__(256) void k_cc_init(int* __restrict__ lab, int* __restrict__ par, int N) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v < N) {
    lab[v] = v;
    par[v] = v;
  }
}

__global__ __launch_bounds__(256) void k_cc_hook(const int* __restrict__ ptr, const int* __restrict__ col,
                                                 const int* __restrict__ lab, int* __restrict__ par, int N,
                                                 int* __restrict__ changed) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= N) return;
  const int lu = lab[u];
  int lowest = lu;
  bool crossing = false;
  for (int j = ptr[u], e = ptr[u + 1]; j < e; ++j) {
    const int v = col[j];
    if ((unsigned)v >= (unsigned)N) continue;  // (never in a validated CSR; keeps every access inside lab / par)
    const int lv = lab[v];
    if (lv == lu) continue;
    crossing = true;
    if (lv > lu) atomicMin(&par[lv], lu);  // the mirror entry may be absent (a Laplacian uploaded as it is)
    lowest = min(lowest, lv);
  }
  if (lowest < lu) atomicMin(&par[lu], lowest);
  if (crossing) *changed = 1;
}

__global__ __launch_bounds__(256) void k_cc_shorten(int* __restrict__ lab, int* __restrict__ par, int N) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= N) return;
  int x = lab[v];
  int p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (p != x) {  // p < x: every pass moves to a smaller index
    const int pp = __hip_atomic_load(&par[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (pp != p) __hip_atomic_store(&par[x], pp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = pp;
  }
  lab[v] = x;
}

// mark[v] = 1 where v names its own set, mark[N] = 0: the exclusive scan of mark numbers the sets, scan[N] counts them
__global__ __launch_bounds__(256) void k_cc_mark(const int* __restrict__ lab, int N, int* __restrict__ mark) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v <= N) mark[v] = v < N && lab[v] == v;
}

__global__ __launch_bounds__(256) void k_cc_rename(const int* __restrict__ lab, const int* __restrict__ number, int N,
                                                   int* __restrict__ out) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v < N) out[v] = number[lab[v]];
}

}  // namespace gspx

// The round cap.  Call the sets between rounds supervertices, H_t the graph they form before round t (an edge where a
// stored entry joins two of them) and n_t their number inside one connected component.  In round t a supervertex
// hooks unless its label is a local minimum of H_t, so the supervertices of H_{t+1} are the local minima of H_t, and
// those of H_{t+2} are among them.  Let m survive both rounds while n_t >= 2.  m has a neighbour in H_t, and every
// neighbour v of m hooked onto m itself: had v hooked onto a smaller label m', v would sit in a tree whose root is at
// most m', next to m's tree, and m would not be a local minimum of H_{t+1}.  So the closed neighbourhoods {m} + N(m)
// in H_t of two such survivors are disjoint (a common neighbour hooked onto one label only; survivors are not
// adjacent), each holds at least two supervertices, and n_{t+2} <= n_t / 2.  From n_0 <= N a component is one
// supervertex after 2 ceil(log2 N) rounds; one more round finds nothing to hook and ends the loop.
static int cc_round_cap(int64_t N) {
  int lg = 0;
  while (((int64_t)1 << lg) < N) ++lg;
  return 2 * lg + 1;
}

extern "C" int gspx_components_round_cap(int64_t N, int* cap) {
  if (N < 0 || !cap) return set_err(GSPX_ERR_INVALID, "negative N or null output");
  *cap = cc_round_cap(N);
  return GSPX_OK;
}

extern "C" int gspx_graph_components_dev(gspx_graph* g, int32_t* labels_dev, int64_t* n_components, int* rounds,
                                         double* kernel_ms) {
  if (g) replay_reset(g->ctx);
  if (!g || !n_components) return set_err(GSPX_ERR_INVALID, "null graph or null component count");
  gspx_ctx* ctx = g->ctx;
  hipStream_t st = ctx->stream;
  const int N = (int)g->N;
  *n_components = 0;
  if (rounds) *rounds = 0;
  if (kernel_ms) *kernel_ms = 0;
  if (N == 0) return GSPX_OK;
  HIPCHK(hipSetDevice(ctx->device));
  const int cap = cc_round_cap(N);
  const dim3 grid((unsigned)((N + 256) / 256)), block(256);  // (covers N + 1 threads: k_cc_mark writes mark[N])
  DevMem lab, par, flag;
  CHK(lab.alloc((size_t)(N + 1) * sizeof(int)));
  CHK(par.alloc((size_t)(N + 1) * sizeof(int)));
  CHK(flag.alloc(sizeof(int)));
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL(k_cc_init, grid, block, 0, st, lab.as<int>(), par.as<int>(), N);
  int done = 0, changed = 1;
  while (changed) {
    if (done == cap)
      return set_err(GSPX_ERR_INTERNAL, "connected components: labels still change after %d rounds, the bound for %d "
                     "vertices", cap, N);
    HIPCHK(hipMemsetAsync(flag.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_cc_hook, grid, block, 0, st, g->lptr.as<int>(), g->lcol.as<int>(), lab.as<int>(),
                       par.as<int>(), N, flag.as<int>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&changed, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ++done;
    if (changed) hipLaunchKernelGGL(k_cc_shorten, grid, block, 0, st, lab.as<int>(), par.as<int>(), N);
  }
  // par is free now: it takes the marks, then their scan
  hipLaunchKernelGGL(k_cc_mark, grid, block, 0, st, lab.as<int>(), N, par.as<int>());
  HIPCHK(hipGetLastError());
  int count = 0;
  CHK(scan_exclusive(ctx, par.as<int>(), par.as<int>(), N + 1, &count));
  if (labels_dev) hipLaunchKernelGGL(k_cc_rename, grid, block, 0, st, lab.as<int>(), par.as<int>(), N, labels_dev);
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  CHK(finish_timed(ctx, kernel_ms));
  *n_components = count;
  if (rounds) *rounds = done;
  return GSPX_OK;
}

extern "C" int gspx_graph_components(gspx_graph* g, int32_t* labels_host, int64_t* n_components, int* rounds,
                                     double* kernel_ms) {
  if (!g || !n_components) return set_err(GSPX_ERR_INVALID, "null graph or null component count");
  if (!labels_host || g->N == 0) return gspx_graph_components_dev(g, nullptr, n_components, rounds, kernel_ms);
  HIPCHK(hipSetDevice(g->ctx->device));
  DevMem out;
  CHK(out.alloc((size_t)g->N * sizeof(int)));
  CHK(gspx_graph_components_dev(g, out.as<int32_t>(), n_components, rounds, kernel_ms));
  HIPCHK(hipMemcpy(labels_host, out.p, (size_t)g->N * sizeof(int), hipMemcpyDeviceToHost));
  return GSPX_OK;
}
