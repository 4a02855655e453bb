// gspx_linegraph.hip.h - the line graph of an undirected graph without self-loops, built on the device from the edge
// tables of gspx_ops.hip.h (pygsp/graphs/linegraph.py forms B^T B - I with scipy on the host).  gfx950 only.
// Included by gspx.hip after gspx_setup.hip.h (uses edges_for, the adjacency frame and scan_exclusive of
// gspx_adjacency.hip.h, DevMem, HIPCHK, CHK).
//
// Line-graph vertex e is edge e of Graph.get_edge_list(): the upper triangle of W in row-major order, in the caller's
// vertex order.  For a vertex v, I(v) is the ascending list of the edges incident to v: the edges that END in v
// (e_tedge[e_toff[v] .. e_toff[v + 1]), they lie in earlier rows, so their ids are smaller) followed by the edges that
// START in v (the contiguous block e_off[v] .. e_off[v + 1] - 1).  Row e = (s, t) of the adjacency is the merge of
// I(s) \ {e} and I(t) \ {e}; in a simple graph the two lists share e alone, so the row holds deg(s) + deg(t) - 2
// distinct ids and every value is 1.
//
// Three passes on the context's stream: row lengths (with a 64-bit total: the entry count may pass 2^31 long before
// the edge count does), a scan into row offsets, and the fill.  The fill is a flat grid over the OUTPUT ENTRIES, not
// over the rows - a hub gives rows of length ~N next to rows of length 2: entry k finds its row by a binary search in
// rowptr and its place in the row by rank, (index in its own list) + (lower bound of its id in the other list), less
// one for each list in which e comes before it.  One entry per lane, no atomics, no per-row loop; the result is
// fully determined by the input, so identical calls give identical bits.
#pragma once

namespace gspx {

struct LgTables {  // the edge tables of a graph (ensure_edges), caller's vertex order
  const int* eoff;   // N + 1: first id of the edges that start in a vertex
  const int* toff;   // N + 1: offsets into tedge
  const int* tedge;  // ids of the edges that end in a vertex, ascending
  const int* esrc;   // endpoints of every edge, esrc < edst
  const int* edst;
};

__device__ __forceinline__ int lg_deg(const LgTables& t, int v) {
  return (t.toff[v + 1] - t.toff[v]) + (t.eoff[v + 1] - t.eoff[v]);
}

// number of ids of I(v) that are smaller than `id`
__device__ __forceinline__ int lg_lower(const LgTables& t, int v, int id) {
  const int b0 = t.eoff[v], t0 = t.toff[v], t1 = t.toff[v + 1];
  if (id >= b0) return (t1 - t0) + min(id - b0, t.eoff[v + 1] - b0);  // past every edge that ends in v
  int a = t0, b = t1;
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (t.tedge[mid] < id) a = mid + 1; else b = mid;
  }
  return a - t0;
}

// the i-th id of I(v)
__device__ __forceinline__ int lg_at(const LgTables& t, int v, int i) {
  const int t0 = t.toff[v], nt = t.toff[v + 1] - t0;
  return i < nt ? t.tedge[t0 + i] : t.eoff[v] + (i - nt);
}

// the row of entry k: the e in [lo, hi) with rowptr[e] <= k < rowptr[e + 1], given rowptr[lo] <= k < rowptr[hi]
// (never an empty row: those have rowptr[e] == rowptr[e + 1])
__device__ __forceinline__ int lg_row(const int* __restrict__ rowptr, int lo, int hi, int k) {
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (rowptr[mid] <= k) lo = mid; else hi = mid;
  }
  return lo;
}

// row lengths (len: E ints, or null when only the total is wanted) and one 64-bit partial sum per workgroup
__global__ __launch_bounds__(256) void k_lg_len(LgTables t, int E, int* __restrict__ len,
                                                unsigned long long* __restrict__ partial) {
  unsigned long long sum = 0;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < E; e += (int64_t)gridDim.x * 256) {
    const int n = lg_deg(t, t.esrc[e]) + lg_deg(t, t.edst[e]) - 2;
    if (len) len[e] = n;
    sum += (unsigned long long)n;
  }
  __shared__ unsigned long long ws[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// second pass: the partials in a fixed order, one workgroup
__global__ __launch_bounds__(256) void k_lg_total(const unsigned long long* __restrict__ partial, int nparts,
                                                  unsigned long long* __restrict__ out) {
  unsigned long long sum = 0;
  for (int b = threadIdx.x; b < nparts; b += 256) sum += partial[b];
  __shared__ unsigned long long ws[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// one lane per stored entry: entry k of the flat output belongs to row e (rowptr[e] <= k < rowptr[e + 1]); its first
// deg(s) - 1 source slots walk I(s) \ {e}, the others I(t) \ {e}
__global__ __launch_bounds__(256) void k_lg_fill(LgTables t, const int* __restrict__ rowptr, int E, int nnz,
                                                 int* __restrict__ col, double* __restrict__ val) {
  const int64_t k64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k64 >= nnz) return;
  const int k = (int)k64;
  // the rows of this workgroup's first and last entry (the same for every lane), then the lane's own row between them
  const int64_t kb = (int64_t)blockIdx.x * 256;
  const int row_b = lg_row(rowptr, 0, E, (int)kb);
  const int row_e = lg_row(rowptr, row_b, E, (int)min(kb + 255, (int64_t)nnz - 1));
  const int lo = lg_row(rowptr, row_b, row_e + 1, k);
  const int e = lo, r0 = rowptr[e], q = k - r0;
  const int s = t.esrc[e], d = t.edst[e];
  const int ds = lg_deg(t, s);
  const bool first = q < ds - 1;
  const int own = first ? s : d, other = first ? d : s;
  const int i = first ? q : q - (ds - 1);       // index in I(own) \ {e}
  const int pe = lg_lower(t, own, e);            // where e itself sits in I(own)
  const int id = lg_at(t, own, i + (i >= pe));
  const int pos = i + lg_lower(t, other, id) - (id > e);  // (e is in the other list too)
  val[k] = 1.0;  // every value is one: written where the lane stands
  if (pos >= 0 && pos < rowptr[e + 1] - r0) col[r0 + pos] = id;
}

}  // namespace gspx

// the graph's edge tables, or the reason why the device builder does not serve it
static int linegraph_tables(gspx_graph* g, const char* who, gspx::LgTables* t) {
  CHK(edges_for(g));
  if (g->edges_custom)
    return set_err(GSPX_ERR_INVALID,
                   "%s: the graph carries a caller's edge list (a directed graph or one with self-loops); its line "
                   "graph is formed on the host", who);
  t->eoff = g->e_off.as<int>();
  t->toff = g->e_toff.as<int>();
  t->tedge = g->e_tedge.as<int>();
  t->esrc = g->e_src.as<int>();
  t->edst = g->e_dst.as<int>();
  return GSPX_OK;
}

static unsigned linegraph_len_blocks(int64_t E) { return (unsigned)std::min<int64_t>((E + 255) / 256, 4096); }

extern "C" int gspx_linegraph_size(gspx_graph* g, int64_t* n_vertices, int64_t* nnz) {
  if (!n_vertices || !nnz) return set_err(GSPX_ERR_INVALID, "gspx_linegraph_size: null output");
  *n_vertices = *nnz = 0;
  gspx::LgTables t{};
  CHK(linegraph_tables(g, "gspx_linegraph_size", &t));
  const int64_t E = g->n_edges;
  *n_vertices = E;
  if (E == 0) return GSPX_OK;
  if (E >= ((int64_t)1 << 31)) return set_err(GSPX_ERR_INVALID, "gspx_linegraph_size: %lld edges", (long long)E);
  hipStream_t st = g->ctx->stream;
  const unsigned nb = linegraph_len_blocks(E);
  DevMem partial;
  CHK(partial.alloc(((size_t)nb + 1) * sizeof(unsigned long long)));
  unsigned long long* p = partial.as<unsigned long long>();
  hipLaunchKernelGGL(gspx::k_lg_len, dim3(nb), dim3(256), 0, st, t, (int)E, (int*)nullptr, p);
  hipLaunchKernelGGL(gspx::k_lg_total, dim3(1), dim3(256), 0, st, p, (int)nb, p + nb);
  HIPCHK(hipGetLastError());
  unsigned long long total = 0;
  HIPCHK(hipMemcpyAsync(&total, p + nb, sizeof(total), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  *nnz = (int64_t)total;
  return GSPX_OK;
}

extern "C" int gspx_linegraph_build(gspx_graph* g, gspx_knn** out, double* kernel_ms) {
  if (!out) return set_err(GSPX_ERR_INVALID, "gspx_linegraph_build: null output");
  *out = nullptr;
  if (kernel_ms) *kernel_ms = 0;
  int64_t E = 0, nnz = 0;
  CHK(gspx_linegraph_size(g, &E, &nnz));  // (refuses a null graph, a graph not made from W, a caller's edge list)
  const int64_t cap = ((int64_t)1 << 31) - 1;
  if (E > cap || nnz > cap)  // before anything of the output is allocated
    return set_err(GSPX_ERR_INVALID,
                   "gspx_linegraph_build: the line graph has %lld vertices and %lld stored entries; both must be at "
                   "most %lld (32-bit indices)", (long long)E, (long long)nnz, (long long)cap);
  gspx::LgTables t{};
  CHK(linegraph_tables(g, "gspx_linegraph_build", &t));
  gspx_ctx* ctx = g->ctx;
  hipStream_t st = ctx->stream;
  replay_reset(ctx);
  const auto t0 = std::chrono::steady_clock::now();
  std::unique_ptr<gspx_knn> h;
  CHK(adjacency_open(ctx, E, h));
  h->nnz = nnz;  // known beforehand: col and val are allocated here, outside the timed bracket, not by adjacency_offsets
  if (nnz > 0) {
    DevMem partial;
    const unsigned nb = linegraph_len_blocks(E);
    CHK(partial.alloc((size_t)nb * sizeof(unsigned long long)));
    CHK(h->col.alloc((size_t)nnz * sizeof(int)));
    CHK(h->val.alloc((size_t)nnz * sizeof(double)));
    HIPCHK(hipEventRecord(ctx->ev[0], st));
    hipLaunchKernelGGL(gspx::k_lg_len, dim3(nb), dim3(256), 0, st, t, (int)E, h->rowptr.as<int>(),
                       partial.as<unsigned long long>());
    CHK(scan_exclusive(ctx, h->rowptr.as<int>(), h->rowptr.as<int>(), (int)E + 1));  // lengths -> offsets, in place
    hipLaunchKernelGGL(gspx::k_lg_fill, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, t, h->rowptr.as<int>(),
                       (int)E, (int)nnz, h->col.as<int>(), h->val.as<double>());
    HIPCHK(hipEventRecord(ctx->ev[1], st));
    CHK(finish_timed(ctx, kernel_ms));
  } else {
    HIPCHK(hipStreamSynchronize(st));
  }
  adjacency_close(h, t0, out);
  return GSPX_OK;
}
