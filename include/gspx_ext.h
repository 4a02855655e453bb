/*
 * gspx_ext.h - entry points of libgspx BESIDE the drop-in boundary of include/gspx.h: the rows SURVEY.md
 * section 8 marks "next" (operators on the same device CSR, nearest-neighbour / SBM graph construction),
 * the opt-in Newton-form evaluation, host-built tiles, the schedule export used by the CPU tests and the
 * bandwidth calibration kernels.  Same conventions as gspx.h (status codes, ownership, one ctx = one
 * stream).  A binding that only replaces pygsp.filters.approximations.cheby_op needs none of these.
 */
#ifndef GSPX_EXT_H
#define GSPX_EXT_H

#include "gspx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The same polynomial in NEWTON form (single filter, analysis), evaluated by Horner:
 *     y = sum_{j=0..K} d_j prod_{i<j} (Lt - r_i I) x,    Lt = (L - a2 I)/a1,  a1 = a2 = lmax/2
 * `nodes` = r_0..r_{K-1}, `dcoef` = d_0..d_K (host, float64).  A two-term recurrence: 3 panel
 * passes per order and no accumulator, against 3 + 2/3 for the three-term Chebyshev recurrence
 * of gspx_cheby_filter*.  The caller derives (nodes, dcoef) from the reference's Chebyshev
 * coefficients in exact arithmetic (pygsp_amd/filters.py::cheb_to_newton), so both entry points
 * evaluate the identical polynomial; they agree to rounding (~1e-14 in float64).
 * x: [N][Nsig], y: [N][Nsig].  K < 1 -> GSPX_ERR_COEFF. */
int gspx_newton_filter_dev(gspx_graph* g, double lmax, int K, const double* nodes,
                           const double* dcoef, int64_t Nsig, const void* x_dev, void* y_dev,
                           double* kernel_ms);
int gspx_newton_filter(gspx_graph* g, double lmax, int K, const double* nodes, const double* dcoef,
                       int64_t Nsig, const void* x_host, void* y_host, double* kernel_ms);

/* A polynomial of the scaled operator t = (2 / lmax) L - I evaluated as a PROGRAM of S steps on N x Nsig panels:
 *     h_0 = x;   h_{s+1} = scale_s * (2 t) h_s + beta_s * h_s + gamma_s * o_s;   y = h_S,
 * o_s = x for every step (old_is_x != 0: the Newton form above is such a program) or o_s = h_{s-1} (old_is_x == 0, gamma_0
 * ignored: the PRODUCT form - a real root r of the polynomial is one step with scale sigma / 2, beta -sigma r, gamma 0, which
 * reads one panel and writes one; a conjugate pair a +- ib is two steps, the second with gamma sigma^2 b^2).  The same
 * polynomial as approximations.py:93-112 evaluates when the program is built from its Chebyshev coefficients
 * (pygsp_amd.filters.cheb_to_product, behind filters.product_guard): 2.2 - 2.5 panel passes per order instead of 3 2/3.
 * Single filter, analysis.  _dev: device pointers; the other: host arrays.  S < 1 -> GSPX_ERR_COEFF. */
int gspx_poly_program_dev(gspx_graph* g, double lmax, int S, const double* scale, const double* beta, const double* gamma,
                          int old_is_x, int64_t Nsig, const void* x_dev, void* y_dev, double* kernel_ms);
int gspx_poly_program(gspx_graph* g, double lmax, int S, const double* scale, const double* beta, const double* gamma,
                      int old_is_x, int64_t Nsig, const void* x_host, void* y_host, double* kernel_ms);

/* The internal padded CSR pattern (engine vertex order; rowptr low 2 bits = pad counts, pads have col == N): what
 * host-built tiles (pygsp_amd/tiling.py) are computed from. */
int gspx_graph_download_internal(gspx_graph* g, int32_t* rowptr, int32_t* col);

/* Optional acceleration structure for gspx_cheby_filter* with ONE filter: one-level row tiles
 * (64-row blocks of the internal vertex order: per block the distinct rows it gathers, s1ptr /
 * s1rows; per stored entry the 16-bit position of its column in that list, lidx, pads = 0;
 * pygsp_amd/tiling.py builds them from gspx_graph_download_internal).  With tiles set (and option
 * "tile_gather" = 1, the default) every recurrence step stages the gathered panel in LDS
 * (k_step_tile).  block_rows == 0 drops the tiles.  stats (nullable): blocks, blocks on the
 * plain-gather path (tile too large for LDS), dynamic LDS bytes per workgroup. */
int gspx_graph_set_gather_tiles(gspx_graph* g, int block_rows, int nb, const int32_t* s1ptr,
                                const int32_t* s1rows, const uint16_t* lidx, int64_t* stats);

/* ---- operators on the same device CSR --------------------------------
 * Panels are DEVICE pointers (gspx_buf_ptr or any other device allocation), row-major N x Nsig,
 * compute dtype of the graph, caller's vertex order.
 *
 * y = L x: the product inside Graph.dirichlet_energy (pygsp/graphs/graph.py:702) and inside the
 * operator of learning.regression_tikhonov (pygsp/learning.py:330). */
int gspx_laplacian_apply_dev(gspx_graph* g, int64_t Nsig, const void* x_dev, void* y_dev,
                             double* kernel_ms);
/* gram_host[Nsig*Nsig] (double, row-major, HOST) = X^T (L X): Graph.dirichlet_energy,
 * graph.py:642-702 (a scalar for one signal). */
int gspx_dirichlet_energy_dev(gspx_graph* g, int64_t Nsig, const void* x_dev, double* gram_host,
                              double* kernel_ms);
/* ---- dense fp64 panel primitives (partial Fourier basis, pygsp_amd/fourier.py) ---------------------------
 * Panels: fp64 DEVICE pointers, row-major, N rows, leading dimension ld* >= width (elements); widths 1..512 unless
 * an entry point says otherwise; any N >= 0.  Matrix-core (f64 MFMA) kernels; every reduction goes through per-workgroup partials and a fixed-order
 * second pass, so the same inputs give the same bits on every call.  Vertex order: whatever the caller's panels use.
 * C_host (na x nb, row-major, HOST) = A^T B. */
int gspx_panel_gram_dev(gspx_ctx* ctx, int64_t N, const double* A, int64_t lda, int na, const double* B, int64_t ldb,
                        int nb, double* C_host, double* kernel_ms);
/* Y = X Q, Q (p x q, row-major, HOST) staged in LDS tiles; Y must not overlap X (GSPX_ERR_INVALID). */
int gspx_panel_combine_dev(gspx_ctx* ctx, int64_t N, const double* X, int64_t ldx, int p, const double* Q_host, int q,
                           double* Y, int64_t ldy, double* kernel_ms);
/* C (na x nb, row-major, leading dimension ldc >= nb, DEVICE) = alpha A^T diag(rowscale) B for ANY widths na, nb >= 0
 * (not capped at 512): the Gram whose result stays on the device.  rowscale: N doubles on the DEVICE, or NULL for the
 * plain A^T B.  C must not overlap A, B or rowscale.  N == 0 or an empty width: nothing is written. */
int gspx_panel_gram_to_dev(gspx_ctx* ctx, int64_t N, const double* A, int64_t lda, int na, const double* B, int64_t ldb,
                           int nb, const double* rowscale, double alpha, double* C, int64_t ldc, double* kernel_ms);
/* Exact Fourier filtering's product Y_g = U Q_g (filter.py:292-301), Q_g formed from the coefficients S and the
 * multipliers H (all DEVICE) while its tiles are staged, never materialised.  U: N x n, leading dimension ldu; any
 * contraction length n >= 1, any width w >= 0.  mode 0 (plain, igft): Y = U S, nf = 1, H unused.  mode 1 (analysis):
 * S one n x w panel, H nf x n row-major, Y nf planes [filter][vertex][signal] (plane stride N ldy),
 * Q_g[k][c] = H[g][k] S[k][c].  mode 2 (synthesis): S nf panels (plane stride n lds), one output plane,
 * Q[k][c] = sum_f H[f][k] S_f[k][c] in filter order.  Y must not overlap U, S or H.  The contraction runs in one
 * fixed order: the same bits on every call.  N == 0 or w == 0: nothing is written. */
int gspx_spectral_apply_dev(gspx_ctx* ctx, int64_t N, const double* U, int64_t ldu, int n, const double* S, int64_t lds,
                            int w, int mode, int nf, const double* H, double* Y, int64_t ldy, double* kernel_ms);
/* out_host[i] (HOST) = || LX[:, i] - theta_host[i] X[:, i] ||_2, both panels read once (no ||LX||^2 - theta^2). */
int gspx_panel_residual_norms_dev(gspx_ctx* ctx, int64_t N, const double* X, const double* LX, int64_t ld, int p,
                                  const double* theta_host, double* out_host, double* kernel_ms);
/* Y[:, 0:w] = X[:, 0:w] row by row (hipMemcpy2DAsync), e.g. a column block of a wider panel out or back in;
 * Y must not overlap X.  kernel_ms of all four: the device work only, not the small host copies of Q / theta / C. */
int gspx_panel_copy_dev(gspx_ctx* ctx, int64_t N, const double* X, int64_t ldx, int w, double* Y, int64_t ldy,
                        double* kernel_ms);
/* ---- Lanczos filtering (pygsp_amd/lanczos.py; approximations.lanczos_op of the reference) -----------------------
 * fp64 graphs only (an fp32 graph: GSPX_ERR_INVALID).  x_dev: N x Nsig fp64 (DEVICE, caller's vertex order, leading
 * dimension ldx >= Nsig), Nsig 0..256 and, with the `order` stack panels and three work panels, within the context's
 * ws_limit_mb.  V_dev: order x N x Nsig fp64 (DEVICE), written as the Krylov stack in the graph's INTERNAL vertex
 * order (column c of panel j = q_j of signal c; zero where a column has stopped).  HOST outputs, row-major
 * order x Nsig: alpha_host (H's diagonal), beta_host (row 0 = ||x||, row k = beta_k, H's off-diagonal), proj_host
 * (V^T x); steps_host: Nsig ints, the Krylov dimension m of each column (0 for a zero column).  A column stops at
 * step k when beta_k <= breakdown.  phase_ms (6 doubles or NULL: permute, product, three-term, dots, update,
 * projection) times every launch with events when given.  The same inputs give the same bits on every call. */
int gspx_lanczos_krylov_dev(gspx_graph* g, int order, int64_t Nsig, const void* x_dev, int64_t ldx, double breakdown,
                            void* V_dev, double* alpha_host, double* beta_host, double* proj_host, int32_t* steps_host,
                            double* phase_ms, double* kernel_ms);
/* y[f N + n][c] = sum_j weights_host[f][j][c] V_j[n][c] for the Nf filters (HOST weights Nf x order x Nsig), one pass
 * over the stack V_dev of gspx_lanczos_krylov_dev; y_dev (DEVICE, Nf N rows, leading dimension ldy >= Nsig) in the
 * caller's vertex order. */
int gspx_lanczos_combine_dev(gspx_graph* g, int order, int64_t Nsig, const void* V_dev, int Nf,
                             const double* weights_host, void* y_dev, int64_t ldy, double* kernel_ms);
/* Tikhonov regression with tau > 0 (pygsp/learning.py:324-337): solves (diag(M) + tau L) x = M y,
 * one conjugate-gradient run per column with scipy.sparse.linalg.cg's recurrence and stopping rule
 * (x0 = 0, ||r|| < max(atol, rtol ||b||); scipy's defaults are rtol 1e-5, atol 0, maxiter 10 N).
 * mask_dev: N values of the compute dtype (1 = measured, 0 = not).  iterations: Nsig ints (HOST)
 * or NULL. */
int gspx_tikhonov_cg_dev(gspx_graph* g, double tau, const void* mask_dev, int64_t Nsig,
                         const void* y_dev, void* x_dev, double rtol, double atol, int64_t maxiter,
                         int32_t* iterations, double* kernel_ms);
/* Harmonic extension (regression_tikhonov with tau = 0, pygsp/learning.py:349-367): x = y on the measured vertices
 * (mask != 0); on the others x_u solves L_uu x_u = -L_ul y_l, one conjugate-gradient run per column, the recurrence
 * and stopping rule of gspx_tikhonov_cg_dev (x0 = 0, ||r|| < max(atol, rtol ||b||), b = -L_ul y_l), all columns
 * advanced together.  L is the graph's Laplacian of whatever lap_type it was built with.  y is READ ONLY AT MEASURED
 * ROWS (a select, not a product: NaN at unmeasured rows is harmless).  A component without a measured vertex has
 * b = 0 there and keeps x = 0 (the minimum-norm solution; the reference's spsolve fails on it).  mask_dev: N values
 * of the compute dtype; y_dev, x_dev: N x Nsig, compute dtype, caller's vertex order, distinct buffers; iterations:
 * Nsig ints (HOST) or NULL; fp32 and fp64 graphs; any Nsig >= 0 in column batches of at most 256.  The same inputs
 * give the same bits on every call. */
int gspx_dirichlet_cg_dev(gspx_graph* g, const void* mask_dev, int64_t Nsig, const void* y_dev, void* x_dev,
                          double rtol, double atol, int64_t maxiter, int32_t* iterations, double* kernel_ms);
/* classification_tikhonov_simplex (pygsp/learning.py:111-180): argmin over X (N x n_classes, every row on the
 * probability simplex) of tau sum(X * L X) + sum_i m_i ||X_i - Y_i||^2, by accelerated forward-backward (FISTA) with
 * the fixed `step`, started at X_0 = Y; Y is one-hot, zero rows where unmeasured.  float64 graphs only.
 * labels_dev: N int32 (DEVICE, caller's vertex order), the class 0..n_classes-1 of a measured vertex, -1 for an
 * unmeasured one (another value: GSPX_ERR_INVALID after one small device pass); n_classes 1..256.  Stopping rule,
 * tested after every iteration k in this order: obj_k < atol, |obj_k - obj_{k-1}| < dtol, |obj_k - obj_{k-1}| / d <
 * rtol (d = obj_k, else obj_{k-1}, else 1), ||X_k - X_{k-1}||_F / sqrt(N n_classes) < xtol, k >= maxit (1..1e7); a
 * negative tolerance disables its criterion.  x_dev: N x n_classes fp64 (DEVICE, caller's order) receives X_niter.
 * HOST outputs: niter, crit (1 atol, 2 dtol, 3 rtol, 4 xtol, 5 maxit), objective_host (room for maxit + 1 doubles)
 * obj_0 .. obj_niter.  The same inputs give the same bits on every call. */
int gspx_tikhonov_simplex_dev(gspx_graph* g, double tau, double step, const int32_t* labels_dev, int n_classes,
                              double rtol, double atol, double dtol, double xtol, int64_t maxit, void* x_dev,
                              int64_t* niter, int32_t* crit, double* objective_host, double* kernel_ms);
/* Proximal operator of the graph total variation: argmin over z (N x Nsig) of 1/2 ||x - z||^2 + gamma ||D^T z||_1, D
 * the differential operator below (the edge list the graph holds when called: the default upper triangle or the one of
 * gspx_graph_set_edge_list).  FISTA on the dual min_{|u| <= gamma} 1/2 ||x - D u||^2 with the fixed `step` (<= 1 /
 * lambda_max(D D^T)), u_0 = 0, primal iterate z_k = x - D u_k; one objective, obj_k = 1/2 ||x - z_k||^2 + gamma
 * ||D^T z_k||_1, for the whole panel.  float64 graphs only; Nsig 1..256; gamma >= 0; x_dev / z_dev: N x Nsig fp64
 * (DEVICE, caller's vertex order; they may be the same buffer).  Stopping rule, outputs and reproducibility as for
 * gspx_tikhonov_simplex_dev, with ||z_k - z_{k-1}||_F / sqrt(N Nsig) for xtol; objective_host: room for maxit + 1. */
int gspx_prox_tv_dev(gspx_graph* g, double gamma, double step, int64_t Nsig, const void* x_dev, void* z_dev,
                     double rtol, double atol, double dtol, double xtol, int64_t maxit, int64_t* niter, int32_t* crit,
                     double* objective_host, double* kernel_ms);
/* Differential operator D (L = D D^T) of an UNDIRECTED graph without self loops created from W
 * (pygsp/graphs/difference.py:26-166).  Edges = stored entries (i, j > i) in row-major order, the
 * order of Graph.get_edge_list (graph.py:1019-1029).  Built on the device at first use.
 * download: any output may be NULL; d_source / d_target are D[i, k] at the edge's source (negative)
 * and target (positive). */
int gspx_graph_n_edges(gspx_graph* g, int64_t* n_edges);
int gspx_graph_download_edges(gspx_graph* g, int32_t* sources, int32_t* targets, void* weights,
                              void* d_source, void* d_target);
/* The differential operator of a DIRECTED graph, or of a graph with self-loops, from the caller's edge list
 * (Graph.get_edge_list, graph.py:1019-1029: every stored entry of W for a directed graph, the upper triangle
 * including the diagonal otherwise; sources non-decreasing).  The device graph was built from the symmetrised W
 * (graph.py:613-616), whose degrees are the reference's dw of the directed graph, so the D values of
 * difference.py:151-161 are formed on the device: -sqrt(w) / +sqrt(w), or -sqrt(w / dw[source]) /
 * +sqrt(w / dw[target]), divided by sqrt(2) when `directed`.  Replaces the edge list gspx_graph_n_edges /
 * gspx_graph_download_edges / gspx_grad_dev / gspx_div_dev work on (by default the upper triangle of the graph's
 * own Laplacian). */
int gspx_graph_set_edge_list(gspx_graph* g, int64_t n_edges, const int32_t* sources, const int32_t* targets,
                             const double* weights, int directed);

/* grad: y (n_edges x Nsig) = D^T x   (difference.py:168-244)
 * div:  z (N x Nsig)       = D y     (difference.py:246-331) */
int gspx_grad_dev(gspx_graph* g, int64_t Nsig, const void* x_dev, void* y_dev, double* kernel_ms);
int gspx_div_dev(gspx_graph* g, int64_t Nsig, const void* y_dev, void* z_dev, double* kernel_ms);

/* ---- k-nearest-neighbour graph construction on the device ---------------
 * Replaces, for NNtype='knn' and 1..4096 dimensions (a uniform grid in 1-3 dimensions; beyond that a tiled brute
 * force whose pair distances run on the matrix cores, candidates re-evaluated in the KD-tree's arithmetic; up to
 * 64 dimensions with the queries in registers, beyond that with a run-time dimension loop and one wave per query
 * in the exact stages - chosen by d > 64 alone, same plan, same statistics, same bits; 1 <= k <= 64),
 * the KD-tree query, the Gaussian weights and the symmetrisation of NNGraph
 * (pygsp/graphs/nngraphs/nngraph.py:213-226, 289-297):
 *   D, NN = KDTree(X).query(X, k + 1);  sigma = mean(D[:, 1:]);  w = exp(-D^2 / sigma);
 *   W = (W + W.T) / 2
 * coords: N x d doubles on the HOST, already centred / rescaled by the caller (nngraph.py:129-137).
 * sigma == 0 selects the mean neighbour distance.  metric: 0 euclidean, 1 manhattan, 2 max_dist (the
 * reference's dist_type; 'minkowski' with order 1, 2 or inf maps onto them).  symmetrize: 0 'average',
 * 1 'maximum' (= 'fill' for a k-NN matrix), 2 'tril', 3 'triu' (utils.symmetrize, utils.py:247-275).  Neighbours and distances
 * equal scipy's KD-tree bit for bit (ties ordered by vertex index); a point is never its own neighbour.  Context option "knn_f32": the candidate sweep beyond three
 * dimensions on the fp32 matrix cores - 1 (default) when its rounding margin is small against the bounds, 0 never,
 * 2 always; the selection is exact either way.
 * The handle is the device adjacency (CSR weight matrix) of EVERY builder declared below that hands out a gspx_knn -
 * radius, block model, line graph, Kron reduction, learned graph, coarse graph - and gspx_knn_destroy / _info /
 * _download_w serve them all; the name is historical (the k-NN builder came first). */
typedef struct gspx_knn gspx_knn;
int gspx_knn_build(gspx_ctx* ctx, int64_t N, int d, const double* coords, int k, double sigma,
                   int metric, int symmetrize, gspx_knn** out);
int gspx_knn_destroy(gspx_knn* h);
int gspx_knn_info(gspx_knn* h, int64_t* nnz, double* sigma, double* build_ms);
/* how the neighbour search of the last build ran in more than three dimensions (tiled brute force, pair
 * distances on MFMA): out[0] sample size behind the per-query bounds, out[1] candidate capacity per query,
 * out[2] mean candidates per query, out[3] queries that took the exact scan (zeros for the 1-3-D grid search) */
int gspx_knn_search_stats(gspx_knn* h, double out[4]);
/* symmetric W as CSR (sorted columns), float64 */
int gspx_knn_download_w(gspx_knn* h, int32_t* indptr, int32_t* indices, double* data);
/* NN[:, 1:] and D[:, 1:] of the reference: N x k, nearest first (either may be NULL) */
int gspx_knn_download_neighbors(gspx_knn* h, int32_t* nn, double* dist);

/* Radius graphs: NNtype='radius' of NNGraph (nngraph.py:228-287) - neighbours within epsilon (the
 * KD-tree's ball query, squared distance <= epsilon^2), weights exp(-d^2 / sigma), sigma == 0 selects
 * the mean neighbour distance ("No neighbors found" -> GSPX_ERR_INVALID, as the reference's ValueError).
 * 1 to 4096 dimensions: a grid of epsilon-sized cells up to 3-D; beyond that the candidate pairs come from an MFMA
 * distance sweep (a counting pass, then a filling pass into rows of exactly those lengths) and are tested in the
 * KD-tree's arithmetic.  Result read with gspx_knn_info / gspx_knn_download_w, freed with gspx_knn_destroy. */
int gspx_radius_build(gspx_ctx* ctx, int64_t N, int d, const double* coords, double epsilon,
                      double sigma, int metric, gspx_knn** out);

/* Stochastic block model / Erdos-Renyi graph sampled on the device: every unordered pair (r, c) of
 * distinct vertices is an edge (unit weight) independently with probability M[z_r][z_c] - the
 * distribution of pygsp/graphs/stochasticblockmodel.py:125-144 (directed=False, self_loops=False)
 * and erdosrenyi.py (k = 1), in O(edges) instead of the reference's N^2 Python loop.  The random
 * stream is the engine's own (counter-based), so graphs equal the reference's in distribution, not
 * bit for bit.  order: the vertices grouped by block (a stable argsort of z), bounds[k + 1]: where
 * each block starts in it, M: k x k symmetric, row-major.  The result is read with
 * gspx_knn_info / gspx_knn_download_w and freed with gspx_knn_destroy. */
int gspx_sbm_build(gspx_ctx* ctx, int64_t N, int k, const int32_t* order, const int64_t* bounds,
                   const double* M, uint64_t seed, gspx_knn** out);
/* The same sampler with the reference's other two switches (stochasticblockmodel.py:69-70, 128-130): flags bit 0
 * = directed (every ORDERED pair (r, c) is an entry W[r, c] = 1 with probability M[z_r][z_c]; M need not be
 * symmetric), bit 1 = self_loops (the pairs r == c take part; an undirected self-loop is one stored entry).
 * flags = 0 is gspx_sbm_build.  `connected=True` is a loop of the host layer over seeds (n_try). */
int gspx_sbm_build_ex(gspx_ctx* ctx, int64_t N, int k, const int32_t* order, const int64_t* bounds,
                      const double* M, uint64_t seed, int flags, gspx_knn** out);

/* The line graph of an undirected graph without self-loops (pygsp/graphs/linegraph.py), built on the device from the
 * edge tables of grad / div.  g: a graph created from W, either compute dtype and lap_type - only the pattern of its
 * Laplacian is read; a graph created from L is refused with the differential operator's error, a graph that carries
 * a caller's edge list (a directed graph, self-loops) with GSPX_ERR_INVALID - the host layer forms those.
 * Line-graph vertex e is edge e of Graph.get_edge_list: the upper triangle of W, row-major, caller's vertex order.
 * size: the vertex count (= n_edges) and the stored entries of the adjacency, sum over edges (s, t) of
 * deg(s) + deg(t) - 2, from a 64-bit reduction - it may exceed 32 bits, and nothing is allocated for it.
 * build: the adjacency as a handle read with the k-NN handle's info / download calls, handed to the set-up from a
 * handle and freed with its destroy call: canonical CSR with sorted columns, every value exactly 1.0, no diagonal,
 * no stored zero (its neighbour / distance members stay empty).  GSPX_ERR_INVALID with both counts in the message,
 * before any allocation of the output, when either exceeds 2^31 - 1.  A graph without edges gives an empty handle
 * (N = 0, nnz = 0).  kernel_ms (may be NULL): length pass, scan and fill on the context's stream.  The result is
 * fully determined by the input: identical calls give identical bits. */
int gspx_linegraph_size(gspx_graph* g, int64_t* n_vertices, int64_t* nnz);
int gspx_linegraph_build(gspx_graph* g, gspx_knn** out, double* kernel_ms);

/* Schur complements of A = L + shift I, shift >= 0 (pygsp/reduction.py: kron_reduction, interpolate).
 * schur_cg: the harmonic extension of gspx_dirichlet_cg_dev at a shift.  x = f on the kept vertices (mask != 0) and
 * A_uu x_u = -A_uk f_k on the others, the same conjugate-gradient loop, column batches (<= 256), dtypes (fp32, fp64),
 * stopping rule and reproducibility.  f_dev (N x Nsig) is read only at kept rows.  x_dev (may be NULL) receives the
 * extension; alpha_dev (may be NULL) receives (A x) at the kept rows - the Schur complement applied to f_k, K_reg f of
 * reduction.interpolate - and exact zeros elsewhere, N x Nsig in the caller's vertex order; eliminated rows are not
 * computed.  With shift == 0, x_dev holds the bytes gspx_dirichlet_cg_dev writes.
 * kron_build: the Kron reduction A_kk - A_ku A_uu^-1 A_uk for the kept vertices ind_host[0 .. nk) (HOST; any order,
 * unique and in range: vertex ind[c] becomes vertex c of the result).  fp64 graphs only.  lnew_dev (may be NULL): the
 * dense nk x nk matrix (DEVICE, row-major), symmetrised as (S + S^T) / 2, diagonal included.  w_out (may be NULL):
 * W = max(0, -offdiag) as a handle of the kind gspx_linegraph_build returns - canonical CSR, no diagonal, no stored
 * zero or negative value, equal to its transpose bit for bit, the same bits on every call.  An entry the iteration
 * never reaches (two kept vertices further apart than its step count) is an exact zero; a direct solve leaves a
 * value below the tolerance there.  iterations: nk ints (HOST) or NULL.  kernel_ms: the whole device work; after the
 * call gspx_last_timing holds its parts - [0] the solves, [1] the row products, [2] the finalising pass.  GSPX_ERR_INVALID, with the sizes in the
 * message, when the nk x nk buffer and the work panels of one batch exceed the context's ws_limit_mb. */
int gspx_schur_cg_dev(gspx_graph* g, double shift, const void* mask_dev, int64_t Nsig, const void* f_dev, void* x_dev,
                      void* alpha_dev, double rtol, double atol, int64_t maxiter, int32_t* iterations,
                      double* kernel_ms);
int gspx_kron_build(gspx_graph* g, double shift, const int32_t* ind_host, int64_t nk, double rtol, int64_t maxiter,
                    double* lnew_dev, gspx_knn** w_out, int32_t* iterations, double* kernel_ms);

/* Multilevel coarsening by heavy-edge matching and pooling over the resulting partitions (pygsp_amd.reduction.coarsen,
 * pygsp_amd.nn.GraphPool; DESIGN.md "Coarsening and pooling").  match and build take an fp64 graph created from W with
 * the combinatorial Laplacian; they read its canonical Laplacian (caller's vertex order: w_ij = -L_ij off the
 * diagonal, so a self-loop is never seen) and its weighted degrees, never the internal order.
 * match_heavy_edges: handshake rounds.  Every unmatched vertex proposes to its unmatched neighbour of largest score -
 * metric 0: w_ij (1 / d_i + 1 / d_j), metric 1: w_ij, fp64 - ties to the smaller vertex index; mutual proposals are
 * matched.  While an edge joins two unmatched vertices a round matches at least one pair; the loop ends at the first
 * round that matches nothing (the matching is then maximal) or after max_rounds productive rounds (max_rounds < 0:
 * no limit; a path with monotone weights needs N / 2).  mate_host (N int32, HOST): the partner, mate[i] == i for a
 * singleton; rounds: the rounds that matched something; pairs; kernel_ms (each may be NULL but mate_host).
 * coarsen_build: Wc = P^T W P without its diagonal for the cluster map parent_host (N int32 in [0, n_clusters), HOST;
 * every cluster has a member, any size).  An entry above the diagonal is the sum of its fine entries in ascending
 * (fine row, fine column) order; the entry below is a copy of it.  out: a handle of the kind gspx_linegraph_build
 * returns under gspx_kron_build's contract - canonical CSR, sorted columns, no diagonal, no stored zero, equal to its
 * transpose bit for bit.  No atomics; identical calls give identical bits.
 * segment_pool: y[c][:] = max | mean | sum (mode 0 | 1 | 2) of x[idx[m]][:] over ptr[c] <= m < ptr[c + 1], row-major
 * panels N x width -> Nc x width of dtype GSPX_F32 / GSPX_F64, all DEVICE pointers; ptr / idx a partition of the N rows
 * (every row in exactly one segment, no empty segment - not checked here), members visited in the order of idx: mean is
 * that sum divided by the size, max keeps the first maximum.  16-byte accesses when width is a multiple of 16 bytes and
 * the panels are aligned.  segment_pool_vjp: gx[idx[m]][:] from g[c][:] - sum: a copy (this is unpooling), mean:
 * g / size, max: g at the first member that attains the maximum of x_dev (read for max only, else may be NULL), zero
 * at the others.  Writes are disjoint: no atomics. */
int gspx_match_heavy_edges(gspx_graph* g, int metric, int64_t max_rounds, int32_t* mate_host, int32_t* rounds,
                           int64_t* pairs, double* kernel_ms);
int gspx_coarsen_build(gspx_graph* g, const int32_t* parent_host, int64_t n_clusters, gspx_knn** out,
                       double* kernel_ms);
int gspx_segment_pool_dev(gspx_ctx* ctx, int dtype, int mode, int64_t N, int64_t Nc, int64_t width,
                          const int32_t* ptr_dev, const int32_t* idx_dev, const void* x_dev, void* y_dev,
                          double* kernel_ms);
int gspx_segment_pool_vjp_dev(gspx_ctx* ctx, int dtype, int mode, int64_t N, int64_t Nc, int64_t width,
                              const int32_t* ptr_dev, const int32_t* idx_dev, const void* x_dev, const void* g_dev,
                              void* gx_dev, double* kernel_ms);

/* Learning the weights of a graph from smooth signals (pygsp_amd.graph_learning; the log-degree model of Kalofolias
 * 2016 on a fixed pattern as in Kalofolias & Perraudin 2019; the definition is tests/graphlearn_helpers.py).
 * Both calls take an fp64 graph created from W that carries its default edge list - edge e = (s, t), s < t, is edge e
 * of Graph.get_edge_list, caller's vertex order; only the pattern is read.  A float32 graph, a graph created from L and a
 * graph carrying a caller's edge list (a directed graph, self-loops) are GSPX_ERR_INVALID with the reason in the message.
 * edge_sqdist: z_dev[e] = ||x_s - x_t||^2 (n_edges fp64, DEVICE) for x_dev an N x F fp64 row-major panel (DEVICE,
 * caller's vertex order), 1 <= F <= 4096.  A group of lanes per edge (a power of two, at most a wavefront) walks the
 * two rows with 16-byte loads where F is even and x_dev 16-byte aligned; every lane sums its columns in ascending
 * order in fp64 and the lanes are combined by a fixed tree: every entry is within F eps of the exact sum, the same
 * bits on every call.
 * learn_log_degrees: argmin over w >= 0 (n_edges values) of 2 z^T w - a sum_i log (S w)_i + b ||w||^2, (S w)_i the sum
 * of w over the edges at vertex i (vertices without edges take no part), by forward-backward-forward primal-dual
 * iterations with the fixed step step_gamma (valid below 1 / (2 b + sqrt(2 dmax)), dmax the largest vertex degree), from
 * w_0 = w0_dev (NULL: zeros) and v_0 = S w_0:
 *   Y = w - g (2 b w + S^T v), y = v + g S w;  P = max(0, Y - 2 g z), p = prox(y);  Q = P - g (2 b P + S^T p),
 *   q = p + g S P;  w <- w - Y + Q, v <- v - y + q;  prox(y) = (y - r) / 2 for y <= 0, -2 a g / (y + r) for y > 0,
 *   r = sqrt(y^2 + 4 a g).
 * Stops after iteration k when ||w_k - w_{k-1}|| <= tol ||w_k|| and ||v_k - v_{k-1}|| <= tol ||v_k|| (*crit = 1; a
 * negative tol disables it) or k >= maxit (*crit = 5).  p_dev (n_edges fp64, DEVICE) receives P of the last iteration:
 * non-negative with exact zeros; w_dev (may be NULL) the last w, for warm starts.  w_out (may be NULL): P as a symmetric
 * adjacency, a handle of the kind gspx_linegraph_build returns under gspx_kron_build's contract - canonical CSR in the
 * caller's vertex order, sorted columns, no diagonal, no stored zero, equal to its transpose bit for bit; no handle is
 * left behind by a failing call.  HOST outputs: niter, crit, history_host (room for 4 maxit doubles): ||w_k - w_{k-1}||,
 * ||w_k||, ||v_k - v_{k-1}||, ||v_k|| for k = 1 .. niter.  kernel_ms (may be NULL): the iterations, without the adjacency.
 * GSPX_ERR_INVALID: a not positive or not finite, b negative, step_gamma not positive, maxit outside 1..1e7, NaN tol,
 * null pointers with n_edges > 0, and - after one small device pass - a NaN or negative entry of z.  n_edges = 0
 * returns at once with niter 0 (and an empty adjacency).  Three launches per iteration (edge pass, vertex pass, a
 * one-workgroup rule kernel), the done flag read by the host every 4 iterations, no atomics: the same inputs give the
 * same bits on every call. */
int gspx_edge_sqdist_dev(gspx_graph* g, int64_t F, const void* x_dev, void* z_dev, double* kernel_ms);
int gspx_learn_log_degrees_dev(gspx_graph* g, const void* z_dev, double a, double b, double step_gamma, double tol,
                               int64_t maxit, const void* w0_dev, void* p_dev, void* w_dev, gspx_knn** w_out,
                               int64_t* niter, int32_t* crit, double* history_host, double* kernel_ms);

/* Space-filling-curve keys of N points (coords: N x d doubles on the HOST, d >= 2; the first two /
 * three axes are used): curve 0 = Morton, 1 = Hilbert (2-D).  The engine's internal vertex order
 * for graphs with coordinates is the stable argsort of these keys (pygsp_amd.engine.locality_order). */
int gspx_curve_keys(gspx_ctx* ctx, int64_t N, int d, const double* coords, int curve, uint64_t* keys);

/* The vertex order itself: the stable argsort of those keys (what numpy.argsort(keys, kind="stable") returns),
 * by a radix sort on the device.  perm[new] = old, N int32 on the HOST. */
int gspx_curve_order(gspx_ctx* ctx, int64_t N, int d, const double* coords, int curve, int32_t* perm);

/* Graph set-up in ONE call, on the device: what pygsp/graphs/graph.py:98-176 (the checks of Graph.__init__),
 * Graph.is_directed (graph.py:357-405) and Graph.compute_laplacian (graph.py:510-630) do to W, plus this engine's
 * own preparation (CSR validation, curve order of the vertices and its locality score).  W (host CSR; data_dtype
 * GSPX_F32, GSPX_F64 or 2 = int64) is uploaded once and inspected in place; coords (N x d doubles on the HOST,
 * nullable) feed the internal order: order_mode 0 none, 1 auto (Hilbert in 2-D / Morton in 3-D, kept only when
 * it beats the graph's own order by 0.05 of locality score), 2 Morton, 3 Hilbert, 4 the permutation perm_in.
 * report[12]: [0] NaN entries, [1] infinite, [2] negative, [3] explicit zeros, [4] non-zero diagonal entries
 * (self-loops), [5] entries that differ from their mirror entry, a mirror that is not stored counting as zero
 * (> 0: W - W.T has a nonzero = Graph.is_directed), [6] CSR violations,
 * [7] 1 when an internal order is in use, [8] / [9] locality score x 1e9 of the graph's own / the curve order
 * (auto mode), [10] 0 = graph built, 1 = not built, [11] microseconds of the whole call.
 * NaN / inf / CSR violations: GSPX_ERR_INVALID with the reference's message.  A directed graph, or explicit zeros:
 * the Laplacian is built from (W + W.T) / 2 without stored zeros - utils.symmetrize(W, 'average'), graph.py:613-616,
 * utils.py:247-248; graph.py:126-128 - prepared on the device in the same call (transpose by radix sort, row merge;
 * degrees = its row sums = (in + out) / 2, graph.py:834-837); the caller keeps W itself (and drops its zeros).
 * Only a union pattern beyond 32-bit indices returns GSPX_OK with *out == NULL and report[10] == 1. */
int gspx_graph_setup(gspx_ctx* ctx, int64_t N, int64_t nnz, const int32_t* indptr, const int32_t* indices,
                     const void* data, int data_dtype, int lap_type, int compute_dtype, const double* coords,
                     int d, int order_mode, const int32_t* perm_in, int64_t report[12], gspx_graph** out);
/* The same set-up for the W a device builder left on the device (gspx_knn_build / gspx_radius_build /
 * gspx_sbm_build; the handle stays valid and still serves gspx_knn_download_w): the generator classes NNGraph /
 * Sensor / StochasticBlockModel / ErdosRenyi (nngraph.py:289-313, stochasticblockmodel.py:144-181 end in
 * Graph.__init__(W)) hand the builder's handle over - no download and re-upload of W; its host copy is made
 * when somebody reads G.W.  coords may be NULL (order_mode 0 or 4).  report / *out as gspx_graph_setup.
 * coords of both set-ups: 1 to 64 columns, of which a curve reads the first two (Hilbert) or three (Morton) - the
 * builders take up to 4096, so for a wider cloud the caller hands over its leading columns only
 * (engine.DeviceGraph._order_args does). */
int gspx_graph_setup_from_knn(gspx_knn* h, int lap_type, int compute_dtype, const double* coords, int d,
                              int order_mode, const int32_t* perm_in, int64_t report[12], gspx_graph** out);
/* The ingredients of Graph._get_upper_bound (graph.py:933-960: the smallest of four classical upper bounds of
 * lambda_max of the combinatorial Laplacian), taken in one pass while W was on the device - float64 graphs built
 * from W: out[0] max W_ij, out[1] max dw, out[2] max (dw_i + dw_j) over the stored entries, out[3] max (dw_i +
 * (W dw)_i / dw_i), NaN when a vertex has degree zero (numpy's 0 / 0; the reference's min() then ignores it).
 * The bounds are N out[0], 2 out[1], out[2], out[3]. */
int gspx_graph_lmax_bounds(gspx_graph* g, double out[4]);
/* the internal vertex order of a graph (perm[new] = old); GSPX_ERR_INVALID when it has none */
int gspx_graph_download_perm(gspx_graph* g, int32_t* perm);

/* Connected components of the graph's undirected pattern - the off-diagonal stored entries of its Laplacian, read in
 * both directions - labelled on the device (Graph.is_connected / extract_components, graph.py:294-366, 444-508;
 * scipy.sparse.csgraph.connected_components(W, directed=False)).  labels_dev: N int32 (DEVICE, caller's vertex order)
 * or NULL when only the count is wanted; vertex v gets the number 0 .. *n_components - 1 of its component,
 * components numbered by their smallest vertex (scipy's numbering).  Isolated vertices are components of their own,
 * self-loops never matter, N = 0 gives 0 components; fp32 and fp64 graphs, every vertex order.  The pattern is the
 * Laplacian's: a normalized Laplacian of a graph with negative weights has lost the rows of vertices whose weights
 * cancel (graph.py:621-628), the caller labels such a W itself.  Hook-to-the-smaller-label rounds with pointer
 * shortening; *rounds (nullable): how many ran, at most the cap gspx_components_round_cap(N) = 2 ceil(log2 N) + 1
 * (derived in gspx_components.hip.h) - labels that still change then are GSPX_ERR_INTERNAL, never a longer loop.
 * kernel_ms (nullable): device time of the whole call.  gspx_graph_components: the same with a HOST labels array. */
int gspx_graph_components_dev(gspx_graph* g, int32_t* labels_dev, int64_t* n_components, int* rounds,
                              double* kernel_ms);
int gspx_graph_components(gspx_graph* g, int32_t* labels_host, int64_t* n_components, int* rounds, double* kernel_ms);
int gspx_components_round_cap(int64_t N, int* cap);

/* Spring layout (Fruchterman-Reingold; Graph.set_coordinates('spring'), pygsp/graphs/_layout.py:169-219) iterated on
 * the device.  A_ij = 1 where the graph's Laplacian stores an off-diagonal entry (i, j) - only the pattern is read, so
 * fp32 and fp64 graphs both work, and the caller has ruled out what the pattern does not show (a directed W, negative
 * weights).  dim 2 or 3; pos_dev: N x dim fp64 (DEVICE, caller's vertex order), start positions in, result out;
 * fixed_dev: N uint8 (DEVICE, caller's order; nonzero = the vertex never moves, bit for bit) or NULL.  Iteration it =
 * 0 .. iterations - 1 runs at temperature t_it, t_0 = t0 and t_{it+1} = t_it - dt in fp64 (the reference: t0 = 0.1, dt =
 * t0 / (iterations + 1)): for every vertex i that is not fixed disp_i = sum over ALL j of (pos_i - pos_j) (k^2 / d^2 -
 * A_ij d / k), d = max(||pos_i - pos_j||, 0.01); then pos_i += disp_i t / len_i, len_i = ||disp_i|| replaced by 0.1
 * where < 0.01, every position after all displacements.  One step at a given temperature (iterations = 1) and the
 * continuation of a longer run are the same call.  The all-pairs sum is exact (no grid, no tree) and every sum has a
 * fixed order: the same inputs give the same bits on every call for a given split count - gspx_layout_splits: what the
 * call uses for this graph, derived from N and the CU count unless the context option "layout_splits" (> 0) forces it.
 * iterations = 0 and N = 0 leave pos untouched; dim outside {2, 3}, k <= 0, iterations < 0, a non-finite k / t0 / dt:
 * GSPX_ERR_INVALID.  kernel_ms (nullable): device time of the whole call. */
int gspx_layout_spring_dev(gspx_graph* g, int dim, double k, const void* fixed_dev, int64_t iterations, double t0,
                           double dt, void* pos_dev, double* kernel_ms);
int gspx_layout_splits(gspx_graph* g, int64_t* splits);

/* The full Fourier basis on the device: every eigenpair of a dense symmetric fp64 matrix by two-sided cyclic block
 * Jacobi (blocks of 32, 64 x 64 subproblems solved in LDS by scalar rotations, updates on the matrix cores).
 * A: n x n (DEVICE, row-major, leading dimension lda), symmetric - the subproblems read (S + S^T) / 2 -; only read.
 * V (DEVICE out, n x n, leading dimension ldv): orthonormal eigenvectors in columns, ascending eigenvalue; entries
 * beyond column n of a row are left alone.  e_host (HOST out): the n eigenvalues, ascending, Rayleigh quotients of the
 * returned columns.  A sweep rotates every block pair once (gspx_sym_eig_schedule_describe); pairs whose 64 x 64 block
 * is already diagonal to the tolerance are skipped.  Before each sweep: stop when off(A) <= tol ||A||_F and no row's
 * off-diagonal norm exceeds tol max |a_ii| (off: the square root of the sum of the squared off-diagonal entries,
 * summed directly).  After max_sweeps sweeps without that: GSPX_ERR_NOCONV, V and e_host unspecified, the library
 * usable.  The finish orders the columns, takes one Newton-Schulz step V (3 I - V^T V) / 2 and forms the Rayleigh
 * quotients.  No atomics: the same inputs give the same bits.  info (HOST, 12 doubles, nullable): [0] sweeps,
 * [1] final off(A) / ||A||_F, [2] pairs rotated, [3] pairs skipped, [4..8] device ms of the subproblems, the column
 * updates, the row updates, the off-norms and the finish, [9] wall ms of the call, [10] max_i ||A v_i - e_i v_i||_2,
 * [11] the largest entry of a returned column outside the first n rows of the padded work matrix (0: the padding
 * never mixed).  skipped_per_sweep (HOST, max_sweeps entries, nullable): pairs skipped in each sweep run.
 * n = 0: nothing to do.  n < 0, n > 32768, lda < n, ldv < n, null pointers with n > 0, tol <= 0, max_sweeps < 1,
 * V overlapping A, non-finite entries: GSPX_ERR_INVALID - all but the last before any device work. */
#define GSPX_ERR_NOCONV 7 /* an iteration used up its sweeps -> ValueError */
int gspx_sym_eig_dev(gspx_ctx* ctx, int n, const double* A, int64_t lda, double* V, int64_t ldv, double* e_host,
                     double tol, int max_sweeps, double* info, int64_t* skipped_per_sweep);
/* Host-only: the block pairs of one sweep over n_blocks blocks (1..1024), in the order the solver visits them.
 * *n_rounds = ceil(n_blocks / 2) * 2 - 1 rounds of floor(n_blocks / 2) disjoint pairs each (an odd count leaves one
 * block out per round); pairs_out (nullable): n_rounds * floor(n_blocks / 2) * 2 ints, (i, j) with i < j, round-major. */
int gspx_sym_eig_schedule_describe(int n_blocks, int* pairs_out, int* n_rounds);
/* X[:, c] *= s[c] for the w columns of an N-row fp64 panel (DEVICE, leading dimension ldx); s_host: w doubles (HOST).
 * The sign rule of a Fourier basis applied to its device copy, for widths beyond gspx_panel_combine_dev's 512. */
int gspx_panel_scale_cols_dev(gspx_ctx* ctx, int64_t N, double* X, int64_t ldx, int w, const double* s_host);

/* Columns [j0, j0 + w) of the N x N identity as a row-major N x w panel in device memory (dtype GSPX_F32 /
 * GSPX_F64), queued on the context's stream: the input of Filter.compute_frame (filter.py:593-600 filters
 * np.identity(N)) produced where it is consumed. */
int gspx_identity_panel_dev(gspx_ctx* ctx, int dtype, int64_t N, int64_t j0, int64_t w, void* out_dev);
/* Squared column norms of a filterbank applied to DEVICE signals, without its outputs: out (HOST, Nf x Nsig fp64)
 * [f][j] = sum_n ((p_f(L) x)[n][j])^2.  Arguments as gspx_cheby_filter_dev in analysis mode, M <= 256.  Every output
 * element is formed, squared and summed in fp64 for both graph dtypes; identical calls give identical bits.  With the
 * identity panels of gspx_identity_panel_dev: the row norms of Filter.compute_frame (pygsp.features.compute_norm_tig,
 * compute_spectrogram) without the frame. */
int gspx_cheby_sqnorms_dev(gspx_graph* g, double lmax, int Nf, int M, const double* coeffs, int64_t Nsig,
                           const void* x_dev, double* out, double* kernel_ms);
/* Chebyshev self-moments of DEVICE signals: out (HOST, M x Nsig fp64, row-major)
 *   out[k][j] = sum_n x[n][j] * (T_k(Lt) x)[n][j],  Lt = (L - a I)/a, a = lmax/2 (approximations.py:93-99), k < M.
 * x_dev as for gspx_cheby_filter_dev (N x Nsig, row-major, the graph's compute dtype, the caller's vertex order);
 * 2 <= M <= 2048.  L is symmetric, so T_i T_j = (T_{i+j} + T_{|i-j|}) / 2 yields M moments from floor(M / 2)
 * recurrence steps: the inner products <T_i, T_i> and <T_{i+1}, T_i> of the kept T_0 .. T_{floor(M/2)} are formed
 * in fp64 for both graph dtypes (k_slot_dots) and doubled on the host.  Identical calls give identical bits.  The
 * moments of random +-1 vectors are the kernel polynomial method's estimate of the density of states
 * (pygsp_amd.spectrum).  Nsig == 0: nothing happens; N == 0: zeros. */
int gspx_cheby_moments_dev(gspx_graph* g, double lmax, int M, int64_t Nsig, const void* x_dev,
                           double* out, double* kernel_ms);

/* Chebyshev CROSS-moments of DEVICE signals: out (HOST, Nf x M x Nsig fp64, row-major)
 *   out[f][k][j] = sum_n z[f][n][j] * (T_k(Lt) x)[n][j],  k < M,
 * the inner products of the recurrence on x with Nf foreign planes - what the derivative of a Chebyshev filter's output
 * with respect to its coefficients is made of (pygsp_amd.filters.cheby_op_vjp).  x_dev: N x Nsig; z_dev: Nf planes
 * [f][n][s] of N x Nsig; both row-major, the graph's compute dtype, the CALLER's vertex order.  2 <= M <= 256, Nf >= 1.
 * M - 1 recurrence steps (no doubling: z is not x); every product and sum is fp64 for both graph dtypes
 * (k_slot_cross_dots) and identical calls give identical bits.  z_dev == x_dev with Nf = 1 is legal (the self-moments,
 * the long way).  Nsig == 0: nothing happens; N == 0: zeros. */
int gspx_cheby_cross_moments_dev(gspx_graph* g, double lmax, int M, int64_t Nsig, const void* x_dev, int Nf,
                                 const void* z_dev, double* out, double* kernel_ms);
/* The device ordinal of a pointer, asked of the HIP runtime libgspx itself is bound to (hipPointerGetAttributes):
 * GSPX_OK and *device for device memory that runtime knows; GSPX_ERR_INVALID for anything else - host memory, a null
 * pointer, memory of ANOTHER HIP runtime loaded into the same process - with the runtime's error state cleared.
 * Launches nothing and touches no memory: the gate a binding puts in front of pointers it did not allocate. */
int gspx_ptr_device(const void* p, int* device);

/* Chebyshev graph convolution of DEVICE signals (the ChebNet layer; pygsp_amd.filters.cheby_conv, pygsp_amd.nn.ChebConv):
 *   y[n][b][:] = sum_{k < M} (T_k(Lt) x)[n][b][:] theta[k],   theta[k] a Fin x Fout matrix,
 * a PLAIN sum: theta[0] is not halved (theta[k] = c_k I for k >= 1 and theta[0] = (c_0 / 2) I gives gspx_cheby_filter_dev
 * of one filter c).  theta: HOST, M x Fin x Fout doubles, row-major, finite.  x_dev: N x B*Fin, y_dev: N x B*Fout;
 * row-major, the graph's compute dtype, the CALLER's vertex order, the feature index fastest: element (n, b, i) at
 * n*B*Fin + b*Fin + i.  M Clenshaw steps on panels of B*Fout columns - the steps of a synthesis call with one input
 * panel - each fed by one dense product x theta[k] on the matrix cores (k_group_mix), in the compute dtype.  Column
 * batches hold whole samples.  L is symmetric: the same call with every theta[k] transposed (Fin and Fout swapped) is
 * the derivative with respect to x.
 * GSPX_ERR_COEFF for M < 2; GSPX_ERR_INVALID for M > 256, Fin or Fout outside 1..128, B < 0, lmax not positive and
 * finite (all checked before the graph is looked at), a null graph or pointer, x_dev == y_dev, a non-finite theta, or
 * B*max(Fin, Fout) beyond the signal-count limit.  B == 0: nothing happens; N == 0: nothing is written. */
int gspx_cheby_conv_dev(gspx_graph* g, double lmax, int M, int Fin, int Fout, const double* theta, int64_t B,
                        const void* x_dev, void* y_dev, double* kernel_ms);
/* The cross-Grams of the recurrence on x with a second signal z: out (HOST, M x Fin x Fout fp64, row-major)
 *   out[k][i][o] = sum_{n, b} (T_k(Lt) x)[n][b][i] * z[n][b][o],   k < M,
 * the derivative of gspx_cheby_conv_dev's output with respect to theta when z is the cotangent.  x_dev: N x B*Fin,
 * z_dev: N x B*Fout, laid out as above.  M - 1 recurrence steps into M kept slots, then one Gram product per slot on the
 * fp64 matrix cores (k_slot_cross_gram): every product and sum is fp64 for both graph dtypes, there are no atomics, and
 * identical calls give identical bits.  Column batches hold whole samples; their Grams are added in batch order.
 * Errors as gspx_cheby_conv_dev (no theta, and z_dev may be x_dev).  B == 0: nothing happens; N == 0: zeros. */
int gspx_cheby_cross_grams_dev(gspx_graph* g, double lmax, int M, int Fin, int Fout, int64_t B, const void* x_dev,
                               const void* z_dev, double* out, double* kernel_ms);

/* The derivative of a Chebyshev filter's output with respect to the entries of the Laplacian, at FIXED lmax and with
 * the entries taken as independent (pygsp_amd.filters.cheby_op_vjp_weights, pygsp_amd.nn.WeightedGraph).  For
 *   y_f = c_f0/2 x + sum_{k >= 1} c_fk T_k(Lt) x,  Lt = (2/lmax) L - I,  and cotangent planes z_f = dl/dy_f:
 *   Gbar = dl/dL = (2/lmax) sum_{k=1}^{M-1} phi_k b_k t_{k-1}^T,   phi_1 = 1, phi_k = 2 otherwise,
 * t_k = T_k(Lt) x and b_k the Clenshaw sequence of the cotangent (b_k = sum_f c_fk z_f + 2 Lt b_{k+1} - b_{k+2}).  Two
 * restrictions of Gbar are written, both summed over the signal columns:
 *   gdiag_dev[i] = Gbar_ii (N doubles);   goff_dev[p] = Gbar_st + Gbar_ts for vertex couple p = (s, t) of a list.
 * coeffs: HOST, Nf x M, as for gspx_cheby_filter_dev, 2 <= M <= 256.  x_dev: N x Nsig; z_dev: Nf planes [f][n][s] as
 * for gspx_cheby_cross_moments_dev; both the graph's compute dtype, the CALLER's vertex order.  src_dev / dst_dev:
 * DEVICE int32 arrays of n_pairs vertices each, the caller's vertex order, either orientation, repeats allowed, edges
 * of the graph or not (for a non-edge: the derivative with respect to giving it weight).  src_dev == NULL (then
 * dst_dev must be NULL and n_pairs is ignored): the graph's own edge list, the order of Graph.get_edge_list, goff_dev
 * of gspx_graph_n_edges entries.  gdiag_dev and goff_dev are DEVICE fp64 buffers for both graph dtypes, OVERWRITTEN;
 * either may be NULL.  Per column batch: M - 2 recurrence steps into M - 1 kept slots, M - 1 Clenshaw steps, and after
 * each the two bandwidth kernels k_pair_cross / k_row_cross; products and sums are fp64, there are no atomics, later
 * batches add in batch order on one stream, and identical calls give identical bits.
 * GSPX_ERR_INVALID for what gspx_cheby_cross_moments_dev refuses, sources without targets (or the reverse), a negative
 * n_pairs, null or non-finite coefficients (all checked before the graph is looked at), a graph whose edge list cannot
 * be built when it is asked for, and - found by one device pass before anything is written - a vertex outside
 * 0 .. N-1 or a couple with s == t.  Nsig == 0 or N == 0: zeros. */
int gspx_cheby_laplacian_grad_dev(gspx_graph* g, double lmax, int Nf, int M, const double* coeffs, int64_t Nsig,
                                  const void* x_dev, const void* z_dev, int64_t n_pairs, const int32_t* src_dev,
                                  const int32_t* dst_dev, double* gdiag_dev, double* goff_dev, double* kernel_ms);

/* PCI address ("0000:c1:00.0", NUL-terminated) of HIP device `device`: what a host driver needs to find the NUMA
 * node the GPU hangs off (/sys/bus/pci/devices/<address>/numa_node) and pin the thread - and the packing threads
 * libgspx starts from it - that feeds this GPU to the cores next to it (pygsp_amd.multi). */
int gspx_device_pci_bus_id(int device, char* out, int capacity);

/* A signal cube between its two layouts, on the device (queued on the context's stream): the row-major
 * (N, S, F) tensor Filter.filter takes and returns (filter.py:146-328: vertices x signals x features) and the F
 * feature planes [f][n][s] the engine works on (the (Nf N, Nsig) stacking of approximations.py:88,
 * filter.py:315-316).  to_planes != 0: src is the cube, dst the planes; 0: the other way.  Needed only when a
 * device-resident array arrives in the other layout than the call reads it in (an (N, Nf) panel of Nf signals
 * taken as ONE signal with Nf features, filter.py:270-278). */
int gspx_planes_pack_dev(gspx_ctx* ctx, int dtype, int64_t N, int64_t S, int64_t F, const void* src_dev,
                         void* dst_dev, int to_planes);

/* Host-only: the step schedule the engine would run for (Nf, M) under the ctx's current
 * options, for CPU-side verification of the schedule logic (no device work).  Each of the
 * K = M-1 rows of `plan` is 4 + 3*Nf doubles:
 *   [scale, gamma, flush (0 none / 1 write / 2 accumulate), final (0/1),
 *    then for each filter f: w_new, w_cur, w_old]
 * `plan` must hold (M-1)*(4+3*Nf) doubles.  a1 = a2 = lmax/2 as approximations.py:93-96. */
int gspx_plan_describe(gspx_ctx* ctx, int Nf, int M, const double* coeffs, double* plan);
/* Host-only: the signal-column batches (widths[0 .. *n_batches), they add up to Nsig; 0 batches = the one-shot
 * form) and the host threads per direction the pipelined gspx_cheby_filter would use for a call of N x Nsig
 * elements of `dtype` with `planes_total` = Nf + 1 panels, under the options "host_pipeline" (mode),
 * "host_batch", "host_edge", "host_threads". */
int gspx_host_pipeline_describe(int mode, int64_t host_batch, int64_t host_edge, int64_t host_threads, int dtype,
                                int64_t N, int64_t Nsig, int planes_total, int64_t* widths, int capacity,
                                int* n_batches, int* threads);

/* Stage times of the LAST gspx_cheby_filter call on this context (milliseconds): out[0] wall time of the
 * pipelined call, out[1] packing (busiest host thread), out[2] host-to-device DMA (sum over batches), out[3]
 * kernels (sum of device times), out[4] device-to-host DMA, out[5] unpacking (busiest host thread), out[6]
 * batches (0: the call was not pipelined), out[7] signals per batch, out[8] host threads per direction. */
int gspx_last_host_timing(gspx_ctx* ctx, double out[9]);
/* Which step kernels the LAST gspx_cheby_filter*, gspx_newton_filter* or gspx_poly_program* call on this context
 * launched: out[0] launches of the LDS-staged tile kernel (k_step_tile), out[1] launches of the plain step kernels.
 * Counted on the host where the launches are issued (no kernel takes part, no device traffic); zeroed where the
 * call's timings are; summed over the column batches of a call, pipelined host-array calls included.  A replayed
 * recurrence call (option "graph_launch") issues no launch: it reports the counts stored with its recording.  Other
 * entry points that use a step kernel (gspx_laplacian_apply_dev, gspx_lanczos_lmax, ...) add to the counts without
 * zeroing them: read the counts right after the call they are about. */
int gspx_last_step_kinds(gspx_ctx* ctx, int64_t out[2]);
/* Host clock of the last pipelined gspx_cheby_filter, per batch, in ms since the call began: [6 b + 0] packed,
 * [+1] H2D issued, [+2] kernels begun, [+3] kernels done, [+4] D2H done, [+5] unpacked.  *batches: how many there
 * were; out (capacity doubles) may be NULL. */
int gspx_last_host_timeline(gspx_ctx* ctx, double* out, int capacity, int* batches);

/* Calibration: read+write GB/s of the engine's 16-byte-per-lane streaming copy kernel over two
 * `bytes`-sized buffers (the measured HBM ceiling reported beside roofline fractions). */
int gspx_bench_copy(gspx_ctx* ctx, int64_t bytes, int iters, double* gbps);

/* Calibration: read-only GB/s of a `bytes`-sized buffer streamed `passes` times in one launch. */
int gspx_bench_read(gspx_ctx* ctx, int64_t bytes, int passes, double* gbps);

/* Placement tuning of a context's streamed workspaces for one single-filter analysis call (the arguments of
 * gspx_cheby_filter_dev with Nf = 1): `candidates` (1-32) physical backings are drawn - the previous ones held meanwhile,
 * so every draw gets other pages -, the call itself runs three times on each, the fastest stays in the context and
 * the others are released.  Why: on MI355X the recurrence on panels beyond the Infinity Cache runs 0.54-0.60 of 8 TB/s
 * depending on which physical pages back its work panels, and what a process draws first it keeps
 * (profiles/r06_placement.md).  out[i]: ms per recurrence launch with candidate i (0: the backing the context already
 * had, if any; 0: never drawn, memory ran out); out[candidates]: index kept.  stride_mb > 0: a pad of that many MB is
 * allocated and held before every further draw (released at the end), so that the candidates sample the card's memory at
 * that stride - fast and slow pages come in zones of tens of GB in allocation order.  y_dev holds the call's result
 * afterwards; results are bit-identical whichever backing is kept. */
int gspx_ctx_tune_placement(gspx_graph* g, double lmax, int M, const double* coeffs, int64_t Nsig, const void* x_dev,
                            void* y_dev, int candidates, int64_t stride_mb, double* out);

/* Calibration: total GB/s of n_read (0-4) read streams and n_write (0-2) write streams of bytes_per_stream each, walked
 * together by workgroups_per_cu persistent workgroups per CU, 16 bytes per lane (nt: bit 0 non-temporal loads, bit 1
 * non-temporal stores, bit 2 write stream w overwrites read stream w in place, bit 3 the recurrence step's walk - every
 * workgroup takes 32 KB blocks of its XCD's eighth of every stream - instead of a grid-stride sweep, bit 4 the streams lie
 * in the context's own T workspace instead of fresh allocations - GSPX_ERR_INVALID when it is smaller) - what the memory
 * system delivers to a read : write ratio with nothing else in the way. */
int gspx_bench_streams(gspx_ctx* ctx, int64_t bytes_per_stream, int n_read, int n_write, int nt, int workgroups_per_cu,
                       int iters, double* gbps);

/* Calibration, the MIX CEILING of the LDS-staged recurrence step: exactly the call
 * gspx_cheby_filter_dev(g, lmax, 1, M, coeffs, Nsig, x_dev, y_dev, GSPX_ANALYSIS, NULL) would make - the same plan, the
 * same M-1 k_step_tile launches on the same grid over the same buffers, the same LDS-DMA tile loads of the same row
 * lists, the same T_{k-2} / accumulator loads, entry stream, stores, flush steps, sweep directions and cache bits - with
 * the ARITHMETIC REMOVED from every launch: the per-entry LDS gathers and multiply-adds of the row products are
 * replaced by one tile read per row.  mode 1 keeps the two workgroup barriers of a pass, mode 2 drops them as well
 * (the access mix alone).  y_dev receives numbers without meaning.  Times are read with gspx_last_timing as after
 * any filter call.  Only for calls that run the wide builds (gather tiles, rows of more than 128 bytes); the one
 * launch per call that reads T_{k-2} from the caller's unpermuted panel (step 2, "fuse_input") runs unmodified.
 * What it answers: step time == mix time  =>  the step is bound by the memory system serving this access mix (on
 * this box), not by its arithmetic or LDS traffic; step time > mix time  =>  the compute phase is exposed. */
int gspx_bench_step_mix(gspx_graph* g, double lmax, int M, const double* coeffs, int64_t Nsig, const void* x_dev,
                        void* y_dev, int mode);

/* Calibration for graphs WITHOUT vertex locality (BASELINE configs 2, 3: Erdos-Renyi, block model): the rate
 * of random row gathers, measured with nothing else in the way.  n_gathers rows of row_bytes (64 / 128 / 256 /
 * 512; 16 bytes per lane, the step kernels' lane layout) are fetched from a panel of panel_rows rows by 32-bit
 * indices, in_flight (2 / 4 / 8 / 16) independent gathers per lane before the first use; no matrix values, no
 * FMA, no panel writes.  blocks == 1: indices uniform over the panel (ER); blocks > 1: the panel is cut into
 * that many row ranges and a gather lands in the range of the row it is issued "from" with probability p_intra
 * (SBM), each XCD walking a contiguous eighth of the stream; blocks == 0: UNIQUE rows - panel_rows a power of two,
 * n_gathers <= panel_rows, every row fetched at most once per launch in a scattered order (known bytes and no reuse:
 * the calibration of the fabric counters on gathers, tools/gather_calibration.py).  ms: per launch; gbps: row bytes
 * per second. */
int gspx_bench_gather(gspx_ctx* ctx, int64_t panel_rows, int row_bytes, int64_t n_gathers, int in_flight,
                      int blocks, double p_intra, int workgroups_per_cu, int iters, double* ms, double* gbps);

/* What RCCL itself reports, for self-validating multi-GPU records (bench.py --gpus N): out[0] RCCL version code
 * (ncclGetVersion, e.g. 22203; 0 when RCCL cannot be loaded), out[1] ranks the communicator spans as the communicator
 * says (ncclCommCount) - for comm == NULL the device set of this process's last RCCL gspx_gather (0: none ran) -,
 * out[2] this handle's rank (ncclCommUserRank; -1 for NULL). */
int gspx_comm_info(gspx_comm* comm, int64_t out[3]);

/* k-means on a row-major fp64 device panel X (N x d, pitch ldx >= d doubles): pygsp_amd/clustering.py.  Limits:
 * 1 <= d <= 128, 1 <= C <= min(N, 1024), C * d <= 8192 (64 KiB of centroids; the assignment kernel keeps them in LDS
 * at a padded pitch, up to 91 456 bytes with its staging and reduction space, the update kernel up to 79 872 bytes);
 * anything else is GSPX_ERR_INVALID.  Squared distances are acc = acc + (x_j - c_j) * (x_j - c_j), j = 0 .. d - 1, without FMA; every sum
 * has one fixed order, no atomics, the same bits on every call.
 *
 * gspx_kmeans_block_rows: update_rows = the rows per block of the update's and the seeding's partial sums (a constant),
 * assign_rows = the rows per workgroup of the assignment kernel, whose partial inertia is summed per workgroup (a
 * function of d alone).  Needs no device.
 *
 * gspx_kmeans_dev: Lloyd's iteration from the C x d centroids in `cent` (device, dense rows; overwritten with the
 * result).  Assign; stop converged when no label changed (the first assignment counts every row); stop unconverged
 * when max_iter updates have been made; else update and repeat.  labels (device, N int32), mind (device, N doubles or
 * NULL: each row's squared distance to its centroid) and *inertia belong to the returned centroids; *n_iter = updates
 * made.  A cluster without members keeps its centroid.
 *
 * gspx_kmeans_seed_dev: k-means++ from C host draws u[c] in [0, 1): the chosen rows are copied to `cent` (device,
 * C x d) and their indices to `chosen` (host).  The rule is stated above the function in csrc/gspx_cluster.hip.h.
 *
 * gspx_rows_normalize_dev: in place, each row divided by the square root of acc = acc + x_j * x_j; a zero row stays
 * (any d >= 1). */
int gspx_kmeans_block_rows(int d, int* update_rows, int* assign_rows);
int gspx_kmeans_dev(gspx_ctx* ctx, int64_t N, int d, int C, const double* X, int64_t ldx, double* cent,
                    int64_t max_iter, int32_t* labels, double* mind, double* inertia, int64_t* n_iter,
                    int32_t* converged, double* kernel_ms);
int gspx_kmeans_seed_dev(gspx_ctx* ctx, int64_t N, int d, int C, const double* X, int64_t ldx, const double* u,
                         double* cent, int64_t* chosen, double* kernel_ms);
int gspx_rows_normalize_dev(gspx_ctx* ctx, int64_t N, int d, double* X, int64_t ldx, double* kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* GSPX_EXT_H */
