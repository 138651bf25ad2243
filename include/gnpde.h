/*
 * gnpde.h — C ABI of the MI355X-native GRAND/BLEND ODE right-hand side.
 *
 * One shared library, libgnpde.so (graph-neural-pde_amd/gnpde/), built with
 * `hipcc --offload-arch=gfx950`.  Plain pointers and sizes only; no torch
 * types.  Every device pointer is owned by the caller (the Python host passes
 * torch tensors' data_ptr()); the library never allocates device memory and
 * keeps no state besides its kernels.  Every call enqueues on the caller's
 * `stream` (a hipStream_t passed as void*; NULL = legacy default stream) and
 * never synchronises, except gnpde_plan_build, which is documented as a
 * once-per-graph synchronous call.  All calls are graph-capturable except
 * gnpde_plan_build.
 *
 * Return codes: 0 ok, GNPDE_EINVAL (-1) invalid argument, GNPDE_EHIP (-2) HIP
 * runtime error, GNPDE_EUNSUPPORTED (-3) unsupported shape/dtype.  The message
 * of the last failure on the calling thread is returned by gnpde_last_error().
 *
 * Reference interfaces replaced (alimt1992/graph-neural-pde @ 2025-01-17):
 *   - the per-RHS COO->dense->matmul of LaplacianODEFunc.sparse_multiply,
 *     src/function_laplacian_diffusion.py:39-58, and of
 *     ODEFuncTransformerAtt.multiply_attention, src/function_transformer_attention.py:33-41;
 *   - the RHS epilogue f = sigma(alpha)(ax - x) [+ beta x0],
 *     src/function_laplacian_diffusion.py:69-77, src/function_transformer_attention.py:52-59;
 *   - SpGraphTransAttentionLayer.forward's Q/K projections, gathers, scaled_dot
 *     score and edge softmax, src/function_transformer_attention.py:224-266 and
 *     utils.softmax, src/utils.py:116-127;
 *   - the torchdiffeq stage combinations y0 + dt*sum(b_j k_j) the solver does
 *     between RHS calls (src/block_constant.py:46-51 calls odeint).
 *
 * Layout: graphs are block-diagonal over the batch: global node id
 * r = b*N + n (b < B, n < N), R = B*N rows.  Node features are row-major
 * [R, C] with leading dimension ld (elements).  A "CSR" here is rowptr[R+1],
 * col[nnz] (global node ids), perm[nnz] (CSR position -> COO edge id b*E+e).
 * Grouping by source (edge_index[:,0]) gives the aggregation CSR; grouping by
 * destination (edge_index[:,1]) gives the CSC used for destination-grouped
 * softmax (attention_norm_idx = 1).
 */
#ifndef GNPDE_H_
#define GNPDE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNPDE_ABI_VERSION 8

#define GNPDE_OK 0
#define GNPDE_EINVAL (-1)
#define GNPDE_EHIP (-2)
#define GNPDE_EUNSUPPORTED (-3)

/* flags for the RHS epilogue */
#define GNPDE_EPI_PLAIN 0          /* f = ax                                   */
#define GNPDE_EPI_RHS 1            /* f = a*(ax - x) [+ b*x0]                  */
#define GNPDE_ALPHA_SIGMOID 2      /* a = sigmoid(*alpha) instead of *alpha    */
#define GNPDE_ADD_SOURCE 4         /* add b*x0 (b = *beta)                      */
#define GNPDE_LIVE_ITEMS 8         /* a hint, no arithmetic: the launch runs the live items of a graph in the node
                                      layout's numbering (rows by in-degree, the frozen rows of an rk4 solve left
                                      out): the launches measured to gain from column stripes */

/* score modes of the attention RHS (function_transformer_attention.py:246-259) */
#define GNPDE_SCORE_REFERENCE 0    /* fork scaled_dot: q_src . (sum_e' k_dst(e')) / sqrt(dk)      */
#define GNPDE_SCORE_DOT 1          /* per-edge scaled_dot: q_src . k_dst / sqrt(dk) (upstream)    */
#define GNPDE_SCORE_EXP_KERNEL 2   /* ov^2 exp(-|q_src - k_dst|^2 / (2 ls^2))                     */
#define GNPDE_SCORE_COSINE 3       /* cosine similarity, eps 1e-5                                 */
#define GNPDE_SCORE_PEARSON 4      /* centred cosine similarity                                   */
#define GNPDE_SCORE_UNIFORM 5      /* every score 0: the fork's scaled_dot under source-grouped    */
                                   /* softmax (norm_idx 0), where all scores of a group are equal  */
#define GNPDE_SCORE_GAT 6          /* GAT (function_GAT_attention.py:131-134): LeakyReLU(sl[src,h] + */
                                   /* sr[dst,h]); cs = the node-score pairs [R, 2*heads] fp64      */
                                   /* = [sl | sr] (gnpde_gat_scores_f32), score_p0 = the slope;    */
                                   /* heads <= 8; q, k unused.  Taken by gnpde_softmax_stats_f32,   */
                                   /* gnpde_seg_softmax_f32 (out_kind 1, either grouping, plans     */
                                   /* with hub / long items), gnpde_attn_weights_f32 and            */
                                   /* gnpde_edge_attention_f32.                                     */

int gnpde_abi_version(void);
const char* gnpde_last_error(void);
/* Hash of the sources the library was built from (graph-neural-pde_amd/srchash.py). */
const char* gnpde_build_id(void);

/* ---------------------------------------------------------------- graph build
 * COO edge_index [B,2,E] (int64, values in [0,N) — caller-validated) -> CSR
 * grouped by row `key_row` (0 = source, 1 = destination).  Stable: inside a
 * row, edges keep their COO order.  Replaces the per-call index building of
 * function_laplacian_diffusion.py:41-44 (done once per graph here).         */
size_t gnpde_csr_workspace_bytes(int64_t B, int64_t E, int64_t N);
int gnpde_csr_build(const int64_t* edge_index, int64_t B, int64_t E, int64_t N, int key_row,
                    int32_t* rowptr, int32_t* col, int32_t* perm,
                    void* workspace, size_t workspace_bytes, void* stream);

/* rowidx[p] = the row of CSR position p (once per graph; drives the
 * edge-parallel attention-weight kernels).                                   */
int gnpde_csr_rowidx(const int32_t* rowptr, int64_t R, int64_t nnz, int32_t* rowidx, void* stream);

/* w_out[p] = mean_{h<H} w_in[perm[p]*H + h]  (H = 1: plain permutation).
 * Head-mean of attention weights, function_laplacian_diffusion.py:45-49.    */
int gnpde_gather_weights_f32(const float* w_in, int64_t nnz, int H, const int32_t* perm, float* w_out,
                             void* stream);

/* ---------------------------------------------------------------- block weight producers
 * out[i] = mean_{h<H} att[i*H + h]  (H = 1: copy), and when gamma != NULL
 * out[i] = mean * (1 - sigmoid(*gamma)) + ew[i] * sigmoid(*gamma)  (COO order,
 * n = B*E).  gamma is a device scalar (pre-sigmoid).  Replaces
 * MixedODEblock.get_mixed_attention, src/block_mixed.py:29-33, and the
 * head mean of HardAttODEblock.forward, src/block_transformer_hard_attention.py:42,60. */
int gnpde_mix_weights_f32(const float* att, int H, const float* ew, const float* gamma, int64_t n, float* out,
                          void* stream);

/* w_out[e] = w_in[e] / (sum of w_in over e's group + 1e-16), groups = the rows
 * of a grouped CSR (rowptr[R+1], perm[nnz] = CSR position -> COO edge id),
 * COO order in and out; fixed summation order (deterministic).  Replaces
 * HardAttODEblock.renormalise_attention, src/block_transformer_hard_attention.py:32-35.
 * ABI 7: a workspace of gnpde_group_normalize_workspace_bytes(nnz) (the weights in
 * group order, so each group's sum streams a contiguous run). */
size_t gnpde_group_normalize_workspace_bytes(int64_t nnz);
int gnpde_group_normalize_f32(const int32_t* rowptr, const int32_t* perm, int64_t R, int64_t nnz, const float* w_in,
                              float* w_out, void* workspace, size_t workspace_bytes, void* stream);

/* *out = torch.quantile(v[0:n], q) (linear interpolation; rank q*(n-1) in
 * fp32, ATen's lerp) written to DEVICE memory; radix sort into the workspace.
 * The attention-sampling threshold of src/block_transformer_hard_attention.py:52. */
size_t gnpde_quantile_workspace_bytes(int64_t n);
int gnpde_quantile_f32(const float* v, int64_t n, double q, float* out, void* workspace, size_t workspace_bytes,
                       void* stream);

/* The training-mode attention sampling as a weight mask over the full edge list
 * (src/block_transformer_hard_attention.py:52-55): out[i] = v[i] > *thr ? v[i] : 0,
 * *count (device int64) = the retained edges.  With these weights the RHS over the
 * full graph equals the RHS over the compacted edge list (zero weights add exact
 * zeros), so a training forward needs no new CSR / plan.  thr: device (the
 * gnpde_quantile_f32 output).                                                 */
int gnpde_threshold_mask_f32(const float* v, int64_t n, const float* thr, float* out, int64_t* count, void* stream);
/* The sampled graph of HardAttODEblock training over a work plan (ABI 7;
 * src/block_transformer_hard_attention.py:52-56 keeps the edges above the
 * threshold and integrates over that edge list): for every plan item
 * {row, edge_begin, edge_end, slot} of gnpde_plan_build, the positions of
 * [edge_begin, edge_end) whose weight w (grouped order, e.g. gnpde_threshold_mask_f32
 * then gnpde_gather_weights_f32) is nonzero are written, in order, to
 * col_out / w_out from edge_begin on, and items_out = {row, edge_begin,
 * edge_begin + kept, slot}.  Launching K1 with items_out / col_out / w_out (and the
 * plan's heavy entries unchanged) aggregates the retained edges only, in the
 * order and hub chunks of the full plan: the same result as the masked full graph.
 * No host synchronisation; outputs the size of the inputs; no aliasing.        */
int gnpde_compact_items_f32(const int32_t* items, int64_t n_items, const int32_t* col, const float* w,
                            int32_t* col_out, float* w_out, int32_t* items_out, void* stream);

/* deg[r] = #{p : idx[p] == r}, r < R (memset + integer atomics: deterministic).
 * With idx = the aggregation CSR's col this is the in-degree used by the
 * reference-mode key sum.                                                   */
int gnpde_indegree_i32(const int32_t* idx, int64_t nnz, int64_t R, int32_t* deg, void* stream);

/* ---------------------------------------------------------------- graph normalisation
 * ODEblock.reset_graph_data (src/base_classes.py:70-90) with the intended
 * semantics of add_remaining_self_loops / get_rw_adj / gcn_norm_fill_val
 * (src/utils.py:16-42, :215-233, :177-194; pinned by test/test_utils.py:111-161
 * and test/test_function_laplacian_diffusion.py:56-86), once per graph.
 *
 * gnpde_self_loops_count: nonloop[b] = #{e : edge_index[b,0,e] != edge_index[b,1,e]}
 *   written to HOST memory (SYNCHRONOUS, like gnpde_plan_build).
 * gnpde_add_self_loops: per batch element, the K non-loop edges in COO order,
 *   then one loop (n, n) per node n < N whose weight is the weight of the node's
 *   LAST existing loop in COO order, or `fill` (w NULL: every weight 1).  K must
 *   be the same for every batch element (the [B,2,K+N] layout); outputs
 *   ei_out [B,2,K+N] int64, w_out [B,K+N] fp32.
 * gnpde_norm_weights_f32: fac[r] = deg(r)^-1 (RW_*) or deg^-1/2 with inf -> 0
 *   (GCN), deg summed sequentially in COO order over the grouped CSR (rowptr,
 *   perm) of gnpde_csr_build — grouped by source (key_row 0) for RW_ROW, by
 *   destination (key_row 1) for RW_COL and GCN; then
 *   RW_ROW: w_out = fac[row] * w,  RW_COL: w_out = w * fac[col],
 *   GCN:    w_out = fac[row] * w * fac[col]  (fac [B*N] is caller scratch).  */
#define GNPDE_NORM_RW_ROW 0  /* get_rw_adj(norm_dim=0)        */
#define GNPDE_NORM_RW_COL 1  /* get_rw_adj(norm_dim=1)        */
#define GNPDE_NORM_GCN 2     /* gcn_norm_fill_val             */
size_t gnpde_self_loops_workspace_bytes(int64_t B, int64_t E, int64_t N);
int gnpde_self_loops_count(const int64_t* edge_index, int64_t B, int64_t E, int64_t* nonloop, void* workspace,
                           size_t workspace_bytes, void* stream);
int gnpde_add_self_loops(const int64_t* edge_index, const float* w, int64_t B, int64_t E, int64_t N, float fill,
                         int64_t K, int64_t* ei_out, float* w_out, void* workspace, size_t workspace_bytes,
                         void* stream);
int gnpde_norm_weights_f32(const int64_t* edge_index, const float* w, int64_t B, int64_t E, int64_t N,
                           const int32_t* rowptr, const int32_t* perm, int mode, float* fac, float* w_out,
                           void* stream);

/* ---------------------------------------------------------------- work plan
 * Splits rows with more than `chunk` edges into balanced chunks so that one
 * power-law hub does not serialise a wavefront.  items[n_items] is int4
 * {row, edge_begin, edge_end, slot} (slot = -1: the item owns its row;
 * slot >= 0: partial-sum slot); heavy[n_heavy] is int4 {row, first_slot,
 * n_chunks, 0}.  Capacity: items >= R + 2*nnz/chunk + 1, heavy >= nnz/chunk + 1.
 * SYNCHRONOUS (copies the two counts to the host); call once per graph.     */
int gnpde_plan_build(const int32_t* rowptr, int64_t R, int32_t chunk,
                     int32_t* items, int64_t items_capacity, int32_t* heavy, int64_t heavy_capacity,
                     int64_t* n_items, int64_t* n_heavy, int64_t* n_slots,
                     void* workspace, size_t workspace_bytes, void* stream);
size_t gnpde_plan_workspace_bytes(int64_t R);

/* ---------------------------------------------------------------- fused solver epilogue
 * Optional stage outputs of the RHS kernels, so a Runge-Kutta stage combination
 * y0 + dt*sum_j b_j k_j is produced by the same pass that computes k_i (no
 * separate read of k_i, no extra launch).  A stage has nk shared operand
 * arrays k[0..nk-1] (each read once per row however many outputs use it); with
 * f = the RHS value of row r:
 *   f_out[r]    = f                                            (f_out may be NULL)
 *   o[i].out[r] = cb*base[r] + cf*f + sum_{j<nk} o[i].c[j]*k[j][r]   for i < n_out
 * base may be NULL (0), equal to the RHS input x (the row already read by the
 * epilogue is reused) or equal to o[i].out (in-place accumulation).  Every
 * array has the leading dimension ldf of the RHS output.  No output may alias
 * the RHS input x (other rows of x are still being gathered).
 * Aliasing rule: an output may be the same array as its base or as a k operand
 * (the whole array: same pointer, leading dimension and element type) — every
 * element is read by the lane that stores it, before its store — but only
 * without out_rows (GNPDE_EINVAL otherwise: a row would be stored where another
 * lane still reads).  Partly overlapping arrays are never allowed.
 * out_rows (NULL = identity): the o[i].out stores of row r go to row
 * out_rows[r] instead (base, k and f_out stay at row r) — the last step of a
 * solve run in a renumbered node order writes its result straight into the
 * caller's numbering (gnpde.integrator); it must be a permutation of [0, R).
 * dot_rows (NULL = none; fp32 state, power-of-two lanes per row): per row,
 *   dot_rows[r] (+)= dot_coef * sum_c f[r,c] * dot_with[r,c]   (fp64; "+=" when
 * dot_accumulate), summed over the row's lanes in a fixed order — the per-row
 * terms of a parameter gradient <f, y> that the caller reduces once
 * (gnpde_sum_f64), instead of a separate pass re-reading f.
 * err_rows (NULL = none): the error estimate of an embedded Runge-Kutta pair
 * (torchdiffeq's RKAdaptiveStepsizeODESolver: error_ratio = RMS(e / tol)):
 *   e      = err.cb*err.base + err.cf*f + sum_{j<nk} err.c[j]*k[j]   (err.out unused)
 *   y1     = the RHS input x (err_y1 = -1), err_y0 itself (err_y1 = -2, ABI 8: tol =
 *            atol + rtol |y0|, the scale of torchdiffeq's initial-step selection) or
 *            the value of output err_y1
 *   tol    = atol + rtol * max(|err_y0|, |y1|)
 *   err_rows[r] = sum_c (e / tol)^2     (fp64, the row's lanes in a fixed order)
 * which the caller sums (gnpde_sum_f64) into the squared norm of one step.
 * scale_rows (NULL = none; ABI 8; with err_rows, the plain-weight K1 only, not beside
 * dot_rows): scale_rows[r] = sum_c (err_y0 / tol)^2 — with e = f and err_y1 = -2 the
 * f0 launch of an adaptive solve yields both squared sums of the initial-step
 * selection (gnpde_initial_step_rows).
 * coef_scale (NULL = 1): a device fp32 scalar multiplying every cf and c[j] of the
 * outputs and of err (not cb): the step size of an adaptive solve, so the
 * launches of a step do not change with it (hipGraph-replayable, one graph per
 * step whatever dt).
 * f_lin (0 = off): the RHS value becomes f = x + coef_scale*f_lin*f before any
 * store or combination (x = the RHS input row): for an affine RHS f(y) = L y + s
 * evaluated on the input k WITHOUT the source term (flags: no GNPDE_ADD_SOURCE),
 * f(y0 + h k) = k + h L k with k = f(y0) — an adaptive step's first stage derivative
 * without materialising its stage input y0 + h k (gnpde.integrator, ABI 5).
 * unscaled_outs (0 = none; ABI 6): bit i set — output i takes its cf and c[j]
 * WITHOUT coef_scale (the error term always takes it): a combination whose
 * operands already carry the step size, e.g. the next step's f0 = sum_p B[p] u_p
 * of the affine Krylov step (u_p = (h L)^p f0, gnpde.integrator).
 * A k operand (or base) equal to the RHS input x reuses the row already read.
 * err_rows and 3..6 operands take the wide epilogue (operands loaded after the
 * aggregation); since ABI 7 it carries dot_rows too, beside err_rows or with up to
 * 6 operands (a second fp64 row sum: the adaptive adjoint's alpha integrand
 * <L^T a_i, y_i> in the launch that forms the next adjoint stage input and its
 * error rows, gnpde.integrator), fused into the plain-weight
 * K1 (gnpde_spmm_rhs_f32 / _bf16); the attention kernels return
 * GNPDE_EUNSUPPORTED for it (the caller applies it with gnpde_stage_apply_*).
 * dense_out (NULL = none; ABI 8; plain-weight K1 with err_rows only): the dense
 * output of the adaptive step folded into its last launch.  With the device
 * fp64 scalars t0 = dense_t[0] (the step's start), t_out = dense_t[1] and
 * h = *dense_dt (the step size), when t0 < t_out <= t0 + h (the step crosses the
 * output time; wave-uniform, nothing is written otherwise):
 *   x = (t_out - t0)/h, the basis w = {cy0 + cy1 + cym, h cy1, h cym, cf0, cf1}
 *   of torchdiffeq's 4th-order interpolant (cy0 = 1 - 11x^2 + 18x^3 - 8x^4,
 *   cy1 = -5x^2 + 14x^3 - 8x^4, cym = 16x^2 - 32x^3 + 16x^4,
 *   cf0 = h (x - 4x^2 + 5x^3 - 2x^4), cf1 = h (x^2 - 3x^3 + 2x^4)),
 *   out[dense_rows[r]] = sum_m w[m] (dense_m[m][0] o[0].base[r]
 *                        + sum_{j<nk} dense_m[m][1+j] k[j][r] + dense_m[m][7] f[r])
 * (coefficients formed in fp64, applied in fp32; f after f_lin), out = *dense_out
 * (a device slot holding the output array: the launch can be captured once and
 * its output redirected per solve).  dense_tab: device scratch of
 * GNPDE_STAGE_MAX_K + 3 floats holding the crossing flag and the coefficients of
 * the launch's step, which an EARLIER launch of the same step forms: a K1 launch
 * whose stage sets dense_tab, dense_t, dense_dt and dense_m but not dense_out writes
 * them (a one-wavefront launch ahead of its aggregation) — the first launch of
 * the step, so the one that applies them reads them into scalar registers.    */
#define GNPDE_STAGE_MAX_OUT 2
#define GNPDE_STAGE_MAX_K 6
#define GNPDE_DENSE_BASIS 5
typedef struct {
  float* out;
  const float* base;
  float cb;
  float cf;
  float c[GNPDE_STAGE_MAX_K];
} gnpde_stage_out_t;

typedef struct {
  float* f_out;
  int n_out;
  gnpde_stage_out_t o[GNPDE_STAGE_MAX_OUT];
  int nk;
  const float* k[GNPDE_STAGE_MAX_K];
  const int32_t* out_rows;
  const float* dot_with;
  double* dot_rows;
  double dot_coef;
  int dot_accumulate;
  double* err_rows;
  gnpde_stage_out_t err;
  const float* err_y0;
  int err_y1;
  double atol;
  double rtol;
  const float* coef_scale;
  float f_lin;
  int unscaled_outs;
  float* const* dense_out;
  const int32_t* dense_rows;
  const double* dense_t;
  const double* dense_dt;
  float* dense_tab;
  float dense_m[GNPDE_DENSE_BASIS][GNPDE_STAGE_MAX_K + 2];
  double* scale_rows;
} gnpde_stage_epilogue_t;

/* The stage epilogue as a pass of its own, over rows [0, R) of C columns
 * (leading dimension ld, every array of the stage included): f [R, ld] is the
 * RHS value (NULL: every cf term is 0 — a plain combination such as a stage
 * input y0 + dt*b0*k0 or dense output), x the RHS input (needed when a base is
 * x or err_y1 = -1; may be NULL otherwise).  Same arithmetic, per element, as
 * the fused epilogue (fp32; err_rows in fp64).  bf16: every row array is bf16
 * (the struct's float* reinterpreted), the arithmetic fp32.  Used by the
 * adaptive solvers for the attention RHS kernels that fuse only the fixed-grid
 * stages, and for the pre-step and dense-output combinations.               */
int gnpde_stage_apply_f32(int64_t R, int64_t C, int64_t ld, const float* f, const float* x,
                          const gnpde_stage_epilogue_t* stage, void* stream);
int gnpde_stage_apply_bf16(int64_t R, int64_t C, int64_t ld, const uint16_t* f, const uint16_t* x,
                           const gnpde_stage_epilogue_t* stage, void* stream);

/* ---------------------------------------------------------------- K1: SpMM RHS
 * ax[r,:] = sum_{p in row r} w[p] * x[col[p],:]
 * f[r,:]  = ax                                  (flags & 1 == 0)
 *         = a*(ax - x[r,:]) [+ b*x0[r,:]]        (GNPDE_EPI_RHS)
 * a = *alpha or sigmoid(*alpha), b = *beta: device scalars (no host sync).
 * partials: n_slots*C floats of scratch (NULL if n_slots == 0; n_slots from
 * gnpde_plan_build); n_slots*C*4 must stay below 0xffffff00 bytes (the hub
 * partials are addressed with 32-bit buffer offsets): GNPDE_EUNSUPPORTED past
 * it — plan the graph with a larger chunk.
 * heavy: the hub table of gnpde_plan_build.  The chunks of a hub row are
 * combined inside the launch by the chunk that finishes last, which it learns
 * from an arrival ticket kept in the 4th word of the row's heavy entry
 * (plan_build writes 0; every launch leaves 0).  Launches that share one plan
 * must therefore be ordered (one stream, or events) — never concurrent.
 * stage: NULL -> f[r,:] is stored to f; otherwise the stage epilogue above
 * decides what is stored (f is ignored).
 * Replaces function_laplacian_diffusion.py:39-77 per RHS evaluation.        */
int gnpde_spmm_rhs_f32(const int32_t* items, int64_t n_items, int32_t* heavy, int64_t n_heavy,
                       const int32_t* col, const float* w, int64_t C,
                       const float* x, int64_t ldx, const float* x0, int64_t ldx0,
                       const float* alpha, const float* beta, int flags,
                       float* f, int64_t ldf, float* partials, int64_t n_slots,
                       const gnpde_stage_epilogue_t* stage, void* stream);

/* The last K1 launch of an rk4 solve over a graph with FROZEN rows: rows whose only
 * edge is their own self loop of weight exactly 1.0f and that no other row gathers
 * (f = a*(1*x - x) = 0, so a step changes the row by the rounding of its last
 * combination alone, which reads nothing but the row; the caller classifies them
 * and numbers them last: rows [row0, row1), their items behind the plan's first
 * n_live_items, and leaves them out of every earlier launch of the solve by
 * passing gnpde_spmm_rhs_f32 the first n_live_items items only).  This launch runs
 * the first n_live_items items as gnpde_spmm_rhs_f32 does and, behind them, streams
 * the frozen rows from `home` [.., ldx] — the state the solve began with — through
 * `steps` >= 1 steps' stage epilogues with the own row, the base and every k operand
 * set to the row: the bits of `steps` full steps, every one with this stage's
 * coefficients (f is 0, or NaN for a non-finite entry, whatever the step size; the
 * steps of a solve share the sign of dt).  `home` may be the stage's output (in
 * place: a lane reads its slice before it stores), but not under out_rows.  fp32
 * rows of 65-128 columns in 16-byte slices, GNPDE_EPI_RHS without GNPDE_ADD_SOURCE,
 * a fixed-grid stage (one output, no f_out, at most two k operands, f_lin 0, no
 * dot / error / dense term); GNPDE_EUNSUPPORTED otherwise.  Other arguments as
 * gnpde_spmm_rhs_f32.                                                         */
int gnpde_spmm_rhs_frozen_f32(const int32_t* items, int64_t n_live_items, int32_t* heavy, int64_t n_heavy,
                              const int32_t* col, const float* w, int64_t C, const float* x, int64_t ldx,
                              const float* alpha, int flags, int64_t ldf, float* partials, int64_t n_slots,
                              const gnpde_stage_epilogue_t* stage, const float* home, int64_t row0, int64_t row1,
                              int64_t steps, void* stream);

/* Column stripes of K1's headline geometry (fp32 rows of 65-128 columns in 16-byte
 * slices, plain weights, stage kinds 0 and 1: store f, or one fixed-grid stage
 * output).  On a graph whose gathered rows overflow one XCD's L2, gnpde_spmm_rhs_f32
 * has each workgroup aggregate 128 / S columns of all its rows (S = 4 or 2) and
 * deals the stripes to the XCDs, so that a row slice is fetched by 8 / S of the
 * eight L2s instead of nearly all of them.  The bits are those of the unstriped
 * launch.  The environment variable GNPDE_K1_STRIPES = 0 | 2 | 4 (read once)
 * selects no stripes, S = 2 or S = 4 for EVERY launch of that geometry, whatever its
 * size; unset, the launch code decides from the shape: S = 2 for the stage launches
 * (one fixed-grid stage output) of at least 65,536 rows x 128 columns of state that
 * carry GNPDE_LIVE_ITEMS, no stripes otherwise.  gnpde_k1_stripes_set
 * overrides the variable: 0, 2, 4 as above; -1 removes the override.
 * gnpde_k1_stripes_for: the stripe count (0, 2, 4) a launch of n_items items of C
 * columns, stage kind 0 (store f) or 1 (a stage output) and flags `flags` in that
 * geometry takes under the current setting.
 * gnpde_k1_striped_launches: striped launches issued by this process so far.    */
int gnpde_k1_stripes_set(int stripes);
int gnpde_k1_stripes_for(int64_t n_items, int64_t C, int stage_kind, int flags);
int64_t gnpde_k1_striped_launches(void);

/* K1 on bfloat16 storage (configs[3], BLEND in bf16): x, x0, f and every
 * stage pointer of `stage` address bf16 arrays (raw uint16 bits; the stage
 * struct's float* fields are reinterpreted); weights, alpha, beta and the
 * partials stay fp32, and every sum and the epilogue run in fp32 — only the
 * stored rows are rounded (nearest even).  Otherwise as gnpde_spmm_rhs_f32.  */
int gnpde_spmm_rhs_bf16(const int32_t* items, int64_t n_items, int32_t* heavy, int64_t n_heavy,
                        const int32_t* col, const float* w, int64_t C, const uint16_t* x, int64_t ldx,
                        const uint16_t* x0, int64_t ldx0, const float* alpha, const float* beta, int flags, uint16_t* f,
                        int64_t ldf, float* partials, int64_t n_slots, const gnpde_stage_epilogue_t* stage,
                        void* stream);

/* K1 with the attention weights computed on the fly for the fork's scaled_dot
 * (reference score mode) under destination-grouped softmax (attention_norm_idx
 * 1): w_p = mean_h exp(cs[row,h] - m[col_p,h]) * rl[col_p,h], cs [R,H] fp64 node
 * scores (gnpde_ref_scores_f32), m [R,H] fp64 / rl [R,H] group statistics
 * (gnpde_softmax_stats_f32 / gnpde_seg_softmax_f32 over the CSC), or, when
 * mr is given (heads == 2, 16-byte aligned), the packed statistics records
 * those kernels write into mr (GNPDE_STATS_RECORD_FLOATS(heads) floats per
 * group: m[0..h-1], then rl[0..h-1]): one 16-byte load per edge.  Every
 * statistics kernel stores the group max rounded to fp32 (exact in both forms)
 * and the sum relative to it, so both forms hold the same values.
 * Equals gnpde_attn_weights_f32 + gnpde_spmm_rhs_f32 bit for bit, in one pass:
 * ODEFuncTransformerAtt.forward, function_transformer_attention.py:44-59.
 * Other arguments as gnpde_spmm_rhs_f32.                                     */
#define GNPDE_STATS_RECORD_FLOATS(h) ((2 * (h) + 3) & ~3)
int gnpde_attn_ref_rhs_f32(const int32_t* items, int64_t n_items, int32_t* heavy, int64_t n_heavy,
                           const int32_t* col, const double* cs, const double* m, const float* rl, const float* mr,
                           int64_t heads,
                           int64_t C, const float* x, int64_t ldx, const float* x0, int64_t ldx0, const float* alpha,
                           const float* beta, int flags, float* f, int64_t ldf, float* partials, int64_t n_slots,
                           const gnpde_stage_epilogue_t* stage, void* stream);

/* The per-edge scaled_dot attention RHS under source-grouped softmax
 * (attention_norm_idx 0; upstream GRAND's transformer RHS) in ONE aggregation
 * pass over the CSR plan (csrc/flash.hip): every row slot scores the edges it
 * gathers, s_e,h = q[row,h] . k[col_e,h] / sqrt(dk), forms its group's
 * statistics (max M_h, sum L_h of exp(s - M_h)) and aggregates with
 *   w_e = (1/H) sum_h exp(s_e,h - M_h) / (L_h + 1e-16)
 * = multiply_attention with the head mean of utils.softmax over edge_index[0]
 * (function_transformer_attention.py:33-41, 246-266; src/utils.py:116-127),
 * then the RHS epilogue, or a single-output stage epilogue without a dot
 * term (the forward integrator's; others: GNPDE_EUNSUPPORTED), as
 * gnpde_spmm_rhs_f32.  Replaces
 * gnpde_seg_softmax_f32(out_kind 0) + gnpde_spmm_rhs_f32 (no [nnz] weights).
 * q, k: [R, ldqk] fp32 (gnpde_linear_f32), 16-byte aligned rows.  Hub rows
 * (heavy entries of the plan): each chunk keeps its own statistics and
 * per-head sums in a partial slot, merged in-launch by the last chunk to
 * arrive (heavy[].w tickets, as K1).  workspace:
 * gnpde_attn_dot_workspace_floats(heads, C, n_slots) floats, 16-byte aligned.
 * Shapes:
 * gnpde_attn_dot_supported(heads, dk, C) != 0 (heads in {1, 2, 4}, dk % 4 ==
 * 0, heads*dk in {8, 16, 32, 64}, C % 4 == 0, C <= 256); otherwise
 * GNPDE_EUNSUPPORTED.  Exponentials in base 2 (1-2 ulp from expf).
 * dst_stats != NULL: destination-grouped softmax (attention_norm_idx 1)
 * instead — the packed statistics records of every destination
 * (GNPDE_STATS_RECORD_FLOATS(heads) floats: m[h] then rl[h], from
 * gnpde_seg_softmax_f32 over the CSC, 16-byte aligned) weight each scored
 * edge, w_e = (1/H) sum_h exp(s_e,h - m[c,h]) rl[c,h]: replaces
 * gnpde_attn_weights_f32 + gnpde_spmm_rhs_f32.                              */
int gnpde_attn_dot_supported(int64_t heads, int64_t dk, int64_t C);
int64_t gnpde_attn_dot_workspace_floats(int64_t heads, int64_t C, int64_t n_slots);
int gnpde_attn_dot_rhs_f32(const int32_t* items, int64_t n_items, int32_t* heavy, int64_t n_heavy,
                           const int32_t* col, const float* q, const float* k, int64_t ldqk, int64_t heads, int64_t dk,
                           const float* dst_stats, int64_t C, const float* x, int64_t ldx, const float* x0, int64_t ldx0,
                           const float* alpha, const float* beta, int flags, float* f, int64_t ldf, float* workspace,
                           int64_t n_slots, const gnpde_stage_epilogue_t* stage, void* stream);
/* The same over a bf16 state (x, x0, f and the stage rows bf16, 8-byte aligned
 * 4-element slices; q, k, dst_stats and the workspace fp32): source-grouped
 * softmax (dst_stats NULL) with the plain RHS or a single-output stage only,
 * GNPDE_EUNSUPPORTED otherwise (the binding then takes K2 + gnpde_spmm_rhs_bf16). */
int gnpde_attn_dot_rhs_bf16(const int32_t* items, int64_t n_items, int32_t* heavy, int64_t n_heavy,
                            const int32_t* col, const float* q, const float* k, int64_t ldqk, int64_t heads,
                            int64_t dk, const float* dst_stats, int64_t C, const void* x, int64_t ldx, const void* x0,
                            int64_t ldx0, const float* alpha, const float* beta, int flags, void* f, int64_t ldf,
                            float* workspace, int64_t n_slots, const gnpde_stage_epilogue_t* stage, void* stream);

/* ---------------------------------------------------------------- attention
 * Node-level projection on the matrix cores (K % 16 == 0, K <= 128: exact
 * three-piece bf16 splits of both operands on v_mfma_f32_32x32x16_bf16, f32-GEMM
 * accuracy; other shapes: v_mfma_f32_32x32x2_f32):
 *   out[r, j] = sum_k x[r,k] * W[j,k] + bias[j], j < Nout; columns [0, split)
 *   go to out_a (ld lda), [split, Nout) to out_b (ld ldb).
 * Replaces the nn.Linear Q/K of function_transformer_attention.py:224-225.  */
int gnpde_linear_f32(const float* x, int64_t R, int64_t K, int64_t ldx, const float* W, const float* bias,
                     int64_t Nout, int64_t split, float* out_a, int64_t lda, float* out_b, int64_t ldb,
                     void* stream);
/* The same projection of a bf16 state (x: [R, ldx] bf16): the elements are widened
 * to fp32 exactly on load, so the outputs equal gnpde_linear_f32 of the fp32 copy of
 * x bit for bit (a bf16 state's per-edge attention scores without that copy). */
int gnpde_linear_bf16(const void* x, int64_t R, int64_t K, int64_t ldx, const float* W, const float* bias,
                      int64_t Nout, int64_t split, float* out_a, int64_t lda, float* out_b, int64_t ldb,
                      void* stream);

/* The output product of the GAT value projection fused with the RHS epilogue and
 * the fixed-grid stage combination (mix_features, function_GAT_attention.py:38 and
 * :60-68; an entry point added under ABI 8, no struct changed):
 *   ax[r,:] = sum_k z[r,k] * Wt[:,k]      z [R, ldz] fp32, Wt [C, K] row-major = Wout^T
 *   f[r,:]  = ax                                  (flags & 1 == 0; x may be NULL)
 *           = a*(ax - x[r,:]) [+ b*x0[r,:]]        (GNPDE_EPI_RHS)
 * flags, the sigmoid and the device scalars alpha / beta exactly as in
 * gnpde_spmm_rhs_f32.  stage: NULL -> f is stored; otherwise the fixed-grid stage
 * epilogue decides what is stored (f is ignored): f_out, n_out <= GNPDE_STAGE_MAX_OUT
 * outputs, at most two shared operands, the aliasing rule above; no output (nor f)
 * may be z or the RHS input x.  err_rows, dot_rows, dense_*, scale_rows, f_lin,
 * out_rows, coef_scale or more than two operands: GNPDE_EUNSUPPORTED (the caller
 * stores f and applies the stage with gnpde_stage_apply_f32).  The stage arithmetic
 * is the one K1 and gnpde_stage_apply_f32 run per element, so the fused stage equals
 * f followed by gnpde_stage_apply_f32 bit for bit.  No atomics: repeated launches
 * give the same bits.  K % 16 == 0, K <= 128, C % 4 == 0 and 16-byte aligned rows:
 * the split-bf16 product of gnpde_linear_f32 on v_mfma_f32_32x32x16_bf16 (f32-GEMM
 * accuracy); any other K >= 1, C >= 1: one exact-f32 fma chain per output.      */
int gnpde_linear_rhs_f32(const float* z, int64_t R, int64_t K, int64_t ldz,
                         const float* Wt /* [C, K] row-major = Wout^T */, int64_t C,
                         const float* x, int64_t ldx, const float* x0, int64_t ldx0,
                         const float* alpha, const float* beta, int flags,
                         float* f, int64_t ldf,
                         const gnpde_stage_epilogue_t* stage, void* stream);

/* The same with an output bias (the transformer layer's Wout, an nn.Linear with a bias:
 * function_transformer_attention.py:31; an entry point added under ABI 8):
 *   ax[r,:] = sum_k z[r,k] * Wt[:,k] + bias[:]      bias [C] fp32, 16-byte aligned on the
 * fast path; bias NULL: gnpde_linear_rhs_f32 itself (the same kernels, the same bits).
 * The bias is added to the finished product ahead of the epilogue, on both kernels and
 * under the fused stage.                                                          */
int gnpde_linear_rhs_bias_f32(const float* z, int64_t R, int64_t K, int64_t ldz,
                              const float* Wt /* [C, K] row-major */, int64_t C, const float* bias,
                              const float* x, int64_t ldx, const float* x0, int64_t ldx0,
                              const float* alpha, const float* beta, int flags,
                              float* f, int64_t ldf,
                              const gnpde_stage_epilogue_t* stage, void* stream);

/* The per-head value aggregation of the transformer layer's mix_features branch
 * (function_transformer_attention.py:23-32; entry points added under ABI 8):
 *   z[r, d] = (1/heads) * sum over CSR positions p of row r, sum over h:
 *                 w[p, h] * v[col[p], h*dk + d]          z [R, ldz] (dk columns)
 * v [R, ldv] fp32 holds att = heads*dk columns, head h owning h*dk .. h*dk+dk-1.
 * w: per-head edge weights, [nnz, heads] in aggregation-CSR order (perm NULL), or in COO
 * order read as w[perm[p], h] (perm = the CSR's position -> COO edge map).  items / heavy:
 * the plan of the aggregation CSR, consumed as gnpde_spmm_rhs_f32 consumes it (hub rows
 * in chunk items, partial rows in `workspace`, combined in-launch by the last chunk to
 * arrive, heavy[].w tickets reset for the next launch: launches on one plan must be
 * ordered).  workspace: gnpde_head_aggregate_workspace_floats(dk, n_slots) floats,
 * 16-byte aligned.  gnpde_head_aggregate_fast(heads, dk) != 0 (dk % 4 == 0, heads and
 * heads*dk/4 powers of two, heads*dk <= 256) with 16-byte aligned rows: one wavefront per
 * item; any other shape: one fp32 chain per output element over rowptr / col (the plan
 * is not read).  No float atomics, fixed summation orders: repeated launches give the
 * same bits.  A row without edges gets zeros.                                      */
int gnpde_head_aggregate_fast(int64_t heads, int64_t dk);
int64_t gnpde_head_aggregate_workspace_floats(int64_t dk, int64_t n_slots);
int gnpde_head_aggregate_f32(const int32_t* items, int64_t n_items, int32_t* heavy, int64_t n_heavy,
                             const int32_t* rowptr, const int32_t* col, const int32_t* perm, int64_t R,
                             const float* w, int64_t heads, int64_t dk, const float* v, int64_t ldv,
                             float* z, int64_t ldz, float* workspace, int64_t n_slots, void* stream);

/* Weight gradient of the projection: gW[m, k] = sum_r gy[r, m] * x[r, k]
 * (gy [R, M] ld ldg = dL/d[q | k], x [R, K] ld ldx; gW [M, K] ld ldw), the
 * backward of nn.Linear's weight for the Q / K of
 * function_transformer_attention.py:224-225.  fp32 matrix cores
 * (v_mfma_f32_32x32x2_f32), the rows split over up to 512 wavefronts (at least
 * 128 rows each, and no more partial tiles than 64 MiB hold) whose partial tiles
 * are summed in wave order (deterministic).  workspace:
 * gnpde_linear_wgrad_workspace_bytes(R, M, K) bytes.                         */
size_t gnpde_linear_wgrad_workspace_bytes(int64_t R, int64_t M, int64_t K);
int gnpde_linear_wgrad_f32(const float* gy, int64_t R, int64_t M, int64_t ldg, const float* x, int64_t K, int64_t ldx,
                           float* gW, int64_t ldw, void* workspace, size_t workspace_bytes, void* stream);

/* Reference-mode node scores (fork scaled_dot, function_transformer_attention.py:249):
 *   S_b = Wk * (sum_n indeg(n) x_n) + (sum_n indeg(n)) bk    (fp64)
 *   cs[r,h] = (q_r,h . S_b,h) / sqrt(dk),  q = Wq x + bq      (fp64 out)
 * indeg: in-degree per global node (int32, R); ws: gnpde_keysum_workspace_bytes
 * (scratch, no state between calls).  Three launches: indegree-weighted column
 * sums over ~256 fp64 row tiles; one workgroup per batch element summing the
 * tiles in fixed order and forming S_b, U = Wq^T S / sqrt(dk) and v; the node
 * scores cs = x U + v.  attention_dim <= 4096.                               */
size_t gnpde_keysum_workspace_bytes(int64_t B, int64_t N, int64_t C, int64_t att);
int gnpde_ref_scores_f32(const float* x, int64_t B, int64_t N, int64_t C, int64_t ldx, const int32_t* indeg,
                         const float* Wq, const float* bq, const float* Wk, const float* bk,
                         int64_t att, int64_t heads, double* cs, void* workspace, size_t workspace_bytes,
                         void* stream);

/* The same in two phases, for a state split into column stripes (gnpde.dist):
 * S and cs are linear in the columns, so each stripe forms its share and the
 * caller sums the shares over the stripes between the phases (one all-reduce of
 * S [B, att] fp64, one of cs [R, heads] fp64):
 *   gnpde_ref_keysum_f32:             S[b] = Wk xbar_b + (sum_n indeg(n)) bk   (fp64 [B][att];
 *                                     the stripe's columns of Wk, bk on one stripe only)
 *   gnpde_ref_scores_from_keysum_f32: cs[r,h] = q_r,h . S_b,h / sqrt(dk) from a given S
 *                                     (the stripe's columns of Wq, bq on one stripe only).
 * x, Wk, Wq: the stripe's columns (C of them, contiguous [att, C] weights);
 * workspace as gnpde_ref_scores_f32.                                          */
int gnpde_ref_keysum_f32(const float* x, int64_t B, int64_t N, int64_t C, int64_t ldx, const int32_t* indeg,
                         const float* Wk, const float* bk, int64_t att, double* S, void* workspace,
                         size_t workspace_bytes, void* stream);
int gnpde_ref_scores_from_keysum_f32(const float* x, int64_t B, int64_t N, int64_t C, int64_t ldx, const double* S,
                                     const float* Wq, const float* bq, int64_t att, int64_t heads, double* cs,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* Destination- or source-grouped softmax statistics over a grouped CSR
 * (items from gnpde_plan_build over the CSC for norm_idx=1, the CSR for
 * norm_idx=0; gidx = the OTHER endpoint of each edge):
 * m[g,h] = max_e s_e,h rounded to fp32 (stored as fp64), rl[g,h] = 1/(sum_e exp(s_e,h - m) + 1e-16).
 * partials: 2*heads doubles per plan slot.
 * Edge scores by `mode` from cs (REFERENCE) or q/k (per-edge modes).
 * Groups of 8 lanes per item: plan it with a small chunk (e.g. 64).
 * m, rl and mr (packed records, see gnpde_attn_ref_rhs_f32) are each optional;
 * m and rl come as a pair, and at least one of the two forms is written.
 * Restates utils.softmax, src/utils.py:116-127.                              */
int gnpde_softmax_stats_f32(const int32_t* items, int64_t n_items, const int32_t* heavy, int64_t n_heavy,
                            const int32_t* gidx, int group_is_dst, int mode, int64_t heads, int64_t dk,
                            const double* cs, const float* q, const float* k, int64_t ldqk,
                            float score_p0, float score_p1,
                            double* m, float* rl, float* mr, double* partials, void* stream);

/* Head-mean attention weights in aggregation-CSR order (edge-parallel):
 *   w[p] = (1/h) sum_h exp(s_p,h - m[g,h]) * rl[g,h],  g = src (norm_idx 0) or dst (1)
 * (utils.softmax then attention.mean(dim=2), function_transformer_attention.py:34).
 * The attention RHS is then gnpde_spmm_rhs_f32 with these weights
 * (multiply_attention :33-41 + forward :52-59).                              */
int gnpde_attn_weights_f32(const int32_t* rowidx, const int32_t* col, int64_t nnz, int norm_idx, int mode,
                           int64_t heads, int64_t dk, const double* cs, const float* q, const float* k, int64_t ldqk,
                           float score_p0, float score_p1, const double* m, const float* rl, float* w_out,
                           void* stream);

/* K2: edge-block segmented softmax over a grouped CSR (the aggregation CSR
 * for norm_idx 0, the CSC for norm_idx 1; gidx = the other endpoint, rowidx =
 * the group of every position, group_is_dst as in gnpde_softmax_stats_f32).
 * One wavefront per item = at most EB consecutive edges (EB =
 * gnpde_seg_block_edges(mode, heads, dk); 0 means unsupported): items are
 * int4 {e_begin, e_end, -1, first_group} covering consecutive whole groups
 * (packed greedily up to EB edges); chunk_items {e_begin, e_end, slot, group}
 * split groups of degree > EB, heavy {group, first_slot, n_chunks, 0} lists
 * those groups (partials: 2*heads doubles per slot; m/rl scratch).
 * Reference scores with out_kind 1 over the CSC (norm_idx 1) also take, at the
 * front of `items`, n_hub_items HUB CHUNK items {e_begin, e_end, slot, hub}
 * (gnpde_seg_long_edges()-edge chunks of the longer groups, one wavefront each;
 * heavy[hub] = {group, first_slot, n_chunks, 0} lists those groups, n_heavy of
 * them, and partials holds 2*heads doubles per slot: the last chunk of a group to
 * arrive merges its slots in chunk order and resets heavy[hub].w, so two launches
 * on one plan must not overlap) and then n_long_items LONG items {e_begin, e_end,
 * -2, group} (a whole group of at most gnpde_seg_long_edges() edges, one wavefront
 * each); the rest are whole-group items, taken two per wavefront, and
 * n_chunk_items is 0.  (n_hub_items = n_long_items = 0 for other plans.)
 * gnpde_seg_plan_build builds them from a HOST copy of rowptr into HOST
 * arrays (plain C++, once per graph; capacities: items >= R, chunk_items >=
 * nnz/eb + R, heavy >= nnz/eb + 1).  When chunk_items == items + 4*n_items
 * (stored back to back) both item kinds run in one launch.
 *   out_kind 0: w[p] = (1/H) sum_h softmax_p,h in grouped order (per-edge
 *               modes with norm_idx 0: the aggregation weights of K1);
 *   out_kind 1: m[g,h] = max (fp64), rl[g,h] = 1/(sum exp(s - m) + 1e-16),
 *               into m/rl and/or the packed records mr (gnpde_attn_ref_rhs_f32).
 * Per-group max and sum come from segmented scans across the lanes (fixed
 * order, deterministic).  Restates utils.softmax, src/utils.py:116-127, with
 * the scores of function_transformer_attention.py:246-259 and the head mean of
 * :34.  Returns GNPDE_EUNSUPPORTED for shapes outside the kernel (dk % 4 != 0,
 * non-power-of-two teams, uniform scores, reference scores with out_kind 0).  */
int gnpde_seg_block_edges(int mode, int64_t heads, int64_t dk);
/* Edges of one long item of the reference statistics (whole groups up to it,
 * chunks of it beyond): the plan builder's unit. */
int gnpde_seg_long_edges(void);
/* Edges one wavefront covers in ONE pass over a long item of `heads` heads
 * (<= gnpde_seg_long_edges()): the long-item size of a small graph's plan, whose
 * launch is latency-bound (every item one pass; longer groups as hub chunks). */
int gnpde_seg_long_pass_edges(int64_t heads);
int gnpde_seg_plan_build(const int32_t* rowptr, int64_t R, int32_t eb, int32_t* items, int64_t items_capacity,
                         int32_t* chunk_items, int64_t chunks_capacity, int32_t* heavy, int64_t heavy_capacity,
                         int64_t* n_items, int64_t* n_chunks, int64_t* n_heavy);
int gnpde_seg_softmax_f32(const int32_t* items, int64_t n_items, int64_t n_hub_items, int64_t n_long_items,
                          const int32_t* chunk_items,
                          int64_t n_chunk_items, int32_t* heavy, int64_t n_heavy, const int32_t* rowptr,
                          const int32_t* rowidx,
                          const int32_t* gidx, int group_is_dst, int out_kind, int mode, int64_t heads, int64_t dk,
                          const double* cs, const float* q, const float* k, int64_t ldqk,
                          float score_p0, float score_p1, float* w, double* m, float* rl, float* mr,
                          double* partials, void* stream);

/* Per-edge, per-head attention in COO order (the [B,E,h] `attention` that
 * SpGraphTransAttentionLayer.forward returns, function_transformer_attention.py:265-267):
 *   att[perm[p]*heads + h] = exp(s_p,h - m[g,h]) * rl[g,h]  over the aggregation CSR. */
int gnpde_edge_attention_f32(const int32_t* rowidx, const int32_t* col, const int32_t* perm, int64_t nnz,
                             int norm_idx, int mode, int64_t heads, int64_t dk,
                             const double* cs, const float* q, const float* k, int64_t ldqk,
                             float score_p0, float score_p1, const double* m, const float* rl,
                             float* att, void* stream);
/* The same values in aggregation-CSR order, att[p*heads + h] (no perm): the per-head
 * weights of gnpde_head_aggregate_f32 (an entry point added under ABI 8).              */
int gnpde_edge_attention_csr_f32(const int32_t* rowidx, const int32_t* col, int64_t nnz,
                                 int norm_idx, int mode, int64_t heads, int64_t dk,
                                 const double* cs, const float* q, const float* k, int64_t ldqk,
                                 float score_p0, float score_p1, const double* m, const float* rl,
                                 float* att, void* stream);

/* ---------------------------------------------------------------- solver glue
 * out[i] = y0[i] + scale * sum_{j<nk} coef[j] * k_j[i]   (nk <= 8; y0 may be NULL = 0)
 * One pass for a Runge-Kutta stage input or step update (torchdiffeq
 * rk4_alt_step_func / _runge_kutta_step combinations).                      */
int gnpde_rk_combine_f32(int64_t n, const float* y0, int nk, const float* const* ks, const double* coef,
                         double scale, float* out, void* stream);

/* The row passes of the ODE regularisers (gnpde.regularized_ODE_function; entry points
 * added under ABI 8).  Arrays are [R, C] fp32, contiguous, 1 <= C <= 256; a team of lanes
 * of one wavefront owns a row (64 / L short rows per wavefront), 16-byte accesses when
 * C % 4 == 0 and every base is 16-byte aligned, a scalar form otherwise.  No atomics, a
 * fixed summation order per row: the same bits whatever the grid.
 *
 *   s[r] = sum_{i<n} coef[i] * sum_c ks[i][r,c]^2      (1 <= n <= 4; carried in fp64)
 *   acc (may be NULL): acc[r] = s[r], or acc[r] += s[r] with accumulate != 0 (fp64: the
 *       running regulariser state of a fused solve);
 *   out (may be NULL): out[r] = (float)s[r] (the per-RHS value).  One of the two at least. */
int gnpde_row_energy_f32(int64_t R, int64_t C, int n, const float* const* ks, const double* coef, double* acc,
                         int accumulate, float* out, void* stream);
/*   out[r,:] = base[r,:] + sum_{j<n} coef[j] * g[j][r] * src[j][r,:]     (0 <= n <= 2)
 * base may be NULL (= 0) and may be out itself; g[j] are [R], fp64 when g_f64 != 0, else
 * fp32.  Every element is an fp64 sum rounded to fp32 once.                              */
int gnpde_row_axpy_f32(int64_t R, int64_t C, const float* base, int n, const float* const* src,
                       const void* const* g, int g_f64, const double* coef, float* out, void* stream);

/* Entry of a solve (gnpde.integrator): dst[k] = src[order[k]] for k < rows
 * (order NULL: identity), rows of row_bytes bytes (a multiple of 16, 16-byte
 * aligned pointers); dst_copy (may be NULL) receives src unchanged,
 * dst_copy[order[k]] = src[order[k]], from the same read — the solution's
 * t0 slice and the renumbered working state in one pass.  No aliasing.      */
int gnpde_rows_copy(const void* src, int64_t rows, int64_t row_bytes, const int64_t* order, void* dst,
                    void* dst_copy, void* stream);

/* The early-stop test integrator's score of one state (gnpde.early_stop_solver;
 * src/early_stop_solver.py:108-128): for every row r < R of y [R, ld] whose split
 * mask is non-zero,
 *   z = relu(y[r, 0:Cd]),  logit[c] = b[c] + sum_j W[c, j] z[j]   (W [K, Cd] row-major,
 *   fp32 fused multiply-adds, j ascending; b NULL = 0),  pred = argmax_c logit[c]
 *   (the lowest class wins a tie),
 * and each set bit of the row's mask (bit 0 train, bit 1 validation, bit 2 test)
 * adds 1 to counts[bit] when pred equals the row's label.  counts[3] is ADDED to
 * (integer atomics): the caller zeroes it, or aims it at a slot of a per-solve
 * record.  rows (may be NULL = identity): state row r takes its mask and label from
 * split[rows[r]], label[rows[r]] (a state kept in a node renumbering; an entry
 * outside [0, R) leaves the row unscored).  pred_out (may be NULL): pred of state row
 * r, -1 for an unscored row.  A row with mask 0 is not read.  Cd <= ld (an augmented
 * state is scored on its first half).  One launch, no workspace, no host read.
 * GNPDE_EINVAL: K < 1, Cd < 1, Cd > ld, R < 0, a NULL required pointer;
 * GNPDE_EUNSUPPORTED: K > 128 or Cd > 512.                                   */
int gnpde_decode_score_f32(const float* y, int64_t R, int64_t ld, int64_t Cd, const float* W, const float* b,
                           int64_t K, const uint8_t* split, const int32_t* label, const int32_t* rows,
                           int32_t* counts, int32_t* pred_out, void* stream);

/* <a, b> of two fp32 arrays in fp64 (n elements), written to *out on the device:
 * the parameter gradients of the RHS backward, d alpha_train = sigma'(alpha)
 * <gf, A x - x> and d beta_train = <gf, x0> (torch autograd of
 * function_laplacian_diffusion.py:69-76).  Fixed reduction order (deterministic);
 * two launches; workspace: gnpde_dot_workspace_bytes().                      */
size_t gnpde_dot_workspace_bytes(void);
/* *out (+)= sum_i v[i] for n fp64 values (the per-row terms of the stage
 * epilogue's dot_rows), fixed order; accumulate: add to *out instead of storing.
 * Workspace gnpde_dot_workspace_bytes().                                      */
int gnpde_sum_f64(int64_t n, const double* v, double* out, int accumulate, void* workspace, size_t workspace_bytes,
                  void* stream);
int gnpde_dot_f64(int64_t n, const float* a, const float* b, double* out, void* workspace, size_t workspace_bytes,
                  void* stream);

/* The first step of an adaptive solve on the device: torchdiffeq's
 * _select_initial_step (RKAdaptiveStepsizeODESolver._before_integrate, order =
 * the tableau's order: 5 for dopri5) over n state elements, replacing the
 * Python-side torch elementwise chain and its host syncs (gnpde.integrator):
 *   scale = atol + |y0| rtol (fp32, as torch on an fp32 state)
 *   phase 0 (f1 == NULL): d0 = rms(y0/scale), d1 = rms(f0/scale),
 *     h[0] = h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 d0/d1, h[1] = d1,
 *     *hf = (float)h0 (the coef_scale of the probe y0 + h0 f0);
 *   phase 1 (f1 = f(t0 + h0, y0 + h0 f0)): d2 = rms((f1 - f0)/scale)/h0,
 *     h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? max(1e-6, 1e-3 h0) : (0.01/max(d1,d2))^(1/order),
 *     h[2] = min(100 h0, h1)  (reads h[0], h[1] of phase 0); *hf = (float)h[2] when hf
 *     is given (the first step's coef_scale, so the host need not write it).
 * Squares summed in fp64 in a fixed order (two launches per phase); h [3]
 * fp64 and hf are device memory.  Workspace gnpde_initial_step_workspace_bytes(). */
/* torchdiffeq's step-size controller after one adaptive step, on the device
 * (rk_common.py _optimal_step_size with the loop's accept test error_ratio <= 1),
 * fused with the reduction of the step's error rows (the stage epilogue's err_rows):
 *   e2    = sum_r err_rows[r]   (fixed order, as gnpde_sum_f64)
 *   ratio = sqrt(e2 / n)        (the RMS error ratio over n state elements)
 *   next  = ratio == 0 ? dt ifactor
 *         : dt min(ifactor, max(safety ratio^(-1/order), ratio < 1 ? 1 : dfactor))
 * rec[0..3] = {ratio, dt, next, e2}; *dt = next; *scale = (float)next (the
 * coef_scale of the next step's launches); t (ABI 8, NULL = none): the device
 * time of the solve, *t += dt when the step is accepted (ratio <= 1) — the step
 * start a folded dense output reads (stage dense_t).  Device pointers; two
 * launches; workspace gnpde_dot_workspace_bytes().                           */
int gnpde_adaptive_control(int64_t nrows, const double* err_rows, double n, double order, double safety,
                           double ifactor, double dfactor, double* dt, float* scale, double* rec, double* t,
                           void* workspace, size_t workspace_bytes, void* stream);
size_t gnpde_initial_step_workspace_bytes(void);
/* Phase 1 of gnpde_initial_step_f32 for an affine RHS f(y) = L y + s (ABI 8), from
 * v = L f0 (the linear part evaluated on f0, which is also the first step's u_1 / dt):
 *   d2 = rms(v / scale)   (= rms((f1 - f0)/scale)/h0 for f1 = f(y0 + h0 f0), without the
 *                          fp32 cancellation of f1 - f0)
 * then h[2] and *hf (when given) as phase 1; reads h[0], h[1] of phase 0.  scale, the
 * quotient and the fp64 squares as gnpde_initial_step_f32.  Two launches; workspace
 * gnpde_initial_step_workspace_bytes().                                        */
int gnpde_initial_step_lin_f32(int64_t n, const float* y0, const float* v, double atol, double rtol, double order,
                               double* h, float* hf, void* workspace, size_t workspace_bytes, void* stream);
int gnpde_initial_step_lin_bf16(int64_t n, const uint16_t* y0, const uint16_t* v, double atol, double rtol,
                                double order, double* h, float* hf, void* workspace, size_t workspace_bytes,
                                void* stream);
/* gnpde_initial_step_f32's scalar rules from per-row squared sums formed by the RHS
 * launches themselves (ABI 8; an affine RHS f(y) = L y + s): phase 0 (rows_b given)
 * with rows_a = the f0 launch's err_rows (e = f0, err_y1 = -2: sum (f0/scale)^2) and
 * rows_b = its scale_rows (sum (y0/scale)^2); phase 1 (rows_b NULL) with rows_a =
 * the err_rows of a launch evaluating L f0 (the linear part on f0, e = f): then
 *   d2 = rms(L f0 / scale)   (= rms((f1 - f0)/scale)/h0 for f1 = f(y0 + h0 f0))
 * and h[2], *hf as gnpde_initial_step_f32's phase 1.  scale = atol + rtol |y0| in
 * fp64 (the epilogue's tolerance), n the state's element count.  Two launches;
 * workspace gnpde_initial_step_workspace_bytes().                             */
int gnpde_initial_step_rows(int64_t nrows, const double* rows_a, const double* rows_b, double n, double order,
                            double* h, float* hf, void* workspace, size_t workspace_bytes, void* stream);
/* The squared sums of gnpde_initial_step_f32 without its scalar rules (ABI 7): the
 * per-component pieces of a mixed norm (torchdiffeq's adjoint norm: the max over the
 * components [y | adj_y | adj_params] of their RMS norms), the caller combining them:
 *   f1 == NULL: out[0] = sum (y0/scale)^2, out[1] = sum (f0/scale)^2
 *   else:       out[0] = sum ((f1 - f0)/scale)^2, out[1] = 0
 * scale = atol + |y0| rtol in fp32, squares in fp64, the fixed order of
 * gnpde_initial_step_f32.  Workspace gnpde_initial_step_workspace_bytes().     */
int gnpde_scaled_sq_sums_f32(int64_t n, const float* y0, const float* f0, const float* f1, double atol, double rtol,
                             double* out, void* workspace, size_t workspace_bytes, void* stream);
/* out[s] = sum_{i < len} v[s*len + i] for s < nseg (ABI 7): the row sums of several
 * epilogue channels of one adaptive step (the y and adjoint error rows, the alpha
 * integrand's rows of every stage) in one pass, each in a fixed order
 * (deterministic).  Workspace gnpde_segment_sums_workspace_bytes(nseg).        */
size_t gnpde_segment_sums_workspace_bytes(int64_t nseg);
int gnpde_segment_sums_f64(int64_t nseg, int64_t len, const double* v, double* out, void* workspace,
                           size_t workspace_bytes, void* stream);
int gnpde_initial_step_f32(int64_t n, const float* y0, const float* f0, const float* f1, double atol, double rtol,
                           double order, double* h, float* hf, void* workspace, size_t workspace_bytes, void* stream);
int gnpde_initial_step_bf16(int64_t n, const uint16_t* y0, const uint16_t* f0, const uint16_t* f1, double atol,
                            double rtol, double order, double* h, float* hf, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ---------------------------------------------------------------- backward
 * Gradients of the RHS f = a (A(w) x - x) [+ b x0] and of the attention that
 * produces w; torch autograd of the reference (function_laplacian_diffusion.py:
 * 39-77, function_transformer_attention.py:218-267, utils.py:116-127) restated
 * as graph passes.  All sums in a fixed order (no float atomics).
 *
 * d f / d w: g_out[perm[p]*heads + h] = a * <gf[rowidx[p]], x[col[p]]> / heads
 * for every head h < heads <= 64 (COO order; heads > 1: w is the head mean of [B,E,heads]).
 * a = sigmoid(*alpha) / *alpha / 1 (alpha NULL), as the RHS epilogue.        */
int gnpde_sddmm_f32(const int32_t* rowidx, const int32_t* col, const int32_t* perm, int64_t nnz, int64_t C,
                    const float* gf, int64_t ldg, const float* x, int64_t ldx, const float* alpha, int alpha_sigmoid,
                    int heads, float* g_out, void* stream);

/* Edge-softmax backward per group of a grouped CSR (rowptr, perm -> COO ids):
 * gs[i,h] = att[i,h] * (g[i,h] - sum_{j in grp(i)} att[j,h] g[j,h]), COO [nnz, heads]. */
int gnpde_softmax_backward_f32(const int32_t* rowptr, const int32_t* perm, int64_t R, int64_t nnz, int heads,
                               const float* att, const float* g, float* gs, void* stream);

/* out[r,h] = sum_{p in row r} vals[perm[p]*heads + h]  (fp64 out, [R, heads]). */
int gnpde_segment_sum_f64(const int32_t* rowptr, const int32_t* perm, int64_t R, int64_t nnz, int heads,
                          const float* vals, double* out, void* stream);

/* y[b][h][c] = sum_n w[b*N+n, h] x[b*N+n, c], y[b][h][C] = sum_n w[b*N+n, h]
 * (fp64, y is [B][heads][C+1]); workspace gnpde_wcolsum_workspace_bytes.    */
size_t gnpde_wcolsum_workspace_bytes(int64_t B, int64_t N, int64_t C, int heads);
int gnpde_wcolsum_f64(const float* x, int64_t B, int64_t N, int64_t C, int64_t ldx, const double* w, int heads,
                      double* y, void* workspace, size_t workspace_bytes, void* stream);

/* Input gradient of the reference-mode node scores cs = x U_b + v_b and of the
 * key sum xbar_b = sum_n deg[n] x_n:
 *   gx[n,c] (+)= sum_h gcs[n,h] U[b][c][h] + deg[n] gxbar[b][c]   (b = n / N). */
int gnpde_score_input_grad_f32(const double* gcs, const double* U, const int32_t* deg, const double* gxbar, int64_t B,
                               int64_t N, int64_t C, int heads, float* gx, int64_t ldgx, int accumulate,
                               void* stream);

/* out[p] = scale * w[perm[p]*heads + h]: one head of COO per-edge values in a
 * grouped CSR's order (per-head weights of the per-edge score backward).     */
int gnpde_gather_head_f32(const float* w, int64_t nnz, int heads, int h, const int32_t* perm, float scale, float* out,
                          void* stream);

/* Backward of the per-edge scores (SCORE_DOT / EXP_KERNEL / COSINE / PEARSON,
 * function_transformer_attention.py:246-259) onto the projections: over a
 * grouped CSR whose rows receive the gradient (side 0: the aggregation CSR,
 * rows = sources, own operand q; side 1: the CSC, rows = destinations, own k;
 * col = the other endpoint, perm -> COO ids), with gs [E, heads] = dL/ds in
 * COO order:
 *   out[r, h*dk + d] = sum_{e in row r} gs[e,h] * ds_e,h / d own[r, h*dk + d]
 * (out [R, ldo], overwritten; fixed order, deterministic).  For EXP_KERNEL and
 * gp != NULL also gp[e*2H + h] = gs * ds/d(output_var), gp[e*2H + H + h] =
 * gs * ds/d(lengthscale) (COO order; the caller sums them).  attention_dim
 * <= 1024.                                                                   */
int gnpde_score_grad_f32(const int32_t* rowptr, const int32_t* col, const int32_t* perm, int64_t R, int64_t nnz,
                         int side, int mode, int64_t heads, int64_t dk, const float* q, const float* k, int64_t ldqk,
                         float score_p0, float score_p1, const float* gs, float* out, int64_t ldo, float* gp,
                         void* stream);

/* gnpde_score_grad_f32's EXP_KERNEL path for heads made of two parts (the beltrami
 * product kernel folded into one exp_kernel): elements [0, dk_split) and
 * [dk_split, dk) of every head.  out as above (the gradient of the whole head); for gp !=
 * NULL, gp [nnz, 3*heads] in COO order, the squared distance summed per part:
 *   gp[e*3H + h]      = gs * 2 s / score_p0,
 *   gp[e*3H + H + h]  = gs * s * |own - oth|^2 over the first part  / score_p1^2,
 *   gp[e*3H + 2H + h] = gs * s * |own - oth|^2 over the second part / score_p1^2
 * (the caller sums the columns; fixed order, no atomics: deterministic).  0 <= dk_split
 * <= dk, attention_dim <= 1024.                                                          */
int gnpde_score_grad_split_f32(const int32_t* rowptr, const int32_t* col, const int32_t* perm, int64_t R, int64_t nnz,
                               int side, int64_t heads, int64_t dk, int64_t dk_split, const float* q, const float* k,
                               int64_t ldqk, float score_p0, float score_p1, const float* gs, float* out, int64_t ldo,
                               float* gp, void* stream);

/* ---- GAT attention function (function_GAT_attention.py: ODEFuncAtt, SpGraphAttentionLayer) ----
 * Node-score pairs sp [B*N, 2*heads] fp64 = [sl | sr] = x U, where U [C, 2*heads] is W
 * [C, att] (row-major) folded with a [2*dk] (dk = att / heads, the same a for every
 * head): U[c][h] = sum_d W[c, h*dk+d] a[d], U[c][heads+h] = sum_d W[c, h*dk+d] a[dk+d].
 * U is formed on the device (one workgroup per batch element, fp64) into the
 * workspace (gnpde_gat_scores_workspace_bytes), then x is read exactly once
 * (fp64 accumulation): 4*R*C bytes in, 16*heads*R out.  heads <= 8.
 * Restates wx = x W; edge_e = leakyrelu(sum(a * [wx_src | wx_dst])) without wx. */
size_t gnpde_gat_scores_workspace_bytes(int64_t B, int64_t C);
int gnpde_gat_scores_f32(const float* x, int64_t B, int64_t N, int64_t C, int64_t ldx, const float* W, const float* a,
                         int64_t att, int64_t heads, double* sp, void* workspace, size_t workspace_bytes,
                         void* stream);

/* K1 with the GAT attention weights formed in the gather loop:
 *   w_p = mean_h exp(leakyrelu(sl[row,h] + sr[col_p,h]) - m[g,h]) * rl[g,h],
 * g = row (norm_idx 0, statistics over the CSR) or col_p (norm_idx 1, over the CSC),
 * sp the pairs of gnpde_gat_scores_f32, m / rl the group statistics of mode
 * GNPDE_SCORE_GAT.  Equals gnpde_attn_weights_f32 (mode GAT) + gnpde_spmm_rhs_f32 bit
 * for bit, in one pass.  The wide (adaptive-solver) stage epilogue is fused with plain
 * weights only (GNPDE_EUNSUPPORTED here).  Other arguments as gnpde_spmm_rhs_f32.  */
int gnpde_attn_gat_rhs_f32(const int32_t* items, int64_t n_items, int32_t* heavy, int64_t n_heavy,
                           const int32_t* col, const double* sp, const double* m, const float* rl, int norm_idx,
                           int64_t heads, float slope, int64_t C, const float* x, int64_t ldx, const float* x0,
                           int64_t ldx0, const float* alpha, const float* beta, int flags, float* f, int64_t ldf,
                           float* partials, int64_t n_slots, const gnpde_stage_epilogue_t* stage, void* stream);

/* Backward of the GAT edge score through its LeakyReLU, edge-parallel over the
 * aggregation CSR (rowidx = source, col = destination, perm -> COO ids):
 *   ge[e,h] = gs[e,h] * (sl[src,h] + sr[dst,h] > 0 ? 1 : slope)   (COO [nnz, heads]). */
int gnpde_gat_score_backward_f32(const int32_t* rowidx, const int32_t* col, const int32_t* perm, int64_t nnz,
                                 int64_t heads, const double* sp, float slope, const float* gs, float* ge,
                                 void* stream);

/* ---- squareplus attention normalisation (opt['square_plus'], src/utils.py:129-140) ----
 *   M_b      = max over all edges e and heads h of s[b,e,h]   (one scalar per batch element)
 *   p        = 2 / (sqrt(t^2 + 4) - t),  t = s - M_b <= 0     (= (t + sqrt(t^2 + 4)) / 2, stable)
 *   rl[g,h]  = 1 / (sum of p over the edges of group g + 1e-16)
 *   att[e,h] = p[e,h] * rl[g(e),h],   w[e] = mean_h att[e,h]
 * Score modes REFERENCE, DOT, EXP_KERNEL, COSINE, PEARSON; UNIFORM and GAT return
 * GNPDE_EUNSUPPORTED.  Every sum and maximum has a fixed order (no float atomics).
 *
 * gnpde_score_max_f32: M [B] fp64 and amax [B] (optional) = the flat COO position
 * (b*E + e)*heads + h of the maximum, the smallest one among equal scores (-1 and M = 0
 * for E = 0).  rowptr / rowidx / col / perm: the aggregation CSR (rows = sources).
 * REFERENCE: the maximum of the node scores cs [B*N, heads] fp64 over the rows that have
 * an out-edge.  Per-edge modes: one pass over the edges, which also stores the scores
 * sc [B*E, heads] fp32 in COO order when sc != NULL (the later passes read them instead of
 * repeating the dk-long products).  Workgroup partials in the workspace, then a final pass. */
size_t gnpde_score_max_workspace_bytes(int64_t B);
int gnpde_score_max_f32(const int32_t* rowptr, const int32_t* rowidx, const int32_t* col, const int32_t* perm,
                        int64_t B, int64_t N, int64_t E, int mode, int64_t heads, int64_t dk, const double* cs,
                        const float* q, const float* k, int64_t ldqk, float score_p0, float score_p1, double* M,
                        int64_t* amax, float* sc, void* workspace, size_t workspace_bytes, void* stream);

/* rl [R, heads] over a plan of the groups' rows (gnpde_plan_build of the CSR, norm_idx 0, or
 * of the CSC, norm_idx 1 = group_is_dst): items {row, e_begin, e_end, slot}, a hub row's
 * chunk items store their sums to partials [n_slots * heads] fp64 and heavy {row,
 * first_slot, n_chunks, -} merges them in a fixed order.  gcol / gperm: the grouped CSR's
 * col and perm.  REFERENCE: p is per node — pn [R, heads] fp32 = p(cs - M_b) is written
 * here (the difference in fp64) and the statistics are a gather-sum of it; per-edge modes
 * read the stored scores sc.  rl of a row without edges is never read.                   */
int gnpde_squareplus_stats_f32(const int32_t* items, int64_t n_items, const int32_t* heavy, int64_t n_heavy,
                               const int32_t* gcol, const int32_t* gperm, int group_is_dst, int64_t R, int64_t N,
                               int mode, int64_t heads, const double* cs, const float* sc, const double* M, float* pn,
                               float* rl, double* partials, void* stream);

/* Head-mean weights w [nnz] in aggregation-CSR order / attention att [B*E, heads] in COO
 * order from (M, rl); rowidx / col / perm: the aggregation CSR.  REFERENCE reads pn,
 * the per-edge modes sc.  The counterparts of gnpde_attn_weights_f32 / gnpde_edge_attention_f32. */
int gnpde_squareplus_weights_f32(const int32_t* rowidx, const int32_t* col, const int32_t* perm, int64_t nnz,
                                 int64_t N, int norm_idx, int mode, int64_t heads, const float* pn, const float* sc,
                                 const double* M, const float* rl, float* w_out, void* stream);
int gnpde_squareplus_attention_f32(const int32_t* rowidx, const int32_t* col, const int32_t* perm, int64_t nnz,
                                   int64_t N, int norm_idx, int mode, int64_t heads, const float* pn, const float* sc,
                                   const double* M, const float* rl, float* att, void* stream);
/* gnpde_squareplus_attention_f32's values in aggregation-CSR order, att[p*heads + h] (perm still
 * locates the stored scores sc of the per-edge modes): the per-head weights of
 * gnpde_head_aggregate_f32 (an entry point added under ABI 8).                          */
int gnpde_squareplus_attention_csr_f32(const int32_t* rowidx, const int32_t* col, const int32_t* perm, int64_t nnz,
                                       int64_t N, int norm_idx, int mode, int64_t heads, const float* pn,
                                       const float* sc, const double* M, const float* rl, float* att, void* stream);

/* K1 with the squareplus weights of the reference scores under destination groups formed
 * in the gather loop: w_p = (1/heads) sum_h pn[row,h] * rl[col_p,h] (no transcendental per
 * edge).  Equals gnpde_squareplus_weights_f32 + gnpde_spmm_rhs_f32 bit for bit, in one
 * pass.  The wide (adaptive-solver) stage epilogue is fused with plain weights only
 * (GNPDE_EUNSUPPORTED here).  Other arguments as gnpde_spmm_rhs_f32.                      */
int gnpde_attn_sp_rhs_f32(const int32_t* items, int64_t n_items, int32_t* heavy, int64_t n_heavy, const int32_t* col,
                          const float* pn, const float* rl, int64_t heads, int64_t C, const float* x, int64_t ldx,
                          const float* x0, int64_t ldx0, const float* alpha, const float* beta, int flags, float* f,
                          int64_t ldf, float* partials, int64_t n_slots, const gnpde_stage_epilogue_t* stage,
                          void* stream);

/* Backward of the squareplus normalisation over the groups of a grouped CSR (COO
 * [nnz, heads] in and out, nnz = B*E).  With p = att / rl and r = sqrt(t^2 + 4) = p + 1/p:
 *   gs' = att / r * (g_att - sum over the group of att * g_att)
 *   gs  = gs' - [position == amax[b]] * (sum over all e, h of gs'[b])    (the max term)
 * No score is recomputed.                                                                */
size_t gnpde_squareplus_backward_workspace_bytes(int64_t B);
int gnpde_squareplus_backward_f32(const int32_t* rowptr, const int32_t* perm, int64_t R, int64_t nnz, int64_t B,
                                  int heads, const float* att, const float* g_att, const float* rl,
                                  const int64_t* amax, float* gs, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* Exact k nearest neighbours of the rows of x [B, N, C] (row stride ld) within each graph, by
 * the squared distance d_ij = sum_c (x_ic - x_jc)^2 in fp32 (the difference form; the self
 * index is a candidate, d_ii = 0), in ascending (d_ij, j): the kNN rewiring of
 * src/graph_rewiring.py:122-161 (an entry point added under ABI 8).  A row that is all
 * zero or holds a non-finite value is masked: never a candidate, and as a query it
 * returns its own index k times (distance 0).  idx_out [B, N, k] holds per-graph indices
 * in [0, N); dist_out [B, N, k] (or NULL) the distances; n_valid [B] the unmasked rows of
 * each graph, written by the mask pre-pass (a graph with n_valid < k pads its rows with
 * index -1 / distance +inf).  workspace: gnpde_knn_workspace_bytes(B, N) bytes (the row
 * masks).  1 <= k <= 64, else GNPDE_EUNSUPPORTED.  Everything is enqueued on the stream;
 * the result does not depend on the launch geometry.                                   */
size_t gnpde_knn_workspace_bytes(int64_t B, int64_t N);
int gnpde_knn_f32(const float* x, int64_t B, int64_t N, int64_t C, int64_t ld, int64_t k, int32_t* idx_out,
                  float* dist_out, int32_t* n_valid, void* workspace, void* stream);

/* Cross-attention of the node rows against a second modality's tokens (multi_modal,
 * src/function_laplacian_diffusion.py:61-63; an entry point added under ABI 8):
 *   out[b,n,:] = softmax_m(scale * <q[b,n,:], k[b,m,:]>) v[b,m,:]
 * q [B, N, C] (row stride ldq), k / v [B, M, C] contiguous, out [B, N, C] (row stride ldo).
 * Flash style on the fp32 matrix cores (exact fp32 products): the [N, M] scores are never
 * stored.  lse [B*N] (or NULL) receives max_m + ln(sum_m exp) of the scaled scores, from
 * which a backward recomputes the softmax.  1 <= C <= 256, else GNPDE_EUNSUPPORTED; any
 * N >= 0 and M >= 1.  No atomics, a fixed reduction order: the same bits on every run.  */
int gnpde_cross_attention_f32(const float* q, int64_t ldq, const float* k, const float* v, int64_t B, int64_t N,
                              int64_t M, int64_t C, float scale, float* out, int64_t ldo, float* lse, void* stream);

/* The Adams-Bashforth-Moulton multistep solvers (gnpde.integrator: explicit_adams /
 * implicit_adams; entry points added under ABI 8).  fp32 arrays of n elements, no
 * aliasing except where stated; everything is enqueued on the stream.
 *
 * Predictor: one read of y0 and of each of the nh (1 <= nh <= GNPDE_ADAMS_MAX_HISTORY)
 * history arrays hist[j] (newest first),
 *   dy[i]    = fl32(sum_j cdy[j] hist[j][i])
 *   x[i]     = fl32(y0[i] + sum_j cdy[j] hist[j][i])
 *   delta[i] = fl32(sum_j cdelta[j] hist[j][i])        (delta and cdelta both NULL: skipped)
 * each sum carried in fp64 per element (j ascending, fused multiply-adds) and rounded to
 * fp32 once at its store; the coefficients arrive multiplied by dt.                      */
#define GNPDE_ADAMS_MAX_HISTORY 11
int gnpde_adams_predict_f32(int64_t n, const float* y0, int nh, const float* const* hist, const double* cdy,
                            const double* cdelta, float* dy, float* x, float* delta, void* stream);

/* The corrector's device status record (16 bytes) followed by the reduction's arrival
 * counter; the workspace of gnpde_adams_correct_f32 starts with one.                     */
typedef struct {
  int32_t converged;  /* 1 once an iteration's ratio was < 1                                */
  int32_t iterations; /* corrector iterations applied (launches that were not gated off)    */
  float ratio;        /* the last applied iteration's convergence ratio (NaN propagates)    */
  int32_t reserved;
  uint32_t arrivals;  /* workgroups that finished the running launch (0 between launches)   */
  uint32_t pad[3];
} gnpde_adams_status_t;
size_t gnpde_adams_workspace_bytes(void);
/* Zero the status record and the arrival counter (a memset node; once per step).         */
int gnpde_adams_status_reset(void* workspace, void* stream);
/* One corrector iteration, gated: a launch that finds status.converged set returns without
 * touching dy, x or the status.  Otherwise, with d = dy[i] before the launch,
 *   dy[i] = fl32(cf f[i] + delta[i])         (fp64 multiply-add, one rounding)
 *   x[i]  = fl32(y0[i] + cf f[i] + delta[i]) (the same fp64 sum, one rounding)
 *   ratio = max_i |d - dy[i]| / (atol + rtol max(|d|, |dy[i]|))   (numerators and denominators
 *           in fp64 per element, compared by cross-multiplication; a NaN quotient anywhere
 *           (a NaN operand, 0 / 0, inf / inf) makes the ratio NaN)
 * and status becomes {converged = ratio < 1, iterations + 1, ratio}.  The ratio is reduced
 * per workgroup and finished by the workgroup that arrives last: a fixed reduction of a
 * maximum, the same bits on every run.  workspace: gnpde_adams_workspace_bytes() bytes,
 * 16-byte aligned, reset by gnpde_adams_status_reset before the first iteration of a step. */
int gnpde_adams_correct_f32(int64_t n, const float* f, const float* delta, const float* y0, double cf, double rtol,
                            double atol, float* dy, float* x, void* workspace, size_t workspace_bytes, void* stream);

/* The two-hop product of the rewire_attention block (gnpde.block_transformer_rewiring,
 * src/block_transformer_rewiring.py:65-93; entry points added under ABI 8).  W is a
 * COALESCED CSR of N rows: int32 rowptr [N+1] and col (values in [0, N), ascending inside
 * a row, no duplicates — caller-validated), fp32 val.  The product's positions are the
 * structural non-zeros of W·W (some m with (i, m) and (m, j) stored), in ascending
 * (row, column) order, each once, the diagonal included; their values
 *   S[i, j] = 0.5 * ((sum_m W[i, m] W[m, j]) + W[i, j]),   S[i, i] = 0,
 * the sum an fma chain over the m of row i in CSR order, W[i, j] added after it, the
 * halving exact: no floating-point atomic, the same bits on every call.
 *
 * gnpde_coalesce_sum_f32 (the prep pass): w_sorted [E] in (row, column) order, first[p] = 1
 * where p starts a run of equal (row, column), uid[p] = the run's index; out[uid] = the run's
 * sum, its entries added one after another in that order.
 * gnpde_two_hop_bound_i32: ub[i] = sum over the m of row i of len(row m), the upper bound of
 * row i's width that selects its regime: 0 nothing, <= lds_max a hash table in LDS
 * (lds_max <= gnpde_two_hop_lds_max()), beyond it a dense accumulator acc [n_waves * N] fp32
 * and a bitmap bits [n_waves * ceil(N / 32)] (ZERO on entry, zero again on return) in global
 * scratch, one slice per resident wavefront (1 <= n_waves <= 65536).
 * gnpde_two_hop_count_i32 (symbolic): count[i] = positions of row i.  The caller forms
 * out_ptr [N+1], the exclusive scan, and nnz_out = out_ptr[N] < 2^31.
 * gnpde_two_hop_fill_f32 (numeric): out_col / out_val [nnz_out] and the COO list
 * out_ei [2, nnz_out] (int64) in the same order.  ub, lds_max as in the symbolic pass.    */
int gnpde_two_hop_lds_max(void);
int gnpde_coalesce_sum_f32(const float* w_sorted, const uint8_t* first, const int64_t* uid, int64_t E, float* out,
                           void* stream);
int gnpde_two_hop_bound_i32(const int32_t* rowptr, const int32_t* col, int64_t N, int32_t* ub, void* stream);
int gnpde_two_hop_count_i32(const int32_t* rowptr, const int32_t* col, int64_t N, const int32_t* ub, int64_t lds_max,
                            int64_t n_waves, float* acc, uint32_t* bits, int32_t* count, void* stream);
int gnpde_two_hop_fill_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N, const int32_t* ub,
                           int64_t lds_max, int64_t n_waves, float* acc, uint32_t* bits, const int32_t* out_ptr,
                           int64_t nnz_out, int32_t* out_col, float* out_val, int64_t* out_ei, void* stream);

/* ---------------------------------------------------------------- column top-k
 * The sparsification of a GDC diffusion block (gnpde.ops.gdc; PyG GDC's `topk` with dim = 0,
 * src/graph_rewiring.py:50-51; entry points added under ABI 8): for every column c < ncols
 * of the row-major block y [N, ld] (fp32, finite values of either sign) the k entries that
 * are largest in the total order (value descending, row ascending; -0 counts as +0), in that
 * order:
 *   idx_out [ncols, k] the rows, val_out [ncols, k] their values,
 *   wnorm_out [ncols, k] (NULL: not written) = val / (val_0 + val_1 + ... + val_{k-1}), the
 *   sum taken sequentially in rank order in fp32, 0 when the sum is 0.
 * The rows are split into runs of rows_per_wg rows (rounded up to a multiple of 64; 0 = chosen
 * from the shape) that workgroups scan on their own; with more than one run their sorted
 * partial lists go through `workspace` (gnpde_topk_cols_workspace_bytes of the same N, ncols,
 * k, rows_per_wg; 8-byte aligned) and are merged in the same key order, so the outputs do
 * not depend on rows_per_wg.  No floating-point atomics: the same bits on every call.
 * 1 <= k <= 128, otherwise GNPDE_EUNSUPPORTED; k > N or ncols > ld: GNPDE_EINVAL; all
 * arguments are validated on the host before any launch.                              */
size_t gnpde_topk_cols_workspace_bytes(int64_t N, int64_t ncols, int64_t k, int64_t rows_per_wg);
int gnpde_topk_cols_f32(const float* y, int64_t N, int64_t ncols, int64_t ld, int64_t k, int32_t* idx_out,
                        float* val_out, float* wnorm_out, int64_t rows_per_wg, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- positional-encoding distances
 * The pos_enc_knn rewiring (gnpde.graph_rewiring.apply_pos_dist_rewire,
 * src/graph_rewiring.py:318-375; entry points added under ABI 8).  With d_ij = sum_c (x_ic -
 * x_jc)^2 in fp32 (the difference form of gnpde_knn_f32) the rank value of a pair is
 *   u_ij = d_ij (r_i r_j),   r_i = 1 / max(1 - |x_i|^2, 2^-52)  (GNPDE_METRIC_POINCARE; |x|^2,
 *                            1 - |x|^2 and r in fp64, r rounded to fp32 once)
 *                            r_i = 1                             (GNPDE_METRIC_EUCLID)
 * and the distance D = arccosh(1 + 2 u) (Poincare) or sqrt(u) (Euclid) is monotone in it: all
 * ranking is done on the fp32 u.  u_ij and u_ji are bit-equal, and every entry point below
 * computes the same bits for a pair.  The [N, N] matrix is never stored.
 *
 * gnpde_pos_knn_f32: the contract of gnpde_knn_f32 (ascending (u, j), the self index a
 * candidate, 1 <= k <= 64) except that only a row with a non-finite value is masked (an
 * all-zero row is the origin, a point like any other) and that dist_out (or NULL) holds D:
 * sqrt(u), or log1p(2 u + 2 sqrt(u (u + 1))).  workspace: gnpde_pos_knn_workspace_bytes(B, N)
 * bytes, 16-byte aligned (the masks and r).
 *
 * gnpde_pair_select_f32 (one graph): *u_out = the u of 0-based rank `rank` among all N^2
 * entries in ascending order, the diagonal included; *count_le_out = the number of entries
 * with u <= *u_out.  A most-significant-first radix select on the bits of u (digits of 11, 11
 * and 10 bits: three sweeps over the tiles on and above the diagonal); all counts are 64-bit
 * integers and only integer atomics are used: the same bits on every call.  An entry of a row
 * with a non-finite value ranks as +inf.
 *
 * gnpde_pair_threshold_count_f32: row_count[i] = #{j : u_ij <= *u_thr}.
 * gnpde_pair_threshold_fill_f32: with row_ptr [N] the exclusive scan of row_count and E its
 * total, ei_out [2, E] (int64) = the pairs (i, j) with u_ij <= *u_thr, i ascending and j
 * ascending within i (numpy.where order): ei_out[0] the rows, ei_out[1] the columns.
 *
 * workspace of the three pair entry points: gnpde_pair_workspace_bytes(N) bytes, 16-byte
 * aligned, linear in N (r, one 2048-bin histogram, the select's state).  1 <= N <= 2^24 (N =
 * 0: nothing to do, except for the select), else GNPDE_EUNSUPPORTED; all arguments are
 * validated on the host before any launch.                                              */
#define GNPDE_METRIC_EUCLID 0
#define GNPDE_METRIC_POINCARE 1
size_t gnpde_pos_knn_workspace_bytes(int64_t B, int64_t N);
int gnpde_pos_knn_f32(const float* x, int64_t B, int64_t N, int64_t C, int64_t ld, int64_t k, int metric,
                      int32_t* idx_out, float* dist_out, int32_t* n_valid, void* workspace, void* stream);
size_t gnpde_pair_workspace_bytes(int64_t N);
int gnpde_pair_select_f32(const float* x, int64_t N, int64_t C, int64_t ld, int metric, int64_t rank, float* u_out,
                          int64_t* count_le_out, void* workspace, size_t workspace_bytes, void* stream);
int gnpde_pair_threshold_count_f32(const float* x, int64_t N, int64_t C, int64_t ld, int metric, const float* u_thr,
                                   int64_t* row_count, void* workspace, size_t workspace_bytes, void* stream);
int gnpde_pair_threshold_fill_f32(const float* x, int64_t N, int64_t C, int64_t ld, int metric, const float* u_thr,
                                  const int64_t* row_ptr, int64_t E, int64_t* ei_out, void* workspace,
                                  size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNPDE_H_ */
