/*
 * pcacc.h -- C ABI of libpcacc_hip.so, the MI355X (gfx950) implementation of the PCAccumulation
 * per-frame forward hot path.
 *
 * The reference has no FFI for this path: it is Python calling torch / torch_scatter / numba and one
 * JIT-built torch extension (chamfer_distance).  Each entry point below therefore names the Python
 * (or C++) interface of the reference it stands in for, `file:line` relative to the reference root.
 * The host mirror (the .py files in pcaccumulation_amd/) binds these with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its comment says "host";
 *   - no allocation, no synchronisation, no global state: the caller owns all buffers, passes scratch
 *     through `workspace` (size from the matching *_workspace_bytes) and the HIP stream to launch on;
 *   - return value: 0 on success, a negative PCACC_E_* code otherwise (launch errors are reported,
 *     never printed-and-ignored as chamfer_distance.cu:152-154 does);
 *   - tensors are dense row-major; BEV canvases and feature maps are CHANNELS-LAST
 *     ([frame, y, x, channel]) -- the layout the scatter/gather kernels coalesce on;
 *   - `dtype` arguments: PCACC_F32 or PCACC_BF16 for the canvas / feature-map element type.
 */
#ifndef PCACC_H_
#define PCACC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCACC_OK 0
#define PCACC_E_ARG (-1)      /* bad argument (null pointer, negative size, unsupported channel count) */
#define PCACC_E_WORKSPACE (-2) /* workspace too small */
#define PCACC_E_LAUNCH (-3)   /* hipGetLastError() != hipSuccess after a launch */

#define PCACC_F32 0
#define PCACC_BF16 1

/* Library / build identification: returns the gfx target string the kernels were compiled for. */
const char *pcacc_target(void);

/* torch.cat((a, b), 1) of two channels-last maps as rows: out [rows, a_row_bytes + b_row_bytes] = a [rows, a_row_bytes] | b [rows, b_row_bytes]; row sizes
 * and pointers multiples of 16 bytes.  The decoder concatenations of models/unet.py:101-113. */
int pcacc_cat2_rows(const void *a, int32_t a_row_bytes, const void *b, int32_t b_row_bytes, int64_t rows, void *out, void *stream);

/* The launchers' switches (PCACC_CONV_FRAME_MAJOR, PCACC_CONV_SWZ_OFF, PCACC_CONV_RES, PCACC_ROWS_FM_OFF, PCACC_CONV_PLAN, PCACC_XCD_REMAP: the ones
 * the equality tests set; the scatter-variant switches of rounds 5 and 6 are retired) are read from the environment once per process; this reads
 * them again.  Returns 0. */
int pcacc_reload_switches(void);

/* ------------------------------------------------------------------------------------------------
 * A1. 4-D pillar voxelisation, first-touch numbering, bit-exact.
 * Replaces libs/voxel_generator.py:4-61 (_points_to_voxel_reverse_kernel), :64-114 (points_to_voxel)
 * and the array part of Voxelization.__call__ (:131-154).
 *   points      [n,4] f32 (x,y,z,t)
 *   voxel_size  host float[3], range host float[6] (xyz min, xyz max)
 *   coords      [max_voxels,4] i32 (z,y,x,t); rows >= *num_voxels are left untouched
 *   p2v         [n] i32, pillar id or -1 (out of range, t outside [0,nt), or beyond max_voxels)
 *   num_voxels  [1] i32 (device)
 * Pillar ids are the order in which cells are first touched when the points are visited in index
 * order, exactly as the sequential reference numbers them.
 * ---------------------------------------------------------------------------------------------- */
int pcacc_voxelize_workspace_bytes(int64_t n, int nx, int ny, int nz, int nt, size_t *bytes /*host*/);
int pcacc_voxelize(const float *points, int64_t n, const float *voxel_size, const float *range,
                   int nx, int ny, int nz, int nt, int max_voxels,
                   int32_t *coords, int32_t *p2v, int32_t *num_voxels,
                   void *workspace, size_t workspace_bytes, void *stream);

/* A1 + A2 for a whole batch of samples that already live in HBM: libs/dataset.py:183-199 (the voxelisation at the end of prep_input, per sample) and
 * libs/dataloader.py:7-40 (collate_fn: concatenation, the batch column, pillar ids offset by the pillars of the samples before) in ONE set of launches.
 *   points[b] [n_b,3] f64, time[b] [n_b] i64 (frame index), sd / inst / fb [b] [n_b] i64 (each of the three arrays may be NULL): DEVICE pointers in HOST
 *   arrays of n_samples <= 16 entries; counts host int64 [n_samples], every n_b >= 1.
 *   points_out [N,3] f64, time_out [N,2] f64 (sample, frame), sd_out / inst_out / fb_out [N] i64, coords_out [capacity >= N, 5] f64 rows
 *   (sample, z, y, x, t) in first-touch order (rows >= the total pillar count untouched), p2v_out [N] i32 (row of coords_out; a point outside the grid or with t outside [0, nt) gets
 *   (pillars of the samples before its own) - 1, what collate_fn's blind offset makes of its -1), num_voxels [n_samples] i32 -- all device.  Bit-identical to pcacc_voxelize per sample + the reference's collate_fn. */
int pcacc_collate_voxelize_workspace_bytes(int64_t n_total, int32_t n_samples, int nx, int ny, int nz, int nt, size_t *bytes /*host*/);
int pcacc_collate_voxelize(const double *const *points /*host*/, const int64_t *const *time /*host*/, const int64_t *const *sd /*host*/,
                           const int64_t *const *inst /*host*/, const int64_t *const *fb /*host*/, const int64_t *counts /*host*/, int32_t n_samples,
                           const float *voxel_size, const float *range, int nx, int ny, int nz, int nt, double *points_out, double *time_out,
                           int64_t *sd_out, int64_t *inst_out, int64_t *fb_out, double *coords_out, int32_t *p2v_out, int32_t *num_voxels,
                           void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * A2'. Decode the collated `coordinates` tensor once per forward.
 * Replaces the index arithmetic repeated in models/pillar_encoder.py:153-158 and :188-197:
 * cell = b*nt*ny*nx + t*ny*nx + y*nx + x from rows (b,z,y,x,t).
 *   coords        [m,5] f64 (collate_fn layout, libs/dataloader.py:18-20) when coords_is_f64 != 0,
 *                 else [m,5] i32
 *   cell          [m] i32
 *   cell2pillar   [n_batch*nt*ny*nx] i32: pillar id occupying the cell, -1 if empty; on duplicate
 *                 cells the highest pillar id wins ("later writes win", pillar_encoder.py:163)
 * ---------------------------------------------------------------------------------------------- */
int pcacc_cell_index(const void *coords, int coords_is_f64, int64_t m, int nx, int ny, int nt, int n_batch,
                     int32_t *cell, int32_t *cell2pillar, void *stream);

/* Occupied pillars of every frame in ascending cell order -- the order in which
 * models/egomotion.py:419-424 enumerates them through the boolean occupancy mask.
 *   sorted_pillars [m] i32; frame_offsets [n_frames+1] i32 (n_frames = n_batch*nt) */
int pcacc_frame_pillars_workspace_bytes(int64_t n_cells, size_t *bytes /*host*/);
int pcacc_frame_pillars(const int32_t *cell2pillar, int64_t n_cells, int64_t cells_per_frame,
                        int32_t *sorted_pillars, int32_t *frame_offsets,
                        void *workspace, size_t workspace_bytes, void *stream);

/* Indices of the non-zero entries of a byte mask, ascending: the boolean-mask indexing of models/motionnet.py:222-243 (`points[fb_mask]`,
 * `inst_labels[rec_mask]`) and models/egomotion.py:419-424 (background pillars), as ONE index list the caller gathers with -- the reference
 * re-evaluates the mask at every indexed tensor.  Wave ballot + popcount per 2048-entry chunk, a one-workgroup scan of the chunk sums, ranks by
 * ballot prefix inside a wave ([r5]: replaces three torch.nonzero_static calls = 0.3 ms of library select kernels behind the forward's host sync).
 *   mask [n] u8 (torch.bool); indices [capacity] i64: the first min(count, capacity) entries are written; count_out [1] i32 may be NULL */
int pcacc_compact_mask_workspace_bytes(int64_t n, size_t *bytes /*host*/);
int pcacc_compact_mask(const uint8_t *mask, int64_t n, int64_t *indices, int64_t capacity, int32_t *count_out,
                       void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Point -> pillar CSR (points grouped by pillar, ascending point index inside a pillar for
 * pillars of <= 64 points).  Internal layout shared by every per-pillar reduction below; it is what
 * removes the atomics torch_scatter uses (models/motionnet.py:159-160, models/pillar_encoder.py:116,120).
 *   p2v [n] i32 (all >= 0), seg_offsets [m+1] i32, order [n] i32
 * ---------------------------------------------------------------------------------------------- */
int pcacc_csr_workspace_bytes(int64_t n, int64_t m, size_t *bytes /*host*/);
int pcacc_csr_build(const int32_t *p2v, int64_t n, int64_t m, int32_t *seg_offsets, int32_t *order,
                    void *workspace, size_t workspace_bytes, void *stream);

/* A3. scatter(points, p2v, 'mean') and scatter(fb_labels, p2v, 'max') -- models/motionnet.py:159-160.
 *   points [n,3] f32; labels [n] i64 or NULL; mean [m,3] f32; max_label [m] i64 (ignored if labels NULL) */
int pcacc_segment_mean3_maxlabel(const float *points, const int64_t *labels, const int32_t *seg_offsets,
                                 const int32_t *order, int64_t m, float *mean, int64_t *max_label, void *stream);

/* A4 (pooling step). scatter(net, p2v, dim=0, reduce='max') -- models/pillar_encoder.py:116,120.
 *   src [n,c] f32, c % 4 == 0, c <= 256; out [m,c] f32; arg [m,c] i32 = lowest point index attaining
 *   the maximum (the element torch_scatter routes the gradient to), -1 for an empty segment (value 0).
 *   When n/m > 16 (the per-instance poolings of models/tpointnet.py:227-259, few rows with thousands of
 *   inputs each) the reduction runs in two levels over 64-row pieces and needs the workspace. */
int pcacc_segment_workspace_bytes(int64_t n, int64_t m, int c, size_t *bytes /*host*/);
int pcacc_segment_max(const float *src, int c, const int32_t *seg_offsets, const int32_t *order, int64_t n, int64_t m,
                      float *out, int32_t *arg, void *workspace, size_t workspace_bytes, void *stream);
/* Backward of segment_max followed by the [p2v] gather is not needed separately: both reduce to
 * grad_src[i,k] += grad_out[p2v[i],k] * (arg[p2v[i],k] == i). */
int pcacc_segment_max_backward(const float *grad_out, const int32_t *arg, const int32_t *p2v, int64_t n, int c,
                               float *grad_src, void *stream);

/* Per-pillar sum of point rows: the backward of the `[point_to_voxel_map]` broadcast that follows each
 * pooling (models/pillar_encoder.py:116).  src [n,c] f32, out [m,c] f32, c % 4 == 0, c <= 256. */
int pcacc_segment_sum(const float *src, int c, const int32_t *seg_offsets, const int32_t *order, int64_t n, int64_t m,
                      float *out, void *workspace, size_t workspace_bytes, void *stream);
/* The same three with the element type of the rows as a parameter (PCACC_F32 | PCACC_BF16; reductions in f32).  Short
 * segments (n/m <= 16, the pillar encoder): results in the rows' type.  Long segments (the per-instance poolings): rows in
 * either type, results always f32.  max_backward: grad_out and grad_src types are independent. */
int pcacc_segment_max_t(const void *src, int dtype, int c, const int32_t *seg_offsets, const int32_t *order, int64_t n,
                        int64_t m, void *out, int32_t *arg, void *workspace, size_t workspace_bytes, void *stream);
/* segment_max on f32 rows of SHORT segments with a second output: out16 [m,c] = `out` rounded to bf16, from the same store (the 'mixed' mode's
 * shadow of the pooled rows: models/pillar_encoder.py:116,120 -- it was a conversion pass over [m,c] after each of the three poolings).
 * PCACC_E_ARG when the segments are long (n / m > 16: the two-level reduction has no second output). */
int pcacc_segment_max_dual(const float *src, int c, const int32_t *seg_offsets, const int32_t *order, int64_t n, int64_t m, float *out,
                           uint16_t *out16, int32_t *arg, void *workspace, size_t workspace_bytes, void *stream);
int pcacc_segment_max_backward_t(const void *grad_out, int dtype, const int32_t *arg, const int32_t *p2v, int64_t n, int c,
                                 void *grad_src, int out_dtype, void *stream);
int pcacc_segment_sum_t(const void *src, int dtype, int c, const int32_t *seg_offsets, const int32_t *order, int64_t n,
                        int64_t m, void *out, void *workspace, size_t workspace_bytes, void *stream);
/* max_backward added into grad_src (in/out): the rows' gradient from their other consumer is already there -- the pooled PFN blocks,
 * models/pillar_encoder.py:116-118, where `net` feeds both the max-pool and the concatenation.  out_amax: 256 zeroed f32 slots that
 * receive the largest magnitude of the sums (pcacc_absmax256 layout), or NULL. */
int pcacc_segment_max_backward_acc(const void *grad_out, int dtype, const int32_t *arg, const int32_t *p2v, int64_t n, int c,
                                   void *grad_src, int out_dtype, float *out_amax, void *stream);

/* A4 (feature build). The nine per-point inputs of the pillar encoder -- models/pillar_encoder.py:98-110:
 * [xyz, xyz - pillar_mean, xy - pillar_centre, t], first eight divided by `scale` (= |x_min|), t by n_frames.
 *   points [n,3] f32; p2v [n] i32; pillar_mean [m,3] f32; coords [m,5] (b,z,y,x,t) f64 or i32;
 *   time_col: pointer to the t entry of row 0 of the collated `time_indice` (f64), time_stride = row stride in doubles (2);
 *   vx, vy = pillar size; x_offset = vx/2 + x_min, y_offset = vy/2 + y_min (pillar_encoder.py:91-94); out [n,9] f32. */
int pcacc_pfn_features(const float *points, const int32_t *p2v, const float *pillar_mean, const void *coords,
                       int coords_is_f64, const double *time_col, int64_t time_stride, int64_t n,
                       double vx, double vy, double x_offset, double y_offset, float scale, float n_frames,
                       float *out, void *stream);
/* The same rows in the order of `order` [n] i32 (row r = point order[r]; NULL = point order): with the point -> pillar CSR's point list the rows come out
 * pillar-major like the reference's own [M, max_points, C] tensor (libs/voxel_generator.py:41-58) and every per-pillar pass behind this call streams. */
int pcacc_pfn_features_ordered(const float *points, const int32_t *p2v, const float *pillar_mean, const void *coords,
                               int coords_is_f64, const double *time_col, int64_t time_stride, int64_t n,
                               double vx, double vy, double x_offset, double y_offset, float scale, float n_frames,
                               const int32_t *order, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * A4 (MLP part). Per-point linear layers: nn.Linear applied to 10^5..10^6 rows with <= 128 features, as the pillar
 * encoder (models/pillar_encoder.py:46-55, 112-121), the STPN point heads (models/stpn.py:94-102) and the TubeNet
 * embeddings (models/tpointnet.py:170-193) use them.  One HBM pass per layer.
 *   y[r,:] = post( pre(x[r,:]) @ w^T + bias + residual[r,:] )
 *   x [rows,k] f32, k in {2,3,4,9,32,64,128}; w [n,k] f32, n <= 128; bias [n] or NULL; residual [rows,n] or NULL
 *   flags: 1 = ReLU on x at load, 2 = ReLU on y before the store
 *   in_mask [rows,k] or NULL: x is zeroed where in_mask <= 0;  out_mask [rows,n] or NULL: y is zeroed where out_mask <= 0
 * The backward-data pass is the same entry point with w transposed, the forward output as in_mask (post-ReLU layers)
 * and the forward input as out_mask (pre-ReLU layers).
 *
 * The mask rule of EVERY row entry point, in all three compute modes -- in_mask, out_mask, out_mask_a / out_mask_b and dy_mask of
 * pcacc_rows_linear, _few_dual, _mixed, _bf16, _cat_bf16, _split, _split_dual, _cat_split and of pcacc_rows_wgrad, _mixed, _few, _bf16,
 * _cat_bf16, _split, _cat_split: an element is KEPT where its mask element is > 0 and zeroed everywhere else.  -1, -0.0, +0.0 and NaN
 * (either sign) drop; the smallest positive normal keeps.  "<= 0" above and below is shorthand for "not > 0".
 *   Where this differs from the library: aten::threshold_backward(grad, y, 0) keeps grad where y is NaN (NaN <= 0 is false); these
 *   kernels zero it.  A NaN mask element is a NaN forward activation: the step's loss is NaN already and the step is skipped by the
 *   non-finite check of the gradient norm (toolbox/utils.py:147-157), so no training step's gradient depends on the choice; one rule for all of them is what the kernels implement
 *   (mm_mask2, x3_mask4, `!(m > 0)` in mlp.hip) and what tests/test_rows_exact.py holds them to.  The convolution kernels keep on NaN
 *   (conv_mask2, x3_outmask4): a separate contract.
 *   ReLU on load / before the store (flags, x_relu) is max(v, 0) with -0.0 -> +0.0; the PFN blocks' x > 0 / h > 0 decisions follow the
 *   same "> 0" rule (xmask / hmask bits, and the bf16 block's tests of x and relu_h in its backward).
 * Where a bf16 value is held (tests/test_rows_exact.py checks each as "the exact value rounded once, to nearest even"):
 *   y of pcacc_rows_linear_bf16 / _cat_bf16 (and y2), y of _mixed with dtypes bit 16, y16 of _few_dual / _split_dual;
 *   with a residual the bf16 kernels round TWICE, y = bf16(bf16(x w^T + bias) + residual): the result tile is staged as bf16 before the
 *   coalesced store phase adds the residual -- the sequence of an unfused bf16 chain (linear, then add).  Weights are rounded to bf16
 *   once per launch, to nearest even.  fp32 outputs (every _split entry point, dw_aug) carry no rounding of this kind.
 * pcacc_rows_wgrad: dw_aug [n, k+1] f32 = dYeff^T @ [Xeff | 1] (column k is the bias gradient), fp32 MFMA;
 *   dy [rows,n], dy_mask [rows,n] or NULL (dY zeroed where dy_mask <= 0), x [rows,k], x_relu: ReLU on x at load.
 * ---------------------------------------------------------------------------------------------- */
int pcacc_rows_linear(const float *x, const float *in_mask, const float *w, const float *bias, const float *residual,
                      const float *out_mask, float *y, int64_t rows, int k, int n, int flags, void *stream);
int pcacc_rows_wgrad(const float *dy, const float *dy_mask, const float *x, int x_relu, int64_t rows, int k, int n,
                     float *dw_aug, void *stream);

/* 'mixed' mode, k <= 9 inputs (the position layer of the pillar encoder, models/pillar_encoder.py:100-108): pcacc_rows_linear on f32 rows in plain
 * fp32 arithmetic with two more outputs from the same store phase: y16 = y as bf16 [rows][n], y_amax = 256 partial absolute maxima of y
 * (zero-filled by the caller; layout of pcacc_absmax256).  n in {8,16,32,64,128}; flags as pcacc_rows_linear. */
int pcacc_rows_linear_few_dual(const float *x, const float *w, const float *bias, const float *residual, float *y, uint16_t *y16,
                               float *y_amax, int64_t rows, int k, int n, int flags, void *stream);

/* bf16 compute mode of the same layers (cfg misc.compute_dtype = bf16): rows stored as bf16, fp32 accumulation.
 *   pcacc_rows_linear_bf16: x, in_mask, residual, out_mask, y all bf16; k, n in {32, 64, 128}; w, bias f32 (rounded to
 *     bf16 once per launch); the product runs on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16).
 *   pcacc_rows_linear_mixed / pcacc_rows_wgrad_mixed: the fp32-arithmetic kernels above with per-tensor element types,
 *     for the layers at the edges of a bf16 chain (k < 32, n = 2) and for the weight gradients.
 *     rows_linear dtypes bits: 1 = x, 2 = in_mask, 4 = residual, 8 = out_mask, 16 = y are bf16 (clear = f32);
 *     rows_wgrad  dtypes bits: 1 = dy, 2 = dy_mask, 4 = x are bf16. */
int pcacc_rows_linear_bf16(const uint16_t *x, const uint16_t *in_mask, const float *w, const float *bias,
                           const uint16_t *residual, const uint16_t *out_mask, uint16_t *y, int64_t rows, int32_t k,
                           int32_t n, int32_t flags, void *stream);
int pcacc_rows_linear_mixed(const void *x, const void *in_mask, const float *w, const float *bias, const void *residual,
                            const void *out_mask, void *y, int64_t rows, int k, int n, int flags, int dtypes, void *stream);
int pcacc_rows_wgrad_mixed(const void *dy, const void *dy_mask, const void *x, int x_relu, int64_t rows, int k, int n,
                           float *dw_aug, int dtypes, void *stream);
/* all-bf16 rows (k, n multiples of 32, <= 128): the same product on the bf16 matrix cores, dw_aug f32.
 * x_relu is a flags word here, in pcacc_rows_wgrad_cat_bf16 and in pcacc_rows_wgrad_few: bit 0 = ReLU on X; bit 1 = split result layout:
 * dw_aug holds dW [n,k] followed by the bias gradients [n], each contiguous (what an optimizer wants), instead of [n,k+1] rows. */
int pcacc_rows_wgrad_bf16_workspace_bytes(int64_t rows, int32_t k, int32_t n, size_t *bytes /*host*/);
int pcacc_rows_wgrad_bf16(const uint16_t *dy, const uint16_t *dy_mask, const uint16_t *x, int32_t x_relu, int64_t rows,
                          int32_t k, int32_t n, float *dw_aug, void *workspace, size_t workspace_bytes, void *stream);
/* The two kernels above on rows made of two pieces -- models/pillar_encoder.py:116-118 feeds every PFN block
 * cat(point row, pooled row of the point's pillar): x[row] = cat(xa[row] (ka columns), xb[b_index[row]] (k - ka columns)), read
 * in place (no gather, no concatenation; b_index NULL: xb[row]).  Forward: pcacc_rows_linear_cat_bf16 with y2 = NULL.
 * Backward-data: xa = the output gradient (xb NULL), w = W^T; the [rows,n] result leaves as y [rows,na] and y2 [rows,n-na],
 * masked where the forward input cat(out_mask_a[row], out_mask_b[b_index[row]]) was <= 0 (out_mask_* NULL: no mask). */
int pcacc_rows_linear_cat_bf16(const uint16_t *xa, const uint16_t *xb, const int32_t *b_index, int32_t ka, const uint16_t *in_mask,
                               const float *w, const float *bias, const uint16_t *residual, const uint16_t *out_mask_a,
                               const uint16_t *out_mask_b, uint16_t *y, uint16_t *y2, int32_t na, int64_t rows, int32_t k,
                               int32_t n, int32_t flags, void *stream);
int pcacc_rows_wgrad_cat_bf16(const uint16_t *dy, const uint16_t *dy_mask, const uint16_t *xa, const uint16_t *xb,
                              const int32_t *b_index, int32_t ka, int32_t x_relu, int64_t rows, int32_t k, int32_t n,
                              float *dw_aug, void *workspace, size_t workspace_bytes, void *stream);

/* [r6] The encoder's last max-pooling and the pillar scatter as ONE pass -- models/pillar_encoder.py:119-122 (scatter(net, point_to_voxel_map, 'max')) followed by
 * models/pillar_encoder.py:125-174 (scatter_point_pillar): the kernel walks the canvas cells; an occupied cell (cell2pillar >= 0) reduces its pillar's point
 * rows and stores the maximum at the cell, an empty cell stores zeros.  No [m, c] pooled-row table in between.  'mixed' mode form: fp32 rows in, the fp32
 * canvas AND its bf16 shadow out; arg [m, c] i32 = winners (lowest point index attaining the maximum), as pcacc_segment_max.  Short segments only
 * (n / m <= 16; PCACC_E_ARG otherwise: pool and fill separately).  start_event / stop_event: optional hipEvents attached to the dispatch (both or neither).
 *   src [n,c] f32; seg_offsets [m+1], order [n] (pcacc_csr_build); cell2pillar [n_cells] i32; canvas32 [n_cells,c] f32; canvas16 [n_cells,c] bf16
 * Backward: grad_src[i,k] = grad_canvas[cell[p2v[i]],k] where point i won channel k of its pillar, else 0; cell [m] i32 = the pillars' cell numbers. */
int pcacc_segment_max_canvas(const float *src, int c, const int32_t *seg_offsets, const int32_t *order, int64_t n, int64_t m,
                             const int32_t *cell2pillar, int64_t n_cells, float *canvas32, uint16_t *canvas16, int32_t *arg,
                             void *start_event, void *stop_event, void *stream);
int pcacc_segment_max_canvas_backward(const void *grad_canvas, int dtype, const int32_t *arg, const int32_t *p2v, const int32_t *cell, int64_t n,
                                      int c, void *grad_src, int out_dtype, void *stream);

/* Sum of rows per index for FEW output rows (m*c <= 8192), no CSR needed: LDS-privatised accumulation.
 * The per-instance 'sum' / 'mean' poolings of models/tpointnet.py:227,251,283-284 and libs/loss.py:216 (torch_scatter: fp32 atomics in arrival order).
 * [r6] run-to-run identical: every workgroup sums its slice in 64-bit fixed point (scaled by the slice's own maximum; integer additions commute) and the
 * workgroups' fp32 partials meet in a fixed order.  A non-finite input element makes the affected partial -- and so every output element -- NaN.
 *   src [n,c] f32; idx [n] i32 in [0,m) (negative = skip); out [m,c] f32 (every element written); workspace: the per-workgroup partials */
int pcacc_scatter_sum_small_workspace_bytes(int64_t n, int c, int m, size_t *bytes /*host*/);
int pcacc_scatter_sum_small(const float *src, const int32_t *idx, int64_t n, int c, int m, float *out, void *workspace, size_t workspace_bytes,
                            void *stream);

/* ------------------------------------------------------------------------------------------------
 * A5. Pillar scatter into the BEV canvas -- models/pillar_encoder.py:125-174 (scatter_point_pillar).
 * One pass writes every canvas element exactly once (feature row or zeros), so there is no separate
 * zero-fill: canvas[cell, :] = cell2pillar[cell] >= 0 ? feats[cell2pillar[cell], :] : 0.
 *   feats [m,c] f32, c % 4 == 0 or c in {1,2,3}; canvas [n_cells, c] of `dtype` (channels-last)
 * ---------------------------------------------------------------------------------------------- */
int pcacc_pillar_scatter(const float *feats, const int32_t *cell2pillar, int64_t n_cells, int c,
                         void *canvas, int dtype, void *stream);
/* The same launch with two events attached to the dispatch (bench.py's roofline object): after the stream has been
 * synchronised, pcacc_timer_elapsed_us(start, stop) is the kernel's own begin-to-end time, as a kernel trace reports it. */
int pcacc_pillar_scatter_timed(const float *feats, const int32_t *cell2pillar, int64_t n_cells, int c, void *canvas, int dtype,
                               void *start_event, void *stop_event, void *stream);
/* Typed form: feats [m,c] of `feats_dtype` (PCACC_F32, or PCACC_BF16 with a PCACC_BF16 canvas and c % 8 == 0: the bf16 compute mode,
 * where the pillar encoder's last pooling leaves bf16 rows and the kernel moves exactly SURVEY.md 8d's bytes with s = 2:
 * c*2*n_cells written, c*2*m + 4*n_cells read).  start_event / stop_event: both NULL, or the two events of pcacc_timer_create. */
int pcacc_pillar_scatter_t(const void *feats, int feats_dtype, const int32_t *cell2pillar, int64_t n_cells, int c, void *canvas,
                           int dtype, void *start_event, void *stop_event, void *stream);
int pcacc_timer_create(void **start_event, void **stop_event);
int pcacc_timer_elapsed_us(void *start_event, void *stop_event, float *us);
int pcacc_timer_destroy(void *start_event, void *stop_event);

/* A6 and the backward of A5: row gather out[i,:] = src[idx[i],:] for rows of row_bytes bytes
 * (row_bytes % 4 == 0).  Replaces models/pillar_encoder.py:177-204 (inverse_scatter_point_pillar)
 * and the [point_to_voxel_map] gathers at models/motionnet.py:192-193. */
int pcacc_gather_rows(const void *src, int row_bytes, const int32_t *idx, int64_t n_idx, void *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * A11. Per-point bilinear feature gather ("ungrid") -- models/pillar_encoder.py:231-267 and
 * temporal_ungrid :206-228.  Direct 4-tap gather; the reference's replication of the feature map
 * into fake H x W grids is not reproduced.  grid_sample semantics: bilinear, padding 'border',
 * align_corners=False; u = x / x_scale, v = y / y_scale (fp32 division as in pillar_encoder.py:247-249).
 *   fmap [n_maps,h,w,c] `dtype` channels-last; points [k,3] f32; map_idx [k] i32; out [k,c] f32; c % 4 == 0
 * Backward accumulates into grad_fmap [n_maps,h,w,c] f32 (caller zero-fills) with fp32 atomics.
 * ---------------------------------------------------------------------------------------------- */
int pcacc_bilinear_gather(const void *fmap, int dtype, int n_maps, int h, int w, int c,
                          const float *points, const int32_t *map_idx, int64_t k,
                          float x_scale, float y_scale, float *out, void *stream);
int pcacc_bilinear_gather_backward(const float *grad_out, int n_maps, int h, int w, int c,
                                   const float *points, const int32_t *map_idx, int64_t k,
                                   float x_scale, float y_scale, float *grad_fmap, void *stream);
/* The same gradient without atomics (index-ordered sums): pcacc_bilinear_base_cells writes, per point, the cell of its
 * upper-left tap (n_maps*h*w for points of no map); after pcacc_csr_build over those keys (m = n_maps*h*w + 1),
 * pcacc_bilinear_gather_backward_sorted sums, per map cell, the contributions of the four neighbouring base cells in
 * index order (two launches: tap weights and gradient rows laid out in CSR order, then the per-cell sums over consecutive
 * rows; workspace = those two tables).  grad_out [k,c] and grad_fmap [n_maps,h,w,c] may each be f32 or bf16. */
int pcacc_bilinear_base_cells(const float *points, const int32_t *map_idx, int64_t k, int n_maps, int h, int w,
                              float x_scale, float y_scale, int32_t *cell, void *stream);
int pcacc_bilinear_sorted_workspace_bytes(int64_t k, int c, int grad_dtype, size_t *bytes /*host*/);
int pcacc_bilinear_gather_backward_sorted(const void *grad_out, int grad_dtype, int n_maps, int h, int w, int c,
                                          const float *points, const int32_t *seg_offsets, const int32_t *order, int64_t k,
                                          float x_scale, float y_scale, void *grad_fmap, int out_dtype, void *workspace,
                                          size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * A9. Ego-motion BEV warp -- models/motionnet.py:45-80 (get_transformed_grid) + :82-114 (warp_feats).
 *   bev    [n_batch, nt, h, w, c] `dtype`; out same shape/dtype
 *   inv_pose [n_batch, nt, 16] f32 row-major 4x4 = inverse of the estimated pose of frame t
 * Frames 1..nt-1 are resampled bilinearly (zeros padding, align_corners=False) on the grid
 * inv_pose[:2,:2] @ (pixel centre in metres) + inv_pose[:2,3], divided by |x_min|, |y_min|.
 * Slot 0 receives frame nt-1 UNWARPED: bug-compatible with the leaked loop variable at
 * models/motionnet.py:100,111 (trap 1).
 * ---------------------------------------------------------------------------------------------- */
int pcacc_bev_warp(const void *bev, int dtype, int n_batch, int nt, int h, int w, int c,
                   const float *inv_pose, float x_reso, float y_reso, float x_min, float y_min,
                   void *out, void *stream);
/* [r6] 'mixed' mode form: fp32 map in, the fp32 result AND its bf16 copy (same element offsets) out of one pass. */
int pcacc_bev_warp_dual(const float *bev, int n_batch, int nt, int h, int w, int c, const float *inv_pose, float x_reso, float y_reso, float x_min,
                        float y_min, float *out, uint16_t *out16, void *stream);

/* A10. Per-point rigid transform -- models/motionnet.py:117-135 (transform_points).
 *   points [n,3] f32; frame_idx [n] i32 = b*nt + t; tsfm [n_frames,16] f32; out [n,3] f32 */
int pcacc_rigid_transform(const float *points, const int32_t *frame_idx, const float *tsfm, int64_t n,
                          float *out, void *stream);

/* Key-point draws of the ego-motion head -- models/egomotion.py:156-166 (torch.randperm(n)[:k], or arange clamped to n-1
 * when n <= k).  counts [n_draws] i32 (device): population of every draw; out [n_draws, k] i64: k distinct indices per
 * draw (keyed Feistel permutation of [0, n) evaluated at 0..k-1), all draws in one launch.  This is the 'device' sampler
 * (cfg pose_estimation.kpt_sampler); the default sampler reproduces the reference's host RNG stream instead. */
int pcacc_sample_subsets(const int32_t *counts, int32_t n_draws, int32_t k, uint64_t seed, int64_t *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * A8. Key-point matching of the ego-motion head, forward pass, fp32, for n_pairs (frame, anchor) pairs at once --
 * models/egomotion.py:169-192 after the key-point choice: square_distance (toolbox/utils.py:125-144), affinity,
 * sinkhorn with slack row/column (egomotion.py:100-137), exp * support, soft targets, weighted Kabsch with a 3x3 SVD
 * and reflection fix (toolbox/register_utils.py:247-317).
 *   feats_s, feats_t [n_pairs,k,c] f32 (L2-normalised rows); coor_s, coor_t [n_pairs,k,3] f32;
 *   thr2 [n_pairs] f32 = (duration * max_speed)^2;  params [2] f32 (device) = {softplus(alpha), exp(beta) + 0.02}
 *   perm [n_pairs,k,k] f32 out;  pose [n_pairs,16] f32 out (row-major 4x4)
 * Used when no gradient is needed (eval / val / test); training keeps the batched torch formulation for autograd.
 * ---------------------------------------------------------------------------------------------- */
/* Sinkhorn normalisation as a differentiable op (training) -- models/egomotion.py:100-137 with add_slack: the [P,k,k]
 * log-affinity is padded with a zero slack row / column, n_iters x (row, column) log-sum-exp normalisations that leave the
 * slack row / column themselves un-normalised, result = the un-padded block.  forward records the subtracted
 * log-sum-exps (lse_rows, lse_cols [n_iters][P][k], may be NULL when n_iters = 0); backward replays the half-steps in reverse from log_alpha and those
 * vectors.  workspace: one padded [P,k+1,k+1] f32 matrix (pcacc_sinkhorn_train_workspace_bytes). */
int pcacc_sinkhorn_train_workspace_bytes(int n_pairs, int k, size_t *bytes /*host*/);
int pcacc_sinkhorn_forward(const float *log_alpha, int n_pairs, int k, int n_iters, float *log_perm, float *lse_rows,
                           float *lse_cols, void *workspace, size_t workspace_bytes, void *stream);
int pcacc_sinkhorn_backward(const float *grad_log_perm, const float *log_alpha, const float *lse_rows, const float *lse_cols,
                            int n_pairs, int k, int n_iters, float *grad_log_alpha, void *workspace, size_t workspace_bytes,
                            void *stream);
/* The matching stage around the Sinkhorn iterations in the TRAINING path (models/egomotion.py:169-184 under autograd), P pairs at once:
 *  ego_affinity_forward   affinity [P,k,k] = -(max(2 - 2 <fs_i, ft_j>, 1e-12) - params[0]) / params[1]; feats [P,k,c] f32 (L2-normalised rows),
 *                         params [2] f32 on the device = (softplus(alpha), exp(beta) + 0.02)
 *  ego_affinity_backward  grad_dot [P,k,k] = d loss / d <fs_i, ft_j> (feature gradients: grad_dot @ ft, grad_dot^T @ fs), grad_params [2]
 *  ego_perm_forward       perm = exp(log_perm) * [ |cs_i - ct_j|^2 < thr2[p] ], rowsum [P,k], weighted_t [P,k,3] = perm @ ct / (rowsum + 1e-20),
 *                         colsum [P,k] (NULL = not wanted): with rowsum all the outlier loss (libs/outlier_loss.py) reads of perm
 *  ego_perm_backward      grad_log_perm from the gradients of perm / rowsum / weighted_t / colsum (any of them NULL = 0) */
int pcacc_ego_affinity_forward(const float *feats_s, const float *feats_t, const float *params, int n_pairs, int k, int c, float *affinity,
                               void *stream);
int pcacc_ego_affinity_backward_workspace_bytes(size_t *bytes /*host*/);
int pcacc_ego_affinity_backward(const float *grad_affinity, const float *affinity, const float *params, int64_t n, float *grad_dot,
                                float *grad_params, void *workspace, size_t workspace_bytes, void *stream);
int pcacc_ego_perm_forward(const float *log_perm, const float *coor_s, const float *coor_t, const float *thr2, int n_pairs, int k, float *perm,
                           float *rowsum, float *weighted_t, float *colsum, void *stream);
int pcacc_ego_perm_backward(const float *grad_perm, const float *grad_rowsum, const float *grad_weighted_t, const float *grad_colsum,
                            const float *perm, const float *coor_t, const float *rowsum, const float *weighted_t, int n_pairs, int k,
                            float *grad_log_perm, void *stream);
/* Weighted Kabsch in front of its 3x3 SVD, under autograd (toolbox/register_utils.py:263-291), P pairs at once: weights w [P,k] normalised by
 * (sum w + 1e-7), weighted means m1, m2 [P,3] of x1, x2 [P,k,3] (divided by sum wn + 1e-7), covariance cov [P,3,3] of the centred clouds;
 * norm [P,2] = the two normalisers, kept for the backward.  backward: grad_x2, grad_w (x1 -- pillar means -- carries no gradient). */
int pcacc_kabsch_cov_forward(const float *x1, const float *x2, const float *w, int n_pairs, int k, float *cov, float *m1, float *m2, float *norm,
                             void *stream);
int pcacc_kabsch_cov_backward(const float *x1, const float *x2, const float *w, const float *m1, const float *m2, const float *norm,
                              const float *grad_cov, const float *grad_m1, const float *grad_m2, int n_pairs, int k, float *grad_x2,
                              float *grad_w, void *stream);
/* ... and behind the SVD (toolbox/register_utils.py:305-313): rot [n,3,3] = V diag(1, 1, det(V U^T)) U^T, trans [n,3] = m2 - rot m1, from the
 * singular vectors u, v [n,3,3] and the weighted means m1, m2 [n,3]; backward from grad_rot / grad_trans (NULL = 0) incl. the path through
 * the determinant (its derivative is the cofactor matrix: no LU factorisation of a 3x3 matrix). */
int pcacc_kabsch_rt_forward(const float *u, const float *v, const float *m1, const float *m2, int n, float *rot, float *trans, void *stream);
int pcacc_kabsch_rt_backward(const float *u, const float *v, const float *m1, const float *grad_rot, const float *grad_trans, int n,
                             float *grad_u, float *grad_v, float *grad_m1, float *grad_m2, void *stream);
/* Batched 3x3 SVD of the Kabsch solve in the training path -- toolbox/register_utils.py:293 (`torch.svd(cov_mat)`):
 * a [n,3,3] f32 = u diag(s) v^T, s descending, no status word read back on the host.  backward: grad_a from the gradients of
 * u, s, v (any of them NULL = 0), closed form for distinct singular values. */
int pcacc_svd3(const float *a, int64_t n, float *u, float *s, float *v, void *stream);
int pcacc_svd3_backward(const float *u, const float *s, const float *v, const float *grad_u, const float *grad_s,
                        const float *grad_v, int64_t n, float *grad_a, void *stream);
int pcacc_sinkhorn_kabsch_workspace_bytes(int n_pairs, int k, size_t *bytes /*host*/);
int pcacc_sinkhorn_kabsch(const float *feats_s, const float *feats_t, const float *coor_s, const float *coor_t,
                          const float *thr2, const float *params, int n_pairs, int k, int c, int n_iters,
                          float *perm, float *pose, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * A12. Chamfer nearest neighbour -- chamfer_distance/chamfer_distance.cu:6-155 (forward kernel and
 * launcher), chamfer_distance.cpp:59-111 (CPU twin), called through
 * chamfer_distance/chamfer_distance.py:9-31.  dist = squared fp32 distance (x*x + y*y) + z*z of
 * (target - query), idx = LOWEST target index attaining it (chamfer_distance.cu:39,49,129).
 *   xyz1 [b,n,3], xyz2 [b,m,3] f32; dist1 [b,n], dist2 [b,m] f32; idx1 [b,n], idx2 [b,m] i32
 * Backward -- chamfer_distance.cu:158-209 / chamfer_distance.cpp:114-177; grad_xyz* are zero-filled
 * by the call.
 * ---------------------------------------------------------------------------------------------- */
int pcacc_chamfer_workspace_bytes(int b, int n, int m, size_t *bytes /*host*/);
int pcacc_chamfer_forward(const float *xyz1, const float *xyz2, int b, int n, int m,
                          float *dist1, int32_t *idx1, float *dist2, int32_t *idx2,
                          void *workspace, size_t workspace_bytes, void *stream);
int pcacc_chamfer_backward(const float *xyz1, const float *xyz2, int b, int n, int m,
                           const float *grad_dist1, const int32_t *idx1, const float *grad_dist2, const int32_t *idx2,
                           float *grad_xyz1, float *grad_xyz2, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C1. Test-mode instance clustering -- models/cluster.py:86-111 (Cluster.forward with fb_labels=None),
 * :52-84 (cluster_per_batch), :23-49 (cluster), :9-13 (voxel_downsample); called from
 * models/motionnet.py:238.  Replaces the host round trip through torchsparse v1.4.0 sparse_quantize
 * (README.md:27) and sklearn.cluster.DBSCAN(metric='euclidean') with one set of launches for the whole
 * batch; same labels, bit for bit (DESIGN.md section 9 has the argument).
 *   points [n,3] f32   ego-motion-compensated points (results['transformed_points'])
 *   offset [n,2] f32   predicted centre offsets, added to x,y before clustering (use_offset=True), or NULL
 *   sel    [n]   u8    1 = predicted moving (mos.argmax(1) == 1)
 *   batch  [n]   i32   sample index of every point, 0 <= batch < n_batches <= 64
 *   voxel_size         0.05 with offsets, 0.15 without (cluster.py:76,80)
 *   eps, min_samples   DBSCAN parameters (cfg.cluster.eps_dbscan, min_samples_dbscan); z is ignored
 *   min_p_cluster      clusters with fewer down-sampled points are dropped, and a sample with
 *                      <= min_p_cluster selected points is not clustered at all (cluster.py:38-41,66)
 *   labels [n]   i64   0 = no instance, 1..K per sample in canonical order (toolbox/utils.py:237-250)
 * Voxel indices are packed in 19 bits per axis: |coordinate / voxel_size| must stay below 2^18.
 * ---------------------------------------------------------------------------------------------- */
int pcacc_cluster_workspace_bytes(int64_t n, size_t *bytes /*host*/);
int pcacc_cluster(const float *points, const float *offset, const uint8_t *sel, const int32_t *batch, int64_t n,
                  int32_t n_batches, float voxel_size, double eps, int32_t min_samples, int32_t min_p_cluster,
                  int64_t *labels, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C2. Instance-segmentation evaluation of the test loop -- toolbox/cluster_eval.py:71-152 (ClusterEvaluation.forward:
 * instances and their classes :79-95, coverage :98-124, precision / recall :127-152) for every sample of a batch in one
 * call, as libs/loss.py:261-270 (evaluate_cluster) runs it sample by sample from libs/tester.py:93.  Replaces the double
 * loop over (estimated, ground-truth) instance pairs -- two masks of length n and two host syncs per pair -- with one pass
 * over the points and one over the non-empty pairs.  Integer atomics only: deterministic, and every number is the
 * reference's, bit for bit.
 *   inst_est, inst_gt [n] i64   instance ids, any value; 0 = background; compared per sample only
 *   mos [n]                     ground-truth moving label, zero / non-zero, of type mos_dtype (PCACC_MOS_*):
 *                               input_dict['sd_labels'][:, 0] as it is (i64), its .float(), or a bool tensor
 *   batch [n] i32               sample of every point, 0 <= batch < n_batches
 *   inst_capacity               rows per table (all samples together); pair_capacity: non-empty (est, gt) pairs
 *   out                         16 i32 header words, then inst_capacity rows of estimated and inst_capacity rows of
 *                               ground-truth instances; out_bytes >= 64 + 2 * inst_capacity * 32
 *     header  [0] status: 0, or a sum of 1 = more instances than inst_capacity, 2 = more pairs than pair_capacity (call
 *             again with more: nothing is truncated silently), 4 = a sample has more than 2^24 points (the class of an
 *             instance is round() of an fp32 mean of 0/1 values, cluster_eval.py:85,94; below 2^24 points that is the
 *             integer rule used here, above it the reference's own sum is no longer exact), 8 = a batch index out of range;
 *             [1] estimated rows, [2] ground-truth rows, [3] non-empty pairs.  With status != 0 the rows are void.
 *     row     { i64 id; u32 count; u32 moving; i32 sample; i32 class; f32 best_iou; i32 pad } in order of first sight --
 *             the reference visits them by ascending id inside a sample (torch.unique), the host sorts.
 *             class = 1 iff 2 * moving > count (Python's round(): a tie goes to 0).  best_iou = max over the instances
 *             of the other table, same sample and class, of fp32(inter) / fp32(count_est + count_gt - inter), one IEEE
 *             division as torch divides two int64 sums; 0.0 when none overlaps; -1.0 for an ESTIMATED instance whose
 *             class has no ground-truth instance in its sample (cluster_eval.py:135).
 * A status that only the device knows cannot be the return value (no synchronisation here): the return value covers the
 * arguments, including n > n_batches * 2^24, where some sample is too large whatever `batch` holds.
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_MOS_I64 0
#define PCACC_MOS_F32 1
#define PCACC_MOS_U8 2
int pcacc_cluster_eval_workspace_bytes(int64_t n, int32_t n_batches, int32_t inst_capacity, int32_t pair_capacity, size_t *bytes /*host*/);
int pcacc_cluster_eval(const int64_t *inst_est, const int64_t *inst_gt, const void *mos, int32_t mos_dtype, const int32_t *batch, int64_t n,
                       int32_t n_batches, int32_t inst_capacity, int32_t pair_capacity, void *out, size_t out_bytes,
                       void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C3. Point-to-point ICP pose refinement, J independent jobs in one call -- models/egomotion.py:9-28 (refine_pose_with_icp),
 * :360-384 (pose_refinement: every frame t >= 1 of a sample onto its anchor frame, model.ego_icp) and models/alignnet.py:54-112
 * (run_icp / refine_pose_by_icp: every frame of an instance onto the instance's frame 0, model.tpointnet_icp).  Replaces one
 * Open3D registration_icp(source, target, threshold, eye(4), TransformationEstimationPointToPoint(),
 * ICPConvergenceCriteria(max_iteration)) call on the host per frame and per instance.
 *   points [n,3] f32          all points; a segment s is the rows seg_offsets[s] .. seg_offsets[s+1]
 *   seg_offsets [n_seg+1] i32 ascending, 0 <= offset <= n; n_seg <= 65535
 *   jobs [n_jobs,2] i32       { source segment, target segment }; jobs may share a target (its index is built once per call)
 *   init [n_jobs,4,4] f64     initial pose, applied to the source first (rows 0-2 are read, row 3 is taken as 0 0 0 1); NULL = identity
 *   threshold                 maximum correspondence distance (> 0); also the edge of the grid cells
 *   out_T [n_jobs,4,4] f64    T @ init, T the transformation registration_icp would return for the pre-transformed source: the
 *                             refined pose both call sites form (`tsfm @ initial_pose`, egomotion.py:25)
 *   out_fitness, out_rmse [n_jobs] f64   correspondences / source points, sqrt(sum d^2 / correspondences) (0 without any) of the last evaluation
 *   out_iters [n_jobs] i32    updates applied (1 .. max_iter; 0 when max_iter = 0)
 *   out_status [n_jobs] i32   a sum of PCACC_ICP_* below
 * Algorithm (all float64, fp32 inputs promoted): correspondence of a source point = its nearest target point if within the
 * threshold (equal distances: the LOWEST target index); then at most max_iter rounds of { update = least-squares rigid
 * transform of the correspondences (Umeyama without scale: centroids, 3x3 covariance, the SVD of csrc/svd3.h, reflection fix), identity without
 * correspondences; T = update @ T; correspondences again; stop when |d fitness| < 1e-6 and |d rmse| < 1e-6 }.  The source is
 * transformed by the composed pose each round (Open3D transforms it round by round: the same up to float64 rounding).
 * Deterministic: no floating-point atomics, fixed-order sums; two calls give the same bits.  Convergence is decided per job on
 * the device; the call never synchronises.
 * Supported range: a point takes part only if its coordinates are finite and |coordinate| / threshold < 32767 (cells of edge
 * `threshold`, 16 bits per axis); any other point -- as source after the current pose, or as target -- has no correspondence
 * (it is never clamped into an edge cell and forms no address), and still counts in the denominator of the fitness.
 * Empty source, empty target, no correspondence: identity update, fitness 0, rmse 0.  Fewer than three non-collinear
 * correspondences (rank-deficient covariance) are outside the parity claim: csrc/svd3.h completes the missing singular vectors
 * to a right-handed orthonormal basis (u0 x e_m for the axis m on which u0 is smallest, then u0 x u1), a zero covariance gives the
 * identity rotation -- always a finite proper rotation, the same every run.  A singular value at or below 1e-10 * mean(t . q)
 * (the rounding noise of the uncentred float64 sums the covariance is formed from) counts as zero (jacobi_svd3_floor).
 * The whole round is header code (csrc/icp_round.h) that a g++ build compiles as well: the kernels give that build's bits.
 * Tables that cannot be trusted (offsets not ascending or outside [0, n], a job naming a segment outside [0, n_seg)) address
 * nothing: every job returns identity with PCACC_ICP_BAD_TABLE.
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_ICP_EMPTY_SOURCE 1
#define PCACC_ICP_EMPTY_TARGET 2
#define PCACC_ICP_NO_CORRESPONDENCE 4   /* the last evaluation found none */
#define PCACC_ICP_RANK_DEFICIENT 8      /* some update completed a singular vector */
#define PCACC_ICP_BAD_TABLE 16
int pcacc_icp_point_to_point_workspace_bytes(int64_t n, int32_t n_seg, int32_t n_jobs, size_t *bytes /*host*/);
int pcacc_icp_point_to_point(const float *points, int64_t n, const int32_t *seg_offsets, int32_t n_seg, const int32_t *jobs,
                             int32_t n_jobs, const double *init, double threshold, int32_t max_iter, double *out_T,
                             double *out_fitness, double *out_rmse, int32_t *out_iters, int32_t *out_status,
                             void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C4. Accumulated scene cloud: a persistent voxel map that takes the points of one window per call and hands back one centroid per
 * occupied voxel.  The reference has no such function (it shows per-window clouds with Open3D); this replaces the copy of every
 * window's results['rec_est'] to the host and np.unique / Open3D voxel_down_sample there.
 * Inputs of one add
 *   points [n,3] f32          the window's points, 1 <= n <= 2^30
 *   pose [4,4] f64            window-to-world, rows 0-2 are read; NULL = identity
 *   moving [n] u8             predicted-moving flag (non-zero = moving); NULL = all 0
 *   stamp                     one time stamp for the whole call
 *   voxel_size                > 0, finite, the same for every call on a map
 * Per point, all float64 with no FMA contraction, in this order and no other:
 *   w_a = ((r_a0 * x + r_a1 * y) + r_a2 * z) + t_a;  i_a = floor(w_a / voxel_size) (one IEEE division);
 *   q_a = llrint(w_a * 65536) (round to nearest even).
 * A point is valid iff every w_a is finite, |w_a| < 32768 and -2^20 <= i_a < 2^20.  An invalid point is counted (`dropped`) and
 * contributes nothing: it is never clamped and forms no address.
 * Key of a voxel: (i_x + 2^20) << 42 | (i_y + 2^20) << 21 | (i_z + 2^20); ascending keys = lexicographic (x, y, z).
 * The map: `capacity` rows, of which the first state[PCACC_ACCUM_NUM_VOXELS] are in use, ascending and duplicate-free in `keys`:
 *   keys   [capacity] i64
 *   acc    [5][capacity] i64      field-major: count, moving, sum q_x, sum q_y, sum q_z
 *   stamps [2][capacity] i32      smallest and largest stamp of the calls that touched the voxel
 *   state  [PCACC_ACCUM_STATE_WORDS] i64 device words, all 0 for an empty map (indices below)
 * Everything is an integer and integer additions commute: the map depends on the SET of (point, flag, stamp) triples it was given,
 * not on the order of points inside a call, of the calls, or on the run.
 * pcacc_accum_add merges OUT OF PLACE: it reads in_* (in_capacity rows; may be NULL when in_capacity = 0) and writes the merged map
 * to out_* (out_capacity rows, distinct buffers).  If the merged map has more than out_capacity voxels NOTHING is written to out_*,
 * state[STATUS] = PCACC_ACCUM_TOO_SMALL and state[NEEDED] = the rows it takes; NUM_VOXELS and DROPPED stay, in_* are intact, and the
 * caller repeats the call with larger out_* tables.  Otherwise state[STATUS] = 0, state[NUM_VOXELS] = rows of out_*, state[DROPPED]
 * grows by this call's invalid points.  A state[NUM_VOXELS] outside [0, in_capacity] addresses nothing: PCACC_ACCUM_BAD_STATE.
 * The status lives in a device word because only the device knows it (no synchronisation here); the return value covers the arguments.
 * pcacc_accum_extract: the first m rows of a map, in key order, of which a row is kept iff count >= min_count and, when
 * use_fraction != 0, float64(moving) / float64(count) <= max_moving_fraction.  Every output has room for m rows; *out_n = rows kept.
 *   out_points [m,3] f32      float32((float64(sum q_a) / float64(count)) * 2^-16)
 *   out_coords [m,3] i32      voxel indices (i_x, i_y, i_z)
 *   out_count, out_moving [m] i64;  out_t_first, out_t_last [m] i32
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_ACCUM_STATE_WORDS 8
#define PCACC_ACCUM_NUM_VOXELS 0       /* rows in use */
#define PCACC_ACCUM_DROPPED 1          /* invalid points of all successful calls */
#define PCACC_ACCUM_STATUS 2           /* of the last add: 0 or one of the two below */
#define PCACC_ACCUM_NEEDED 3           /* rows the last add's merged map takes */
#define PCACC_ACCUM_WINDOW_VOXELS 4    /* distinct voxels of the last add's points */
#define PCACC_ACCUM_WINDOW_DROPPED 5   /* invalid points of the last add */
#define PCACC_ACCUM_OK 0
#define PCACC_ACCUM_TOO_SMALL 1
#define PCACC_ACCUM_BAD_STATE 2
int pcacc_accum_add_workspace_bytes(int64_t n, size_t *bytes /*host*/);
int pcacc_accum_add(const float *points, int64_t n, const double *pose, const uint8_t *moving, int32_t stamp, double voxel_size,
                    const int64_t *in_keys, const int64_t *in_acc, const int32_t *in_stamps, int64_t in_capacity,
                    int64_t *out_keys, int64_t *out_acc, int32_t *out_stamps, int64_t out_capacity,
                    int64_t *state, void *workspace, size_t workspace_bytes, void *stream);
int pcacc_accum_extract_workspace_bytes(int64_t m, size_t *bytes /*host*/);
int pcacc_accum_extract(const int64_t *keys, const int64_t *acc, const int32_t *stamps, int64_t capacity, int64_t m, int64_t min_count,
                        int32_t use_fraction, double max_moving_fraction, float *out_points, int32_t *out_coords, int64_t *out_count,
                        int64_t *out_moving, int32_t *out_t_first, int32_t *out_t_last, int64_t *out_n,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C5. Per-voxel surface normals of the accumulated scene cloud: the covariance of the centroids around every kept voxel, its 3x3
 * decomposition and an oriented normal.  Replaces the copy of up to 8 M centroids to the host and a KD-tree PCA there.  Adds no lookup,
 * no nearest-neighbour query and no registration.
 * Inputs
 *   keys, acc, stamps, capacity, m                    the first m rows of a map, as for pcacc_accum_extract
 *   min_count, use_fraction, max_moving_fraction      extract's filter
 *   radius                    r in {1, 2, 3}, in voxels
 *   min_neighbors             >= 3
 *   viewpoints [S,3] f64      sensor position per stamp, or NULL with n_viewpoints = 0;  stamp_base: the stamp of its row 0
 * Participating set: a row participates iff extract keeps it (count >= min_count, count > 0 and, when use_fraction != 0,
 * float64(moving) / float64(count) <= max_moving_fraction).  Rows that do not participate are neither output rows nor neighbours.
 * Output rows: the participating rows in key order -- row j of every output is row j of pcacc_accum_extract under the same filter.
 * Every output has room for m rows; *out_n = rows written.
 * Centroid of a row: c_a = (float64(sum q_a) / float64(count)) * 2^-16, the float64 value (not its float32 rounding).
 * Neighbourhood of voxel i = (x, y, z): every participating voxel with |delta|_inf <= r, itself included, visited in ASCENDING KEY
 * ORDER (dx = -r..r, inside it dy = -r..r, inside it z ascending).  An offset whose index leaves [-2^20, 2^20) on any axis is skipped
 * BEFORE a key is formed: nothing out of range is clamped or turned into an address (a key whose y or z field overflowed would
 * alias another voxel).  k = voxels visited (>= 1).
 * Arithmetic, all float64 with no FMA contraction, in this order and no other (every sum starts at 0.0, terms in visiting order):
 *   d = c_j - c_i;  S1_a += d_a (a = x, y, z);  S2_xx += d_x d_x, S2_xy += d_x d_y, S2_xz += d_x d_z, S2_yy += d_y d_y,
 *   S2_yz += d_y d_z, S2_zz += d_z d_z;  then mu_a = S1_a / k;  C_ab = S2_ab / k - mu_a * mu_b (a <= b, mirrored);
 *   jacobi_svd3(C) of csrc/svd3.h -> s descending and u;  normal = u[:,2].
 *   out_eigenvalues [m,3] f32 = s;   out_neighbors [m] i32 = k;   out_flags [m] u8;   out_normals [m,3] f32
 * Flags: PCACC_NORMAL_FEW_NEIGHBORS when k < min_neighbors; PCACC_NORMAL_DEGENERATE when s[1] <= 64 * 2^-52 * s[0] (SVD3_RANK_TOL:
 * collinear, or a single point).  A row with either gets the normal (0, 0, 0) and no sign rule; eigenvalues and k are written for
 * every row.
 * Sign of a valid normal n: t = t_first - stamp_base.  With viewpoints and 0 <= t < S: e = viewpoint_t - c_i, n is negated iff
 * (n_x e_x + n_y e_y) + n_z e_z < 0, and PCACC_NORMAL_VIEWPOINT is set (the normal was oriented by a viewpoint).  Otherwise n is
 * negated iff the first non-zero of (n_z, n_y, n_x) is negative (-0.0 counts as zero).  Negation is 0.0 - n_a.
 * A result depends on the set of integer records alone, visited in key order: two runs give the same bits, and so do two maps built
 * from the same points in any order.  No floating-point atomics.
 * Return value: PCACC_E_ARG for radius outside 1..3, min_neighbors < 3, m outside [0, capacity], n_viewpoints < 0 or a NULL table
 * with n_viewpoints > 0; nothing is launched then.
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_NORMAL_FEW_NEIGHBORS 1
#define PCACC_NORMAL_DEGENERATE 2
#define PCACC_NORMAL_VIEWPOINT 4
int pcacc_accum_normals_workspace_bytes(int64_t m, size_t *bytes /*host*/);
int pcacc_accum_normals(const int64_t *keys, const int64_t *acc, const int32_t *stamps, int64_t capacity, int64_t m, int64_t min_count,
                        int32_t use_fraction, double max_moving_fraction, int32_t radius, int32_t min_neighbors, const double *viewpoints,
                        int64_t n_viewpoints, int64_t stamp_base, float *out_normals, float *out_eigenvalues, int32_t *out_neighbors,
                        uint8_t *out_flags, int64_t *out_n, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C6. Scan-to-map registration against the accumulated scene cloud: point-to-plane ICP of one scan onto the kept voxels of a map, with the
 * normals of C5.  It returns the scan-to-world pose to hand to pcacc_accum_add.  Replaces the copy of the scan and of up to 8 M centroids to
 * the host and a KD-tree ICP there.  Adds no lookup and no nearest-neighbour query, and does not modify the map.
 * Inputs
 *   points [n,3] f32, 0 <= n <= 2^24;  moving [n] u8 or NULL (non-zero = predicted moving: the point takes part in nothing)
 *   init_pose [4,4] f64       rows 0-2 are read, row 3 is taken as 0 0 0 1; NULL = identity
 *   voxel_size                of the map;  max_distance in (0, voxel_size];  max_iter in [0, 10000]
 *   keys, acc, capacity, m; min_count, use_fraction, max_moving_fraction     the map and extract's filter, as for pcacc_accum_normals
 *   normals [n_rows,3] f32, flags [n_rows] u8     out_normals / out_flags of pcacc_accum_normals on this map under this filter;
 *                             n_rows = the rows it wrote (its *out_n), which the caller knows
 * Per point, all float64 with no FMA contraction, in the order csrc/accum_register.h writes down and no other:
 *   w = pose . p with C4's transform; valid iff C4's rule holds (every w_a finite, |w_a| < 32768, floor(w_a / voxel_size) in [-2^20, 2^20)).
 *   An invalid point has no correspondence: it is never clamped and forms no key.  It still counts in the fitness denominator.
 *   Candidates: every map row the filter keeps whose normal has neither PCACC_NORMAL_FEW_NEIGHBORS nor PCACC_NORMAL_DEGENERATE, in the
 *   3 x 3 x 3 voxels around the point's voxel, visited in ascending key order; offsets that leave [-2^20, 2^20) are skipped before a key
 *   is formed.  Correspondence: the candidate with the smallest d2 = |w - c_j|^2 (c_j the float64 centroid of C5; strict <: ties go to the
 *   lowest key), accepted iff d2 <= max_distance^2.  The contract IS this 27-voxel search; nothing is claimed about a global nearest
 *   neighbour.  With n_j the float32 normal widened to double: r = n . (w - c), J = (w x n, n); the 21 upper entries of J J^T, the 6 of
 *   J r, r^2 and 1 are summed over the scan in a fixed order (slots of 256 consecutive points: a tree at strides 32..1 inside each group
 *   of 64, the 4 group sums left to right, the slots in ascending order) -- no floating-point atomics.
 * Per round: A = sum J J^T scaled to unit diagonal, Cholesky in float64; a diagonal entry that is not > 0 or a pivot <= 1e-10 (a plane,
 * an edge, too few points leave a direction unconstrained) sets PCACC_REGISTER_DEGENERATE and ends the job with the pose so far;
 * otherwise A x = -b for x = (omega, t), R_d = the rotation of the unit quaternion (1, omega / 2) / |.|, pose <- [R_d | t] pose.
 * fitness = correspondences / eligible points (eligible = not flagged moving), rmse = sqrt(sum r^2 / correspondences).  Stop when
 * |d fitness| < 1e-6 and |d rmse| < 1e-6 against the previous round, or after max_iter updates (PCACC_REGISTER_MAX_ITER).  The stop is
 * decided on the device: 2 (max_iter + 1) launches are queued and the call never synchronises.
 * Outputs (device): out_pose [4,4] f64 scan-to-world; out_fitness, out_rmse f64; out_iterations (updates applied), out_status (a sum of
 * the bits below), out_correspondences (of the last evaluation) i32.  Every status bit except PCACC_REGISTER_MAX_ITER leaves fitness and
 * rmse at 0 and the pose at the last good value: the pose so far for DEGENERATE, the pose of the last evaluation that had
 * correspondences otherwise -- init_pose when nothing ever matched.
 * normals / flags that do not have the rows the filter keeps (n_rows differs from the kept count): PCACC_REGISTER_BAD_TABLE, init_pose,
 * no round runs.  Every table index is range-checked against m, n_rows and capacity: a table that does not fit addresses nothing.
 * Return value: PCACC_E_ARG for n outside [0, 2^24], m outside [0, capacity], n_rows outside [0, m], max_distance outside
 * (0, voxel_size], max_iter outside [0, 10000] or a NULL table of non-zero size; nothing is launched then.
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_REGISTER_NO_ELIGIBLE 1        /* every point is flagged moving, or n = 0 */
#define PCACC_REGISTER_NO_CANDIDATE 2       /* no kept map row has a valid normal */
#define PCACC_REGISTER_NO_CORRESPONDENCE 4
#define PCACC_REGISTER_DEGENERATE 8
#define PCACC_REGISTER_MAX_ITER 16
#define PCACC_REGISTER_BAD_TABLE 32
int pcacc_accum_register_workspace_bytes(int64_t n, int64_t m, size_t *bytes /*host*/);
int pcacc_accum_register(const float *points, int64_t n, const uint8_t *moving, const double *init_pose, double voxel_size,
                         double max_distance, int32_t max_iter, const int64_t *keys, const int64_t *acc, int64_t capacity, int64_t m,
                         int64_t min_count, int32_t use_fraction, double max_moving_fraction, const float *normals, const uint8_t *flags,
                         int64_t n_rows, double *out_pose, double *out_fitness, double *out_rmse, int32_t *out_iterations,
                         int32_t *out_status, int32_t *out_correspondences, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C7. Rays through the accumulated scene cloud: for every voxel of a map, the number of measured laser rays that pass straight through it -- the
 * geometric (visibility) signal beside the network's per-point moving flag: a voxel that was occupied and that later rays pierce was not static.
 * Replaces the copy of every scan and of up to 8 M keys to the host and a ray cast there.  Removes no row, keeps no free-space map and
 * does not modify the map's records.
 * Inputs
 *   points [n,3] f32, 0 <= n <= 2^30          the scan's points (scan frame);  moving [n] u8 or NULL (non-zero = predicted moving)
 *   origins [S,3] f64, S >= 1                 sensor positions (scan frame);  origin_index [n] i32 or NULL (= all 0): the row of a point's origin
 *   pose [4,4] f64                            scan-to-world, rows 0-2 are read; NULL = identity
 *   voxel_size                                of the map;  margin >= 0, finite;  max_range: < 0 = none;  use_stamp, stamp;  max_steps in [1, 2^16]
 *   keys, stamps, capacity, m                 the first m rows of a map, as for pcacc_accum_extract
 * Per ray, all float64 with no FMA contraction, only + - * / and sqrt, in the order csrc/accum_pierce.h writes down and no other:
 *   End points: e = pose . p, o = pose . origin with C4's transform ((r0 x + r1 y) + r2 z) + t.  The ray is DROPPED when origin_index lies
 *   outside [0, S) or a coordinate w of o or e is not finite, has |w| >= 32768 or floor(w / voxel_size) outside [-2^20, 2^20): it is never
 *   clamped and forms no key and no address.
 *   Eligibility (after the drop rule): a point flagged moving is SKIPPED (the network has moved it: its ray is no measured ray).
 *   d = e - o, L = sqrt((d_x^2 + d_y^2) + d_z^2), t_end = 1 - margin / L, with a max_range t_end = min(t_end, max_range / L);
 *   !(L > 0) or !(t_end > 0): SKIPPED.  The margin keeps a ray away from the surface it measured.  Every other ray is WALKED.
 *   Walk: i_a = floor(o_a / voxel_size); visit i; for every axis with d_a != 0, b_a = double(i_a + (d_a > 0 ? 1 : 0)) * voxel_size and
 *   t_a = (b_a - o_a) / d_a, both afresh at every step; the smallest t_a by strict < (ties to x, then y, then z); !(t_a < t_end) ends the walk;
 *   otherwise i_a +-= 1, and an index that leaves [-2^20, 2^20) ends the walk.  A walk that would make visit number max_steps + 1 ends instead
 *   and the ray is TRUNCATED (the visits made stay): max_steps bounds the work of one ray.
 *   Visit: the row of key(i) by binary search; on a hit, and with use_stamp != 0 only when t_last < stamp or t_first > stamp (the voxel was not
 *   being filled at that time), pierced[row] += 1 and hits += 1.  Rows are not filtered by count or moving fraction.
 * Outputs, both in/out (the call ADDS): pierced [capacity] i32;  counters [PCACC_PIERCE_COUNTERS] i64: rays walked, dropped, skipped,
 * truncated, hits.  Everything is an integer added with integer atomics: the result is a function of the SET of rays -- not of their order,
 * of how they were split over calls, or of the run.  No workspace is needed today (the query answers 0).
 * Return value: PCACC_E_ARG for n outside [0, 2^30], S < 1, m outside [0, capacity], a margin that is negative or not finite, a NaN max_range,
 * max_steps outside [1, 2^16], a voxel size that is not positive and finite or a NULL table of non-zero size; nothing is launched then.
 * n = 0 launches nothing; m = 0 walks the rays for the counters and addresses no table.
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_PIERCE_COUNTERS 5
#define PCACC_PIERCE_WALKED 0
#define PCACC_PIERCE_DROPPED 1
#define PCACC_PIERCE_SKIPPED 2
#define PCACC_PIERCE_TRUNCATED 3
#define PCACC_PIERCE_HITS 4
int pcacc_accum_pierce_workspace_bytes(int64_t n, int64_t m, size_t *bytes /*host*/);
int pcacc_accum_pierce(const float *points, int64_t n, const uint8_t *moving, const double *origins, int64_t n_origins,
                       const int32_t *origin_index, const double *pose, double voxel_size, double margin, double max_range,
                       int32_t use_stamp, int32_t stamp, int32_t max_steps, const int64_t *keys, const int32_t *stamps, int64_t capacity,
                       int64_t m, int32_t *pierced, int64_t *counters, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C8. Removing rows from the accumulated scene cloud: voxels that rays pierced, that nothing has touched for a while, that lie outside a box or
 * that have too few neighbours leave the map, on the device, by a predicate on the records.  Replaces the copy of the records to the host, a
 * mask there and a load.  Merges no maps, shrinks no table, is not iterated and returns no removed row.
 * Inputs
 *   in_keys, in_acc, in_stamps, in_capacity, m        the first m rows of a map, as for pcacc_accum_extract
 *   in_pierced [in_capacity] i32 or NULL              the sidecar of pcacc_accum_pierce
 *   min_count, use_fraction, max_moving_fraction      extract's filter
 *   use_stamp, before_stamp;  use_box, lo_x .. hi_z (voxel indices, inclusive);  min_pierced, use_ratio, ratio;  min_neighbors, radius
 * Stage A, per row, from that row's record alone; the tests run in this order and the first that holds is the row's reason:
 *   FILTER    extract does not keep the row (count < min_count, count <= 0 or, when use_fraction != 0, float64(moving) / float64(count) >
 *             max_moving_fraction or unordered)
 *   STALE     use_stamp != 0 and t_last < before_stamp
 *   BOX       use_box != 0 and a voxel index of the row lies outside [lo_a, hi_a]
 *   PIERCED   min_pierced > 0, in_pierced given, p = in_pierced[row] >= min_pierced and, when use_ratio != 0, float64(p) / float64(count) > ratio
 *             (one IEEE division, strict).  Without a sidecar no row leaves for this reason.
 * Stage B, when min_neighbors > 0, per stage-A survivor: k = the stage-A survivors with |delta|_inf <= radius, itself included, found as C5
 * finds neighbours (offsets that leave [-2^20, 2^20) are skipped before a key is formed).  ISOLATED iff k < min_neighbors.  One pass: k counts
 * stage-A survivors, never stage-B survivors, so the result is a function of the map alone.
 * Outputs
 *   out_keys, out_acc, out_stamps, out_pierced (out_capacity rows, distinct buffers): the surviving rows in key order, every record
 *   bit-identical to what it was; out_pierced is written iff in_pierced is given.
 *   counters [PCACC_PRUNE_COUNTERS] i64 (written, not added to): rows kept and rows removed per reason; they sum to m.
 *   dry_run != 0 computes only the counters: no table and no state word is written, and the out_* tables and state may be NULL.
 *   Otherwise state[PCACC_ACCUM_NUM_VOXELS] = rows kept, on the device; every other state word is left alone.
 * Return value: PCACC_E_ARG, and nothing is launched, for m outside [0, in_capacity], out_capacity < m (there is no "too small" path), an
 * output table that shares memory with an input table, min_neighbors outside [0, 343], radius outside 1..3 while min_neighbors > 0, a ratio
 * that is NaN or negative while use_ratio != 0, lo_a > hi_a or a bound outside [-2^20, 2^20) while use_box != 0, or a NULL table of non-zero
 * size.  m = 0 writes the zero counters and launches nothing else.
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_PRUNE_COUNTERS 6
#define PCACC_PRUNE_KEPT 0
#define PCACC_PRUNE_FILTER 1
#define PCACC_PRUNE_STALE 2
#define PCACC_PRUNE_BOX 3
#define PCACC_PRUNE_PIERCED 4
#define PCACC_PRUNE_ISOLATED 5
int pcacc_accum_prune_workspace_bytes(int64_t m, size_t *bytes /*host*/);
int pcacc_accum_prune(const int64_t *in_keys, const int64_t *in_acc, const int32_t *in_stamps, const int32_t *in_pierced, int64_t in_capacity,
                      int64_t m, int64_t min_count, int32_t use_fraction, double max_moving_fraction, int32_t use_stamp, int32_t before_stamp,
                      int32_t use_box, int32_t lo_x, int32_t lo_y, int32_t lo_z, int32_t hi_x, int32_t hi_y, int32_t hi_z, int32_t min_pierced,
                      int32_t use_ratio, double ratio, int32_t min_neighbors, int32_t radius, int32_t dry_run, int64_t *out_keys,
                      int64_t *out_acc, int32_t *out_stamps, int32_t *out_pierced, int64_t out_capacity, int64_t *counters, int64_t *state,
                      void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C9. Looking a scan's points up in the accumulated scene cloud: for every point, what the map knows at that place -- the record of the point's
 * own voxel, the nearest kept centroid among the 27 voxels around it and the signed distance to that voxel's plane.  Replaces the copy of up to
 * 8 M centroids to the host and a KD-tree there.  Answers one nearest neighbour within one voxel, not k and not a radius; does not modify the map.
 * Inputs
 *   points [n,3] f32, 0 <= n <= 2^30;  pose [4,4] f64 scan-to-world, rows 0-2 are read; NULL = identity
 *   voxel_size                of the map;  max_distance in (0, voxel_size]
 *   keys, acc, stamps, capacity, m; min_count, use_fraction, max_moving_fraction     the map and extract's filter, as for pcacc_accum_normals
 *   pierced [capacity] i32 or NULL                the sidecar of pcacc_accum_pierce
 *   normals [n_rows,3] f32, flags [n_rows] u8     out_normals / out_flags of pcacc_accum_normals on this map under this filter, or both NULL
 *   require_normal            non-zero: only rows with a valid normal are candidates (C6's candidate set); needs the tables
 * Per point, all float64 with no FMA contraction, only + - * / and sqrt, in the order csrc/accum_query.h writes down and no other:
 *   World: w = pose . p with C4's transform and C4's validity rule.  An invalid point gets PCACC_QUERY_INVALID and every other output at its
 *   default: it is never clamped and forms no key and no address.
 *   Own voxel: the map row whose key is the key of the point's voxel, if there is one: PCACC_QUERY_OCCUPIED; count, moving, t_first, t_last are
 *   the row's, pierced the sidecar's entry (0 without a sidecar); PCACC_QUERY_KEPT iff extract's filter keeps the row.  Without a row all are 0.
 *   Nearest kept centroid: C6's search -- the rows the filter keeps (with require_normal: that also have neither PCACC_NORMAL_FEW_NEIGHBORS nor
 *   PCACC_NORMAL_DEGENERATE) in the 3 x 3 x 3 voxels around the point's voxel, visited in ascending key order; offsets that leave [-2^20, 2^20)
 *   are skipped before a key is formed; d2 = (e_x e_x + e_y e_y) + e_z e_z against the float64 centroid, strict < (ties to the lowest key),
 *   accepted iff d2 <= max_distance^2.  On a match PCACC_QUERY_MATCHED, row = the row of pcacc_accum_extract under this filter (valid until the
 *   map changes), nearest = the float32 of the centroid (extract's point), distance = sqrt(d2).
 *   A centroid lies within 2^-17 m of its voxel, so one outside the 27 voxels is farther than voxel_size - 2^-17 from the point: for
 *   max_distance <= 0.9 voxel_size (voxel sizes of 1e-4 m and up) the match is the global nearest kept centroid within max_distance.  At
 *   max_distance = voxel_size the 27-voxel search itself is the contract, as in C6.
 *   Plane distance: with the tables and a matched row whose normal has neither flag: PCACC_QUERY_NORMAL and
 *   plane_distance = (n_x e_x + n_y e_y) + n_z e_z, n the float32 normal widened to double, e = w - centroid: C6's residual, signed.
 *   Defaults: row -1, nearest 0, distance and plane_distance +inf.
 * Outputs (device, n rows each, every row written once): out_status u8 (a sum of the bits below), out_count, out_moving i64, out_t_first,
 * out_t_last, out_pierced, out_row i32, out_nearest [n,3] f32, out_distance, out_plane_distance f64;
 * counters [PCACC_QUERY_COUNTERS] i64 (written, not added to): points, invalid, occupied, kept, matched, with a normal, and BAD_TABLE (0 / 1).
 * BAD_TABLE = 1: tables were given and n_rows differs from the rows the filter keeps (decided on the device): no normal table is addressed and
 * no point is MATCHED; world and own voxel are reported as always.  Every table index is range-checked against m, n_rows and capacity.
 * Return value: PCACC_E_ARG, and nothing is launched, for n outside [0, 2^30], m outside [0, capacity], a voxel size that is not positive and
 * finite, a max_distance that is NaN or outside (0, voxel_size], exactly one of normals / flags, require_normal without them, n_rows outside
 * [0, m] (or > 0 without tables), a NULL table or output of non-zero size, or a workspace that is too small.  n = 0 writes the zero counters and
 * launches nothing else; m = 0 launches only the point kernel: every valid point gets status 0.
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_QUERY_INVALID 1
#define PCACC_QUERY_OCCUPIED 2
#define PCACC_QUERY_KEPT 4
#define PCACC_QUERY_MATCHED 8
#define PCACC_QUERY_NORMAL 16
#define PCACC_QUERY_COUNTERS 7
#define PCACC_QUERY_N_POINTS 0
#define PCACC_QUERY_N_INVALID 1
#define PCACC_QUERY_N_OCCUPIED 2
#define PCACC_QUERY_N_KEPT 3
#define PCACC_QUERY_N_MATCHED 4
#define PCACC_QUERY_N_NORMAL 5
#define PCACC_QUERY_BAD_TABLE 6
int pcacc_accum_query_workspace_bytes(int64_t m, size_t *bytes /*host*/);
int pcacc_accum_query(const float *points, int64_t n, const double *pose, double voxel_size, double max_distance, const int64_t *keys,
                      const int64_t *acc, const int32_t *stamps, const int32_t *pierced, int64_t capacity, int64_t m, int64_t min_count,
                      int32_t use_fraction, double max_moving_fraction, const float *normals, const uint8_t *flags, int64_t n_rows,
                      int32_t require_normal, uint8_t *out_status, int64_t *out_count, int64_t *out_moving, int32_t *out_t_first,
                      int32_t *out_t_last, int32_t *out_pierced, int32_t *out_row, float *out_nearest, double *out_distance,
                      double *out_plane_distance, int64_t *counters, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C10. Casting rays into the accumulated scene cloud: looking from an origin towards a target, the first voxel the map keeps and how far away it
 * is -- a range image of the map from a sensor pose, the range the map predicts along a measured beam, visibility between two places.
 * Replaces the copy of up to 8 M keys to the host and a ray cast there.  Intersects no surfel or plane (the answer is a voxel and its centroid),
 * skips no empty space with a coarser structure, takes no stamp and does not modify the map.
 * Inputs
 *   targets [n,3] f32, 0 <= n <= 2^30         where the rays point (caller's frame)
 *   origins [S,3] f64, S >= 1                 where they start (caller's frame);  origin_index [n] i32 or NULL (= all 0): the row of a ray's origin
 *   pose [4,4] f64                            caller's frame to world, rows 0-2 are read; NULL = identity
 *   voxel_size                                of the map;  min_range >= 0, finite;  max_range: < 0 = none;  margin >= 0, finite, read only
 *                                             without a max_range;  max_steps in [1, 2^16]
 *   keys, acc, capacity, m; min_count, use_fraction, max_moving_fraction     the map and extract's filter, as for pcacc_accum_normals
 * Per ray, all float64 with no FMA contraction, only + - * / and sqrt, in the order csrc/accum_raycast.h writes down and no other:
 *   End points: o = pose . origin, e = pose . p with C4's transform.  PCACC_RAYCAST_DROPPED when origin_index lies outside [0, S) or a
 *   coordinate of o or e fails C4's validity rule: the ray is never clamped and forms no key and no address.
 *   Extent: d = e - o, L = sqrt((d_x^2 + d_y^2) + d_z^2), t_start = min_range / L; t_end = max_range / L with a max_range (the ray may run past
 *   its target), else 1 - margin / L (C7's formula: the ray runs to its target).  !(L > 0), !(t_end > 0) or !(t_start < t_end):
 *   PCACC_RAYCAST_SKIPPED.
 *   Walk: C7's, bit for bit.  The start voxel floor(o_a / voxel_size) has t_in = 0; per step b_a and t_a afresh, the smallest t_a by strict <
 *   (ties to x, then y, then z); !(t_a < t_end) ends the walk; otherwise the index moves, an index that leaves [-2^20, 2^20) ends the walk, and
 *   the entered voxel has t_in = t_a.  A walk that would make visit number max_steps + 1 ends instead: PCACC_RAYCAST_TRUNCATED.
 *   Visit: visits += 1.  A voxel with t_in < t_start is walked without a search.  Every other voxel is looked up by binary search; it is the
 *   HIT iff the map has its row and extract's filter keeps that row.  The walk stops at the first HIT; a walk that ends without one is a MISS.
 * Outputs (device, n rows each, every row written once): out_status u8 (one of the codes below); out_row i32: the row of pcacc_accum_extract
 * under this filter (valid until the map changes); out_coords [n,3] i32: the hit voxel; out_point [n,3] f32: the float32 of its float64 centroid
 * c (extract's point); out_range_in f64 = t_in L, where the ray enters the voxel; out_depth f64 = (((c_x - o_x) d_x + (c_y - o_y) d_y) +
 * (c_z - o_z) d_z) / L, the centroid's range along the ray; out_length f64 = L (0 for DROPPED); out_visits i32.  Without a HIT: row -1, coords
 * and point 0, range_in and depth +inf.  |depth - range_in| <= sqrt(3) voxel_size + 2^-17 plus rounding: a centroid lies within 2^-17 m of its
 * voxel.
 * counters [PCACC_RAYCAST_COUNTERS] i64 (written, not added to): rays, dropped, skipped, hit, missed, truncated -- the first is the sum of the
 * next five -- and the visits of all rays.
 * Return value: PCACC_E_ARG, and nothing is launched, for n outside [0, 2^30], S < 1, m outside [0, capacity], a voxel size that is not positive
 * and finite, a min_range or margin that is negative or not finite, a NaN max_range, max_steps outside [1, 2^16], a NULL table or output of
 * non-zero size, or a workspace that is too small.  n = 0 writes the zero counters and launches nothing else; m = 0 walks the rays and
 * addresses no table: every valid ray is MISS or TRUNCATED.
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_RAYCAST_MISS 0
#define PCACC_RAYCAST_HIT 1
#define PCACC_RAYCAST_TRUNCATED 2
#define PCACC_RAYCAST_SKIPPED 3
#define PCACC_RAYCAST_DROPPED 4
#define PCACC_RAYCAST_COUNTERS 7
#define PCACC_RAYCAST_N_RAYS 0
#define PCACC_RAYCAST_N_DROPPED 1
#define PCACC_RAYCAST_N_SKIPPED 2
#define PCACC_RAYCAST_N_HIT 3
#define PCACC_RAYCAST_N_MISSED 4
#define PCACC_RAYCAST_N_TRUNCATED 5
#define PCACC_RAYCAST_N_VISITS 6
int pcacc_accum_raycast_workspace_bytes(int64_t m, size_t *bytes /*host*/);
int pcacc_accum_raycast(const float *targets, int64_t n, const double *origins, int64_t n_origins, const int32_t *origin_index,
                        const double *pose, double voxel_size, double min_range, double max_range, double margin, int32_t max_steps,
                        const int64_t *keys, const int64_t *acc, int64_t capacity, int64_t m, int64_t min_count, int32_t use_fraction,
                        double max_moving_fraction, uint8_t *out_status, int32_t *out_row, int32_t *out_coords, float *out_point,
                        double *out_range_in, double *out_depth, double *out_length, int32_t *out_visits, int64_t *counters, void *workspace,
                        size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C11. Connected components of the accumulated scene cloud: which voxels belong together, with the size, box, centroid and stamps of every
 * connected set, and the removal of the small ones -- floating blobs that every per-voxel neighbour count lets through.  Replaces the copy of the
 * records to the host, a flood fill there and a load.  26-connectivity widened by a radius only: no 6- or 18-connectivity, no edge conditioned on
 * a distance or a normal, no label column stored in the map, no incremental relabelling.
 * pcacc_accum_components: inputs
 *   keys, acc, stamps, capacity, m; min_count, use_fraction, max_moving_fraction     the map and extract's filter, as for pcacc_accum_normals
 *   mask [mask_rows] u8 or NULL      over the rows of pcacc_accum_extract under the same filter; radius 1, 2 or 3
 * Map row i takes part iff the filter keeps it (extract row j) and, with a mask, mask[j] != 0.  Two rows that take part are adjacent iff
 * |delta|_inf <= radius; neighbours are found as C5 finds them (offsets that leave [-2^20, 2^20) are skipped before a key is formed).  The
 * components of that graph are numbered 0 .. K-1 in ascending order of their smallest key = their smallest extract row: a function of the map.
 * Outputs (device; every table has room for m rows)
 *   out_label [kept] i32             aligned with extract: the component of the row, -1 where the mask excludes it
 *   per component, K rows, each a function of the member set alone (integer sums, minima and maxima):
 *   out_voxels i32; out_points, out_moving i64 (sums of count and moving); out_sum_q [K,3] i64 (sums of the records' sum q; |.| < 2^62);
 *   out_centroid [K,3] f32 = float32(((double)sum_q_a / (double)points) * 2^-16); out_lo, out_hi [K,3] i32 (voxel indices, inclusive);
 *   out_t_first (minimum), out_t_last (maximum), out_first_row (extract row of the smallest key) i32
 *   counters [PCACC_COMPONENTS_COUNTERS] i64 (written, not added to): map rows = rows that take part + rows outside the filter + rows masked
 *   out; K; voxels of the largest component; status.
 * Status PCACC_COMPONENTS_BAD_MASK: a mask was given and mask_rows differs from the rows the filter keeps (decided on the device): no row takes
 * part, every label is -1, K = 0, every kept row counts as masked out.  PCACC_COMPONENTS_GAVE_UP: a join lost its compare-and-swap
 * 1024 times in a row against other lanes and was abandoned; the labels are then not to be used.  Rows of a table behind K (behind kept for
 * out_label) are not written.  The map is not modified.
 * pcacc_accum_remove_components: the second stage.  label, voxels, points, components_counters are out_label, out_voxels, out_points and counters
 * of pcacc_accum_components on this map under this filter, still on the device.  A row that takes part (label >= 0) is SMALL iff its component
 * has voxels < min_voxels or points < min_points (a threshold of 0 is off); rows that do not take part stay.  The surviving rows go, in key
 * order and every record bit-identical, to out_keys, out_acc, out_stamps and (iff in_pierced is given) out_pierced, as for pcacc_accum_prune.
 *   counters [PCACC_COMPONENTS_REMOVE_COUNTERS] i64 (written): rows kept, rows SMALL, components removed, components kept.
 *   dry_run != 0, or a first-stage status other than OK, computes only the counters: no table and no state word is written.
 *   Otherwise state[PCACC_ACCUM_NUM_VOXELS] = rows kept, on the device; every other state word is left alone.
 * Return value: PCACC_E_ARG, and nothing is launched, for m outside [0, capacity], radius outside 1..3, a negative threshold, mask_rows < 0, a
 * NULL table or output of non-zero size, a workspace that is too small and, for the removal, out_capacity < m or an output table that shares
 * memory with an input table.  m = 0 writes the zero counters and launches nothing else.  One workspace size serves both entries.
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_COMPONENTS_COUNTERS 7
#define PCACC_COMPONENTS_ROWS 0
#define PCACC_COMPONENTS_PARTICIPATING 1
#define PCACC_COMPONENTS_OUTSIDE 2
#define PCACC_COMPONENTS_MASKED 3
#define PCACC_COMPONENTS_K 4
#define PCACC_COMPONENTS_LARGEST 5
#define PCACC_COMPONENTS_STATUS 6
#define PCACC_COMPONENTS_OK 0
#define PCACC_COMPONENTS_BAD_MASK 1
#define PCACC_COMPONENTS_GAVE_UP 2
#define PCACC_COMPONENTS_REMOVE_COUNTERS 4
#define PCACC_COMPONENTS_REMOVE_KEPT 0
#define PCACC_COMPONENTS_REMOVE_SMALL 1
#define PCACC_COMPONENTS_REMOVED 2
#define PCACC_COMPONENTS_SURVIVED 3
int pcacc_accum_components_workspace_bytes(int64_t m, size_t *bytes /*host*/);
int pcacc_accum_components(const int64_t *keys, const int64_t *acc, const int32_t *stamps, int64_t capacity, int64_t m, int64_t min_count,
                           int32_t use_fraction, double max_moving_fraction, const uint8_t *mask, int64_t mask_rows, int32_t radius,
                           int32_t *out_label, int32_t *out_voxels, int64_t *out_points, int64_t *out_moving, int64_t *out_sum_q,
                           float *out_centroid, int32_t *out_lo, int32_t *out_hi, int32_t *out_t_first, int32_t *out_t_last,
                           int32_t *out_first_row, int64_t *counters, void *workspace, size_t workspace_bytes, void *stream);
int pcacc_accum_remove_components(const int64_t *in_keys, const int64_t *in_acc, const int32_t *in_stamps, const int32_t *in_pierced,
                                  int64_t in_capacity, int64_t m, int64_t min_count, int32_t use_fraction, double max_moving_fraction,
                                  const int32_t *label, const int32_t *voxels, const int64_t *points, const int64_t *components_counters,
                                  int64_t min_voxels, int64_t min_points, int32_t dry_run, int64_t *out_keys, int64_t *out_acc,
                                  int32_t *out_stamps, int32_t *out_pierced, int64_t out_capacity, int64_t *counters, int64_t *state,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C12. Two accumulated scene clouds into one, and a map under a rigid pose and / or a new voxel size.  Replaces the copy of both maps' records to
 * the host, a numpy join there and a load.  Applies no filter to either map, takes two maps per call, merges out of place, shrinks no table, and
 * computes no intersection or difference.
 * pcacc_accum_merge: two maps on ONE grid, exact.  Inputs
 *   a_keys, a_acc, a_stamps, a_capacity, ma           the first ma rows of map A;  b_*, b_capacity, mb: the first mb rows of map B
 *   a_pierced, b_pierced [capacity] i32 or NULL       the sidecars of pcacc_accum_pierce
 *   add_dropped                                       B's dropped points, which the host knows
 * Both maps are ascending and duplicate-free.  A and B may be the same tables.  The result goes OUT OF PLACE to out_keys, out_acc, out_stamps
 * (out_capacity rows) and, iff at least one sidecar is given, out_pierced: the keys are the ascending union.  A key in both maps gets count, moving
 * and the three coordinate sums added (int64), t_first = the minimum, t_last = the maximum and pierced = min(int64(a) + int64(b), 2^31 - 1); a key in
 * one map only is copied bit for bit, with a ray count of 0 when that side has no sidecar.  The result is the map one accumulator would hold had
 * it been given every add of both.
 *   counters [PCACC_MERGE_COUNTERS] i64 (written, not added to): status, rows of the union, keys in both maps, keys of B that A lacks, ray counts
 *   that were clamped.
 * Only the device knows ma + NEW.  If it exceeds out_capacity NOTHING is written to out_* or state, counters[STATUS] = PCACC_ACCUM_TOO_SMALL and
 * counters[NEEDED] says what it takes; A and B are intact.  Otherwise counters[STATUS] = 0, state[PCACC_ACCUM_NUM_VOXELS] = NEEDED,
 * state[PCACC_ACCUM_DROPPED] grows by add_dropped, and every other state word is left alone.
 * Return value: PCACC_E_ARG, and nothing is launched, for ma or mb outside [0, capacity], a capacity above 2^30, a NULL table of non-zero size or
 * an output table that shares memory with an input table; PCACC_E_WORKSPACE for a workspace that is too small.  ma = mb = 0 writes the zero
 * counters and state[NUM_VOXELS] = 0 and launches nothing else.
 * pcacc_accum_regrid: a map under a pose and / or on a grid of out_voxel_size.  A voxel is treated as `count` points at its centroid: LOSSY by
 * design (the points of a voxel that the new grid would separate stay together).  Per input row i < m, all float64 with no FMA contraction:
 *   usable iff 0 < count <= 2^31;  c_a = (float64(sum q_a) / float64(count)) * 2^-16, the centroid of C5
 *   w_a = ((r_a0 * c_x + r_a1 * c_y) + r_a2 * c_z) + t_a from rows 0-2 of pose (NULL = identity, through the same arithmetic)
 *   validity, i_a = floor(w_a / out_voxel_size), the key and q_a = llrint(w_a * 65536) exactly as C4 has them for a point
 * A usable, valid row contributes count, moving, count * q_a (|.| < 2^62), t_first, t_last and its ray count to the row of its key.  An unusable
 * or invalid row is never clamped and forms no address: it adds 1 to DROPPED_ROWS and max(count, 0) to DROPPED_POINTS.
 * Output: a new sorted map in out_keys, out_acc, out_stamps (out_capacity >= m rows: the result never has more rows than the input, there is no
 * "too small" path) and, iff in_pierced is given, out_pierced: rows with one key summed, stamps min / max, ray counts summed in int64 and stored
 * as min(sum, 2^31 - 1).  All eight words of the new map's state are written: NUM_VOXELS = rows, DROPPED = carry_dropped + DROPPED_POINTS, the
 * rest 0.  Integer sums commute: the result is bit-identical from run to run.
 *   counters [PCACC_REGRID_COUNTERS] i64 (written): rows in, rows out, rows dropped, points dropped, ray counts that were clamped.
 * Return value: PCACC_E_ARG, and nothing is launched, for m outside [0, in_capacity], out_capacity < m, a capacity above 2^30, an out_voxel_size
 * that is not positive and finite, a NULL table of non-zero size or an output table that shares memory with an input table.
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_MERGE_COUNTERS 5
#define PCACC_MERGE_STATUS 0           /* PCACC_ACCUM_OK or PCACC_ACCUM_TOO_SMALL */
#define PCACC_MERGE_NEEDED 1           /* rows of the union */
#define PCACC_MERGE_SHARED 2           /* keys in both maps */
#define PCACC_MERGE_NEW 3              /* keys of B that A lacks */
#define PCACC_MERGE_SATURATED 4        /* ray counts stored as 2^31 - 1 because the sum did not fit */
#define PCACC_REGRID_COUNTERS 5
#define PCACC_REGRID_ROWS_IN 0
#define PCACC_REGRID_ROWS_OUT 1
#define PCACC_REGRID_DROPPED_ROWS 2
#define PCACC_REGRID_DROPPED_POINTS 3
#define PCACC_REGRID_SATURATED 4
int pcacc_accum_merge_workspace_bytes(int64_t ma, int64_t mb, size_t *bytes /*host*/);
int pcacc_accum_merge(const int64_t *a_keys, const int64_t *a_acc, const int32_t *a_stamps, const int32_t *a_pierced, int64_t a_capacity,
                      int64_t ma, const int64_t *b_keys, const int64_t *b_acc, const int32_t *b_stamps, const int32_t *b_pierced,
                      int64_t b_capacity, int64_t mb, int64_t add_dropped, int64_t *out_keys, int64_t *out_acc, int32_t *out_stamps,
                      int32_t *out_pierced, int64_t out_capacity, int64_t *counters, int64_t *state, void *workspace, size_t workspace_bytes,
                      void *stream);
int pcacc_accum_regrid_workspace_bytes(int64_t m, size_t *bytes /*host*/);
int pcacc_accum_regrid(const int64_t *in_keys, const int64_t *in_acc, const int32_t *in_stamps, const int32_t *in_pierced, int64_t in_capacity,
                       int64_t m, const double *pose, double out_voxel_size, int64_t carry_dropped, int64_t *out_keys, int64_t *out_acc,
                       int32_t *out_stamps, int32_t *out_pierced, int64_t out_capacity, int64_t *counters, int64_t *state, void *workspace,
                       size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C13. Two accumulated scene clouds compared -- what changed? -- and the rows of pcacc_accum_extract that a mask names as a new map.  Replaces the
 * copy of both maps' records to the host and a numpy join there, and two one-way pcacc_accum_query calls on float32 centroids that name no row of
 * the other map.  Takes no pose and one voxel size, finds one nearest centroid within one voxel, compares no normals or stamps, makes no
 * free-space test, takes two maps per call and selects out of place.
 * pcacc_accum_compare: both directions in one call.  Inputs
 *   a_keys, a_acc, a_capacity, ma                      the first ma rows of map A;  b_*, b_capacity, mb: the first mb rows of map B
 *   a_pierced, b_pierced [capacity] i32 or NULL        the sidecars of pcacc_accum_pierce
 *   voxel_size; max_distance in (0, voxel_size]; min_count >= 1, use_fraction, max_moving_fraction: ONE filter for both maps, extract's
 * Both maps are ascending and duplicate-free, on ONE grid.  A and B may be the same tables.  Neither is modified.
 * Outputs (device), per side one row per row pcacc_accum_extract returns under the filter, in its order (every column has room for that side's
 * m rows; rows behind KEPT are not written).  For own row i that the filter keeps, against the other map O, all float64 with no FMA contraction:
 *   key = keys[i], idx = its voxel;  w_a = (float64(sum q_a) / float64(count)) * 2^-16, the centroid of C5
 *   HELD iff O holds the key, at its row q;  out_pierced = O's ray count at q (0 without a sidecar or without HELD)
 *   SAME iff HELD and the filter keeps O's row q;  out_same_row = that row's row of O's extract, else -1
 *   NEAR iff C9's nearest search finds a centroid: the kept rows of O in the 3 x 3 x 3 voxels around idx in ascending key order,
 *     d2 = (e_x e_x + e_y e_y) + e_z e_z, strict < (ties to the lowest key), accepted iff d2 <= max_distance^2;  out_row = its row of O's extract,
 *     out_distance = sqrt(d2); -1 and +inf without one.  For max_distance <= 0.9 voxel_size this is the nearest kept centroid of the whole of O.
 *   out_status u8 = a sum of PCACC_COMPARE_SAME, _HELD, _NEAR
 *   counters [PCACC_COMPARE_COUNTERS] i64 (written, not added to): for A at 0 and for B at PCACC_COMPARE_SIDE_COUNTERS, map rows, rows the filter
 *   keeps, and of those the rows with SAME, with HELD, with NEAR, and with neither SAME nor NEAR (ONLY).
 * A side with 0 rows has KEPT = 0 and nothing of it is addressed; every kept row of the other side is then ONLY.  ma = mb = 0 writes the zero
 * counters and launches nothing else.  Nothing is read back.
 * Return value: PCACC_E_ARG, and nothing is launched, for ma or mb outside [0, capacity], a capacity above 2^30, min_count < 1, a voxel_size or
 * max_distance that is not positive and finite, max_distance > voxel_size, a NULL table of non-zero size or an output column that is NULL while
 * its side has rows; PCACC_E_WORKSPACE for a workspace that is too small.
 * pcacc_accum_select: map row i is written iff the filter keeps it (extract row j) and (mask[j] != 0) != (invert != 0); mask [mask_rows] u8 over
 * the rows of pcacc_accum_extract under the same filter.  The selected rows go, in key order and every record and ray count bit-identical, to
 * out_keys, out_acc, out_stamps (out_capacity >= m rows: there is no "too small" path) and, iff in_pierced is given, out_pierced.  All eight words
 * of the new map's state are written: NUM_VOXELS = SELECTED, the rest 0.  The input map is not modified.
 *   counters [PCACC_SELECT_COUNTERS] i64 (written): status, map rows, rows the filter keeps, rows selected.
 * Status PCACC_SELECT_BAD_MASK: mask_rows differs from the rows the filter keeps (decided on the device): no mask entry is addressed and nothing
 * is written to the output tables or the state.
 * Return value: PCACC_E_ARG, and nothing is launched, for m outside [0, in_capacity], out_capacity < m, a capacity above 2^30, min_count < 1,
 * mask_rows < 0, a NULL table or mask of non-zero size, or an output table that shares memory with an input table; PCACC_E_WORKSPACE for a
 * workspace that is too small.
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_COMPARE_SAME 1
#define PCACC_COMPARE_HELD 2
#define PCACC_COMPARE_NEAR 4
#define PCACC_COMPARE_COUNTERS 12
#define PCACC_COMPARE_SIDE_COUNTERS 6  /* side A at 0, side B at 6 */
#define PCACC_COMPARE_ROWS 0           /* rows of the side's map */
#define PCACC_COMPARE_KEPT 1           /* rows the filter keeps = rows of the side's columns */
#define PCACC_COMPARE_N_SAME 2
#define PCACC_COMPARE_N_HELD 3
#define PCACC_COMPARE_N_NEAR 4
#define PCACC_COMPARE_N_ONLY 5         /* kept rows with neither SAME nor NEAR */
#define PCACC_SELECT_COUNTERS 4
#define PCACC_SELECT_STATUS 0          /* PCACC_SELECT_OK or PCACC_SELECT_BAD_MASK */
#define PCACC_SELECT_ROWS 1
#define PCACC_SELECT_KEPT 2
#define PCACC_SELECT_SELECTED 3
#define PCACC_SELECT_OK 0
#define PCACC_SELECT_BAD_MASK 1
int pcacc_accum_compare_workspace_bytes(int64_t ma, int64_t mb, size_t *bytes /*host*/);
int pcacc_accum_compare(const int64_t *a_keys, const int64_t *a_acc, const int32_t *a_pierced, int64_t a_capacity, int64_t ma,
                        const int64_t *b_keys, const int64_t *b_acc, const int32_t *b_pierced, int64_t b_capacity, int64_t mb,
                        double voxel_size, double max_distance, int64_t min_count, int32_t use_fraction, double max_moving_fraction,
                        uint8_t *out_a_status, int32_t *out_a_same_row, int32_t *out_a_row, double *out_a_distance, int32_t *out_a_pierced,
                        uint8_t *out_b_status, int32_t *out_b_same_row, int32_t *out_b_row, double *out_b_distance, int32_t *out_b_pierced,
                        int64_t *counters, void *workspace, size_t workspace_bytes, void *stream);
int pcacc_accum_select_workspace_bytes(int64_t m, size_t *bytes /*host*/);
int pcacc_accum_select(const int64_t *in_keys, const int64_t *in_acc, const int32_t *in_stamps, const int32_t *in_pierced, int64_t in_capacity,
                       int64_t m, int64_t min_count, int32_t use_fraction, double max_moving_fraction, const uint8_t *mask, int64_t mask_rows,
                       int32_t invert, int64_t *out_keys, int64_t *out_acc, int32_t *out_stamps, int32_t *out_pierced, int64_t out_capacity,
                       int64_t *counters, int64_t *state, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C14. Observed space: a second sorted voxel table, on C4's grid and key, of the voxels that measured laser rays crossed -- where the sensor looked
 * and found nothing.  With it a voxel has three states: occupied (a cloud holds it), free (rays crossed it), unknown (neither).  Replaces the copy
 * of every scan to the host and a ray walk into a dict there.  Counts no ray ends, keeps no hit / miss ratio or probability, decays nothing, merges
 * no two tables and regrids none.
 * The table: `capacity` rows, of which the first state[PCACC_OBSERVE_NUM_VOXELS] are in use, ascending and duplicate-free in `keys`:
 *   keys   [capacity] i64          C4's key
 *   rays   [capacity] i64          walked rays, over all calls, whose walk visited the voxel
 *   stamps [2][capacity] i32       smallest and largest stamp of the calls in which some ray visited the voxel
 *   state  [PCACC_OBSERVE_STATE_WORDS] i64 device words, all 0 for an empty table (indices below)
 * pcacc_accum_observe.  Inputs
 *   points, n, moving, origins, n_origins, origin_index, pose     the scan and origin arguments of pcacc_accum_pierce
 *   stamp; voxel_size; margin >= 0, finite; use_range, max_range >= 0 (read when use_range != 0); max_steps in [1, 2^16]
 *   visit_capacity in [1, 2^31)                                   the visits one call may make: the workspace is sized by it
 * A ray is C7's ray, bit for bit, up to the visit (csrc/accum_observe.h restates the loop of csrc/accum_pierce.h; the host build asserts the two
 * visit sequences equal): end points, the drop rule, "moving is SKIPPED", t_end with margin and max_range, the walk, max_steps and TRUNCATED.
 * Every visited voxel contributes its key -- the start voxel included, whether or not any cloud keeps the voxel.  The walk is monotone: one ray
 * visits a voxel at most once.  After the call rays[v] has grown by the walked rays of this call that visited v, and the stamps of those voxels
 * have taken `stamp` into their minimum and maximum.  All integers: the table is a function of the SET of (ray, stamp) pairs -- not of the order
 * of the rays, of how they were split over calls, or of the run.
 * Route: count the visits of every ray; scan; V = their total.  V > visit_capacity: state[STATUS] = PCACC_OBSERVE_TOO_MANY, state[NEEDED_VISITS]
 * = V and nothing else happens (the caller splits the rays).  Otherwise the walk runs again and writes its keys; radix sort; the length of a run
 * of equal keys is a voxel's ray count in this call (no atomics); every run is searched in the table; m + misses against out_capacity:
 * PCACC_ACCUM_TOO_SMALL and state[NEEDED] exactly as in pcacc_accum_add; otherwise the merge, OUT OF PLACE, into out_*.  Up to that decision no
 * table is touched.  On any status other than PCACC_ACCUM_OK, NUM_VOXELS and the cumulative counters stay: a retry counts nothing twice.  On OK
 * state[NUM_VOXELS] = rows of out_* and the five cumulative counters grow by this call's rays walked, dropped, skipped, truncated and by V.
 * A state[NUM_VOXELS] outside [0, in_capacity] addresses nothing: PCACC_ACCUM_BAD_STATE.
 * Return value: PCACC_E_ARG, and nothing is launched, for n outside [0, 2^30], n * max_steps >= 2^31 (the offsets are an int32 scan), S < 1, a
 * visit_capacity outside [1, 2^31), a margin that is negative or not finite, use_range with a max_range that is not >= 0, max_steps outside
 * [1, 2^16], a voxel size that is not positive and finite, a capacity above 2^30, out_capacity < 1, a NULL table of non-zero size or an output
 * table that shares memory with an input table; PCACC_E_WORKSPACE for a workspace that is too small.  n = 0 launches nothing (the state is not
 * touched); in_capacity = 0 or state[NUM_VOXELS] = 0 is a plain build of the table.
 * pcacc_accum_observed_lookup: what the first m rows of a table know about n rows.  Exactly one of points [n,3] f32 (through pose, C4's transform
 * and validity rule) and coords [n,3] i32 (voxel indices; valid iff every index lies in [-2^20, 2^20)) is non-NULL.
 *   out_status [n] u8 = a sum of PCACC_OBSERVED_VALID, _SEEN (the table holds the key), _ENOUGH (SEEN and rays >= min_rays)
 *   out_rays [n] i64, out_stamps [2][n] i32 (t_first, t_last): the row's record; 0 where unseen or invalid.  Every output of every row is written.
 *   counters [PCACC_OBSERVED_COUNTERS] i64 (written, not added to): rows, valid, seen, enough.
 * One launch, one lane per row, nothing read back.  Every table index comes out of a binary search and is checked against m.
 * Return value: PCACC_E_ARG, and nothing is launched, for n outside [0, 2^30], m outside [0, capacity] (a table that does not fit addresses
 * nothing), a capacity above 2^30, a voxel size that is not positive and finite, both or neither of points and coords with n > 0, or a NULL
 * table or output of non-zero size.  n = 0 writes the zero counters and launches nothing.
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_OBSERVE_STATE_WORDS 16
#define PCACC_OBSERVE_NUM_VOXELS 0     /* rows in use */
#define PCACC_OBSERVE_STATUS 1         /* of the last call: PCACC_ACCUM_OK, _TOO_SMALL, _BAD_STATE or PCACC_OBSERVE_TOO_MANY */
#define PCACC_OBSERVE_NEEDED 2         /* rows the last call's merged table takes */
#define PCACC_OBSERVE_NEEDED_VISITS 3  /* V of the last call that was TOO_MANY */
#define PCACC_OBSERVE_CALL_VISITS 4    /* V of the last call */
#define PCACC_OBSERVE_CALL_VOXELS 5    /* distinct voxels the last call's rays visited */
#define PCACC_OBSERVE_WALKED 6         /* cumulative, of all calls that ended OK: rays walked, ... */
#define PCACC_OBSERVE_DROPPED 7
#define PCACC_OBSERVE_SKIPPED 8
#define PCACC_OBSERVE_TRUNCATED 9
#define PCACC_OBSERVE_VISITS 10        /* ... and voxels visited */
#define PCACC_OBSERVE_TOO_MANY 3
#define PCACC_OBSERVED_VALID 1
#define PCACC_OBSERVED_SEEN 2
#define PCACC_OBSERVED_ENOUGH 4
#define PCACC_OBSERVED_COUNTERS 4
#define PCACC_OBSERVED_ROWS 0
#define PCACC_OBSERVED_N_VALID 1
#define PCACC_OBSERVED_N_SEEN 2
#define PCACC_OBSERVED_N_ENOUGH 3
int pcacc_accum_observe_workspace_bytes(int64_t n, int64_t visit_capacity, int64_t in_m, size_t *bytes /*host*/);
int pcacc_accum_observe(const float *points, int64_t n, const uint8_t *moving, const double *origins, int64_t n_origins,
                        const int32_t *origin_index, const double *pose, int32_t stamp, double voxel_size, double margin, int32_t use_range,
                        double max_range, int32_t max_steps, int64_t visit_capacity, const int64_t *in_keys, const int64_t *in_rays,
                        const int32_t *in_stamps, int64_t in_capacity, int64_t *out_keys, int64_t *out_rays, int32_t *out_stamps,
                        int64_t out_capacity, int64_t *state, void *workspace, size_t workspace_bytes, void *stream);
int pcacc_accum_observed_lookup_workspace_bytes(int64_t n, int64_t m, size_t *bytes /*host*/);
int pcacc_accum_observed_lookup(const float *points, const int32_t *coords, int64_t n, const double *pose, double voxel_size, const int64_t *keys,
                                const int64_t *rays, const int32_t *stamps, int64_t capacity, int64_t m, int64_t min_rays, int64_t *out_rays,
                                int32_t *out_stamps, uint8_t *out_status, int64_t *counters, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C15. Two tables of observed space (C14) into one, and a table under a rigid pose and / or a new voxel size.  Replaces the copy of both tables'
 * records to the host, a numpy join there and a load.  Keeps no hit / miss ratio, re-observes nothing under a pose (that needs the rays), keeps no
 * upper-bound column beside the maximum and no pyramid, takes two tables per call, merges out of place and filters no row.
 * pcacc_accum_observed_merge: two tables on ONE grid, exact.  Inputs
 *   a_keys, a_rays, a_stamps, a_capacity, ma          the first ma rows of table A;  b_*, b_capacity, mb: the first mb rows of table B
 *   b_state [16] (read), state [16] (read and written) the state words of B and of A
 * Both tables are ascending and duplicate-free.  A and B may be the same tables and the same state words: B's words are read before any word of
 * `state` is written.  The result goes OUT OF PLACE to out_keys, out_rays, out_stamps (out_capacity rows): the keys are the ascending duplicate-free
 * union.  A key in both tables gets rays = a + b (int64, not clamped: a ray count is at most the WALKED word of its table, which grows by at most
 * 2^30 per observe call, so 2^63 is out of reach), t_first = the minimum, t_last = the maximum; a key in one table only is copied bit for bit.
 * The tables and the five cumulative counters are, integer for integer, what ONE table would hold had it been given every observe of both.
 *   counters [PCACC_OBSERVED_MERGE_COUNTERS] i64 (written, not added to): status, rows of the union, keys in both tables, keys of B that A lacks.
 * Route: one lane per row of B searches A; the misses are scanned; one thread decides; old row p goes to p + (misses below it) with B's row added
 * where it hit, missed row j to position + rank.  No atomic.  Up to the decision no table is touched.
 * state[NUM_VOXELS] != ma or b_state[NUM_VOXELS] != mb: counters[STATUS] = PCACC_ACCUM_BAD_STATE, the other counters 0, and no table is addressed.
 * NEEDED > out_capacity: counters[STATUS] = PCACC_ACCUM_TOO_SMALL, counters[NEEDED] says what it takes and NOTHING is written to out_* or state.
 * Otherwise counters[STATUS] = 0 and state[NUM_VOXELS] = NEEDED, state[STATUS] = 0, state[NEEDED] = NEEDED, state[NEEDED_VISITS] =
 * state[CALL_VISITS] = state[CALL_VOXELS] = 0 (a merge walks nothing), the five cumulative counters become A's plus B's; words 11 - 15 are left alone.
 * Return value: PCACC_E_ARG, and nothing is launched, for ma or mb outside [0, capacity], a capacity above 2^30, a NULL table of non-zero size or
 * an output table that shares a byte with an input table; PCACC_E_WORKSPACE for a workspace that is too small.  ma = mb = 0 writes the zero
 * counters and launches nothing else.
 * pcacc_accum_observed_regrid: a table under a pose and / or on a grid of out_voxel_size.  A row is treated as the CENTRE of its voxel: LOSSY by
 * declared contract.  Per input row i < m, all float64 with no FMA contraction:
 *   c = the voxel indices of the key;  p_a = (float64(c_a) + 0.5) * in_voxel_size
 *   w_a, validity, i_a = floor(w_a / out_voxel_size) and the key exactly as pcacc_accum_regrid (C12) has them for a centroid: rows 0-2 of pose (NULL =
 *   identity, through the same arithmetic), C4's validity rule (|w_a| < 32768 included)
 * A row whose centre is invalid is never clamped and forms no address: it adds 1 to DROPPED_ROWS.  Rows that land on one key become one row: rays =
 * the MAXIMUM over the sources, t_first = the minimum, t_last = the maximum.  The maximum and not C12's sum: a ray that crossed k source voxels of one
 * destination voxel is one ray, and overstating the evidence for "free" is the unsafe direction.  For a nested coarsening the maximum is a lower
 * bound on the rays that crossed the coarse voxel; under a rotation it is an estimate, and at an unchanged voxel size some destination voxels
 * receive no centre at all (they read unknown): give a coarser out_voxel_size with a rotation.
 * Two properties are part of the contract: (a) NULL or identity pose and out_voxel_size == in_voxel_size returns the input table bit for bit (for
 * rows whose centre is valid, which every row that pcacc_accum_observe wrote is); (b) identity pose and out_voxel_size = f * in_voxel_size for an
 * integer f gives floor(i / f) per axis.
 * Output: a new sorted table in out_keys, out_rays, out_stamps (out_capacity >= m rows: the result never has more rows than the input, there is no
 * "too small" path).  All sixteen words of out_state are written: NUM_VOXELS = rows out, the five cumulative counters copied from in_state, the
 * rest 0.  The counters describe the RAYS the input was given, which are not walked again: VISITS no longer equals the sum of `rays`.
 *   counters [PCACC_OBSERVED_REGRID_COUNTERS] i64 (written): rows in, rows out, rows dropped.
 * in_state[NUM_VOXELS] != m: out_state[STATUS] = PCACC_ACCUM_BAD_STATE, the counters are zero (ROWS_IN != m tells the caller) and nothing else is
 * written.  Integer max and min commute: the result is bit-identical from run to run.
 * Return value: PCACC_E_ARG, and nothing is launched, for m outside [0, in_capacity], out_capacity < m, a capacity above 2^30, a voxel size on either
 * side that is not positive and finite, a NULL table of non-zero size or an output table that shares a byte with an input table.
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_OBSERVED_MERGE_COUNTERS 4
#define PCACC_OBSERVED_MERGE_STATUS 0  /* PCACC_ACCUM_OK, _TOO_SMALL or _BAD_STATE */
#define PCACC_OBSERVED_MERGE_NEEDED 1  /* rows of the union */
#define PCACC_OBSERVED_MERGE_SHARED 2  /* keys in both tables */
#define PCACC_OBSERVED_MERGE_NEW 3     /* keys of B that A lacks */
#define PCACC_OBSERVED_REGRID_COUNTERS 3
#define PCACC_OBSERVED_REGRID_ROWS_IN 0
#define PCACC_OBSERVED_REGRID_ROWS_OUT 1
#define PCACC_OBSERVED_REGRID_DROPPED_ROWS 2
int pcacc_accum_observed_merge_workspace_bytes(int64_t ma, int64_t mb, size_t *bytes /*host*/);
int pcacc_accum_observed_merge(const int64_t *a_keys, const int64_t *a_rays, const int32_t *a_stamps, int64_t a_capacity, int64_t ma,
                               const int64_t *b_keys, const int64_t *b_rays, const int32_t *b_stamps, int64_t b_capacity, int64_t mb,
                               const int64_t *b_state, int64_t *out_keys, int64_t *out_rays, int32_t *out_stamps, int64_t out_capacity,
                               int64_t *counters, int64_t *state, void *workspace, size_t workspace_bytes, void *stream);
int pcacc_accum_observed_regrid_workspace_bytes(int64_t m, size_t *bytes /*host*/);
int pcacc_accum_observed_regrid(const int64_t *in_keys, const int64_t *in_rays, const int32_t *in_stamps, int64_t in_capacity, int64_t m,
                                const int64_t *in_state, const double *pose, double in_voxel_size, double out_voxel_size, int64_t *out_keys,
                                int64_t *out_rays, int32_t *out_stamps, int64_t out_capacity, int64_t *counters, int64_t *out_state,
                                void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C16. The k nearest kept centroids of the accumulated scene cloud within a few voxels: of every point of a scan (pcacc_accum_knn), or of
 * every kept centroid of the map itself (pcacc_accum_knn_self: the base of a statistical outlier removal).  Replaces the copy of the map to
 * the host and a KD-tree there.  Does not modify the map.  C9 answers one neighbour within one voxel; this answers k within `radius` voxels.
 * Inputs
 *   k in [1, PCACC_KNN_MAX_K], radius in [1, PCACC_KNN_MAX_RADIUS] voxels, max_distance in (0, radius * voxel_size]
 *   points [n,3] f32, 0 <= n <= 2^30;  pose [4,4] f64 scan-to-world, rows 0-2 are read; NULL = identity            (pcacc_accum_knn only)
 *   keys, acc, capacity, m; min_count, use_fraction, max_moving_fraction      the map and extract's filter, as for pcacc_accum_normals
 * Per query, all float64 with no FMA contraction, only + - * / and sqrt, in the order csrc/accum_knn.h writes down and no other:
 *   Query: a scan point under the pose with C4's transform and validity rule (an invalid point gets PCACC_KNN_INVALID, found 0 and padding:
 *   never clamped, no key, no address), or kept row j of the map: its float64 centroid in the voxel of its KEY, the row itself excluded.
 *   Candidates: the rows the filter keeps in the (2 radius + 1)^3 voxels around the query's voxel; offsets that leave [-2^20, 2^20) are
 *   skipped before a key is formed.  d2 = (e_x e_x + e_y e_y) + e_z e_z against the float64 centroid (C9's arithmetic); accepted iff
 *   d2 <= max_distance^2.
 *   Result: the up-to-k accepted candidates with the smallest (d2, key) -- a total order: the answer does not depend on the order the voxels
 *   are visited in, ties go to the lower key = the lower row of pcacc_accum_extract -- in that ascending order: out_rows [.,k] = extract's row
 *   (valid until the map changes), out_distance [.,k] = sqrt(d2); padded with -1 / +inf; out_found in [0, k]; out_status = PCACC_KNN_INVALID,
 *   or PCACC_KNN_FOUND (found >= 1) plus PCACC_KNN_FULL (found == k).  Self mode adds out_mean_distance = (((d_0 + d_1) + d_2) + ...) / found
 *   in that order, +inf for found = 0.
 *   A centroid lies within 2^-17 m of its voxel.  A scan point lies in its voxel, so a centroid outside the block is farther than
 *   radius * voxel_size - 2^-17; a self query may itself lie 2^-17 outside its voxel: radius * voxel_size - 2^-16.  For max_distance <=
 *   (radius - 0.1) voxel_size and voxel sizes of 1 mm and up the result is the k nearest kept centroids of the WHOLE map within
 *   max_distance.  At max_distance = radius * voxel_size the block search itself is the contract.
 * Outputs (device; pcacc_accum_knn: n rows, every row written once; pcacc_accum_knn_self: room for m rows, the first *out_n -- the rows of
 * pcacc_accum_extract under this filter, row for row -- written once each): out_rows i32 [.,k], out_distance f64 [.,k], out_found i32,
 * out_status u8, out_mean_distance f64; counters [PCACC_KNN_COUNTERS] i64 (written, not added to): queries, invalid, with at least one
 * neighbour, with k neighbours, neighbours in total.  Every table index is range-checked against m and capacity.
 * Return value: PCACC_E_ARG, and nothing is launched, for k, radius or n outside their ranges, m outside [0, capacity], a capacity above 2^30,
 * a voxel size that is not positive and finite, a max_distance that is NaN or outside (0, radius * voxel_size], a NULL table or output of
 * non-zero size, or a workspace that is too small.  n = 0 writes the zero counters and launches nothing else; m = 0 gives padding everywhere
 * (pcacc_accum_knn) / *out_n = 0 and the zero counters (pcacc_accum_knn_self).
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_KNN_MAX_K 16
#define PCACC_KNN_MAX_RADIUS 4
#define PCACC_KNN_INVALID 1
#define PCACC_KNN_FOUND 2
#define PCACC_KNN_FULL 4
#define PCACC_KNN_COUNTERS 5
#define PCACC_KNN_N_QUERIES 0
#define PCACC_KNN_N_INVALID 1
#define PCACC_KNN_N_FOUND 2
#define PCACC_KNN_N_FULL 3
#define PCACC_KNN_N_NEIGHBORS 4
int pcacc_accum_knn_workspace_bytes(int64_t m, size_t *bytes /*host*/);
int pcacc_accum_knn(const float *points, int64_t n, const double *pose, double voxel_size, double max_distance, int32_t k, int32_t radius,
                    const int64_t *keys, const int64_t *acc, int64_t capacity, int64_t m, int64_t min_count, int32_t use_fraction,
                    double max_moving_fraction, int32_t *out_rows, double *out_distance, int32_t *out_found, uint8_t *out_status,
                    int64_t *counters, void *workspace, size_t workspace_bytes, void *stream);
int pcacc_accum_knn_self(double voxel_size, double max_distance, int32_t k, int32_t radius, const int64_t *keys, const int64_t *acc,
                         int64_t capacity, int64_t m, int64_t min_count, int32_t use_fraction, double max_moving_fraction, int32_t *out_rows,
                         double *out_distance, int32_t *out_found, uint8_t *out_status, double *out_mean_distance, int64_t *out_n,
                         int64_t *counters, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C17. The (x, y) columns of the accumulated scene cloud: the local ground under every column, the height of every voxel above it, what stands
 * in a height band, and bird's-eye-view rasters of a window of columns.  Replaces the copy of extract() to the host, an np.unique over (x, y) and
 * a minimum filter there.  Does not modify the map.  The contract is csrc/accum_columns.h, the same code in the kernels and in a g++ build.
 * Inputs
 *   keys, acc, stamps, capacity, m; min_count, use_fraction, max_moving_fraction     the map and extract's filter, as for pcacc_accum_normals
 *   ground_radius R in [0, PCACC_COLUMNS_MAX_RADIUS] columns; thickness in [0, PCACC_COLUMNS_MAX_HEIGHT] voxels;
 *   0 <= band_lo <= band_hi <= PCACC_COLUMNS_MAX_HEIGHT voxels above the ground
 * Everything is over the rows the filter keeps; j is a row of pcacc_accum_extract under the same filter.  Keys ascend in (x, y, z), so a column
 * is a run of consecutive rows, ascending in z.
 *   Columns: column key = key >> 21; row j is a head iff j == 0 or its column key differs from that of row j - 1; columns are numbered in key
 *   order, C of them.  Per column (C rows): col_key i64 (x + 2^20) << 21 | (y + 2^20); col_xy i32 [.,2]; col_first_row, col_voxels i32 (the column
 *   is rows [first_row, first_row + voxels)); col_points, col_moving i64 (sums of count and moving); col_z_low, col_z_high i32 (voxel index z of
 *   the first and the last row); col_t_first = min, col_t_last = max of the stamps.
 *   Ground: col_ground_z = min col_z_low over the columns that exist within R of the column on both axes, itself included; the supplier minimises
 *   (z_low, column key), a total order: ties go to the lower key; col_ground_row = the supplier's first_row, col_ground_column = its index.  A
 *   neighbour outside [-2^20, 2^20) contributes nothing and forms no key.
 *   Band: col_band_voxels = rows of the column with band_lo <= z - ground_z <= band_hi; col_band_top = the largest such z - ground_z, or -1.
 *   Per row j: row_column i32; row_height i32 = z - ground_z(column) >= 0; row_is_ground u8 = height <= thickness; row_height_m f64 = the float64
 *   z centroid ((sum q_z / count) * 2^-16) of row j minus that of ground_row(column), one subtraction; it may be slightly negative (a centroid
 *   can lie 2^-17 m outside its voxel).
 * Outputs (device): every column table and every row table has room for m rows; the first out_n[1] = C rows of the column tables and the first
 * out_n[0] = kept rows of the row tables are written, once each; out_n [2] i64; counters [PCACC_COLUMNS_COUNTERS] i64 (written, not added to):
 * kept rows, columns, ground rows, rows in the band, columns whose ground came from another column.
 * pcacc_accum_bev: a width x height window of columns at the integer origin (x0, y0), |x0|, |y0| <= 2^31, width, height >= 1, width * height <=
 * PCACC_BEV_MAX_PIXELS; pixel (r, c) = element r * width + c is column (x0 + c, y0 + r).  It takes the column tables of pcacc_accum_columns
 * (n_columns = C, from the host) and the map under the SAME filter.  A pixel whose column lies outside the grid or is not in the list is empty:
 * out_column -1, out_elevation and out_ground NaN, out_band_top -1, out_voxels 0.  Otherwise out_column i32 = its index, out_elevation f32 =
 * pcacc_accum_extract's z of the column's top row (first_row + voxels - 1), out_ground f32 = that of ground_row, out_band_top, out_voxels i32.
 * Every pixel is written once.  n_columns = 0 gives an all-empty image.
 * Return value: PCACC_E_ARG, and nothing is launched, for a NULL table or output of non-zero size, NULL out_n, counters or workspace, m outside
 * [0, capacity], a capacity above 2^30, n_columns outside [0, m], a radius, thickness, band or window outside its range, a workspace below
 * pcacc_accum_columns_workspace_bytes(m) (both entries), or an output that shares a byte with a table of the map.  m = 0: zero counts.
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_COLUMNS_MAX_RADIUS 8
#define PCACC_COLUMNS_MAX_HEIGHT 2097151
#define PCACC_BEV_MAX_PIXELS ((int64_t)1 << 28)
#define PCACC_COLUMNS_COUNTERS 5
#define PCACC_COLUMNS_N_ROWS 0
#define PCACC_COLUMNS_N_COLUMNS 1
#define PCACC_COLUMNS_N_GROUND 2
#define PCACC_COLUMNS_N_BAND 3
#define PCACC_COLUMNS_N_BORROWED 4
int pcacc_accum_columns_workspace_bytes(int64_t m, size_t *bytes /*host*/);
int pcacc_accum_columns(const int64_t *keys, const int64_t *acc, const int32_t *stamps, int64_t capacity, int64_t m, int64_t min_count,
                        int32_t use_fraction, double max_moving_fraction, int32_t ground_radius, int32_t thickness, int32_t band_lo,
                        int32_t band_hi, int64_t *col_key, int32_t *col_xy, int32_t *col_first_row, int32_t *col_voxels, int64_t *col_points,
                        int64_t *col_moving, int32_t *col_z_low, int32_t *col_z_high, int32_t *col_t_first, int32_t *col_t_last,
                        int32_t *col_ground_z, int32_t *col_ground_row, int32_t *col_ground_column, int32_t *col_band_voxels,
                        int32_t *col_band_top, int32_t *row_column, int32_t *row_height, uint8_t *row_is_ground, double *row_height_m,
                        int64_t *out_n, int64_t *counters, void *workspace, size_t workspace_bytes, void *stream);
int pcacc_accum_bev(const int64_t *keys, const int64_t *acc, int64_t capacity, int64_t m, int64_t min_count, int32_t use_fraction,
                    double max_moving_fraction, const int64_t *col_key, const int32_t *col_first_row, const int32_t *col_voxels,
                    const int32_t *col_ground_row, const int32_t *col_band_top, int64_t n_columns, int64_t x0, int64_t y0, int64_t width,
                    int64_t height, int32_t *out_column, float *out_elevation, float *out_ground, int32_t *out_band_top, int32_t *out_voxels,
                    void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C18. Planar segments of the accumulated scene cloud by normal-gated region growing: which voxels lie on one surface, with the size, box, stamps
 * and least-squares plane of every segment and every voxel's distance to its plane.  C11 joins every voxel within `radius` of another, so a floor
 * and the walls on it are one component; here an edge also needs the two normals of C5 to agree and each centroid to lie near the other's tangent
 * plane.  Replaces the copy of extract() and normals() to the host and a region growing there.  The contract is csrc/accum_planes.h, the same code
 * in the kernels and in a g++ build.  No RANSAC or growth against a running plane (order-dependent), no merging of coplanar segments across gaps,
 * no cylinders, no label column stored in the map, no incremental relabelling, no planes across two maps, no viewpoint-oriented segment normals.
 * Inputs
 *   keys, acc, stamps, capacity, m; min_count, use_fraction, max_moving_fraction     the map and extract's filter, as for pcacc_accum_normals
 *   normals, eigenvalues [n_rows,3] f32, flags [n_rows] u8     the outputs of pcacc_accum_normals on this map under this filter, on the device
 *   mask [mask_rows] u8 or NULL      over the rows of pcacc_accum_extract under the same filter
 *   radius 1, 2 or 3 voxels; cos_angle in [0, 1]; max_offset >= 0 metres; max_variation in [0, 1]
 * Extract row j takes part iff the filter keeps it, mask[j] != 0 (with a mask), flags[j] has neither FEW_NEIGHBORS nor DEGENERATE, and
 * (double)e2 <= max_variation * (((double)e0 + (double)e1) + (double)e2) with e = eigenvalues[j]; the first test that fails names the counter.
 * Two rows i, p that take part with |delta|_inf <= radius (found as C11 finds them) are joined iff, in float64 with no FMA contraction,
 *   |(n_ix n_px + n_iy n_py) + n_iz n_pz| >= cos_angle, and with d = c_p - c_i (c: ((double)sum q_a / (double)count) * 2^-16)
 *   |(n_ix d_x + n_iy d_y) + n_iz d_z| <= max_offset and |(n_px d_x + n_py d_y) + n_pz d_z| <= max_offset.
 * The rule is symmetric bit for bit, so the segments -- the connected components of that graph, numbered 0 .. K-1 by their smallest extract row --
 * are a function of the records and the given normals alone.
 * Outputs (device; every table has room for m rows)
 *   out_label [kept] i32             the segment of the row, -1 where it does not take part
 *   out_distance [kept] f64          ((n_x c_x + n_y c_y) + n_z c_z) - offset against the row's own segment; 0.0 for label -1 or a degenerate one
 *   per segment, K rows: out_voxels i32; out_points i64; out_lo, out_hi [K,3] i32; out_first_row, out_t_first, out_t_last i32 as in C11;
 *   out_anchor [K,3] i32 = A, the integer centroid u_a = floor(sum q_a / count) of first_row; out_spread i64 = D = max over members and axes of
 *   |u_a - A_a|; out_shift i32 = s, the smallest s >= 0 with t = (D >> s) + 1 <= 2^31 and t t <= 2^62 / voxels; with e_a = (u_a - A_a) >> s:
 *   out_s1 [K,3] i64 = sum e_a, out_s2 [K,6] i64 = sum e_a e_b (xx, xy, xz, yy, yz, zz), each voxel once: integers, so any order gives these bits.
 *   The fit, a fixed float64 sequence per segment: mu_a = S1_a / voxels; C_ab = S2_ab / voxels - mu_a mu_b; the 3x3 SVD of svd3.h gives
 *   s0 >= s1 >= s2 and u; scale = 2^(s - 16); out_normal [K,3] f64 = u[:,2], flipped iff the first non-zero of (n_z, n_y, n_x) is negative;
 *   out_eigenvalues [K,3] f64 = s_k (scale scale); out_centroid [K,3] f64 = (A_a + mu_a 2^s) 2^-16; out_offset f64 = (n_x c_x + n_y c_y) + n_z c_z;
 *   out_mse f64 = s2 (scale scale); out_flags u8: PCACC_PLANE_DEGENERATE when s1 <= 64 * 2^-52 * s0 (fewer than three voxels that are not
 *   collinear): normal, offset and mse are then 0.0.
 *   counters [PCACC_PLANES_COUNTERS] i64 (written, not added to): map rows = rows that take part + outside the filter + masked out + without a
 *   valid normal + not flat; K; voxels of the largest segment; status.
 * Status PCACC_PLANES_BAD_ROWS: n_rows, or mask_rows with a mask, differs from the rows the filter keeps (decided on the device): no row takes
 * part, every label is -1, K = 0, every kept row counts as masked out.  PCACC_PLANES_GAVE_UP: as PCACC_COMPONENTS_GAVE_UP.  Rows of a table
 * behind K (behind kept for out_label and out_distance) are not written.  The map is not modified.
 * Return value: PCACC_E_ARG, and nothing is launched, for m outside [0, capacity], radius outside 1..3, cos_angle or max_variation outside [0, 1]
 * or NaN, a negative or NaN max_offset, a negative row count, a NULL table or output of non-zero size, a workspace that is too small, or an output
 * that shares a byte with a table of the map or with an input.  m = 0 writes the zero counters and launches nothing else.
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_PLANES_COUNTERS 9
#define PCACC_PLANES_ROWS 0
#define PCACC_PLANES_PARTICIPATING 1
#define PCACC_PLANES_OUTSIDE 2
#define PCACC_PLANES_MASKED 3
#define PCACC_PLANES_INVALID 4
#define PCACC_PLANES_NOT_FLAT 5
#define PCACC_PLANES_K 6
#define PCACC_PLANES_LARGEST 7
#define PCACC_PLANES_STATUS 8
#define PCACC_PLANES_OK 0
#define PCACC_PLANES_BAD_ROWS 1
#define PCACC_PLANES_GAVE_UP 2
#define PCACC_PLANE_DEGENERATE 1
int pcacc_accum_planes_workspace_bytes(int64_t m, size_t *bytes /*host*/);
int pcacc_accum_planes(const int64_t *keys, const int64_t *acc, const int32_t *stamps, int64_t capacity, int64_t m, int64_t min_count,
                       int32_t use_fraction, double max_moving_fraction, const float *normals, const float *eigenvalues, const uint8_t *flags,
                       int64_t n_rows, const uint8_t *mask, int64_t mask_rows, int32_t radius, double cos_angle, double max_offset,
                       double max_variation, int32_t *out_label, double *out_distance, int32_t *out_voxels, int64_t *out_points,
                       int32_t *out_lo, int32_t *out_hi, int32_t *out_first_row, int32_t *out_t_first, int32_t *out_t_last,
                       int32_t *out_anchor, int64_t *out_spread, int32_t *out_shift, int64_t *out_s1, int64_t *out_s2, double *out_normal,
                       double *out_eigenvalues, double *out_centroid, double *out_offset, double *out_mse, uint8_t *out_flags,
                       int64_t *counters, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * C19. The exact, truncated Euclidean distance field of a box of voxels of the accumulated scene cloud, with the nearest row (a feature transform):
 * how far is every voxel of the box from the nearest voxel of the map, and which one is it.  Its planar (x, y) form is a bird's-eye-view clearance
 * map.  Replaces the copy of extract() to the host and scipy.ndimage.distance_transform_edt there.  Does not modify the map.  The contract is
 * csrc/accum_field.h, the same code in the kernels and in a g++ build.  No lower-envelope transform, no radius above 128 voxels and no untruncated
 * field, no signed distance, no distance to centroids (gather extract's points by out_nearest), no incremental update, no gradient.
 * Inputs
 *   keys, acc, capacity, m; min_count, use_fraction, max_moving_fraction     the map and extract's filter, as for pcacc_accum_columns
 *   x0, y0, z0, each |.| <= 2^31; nx, ny, nz >= 1: a box of voxels; max_radius R in [1, PCACC_FIELD_MAX_RADIUS] voxels; planar 0 or not
 * Cells: nx ny nz_out with nz_out = planar ? 1 : nz, at most PCACC_FIELD_MAX_CELLS.  Cell (i, j, k) is element (i ny + j) nz_out + k (x slowest, as
 * in the key) and stands for voxel (x0 + i, y0 + j, z0 + k).
 * Sites: the rows of pcacc_accum_extract under the same filter whose voxel index lies inside the box (indices are subtracted in int64; a cell outside
 * [-2^20, 2^20) never holds a site and no key is formed for it).  Row numbers are extract's: they ascend in key order.
 * Result, planar = 0: for a cell c the lexicographic minimum over the sites s of (|c - s|^2, row(s)), |.|^2 the integer squared Euclidean distance of
 * the indices.  If that d2 <= R^2: out_dist2[c] = d2, out_nearest[c] = row (i32 both), otherwise both are -1.  dist2 is exact wherever something
 * lies within R voxels, and ties go to the lowest row, always.
 * Result, planar = 1: the same in (x, y) only, d2 = dx^2 + dy^2; a site is any kept voxel of the box whatever its z inside [z0, z0 + nz), and the
 * row reported for a column is the lowest row among the sites at the minimum: rows ascend in z within a column, so the lowest such voxel of the
 * nearest column.  One plane is written.
 * counters [PCACC_FIELD_COUNTERS] i64 (written, not added to): kept rows, sites, cells with a result, cells without one; the last two sum to the
 * cells whenever m > 0.  m = 0 writes -1 to every cell and zero counters.  Every cell is written once.
 * pcacc_accum_field_lookup: n rows, exactly one of points [n,3] f32 (through pose, rows 0-2 of a row-major 4x4 f64 or NULL = identity, by
 * pcacc_accumulate's per-point arithmetic and validity rule at voxel_size) and coords [n,3] i32 (voxel rows, valid iff inside [-2^20, 2^20)),
 * against the box, planar and the two grids dist2, nearest of a field call.  Per row: out_status u8 with PCACC_FIELD_VALID, PCACC_FIELD_INSIDE (the
 * voxel lies in the box; planar: z is ignored for the cell but must lie in [z0, z0 + nz)) and PCACC_FIELD_NEAR (the cell has a result); out_dist2,
 * out_row i32, both -1 unless NEAR.  Every output of every row is written.  counters [PCACC_FIELD_LOOKUP_COUNTERS] i64 (written): rows, valid,
 * inside, near.  One launch, nothing is read back.
 * Return value: PCACC_E_ARG, and nothing is launched, for a NULL table or output of non-zero size, NULL counters or workspace, m outside
 * [0, capacity], a capacity above 2^30, a radius, origin, shape or cell count outside its range, a workspace below
 * pcacc_accum_field_workspace_bytes(m, cells), or an output that shares a byte with a table of the map or with another output; for the lookup: n
 * outside [0, 2^30], a voxel_size that is not positive and finite, both or neither of points and coords, a NULL grid, a box out of range.
 * ---------------------------------------------------------------------------------------------- */
#define PCACC_FIELD_MAX_RADIUS 128
#define PCACC_FIELD_MAX_CELLS ((int64_t)1 << 28)
#define PCACC_FIELD_COUNTERS 4
#define PCACC_FIELD_N_ROWS 0
#define PCACC_FIELD_N_SITES 1
#define PCACC_FIELD_N_NEAR 2
#define PCACC_FIELD_N_FAR 3
#define PCACC_FIELD_VALID 1
#define PCACC_FIELD_INSIDE 2
#define PCACC_FIELD_NEAR 4
#define PCACC_FIELD_LOOKUP_COUNTERS 4
#define PCACC_FIELD_LOOKUP_ROWS 0
#define PCACC_FIELD_LOOKUP_N_VALID 1
#define PCACC_FIELD_LOOKUP_N_INSIDE 2
#define PCACC_FIELD_LOOKUP_N_NEAR 3
int pcacc_accum_field_workspace_bytes(int64_t m, int64_t cells, size_t *bytes /*host*/);
int pcacc_accum_field(const int64_t *keys, const int64_t *acc, int64_t capacity, int64_t m, int64_t min_count, int32_t use_fraction,
                      double max_moving_fraction, int64_t x0, int64_t y0, int64_t z0, int64_t nx, int64_t ny, int64_t nz, int32_t max_radius,
                      int32_t planar, int32_t *out_dist2, int32_t *out_nearest, int64_t *counters, void *workspace, size_t workspace_bytes,
                      void *stream);
int pcacc_accum_field_lookup(const float *points, const int32_t *coords, int64_t n, const double *pose, double voxel_size, int64_t x0, int64_t y0,
                             int64_t z0, int64_t nx, int64_t ny, int64_t nz, int32_t planar, const int32_t *dist2, const int32_t *nearest,
                             uint8_t *out_status, int32_t *out_dist2, int32_t *out_row, int64_t *counters, void *stream);

/* ------------------------------------------------------------------------------------------------
 * A6/A9. 3x3 convolution + bias + ReLU on the bf16 matrix cores -- the nn.Conv2d(3x3, stride 1, padding 1)
 * layers of models/unet.py:15-27 (conv3x3), :45-71 (DownConv), :74-113 (UpConv), :196-199 (conv_final),
 * the STPN backbone models/stpn.py:24-43, and with kt = 3 the Conv3d(3x3x3, padding 1) + ReLU stack of
 * models/stpn.py:13-22 evaluated on [B*T] frames (frame t reads frames t-1, t, t+1 of its own sample).
 *   in   [n_img, h, w, c_in]  bf16 channels-last;  out [n_img, h, w, c_out] bf16
 *   wp   prepared weights, bf16 [kt*9][c_out][c_in] (pcacc_conv3x3_prepare_weights)
 *   bias [c_out] f32 or NULL;  relu != 0 clamps at 0 before the store
 *   frames: images per sample (T) when kt = 3, else 1;  n_img % frames == 0
 *   c_in, c_out multiples of 32.  fp32 accumulation; the result is rounded to bf16 once.
 * prepare_weights: w f32 [c_out][c_in][kt][3][3] (torch layout) -> wp.  transpose != 0 builds the weights
 * of the data gradient instead (bf16 [kt*9][c_in][c_out], taps mirrored): dX = conv(dY, wp_T) with the
 * same entry point and c_in / c_out exchanged.
 * ---------------------------------------------------------------------------------------------- */
int pcacc_conv3x3_prepare_weights(const float *w, int32_t c_out, int32_t c_in, int32_t kt, int32_t transpose,
                                  uint16_t *out, void *stream);
/* Both prepared forms of one weight tensor in one launch (out_fwd = transpose 0, out_bwd = transpose 1 of the entry point above), the fp32
 * weight read through `strides` (host array, in elements: o, i, [t,] y, x -- contiguous or channels-last storage). */
int pcacc_conv3x3_prepare_weights_pair(const float *w, int32_t c_out, int32_t c_in, int32_t kt, const int64_t *strides /*host*/,
                                       uint16_t *out_fwd, uint16_t *out_bwd, void *stream);
int pcacc_conv3x3_bf16(const uint16_t *in, const uint16_t *wp, const float *bias, uint16_t *out, int32_t n_img,
                       int32_t frames, int32_t h, int32_t w, int32_t c_in, int32_t c_out, int32_t kt, int32_t relu,
                       void *stream);
/* Weight gradient of the same layers (c_in, c_out in {32, 64}): dw = [c_out][9][c_in] f32 followed by [c_out] f32 (bias
 * gradient = sum of dy over the images and pixels this launch visits; complete for dt = 0);  dw[co][tap][ci] = sum of
 * dy[n][px][co] * x[n + dt][px + tap offset][ci]; dt in {-1, 0, 1} selects the frame tap of a kt = 3 layer (0 for kt = 1),
 * frames as above.  bf16 MFMA with fp32 accumulation; per-workgroup partials in `workspace`, summed by a second launch. */
/* The deep layers (c_in >= 128 in steps of 64, c_out in steps of 64, kt = 1: the 128..512-channel layers of models/unet.py:45-113 and
 * models/stpn.py:24-43 on 18^2 .. 144^2 images): tiles of 32 consecutive pixels of a strip instead of 8 x 32 image tiles, the strip's
 * input patch resident in LDS per channel slice, weight tiles double buffered.  pcacc_conv3x3_bf16 routes such shapes here itself;
 * pcacc_conv3x3_deep_supported tells whether a shape qualifies (1) or not (0). */
int pcacc_conv3x3_deep_supported(int32_t h, int32_t w, int32_t c_in, int32_t c_out);
int pcacc_conv3x3_deep_bf16(const uint16_t *in, const uint16_t *in_mask, const uint16_t *wp, const float *bias, uint16_t *out, int32_t n_img,
                            int32_t h, int32_t w, int32_t c_in, int32_t c_out, int32_t relu, void *stream);
/* ReLU backward fused into the consumers of the gradient: `in_mask` / `dy_mask` (NULL = none) is the forward OUTPUT of the ReLU layer
 * whose gradient `in` / `dy` is, same shape; elements where it is not > 0 are read as zero (aten::threshold_backward on the fly, no
 * separate pass over the gradient map).  Deep layers only (pcacc_conv3x3_deep_supported / pcacc_conv3x3_wgrad_deep_supported): they
 * are MFMA-bound, the second read is free; PCACC_E_ARG for a mask on any other shape. */
int pcacc_conv3x3_masked_bf16(const uint16_t *in, const uint16_t *in_mask, const uint16_t *wp, const float *bias, uint16_t *out,
                              int32_t n_img, int32_t frames, int32_t h, int32_t w, int32_t c_in, int32_t c_out, int32_t kt,
                              int32_t relu, void *stream);
/* ReLU backward on the OUTPUT side of a data gradient: the convolution's result is stored as zero where out_mask [n_img,h,w,c_out] (the
 * forward input of the layer, itself a ReLU output: models/unet.py:45-71 conv -> ReLU -> conv) is <= 0, so the producing layer needs no
 * threshold pass.  No bias, no ReLU.  The layers the strip kernels would take are not supported (pcacc_conv3x3_outmask_supported = 0). */
int pcacc_conv3x3_outmask_supported(int32_t h, int32_t w, int32_t c_in, int32_t c_out, int32_t kt);
int pcacc_conv3x3_outmask_bf16(const uint16_t *in, const uint16_t *wp, const uint16_t *out_mask, uint16_t *out, int32_t n_img, int32_t frames,
                               int32_t h, int32_t w, int32_t c_in, int32_t c_out, int32_t kt, void *stream);
/* Weight gradient of the same deep layers (c_in, c_out multiples of 64, at least one of them > 64; kt = 1): dw [c_out][9][c_in] f32 and
 * db [c_out] f32 = bias gradient, from dy [n_img,h,w,c_out] and x [n_img,h,w,c_in] (bf16, channels-last).  64 x 64 blocks of the weight
 * tensor per workgroup, strips of consecutive pixels, per-workgroup partial slots in the workspace + a reduce launch. */
int pcacc_conv3x3_wgrad_deep_supported(int32_t h, int32_t w, int32_t c_in, int32_t c_out);
int pcacc_conv3x3_wgrad_deep_workspace_bytes(int32_t n_img, int32_t h, int32_t w, int32_t c_in, int32_t c_out, size_t *bytes /*host*/);
int pcacc_conv3x3_wgrad_deep_bf16(const uint16_t *dy, const uint16_t *dy_mask, const uint16_t *x, float *dw, float *db, int32_t n_img,
                                  int32_t h, int32_t w, int32_t c_in, int32_t c_out, void *workspace, size_t workspace_bytes, void *stream);
/* ------------------------------------------------------------------------------------------------
 * A6/A9 at fp32 accuracy ("fp32x3" compute mode): the same layers -- fp32 convolutions in the reference, models/unet.py:11-20,45-113,
 * models/stpn.py:13-43 -- on fp32 channels-last maps, every product formed on the 16-bit matrix cores from fp16 hi / lo halves of
 * power-of-two scaled operands (w_hi x_lo + w_lo x_hi + w_hi x_hi, fp32 accumulation; 22 significant bits per factor, relative error
 * ~3e-7 per product).  One kernel family for all layers (c_in, c_out multiples of 32; kt = 1 or 3): tiles of rows x band-width pixels,
 * hi / lo planes of the patch and of the per-tap weight tiles in LDS (csrc/conv_split.hip).
 *   absmax256: parts[256] f32 <- partial maxima of |x| over n f32 elements (x 16-byte aligned; a NaN gives +inf).  Every consumer below
 *       takes such an array for each fp32 tensor it splits and derives the tensor's scale from it (no host round trip).
 *   prepare_weights: w f32 [c_out][c_in][kt][3][3] read through `strides` (host, elements: o, i, [t,] y, x) ->
 *       out_fwd fp16 [2 = hi, lo][kt*9][c_out][c_in] + scale_fwd f32 [c_out]; out_bwd fp16 [2][kt*9][c_in][c_out] (taps mirrored:
 *       data gradient) + scale_bwd f32 [c_in]; scale = 1 / (power-of-two scale of that output-channel row)
 *   split:  in [n_img,h,w,c_in] f32 (+ in_amax) -> out [n_img,h,w,c_out] f32; in_mask (NULL = none): same shape as `in`, elements of `in`
 *       are read as zero where in_mask <= 0 (ReLU backward of the layer whose gradient `in` is, fused into the staging); wp / wscale from
 *       prepare_weights; bias / relu / frames / kt as pcacc_conv3x3_bf16; out_amax (NULL = not wanted): 256 f32 slots, ZEROED by the caller,
 *       receive partial maxima of |out| -- an absmax256 array of the result for the kernel that consumes it
 *   wgrad_split: dw [c_out][9][c_in] f32, db [c_out] f32 (NULL = not wanted; complete for dt = 0) from dy [n_img,h,w,c_out] f32
 *       (dy_mask as in_mask) and x [n_img,h,w,c_in] f32 with their absmax256 arrays; dt / frames as pcacc_conv3x3_wgrad_bf16
 * ---------------------------------------------------------------------------------------------- */
int pcacc_absmax256(const float *x, int64_t n, float *parts, void *stream);
int pcacc_conv3x3_split_prepare_weights(const float *w, int32_t c_out, int32_t c_in, int32_t kt, const int64_t *strides /*host*/,
                                        uint16_t *out_fwd, float *scale_fwd, uint16_t *out_bwd, float *scale_bwd, void *stream);
int pcacc_conv3x3_split_supported(int32_t h, int32_t w, int32_t c_in, int32_t c_out);
int pcacc_conv3x3_split(const float *in, const float *in_amax, const float *in_mask, const uint16_t *wp, const float *wscale,
                        const float *bias, float *out, float *out_amax, int32_t n_img, int32_t frames, int32_t h, int32_t w, int32_t c_in,
                        int32_t c_out, int32_t kt, int32_t relu, void *stream);
/* pcacc_conv3x3_split with a second result, out16 [n_img,h,w,c_out] bf16 = the fp32 result rounded to nearest even, written by the same epilogue
 * ('mixed' compute mode: fp32x3 forward values, bf16 gradient graph -- the shadow the bf16 data / weight gradient kernels read; 2 extra bytes per
 * element stored instead of a 6-byte cast pass).  models/unet.py:11-20,45-113, models/stpn.py:13-43. */
int pcacc_conv3x3_split_dual(const float *in, const float *in_amax, const float *in_mask, const uint16_t *wp, const float *wscale,
                             const float *bias, float *out, float *out_amax, uint16_t *out16, int32_t n_img, int32_t frames, int32_t h,
                             int32_t w, int32_t c_in, int32_t c_out, int32_t kt, int32_t relu, void *stream);

/* The same convolution (no bias, no ReLU; in_mask as above) with its result stored as zero where out_mask [n_img,h,w,c_out] f32 is <= 0: the
 * data gradient of conv -> ReLU -> conv masked for the first ReLU in the epilogue (the fp32x3 twin of pcacc_conv3x3_outmask_bf16). */
/* pcacc_conv3x3_split_dual (kt = 1, no input mask) on the channel concatenation of TWO inputs read in place: in_a [n_img][h][w][c_a], in_b
 * [n_img][h][w][c_in - c_a] -- conv1(cat(upconv(x), skip)) of a decoder stage (models/unet.py:101-113) without writing the fp32 concatenation.
 * in_amax bounds both inputs (element-wise maximum of their pcacc_absmax256 arrays); out16 may be NULL; c_a and c_in - c_a multiples of 32. */
int pcacc_conv3x3_split_cat(const float *in_a, const float *in_b, int32_t c_a, const float *in_amax, const uint16_t *wp, const float *wscale,
                            const float *bias, float *out, float *out_amax, uint16_t *out16, int32_t n_img, int32_t h, int32_t w, int32_t c_in,
                            int32_t c_out, int32_t relu, void *stream);
int pcacc_conv3x3_split_outmask(const float *in, const float *in_amax, const float *in_mask, const uint16_t *wp, const float *wscale,
                                const float *out_mask, float *out, float *out_amax, int32_t n_img, int32_t frames, int32_t h, int32_t w,
                                int32_t c_in, int32_t c_out, int32_t kt, void *stream);
int pcacc_conv3x3_wgrad_split_workspace_bytes(int32_t n_img, int32_t h, int32_t w, int32_t c_in, int32_t c_out, size_t *bytes /*host*/);
int pcacc_conv3x3_wgrad_split(const float *dy, const float *dy_amax, const float *dy_mask, const float *x, const float *x_amax, float *dw,
                              float *db, int32_t n_img, int32_t frames, int32_t dt, int32_t h, int32_t w, int32_t c_in, int32_t c_out,
                              void *workspace, size_t workspace_bytes, void *stream);
/* nn.ConvTranspose2d(kernel 2, stride 2) of the two decoders (models/unet.py:22-30,101-113) in the fp32x3 mode: a 1-tap product on the
 * tiles of pcacc_conv3x3_split whose epilogue scatters a pixel's 4 c_up results to its 2 x 2 output pixels (direction 0), its data
 * gradient reading dy space-to-depth (direction 1), and the weight gradient on pcacc_conv3x3_wgrad_split's kernel.  c_in, c_up
 * multiples of 32; h, w = the small map's size.
 *   prepare_weights: w f32 [c_in][c_up][2][2] through `strides` (host, elements: i, o, y, x) -> out_fwd fp16 [2][4 c_up][c_in] (rows
 *       (a, b, co)) + scale_fwd [4 c_up], out_bwd fp16 [2][c_in][4 c_up] + scale_bwd [c_in]
 *   upconv2x2_split: direction 0: in [n,h,w,c_in] -> out [n,2h,2w,c_up] (+ bias [c_up]); direction 1: in = dy [n,2h,2w,c_up] -> out
 *       [n,h,w,c_in]; in_amax / out_amax as pcacc_conv3x3_split
 *   wgrad: dw [4 c_up][c_in] f32 (row (a, b, co)), db4 [4 c_up] f32 (sums of dy per (a, b, co); the bias gradient is the sum of the four groups) */
int pcacc_upconv2x2_split_prepare_weights(const float *w, int32_t c_in, int32_t c_up, const int64_t *strides /*host*/, uint16_t *out_fwd,
                                          float *scale_fwd, uint16_t *out_bwd, float *scale_bwd, void *stream);
int pcacc_upconv2x2_split_supported(int32_t h, int32_t w, int32_t c_in, int32_t c_up);

/* The same layer (nn.ConvTranspose2d(kernel 2, stride 2), models/unet.py:22-30,101-113) on bf16 channels-last rows -- the bf16 compute mode's forward
 * and backward, the 'mixed' mode's backward -- on the bf16 matrix cores, fp32 accumulation.  c_in a multiple of 64, c_up a multiple of 32.
 *   prepare_weights: w f32 [c_in][c_up][2][2] through `strides` (host, elements: i, o, y, x) -> out_fwd bf16 [4 c_up][c_in] (rows (a, b, co)),
 *       out_bwd bf16 [c_in][4 c_up]
 *   upconv2x2_bf16: direction 0: in [n,h,w,c_in] (pixel pitch in_pitch >= c_in elements), wp = out_fwd -> out [n,2h,2w,c_up] (pixel pitch out_pitch),
 *       + bias[c_up] (f32, may be NULL); direction 1: in = dy [n,2h,2w,c_up] (pixel pitch in_pitch: dy may be a channel slice of a wider map),
 *       wp = out_bwd -> out [n,h,w,c_in] (pixel pitch out_pitch).  Pitches are multiples of 8 elements, pointers 16-byte aligned.
 *   wgrad: dy as above, x [n,h,w,c_in] (pitch x_pitch) -> dw f32 [c_in][c_up][2][2] written through `dw_strides` (host, elements: i, o, y, x -- the
 *       layout of the weight the gradient belongs to; NULL = contiguous), db f32 [c_up] (may be NULL); workspace from
 *       pcacc_upconv2x2_bf16_wgrad_workspace_bytes. */
int pcacc_upconv2x2_bf16_supported(int32_t c_in, int32_t c_up);
int pcacc_upconv2x2_bf16_prepare_weights(const float *w, int32_t c_in, int32_t c_up, const int64_t *strides /*host*/, uint16_t *out_fwd,
                                         uint16_t *out_bwd, void *stream);
int pcacc_upconv2x2_bf16(const uint16_t *in, const uint16_t *wp, const float *bias, uint16_t *out, int32_t n_img, int32_t h, int32_t w,
                         int32_t c_in, int32_t c_up, int32_t direction, int32_t in_pitch, int32_t out_pitch, void *stream);
int pcacc_upconv2x2_bf16_wgrad_workspace_bytes(int32_t n_img, int32_t h, int32_t w, int32_t c_in, int32_t c_up, size_t *bytes);
int pcacc_upconv2x2_bf16_wgrad(const uint16_t *dy, int32_t dy_pitch, const uint16_t *x, int32_t x_pitch, float *dw, const int64_t *dw_strides /*host*/,
                               float *db, int32_t n_img, int32_t h, int32_t w, int32_t c_in, int32_t c_up, void *workspace, size_t workspace_bytes,
                               void *stream);

/* Every prepared form of every weight of a model in ONE launch (a training step re-prepares ~90 forms right after the optimizer wrote the
 * parameters -- the per-layer weight handling of the reference's nn.Conv2d / nn.Conv3d / nn.ConvTranspose2d, models/unet.py:22-113,
 * models/stpn.py:39-70).  `jobs` = DEVICE table, 16 int64 per job:
 *   [0] w (f32, device)  [1] out_fwd  [2] scale_fwd  [3] out_bwd  [4] scale_bwd  [5..9] strides of w in elements
 *   [10] a  [11] b  [12] kt  [13] kind  [14] first workgroup of the job (ascending, job 0 starts at 0)  [15] workgroups of the job
 * kind 0 = pcacc_conv3x3_split_prepare_weights   (a = c_out, b = c_in; strides o, i, t, y, x; a + b workgroups)
 * kind 1 = pcacc_upconv2x2_split_prepare_weights (a = c_in, b = c_up; strides i, o, -, y, x; 4 b + a workgroups)
 * kind 2 = pcacc_conv3x3_prepare_weights_pair    (a = c_out, b = c_in; strides o, i, t, y, x; any number of workgroups >= 1; no scales)
 * kind 3 = pcacc_upconv2x2_bf16_prepare_weights  (a = c_in, b = c_up; strides i, o, -, y, x; any number of workgroups >= 1; no scales)
 * with the outputs of those entry points; total_blocks = [14] + [15] of the last job. */
int pcacc_prepare_weights_batch(const int64_t *jobs, int32_t n_jobs, int32_t total_blocks, void *stream);
int pcacc_upconv2x2_split(const float *in, const float *in_amax, const uint16_t *wp, const float *wscale, const float *bias, float *out,
                          float *out_amax, int32_t n_img, int32_t h, int32_t w, int32_t c_in, int32_t c_up, int32_t direction, void *stream);
/* pcacc_upconv2x2_split (direction 0) with the bf16 shadow of its result as a second output ('mixed' mode, see pcacc_conv3x3_split_dual).
 * out_pitch: elements between consecutive pixels of out and out16 (0 = c_up, dense; 2 c_up: both results are the first half of the decoder's
 * concatenation buffers [n,2h,2w,2 c_up], models/unet.py:101-113 -- the up-sampled half is never copied). */
int pcacc_upconv2x2_split_dual(const float *in, const float *in_amax, const uint16_t *wp, const float *wscale, const float *bias, float *out,
                               float *out_amax, uint16_t *out16, int32_t n_img, int32_t h, int32_t w, int32_t c_in, int32_t c_up,
                               int32_t out_pitch, void *stream);
int pcacc_upconv2x2_wgrad_split_workspace_bytes(int32_t n_img, int32_t h, int32_t w, int32_t c_in, int32_t c_up, size_t *bytes /*host*/);
int pcacc_upconv2x2_wgrad_split(const float *dy, const float *dy_amax, const float *x, const float *x_amax, float *dw, float *db4, int32_t n_img,
                                int32_t h, int32_t w, int32_t c_in, int32_t c_up, void *workspace, size_t workspace_bytes, void *stream);
/* The last convolution of a SegHead2D -- models/unet.py:259-277: Conv2d(mid, 2, 3, padding 1), the fg / bg logits -- c_in = 32 or 64,
 * c_out <= 4: exact fp32 arithmetic on f32 (dtype 0) or bf16 (1) channels-last rows, streamed (csrc/head_conv.hip; matrix-core tiles
 * would be 94 % padding).  w f32 [c_out][c_in][3][3] read through `w_strides` (host, elements: o, i, y, x).
 *   forward: y [n,h,w,c_out] f32 = conv(x) + bias;  dgrad: dx [n,h,w,c_in] (f32 / bf16) from dy [n,h,w,c_out] f32;
 *   wgrad: dw [c_out][c_in][3][3] f32 contiguous, db [c_out] f32 or NULL; per-workgroup partials in `workspace`, summed in a fixed order. */
int pcacc_head_conv3x3_supported(int32_t c_in, int32_t c_out);
int pcacc_head_conv3x3_forward(const void *x, int32_t x_dtype, const float *w, const int64_t *w_strides /*host*/, const float *bias, float *y,
                               int32_t n_img, int32_t h, int32_t wd, int32_t c_in, int32_t c_out, void *stream);
int pcacc_head_conv3x3_dgrad(const float *dy, const float *w, const int64_t *w_strides /*host*/, void *dx, int32_t dx_dtype, int32_t n_img,
                             int32_t h, int32_t wd, int32_t c_in, int32_t c_out, void *stream);
int pcacc_head_conv3x3_wgrad_workspace_bytes(int32_t n_img, int32_t h, int32_t wd, int32_t c_in, int32_t c_out, size_t *bytes /*host*/);
int pcacc_head_conv3x3_wgrad(const float *dy, const void *x, int32_t x_dtype, float *dw, float *db, int32_t n_img, int32_t h, int32_t wd,
                             int32_t c_in, int32_t c_out, void *workspace, size_t workspace_bytes, void *stream);
/* The per-point linear layers in the fp32x3 mode (csrc/mlp_split.hip): the contracts of pcacc_rows_linear_bf16 / _cat_bf16 /
 * pcacc_rows_wgrad_bf16 / _cat_bf16 above on fp32 rows (x, masks, residual, y all f32; k, n in {32, 64, 128}), products from scaled
 * fp16 hi / lo halves as in pcacc_conv3x3_split; every fp32 row tensor that is split comes with its pcacc_absmax256 array
 * (x_amax; two-piece rows: one per piece; dy_amax), the weight matrix is scaled per output row inside the kernel; y_amax (NULL = not
 * wanted; 256 f32 slots zeroed by the caller) receives partial maxima of |y| (of y and y2 together), as out_amax above.  nn.Linear of
 * models/pillar_encoder.py:13-55,113-122, models/stpn.py:94-102, models/tpointnet.py:176-196 (fp32 in the reference). */
int pcacc_rows_linear_split(const float *x, const float *x_amax, const float *in_mask, const float *w, const float *bias,
                            const float *residual, const float *out_mask, float *y, float *y_amax, int64_t rows, int32_t k, int32_t n,
                            int32_t flags, void *stream);
/* 'mixed' compute mode: pcacc_rows_linear_split with y16 [rows,n] = bf16(y) as a second output of the same epilogue (see pcacc_conv3x3_split_dual). */
int pcacc_rows_linear_split_dual(const float *x, const float *x_amax, const float *in_mask, const float *w, const float *bias,
                                 const float *residual, const float *out_mask, float *y, uint16_t *y16, float *y_amax, int64_t rows, int32_t k,
                                 int32_t n, int32_t flags, void *stream);
int pcacc_rows_linear_cat_split(const float *xa, const float *xa_amax, const float *xb, const float *xb_amax, const int32_t *b_index,
                                int32_t ka, const float *in_mask, const float *w, const float *bias, const float *residual,
                                const float *out_mask_a, const float *out_mask_b, float *y, float *y2, int32_t na, float *y_amax, int64_t rows,
                                int32_t k, int32_t n, int32_t flags, void *stream);
int pcacc_rows_wgrad_split_workspace_bytes(int64_t rows, int32_t k, int32_t n, size_t *bytes /*host*/);
int pcacc_rows_wgrad_split(const float *dy, const float *dy_amax, const float *dy_mask, const float *x, const float *x_amax, int32_t x_relu,
                           int64_t rows, int32_t k, int32_t n, float *dw_aug, void *workspace, size_t workspace_bytes, void *stream);
int pcacc_rows_wgrad_cat_split(const float *dy, const float *dy_amax, const float *dy_mask, const float *xa, const float *xa_amax,
                               const float *xb, const float *xb_amax, const int32_t *b_index, int32_t ka, int32_t x_relu, int64_t rows,
                               int32_t k, int32_t n, float *dw_aug, void *workspace, size_t workspace_bytes, void *stream);
int pcacc_conv3x3_wgrad_workspace_bytes(int32_t n_img, int32_t h, int32_t w, int32_t c_in, int32_t c_out, size_t *bytes /*host*/);
int pcacc_conv3x3_wgrad_bf16(const uint16_t *dy, const uint16_t *x, float *dw, int32_t n_img, int32_t frames, int32_t dt,
                             int32_t h, int32_t w, int32_t c_in, int32_t c_out, void *workspace, size_t workspace_bytes,
                             void *stream);

/* ------------------------------------------------------------------------------------------------
 * D1. Data step in front of the path -- libs/dataset.py:147-182 (BaseDataset.prep_input before the voxeliser),
 * :93-104 (apply_data_augmentation), toolbox/register_utils.py:199-206 (apply_tsfm).  One pass over the raw points:
 *   points [m,3] f64;  tsfm12 [12] f64 on the device = 3x3 rotation (row-major) then translation, or NULL;
 *   noise [m,3] f64 uniform(0,1) draws or NULL (added as (u - 0.5) * noise_scale);  scale: global factor applied when
 *   tsfm12 or noise is given;  crop_xy, z_min, z_max: crop box;  remove_ground / ground_z: keep only z > ground_z;
 *   out_points [m,3] f64: augmented points;  keep [m] u8: 1 where the point passes crop (and ground) tests.
 * The kept rows are compacted by the caller (stable order); libs/dataset.py:166-181.
 * ---------------------------------------------------------------------------------------------- */
int pcacc_prep_points(const double *points, const double *tsfm12, const double *noise, double noise_scale, double scale,
                      double crop_xy, double z_min, double z_max, int32_t remove_ground, double ground_z, int64_t m,
                      double *out_points, uint8_t *keep, void *stream);

/* ------------------------------------------------------------------------------------------------
 * L1. Two-class segmentation loss on selected rows -- libs/loss.py:110-137 (FuseLoss.get_seg_loss: weighted cross entropy
 * with the class weights of :90-108, Lovasz-Softmax of libs/lovasz_softmax.py:56-94, IoU counters of compute_iou :17-50),
 * as called on the occupied pillars (:167-191) and on the foreground points (:140-165).
 *   logits: f32 or bf16 (PCACC_F32 | PCACC_BF16), row i at [i][2] (plane = 0) or as planes [i / plane][2][i % plane]
 *           (an NCHW head output read in place, plane = H*W);  labels [n_total] i64 (0, 1, or -1 = ignored by the cross
 *           entropy and background of both classes in the Lovasz term, as in the reference);  rows [n] i64 = the selected
 *           rows (NULL: rows 0..n-1)
 *   out_loss [2] f32 = (cross entropy, Lovasz);  out_metric [4][2] f64 = intersection, union, predicted, labelled per
 *   class, each / 1e3;  lovasz_grad [2][n] f32 and saved [8] f32 are what backward needs (the Jaccard gradient of each
 *   row's rank per class; the class weights, their sum over the rows and the share of each present class)
 *   backward: grad_bce, grad_lovasz = device scalars (NULL = 0);  grad_logits has the layout and type of logits over all
 *   n_total rows (rows outside the selection get 0).  Equal errors are ranked by row index.
 * ---------------------------------------------------------------------------------------------- */
int pcacc_seg_loss_workspace_bytes(int64_t n, size_t *bytes /*host*/);
int pcacc_seg_loss_forward(const void *logits, int logits_dtype, int64_t plane, const int64_t *labels, const int64_t *rows,
                           int64_t n, float *out_loss, double *out_metric, float *lovasz_grad, float *saved,
                           void *workspace, size_t workspace_bytes, void *stream);
int pcacc_seg_loss_backward(const void *logits, int logits_dtype, int64_t plane, const int64_t *labels, const int64_t *rows,
                            int64_t n, int64_t n_total, const float *lovasz_grad, const float *saved, const float *grad_bce,
                            const float *grad_lovasz, void *grad_logits, void *stream);

/* ------------------------------------------------------------------------------------------------
 * L2. Offset loss -- libs/loss.py:194-250 (FuseLoss.get_offset_loss): every point is reconstructed with the ground truth
 * (toolbox/register_utils.py:59-93: ego pose of its frame, then the motion of its instance), the instance centres are the
 * means of the reconstructed points per instance, and the selected (foreground) rows compare the offset to their centre
 * with the estimate.
 *   points [n,3] f32;  time_indice [n,2] i64 (sample, frame);  inst_labels [n] i64 (per sample);  label_base [B] i64 =
 *   first row of each sample in inst_motion;  ego_motion [B,T,16] f32;  inst_motion [k,T,16] f32 (all samples
 *   concatenated);  transformed_points [n,3] f32;  offset_est [n,2] f32;  rows [m] i64 (NULL: all rows)
 *   out [3] f32 = (L1 term, direction term, mean L2 error);  offset_gt [m,2] f32 = predictions['offset_gt'] (:246)
 *   backward: grad_norm / grad_dir = device scalars (NULL = 0);  grad_est [n,2] f32 (0 outside the selection).
 * ---------------------------------------------------------------------------------------------- */
int pcacc_offset_loss_workspace_bytes(int64_t m, int64_t k, size_t *bytes /*host*/);
int pcacc_offset_loss_forward(const float *points, const int64_t *time_indice, const int64_t *inst_labels,
                              const int64_t *label_base, const float *ego_motion, const float *inst_motion, int32_t n_frames,
                              int64_t n, int64_t k, const float *transformed_points, const float *offset_est,
                              const int64_t *rows, int64_t m, float *out, float *offset_gt, void *workspace,
                              size_t workspace_bytes, void *stream);
int pcacc_offset_loss_backward(const float *offset_gt, const float *offset_est, const int64_t *rows, int64_t m, int64_t n,
                               const float *grad_norm, const float *grad_dir, float *grad_est, void *stream);

/* A9. Max over the frames of a map stack -- models/stpn.py:83 (`torch.max(x, dim=2)` between the temporal convolutions and the
 * U-Net): x [n_seq, frames, plane] f32 or bf16 (plane = H*W*C contiguous elements, a multiple of 4 / 8), out [n_seq, plane],
 * arg [n_seq, plane] u8 = the winning frame (lowest on ties; a NaN wins).  backward: grad_x[s,t,p] = arg[s,p] == t ? grad_out[s,p] : 0,
 * every element written. */
int pcacc_frames_max(const void *x, int dtype, int64_t n_seq, int32_t frames, int64_t plane, void *out, uint8_t *arg, void *stream);
int pcacc_frames_max_backward(const void *grad_out, const uint8_t *arg, int dtype, int64_t n_seq, int32_t frames, int64_t plane,
                              void *grad_x, void *stream);

/* A10 point heads: nn.BatchNorm1d in training mode over [rows, c] rows -- models/unet.py:240-245 (SegHead1D: Linear, BatchNorm1d,
 * ReLU, Linear on the K foreground points; batch statistics over the rows).  x, y: f32 or bf16 (PCACC_F32 | PCACC_BF16), c a
 * multiple of 4 / 8 with 256 % (c / 4 | 8) == 0, c <= 256;  gamma, beta [c] f32 or NULL;  running_mean / running_var [c] f32
 * updated in place when given (momentum; unbiased variance, as torch);  save_mean, save_invstd [c] f32 out (for backward).
 * backward: grad_x in the type of x, grad_gamma / grad_beta [c] f32. */
int pcacc_bn_rows_workspace_bytes(int64_t rows, int32_t c, size_t *bytes /*host*/);
int pcacc_bn_rows_forward(const void *x, int dtype, int64_t rows, int32_t c, const float *gamma, const float *beta, float eps,
                          float momentum, float *running_mean, float *running_var, void *y, float *save_mean,
                          float *save_invstd, void *workspace, size_t workspace_bytes, void *stream);
int pcacc_bn_rows_backward(const void *grad_y, const void *x, int dtype, int64_t rows, int32_t c, const float *gamma,
                           const float *save_mean, const float *save_invstd, void *grad_x, float *grad_gamma, float *grad_beta,
                           void *workspace, size_t workspace_bytes, void *stream);

/* BatchNorm + ReLU in the same passes (SegHead2D, models/unet.py:264-268: conv, BatchNorm2d, ReLU, conv): y = max(bn(x), 0); the backward
 * takes grad_y only where that output was > 0 -- recomputed from x, the saved statistics, gamma and beta (NULL = 1 / 0), no mask tensor. */
int pcacc_bn_relu_rows_forward(const void *x, int dtype, int64_t rows, int32_t c, const float *gamma, const float *beta, float eps,
                               float momentum, float *running_mean, float *running_var, void *y, float *save_mean, float *save_invstd,
                               void *workspace, size_t workspace_bytes, void *stream);
int pcacc_bn_relu_rows_backward(const void *grad_y, const void *x, int dtype, int64_t rows, int32_t c, const float *gamma, const float *beta,
                                const float *save_mean, const float *save_invstd, void *grad_x, float *grad_gamma, float *grad_beta,
                                void *workspace, size_t workspace_bytes, void *stream);
/* pcacc_bn_rows_forward / pcacc_bn_relu_rows_forward (relu != 0) on f32 rows with two more outputs from the same store phase ('mixed' compute mode):
 * y16 = y as bf16 [rows][c], y_amax = 256 partial absolute maxima of y (zero-filled by the caller; layout of pcacc_absmax256); either may be NULL */
int pcacc_bn_rows_forward_dual(const float *x, int64_t rows, int32_t c, const float *gamma, const float *beta, float eps, float momentum,
                               float *running_mean, float *running_var, int32_t relu, float *y, uint16_t *y16, float *y_amax, float *save_mean,
                               float *save_invstd, void *workspace, size_t workspace_bytes, void *stream);

/* the two backward entries above (relu != 0: pcacc_bn_relu_rows_backward with its `beta`) with a second output from the same store phase:
 * grad_x_amax = 256 partial absolute maxima of grad_x (zero-filled by the caller; layout of pcacc_absmax256) -- the fp32x3 layer in front of
 * the normalisation scales its incoming gradient by them */
int pcacc_bn_rows_backward_m(const void *grad_y, const void *x, int dtype, int64_t rows, int32_t c, const float *gamma, const float *beta,
                             int32_t relu, const float *save_mean, const float *save_invstd, void *grad_x, float *grad_x_amax, float *grad_gamma,
                             float *grad_beta, void *workspace, size_t workspace_bytes, void *stream);

/* A ResnetBlockFC of the pillar encoder -- models/pillar_encoder.py:13-55 with size_in 64, size_h 32, size_out 32 and the linear
 * shortcut (the blocks of PillarFeatureNet, :76-78) -- fused over bf16 point rows:
 *     h = relu(x) w0^T + b0,   out = relu(h) w1^T + b1 + x ws^T          w0, ws [32,64], w1 [32,32], b0, b1 [32] f32
 * x [rows,64] = `xa` when pooled == NULL, else cat(xa[row] [32], pooled[p2v[row]] [32]) (models/pillar_encoder.py:116-118).
 * forward: out [rows,32], relu_h [rows,32] (kept for the backward; may be NULL).
 * backward: grad_xa [rows,64] (pooled == NULL) or grad_xa [rows,32] + grad_xb [rows,32] (per point: the caller sums it over each
 * pillar's points); grad_params [5184] f32 = d w1 [32,32] | d b1 [32] | d ws [32,64] | d w0 [32,64] | d b0 [32].
 * bf16 values: relu_h = bf16(relu(h)) is what the second product reads (and what the backward gets); out is rounded once; the backward holds
 * d(h) = (grad_out w1) where relu_h > 0 as bf16 between its two products and in d w0 / d b0; grad_xa / grad_xb are rounded once; the weights
 * are rounded to bf16 once per launch; grad_params is fp32.  "> 0" as in the mask rule of the row layers above (NaN counts as not > 0). */
int pcacc_pfn_block_forward(const uint16_t *xa, const uint16_t *pooled, const int32_t *p2v, const float *w0, const float *b0,
                            const float *ws, const float *w1, const float *b1, uint16_t *out, uint16_t *relu_h, int64_t rows, void *stream);
int pcacc_pfn_block_backward_workspace_bytes(int64_t rows, size_t *bytes /*host*/);
int pcacc_pfn_block_backward(const uint16_t *xa, const uint16_t *pooled, const int32_t *p2v, const uint16_t *relu_h,
                             const uint16_t *grad_out, const float *w0, const float *ws, const float *w1, uint16_t *grad_xa,
                             uint16_t *grad_xb, float *grad_params, int64_t rows, void *workspace, size_t workspace_bytes, void *stream);

/* The same block on fp32 point rows at fp32 accuracy (compute mode fp32x3: products on the matrix cores from scaled fp16 hi / lo
 * halves, csrc/pfn_block_split.hip).  *_amax arguments are pcacc_absmax256 arrays of the tensor they follow (inputs), or 256 zeroed
 * slots the kernel's store phase fills (outputs; may be NULL).
 * forward: out, relu_h [rows,32] f32; xmask [rows] u64 / hmask [rows] u32: bit c set where x[row][c] > 0 / h[row][c] > 0 -- all the
 * data-gradient kernel needs of x and h.
 * dgrad: grad_xa [rows,64] (grad_xb == NULL) or grad_xa [rows,32] + grad_xb [rows,32]; grad_h [rows,32] = d(h), the operand of fc_0's
 * weight gradient.  The three weight gradients are pcacc_rows_wgrad_split / _cat_split calls on (grad_out, relu_h), (grad_out, x)
 * and (grad_h, relu(x)). */
int pcacc_pfn_block_split_forward(const float *xa, const float *xa_amax, const float *pooled, const float *pooled_amax, const int32_t *p2v,
                                  const float *w0, const float *b0, const float *ws, const float *w1, const float *b1, float *out,
                                  float *relu_h, uint64_t *xmask, uint32_t *hmask, float *out_amax, float *hr_amax, int64_t rows,
                                  void *stream);
/* 'mixed' compute mode: pcacc_pfn_block_split_forward's fp32 result plus the two operands of the bf16 backward kernel pcacc_pfn_block_backward,
 * written by the same epilogue: out16 = bf16(out), hr16 = bf16(relu(h)) [rows,32]; no fp32 relu(h), no sign masks.  models/pillar_encoder.py:13-55. */
int pcacc_pfn_block_split_forward_dual(const float *xa, const float *xa_amax, const float *pooled, const float *pooled_amax, const int32_t *p2v,
                                       const float *w0, const float *b0, const float *ws, const float *w1, const float *b1, float *out,
                                       uint16_t *out16, uint16_t *hr16, float *out_amax, int64_t rows, void *stream);
int pcacc_pfn_block_split_dgrad(const float *grad_out, const float *grad_out_amax, const uint64_t *xmask, const uint32_t *hmask,
                                const float *w0, const float *ws, const float *w1, float *grad_xa, float *grad_xb, float *grad_h,
                                float *gx_amax, float *dh_amax, int64_t rows, void *stream);

/* Tail of a U-Net encoder stage -- models/unet.py:60-71 (DownConv: ... conv, ReLU, 2x2 max-pool; returns the pooled map and the map
 * before the pool).  Channels-last bf16 maps [n_img, h, w, c], c a multiple of 8.
 *  maxpool2x2                out [n_img, h/2, w/2, c]: nn.MaxPool2d(2, 2) (floor mode; NaN propagates), no index map.
 *  pool_skip_relu_backward   grad_y = (un-pool(grad_pooled) + grad_skip) where y > 0, else 0: the gradient of the stage's ReLU input
 *                            from the gradients of its two consumers in one pass (the window's first maximum in scan order takes
 *                            the pooled gradient, as the library's forward picks it); either gradient may be NULL (= 0). */
int pcacc_maxpool2x2_bf16(const uint16_t *x, int64_t n_img, int32_t h, int32_t w, int32_t c, uint16_t *out, void *stream);
int pcacc_pool_skip_relu_backward_bf16(const uint16_t *y, const uint16_t *grad_pooled, const uint16_t *grad_skip, int64_t n_img, int32_t h,
                                       int32_t w, int32_t c, uint16_t *grad_y, void *stream);
/* The same two passes on fp32 rows (c % 4 == 0; compute mode fp32x3).  out_amax: 256 zeroed f32 slots receiving the largest magnitude of
 * grad_y (pcacc_absmax256 layout) for the split kernels that read it, or NULL. */
int pcacc_maxpool2x2_f32(const float *x, int64_t n_img, int32_t h, int32_t w, int32_t c, float *out, void *stream);
int pcacc_pool_skip_relu_backward_f32(const float *y, const float *grad_pooled, const float *grad_skip, int64_t n_img, int32_t h, int32_t w,
                                      int32_t c, float *grad_y, float *out_amax, void *stream);
/* grad_skip read in place from a wider map (skip_pitch = elements between consecutive pixels, >= c, a multiple of 8 (bf16) / 4 (f32), the
 * pointer 16-byte aligned): the skip half of the decoder's concatenation gradient (models/unet.py:101-113) without a contiguous copy. */
int pcacc_pool_skip_relu_backward_strided_bf16(const uint16_t *y, const uint16_t *grad_pooled, const uint16_t *grad_skip, int64_t skip_pitch,
                                               int64_t n_img, int32_t h, int32_t w, int32_t c, uint16_t *grad_y, void *stream);
int pcacc_pool_skip_relu_backward_strided_f32(const float *y, const float *grad_pooled, const float *grad_skip, int64_t skip_pitch,
                                              int64_t n_img, int32_t h, int32_t w, int32_t c, float *grad_y, float *out_amax, void *stream);
/* 'mixed' compute mode: y f32 (the forward's own values decide the window's winner -- a bf16 copy of y ties values closer than 2^-8 and sends
 * ~1 % of the windows' gradient to the wrong pixel), gradients and result bf16; c a multiple of 8. */
int pcacc_pool_skip_relu_backward_strided_y32(const float *y, const uint16_t *grad_pooled, const uint16_t *grad_skip, int64_t skip_pitch,
                                              int64_t n_img, int32_t h, int32_t w, int32_t c, uint16_t *grad_y, void *stream);

/* Batched inverse of n 4x4 f32 matrices (the pose tables: torch.linalg.inv at models/motionnet.py:100 and models/alignnet.py:33),
 * Gauss-Jordan with partial pivoting, one launch; a singular matrix yields inf / nan entries (no status word). */
int pcacc_inv4x4(const float *m, int64_t n, float *out, void *stream);

/* Weight gradient of a row-linear layer with few inputs (k in {1,2,3,4,9}, n in {32,64,128}: first layers of the point chains) or few
 * outputs (n in {1,2,3,4,9}, k in {32,64,128}: the heads) -- same result and operand conventions as pcacc_rows_wgrad_mixed
 * (dw_aug [n, k+1] f32, bias gradient in the last column; dtypes bit 0 dY, bit 1 dy_mask, bit 2 X set = bf16), streamed at HBM speed
 * instead of padded into 32 x 32 matrix-core tiles; summed in a fixed order through workspace partials (no atomics). */
int pcacc_rows_wgrad_few_supported(int32_t k, int32_t n);
int pcacc_rows_wgrad_few_workspace_bytes(int64_t rows, int32_t k, int32_t n, size_t *bytes /*host*/);
int pcacc_rows_wgrad_few(const void *dy, const void *dy_mask, const void *x, int32_t x_relu, int64_t rows, int32_t k, int32_t n,
                         float *dw_aug, int32_t dtypes, void *workspace, size_t workspace_bytes, void *stream);

/* TubeNet slot algebra -- models/tpointnet.py:249-305 (TPointNet.forward after the pooled embeddings) and the refinement loop of
 * models/alignnet.py:236-263, per refinement iteration.  A slot s = k * n_frames + t is instance k in frame t; slot [n] i32 is the
 * slot of every foreground point; slot_centre [S,3] the per-slot centroids (the anchor frame's row k * n_frames is the one used).
 *  rows           rows [n,4] = (xyz - centre of the instance's anchor frame, t / n_frames): input of the positional embedding
 *                 (tpointnet.py:246-251).
 *  code           code [S,4c] = (geo[k], motion[k], frame[s], frame[k * n_frames]) (tpointnet.py:259-262); backward: the three gradients.
 *  pose_forward   pose_vec [S,7] (quaternion xyzw, translation) -> pose_c / gt_c [S,12] (R row-major, t): estimated pose and ground truth
 *                 `remaining` [S,4,4] re-expressed for the centred cloud (batch_quat2mat / batch_mat2quat, tpointnet.py:20-73);
 *                 loss_rt [2] f64 = weighted means of |q_gt - q| and |t_gt - t| (evaluate_pose, :76-94; q_gt by scipy's branch scheme
 *                 in f64); step [S,4,4] = the un-centred pose, frame 0 = identity (:291-296); remaining_out = remaining @ step^-1 and
 *                 total_out = step @ total_in (alignnet.py:257-263; total_in NULL = identity); wsum [1] = sum(weights) + 1e-20.
 *  gap_forward    pp [n,4] = (|est - gt|_2, |est - gt|_1, 0, 0) of the centred point under the two poses (tpointnet.py:276-281).
 *  finish         l12 [2] = sum_s weights[s] * slot_sums[s][0|1] / max(count[s], 1) / wsum (tpointnet.py:282-286).
 *  gap_backward   grad_rows16 [n,16]: per point gradient of (grad_l1 * l12[0] + grad_l2 * l12[1]) w.r.t. pose_c of its slot (12 + 4 zeros);
 *                 their per-slot sums are grad_pose [S,stride] of
 *  pose_backward  grad_vec [S,7], including the loss_rt terms (grad_rot, grad_trans f64 scalars; NULL = 0).
 * The slot-level kernels run in one workgroup each. */
int pcacc_tube_rows(const float *xyz, const int32_t *slot, const float *slot_centre, int64_t n, int32_t n_frames, float *rows, void *stream);
int pcacc_tube_code(const float *geo, const float *motion, const float *frame, int64_t n_inst, int32_t n_frames, int32_t c, float *code,
                    void *stream);
int pcacc_tube_code_backward(const float *grad_code, int64_t n_inst, int32_t n_frames, int32_t c, float *grad_geo, float *grad_motion,
                             float *grad_frame, void *stream);
int pcacc_tube_pose_forward(const float *pose_vec, const float *remaining, const float *total_in, const float *slot_centre,
                            const float *weights, int32_t n_slots, int32_t n_frames, float *pose_c, float *gt_c, float *step,
                            float *remaining_out, float *total_out, double *loss_rt, float *wsum, void *stream);
int pcacc_tube_gap_forward(const float *rows, const int32_t *slot, const float *pose_c, const float *gt_c, int64_t n, float *pp, void *stream);
int pcacc_tube_finish(const float *slot_sums, int32_t stride, const float *count, const float *weights, const float *wsum, int32_t n_slots,
                      float *l12, void *stream);
int pcacc_tube_gap_backward(const float *rows, const int32_t *slot, const float *pose_c, const float *gt_c, const float *weights,
                            const float *count, const float *wsum, const float *grad_l1, const float *grad_l2, int64_t n,
                            float *grad_rows16, void *stream);
int pcacc_tube_pose_backward(const float *pose_vec, const float *remaining, const float *slot_centre, const float *weights, const float *wsum,
                             const float *grad_pose, int32_t stride, const double *grad_rot, const double *grad_trans, int32_t n_slots,
                             int32_t n_frames, float *grad_vec, void *stream);

/* Host words -> device memory as kernel arguments (asynchronous, unlike a pageable hipMemcpy on the compute stream):
 * n 32-bit words from host_words to dst, 240 per launch.  For the per-step index tables a host loop of the reference
 * becomes (sample offsets, per-pair counts, thresholds). */
int pcacc_upload_words(const uint32_t *host_words, int64_t n, uint32_t *dst, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PCACC_H_ */
