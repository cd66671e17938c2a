/*
 * ococc_hip.h -- C ABI of libococc_hip.so, the MI355X (gfx950) kernels behind
 * the OcOccNet hot path of Ghostish/ObjectCentricOccCompletion.
 *
 * Drop-in boundary.  The reference binds this path through pybind11 torch
 * extensions that take at::Tensor (mmdet3d/ops/voxel/src/voxelization.cpp:6-11,
 * mmdet3d/ops/spconv/src/all.cc:21-51) plus three un-vendored CUDA packages
 * (TorchEx, torch_scatter, SpConv2).  This header replaces those bindings with
 * plain pointers and sizes; INTEGRATION.md shows the ctypes stub a reference
 * maintainer would add in the mmdet3d/ops python files to call it.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer unless the parameter is called host_*; arrays `T x[k]`, host_* pointers and
 *     the descriptor structs (`const ococc_<struct>* x`) are HOST memory, read or written before the call returns.
 *     The Python binding derives its ctypes signatures from this header by that rule ("C ABI binding");
 *   - the caller owns every buffer, including `workspace` whose size comes from
 *     the matching *_workspace_bytes() query (pure host arithmetic);
 *   - nothing allocates, frees, synchronises or throws; work is queued on
 *     `stream` (a hipStream_t passed as void*, NULL = the null stream);
 *   - variable-size results are written into worst-case sized buffers and
 *     their length into a device int32 the caller reads back when it needs it;
 *   - return 0 on success, a negative OCOCC_E* code otherwise;
 *     ococc_last_error() returns the message of the calling thread's last
 *     failure;
 *   - row-major contiguous tensors; "bf16" buffers are uint16_t bit patterns.
 */
#ifndef OCOCC_HIP_H_
#define OCOCC_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCOCC_OK 0
#define OCOCC_EINVAL (-1)      /* bad argument (message says which) */
#define OCOCC_EHIP (-2)        /* HIP runtime error */
#define OCOCC_EUNSUPPORTED (-3) /* shape / dtype outside the compiled kernels */
#define OCOCC_ESTRANDED (-4)   /* a grid barrier of an earlier one-launch SIR layer gave up: its results are incomplete */

/* element types of feature buffers */
#define OCOCC_F32 0
#define OCOCC_BF16 1

/* reduce types; values follow reduce_t of the reference
 * (mmdet3d/ops/voxel/src/scatter_points_cuda.cu:6) */
#define OCOCC_REDUCE_SUM 0
#define OCOCC_REDUCE_MEAN 1
#define OCOCC_REDUCE_MAX 2

typedef void* ococc_stream_t; /* hipStream_t */

const char* ococc_last_error(void);
int ococc_version(void);
/* compiled for: returns "gfx950" */
const char* ococc_arch(void);

/* ------------------------------------------------------------------------ *
 * B1  dynamic voxelisation
 * replaces voxelization::dynamic_voxelize
 *   (mmdet3d/ops/voxel/src/voxelization.h:77-88, kernels
 *    voxelization_cuda.cu:25-65 / voxelization_cpu.cpp:8-41)
 * coors[i] = (z,y,x) int32, c = floor((p - min) / voxel) CLAMPED to
 * [0, grid-1] (this fork clamps; upstream mmdet3d writes -1),
 * grid = ceil((max - min) / voxel)  (voxelization_cpu.cpp:155-158).
 * points: [num_points, num_features] f32, first three columns are x,y,z.
 * ------------------------------------------------------------------------ */
int ococc_dynamic_voxelize_f32(const float* points, int64_t num_points, int32_t num_features,
                               const float host_voxel_size[3], const float host_coors_range[6],
                               int32_t* coors, ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * hard voxelisation (max_points / max_voxels caps, first-come order)
 * replaces voxelization::hard_voxelize
 *   (voxelization.h:60-75, voxelization_cpu.cpp:44-143).
 * grid = round((max - min) / voxel) (voxelization_cpu.cpp:119-122).
 * voxels [max_voxels,max_points,num_features] f32 (caller zero-fills),
 * coors [max_voxels,3] i32, num_points_per_voxel [max_voxels] i32 (zeroed),
 * voxel_num: device int32 receiving the number of voxels produced.
 * ------------------------------------------------------------------------ */
int64_t ococc_hard_voxelize_workspace_bytes(int64_t num_points, const float host_voxel_size[3],
                                            const float host_coors_range[6]);
int ococc_hard_voxelize_f32(const float* points, int64_t num_points, int32_t num_features,
                            const float host_voxel_size[3], const float host_coors_range[6],
                            int32_t max_points, int32_t max_voxels, float* voxels, int32_t* coors,
                            int32_t* num_points_per_voxel, int32_t* voxel_num, void* workspace,
                            int64_t workspace_bytes, ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * unique rows of integer coordinates on a bounded grid
 * replaces at::unique_dim(coors, 0, sorted, inverse, counts) as used by
 *   dynamic_point_to_voxel_forward (scatter_points_cuda.cu:199-210) and
 *   torch.unique(coors, dim=0, return_inverse=True) in scatter_v2
 *   (mmdet3d/ops/sst/sst_ops.py:150-181).
 * coors [n, ndim] int32 (ndim 1..4), host_dims[ndim] = exclusive upper bound
 * of each column.  Rows with any negative entry are dropped (inv = -1), as
 * DynamicScatter does; rows with an entry >= its bound set *status to 1.
 * Outputs are in lexicographic order of the rows (== torch.unique order):
 * out_coors [>= num_unique, ndim], inv [n] (row -> unique row), counts
 * [>= num_unique], num_unique (device int32).  out_capacity bounds the rows
 * written to out_coors/counts (use min(n, prod(dims))).
 * ------------------------------------------------------------------------ */
int64_t ococc_grid_unique_workspace_bytes(int32_t ndim, const int32_t host_dims[4]);
/* Byte offsets of the cell bitmap (1 bit per cell, row-major over dims) and of its exclusive popcount
 * prefix (one u32 per 32 cells) inside the grid_unique workspace: after ococc_grid_unique_i32 they
 * describe the sorted voxel set and can be handed to ococc_subm_rulebook_build_sorted. */
int ococc_grid_unique_workspace_layout(int32_t ndim, const int32_t host_dims[4], int64_t* host_bitmap_offset,
                                       int64_t* host_prefix_offset);
int ococc_grid_unique_i32(const int32_t* coors, int64_t n, int32_t ndim, const int32_t host_dims[4],
                          int32_t* out_coors, int64_t out_capacity, int32_t* inv, int32_t* counts,
                          int32_t* num_unique, int32_t* status, void* workspace,
                          int64_t workspace_bytes, ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * A5 / B2  segment (scatter) reduce, forward and backward
 * replaces feats_reduce_kernel + traceback kernels
 *   (scatter_points_cuda.cu:81-179) and torch_scatter.scatter_max /
 *   scatter(reduce='mean'|'sum') called at sst_ops.py:171-174.
 * feats [n, c] f32, inv [n] int32 in [-1, num_segments) (-1 rows ignored),
 * out [num_segments, c] f32.  counts [num_segments] int32 is required for
 * MEAN (divide) and optional otherwise (segments with count 0 -> 0 for MAX,
 * as torch_scatter does; MAX with counts == NULL leaves them at -inf: nothing
 * tells an empty segment from a written one).  SUM gives empty segments 0
 * either way.  arg [num_segments, c] int32 (MAX only, may be
 * NULL): smallest row index attaining the max -- the tie rule of
 * max_reduce_traceback_scatter_idx_kernel (scatter_points_cuda.cu:136-160).
 * ------------------------------------------------------------------------ */
int ococc_segment_count_i32(const int32_t* inv, int64_t n, int32_t* counts, int64_t num_segments,
                            ococc_stream_t stream);
int ococc_segment_reduce_f32(const float* feats, const int32_t* inv, int64_t n, int32_t c,
                             int32_t reduce_type, const int32_t* counts, float* out, int32_t* arg,
                             int64_t num_segments, ococc_stream_t stream);
/* grad_feats [n, c] is fully written (no pre-zeroing needed).
 * SUM:  g[i] = go[inv[i]];  MEAN: g[i] = go[inv[i]] / counts[inv[i]];
 * MAX:  g[i][ch] = arg[inv[i]][ch] == i ? go[inv[i]][ch] : 0. */
int ococc_segment_reduce_bwd_f32(const float* grad_out, const int32_t* inv, int64_t n, int32_t c,
                                 int32_t reduce_type, const int32_t* counts, const int32_t* arg,
                                 float* grad_feats, int64_t num_segments, ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * B1 + B2 fused: dynamic voxelisation followed by DynamicScatter(mean)
 * replaces, for the per-object grid front end, the sequence
 *   voxelization::dynamic_voxelize      (mmdet3d/ops/voxel/src/voxelization.h:77-88)
 *   coors = cat(batch_idx, zyx)         (mmdet3d/models/detectors: every voxel pipeline)
 *   DynamicScatter.forward_single(mean) (mmdet3d/ops/voxel/scatter_points.py:53-107,
 *                                        scatter_points_cuda.cu:199-241)
 * with the results of running ococc_dynamic_voxelize_f32 + ococc_grid_unique_i32 +
 * ococc_segment_reduce_f32(MEAN) one after the other: voxel rows in ascending (b,z,y,x) order,
 * inv[i] = row of point i (-1: batch_idx[i] < 0, dropped), counts, and the mean of the point
 * features per voxel (sums of >= 3 points may differ in the last bit: float atomics, as there).
 * points [n, num_point_features] f32 (x,y,z first), batch_idx [n] int32 in [0, batch_size)
 * (>= batch_size sets *status = 1 and drops the point), feats [n, c] f32.
 * host_grid_zyx must equal ceil((max - min) / voxel) per axis (checked).
 * All out_capacity rows are written: rows past *num_voxels get -1 coordinates, count 0 and zero
 * features (the fixed-capacity form HIP-graph capture needs; use out_capacity = min(n, cells)).
 * voxel_feats [out_capacity, c] f32 is required (it is where the sums live); voxel_feats_bf16
 * (optional) receives the same means rounded to bf16 for the convolutions.
 * num_voxels / status: ONE device int32[2].  The workspace keeps the grid's cell bitmap and
 * popcount prefix at the offsets ococc_grid_unique_workspace_layout reports for
 * dims = {batch, D, H, W}, ready for ococc_subm_rulebook_build_sorted.
 * ------------------------------------------------------------------------ */
int64_t ococc_voxelize_scatter_workspace_bytes(int64_t n, int32_t batch_size, const int32_t host_grid_zyx[3]);
int ococc_voxelize_scatter_mean_f32(const float* points, int32_t num_point_features, const int32_t* batch_idx,
                                    int64_t n, const float* feats, int32_t c, const float host_voxel_size[3],
                                    const float host_coors_range[6], int32_t batch_size,
                                    const int32_t host_grid_zyx[3], int32_t* voxel_coors, int64_t out_capacity,
                                    int32_t* inv, int32_t* counts, float* voxel_feats, uint16_t* voxel_feats_bf16,
                                    int32_t* num_voxels, int32_t* status, void* workspace, int64_t workspace_bytes,
                                    ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * B1 + B2 + B3 for a batch of per-object grids in three launches: the outputs of
 * ococc_voxelize_scatter_mean_f32 (replaces Voxelization dynamic + DynamicScatter mean,
 * ops/voxel/voxelize.py:10-113, ops/voxel/scatter_points.py:53-107) AND of the 3x3x3 dilation-1
 * ococc_subm_rulebook_build_sorted on those voxels (replaces getIndicePair<3> with subM,
 * ops/spconv/include/spconv/spconv_ops.h:27-104 / geometry.h:247-297), bit for bit, in the
 * fixed-capacity form (every one of `capacity` rows is written; rows past *num_voxels carry -1
 * coordinates, count 0, zero features, -1 neighbours; indice_pairs[k][.][indice_num[k]..] is left
 * unwritten, as with fill_pair_tails = 0).
 * Preconditions beyond those of the two entry points: batch_idx is non-decreasing (points arrive
 * grouped by object grid; anything else sets *status = 1 and drops the offending points), the cells of
 * one grid are a multiple of 32 and at most 512 Ki (bitmap + prefix of one grid live in LDS),
 * capacity = min(n, batch * cells).  slices (1..8): workgroups per grid in the emit launch.
 * nbr_t [27, capacity] int32, blockmask [ceil(capacity/16)] u32, indice_pairs [27, 2, capacity] int32,
 * indice_num [27] int32.  The workspace starts with the grid_unique layout (bitmap | prefix), as the
 * voxelize_scatter workspace does.
 * ------------------------------------------------------------------------ */
int64_t ococc_object_grid_geometry_workspace_bytes(int64_t n, int32_t batch_size, const int32_t host_grid_zyx[3],
                                                   int32_t slices);
int ococc_object_grid_geometry_f32(const float* points, int32_t num_point_features, const int32_t* batch_idx,
                                   int64_t n, const float* feats, int32_t c, const float host_voxel_size[3],
                                   const float host_coors_range[6], int32_t batch_size,
                                   const int32_t host_grid_zyx[3], int32_t slices, int32_t* voxel_coors,
                                   int64_t capacity, int32_t* inv, int32_t* counts, float* voxel_feats,
                                   uint16_t* voxel_feats_bf16, int32_t* num_voxels, int32_t* status, int32_t* nbr_t,
                                   uint32_t* blockmask, int32_t* indice_pairs, int32_t* indice_num, void* workspace,
                                   int64_t workspace_bytes, ococc_stream_t stream);
/* The same, also building the neighbour-pattern row order (ococc_subm_row_order below) of the table it writes, where
 * the rows' 27 table entries sit in registers anyway: order_counters as there, order_rowrec [capacity, 4] int32, 16-byte
 * aligned (scratch: the per-row records), capacity below 2^20.
 *   order_rec [capacity, 4] int32 + order_hdr [8] int32 given: the finished order, as ococc_subm_row_order leaves it
 *     (heavy_blocks / mid_blocks as there): ococc_subm_row_order_place runs behind the last kernel.
 *   order_rec / order_hdr NULL: only the row records; follow with ococc_subm_row_order_place(order_rowrec, 27, 13,
 *     capacity, ...).
 * order_counters and order_rowrec NULL: exactly the call above. */
int ococc_object_grid_geometry_order_f32(const float* points, int32_t num_point_features, const int32_t* batch_idx,
                                         int64_t n, const float* feats, int32_t c, const float host_voxel_size[3],
                                         const float host_coors_range[6], int32_t batch_size,
                                         const int32_t host_grid_zyx[3], int32_t slices, int32_t* voxel_coors,
                                         int64_t capacity, int32_t* inv, int32_t* counts, float* voxel_feats,
                                         uint16_t* voxel_feats_bf16, int32_t* num_voxels, int32_t* status, int32_t* nbr_t,
                                         uint32_t* blockmask, int32_t* indice_pairs, int32_t* indice_num, void* workspace,
                                         int64_t workspace_bytes, void* order_counters, int32_t* order_rowrec,
                                         int32_t* order_rec, int32_t* order_hdr, int32_t heavy_blocks, int32_t mid_blocks,
                                         ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * visibility ray test of the GT-occupancy annotation
 * replaces point_cloud_to_range_image_idx (tools/occ/occ_annotate.py:141-207) and the gather /
 * compare / max-over-frames-and-sensors around it in OccAnnotator.annotate_trk (:488-556).
 * centers [n,3] f64: unoccupied cell centres in the object frame.  Frame f, sensor c (index
 * sf = c * frames + f):  p_ego = to_ego[f] (p),  p_sensor = to_sensor[sf] (p_ego)  with affines
 * stored as 12 doubles (row-major 3x3 rotation, then the translation; to_sensor = inverse of the
 * LiDAR extrinsic), az_corr[sf] = atan2(extrinsic[1][0], extrinsic[0][0]), inclinations
 * [sensors*frames, height] f64 in the order the range-image rows use (the reference flips the beam
 * table first), range_images[sf] -> device [height, width] f32 (range_dtype 0) or f64 (2).
 * visibility [n] int32 (optional): 2 where some sensor in some frame measured a range >= the
 * centre's range in the centre's pixel (the ray crossed the cell: empty), else 0.
 * dbg_indices [sensors*frames, n, 2] int32 (row, col) / dbg_range [sensors*frames, n] f64 (optional,
 * together): the outputs of point_cloud_to_range_image_idx, for parity tests.
 * ------------------------------------------------------------------------ */
int ococc_occ_visibility_f64(const double* centers, int64_t n, const double* to_ego, int32_t frames,
                             const double* to_sensor, const double* az_corr, const double* inclinations,
                             int32_t sensors, int32_t height, int32_t width, const void* const* range_images,
                             int32_t range_dtype, int32_t* visibility, int32_t* dbg_indices, double* dbg_range,
                             ococc_stream_t stream);

/* Same rulebook when the rows of `indices` are exactly the occupied cells of a [batch, D, H, W] grid in
 * ascending cell order and the caller still holds that grid's bitmap + popcount prefix (the state
 * ococc_grid_unique_i32 leaves in its workspace, see ococc_grid_unique_workspace_layout): the
 * marking, scanning and row-permutation passes are skipped.  Rows with negative coordinates
 * (fixed-capacity padding) take part in no pair.  fill_pair_tails = 0 leaves indice_pairs[k][.][indice_num[k]..]
 * unwritten (the reference format fills them with -1: 27 MB of stores per call that a fixed-capacity training
 * step never reads).  Workspace size as for ococc_subm_rulebook_build. */
int ococc_subm_rulebook_build_sorted(const int32_t* indices, int64_t n, int32_t batch_size,
                                     const int32_t host_shape[3], const int32_t host_ksize[3],
                                     const uint32_t* grid_bitmap, const uint32_t* grid_prefix, int32_t* nbr_t,
                                     uint32_t* blockmask, int32_t* indice_pairs, int32_t* indice_num,
                                     int32_t fill_pair_tails, void* workspace, int64_t workspace_bytes,
                                     ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * B3  sub-manifold rulebook
 * replaces spconv::getIndicePair<3>(subM) (include/spconv/spconv_ops.h:27-104
 * -> geometry.h:247-297 CPU / indice.cu.h:147-234 GPU).
 * indices [n, 4] int32 (batch, z, y, x); spatial shape host_shape[3] (D,H,W);
 * kernel size host_ksize[3] (odd), dilation host_dilation[3].
 * Products:
 *   nbr_t     [kvol, n] int32  nbr_t[k][o] = input row feeding output row o
 *                              through kernel offset k, or -1;
 *   blockmask [ceil(n/16)] u32 bit k set iff rows 16b..16b+15 have any
 *                              neighbour at offset k (kvol <= 32 only,
 *                              otherwise pass NULL);
 *   indice_pairs [kvol,2,n] int32 and indice_num [kvol] int32 -- the
 *     reference rulebook, filled with -1 beyond indice_num[k], in the exact
 *     order of the CPU functor (ascending input row within an offset).
 * offset index k = sum_d m_d * (in_d - out_d + pad_d), last dim fastest
 * (geometry.h:61-72).
 * ------------------------------------------------------------------------ */
int64_t ococc_subm_rulebook_workspace_bytes(int64_t n, int32_t batch_size,
                                            const int32_t host_shape[3],
                                            const int32_t host_ksize[3]);
int ococc_subm_rulebook_build(const int32_t* indices, int64_t n, int32_t batch_size,
                              const int32_t host_shape[3], const int32_t host_ksize[3],
                              const int32_t host_dilation[3], int32_t* nbr_t, uint32_t* blockmask,
                              int32_t* indice_pairs, int32_t* indice_num, void* workspace,
                              int64_t workspace_bytes, ococc_stream_t stream);

/* Regular (strided) / transposed sparse conv rulebook: the non sub-manifold branch of
 * spconv::getIndicePair (spconv_ops.h:105-141; geometry.h:144-245, indice.cu.h:22-145).
 * Active outputs are numbered in sorted order of their flat grid index (the reference's GPU
 * path; its CPU functor numbers by first appearance); pairs of an offset are in ascending
 * input row.  out_indices [out_capacity,4] (use n*kvol as the safe bound or
 * min(n*kvol, batch*D*H*W)), indice_pairs [kvol,2,n] (-1 filled), indice_num [kvol],
 * num_out: device int32.  kvol <= 255. */
int64_t ococc_conv_rulebook_workspace_bytes(int64_t n, int32_t batch_size,
                                            const int32_t host_out_shape[3],
                                            const int32_t host_ksize[3]);
int ococc_conv_rulebook_build(const int32_t* indices, int64_t n, int32_t batch_size,
                              const int32_t host_out_shape[3], const int32_t host_ksize[3],
                              const int32_t host_stride[3], const int32_t host_padding[3],
                              const int32_t host_dilation[3], int32_t transpose,
                              int32_t* out_indices, int64_t out_capacity, int32_t* indice_pairs,
                              int32_t* indice_num, int32_t* num_out, void* workspace,
                              int64_t workspace_bytes, ococc_stream_t stream);

/* Rebuild the gather tables from a reference-format rulebook (any conv type:
 * regular / inverse / user supplied).  Each (row, offset) may appear at most
 * once on the chosen side (true for every spconv rulebook).
 * side = 1: table[k][pairs[k][1][p]] = pairs[k][0][p]  (forward: out <- in)
 * side = 0: table[k][pairs[k][0][p]] = pairs[k][1][p]  (dgrad:   in  <- out)
 * table [kvol, num_rows] int32 is fully written (-1 where empty). */
int ococc_rulebook_pairs_to_table(const int32_t* indice_pairs, const int32_t* indice_num,
                                  int32_t kvol, int64_t pair_capacity, int32_t side,
                                  int64_t num_rows, int32_t* table, uint32_t* blockmask,
                                  ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * B4  sparse convolution:  out[o] = sum_k  feat[table[k][o]] @ W[k]
 * replaces indiceConv / indiceConvBackward (spconv_ops.h:260-456): the
 * reference runs, per offset, gather kernel + GEMM + scatter-add kernel
 * (reordering.cu.h:21-157); here one output-stationary kernel gathers rows
 * straight into MFMA operand registers with the weights resident in LDS.
 *
 * feat   [n_in, kd] bf16        kd multiple of 16, <= 256
 * wn     [kvol, ncols, kd] bf16 weights with the contraction dim innermost
 *                               (forward: W[k]^T; dgrad: W[k'] as stored, see
 *                               ococc_weight_prepare_bf16)
 * table  [kvol, n_out] int32, blockmask [ceil(n_out/16)] (kvol <= 32)
 * bias   [ncols] f32 or NULL
 * out    [n_out, ncols] bf16 (out_dtype OCOCC_BF16) or f32; ncols mult. of 16
 * ln     NULL (plain convolution) or the LayerNorm epilogue below
 *
 * The three convolution kernels (this one, tile, sorted) take an optional
 * epilogue: the norm/activation pair of make_sparse_convmodule
 * (mmdet3d/ops/sparse_block.py:216-289: conv -> LayerNorm(eps) -> act).
 *   backward = 0  out = conv_out [n_out, ncols] bf16 (what the LN backward
 *                 needs), y = act(LN(conv_out)) bf16, mean_rstd [n_out, 2] f32,
 *                 as ococc_layernorm_act_fwd writes them: the norm sees the
 *                 bf16-rounded conv output, as the separate call would.
 *   backward = 1  the input-gradient pass of layer L+1 (feat = d conv_out of
 *                 layer L+1, wn = its dgrad operand, table = its table for the
 *                 backward direction) with the LayerNorm (+ act) BACKWARD of
 *                 the block in front (layer L) in its epilogue: with layer L's
 *                 saved conv output block_conv_out and statistics mean_rstd,
 *                 out = d_conv_out [n_out, ncols] bf16, the gradient of layer
 *                 L's CONV output (bit-identical to ococc_layernorm_act_bwd on
 *                 the bf16 dgrad output), plus one row of partial sums
 *                 [d gamma | d beta] per workgroup into partials [partial_rows,
 *                 2 ncols] f32, every row written (ococc_layernorm_param_reduce_multi
 *                 or a column sum finishes them).  ncols in {32, 64}.
 * With an epilogue, bias must be NULL and out_dtype OCOCC_BF16.  A shape that
 * has no fused kernel returns OCOCC_EUNSUPPORTED (then make the two calls).
 * The gather-GEMM kernel has no backward epilogue (OCOCC_EUNSUPPORTED).
 * ------------------------------------------------------------------------ */
typedef struct ococc_conv_ln {
  int32_t backward;               /* 0: LN(+act) forward epilogue; 1: LN(+act) backward of the block in front */
  int32_t act;                    /* 0 none, 1 GELU */
  float eps;                      /* forward */
  const float* gamma;             /* [ncols] f32 */
  const float* beta;              /* [ncols] f32 */
  uint16_t* y;                    /* forward: act(LN(out)) [n_out, ncols] bf16 */
  float* mean_rstd;               /* [n_out, 2] f32: written by the forward, read by the backward */
  const uint16_t* block_conv_out; /* backward: the block's saved conv output [n_out, ncols] bf16 */
  float* partials;                /* backward: [partial_rows, 2*ncols] f32 */
  int64_t partial_rows;
} ococc_conv_ln;
int ococc_sparse_conv_gather_gemm_bf16(const uint16_t* feat, int64_t n_in, int32_t kd,
                                       const uint16_t* wn, int32_t kvol, int32_t ncols,
                                       const int32_t* table, const uint32_t* blockmask,
                                       int64_t n_out, const float* bias, void* out,
                                       int32_t out_dtype, const ococc_conv_ln* ln, ococc_stream_t stream);

/* The same convolution for SUB-MANIFOLD tables over sparse active sets (a voxel has only a few
 * neighbours): the centre offset dense_k (every row is its own neighbour; -1: none) is a dense pass,
 * every other offset's rows are compacted to the ones that do have a neighbour before they are
 * gathered and multiplied, with f32 accumulators of a 512-row tile in LDS.  Same operands and the
 * same result (f32 accumulation, centre first, then ascending offsets: deterministic) as
 * ococc_sparse_conv_gather_gemm_bf16; faster below ~2-3 rulebook pairs per output row
 * (tools/density_sweep.py), slower on dense neighbourhoods.  kd in {32, 64, 128}, ncols in {32, 64, 128}; no block masks needed.
 * ln: the LayerNorm epilogue of ococc_sparse_conv_gather_gemm_bf16, applied where the finished f32 row sits in LDS --
 * forward on shapes up to 64 x 64 channels (OCOCC_EUNSUPPORTED otherwise), backward with ncols in {32, 64} and
 * partial_rows >= ococc_sparse_conv_tile_lnbwd_partial_rows(n_out, kd, ncols). */
int ococc_sparse_conv_tile_bf16(const uint16_t* feat, int64_t n_in, int32_t kd, const uint16_t* wn, int32_t kvol,
                                int32_t ncols, const int32_t* table, int32_t dense_k, int64_t n_out,
                                const float* bias, void* out, int32_t out_dtype, const ococc_conv_ln* ln,
                                ococc_stream_t stream);
int64_t ococc_sparse_conv_tile_lnbwd_partial_rows(int64_t n_out, int32_t kd, int32_t ncols);
/* The same convolution with the OUTPUT rows processed in neighbour-pattern order (sub-manifold tables, kvol <= 32).
 * ococc_subm_row_order buckets the rows of an offset-major gather table by (number of neighbours besides dense_k: 3+,
 * 2, 1, 0; lowest two neighbour offsets) -- rows that share their offsets become neighbours in the order, so a
 * workgroup walks only the offsets its rows have and 16-row MFMA blocks are nearly full.  The order is a property of
 * the table: build it once per rulebook, use it for every layer and direction that gathers through the table.
 *   counters ococc_subm_row_order_counter_bytes() bytes of scratch: cleared by every build before it counts (a memset node
 *            here; inside the first geometry kernel in ococc_object_grid_geometry_order_f32), contents undefined after
 *   scratch  ococc_subm_row_order_scratch_bytes(n) bytes, 16-byte aligned (the row records: n below 2^20)
 *   rec      [n, 4] int32, 16-byte aligned: per slot {row, offset mask (bit k: table[k][row] >= 0), table entries at the
 *            row's lowest and second lowest neighbour offsets (-1: none)}
 *   hdr      [8] int32   tile plan read by the kernel (heavy_blocks / mid_blocks: 16-row blocks per workgroup tile
 *                        for the 3+ / 2 neighbour classes: 4, 8 or 16; the rest uses 16)
 * Slots inside a bucket are handed out with atomics: the order may differ between two builds, the convolution's
 * result does not (each output row accumulates its own products in ascending offset order, in f32).
 * ococc_sparse_conv_sorted_bf16: operands as ococc_sparse_conv_gather_gemm_bf16 (wn row-major [kvol, ncols, kd]), same
 * result bit for bit; kd, ncols in {32, 64, 128}, not both 128.  Replaces indiceConv's per-offset gather / GEMM /
 * scatter-add (spconv_ops.h:300-354).
 * ln: the LayerNorm epilogue of ococc_sparse_conv_gather_gemm_bf16, for rulebooks that run in neighbour-pattern order;
 * the finished f32 row sits in the registers of the four lanes that share a slot, and the norm sums in the order of
 * ococc_layernorm_act_fwd, so the results equal the two-launch pair's (round 6: the 64 -> 128 forward of configs[1],
 * whose separate LN launch re-read 32 MB).  Backward: ncols in {32, 64}, partial_rows >=
 * ococc_sparse_conv_sorted_lnbwd_partial_rows(n_out); it replaces indiceConvBackward's input-gradient loop
 * (spconv_ops.h:363-456) followed by the LayerNorm backward of sparse_block.py:216-289's norm layer. */
int64_t ococc_subm_row_order_counter_bytes(void);
int64_t ococc_subm_row_order_scratch_bytes(int64_t n);
int ococc_subm_row_order(const int32_t* table, int32_t kvol, int32_t dense_k, int64_t n, int32_t heavy_blocks,
                         int32_t mid_blocks, void* counters, void* scratch, int32_t* rec, int32_t* hdr,
                         ococc_stream_t stream);
/* The second half of ococc_subm_row_order alone, for row records some other kernel left while it wrote the table
 * (ococc_object_grid_geometry_order_f32 without order_rec, which also counted them into ``counters``): records ->
 * slots, header. */
int ococc_subm_row_order_place(const int32_t* rowrec, int32_t kvol, int32_t dense_k, int64_t n, int32_t heavy_blocks,
                               int32_t mid_blocks, void* counters, int32_t* rec, int32_t* hdr, ococc_stream_t stream);
int ococc_sparse_conv_sorted_bf16(const uint16_t* feat, int64_t n_in, int32_t kd, const uint16_t* wn, int32_t kvol,
                                  int32_t ncols, const int32_t* table, const int32_t* rec, const int32_t* hdr,
                                  int64_t n_out, const float* bias, void* out, int32_t out_dtype, const ococc_conv_ln* ln,
                                  ococc_stream_t stream);
int64_t ococc_sparse_conv_sorted_lnbwd_partial_rows(int64_t n_out);

/* weights [kvol, cin, cout] (the reference layout (kD,kH,kW,Cin,Cout),
 * spconv/conv.py:98-99) in f32 or bf16 ->
 *   mode 0 (forward): wn[k][cout][cin]  = W[k][cin][cout]
 *   mode 1 (dgrad, sub-manifold): wn[k][cin][cout] = W[kvol-1-k][cin][cout]
 *   mode 2 (dgrad, generic table side 0): wn[k][cin][cout] = W[k][cin][cout]
 * always bf16 out. */
/* Same conversion for up to 16 f32 weight tensors in ONE launch (host arrays of device pointers and
 * sizes; argument meaning per entry as ococc_weight_prepare_bf16). */
int ococc_weight_prepare_multi_bf16(int32_t count, const void* const* host_w, const int32_t* host_kvol,
                                    const int32_t* host_cin, const int32_t* host_cout, const int32_t* host_mode,
                                    void* const* host_wn, ococc_stream_t stream);

int ococc_weight_prepare_bf16(const void* w, int32_t w_dtype, int32_t kvol, int32_t cin,
                              int32_t cout, int32_t mode, uint16_t* wn, ococc_stream_t stream);

/* dW[k] = sum_p x[pairs[k][0][p]]^T dy[pairs[k][1][p]]  over the rulebook.
 * x [n_in, cin] bf16, dy [n_out, cout] bf16, cin/cout multiples of 16,
 * dw [kvol, cin, cout] f32 (fully written).  Deterministic: partial sums go
 * to per-workgroup slabs in `workspace` and are added in a fixed order. */
int64_t ococc_sparse_conv_wgrad_workspace_bytes(int32_t kvol, int64_t pair_capacity, int32_t cin,
                                                int32_t cout);
int ococc_sparse_conv_wgrad_bf16(const uint16_t* x, int64_t n_in, int32_t cin, const uint16_t* dy,
                                 int64_t n_out, int32_t cout, const int32_t* indice_pairs,
                                 const int32_t* indice_num, int32_t kvol, int64_t pair_capacity,
                                 float* dw, void* workspace, int64_t workspace_bytes,
                                 ococc_stream_t stream);
/* Sparse max pooling over a rulebook -- replaces indice_maxpool_fp32/half and indice_maxpool_backward_fp32/half
 * (mmdet3d/ops/spconv/ops.py:162-184, src/maxpool.cc:9-55).  The reference's semantics: the output starts at ZERO and
 * takes an input only where that is larger (an output whose inputs are all negative holds 0); the backward pass gives
 * an output's gradient to every input equal to it.  table [kvol, n_out]: input row of (offset, output row) or -1
 * (ococc_rulebook_pairs_to_table, side of the forward direction); table_bwd [kvol, n_in]: output row of (offset, input
 * row) or -1.  dtype OCOCC_F32 / OCOCC_BF16 for features, out, out_bp and input_bp alike.  Sums in ascending offset
 * order, as the reference's CPU functor: f32 results bit for bit. */
int ococc_indice_maxpool(const void* features, int32_t dtype, int64_t n_in, int32_t channels, const int32_t* table,
                         int32_t kvol, int64_t n_out, void* out, ococc_stream_t stream);
int ococc_indice_maxpool_backward(const void* features, const void* out_features, const void* out_bp, int32_t dtype,
                                  int64_t n_in, int32_t channels, const int32_t* table_bwd, int32_t kvol, int64_t n_out,
                                  void* input_bp, ococc_stream_t stream);
/* The slab pass of ococc_sparse_conv_wgrad_bf16 (dw == NULL form) for TWO or THREE layers in one launch: arrays of
 * ``count``, shapes 16 x 32, 32 x 64 and 64 x 128 (OCOCC_EUNSUPPORTED otherwise; put the longest first).  Each is a few
 * hundred latency-bound work items that fill a fifth of the chip: side by side they take little more than the longest.
 * Every host_* argument is a HOST array of ``count`` entries (device pointers or sizes), read before the call returns.
 * Same slabs as separate calls, bit for bit; finish them with ococc_sparse_conv_wgrad_reduce_multi /
 * ococc_backward_param_reduce_multi. */
int ococc_sparse_conv_wgrad_multi_bf16(int32_t count, const uint16_t* const* host_x, const uint16_t* const* host_dy,
                                       const int32_t* host_cin, const int32_t* host_cout,
                                       const int32_t* const* host_indice_pairs, const int32_t* const* host_indice_num,
                                       const int32_t* host_kvol, const int64_t* host_pair_capacity,
                                       void* const* host_workspaces, const int64_t* host_workspace_bytes,
                                       ococc_stream_t stream);
/* Both kinds of end-of-backward parameter-gradient sums in ONE launch: the weight-gradient slab sums of
 * ococc_sparse_conv_wgrad_reduce_multi (first five tables) and the LayerNorm d gamma / d beta column sums of
 * ococc_layernorm_param_reduce_multi (last five); same results as the two calls, bit for bit.  (No reference
 * counterpart: indiceConvBackward and torch's native_layer_norm_backward reduce inside their own kernels.) */
int ococc_backward_param_reduce_multi(int32_t wcount, const void* const* host_workspaces,
                                      const int32_t* const* host_indice_nums, const int32_t* host_kvols,
                                      const int64_t* host_elems, float* const* host_dws, int32_t lcount,
                                      const void* const* host_partials, const int32_t* host_rows, const int32_t* host_c,
                                      void* const* host_dgamma, void* const* host_dbeta, ococc_stream_t stream);
/* dw == NULL above stops after the per-work-item slabs (left in `workspace`); this call finishes up to 8 such
 * weight gradients in one launch: host_dws[i][k][e] = sum of the slabs of offset k, fixed order (deterministic).
 * host_elems[i] = cin * cout of layer i.  Used to move the reductions of a backward pass behind its last kernel. */
int ococc_sparse_conv_wgrad_reduce_multi(int32_t count, const void* const* host_workspaces,
                                         const int32_t* const* host_indice_nums, const int32_t* host_kvols,
                                         const int64_t* host_elems, float* const* host_dws, ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * B5  fused LayerNorm + GELU(erf) over feature rows (the norm/act pair that
 * make_sparse_convmodule appends to a sparse conv, ops/sparse_block.py:216-289;
 * also every Linear->LN->GELU of build_mlp, sst_ops.py:333-360).
 * x, y [n, c] in `dtype` (f32 or bf16); gamma, beta [c] f32.
 * act: 0 = none (plain LayerNorm), 1 = GELU(erf).
 * mean_rstd [n, 2] f32 is written by forward and read by backward.
 * Backward: dx [n,c] in dtype; dgamma, dbeta [c] f32 are OVERWRITTEN with the sum
 * of per-workgroup partials taken in a fixed order (deterministic).
 * ------------------------------------------------------------------------ */
int ococc_layernorm_act_fwd(const void* x, int64_t n, int32_t c, const float* gamma,
                            const float* beta, float eps, int32_t act, void* y, float* mean_rstd,
                            int32_t dtype, ococc_stream_t stream);
int64_t ococc_layernorm_act_bwd_workspace_bytes(int64_t n, int32_t c);
int ococc_layernorm_act_bwd(const void* x, const void* dy, int64_t n, int32_t c,
                            const float* gamma, const float* beta, const float* mean_rstd,
                            int32_t act, void* dx, float* dgamma, float* dbeta, int32_t dtype,
                            void* workspace, int64_t workspace_bytes, ococc_stream_t stream);
/* The same two kernels with the Dropout that follows the activation in build_mlp's Sequential(Linear, norm, act,
 * Dropout) (mmdet3d/ops/sst/sst_ops.py:333-360; occ_dropout = 0.1 in configs/ococc/ococcnet.py) folded in: y =
 * dropout(act(LN(x))).  The keep mask is a counter-based hash of (seed, element index), 16 bits per element against
 * drop_threshold = round(p * 65536) (0: no dropout; kept values are scaled by 65536 / (65536 - drop_threshold)); the
 * backward regenerates it from the same (drop_threshold, seed), no mask is stored.  bf16 rows of 8 * 2^k <= 512 or
 * 1024 / 1536 / 2048 channels; OCOCC_EUNSUPPORTED otherwise.  (torch's own Philox stream cannot be reproduced by a
 * different kernel anyway; the statistics are what is kept.) */
int ococc_layernorm_act_dropout_fwd_bf16(const uint16_t* x, int64_t n, int32_t c, const float* gamma, const float* beta,
                                         float eps, int32_t act, uint32_t drop_threshold, uint64_t seed, uint16_t* y,
                                         float* mean_rstd, ococc_stream_t stream);
int ococc_layernorm_act_dropout_bwd_bf16(const uint16_t* x, const uint16_t* dy, int64_t n, int32_t c,
                                         const float* gamma, const float* beta, const float* mean_rstd, int32_t act,
                                         uint32_t drop_threshold, uint64_t seed, uint16_t* dx, float* dgamma,
                                         float* dbeta, void* workspace, int64_t workspace_bytes, ococc_stream_t stream);
/* dgamma == dbeta == NULL in ococc_layernorm_act_bwd: dx and the per-block partial sums only (the workspace
 * then holds ococc_layernorm_act_bwd_partial_rows(n, c, dtype) rows of [2c] f32 and must stay alive).
 * ococc_layernorm_param_reduce_multi finishes up to 16 such layers in ONE launch -- the host mirror queues it
 * to the end of the autograd backward pass (torch's LayerNorm backward, which the reference's
 * build_norm_layer(dict(type='LN')) layers use, returns the parameter gradients per layer:
 * mmdet3d/ops/sparse_block.py:216-289). */
int32_t ococc_layernorm_act_bwd_partial_rows(int64_t n, int32_t c, int32_t dtype);
int ococc_layernorm_param_reduce_multi(int32_t count, const void* const* host_partials, const int32_t* host_rows,
                                       const int32_t* host_c, void* const* host_dgamma, void* const* host_dbeta,
                                       ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * A3  points-in-rotated-box pooling
 * replaces TorchEx dynamic_point_pool_ext.dynamic_point_pool_mixed_gpu as called at
 *   mmdet3d/ops/dynamic_point_pool_op.py:81-87 (source not vendored; contract from the
 *   call site and the debug assertions of
 *   models/roi_heads/roi_extractors/dynamic_point_roi_extractor.py:222-234).
 * rois [R,7] f32 (x,y,z_bottom,w,l,h,yaw), rois_key [R] i32, pts [N,3] f32, pts_key [N] i32.
 * A pair (point, RoI) is emitted when the keys match and the point is inside the RoI
 * enlarged by host_extra_wlh (w,l,h; extra/2 per side).  Rows are written SORTED by
 * (RoI, point index): out_pts_idx / out_roi_idx [>= num_out] i64, out_pts_feats
 * [>= num_out, 13] f32 = xyz, box-frame xyz, 6 face distances of the original box,
 * is_in_margin.  Caps: max_inbox_point per RoI, max_all_pts rows in total (the smallest
 * point indices / RoI indices are kept).  roi_counts [R] i32 (may be NULL) = rows kept per
 * RoI; num_out = rows written (device int32).
 * ------------------------------------------------------------------------ */
int64_t ococc_point_pool_workspace_bytes(int64_t num_points, int64_t num_rois);
int ococc_dynamic_point_pool_mixed(const float* rois, const int32_t* rois_key, int64_t num_rois,
                                   const float* pts, const int32_t* pts_key, int64_t num_points,
                                   const float host_extra_wlh[3], int32_t max_inbox_point,
                                   int64_t max_all_pts, int64_t* out_pts_idx, int64_t* out_roi_idx,
                                   float* out_pts_feats, int32_t* roi_counts, int32_t* num_out,
                                   void* workspace, int64_t workspace_bytes, ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * A2  pairwise (i-th with i-th) 3-D IoU of rotated boxes
 * replaces LiDARInstance3DBoxes.aligned_iou_3d
 *   (mmdet3d/core/bbox/structures/lidar_box3d.py:404-448 -> TorchEx boxes_overlap_1to1).
 * boxes [n,7] f32 (x, y, z_bottom, w, l, h, yaw); iou [n] f32.
 * ------------------------------------------------------------------------ */
int ococc_aligned_iou3d_f32(const float* boxes1, const float* boxes2, int64_t n, float* iou,
                            ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * CTRL tracklet data preparation, host layer: objectcentricocccompletion_amd/ctrl_prep.py
 *
 * Max IoU of every (predicted, ground-truth) tracklet pair of one segment
 * replaces the per-pair loop of tools/ctrl/generate_candidates.py:61-65 over LiDARTracklet.max_iou
 *   (mmdet3d/core/bbox/structures/lidar_tracklet.py:210-229: timestamp intersection, two uploads, one
 *   aligned_iou_3d launch and an .item() per pair) by ONE launch per segment.
 * pd_boxes [sum Lp, 7] f32 the boxes of the P predicted tracklets back to back, pd_offsets [P+1] i32,
 * pd_frames [sum Lp] i32: index of the box's timestamp in the segment's sorted timestamp list, strictly increasing
 * within a tracklet; gt_* the same for the G ground-truth tracklets.  max_iou [P, G] f32: the maximum over the common
 * frames of the one-to-one IoU (the arithmetic of ococc_aligned_iou3d_f32, bit for bit), 0 without a common frame.
 * ------------------------------------------------------------------------ */
int ococc_tracklet_max_iou_f32(const float* pd_boxes, const int32_t* pd_offsets, const int32_t* pd_frames,
                               int32_t num_pd, const float* gt_boxes, const int32_t* gt_offsets,
                               const int32_t* gt_frames, int32_t num_gt, float* max_iou, ococc_stream_t stream);

/* Points of many frames into the boxes of their frames, the cloud's order kept
 * replaces the per-frame, per-box loop of tools/ctrl/generate_track_input.py:84-99 (box upload, points_in_boxes over
 *   the whole cloud, mask compaction, device-to-host copy, each per box) by one count launch, one read-back of
 *   counts and one fill launch per batch of frames.  Membership: check_pt_in_box3d
 *   (mmdet3d/ops/roiaware_pool3d/src/points_in_boxes_cuda.cu:24-49), every box on its own (a point may be in several).
 * points [N, point_dim] f32 (point_dim >= 3, xyz read) of `frames` frames back to back, point_offsets [frames+1] i64;
 * boxes [B, 7] f32 (x, y, z_bottom, w, l, h, yaw; already enlarged) grouped by frame, box_offsets [frames+1] i64;
 * max_frame_points: the largest frame's point count (the host made the offsets).  frames <= 65535.
 * workspace: ceil(max_frame_points / 4096) * 4 * B * 4 bytes, written by _count and read by _fill of the SAME input.
 * _count: counts [B] i64.  _fill: scan [B+1] i64 = exclusive scan of counts (made by the host after the read-back),
 * out_index [scan[B]] i64: the frame-local point indices of box b at [scan[b], scan[b+1]) in ASCENDING order. */
int ococc_tracklet_crop_count(const float* points, int64_t num_points, int32_t point_dim,
                              const int64_t* point_offsets, const float* boxes, int64_t num_boxes,
                              const int64_t* box_offsets, int32_t frames, int64_t max_frame_points, int64_t* counts,
                              void* workspace, int64_t workspace_bytes, ococc_stream_t stream);
int ococc_tracklet_crop_fill(const float* points, int64_t num_points, int32_t point_dim, const int64_t* point_offsets,
                             const float* boxes, int64_t num_boxes, const int64_t* box_offsets, int32_t frames,
                             int64_t max_frame_points, const int64_t* scan, const void* workspace,
                             int64_t workspace_bytes, int64_t* out_index, ococc_stream_t stream);

/* Which boxes hold at least one point of their frame: the third mode of the same kernel
 * replaces the per-box loop of tools/ctrl/remove_empty.py:115-134 (group_size 1: box upload, points_in_boxes over the
 *   whole cloud, torch.unique and a device-to-host copy, each per box) by one launch per batch of frames.
 * Arguments as ococc_tracklet_crop_count (the bottom lift of remove_empty is applied to the boxes by the caller);
 * no workspace.  flags [B] i32: 1 where ococc_tracklet_crop_count would count at least one point (the same
 * arithmetic, bit for bit), else 0.  The call zero-fills flags; plain stores of 1, no atomics. */
int ococc_tracklet_nonempty(const float* points, int64_t num_points, int32_t point_dim, const int64_t* point_offsets,
                            const float* boxes, int64_t num_boxes, const int64_t* box_offsets, int32_t frames,
                            int64_t max_frame_points, int32_t* flags, ococc_stream_t stream);

/* One sensor frame's scene cloud into the step rows of online inference (csrc/scene_rows.hip), host layer:
 * objectcentricocccompletion_amd/scene_rows.py
 * replaces, for one frame, the offline chain in front of TrackletRoIHeadOCC.simple_test_step: the crop of
 *   tools/ctrl/generate_track_input.py:84-99, the per-frame cap of LoadTrackletPoints
 *   (mmdet3d/datasets/pipelines/tracklet_pipelines.py:26-91), TrackletPoseTransform (tracklet_pipelines.py:228-303),
 *   PointDecoration (yaw / 3.1415, size / 10, score) and PointsRangeFilter, each a pass of its own over the points, by
 *   one count launch, one read-back of counts and one fill launch that writes the rows.
 * points [N, point_dim] f32 (point_dim >= 3), crop_boxes [n, 7] f32 (x, y, z_bottom, w, l, h, yaw; already enlarged),
 * both in the cloud's frame.  N, n <= 2^31 - 1; N == 0 or n == 0 is an empty result (counts zero-filled).
 * Membership of a point in box b (the same in both passes): the test of ococc_tracklet_crop_count on the untransformed
 *   point, bit for bit (a point may be in several boxes; a NaN x or y is in none, a NaN z passes the height test there
 *   and here), and, with `host_range`, the WRITTEN xyz (a NaN is outside every range)
 *   strictly inside host_range = (x0, y0, z0, x1, y1, z1), a HOST array of 6 floats or null.
 * transforms [n, 12] f32 or null: row b's row-major 3x4 matrix m; the written xyz is
 *   x' = fmaf(z, m02, fmaf(y, m01, fmaf(x, m00, m03))), y' and z' the same with rows 1 and 2 (the identity returns the
 *   input bits, but for -0.0, which becomes +0.0); null: the input bits.
 * workspace: ococc_scene_rows_workspace_bytes(N, n) = ceil(N / 4096) * 4 * n * 4 bytes, written by _count and read by
 *   _fill of the SAME input.
 * _count: counts [n] i64, uncapped (integer atomics; the only atomics of the two).
 * _fill: scan_all [n+1] i64 = exclusive scan of counts, scan_out [n+1] i64 = exclusive scan of min(counts, max_points)
 *   (of counts when max_points <= 0), both made by the host after the read-back; M = scan_out[n].  With
 *   cap = max_points > 0 and m = counts[b] > cap, member j of the box (cloud order) is kept iff
 *   (j+1)*cap/m > j*cap/m in int64 floor division and goes to place j*cap/m of the box: exactly cap rows, ascending.
 *   Row r of box b, r in [scan_out[b], scan_out[b+1]), of point i: out_xyz [M, 3] f32 the written xyz, out_feats
 *   [M, attr_dims + row_feat_dim] f32 = points[i, 3 : 3+attr_dims] followed by row_feats[b, :] (row_feats
 *   [n, row_feat_dim] f32; copies, no arithmetic), out_row [M] i64 = b.  Rows sorted by (box, point index); vector
 *   stores only; nothing is written at or past row M. */
int64_t ococc_scene_rows_workspace_bytes(int64_t num_points, int64_t num_boxes);
int ococc_scene_rows_count(const float* points, int64_t num_points, int32_t point_dim, const float* crop_boxes,
                           int64_t num_boxes, const float* transforms, const float* host_range, int64_t* counts,
                           void* workspace, int64_t workspace_bytes, ococc_stream_t stream);
int ococc_scene_rows_fill(const float* points, int64_t num_points, int32_t point_dim, const float* crop_boxes,
                          int64_t num_boxes, const float* transforms, const float* host_range, int32_t attr_dims,
                          const float* row_feats, int32_t row_feat_dim, int64_t max_points, const int64_t* scan_all,
                          const int64_t* scan_out, float* out_xyz, float* out_feats, int64_t* out_row,
                          const void* workspace, int64_t workspace_bytes, ococc_stream_t stream);

/* The scene clouds of SEVERAL sensor frames into the step rows of a chunked online step (csrc/scene_rows.hip, the
 * same kernel with blockIdx.y = frame), host layer: objectcentricocccompletion_amd/scene_rows.py (scene_steps_rows)
 * replaces, for F frames in one call, the chain ococc_scene_rows_count / _fill replace for one: the crop of
 *   tools/ctrl/generate_track_input.py:84-99, the per-frame cap of LoadTrackletPoints
 *   (mmdet3d/datasets/pipelines/tracklet_pipelines.py:26-91), TrackletPoseTransform (tracklet_pipelines.py:228-303),
 *   PointDecoration and PointsRangeFilter -- there a pass each per frame, and with the one-cloud exports a count launch,
 *   a read-back and a fill launch per frame -- by ONE count launch, one read-back and one fill launch.
 * points [N, point_dim] f32 the clouds of `frames` frames back to back, cloud_offsets [frames+1] i64 (device);
 * crop_boxes [n, 7] f32 GROUPED BY FRAME, box_offsets [frames+1] i64 (device); box b of frame f sees the points
 * [cloud_offsets[f], cloud_offsets[f+1]) only.  max_frame_points / max_frame_boxes: the largest frame's points / boxes
 * (the host made the offsets; a frame whose offsets leave [0, N] or [0, n] is skipped).  frames <= 65535, N, n <= 2^31 - 1;
 * frames, N or n == 0 is an empty result (counts zero-filled).
 * Membership, transforms [n, 12], host_range and the written xyz: those of ococc_scene_rows_count, bit for bit.
 * workspace: ococc_scene_rows_workspace_bytes(max_frame_points, n), written by _count and read by _fill of the SAME input.
 * _count: counts [n] i64, uncapped, in the boxes' (frame-major) order.
 * _fill: caller_rows [n] i64, the caller's row number of each box; box_totals [n] i64 = counts; box_starts [n] i64, the
 *   first output row of each box -- the host orders the boxes by caller's row and scans min(counts, max_points) (counts
 *   when max_points <= 0) in THAT order; num_out = M, the rows in all.  The pick under the cap is that of
 *   ococc_scene_rows_fill.  Row r of box b, r in [box_starts[b], box_starts[b] + min(counts[b], cap)): out_xyz, out_feats
 *   as there (row_feats [n, row_feat_dim] in the boxes' order), out_row [M] i64 = caller_rows[b].  With distinct caller
 *   rows the output is sorted by (caller's row, point index within the frame); written straight to the final places,
 *   vector stores only, nothing at or past row M. */
int ococc_scene_rows_frames_count(const float* points, int64_t num_points, int32_t point_dim,
                                  const int64_t* cloud_offsets, const float* crop_boxes, int64_t num_boxes,
                                  const int64_t* box_offsets, int32_t frames, int64_t max_frame_points,
                                  int64_t max_frame_boxes, const float* transforms, const float* host_range,
                                  int64_t* counts, void* workspace, int64_t workspace_bytes, ococc_stream_t stream);
int ococc_scene_rows_frames_fill(const float* points, int64_t num_points, int32_t point_dim,
                                 const int64_t* cloud_offsets, const float* crop_boxes, int64_t num_boxes,
                                 const int64_t* box_offsets, int32_t frames, int64_t max_frame_points,
                                 int64_t max_frame_boxes, const float* transforms, const float* host_range,
                                 int32_t attr_dims, const float* row_feats, int32_t row_feat_dim,
                                 const int64_t* caller_rows, int64_t max_points, const int64_t* box_totals,
                                 const int64_t* box_starts, int64_t num_out, float* out_xyz, float* out_feats,
                                 int64_t* out_row, const void* workspace, int64_t workspace_bytes,
                                 ococc_stream_t stream);

/* Track extension by a constant-velocity model, all tracklets of a call in one launch
 * replaces the per-tracklet loop of tools/ctrl/extend_tracks.py:156-190 over LiDARTracklet.frame_transform,
 *   set_velocity, extend / extend_all and shared2ego (mmdet3d/core/bbox/structures/lidar_tracklet.py:345-387, 452-498,
 *   638-652, 669-791): a dozen small torch operators and a 4x4 inverse per tracklet.
 * boxes [num_boxes, 7] f32 (x, y, z_bottom, w, l, h, yaw) of the tracklets back to back, each in its frame's ego frame;
 * offsets [num_tracklets+1] i32; frames [num_boxes] i32: index of the box's timestamp in its SEGMENT's sorted
 * timestamp list, strictly increasing within a tracklet; segments [num_tracklets] i32; scores [num_boxes] f64.
 * poses [num_frames, 16] f32 (ego -> world, row major) and timestamps [num_frames] i64 (microseconds) of all segments
 * back to back, seg_offsets [num_segments+1] i32.
 * The plan is the host's (integer arithmetic on timestamps): num_back / num_fwd [num_tracklets] i32, the frames added
 * in front of the first and behind the last observed box (the frames frames[first] - num_back ... and
 * frames[last] + 1 ...), and out_offsets [num_tracklets+1] i32 with out_offsets[t+1] - out_offsets[t] =
 * num_back[t] + length(t) + num_fwd[t], out_offsets[num_tracklets] = num_out.  A tracklet whose plan leaves its
 * segment's frame table or the output is skipped.
 * out_boxes [num_out, 7] f32 in each output frame's own ego frame, out_scores [num_out] f64, out_frames [num_out] i32;
 * per tracklet: the added frames in front in ascending time (score s_first * m^(i+1), i counted from the EARLIEST),
 * the observed boxes (through the shared frame and back), the added frames behind (s_last * m^(i+1) outward).
 * float64 inside, one rounding to float32 on store; every output word has one writer. */
int ococc_track_extend_f64(const float* boxes, const int32_t* offsets, const int32_t* frames, const int32_t* segments,
                           const double* scores, int32_t num_tracklets, int64_t num_boxes, const float* poses,
                           const int64_t* timestamps, const int32_t* seg_offsets, int32_t num_segments,
                           int64_t num_frames, const int32_t* num_back, const int32_t* num_fwd,
                           const int32_t* out_offsets, int64_t num_out, double score_multiplier,
                           int32_t velo_window_size, float* out_boxes, double* out_scores, int32_t* out_frames,
                           ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Detection matching of the native Waymo metric: per frame, the full 3-D IoU of every (prediction, ground truth)
 * pair of equal type and the score-first greedy assignment
 * replaces the matching stage of compute_detection_metrics_main, the compiled waymo-open-dataset tool that
 *   WaymoTrackletDataset.evaluate runs (mmdet3d/datasets/waymo_tracklet_dataset.py:352-366) and the reference ships
 *   no source for; the protocol is the one DESIGN.md states (score-first matcher, not the tool's Hungarian default).
 * ococc_frame_match_workspace_bytes: the overlap matrix of `num_pairs` pairs (pure host arithmetic).
 * ------------------------------------------------------------------------ */
int64_t ococc_frame_match_workspace_bytes(int64_t num_pairs);
/* replaces the same stage of compute_detection_metrics_main (see above): two launches per call, whatever the number
 *   of frames.
 * pd_boxes [P, 7] f32 (centre x, y, z, length, width, height, heading) grouped by frame and, inside a frame, sorted by
 * (type, descending score, file order); pd_type / pd_eligible [P] i32; pd_offsets [F+1] i32.  gt_* the same for the G
 * ground-truth boxes, grouped by frame in file order.  pair_offsets [F+1] i64: the running sum of n_pd(f) * n_gt(f).
 * The call handles the frames [frame_begin, frame_end), whose pairs are [pair_begin, pair_end) =
 * pair_offsets[frame_begin], pair_offsets[frame_end] (host copies); max_frame_gt: the largest n_gt among them
 * (<= 4096).  host_iou_thresh[5]: threshold per type 0..4 (entry 0 unused; 1..4 in (0, 1]).
 * match_gt [P] i32: the index into gt_boxes of the box the prediction took, or -1; match_iou [P] f32: its IoU, or 0.
 * Written for the predictions of the frames of the call only.  A prediction takes the not-yet-taken eligible
 * ground-truth box of its type with the largest IoU >= threshold (equal IoU: the lower index); ineligible, degenerate
 * (extent <= 0, non-finite) and unknown-type boxes never match.  No atomics: the same input gives the same bytes. */
int ococc_frame_match_f32(const float* pd_boxes, const int32_t* pd_type, const int32_t* pd_eligible,
                          const int32_t* pd_offsets, int64_t num_pd, const float* gt_boxes, const int32_t* gt_type,
                          const int32_t* gt_eligible, const int32_t* gt_offsets, int64_t num_gt,
                          const int64_t* pair_offsets, int32_t frame_begin, int32_t frame_end, int64_t pair_begin,
                          int64_t pair_end, int32_t max_frame_gt, const float host_iou_thresh[5], int32_t* match_gt,
                          float* match_iou, void* workspace, int64_t workspace_bytes, ococc_stream_t stream);
/* replaces the same stage of compute_detection_metrics_main with the tool's default matcher as DESIGN.md states it
 *   (rule 4b: Hungarian, i.e. maximum total overlap, one matching per score cutoff) in place of the score-first greedy
 *   pass of ococc_frame_match_f32: the overlap launch of that export unchanged, then one assignment launch.
 * Inputs as ococc_frame_match_f32 (the workspace too: ococc_frame_match_workspace_bytes), plus max_frame_pd: the largest
 * n_pd among the frames of the call; 18 B * align64(max_frame_gt) + 2 B * align64(max_frame_pd) must fit 64 KiB of LDS.
 * An edge is an eligible equal-type pair with IoU >= threshold, its weight (int)(iou * 1000.0f) (0: no edge).
 * Predictions are inserted in their order, one shortest-augmenting-path search each (integer potentials, cost =
 * -weight, a private zero-cost "unmatched" column per prediction): after n insertions the matching has maximum total
 * weight for the first n predictions of the (frame, type) group.  Ties: a real column before a private one, the lower
 * ground-truth index among real columns, the row reached first among private ones.
 * snap_offsets [P] i64: -1, or where the snapshot that ends at this prediction starts in snapshots [num_snap_words] i32:
 * snapshots[snap_offsets[p] + r] = the index into gt_boxes of the partner of the r-th prediction of p's (frame, type)
 * group, or -1, in the matching of the group's predictions up to and including p (r = 0 .. p - group start).  The host
 * sets an offset at the last prediction of every score-cutoff bucket and sizes the buffer; snapshots that would not
 * fit num_snap_words are not written.  No atomics, one writer per word: the same input gives the same bytes. */
int ococc_frame_assign_i32(const float* pd_boxes, const int32_t* pd_type, const int32_t* pd_eligible,
                           const int32_t* pd_offsets, int64_t num_pd, const float* gt_boxes, const int32_t* gt_type,
                           const int32_t* gt_eligible, const int32_t* gt_offsets, int64_t num_gt,
                           const int64_t* pair_offsets, int32_t frame_begin, int32_t frame_end, int64_t pair_begin,
                           int64_t pair_end, int32_t max_frame_gt, int32_t max_frame_pd, const float host_iou_thresh[5],
                           const int64_t* snap_offsets, int64_t num_snap_words, int32_t* snapshots, void* workspace,
                           int64_t workspace_bytes, ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * occupancy IoU counts of one chunk of RoIs, replacing the ATen chain of TrackletRoIHeadOCC.test_occ
 *   (mmdet3d/models/roi_heads/tracklet_roi_head_occ.py:394-486: repeat, inside-box test, *, ==, &, |, two sums).
 * logits [n, K] f32 (decoder output, cls_dim 1); labels [K] int64 (occupied: == 1);
 * roi_xyz [n, K, 3] f32 RoI-frame query points and half_sizes [n, 3] f32, both NULL or both set (ignore_outside_occ:
 *   a cell outside -half <= xyz <= half, bounds inclusive, is predicted empty).
 * Predicted occupied: 1 / (1 + exp(-logit)) > pos_thresh in f32 (ATen's sigmoid; NaN is empty).
 * Adds (inter, union) of RoI i to counts[row0 + i, 0:2] of an int64 [rows, 2] device buffer (zeroed by the caller
 *   once per tracklet): ballots + popcounts per wave, one 64-bit vector atomic per wave, RoI and count.
 * ------------------------------------------------------------------------ */
int ococc_occ_iou_count(const float* logits, const int64_t* labels, const float* roi_xyz, const float* half_sizes,
                        int32_t n, int64_t K, float pos_thresh, int64_t* counts, int64_t row0, int64_t rows,
                        ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * sample masks of the train_cfg variants of OccBBoxHead.loss_occ (csrc/occ_loss_masks.hip), replacing the ATen chains of
 *   mmdet3d/models/roi_heads/bbox_heads/ococc_bbox_head.py:706-710 (zeros_like, masked assignment, view, repeat),
 *   :713-722 (no_loss_for_outside: neg, div, two compares, two all, &, float, *), :730-734 (no_loss_for_observed_feats:
 *   get_cls_from_pred, ==, float, *), :749-753 (residual_loss: get_cls_from_pred, !=, sum) and :792 (weights > 0).
 * Row i * K + k is sample k of positive RoI i.  xyz [M * K, 3] f32 the sample in the RoI frame; box_size [M, 3] f32
 * (rois[pos][:, 4:7]); score [M] f32 the label confidence; ori_logits [M * K] f32 the decoder's logits of
 * ori_roi_feats (cls_dim 1); labels [M * K] int64 (occupied: == 1).  flags: 1 outside | 2 observed | 4 unmatched;
 * xyz / box_size are read only with 1, ori_logits only with 2 or 4, labels only with 4 (NULL otherwise).
 *   weights [M * K] f32 = (score[i] > score_thresh)            strict; NaN is 0
 *       [1] * (-size / 2 <= xyz <= size / 2 on all three axes)   f32 compares, bounds inclusive, a NaN coordinate is outside
 *       [2] * (class of ori_logits == 0)
 *   unmatched [M * K] u8 = (labels == 1) != (class of ori_logits)   written only with flag 4
 *   counts [3] int64 (zeroed here): #(weights > 0), #unmatched, #(unmatched and weights > 0); the last two 0 without 4
 * class = 1 / (1 + exp(-logit)) > pos_thresh in f32 (ATen's sigmoid; NaN is class 0), the device function of
 * ococc_occ_iou_count.  16-byte loads and stores when every pointer is 16-byte aligned, element-wise ones otherwise.
 * Ballots + popcounts per wave, one 64-bit vector atomic per wave and count; integer sums only: the same input gives
 * the same bytes.  M == 0 or K == 0: no launch, counts zero.  One grid pass covers ococc_occ_loss_masks_pass_rows()
 * rows; more rows take further trips of the grid-stride loop.
 * ------------------------------------------------------------------------ */
int64_t ococc_occ_loss_masks_pass_rows(void);
int ococc_occ_loss_masks_f32(const float* xyz, const float* box_size, const float* score, const float* ori_logits,
                             const int64_t* labels, int64_t M, int64_t K, float score_thresh, float pos_thresh,
                             int32_t flags, float* weights, uint8_t* unmatched, int64_t* counts, ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * completed-occupancy export (csrc/occ_export.hip): the dense-grid decode around the decoder and the compaction of its
 * occupied cells, behind OccDecoder.get_occ_packed and TrackletRoIHeadOCC.save_occ_from_tracklet
 *   (mmdet3d/models/roi_heads/tracklet_roi_head_occ.py:612-745).
 * The cells of R RoIs are one flat list, RoI after RoI, x slowest and z fastest inside an RoI:
 *   sizes [R, 3] f32 the enlarged box sizes, dims [R, 3] i32 = ceil(size / voxel_size) (fewer than 2^31 cells per RoI),
 *   start [R + 1] i64 the exclusive prefix of dims.prod(1) (start[0] = 0, start[R] = n cells).
 * The centre of cell c of an axis is (c * voxel_size + (-size / 2)) + voxel_size / 2, each operation rounded to f32 on
 * its own (no fused multiply-add): bit for bit what the ATen chain gives.  R == 0 is an empty result, not an error.
 *
 * ococc_dense_grid_cells_f32 replaces generate_dense_voxel_centers (mmdet3d/ops/occ/occ_ops.py:5-50) and the per-box
 *   feature repeat of get_occ (mmdet3d/models/occ/occ_base.py:300-308) for the cells [lo, hi) of the list:
 *   centers [hi - lo, 3] f32 and roi_index [hi - lo] i32 (the add_index of ococc_occ_mlp_fwd_bf16).  One launch.
 *
 * ococc_occ_select_count replaces the sigmoid / compare / bincount of get_occ (occ_base.py:310-327) on logits [n] f32 of
 *   the one-logit decoder.  The list is cut into tiles of 1024 consecutive cells of one RoI (never two RoIs in a tile):
 *   it writes tile_start [R + 1] i64, the exclusive prefix of ceil(cells / 1024) per RoI (derived from start by a
 *   one-wave launch in front), tile_counts [max_tiles] i32 (occupied cells per tile; 0 behind the last tile) and
 *   roi_counts [R] i64 (zeroed here).  max_tiles >= ococc_occ_select_max_tiles(n, R) = n / 1024 + R, known without
 *   reading the device.  Occupied: 1 / (1 + exp(-logit)) > pos_thresh in f32 (ATen's sigmoid; NaN is empty), the same
 *   device function as ococc_occ_iou_count.  Integer atomics only.
 *
 * ococc_occ_select_fill replaces the boolean index and the transform of get_occ (occ_base.py:312-336): given tile_scan
 *   [max_tiles] i64, the exclusive prefix of tile_counts, it writes the occupied cells in cell order to
 *   out [n_out, cols] f32 (n_out = sum of roi_counts; rows past n_out are not written).  Columns 0-2: the cell centre in
 *   the box frame, or with to_lidar in the LiDAR frame: x' = x c + y s, y' = -x s + y c, then + the box centre
 *   (rois[r, 1:4]), then z + rois[r, 6] / 2, each operation rounded on its own; rois are rows of roi_stride >= 7 floats
 *   (batch, x, y, z_bottom, w, l, h, yaw, ...), cos_yaw / sin_yaw [R] the caller's cos / sin of the yaw (no
 *   trigonometric function is evaluated here).  cols == 4 adds roi_value[r] when roi_value [R] is given (the per-frame
 *   box score save_occ_from_tracklet pads with, :732-737), else sigmoid(logit); out is then 16-byte aligned.
 *   Ballots and popcounts keep the order (the idiom of ococc_tracklet_crop_fill); no atomics.
 * ------------------------------------------------------------------------ */
int ococc_dense_grid_cells_f32(const float* sizes, const int32_t* dims, const int64_t* start, int32_t R,
                               float voxel_size, int64_t lo, int64_t hi, float* centers, int32_t* roi_index,
                               ococc_stream_t stream);
int64_t ococc_occ_select_max_tiles(int64_t n, int32_t R);
int ococc_occ_select_count(const float* logits, int64_t n, const int64_t* start, int32_t R, float pos_thresh,
                           int64_t* tile_start, int32_t* tile_counts, int64_t max_tiles, int64_t* roi_counts,
                           ococc_stream_t stream);
int ococc_occ_select_fill(const float* logits, int64_t n, const int64_t* start, const int64_t* tile_start, int32_t R,
                          float pos_thresh, const int64_t* tile_scan, int64_t max_tiles, const float* sizes,
                          const int32_t* dims, float voxel_size, int32_t to_lidar, const float* rois,
                          int64_t roi_stride, const float* cos_yaw, const float* sin_yaw, const float* roi_value,
                          int32_t cols, float* out, int64_t n_out, ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * completed occupancy of one online step (csrc/occ_frame.hip): the cells the decoder predicts occupied joined with the
 * cells the sensor hit in this frame, behind occ_ops.occ_frame_select, OccDecoder.get_frame_occ and the ``occ=True``
 * results of TrackletRoIHeadOCC.simple_test_step / simple_test_steps / simple_test_scene_step.  The flat cell list
 * (sizes, dims, start), its tiles of 1024 cells of one RoI and ococc_occ_select_max_tiles are those of the export above.
 *
 * ococc_occ_frame_mark replaces the rasterisation of OccAutoEncoder.sample_observation
 *   (mmdet3d/models/roi_heads/bbox_heads/occ_ae_head.py:65-126 with quantize_points, mmdet3d/ops/occ/occ_ops.py:53-93):
 *   local_xyz [M, 3] f32 the pooled points in the box frame (after the compensate_encoder_coors turn), pts_roi [M] i32
 *   the RoI of each.  Per axis floor((p - (-size / 2)) / voxel_size) in f32, each operation rounded on its own, the
 *   quotient a true division; a point whose index is < 0 or >= dim on any axis, whose coordinate is NaN or whose RoI
 *   is outside [0, R) marks nothing.  observed [n] u8 (n = start[R]) is zeroed here, then 1 where a point fell into
 *   the cell: byte stores of one value, no atomic.  M == 0: the memset only.
 *
 * ococc_occ_frame_count / ococc_occ_frame_fill replace the sigmoid / compare / boolean index / transform of get_occ
 *   (mmdet3d/models/occ/occ_base.py:238-342) for the union of prediction and observation.  A cell is selected when
 *   (1 / (1 + exp(-logit)) > pos_thresh or observed[cell] != 0) and row_keep[RoI] != 0; observed NULL: no observation;
 *   row_keep [R] u8 NULL: every RoI kept (test_cfg.filter_empty_roi without a host decision).
 *   count writes tile_start [R + 1] i64, tile_counts [max_tiles] i32 and roi_counts [R] i64 (zeroed here) as
 *   ococc_occ_select_count does.  fill, given tile_scan [max_tiles] i64 the exclusive prefix of tile_counts, writes per
 *   selected cell, in cell order, out [n_out, 4] f32 (16-byte aligned, one 16-byte store per row) and flags [n_out] u8:
 *     columns 0-2 the cell centre in the LiDAR frame by the arithmetic of ococc_occ_select_fill with to_lidar (rois rows
 *     of roi_stride >= 7 floats, cos_yaw / sin_yaw [R] the caller's), then with transforms [R, 12] f32 (row-major 3x4,
 *     NULL: none) x' = ((t0 x + t1 y) + t2 z) + t3 and likewise y', z', each operation rounded once;
 *     column 3 the sigmoid of the logit; flags bit 0 predicted, bit 1 observed.
 *   With transforms NULL and nothing observed the xyz columns are those of ococc_occ_select_fill bit for bit.
 * Integer atomics only; the same input gives the same bytes.  R == 0 or n == 0 is an empty result, not an error.
 * ------------------------------------------------------------------------ */
int ococc_occ_frame_mark(const float* local_xyz, const int32_t* pts_roi, int64_t M, const float* sizes,
                         const int32_t* dims, const int64_t* start, int32_t R, float voxel_size, uint8_t* observed,
                         int64_t n, ococc_stream_t stream);
int ococc_occ_frame_count(const float* logits, const uint8_t* observed, const uint8_t* row_keep, int64_t n,
                          const int64_t* start, int32_t R, float pos_thresh, int64_t* tile_start, int32_t* tile_counts,
                          int64_t max_tiles, int64_t* roi_counts, ococc_stream_t stream);
int ococc_occ_frame_fill(const float* logits, const uint8_t* observed, const uint8_t* row_keep, int64_t n,
                         const int64_t* start, const int64_t* tile_start, int32_t R, float pos_thresh,
                         const int64_t* tile_scan, int64_t max_tiles, const float* sizes, const int32_t* dims,
                         float voxel_size, const float* rois, int64_t roi_stride, const float* cos_yaw,
                         const float* sin_yaw, const float* transforms, float* out, uint8_t* flags, int64_t n_out,
                         ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * occupancy-enhanced scene cloud (csrc/occ_merge.hip): the frame's cloud followed by the completed-occupancy cells that
 * pass the score test, behind occ_ops.occ_merge and the ``merged=`` result of TrackletRoIHeadOCC.simple_test_scene_step.
 * Replaces, for a cloud and cells already on the device, the column slice, `occ_points[:, -1] > score_threshold`, the
 * np.pad calls and the np.concatenate of LoadPointsAndOccPredFromFile.__call__ and LoadOccPredFromFile.__call__
 *   (mmdet3d/datasets/pipelines/occ_pinelines.py:639-694 and :757-805).
 * points [N, C] f32 row-major, the scene cloud.  host_use_dim: a HOST array of D column indices, 3 <= D <= 16, each in
 *   [0, C), repeats allowed, the first three taken as x, y, z; checked here, passed to the kernel by value.
 * occ [M, 4] f32 (x, y, z, value), the packed rows of ococc_occ_frame_fill; start [R + 1] i64 on the device, the
 *   exclusive prefix of the cells per row: cell m belongs to row r with start[r] <= m < start[r + 1].
 * The score of a cell is row_score[r] (row_score [R] f32), or with row_score NULL column 3 of the cell (what the
 *   exported files carry there).  A cell survives iff score > score_threshold in f32 -- strict; a NaN score never
 *   survives -- and, with flags [M] u8 given and drop_observed != 0, (flags[m] & 2) == 0 (no real point fell into it).
 * Tiles: 1024 consecutive cells of one row, at most ococc_occ_select_max_tiles(M, R) of them, one wave per tile.
 * ococc_occ_merge_count checks start on the device in a one-wave launch of its own: start[r] >= 0,
 *   start[r] <= start[r + 1], start[R] <= M.  A table that fails is not read through: tile_start = 0, no tile runs and
 *   row_counts [R] i64 = -1 (the caller reports it after its read-back, as with ococc_tune_sample_count).  Otherwise it
 *   writes tile_start [R + 1] i64, tile_counts [max_tiles] i32 (0 for the unused tail) and row_counts, the survivors
 *   per row (one integer atomic per tile).
 * ococc_occ_merge_fill: given tile_scan [max_tiles] i64, the exclusive prefix of tile_counts, and K, their sum, writes
 *   merged [N + K, D + 2] f32 in ONE launch with two block roles:
 *     row i < N: points[i, host_use_dim[j]] for j < D, then 0.0f, 0.0f;
 *     row N + k: the k-th survivor in input order: its x, y, z, 0.0f for the D - 3 other attributes, its score, 1.0f.
 *   One thread per output element.  Every value is copied as a 32-bit word: a NaN or denormal passes bit for bit.
 *   K == 0 (or M == 0, R == 0): the real rows only, nothing of occ / start / tile_scan is read.
 * N == 0, M == 0 and R == 0 are empty parts, not errors.  Integer atomics only; the same input gives the same bytes.
 * ------------------------------------------------------------------------ */
int ococc_occ_merge_count(const float* occ, int64_t M, const int64_t* start, int32_t R, const float* row_score,
                          const uint8_t* flags, int32_t drop_observed, float score_threshold, int64_t* tile_start,
                          int32_t* tile_counts, int64_t max_tiles, int64_t* row_counts, ococc_stream_t stream);
int ococc_occ_merge_fill(const float* points, int64_t N, int32_t C, const int32_t* host_use_dim, int32_t D,
                         const float* occ, int64_t M, const int64_t* start, const int64_t* tile_start, int32_t R,
                         const float* row_score, const uint8_t* flags, int32_t drop_observed, float score_threshold,
                         const int64_t* tile_scan, int64_t max_tiles, float* merged, int64_t K, ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * occupancy-enhanced scene clouds of SEVERAL frames in one call (csrc/occ_merge.hip, the kernels of the pair above with a
 * frame table), behind occ_ops.occ_merge_frames and TrackletRoIHeadOCC.simple_test_scene_steps_merged: what F calls of
 * ococc_occ_merge_count / _fill write, frame after frame in one array, with one table, one count and one fill launch and
 * one read-back for any F.
 * points [N, C] f32: the F clouds back to back; cloud_start [F + 1] i64 their exclusive prefix (0 ... N).
 * occ [M, 4], start [R + 1], row_score [R], flags [M], drop_observed, score_threshold, host_use_dim, D and the survival
 *   rule: those of the pair above.  The R rows are in the CALLER's order (slot-major in a chunked step), not by frame.
 * row_frame [R] i64: the frame 0..F-1 of every row.  order [R] i64: the rows sorted by frame, stable (a frame's rows
 *   keep the caller's order); frame_first [F + 1] i64: where the rows of frame f begin in order (0 ... R).  All five
 *   tables are on the device; the caller builds them on the host and may send them up in one copy.  0 <= F <= 65535;
 *   F == 0 needs R == 0 and N == 0.
 * Tiles are laid out along the order: tile_start [R + 1] i64 is the prefix of ceil(cells / 1024) of row order[p], so
 *   tile_scan, the exclusive prefix of tile_counts, ranks a survivor among the survivors of the whole call, frame major.
 * ococc_occ_merge_frames_count checks, in its one-wave launch: start as above; order[p] in [0, R); row_frame[r] in
 *   [0, F) and non-decreasing along the order, with frame_first[f] <= p < frame_first[f + 1] for f = row_frame[order[p]];
 *   cloud_start ascending from 0 to N; frame_first ascending from 0 to R.  A failed check: tile_start = 0, no tile runs,
 *   row_counts [R] = -1 (reported by the caller after its read-back).  Otherwise row_counts[r] is the survivors of row
 *   r, in the caller's row order.
 * ococc_occ_merge_frames_fill writes merged [N + K, D + 2] f32, K the sum of tile_counts, in one launch.  With S_f the
 *   survivors of the frames before f -- taken on the device from tile_scan at the first tile of frame f, K past the last
 *   tile; nothing is uploaded after the read-back -- segment f begins at row cloud_start[f] + S_f and holds
 *     the rows of cloud f: points[i, host_use_dim[j]] for j < D, then 0.0f, 0.0f;
 *     then the survivors of the rows r with row_frame[r] == f, r ascending, a row's cells in input order: x, y, z,
 *     0.0f for the D - 3 other attributes, the score, 1.0f.
 *   Segment f is byte for byte what ococc_occ_merge_fill writes for cloud f and the cells of its rows.  Every index
 *   taken from a table is clamped: a wrong table reads nothing outside [0, M) and [0, N) and writes inside merged.
 *   K == 0 (or M == 0, R == 0): the real rows only, no table is read.
 * Integer atomics only; the same input gives the same bytes.
 * ------------------------------------------------------------------------ */
int ococc_occ_merge_frames_count(const float* occ, int64_t M, const int64_t* start, const int64_t* order,
                                 const int64_t* row_frame, int32_t R, const int64_t* cloud_start,
                                 const int64_t* frame_first, int32_t F, int64_t N, const float* row_score,
                                 const uint8_t* flags, int32_t drop_observed, float score_threshold,
                                 int64_t* tile_start, int32_t* tile_counts, int64_t max_tiles, int64_t* row_counts,
                                 ococc_stream_t stream);
int ococc_occ_merge_frames_fill(const float* points, int64_t N, int32_t C, const int32_t* host_use_dim, int32_t D,
                                const float* occ, int64_t M, const int64_t* start, const int64_t* order,
                                const int64_t* row_frame, const int64_t* tile_start, int32_t R,
                                const int64_t* cloud_start, const int64_t* frame_first, int32_t F,
                                const float* row_score, const uint8_t* flags, int32_t drop_observed,
                                float score_threshold, const int64_t* tile_scan, int64_t max_tiles, float* merged,
                                int64_t K, ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * observation sample of one online step (csrc/tune_sample.hip): the rows the shape latent of a step is tuned against,
 * behind occ_ops.tune_sample and the ``tune=`` argument of OccBBoxHead.forward_step / forward_steps.  Replaces, for the
 * step, OccAutoEncoder.sample_observation with balance_sample and its cap
 *   (mmdet3d/models/roi_heads/bbox_heads/occ_ae_head.py:65-201: the label volume per RoI, torch.multinomial per RoI for
 *   the free cells and again for downsample_size).
 * The flat cell list (start [K + 1] i64, sizes, dims) is that of the exports above and observed [n] u8 is what
 * ococc_occ_frame_mark wrote.  Random numbers are integers: mix64 the splitmix64 finaliser,
 *   key(s, c) = high 32 bits of mix64(s + (c + 1) * 0x9E3779B97F4A7C15); cell c of a RoI with seed s = row_seeds[r]
 *   carries key(s, c), position p of the RoI's list carries key(s ^ 0xD1B54A32D192ED03, p); every order is on
 *   (key, index), equal keys towards the smaller index.
 * Rows of RoI r with k cells, npos of them observed, nneg = k - npos (row_keep [K] u8, NULL: every RoI kept):
 *   row_keep[r] == 0: none.  balance == 0: every cell, label = observed (cap must be <= 0).  npos == 0: cell 0 with
 *   label 0.  nneg == 0: none.  npos <= nneg: the observed cells and the npos free cells of smallest (key, c).
 *   npos > nneg > 0: the observed cells, every free cell npos / nneg times, the npos % nneg free cells of smallest
 *   (key, c) once more.  Rows in grid order, copies adjacent; cap > 0 and more than cap rows: the cap rows of smallest
 *   (cap key, position), still in list order.
 * ococc_tune_sample_count writes counts [K] i32 (-1: start is no ascending table inside [0, n], or a RoI has more than
 *   2^30 cells) and plan [K, 4] i64 (the case and the two thresholds, for fill).  ococc_tune_sample_fill, given both,
 *   writes S = sum of the counts rows: xyz [S, 3] f32 the cell centre (bit for bit ococc_dense_grid_cells_f32),
 *   labels [S] i32, index [S] i32 non-decreasing, weights [S] f32 = 1.0f / (float)counts[r], one rounded division.
 * Integer atomics in LDS only; the same input gives the same bytes.  K == 0 is an empty result, not an error.
 * ------------------------------------------------------------------------ */
int ococc_tune_sample_count(const uint8_t* observed, int64_t n, const int64_t* start, int32_t K,
                            const int64_t* row_seeds, const uint8_t* row_keep, int32_t balance, int32_t cap,
                            int32_t* counts, int64_t* plan, ococc_stream_t stream);
int ococc_tune_sample_fill(const uint8_t* observed, int64_t n, const int64_t* start, int32_t K, const float* sizes,
                           const int32_t* dims, float voxel_size, const int64_t* row_seeds, const int32_t* counts,
                           const int64_t* plan, float* xyz, int32_t* labels, int32_t* index, float* weights, int64_t S,
                           ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * ground-truth occupancy export (csrc/gt_occ_crop.hip): the occupied label cells of one object, moved into the LiDAR
 * frame of every frame that has a GT box and cropped to that frame's proposal box, behind bbox.crop_gt_occ_packed and
 * TrackletRoIHeadOCC.save_gt_occ_from_tracklet.  Replaces the save_gt_occ=True branch of save_occ_from_tracklet
 *   (mmdet3d/models/roi_heads/tracklet_roi_head_occ.py:634-702: the [N, K, 3] repeat, rotation_3d_in_axis, the three
 *   in-place adds of :661-670, points_in_boxes_gpu and the boolean index per frame of :681-689) and check_pt_in_box3d
 *   (mmdet3d/ops/roiaware_pool3d/src/points_in_boxes_cuda.cu:24-49).
 * cells [K, 3] f32: gravity centres in the GT box frame.  gt_boxes / roi_boxes: N rows of gt_stride / roi_stride >= 7
 * floats (x, y, z_bottom, w, l, h, yaw).  cos_gt / sin_gt [N]: the caller's cos / sin of the GT yaw; cos_roi / sin_roi
 * [N]: of float((double)roi_yaw + pi / 2), the .cu's rot_angle.  No trigonometric function is evaluated here.
 * Pair n * K + k is (frame n, cell k).  Per pair, every operation rounded to f32 on its own (no fused multiply-add):
 *   x' = (x c + y s) + gt_x, y' = (-x s + y c) + gt_y, z' = (z + gt_z) + gt_h / 2;
 *   kept unless |z' - (roi_z + roi_h / 2)| > roi_h / 2 (a cell on the top or bottom face is kept), and if
 *   -l / 2 < dx cosa + dy (-sina) < l / 2 and -w / 2 < dx sina + dy cosa < w / 2 with (dx, dy) = (x' - roi_x, y' - roi_y),
 *   all four strict (a cell on a side face is dropped).
 * Tiles: 1024 consecutive pairs of one frame, ococc_gt_occ_crop_tiles(N, K) = N * ceil(K / 1024) of them (host
 * arithmetic; every frame has K cells, so tile t is frame t / ceil(K / 1024) and no table is read).  One wave per tile,
 * one ballot per 64 pairs.
 * ococc_gt_occ_crop_count writes tile_counts [tiles] i32 and frame_counts [N] i64 (zeroed here; integer atomics only).
 * ococc_gt_occ_crop_fill: given tile_scan [tiles] i64, the exclusive prefix of tile_counts, writes the kept cells in
 *   frame order and ascending cell order inside a frame to out [n_out, 4] f32 (16-byte aligned; n_out = sum of
 *   frame_counts, rows past it are not written): x', y', z' recomputed, and value[n] (1 when value is NULL).
 * N == 0 or K == 0 is an empty result, not an error.  No float atomics: the same input gives the same bytes.
 * ------------------------------------------------------------------------ */
int64_t ococc_gt_occ_crop_tiles(int64_t N, int64_t K);
int ococc_gt_occ_crop_count(const float* cells, int64_t K, const float* gt_boxes, int64_t gt_stride,
                            const float* roi_boxes, int64_t roi_stride, int64_t N, const float* cos_gt,
                            const float* sin_gt, const float* cos_roi, const float* sin_roi, int32_t* tile_counts,
                            int64_t tiles, int64_t* frame_counts, ococc_stream_t stream);
int ococc_gt_occ_crop_fill(const float* cells, int64_t K, const float* gt_boxes, int64_t gt_stride,
                           const float* roi_boxes, int64_t roi_stride, int64_t N, const float* cos_gt,
                           const float* sin_gt, const float* cos_roi, const float* sin_roi, const int64_t* tile_scan,
                           int64_t tiles, const float* value, float* out, int64_t n_out, ococc_stream_t stream);

/* ------------------------------------------------------------------------
 * A12 glue, one launch each (f32; the element-wise chains they replace were 12-35 launches of a few hundred elements):
 * ococc_rotate_z_f32: rotation_3d_in_axis(points [n, m, 3], angles [n], axis=2)
 *   (mmdet3d/core/bbox/structures/utils.py:21-61; the reference's transposed-matrix convention: x' = x c + y s, y' = -x s + y c).
 * ococc_points_box_to_box_f32: points [n, m, 3] given in the frame of from_boxes[i] (gravity centred) -> the frame of
 *   to_boxes[i]: rotate by yaw_from, + centre_from, z + h_from / 2, - centre_to, z - h_to / 2, rotate by -yaw_to
 *   (ococc_bbox_head.py:1279-1290, 714-724; boxes are rows of ld >= 7 floats: x, y, z_bottom, w, l, h, yaw).
 * ococc_roi_box_targets_f32: GT boxes in the canonical frame of their RoIs -> DeltaXYZWLHRBBoxCoder deltas [n, 7]
 *   (ococc_bbox_head.py:1190-1222, delta_xyzwhlr_bbox_coder.py:21-50). */
int ococc_rotate_z_f32(const float* points, const float* angles, int64_t n, int64_t m, float* out, ococc_stream_t stream);
int ococc_points_box_to_box_f32(const float* points, const float* from_boxes, int64_t ld_from, const float* to_boxes,
                                int64_t ld_to, int64_t n, int64_t m, float* out, ococc_stream_t stream);
int ococc_roi_box_targets_f32(const float* rois, int64_t ld_rois, const float* gt_boxes, int64_t ld_gt, int64_t n, float* out,
                              ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * B6  in-group ranks of integer keys (SST window bookkeeping)
 * replaces TorchEx ingroup_indices.forward (mmdet3d/ops/sst/sst_ops.py:243-263; python twin
 * get_inner_win_inds_deprecated :194-241) and make_continuous_inds (:316-330).
 * keys [n] int32 in [0, key_bound) (negative keys are skipped: conti = inner = -1).
 * conti [n]: rank of the key among the distinct keys; inner [n]: number of earlier elements
 * with the same key (stable); counts [>= num_groups] (buffer of n ints, may be NULL);
 * num_groups, status (1 if a key >= key_bound was seen): device int32.
 * ------------------------------------------------------------------------ */
int64_t ococc_group_rank_workspace_bytes(int64_t n, int64_t key_bound);
int ococc_group_rank_i32(const int32_t* keys, int64_t n, int64_t key_bound, int32_t* conti, int32_t* inner,
                         int32_t* counts, int32_t* num_groups, int32_t* status, void* workspace,
                         int64_t workspace_bytes, ococc_stream_t stream);

/* ------------------------------------------------------------------------ *
 * B7  window attention core  out = softmax(q k^T * scale + key mask) v  per (window, head)
 * replaces the attention inside nn.MultiheadAttention as WindowAttention calls it on padded
 * [num_windows, max_tokens, C] tensors (mmdet3d/models/sst/sst_basic_block_v2.py:41-75).
 * q, k, v: bf16 rows with the given row strides (elements), head h in columns [16h, 16h+16);
 * key_len [num_windows] int32 = valid tokens (a prefix) of each window; out bf16 like q;
 * lse [num_windows, num_heads, max_tokens] f32 (log-sum-exp of the scaled scores, saved for
 * backward).  head_dim must be 16, max_tokens <= 160.
 *
 * Layout.  token_index == NULL: padded, the row of window slot t is window * max_tokens + t.
 * Otherwise flat: q/k/v/out (and dout, dq/dk/dv) are [num_tokens, .] tensors in the model's token
 * order and token_index [num_windows * max_tokens] int32 names the row of every window slot (-1 =
 * padding; valid slots are a prefix of each window, key_len of them).  The kernel gathers a
 * window's tokens itself and writes every output row exactly once, so the padded [nW, T, C] copies
 * that flat2window / window2flat build in the reference (sst_ops.py:66-148) never exist.  lse
 * stays [nW, H, T] in both layouts.
 *
 * Dropout: nn.MultiheadAttention(dropout=dropout_p) as SST's WindowAttention builds it
 * (mmdet3d/models/sst/sst_basic_block_v2.py:16-35, 79-81; CosineMultiheadAttention, cosine_msa.py:181-182, 431-433).
 * dropout_p in [0, 1); seed is a device pointer to one uint64 (required when dropout_p > 0, may be NULL otherwise; read
 * by the kernel, so a captured graph that redraws it draws a new mask per replay).  After the key mask and the softmax a
 * probability is kept iff hash24(seed, head, query row, key row) >= floor(dropout_p * 2^24) and then scaled by
 * 1 / (1 - dropout_p) in f32, rounded to bf16 as the P V operand; rows are the rows of the layout above (token_index
 * rows, or window * max_tokens + slot).  lse stays that of the undropped softmax; the backward regenerates the mask
 * (dV = P_drop^T dO, dS = P o (keep dP / (1 - p) - delta), delta = dO . O).  dropout_p = 0 runs no mask at all.
 * ------------------------------------------------------------------------ */
int ococc_window_attn_fwd_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t q_stride,
                               int64_t k_stride, int64_t v_stride, const int32_t* token_index,
                               const int32_t* key_len, int64_t num_windows, int32_t max_tokens,
                               int32_t num_heads, int32_t head_dim, float scale, uint16_t* out,
                               int64_t out_stride, float* lse, float dropout_p, const uint64_t* seed,
                               ococc_stream_t stream);
int ococc_window_attn_bwd_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t q_stride,
                               int64_t k_stride, int64_t v_stride, const uint16_t* out, const uint16_t* dout,
                               int64_t o_stride, const float* lse, const int32_t* token_index,
                               const int32_t* key_len, int64_t num_windows, int32_t max_tokens,
                               int32_t num_heads, int32_t head_dim, float scale, uint16_t* dq, uint16_t* dk,
                               uint16_t* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride,
                               float dropout_p, const uint64_t* seed, ococc_stream_t stream);

/* ------------------------------------------------------------------------
 * B7, fused  one SST encoder layer as two tile kernels per direction
 * replaces EncoderLayer.forward (post-norm, mmdet3d/models/sst/sst_basic_block_v2.py:105-127):
 *   window_attn_block:  y1 = norm1(x + self_attn(q = k = x + pos, v = x))   (WindowAttention.forward :41-75 around
 *                        nn.MultiheadAttention on flat2window_v2 / window2flat_v2 copies, sst_ops.py:66-148)
 *   token_ffn_block:    y2 = norm2(y1 + linear2(act(linear1(y1))))
 * d_model 128, 8 heads of 16, feed-forward 256; tokens bf16 [num_tokens, 128] in the model's flat order; all sums f32.
 *
 * Weights arrive as MFMA A-operand fragments: ococc_linear_fragments_bf16 turns f32 matrices S (rows x cols, any
 * element strides -- a transposed view is just swapped strides) into bf16 [rows/16][cols/32][64 lanes][8]:
 * lane 16 g + r of block (rb, cs) holds S[16 rb + r][32 cs + 8 g .. + 7].  For y = x W^T pass W ([out, in] as
 * nn.Linear stores it); for the input gradient dx = dy W pass W^T (rows = in, cols = out).
 *
 * Windows -> tiles: ococc_window_tile_plan packs whole windows (win_len[w] <= 64 tokens, their flat rows at
 * tok[win_off[w] .. + win_len[w])) greedily, in the given order, into tiles of 64 token slots: tile_rows [tiles*64]
 * = flat row of the slot or -1, tile_span [tiles*64] = lo | hi << 8, the slots of the slot's window (0: empty).
 * cap_tiles >= num_windows rows of both arrays are initialised; *num_tiles (device) receives the tiles in use.
 * A slot attends exactly the slots of its span: the key_padding_mask of the reference is the span.
 *
 * Backward kernels recompute their block from its input (nothing else is saved by the forward) and also write the
 * operands of the weight gradients -- attention block: dqkv [*,384] (gradients of q | k | v), attn_out [*,128] (input
 * of out_proj), dz [*,128] (gradient at norm1's input = gradient of out_proj's output); FFN block: act_out [*,256]
 * (input of linear2), dh [*,256] (gradient of linear1's output), dz [*,128] (gradient of linear2's output) -- and one
 * row [dgamma(128) | dbeta(128)] f32 of LayerNorm parameter-gradient partial sums per persistent workgroup
 * (ln_partial: ococc_window_block_partial_rows(tiles) rows; an FFN block has ceil(num_tokens / 64) tiles).
 * dx includes the residual path.  No atomics: bit-reproducible.
 * All four kernels run as persistent workgroups that keep the block's weight fragments in registers.
 * ------------------------------------------------------------------------ */
int ococc_linear_fragments_bf16(int32_t count, const void* const* host_src, const int64_t* host_rows,
                                const int64_t* host_cols, const int64_t* host_row_stride, const int64_t* host_col_stride,
                                void* const* host_dst, ococc_stream_t stream);
int64_t ococc_window_tile_plan_workspace_bytes(int64_t num_windows);
int64_t ococc_window_block_partial_rows(int64_t num_tiles);
int ococc_window_tile_plan(const int32_t* win_len, const int64_t* win_off, const int32_t* tok, int64_t num_windows,
                           int32_t tile_slots, int64_t cap_tiles, int32_t* tile_rows, int32_t* tile_span,
                           int32_t* num_tiles, void* workspace, int64_t workspace_bytes, ococc_stream_t stream);
/* Attention block.  Inference: attn_save = lse_save = NULL.  A training step that keeps the attention output and the
 * softmax's log-sum-exp (round 5) passes both, 16-byte aligned: the forward also writes attn_save [num_tokens, d_model]
 * bf16 (rows of the plan's tokens) and lse_save [num_tokens, num_heads] f32, and the backward, given attn_saved /
 * lse_saved and attn_out = NULL, reads them back instead of running the attention forward again (28 % of its time, for
 * 288 B per token) and no longer writes attn_out -- the weight gradient of the out-projection reads attn_saved.  Without
 * them (attn_saved = lse_saved = NULL) the backward recomputes the attention and writes attn_out; exactly one of the two
 * forms must be given.  Same results either way (the attention forward it skips is deterministic).
 *
 * Dropout: the attention of EncoderLayer with its reference default dropout=0.1 (sst_basic_block_v2.py:79-81, 133 ->
 * nn.MultiheadAttention(dropout=...) / CosineMultiheadAttention, cosine_msa.py:181-182).  dropout_p and seed as for
 * ococc_window_attn_fwd_bf16; the mask is that of the window-attention calls over the flat rows of tile_rows -- the gather
 * kernels and these make the same decision for the same (seed, head, query row, key row).  lse_save stays the
 * log-sum-exp of the undropped softmax; attn_save / attn_out is the dropped attention output (the out-projection's
 * input).  dropout_p = 0 runs no mask at all. */
int ococc_window_attn_block_fwd_bf16(const uint16_t* x, const uint16_t* pos, const int32_t* tile_rows,
                                     const int32_t* tile_span, int64_t num_tiles, int32_t d_model, int32_t num_heads,
                                     const uint16_t* wqkv_frag, const float* bqkv, const uint16_t* wo_frag,
                                     const float* bo, const float* ln_weight, const float* ln_bias, float eps,
                                     uint16_t* y, uint16_t* attn_save, float* lse_save, float dropout_p,
                                     const uint64_t* seed, ococc_stream_t stream);
int ococc_window_attn_block_bwd_bf16(const uint16_t* x, const uint16_t* pos, const uint16_t* dy,
                                     const int32_t* tile_rows, const int32_t* tile_span, int64_t num_tiles,
                                     int32_t d_model, int32_t num_heads, const uint16_t* wqkv_frag, const float* bqkv,
                                     const uint16_t* wo_frag, const float* bo, const float* ln_weight, float eps,
                                     const uint16_t* wo_t_frag, const uint16_t* wqkv_t_frag, const uint16_t* attn_saved,
                                     const float* lse_saved, uint16_t* dx, uint16_t* dqkv, uint16_t* dz,
                                     uint16_t* attn_out, float* ln_partial, float dropout_p, const uint64_t* seed,
                                     ococc_stream_t stream);
int ococc_token_ffn_block_fwd_bf16(const uint16_t* x, int64_t num_tokens, int32_t d_model, int32_t d_ffn,
                                   const uint16_t* w1_frag, const float* b1, const uint16_t* w2_frag, const float* b2,
                                   const float* ln_weight, const float* ln_bias, float eps, int32_t act, uint16_t* y,
                                   ococc_stream_t stream);
int ococc_token_ffn_block_bwd_bf16(const uint16_t* x, const uint16_t* dy, int64_t num_tokens, int32_t d_model,
                                   int32_t d_ffn, const uint16_t* w1_frag, const float* b1, const uint16_t* w2_frag,
                                   const float* b2, const float* ln_weight, float eps, int32_t act,
                                   const uint16_t* w2_t_frag, const uint16_t* w1_t_frag, uint16_t* dx,
                                   uint16_t* act_out, uint16_t* dh, uint16_t* dz, float* ln_partial,
                                   ococc_stream_t stream);

/* Weight gradients of token-wise linears (replaces the dW / db that autograd derives for nn.Linear /
 * nn.MultiheadAttention's in_proj in the reference, sst_basic_block_v2.py:41-127): for each of `count` pairs
 *   dW_i[n][k] = sum_t G_i[t][n] X_i[t][k],  db_i[n] = sum_t G_i[t][n]
 * G_i: bf16 [num_tokens, ldg_i] (n_i columns used, n_i a multiple of 64), X_i: bf16 [num_tokens, k_i], k_i 128 or 256;
 * xadd_i (optional): a second bf16 [num_tokens, k_i] operand, rows n < add_rows_i of dW use bf16(X + xadd) (the q | k
 * rows of in_proj see x + pos, the v rows x).  The token range is cut into `slabs` (ococc_token_wgrad_slabs) and every
 * slab leaves f32 partials dw_partial_i [slabs, n_i, k_i], db_partial_i [slabs, n_i];
 * ococc_partial_rows_sum_f32 (dst[c] = sum_r src[r][c], fixed order) finishes them.  No atomics.  Entry i of every
 * host_* table (HOST arrays of `count` entries) describes pair i: host_g[i] = G_i, host_ldg[i] = ldg_i, and so on. */
int64_t ococc_token_wgrad_slabs(int64_t num_tokens);
int ococc_token_wgrad_bf16(int32_t count, const void* const* host_g, const int64_t* host_ldg, const int64_t* host_n,
                           const void* const* host_x, const void* const* host_xadd, const int64_t* host_add_rows,
                           const int64_t* host_k, int64_t num_tokens, int64_t slabs, void* const* host_dw_partial,
                           void* const* host_db_partial, ococc_stream_t stream);
int ococc_partial_rows_sum_f32(int32_t count, const void* const* host_src, const int64_t* host_rows,
                               const int64_t* host_cols, void* const* host_dst, ococc_stream_t stream);

/* ------------------------------------------------------------------------
 * A6, fused  one per-point layer of the SIR encoders:  y = act(LayerNorm(W x)),  x assembled per row as
 *   x = [ a (*) mul (*) colscale | b * bscale | v[inv] ]      (parts with 0 columns are absent)
 * optionally with the segment maximum of y (rows sorted by segment: inv non-decreasing) in the same launch.
 * replaces, per layer: the torch.cat / element-wise products that build the input, DynamicVFELayerV2
 * (Linear(bias=False) -> LN -> GELU, mmdet3d/models/voxel_encoders/utils.py:174-189), scatter_v2(mode='max')
 * (mmdet3d/ops/sst/sst_ops.py:150-181) and voxel_feats[unq_inv] of SIRLayer.forward
 * (mmdet3d/models/voxel_encoders/voxel_encoder.py:764-832), and the layers of rel_mlp (sst_ops.py:333-360).
 * All f32 (the reference runs these layers under force_fp32).  a [rows, lda] (ka columns used), mul [rows, ldm] or
 * null, colscale [ka] or null, b [rows, ldb] (kb columns), v [num_segments, kv], inv [rows] int32;
 * 1 <= ka + kb + kv <= 256, 1 <= n <= 144.  w_frag: ococc_point_mlp_pack_f32 of the Linear's weight [n, k]
 * (ococc_point_mlp_fragment_floats(n, k) floats); wt_frag: the same call on the transposed view (rows k, cols n).
 * ln_weight / ln_bias null: no normalisation.  act: 0 none, 1 GELU (erf), 2 ReLU.
 * fwd: y [rows, n]; seg_max [num_segments, n] or null (filled with -inf, then maxima; every segment must own a row).
 * ococc_point_mlp_segment_argmax: seg_arg [num_segments, n] = smallest row attaining the maximum.
 * bwd (recomputes the layer): dy [rows, n] or null, d_seg_max + seg_arg or null ->
 *   dz [rows, n] (gradient at the Linear's output), x_cat [rows, k] or null (the assembled input: dW = dz^T x_cat),
 *   da, dmul [rows, ka], db [rows, kb] (each or null), dv [num_segments, kv] (caller-zeroed, added to with float
 *   atomics at segment-run ends), ln_partial [ococc_point_mlp_tiles(rows), 2, n] (dgamma | dbeta partial sums).
 * ------------------------------------------------------------------------ */
int64_t ococc_point_mlp_fragment_floats(int32_t n, int32_t k);
int64_t ococc_point_mlp_tiles(int64_t rows);
/* rows per workgroup tile of the fwd / bwd launches: 0 = by input size (16 up to 4 k rows, 32 up to 131 k rows, else 64),
 * 16, 32 or 64 pinned (tests); ococc_point_mlp_tiles follows. */
int ococc_point_mlp_force_tile(int32_t tile_rows);
int ococc_point_mlp_pack_f32(const float* w, int32_t n, int32_t k, int64_t row_stride, int64_t col_stride, float* frag,
                             ococc_stream_t stream);
/* the same for up to 32 matrices in one launch (HOST tables) */
int ococc_point_mlp_pack_multi_f32(int32_t count, const void* const* host_w, const int32_t* host_n, const int32_t* host_k,
                                   const int64_t* host_row_stride, const int64_t* host_col_stride, void* const* host_frag,
                                   ococc_stream_t stream);
int ococc_point_mlp_fwd_f32(const float* a, int32_t ka, int32_t lda, const float* mul, int32_t ldm, const float* colscale,
                            const float* b, int32_t kb, int32_t ldb, float bscale, const float* v, int32_t kv,
                            const int32_t* inv, int64_t rows, const float* w_frag, int32_t n, const float* ln_weight,
                            const float* ln_bias, float eps, int32_t act, float* y, float* seg_max, int64_t num_segments,
                            ococc_stream_t stream);
int ococc_point_mlp_segment_argmax(const float* y, const float* seg_max, const int32_t* inv, int64_t rows, int32_t n,
                                   int64_t num_segments, int32_t* seg_arg, ococc_stream_t stream);
/* weight gradient of a layer from the backward call's dz [rows, n] and x_cat [rows, k]: partial [slices][n][k], one
 * product per row slice (slices = ococc_point_mlp_wgrad_slices(rows), <= 64); dW = their sum -- e.g. through
 * ococc_layernorm_param_reduce_multi with the slab read as [slices][2][n k / 2].  Replaces the torch.mm of
 * nn.Linear's backward (voxel_encoders/utils.py:147-189 DynamicVFELayerV2.linear). */
int32_t ococc_point_mlp_wgrad_slices(int64_t rows);
int ococc_point_mlp_wgrad_f32(const float* dz, const float* x_cat, int64_t rows, int32_t n, int32_t k, float* partial,
                              ococc_stream_t stream);
/* The same product for ``count`` (1..8) layers over the same rows in one launch: host_dz[j] [rows, host_n[j]],
 * host_x_cat[j] [rows, host_k[j]], host_partial[j] as above (HOST tables of device pointers and sizes).  (The blocks of one
 * SIR layer's backward.) */
int ococc_point_mlp_wgrad_multi_f32(int32_t count, const float* const* host_dz, const float* const* host_x_cat,
                                    int64_t rows, const int32_t* host_n, const int32_t* host_k, float* const* host_partial,
                                    ococc_stream_t stream);
int ococc_point_mlp_bwd_f32(const float* a, int32_t ka, int32_t lda, const float* mul, int32_t ldm, const float* colscale,
                            const float* b, int32_t kb, int32_t ldb, float bscale, const float* v, int32_t kv,
                            const int32_t* inv, int64_t rows, const float* w_frag, const float* wt_frag, int32_t n,
                            const float* ln_weight, const float* ln_bias, float eps, int32_t act, const float* dy,
                            const float* d_seg_max, const int32_t* seg_arg, float* dz, float* x_cat, float* da,
                            float* dmul, float* db, float* dv, float* ln_partial, ococc_stream_t stream);

/* ------------------------------------------------------------------------
 * A whole SIRLayer per call: SIRLayer.forward (mmdet3d/models/voxel_encoders/voxel_encoder.py:764-832) with LayerNorm
 * blocks and max pooling: the tile bodies of the ococc_point_mlp_* launches above plus the joins between them.
 * Blocks are numbered rel_mlp first, then vfe_layers; block b is Linear(k_b -> n[b], no bias) -> LayerNorm -> act[b]
 * (0 none, 1 GELU, 2 ReLU) with k_b = cluster_cols | n[b-1] (rel), feat_cols (+ cluster_cols) (first vfe), 2 n[b-1] (later
 * vfe).  features [rows, feat_cols] (xyz first), f_cluster [rows, cluster_cols], inv int32 non-decreasing.
 *   fwd: y_out [rows, n[last]] (+ features[:, 3:] when shortcut), groups_out [groups, sum of the vfe widths]; slab: the
 *        intermediates the backward call reads (ococc_sir_layer_fwd_floats floats).
 *   bwd: dy [rows, ld_dy >= n[last]] / d_groups [groups, ld_dgroups >= sum] (row strides in floats: column slices of wider
 *        gradients are read in place; either may be null = zero) -> dfeat [rows, feat_cols] (may be null),
 *        and per block the LayerNorm partial rows [tiles][2][n] and weight-gradient slices [slices][n][k] inside slab at
 *        the offsets ococc_sir_layer_bwd_layout reports (finish with ococc_layernorm_param_reduce_multi).  y_out: the
 *        forward's output when there is no shortcut (it is the last block's y), else unused. */
typedef struct {
  int32_t n_rel, n_vfe;
  int32_t feat_cols, cluster_cols;
  int32_t with_cluster_center, shortcut;
  float bscale;                      /* factor of the f_cluster columns appended to the first vfe block's input */
  int32_t inference;                 /* nonzero: forward only -- the arg-max rows the backward call reads are not recorded */
  const float* rel_colscale;         /* [cluster_cols] scale of the rel_mlp input, or null */
  const float* colscale;             /* [feat_cols] scale of the feature columns, or null */
  int32_t n[8];
  int32_t act[8];
  float eps[8];
  const float* w_frag[8];            /* ococc_point_mlp_pack_f32 of the weight ... */
  const float* wt_frag[8];           /* ... and of its transposed view (backward only) */
  const float* ln_weight[8];
  const float* ln_bias[8];
  const float* gate;                 /* n_rel == 0 only: a gate [rows, feat_cols] computed elsewhere (ococc_sir_rel_chains_*), or null */
  float* dgate;                      /* ... and, for the backward call, where its gradient [rows, feat_cols] goes */
} ococc_sir_layer;
int64_t ococc_sir_layer_fwd_floats(const ococc_sir_layer* layer, int64_t rows, int64_t groups);
int ococc_sir_layer_fwd_f32(const ococc_sir_layer* layer, const float* features, const float* f_cluster, const int32_t* inv,
                            int64_t rows, int64_t groups, float* slab, float* y_out, float* groups_out,
                            ococc_stream_t stream);
int ococc_sir_layer_bwd_layout(const ococc_sir_layer* layer, int64_t rows, int64_t groups, int64_t* host_ln_partial_off,
                               int64_t* host_w_partial_off, int64_t* host_tiles, int32_t* host_slices,
                               int64_t* host_total_floats);
int ococc_sir_layer_bwd_f32(const ococc_sir_layer* layer, const float* features, const float* f_cluster, const int32_t* inv,
                            int64_t rows, int64_t groups, const float* fwd_slab, const float* y_out, const float* dy,
                            int64_t ld_dy, const float* d_groups, int64_t ld_dgroups, float* slab, float* dfeat,
                            ococc_stream_t stream);
/* One launch per layer and direction (+ one for the weight-gradient products): while every row tile has a workgroup of
 * its own (MI355X: up to 896 tiles of 32 rows = 28 k points) and the layer's blocks are one of the shapes of
 * csrc/sir_fused.hpp (rel_mlp of 3 blocks, 2 vfe blocks: every SIRLayer of configs[2]), each of the two calls runs the
 * blocks of a tile back to back in a persistent grid that meets at a grid-wide barrier where the segment maxima
 * (backward: their gradients) cross tiles.  Everything that crosses workgroups inside the launch goes through
 * device-scope atomics; the barrier words live in a per-(device, stream) buffer the library allocates at the first call on
 * a stream (not under stream capture).  Otherwise -- and always after ococc_sir_layer_set_fused(0) -- the same tile
 * bodies run as one launch per block: the same arithmetic, the forward results are equal to the bit.
 * ococc_sir_layer_set_fused(1) takes the one-launch form at any row count (a workgroup then walks several tiles);
 * -1 restores the default (OCOCC_SIR_FUSED=0 in the environment = 0).  A barrier wait is bounded (2 s): instead of
 * hanging the device an incomplete barrier leaves its index + 1 in a sticky device word, which ococc_sir_layer_fused_status
 * reads back (synchronises the stream; 0 = every barrier completed), AND in a host-mapped word that the library reads in
 * front of its next one-launch layer: that call (ococc_sir_layer_fwd_f32 / _bwd_f32) then returns OCOCC_ESTRANDED and every
 * later layer of the process runs as per-block launches.  ococc_sir_layer_fused_check() is the same test without a launch
 * (no synchronisation, no copy: call it wherever the host has waited for the device anyway -- end of a step, a checkpoint).
 * The persistent grid takes at most 7/8 of the workgroups that were resident TOGETHER in a one-off census launch of the same
 * kernel with the same LDS size (never more than hipOccupancyMaxActiveBlocksPerMultiprocessor promises: that API reads high
 * for some register counts) and needs all of its workgroups resident at once: meant for one process per GPU, as the
 * reference trains (tools/dist_train.sh), with ONE such layer in flight per device -- two processes or streams that put
 * such launches of ~a thousand tiles on one device at the same time can starve each other until the bounded wait gives up
 * (ococc_sir_layer_set_fused(0) / OCOCC_SIR_FUSED=0 for that case).
 * ococc_sir_layer_fused_debug(grid, timeout_ms): test hooks -- launch `grid` workgroups whatever the device holds, bound a
 * wait by `timeout_ms`; 0 restores either default, (0, 0) also clears the status words (synchronises the device). */
int ococc_sir_layer_set_fused(int32_t mode);
int ococc_sir_layer_fused_check(void);
int ococc_sir_layer_fused_debug(int32_t grid, int32_t timeout_ms);
/* The rel_mlp chains of several SIRLayers in one launch per direction (the layers of a SIR stack share the cluster
 * offsets their gates are computed from: mmdet3d/models/backbones/sir.py:67-88, ococc_bbox_head.py:237-316).
 * Chain c, block j: y = act(LayerNorm(W x)), x = f_cluster * rel_colscale (j = 0) or the block before (build_mlp,
 * sst_ops.py:333-360); the last block's y is the layer's gate (ococc_sir_layer.gate of a descriptor with n_rel = 0).
 * All chains of a call have the same depth (<= 3 blocks) and cluster_cols; <= 8 chains per call.  Block widths: <= 64
 * output channels, the last block <= 64 or 129..144 -- ococc_sir_rel_chain_fwd_floats returns -1 for a chain outside
 * that (run its rel_mlp inside its layer: n_rel > 0).
 *   fwd: host_slabs[c] (ococc_sir_rel_chain_fwd_floats floats) keeps the inner blocks' rows, host_gates[c] [rows, n last]
 *        (HOST tables of `count` device pointers, as `chains` is a HOST array of `count` descriptors).
 *   bwd: host_dgates[c] [rows, n last] -> per block the LayerNorm partial rows [tiles][2][n] and weight-gradient slices
 *        [slices][n][k] inside host_slabs[c] at the offsets ococc_sir_rel_chain_bwd_layout reports (finish with
 *        ococc_layernorm_param_reduce_multi); f_cluster receives no gradient (the reference detaches it: voxel_encoder.py:781). */
typedef struct {
  int32_t n_blocks, cluster_cols;
  const float* rel_colscale;         /* [cluster_cols] or null */
  int32_t n[4];
  int32_t act[4];
  float eps[4];
  const float* w_frag[4];
  const float* wt_frag[4];
  const float* ln_weight[4];
  const float* ln_bias[4];
} ococc_sir_rel_chain;
int64_t ococc_sir_rel_chain_fwd_floats(const ococc_sir_rel_chain* chain, int64_t rows);
int ococc_sir_rel_chain_bwd_layout(const ococc_sir_rel_chain* chain, int64_t rows, int64_t* host_ln_partial_off,
                                   int64_t* host_w_partial_off, int64_t* host_tiles, int32_t* host_slices,
                                   int64_t* host_total_floats);
int ococc_sir_rel_chains_fwd_f32(int32_t count, const ococc_sir_rel_chain* chains, const float* f_cluster, int64_t rows,
                                 float* const* host_slabs, float* const* host_gates, ococc_stream_t stream);
int ococc_sir_rel_chains_bwd_f32(int32_t count, const ococc_sir_rel_chain* chains, const float* f_cluster, int64_t rows,
                                 const float* const* host_fwd_slabs, const float* const* host_gates,
                                 const float* const* host_dgates, float* const* host_slabs, ococc_stream_t stream);
int ococc_sir_layer_fused_status(ococc_stream_t stream, int32_t* host_status);

/* ------------------------------------------------------------------------
 * A9 / A10  f32 matrix products on the bf16 matrix cores at f32-level accuracy: the operand split.
 * Replaces the f32 GEMMs behind nn.Linear / nn.MultiheadAttention of the temporal transformer and the RoI-level MLPs
 * (mmdet3d/models/occ/layers.py:35-87, mmdet3d/models/roi_heads/bbox_heads/ococc_bbox_head.py:116-193,849-908) from a few
 * hundred rows on: x = hi + lo + O(2^-17 |x|) with hi = bf16(x), lo = bf16(x - hi), and
 *   x w ~ hi_x hi_w + hi_x lo_w + lo_x hi_w   (relative error 4.5e-6 against f64; the f32 GEMM: 7e-7; bf16 operands: 2.3e-3)
 * is ONE bf16 GEMM with f32 accumulation over a three times longer contraction.  ococc_split3_bf16 makes the three-part
 * operand of an f32 matrix src [rows, cols] (row stride ld_src floats) in one pass, in either or both forms:
 *   cat_cols   [rows, 3 cols] bf16: the parts side by side (the matrix's ROWS are contracted against another's rows)
 *   stack_rows [3 rows, cols] bf16: the parts stacked (its COLUMNS stay, the three row blocks are contracted)
 * pattern 0 = (hi, hi, lo), 1 = (hi, lo, hi): one operand of a product takes 0, the other 1.  cols % 8 == 0. */
int ococc_split3_bf16(const float* src, int64_t rows, int64_t cols, int64_t ld_src, uint16_t* cat_cols, int32_t cat_pattern,
                      uint16_t* stack_rows, int32_t stack_pattern, ococc_stream_t stream);

/* ------------------------------------------------------------------------
 * A9  the attention core of the temporal transformer, one launch per direction (csrc/causal_attn.hip).
 * Replaces, inside nn.MultiheadAttention as SimpleEncoderLayer calls it (mmdet3d/models/occ/layers.py:35-87; callers
 * ococc_bbox_head.py:849-995), the chain  (q / sqrt(D)) k^T -> masked_fill(attn_mask, key_padding_mask) -> softmax ->
 * dropout -> @ v  and its backward (ten launches on [B H, L, S] tensors at L = 32).
 * q, k, v: f32 token-major rows t = l * batch + b (the reference's [L, B, E] layout flattened), head h in columns
 * h * head_dim .. + head_dim - 1, row strides ldq / ldk / ldv floats (q and k may be column slices of one projection).
 * attn_mask [L, S] / key_padding_mask [batch, S]: bytes, 1 = masked, or null.  dropout_p in [0, 1): the keep mask is a
 * counter-based hash of (seed, element), regenerated by the backward call from the same seed; seed_dev non-null: the seed
 * is read from device memory (inside a captured graph every replay then draws its own).  probs [batch * heads, L, S]: the
 * probabilities before dropout, written by the forward call and read by the backward call.  out [L * batch, ldo].
 * L, S <= 256, head_dim % 4 == 0 and <= 384 (OCOCC_EUNSUPPORTED otherwise).  No atomics; deterministic. */
int ococc_temporal_attention_fwd_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                     const uint8_t* attn_mask, const uint8_t* key_padding_mask, int32_t batch, int32_t heads,
                                     int32_t L, int32_t S, int32_t head_dim, float scale, float dropout_p, uint64_t seed,
                                     const uint64_t* seed_dev, float* probs, float* out, int64_t ldo, ococc_stream_t stream);
int ococc_temporal_attention_bwd_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                     int32_t batch, int32_t heads, int32_t L, int32_t S, int32_t head_dim, float scale,
                                     float dropout_p, uint64_t seed, const uint64_t* seed_dev, const float* probs,
                                     const float* out, int64_t ldo, const float* d_out, int64_t lddo, float* dq, int64_t lddq,
                                     float* dk, int64_t lddk, float* dv, int64_t lddv, ococc_stream_t stream);

/* ------------------------------------------------------------------------
 * A9, online  one frame of that attention core against cached keys and values (csrc/causal_attn_step.hip).
 * Replaces, for a tracklet that arrives frame by frame, the re-run of the chain above on the growing prefix: under the
 * causal mask of OccBBoxHead.get_future_mask (ococc_bbox_head.py:1034-1043; test_cfg.attn_window_size) row t of
 * nn.MultiheadAttention as SimpleEncoderLayer calls it (mmdet3d/models/occ/layers.py:35-87) reads keys lo .. t only.
 * q, k_new, v_new: f32 [n, heads * head_dim], one row per stepping tracklet, head h in columns h * head_dim .., row
 * strides ldq / ldk / ldv floats.  slot [n]: the cache slot of each row (device, distinct, in [0, slots)); pos [slots]:
 * the frames already cached per slot (device).  k_cache, v_cache: f32 [slots, cap, heads * head_dim], contiguous.
 * For row i with s = slot[i], t = pos[s]: k_new[i] / v_new[i] are written to cache row (s, t), and
 *   out[i] = softmax(scale q[i] . K[s, lo .. t]) V[s, lo .. t]  per head,  lo = max(0, t - window + 1) (window <= 0: 0).
 * pos is NOT advanced (every encoder layer has its own cache and shares pos; the caller bumps it after the last layer).
 * No cache row outside [lo, t] is read, none but t is written; a row whose slot or pos[slot] is out of range is skipped
 * (nothing written, out[i] untouched).  cap <= 256, head_dim % 4 == 0 and <= 384, 16-byte aligned rows (OCOCC_EINVAL
 * otherwise, nothing launched).  No dropout (inference); no atomics; deterministic. */
int ococc_temporal_attention_step_f32(const float* q, int64_t ldq, const float* k_new, int64_t ldk, const float* v_new,
                                      int64_t ldv, const int32_t* slot, const int32_t* pos, float* k_cache, float* v_cache,
                                      int32_t n, int32_t slots, int32_t cap, int32_t heads, int32_t head_dim, float scale,
                                      int32_t window, float* out, int64_t ldo, ococc_stream_t stream);

/* A9, online, past 256 frames  the same kernel template with the scores kept in LDS (csrc/causal_attn_step.hip): the
 * step of nn.MultiheadAttention as SimpleEncoderLayer calls it (mmdet3d/models/occ/layers.py:35-87) under the causal mask
 * of OccBBoxHead.get_future_mask (ococc_bbox_head.py:1034-1043; test_cfg.attn_window_size) for tracklets longer than the
 * 256 frames the export above takes.  Arguments as above, and ``ring`` after ``window``:
 *   ring == 0: frame f of a slot lives in cache row f; cap <= 4096; a row with pos[slot] >= cap is skipped.
 *   ring != 0: frame f lives in cache row f % cap, and 1 <= window <= cap is required: the row of frame t = pos[slot]
 *              overwrites frame t - cap, which the window no longer reads, so pos[slot] may grow to 2^31 - 1.
 * out[i] = softmax(scale q[i] . K[frames lo .. t]) V[frames lo .. t] per head, lo = max(0, t - window + 1) (window <= 0: 0).
 * With more than 256 keys a thread owns the scores tid, tid + 256, ...; for <= 256 keys the arithmetic is, operation for
 * operation, that of ococc_temporal_attention_step_f32.  pos is not advanced.  cap > 4096, ring with window < 1 or
 * window > cap, n > slots, head_dim % 4 != 0 or > 384, null pointers, unaligned rows: OCOCC_EINVAL, nothing launched.
 * No dropout (inference); no atomics; deterministic. */
int ococc_temporal_attention_step_long_f32(const float* q, int64_t ldq, const float* k_new, int64_t ldk, const float* v_new,
                                           int64_t ldv, const int32_t* slot, const int32_t* pos, float* k_cache,
                                           float* v_cache, int32_t n, int32_t slots, int32_t cap, int32_t heads,
                                           int32_t head_dim, float scale, int32_t window, int32_t ring, float* out,
                                           int64_t ldo, ococc_stream_t stream);

/* A9, online, several frames per call  the chunk mode of the same kernel template (csrc/causal_attn_step.hip): one call
 * advances every slot by one or more frames -- a tracklet that arrives with history (track birth, catch-up), or a
 * recorded one fed T frames at a time.  Arguments as above, and ``off`` [n] (device) after ``slot``.  The rows of one slot
 * are consecutive and in frame order, off[i] = 0, 1, 2, ... inside the slot's run; row i is frame t = pos[s] + off[i] of
 * slot s = slot[i] and
 *   out[i] = softmax(scale q[i] . K[frames lo .. t]) V[frames lo .. t]  per head,  lo as above,
 * with the frames < pos[s] taken from the cache (row f, ring != 0: row f % cap) and the frames pos[s] .. t from the call's
 * own rows k_new / v_new[i - off[i] + (f - pos[s])] -- in the order, operation for operation, of the step exports, so a
 * chunk returns bit for bit what the single steps return.  The attention kernel neither writes the cache nor reads a row
 * at or past pos[s]; a second kernel on the same stream then writes k_new / v_new to the rows of the new frames (in a ring
 * whose run is longer than cap only the frame that ends up in each row).  pos is not advanced.  n may exceed slots.
 * cap <= 256 and ring == 0: one score per thread; otherwise the long instance (cap <= 4096).  A row is skipped (nothing
 * written, out[i] untouched) when its slot is out of range, off[i] < 0 or > i, slot[i - off[i]] != slot[i], without ring
 * t >= cap, or it has more keys than the instance holds.  cap > 4096, ring with window < 1 or window > cap,
 * head_dim % 4 != 0 or > 384, null pointers, unaligned rows: OCOCC_EINVAL, nothing launched.  No dropout; deterministic. */
int ococc_temporal_attention_chunk_f32(const float* q, int64_t ldq, const float* k_new, int64_t ldk, const float* v_new,
                                       int64_t ldv, const int32_t* slot, const int32_t* off, const int32_t* pos,
                                       float* k_cache, float* v_cache, int32_t n, int32_t slots, int32_t cap, int32_t heads,
                                       int32_t head_dim, float scale, int32_t window, int32_t ring, float* out, int64_t ldo,
                                       ococc_stream_t stream);

/* ------------------------------------------------------------------------
 * A11 / A10, fused  the occupancy decoder's per-query MLP, one launch per layer (or one for the whole MLP):
 *   y = dropout(act(LayerNorm(x W^T + bias + add_rows[add_index]))),  optionally  head = y . head_weight + head_bias
 * replaces OccDecoder.forward's conv_occ (mmdet3d/models/occ/occ_base.py:99-153): build_mlp's
 * Sequential(Linear(bias=False), LN, GELU, Dropout) blocks 1596 -> 512 -> 1024 -> 1024 and the Linear(1024 -> 1) head
 * (mmdet3d/ops/sst/sst_ops.py:333-360), and PosEncode.forward (occ_base.py:33-57).
 * bf16 operands, f32 accumulation, f32 LayerNorm statistics over the f32 sums, bf16 activations.
 * ococc_pos_encode_bf16: xyz f32 [rows, 3] -> out bf16 [rows, ld], columns [sin(pi 2^l x^) | cos(pi 2^l x^)] in the
 *   reference's [2L][3] order, x^ = x normalised to [-1, 1] by host_bound = {lo xyz, hi xyz} (HOST pointer; null: x^ = x),
 *   columns 6L .. ld - 1 zero.
 * ococc_linear_fragments32_bf16: `count` (<= 16) f32 matrices S_i [rows_i, cols_i] (any strides; rows a multiple of
 *   32) -> bf16 operand fragments of v_mfma_f32_32x32x16_bf16, columns zero-padded to padded_cols_i (multiple of 16):
 *   dst_i[rb][cs][lane][j] = S_i[32 rb + (lane & 31)][16 cs + 8 (lane >> 5) + j].  The tables are HOST arrays.
 * ococc_mlp_layer_fwd_bf16: x bf16 [rows, k], k a multiple of 64 up to 1024; w_frag the fragments of W [n, k],
 *   n 512 or 1024; bias [n], add_rows f32 [*, n] with add_index int32 [rows], ln_weight / ln_bias [n], head_weight [n] with
 *   head_bias [1] (device): each optional.  act: 0 none, 1 GELU (erf).  drop_threshold > 0: the counter-based keep mask of
 *   ococc_layernorm_act_dropout_fwd_bf16 (same threshold and seed -> same mask).  y bf16 [rows, n] or null when only the head is wanted;
 *   head_out f32 [rows] (the head reads the bf16-rounded activation, as the next Linear would).
 * ococc_occ_mlp_fwd_bf16: the reference's decoder widths, 60 (padded to 64) -> 512 -> 1024 -> 1024 -> 1, in ONE launch;
 *   a 64-row tile's activations stay in LDS between the layers.  pe bf16 [rows, 64] (ococc_pos_encode_bf16), add_rows
 *   f32 [*, 512] with add_index [rows] (the per-RoI half of the first layer); host_w_frag / host_ln_weight /
 *   host_ln_bias: HOST tables
 *   of 3 device pointers (fragments of [512, 64], [1024, 512], [1024, 1024]; f32 [n]); GELU after every LayerNorm;
 *   head_weight f32 [1024], head_bias [1] or null; host_dropout_seeds: HOST array of 3 (read when drop_threshold > 0), the
 *   masks of ococc_mlp_layer_fwd_bf16 called per layer with the same seeds.  out f32 [rows];  y0_out bf16 [rows, 512]
 *   / y1_out bf16 [rows, 1024]: optional copies of the hidden activations (what a backward pass starts from).
 *   Bit-identical to three ococc_mlp_layer_fwd_bf16 calls.
 * ------------------------------------------------------------------------ */
int ococc_pos_encode_bf16(const float* xyz, int64_t rows, const float* host_bound, int32_t num_freqs, uint16_t* out,
                          int32_t ld, ococc_stream_t stream);
int ococc_linear_fragments32_bf16(int32_t count, const void* const* host_src, const int64_t* host_rows,
                                  const int64_t* host_cols, const int64_t* host_padded_cols, const int64_t* host_row_stride,
                                  const int64_t* host_col_stride, void* const* host_dst, ococc_stream_t stream);
int ococc_mlp_layer_fwd_bf16(const uint16_t* x, int64_t rows, int32_t k, const uint16_t* w_frag, int32_t n,
                             const float* bias, const float* add_rows, const int32_t* add_index, const float* ln_weight,
                             const float* ln_bias, float eps, int32_t act, uint32_t drop_threshold, uint64_t dropout_seed,
                             uint16_t* y, const float* head_weight, const float* head_bias, float* head_out,
                             ococc_stream_t stream);
int ococc_occ_mlp_fwd_bf16(const uint16_t* pe, int64_t rows, const float* add_rows, const int32_t* add_index,
                           const void* const* host_w_frag, const void* const* host_ln_weight,
                           const void* const* host_ln_bias, float eps, const float* head_weight, const float* head_bias,
                           uint32_t drop_threshold, const uint64_t* host_dropout_seeds, uint16_t* y0_out, uint16_t* y1_out,
                           float* out, ococc_stream_t stream);
/* the same launch in a training step: per layer l it also writes the LayerNorm input z_out[l] (bf16 [rows, n_l]; the
 * LayerNorm works on these rounded values), its row statistics stats_out[l] (f32 [rows, 2]: mean, rstd) and the activation
 * y_out[l] (bf16, after GELU and dropout) -- what the backward pass of OccDecoder.forward's conv_occ reads
 * (ococc_layernorm_act_bwd / _dropout_bwd_bf16 with the same (threshold, seed) per layer).  host_z_out, host_y_out,
 * host_stats_out: HOST tables of 3 device pointers, every entry required (a null one is an argument error). */
int ococc_occ_mlp_train_fwd_bf16(const uint16_t* pe, int64_t rows, const float* add_rows, const int32_t* add_index,
                                 const void* const* host_w_frag, const void* const* host_ln_weight,
                                 const void* const* host_ln_bias, float eps, const float* head_weight,
                                 const float* head_bias, uint32_t drop_threshold, const uint64_t* host_dropout_seeds,
                                 void* const* host_z_out, void* const* host_y_out, void* const* host_stats_out, float* out,
                                 ococc_stream_t stream);

/* ------------------------------------------------------------------------
 * Test-time tuning of the fused shape latent (OccBBoxHead.online_tuning, ococc_bbox_head.py:402-431;
 * OccAutoEncoder.online_tuning_forward, occ_ae_head.py:346-391): what is specific to tuning around the backward chain of
 * the frozen decoder.  Zero rows: OCOCC_OK without a launch.
 *
 * ococc_occ_tune_head_lnbwd_bf16 replaces, per iteration, the backward of loss_ae.backward() (occ_ae_head.py:381-385)
 *   through CrossEntropyLoss(use_sigmoid, reduction 'none').mean(), the head Linear and the last LayerNorm + GELU of
 *   conv_occ (occ_base.py:99-153): per row d = scale * weights[i] * (sigmoid(logits[i]) - labels[i]) (scale =
 *   loss_weight / rows; weights null = 1), dy = d * head_weight (registers only), then the GELU and LayerNorm backward of
 *   ococc_layernorm_act_bwd from the stored z (bf16 [rows, 1024]) and mean_rstd (f32 [rows, 2]) to dz (bf16 [rows, 1024]).
 *   No parameter-gradient partials.  labels int32 [rows]; c must be 1024.
 * ococc_segment_sum_bf16 replaces the gather's backward (roi_feats[pts_roi_inds], ococc_bbox_head.py:711): out[k, :] = sum
 *   of the rows of x (bf16 [rows, 512]) whose index is k, f32 [num_segments, 512], accumulated in f32 in an order that
 *   depends on the segment's extent alone (no atomics: two runs give equal bits).  index int32 [rows], non-decreasing; a
 *   segment without rows gets a zero row; rows whose index is outside [0, num_segments) are left out.  c must be 512.
 * ococc_latent_ln_adam_f32 replaces the backward of OccDecoder.ln (occ_base.py:104-106) and optimizer.step() /
 *   scheduler.step() of torch.optim.Adam([roi_embed], lr=0.01) + StepLR (occ_ae_head.py:362-363, 386-387): per row of e
 *   (f32 [rows, d], updated in place) it recomputes mean / rstd, takes d_n (the gradient of LN(e)) through the LayerNorm
 *   backward with gamma to de (use_ln == 0: de = d_n, gamma may be null), and applies Adam's step t (counted from 1) in
 *   place on e, m, v: m = m + (de - m)(1 - beta1), v = beta2 v + (1 - beta2) de^2,
 *   e -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps).  lr is the step's learning rate (the schedule is the
 *   caller's); lr, the betas and eps are doubles: 1 - beta, the bias corrections and the step size are worked out in double on
 *   the host and rounded once.  de_out (f32 [rows, d], may be null) receives de.  d a multiple of 4 in [4, 2048].
 * ------------------------------------------------------------------------ */
int ococc_occ_tune_head_lnbwd_bf16(const float* logits, const int32_t* labels, const float* weights, float scale,
                                   const float* head_weight, const uint16_t* z, const float* mean_rstd,
                                   const float* gamma, const float* beta, int64_t rows, int32_t c, uint16_t* dz,
                                   ococc_stream_t stream);
int ococc_segment_sum_bf16(const uint16_t* x, const int32_t* index, int64_t rows, int32_t c, float* out,
                           int64_t num_segments, ococc_stream_t stream);
int ococc_latent_ln_adam_f32(float* e, const float* d_n, float* m, float* v, int64_t rows, int32_t d, const float* gamma,
                             float ln_eps, int32_t use_ln, double lr, double beta1, double beta2, double eps, int32_t t,
                             float* de_out, ococc_stream_t stream);

/* ------------------------------------------------------------------------
 * B6, element-wise halves of the SST input layer, one launch each (the mirror ran 20-50 torch operators per call):
 * ococc_sst_window_coors_i64: get_window_coors (mmdet3d/ops/sst/sst_ops.py:266-313) for BOTH window shifts.
 *   coors int64 [n, 4] (b, z, y, x); shapes (host_*_shape_xyz) as (x, y, z) HOST triples (2-D windows: pass window z =
 *   sparse z);
 *   win_ids int64 [2, n] (shift 0 = unshifted, 1 = shifted by half a window), coors_in_win int64 [2, n, 3] (z, y, x).
 * ococc_sst_drop_level_i64: the level / keep decision of SSTInputLayerV2.drop_single_shift
 *   (mmdet3d/models/middle_encoders/sst_input_layer_v2.py:128-148) from one group-rank pass: window population =
 *   counts[conti[i]]; the LAST table row whose [host_lower, host_upper) holds it gives host_level_ids[r] and
 *   host_max_tokens[r] (none: -1, 0); keep[i] = inner[i] < max_tokens.  The table's columns are HOST arrays (<= 8 rows).
 * ococc_sst_pos_embed: get_pos_embed (sst_input_layer_v2.py:239-305) in flat token order: out [n, feat_dim] f32 / bf16,
 *   columns [x | y | z] blocks of pos_length (sin at even, cos at odd columns of e = p / inv_freq), zero padded;
 *   inv_freq: DEVICE f32 [pos_length], the table the reference builds with torch.pow.
 * ------------------------------------------------------------------------ */
int ococc_sst_window_coors_i64(const int64_t* coors, int64_t n, const int32_t* host_sparse_shape_xyz,
                               const int32_t* host_window_shape_xyz, int64_t* win_ids, int64_t* coors_in_win,
                               ococc_stream_t stream);
int ococc_sst_drop_level_i64(const int32_t* conti, const int32_t* inner, const int32_t* counts, int64_t n,
                             int32_t num_levels, const int64_t* host_lower, const int64_t* host_upper,
                             const int64_t* host_max_tokens, const int64_t* host_level_ids, uint8_t* keep, int64_t* level,
                             ococc_stream_t stream);
int ococc_sst_pos_embed(const int64_t* coors_in_win, int64_t n, const int32_t* host_window_shape_xyz, int32_t ndim,
                        int32_t normalize_pos, const float* inv_freq, int32_t pos_length, int32_t feat_dim, void* out,
                        int32_t out_dtype, ococc_stream_t stream);

/* f32 <-> bf16 row casts (round to nearest even) */
int ococc_cast_f32_to_bf16(const float* src, uint16_t* dst, int64_t count, ococc_stream_t stream);
int ococc_cast_bf16_to_f32(const uint16_t* src, float* dst, int64_t count, ococc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Fused multi-tensor AdamW step, torch.optim.AdamW semantics (amsgrad / maximize off) -- the
 * optimizer the reference configures at configs/_base_/schedules/cosine_2x.py:2-8 (lr override
 * configs/ococc/ococcnet.py:468-470).  host_params / host_grads / host_exp_avg / host_exp_avg_sq are HOST arrays of
 * num_tensors (<= 48) device pointers to contiguous f32 tensors of host_numel[i] elements.  `step` is a
 * DEVICE float holding the number of steps taken so far: the kernel uses step + 1 for the bias
 * corrections; with bump_step = 1 a one-thread kernel queued behind it stores step + 1 (pass 0 on all
 * but the last call when one optimizer step needs several calls), so the sequence can be replayed from
 * a captured HIP graph.  bump_step = 2: `step` points to {float count; uint32 ticket}, ticket zero before
 * the first call; launches of up to 2048 workgroups (2 M elements) then store count + 1 from their last
 * workgroup instead of a second launch (larger ones fall back to the one-thread kernel).
 * ------------------------------------------------------------------------------------------- */
int ococc_adamw_f32(int32_t num_tensors, void* const* host_params, const void* const* host_grads,
                    void* const* host_exp_avg, void* const* host_exp_avg_sq, const int64_t* host_numel, float lr,
                    float beta1, float beta2, float eps, float weight_decay, float* step,
                    int32_t bump_step, ococc_stream_t stream);
/* The same update with the learning rate read from device memory at run time (one float): a learning-rate schedule
 * (the reference's cyclic policy, configs/_base_/schedules/cosine_2x.py:10-15, applied per iteration by mmcv's
 * CyclicLrUpdaterHook) then takes effect between replays of a captured HIP graph, where a scalar launch argument
 * would stay frozen at its capture-time value. */
int ococc_adamw_lr_dev_f32(int32_t num_tensors, void* const* host_params, const void* const* host_grads,
                           void* const* host_exp_avg, void* const* host_exp_avg_sq, const int64_t* host_numel,
                           const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                           float* step, int32_t bump_step, ococc_stream_t stream);
/* The same update that ALSO refreshes the bf16 kernel operands of convolution weights it has just written (what
 * ococc_weight_prepare_multi_bf16 would compute at the start of the next step: one launch less per step).  lr_dev null:
 * lr is used.  Operand o belongs to tensor host_operand_tensor[o] (an index into host_params, a contiguous f32
 * [kvol, cin, cout]), is written in layout host_operand_mode[o] (the modes of ococc_weight_prepare_bf16, + 4 =
 * fragment-major) to host_operand_dst[o] (bf16, kvol * cin * cout elements); at most 8 operands per call.  All tables are
 * HOST arrays. */
int ococc_adamw_operands_f32(int32_t num_tensors, void* const* host_params, const void* const* host_grads,
                             void* const* host_exp_avg, void* const* host_exp_avg_sq, const int64_t* host_numel, float lr,
                             const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, float* step,
                             int32_t bump_step, int32_t num_operands, const int32_t* host_operand_tensor,
                             const int32_t* host_operand_mode, const int32_t* host_operand_kvol,
                             const int32_t* host_operand_cin, const int32_t* host_operand_cout,
                             void* const* host_operand_dst, ococc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Stream timers (HIP events) for the measurement harness (bench.py roofline line).  No reference
 * counterpart.  in_graph != 0 records with hipEventRecordExternal, i.e. as an event-record node
 * of the HIP graph being captured on `stream`, so that a kernel inside a replayed graph can be
 * timed; the elapsed time is read after the stream has been synchronised.
 * ------------------------------------------------------------------------------------------- */
int ococc_timer_create(void** host_timer);
int ococc_timer_record(void* timer, int32_t in_graph, ococc_stream_t stream);
int ococc_timer_elapsed_ms(void* start, void* stop, float* host_ms);
int ococc_timer_destroy(void* timer);

#ifdef __cplusplus
}
#endif
#endif /* OCOCC_HIP_H_ */
