// Completed occupancy of ONE online step: what the decoder predicts occupied, joined with what the sensor hit in this
// frame, compacted in cell order into rows (x, y, z, probability) plus a flag byte per row.  Stands behind
// occ_ops.occ_frame_select / OccDecoder.get_frame_occ and the ``occ=True`` results of TrackletRoIHeadOCC.simple_test_step,
// simple_test_steps and simple_test_scene_step; replaces, for the step, OccAutoEncoder.sample_observation's
// rasterisation (mmdet3d/models/roi_heads/bbox_heads/occ_ae_head.py:65-126, about 25 ATen launches with int64 index
// tensors) and the select / transform of OccDecoder.get_occ (mmdet3d/models/occ/occ_base.py:238-342).
//
// The flat cell list and its tiles of 1024 cells of one RoI are those of occ_export.hip, and count and fill ARE its
// select kernel, reached through occ_select_count / occ_select_fill (occ_tiles.hpp); this file holds the mark kernel and
// the argument checks of the three exports.
//
//   mark   : one thread per pooled point (box-frame xyz, RoI index).  Cell index per axis with the f32 arithmetic of
//            occ_ops.quantize_points, floor((p - (-size / 2)) / voxel), a true division; an index < 0 or >= dim on any
//            axis marks nothing (the points were pooled from an enlarged box).  observed[cell] = 1: a byte store, all
//            points of a cell store the same value, so no atomic.  observed is zeroed in front (one memset).
//   count  : selected = (ococc_occupied(logit) or observed[cell]) and row_keep[RoI] != 0 (row_keep null: every RoI kept).
//   fill   : row = centre through ococc_box_to_lidar with the RoI's pose, then optionally through the RoI's 3x4 matrix
//            T: x' = ((t0 x + t1 y) + t2 z) + t3, every operation rounded once; column 3 ococc_sigmoid_aten(logit).
//            One 16-byte store per row and one byte of flags: bit 0 predicted, bit 1 observed.
//
// Algorithmic bytes: mark 16 B in, 1 B out per point; count 5 B in per cell; fill 5 B in per cell, 17 B out per
// selected cell.  Memory bound and small next to the decoder (about 4.8 MFLOP per cell).  No float atomics, integer
// counts: the same input gives the same bytes.  Vector stores only.
#include "common.hpp"
#include "occ_tiles.hpp"

// every float product, quotient and sum below is rounded on its own, as the ATen chain rounds them
#pragma clang fp contract(off)

namespace {

constexpr int kMarkBlock = 256;

__global__ void __launch_bounds__(kMarkBlock)
occ_frame_mark_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ pts_roi, int64_t M,
                      const float* __restrict__ sizes, const int32_t* __restrict__ dims,
                      const int64_t* __restrict__ start, int R, float voxel_size, uint8_t* __restrict__ observed,
                      int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kMarkBlock + threadIdx.x; i < M; i += (int64_t)gridDim.x * kMarkBlock) {
    const int r = pts_roi[i];
    if (r < 0 || r >= R) continue;
    const float* s = sizes + r * 3;
    const int32_t* d = dims + r * 3;
    int idx[3];
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float lo = -s[a] / 2.0f;                                        // min_bound of quantize_points
      const float q = floorf(__fdiv_rn(xyz[i * 3 + a] - lo, voxel_size));   // NaN: no comparison holds
      const bool ok = q >= 0.0f && q < (float)d[a];
      inside = inside && ok;
      idx[a] = ok ? (int)q : 0;
    }
    if (!inside) continue;
    const int64_t cell = start[r] + ((int64_t)idx[0] * d[1] + idx[1]) * d[2] + idx[2];
    if (cell < 0 || cell >= start[r + 1] || cell >= n) continue;   // (a start that is no prefix of dims: no cell)
    observed[cell] = 1;
  }
}

}  // namespace

extern "C" int ococc_occ_frame_mark(const float* local_xyz, const int32_t* pts_roi, int64_t M, const float* sizes,
                                    const int32_t* dims, const int64_t* start, int32_t R, float voxel_size,
                                    uint8_t* observed, int64_t n, ococc_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OCOCC_REQUIRE(M >= 0 && R >= 0 && n >= 0, "M < 0, R < 0 or n < 0");
  OCOCC_REQUIRE(voxel_size > 0.f, "voxel_size <= 0");
  if (n == 0) return OCOCC_OK;
  OCOCC_REQUIRE(observed, "null pointer: observed");
  OCOCC_HIP(hipMemsetAsync(observed, 0, (size_t)n, stream));
  if (M == 0 || R == 0) return OCOCC_OK;
  OCOCC_REQUIRE(local_xyz && pts_roi && sizes && dims && start, "null pointer");
  hipLaunchKernelGGL(occ_frame_mark_kernel, dim3(ococc_grid_1d(M, kMarkBlock, 2048)), dim3(kMarkBlock), 0, stream,
                     local_xyz, pts_roi, M, sizes, dims, start, R, voxel_size, observed, n);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}

extern "C" int ococc_occ_frame_count(const float* logits, const uint8_t* observed, const uint8_t* row_keep, int64_t n,
                                     const int64_t* start, int32_t R, float pos_thresh, int64_t* tile_start,
                                     int32_t* tile_counts, int64_t max_tiles, int64_t* roi_counts,
                                     ococc_stream_t stream_) {
  return occ_select_count(__func__, logits, observed, row_keep, n, start, R, pos_thresh, tile_start, tile_counts, max_tiles,
                          roi_counts, (hipStream_t)stream_);
}

extern "C" int ococc_occ_frame_fill(const float* logits, const uint8_t* observed, const uint8_t* row_keep, int64_t n,
                                    const int64_t* start, const int64_t* tile_start, int32_t R, float pos_thresh,
                                    const int64_t* tile_scan, int64_t max_tiles, const float* sizes, const int32_t* dims,
                                    float voxel_size, const float* rois, int64_t roi_stride, const float* cos_yaw,
                                    const float* sin_yaw, const float* transforms, float* out, uint8_t* flags,
                                    int64_t n_out, ococc_stream_t stream) {
  OCOCC_REQUIRE(n >= 0 && R >= 0 && n_out >= 0, "n < 0, R < 0 or n_out < 0");
  OCOCC_REQUIRE(voxel_size > 0.f, "voxel_size <= 0");
  OCOCC_REQUIRE(max_tiles >= ococc_occ_select_max_tiles(n, R), "max_tiles < ococc_occ_select_max_tiles(n, R)");
  OCOCC_REQUIRE(R == 0 || roi_stride >= 7, "roi_stride < 7: columns 1-3 (centre) and 6 (height) are read");
  if (R == 0 || n == 0 || n_out == 0 || max_tiles == 0) return OCOCC_OK;
  OCOCC_REQUIRE(rois && cos_yaw && sin_yaw, "null pointer: rois, cos_yaw and sin_yaw give the pose of every RoI");
  OCOCC_REQUIRE(logits && start && tile_start && tile_scan && sizes && dims && out && flags, "null pointer");
  OCOCC_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "out [n, 4] must be 16-byte aligned");
  const OccFillArgs a{tile_scan, sizes, dims, voxel_size, rois, roi_stride, cos_yaw, sin_yaw, transforms, nullptr, 4, out,
                      flags, n_out};
  return occ_select_fill(__func__, logits, observed, row_keep, n, start, tile_start, R, pos_thresh, max_tiles, a,
                         (hipStream_t)stream);
}
