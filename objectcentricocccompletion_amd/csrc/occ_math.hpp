// Device arithmetic shared by the occupancy kernels (occ_iou_count.hip, occ_export.hip, gt_occ_crop.hip), written so that a result is
// the f32 value the ATen chain it replaces gives: every operation rounded on its own, no fused multiply-add.
#pragma once
#include "common.hpp"

// ATen's sigmoid in f32: one / (one + std::exp(-a))
__device__ __forceinline__ float ococc_sigmoid_aten(float x) { return 1.0f / (1.0f + expf(-x)); }

// "occupied" of the one-logit decoder (OccDecoder._occupied / get_cls_from_pred): sigmoid(logit) > pos_thresh; false
// for NaN
__device__ __forceinline__ bool ococc_occupied(float logit, float pos_thresh) {
  return ococc_sigmoid_aten(logit) > pos_thresh;
}

// Centre of cell c of an axis of the dense grid of a box of (enlarged) extent `size` (occ_ops.py:5-50):
//   (c * voxel_size + (-size / 2)) + voxel_size / 2, as dense_voxel_centers_batched evaluates it operator by operator
__device__ __forceinline__ float ococc_cell_centre(int c, float size, float voxel_size) {
#pragma clang fp contract(off)   // (hipcc's default fuses a * b + c, also when written as __fadd_rn(__fmul_rn(a, b), c))
  const float at = (float)c * voxel_size;
  const float lo = at + (-size / 2.0f);
  return lo + voxel_size / 2.0f;
}

// A point of a box's gravity-centred frame in the LiDAR frame (OccDecoder._to_lidar, occ_base.py:220-230, 330-336;
// tracklet_roi_head_occ.py:665-670): rotation_3d_in_axis(axis=2) with the transposed matrix, x c + y s and -x s + y c,
// then + the bottom centre (bx, by, bz), then z + half_h; (c, s) the cos / sin of the yaw
__device__ __forceinline__ void ococc_box_to_lidar(float& x, float& y, float& z, float c, float s, float bx, float by,
                                                   float bz, float half_h) {
#pragma clang fp contract(off)
  const float xc = x * c, ys = y * s, xs = -x * s, yc = y * c;
  x = (xc + ys) + bx, y = (xs + yc) + by, z = (z + bz) + half_h;
}
