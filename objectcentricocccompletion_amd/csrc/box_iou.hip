// A2 pairwise ("1 to 1") 3-D IoU of rotated boxes: the arithmetic of
// LiDARInstance3DBoxes.aligned_iou_3d (mmdet3d/core/bbox/structures/lidar_box3d.py:404-448),
// whose BEV part is TorchEx boxes_overlap_1to1 (source not vendored; we follow the iou3d
// convention the fork's own iou3d op uses: BEV rectangle (x,y,w,l) with w along x at yaw 0,
// corners turned CLOCKWISE by yaw).  IoU = inter_bev * overlap_h / max(v1 + v2 - inter, 1e-8).
// One thread per pair: Sutherland-Hodgman clipping of two convex quads (<= 8 vertices) and the
// shoelace area.  A few hundred pairs per step: latency only, no roofline to speak of.
#include "box_iou.hpp"

namespace {

__global__ void __launch_bounds__(256)
aligned_iou3d_kernel(const float* __restrict__ b1, const float* __restrict__ b2, int64_t n,
                     float* __restrict__ iou) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  iou[i] = aligned_iou3d_pair(b1 + i * 7, b2 + i * 7);
}

}  // namespace

extern "C" int ococc_aligned_iou3d_f32(const float* boxes1, const float* boxes2, int64_t n,
                                       float* iou, ococc_stream_t stream) {
  OCOCC_REQUIRE(n >= 0, "n < 0");
  if (n == 0) return OCOCC_OK;
  OCOCC_REQUIRE(boxes1 && boxes2 && iou, "null pointer");
  hipLaunchKernelGGL(aligned_iou3d_kernel, dim3((unsigned)ococc_cdiv(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, boxes1, boxes2, n, iou);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}
