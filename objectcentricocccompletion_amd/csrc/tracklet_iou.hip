// Max IoU of every (predicted tracklet, ground-truth tracklet) pair of one segment: the affinity of CTRL's candidate
// generation (tools/ctrl/generate_candidates.py:61-65 -> LiDARTracklet.max_iou,
// mmdet3d/core/bbox/structures/lidar_tracklet.py:210-229).  The reference does, PER PAIR, a Python timestamp
// intersection, two uploads, one aligned_iou_3d launch and an .item(): P x G synchronising round trips per segment.
// Here: one launch per segment.  One wave per pair; lane l takes the predicted tracklet's boxes l, l + 64, ..., finds
// the GT box of the same frame by binary search in the GT tracklet's strictly increasing frame list, and computes the
// one-to-one IoU with the arithmetic of box_iou.hpp (shared with aligned_iou3d_kernel, bit for bit); the wave maximum
// is taken with shuffles -- no float atomics.  Exact early-out: when the BEV circumscribed circles of the two boxes are
// apart (by 1 cm more than f32 rounding could hide) the rectangles are disjoint and the clip would return an empty
// polygon, when the height intervals do not meet the overlap height is 0: the IoU is exactly +0 either way.
// Latency / ALU bound (the clip is ~1k instructions per overlapping pair of boxes); bytes: (sum Lp + sum Lg) * 32 B of
// boxes and frame indices, re-read from L2 per pair, P * G * 4 B out.
#include "box_iou.hpp"

namespace {

__global__ void __launch_bounds__(256)
tracklet_max_iou_kernel(const float* __restrict__ pd_boxes, const int32_t* __restrict__ pd_offsets,
                        const int32_t* __restrict__ pd_frames, int32_t P, const float* __restrict__ gt_boxes,
                        const int32_t* __restrict__ gt_offsets, const int32_t* __restrict__ gt_frames, int32_t G,
                        float* __restrict__ max_iou) {
  const int lane = threadIdx.x & 63;
  const int64_t pair = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (pair >= (int64_t)P * G) return;   // (wave-uniform)
  const int p = (int)(pair / G), g = (int)(pair % G);
  const int p0 = pd_offsets[p], p1 = pd_offsets[p + 1], g0 = gt_offsets[g], g1 = gt_offsets[g + 1];
  float best = 0.f;
  // no common frame possible when the two frame ranges do not meet (both lists are strictly increasing)
  const bool meet = p1 > p0 && g1 > g0 && pd_frames[p0] <= gt_frames[g1 - 1] && gt_frames[g0] <= pd_frames[p1 - 1];
  if (meet) {
    for (int i = p0 + lane; i < p1; i += 64) {
      const int fr = pd_frames[i];
      int lo = g0, hi = g1;             // first GT entry with frame >= fr
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (gt_frames[mid] < fr) lo = mid + 1;
        else hi = mid;
      }
      if (lo >= g1 || gt_frames[lo] != fr) continue;
      const float* a = pd_boxes + (int64_t)i * 7;
      const float* b = gt_boxes + (int64_t)lo * 7;
      const float top = fminf(a[2] + a[5], b[2] + b[5]), bot = fmaxf(a[2], b[2]);
      if (top - bot <= 0.f) continue;   // overlap height 0: IoU +0
      const float dx = a[0] - b[0], dy = a[1] - b[1];
      const float ra = 0.5f * sqrtf(a[3] * a[3] + a[4] * a[4]), rb = 0.5f * sqrtf(b[3] * b[3] + b[4] * b[4]);
      const float reach = (ra + rb) * 1.0001f + 0.01f;
      if (dx * dx + dy * dy > reach * reach) continue;   // disjoint rectangles: the clip is empty, IoU +0
      best = fmaxf(best, aligned_iou3d_pair(a, b));
    }
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) best = fmaxf(best, __shfl_xor(best, s, 64));
  if (lane == 0) max_iou[pair] = best;
}

}  // namespace

extern "C" int ococc_tracklet_max_iou_f32(const float* pd_boxes, const int32_t* pd_offsets, const int32_t* pd_frames,
                                          int32_t num_pd, const float* gt_boxes, const int32_t* gt_offsets,
                                          const int32_t* gt_frames, int32_t num_gt, float* max_iou,
                                          ococc_stream_t stream) {
  OCOCC_REQUIRE(num_pd >= 0 && num_gt >= 0, "negative tracklet count");
  if (num_pd == 0 || num_gt == 0) return OCOCC_OK;
  OCOCC_REQUIRE(pd_boxes && pd_offsets && pd_frames && gt_boxes && gt_offsets && gt_frames && max_iou, "null pointer");
  const int64_t pairs = (int64_t)num_pd * num_gt;
  OCOCC_REQUIRE(ococc_cdiv(pairs, 4) <= 0x7fffffffLL, "too many pairs for one launch");
  hipLaunchKernelGGL(tracklet_max_iou_kernel, dim3((unsigned)ococc_cdiv(pairs, 4)), dim3(256), 0, (hipStream_t)stream,
                     pd_boxes, pd_offsets, pd_frames, num_pd, gt_boxes, gt_offsets, gt_frames, num_gt, max_iou);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}
