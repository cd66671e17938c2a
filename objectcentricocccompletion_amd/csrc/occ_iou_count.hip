// Occupancy IoU counts of test_occ (mmdet3d/models/roi_heads/tracklet_roi_head_occ.py:394-486) in one launch per chunk
// of RoIs: for RoI i and GT voxel k, predicted occupied = sigmoid(logit[i,k]) > pos_thresh (the f32 expression of ATen's
// sigmoid, so that logits next to the threshold decide alike; NaN is empty), optionally only inside the RoI's box
// (-half <= xyz <= half on all three axes, bounds inclusive); label occupied = labels[k] == 1.
//   inter[i] += #(pred & label), union[i] += #(pred | label)
// Lanes ballot their two bits, the wave sums popcounts over its grid-stride loop (wave-uniform), and lane 0 adds the two
// totals with one 64-bit vector atomic each.  Integer sums: the same result in any order.  Memory bound and tiny next to
// the decoder that produced the logits; what it saves is the ATen chain and the host read-back per chunk.
#include "common.hpp"
#include "occ_math.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kCellsPerThread = 8;   // grid-stride depth before the grid widens: fewer waves adding into the same two words
constexpr int kMaxBlocksPerRoi = 64;

__global__ void __launch_bounds__(kBlock)
occ_iou_count_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                     const float* __restrict__ roi_xyz, const float* __restrict__ half_sizes, int64_t K,
                     float pos_thresh, unsigned long long* __restrict__ counts) {
  const int64_t roi = blockIdx.y;
  const float* lg = logits + roi * K;
  const float* q = roi_xyz ? roi_xyz + roi * K * 3 : nullptr;
  float hx = 0.f, hy = 0.f, hz = 0.f;
  if (q) {
    hx = half_sizes[roi * 3 + 0];
    hy = half_sizes[roi * 3 + 1];
    hz = half_sizes[roi * 3 + 2];
  }
  unsigned long long inter = 0, uni = 0;
  // (base is uniform over the block: every lane of a wave reaches both ballots)
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < K; base += (int64_t)gridDim.x * kBlock) {
    const int64_t k = base + threadIdx.x;
    bool pred = false, lab = false;
    if (k < K) {
      pred = ococc_occupied(lg[k], pos_thresh);   // ATen's f32 sigmoid; false for NaN (occ_math.hpp)
      if (q && pred) {
        const float px = q[k * 3 + 0], py = q[k * 3 + 1], pz = q[k * 3 + 2];
        pred = (px >= -hx) && (px <= hx) && (py >= -hy) && (py <= hy) && (pz >= -hz) && (pz <= hz);
      }
      lab = labels[k] == 1;
    }
    inter += (unsigned long long)__popcll(__ballot(pred && lab));
    uni += (unsigned long long)__popcll(__ballot(pred || lab));
  }
  if ((threadIdx.x & 63) == 0 && (inter | uni)) {
    atomicAdd(counts + roi * 2 + 0, inter);
    atomicAdd(counts + roi * 2 + 1, uni);
  }
}

}  // namespace

extern "C" int ococc_occ_iou_count(const float* logits, const int64_t* labels, const float* roi_xyz,
                                   const float* half_sizes, int32_t n, int64_t K, float pos_thresh, int64_t* counts,
                                   int64_t row0, int64_t rows, ococc_stream_t stream) {
  OCOCC_REQUIRE(n >= 0 && K >= 0, "n < 0 or K < 0");
  OCOCC_REQUIRE(row0 >= 0 && row0 + n <= rows, "rows [row0, row0 + n) outside the count buffer");
  OCOCC_REQUIRE((roi_xyz == nullptr) == (half_sizes == nullptr), "roi_xyz and half_sizes go together");
  OCOCC_REQUIRE(n <= 65535, "n > 65535 RoIs in one launch");
  if (n == 0 || K == 0) return OCOCC_OK;
  OCOCC_REQUIRE(logits && labels && counts, "null pointer");
  int64_t gx = ococc_cdiv(K, (int64_t)kBlock * kCellsPerThread);
  if (gx > kMaxBlocksPerRoi) gx = kMaxBlocksPerRoi;
  hipLaunchKernelGGL(occ_iou_count_kernel, dim3((unsigned)gx, (unsigned)n), dim3(kBlock), 0, (hipStream_t)stream,
                     logits, labels, roi_xyz, half_sizes, K, pos_thresh,
                     reinterpret_cast<unsigned long long*>(counts + row0 * 2));
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}
