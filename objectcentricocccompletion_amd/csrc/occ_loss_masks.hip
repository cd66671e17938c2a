// The sample masks of OccBBoxHead.loss_occ's train_cfg variants (mmdet3d/models/roi_heads/bbox_heads/ococc_bbox_head.py:
// 706-710, 713-734, 749-753, 792) in one launch: for sample k of positive RoI i (row i * K + k)
//   weight    = score[i] > score_thresh                                      (:708-710; strict, NaN is 0)
//             * (-size[i] / 2 <= xyz <= size[i] / 2 on all three axes)         kOutside  (:713-722; a NaN coordinate is outside)
//             * (class of the ori logit == 0)                                  kObserved (:723-734)
//   unmatched = (label == 1) != (class of the ori logit)                       kUnmatched (:749-752)
// with class = sigmoid(logit) > pos_thresh decided as ATen's f32 sigmoid decides it (ococc_occupied, occ_math.hpp: NaN is
// class 0), and three integer counts: #(weight > 0), #unmatched, #(unmatched and weight > 0).
// A streaming kernel: a lane takes four consecutive rows (three 16-byte loads of xyz, one of the logits, two of the
// labels, one 16-byte store of the weights and one 4-byte store of the unmatched bytes) when every pointer is 16-byte
// aligned, the same rows one element at a time when not, and in the ragged last group of four.  Four consecutive rows may
// lie in two RoIs (K is arbitrary): the RoI of the first is one 64-bit division, the others follow by counting.  Lanes
// ballot their bits, the wave sums popcounts over its grid-stride loop (wave-uniform) and lane 0 adds the totals with
// one 64-bit vector atomic each (the idiom of occ_iou_count.hip).  Integer sums: the same bits in any order.  No LDS.
#include "common.hpp"
#include "occ_math.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kRows = 4;                 // rows per lane and trip
// Every wave ends in three atomics on the same three words, and those serialise: at 2^20 rows a cap of 1024 workgroups
// took 0.119 ms per call, 512 0.078, 256 0.051, 128 0.041, 64 0.048 (MI355X, memset and host side included).  The
// rows beyond one pass take further trips of the grid-stride loop.
constexpr int kMaxBlocks = 128;
constexpr int kOutside = 1, kObserved = 2, kUnmatched = 4;

typedef long long ll2 __attribute__((ext_vector_type(2)));

template <bool kVec>
__global__ void __launch_bounds__(kBlock)
occ_loss_masks_kernel(const float* __restrict__ xyz, const float* __restrict__ box_size, const float* __restrict__ score,
                      const float* __restrict__ ori_logits, const int64_t* __restrict__ labels, int64_t N, int64_t K,
                      float score_thresh, float pos_thresh, int flags, float* __restrict__ weights,
                      uint8_t* __restrict__ unmatched, unsigned long long* __restrict__ counts) {
  const bool f_out = flags & kOutside, f_obs = flags & kObserved, f_unm = flags & kUnmatched;
  const int64_t groups = (N + kRows - 1) / kRows;
  unsigned long long n_w = 0, n_u = 0, n_uw = 0;
  // (base is uniform over the block: every lane of a wave reaches the ballots)
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < groups; base += (int64_t)gridDim.x * kBlock) {
    const int64_t r0 = (base + threadIdx.x) * kRows;
    bool w[kRows] = {false, false, false, false}, u[kRows] = {false, false, false, false};
    if (r0 < N) {
      const int n = N - r0 < kRows ? (int)(N - r0) : kRows;
      const bool wide = kVec && n == kRows;
      float p[kRows * 3] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      float lg[kRows] = {0.f, 0.f, 0.f, 0.f};
      bool lab[kRows] = {false, false, false, false};
      if (wide) {
        if (f_out) {
          const float4* q = reinterpret_cast<const float4*>(xyz + r0 * 3);
          const float4 a = q[0], b = q[1], c = q[2];
          p[0] = a.x, p[1] = a.y, p[2] = a.z, p[3] = a.w, p[4] = b.x, p[5] = b.y, p[6] = b.z, p[7] = b.w;
          p[8] = c.x, p[9] = c.y, p[10] = c.z, p[11] = c.w;
        }
        if (f_obs || f_unm) {
          const float4 l = *reinterpret_cast<const float4*>(ori_logits + r0);
          lg[0] = l.x, lg[1] = l.y, lg[2] = l.z, lg[3] = l.w;
        }
        if (f_unm) {
          const ll2* q = reinterpret_cast<const ll2*>(labels + r0);
          const ll2 a = q[0], b = q[1];
          lab[0] = a.x == 1, lab[1] = a.y == 1, lab[2] = b.x == 1, lab[3] = b.y == 1;
        }
      } else {
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
          if (j < n) {
            if (f_out) p[j * 3 + 0] = xyz[(r0 + j) * 3 + 0], p[j * 3 + 1] = xyz[(r0 + j) * 3 + 1], p[j * 3 + 2] = xyz[(r0 + j) * 3 + 2];
            if (f_obs || f_unm) lg[j] = ori_logits[r0 + j];
            if (f_unm) lab[j] = labels[r0 + j] == 1;
          }
        }
      }
      int64_t roi = r0 / K, rem = r0 - roi * K;   // (N > 0 here, so K > 0)
      bool confident = false;
      float hx = 0.f, hy = 0.f, hz = 0.f;
      bool fresh = true;
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        if (j < n) {
          if (fresh) {   // the first row, and the first row of the next RoI (roi < M: row r0 + j < N = M * K)
            confident = score[roi] > score_thresh;
            if (f_out) hx = box_size[roi * 3 + 0] / 2.0f, hy = box_size[roi * 3 + 1] / 2.0f, hz = box_size[roi * 3 + 2] / 2.0f;
            fresh = false;
          }
          bool keep = confident;
          if (f_out) {
            const float x = p[j * 3 + 0], y = p[j * 3 + 1], z = p[j * 3 + 2];
            keep = keep && (x >= -hx) && (x <= hx) && (y >= -hy) && (y <= hy) && (z >= -hz) && (z <= hz);
          }
          bool cls = false;
          if (f_obs || f_unm) cls = ococc_occupied(lg[j], pos_thresh);   // ATen's f32 sigmoid; false for NaN
          if (f_obs) keep = keep && !cls;
          w[j] = keep;
          u[j] = f_unm && (lab[j] != cls);
          if (++rem == K) rem = 0, ++roi, fresh = true;
        }
      }
      if (wide) {
        *reinterpret_cast<float4*>(weights + r0) = make_float4(w[0] ? 1.f : 0.f, w[1] ? 1.f : 0.f, w[2] ? 1.f : 0.f, w[3] ? 1.f : 0.f);
        if (f_unm)
          *reinterpret_cast<uint32_t*>(unmatched + r0) = (uint32_t)u[0] | ((uint32_t)u[1] << 8) | ((uint32_t)u[2] << 16) | ((uint32_t)u[3] << 24);
      } else {
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
          if (j < n) {
            weights[r0 + j] = w[j] ? 1.f : 0.f;
            if (f_unm) unmatched[r0 + j] = (uint8_t)u[j];
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      n_w += (unsigned long long)__popcll(__ballot(w[j]));
      if (f_unm) {   // (wave-uniform)
        n_u += (unsigned long long)__popcll(__ballot(u[j]));
        n_uw += (unsigned long long)__popcll(__ballot(u[j] && w[j]));
      }
    }
  }
  if ((threadIdx.x & 63) == 0) {
    if (n_w) atomicAdd(counts + 0, n_w);
    if (n_u) atomicAdd(counts + 1, n_u);
    if (n_uw) atomicAdd(counts + 2, n_uw);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int64_t ococc_occ_loss_masks_pass_rows(void) { return (int64_t)kMaxBlocks * kBlock * kRows; }

extern "C" int ococc_occ_loss_masks_f32(const float* xyz, const float* box_size, const float* score, const float* ori_logits,
                                        const int64_t* labels, int64_t M, int64_t K, float score_thresh, float pos_thresh,
                                        int32_t flags, float* weights, uint8_t* unmatched, int64_t* counts,
                                        ococc_stream_t stream) {
  OCOCC_REQUIRE(M >= 0 && K >= 0, "M < 0 or K < 0");
  OCOCC_REQUIRE((flags & ~(kOutside | kObserved | kUnmatched)) == 0, "flags beyond outside (1) | observed (2) | unmatched (4)");
  OCOCC_REQUIRE(counts, "null pointer");
  OCOCC_REQUIRE(K == 0 || M <= INT64_MAX / K, "M * K overflows");
  OCOCC_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), (hipStream_t)stream));
  const int64_t N = M * K;
  if (N == 0) return OCOCC_OK;
  OCOCC_REQUIRE(score && weights, "null pointer");
  OCOCC_REQUIRE(!(flags & kOutside) || (xyz && box_size), "the outside flag needs xyz and box_size");
  OCOCC_REQUIRE(!(flags & (kObserved | kUnmatched)) || ori_logits, "the observed / unmatched flags need ori_logits");
  OCOCC_REQUIRE(!(flags & kUnmatched) || (labels && unmatched), "the unmatched flag needs labels and the unmatched output");
  int64_t grid = ococc_cdiv(N, (int64_t)kBlock * kRows);
  if (grid > kMaxBlocks) grid = kMaxBlocks;
  const bool vec = aligned16(xyz) && aligned16(ori_logits) && aligned16(labels) && aligned16(weights) && aligned16(unmatched);
  auto* c = reinterpret_cast<unsigned long long*>(counts);
  if (vec)
    hipLaunchKernelGGL(occ_loss_masks_kernel<true>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, xyz, box_size,
                       score, ori_logits, labels, N, K, score_thresh, pos_thresh, (int)flags, weights, unmatched, c);
  else
    hipLaunchKernelGGL(occ_loss_masks_kernel<false>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, xyz, box_size,
                       score, ori_logits, labels, N, K, score_thresh, pos_thresh, (int)flags, weights, unmatched, c);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}
