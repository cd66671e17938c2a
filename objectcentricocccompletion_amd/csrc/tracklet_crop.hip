// Points of many frames into the (enlarged) tracklet boxes of their frames, the cloud's order kept: the crop of CTRL's
// track-input generation (tools/ctrl/generate_track_input.py:84-99).  The reference does, per frame and per box, one
// upload of the box, one points_in_boxes launch over the whole cloud, one boolean-mask compaction and one
// device-to-host copy.  Here: one count launch, one read-back of counts [B], one fill launch per batch of frames.
//
// Membership is check_pt_in_box3d, each box on its own, so a point may fall into several (overlapping, enlarged) boxes.
// The test, the staged boxes and the wave tile of points are box_crop.hpp's, shared with scene_rows.hip.
//
// Work split: blockIdx.y = frame, a workgroup of 4 waves takes 4096 consecutive points of the frame, each wave 1024
// consecutive ones ("wave tile": 16 rounds of 64, lane = point, kept in registers, every point read ONCE per pass
// however many boxes the frame has).  The frame's boxes are staged 64 at a time in LDS once per workgroup and read as
// broadcasts.  Per box and round one ballot: its popcount is the count, the popcount below the lane the rank -- (wave
// tile, round, lane) IS ascending point order, so no sort.  Two levels: the count pass leaves the per-(wave tile, box)
// counts in the workspace [wave tiles per frame, B] i32 (box-minor: the fill pass reads 64 boxes of one wave tile as one
// 256 B line); the fill pass sums the earlier wave tiles of its frame in front of its own ranks.
//
// Algorithmic bytes per pass: N * 12 B of xyz (the rows are C * 4 B apart, so N * C * 4 B of cache lines move: 24 B
// at C = 6), B * 28 B of boxes per workgroup (L2);  count: + T * B * 4 B workspace out, B * 8 B counts;
// fill: + about T/2 * B * 4 B workspace in per wave tile (L2) and sum(counts) * 8 B of indices out.
// T = wave tiles of the largest frame.  Vector stores only.
//
// Third mode, non-empty flags (tools/ctrl/remove_empty.py:115-134 with group_size 1: one upload, one points_in_boxes
// launch, one torch.unique and one read-back per box): the same membership test, but per box and round the ballot is
// only tested against zero, the rounds of a box stop at its first hit, and one lane stores 1 into flags [B] i32
// (zero-filled by the caller side of the export; a plain store of the same value from every wave tile that hits).
// No workspace, no second pass.  Algorithmic bytes: N * 12 B of xyz in, B * 4 B out.
#include "common.hpp"
#include "box_crop.hpp"

namespace {

constexpr int kWaves = kCropWaves;
constexpr int kBlockTile = kCropBlockTile;
constexpr int kChunk = kCropChunk;

enum CropMode { kCount = 0, kFill = 1, kFlag = 2 };

// tile_counts: the workspace of kCount / kFill; the flags [B] of kFlag
template <int MODE>
__global__ void __launch_bounds__(64 * kWaves)
tracklet_crop_kernel(const float* __restrict__ points, int32_t C, const int64_t* __restrict__ point_offsets,
                     const float* __restrict__ boxes, const int64_t* __restrict__ box_offsets, int64_t B,
                     int32_t* __restrict__ tile_counts, unsigned long long* __restrict__ counts,
                     const int64_t* __restrict__ scan, int64_t* __restrict__ out_index) {
  __shared__ BoxChunk sb;
  const int f = blockIdx.y;
  const int64_t p0 = point_offsets[f], n = point_offsets[f + 1] - p0;
  const int64_t tile0 = (int64_t)blockIdx.x * kBlockTile;
  if (tile0 >= n) return;
  const int64_t b0 = box_offsets[f];
  const int nb = (int)(box_offsets[f + 1] - b0);
  if (nb <= 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t w0 = tile0 + (int64_t)wave * kCropWaveTile;   // frame-local index of this wave's first point
  const int64_t wt = (int64_t)blockIdx.x * kWaves + wave;      // wave tile of the frame

  WavePoints p;
  p.load(points + p0 * C, C, n, w0, lane);

  for (int c0 = 0; c0 < nb; c0 += kChunk) {
    const int cn = min(kChunk, nb - c0);
    __syncthreads();
    if (tid < cn) sb.stage(tid, boxes + (b0 + c0 + tid) * 7);
    __syncthreads();

    constexpr bool FILL = MODE == kFill;
    int64_t base = 0, end = 0;   // lane j: where box c0 + j's points of this wave tile start / the box's end
    if (FILL) {
      if (lane < cn) {
        const int64_t b = b0 + c0 + lane;
        base = scan[b], end = scan[b + 1];
        for (int64_t k = 0; k < wt; ++k) base += tile_counts[k * B + b];
      }
    }
    int mine = 0;                // lane j: count of box c0 + j in this wave tile
    for (int j = 0; j < cn; ++j) {
      const StagedBox box = sb.get(j);
      const int64_t base_j = FILL ? __shfl(base, j, 64) : 0, end_j = FILL ? __shfl(end, j, 64) : 0;
      int cnt = 0;               // wave-uniform
#pragma unroll
      for (int r = 0; r < kCropRounds; ++r) {
        const bool in = box.holds(p.x[r], p.y[r], p.z[r]);
        const unsigned long long bal = __ballot(in);
        if (MODE == kFlag) {
          if (bal) {
            cnt = 1;
            break;
          }
          continue;
        }
        if (FILL && in) {
          const int64_t pos = base_j + cnt + wave_rank(bal, lane);
          if (pos < end_j) out_index[pos] = w0 + r * 64 + lane;   // (pos < end_j: counts and scan of the same input)
        }
        cnt += __popcll(bal);
      }
      if (lane == j) mine = cnt;
    }
    if (MODE == kFlag) {
      if (lane < cn && mine) tile_counts[b0 + c0 + lane] = 1;
    } else if (!FILL && lane < cn) {
      const int64_t b = b0 + c0 + lane;
      tile_counts[wt * B + b] = mine;   // zeros too: the fill pass reads every earlier wave tile of the frame
      if (mine) atomicAdd(&counts[b], (unsigned long long)mine);
    }
  }
}

int crop_check(const float* points, int64_t n, int32_t c, const int64_t* point_offsets, const float* boxes, int64_t b,
               const int64_t* box_offsets, int32_t frames, int64_t max_frame_points, const void* workspace,
               int64_t workspace_bytes, const char* fn, bool needs_workspace = true) {
  if (n < 0 || b < 0 || frames < 0 || max_frame_points < 0 || max_frame_points > n)
    return ococc_fail(OCOCC_EINVAL, fn, "negative size, or max_frame_points > num_points");
  if (c < 3) return ococc_fail(OCOCC_EINVAL, fn, "points need at least 3 columns");
  if (frames > 65535) return ococc_fail(OCOCC_EINVAL, fn, "at most 65535 frames per call");
  if (b == 0 || n == 0 || frames == 0) return 1;
  if (!points || !point_offsets || !boxes || !box_offsets || (needs_workspace && !workspace))
    return ococc_fail(OCOCC_EINVAL, fn, "null pointer");
  if (!needs_workspace) return OCOCC_OK;
  const int64_t tiles = ococc_cdiv(max_frame_points, kBlockTile) * kWaves;
  if (workspace_bytes < tiles * b * (int64_t)sizeof(int32_t))
    return ococc_fail(OCOCC_EINVAL, fn, "workspace too small: ceil(max_frame_points / 4096) * 4 * num_boxes * 4 bytes");
  return OCOCC_OK;
}

}  // namespace

extern "C" int ococc_tracklet_crop_count(const float* points, int64_t num_points, int32_t point_dim,
                                         const int64_t* point_offsets, const float* boxes, int64_t num_boxes,
                                         const int64_t* box_offsets, int32_t frames, int64_t max_frame_points,
                                         int64_t* counts, void* workspace, int64_t workspace_bytes,
                                         ococc_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = crop_check(points, num_points, point_dim, point_offsets, boxes, num_boxes, box_offsets, frames,
                            max_frame_points, workspace, workspace_bytes, __func__);
  if (rc < 0) return rc;
  if (num_boxes > 0) {
    OCOCC_REQUIRE(counts, "null counts");
    OCOCC_HIP(hipMemsetAsync(counts, 0, num_boxes * sizeof(int64_t), stream));
  }
  if (rc == 1 || max_frame_points == 0) return OCOCC_OK;
  const dim3 grid((unsigned)ococc_cdiv(max_frame_points, kBlockTile), (unsigned)frames);
  hipLaunchKernelGGL(tracklet_crop_kernel<kCount>, grid, dim3(64 * kWaves), 0, stream, points, point_dim, point_offsets,
                     boxes, box_offsets, num_boxes, (int32_t*)workspace, (unsigned long long*)counts,
                     (const int64_t*)nullptr, (int64_t*)nullptr);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}

extern "C" int ococc_tracklet_crop_fill(const float* points, int64_t num_points, int32_t point_dim,
                                        const int64_t* point_offsets, const float* boxes, int64_t num_boxes,
                                        const int64_t* box_offsets, int32_t frames, int64_t max_frame_points,
                                        const int64_t* scan, const void* workspace, int64_t workspace_bytes,
                                        int64_t* out_index, ococc_stream_t stream_) {
  const int rc = crop_check(points, num_points, point_dim, point_offsets, boxes, num_boxes, box_offsets, frames,
                            max_frame_points, workspace, workspace_bytes, __func__);
  if (rc < 0) return rc;
  if (rc == 1 || max_frame_points == 0) return OCOCC_OK;
  OCOCC_REQUIRE(scan && out_index, "null scan or out_index");
  const dim3 grid((unsigned)ococc_cdiv(max_frame_points, kBlockTile), (unsigned)frames);
  hipLaunchKernelGGL(tracklet_crop_kernel<kFill>, grid, dim3(64 * kWaves), 0, (hipStream_t)stream_, points, point_dim,
                     point_offsets, boxes, box_offsets, num_boxes, (int32_t*)const_cast<void*>(workspace),
                     (unsigned long long*)nullptr, scan, out_index);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}

extern "C" int ococc_tracklet_nonempty(const float* points, int64_t num_points, int32_t point_dim,
                                       const int64_t* point_offsets, const float* boxes, int64_t num_boxes,
                                       const int64_t* box_offsets, int32_t frames, int64_t max_frame_points,
                                       int32_t* flags, ococc_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = crop_check(points, num_points, point_dim, point_offsets, boxes, num_boxes, box_offsets, frames,
                            max_frame_points, nullptr, 0, __func__, false);
  if (rc < 0) return rc;
  if (num_boxes > 0) {
    OCOCC_REQUIRE(flags, "null flags");
    OCOCC_HIP(hipMemsetAsync(flags, 0, num_boxes * sizeof(int32_t), stream));
  }
  if (rc == 1 || max_frame_points == 0) return OCOCC_OK;
  const dim3 grid((unsigned)ococc_cdiv(max_frame_points, kBlockTile), (unsigned)frames);
  hipLaunchKernelGGL(tracklet_crop_kernel<kFlag>, grid, dim3(64 * kWaves), 0, stream, points, point_dim, point_offsets,
                     boxes, box_offsets, num_boxes, flags, (unsigned long long*)nullptr, (const int64_t*)nullptr,
                     (int64_t*)nullptr);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}
