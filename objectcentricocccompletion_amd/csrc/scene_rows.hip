// One sensor frame's scene cloud into the step rows of online inference (TrackletRoIHeadOCC.simple_test_scene_step): per
// (enlarged) tracklet box the points inside it, in the cloud's order, moved into the box's own fixed frame, range-filtered,
// capped and decorated -- what the offline chain makes of a frame with tools/ctrl/generate_track_input.py:84-99 (the crop),
// LoadTrackletPoints (tracklet_pipelines.py:26-91: the cap), TrackletPoseTransform (tracklet_pipelines.py:228-303),
// PointDecoration and PointsRangeFilter, each a pass of its own over the points.  Here: one count launch, one read-back of
// counts [n], one fill launch that writes the ROWS (xyz, features, row index), not indices.
//
// The plan is that of tracklet_crop.hip, and the split, the staged boxes, the wave tile of points and the box test are
// the same code (box_crop.hpp): a workgroup of 4 waves takes 4096 consecutive points (and, by blockIdx.y, a span of the
// boxes: the points of one frame alone would leave most CUs idle -- box_span), each wave 1024 consecutive ones, read once
// per pass however many boxes there are; the boxes are staged 64 at a time in LDS, here with the box's 3x4 matrix.  Per box
// and round one ballot: its popcount is the count, the popcount below the lane the rank -- (wave tile, round, lane) is
// ascending point order, so no sort.  The count pass leaves the per-(wave tile, box) counts in the workspace
// [wave tiles, n] i32 (box-minor); the fill pass sums the earlier wave tiles in front of its own ranks.
//
// Membership of point p in box b, the same in both passes:
//   1. StagedBox::holds on the UNTRANSFORMED point; a NaN z passes it and is dropped by the range, when one is given.
//   2. with a range: the WRITTEN xyz strictly inside (x0, y0, z0, x1, y1, z1) (PointsRangeFilter).
// The written xyz: with transforms, row b's row-major 3x4 matrix m applied as x' = fmaf(z, m02, fmaf(y, m01, fmaf(x, m00,
// m03))) (y', z' with rows 1, 2); the identity returns the input bits (a -0.0 comes out as +0.0); without, the input bits.
//
// Cap (fill only; counts stay uncapped): box b has m = scan_all[b+1] - scan_all[b] members; with cap > 0 and m > cap its
// member j (cloud order) is kept iff (j+1)*cap/m > j*cap/m (int64 floor division) and goes to place j*cap/m of the box --
// exactly cap rows, ascending, an even pick where LoadTrackletPoints draws a random subset.
//
// Algorithmic bytes per pass: N * 12 B of xyz per span of boxes (rows C * 4 B apart: N * C * 4 B of cache lines, 24 B at
// C = 6; the spans after the first read them from L2), n * (28 + 48) B
// of boxes and matrices per workgroup (L2); count: + T * n * 4 B workspace out, n * 8 B counts (integer atomics, the only
// ones); fill: + about T/2 * n * 4 B workspace in per wave tile (L2), M * A * 4 B of attributes in (the lines of the xyz) and
// M * (12 + (A + K) * 4 + 8) B of rows out.  T = ceil(N / 1024) wave tiles, M = scan_out[n].  Vector stores only.
//
// Several frames per call (ococc_scene_rows_frames_count / _fill; TrackletRoIHeadOCC.simple_test_scene_steps): the same
// kernel with blockIdx.y = frame, as tracklet_crop.hip has it -- the clouds back to back with cloud_offsets [F+1], the
// boxes grouped by frame with box_offsets [F+1], and box b tested against the points of ITS frame only, so the work is
// sum_f N_f * n_f and not N * n.  blockIdx.z splits the frame's boxes by the rule of box_span over ALL frames' workgroups:
// at one frame the launch is the one-cloud launch, from about 14 frames of 150 000 points on the split is gone.  The
// workspace is [wave tiles of the LARGEST frame, n].  The output is in the CALLER's row order, not frame-major: the host,
// which has the counts, gives every box its first output row (box_starts) and its total (box_totals, for the pick), the
// kernel writes row caller_rows[b] -- straight to the final places, no gather afterwards.  Per pass the bytes are those
// above summed over the frames, plus 32 B of offsets per workgroup and, in the fill pass, n * 24 B of starts, totals
// and caller rows where the one-cloud pass reads n * 16 B of scans.
#include "common.hpp"
#include "box_crop.hpp"

namespace {

constexpr int kWaves = kCropWaves;
constexpr int kBlockTile = kCropBlockTile;
constexpr int kChunk = kCropChunk;

struct Range6 {
  float v[6];
};

// What the many-cloud exports add (FRAMES; all null / 0 otherwise): where each frame's points and boxes lie, the
// caller's row number of every box, and the rows of the output
struct FrameArgs {
  const int64_t* cloud_offsets;   // [frames + 1]
  const int64_t* box_offsets;     // [frames + 1]
  const int64_t* caller_rows;     // [nb] (fill)
  int64_t num_out;                // (fill)
};

// XR: a transform or a range is given (without either, the test is the box's alone and needs fewer registers).
// FRAMES: blockIdx.y = frame, blockIdx.z = a span of the frame's boxes; `n` is then the points of ALL frames and the
// frame's own are cloud_offsets[f] .. cloud_offsets[f+1]; the boxes are frame-major, the workspace is [wave tiles of the
// largest frame, nb], and in the fill pass scan_all is the boxes' totals [nb] and scan_out their first output rows [nb]
// (the output is in the caller's row order, which the host scans).  Otherwise: one cloud, blockIdx.y = a span of the boxes.
template <bool FILL, bool XR, bool FRAMES>
__global__ void __launch_bounds__(64 * kWaves)
scene_rows_kernel(const float* __restrict__ points, int64_t n, int32_t C, const float* __restrict__ boxes, int32_t nb,
                  int32_t span, const float* __restrict__ transforms, Range6 range, int32_t has_range, int32_t* __restrict__ tile_counts,
                  unsigned long long* __restrict__ counts, int32_t A, const float* __restrict__ row_feats, int32_t K,
                  int64_t cap, const int64_t* __restrict__ scan_all, const int64_t* __restrict__ scan_out,
                  float* __restrict__ out_xyz, float* __restrict__ out_feats, int64_t* __restrict__ out_row, FrameArgs fr) {
  __shared__ BoxChunk sb;
  __shared__ float sm[12][kChunk];   // the box's 3x4 matrix, row-major
  int b_begin = 0, b_end = 0;        // this workgroup's boxes
  if (FRAMES) {
    const int f = blockIdx.y;
    const int64_t p0 = fr.cloud_offsets[f], p1 = fr.cloud_offsets[f + 1];
    const int64_t b0 = fr.box_offsets[f], b1 = fr.box_offsets[f + 1];
    if (p0 < 0 || p1 > n || p1 <= p0 || b0 < 0 || b1 > nb || b1 <= b0) return;   // an empty frame, or offsets that lie
    if ((int64_t)blockIdx.z * span >= b1 - b0) return;
    b_begin = (int)(b0 + (int64_t)blockIdx.z * span);
    b_end = (int)min(b1, (int64_t)b_begin + span);
    points += p0 * C;
    n = p1 - p0;
  }
  const int64_t tile0 = (int64_t)blockIdx.x * kBlockTile;
  if (tile0 >= n) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t w0 = tile0 + (int64_t)wave * kCropWaveTile;   // index of this wave's first point (in its cloud)
  const int64_t wt = (int64_t)blockIdx.x * kWaves + wave;  // wave tile (of its cloud)
  const bool xform = XR && transforms != nullptr;

  WavePoints p;
  p.load(points, C, n, w0, lane);

  if (!FRAMES) {   // [blockIdx.y * span, b_end)
    b_begin = blockIdx.y * span;
    b_end = (int)min((int64_t)nb, ((int64_t)blockIdx.y + 1) * span);
  }
  for (int c0 = b_begin; c0 < b_end; c0 += kChunk) {
    const int cn = min(kChunk, b_end - c0);
    __syncthreads();
    if (tid < cn) {
      sb.stage(tid, boxes + (int64_t)(c0 + tid) * 7);
      if (xform) {
        const float* m = transforms + (int64_t)(c0 + tid) * 12;
#pragma unroll
        for (int k = 0; k < 12; ++k) sm[k][tid] = m[k];
      }
    }
    __syncthreads();

    // lane j: where box c0 + j's members of this wave tile start (in members of the box), the box's member count, its
    // first output row and its output end
    int64_t base = 0, total = 0, start = 0, end = 0;
    if (FILL) {
      if (lane < cn) {
        const int64_t b = c0 + lane;
        if (FRAMES) {
          total = scan_all[b], start = scan_out[b];
          end = start + ((cap > 0 && total > cap) ? cap : total);
          if (start < 0 || end > fr.num_out) end = start = 0;   // (a start the host did not make: nothing is written)
        } else {
          total = scan_all[b + 1] - scan_all[b];
          start = scan_out[b], end = scan_out[b + 1];
        }
        for (int64_t k = 0; k < wt; ++k) base += tile_counts[k * nb + b];
      }
    }
    int mine = 0;                // lane j: count of box c0 + j in this wave tile
    for (int j = 0; j < cn; ++j) {
      const StagedBox box = sb.get(j);
      const int64_t base_j = FILL ? __shfl(base, j, 64) : 0, total_j = FILL ? __shfl(total, j, 64) : 0;
      const int64_t start_j = FILL ? __shfl(start, j, 64) : 0, end_j = FILL ? __shfl(end, j, 64) : 0;
      const bool pick = FILL && cap > 0 && total_j > cap;   // wave-uniform
      int cnt = 0;               // wave-uniform
#pragma unroll
      for (int r = 0; r < kCropRounds; ++r) {
        bool in = box.holds(p.x[r], p.y[r], p.z[r]);
        float ox = p.x[r], oy = p.y[r], oz = p.z[r];
        if (XR && __ballot(in)) {   // wave-uniform: most (box, round) pairs have no point in the box
          if (in && xform) {
            ox = fmaf(p.z[r], sm[2][j], fmaf(p.y[r], sm[1][j], fmaf(p.x[r], sm[0][j], sm[3][j])));
            oy = fmaf(p.z[r], sm[6][j], fmaf(p.y[r], sm[5][j], fmaf(p.x[r], sm[4][j], sm[7][j])));
            oz = fmaf(p.z[r], sm[10][j], fmaf(p.y[r], sm[9][j], fmaf(p.x[r], sm[8][j], sm[11][j])));
          }
          if (in && has_range)
            in = (ox > range.v[0]) & (oy > range.v[1]) & (oz > range.v[2]) & (ox < range.v[3]) & (oy < range.v[4]) &
                 (oz < range.v[5]);
        }
        const unsigned long long bal = __ballot(in);
        if (FILL && in) {
          const int64_t jm = base_j + cnt + wave_rank(bal, lane);   // member index in the box
          int64_t pos = jm;
          bool keep = jm < total_j;            // (counts and scans of the same input: always)
          if (pick) {
            pos = jm * cap / total_j;
            keep = keep && (jm + 1) * cap / total_j > pos;
          }
          pos += start_j;
          if (keep && pos < end_j) {           // (pos < end_j: scan_out of the same counts and cap)
            const int64_t i = w0 + r * 64 + lane;
            float* o = out_xyz + pos * 3;
            o[0] = ox, o[1] = oy, o[2] = oz;
            out_row[pos] = FRAMES ? fr.caller_rows[c0 + j] : (int64_t)(c0 + j);
            float* f = out_feats + pos * (A + K);
            const float* q = points + i * C + 3;
            for (int a = 0; a < A; ++a) f[a] = q[a];
            const float* rf = row_feats + (int64_t)(c0 + j) * K;
            for (int k = 0; k < K; ++k) f[A + k] = rf[k];
          }
        }
        cnt += __popcll(bal);
      }
      if (lane == j) mine = cnt;
    }
    if (!FILL && lane < cn) {
      const int64_t b = c0 + lane;
      tile_counts[wt * nb + b] = mine;   // zeros too: the fill pass reads every earlier wave tile
      if (mine) atomicAdd(&counts[b], (unsigned long long)mine);
    }
  }
}

// ---- the host side: one check and one pass behind the four exports (as merge_count / merge_fill, occ_merge.hip)
#define ROWS_REQUIRE(cond, msg)                               \
  do {                                                        \
    if (!(cond)) return ococc_fail(OCOCC_EINVAL, fn, msg);    \
  } while (0)
#define ROWS_HIP(call)                                                                   \
  do {                                                                                   \
    hipError_t e__ = (call);                                                             \
    if (e__ != hipSuccess) return ococc_fail(OCOCC_EHIP, fn, hipGetErrorString(e__));    \
  } while (0)

// An export's arguments.  The one-cloud exports (`many` false) have one frame, and its largest frame is the cloud; the
// count exports leave what follows `fr` zero.
struct RowsArgs {
  const float* points;
  int64_t n;
  int32_t c;
  const float* boxes;
  int64_t b;
  const float *transforms, *range;
  const void* workspace;
  int64_t workspace_bytes;
  bool many;
  int32_t frames;
  int64_t max_points, max_boxes;   // of the largest frame
  FrameArgs fr;
  int32_t A, K;   // attr_dims, row_feat_dim
  const float* row_feats;
  int64_t cap;
  const int64_t *scan_all, *scan_out;   // many: the boxes' totals and first output rows
  float *out_xyz, *out_feats;
  int64_t* out_row;
};

// 1: nothing to do (an empty cloud or no boxes), 0: launch, < 0: reported
int rows_check(const char* fn, const RowsArgs& in) {
  if (in.n < 0 || in.b < 0 || in.frames < 0 || in.max_points < 0 || in.max_boxes < 0)
    return ococc_fail(OCOCC_EINVAL, fn, "negative size");
  if (in.n > 2147483647LL || in.b > 2147483647LL) return ococc_fail(OCOCC_EINVAL, fn, "at most 2^31 - 1 points and boxes");
  if (in.max_points > in.n || in.max_boxes > in.b)
    return ococc_fail(OCOCC_EINVAL, fn, "max_frame_points > num_points or max_frame_boxes > num_boxes");
  if (in.c < 3) return ococc_fail(OCOCC_EINVAL, fn, "points need at least 3 columns");
  if (in.frames > 65535) return ococc_fail(OCOCC_EINVAL, fn, "at most 65535 frames per call");
  if (in.b == 0 || in.n == 0 || in.frames == 0 || in.max_points == 0 || in.max_boxes == 0) return 1;
  if (!in.points || !in.boxes || !in.workspace || (in.many && (!in.fr.cloud_offsets || !in.fr.box_offsets)))
    return ococc_fail(OCOCC_EINVAL, fn, "null pointer");
  if (in.workspace_bytes < ococc_scene_rows_workspace_bytes(in.max_points, in.b))
    return ococc_fail(OCOCC_EINVAL, fn,
                      in.many ? "workspace too small: ococc_scene_rows_workspace_bytes(max_frame_points, num_boxes)"
                              : "workspace too small: ococc_scene_rows_workspace_bytes(num_points, num_boxes)");
  return OCOCC_OK;
}

// Boxes per workgroup (blockIdx.y takes `span` consecutive boxes).  One sensor frame is few workgroups along the points
// (37 at 150 000 points), so the boxes are split until about two workgroups per CU are in flight, 8 boxes at the least;
// every split re-reads the cloud (L2), which is small beside the box tests it spreads.
// Several frames: n and b are the largest frame's, and every frame brings its workgroups along the points.
int32_t box_span(int64_t n, int64_t b, int64_t frames = 1) {
  const int64_t tiles = ococc_cdiv(n, kBlockTile) * frames;
  int64_t parts = ococc_cdiv(512, tiles);
  if (parts > ococc_cdiv(b, 8)) parts = ococc_cdiv(b, 8);
  if (parts > 65535) parts = 65535;
  return (int32_t)ococc_cdiv(b, parts < 1 ? 1 : parts);
}

Range6 range_arg(const float* range) {
  Range6 r = {{0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
  if (range) memcpy(r.v, range, sizeof(r.v));
  return r;
}

// Either pass: the checks, then the launch.  Grid: blockIdx.x the workgroups along the (largest frame's) points; one cloud:
// y the spans of the boxes; many: y the frame, z the spans of the frame's boxes.
int rows_pass(bool fill, const char* fn, const RowsArgs& in, int64_t* counts, hipStream_t stream) {
  const int rc = rows_check(fn, in);
  if (rc < 0) return rc;
  if (!fill && in.b > 0) {
    ROWS_REQUIRE(counts, "null counts");
    ROWS_HIP(hipMemsetAsync(counts, 0, in.b * sizeof(int64_t), stream));
  }
  if (fill) {
    ROWS_REQUIRE(in.A >= 0 && in.K >= 0 && 3 + (int64_t)in.A <= in.c,
                 "attr_dims and row_feat_dim are >= 0, and 3 + attr_dims <= point_dim");
    ROWS_REQUIRE(in.cap <= 2147483647LL, "max_points is at most 2^31 - 1 (<= 0: no cap)");
    ROWS_REQUIRE(in.fr.num_out >= 0, "negative num_out");
  }
  if (rc == 1 || (fill && in.many && in.fr.num_out == 0)) return OCOCC_OK;
  if (fill) {
    ROWS_REQUIRE(in.scan_all && in.scan_out && in.out_xyz && in.out_row && (in.fr.caller_rows || !in.many),
                 in.many ? "null caller_rows, box_totals, box_starts, out_xyz or out_row"
                         : "null scan_all, scan_out, out_xyz or out_row");
    ROWS_REQUIRE(in.K == 0 || in.row_feats, "null row_feats");
    ROWS_REQUIRE(in.A + in.K == 0 || in.out_feats, "null out_feats");
  }
  static const decltype(&scene_rows_kernel<false, true, false>) kernels[2][2][2] = {   // [many][fill][no transforms, no range]
      {{scene_rows_kernel<false, true, false>, scene_rows_kernel<false, false, false>},
       {scene_rows_kernel<true, true, false>, scene_rows_kernel<true, false, false>}},
      {{scene_rows_kernel<false, true, true>, scene_rows_kernel<false, false, true>},
       {scene_rows_kernel<true, true, true>, scene_rows_kernel<true, false, true>}}};
  const auto kernel = kernels[in.many][fill][!(in.transforms || in.range)];
  const int32_t span = box_span(in.max_points, in.max_boxes, in.frames);
  const unsigned tiles = (unsigned)ococc_cdiv(in.max_points, kBlockTile), spans = (unsigned)ococc_cdiv(in.max_boxes, span);
  hipLaunchKernelGGL(kernel, in.many ? dim3(tiles, (unsigned)in.frames, spans) : dim3(tiles, spans), dim3(64 * kWaves), 0,
                     stream, in.points, in.n, in.c, in.boxes, (int32_t)in.b, span, in.transforms, range_arg(in.range),
                     (int32_t)(in.range != nullptr), (int32_t*)const_cast<void*>(in.workspace), (unsigned long long*)counts,
                     in.A, in.row_feats, in.K, in.cap, in.scan_all, in.scan_out, in.out_xyz, in.out_feats, in.out_row, in.fr);
  ROWS_HIP(hipGetLastError());
  return OCOCC_OK;
}

}  // namespace

extern "C" int64_t ococc_scene_rows_workspace_bytes(int64_t num_points, int64_t num_boxes) {
  if (num_points < 0 || num_boxes < 0) return -1;
  return ococc_cdiv(num_points, kBlockTile) * kWaves * num_boxes * (int64_t)sizeof(int32_t);
}

extern "C" int ococc_scene_rows_count(const float* points, int64_t num_points, int32_t point_dim,
                                      const float* crop_boxes, int64_t num_boxes, const float* transforms,
                                      const float* range, int64_t* counts, void* workspace, int64_t workspace_bytes,
                                      ococc_stream_t stream) {
  return rows_pass(false, __func__, RowsArgs{points, num_points, point_dim, crop_boxes, num_boxes, transforms, range,
                                             workspace, workspace_bytes, false, 1, num_points, num_boxes},
                          counts, (hipStream_t)stream);
}

extern "C" int ococc_scene_rows_fill(const float* points, int64_t num_points, int32_t point_dim, const float* crop_boxes,
                                     int64_t num_boxes, const float* transforms, const float* range, int32_t attr_dims,
                                     const float* row_feats, int32_t row_feat_dim, int64_t max_points,
                                     const int64_t* scan_all, const int64_t* scan_out, float* out_xyz, float* out_feats,
                                     int64_t* out_row, const void* workspace, int64_t workspace_bytes,
                                     ococc_stream_t stream) {
  return rows_pass(true, __func__, RowsArgs{points, num_points, point_dim, crop_boxes, num_boxes, transforms, range,
                                            workspace, workspace_bytes, false, 1, num_points, num_boxes, FrameArgs{},
                                            attr_dims, row_feat_dim, row_feats, max_points, scan_all, scan_out, out_xyz,
                                            out_feats, out_row},
                         nullptr, (hipStream_t)stream);
}

extern "C" int ococc_scene_rows_frames_count(const float* points, int64_t num_points, int32_t point_dim,
                                             const int64_t* cloud_offsets, const float* crop_boxes, int64_t num_boxes,
                                             const int64_t* box_offsets, int32_t frames, int64_t max_frame_points,
                                             int64_t max_frame_boxes, const float* transforms, const float* range,
                                             int64_t* counts, void* workspace, int64_t workspace_bytes,
                                             ococc_stream_t stream) {
  return rows_pass(false, __func__, RowsArgs{points, num_points, point_dim, crop_boxes, num_boxes, transforms, range,
                                             workspace, workspace_bytes, true, frames, max_frame_points, max_frame_boxes,
                                             FrameArgs{cloud_offsets, box_offsets, nullptr, 0}},
                          counts, (hipStream_t)stream);
}

extern "C" int ococc_scene_rows_frames_fill(const float* points, int64_t num_points, int32_t point_dim,
                                            const int64_t* cloud_offsets, const float* crop_boxes, int64_t num_boxes,
                                            const int64_t* box_offsets, int32_t frames, int64_t max_frame_points,
                                            int64_t max_frame_boxes, const float* transforms, const float* range,
                                            int32_t attr_dims, const float* row_feats, int32_t row_feat_dim,
                                            const int64_t* caller_rows, int64_t max_points, const int64_t* box_totals,
                                            const int64_t* box_starts, int64_t num_out, float* out_xyz,
                                            float* out_feats, int64_t* out_row, const void* workspace,
                                            int64_t workspace_bytes, ococc_stream_t stream) {
  return rows_pass(true, __func__, RowsArgs{points, num_points, point_dim, crop_boxes, num_boxes, transforms, range,
                                            workspace, workspace_bytes, true, frames, max_frame_points, max_frame_boxes,
                                            FrameArgs{cloud_offsets, box_offsets, caller_rows, num_out}, attr_dims,
                                            row_feat_dim, row_feats, max_points, box_totals, box_starts, out_xyz,
                                            out_feats, out_row},
                         nullptr, (hipStream_t)stream);
}
