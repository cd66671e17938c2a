// Track extension of CTRL (tools/ctrl/extend_tracks.py over LiDARTracklet.frame_transform / set_velocity / extend /
// extend_all / shared2ego, mmdet3d/core/bbox/structures/lidar_tracklet.py:345-387, 452-498, 638-652, 669-791): every
// tracklet is moved into the frame of its first pose, gets the mean velocity of its first (last) observed boxes, is
// extended backward (and, for extend_all, forward) in time by a constant-velocity model and moved back into each
// frame's own ego pose.  The reference does this with a Python loop of a dozen small torch operators per tracklet;
// here all tracklets of a call are ONE launch.
//
// The PLAN (which tracklets are extended, by how many frames on either side, where their output rows start) is integer
// arithmetic on timestamps and is made on the host (ctrl_prep.plan_extension): the kernel receives, per tracklet, the
// number of frames added in front and behind and its output offset, so nothing is read back between planning and the
// launch and extend_length / min_length / extend_all never reach the device.
//
// Mapping: one wave per tracklet, four tracklets per workgroup.  Lane i takes the boxes i, i + 64, ... .  The velocity
// rows the mean needs are recomputed from the two boxes they difference (rows 0 and 1 are the same row, as
// set_velocity's cat([velo[:1], velo])) rather than staged in LDS: a tracklet has no length bound, the window is a
// handful of rows, and a row costs two 3x4 transforms; the mean is a wave reduction over shuffles in a fixed order.
// All 3x4 products, the inverses of the poses, sin / cos / atan2 and pow are float64; the result is rounded to float32
// ONCE, on store (the reference's float32 chain loses centimetres on poses kilometres from the origin).  The inverse
// is the affine one (cofactors of the 3x3 block, -R^-1 t): the float32 poses are orthonormal only to float32 rounding,
// and the reference inverts them as general matrices (torch.linalg.inv).
//
// Every output word has exactly one writer: no atomics, the same input gives the same bytes.  Vector stores only.
// Algorithmic bytes: sum L * (28 + 4 + 8) B of boxes / frame indices / scores in, sum L' * 64 B of poses (L2 after the
// first tracklet of a segment), sum L' * (28 + 8 + 4) B out.
#include "common.hpp"

namespace {

constexpr int kWaves = 4;

struct Affine {   // rows of [R | t]
  double m[12];
};

__device__ __forceinline__ Affine load_pose(const float* __restrict__ p) {
  Affine a;
#pragma unroll
  for (int i = 0; i < 12; ++i) a.m[i] = (double)p[i];
  return a;
}

__device__ __forceinline__ Affine inverse(const Affine& a) {
  const double* m = a.m;
  const double c00 = m[5] * m[10] - m[6] * m[9], c01 = m[6] * m[8] - m[4] * m[10], c02 = m[4] * m[9] - m[5] * m[8];
  const double det = m[0] * c00 + m[1] * c01 + m[2] * c02, r = 1.0 / det;
  Affine o;
  o.m[0] = c00 * r, o.m[1] = (m[2] * m[9] - m[1] * m[10]) * r, o.m[2] = (m[1] * m[6] - m[2] * m[5]) * r;
  o.m[4] = c01 * r, o.m[5] = (m[0] * m[10] - m[2] * m[8]) * r, o.m[6] = (m[2] * m[4] - m[0] * m[6]) * r;
  o.m[8] = c02 * r, o.m[9] = (m[1] * m[8] - m[0] * m[9]) * r, o.m[10] = (m[0] * m[5] - m[1] * m[4]) * r;
#pragma unroll
  for (int i = 0; i < 3; ++i) o.m[4 * i + 3] = -(o.m[4 * i] * m[3] + o.m[4 * i + 1] * m[7] + o.m[4 * i + 2] * m[11]);
  return o;
}

__device__ __forceinline__ Affine mul(const Affine& a, const Affine& b) {   // a @ b
  Affine o;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      o.m[4 * i + j] = a.m[4 * i] * b.m[j] + a.m[4 * i + 1] * b.m[4 + j] + a.m[4 * i + 2] * b.m[8 + j] + (j == 3 ? a.m[4 * i + 3] : 0.0);
  }
  return o;
}

struct Pose3 {
  double x, y, z, yaw;
};

// centre through mm, yaw from the heading vector (sin, cos, 0) through mm's rotation (frame_transform / shared2ego)
__device__ __forceinline__ Pose3 apply(const Affine& mm, const Pose3& b) {
  Pose3 o;
  o.x = mm.m[0] * b.x + mm.m[1] * b.y + mm.m[2] * b.z + mm.m[3];
  o.y = mm.m[4] * b.x + mm.m[5] * b.y + mm.m[6] * b.z + mm.m[7];
  o.z = mm.m[8] * b.x + mm.m[9] * b.y + mm.m[10] * b.z + mm.m[11];
  const double s = sin(b.yaw), c = cos(b.yaw);
  o.yaw = atan2(mm.m[0] * s + mm.m[1] * c, mm.m[4] * s + mm.m[5] * c);
  return o;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

struct Args {
  const float* boxes;
  const int32_t* offsets;
  const int32_t* frames;
  const int32_t* segments;
  const double* scores;
  const float* poses;
  const int64_t* timestamps;
  const int32_t* seg_offsets;
  const int32_t* num_back;
  const int32_t* num_fwd;
  const int32_t* out_offsets;
  float* out_boxes;
  double* out_scores;
  int32_t* out_frames;
  double score_multiplier;
  int32_t num_tracklets, num_segments, velo_window_size;
  int64_t total_in, total_out, total_frames;
};

__global__ void __launch_bounds__(64 * kWaves) track_extend_kernel(const Args a) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (t >= a.num_tracklets) return;
  const int64_t o0 = a.offsets[t];
  const int len = a.offsets[t + 1] - (int)o0;
  const int seg = a.segments[t];
  const int back = a.num_back[t], fwd = a.num_fwd[t];
  const int64_t q0 = a.out_offsets[t];
  // the host made all of these (ctrl_prep.extend_tracks_packed checks them); a tracklet they do not fit is left out
  if (len <= 0 || o0 < 0 || o0 + len > a.total_in || seg < 0 || seg >= a.num_segments || back < 0 || fwd < 0 || q0 < 0 ||
      q0 + back + len + fwd > a.total_out)
    return;
  const int64_t s0 = a.seg_offsets[seg];
  const int T = a.seg_offsets[seg + 1] - (int)s0;
  if (s0 < 0 || T <= 0 || s0 + T > a.total_frames) return;
  const int f_first = a.frames[o0], f_last = a.frames[o0 + len - 1];
  if (f_first - back < 0 || f_last + fwd >= T || f_first >= T || f_last < 0) return;
  const float* poses = a.poses + s0 * 16;
  const int64_t* ts = a.timestamps + s0;
  const int32_t* fr = a.frames + o0;
  const float* bx = a.boxes + o0 * 7;

  const Affine p_first = load_pose(poses + (int64_t)f_first * 16);
  const Affine w2s = inverse(p_first);   // world -> the shared frame

  auto in_range = [&](int f) { return f >= 0 && f < T; };
  auto shared = [&](int i) {             // box i of the tracklet in the shared frame
    const float* b = bx + (int64_t)i * 7;
    const Pose3 ego = {(double)b[0], (double)b[1], (double)b[2], (double)b[6]};
    const int f = in_range(fr[i]) ? fr[i] : f_first;
    return apply(mul(w2s, load_pose(poses + (int64_t)f * 16)), ego);
  };
  auto velocity_sum = [&](int row0, int rows, double& vx, double& vy) {   // sum of the velocity rows [row0, row0 + rows)
    double sx = 0.0, sy = 0.0;
    for (int k = row0 + lane; k < row0 + rows; k += 64) {
      const int kk = k < 1 ? 1 : k;                                      // row 0 duplicates row 1
      const Pose3 hi = shared(kk), lo = shared(kk - 1);
      const int fh = in_range(fr[kk]) ? fr[kk] : f_first, fl = in_range(fr[kk - 1]) ? fr[kk - 1] : f_first;
      const double dt = (double)(ts[fh] - ts[fl]) / 1e6;
      sx += (hi.x - lo.x) / dt, sy += (hi.y - lo.y) / dt;
    }
    vx = wave_sum(sx), vy = wave_sum(sy);
  };
  auto store = [&](int64_t q, const Pose3& s, const Affine& s2e, const float* size_of, int frame, double score) {
    const Pose3 e = apply(s2e, s);
    float* o = a.out_boxes + q * 7;
    o[0] = (float)e.x, o[1] = (float)e.y, o[2] = (float)e.z;
    o[3] = size_of[3], o[4] = size_of[4], o[5] = size_of[5];
    o[6] = (float)e.yaw;
    a.out_scores[q] = score;
    a.out_frames[q] = frame;
  };

  // the observed boxes: the round trip ego -> shared -> ego
  for (int i = lane; i < len; i += 64) {
    const int f = fr[i];
    if (!in_range(f)) continue;
    const Affine s2e = mul(inverse(load_pose(poses + (int64_t)f * 16)), p_first);
    store(q0 + back + i, shared(i), s2e, bx + (int64_t)i * 7, f, a.scores[o0 + i]);
  }
  if (len < 2 || back + fwd == 0) return;
  const int window = min(max(a.velo_window_size, 1), len);
  if (back > 0) {
    double vx, vy;
    velocity_sum(0, window, vx, vy);
    vx /= window, vy /= window;
    const Pose3 first = shared(0);
    const double score0 = a.scores[o0];
    for (int j = lane; j < back; j += 64) {
      const int f = f_first - back + j;
      const double dt = (double)(ts[f] - ts[f_first]) / 1e6;     // negative
      const Pose3 s = {first.x + vx * dt, first.y + vy * dt, first.z, first.yaw};
      const Affine s2e = mul(inverse(load_pose(poses + (int64_t)f * 16)), p_first);
      store(q0 + j, s, s2e, bx, f, score0 * pow(a.score_multiplier, (double)(j + 1)));   // the EARLIEST frame gets m ** 1
    }
  }
  if (fwd > 0) {
    double vx, vy;
    velocity_sum(len - window, window, vx, vy);
    vx /= window, vy /= window;
    const Pose3 last = shared(len - 1);
    const double score1 = a.scores[o0 + len - 1];
    for (int j = lane; j < fwd; j += 64) {
      const int f = f_last + 1 + j;
      const double dt = (double)(ts[f] - ts[f_last + 1]) / 1e6;  // from the first EXTENDED frame: that box does not move
      const Pose3 s = {last.x + vx * dt, last.y + vy * dt, last.z, last.yaw};
      const Affine s2e = mul(inverse(load_pose(poses + (int64_t)f * 16)), p_first);
      store(q0 + back + len + j, s, s2e, bx + (int64_t)(len - 1) * 7, f, score1 * pow(a.score_multiplier, (double)(j + 1)));
    }
  }
}

}  // namespace

extern "C" int ococc_track_extend_f64(const float* boxes, const int32_t* offsets, const int32_t* frames,
                                      const int32_t* segments, const double* scores, int32_t num_tracklets,
                                      int64_t num_boxes, const float* poses, const int64_t* timestamps,
                                      const int32_t* seg_offsets, int32_t num_segments, int64_t num_frames,
                                      const int32_t* num_back, const int32_t* num_fwd, const int32_t* out_offsets,
                                      int64_t num_out, double score_multiplier, int32_t velo_window_size,
                                      float* out_boxes, double* out_scores, int32_t* out_frames,
                                      ococc_stream_t stream) {
  OCOCC_REQUIRE(num_tracklets >= 0 && num_boxes >= 0 && num_segments >= 0 && num_frames >= 0 && num_out >= 0, "negative size");
  OCOCC_REQUIRE(num_out >= num_boxes, "num_out < num_boxes: every input box has an output box");
  OCOCC_REQUIRE(velo_window_size >= 1, "velo_window_size must be at least 1");
  OCOCC_REQUIRE(score_multiplier == score_multiplier, "score_multiplier is not a number");
  if (num_tracklets == 0 || num_boxes == 0) return OCOCC_OK;
  OCOCC_REQUIRE(num_segments > 0 && num_frames > 0, "tracklets without a segment table");
  OCOCC_REQUIRE(boxes && offsets && frames && segments && scores && poses && timestamps && seg_offsets && num_back &&
                    num_fwd && out_offsets && out_boxes && out_scores && out_frames,
                "null pointer");
  Args a;
  a.boxes = boxes, a.offsets = offsets, a.frames = frames, a.segments = segments, a.scores = scores;
  a.poses = poses, a.timestamps = timestamps, a.seg_offsets = seg_offsets;
  a.num_back = num_back, a.num_fwd = num_fwd, a.out_offsets = out_offsets;
  a.out_boxes = out_boxes, a.out_scores = out_scores, a.out_frames = out_frames;
  a.score_multiplier = score_multiplier;
  a.num_tracklets = num_tracklets, a.num_segments = num_segments, a.velo_window_size = velo_window_size;
  a.total_in = num_boxes, a.total_out = num_out, a.total_frames = num_frames;
  hipLaunchKernelGGL(track_extend_kernel, dim3((unsigned)ococc_cdiv(num_tracklets, kWaves)), dim3(64 * kWaves), 0,
                     (hipStream_t)stream, a);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}
