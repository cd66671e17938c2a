// The box crop that tracklet_crop.hip (offline CTRL crop) and scene_rows.hip (online step rows) share, each piece defined
// once so that both paths see the same points: the work split, the boxes staged in LDS, the wave tile of points in
// registers, and the membership test.
//
// Membership is check_pt_in_box3d (mmdet3d/ops/roiaware_pool3d/src/points_in_boxes_cuda.cu:24-49), each box on its own:
//   |z - (z_bottom + h/2)| <= h/2;  (dx, dy) turned by yaw + pi/2;  -l/2 < local_x < l/2,  -w/2 < local_y < w/2.
// A NaN x or y is in no box; a NaN z passes the height test (!(|dz| > h/2)).
// (Not gt_occ_crop.hip's inside test: that one is compiled with contraction off and ordered as its ATen comparator.)
#pragma once
#include "common.hpp"
#include "wave_compact.hpp"

constexpr int kCropRounds = kCompactRounds;     // points per lane
constexpr int kCropWaveTile = kCompactTile;     // 1024 consecutive points per wave, every point read once per pass
constexpr int kCropWaves = kCompactWaves;
constexpr int kCropBlockTile = kCropWaveTile * kCropWaves;   // (ctrl_prep._CROP_BLOCK_TILE mirrors it)
constexpr int kCropChunk = 64;                  // boxes staged at a time: one per lane

struct StagedBox {
  float cx, cy, cz, hl, hw, hh, ca, sa, r2;   // gravity centre, half sizes, cos / sin of yaw + pi/2, a BEV radius^2

  __device__ __forceinline__ bool holds(float x, float y, float z) const {
    const float dx = x - cx, dy = y - cy;
    bool in = !(fabsf(z - cz) > hh) && !(dx * dx + dy * dy > r2);   // the radius: a cheap conservative reject
    if (in) {
      const float lx = dx * ca + dy * (-sa), ly = dx * sa + dy * ca;
      in = (lx > -hl) & (lx < hl) & (ly > -hw) & (ly < hw);
    }
    return in;
  }
};

// kCropChunk staged boxes in LDS, read as broadcasts
struct BoxChunk {
  float f[9][kCropChunk];

  // slot <- the box b: x, y, z_bottom, w, l, h, yaw
  __device__ __forceinline__ void stage(int slot, const float* b) {
    const float hh = b[5] * 0.5f, hl = b[4] * 0.5f, hw = b[3] * 0.5f;
    const float rot = (float)((double)b[6] + 1.5707963267948966);
    f[0][slot] = b[0], f[1][slot] = b[1], f[2][slot] = b[2] + hh;
    f[3][slot] = hl, f[4][slot] = hw, f[5][slot] = hh;
    f[6][slot] = cosf(rot), f[7][slot] = sinf(rot);
    f[8][slot] = (hl * hl + hw * hw) * 1.001f + 1e-6f;   // |local|^2 < hl^2 + hw^2 inside; the slack covers rounding
  }
  __device__ __forceinline__ StagedBox get(int j) const {
    return {f[0][j], f[1][j], f[2][j], f[3][j], f[4][j], f[5][j], f[6][j], f[7][j], f[8][j]};
  }
};

// A wave tile of points in registers: round r, lane l holds point w0 + r * 64 + l
struct WavePoints {
  float x[kCropRounds], y[kCropRounds], z[kCropRounds];

  // points: row 0 of the cloud (rows of C floats, xyz first), n its rows
  __device__ __forceinline__ void load(const float* __restrict__ points, int C, int64_t n, int64_t w0, int lane) {
#pragma unroll
    for (int r = 0; r < kCropRounds; ++r) {
      const int64_t i = w0 + r * 64 + lane;
      if (i < n) {
        const float* q = points + i * C;
        x[r] = q[0], y[r] = q[1], z[r] = q[2];
      } else {
        x[r] = 0.f, y[r] = 0.f, z[r] = INFINITY;   // fails the height test of every box
      }
    }
  }
};
