// Ground-truth occupancy export: the occupied label cells of one object, moved into the LiDAR frame of every frame that
// has a GT box and cropped to that frame's proposal box (the save_gt_occ=True branch of
// TrackletRoIHeadOCC.save_occ_from_tracklet, mmdet3d/models/roi_heads/tracklet_roi_head_occ.py:634-702, with
// check_pt_in_box3d of mmdet3d/ops/roiaware_pool3d/src/points_in_boxes_cuda.cu:24-49 as the inside test).
//
// The pair list is frame-major: pair n * K + k is (frame n, cell k), N * K pairs.  Every frame has the same K cells, so
// the tiles need no table: with T = ceil(K / 1024), tile t is cells [j * 1024, min(K, (j + 1) * 1024)) of frame n, where
// n = t / T and j = t % T -- 1024 consecutive pairs of ONE frame, the last tile of a frame short.
//
//   count : one wave per tile, 16 rounds of 64 pairs, lane = pair, one ballot per round; popcounts summed ->
//           tile_counts [N * T] i32 and one 64-bit integer atomic per tile into frame_counts [N].
//   fill  : the same tiles; with scan = exclusive prefix of tile_counts, a kept cell lands where wave_tile_compact
//           (wave_compact.hpp) ranks it: cell order inside a frame and frame order across frames.  The LiDAR-frame
//           point is recomputed, column 3 is value[n] or 1.
//
// Algorithmic bytes: 12 B in per pair in each launch (the K cells are read N times; K * 12 B stays in L2), 4 B out per
// tile, 16 B out per kept pair.  Memory bound and small.  No float atomics; integer counts: the same input gives the
// same bytes.  Vector stores only.  No trigonometric function is evaluated here: the four cos / sin arrays are the
// caller's.
#include "common.hpp"
#include "occ_math.hpp"
#include "wave_compact.hpp"

// every float product and sum below is rounded on its own, as the ATen comparator (bbox.crop_gt_occ_aten) rounds them
#pragma clang fp contract(off)

namespace {

constexpr int kTile = kCompactTile;   // 1024 pairs per wave
constexpr int kWaves = kCompactWaves;
constexpr int kBlock = 64 * kWaves;

struct CropArgs {
  const float* cells;       // [K, 3] gravity centres in the GT box frame
  int64_t K;
  int64_t N;
  const float* gt_boxes;    // rows of gt_stride floats: x, y, z_bottom, w, l, h, yaw
  int64_t gt_stride;
  const float* roi_boxes;   // rows of roi_stride floats, the same columns
  int64_t roi_stride;
  const float* cos_gt;      // [N] cos / sin of the GT yaw
  const float* sin_gt;
  const float* cos_roi;     // [N] cos / sin of float(RoI yaw + pi / 2)
  const float* sin_roi;
  int64_t tiles_per_frame;
  int64_t tiles;            // N * tiles_per_frame
  // count
  int32_t* tile_counts;     // [tiles]
  unsigned long long* frame_counts;   // [N]
  // fill
  const int64_t* scan;      // [tiles] exclusive prefix of tile_counts
  const float* value;       // [N] or null
  float* out;               // [n_out, 4]
  int64_t n_out;
};

struct Pt { float x, y, z; };

template <bool FILL>
__global__ void __launch_bounds__(kBlock) gt_occ_crop_kernel(CropArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);   // wave-uniform from here on
  if (t >= a.tiles) return;
  const int64_t n = t / a.tiles_per_frame;
  const int64_t c0 = (t - n * a.tiles_per_frame) * kTile;
  const int64_t cend = min(a.K, c0 + kTile);

  const float* g = a.gt_boxes + n * a.gt_stride;
  const float* r = a.roi_boxes + n * a.roi_stride;
  const float cg = a.cos_gt[n], sg = a.sin_gt[n], ca = a.cos_roi[n], sa = a.sin_roi[n];
  const float gx = g[0], gy = g[1], gz = g[2], ghh = g[5] / 2.0f;
  const float rx = r[0], ry = r[1];
  const float hw = r[3] / 2.0f, hl = r[4] / 2.0f, hh = r[5] / 2.0f;
  const float cz = r[2] + hh;   // the RoI's gravity centre (cz += h / 2.0 of the .cu: the double sum rounds the same)
  const float val = FILL ? (a.value ? a.value[n] : 1.0f) : 0.f;
  const int64_t base = FILL ? a.scan[t] : 0;

  wave_tile_compact<FILL, Pt>(
      lane, base, a.n_out, a.tile_counts + t, a.frame_counts + n,
      [&](int i, Pt& p) {
        const int64_t cell = c0 + i;
        bool in = false;
        if (cell < cend) {
          const float* q = a.cells + cell * 3;
          p.x = q[0], p.y = q[1], p.z = q[2];
          ococc_box_to_lidar(p.x, p.y, p.z, cg, sg, gx, gy, gz, ghh);
          // check_pt_in_box3d: inclusive on the z faces, strict on the side faces
          const float dz = p.z - cz, dx = p.x - rx, dy = p.y - ry;
          const float xc = dx * ca, ys = dy * (-sa), xs = dx * sa, yc = dy * ca;
          const float lx = xc + ys, ly = xs + yc;
          // (& and not &&: behind a branch on the height test the count pass loads z first and x, y after it)
          in = !(fabsf(dz) > hh) & (lx > -hl) & (lx < hl) & (ly > -hw) & (ly < hw);
        }
        return in;
      },
      [&](int, const Pt& p, int64_t pos) { *reinterpret_cast<f32x4*>(a.out + pos * 4) = f32x4{p.x, p.y, p.z, val}; });
}

// the argument checks both launches share; 1: nothing to launch, 0: go on, < 0: an error
int check_common(const char* fn, int64_t K, int64_t N, int64_t gt_stride, int64_t roi_stride, int64_t tiles) {
  if (K < 0 || N < 0) return ococc_fail(OCOCC_EINVAL, fn, "K < 0 or N < 0");
  if (gt_stride < 7 || roi_stride < 7)
    return ococc_fail(OCOCC_EINVAL, fn, "gt_stride < 7 or roi_stride < 7: columns 0-5 of both boxes are read");
  if (N > INT32_MAX || K >= ((int64_t)1 << 40) || ococc_gt_occ_crop_tiles(N, K) > (int64_t)4 * INT32_MAX)
    return ococc_fail(OCOCC_EINVAL, fn, "N, K or the number of tiles is beyond one launch");
  if (tiles != ococc_gt_occ_crop_tiles(N, K))
    return ococc_fail(OCOCC_EINVAL, fn, "tiles != ococc_gt_occ_crop_tiles(N, K)");
  return N == 0 || K == 0 ? 1 : 0;
}

}  // namespace

extern "C" int64_t ococc_gt_occ_crop_tiles(int64_t N, int64_t K) {
  return N <= 0 || K <= 0 ? 0 : N * ((K + kTile - 1) / kTile);
}

extern "C" int ococc_gt_occ_crop_count(const float* cells, int64_t K, const float* gt_boxes, int64_t gt_stride,
                                       const float* roi_boxes, int64_t roi_stride, int64_t N, const float* cos_gt,
                                       const float* sin_gt, const float* cos_roi, const float* sin_roi,
                                       int32_t* tile_counts, int64_t tiles, int64_t* frame_counts,
                                       ococc_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = check_common(__func__, K, N, gt_stride, roi_stride, tiles);
  if (rc < 0) return rc;
  if (N == 0) return OCOCC_OK;
  OCOCC_REQUIRE(frame_counts, "null pointer");
  OCOCC_HIP(hipMemsetAsync(frame_counts, 0, (size_t)N * sizeof(int64_t), stream));
  if (rc == 1) return OCOCC_OK;
  OCOCC_REQUIRE(cells && gt_boxes && roi_boxes && cos_gt && sin_gt && cos_roi && sin_roi && tile_counts, "null pointer");
  CropArgs a{};
  a.cells = cells, a.K = K, a.N = N, a.gt_boxes = gt_boxes, a.gt_stride = gt_stride, a.roi_boxes = roi_boxes;
  a.roi_stride = roi_stride, a.cos_gt = cos_gt, a.sin_gt = sin_gt, a.cos_roi = cos_roi, a.sin_roi = sin_roi;
  a.tiles_per_frame = tiles / N, a.tiles = tiles, a.tile_counts = tile_counts;
  a.frame_counts = reinterpret_cast<unsigned long long*>(frame_counts);
  hipLaunchKernelGGL(gt_occ_crop_kernel<false>, dim3((unsigned)ococc_cdiv(tiles, kWaves)), dim3(kBlock), 0, stream, a);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}

extern "C" int ococc_gt_occ_crop_fill(const float* cells, int64_t K, const float* gt_boxes, int64_t gt_stride,
                                      const float* roi_boxes, int64_t roi_stride, int64_t N, const float* cos_gt,
                                      const float* sin_gt, const float* cos_roi, const float* sin_roi,
                                      const int64_t* tile_scan, int64_t tiles, const float* value, float* out,
                                      int64_t n_out, ococc_stream_t stream) {
  const int rc = check_common(__func__, K, N, gt_stride, roi_stride, tiles);
  if (rc < 0) return rc;
  OCOCC_REQUIRE(n_out >= 0, "n_out < 0");
  if (rc == 1 || n_out == 0) return OCOCC_OK;
  OCOCC_REQUIRE(cells && gt_boxes && roi_boxes && cos_gt && sin_gt && cos_roi && sin_roi && tile_scan && out,
                "null pointer");
  OCOCC_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "out [n_out, 4] must be 16-byte aligned");
  CropArgs a{};
  a.cells = cells, a.K = K, a.N = N, a.gt_boxes = gt_boxes, a.gt_stride = gt_stride, a.roi_boxes = roi_boxes;
  a.roi_stride = roi_stride, a.cos_gt = cos_gt, a.sin_gt = sin_gt, a.cos_roi = cos_roi, a.sin_roi = sin_roi;
  a.tiles_per_frame = tiles / N, a.tiles = tiles, a.scan = tile_scan, a.value = value, a.out = out, a.n_out = n_out;
  hipLaunchKernelGGL(gt_occ_crop_kernel<true>, dim3((unsigned)ococc_cdiv(tiles, kWaves)), dim3(kBlock), 0,
                     (hipStream_t)stream, a);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}
