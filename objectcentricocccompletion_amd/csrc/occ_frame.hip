// Completed occupancy of ONE online step: what the decoder predicts occupied, joined with what the sensor hit in this
// frame, compacted in cell order into rows (x, y, z, probability) plus a flag byte per row.  Stands behind
// occ_ops.occ_frame_select / OccDecoder.get_frame_occ and the ``occ=True`` results of TrackletRoIHeadOCC.simple_test_step,
// simple_test_steps and simple_test_scene_step; replaces, for the step, OccAutoEncoder.sample_observation's
// rasterisation (mmdet3d/models/roi_heads/bbox_heads/occ_ae_head.py:65-126, about 25 ATen launches with int64 index
// tensors) and the select / transform of OccDecoder.get_occ (mmdet3d/models/occ/occ_base.py:238-342).
//
// The flat cell list, the tiles of 1024 cells of one RoI and the ballot / popcount compaction are those of
// occ_export.hip (occ_tiles.hpp, occ_math.hpp).
//
//   mark   : one thread per pooled point (box-frame xyz, RoI index).  Cell index per axis with the f32 arithmetic of
//            occ_ops.quantize_points, floor((p - (-size / 2)) / voxel), a true division; an index < 0 or >= dim on any
//            axis marks nothing (the points were pooled from an enlarged box).  observed[cell] = 1: a byte store, all
//            points of a cell store the same value, so no atomic.  observed is zeroed in front (one memset).
//   count  : one wave per tile, 16 rounds of 64 cells; selected = (ococc_occupied(logit) or observed[cell]) and
//            row_keep[RoI] != 0 (row_keep null: every RoI kept).  tile_counts [max_tiles] i32 and one 64-bit integer
//            atomic per tile into roi_counts [R].
//   fill   : the same tiles; a selected cell lands at scan[tile] + earlier rounds + popcount(ballot below the lane).
//            Row = centre through ococc_box_to_lidar with the RoI's pose, then optionally through the RoI's 3x4 matrix
//            T: x' = ((t0 x + t1 y) + t2 z) + t3, every operation rounded once; column 3 ococc_sigmoid_aten(logit).
//            One 16-byte store per row and one byte of flags: bit 0 predicted, bit 1 observed.
//
// Algorithmic bytes: mark 16 B in, 1 B out per point; count 5 B in per cell; fill 5 B in per cell, 17 B out per
// selected cell.  Memory bound and small next to the decoder (about 4.8 MFLOP per cell).  No float atomics, integer
// counts: the same input gives the same bytes.  Vector stores only.
#include "common.hpp"
#include "occ_math.hpp"
#include "occ_tiles.hpp"

// every float product, quotient and sum below is rounded on its own, as the ATen chain rounds them
#pragma clang fp contract(off)

namespace {

constexpr int kRounds = kOccCompactRounds;
constexpr int kTile = kOccCompactTile;   // 1024 cells per wave
constexpr int kWaves = kOccCompactWaves;
constexpr int kBlock = 64 * kWaves;
constexpr int kMarkBlock = 256;

__global__ void __launch_bounds__(kMarkBlock)
occ_frame_mark_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ pts_roi, int64_t M,
                      const float* __restrict__ sizes, const int32_t* __restrict__ dims,
                      const int64_t* __restrict__ start, int R, float voxel_size, uint8_t* __restrict__ observed,
                      int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kMarkBlock + threadIdx.x; i < M; i += (int64_t)gridDim.x * kMarkBlock) {
    const int r = pts_roi[i];
    if (r < 0 || r >= R) continue;
    const float* s = sizes + r * 3;
    const int32_t* d = dims + r * 3;
    int idx[3];
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float lo = -s[a] / 2.0f;                                        // min_bound of quantize_points
      const float q = floorf(__fdiv_rn(xyz[i * 3 + a] - lo, voxel_size));   // NaN: no comparison holds
      const bool ok = q >= 0.0f && q < (float)d[a];
      inside = inside && ok;
      idx[a] = ok ? (int)q : 0;
    }
    if (!inside) continue;
    const int64_t cell = start[r] + ((int64_t)idx[0] * d[1] + idx[1]) * d[2] + idx[2];
    if (cell < 0 || cell >= start[r + 1] || cell >= n) continue;   // (a start that is no prefix of dims: no cell)
    observed[cell] = 1;
  }
}

struct FrameFill {
  const int64_t* scan;      // [max_tiles] exclusive prefix of tile_counts
  const float* sizes;       // [R, 3] enlarged sizes
  const int32_t* dims;      // [R, 3]
  float voxel_size;
  const float* rois;        // rows of roi_stride floats, columns 1-3 the bottom centre, column 6 the height
  int64_t roi_stride;
  const float* cos_yaw;     // [R]
  const float* sin_yaw;     // [R]
  const float* transforms;  // [R, 12] row-major 3x4, or null
  float* out;               // [n_out, 4]
  uint8_t* flags;           // [n_out]
  int64_t n_out;
};

template <bool FILL>
__global__ void __launch_bounds__(kBlock)
occ_frame_select_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ observed,
                        const uint8_t* __restrict__ row_keep, int64_t n, const int64_t* __restrict__ start,
                        const int64_t* __restrict__ tile_start, int R, int64_t max_tiles, float pos_thresh,
                        int32_t* __restrict__ tile_counts, unsigned long long* __restrict__ roi_counts, FrameFill a) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);   // wave-uniform from here on
  if (t >= max_tiles) return;
  if (t >= tile_start[R]) {
    if (!FILL && lane == 0) tile_counts[t] = 0;
    return;
  }
  const int r = roi_of(tile_start, R, t);
  if (row_keep && row_keep[r] == 0) {   // test_cfg.filter_empty_roi: the RoI emits nothing
    if (!FILL && lane == 0) tile_counts[t] = 0;
    return;
  }
  const int64_t r0 = start[r];
  const int64_t c0 = r0 + (t - tile_start[r]) * kTile;
  const int64_t cend = c0 < 0 ? c0 : min(min(start[r + 1], c0 + kTile), n);   // (c0 < 0, a start that is no prefix: no cell)

  float cy = 0.f, sy = 0.f, bx = 0.f, by = 0.f, bz = 0.f, hh = 0.f;
  float m[12] = {0.f};
  int64_t base = 0;
  if (FILL) {
    base = a.scan[t];
    const float* b = a.rois + r * a.roi_stride;
    cy = a.cos_yaw[r], sy = a.sin_yaw[r];
    bx = b[1], by = b[2], bz = b[3], hh = b[6] / 2.0f;
    if (a.transforms) {
#pragma unroll
      for (int j = 0; j < 12; ++j) m[j] = a.transforms[(int64_t)r * 12 + j];
    }
  }
  int cnt = 0;
#pragma unroll 4
  for (int k = 0; k < kRounds; ++k) {
    const int64_t cell = c0 + k * 64 + lane;
    float lg = 0.f;
    bool pred = false, seen = false;
    if (cell < cend) {
      lg = logits[cell];
      pred = ococc_occupied(lg, pos_thresh);
      seen = observed && observed[cell] != 0;
    }
    const bool sel = pred || seen;
    const unsigned long long bal = __ballot(sel);
    if (FILL && sel) {
      const int64_t pos = base + cnt + __popcll(bal & ((1ull << lane) - 1ull));
      if (pos < a.n_out) {   // (counts, scan and fill of the same inputs: always)
        Cell c = cell_centre((uint32_t)(cell - r0), a.sizes + r * 3, a.dims + r * 3, a.voxel_size);
        ococc_box_to_lidar(c.x, c.y, c.z, cy, sy, bx, by, bz, hh);
        if (a.transforms) {
          const float x = c.x, y = c.y, z = c.z;
          c.x = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
          c.y = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
          c.z = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
        }
        *reinterpret_cast<f32x4*>(a.out + pos * 4) = f32x4{c.x, c.y, c.z, ococc_sigmoid_aten(lg)};
        a.flags[pos] = (uint8_t)((pred ? 1 : 0) | (seen ? 2 : 0));
      }
    }
    cnt += __popcll(bal);
  }
  if (!FILL && lane == 0) {
    tile_counts[t] = cnt;
    if (cnt) atomicAdd(roi_counts + r, (unsigned long long)cnt);
  }
}

}  // namespace

extern "C" int ococc_occ_frame_mark(const float* local_xyz, const int32_t* pts_roi, int64_t M, const float* sizes,
                                    const int32_t* dims, const int64_t* start, int32_t R, float voxel_size,
                                    uint8_t* observed, int64_t n, ococc_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OCOCC_REQUIRE(M >= 0 && R >= 0 && n >= 0, "M < 0, R < 0 or n < 0");
  OCOCC_REQUIRE(voxel_size > 0.f, "voxel_size <= 0");
  if (n == 0) return OCOCC_OK;
  OCOCC_REQUIRE(observed, "null pointer: observed");
  OCOCC_HIP(hipMemsetAsync(observed, 0, (size_t)n, stream));
  if (M == 0 || R == 0) return OCOCC_OK;
  OCOCC_REQUIRE(local_xyz && pts_roi && sizes && dims && start, "null pointer");
  hipLaunchKernelGGL(occ_frame_mark_kernel, dim3(ococc_grid_1d(M, kMarkBlock, 2048)), dim3(kMarkBlock), 0, stream,
                     local_xyz, pts_roi, M, sizes, dims, start, R, voxel_size, observed, n);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}

extern "C" int ococc_occ_frame_count(const float* logits, const uint8_t* observed, const uint8_t* row_keep, int64_t n,
                                     const int64_t* start, int32_t R, float pos_thresh, int64_t* tile_start,
                                     int32_t* tile_counts, int64_t max_tiles, int64_t* roi_counts,
                                     ococc_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OCOCC_REQUIRE(n >= 0 && R >= 0, "n < 0 or R < 0");
  OCOCC_REQUIRE(max_tiles >= ococc_occ_select_max_tiles(n, R), "max_tiles < ococc_occ_select_max_tiles(n, R)");
  if (R == 0) return OCOCC_OK;
  OCOCC_REQUIRE(start && tile_start && roi_counts, "null pointer");
  OCOCC_HIP(hipMemsetAsync(roi_counts, 0, (size_t)R * sizeof(int64_t), stream));
  hipLaunchKernelGGL(tile_table_kernel, dim3(1), dim3(64), 0, stream, start, R, tile_start);
  OCOCC_CHECK_LAUNCH();
  if (max_tiles == 0) return OCOCC_OK;
  OCOCC_REQUIRE(tile_counts && (logits || n == 0), "null pointer");
  hipLaunchKernelGGL(occ_frame_select_kernel<false>, dim3((unsigned)ococc_cdiv(max_tiles, kWaves)), dim3(kBlock), 0,
                     stream, logits, observed, row_keep, n, start, tile_start, R, max_tiles, pos_thresh, tile_counts,
                     reinterpret_cast<unsigned long long*>(roi_counts), FrameFill{});
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}

extern "C" int ococc_occ_frame_fill(const float* logits, const uint8_t* observed, const uint8_t* row_keep, int64_t n,
                                    const int64_t* start, const int64_t* tile_start, int32_t R, float pos_thresh,
                                    const int64_t* tile_scan, int64_t max_tiles, const float* sizes, const int32_t* dims,
                                    float voxel_size, const float* rois, int64_t roi_stride, const float* cos_yaw,
                                    const float* sin_yaw, const float* transforms, float* out, uint8_t* flags,
                                    int64_t n_out, ococc_stream_t stream) {
  OCOCC_REQUIRE(n >= 0 && R >= 0 && n_out >= 0, "n < 0, R < 0 or n_out < 0");
  OCOCC_REQUIRE(voxel_size > 0.f, "voxel_size <= 0");
  OCOCC_REQUIRE(max_tiles >= ococc_occ_select_max_tiles(n, R), "max_tiles < ococc_occ_select_max_tiles(n, R)");
  OCOCC_REQUIRE(R == 0 || roi_stride >= 7, "roi_stride < 7: columns 1-3 (centre) and 6 (height) are read");
  if (R == 0 || n == 0 || n_out == 0 || max_tiles == 0) return OCOCC_OK;
  OCOCC_REQUIRE(rois && cos_yaw && sin_yaw, "null pointer: rois, cos_yaw and sin_yaw give the pose of every RoI");
  OCOCC_REQUIRE(logits && start && tile_start && tile_scan && sizes && dims && out && flags, "null pointer");
  OCOCC_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "out [n, 4] must be 16-byte aligned");
  const FrameFill a{tile_scan, sizes, dims, voxel_size, rois, roi_stride, cos_yaw, sin_yaw, transforms, out, flags, n_out};
  hipLaunchKernelGGL(occ_frame_select_kernel<true>, dim3((unsigned)ococc_cdiv(max_tiles, kWaves)), dim3(kBlock), 0,
                     (hipStream_t)stream, logits, observed, row_keep, n, start, tile_start, R, max_tiles, pos_thresh,
                     (int32_t*)nullptr, (unsigned long long*)nullptr, a);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}
