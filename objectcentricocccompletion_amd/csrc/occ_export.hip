// Completed-occupancy export: the dense-grid decode around the decoder MLP, and the order-preserving compaction of its
// occupied cells into the array the per-frame files are cut from (TrackletRoIHeadOCC.save_occ_from_tracklet,
// mmdet3d/models/roi_heads/tracklet_roi_head_occ.py:612-745, through OccDecoder.get_occ, mmdet3d/models/occ/occ_base.py:238-342).
//
// The cells of all RoIs are ONE flat list, RoI after RoI, x slowest and z fastest inside an RoI; start [R + 1] i64 is
// the exclusive prefix of the cells per RoI (start[0] = 0, start[R] = number of cells).
//
//   cells  : flat cell id -> (centre f32 [3], RoI i32).  One thread per cell, the RoI by binary search over start (in
//            LDS while R + 1 <= 2048 entries = 16 KiB, else in global memory: the table is a few KiB and stays in L2).
//            Replaces generate_dense_voxel_centers (mmdet3d/ops/occ/occ_ops.py:5-50) as
//            occ_ops.dense_voxel_centers_batched states it: no int64 box tensor, no repeat_interleave.
//   count  : the list is cut into tiles of 1024 consecutive cells of ONE RoI (the last tile of an RoI is short; a tile
//            never straddles two RoIs).  tile_start [R + 1] i64, the exclusive prefix of ceil(cells / 1024) per RoI, is
//            derived from start by a one-wave scan kernel in front.  One wave per tile (wave_compact.hpp) ->
//            tile_counts [max_tiles] i32 (0 for the unused tail), one 64-bit integer atomic per tile into roi_counts [R].
//   fill   : the same tiles; with scan = exclusive prefix of tile_counts, an occupied cell lands where
//            wave_tile_compact (wave_compact.hpp) ranks it: ascending cell order, no sort.  The centre is recomputed from
//            the cell id, optionally turned into the LiDAR frame with OccDecoder._to_lidar's arithmetic
//            (occ_base.py:220-230, 330-336), every operation rounded on its own.
// count and fill are ONE kernel with the completed occupancy of an online step (occ_frame.hip), which adds the observed
// cells, row_keep, a 3x4 matrix after the pose and a flag byte per row; occ_frame.hip reaches it through
// occ_select_count / occ_select_fill (occ_tiles.hpp).
//
// Algorithmic bytes: cells 16 B out per cell; count 4 B in per cell, 4 B out per tile; fill 4 B in per cell, 12 or
// 16 B out per occupied cell.  All three are memory bound and small next to the decoder (about 4.8 MFLOP per cell).
// No float atomics; integer counts: the same input gives the same bytes.  Vector stores only.
#include "common.hpp"
#include "occ_math.hpp"
#include "occ_tiles.hpp"

// every float product and sum below is rounded on its own, as the ATen chain rounds them: hipcc's default contracts
// a * b + c into a fused multiply-add (also through __fmul_rn / __fadd_rn, whose bodies sit in front of this pragma)
#pragma clang fp contract(off)

namespace {

constexpr int kTile = kCompactTile;   // 1024 cells per wave
constexpr int kWaves = kCompactWaves;
constexpr int kBlock = 64 * kWaves;
constexpr int kLdsStart = 2048;       // entries of start kept in LDS by the cells kernel

template <bool LDS>
__global__ void __launch_bounds__(kBlock)
dense_grid_cells_kernel(const float* __restrict__ sizes, const int32_t* __restrict__ dims,
                        const int64_t* __restrict__ start, int R, float voxel_size, int64_t lo, int64_t hi,
                        float* __restrict__ centers, int32_t* __restrict__ roi_index) {
  __shared__ int64_t s_start[LDS ? kLdsStart : 1];
  if (LDS) {
    for (int i = threadIdx.x; i <= R; i += kBlock) s_start[i] = start[i];
    __syncthreads();
  }
  const int64_t* st = LDS ? s_start : start;
  for (int64_t i = lo + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < hi; i += (int64_t)gridDim.x * kBlock) {
    const int r = roi_of(st, R, i);
    const Cell c = cell_centre((uint32_t)(i - st[r]), sizes + r * 3, dims + r * 3, voxel_size);
    float* o = centers + (i - lo) * 3;
    o[0] = c.x, o[1] = c.y, o[2] = c.z;
    roi_index[i - lo] = r;
  }
}

// tile_start [R + 1]: exclusive prefix of ceil((start[r + 1] - start[r]) / 1024).  One wave, 64 RoIs per step.
__global__ void __launch_bounds__(64)
tile_table_kernel(const int64_t* __restrict__ start, int R, int64_t* __restrict__ tile_start) {
  const int lane = threadIdx.x;
  int64_t carry = 0;
  if (lane == 0) tile_start[0] = 0;
  for (int base = 0; base < R; base += 64) {
    const int r = base + lane;
    int64_t v = 0;
    if (r < R) {
      const int64_t k = start[r + 1] - start[r];
      v = k > 0 ? (k + kTile - 1) / kTile : 0;
    }
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t u = __shfl_up(v, d, 64);
      if (lane >= d) v += u;
    }
    if (r < R) tile_start[r + 1] = carry + v;
    carry += __shfl(v, 63, 64);
  }
}

struct Picked { float logit; bool pred, seen; };

// FRAME: observed, row_keep, transforms and flags are looked at (the export passes none of them, and without the 3x4
// matrix in registers its fill keeps 8 waves per SIMD)
template <bool FILL, bool FRAME>
__global__ void __launch_bounds__(kBlock)
occ_select_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ observed,
                  const uint8_t* __restrict__ row_keep, int64_t n, const int64_t* __restrict__ start,
                  const int64_t* __restrict__ tile_start, int R, int64_t max_tiles, float pos_thresh,
                  int32_t* __restrict__ tile_counts, unsigned long long* __restrict__ roi_counts, OccFillArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);   // wave-uniform from here on
  if (t >= max_tiles) return;
  if (t >= tile_start[R]) {
    if (!FILL && lane == 0) tile_counts[t] = 0;
    return;
  }
  const int r = roi_of(tile_start, R, t);
  if (FRAME && row_keep && row_keep[r] == 0) {   // test_cfg.filter_empty_roi: the RoI emits nothing
    if (!FILL && lane == 0) tile_counts[t] = 0;
    return;
  }
  const int64_t r0 = start[r];
  const int64_t c0 = r0 + (t - tile_start[r]) * kTile;
  const int64_t cend = c0 < 0 ? c0 : min(min(start[r + 1], c0 + kTile), n);   // (c0 < 0, a start that is no prefix: no cell)

  float cy = 0.f, sy = 0.f, bx = 0.f, by = 0.f, bz = 0.f, hh = 0.f, val = 0.f;
  float m[12] = {0.f};
  int64_t base = 0;
  if (FILL) {
    base = a.scan[t];
    if (a.rois) {
      const float* b = a.rois + r * a.roi_stride;
      cy = a.cos_yaw[r], sy = a.sin_yaw[r];
      bx = b[1], by = b[2], bz = b[3], hh = b[6] / 2.0f;
    }
    if (a.roi_value) val = a.roi_value[r];
    if (FRAME && a.transforms) {
#pragma unroll
      for (int j = 0; j < 12; ++j) m[j] = a.transforms[(int64_t)r * 12 + j];
    }
  }
  wave_tile_compact<FILL, Picked>(
      lane, base, a.n_out, tile_counts + t, roi_counts + r,
      [&](int i, Picked& v) {
        const int64_t cell = c0 + i;
        if (cell < cend) {
          v.logit = logits[cell];
          v.seen = FRAME && observed && observed[cell] != 0;   // (both loads in front of the sigmoid)
          v.pred = ococc_occupied(v.logit, pos_thresh);
        }
        return v.pred || v.seen;
      },
      [&](int i, const Picked& v, int64_t pos) {
        Cell c = cell_centre((uint32_t)(c0 + i - r0), a.sizes + r * 3, a.dims + r * 3, a.voxel_size);
        if (a.rois) {
          // OccDecoder._to_lidar: x c + y s, -x s + y c, z; + centre; z + h / 2
          ococc_box_to_lidar(c.x, c.y, c.z, cy, sy, bx, by, bz, hh);
        }
        if (FRAME && a.transforms) {   // x' = ((t0 x + t1 y) + t2 z) + t3, every operation rounded once
          const float x = c.x, y = c.y, z = c.z;
          c.x = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
          c.y = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
          c.z = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
        }
        float* o = a.out + pos * a.cols;
        if (a.cols == 4) {
          *reinterpret_cast<f32x4*>(o) = f32x4{c.x, c.y, c.z, a.roi_value ? val : ococc_sigmoid_aten(v.logit)};
        } else {
          o[0] = c.x, o[1] = c.y, o[2] = c.z;
        }
        if (FRAME && a.flags) a.flags[pos] = (uint8_t)((v.pred ? 1 : 0) | (v.seen ? 2 : 0));
      });
}

// OCOCC_REQUIRE and OCOCC_HIP with the export's name `fn` in front of the message
#define SELECT_REQUIRE(cond, msg) do { if (!(cond)) return ococc_fail(OCOCC_EINVAL, fn, msg); } while (0)
#define SELECT_HIP(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return ococc_fail(OCOCC_EHIP, fn, hipGetErrorString(e__)); } while (0)

}  // namespace

int occ_select_count(const char* fn, const float* logits, const uint8_t* observed, const uint8_t* row_keep, int64_t n,
                     const int64_t* start, int32_t R, float pos_thresh, int64_t* tile_start, int32_t* tile_counts,
                     int64_t max_tiles, int64_t* roi_counts, hipStream_t stream) {
  SELECT_REQUIRE(n >= 0 && R >= 0, "n < 0 or R < 0");
  SELECT_REQUIRE(max_tiles >= ococc_occ_select_max_tiles(n, R), "max_tiles < ococc_occ_select_max_tiles(n, R)");
  if (R == 0) return OCOCC_OK;
  SELECT_REQUIRE(start && tile_start && roi_counts, "null pointer");
  SELECT_HIP(hipMemsetAsync(roi_counts, 0, (size_t)R * sizeof(int64_t), stream));
  hipLaunchKernelGGL(tile_table_kernel, dim3(1), dim3(64), 0, stream, start, R, tile_start);
  SELECT_HIP(hipGetLastError());
  if (max_tiles == 0) return OCOCC_OK;
  SELECT_REQUIRE(tile_counts && (logits || n == 0), "null pointer");
  const auto kernel = (observed || row_keep) ? occ_select_kernel<false, true> : occ_select_kernel<false, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)ococc_cdiv(max_tiles, kWaves)), dim3(kBlock), 0, stream, logits, observed,
                     row_keep, n, start, (const int64_t*)tile_start, R, max_tiles, pos_thresh, tile_counts,
                     reinterpret_cast<unsigned long long*>(roi_counts), OccFillArgs{});
  SELECT_HIP(hipGetLastError());
  return OCOCC_OK;
}

int occ_select_fill(const char* fn, const float* logits, const uint8_t* observed, const uint8_t* row_keep, int64_t n,
                    const int64_t* start, const int64_t* tile_start, int32_t R, float pos_thresh, int64_t max_tiles,
                    const OccFillArgs& a, hipStream_t stream) {
  const auto kernel = (observed || row_keep || a.transforms || a.flags) ? occ_select_kernel<true, true>
                                                                        : occ_select_kernel<true, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)ococc_cdiv(max_tiles, kWaves)), dim3(kBlock), 0, stream, logits, observed,
                     row_keep, n, start, tile_start, R, max_tiles, pos_thresh, (int32_t*)nullptr,
                     (unsigned long long*)nullptr, a);
  SELECT_HIP(hipGetLastError());
  return OCOCC_OK;
}

extern "C" int ococc_dense_grid_cells_f32(const float* sizes, const int32_t* dims, const int64_t* start, int32_t R,
                                          float voxel_size, int64_t lo, int64_t hi, float* centers,
                                          int32_t* roi_index, ococc_stream_t stream) {
  OCOCC_REQUIRE(R >= 0, "R < 0");
  OCOCC_REQUIRE(lo >= 0 && hi >= lo, "cell range [lo, hi) with lo < 0 or hi < lo");
  OCOCC_REQUIRE(voxel_size > 0.f, "voxel_size <= 0");
  if (R == 0 || hi == lo) return OCOCC_OK;
  OCOCC_REQUIRE(sizes && dims && start && centers && roi_index, "null pointer");
  const int grid = ococc_grid_1d(hi - lo, kBlock * 4, 2048);   // >= 4 cells per thread: the table is staged per block
  if (R + 1 <= kLdsStart)
    hipLaunchKernelGGL(dense_grid_cells_kernel<true>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, sizes, dims,
                       start, R, voxel_size, lo, hi, centers, roi_index);
  else
    hipLaunchKernelGGL(dense_grid_cells_kernel<false>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, sizes, dims,
                       start, R, voxel_size, lo, hi, centers, roi_index);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}

extern "C" int64_t ococc_occ_select_max_tiles(int64_t n, int32_t R) {
  return n < 0 || R < 0 ? 0 : n / kTile + R;
}

extern "C" int ococc_occ_select_count(const float* logits, int64_t n, const int64_t* start, int32_t R, float pos_thresh,
                                      int64_t* tile_start, int32_t* tile_counts, int64_t max_tiles, int64_t* roi_counts,
                                      ococc_stream_t stream) {
  return occ_select_count(__func__, logits, nullptr, nullptr, n, start, R, pos_thresh, tile_start, tile_counts, max_tiles,
                          roi_counts, (hipStream_t)stream);
}

extern "C" int ococc_occ_select_fill(const float* logits, int64_t n, const int64_t* start, const int64_t* tile_start,
                                     int32_t R, float pos_thresh, const int64_t* tile_scan, int64_t max_tiles,
                                     const float* sizes, const int32_t* dims, float voxel_size, int32_t to_lidar,
                                     const float* rois, int64_t roi_stride, const float* cos_yaw, const float* sin_yaw,
                                     const float* roi_value, int32_t cols, float* out, int64_t n_out,
                                     ococc_stream_t stream) {
  OCOCC_REQUIRE(n >= 0 && R >= 0 && n_out >= 0, "n < 0, R < 0 or n_out < 0");
  OCOCC_REQUIRE(cols == 3 || cols == 4, "cols is 3 (xyz) or 4 (xyz, score)");
  OCOCC_REQUIRE(!roi_value || cols == 4, "roi_value needs cols == 4");
  OCOCC_REQUIRE(voxel_size > 0.f, "voxel_size <= 0");
  OCOCC_REQUIRE(max_tiles >= ococc_occ_select_max_tiles(n, R), "max_tiles < ococc_occ_select_max_tiles(n, R)");
  if (to_lidar) {
    OCOCC_REQUIRE(rois && cos_yaw && sin_yaw, "to_lidar needs rois, cos_yaw and sin_yaw");
    OCOCC_REQUIRE(roi_stride >= 7, "roi_stride < 7: columns 1-3 (centre) and 6 (height) are read");
  }
  if (R == 0 || n == 0 || n_out == 0 || max_tiles == 0) return OCOCC_OK;
  OCOCC_REQUIRE(logits && start && tile_start && tile_scan && sizes && dims && out, "null pointer");
  OCOCC_REQUIRE(cols != 4 || (reinterpret_cast<uintptr_t>(out) & 15) == 0, "out [n, 4] must be 16-byte aligned");
  const OccFillArgs a{tile_scan, sizes, dims, voxel_size, to_lidar ? rois : nullptr, roi_stride, cos_yaw, sin_yaw, nullptr,
                      roi_value, cols, out, nullptr, n_out};
  return occ_select_fill(__func__, logits, nullptr, nullptr, n, start, tile_start, R, pos_thresh, max_tiles, a,
                         (hipStream_t)stream);
}
