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
//            derived from start by a one-wave scan kernel in front.  One wave per tile: 16 rounds of 64 cells, lane =
//            cell, one ballot per round; popcounts summed -> tile_counts [max_tiles] i32 (0 for the unused tail) and one
//            64-bit integer atomic per tile into roi_counts [R].
//   fill   : the same tiles; with scan = exclusive prefix of tile_counts, an occupied cell lands at
//            scan[tile] + (occupied cells of earlier rounds) + popcount(ballot below the lane): (tile, round, lane) IS
//            ascending cell order, so no sort (the idiom of tracklet_crop.hip).  The centre is recomputed from the cell
//            id, optionally turned into the LiDAR frame with OccDecoder._to_lidar's arithmetic (occ_base.py:220-230,
//            330-336), every operation rounded on its own.
//
// Algorithmic bytes: cells 16 B out per cell; count 4 B in per cell, 4 B out per tile; fill 4 B in per cell, 12 or
// 16 B out per occupied cell.  All three are memory bound and small next to the decoder (about 4.8 MFLOP per cell).
// No float atomics; integer counts: the same input gives the same bytes.  Vector stores only.
#include "common.hpp"
#include "occ_math.hpp"
#include "occ_tiles.hpp"   // roi_of, cell_centre, tile_table_kernel: shared with occ_frame.hip

// every float product and sum below is rounded on its own, as the ATen chain rounds them: hipcc's default contracts
// a * b + c into a fused multiply-add (also through __fmul_rn / __fadd_rn, whose bodies sit in front of this pragma)
#pragma clang fp contract(off)

namespace {

constexpr int kRounds = kOccCompactRounds;
constexpr int kTile = kOccCompactTile;   // 1024 cells per wave
constexpr int kWaves = kOccCompactWaves;
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

struct FillArgs {
  const int64_t* scan;      // [max_tiles] exclusive prefix of tile_counts
  const float* sizes;       // [R, 3] enlarged sizes
  const int32_t* dims;      // [R, 3]
  float voxel_size;
  const float* rois;        // to_lidar: rows of roi_stride floats, columns 1-3 the bottom centre, column 6 the height
  int64_t roi_stride;
  const float* cos_yaw;     // [R]
  const float* sin_yaw;     // [R]
  const float* roi_value;   // [R] or null
  int cols;                 // 3 or 4
  float* out;               // [n_out, cols]
  int64_t n_out;
};

template <bool FILL>
__global__ void __launch_bounds__(kBlock)
occ_select_kernel(const float* __restrict__ logits, int64_t n, const int64_t* __restrict__ start,
                  const int64_t* __restrict__ tile_start, int R, int64_t max_tiles, float pos_thresh,
                  int32_t* __restrict__ tile_counts, unsigned long long* __restrict__ roi_counts, FillArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);   // wave-uniform from here on
  if (t >= max_tiles) return;
  if (t >= tile_start[R]) {
    if (!FILL && lane == 0) tile_counts[t] = 0;
    return;
  }
  const int r = roi_of(tile_start, R, t);
  const int64_t r0 = start[r];
  const int64_t c0 = r0 + (t - tile_start[r]) * kTile;
  const int64_t cend = c0 < 0 ? c0 : min(min(start[r + 1], c0 + kTile), n);   // (c0 < 0, a start that is no prefix: no cell)

  float cy = 0.f, sy = 0.f, bx = 0.f, by = 0.f, bz = 0.f, hh = 0.f, val = 0.f;
  int64_t base = 0;
  if (FILL) {
    base = a.scan[t];
    if (a.rois) {
      const float* b = a.rois + r * a.roi_stride;
      cy = a.cos_yaw[r], sy = a.sin_yaw[r];
      bx = b[1], by = b[2], bz = b[3], hh = b[6] / 2.0f;
    }
    if (a.roi_value) val = a.roi_value[r];
  }
  int cnt = 0;
#pragma unroll 4
  for (int k = 0; k < kRounds; ++k) {
    const int64_t cell = c0 + k * 64 + lane;
    float lg = 0.f;
    bool occ = false;
    if (cell < cend) {
      lg = logits[cell];
      occ = ococc_occupied(lg, pos_thresh);
    }
    const unsigned long long bal = __ballot(occ);
    if (FILL && occ) {
      const int64_t pos = base + cnt + __popcll(bal & ((1ull << lane) - 1ull));
      if (pos < a.n_out) {   // (counts, scan and fill of the same logits: always)
        Cell c = cell_centre((uint32_t)(cell - r0), a.sizes + r * 3, a.dims + r * 3, a.voxel_size);
        if (a.rois) {
          // OccDecoder._to_lidar: x c + y s, -x s + y c, z; + centre; z + h / 2
          ococc_box_to_lidar(c.x, c.y, c.z, cy, sy, bx, by, bz, hh);
        }
        float* o = a.out + pos * a.cols;
        if (a.cols == 4) {
          *reinterpret_cast<f32x4*>(o) = f32x4{c.x, c.y, c.z, a.roi_value ? val : ococc_sigmoid_aten(lg)};
        } else {
          o[0] = c.x, o[1] = c.y, o[2] = c.z;
        }
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
  hipLaunchKernelGGL(occ_select_kernel<false>, dim3((unsigned)ococc_cdiv(max_tiles, kWaves)), dim3(kBlock), 0, stream,
                     logits, n, start, tile_start, R, max_tiles, pos_thresh, tile_counts,
                     reinterpret_cast<unsigned long long*>(roi_counts), FillArgs{});
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
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
  const FillArgs a{tile_scan, sizes, dims, voxel_size, to_lidar ? rois : nullptr, roi_stride, cos_yaw, sin_yaw,
                   roi_value, cols, out, n_out};
  hipLaunchKernelGGL(occ_select_kernel<true>, dim3((unsigned)ococc_cdiv(max_tiles, kWaves)), dim3(kBlock), 0,
                     (hipStream_t)stream, logits, n, start, tile_start, R, max_tiles, pos_thresh, (int32_t*)nullptr,
                     (unsigned long long*)nullptr, a);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}
