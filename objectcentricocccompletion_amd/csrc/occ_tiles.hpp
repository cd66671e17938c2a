// What the kernels over the flat cell list share (occ_export.hip, occ_frame.hip): the RoI search over a prefix table, the
// centre of a cell from its id, and the host side of the one select kernel (occ_export.hip) that compacts the list.
// The list: RoI after RoI, x slowest and z fastest inside an RoI; start [R + 1] i64 the exclusive prefix of the cells
// per RoI; tiles of kCompactTile consecutive cells of ONE RoI (wave_compact.hpp).
#pragma once
#include "common.hpp"
#include "occ_math.hpp"
#include "wave_compact.hpp"

// the largest r in [0, R) with table[r] <= i, for an ascending table [R + 1] with table[0] <= i: the RoI of cell i (of
// tile i); RoIs without cells (equal neighbours) are stepped over.  Reads entries 1 .. R - 1 only.
__device__ __forceinline__ int roi_of(const int64_t* table, int R, int64_t i) {
  int lo = 0, hi = R;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (table[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

struct Cell { float x, y, z; };

// box-frame centre of cell `local` of an RoI with grid (., dy, dz): x slowest, z fastest
__device__ __forceinline__ Cell cell_centre(uint32_t local, const float* __restrict__ size,
                                            const int32_t* __restrict__ dim, float voxel_size) {
  const uint32_t dy = (uint32_t)max(dim[1], 1), dz = (uint32_t)max(dim[2], 1);
  const uint32_t ix = local / (dy * dz), rem = local - ix * (dy * dz);
  const uint32_t iy = rem / dz, iz = rem - iy * dz;
  return {ococc_cell_centre((int)ix, size[0], voxel_size), ococc_cell_centre((int)iy, size[1], voxel_size),
          ococc_cell_centre((int)iz, size[2], voxel_size)};
}

// What the fill launch of the select kernel writes: a row per selected cell, in cell order.
struct OccFillArgs {
  const int64_t* scan;      // [max_tiles] exclusive prefix of tile_counts
  const float* sizes;       // [R, 3] enlarged sizes
  const int32_t* dims;      // [R, 3]
  float voxel_size;
  const float* rois;        // the pose, or null (box frame): rows of roi_stride floats, columns 1-3 the bottom centre,
  int64_t roi_stride;       //   column 6 the height
  const float* cos_yaw;     // [R]
  const float* sin_yaw;     // [R]
  const float* transforms;  // [R, 12] row-major 3x4 applied after the pose, or null
  const float* roi_value;   // [R] for column 3, or null: sigmoid(logit)
  int cols;                 // 3 or 4
  float* out;               // [n_out, cols]
  uint8_t* flags;           // [n_out] bit 0 predicted, bit 1 observed; or null
  int64_t n_out;
};

// The two launches of the select kernel, behind ococc_occ_select_* and ococc_occ_frame_*; `fn`, the export, heads the
// messages.  Selected: (ococc_occupied(logit) or observed[cell]) and row_keep[RoI] != 0; observed and row_keep may be null.
// count checks its arguments, zeroes roi_counts and derives tile_start in front; fill launches only.
int occ_select_count(const char* fn, const float* logits, const uint8_t* observed, const uint8_t* row_keep, int64_t n,
                     const int64_t* start, int32_t R, float pos_thresh, int64_t* tile_start, int32_t* tile_counts,
                     int64_t max_tiles, int64_t* roi_counts, hipStream_t stream);
int occ_select_fill(const char* fn, const float* logits, const uint8_t* observed, const uint8_t* row_keep, int64_t n,
                    const int64_t* start, const int64_t* tile_start, int32_t R, float pos_thresh, int64_t max_tiles,
                    const OccFillArgs& a, hipStream_t stream);
