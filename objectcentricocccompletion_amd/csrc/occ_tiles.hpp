// What the order-preserving compactions over the flat cell list share (occ_export.hip, occ_frame.hip): the RoI search
// over a prefix table, the centre of a cell from its id, and the one-wave kernel that derives the tile table.
// The list: RoI after RoI, x slowest and z fastest inside an RoI; start [R + 1] i64 the exclusive prefix of the cells
// per RoI; tiles of kOccCompactTile consecutive cells of ONE RoI (occ_math.hpp).
#pragma once
#include "common.hpp"
#include "occ_math.hpp"

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

// tile_start [R + 1]: exclusive prefix of ceil((start[r + 1] - start[r]) / 1024).  One wave, 64 RoIs per step.
// (static: one copy per translation unit that launches it)
static __global__ void __launch_bounds__(64)
tile_table_kernel(const int64_t* __restrict__ start, int R, int64_t* __restrict__ tile_start) {
  const int lane = threadIdx.x;
  int64_t carry = 0;
  if (lane == 0) tile_start[0] = 0;
  for (int base = 0; base < R; base += 64) {
    const int r = base + lane;
    int64_t v = 0;
    if (r < R) {
      const int64_t k = start[r + 1] - start[r];
      v = k > 0 ? (k + kOccCompactTile - 1) / kOccCompactTile : 0;
    }
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t u = __shfl_up(v, d, 64);
      if (lane >= d) v += u;
    }
    if (r < R) tile_start[r + 1] = carry + v;
    carry += __shfl(v, 63, 64);
  }
}
