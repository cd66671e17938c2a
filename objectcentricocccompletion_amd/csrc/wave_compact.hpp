// Ordered compaction, one wave per tile: the survivors of kCompactTile consecutive elements written in input order
// by two launches.  Count leaves the survivors per tile (and one 64-bit integer atomic per tile into the tile's group:
// RoI, frame); with base = the exclusive prefix of the tile counts, fill writes a survivor at base + (survivors of
// earlier rounds) + (survivors below the lane): (tile, round, lane) IS ascending input order, so no sort.
// Integer arithmetic only: the callers' float expressions stay behind their own `#pragma clang fp contract(off)`.
#pragma once
#include "common.hpp"

constexpr int kCompactRounds = 16;                    // elements per lane
constexpr int kCompactTile = 64 * kCompactRounds;     // 1024 elements per wave
constexpr int kCompactWaves = 4;                      // tiles per block

// the rank of `lane` among the set lanes of a ballot
__device__ __forceinline__ int wave_rank(unsigned long long bal, int lane) {
  return __popcll(bal & ((1ull << lane) - 1ull));
}

// One tile.  survives(i, v): does element i in [0, kCompactTile) of the tile survive; v (a default-constructed V) takes
// what was loaded for it.  emit(i, v, pos): write survivor i as entry pos of the output (FILL only, pos < n_out -- always,
// when count, scan and fill saw the same input).  Count: lane 0 stores the tile's count and adds it to its group's.
template <bool FILL, class V, class Survives, class Emit>
__device__ __forceinline__ void wave_tile_compact(int lane, int64_t base, int64_t n_out, int32_t* tile_count,
                                                  unsigned long long* group_count, Survives survives, Emit emit) {
  int cnt = 0;   // wave-uniform
#pragma unroll 4
  for (int k = 0; k < kCompactRounds; ++k) {
    const int i = k * 64 + lane;
    V v{};
    const bool in = survives(i, v);
    const unsigned long long bal = __ballot(in);
    if (FILL && in) {
      const int64_t pos = base + cnt + wave_rank(bal, lane);
      if (pos < n_out) emit(i, v, pos);
    }
    cnt += __popcll(bal);
  }
  if (!FILL && lane == 0) {
    *tile_count = cnt;
    if (cnt) atomicAdd(group_count, (unsigned long long)cnt);
  }
}
