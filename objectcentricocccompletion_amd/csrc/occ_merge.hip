// Occupancy-enhanced scene cloud: the frame's LiDAR cloud followed by the completed-occupancy cells that pass the score
// test, every row with two more columns (objectness score, indicator) -- 0, 0 for a real point, score, 1 for a cell.
// Stands behind occ_ops.occ_merge and the ``merged=`` result of TrackletRoIHeadOCC.simple_test_scene_step; replaces
// the slice / boolean index / np.pad / np.concatenate chain of LoadPointsAndOccPredFromFile and LoadOccPredFromFile
// (mmdet3d/datasets/pipelines/occ_pinelines.py:585-806) for a cloud and cells that are already on the device.
//
// The cells are the packed rows (x, y, z, value) of occ_frame.hip, row after row; start [R + 1] i64 is the exclusive
// prefix of the cells per row.  PER-ROW tiles as occ_tiles.hpp lays them out: kCompactTile consecutive cells of ONE row
// (the last tile of a row is short), tile_start [R + 1] the exclusive prefix of ceil(cells / 1024) per row.  A tile has
// one row, so the row's score is one wave-uniform load and the row's count one integer atomic per tile.
//
//   table  : one wave in front of count.  Checks start (start[r] >= 0, start[r] <= start[r + 1], start[R] <= M) and
//            writes tile_start and row_counts = 0; a table that fails gets tile_start = 0 everywhere -- no tile runs,
//            nothing is read through it -- and row_counts = -1, which the host reports after its one read-back.
//   count  : one wave per tile (wave_compact.hpp).  A cell survives iff score > score_threshold (f32, strict; a NaN
//            score never does) and, with flags, (flags[m] & 2) == 0; score = row_score[r], or column 3 of the cell.
//   fill   : ONE launch, two block roles.  The first cdiv(max_tiles, 4) blocks run the same tiles: wave_tile_compact
//            ranks the survivors, their tile-local indices go to LDS (2 bytes each), and the wave then writes
//            count * (D + 2) consecutive output ELEMENTS, one per lane and step.  The other blocks copy the N real rows,
//            again one thread per output element: element e of the head is points[e / W, use_dim[e % W]] or 0.
//            Loads and stores of neighbouring lanes are neighbouring words at every row width.
//
// Algorithmic bytes: count 4 (+1) B in per cell; fill 4 (D + 2) B out per row, 4 D B in per real row, 12-16 B in per
// survivor.  Memory bound.  The payload moves as 32-bit words: no arithmetic, a NaN or a denormal passes bit for bit.
// Integer atomics only; the same input gives the same bytes.  Vector stores only.
//
// SEVERAL FRAMES PER CALL (ococc_occ_merge_frames_*, occ_ops.occ_merge_frames): the same three kernels with a MergeFrames
// table.  points holds F clouds back to back (cloud_start [F + 1]), the rows of occ are in the caller's order (slot-major
// in a chunked step) and row_frame [R] names the cloud of each.  order [R] is the stable frame-major order of the rows
// and frame_first [F + 1] where each frame begins in it; both are the host's.  The tiles are laid out ALONG THE ORDER:
// tile_start [R + 1] is the prefix of ceil(cells / 1024) of row order[p], so the exclusive scan of tile_counts is the
// rank of a survivor among the survivors of the whole call, frame after frame.  Output, frame after frame: the rows of
// cloud f, then the survivors of the rows of frame f.  With S_f = scan[tile_start[frame_first[f]]], the survivors of
// the frames before f (K past the last tile), a real row i of cloud f is output row i + S_f and tile t of frame f starts
// at output row cloud_start[f + 1] + scan[t]: nothing but the scan is needed on the device, and nothing is uploaded
// after the read-back.  table also checks order (entries in [0, R)), row_frame (in [0, F), non-decreasing along the
// order, frame_first[f] <= p < frame_first[f + 1]) and cloud_start / frame_first (ascending from 0 to N / R); the
// kernels clamp whatever they take from a table, so a wrong one reads nothing outside [0, M) and [0, N) and writes
// nothing outside merged.  Without the table (order null) the kernels are the single-frame ones, byte for byte.
#include "common.hpp"
#include "occ_tiles.hpp"

namespace {

constexpr int kTile = kCompactTile;   // 1024 cells per wave
constexpr int kWaves = kCompactWaves;
constexpr int kBlock = 64 * kWaves;
constexpr int kCopyPerThread = 8;
constexpr int kCopyPerBlock = kBlock * kCopyPerThread;   // output elements of the real rows per block
constexpr int kMaxDims = 16;

struct MergeDims { int32_t d[kMaxDims]; };

// the frames of a call; order null: one frame, the rows in input order
struct MergeFrames {
  const int64_t* order;         // [R] the rows sorted by frame, stable
  const int64_t* row_frame;     // [R] the frame of row r
  const int64_t* cloud_start;   // [F + 1] exclusive prefix of the cloud sizes
  const int64_t* frame_first;   // [F + 1] where the rows of frame f begin in order
  int F;
};

struct MergeIn {
  const uint32_t* occ;         // [M, 4] words of (x, y, z, value)
  int64_t M;
  const int64_t* start;        // [R + 1]
  const int64_t* tile_start;   // [R + 1] along the order
  int R;
  MergeFrames fr;
  int64_t N;
  const float* row_score;      // [R] or null: column 3
  const uint8_t* flags;        // [M] or null: nothing dropped for being observed
  float threshold;
  int64_t max_tiles;
};

struct MergeTile {
  bool active;
  int r;
  int64_t c0, cend;   // cells [c0, cend) of row r
  float score;        // row_score[r], when given
};

struct Nothing {};

__global__ void __launch_bounds__(64)
occ_merge_table_kernel(const int64_t* __restrict__ start, int R, int64_t M, MergeFrames fr, int64_t N,
                       int64_t* __restrict__ tile_start, int64_t* __restrict__ row_counts) {
  const int lane = threadIdx.x;
  bool bad = false;
  for (int base = 0; base < R; base += 64) {
    const int r = base + lane;
    if (r < R) {
      const int64_t s0 = start[r], s1 = start[r + 1];
      bad = bad || s0 < 0 || s1 < s0 || s1 > M;
    }
  }
  if (fr.order) {
    const int F = fr.F;
    for (int base = 0; base < F; base += 64) {   // both prefixes ascend from 0 to their end
      const int f = base + lane;
      if (f < F) {
        const int64_t c0 = fr.cloud_start[f], c1 = fr.cloud_start[f + 1];
        const int64_t p0 = fr.frame_first[f], p1 = fr.frame_first[f + 1];
        bad = bad || c0 < 0 || c1 < c0 || c1 > N || p0 < 0 || p1 < p0 || p1 > R;
        bad = bad || (f == 0 && (c0 != 0 || p0 != 0)) || (f == F - 1 && (c1 != N || p1 != R));
      }
    }
    bad = __any(bad) || F < 1;
    for (int base = 0; base < R && !bad; base += 64) {   // (the prefixes hold: frame_first[f + 1] <= R is read below)
      const int p = base + lane;
      if (p < R) {
        const int64_t o = fr.order[p], o1 = p ? fr.order[p - 1] : -1, own = fr.row_frame[p];
        bool ok = o >= 0 && o < R && own >= 0 && own < F && (p == 0 || (o1 >= 0 && o1 < R));
        if (ok) {
          const int64_t f = fr.row_frame[o];
          ok = f >= 0 && f < F && (p == 0 || fr.row_frame[o1] <= f);
          ok = ok && fr.frame_first[f] <= p && p < fr.frame_first[f + 1];
        }
        bad = bad || !ok;
      }
    }
  }
  bad = __any(bad);
  int64_t carry = 0;
  if (lane == 0) tile_start[0] = 0;
  for (int base = 0; base < R; base += 64) {
    const int r = base + lane;   // position r of the order
    int64_t v = 0;
    if (r < R && !bad) {
      const int64_t o = fr.order ? fr.order[r] : r;
      const int64_t k = start[o + 1] - start[o];
      v = (k + kTile - 1) / kTile;
    }
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t u = __shfl_up(v, d, 64);
      if (lane >= d) v += u;
    }
    if (r < R) {
      tile_start[r + 1] = carry + v;
      row_counts[r] = bad ? -1 : 0;
    }
    carry += __shfl(v, 63, 64);
  }
}

// tile t of the per-row tiles (wave-uniform); every bound is clamped, so a table that count did not derive reads no
// cell outside [0, M)
__device__ __forceinline__ MergeTile merge_tile(const MergeIn& in, int64_t t) {
  MergeTile tl{false, 0, 0, 0, 0.f};
  if (t < 0 || t >= in.max_tiles || t >= in.tile_start[in.R]) return tl;
  const int p = roi_of(in.tile_start, in.R, t);
  tl.r = in.fr.order ? (int)min(max(in.fr.order[p], (int64_t)0), (int64_t)in.R - 1) : p;
  const int64_t off = t - in.tile_start[p];
  const int64_t s0 = in.start[tl.r], s1 = in.start[tl.r + 1];
  if (off < 0 || s0 < 0 || s1 < s0 || s1 > in.M || off >= (s1 - s0 + kTile - 1) / kTile) return tl;
  tl.c0 = s0 + off * kTile;
  tl.cend = min(s1, tl.c0 + kTile);
  tl.score = in.row_score ? in.row_score[tl.r] : 0.f;
  tl.active = true;
  return tl;
}

// the output row where the cells of row r's frame begin, less the survivors in front of them: the end of its cloud
__device__ __forceinline__ int64_t merge_cells_at(const MergeIn& in, int r) {
  if (!in.fr.order) return in.N;
  const int64_t f = min(max(in.fr.row_frame[r], (int64_t)0), (int64_t)in.fr.F - 1);
  return min(max(in.fr.cloud_start[f + 1], (int64_t)0), in.N);
}

// S_f, the survivors of the frames before f: the scan at the frame's first tile, K past the last tile
__device__ __forceinline__ int64_t merge_survivors_before(const MergeIn& in, const int64_t* __restrict__ scan, int f,
                                                          int64_t K) {
  const int64_t p = min(max(in.fr.frame_first[f], (int64_t)0), (int64_t)in.R);
  const int64_t t = in.tile_start[p];
  if (t < 0) return 0;
  if (t >= in.max_tiles) return K;
  return min(max(scan[t], (int64_t)0), K);
}

__device__ __forceinline__ bool merge_survives(const MergeIn& in, const MergeTile& tl, int i) {
  const int64_t m = tl.c0 + i;
  if (m >= tl.cend) return false;
  const float score = in.row_score ? tl.score : __uint_as_float(in.occ[m * 4 + 3]);
  const bool seen = in.flags && (in.flags[m] & 2) != 0;
  return score > in.threshold && !seen;   // (NaN: the comparison does not hold)
}

__global__ void __launch_bounds__(kBlock)
occ_merge_count_kernel(MergeIn in, int32_t* __restrict__ tile_counts, unsigned long long* __restrict__ row_counts) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);   // wave-uniform
  if (t >= in.max_tiles) return;
  const MergeTile tl = merge_tile(in, t);
  if (!tl.active) {
    if (lane == 0) tile_counts[t] = 0;
    return;
  }
  wave_tile_compact<false, Nothing>(
      lane, 0, 0, tile_counts + t, row_counts + tl.r, [&](int i, Nothing&) { return merge_survives(in, tl, i); },
      [](int, const Nothing&, int64_t) {});
}

__global__ void __launch_bounds__(kBlock)
occ_merge_fill_kernel(MergeIn in, const int64_t* __restrict__ scan, unsigned tile_blocks,
                      const uint32_t* __restrict__ points, int64_t N, int C, MergeDims dims, int D,
                      uint32_t* __restrict__ out, int64_t K) {
  const int W = D + 2;
  if (blockIdx.x < tile_blocks) {
    // role 1: the survivors of four tiles, rows (end of the tile's cloud) + scan[t] ...
    __shared__ uint16_t s_idx[kWaves][kTile];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * kWaves + w;   // wave-uniform
    const MergeTile tl = merge_tile(in, t);
    int64_t base = 0, at = in.N;
    int cnt = 0;
    if (tl.active) {
      at = merge_cells_at(in, tl.r);
      base = scan[t];
      const int64_t next = min(t + 1 < in.max_tiles ? scan[t + 1] : K, K);
      cnt = base < 0 ? 0 : (int)max((int64_t)0, min(next - base, (int64_t)kTile));
      wave_tile_compact<true, Nothing>(
          lane, base, K, nullptr, nullptr, [&](int i, Nothing&) { return merge_survives(in, tl, i); },
          [&](int i, const Nothing&, int64_t pos) {
            const int64_t k = pos - base;
            if (k >= 0 && k < cnt) s_idx[w][k] = (uint16_t)i;
          });
    }
    __syncthreads();   // (every wave of the block arrives: no early return above)
    const uint32_t total = (uint32_t)cnt * (uint32_t)W;
    uint32_t* o = out + (at + base) * W;
    const uint32_t score_bits = __float_as_uint(tl.score), one_bits = __float_as_uint(1.0f);
    for (uint32_t e = lane; e < total; e += 64) {
      const uint32_t k = e / (uint32_t)W;
      const int j = (int)(e - k * (uint32_t)W);
      const int64_t m = min(tl.c0 + s_idx[w][k], tl.cend - 1);   // (clamped: a scan that is not count's reads no cell past the tile)
      uint32_t v = 0u;
      if (j < 3) v = in.occ[m * 4 + j];
      else if (j == D) v = in.row_score ? score_bits : in.occ[m * 4 + 3];
      else if (j == D + 1) v = one_bits;
      o[e] = v;
    }
    return;
  }
  // role 2: the real rows, kCopyPerBlock consecutive output elements per block
  __shared__ int s_dim[kMaxDims];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kMaxDims; ++k) s_dim[k] = dims.d[k];
  }
  __syncthreads();
  const int64_t total = N * W;
  const int64_t e0 = (int64_t)(blockIdx.x - tile_blocks) * kCopyPerBlock;
  const int64_t row0 = e0 / W;                       // block-uniform: the one 64-bit division
  const uint32_t rem0 = (uint32_t)(e0 - row0 * W);
  // several frames: the rows of cloud f move down by S_f rows.  f of the block's first row by one search, then carried
  // along the thread's rows (they ascend); a step only at a seam, so lanes part only there.
  const bool frames = in.fr.order != nullptr && e0 < total;
  int f = 0;
  int64_t fend = N, shift = 0;
  if (frames) {
    f = roi_of(in.fr.cloud_start, in.fr.F, row0);
    fend = in.fr.cloud_start[f + 1];
    shift = merge_survivors_before(in, scan, f, K) * W;
  }
#pragma unroll
  for (int u = 0; u < kCopyPerThread; ++u) {
    const uint32_t l = (uint32_t)(u * kBlock) + threadIdx.x;
    if (e0 + l >= total) break;
    const uint32_t x = rem0 + l, q = x / (uint32_t)W;
    const int j = (int)(x - q * (uint32_t)W);
    if (frames && row0 + q >= fend && f + 1 < in.fr.F) {
      do fend = in.fr.cloud_start[++f + 1]; while (row0 + q >= fend && f + 1 < in.fr.F);
      shift = merge_survivors_before(in, scan, f, K) * W;
    }
    out[e0 + l + shift] = j < D ? points[(row0 + q) * C + s_dim[j]] : 0u;   // (shift <= K W: inside merged)
  }
}

MergeIn merge_in(const float* occ, int64_t M, const int64_t* start, const int64_t* tile_start, int R,
                 const MergeFrames& fr, int64_t N, const float* row_score, const uint8_t* flags, int drop_observed,
                 float threshold, int64_t max_tiles) {
  return MergeIn{reinterpret_cast<const uint32_t*>(occ), M, start, tile_start, R, fr, N, row_score,
                 drop_observed ? flags : nullptr, threshold, max_tiles};
}

#define MERGE_REQUIRE(cond, msg)                              \
  do {                                                        \
    if (!(cond)) return ococc_fail(OCOCC_EINVAL, fn, msg);    \
  } while (0)
#define MERGE_CHECK_LAUNCH()                                                             \
  do {                                                                                   \
    hipError_t e__ = hipGetLastError();                                                  \
    if (e__ != hipSuccess) return ococc_fail(OCOCC_EHIP, fn, hipGetErrorString(e__));    \
  } while (0)

// the frames arguments of an ococc_occ_merge_frames_* export; with rows (R > 0) every table is needed
int merge_frames_args(const char* fn, const MergeFrames& fr, int R, int64_t N) {
  MERGE_REQUIRE(fr.F >= 0 && fr.F <= 65535, "F < 0 or more than 65535 frames per call");
  MERGE_REQUIRE(fr.F > 0 || (R == 0 && N == 0), "F == 0 with rows or points");
  return OCOCC_OK;
}

// the launches behind both count exports; fr.order null: one frame
int merge_count(const char* fn, const float* occ, int64_t M, const int64_t* start, int32_t R, const MergeFrames& fr,
                int64_t N, const float* row_score, const uint8_t* flags, int32_t drop_observed, float score_threshold,
                int64_t* tile_start, int32_t* tile_counts, int64_t max_tiles, int64_t* row_counts, hipStream_t stream) {
  MERGE_REQUIRE(M >= 0 && R >= 0, "M < 0 or R < 0");
  MERGE_REQUIRE(max_tiles >= ococc_occ_select_max_tiles(M, R), "max_tiles < ococc_occ_select_max_tiles(M, R)");
  if (R == 0) return OCOCC_OK;
  MERGE_REQUIRE(start && tile_start && row_counts, "null pointer: start, tile_start or row_counts");
  hipLaunchKernelGGL(occ_merge_table_kernel, dim3(1), dim3(64), 0, stream, start, R, M, fr, N, tile_start, row_counts);
  MERGE_CHECK_LAUNCH();
  if (max_tiles == 0) return OCOCC_OK;
  MERGE_REQUIRE(tile_counts && (occ || M == 0), "null pointer: tile_counts or occ");
  hipLaunchKernelGGL(occ_merge_count_kernel, dim3((unsigned)ococc_cdiv(max_tiles, kWaves)), dim3(kBlock), 0, stream,
                     merge_in(occ, M, start, tile_start, R, fr, N, row_score, flags, drop_observed, score_threshold,
                              max_tiles),
                     tile_counts, reinterpret_cast<unsigned long long*>(row_counts));
  MERGE_CHECK_LAUNCH();
  return OCOCC_OK;
}

// the launch behind both fill exports
int merge_fill(const char* fn, const float* points, int64_t N, int32_t C, const int32_t* use_dim, int32_t D,
               const float* occ, int64_t M, const int64_t* start, const int64_t* tile_start, int32_t R,
               const MergeFrames& fr, const float* row_score, const uint8_t* flags, int32_t drop_observed,
               float score_threshold, const int64_t* tile_scan, int64_t max_tiles, float* merged, int64_t K,
               hipStream_t stream) {
  MERGE_REQUIRE(N >= 0 && M >= 0 && R >= 0 && K >= 0, "N < 0, M < 0, R < 0 or K < 0");
  MERGE_REQUIRE(K <= M, "K > M: more survivors than cells");
  MERGE_REQUIRE(D >= 3 && D <= kMaxDims, "use_dim has 3 to 16 entries (x, y, z first)");
  MERGE_REQUIRE(use_dim, "null pointer: use_dim (a host array of D column indices)");
  MERGE_REQUIRE(C >= 1, "C < 1");
  MergeDims dims{};
  for (int j = 0; j < D; ++j) {
    MERGE_REQUIRE(use_dim[j] >= 0 && use_dim[j] < C, "use_dim entry outside [0, C)");
    dims.d[j] = use_dim[j];
  }
  const int64_t W = D + 2;
  MERGE_REQUIRE(N <= (INT64_MAX / 4) / W - M && N <= (INT64_MAX / 4) / C, "N too large");
  MERGE_REQUIRE(max_tiles >= ococc_occ_select_max_tiles(M, R), "max_tiles < ococc_occ_select_max_tiles(M, R)");
  if (N + K == 0) return OCOCC_OK;
  MERGE_REQUIRE(merged && (points || N == 0), "null pointer: merged or points");
  const bool cells = K > 0 && R > 0 && max_tiles > 0;
  if (cells) MERGE_REQUIRE(occ && start && tile_start && tile_scan, "null pointer: occ, start, tile_start or tile_scan");
  const int64_t tile_blocks = cells ? ococc_cdiv(max_tiles, kWaves) : 0;
  const int64_t blocks = tile_blocks + ococc_cdiv(N * W, kCopyPerBlock);
  MERGE_REQUIRE(blocks <= 0x7fffffff, "more than 2^31 - 1 blocks");
  // without survivors no real row moves: the copy of one frame, nothing of the tables is read
  hipLaunchKernelGGL(occ_merge_fill_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream,
                     merge_in(occ, M, start, tile_start, R, cells ? fr : MergeFrames{}, N, row_score, flags,
                              drop_observed, score_threshold, max_tiles),
                     tile_scan, (unsigned)tile_blocks, reinterpret_cast<const uint32_t*>(points), N, (int)C, dims, (int)D,
                     reinterpret_cast<uint32_t*>(merged), K);
  MERGE_CHECK_LAUNCH();
  return OCOCC_OK;
}

}  // namespace

extern "C" int ococc_occ_merge_count(const float* occ, int64_t M, const int64_t* start, int32_t R, const float* row_score,
                                     const uint8_t* flags, int32_t drop_observed, float score_threshold,
                                     int64_t* tile_start, int32_t* tile_counts, int64_t max_tiles, int64_t* row_counts,
                                     ococc_stream_t stream) {
  return merge_count(__func__, occ, M, start, R, MergeFrames{}, 0, row_score, flags, drop_observed, score_threshold,
                     tile_start, tile_counts, max_tiles, row_counts, (hipStream_t)stream);
}

extern "C" int ococc_occ_merge_fill(const float* points, int64_t N, int32_t C, const int32_t* use_dim, int32_t D,
                                    const float* occ, int64_t M, const int64_t* start, const int64_t* tile_start,
                                    int32_t R, const float* row_score, const uint8_t* flags, int32_t drop_observed,
                                    float score_threshold, const int64_t* tile_scan, int64_t max_tiles, float* merged,
                                    int64_t K, ococc_stream_t stream) {
  return merge_fill(__func__, points, N, C, use_dim, D, occ, M, start, tile_start, R, MergeFrames{}, row_score, flags,
                    drop_observed, score_threshold, tile_scan, max_tiles, merged, K, (hipStream_t)stream);
}

extern "C" int ococc_occ_merge_frames_count(const float* occ, int64_t M, const int64_t* start, const int64_t* order,
                                            const int64_t* row_frame, int32_t R, const int64_t* cloud_start,
                                            const int64_t* frame_first, int32_t F, int64_t N, const float* row_score,
                                            const uint8_t* flags, int32_t drop_observed, float score_threshold,
                                            int64_t* tile_start, int32_t* tile_counts, int64_t max_tiles,
                                            int64_t* row_counts, ococc_stream_t stream) {
  const char* fn = __func__;
  const MergeFrames fr{order, row_frame, cloud_start, frame_first, F};
  MERGE_REQUIRE(N >= 0, "N < 0");
  if (int rc = merge_frames_args(fn, fr, R, N)) return rc;
  if (R > 0) MERGE_REQUIRE(order && row_frame && cloud_start && frame_first, "null pointer: order, row_frame, cloud_start or frame_first");
  return merge_count(fn, occ, M, start, R, fr, N, row_score, flags, drop_observed, score_threshold, tile_start,
                     tile_counts, max_tiles, row_counts, (hipStream_t)stream);
}

extern "C" int ococc_occ_merge_frames_fill(const float* points, int64_t N, int32_t C, const int32_t* use_dim, int32_t D,
                                           const float* occ, int64_t M, const int64_t* start, const int64_t* order,
                                           const int64_t* row_frame, const int64_t* tile_start, int32_t R,
                                           const int64_t* cloud_start, const int64_t* frame_first, int32_t F,
                                           const float* row_score, const uint8_t* flags, int32_t drop_observed,
                                           float score_threshold, const int64_t* tile_scan, int64_t max_tiles,
                                           float* merged, int64_t K, ococc_stream_t stream) {
  const char* fn = __func__;
  const MergeFrames fr{order, row_frame, cloud_start, frame_first, F};
  MERGE_REQUIRE(N >= 0 && R >= 0, "N < 0 or R < 0");
  if (int rc = merge_frames_args(fn, fr, R, N)) return rc;
  if (K > 0 && R > 0) MERGE_REQUIRE(order && row_frame && cloud_start && frame_first, "null pointer: order, row_frame, cloud_start or frame_first");
  return merge_fill(fn, points, N, C, use_dim, D, occ, M, start, tile_start, R, fr, row_score, flags, drop_observed,
                    score_threshold, tile_scan, max_tiles, merged, K, (hipStream_t)stream);
}
