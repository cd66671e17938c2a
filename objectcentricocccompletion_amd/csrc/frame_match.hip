// Detection matching of the native Waymo metric (objectcentricocccompletion_amd/waymo_metrics.py): per frame, the full 3-D
// IoU of every (prediction, ground truth) pair of equal type, then the score-first greedy assignment.  It replaces the
// matching stage of compute_detection_metrics_main (the compiled waymo-open-dataset tool the reference calls from
// mmdet3d/datasets/waymo_tracklet_dataset.py:352-366 and ships no source for).
//
// Boxes are [7] f32 in the Waymo convention: centre x, y, z, length (along the heading), width, height, heading.
// Predictions arrive sorted by (frame, type, descending score, file order), ground truth grouped by frame in file order.
//
// Two launches per call, whatever the number of frames:
//
//  frame_overlap_kernel   the pairs of all frames of the call are ONE flat index space (pair_offsets [F+1], the running
//    sum of n_pd * n_gt); a wave owns 1024 consecutive pairs, so a frame of 3 boxes and a frame of 600 fill lanes alike.
//    Pass A, 16 x 64 pairs: type / eligibility, then the cheap rejects (BEV centre distance against the sum of the half
//    diagonals, height intervals) -- nearly every pair of a frame ends here with a coalesced store of +0.  Survivors are
//    compacted into the wave's LDS list with a ballot and a popcount (no atomics).  Pass B: the wave clips its survivors
//    64 at a time, so the ~1k-instruction clip runs on full waves instead of on the one or two lanes of 64 that survive.
//    The clip works in the ground-truth box's own frame (translated AND rotated: the box is the axis-aligned rectangle
//    [-l/2, l/2] x [-w/2, w/2], the prediction's corners are clipped against four axis-parallel lines), so no product
//    ever sees a coordinate of 75 m and the f32 cancellation of aligned_iou3d_pair far from the origin cannot occur.
//
//  frame_greedy_kernel    one wave per frame: predictions in their (score) order, lanes over the frame's ground truth;
//    each step is one row read of the overlap matrix, a wave arg-max by shuffles (larger IoU, then lower index) and one
//    bit of the `taken` mask that lane (g & 63) keeps for g, g + 64, ... in a 64-bit register (<= 4096 ground-truth
//    boxes per frame).  Types never compete (the matrix holds +0 across types), so one pass serves all types.
//
//  frame_assign_kernel    (ococc_frame_assign_i32, in place of frame_greedy_kernel) one wave per frame: the maximum-weight
//    assignment of every (frame, type) group at every score cutoff by sequential shortest augmenting paths on integer
//    weights; described where it stands, below.
//
// Every output word is written by exactly one lane from values that depend on the input alone: no atomics, no
// dependence on launch or wave order, the same bytes on every run.
// Bytes: pairs * 4 B written and read once (the matrix), boxes re-read from L2; ALU bound in pass B.
#include "common.hpp"

namespace {

constexpr int kWavePairs = 1024;    // pairs per wave in frame_overlap_kernel (16 rounds of 64)
constexpr int kWaves = 4;

struct Thresholds { float v[5]; };

struct Pt { float x, y; };

// area of  [-hl, hl] x [-hw, hw]  intersected with the convex quadrilateral q (either winding): Sutherland-Hodgman
// against the four axis-parallel lines (at most 8 vertices)
__device__ float clip_area(const Pt* q, float hl, float hw) {
  Pt poly[9], tmp[9];
  int n = 4;
  for (int i = 0; i < 4; ++i) poly[i] = q[i];
  for (int e = 0; e < 4 && n > 0; ++e) {
    // signed distance to edge e, >= 0 inside:  hl - x,  hl + x,  hw - y,  hw + y
    const float sx = e == 0 ? -1.f : (e == 1 ? 1.f : 0.f), sy = e == 2 ? -1.f : (e == 3 ? 1.f : 0.f);
    const float off = e < 2 ? hl : hw;
    int m = 0;
    for (int i = 0; i < n; ++i) {
      const Pt p = poly[i], r = poly[i + 1 == n ? 0 : i + 1];
      const float dp = off + sx * p.x + sy * p.y, dr = off + sx * r.x + sy * r.y;
      if (dp >= 0.f) tmp[m++] = p;
      if ((dp >= 0.f) != (dr >= 0.f)) {
        const float t = dp / (dp - dr);
        tmp[m].x = p.x + t * (r.x - p.x);
        tmp[m].y = p.y + t * (r.y - p.y);
        ++m;
      }
      if (m > 8) m = 8;   // (cannot happen for a convex input; keeps the store in bounds whatever the input)
    }
    n = m;
    for (int i = 0; i < n; ++i) poly[i] = tmp[i];
  }
  float area = 0.f;
  for (int i = 0; i < n; ++i) {
    const Pt p = poly[i], r = poly[i + 1 == n ? 0 : i + 1];
    area += p.x * r.y - r.x * p.y;
  }
  return fabsf(area) * 0.5f;
}

__device__ __forceinline__ bool box_ok(const float* b) {
  bool ok = b[3] > 0.f && b[4] > 0.f && b[5] > 0.f;    // (false for NaN extents)
#pragma unroll
  for (int k = 0; k < 7; ++k) ok = ok && isfinite(b[k]);
  return ok;
}

// 0: certainly no overlap (or a degenerate box), 1: clip it
__device__ __forceinline__ bool may_overlap(const float* p, const float* g) {
  if (!box_ok(p) || !box_ok(g)) return false;
  const float dz = p[2] - g[2];
  const float top = fminf(0.5f * g[5], dz + 0.5f * p[5]), bot = fmaxf(-0.5f * g[5], dz - 0.5f * p[5]);
  if (!(top - bot > 0.f)) return false;
  const float dx = p[0] - g[0], dy = p[1] - g[1];
  const float rp = 0.5f * sqrtf(p[3] * p[3] + p[4] * p[4]), rg = 0.5f * sqrtf(g[3] * g[3] + g[4] * g[4]);
  const float reach = (rp + rg) * 1.0001f + 0.01f;      // 1 cm more than f32 rounding could hide
  return dx * dx + dy * dy <= reach * reach;
}

// full 3-D IoU, prediction p against ground truth g, in g's frame
__device__ float iou3d_local(const float* p, const float* g) {
  const float dx = p[0] - g[0], dy = p[1] - g[1], dz = p[2] - g[2];
  const float cg = cosf(g[6]), sg = sinf(g[6]);
  const float cx = dx * cg + dy * sg, cy = -dx * sg + dy * cg;   // p's centre in g's frame
  const float rel = p[6] - g[6];
  const float cr = cosf(rel), sr = sinf(rel);
  const float hl = 0.5f * p[3], hw = 0.5f * p[4];
  const float ex[4] = {hl, hl, -hl, -hl}, ey[4] = {hw, -hw, -hw, hw};
  Pt q[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    q[k].x = cx + ex[k] * cr - ey[k] * sr;
    q[k].y = cy + ex[k] * sr + ey[k] * cr;
  }
  const float area = clip_area(q, 0.5f * g[3], 0.5f * g[4]);
  const float top = fminf(0.5f * g[5], dz + 0.5f * p[5]), bot = fmaxf(-0.5f * g[5], dz - 0.5f * p[5]);
  const float inter = area * fmaxf(top - bot, 0.f);
  const float uni = p[3] * p[4] * p[5] + g[3] * g[4] * g[5] - inter;
  const float iou = inter / fmaxf(uni, 1e-8f);
  return iou > 0.f ? iou : 0.f;    // (NaN -> 0)
}

// the frame f in [lo, hi] with pair_offsets[f] <= q < pair_offsets[f + 1]
__device__ __forceinline__ int frame_of(const int64_t* __restrict__ pair_offsets, int lo, int hi, int64_t q) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pair_offsets[mid] <= q) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

struct PairRef { int p, g; };

__device__ __forceinline__ PairRef pair_of(const int64_t* __restrict__ pair_offsets, const int32_t* __restrict__ pd_offsets,
                                           const int32_t* __restrict__ gt_offsets, int lo, int hi, int64_t q) {
  const int f = frame_of(pair_offsets, lo, hi, q);
  const int64_t local = q - pair_offsets[f];
  const int g0 = gt_offsets[f], ng = gt_offsets[f + 1] - g0;     // (ng > 0: the frame has a pair)
  PairRef r;
  r.p = pd_offsets[f] + (int)(local / ng);
  r.g = g0 + (int)(local % ng);
  return r;
}

__global__ void __launch_bounds__(kWaves * 64)
frame_overlap_kernel(const float* __restrict__ pd_boxes, const int32_t* __restrict__ pd_type,
                     const int32_t* __restrict__ pd_eligible, const int32_t* __restrict__ pd_offsets,
                     const float* __restrict__ gt_boxes, const int32_t* __restrict__ gt_type,
                     const int32_t* __restrict__ gt_eligible, const int32_t* __restrict__ gt_offsets,
                     const int64_t* __restrict__ pair_offsets, int frame_begin, int frame_end, int64_t pair_begin,
                     int64_t pair_end, float* __restrict__ overlap) {
  __shared__ uint16_t survivors[kWaves][kWavePairs];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile = pair_begin + ((int64_t)blockIdx.x * kWaves + wave) * kWavePairs;
  const int64_t tile_end = tile + kWavePairs < pair_end ? tile + kWavePairs : pair_end;
  int count = 0;                                    // wave-uniform
  int f_lo = frame_begin, f_hi = frame_begin;
  if (tile < tile_end) {                            // wave-uniform
    f_lo = frame_of(pair_offsets, frame_begin, frame_end - 1, tile);
    f_hi = frame_of(pair_offsets, f_lo, frame_end - 1, tile_end - 1);
    for (int r = 0; r < kWavePairs / 64; ++r) {
      const int64_t q = tile + r * 64 + lane;
      bool keep = false;
      if (q < tile_end) {
        const PairRef pr = pair_of(pair_offsets, pd_offsets, gt_offsets, f_lo, f_hi, q);
        const int t = pd_type[pr.p];
        if (t == gt_type[pr.g] && t >= 1 && t <= 4 && pd_eligible[pr.p] != 0 && gt_eligible[pr.g] != 0)
          keep = may_overlap(pd_boxes + (int64_t)pr.p * 7, gt_boxes + (int64_t)pr.g * 7);
        if (!keep) overlap[q - pair_begin] = 0.f;
      }
      const unsigned long long mask = __ballot(keep);
      if (keep) survivors[wave][count + __popcll(mask & ((1ull << lane) - 1ull))] = (uint16_t)(r * 64 + lane);
      count += __popcll(mask);
    }
  }
  __syncthreads();
  for (int i = lane; i < count; i += 64) {
    const int64_t q = tile + survivors[wave][i];
    const PairRef pr = pair_of(pair_offsets, pd_offsets, gt_offsets, f_lo, f_hi, q);
    overlap[q - pair_begin] = iou3d_local(pd_boxes + (int64_t)pr.p * 7, gt_boxes + (int64_t)pr.g * 7);
  }
}

__global__ void __launch_bounds__(kWaves * 64)
frame_greedy_kernel(const int32_t* __restrict__ pd_type, const int32_t* __restrict__ pd_offsets,
                    const int32_t* __restrict__ gt_offsets, const int64_t* __restrict__ pair_offsets, int frame_begin,
                    int frame_end, int64_t pair_begin, const float* __restrict__ overlap, Thresholds thr,
                    int32_t* __restrict__ match_gt, float* __restrict__ match_iou) {
  const int lane = threadIdx.x & 63;
  const int f = frame_begin + blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (f >= frame_end) return;                       // (wave-uniform)
  const int p0 = pd_offsets[f], np = pd_offsets[f + 1] - p0, g0 = gt_offsets[f], ng = gt_offsets[f + 1] - g0;
  const float* rows = overlap + (pair_offsets[f] - pair_begin);
  const int chunks = (ng + 63) >> 6;                // <= 64 (checked by the caller)
  unsigned long long taken = 0ull;                  // bit j: ground truth lane + 64 j of this frame
  for (int pl = 0; pl < np; ++pl) {
    const int t = pd_type[p0 + pl];
    // a type outside 1..4 has an all-zero row; +inf can never be reached
    const float need = t >= 1 && t <= 4 ? thr.v[t] : __builtin_inff();
    float best = -1.f;
    int best_g = 0x7fffffff;
    for (int j = 0; j < chunks; ++j) {
      const int gl = lane + (j << 6);
      if (gl < ng && !((taken >> j) & 1ull)) {
        const float v = rows[(int64_t)pl * ng + gl];
        if (v >= need && v > best) { best = v; best_g = gl; }   // ascending gl: the first of equal values stays
      }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const float ob = __shfl_xor(best, s, 64);
      const int og = __shfl_xor(best_g, s, 64);
      if (ob > best || (ob == best && og < best_g)) { best = ob; best_g = og; }
    }
    const bool hit = best_g != 0x7fffffff;          // wave-uniform after the butterfly
    if (hit && (best_g & 63) == lane) taken |= 1ull << (best_g >> 6);
    if (lane == 0) {
      match_gt[p0 + pl] = hit ? g0 + best_g : -1;
      match_iou[p0 + pl] = hit ? best : 0.f;
    }
  }
}


// ---- maximum-weight assignment per score cutoff (DESIGN 3.10 rule 4b) ------------------------------------------------
// One wave per frame, as in frame_greedy_kernel, lanes over the frame's ground-truth columns.  Predictions are inserted
// in the packed order; each insertion is one shortest-augmenting-path search over integer reduced costs
// (cost = -weight, weight = (int)(iou * 1000.0f) where iou >= the type's threshold, otherwise no edge).  Every
// prediction owns a private zero-cost column ("stay unmatched"): it is always free when its row is scanned, its column
// potential stays 0 and a row that sits on it has row potential 0, so the private columns need no storage -- the search
// keeps the nearest one (distance, and the column through which its row was reached) in two registers.  A real column
// wins against a private one of equal distance, the lower ground-truth index among real columns of equal distance, the
// row scanned first among private columns of equal distance.  All per-column state (column potential v, potential u of
// the row on the column, distance, row on the column, predecessor column) lives in the wave's slice of LDS, the
// row -> column map of the frame beside it; `done` (the columns whose distance is final) is one bit per column in a
// 64-bit register of lane (g & 63), as `taken` above.  Types never compete (no edges across types), so the columns of
// all types share one state and a (frame, type) group is still an independent problem.
// A prediction p with snap_offsets[p] >= 0 ends a cutoff bucket: the wave then writes the matching of its group's
// predictions inserted so far, snapshots[snap_offsets[p] + r] for the r-th prediction of the group, r = 0 .. p - group
// start.  A row without an edge costs one row read and a ballot.
constexpr int kAssignInf = 0x3fffffff;
constexpr int kAssignLdsLimit = 64 << 10;

// LDS written by one lane is read by the others of the wave: the hardware keeps a wave's LDS accesses in order, this keeps
// the compiler from moving them across the hand-over
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int edge_weight(float iou, float need) { return iou >= need ? (int)(iou * 1000.0f) : 0; }

// LDS bytes of one wave: four i32 and one i16 per column, one i16 per prediction
__host__ __device__ constexpr int64_t assign_wave_lds(int64_t cols_pad, int64_t rows_pad) { return cols_pad * 18 + rows_pad * 2; }

__global__ void __launch_bounds__(kWaves * 64)
frame_assign_kernel(const int32_t* __restrict__ pd_type, const int32_t* __restrict__ pd_offsets,
                    const int32_t* __restrict__ gt_offsets, const int64_t* __restrict__ pair_offsets, int frame_begin,
                    int frame_end, int64_t pair_begin, const float* __restrict__ overlap, Thresholds thr,
                    const int64_t* __restrict__ snap_offsets, int64_t num_snap_words, int32_t* __restrict__ snapshots,
                    int cols_pad, int rows_pad) {
  extern __shared__ __attribute__((aligned(16))) char assign_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const int f = frame_begin + blockIdx.x * waves + wave;
  if (f >= frame_end) return;                       // (wave-uniform; the kernel has no workgroup barrier)
  const int p0 = pd_offsets[f], np = pd_offsets[f + 1] - p0, g0 = gt_offsets[f], ng = gt_offsets[f + 1] - g0;
  if (ng > cols_pad || np > rows_pad) return;       // (checked by the caller; keeps every LDS index in bounds)
  int32_t* v = (int32_t*)(assign_lds + (int64_t)wave * assign_wave_lds(cols_pad, rows_pad));   // column potential
  int32_t* u = v + cols_pad;                        // potential of the row on the column
  int32_t* dist = u + cols_pad;                     // distance of the column in the running search
  int32_t* row_of = dist + cols_pad;                // frame-local row on the column, -1: free
  int16_t* via_col = (int16_t*)(row_of + cols_pad); // column whose row gave the column its distance, -1: the new row
  int16_t* col_of = via_col + cols_pad;             // column of the frame-local row, -1: unmatched
  const float* rows = overlap + (pair_offsets[f] - pair_begin);
  const int chunks = (ng + 63) >> 6;                // <= 64 (checked by the caller)
  for (int gl = lane; gl < ng; gl += 64) { v[gl] = 0; u[gl] = 0; row_of[gl] = -1; }
  for (int r = lane; r < np; r += 64) col_of[r] = -1;
  wave_sync();
  int group_start = 0, prev_t = 0;
  for (int pl = 0; pl < np; ++pl) {
    const int t = pd_type[p0 + pl];
    if (pl == 0 || t != prev_t) { group_start = pl; prev_t = t; }
    const float need = t >= 1 && t <= 4 ? thr.v[t] : __builtin_inff();
    bool any = false;
    for (int j = 0; j < chunks; ++j) {
      const int gl = lane + (j << 6);
      if (gl < ng) any = any || edge_weight(rows[(int64_t)pl * ng + gl], need) > 0;
    }
    if (__any(any)) {                               // (wave-uniform)
      for (int gl = lane; gl < ng; gl += 64) dist[gl] = kAssignInf;
      unsigned long long done = 0ull;               // bit j: column lane + 64 j has its final distance
      int min_val = 0, i = pl, u_i = 0, via = -1;   // the row being scanned, its potential, the column it came through
      int free_dist = kAssignInf, free_via = -1;    // the nearest private column
      int sink = -1;                                // the free real column the search ends on, -1: a private column
      while (true) {
        if (min_val - u_i < free_dist) { free_dist = min_val - u_i; free_via = via; }
        int low = kAssignInf, low_g = 0x7fffffff;
        const float* row = rows + (int64_t)i * ng;
        for (int j = 0; j < chunks; ++j) {
          const int gl = lane + (j << 6);
          if (gl < ng && !((done >> j) & 1ull)) {
            const int w = edge_weight(row[gl], need);
            int d = dist[gl];
            if (w > 0) {
              const int r = min_val - w - u_i - v[gl];
              if (r < d) { d = r; dist[gl] = r; via_col[gl] = (int16_t)via; }
            }
            if (d < low) { low = d; low_g = gl; }   // ascending gl: the first of equal distances stays
          }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
          const int ol = __shfl_xor(low, s, 64);
          const int og = __shfl_xor(low_g, s, 64);
          if (ol < low || (ol == low && og < low_g)) { low = ol; low_g = og; }
        }
        if (free_dist < low) { min_val = free_dist; break; }     // a real column wins a tie
        min_val = low;
        if ((low_g & 63) == lane) done |= 1ull << (low_g >> 6);
        wave_sync();
        const int r = row_of[low_g];
        if (r < 0) { sink = low_g; break; }
        i = r; u_i = u[low_g]; via = low_g;
      }
      // potentials of the finished columns and of the rows on them (the new row's becomes min_val)
      for (int j = 0; j < chunks; ++j) {
        const int gl = lane + (j << 6);
        if (gl < ng && ((done >> j) & 1ull)) {
          const int delta = min_val - dist[gl];
          u[gl] += delta;
          v[gl] -= delta;
        }
      }
      wave_sync();
      // augment backwards along the predecessor columns; every lane walks, lane 0 writes
      int j = sink;
      if (sink < 0 && free_via >= 0) {              // the row on column free_via moves to its private column
        j = free_via;
        if (lane == 0) col_of[row_of[j]] = -1;
      }
      while (j >= 0) {
        const int pc = via_col[j];
        const int r = pc >= 0 ? row_of[pc] : pl;
        const int ur = pc >= 0 ? u[pc] : min_val;
        wave_sync();            // (all lanes have read column pc before lane 0 overwrites it next turn)
        if (lane == 0) { row_of[j] = r; u[j] = ur; col_of[r] = (int16_t)j; }
        j = pc;
      }
      wave_sync();
    }
    const int64_t so = snap_offsets[p0 + pl];
    const int n = pl - group_start + 1;
    if (so >= 0 && so + n <= num_snap_words) {      // (wave-uniform)
      for (int r = lane; r < n; r += 64) {
        const int c = col_of[group_start + r];
        snapshots[so + r] = c >= 0 ? g0 + c : -1;
      }
    }
  }
}

}  // namespace

extern "C" int64_t ococc_frame_match_workspace_bytes(int64_t num_pairs) {
  if (num_pairs < 0) return -1;
  return ococc_align_up(num_pairs * 4, 256);
}

extern "C" int ococc_frame_match_f32(const float* pd_boxes, const int32_t* pd_type, const int32_t* pd_eligible,
                                     const int32_t* pd_offsets, int64_t num_pd, const float* gt_boxes,
                                     const int32_t* gt_type, const int32_t* gt_eligible, const int32_t* gt_offsets,
                                     int64_t num_gt, const int64_t* pair_offsets, int32_t frame_begin, int32_t frame_end,
                                     int64_t pair_begin, int64_t pair_end, int32_t max_frame_gt,
                                     const float host_iou_thresh[5], int32_t* match_gt, float* match_iou,
                                     void* workspace, int64_t workspace_bytes, ococc_stream_t stream) {
  OCOCC_REQUIRE(num_pd >= 0 && num_gt >= 0 && num_pd <= 0x7fffffffLL / 7 && num_gt <= 0x7fffffffLL / 7, "box counts out of range");
  OCOCC_REQUIRE(frame_begin >= 0 && frame_end >= frame_begin, "frame range");
  OCOCC_REQUIRE(pair_begin >= 0 && pair_end >= pair_begin, "pair range");
  OCOCC_REQUIRE(max_frame_gt >= 0 && max_frame_gt <= 4096, "more than 4096 ground-truth boxes in one frame");
  OCOCC_REQUIRE(host_iou_thresh != nullptr, "null iou thresholds");
  Thresholds thr;
  for (int k = 0; k < 5; ++k) {
    thr.v[k] = host_iou_thresh[k];
    OCOCC_REQUIRE(k == 0 || (thr.v[k] > 0.f && thr.v[k] <= 1.f), "iou thresholds of types 1..4 must lie in (0, 1]");
  }
  const int64_t pairs = pair_end - pair_begin;
  OCOCC_REQUIRE(workspace_bytes >= ococc_frame_match_workspace_bytes(pairs), "workspace too small");
  const int frames = frame_end - frame_begin;
  if (frames == 0 || num_pd == 0) return OCOCC_OK;
  OCOCC_REQUIRE(pd_type && pd_offsets && gt_offsets && pair_offsets && match_gt && match_iou, "null pointer");
  if (pairs > 0) {
    OCOCC_REQUIRE(pd_boxes && pd_eligible && gt_boxes && gt_type && gt_eligible && workspace, "null pointer");
    const int64_t blocks = ococc_cdiv(pairs, (int64_t)kWaves * kWavePairs);
    OCOCC_REQUIRE(blocks <= 0x7fffffffLL, "too many pairs for one launch");
    hipLaunchKernelGGL(frame_overlap_kernel, dim3((unsigned)blocks), dim3(kWaves * 64), 0, (hipStream_t)stream, pd_boxes,
                       pd_type, pd_eligible, pd_offsets, gt_boxes, gt_type, gt_eligible, gt_offsets, pair_offsets,
                       frame_begin, frame_end, pair_begin, pair_end, (float*)workspace);
    OCOCC_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(frame_greedy_kernel, dim3((unsigned)ococc_cdiv(frames, kWaves)), dim3(kWaves * 64), 0,
                     (hipStream_t)stream, pd_type, pd_offsets, gt_offsets, pair_offsets, frame_begin, frame_end, pair_begin,
                     (const float*)workspace, thr, match_gt, match_iou);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}

extern "C" int ococc_frame_assign_i32(const float* pd_boxes, const int32_t* pd_type, const int32_t* pd_eligible,
                                      const int32_t* pd_offsets, int64_t num_pd, const float* gt_boxes,
                                      const int32_t* gt_type, const int32_t* gt_eligible, const int32_t* gt_offsets,
                                      int64_t num_gt, const int64_t* pair_offsets, int32_t frame_begin, int32_t frame_end,
                                      int64_t pair_begin, int64_t pair_end, int32_t max_frame_gt, int32_t max_frame_pd,
                                      const float host_iou_thresh[5], const int64_t* snap_offsets,
                                      int64_t num_snap_words, int32_t* snapshots, void* workspace,
                                      int64_t workspace_bytes, ococc_stream_t stream) {
  OCOCC_REQUIRE(num_pd >= 0 && num_gt >= 0 && num_pd <= 0x7fffffffLL / 7 && num_gt <= 0x7fffffffLL / 7, "box counts out of range");
  OCOCC_REQUIRE(frame_begin >= 0 && frame_end >= frame_begin, "frame range");
  OCOCC_REQUIRE(pair_begin >= 0 && pair_end >= pair_begin, "pair range");
  OCOCC_REQUIRE(max_frame_gt >= 0 && max_frame_gt <= 4096, "more than 4096 ground-truth boxes in one frame");
  OCOCC_REQUIRE(max_frame_pd >= 0 && num_snap_words >= 0, "negative count");
  const int64_t cols_pad = ococc_align_up((int64_t)max_frame_gt, 64), rows_pad = ococc_align_up((int64_t)max_frame_pd, 64);
  const int64_t wave_lds = assign_wave_lds(cols_pad, rows_pad);
  OCOCC_REQUIRE(wave_lds <= kAssignLdsLimit,
                "frame too large for the assignment kernel: 18 B per ground-truth box + 2 B per prediction must fit 64 KiB");
  OCOCC_REQUIRE(host_iou_thresh != nullptr, "null iou thresholds");
  Thresholds thr;
  for (int k = 0; k < 5; ++k) {
    thr.v[k] = host_iou_thresh[k];
    OCOCC_REQUIRE(k == 0 || (thr.v[k] > 0.f && thr.v[k] <= 1.f), "iou thresholds of types 1..4 must lie in (0, 1]");
  }
  const int64_t pairs = pair_end - pair_begin;
  OCOCC_REQUIRE(workspace_bytes >= ococc_frame_match_workspace_bytes(pairs), "workspace too small");
  const int frames = frame_end - frame_begin;
  if (frames == 0 || num_pd == 0) return OCOCC_OK;
  OCOCC_REQUIRE(pd_type && pd_offsets && gt_offsets && pair_offsets && snap_offsets, "null pointer");
  OCOCC_REQUIRE(snapshots || num_snap_words == 0, "null pointer");
  if (pairs > 0) {
    OCOCC_REQUIRE(pd_boxes && pd_eligible && gt_boxes && gt_type && gt_eligible && workspace, "null pointer");
    const int64_t blocks = ococc_cdiv(pairs, (int64_t)kWaves * kWavePairs);
    OCOCC_REQUIRE(blocks <= 0x7fffffffLL, "too many pairs for one launch");
    hipLaunchKernelGGL(frame_overlap_kernel, dim3((unsigned)blocks), dim3(kWaves * 64), 0, (hipStream_t)stream, pd_boxes,
                       pd_type, pd_eligible, pd_offsets, gt_boxes, gt_type, gt_eligible, gt_offsets, pair_offsets,
                       frame_begin, frame_end, pair_begin, pair_end, (float*)workspace);
    OCOCC_CHECK_LAUNCH();
  }
  // as many waves (frames) per workgroup as 64 KiB of LDS hold, at most kWaves
  int waves = kWaves;
  while (waves > 1 && waves * wave_lds > kAssignLdsLimit) waves >>= 1;
  hipLaunchKernelGGL(frame_assign_kernel, dim3((unsigned)ococc_cdiv(frames, waves)), dim3(waves * 64),
                     (size_t)(waves * wave_lds), (hipStream_t)stream, pd_type, pd_offsets, gt_offsets, pair_offsets,
                     frame_begin, frame_end, pair_begin, (const float*)workspace, thr, snap_offsets, num_snap_words,
                     snapshots, (int)cols_pad, (int)rows_pad);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}
