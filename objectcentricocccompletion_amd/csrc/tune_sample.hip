// The observation sample that tunes the shape latent of ONE online step: per RoI, the observed cells of its
// dense grid plus as many free cells, drawn with a counter-based integer generator (tune_rng.hpp), capped, as rows
// (cell centre, label, RoI, weight = 1 / rows of the RoI).  Stands behind occ_ops.tune_sample and the ``tune=`` argument
// of OccBBoxHead.forward_step / forward_steps; replaces, for the step, OccAutoEncoder.sample_observation with
// balance_sample (mmdet3d/models/roi_heads/bbox_heads/occ_ae_head.py:65-201: float64 keys over every cell, two stable
// argsorts, three nonzero read-backs).  The flat cell list is that of occ_export.hip / occ_frame.hip and ``observed`` is
// what ococc_occ_frame_mark wrote: there is no second rasteriser.
//
// One workgroup per RoI, two launches, the per-RoI counts read back in between:
//   count : npos from ballots; the case of the table below; where q of the free cells are drawn, the q-th smallest
//           (key, cell) by a radix select over 8-bit digits of the 64-bit pair with an LDS histogram (it stops at the first
//           digit whose bucket is taken whole: two or three passes over the RoI's cells at 32-bit keys); the same select
//           over list positions for the cap.  Leaves counts[r] and a plan of 4 x i64 per RoI (mode, repeats, thresholds).
//   fill  : walks the cells in grid order, kBlock at a time: copies per cell, a block scan gives the list position, the
//           cap test per position, a second block scan gives the output row.  Keys are recomputed, never stored.
//
//   keep[r] == 0                 no rows            balance, nneg == 0          no rows
//   balance == 0                 every cell         balance, npos <= nneg       observed + the npos free of smallest key
//   balance, npos == 0           cell 0, label 0    balance, npos > nneg > 0    observed + every free npos / nneg times,
//                                                                               the npos % nneg of smallest key once more
//
// No per-cell LDS array (any grid size below 2^30 cells per RoI), integer atomics in LDS only, no float atomics, vector
// stores only: the same input gives the same bytes.
#include "common.hpp"
#include "occ_tiles.hpp"
#include "tune_rng.hpp"

// the one float quotient below is rounded on its own
#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 1024;
constexpr int kWaves = kBlock / 64;
constexpr int64_t kMaxCells = 1ll << 30;   // per RoI: cells and list positions are 32-bit

enum : int64_t { kModeNone = 0, kModeAll = 1, kModeFirst = 2, kModeBalanced = 3, kModeMask = 3, kFlagExtra = 4,
                 kFlagCapped = 8 };
constexpr int kPlan = 4;   // i64 per RoI: mode | flags, repeats of a free cell, select threshold, cap threshold

struct Scratch {
  uint32_t hist[256];
  uint32_t wave_tot[kWaves];
  uint32_t pick[3];
  unsigned long long sum;
};

// exclusive prefix of v over the block, in thread order; *total the block's sum
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* total, uint32_t* wave_tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(inc, d, 64);
    if (lane >= d) inc += t;
  }
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  uint32_t add = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const uint32_t t = wave_tot[w];
    if (w < wave) add += t;
    tot += t;
  }
  __syncthreads();
  *total = tot;
  return inc - v + add;
}

// The q-th smallest (1 <= q <= candidates) of the 64-bit values cand(i, value) accepts for i in [0, n), as a threshold T:
// exactly q candidates have value <= T.  Values are distinct (their low 32 bits are i).  Block-wide, result uniform.
template <class Cand>
__device__ __forceinline__ uint64_t block_select(uint32_t n, uint32_t q, Cand cand, Scratch& sh) {
  uint64_t prefix = 0;
  uint32_t remaining = q;
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    if (threadIdx.x < 256) sh.hist[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
      uint64_t v;
      if (cand(i, v) && (pass == 0 || (v >> (shift + 8)) == (prefix >> (shift + 8))))
        atomicAdd(&sh.hist[(uint32_t)(v >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 64) {   // wave 0: four buckets per lane, the bucket that holds rank `remaining`
      const int lane = threadIdx.x;
      uint32_t h[4], s = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { h[j] = sh.hist[lane * 4 + j]; s += h[j]; }
      uint32_t inc = s;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
      }
      const unsigned long long bal = __ballot(inc >= remaining);
      if (bal == 0ull) {   // (q beyond the candidates: unreachable from the kernels below; everything is taken)
        if (lane == 0) { sh.pick[0] = 255u; sh.pick[1] = 0u; sh.pick[2] = remaining; }
      } else if (lane == __ffsll((long long)bal) - 1) {
        uint32_t before = inc - s;
        int j = 0;
        while (j < 3 && before + h[j] < remaining) { before += h[j]; ++j; }
        sh.pick[0] = (uint32_t)(lane * 4 + j); sh.pick[1] = before; sh.pick[2] = h[j];
      }
    }
    __syncthreads();
    const uint32_t bucket = sh.pick[0], before = sh.pick[1], inside = sh.pick[2];
    remaining -= before;
    prefix |= (uint64_t)bucket << shift;
    if (inside == remaining) return prefix | ((1ull << shift) - 1ull);   // the whole bucket is taken
  }
  return prefix;
}

// the cells of RoI r in the flat list, or false: start is no ascending table inside [0, n], or the RoI is too large
__device__ __forceinline__ bool roi_range(const int64_t* start, int r, int64_t n, int64_t& s0, uint32_t& k) {
  s0 = start[r];
  const int64_t s1 = start[r + 1];
  k = 0;
  if (s0 < 0 || s1 < s0 || s1 > n || s1 - s0 > kMaxCells) return false;
  k = (uint32_t)(s1 - s0);
  return true;
}

__global__ void __launch_bounds__(kBlock)
tune_sample_count_kernel(const uint8_t* __restrict__ observed, int64_t n, const int64_t* __restrict__ start,
                         const int64_t* __restrict__ row_seeds, const uint8_t* __restrict__ row_keep, int balance, int cap,
                         int32_t* __restrict__ counts, int64_t* __restrict__ plan) {
  __shared__ Scratch sh;
  const int r = blockIdx.x;
  int64_t s0;
  uint32_t k;
  const bool ok = roi_range(start, r, n, s0, k);
  int64_t mode = kModeNone, rep = 0;
  uint64_t t_sel = 0, t_cap = ~0ull;
  int32_t m = ok ? 0 : -1;   // -1: the host reports the table
  if (ok && k > 0 && (row_keep == nullptr || row_keep[r] != 0)) {
    if (!balance) {
      mode = kModeAll, m = (int32_t)k;
    } else {
      const uint64_t seed = (uint64_t)row_seeds[r];
      const uint8_t* obs = observed + s0;
      if (threadIdx.x == 0) sh.sum = 0ull;
      __syncthreads();
      uint32_t mine = 0;   // wave-uniform
      for (uint32_t c0 = 0; c0 < k; c0 += kBlock) {
        const uint32_t c = c0 + threadIdx.x;
        mine += (uint32_t)__popcll(__ballot(c < k && obs[c] != 0));
      }
      if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&sh.sum, (unsigned long long)mine);
      __syncthreads();
      const uint32_t npos = (uint32_t)sh.sum, nneg = k - npos;
      if (npos == 0) {
        mode = kModeFirst, m = 1;
      } else if (nneg > 0) {
        mode = kModeBalanced;
        const uint32_t q = npos <= nneg ? npos : npos % nneg;
        rep = npos <= nneg ? 0 : npos / nneg;
        if (q > 0) {
          mode |= kFlagExtra;
          t_sel = q >= nneg ? ~0ull : block_select(k, q, [&](uint32_t c, uint64_t& v) {
            v = tune_select_key(seed, c);
            return obs[c] == 0;
          }, sh);
        }
        const uint32_t m_pre = 2u * npos;   // npos observed + nneg * rep + q free = 2 npos rows
        m = (int32_t)m_pre;
        if (cap > 0 && m_pre > (uint32_t)cap) {
          mode |= kFlagCapped, m = cap;
          t_cap = block_select(m_pre, (uint32_t)cap, [&](uint32_t p, uint64_t& v) {
            v = tune_cap_key(seed, p);
            return true;
          }, sh);
        }
      }
    }
  }
  if (threadIdx.x == 0) {
    counts[r] = m;
    int64_t* p = plan + (int64_t)r * kPlan;
    p[0] = mode, p[1] = rep, p[2] = (int64_t)t_sel, p[3] = (int64_t)t_cap;
  }
}

__global__ void __launch_bounds__(kBlock)
tune_sample_fill_kernel(const uint8_t* __restrict__ observed, int64_t n, const int64_t* __restrict__ start,
                        const float* __restrict__ sizes, const int32_t* __restrict__ dims, float voxel_size,
                        const int64_t* __restrict__ row_seeds, const int32_t* __restrict__ counts,
                        const int64_t* __restrict__ plan, float* __restrict__ xyz, int32_t* __restrict__ labels,
                        int32_t* __restrict__ index, float* __restrict__ weights, int64_t S) {
  __shared__ Scratch sh;
  const int r = blockIdx.x;
  const int32_t m = counts[r];
  int64_t s0;
  uint32_t k;
  if (m <= 0 || !roi_range(start, r, n, s0, k) || k == 0) return;
  // the RoI's first row: the counts in front of it
  if (threadIdx.x == 0) sh.sum = 0ull;
  __syncthreads();
  unsigned long long part = 0;
  for (int j = threadIdx.x; j < r; j += kBlock) part += (unsigned long long)max(counts[j], 0);
  if (part) atomicAdd(&sh.sum, part);
  __syncthreads();
  const int64_t base = (int64_t)sh.sum;
  const int64_t* p = plan + (int64_t)r * kPlan;
  const int64_t mode = p[0] & kModeMask;
  const bool extra = (p[0] & kFlagExtra) != 0, capped = (p[0] & kFlagCapped) != 0;
  const uint32_t rep = (uint32_t)p[1];
  const uint64_t t_sel = (uint64_t)p[2], t_cap = (uint64_t)p[3];
  const uint64_t seed = (uint64_t)row_seeds[r];
  const float w = __fdiv_rn(1.0f, (float)m);
  const float* size = sizes + (int64_t)r * 3;
  const int32_t* dim = dims + (int64_t)r * 3;
  const uint8_t* obs = observed + s0;

  auto emit = [&](int64_t row, uint32_t c, int label) {
    if (row >= S || row >= base + m) return;   // (always false when count and fill saw the same input)
    const Cell ctr = cell_centre(c, size, dim, voxel_size);
    xyz[row * 3 + 0] = ctr.x, xyz[row * 3 + 1] = ctr.y, xyz[row * 3 + 2] = ctr.z;
    labels[row] = label, index[row] = r, weights[row] = w;
  };
  if (mode == kModeFirst) {
    if (threadIdx.x == 0) emit(base, 0u, 0);
    return;
  }
  if (mode == kModeNone) return;
  uint32_t run_pre = 0, run_out = 0;   // list positions and rows in front of this pass
  for (uint32_t c0 = 0; c0 < k && run_out < (uint32_t)m; c0 += kBlock) {
    const uint32_t c = c0 + threadIdx.x;
    const bool valid = c < k;
    const bool seen = valid && obs[c] != 0;
    uint32_t mult = 0;
    if (valid) mult = (mode == kModeAll || seen) ? 1u : rep + ((extra && tune_select_key(seed, c) <= t_sel) ? 1u : 0u);
    uint32_t tot_pre, tot_out;
    const uint32_t p0 = run_pre + block_exclusive_scan(mult, &tot_pre, sh.wave_tot);
    uint32_t kept = mult;
    if (capped) {
      kept = 0;
      for (uint32_t j = 0; j < mult; ++j) kept += tune_cap_key(seed, p0 + j) <= t_cap ? 1u : 0u;
    }
    int64_t row = base + run_out + block_exclusive_scan(kept, &tot_out, sh.wave_tot);
    if (kept) {
      for (uint32_t j = 0; j < mult; ++j)
        if (!capped || tune_cap_key(seed, p0 + j) <= t_cap) emit(row++, c, seen ? 1 : 0);
    }
    run_pre += tot_pre, run_out += tot_out;
  }
}

}  // namespace

extern "C" int ococc_tune_sample_count(const uint8_t* observed, int64_t n, const int64_t* start, int32_t K,
                                       const int64_t* row_seeds, const uint8_t* row_keep, int32_t balance, int32_t cap,
                                       int32_t* counts, int64_t* plan, ococc_stream_t stream) {
  OCOCC_REQUIRE(n >= 0 && K >= 0, "n < 0 or K < 0");
  OCOCC_REQUIRE(balance != 0 || cap <= 0, "cap > 0 with balance == 0: the weighted draw is not built on kernels");
  if (K == 0) return OCOCC_OK;
  OCOCC_REQUIRE(start && counts && plan, "null pointer: start, counts or plan");
  OCOCC_REQUIRE(balance == 0 || row_seeds, "null pointer: row_seeds [K] of the balanced draw");
  OCOCC_REQUIRE(n == 0 || balance == 0 || observed, "null pointer: observed (ococc_occ_frame_mark writes it)");
  hipLaunchKernelGGL(tune_sample_count_kernel, dim3(K), dim3(kBlock), 0, (hipStream_t)stream, observed, n, start,
                     row_seeds, row_keep, (int)balance, (int)cap, counts, plan);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}

extern "C" int ococc_tune_sample_fill(const uint8_t* observed, int64_t n, const int64_t* start, int32_t K,
                                      const float* sizes, const int32_t* dims, float voxel_size, const int64_t* row_seeds,
                                      const int32_t* counts, const int64_t* plan, float* xyz, int32_t* labels,
                                      int32_t* index, float* weights, int64_t S, ococc_stream_t stream) {
  OCOCC_REQUIRE(n >= 0 && K >= 0 && S >= 0, "n < 0, K < 0 or S < 0");
  OCOCC_REQUIRE(voxel_size > 0.f, "voxel_size <= 0");
  if (K == 0 || S == 0 || n == 0) return OCOCC_OK;
  OCOCC_REQUIRE(observed && start && sizes && dims && row_seeds && counts && plan, "null pointer");
  OCOCC_REQUIRE(xyz && labels && index && weights, "null pointer: xyz, labels, index or weights");
  hipLaunchKernelGGL(tune_sample_fill_kernel, dim3(K), dim3(kBlock), 0, (hipStream_t)stream, observed, n, start, sizes,
                     dims, voxel_size, row_seeds, counts, plan, xyz, labels, index, weights, S);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}
