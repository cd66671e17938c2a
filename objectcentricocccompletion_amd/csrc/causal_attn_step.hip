// A9, online  one frame of the temporal transformer's attention against cached keys and values.
//
// Reference: the same block as csrc/causal_attn.hip (SimpleEncoderLayer.forward -> nn.MultiheadAttention,
// mmdet3d/models/occ/layers.py:35-87, under the causal mask of OccBBoxHead.get_future_mask, ococc_bbox_head.py:1034-1043,
// optionally windowed by test_cfg.attn_window_size).  Under that mask row t of the full product reads keys lo..t only, so
// a tracklet that arrives frame by frame needs one query row per frame against the keys and values of the frames before it.
// Here: one workgroup per (row, head).  It appends the row's new key and value to its head's column slice of cache row
// (slot, pos[slot]) and computes  softmax(scale q . K[lo..t]) V[lo..t]  with the new key and value taken from LDS, the
// cached ones straight from global memory into registers with float4 loads (a memory-bound read of at most 2 * 256 * D
// floats: no LDS staging of K / V, no split of the keys across workgroups).  Scores: 16 lanes per key, kSK = 16 keys per pass
// of the workgroup; the softmax over <= 256 scores by wave butterflies; the product with V with the keys dealt round-robin to
// the 16 lane groups and the 16 partial rows summed in a fixed order.  f32 throughout, no atomics, no dropout (inference only).
// The kernel does not advance pos: every encoder layer has a cache of its own and shares pos, the caller bumps it once.
//
// Two instances of ONE kernel template, so the arithmetic lives in one place:
//   ococc_temporal_attention_step_f32       kMaxS = 256: one score per thread, frame f in cache row f, a slot is full at cap.
//   ococc_temporal_attention_step_long_f32  kMaxS = 4096 (kLongMaxS): the scores stay in LDS (16 KB) and a thread owns the
//     scores tid, tid + 256, ...; it takes their maximum and their sum locally before the wave butterflies, so for <= 256
//     keys it does operation for operation what the first instance does.  ``ring``: frame f lives in cache row f % cap, the
//     new frame t overwrites frame t - cap, which a window <= cap no longer reads -- a windowed model follows a tracklet of
//     any length (pos up to 2^31 - 1) in ``window`` rows per slot.  Without ``ring`` a model that attends to all history
//     gets up to 4096 cached frames.  A workgroup still reads and writes only its own head's column slice.
//
// Several frames per slot in one call (ococc_temporal_attention_chunk_f32): the ``kChunk`` mode of the same body, one
// instance per kMaxS.  Row i is frame t = pos[slot] + off[i] of its slot, the rows of a slot consecutive and in frame order.
// The keys and values of the frames < pos[slot] come from the cache, those of the frames pos[slot]..t from the call's own
// rows k_new / v_new[i - off[i] + (f - pos[slot])]; the sums run over the keys lo..t in the order of the step kernel, so a
// chunk gives bit for bit what the single steps give.  This mode never writes the cache and never reads a cache row at or
// past pos[slot]: in a ring the row frame t will occupy may still hold a frame that an earlier row of the same chunk reads
// (any chunk longer than cap - window), so no workgroup may depend on another's write.  The new rows are appended by a
// second small kernel on the same stream (append_chunk_kernel) once every attention workgroup is done; of the frames of
// one slot that fall into the same ring row (a run longer than cap) only the last is written.
#include "common.hpp"

#include <type_traits>

namespace {

constexpr int kST = 256;      // threads per workgroup
constexpr int kSK = 16;       // keys per pass (16 lanes each)
constexpr int kSMaxS = 256;   // cache rows per slot at most (kAMaxS of causal_attn.hip)
constexpr int kLongMaxS = 4096;   // ... of the long instance: 16 KB of scores in LDS, 46 KB in all
constexpr int kSNJ = 6;       // float4 column groups per thread: D <= 16 * 4 * kSNJ = 384 (kANJ of causal_attn.hip)
constexpr int kSMaxD = 64 * kSNJ;

struct StepArgs {
  const float* q;
  const float* k_new;
  const float* v_new;
  int64_t ldq, ldk, ldv;
  const int32_t* slot;   // [n]
  const int32_t* pos;    // [slots]
  float* k_cache;        // [slots, cap, H * D]
  float* v_cache;
  int32_t n, slots, cap, H, D;
  float scale;
  int32_t window;
  int32_t ring;          // long instance only: frame f in cache row f % cap
  float* out;
  int64_t ldo;
};
struct ChunkArgs : StepArgs {   // (a type of its own: the kernel arguments of the step instances stay as they are)
  const int32_t* off;           // [n] the row's place in its slot's run: row i - off[i] is the run's first
  int32_t max_keys;             // append_chunk_kernel: kMaxS of the attention instance, whose guards it repeats
};

// chunk mode: the frame of row i, t = pos[s] + off[i] of slot s, p = pos[s], ``first`` the first row of the slot's run.
// false: the row is skipped (a host bug must not read or write outside the call's rows or the cache).
__device__ __forceinline__ bool chunk_frame(const ChunkArgs& a, int i, int& s, int& p, int& first, int& t) {
  s = a.slot[i];
  if (s < 0 || s >= a.slots) return false;
  const int o = a.off[i];
  if (o < 0 || o > i) return false;
  first = i - o;
  if (a.slot[first] != s) return false;
  p = a.pos[s];
  if (p < 0 || o > 0x7fffffff - p) return false;
  t = p + o;
  return true;
}

__device__ __forceinline__ float dot4(const f32x4 a, const f32x4 b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }
__device__ __forceinline__ float sum16(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  return v;
}

template <int kMaxS, bool kChunk = false>
__global__ void __launch_bounds__(kST) attn_step_kernel(std::conditional_t<kChunk, ChunkArgs, StepArgs> a) {
  constexpr bool kLong = kMaxS > kST;   // several scores per thread, ring addressing
  __shared__ __attribute__((aligned(16))) float sq[kSMaxD];          // the query row, scaled
  __shared__ __attribute__((aligned(16))) float sk[kSMaxD];          // the new key
  __shared__ __attribute__((aligned(16))) float sv[kSMaxD];          // the new value
  __shared__ float ss[kMaxS];                                        // scores -> probabilities of keys lo .. t
  __shared__ float red[2 * (kST / 64)];
  __shared__ __attribute__((aligned(16))) float part[kSK * kSMaxD];  // the 16 partial context rows
  const int i = blockIdx.x, h = blockIdx.y;
  int cs = 0, ct = 0, p = 0, first = 0;   // chunk mode: p = pos[s] frames are cached, row ``first`` is frame p
  if constexpr (kChunk)
    if (!chunk_frame(a, i, cs, p, first, ct)) return;
  const int s = kChunk ? cs : a.slot[i];
  if (s < 0 || s >= a.slots) return;   // (the host checks both; a host bug must not write outside the cache)
  const int t = kChunk ? ct : a.pos[s];
  const bool ring = kLong && a.ring != 0;
  if (t < 0 || (!ring && t >= a.cap)) return;
  const int lo = a.window > 0 && t - a.window + 1 > 0 ? t - a.window + 1 : 0;
  const int nk = t - lo + 1;           // keys lo .. t, the last one the new one
  if (nk > a.cap || nk > kMaxS) return;   // (ring: window <= cap, checked by the host)
  const int trow = ring ? t % a.cap : t;      // the cache row of frame t
  const int row0 = ring ? lo % a.cap : lo;    // ... of frame lo; frame lo + j: row0 + j, wrapped once (j < nk <= cap)
  const int D4 = a.D >> 2, col0 = h * a.D;
  const int64_t ldc = (int64_t)a.H * a.D;
  float* kc = a.k_cache + (int64_t)s * a.cap * ldc + col0;
  float* vc = a.v_cache + (int64_t)s * a.cap * ldc + col0;
  const int tid = threadIdx.x, r = tid >> 4, c0 = tid & 15;

  if (tid < D4) {   // append: this head's slice of cache row t, and the LDS copies the sums below read
    const f32x4 qv = *(const f32x4*)(a.q + (int64_t)i * a.ldq + col0 + tid * 4);
    const f32x4 kv = *(const f32x4*)(a.k_new + (int64_t)i * a.ldk + col0 + tid * 4);
    const f32x4 vv = *(const f32x4*)(a.v_new + (int64_t)i * a.ldv + col0 + tid * 4);
    *(f32x4*)(sq + tid * 4) = qv * a.scale;
    *(f32x4*)(sk + tid * 4) = kv;
    *(f32x4*)(sv + tid * 4) = vv;
    if constexpr (!kChunk) {   // (chunk mode: append_chunk_kernel, afterwards)
      *(f32x4*)(kc + (int64_t)trow * ldc + tid * 4) = kv;
      *(f32x4*)(vc + (int64_t)trow * ldc + tid * 4) = vv;
    }
  }
  __syncthreads();

  // scores: lane group r takes key j0 + r of every pass, its 16 lanes the float4 columns c0, c0 + 16, ...
  for (int j0 = 0; j0 < nk; j0 += kSK) {
    const int j = j0 + r;
    float acc = 0.f;
    if (j < nk) {
      if (j == nk - 1) {
        for (int c4 = c0; c4 < D4; c4 += 16) acc += dot4(*(const f32x4*)(sq + c4 * 4), *(const f32x4*)(sk + c4 * 4));
      } else {
        int row = row0 + j;
        if (ring && row >= a.cap) row -= a.cap;
        const float* krow = kc + (int64_t)row * ldc;
        if constexpr (kChunk)   // a frame of this call: its own row, not the cache
          if (lo + j >= p) krow = a.k_new + (int64_t)(first + (lo + j - p)) * a.ldk + col0;
        for (int c4 = c0; c4 < D4; c4 += 16) acc += dot4(*(const f32x4*)(sq + c4 * 4), *(const f32x4*)(krow + c4 * 4));
      }
    }
    acc = sum16(acc);
    if (j < nk && c0 == 0) ss[j] = acc;
  }
  __syncthreads();

  {   // softmax over the nk scores: thread tid owns the scores tid, tid + 256, ... (one when nk <= 256)
    const int lane = tid & 63, wave = tid >> 6;
    const float x = tid < nk ? ss[tid] : -INFINITY;
    float m = x;
    if constexpr (kLong)
      for (int j = tid + kST; j < nk; j += kST) m = fmaxf(m, ss[j]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float e = tid < nk ? __expf(x - m) : 0.f;
    float sum = e;
    if constexpr (kLong)
      for (int j = tid + kST; j < nk; j += kST) {
        const float ej = __expf(ss[j] - m);
        ss[j] = ej;
        sum += ej;
      }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    const float inv = 1.f / ((red[4] + red[5]) + (red[6] + red[7]));
    if (tid < nk) ss[tid] = e * inv;
    if constexpr (kLong)
      for (int j = tid + kST; j < nk; j += kST) ss[j] *= inv;
  }
  __syncthreads();

  // context: lane group r sums the keys j = r, r + 16, ... in turn; then the 16 partial rows in a fixed order
  f32x4 o[kSNJ];
#pragma unroll
  for (int jj = 0; jj < kSNJ; ++jj) o[jj] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int j = r; j < nk; j += kSK) {
    const float w = ss[j];
    if (j == nk - 1) {
#pragma unroll
      for (int jj = 0; jj < kSNJ; ++jj) {
        const int c4 = c0 + 16 * jj;
        if (c4 < D4) o[jj] += *(const f32x4*)(sv + c4 * 4) * w;
      }
    } else {
      int row = row0 + j;
      if (ring && row >= a.cap) row -= a.cap;
      const float* vrow = vc + (int64_t)row * ldc;
      if constexpr (kChunk)
        if (lo + j >= p) vrow = a.v_new + (int64_t)(first + (lo + j - p)) * a.ldv + col0;
#pragma unroll
      for (int jj = 0; jj < kSNJ; ++jj) {
        const int c4 = c0 + 16 * jj;
        if (c4 < D4) o[jj] += *(const f32x4*)(vrow + c4 * 4) * w;
      }
    }
  }
#pragma unroll
  for (int jj = 0; jj < kSNJ; ++jj) {
    const int c4 = c0 + 16 * jj;
    if (c4 < D4) *(f32x4*)(part + r * kSMaxD + c4 * 4) = o[jj];
  }
  __syncthreads();
  if (tid < D4) {
    f32x4 acc = *(const f32x4*)(part + tid * 4);
#pragma unroll
    for (int g = 1; g < kSK; ++g) acc += *(const f32x4*)(part + g * kSMaxD + tid * 4);
    *(f32x4*)(a.out + (int64_t)i * a.ldo + col0 + tid * 4) = acc;
  }
}

// after the chunk instance of attn_step_kernel on the same stream: one workgroup per row copies the row's new key and
// value (all heads) to the cache row of its frame.  The guards are those of the attention kernel: a row it skipped is
// not appended.  Ring, run longer than cap: row i + cap of the same run is frame t + cap, which lands in the same cache
// row -- row i is superseded and stays unwritten, as if the frames had been written in order.
__global__ void __launch_bounds__(kST) append_chunk_kernel(ChunkArgs a) {
  const int i = blockIdx.x;
  int s, t, p, first;
  if (!chunk_frame(a, i, s, p, first, t)) return;
  const bool ring = a.ring != 0;
  if (!ring && t >= a.cap) return;
  const int lo = a.window > 0 && t - a.window + 1 > 0 ? t - a.window + 1 : 0;
  const int nk = t - lo + 1;
  if (nk > a.cap || nk > a.max_keys) return;
  if (ring && (int64_t)i + a.cap < a.n && a.slot[i + a.cap] == s) return;
  const int trow = ring ? t % a.cap : t;
  const int64_t ldc = (int64_t)a.H * a.D;
  const int E4 = (a.H * a.D) >> 2;
  float* kc = a.k_cache + ((int64_t)s * a.cap + trow) * ldc;
  float* vc = a.v_cache + ((int64_t)s * a.cap + trow) * ldc;
  const float* kn = a.k_new + (int64_t)i * a.ldk;
  const float* vn = a.v_new + (int64_t)i * a.ldv;
  for (int c4 = threadIdx.x; c4 < E4; c4 += kST) {
    *(f32x4*)(kc + c4 * 4) = *(const f32x4*)(kn + c4 * 4);
    *(f32x4*)(vc + c4 * 4) = *(const f32x4*)(vn + c4 * 4);
  }
}

// the launches behind the exports (their checks come first: nothing is dereferenced or launched before they pass)
template <int kMaxS>
int launch_step(const StepArgs& a, ococc_stream_t stream_) {
  hipLaunchKernelGGL(attn_step_kernel<kMaxS>, dim3(a.n, a.H), dim3(kST), 0, (hipStream_t)stream_, a);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}

template <int kMaxS>
int launch_chunk(const ChunkArgs& a, ococc_stream_t stream_) {
  hipLaunchKernelGGL((attn_step_kernel<kMaxS, true>), dim3(a.n, a.H), dim3(kST), 0, (hipStream_t)stream_, a);
  OCOCC_CHECK_LAUNCH();
  hipLaunchKernelGGL(append_chunk_kernel, dim3(a.n), dim3(kST), 0, (hipStream_t)stream_, a);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}

}  // namespace

// The three exports name their common arguments alike, so what they share is written once over those names.
// OCOCC_STEP_CHECKS(the export's own checks): the checks of all three around the export's own, in the order the messages
// have always come in; an empty call returns OCOCC_OK once the checks on the sizes have passed.
#define OCOCC_STEP_CHECKS(...)                                                                                         \
  OCOCC_REQUIRE(n >= 0 && slots >= 1 && cap >= 1 && H >= 1 && D >= 1, "empty cache or negative row count");            \
  __VA_ARGS__                                                                                                          \
  OCOCC_REQUIRE(H <= 65535, "too many heads");                                                                         \
  if (n == 0) return OCOCC_OK;                                                                                         \
  OCOCC_REQUIRE(q && k_new && v_new && slot && pos && k_cache && v_cache && out, "null pointer");                      \
  OCOCC_REQUIRE(ldq >= (int64_t)H * D && ldk >= (int64_t)H * D && ldv >= (int64_t)H * D && ldo >= (int64_t)H * D,      \
                "row stride under heads * head_dim");                                                                  \
  OCOCC_REQUIRE(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldo % 4 == 0 &&                                        \
                    (((uintptr_t)q | (uintptr_t)k_new | (uintptr_t)v_new | (uintptr_t)k_cache | (uintptr_t)v_cache |   \
                      (uintptr_t)out) & 15) == 0,                                                                      \
                "rows must be 16-byte aligned")
#define OCOCC_REQUIRE_LONG_CACHE()                                                                                  \
  OCOCC_REQUIRE(cap <= kLongMaxS, "caches of up to 4096 frames per slot");                                             \
  OCOCC_REQUIRE(ring == 0 || (window >= 1 && window <= cap),                                                           \
                "a ring cache needs a window of 1 .. cap frames (the row of frame t overwrites frame t - cap)")
// the StepArgs of an export's arguments, in the order of the struct's fields
#define OCOCC_STEP_ARGS(ring_)                                                                                         \
  StepArgs { q, k_new, v_new, ldq, ldk, ldv, slot, pos, k_cache, v_cache, n, slots, cap, H, D, scale, window, (ring_), out, ldo }

extern "C" int ococc_temporal_attention_step_f32(const float* q, int64_t ldq, const float* k_new, int64_t ldk,
                                                 const float* v_new, int64_t ldv, const int32_t* slot, const int32_t* pos,
                                                 float* k_cache, float* v_cache, int32_t n, int32_t slots, int32_t cap,
                                                 int32_t H, int32_t D, float scale, int32_t window, float* out, int64_t ldo,
                                                 ococc_stream_t stream_) {
  OCOCC_STEP_CHECKS(
      OCOCC_REQUIRE(n <= slots, "more rows than cache slots (the slots of one step are distinct)");
      OCOCC_REQUIRE(cap <= kSMaxS && D <= kSMaxD && D % 4 == 0,
                    "caches of up to 256 frames per slot, head width a multiple of 4 up to 384"););
  return launch_step<kSMaxS>(OCOCC_STEP_ARGS(0), stream_);
}

extern "C" int ococc_temporal_attention_step_long_f32(const float* q, int64_t ldq, const float* k_new, int64_t ldk,
                                                      const float* v_new, int64_t ldv, const int32_t* slot,
                                                      const int32_t* pos, float* k_cache, float* v_cache, int32_t n,
                                                      int32_t slots, int32_t cap, int32_t H, int32_t D, float scale,
                                                      int32_t window, int32_t ring, float* out, int64_t ldo,
                                                      ococc_stream_t stream_) {
  OCOCC_STEP_CHECKS(
      OCOCC_REQUIRE_LONG_CACHE();
      OCOCC_REQUIRE(n <= slots, "more rows than cache slots (the slots of one step are distinct)");
      OCOCC_REQUIRE(D <= kSMaxD && D % 4 == 0, "head width a multiple of 4 up to 384"););
  return launch_step<kLongMaxS>(OCOCC_STEP_ARGS(ring != 0), stream_);
}

extern "C" int ococc_temporal_attention_chunk_f32(const float* q, int64_t ldq, const float* k_new, int64_t ldk,
                                                  const float* v_new, int64_t ldv, const int32_t* slot, const int32_t* off,
                                                  const int32_t* pos, float* k_cache, float* v_cache, int32_t n,
                                                  int32_t slots, int32_t cap, int32_t H, int32_t D, float scale,
                                                  int32_t window, int32_t ring, float* out, int64_t ldo,
                                                  ococc_stream_t stream_) {
  OCOCC_STEP_CHECKS(
      OCOCC_REQUIRE_LONG_CACHE();
      OCOCC_REQUIRE(D <= kSMaxD && D % 4 == 0, "head width a multiple of 4 up to 384"););
  OCOCC_REQUIRE(off, "null pointer");
  const bool small = cap <= kSMaxS && ring == 0;   // one score per thread, as ococc_temporal_attention_step_f32
  const ChunkArgs a{OCOCC_STEP_ARGS(ring != 0), off, small ? kSMaxS : kLongMaxS};
  return small ? launch_chunk<kSMaxS>(a, stream_) : launch_chunk<kLongMaxS>(a, stream_);
}
