// Attention-probability dropout of the SST window-attention kernels (csrc/window_attn.hip, csrc/window_block.hip):
// nn.MultiheadAttention(dropout=p) / CosineMultiheadAttention (mmdet3d/models/sst/sst_basic_block_v2.py:16-35,
// cosine_msa.py:181-182) drop a softmax probability with probability p and scale the kept ones by 1 / (1 - p).
//
// The mask is a counter-based hash: nothing is stored, the backward kernels regenerate it from the same seed.
//   keep(seed, head, q, k) = hash24(seed, head, q, k) >= floor(p * 2^24)
// q, k are the flat token rows of the query and the key (rows of the [V, *] tensors; the padded layout, token_index =
// NULL, uses the padded row w * T + t), so the tile kernels and the per-window gather kernels make the same decision
// for the same pair.  The tuple is folded in one word at a time, each fold a full 32-bit finaliser (murmur3 fmix32) of
// (state ^ word) * golden + c: no linear counter over q * N + k that would wrap around at millions of rows, and
// (q, k) and (k, q) enter in different rounds, so their decisions are independent.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__host__ __device__ __forceinline__ uint32_t ococc_drop_fmix(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
__host__ __device__ __forceinline__ uint32_t ococc_drop_fold(uint32_t state, uint32_t word) {
  return ococc_drop_fmix((state ^ word) * 0x9E3779B1u + 0x7F4A7C15u);
}
// the seed's and the head's part, once per (kernel, head)
__host__ __device__ __forceinline__ uint32_t ococc_drop_head_state(uint64_t seed, uint32_t head) {
  const uint32_t s = ococc_drop_fold(ococc_drop_fmix((uint32_t)seed ^ 0x3C6EF372u), (uint32_t)(seed >> 32));
  return ococc_drop_fold(s, head);
}
// state = ococc_drop_head_state(seed, head); thr = floor(p * 2^24) (0: keep everything)
__host__ __device__ __forceinline__ bool ococc_drop_keep(uint32_t state, uint32_t q_row, uint32_t k_row, uint32_t thr) {
  return (ococc_drop_fold(ococc_drop_fold(state, k_row), q_row) >> 8) >= thr;
}

// host side of the entry points: p in [0, 1) -> threshold and kept-value scale
struct OcoccDrop {
  uint32_t thr;
  float scale;
};
inline OcoccDrop ococc_drop_params(float p) {
  OcoccDrop d;
  d.thr = (uint32_t)(p * 16777216.0);   // (floor: p >= 0; exact in double)
  d.scale = 1.f / (1.f - p);
  return d;
}
