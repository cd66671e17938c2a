// The counter-based generator of the tuning sample (tune_sample.hip; restated in occ_ops.tune_sample_aten, heads.py and
// tests/tune_sample_ref.py): integers only, wrapping u64 arithmetic, nothing stored -- a key is recomputed wherever it is
// needed, so a draw depends on (row seed, cell) alone and not on the launch shape.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OCOCC_RNG_FN __host__ __device__ __forceinline__
#else
#define OCOCC_RNG_FN static inline
#endif

constexpr uint64_t kTuneGolden = 0x9E3779B97F4A7C15ull;    // the increment of splitmix64
constexpr uint64_t kTuneCapSalt = 0xD1B54A32D192ED03ull;   // xor-ed into the row seed for the cap draw

// the splitmix64 finaliser
OCOCC_RNG_FN uint64_t tune_mix64(uint64_t x) {
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// key(row_seed, c): the high 32 bits of mix64(row_seed + (c + 1) * golden)
OCOCC_RNG_FN uint32_t tune_key(uint64_t row_seed, uint64_t c) {
  return (uint32_t)(tune_mix64(row_seed + (c + 1) * kTuneGolden) >> 32);
}

// (key, index) as one u64: its integer order IS the lexicographic order, equal keys towards the smaller index
OCOCC_RNG_FN uint64_t tune_select_key(uint64_t row_seed, uint32_t cell) {
  return ((uint64_t)tune_key(row_seed, cell) << 32) | cell;
}
OCOCC_RNG_FN uint64_t tune_cap_key(uint64_t row_seed, uint32_t pos) {
  return ((uint64_t)tune_key(row_seed ^ kTuneCapSalt, pos) << 32) | pos;
}
