// The seeded 64-bit n-gram fingerprint of the overlap and repeat units (batch_overlap.hip,
// batch_repeat.hip; include/shredword_encode.h defines it in the overlap section), and the two wave
// reductions their kernels share.
// Included by .hip files only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "draw_hash.h"

namespace shred {
namespace {

constexpr uint64_t kOvFree = ~0ull;  // a free slot's key: no fingerprint takes it

// The definition's pieces, for the kernels, the host and the asserts below.
constexpr __host__ __device__ uint64_t ov_g(uint64_t seed, int32_t id) {
  return draw(seed, (uint64_t)(uint32_t)id, kNgram);
}
constexpr __host__ __device__ uint64_t ov_mult(uint64_t seed, uint64_t w) { return draw(seed, w, kMult) | 1; }
constexpr __host__ __device__ uint64_t ov_print(uint64_t S) {
  const uint64_t f = fmix64(S);
  return f == kOvFree ? kOvFree - 1 : f;
}
// Values of the definition as the tests' numpy reference computes it, under seed 3: the 1-gram [7], the
// multiplier of 13-grams, and the 3-gram [7, -1, 5].
constexpr uint64_t ov_three(uint64_t seed, int32_t a, int32_t b, int32_t c) {
  return ov_print((ov_g(seed, a) * ov_mult(seed, 3) + ov_g(seed, b)) * ov_mult(seed, 3) + ov_g(seed, c));
}
static_assert(ov_print(ov_g(3, 7)) == 0xcafcf3efc9b725e1ull && ov_mult(3, 13) == 0x5c864b2e1a922f5full, "overlap");
static_assert(ov_three(3, 7, -1, 5) == 0xfe2c613d41db9357ull, "overlap");

// A^w, the factor of the id that leaves a rolling fingerprint.
[[maybe_unused]] inline uint64_t ov_power(uint64_t a, int w) {
  uint64_t r = 1;
  for (int i = 0; i < w; ++i) r *= a;
  return r;
}

__device__ __forceinline__ uint64_t ov_sum(uint64_t v) {
  for (int d = 32; d; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d);
  return v;
}
[[maybe_unused]] __device__ __forceinline__ uint64_t ov_min(uint64_t v) {
  for (int d = 32; d; d >>= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, d);
    v = o < v ? o : v;
  }
  return v;
}

}  // namespace
}  // namespace shred
