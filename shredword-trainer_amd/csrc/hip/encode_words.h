// The word walk of the encoder kernels (encode_device.hip) and of the special-token scan
// (encode_special.hip): one workgroup per 4096-byte chunk, one thread per 32-byte span, a word
// belongs to the span it starts in; the span passes (encode_spans.hip) share the geometry and the
// block scan; the long-word pass (encode_long.hip) shares the walk and the rank lookup.  Device code;
// included by those .hip files only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../host/encoder.h"

namespace shred {
namespace {

constexpr int kThreads = 128;              // threads per workgroup
constexpr int kSpan = 32;                  // bytes whose word starts one thread owns
constexpr int kChunk = kThreads * kSpan;   // bytes per workgroup

__device__ __forceinline__ uint32_t is_delim(uint32_t c) { return c == 9u || c == 13u || c == 10u || c == 32u; }

// In-place inclusive scan of s_inc[0 .. kThreads), of which every thread has just written its own
// entry (the first barrier orders those stores).
__device__ __forceinline__ void block_inclusive_scan(uint32_t* s_inc, int tid) {
  __syncthreads();
  for (int d = 1; d < kThreads; d <<= 1) {
    const uint32_t v = tid >= d ? s_inc[tid - d] : 0;
    __syncthreads();
    s_inc[tid] += v;
    __syncthreads();
  }
}

// The first thread whose scanned count (s_inc[t] & mask) exceeds i; i is below the last count.
__device__ __forceinline__ int first_above(const uint32_t* s_inc, uint32_t i, uint32_t mask) {
  int lo = 0, hi = kThreads - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((s_inc[mid] & mask) > i) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// The chunk's text staged in LDS (coalesced 4-byte loads), with a few bytes before it and
// kOverhang after: word scans, hashes and compares read LDS, and global memory only for bytes
// outside the staged window.
constexpr int kOverhang = 256;
constexpr int kStageBytes = 4 + kChunk + kOverhang;

struct TextView {
  const uint8_t* __restrict__ g;
  const uint8_t* l;  // LDS copy of [lo, hi)
  uint64_t lo, hi;
  __device__ __forceinline__ uint32_t operator[](uint64_t i) const { return (i >= lo && i < hi) ? l[i - lo] : g[i]; }
};

__device__ __forceinline__ TextView stage_chunk(const uint8_t* __restrict__ text, uint64_t n, uint64_t chunk,
                                                uint32_t* lds) {
  const uint64_t cbase = chunk * kChunk;
  const uint64_t lo = cbase >= 4 ? cbase - 4 : 0;
  uint64_t hi = lo + kStageBytes;
  if (hi > n) hi = n;
  const uint64_t words = (hi - lo) / 4;
  for (uint64_t w = threadIdx.x; w < words; w += kThreads) {
    const uint8_t* p = text + lo + 4 * w;  // lo is 4-aligned; the text base may not be
    lds[w] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
  }
  __syncthreads();
  return TextView{text, reinterpret_cast<const uint8_t*>(lds), lo, lo + 4 * words};
}

// Rank of the pair (a, b) in the merge-rank table (host/encoder.h), kInf for none.
constexpr int kInf = 0x7fffffff;
__device__ __forceinline__ int pair_rank(const uint64_t* __restrict__ tab, uint64_t mask, int a, int b) {
  if ((uint32_t)a >= (uint32_t)kEncIdLimit || (uint32_t)b >= (uint32_t)kEncIdLimit) return kInf;
  const uint64_t key = (uint64_t)(uint32_t)a << 20 | (uint64_t)(uint32_t)b;
  for (uint64_t i = ((key * 0x9E3779B97F4A7C15ull) >> 24) & mask;; i = (i + 1) & mask) {
    const uint64_t e = tab[i];
    if (e == kEncEmpty) return kInf;
    if ((e >> 20) == key) return (int)(e & 0xFFFFFu);
  }
}

// 0x80 in every byte of w that equals c.
__device__ __forceinline__ uint64_t bytes_equal(uint64_t w, uint64_t c) {
  const uint64_t x = w ^ (c * 0x0101010101010101ull);
  return ~(((x & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | x | 0x7F7F7F7F7F7F7F7Full);
}

// The first delimiter of text[e .. stop), or stop (<= n): the tail of a word longer than the byte
// walk below follows, read 8 bytes at a time once the address is aligned.
__device__ __forceinline__ uint64_t long_word_end(const uint8_t* __restrict__ text, uint64_t e, uint64_t stop) {
  while (e < stop && (reinterpret_cast<uintptr_t>(text + e) & 7)) {
    if (is_delim(text[e])) return e;
    ++e;
  }
  while (e + 8 <= stop) {
    const uint64_t w = *reinterpret_cast<const uint64_t*>(text + e);
    if (bytes_equal(w, 9) | bytes_equal(w, 10) | bytes_equal(w, 13) | bytes_equal(w, 32)) break;
    e += 8;
  }
  while (e < stop && !is_delim(text[e])) ++e;
  return e;
}

// Calls f(s, L, j) for every word starting in the span at `base` (L may exceed kEncMaxWord: it is
// then kEncMaxWord + 1, or with the text's global pointer g and a limit maxw above kEncMaxWord the
// word's length up to maxw + 1).
template <typename T, typename F>
__device__ __forceinline__ void for_each_word(const T& text, uint64_t n, uint64_t base, F f,
                                              const uint8_t* __restrict__ g = nullptr,
                                              uint64_t maxw = (uint64_t)kEncMaxWord) {
  if (base >= n) return;
  const uint64_t lim = n - base < (uint64_t)kSpan ? n - base : (uint64_t)kSpan;
  uint32_t dm = 0;
  for (int k = 0; k < kSpan; ++k) dm |= ((uint64_t)k < lim ? is_delim(text[base + k]) : 1u) << k;
  const uint32_t prevd = base == 0 ? 1u : is_delim(text[base - 1]);
  uint32_t starts = ~dm & ((dm << 1) | prevd);
  while (starts) {
    const int j = __ffs(starts) - 1;
    starts &= starts - 1;
    const uint64_t s = base + j;
    const uint32_t above = dm >> j;
    uint64_t L;
    if (above) {
      L = __ffs(above) - 1;
    } else {
      uint64_t e = base + kSpan;
      while (e < n && e - s <= (uint64_t)kEncMaxWord && !is_delim(text[e])) ++e;
      if (g && e - s > (uint64_t)kEncMaxWord) e = long_word_end(g, e, n - s > maxw + 1 ? s + maxw + 1 : n);
      L = e - s;
    }
    f(s, L, j);
  }
}

}  // namespace
}  // namespace shred
