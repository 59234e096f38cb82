// BPE-dropout on gfx950 (C ABI and the definition: include/shredword_encode.h,
// shred_encoder_set_dropout): the direct path of the encoder (encode_device.hip, k_encode_words) with
// some candidate merges dropped.
//
// A word's ids are still "merge the leftmost adjacent pair of lowest rank until no pair has a
// rank"; dropout masks the rank of a dropped candidate to "none" where the rank is looked up, so the
// min-scan loops are those of encode_device.hip.  A candidate (a, b) of rank r whose right token b
// begins at byte position pos is dropped iff
//     mix(mix(seed + 0x9E3779B97F4A7C15 * (pos + 1)) ^ r) >> 32  <  T,   T = (u64)(p * 2^32)
// (mix: murmur3's fmix64): a function of (seed, pos, r) alone, so a boundary that the loop looks at
// again after a neighbouring merge gets the same answer, and the ids do not depend on how the text
// was staged.  The word cache cannot serve this (every occurrence of a word differs), so a dropout
// call always runs here.
//
// The loop has to know where each token begins:
//   words <= 32 bytes  one 32-bit register per thread: bit k is set iff a token begins at byte k of
//                      the word; a merge clears one bit, token j begins at the j-th set bit.  The LDS
//                      strips are those of k_encode_words (16 KB per workgroup packed, 32 KB
//                      unpacked, + 1 KB byte map): no LDS on top.
//   longer words       a third int32 array next to the tokens and ranks in global scratch, indexed
//                      like them by the word's own text offset (words do not overlap); allocated on
//                      the first dropout call, 4 B per text byte of the largest call seen.
// k_encode_words_drop keeps k_encode_words' walk, its per-thread packing at the first word start and
// its counts, so the scan and k_encode_emit behind it are shared.  Words above kEncMaxWord are the
// long pass's (no dropout there) or an error, as on the plain path.
// All global indices are 64-bit; every store is an ordinary vector store.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../host/encoder.h"
#include "encode_common.h"
#include "encode_words.h"

namespace shred {
namespace {

typedef uint64_t u64;

constexpr int kStrip = 32;  // tokens a word keeps in LDS (encode_device.hip)

struct Drop {
  u64 seed, thresh;  // thresh = T in [1, 2^32]
};

__device__ __forceinline__ u64 mix64(u64 x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// pair_rank with the dropped candidates' ranks masked: pos is the position of b's first byte.
__device__ __forceinline__ int drop_rank(const u64* __restrict__ tab, u64 mask, int a, int b, const Drop& d, u64 pos) {
  const int r = pair_rank(tab, mask, a, b);
  if (r == kInf) return kInf;
  const u64 u = mix64(mix64(d.seed + 0x9E3779B97F4A7C15ull * (pos + 1)) ^ (u64)(uint32_t)r);
  return (u >> 32) < d.thresh ? kInf : r;
}

// Where the tokens of a strip word begin, as a bit mask of the word's bytes.
struct BitStarts {
  uint32_t bits;
  __device__ __forceinline__ void init(int L) { bits = L >= 32 ? ~0u : (1u << L) - 1u; }
  // Tokens p and p + 1 have merged into token p: returns where it begins, and in *next where the
  // token now behind it begins (-1: it is the last).
  __device__ __forceinline__ int merged(int p, int m, int* next) {
    uint32_t b = bits;
    for (int i = 0; i < p; ++i) b &= b - 1;
    const int at = __ffs(b) - 1;
    b &= b - 1;          // lowest bit: token p + 1's begin, which goes
    bits &= ~(b & (0u - b));
    b &= b - 1;
    *next = __ffs(b) - 1;
    return at;
  }
};

// The same for a word in global scratch: one entry per token, kept in step with the tokens.
struct ArrayStarts {
  int32_t* at;
  __device__ __forceinline__ void init(int L) {
    for (int k = 0; k < L; ++k) at[k] = k;
  }
  __device__ __forceinline__ int merged(int p, int m, int* next) {  // m: the token count after the merge
    for (int j = p + 1; j < m; ++j) at[j] = at[j + 1];
    *next = p + 1 < m ? at[p + 1] : -1;
    return at[p];
  }
};

// merge_word of encode_device.hip with drop_rank for pair_rank; wpos: the position of the word's
// first byte.
template <typename Tok, typename Starts>
__device__ __forceinline__ int merge_word_drop(Tok tok, Tok rk, int m, const u64* __restrict__ tab, u64 mask,
                                               const Drop& d, u64 wpos, Starts st) {
  st.init(m);
  for (int j = 0; j + 1 < m; ++j) rk(j) = drop_rank(tab, mask, tok(j), tok(j + 1), d, wpos + j + 1);
  while (m > 1) {
    int best = kInf, p = -1;
    for (int j = 0; j + 1 < m; ++j) {
      const int r = rk(j);
      if (r < best) { best = r; p = j; }
    }
    if (best == kInf) break;
    tok(p) = 256 + best;
    for (int j = p + 1; j + 1 < m; ++j) tok(j) = tok(j + 1);
    for (int j = p + 1; j + 2 < m; ++j) rk(j) = rk(j + 1);
    --m;
    int next;
    const int at = st.merged(p, m, &next);
    if (p > 0) rk(p - 1) = drop_rank(tab, mask, tok(p - 1), tok(p), d, wpos + at);
    if (p + 1 < m) rk(p) = drop_rank(tab, mask, tok(p), tok(p + 1), d, wpos + next);
  }
  return m;
}

__device__ __forceinline__ uint32_t drop_rank16(const u64* __restrict__ tab, u64 mask, uint32_t a, uint32_t b,
                                                const Drop& d, u64 pos) {
  const int r = drop_rank(tab, mask, (int)a, (int)b, d, pos);
  return r == kInf ? 0xFFFFu : (uint32_t)r;
}

// merge_word_packed of encode_device.hip (entry j = tok_j << 16 | rank of (tok_j, tok_j+1)) likewise.
__device__ __forceinline__ int merge_word_packed_drop(uint32_t* e, int m, const u64* __restrict__ tab, u64 mask,
                                                      const Drop& d, u64 wpos) {
#define E(j) e[(j) * kThreads]
  BitStarts st;
  st.init(m);
  for (int j = 0; j + 1 < m; ++j) E(j) |= drop_rank16(tab, mask, E(j) >> 16, E(j + 1) >> 16, d, wpos + j + 1);
  E(m - 1) |= 0xFFFFu;
  while (m > 1) {
    uint32_t best = 0xFFFFu;
    int p = -1;
    for (int j = 0; j + 1 < m; ++j) {
      const uint32_t r = E(j) & 0xFFFFu;
      if (r < best) { best = r; p = j; }
    }
    if (p < 0) break;
    const uint32_t x = 256u + best;
    for (int j = p + 1; j + 1 < m; ++j) E(j) = E(j + 1);
    --m;
    int next;
    const int at = st.merged(p, m, &next);
    E(p) = x << 16 | (p + 1 < m ? drop_rank16(tab, mask, x, E(p + 1) >> 16, d, wpos + next) : 0xFFFFu);
    if (p > 0) E(p - 1) = (E(p - 1) & 0xFFFF0000u) | drop_rank16(tab, mask, E(p - 1) >> 16, x, d, wpos + at);
  }
#undef E
  return m;
}

struct LdsRef {
  int* base;
  __device__ __forceinline__ int& operator()(int j) const { return base[j * kThreads]; }
};
struct GlobalRef {
  int* base;
  __device__ __forceinline__ int& operator()(int j) const { return base[j]; }
};

// encode_word of encode_device.hip under dropout: the ids of text[s .. s + L), L <= kEncMaxWord, to
// out + at; a word above kStrip bytes keeps its tokens at gtok (at or behind out + at), its ranks at
// grank and its tokens' begins at gat.  pos_base + s is the position of the word's first byte.
template <bool kPacked>
__device__ __forceinline__ int encode_word_drop(const uint8_t* __restrict__ text, u64 s, int L, const int* s_map,
                                                int* s_strip, int tid, const u64* __restrict__ tab, u64 mask,
                                                const Drop& d, u64 pos_base, int32_t* gtok, int32_t* grank,
                                                int32_t* gat, int32_t* out, u64 at) {
  const u64 wpos = pos_base + s;
  int m;
  if (L <= kStrip) {
    if (kPacked) {
      uint32_t* e = reinterpret_cast<uint32_t*>(s_strip) + tid;
      for (int k = 0; k < L; ++k) e[k * kThreads] = (uint32_t)s_map[text[s + k]] << 16;
      m = merge_word_packed_drop(e, L, tab, mask, d, wpos);
      for (int k = 0; k < m; ++k) out[at + k] = (int)(e[k * kThreads] >> 16);
    } else {
      LdsRef tok{s_strip + tid}, rk{s_strip + kStrip * kThreads + tid};
      for (int k = 0; k < L; ++k) tok(k) = s_map[text[s + k]];
      m = merge_word_drop(tok, rk, L, tab, mask, d, wpos, BitStarts{});
      for (int k = 0; k < m; ++k) out[at + k] = tok(k);
    }
  } else {
    GlobalRef gt{gtok}, gr{grank};
    for (int k = 0; k < L; ++k) gt(k) = s_map[text[s + k]];
    m = merge_word_drop(gt, gr, L, tab, mask, d, wpos, ArrayStarts{gat});
    if (gtok != out + at)
      for (int k = 0; k < m; ++k) out[at + k] = gt(k);
  }
  return m;
}

// k_encode_words of encode_device.hip with encode_word_drop: the same walk, the same outputs (ids
// packed at each thread's first word start in pad, tcnt, bcnt, the flag in misc[1]).  starts: the
// third scratch array, as long as pad and rank.
template <bool kAligned, bool kPacked>
__global__ __launch_bounds__(kThreads) void k_encode_words_drop(const uint8_t* __restrict__ text, u64 n,
                                                                const int32_t* __restrict__ byte_map,
                                                                const u64* __restrict__ tab, u64 mask, Drop drop,
                                                                u64 pos_base, int32_t* __restrict__ pad,
                                                                int32_t* __restrict__ rank,
                                                                int32_t* __restrict__ starts,
                                                                uint32_t* __restrict__ tcnt, u64* __restrict__ bcnt,
                                                                u64* __restrict__ misc,
                                                                const uint32_t* __restrict__ lcnt) {
  __shared__ int s_map[256];
  __shared__ int s_strip[(kPacked ? 1 : 2) * kStrip * kThreads];
  __shared__ uint32_t s_sum;
  const int tid = threadIdx.x;
  for (int i = tid; i < 256; i += kThreads) s_map[i] = byte_map[i];
  if (tid == 0) s_sum = 0;
  __syncthreads();

  const u64 base = (u64)blockIdx.x * kChunk + (u64)tid * kSpan;
  uint32_t cnt = 0, j0 = 0;
  if (base < n) {
    const u64 lim = n - base < (u64)kSpan ? n - base : (u64)kSpan;
    uint32_t dm = 0;  // bit k: byte base + k is a delimiter (or past the end)
    if (kAligned && lim == (u64)kSpan) {
      const uint4* p = reinterpret_cast<const uint4*>(text + base);
      const uint4 v0 = p[0], v1 = p[1];
      const uint32_t w[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
      for (int k = 0; k < kSpan; ++k) dm |= is_delim((w[k >> 2] >> (8 * (k & 3))) & 255u) << k;
    } else {
      for (int k = 0; k < kSpan; ++k) dm |= ((u64)k < lim ? is_delim(text[base + k]) : 1u) << k;
    }
    const uint32_t prevd = base == 0 ? 1u : is_delim(text[base - 1]);
    uint32_t begins = ~dm & ((dm << 1) | prevd);
    if (begins) j0 = __ffs(begins) - 1;
    u64 wpos = base + j0;
    while (begins) {
      const int j = __ffs(begins) - 1;
      begins &= begins - 1;
      const u64 s = base + j;
      const uint32_t above = dm >> j;  // bit 0 is clear: s starts a word
      u64 L;
      if (above) {
        L = __ffs(above) - 1;
      } else {  // runs past the span
        u64 e = base + kSpan;
        while (e < n && e - s <= (u64)kEncMaxWord && !is_delim(text[e])) ++e;
        L = e - s;
      }
      if (L > (u64)kEncMaxWord) {
        if (!lcnt) {
          atomicOr(reinterpret_cast<unsigned long long*>(misc + 1), 1ull);
          continue;
        }
        // long-word mode: the long pass left the ids at pad + s and their count at the span's entry
        // of lcnt (no dropout there); wpos <= s, so the ascending copy is safe
        const uint32_t m = lcnt[(u64)blockIdx.x * kThreads + tid];
        if (wpos != s)
          for (uint32_t k = 0; k < m; ++k) pad[wpos + k] = pad[s + k];
        wpos += m;
        cnt += m;
        continue;
      }
      // a word above kStrip: tokens at pad + s (wpos <= s, the ascending copy to pad + wpos is
      // safe), ranks at rank + s, begins at starts + s; s + L <= n, the arrays' length
      const int m = encode_word_drop<kPacked>(text, s, (int)L, s_map, s_strip, tid, tab, mask, drop, pos_base, pad + s,
                                              rank + s, starts + s, pad, wpos);
      wpos += m;
      cnt += m;
    }
  }
  tcnt[(u64)blockIdx.x * kThreads + tid] = cnt << 5 | j0;
  if (cnt) atomicAdd(&s_sum, cnt);
  __syncthreads();
  if (tid == 0) bcnt[blockIdx.x] = s_sum;
}

// Dropout's own scratch, allocated on the first dropout call and grown to the largest call seen.
struct DropoutState : PassState {
  DeviceBuf<int32_t> starts;  // token begins of the words above kStrip bytes: 4 B per text byte
};

}  // namespace

bool EncodeDevice::set_dropout(double p, uint64_t seed) {
  if (!(p >= 0.0 && p <= 1.0)) return false;  // NaN too
  drop_p_ = p;
  drop_seed_ = seed;
  drop_thresh_ = (uint64_t)(p * 4294967296.0);
  return true;
}

int EncodeDevice::dropout_words(const uint8_t* text, size_t n, const uint64_t* table, const int32_t* byte_map,
                                int32_t* pad, int32_t* rank, size_t scratch_cap, uint32_t* tcnt, uint64_t* bcnt,
                                uint64_t* misc, const uint32_t* lcnt, uint64_t pos_base, void* stream) {
  DropoutState& ds = pass_state<DropoutState>(pass_[kDropout]);
  if (!ds.starts.grow(scratch_cap)) {
    std::fprintf(stderr, "[ERROR]\t encoder: dropout scratch allocation failed (%zu bytes)\n", scratch_cap * 4);
    return -1;
  }
  const u64 nb = (n + kChunk - 1) / kChunk;
  const bool aligned = (reinterpret_cast<uintptr_t>(text) & 15) == 0;
  auto kern = aligned ? (packed_ ? k_encode_words_drop<true, true> : k_encode_words_drop<true, false>)
                      : (packed_ ? k_encode_words_drop<false, true> : k_encode_words_drop<false, false>);
  kern<<<dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream>>>(text, n, byte_map, table, mask_,
                                                                      Drop{drop_seed_, drop_thresh_}, pos_base, pad, rank,
                                                                      ds.starts.get(), tcnt, bcnt, misc, lcnt);
  ENC_OK(hipGetLastError());
  return 0;
}

}  // namespace shred
