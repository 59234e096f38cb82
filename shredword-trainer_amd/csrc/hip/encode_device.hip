// BPE encoder on gfx950 (C ABI include/shredword_encode.h).
//
// Applies a trained merge list to text.  The replay the trainer performs (merge m over every word
// left to right, reference bpe.cpp:265-296, for m = 0, 1, ...) equals, per word, "merge the
// leftmost adjacent pair of lowest rank until no pair has a rank": a pair created by merge m
// involves the new id 256 + m, so its rank is > m, and no earlier rank can reappear.  The
// kernels therefore encode every word independently:
//
//   k_encode_words  one thread per 32-byte span takes the words that START in it (maximal runs
//                   outside "\t\r\n ", found with a 32-bit delimiter mask of the span), maps
//                   bytes through the byte map, and runs the lowest-rank loop on a per-thread
//                   LDS strip of tokens and cached pair ranks (words <= 32 bytes), or in global
//                   scratch (longer words, <= kEncMaxWord).  Pair ranks come from a read-only
//                   open-addressing table of u64 slots (L2-resident: 16 K slots = 128 KB for
//                   8 K merges).  A thread packs its words' ids at its first word start, so the
//                   spans of different threads never overlap; per-thread and per-block counts.
//   hipCUB scan     inclusive block sums (the last is the total).
//   k_encode_emit   one workgroup per block copies its threads' runs to the output in text
//                   order: each output slot finds its thread by binary search over the block's
//                   inclusive scan, so the stores are coalesced.
// Traffic per text byte: 1 B read + 4 B x (ids / byte) x 3 (pack write, emit read, emit write)
// + 0.125 B of counts; algorithmic: 1 B + 4 B x ids / byte.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../host/encoder.h"
#include "encode_common.h"
#include "encode_words.h"

namespace shred {
namespace {

typedef uint64_t u64;

constexpr int kStrip = 32;                 // tokens a word keeps in LDS (32 KB per workgroup)
// (pair_rank and kInf: encode_words.h)

// Lowest-rank merging of tok[0..m) with cached ranks rk[0..m-1) (LDS strip or global scratch).
// Returns the final length.
template <typename Tok>
__device__ __forceinline__ int merge_word(Tok tok, Tok rk, int m, const u64* __restrict__ tab, u64 mask) {
  for (int j = 0; j + 1 < m; ++j) rk(j) = pair_rank(tab, mask, tok(j), tok(j + 1));
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
    if (p > 0) rk(p - 1) = pair_rank(tab, mask, tok(p - 1), tok(p));
    if (p + 1 < m) rk(p) = pair_rank(tab, mask, tok(p), tok(p + 1));
  }
  return m;
}

// Packed form for vocabularies below 2^16 ids: LDS entry j = tok_j << 16 | rank of (tok_j, tok_j+1)
// (0xFFFF: none), one word per position, so a strip takes half the LDS (twice the occupancy) and
// a shift moves token and rank together.  e points at the thread's column (stride kThreads).
__device__ __forceinline__ uint32_t rank16(const u64* __restrict__ tab, u64 mask, uint32_t a, uint32_t b) {
  const int r = pair_rank(tab, mask, (int)a, (int)b);
  return r == kInf ? 0xFFFFu : (uint32_t)r;
}

__device__ __forceinline__ int merge_word_packed(uint32_t* e, int m, const u64* __restrict__ tab, u64 mask) {
#define E(j) e[(j) * kThreads]
  for (int j = 0; j + 1 < m; ++j) E(j) |= rank16(tab, mask, E(j) >> 16, E(j + 1) >> 16);
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
    E(p) = x << 16 | (p + 1 < m ? rank16(tab, mask, x, E(p + 1) >> 16) : 0xFFFFu);
    if (p > 0) E(p - 1) = (E(p - 1) & 0xFFFF0000u) | rank16(tab, mask, E(p - 1) >> 16, x);
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

// The ids of the word text[s .. s + L), L <= kEncMaxWord, to dst = out + at; returns how many.  A
// word of at most kStrip bytes merges on the thread's LDS strip (s_strip is the workgroup's).  A
// longer one merges in global scratch, tokens at gtok and ranks at grank, and is then copied to dst
// in ascending order: gtok is dst itself (no copy) or lies at or behind it.  (out and at apart:
// the direct path's kernel keeps two registers fewer than with the pointer formed by the caller.)
template <bool kPacked>
__device__ __forceinline__ int encode_word(const uint8_t* __restrict__ text, u64 s, int L, const int* s_map,
                                           int* s_strip, int tid, const u64* __restrict__ tab, u64 mask,
                                           int32_t* gtok, int32_t* grank, int32_t* out, u64 at) {
  int m;
  if (L <= kStrip) {
    if (kPacked) {
      uint32_t* e = reinterpret_cast<uint32_t*>(s_strip) + tid;
      for (int k = 0; k < L; ++k) e[k * kThreads] = (uint32_t)s_map[text[s + k]] << 16;
      m = merge_word_packed(e, L, tab, mask);
      for (int k = 0; k < m; ++k) out[at + k] = (int)(e[k * kThreads] >> 16);
    } else {
      LdsRef tok{s_strip + tid}, rk{s_strip + kStrip * kThreads + tid};
      for (int k = 0; k < L; ++k) tok(k) = s_map[text[s + k]];
      m = merge_word(tok, rk, L, tab, mask);
      for (int k = 0; k < m; ++k) out[at + k] = tok(k);
    }
  } else {
    GlobalRef gt{gtok}, gr{grank};
    for (int k = 0; k < L; ++k) gt(k) = s_map[text[s + k]];
    m = merge_word(gt, gr, L, tab, mask);
    if (gtok != out + at)
      for (int k = 0; k < m; ++k) out[at + k] = gt(k);
  }
  return m;
}

template <bool kAligned, bool kPacked>
__global__ __launch_bounds__(kThreads) void k_encode_words(const uint8_t* __restrict__ text, u64 n,
                                                           const int32_t* __restrict__ byte_map,
                                                           const u64* __restrict__ tab, u64 mask,
                                                           int32_t* __restrict__ pad, int32_t* __restrict__ rank,
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
    uint32_t starts = ~dm & ((dm << 1) | prevd);
    if (starts) j0 = __ffs(starts) - 1;
    u64 wpos = base + j0;
    while (starts) {
      const int j = __ffs(starts) - 1;
      starts &= starts - 1;
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
        // long-word mode: the long pass (encode_long.hip) left the ids at pad + s and their count
        // at the span's entry of lcnt; wpos <= s, so the ascending copy is safe
        const uint32_t m = lcnt[(u64)blockIdx.x * kThreads + tid];
        if (wpos != s)
          for (uint32_t k = 0; k < m; ++k) pad[wpos + k] = pad[s + k];
        wpos += m;
        cnt += m;
        continue;
      }
      // a long word's tokens at pad + s: wpos <= s, so the ascending copy to pad + wpos is safe
      const int m = encode_word<kPacked>(text, s, (int)L, s_map, s_strip, tid, tab, mask, pad + s, rank + s, pad, wpos);
      wpos += m;
      cnt += m;
    }
  }
  tcnt[(u64)blockIdx.x * kThreads + tid] = cnt << 5 | j0;
  if (cnt) atomicAdd(&s_sum, cnt);
  __syncthreads();
  if (tid == 0) bcnt[blockIdx.x] = s_sum;
}

// ---- word cache: every distinct word is encoded once -------------------------------------
// A corpus repeats its words (C3: 1.13 G occurrences of 1.25 M distinct words), so the default
// path encodes each distinct word once and copies its ids to every occurrence:
//   k_cache_insert  per occurrence: 64-bit hash of (bytes, length) into an open-addressing table
//                   of 64-byte slots (key, payload = the inserting occurrence's offset, then the
//                   short word's bytes and ids inline): a read that hits L2 for a hot word, a CAS
//                   only for an empty slot; a full probe window flags an overflow (the table then
//                   grows 4x);
//   k_cache_encode  per used slot: the lowest-rank loop on that occurrence; the ids, then the
//                   word's bytes, go to a dense arena (one entry per distinct word), and the
//                   payload becomes (arena offset, length, id count);
//   k_cache_words   per occurrence: the slot (key and payload in one 16-byte load), a byte compare
//                   with the slot's inline copy (words <= 16 bytes with <= 8 ids: no arena read)
//                   or the arena's (a 64-bit collision is flagged, never trusted); then the
//                   block's ids are written as one contiguous run from its first word start
//                   (per-block count + start);
//   k_block_emit    one workgroup per block copies its run to the output, coalesced.
// An arena overflow or a collision reruns the call on the direct path (k_encode_words): exact
// always.  HBM traffic per text byte: 2 B of text reads (insert, words) + 4 B x ids / byte x 3
// (run write, emit read, emit write); the slot table and arena stay in L2/MALL for a corpus of
// repeated words.
constexpr int kCacheProbes = 128;
// A word-cache slot is one 64-byte line of 8 u64: [0] key, [1] payload (first the inserting
// occurrence's offset), [2..3] the word's bytes and [4..7] its ids inline when it is short
// (<= kInlineBytes bytes, <= kInlineIds ids; most occurrences at any vocab size), so a hot word
// costs k_cache_words one line -- which stays in L2 -- and no arena read.
constexpr int kSlotU64 = 8;
constexpr int kInlineBytes = 16;
constexpr int kInlineIds = 8;
constexpr int kSpanWords = kSpan / 2 + 1;  // words starting in one span, at most

template <typename T>
__device__ __forceinline__ u64 word_hash(const T& t, u64 s, uint32_t L) {
  u64 h = 1469598103934665603ull;
  for (uint32_t k = 0; k < L; ++k) h = (h ^ t[s + k]) * 1099511628211ull;
  h ^= (u64)L * 0x9E3779B97F4A7C15ull;
  // FNV's multiplier barely mixes the middle bits the slot index uses: murmur3's fmix64 does
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h | 1ull;  // 0 marks an empty slot
}

__device__ __forceinline__ void flag(u64* misc, u64 bit) {
  atomicOr(reinterpret_cast<unsigned long long*>(misc + 1), (unsigned long long)bit);
}

__global__ __launch_bounds__(kThreads) void k_cache_insert(const uint8_t* __restrict__ text, u64 n,
                                                           u64* __restrict__ slot, u64 cmask, u64* __restrict__ misc,
                                                           bool long_words) {
  __shared__ uint32_t s_text[kStageBytes / 4];
  const TextView tv = stage_chunk(text, n, blockIdx.x, s_text);
  const u64 base = (u64)blockIdx.x * kChunk + (u64)threadIdx.x * kSpan;
  for_each_word(tv, n, base, [&](u64 s, u64 L, int) {
    if (L > (u64)kEncMaxWord) {  // never cached (the payload's fields hold 16 bits): the long pass's, or an error
      if (!long_words) flag(misc, 1);
      return;
    }
    const u64 h = word_hash(tv, s, (uint32_t)L);
    u64 i = (h >> 17) & cmask;
    for (int p = 0; p < kCacheProbes; ++p, i = (i + 1) & cmask) {
      u64 k = slot[kSlotU64 * i];  // hot words: a read that hits L2, no atomic
      if (k == 0) {
        k = atomicCAS(reinterpret_cast<unsigned long long*>(slot + kSlotU64 * i), 0ull, (unsigned long long)h);
        if (k == 0) {
          slot[kSlotU64 * i + 1] = s;  // any occurrence spells the word (k_cache_words checks them all)
          return;
        }
      }
      if (k == h) return;
    }
    flag(misc, 2);  // window full
  });
}

// Payload of an encoded slot: arena offset (int32 units) | length << 32 | id count << 48.  The arena
// entry at that offset: a header (id count | length << 16), the ids, the word's bytes.
__device__ __forceinline__ u64 pack_payload(u64 off, u64 L, u64 m) { return off | L << 32 | m << 48; }

template <bool kPacked>
__global__ __launch_bounds__(kThreads) void k_cache_encode(const uint8_t* __restrict__ text, u64 n,
                                                           const int32_t* __restrict__ byte_map,
                                                           const u64* __restrict__ tab, u64 mask,
                                                           u64* __restrict__ slot, u64 cap,
                                                           int32_t* __restrict__ arena, u64 arena_cap,
                                                           int32_t* __restrict__ rank, u64* __restrict__ misc) {
  __shared__ int s_map[256];
  __shared__ int s_strip[(kPacked ? 1 : 2) * kStrip * kThreads];
  const int tid = threadIdx.x;
  for (int i = tid; i < 256; i += kThreads) s_map[i] = byte_map[i];
  __syncthreads();
  const u64 i = (u64)blockIdx.x * kThreads + tid;
  if (i >= cap || slot[kSlotU64 * i] == 0) return;
  const u64 s = slot[kSlotU64 * i + 1];
  u64 e = s;
  while (e < n && !is_delim(text[e])) ++e;  // <= kEncMaxWord (insert checked)
  const int L = (int)(e - s);
  const u64 need = 1 + (u64)L + (u64)(L + 3) / 4;  // header (m | L << 16), ids (<= L), then the bytes
  const u64 off = atomicAdd(reinterpret_cast<unsigned long long*>(misc + 2), (unsigned long long)need);
  if (off + need > arena_cap) {
    flag(misc, 8);  // arena full
    return;
  }
  int32_t* ids = arena + off + 1;
  // a long word's tokens in the arena entry itself, its ranks in scratch at the word's own text offset
  const int m = encode_word<kPacked>(text, s, L, s_map, s_strip, tid, tab, mask, ids, rank + s, ids, 0);
  uint32_t* bytes = reinterpret_cast<uint32_t*>(ids + m);
  for (int k = 0; k < L; k += 4) {
    uint32_t w = 0;
    for (int b = 0; b < 4 && k + b < L; ++b) w |= (uint32_t)text[s + k + b] << (8 * b);
    bytes[k / 4] = w;
  }
  arena[off] = m | L << 16;
  u64* sl = slot + kSlotU64 * i;
  if (L <= kInlineBytes && m <= kInlineIds) {  // the bytes and the ids inline (zero-padded)
    u64 b[2] = {0, 0};
    for (int k = 0; k < L; ++k) b[k >> 3] |= (u64)text[s + k] << (8 * (k & 7));
    sl[2] = b[0];
    sl[3] = b[1];
    u64 w[kInlineIds / 2] = {0, 0, 0, 0};
    for (int k = 0; k < m; ++k) w[k >> 1] |= (u64)(uint32_t)ids[k] << (32 * (k & 1));
    for (int k = 0; k < kInlineIds / 2; ++k) sl[4 + k] = w[k];
  }
  sl[1] = pack_payload(off, (u64)L, (u64)m);
}

// Per occurrence: its word's cached ids, written straight to the output at the chunk's place.
// The chunk's place is its exclusive sum over the chunks before it, found by a decoupled
// look-back: chunks are taken in ticket order (a block never waits for one that has not started),
// each publishes its id count, then walks back over the predecessors' published counts until one
// that also published its inclusive sum (status 2), and publishes its own.  The states are 8-B
// agent atomics on both sides (cross-XCD coherent).  No staging copy of the ids.
constexpr u64 kLbValue = (1ull << 62) - 1;
constexpr uint32_t kLongEntry = 0xFFFFFFFFu;  // s_list: the span's long word (no slot has index 2^31 - 1)
__global__ __launch_bounds__(kThreads) void k_cache_words(const uint8_t* __restrict__ text, u64 n,
                                                          const u64* __restrict__ slot, u64 cmask,
                                                          const int32_t* __restrict__ arena, int32_t* __restrict__ out,
                                                          u64 out_cap, u64* __restrict__ bcnt, u64* __restrict__ lb,
                                                          u64 nb, u64* __restrict__ misc,
                                                          const int32_t* __restrict__ lids,
                                                          const uint32_t* __restrict__ lcnt) {
  __shared__ uint32_t s_text[kStageBytes / 4];
  __shared__ uint32_t s_list[kSpanWords * kThreads];  // this chunk's words: arena offsets, column per thread
  __shared__ uint32_t s_inc[kThreads];
  __shared__ u64 s_chunk, s_prefix;
  const int tid = threadIdx.x;
  if (tid == 0) {
    s_chunk = __hip_atomic_fetch_add(lb + nb, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ticket
  }
  __syncthreads();
  const u64 chunk = s_chunk;
  const TextView tv = stage_chunk(text, n, chunk, s_text);  // synchronises
  const u64 cbase = chunk * kChunk;
  const u64 base = cbase + (u64)tid * kSpan;
  uint32_t cnt = 0, nw = 0;
  uint32_t lm = 0;  // long-word mode: the id count of the span's long word (its last word), ids at lids + ls
  u64 ls = 0;
  for_each_word(tv, n, base, [&](u64 s, u64 L, int) {
    if (L > (u64)kEncMaxWord) {  // flagged by k_cache_insert, or encoded by the long pass
      if (lcnt) {
        lm = lcnt[chunk * kThreads + tid];
        ls = s;
        s_list[nw * kThreads + tid] = kLongEntry;
        ++nw;
        cnt += lm;
      }
      return;
    }
    const u64 h = word_hash(tv, s, (uint32_t)L);
    u64 pay = 0, i = (h >> 17) & cmask;
    for (int p = 0; p < kCacheProbes; ++p, i = (i + 1) & cmask) {
      const ulonglong2 sl = *reinterpret_cast<const ulonglong2*>(slot + kSlotU64 * i);  // key and payload: one load
      if (sl.x == h) {
        pay = sl.y;
        break;
      }
      if (sl.x == 0) break;
    }
    if (!pay) return;  // not inserted: an overflow, flagged by k_cache_insert / k_cache_encode
    const uint32_t m = (uint32_t)(pay >> 48), pl = (uint32_t)(pay >> 32) & 0xFFFFu;
    uint32_t diff = pl != (uint32_t)L;
    uint32_t entry;
    if (pl <= (uint32_t)kInlineBytes && m <= (uint32_t)kInlineIds) {  // inline: the slot's own line
      const ulonglong2 sb = *reinterpret_cast<const ulonglong2*>(slot + kSlotU64 * i + 2);
      for (uint32_t k = 0; k < pl && !diff; ++k)
        diff |= (uint32_t)(((k < 8 ? sb.x : sb.y) >> (8 * (k & 7))) & 0xFFu) ^ tv[s + k];
      entry = 0x80000000u | (uint32_t)i;  // (slot indices < 2^31: the table is far smaller)
    } else {
      const uint8_t* ab = reinterpret_cast<const uint8_t*>(arena + (uint32_t)pay + 1 + m);
      for (uint32_t k = 0; k < pl && !diff; ++k) diff |= ab[k] ^ tv[s + k];
      entry = (uint32_t)pay;
    }
    if (diff) {
      flag(misc, 4);  // 64-bit collision
      return;
    }
    s_list[nw * kThreads + tid] = entry;
    ++nw;
    cnt += m;
  });
  s_inc[tid] = cnt;  // the per-thread id counts
  block_inclusive_scan(s_inc, tid);
  if (tid == 0) {
    const u64 agg = s_inc[kThreads - 1];
    u64 prefix = 0;
    if (chunk == 0) {
      __hip_atomic_exchange(lb, (2ull << 62) | agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      __hip_atomic_exchange(lb + chunk, (1ull << 62) | agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (u64 j = chunk - 1;;) {
        const u64 v = __hip_atomic_fetch_add(lb + j, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const u64 status = v >> 62;
        if (status == 0) {
          __builtin_amdgcn_s_sleep(1);
          continue;
        }
        prefix += v & kLbValue;
        if (status == 2 || j == 0) break;
        --j;
      }
      __hip_atomic_exchange(lb + chunk, (2ull << 62) | (prefix + agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    s_prefix = prefix;
    bcnt[chunk] = agg;
    if (prefix + agg > out_cap) flag(misc, 16);  // the output is too small: nothing of this chunk is written
  }
  __syncthreads();
  if (s_prefix + s_inc[kThreads - 1] > out_cap) return;
  int32_t* dst = out + s_prefix + (s_inc[tid] - cnt);
  for (uint32_t w = 0; w < nw; ++w) {
    const uint32_t e = s_list[w * kThreads + tid];
    if (e == kLongEntry) {
      for (uint32_t k = 0; k < lm; ++k) dst[k] = lids[ls + k];
      dst += lm;
      continue;
    }
    if (e & 0x80000000u) {  // inline ids: the slot line the lookup just read
      const u64* sl = slot + kSlotU64 * (u64)(e & 0x7FFFFFFFu);
      const uint32_t m = (uint32_t)(sl[1] >> 48);
      const int32_t* src = reinterpret_cast<const int32_t*>(sl + 4);
      for (uint32_t k = 0; k < m; ++k) dst[k] = src[k];
      dst += m;
      continue;
    }
    const int32_t* src = arena + e;
    const uint32_t m = (uint32_t)src[0] & 0xFFFFu;
    ++src;
    for (uint32_t k = 0; k < m; ++k) dst[k] = src[k];
    dst += m;
  }
}

__global__ __launch_bounds__(kThreads) void k_encode_emit(const int32_t* __restrict__ pad, const uint32_t* __restrict__ tcnt,
                                                          const u64* __restrict__ bcnt, int32_t* __restrict__ out) {
  __shared__ uint32_t s_inc[kThreads];
  __shared__ int s_src[kThreads];  // pad offset of each thread's run (block-relative) minus its exclusive count
  const int tid = threadIdx.x;
  const uint32_t t = tcnt[(u64)blockIdx.x * kThreads + tid];
  const uint32_t cnt = t >> 5;
  s_inc[tid] = cnt;
  block_inclusive_scan(s_inc, tid);
  s_src[tid] = tid * kSpan + (int)(t & 31u) - (int)(s_inc[tid] - cnt);
  __syncthreads();
  const uint32_t total = s_inc[kThreads - 1];
  const u64 base = (u64)blockIdx.x * kChunk;
  int32_t* dst = out + (bcnt[blockIdx.x] - total);  // bcnt: inclusive block sums
  for (uint32_t i = tid; i < total; i += kThreads) {
    dst[i] = pad[(int64_t)base + s_src[first_above(s_inc, i, ~0u)] + (int64_t)i];
  }
}

// The core encoder's state: what create() uploads, and scratch sized for the largest text seen.
struct CoreState : PassState {
  DeviceBuf<u64> table;        // the merge-rank table (host/encoder.h)
  DeviceBuf<int32_t> byte_map;
  DeviceWords misc;            // [0] total ids, [1] flags: 1 long word, 2 probe window full, 4 collision,
                               // 8 arena full, 16 output capacity; [2] word-cache arena top
  PinnedWords host_misc;       // misc's first two words
  EventSet<4> ev;
  size_t cap_bytes = 0;        // text bytes the scratch below is sized for
  DeviceBuf<int32_t> pad;      // ids per word span
  DeviceBuf<int32_t> rank;     // rank cache of long words; the word cache's arena
  DeviceBuf<uint32_t> tcnt;    // per-thread counts
  DeviceBuf<u64> bcnt;         // [0, nb) block counts, [nb, 2 nb) inclusive sums, [2 nb, 3 nb] the
                               // look-back states and the ticket of k_cache_words
  DeviceBuf<uint8_t> scan_tmp;  // hipCUB scan scratch
  size_t scan_tmp_bytes = 0;
  // word cache: one 64-byte slot per distinct word (the layout: kSlotU64 above); the arena is rank
  size_t ccap = 0, ccap_min = 0;  // allocated slots; slots a call starts with
  DeviceBuf<u64> cslot;

  bool reserve(size_t n, std::string* why) {
    if (n <= cap_bytes) return true;
    cap_bytes = 0;
    const size_t nb = (n + kChunk - 1) / kChunk, cap = nb * kChunk;  // every later n <= cap fits
    // word-cache slots: the table is allocated for one slot per 256 text bytes; a call starts with
    // one per 4096 (a small table keeps the probed lines cache-resident) and grows it 4x while a
    // probe window overflows, then takes the direct path
    ccap = 1 << 20;
    while (ccap < cap / 256) ccap <<= 1;
    ccap_min = 1 << 20;
    while (ccap_min < cap / 4096) ccap_min <<= 1;
    if (!cslot.grow(ccap * kSlotU64)) {
      *why = "word-cache allocation failed";
      return false;
    }
    if (!pad.grow(cap) || !rank.grow(cap) || !tcnt.grow(nb * kThreads) || !bcnt.grow(3 * nb + 1) ||
        hipcub::DeviceScan::InclusiveSum(nullptr, scan_tmp_bytes, bcnt.get(), bcnt.get() + nb, (int)nb) != hipSuccess ||
        !scan_tmp.grow(scan_tmp_bytes ? scan_tmp_bytes : 16)) {
      *why = "scratch allocation failed";
      return false;
    }
    cap_bytes = cap;
    return true;
  }
};

}  // namespace

EncodeDevice* EncodeDevice::create(int device, const std::vector<uint64_t>& table, const int32_t* byte_map,
                                   std::string* why) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    *why = "no HIP device visible";
    return nullptr;
  }
  if (device < 0 || device >= count) {
    *why = "device ordinal " + std::to_string(device) + " out of range";
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) {
    *why = "hipSetDevice failed";
    return nullptr;
  }
  EncodeDevice* d = new EncodeDevice();
  d->device_ = device;
  d->mask_ = table.size() - 1;
  // 16-bit packing needs every id (bytes' symbols and 256 + rank) below 0xFFFF: decided from the
  // largest rank in the table (a merge list with repeated pairs has ranks past its distinct pairs)
  uint64_t max_rank = 0;
  for (uint64_t e : table)
    if (e != kEncEmpty) max_rank = std::max<uint64_t>(max_rank, e & 0xFFFFFu);
  d->packed_ = 256 + max_rank < 0xFFFFu;
  for (int b = 0; b < 256; ++b) d->packed_ = d->packed_ && byte_map[b] >= 0 && byte_map[b] < 0xFFFF;
  hipStream_t st = nullptr;
  bool ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
  d->stream_ = st;
  CoreState& c = pass_state<CoreState>(d->pass_[kCore]);
  ok = ok && c.table.grow(table.size()) && c.byte_map.grow(256) && c.misc.ensure(4) && c.host_misc.ensure(2);
  ok = ok && hipMemcpy(c.table.get(), table.data(), table.size() * 8, hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipMemcpy(c.byte_map.get(), byte_map, 256 * 4, hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && c.ev.ensure();
  if (!ok) {
    *why = "device allocation failed";
    delete d;
    return nullptr;
  }
  return d;
}

EncodeDevice::~EncodeDevice() {
  (void)hipSetDevice(device_);
  if (stream_) (void)hipStreamSynchronize((hipStream_t)stream_);
  for (auto& p : pass_) p.reset();
  if (stream_) (void)hipStreamDestroy((hipStream_t)stream_);
}

int64_t EncodeDevice::encode(const uint8_t* text, size_t n, int32_t* out, size_t cap, void* stream, double* kernel_ms,
                             uint64_t pos_base) {
  if (kernel_ms) *kernel_ms = 0;
  if (n == 0) return 0;
  if (!text || !out) return -1;
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  std::string why;
  CoreState& c = pass_state<CoreState>(pass_[kCore]);
  if (!c.reserve(n, &why)) {
    std::fprintf(stderr, "[ERROR]\t encoder: %s (%zu bytes)\n", why.c_str(), n);
    return -1;
  }
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)stream_;
  const u64 nb = (n + kChunk - 1) / kChunk;
  const char* env = std::getenv("SHREDWORD_ENCODE_CACHE");
  // dropout: every occurrence of a word differs, so the word cache cannot serve it (and such a call
  // is no fallback)
  const bool drop = drop_thresh_ != 0;
  bool cached = !drop && !(env && env[0] == '0');
  ENC_OK(hipEventRecord(c.ev[0], st));
  size_t cc = c.ccap_min, cmax = c.ccap;
  // tests: "<start>[:<max>]" slots for this call (powers of two in [kThreads, ccap]: the encode
  // grid is cc / kThreads and the probe mask cc - 1), so a few thousand words reach the growth
  // branch and the overflow after it
  if (const char* e = std::getenv("SHREDWORD_ENCODE_CACHE_SLOTS")) {
    auto slots = [&](const char* s) {
      const unsigned long long want = std::strtoull(s, nullptr, 10);
      size_t v = kThreads;
      while (v < c.ccap && v < want) v <<= 1;
      return v;
    };
    cc = slots(e);
    const char* colon = std::strchr(e, ':');
    cmax = colon ? std::max(cc, slots(colon + 1)) : c.ccap;
  }
  const bool debug = std::getenv("SHREDWORD_ENCODE_DEBUG") != nullptr;
  u64 *const misc = c.misc.get(), *const cslot = c.cslot.get(), *const bcnt = c.bcnt.get();
  int32_t *const pad = c.pad.get(), *const rank = c.rank.get();
  // long-word mode: the words above kEncMaxWord are encoded first, ids at pad + their offset, id
  // counts per span in lcnt; the word passes below then place them like any other word's ids
  const uint32_t* lcnt = nullptr;
  if (long_words_) {
    const int r = long_pass(text, n, c.table.get(), c.byte_map.get(), pad, c.cap_bytes, st, &lcnt);
    if (r < 0) return r;
  }
  for (;;) {
    ENC_OK(hipMemsetAsync(misc, 0, 32, st));
    if (cached) {
      ENC_OK(hipMemsetAsync(cslot, 0, cc * kSlotU64 * 8, st));
      k_cache_insert<<<dim3((unsigned)nb), dim3(kThreads), 0, st>>>(text, n, cslot, cc - 1, misc, long_words_);
      ENC_OK(hipGetLastError());
      auto enck = packed_ ? k_cache_encode<true> : k_cache_encode<false>;
      // arena offsets must stay below 2^31: bit 31 of a payload tags "ids inline in the slot", so
      // a larger arena flags "arena full" and the call reruns on the direct path
      const u64 arena_cap = std::min<u64>(c.cap_bytes, (u64)1 << 31);
      enck<<<dim3((unsigned)(cc / kThreads)), dim3(kThreads), 0, st>>>(text, n, c.byte_map.get(), c.table.get(), mask_,
                                                                       cslot, cc, rank, arena_cap, pad, misc);
      ENC_OK(hipGetLastError());
      // look-back states and the ticket (bcnt[2 nb, 3 nb], zero = "not published")
      ENC_OK(hipMemsetAsync(bcnt + 2 * nb, 0, (nb + 1) * 8, st));
      k_cache_words<<<dim3((unsigned)nb), dim3(kThreads), 0, st>>>(text, n, cslot, cc - 1, rank, out, (u64)cap, bcnt,
                                                                   bcnt + 2 * nb, nb, misc, pad, lcnt);
    } else if (drop) {
      if (dropout_words(text, n, c.table.get(), c.byte_map.get(), pad, rank, c.cap_bytes, c.tcnt.get(), bcnt, misc, lcnt,
                        pos_base, st) < 0)
        return -1;
    } else {
      const bool aligned = (reinterpret_cast<uintptr_t>(text) & 15) == 0;
      auto kern = aligned ? (packed_ ? k_encode_words<true, true> : k_encode_words<true, false>)
                          : (packed_ ? k_encode_words<false, true> : k_encode_words<false, false>);
      kern<<<dim3((unsigned)nb), dim3(kThreads), 0, st>>>(text, n, c.byte_map.get(), c.table.get(), mask_, pad, rank,
                                                          c.tcnt.get(), bcnt, misc, lcnt);
    }
    ENC_OK(hipGetLastError());
    // inclusive block sums into bcnt[nb, 2 nb); the last one is the total
    ENC_OK(hipcub::DeviceScan::InclusiveSum(c.scan_tmp.get(), c.scan_tmp_bytes, bcnt, bcnt + nb, (int)nb, st));
    ENC_OK(hipMemcpyAsync(misc, bcnt + 2 * nb - 1, 8, hipMemcpyDeviceToDevice, st));
    ENC_OK(hipMemcpyAsync(c.host_misc.get(), misc, 16, hipMemcpyDeviceToHost, st));
    ENC_OK(hipStreamSynchronize(st));
    const uint64_t fl = c.host_misc[1];
    if (fl & 1) return -3;
    if (fl & 16) return -2;  // the output capacity (the cached path writes it directly)
    if (!(fl & 14)) break;
    if (fl == 2 && cc < cmax) {  // only a probe window overflowed: a bigger table
      cc = std::min(cmax, cc * 4);
      if (debug) std::fprintf(stderr, "[DEBUG]\t encoder: word cache grows to %zu slots\n", cc);
      continue;
    }
    cached = false;  // cache / arena overflow or a 64-bit word-hash collision: redo on the direct path
    // a slot the full arena left unencoded still holds its text offset where k_cache_words expects
    // a payload, so its occurrences raise the collision flag too: name the arena first
    if (debug)
      std::fprintf(stderr, "[DEBUG]\t encoder: word cache %s (%zu slots); direct path\n",
                   fl & 8 ? "arena overflow" : fl & 4 ? "hash collision" : "overflow", cc);
    ++fallbacks_;
  }
  ENC_OK(hipEventRecord(c.ev[1], st));
  const u64 total = c.host_misc[0];
  if (total > cap) return -2;
  ENC_OK(hipEventRecord(c.ev[2], st));
  if (total && !cached)  // the cached path wrote the ids in place (k_cache_words)
    k_encode_emit<<<dim3((unsigned)nb), dim3(kThreads), 0, st>>>(pad, c.tcnt.get(), bcnt + nb, out);
  ENC_OK(hipGetLastError());
  ENC_OK(hipEventRecord(c.ev[3], st));
  ENC_OK(hipStreamSynchronize(st));
  if (kernel_ms) ENC_OK(c.ev.sum_ms(2, kernel_ms));
  return (int64_t)total;
}

// Host text in pieces of at most kHostPiece bytes, each cut just after a delimiter (words never
// straddle two pieces, so the ids are those of one call): device memory stays at ~14 B per piece
// byte (5 B staging + the scratch reserve() sizes) whatever the text length.
int64_t EncodeDevice::encode_host(const uint8_t* text, size_t n, int32_t* out, size_t cap) {
  if (n == 0) return 0;
  if (!text || !out) return -1;
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  const size_t piece = std::min(n, piece_from_env("SHREDWORD_ENCODE_PIECE", kHostPiece, (size_t)kEncMaxWord + 2));
  HostStage& hs = pass_state<HostStage>(pass_[kStage]);
  if (!hs.reserve(piece)) {
    std::fprintf(stderr, "[ERROR]\t encoder: staging allocation failed (%zu bytes)\n", piece);
    return -1;
  }
  hipStream_t st = (hipStream_t)stream_;
  size_t pos = 0, done = 0;
  while (pos < n) {
    const size_t len = host_piece_len(text, n, pos, piece, max_word());
    if (len == 0) return -3;
    if (len > piece && !hs.reserve(len)) {  // a long word that the budget cut is staged whole
      std::fprintf(stderr, "[ERROR]\t encoder: staging allocation failed (%zu bytes)\n", len);
      return -1;
    }
    ENC_OK(hipMemcpyAsync(hs.text.get(), text + pos, len, hipMemcpyHostToDevice, st));
    const int64_t r = encode(hs.text.get(), len, hs.out.get(), cap - done, nullptr, nullptr, (uint64_t)pos);
    if (r < 0) return r;
    if (r > 0) {
      ENC_OK(hipMemcpyAsync(out + done, hs.out.get(), (size_t)r * 4, hipMemcpyDeviceToHost, st));
      ENC_OK(hipStreamSynchronize(st));
    }
    done += (size_t)r;
    pos += len;
  }
  return (int64_t)done;
}

}  // namespace shred
