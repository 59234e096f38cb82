// Words above kEncMaxWord bytes on gfx950: one workgroup encodes one word (C ABI:
// include/shredword_encode.h, shred_encoder_set_long_words).  The word passes of encode_device.hip
// give a word to one thread, whose lowest-rank loop is O(L^2); this pass runs before them, leaves
// every long word's ids at pad + the word's text offset and its id count at the entry of the
// 32-byte span it starts in, and the word passes place those ids like any other word's.
//
//   k_long_find     the word walk of encode_words.h over the text staged in LDS.  A word whose
//                   byte walk gives up at kEncMaxWord + 1 is followed to its end 8 bytes at a time.
//                   Counts the long words and their longest; flags one above kEncMaxLongWord.  A
//                   second launch (only when there is a long word) lists (start, length).
//   k_long_encode   one workgroup per listed word, in rounds.  A round takes r* = the lowest rank
//                   over all adjacent pairs (block reduction), applies merge r* = (a, b) -> x at
//                   every left-to-right non-overlapping occurrence, compacts the survivors (block
//                   scan) and recomputes the ranks of the pairs that touch a new x.  For a != b two
//                   occurrences cannot overlap and every match is taken.  For a == b the token at
//                   offset k of a maximal run of a's is the left half of a pair iff k is even and
//                   k + 1 lies in the run; the run start in reach of each thread's slab comes from
//                   a block max-scan of the slabs' last run starts.
// Rounds are exact: every pair a round creates holds x = 256 + r*, so its rank is above r* (the
// argument of encode_device.hip's header); rounds visit ranks in increasing order and number at
// most min(M, L - 1).  Merging all local minima in one round would not be: with 0:(a,b)->X,
// 1:(X,c)->Y, 5:(c,d)->Z the text abcd is Y d, and local minima give X Z.
//
// A round walks the word in tiles of kLongTile tokens, kLongSlab consecutive ones per thread: a
// thread loads its slab (and one token before, two after) into registers, the scans run, and the
// survivors go back in place at or below where they were read, so no token is overwritten before
// its reader has it.  The thread that writes a rank also keeps the minimum for the next round.
// Tokens and ranks live in LDS while the word holds at most kLongLds tokens: 2 x 4 B x 18432 =
// 144 KB + 1.2 KB of scan words, three tiles.  The workgroup is alone on its CU whatever the
// threshold: its 1024 threads are 4 waves per SIMD and the kernel holds 82 registers a lane
// (88 allocated: 5 waves per SIMD), so a second workgroup would not fit, and forcing 64 registers
// spills.  The threshold therefore takes what one workgroup can have of the CU's 160 KB.  A
// longer word keeps its tokens in pad itself and its ranks in this pass's scratch, and moves into
// LDS once compaction brings it to kLongLds tokens.
// All global indices are 64-bit; every store is an ordinary vector store.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../host/encoder.h"
#include "encode_common.h"
#include "encode_words.h"

namespace shred {
namespace {

typedef uint64_t u64;

constexpr int kLongThreads = 1024;  // threads of the workgroup that encodes one word
constexpr int kLongSlab = 6;        // consecutive tokens a thread takes per tile
constexpr int kLongTile = kLongThreads * kLongSlab;
constexpr int kLongLds = 18432;     // tokens a word keeps in LDS (with their ranks: 144 KB, one workgroup per CU)
constexpr int kLongWaves = kLongThreads / 64;
constexpr int kNone = -2;           // no token: never an operand (operands are >= 0)
static_assert(kLongLds % kLongTile == 0, "an LDS-resident word is whole tiles");

// misc words of the pass: [0] long words counted, [1] flag: a word above kEncMaxLongWord, [2] the
// longest long word, [3] list entries written, [4] rounds run (all calls).
constexpr int kMiscWords = 5;

template <bool kWrite>
__global__ __launch_bounds__(kThreads) void k_long_find(const uint8_t* __restrict__ text, u64 n, u64 maxw,
                                                        u64* __restrict__ misc, u64* __restrict__ list, u64 list_cap) {
  __shared__ uint32_t s_text[kStageBytes / 4];
  const TextView tv = stage_chunk(text, n, blockIdx.x, s_text);
  const u64 base = (u64)blockIdx.x * kChunk + (u64)threadIdx.x * kSpan;
  for_each_word(
      tv, n, base,
      [&](u64 s, u64 L, int) {
        if (L <= (u64)kEncMaxWord) return;
        if (L > maxw) {
          if (!kWrite) atomicOr(reinterpret_cast<unsigned long long*>(misc + 1), 1ull);
          return;
        }
        if (kWrite) {
          const u64 i = atomicAdd(reinterpret_cast<unsigned long long*>(misc + 3), 1ull);
          if (i < list_cap) {
            list[2 * i] = s;
            list[2 * i + 1] = L;
          }
        } else {
          atomicAdd(reinterpret_cast<unsigned long long*>(misc), 1ull);
          atomicMax(reinterpret_cast<unsigned long long*>(misc + 2), (unsigned long long)L);
        }
      },
      text, maxw);
}

struct LongShared {
  int tok[kLongLds];
  int rk[kLongLds];
  int map[256];
  int wave[kLongWaves];  // the reductions' and scans' per-wave words
  int a, b;              // operands of the round's merge
  int ptok[2], prk[2];   // the token and rank just before a tile, as they were when the round began
};

struct LdsTokens {
  int *t, *r;
  __device__ __forceinline__ int& tok(int j) const { return t[j]; }
  __device__ __forceinline__ int& rk(int j) const { return r[j]; }
};
struct GlobalTokens {
  int32_t *t, *r;
  __device__ __forceinline__ int32_t& tok(int j) const { return t[j]; }
  __device__ __forceinline__ int32_t& rk(int j) const { return r[j]; }
};

struct OpMin {
  static constexpr int kIdentity = kInf;
  __device__ __forceinline__ int operator()(int x, int y) const { return x < y ? x : y; }
};
struct OpMax {
  static constexpr int kIdentity = -1;
  __device__ __forceinline__ int operator()(int x, int y) const { return x > y ? x : y; }
};
struct OpAdd {
  static constexpr int kIdentity = 0;
  __device__ __forceinline__ int operator()(int x, int y) const { return x + y; }
};

// Exclusive scan of v over the workgroup's threads; *total receives the reduction of all of them.
// Two barriers; every thread of the workgroup calls it.
template <class Op>
__device__ __forceinline__ int block_scan(int v, int* s_wave, int tid, int* total) {
  const Op op;
  const int lane = tid & 63, wid = tid >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc = op(inc, o);
  }
  if (lane == 63) s_wave[wid] = inc;
  __syncthreads();
  int before = Op::kIdentity, all = Op::kIdentity;
#pragma unroll
  for (int w = 0; w < kLongWaves; ++w) {
    const int x = s_wave[w];
    if (w < wid) before = op(before, x);
    all = op(all, x);
  }
  __syncthreads();
  *total = all;
  int prev = __shfl_up(inc, 1, 64);
  if (lane == 0) prev = Op::kIdentity;
  return op(before, prev);
}

// One round on tok[0 .. m) / rk[0 .. m): merge rstar = (a, b) applied left to right without overlap.
// Returns the new length; tmin / ta / tb: the lowest rank this thread wrote and its pair.
template <class A>
__device__ __forceinline__ int long_round(const A acc, const int m, const int rstar, const int a, const int b,
                                          const u64* __restrict__ tab, const u64 mask, LongShared& sh, const int tid,
                                          int& tmin, int& ta, int& tb) {
  const int x = 256 + rstar;
  const bool same = a == b;
  int qbase = 0;    // survivors of the tiles before this one
  int cstart = -1;  // a == b: the last run start before this tile
  int tile = 0;
  for (int t0 = 0; t0 < m; t0 += kLongTile, ++tile) {
    const int s0 = t0 + tid * kLongSlab;
    // T[i + 1], R[i + 1]: position s0 + i for i in [-1, kLongSlab + 1], as the round found them
    int T[kLongSlab + 3], R[kLongSlab + 3];
#pragma unroll
    for (int i = -1; i <= kLongSlab + 1; ++i) {
      const int p = s0 + i;
      const bool ok = p >= 0 && p < m && !(i < 0 && tid == 0);
      T[i + 1] = ok ? acc.tok(p) : kNone;
      R[i + 1] = ok ? acc.rk(p) : kInf;
    }
    if (tid == 0 && t0 > 0) {  // the tile before has been compacted: its last thread kept this pair
      T[0] = sh.ptok[tile & 1];
      R[0] = sh.prk[tile & 1];
    }
    if (tid == kLongThreads - 1) {
      sh.ptok[(tile + 1) & 1] = T[kLongSlab];
      sh.prk[(tile + 1) & 1] = R[kLongSlab];
    }
    int cs = cstart;
    if (same) {  // (uniform) the run start in reach of the slab: a max-scan of the slabs' last ones
      int last = -1;
#pragma unroll
      for (int i = 0; i < kLongSlab; ++i)
        if (T[i + 1] == a && T[i] != a) last = s0 + i;
      int all;
      const int before = block_scan<OpMax>(last, sh.wave, tid, &all);
      cs = before > cstart ? before : cstart;
      cstart = all > cstart ? all : cstart;
    }
    // bit i + 1: position s0 + i is the left half of a merged pair
    uint32_t left = 0;
    if (R[0] == rstar && (!same || ((s0 - 1 - cs) & 1) == 0)) left |= 1u;
#pragma unroll
    for (int i = 0; i <= kLongSlab + 1; ++i) {
      if (same && T[i + 1] == a && T[i] != a) cs = s0 + i;
      if (R[i + 1] == rstar && (!same || ((s0 + i - cs) & 1) == 0)) left |= 1u << (i + 1);
    }
    // position s0 + i goes iff s0 + i - 1 is a left half: bit i
    int keep = 0;
#pragma unroll
    for (int i = 0; i < kLongSlab; ++i) keep += (s0 + i < m) && !((left >> i) & 1u);
    int all;
    int q = qbase + block_scan<OpAdd>(keep, sh.wave, tid, &all);
    qbase += all;
    // (every thread has used what it loaded, and passed a barrier since: the writes may begin)
#pragma unroll
    for (int i = 0; i < kLongSlab; ++i) {
      if (s0 + i >= m || ((left >> i) & 1u)) continue;
      const bool li = (left >> (i + 1)) & 1u;
      const int v = li ? x : T[i + 1];
      const int ni = li ? i + 2 : i + 1;  // the next survivor (never removed: two left halves are never adjacent)
      int r = kInf;
      if (s0 + ni < m) {
        const bool ln = (left >> (ni + 1)) & 1u;
        const int w = ln ? x : (li ? T[i + 3] : T[i + 2]);
        r = (li || ln) ? pair_rank(tab, mask, v, w) : R[i + 1];
        if (r < tmin) {
          tmin = r;
          ta = v;
          tb = w;
        }
      }
      acc.tok(q) = v;
      acc.rk(q) = r;
      ++q;
    }
  }
  return qbase;
}

__global__ __launch_bounds__(kLongThreads) void k_long_encode(const uint8_t* __restrict__ text,
                                                              const u64* __restrict__ list,
                                                              const int32_t* __restrict__ byte_map,
                                                              const u64* __restrict__ tab, u64 mask, int32_t* pad,
                                                              int32_t* grank, uint32_t* __restrict__ cnt,
                                                              u64* __restrict__ misc) {
  __shared__ LongShared sh;
  const int tid = threadIdx.x;
  const u64 s = list[2 * (u64)blockIdx.x];
  int m = (int)list[2 * (u64)blockIdx.x + 1];
  for (int i = tid; i < 256; i += kLongThreads) sh.map[i] = byte_map[i];
  __syncthreads();
  const LdsTokens lds{sh.tok, sh.rk};
  const GlobalTokens glb{pad + s, grank ? grank + s : nullptr};  // (grank: there whenever a word is above kLongLds)
  bool in_lds = m <= kLongLds;
  for (int j = tid; j < m; j += kLongThreads) {
    const int v = sh.map[text[s + j]];
    if (in_lds) lds.tok(j) = v; else glb.tok(j) = v;
  }
  __syncthreads();
  int tmin = kInf, ta = 0, tb = 0;
  for (int j = tid; j < m; j += kLongThreads) {
    int r = kInf, v = 0, w = 0;
    if (j + 1 < m) {
      v = in_lds ? lds.tok(j) : glb.tok(j);
      w = in_lds ? lds.tok(j + 1) : glb.tok(j + 1);
      r = pair_rank(tab, mask, v, w);
    }
    if (in_lds) lds.rk(j) = r; else glb.rk(j) = r;
    if (r < tmin) {
      tmin = r;
      ta = v;
      tb = w;
    }
  }
  uint32_t rounds = 0;
  for (;;) {
    int rstar;
    (void)block_scan<OpMin>(tmin, sh.wave, tid, &rstar);  // (its barriers also order the round's writes)
    if (rstar == kInf) break;
    if (tmin == rstar) {  // every such thread holds the same pair
      sh.a = ta;
      sh.b = tb;
    }
    if (!in_lds && m <= kLongLds) {
      for (int j = tid; j < m; j += kLongThreads) {
        lds.tok(j) = glb.tok(j);
        lds.rk(j) = glb.rk(j);
      }
      in_lds = true;
    }
    __syncthreads();
    const int a = sh.a, b = sh.b;
    tmin = kInf;
    const int left = in_lds ? long_round(lds, m, rstar, a, b, tab, mask, sh, tid, tmin, ta, tb)
                            : long_round(glb, m, rstar, a, b, tab, mask, sh, tid, tmin, ta, tb);
    ++rounds;
    m = left;  // (< m: a round always merges its lowest pair)
  }
  if (in_lds)
    for (int j = tid; j < m; j += kLongThreads) pad[s + j] = lds.tok(j);
  if (tid == 0) {
    cnt[s / kSpan] = (uint32_t)m;
    atomicAdd(reinterpret_cast<unsigned long long*>(misc + 4), (unsigned long long)rounds);
  }
}

// The long pass's state, created on the first call with the mode on: the result words and events.
// Scratch, allocated on the first long word and grown to the largest call seen: 16 B per long word
// (the list), 4 B per 32 text bytes (the id counts), and, once a word above kLongLds bytes is met,
// 4 B per text byte (the ranks of such words, at their own offsets).
struct LongState : PassState {
  DeviceWords misc;
  PinnedWords host;
  DeviceBuf<u64> list;       // (start, length) of every long word
  DeviceBuf<uint32_t> cnt;   // id count of the long word that starts in each span
  DeviceBuf<int32_t> rank;   // ranks of the words above kLongLds
  uint64_t words = 0;        // long words encoded so far
  uint64_t scratch_bytes() const { return list.cap() * 16 + cnt.cap() * 4 + rank.cap() * 4; }
};

}  // namespace

void EncodeDevice::long_stats(uint64_t* scratch_bytes, uint64_t* words, uint64_t* rounds) const {
  const LongState* lx = static_cast<const LongState*>(pass_[kLong].get());
  if (scratch_bytes) *scratch_bytes = lx ? lx->scratch_bytes() : 0;
  if (words) *words = lx ? lx->words : 0;
  if (rounds) {
    *rounds = 0;
    DeviceGuard guard;
    if (lx && lx->misc.get() && hipSetDevice(device_) == hipSuccess)
      (void)hipMemcpy(rounds, lx->misc.get() + 4, 8, hipMemcpyDeviceToHost);
  }
}

int EncodeDevice::long_pass(const uint8_t* text, size_t n, const uint64_t* table, const int32_t* byte_map,
                            int32_t* pad, size_t pad_cap, void* stream, const uint32_t** cnt) {
  *cnt = nullptr;
  LongState& lx = pass_state<LongState>(pass_[kLong]);
  if (!lx.misc.get()) {
    if (!lx.misc.ensure(kMiscWords) || !lx.host.ensure(4)) return -1;
    ENC_OK(hipMemset(lx.misc.get(), 0, kMiscWords * 8));
  }
  hipStream_t st = (hipStream_t)stream;
  const u64 nb = (n + kChunk - 1) / kChunk;
  u64* const misc = lx.misc.get();
  ENC_OK(hipMemsetAsync(misc, 0, 32, st));  // (the round count behind them stays)
  k_long_find<false><<<dim3((unsigned)nb), dim3(kThreads), 0, st>>>(text, n, (u64)kEncMaxLongWord, misc, nullptr, 0);
  ENC_OK(hipGetLastError());
  ENC_OK(hipMemcpyAsync(lx.host.get(), misc, 24, hipMemcpyDeviceToHost, st));
  ENC_OK(hipStreamSynchronize(st));
  if (lx.host[1]) return -3;
  const size_t W = (size_t)lx.host[0], longest = (size_t)lx.host[2];
  if (W == 0) return 0;
  if (n > pad_cap) return -1;  // (reserve() sized pad for n)
  if (!lx.list.grow(2 * W) || !lx.cnt.grow(nb * kThreads) || (longest > (size_t)kLongLds && !lx.rank.grow(pad_cap))) {
    std::fprintf(stderr, "[ERROR]\t encoder: long-word scratch allocation failed (%zu words, %zu bytes)\n", W, n);
    return -1;
  }
  k_long_find<true><<<dim3((unsigned)nb), dim3(kThreads), 0, st>>>(text, n, (u64)kEncMaxLongWord, misc, lx.list.get(),
                                                                  (u64)W);
  ENC_OK(hipGetLastError());
  k_long_encode<<<dim3((unsigned)W), dim3(kLongThreads), 0, st>>>(text, lx.list.get(), byte_map, table, mask_, pad,
                                                                  longest > (size_t)kLongLds ? lx.rank.get() : nullptr,
                                                                  lx.cnt.get(), misc);
  ENC_OK(hipGetLastError());
  lx.words += W;
  *cnt = lx.cnt.get();
  return 0;
}

}  // namespace shred
