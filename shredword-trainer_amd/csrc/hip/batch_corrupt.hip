// Span-corruption inputs and targets on gfx950 (T5 / UL2 denoising): every noise run of a row collapses
// to one sentinel in the input stream and follows its sentinel in the target stream (C ABI and
// definitions: include/shredword_encode.h, shred_corrupt_*).  Both streams come out in the flat
// (ids, row_off) format.  The passes share the batch units' tile geometry and wave search
// (batch_common.h), their device-call driver and piece rule (batch_state.h) and the hash of the
// dropout and masked-LM units.
//
// A decision is a function of (seed, index, id) alone: d(x, c) = mix(mix(seed + G (x + 1)) ^ c) with
// c = START for "a span starts at x" and c = LEN for its length, so nothing depends on the staging and
// a piece of the host call is the device call at index_base + its first id.
//
// One workgroup per kTile ids, 4 per lane, in every pass over the ids.  A workgroup finds the rows that
// begin in its tile with two wave searches of row_off (wave_upper_bound; per tile, not per token) and
// marks them in LDS, so no pass keeps per-id row data in global memory.
//
//   k_corrupt_rows     one thread per row_off entry: range, order and end points (word 0 of the result
//                      words; ordinary stores).  The later passes write nothing when it is set.
//   k_corrupt_noise    hashes start and length of the tile's positions and of a halo of len_n positions
//                      before it into LDS, once per position.  A lane looks back from the token before
//                      its four (at most len_n LDS bytes, stopping at a row's first token) and then
//                      carries the furthest reach forward: flags[k] = noise | run-first << 1.  The
//                      tile's aggregate of the per-row run count (a segmented sum: a row's first token
//                      resets it) goes to agg[tile].
//   hipCUB scan        inclusive, segmented sum over the tiles' aggregates: the runs of the current row
//                      before each tile.
//   k_corrupt_count    run rank = runs of the row so far; a run of rank >= Rmax is kept.  The tile's emit
//                      counts (input, target) go to tot[tile].
//   hipCUB scan        one inclusive sum over the tiles' (input, target) pairs.
//   k_corrupt_result   T_in and T_tgt beside word 0: one copy of three result words to the host, which
//                      checks the caps before anything is written.
//   k_corrupt_scatter  ranks and emit counts again from flags (block scans in LDS), then in_ids, in_src
//                      and tgt_ids at tile base + local offset (+ the row's index with closing
//                      sentinels: the count of row boundaries up to the token, scanned in LDS).  The
//                      rows whose offset lies in the tile get in_row_off, tgt_row_off and the closing
//                      sentinel of the row before.
//
// Traffic per id.  Read: 4 (ids, k_corrupt_noise) + 1 (flags, k_corrupt_count) + 4 + 1 (ids and flags,
// k_corrupt_scatter) = 10 B.  Written: 1 (flags) + 12 per input id (in_ids, in_src; 4 without in_src)
// + 4 per target id.  With the default options about 0.89 input and 0.20 target ids per id: about
// 12.5 B written, 22.5 B in all.  Per tile of 1024 ids: 8 + 8 B (agg, carry) and 16 + 16 B (tot, base)
// written and read once, and 6 wave searches of row_off.  Per row: 8 B read by k_corrupt_rows, 8 B read
// by each of the three passes, 16 B written (the two offsets) and 4 B for a closing sentinel.
// All global indices are 64-bit; every global store is an ordinary vector store (the only atomics
// count row boundaries in LDS).
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../host/encoder.h"
#include "batch_common.h"
#include "batch_state.h"
#include "encode_common.h"

namespace shred {
namespace {

constexpr u64 kGolden = 0x9E3779B97F4A7C15ull;
constexpr u64 kStart = (1ull << 40) + 2, kLen = (1ull << 40) + 3;  // beside the masked-LM unit's SEL and ACT
constexpr int kHalo = EncodeDevice::kCorruptMaxSpan;               // positions before a tile that can reach into it
constexpr uint32_t kSeg = 1u << 31;                                // segmented sums: "a row begins here or later"
constexpr u64 kSeg64 = 1ull << 63;

__device__ __forceinline__ u64 mix64(u64 x) {  // murmur3's fmix64
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// What the kernels know of a call's options; passed by value.
struct CorruptRule {
  u64 seed, base;  // base: index_base + the index in the call's ids of the pass's first id
  u64 t_start, rmax;
  u64 cum[EncodeDevice::kCorruptMaxSpan - 1];  // C_1 .. C_{len_n - 1}
  uint32_t len_n, fin;                         // fin: every target row ends with a closing sentinel
  int32_t sent_first, sent_step, sp_lo, sp_hi;
  uint32_t protect_specials, protect_n;
  int32_t protect[EncodeDevice::kMaskMaxProtect];

  __device__ __forceinline__ u64 draw(u64 x, u64 c) const { return mix64(mix64(seed + kGolden * (x + 1)) ^ c); }
  // L(pos) when a span starts at pos, else 0.
  __device__ __forceinline__ uint32_t span(u64 pos) const {
    const u64 h = base + pos;
    if ((draw(h, kStart) >> 32) >= t_start) return 0;
    const u64 v = draw(h, kLen) >> 32;
    uint32_t L = 1;
    for (uint32_t i = 0; i + 1 < len_n; ++i) L += v >= cum[i];
    return L;
  }
  __device__ __forceinline__ bool guarded(int32_t id) const {
    bool hit = protect_specials && id >= sp_lo && id < sp_hi;
    for (uint32_t i = 0; i < protect_n; ++i) hit |= protect[i] == id;
    return hit;
  }
  __device__ __forceinline__ int32_t sentinel(u64 j) const {
    return (int32_t)((int64_t)sent_first + (int64_t)j * (int64_t)sent_step);
  }
};

CorruptRule rule_of(const EncodeDevice::CorruptOpts& o, u64 first) {
  CorruptRule r{};
  r.seed = o.seed, r.base = o.index_base + first, r.t_start = o.t_start, r.rmax = o.rmax;
  for (uint32_t i = 0; i + 1 < o.len_n; ++i) r.cum[i] = o.len_cum[i];
  r.len_n = o.len_n, r.fin = o.closing ? 1u : 0u;
  r.sent_first = o.sent_first, r.sent_step = o.sent_step, r.sp_lo = o.sp_lo, r.sp_hi = o.sp_hi;
  r.protect_specials = o.protect_specials ? 1u : 0u, r.protect_n = o.protect_n;
  for (uint32_t i = 0; i < o.protect_n; ++i) r.protect[i] = o.protect[i];
  return r;
}

// Segmented sum: the count since the last flagged element.  0 is its identity on both sides.
struct SegAdd32 {
  __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const {
    return (b & kSeg) ? b : ((a & kSeg) | ((a & ~kSeg) + b));
  }
};
struct SegAdd64 {
  __host__ __device__ __forceinline__ u64 operator()(u64 a, u64 b) const {
    return (b & kSeg64) ? b : ((a & kSeg64) | ((a & ~kSeg64) + b));
  }
};
struct Add {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const {
    return a + b;
  }
};
struct Pair {
  u64 in, tgt;
};
struct PairAdd {
  __host__ __device__ __forceinline__ Pair operator()(const Pair& a, const Pair& b) const {
    return Pair{a.in + b.in, a.tgt + b.tgt};
  }
};

// Exclusive scan of one value per thread over the workgroup (0: op's identity); *total: all of them.
// s_wave: kThreads / 64 entries of LDS, free again on return.
template <class T, class Op>
__device__ __forceinline__ T block_scan(T v, Op op, T* s_wave, T* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(v, d, 64);
    if (lane >= d) v = op(o, v);
  }
  if (lane == 63) s_wave[w] = v;
  __syncthreads();
  T ex = __shfl_up(v, 1, 64);
  if (lane == 0) ex = T(0);
  T pre = T(0), all = T(0);
  for (int i = 0; i < kThreads / 64; ++i) {
    if (i < w) pre = op(pre, s_wave[i]);
    all = op(all, s_wave[i]);
  }
  *total = all;
  __syncthreads();
  return op(pre, ex);
}

// The row_off entries with a value in [lo, hi]: [s_q[0], s_q[1]).  Ends with a barrier.
__device__ __forceinline__ void tile_rows(const u64* __restrict__ row, u64 R, u64 lo, u64 hi, u64* s_q) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const u64 q0 = lo ? wave_upper_bound(row, 0, R + 1, lo - 1, lane) : 0;
    const u64 q1 = wave_upper_bound(row, q0, R + 1, hi, lane);
    if (lane == 0) s_q[0] = q0, s_q[1] = q1;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void k_corrupt_rows(const int64_t* __restrict__ row, u64 rows, u64 n,
                                                           u64* __restrict__ res) {
  const u64 r = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (r > rows) return;
  const int64_t v = row[r];
  const int64_t prev = r ? row[r - 1] : 0;
  if (v < 0 || (u64)v > n || prev > v || (r == 0 && v != 0) || (r == rows && (u64)v != n)) res[0] = 1;
}

// Four consecutive ids at g (cnt of them inside the array).
__device__ __forceinline__ void load_ids(const int32_t* p, u64 g, int cnt, bool vec, int32_t (&v)[kLane]) {
  if (vec && cnt == kLane) {
    const int4 w = *reinterpret_cast<const int4*>(p + g);
    v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
  } else {
#pragma unroll
    for (int i = 0; i < kLane; ++i) v[i] = i < cnt ? p[g + i] : 0;
  }
}

// flags: n rounded up to kLane bytes allocated; vec: ids may take 16-byte loads.
__global__ __launch_bounds__(kThreads) void k_corrupt_noise(const int32_t* __restrict__ ids, u64 n,
                                                            const u64* __restrict__ row, u64 R, CorruptRule rule,
                                                            uint32_t vec, uint8_t* __restrict__ flags,
                                                            u64* __restrict__ agg, const u64* __restrict__ res) {
  __shared__ uint8_t s_len[kHalo + kTile], s_beg[kHalo + kTile];  // entry kHalo is the tile's first position
  __shared__ u64 s_q[2];
  __shared__ uint32_t s_wave[kThreads / 64];
  if (res[0]) return;
  const int tid = threadIdx.x;
  const u64 tile0 = (u64)blockIdx.x * kTile;
  const int cnt = n - tile0 < (u64)kTile ? (int)(n - tile0) : kTile;
  tile_rows(row, R, tile0, tile0 + cnt - 1, s_q);
  for (int i = tid; i < kHalo + cnt; i += kThreads) {
    const u64 back = i < kHalo ? (u64)(kHalo - i) : 0;  // positions before the tile; those past len_n reach nothing
    s_len[i] = back <= tile0 && back <= rule.len_n ? (uint8_t)rule.span(tile0 + i - kHalo) : 0;
    s_beg[i] = 0;
  }
  __syncthreads();
  const u64 q0 = s_q[0], q1 = s_q[1];
  for (u64 q = q0 + tid; q < q1; q += kThreads) s_beg[row[q] - tile0 + kHalo] = 1;
  if (tid == 0 && q0 > 0) {  // the last row that begins before the tile: it ends the look-back
    const u64 gap = tile0 - row[q0 - 1];
    if (gap <= (u64)kHalo) s_beg[kHalo - (int)gap] = 1;
  }
  __syncthreads();
  const int g = tid * kLane;
  uint32_t seg = 0;
  if (g < cnt) {
    const int c = cnt - g < kLane ? cnt - g : kLane;
    int32_t id[kLane];
    load_ids(ids, tile0 + g, c, vec != 0, id);
    int reach = 0;      // furthest LDS index (exclusive) that a start of this row, seen so far, covers
    bool prev = false;  // the token before is noise
    if (tile0 + g > 0) {
      const int ip = kHalo + g - 1;
      for (int i = 0; i < (int)rule.len_n; ++i) {
        const int k = ip - i;
        const int L = s_len[k];
        if (L) reach = max(reach, k + L);
        if (s_beg[k]) break;
      }
      prev = reach > ip && !rule.guarded(ids[tile0 + g - 1]);
    }
    uint32_t out = 0;
#pragma unroll
    for (int t = 0; t < kLane; ++t) {
      if (t >= c) break;
      const int idx = kHalo + g + t;
      const bool beg = s_beg[idx] != 0;
      if (beg) reach = 0, prev = false;
      const int L = s_len[idx];
      if (L) reach = max(reach, idx + L);
      const bool noise = reach > idx && !rule.guarded(id[t]);
      const bool first = noise && !prev;
      prev = noise;
      out |= ((noise ? 1u : 0u) | (first ? 2u : 0u)) << (8 * t);
      seg = SegAdd32()(seg, (beg ? kSeg : 0u) | (first ? 1u : 0u));
    }
    *reinterpret_cast<uint32_t*>(flags + tile0 + g) = out;
  }
  uint32_t all;
  block_scan(seg, SegAdd32(), s_wave, &all);
  if (tid == 0) agg[blockIdx.x] = ((all & kSeg) ? kSeg64 : 0ull) | (u64)(all & ~kSeg);
}

// What a lane knows of its four tokens before the emit counts: the flags, how many are inside the
// array, and the runs of the row before the first of them.  mark[i] != 0: a row begins at the tile's
// position i.
struct Lane4 {
  uint32_t f;
  int c;
  u64 runs;
};

template <class M>
__device__ __forceinline__ Lane4 lane_runs(const uint8_t* __restrict__ flags, u64 tile0, int cnt, const M* mark,
                                           const u64* __restrict__ carry, uint32_t* s_wave) {
  const int g = threadIdx.x * kLane;
  Lane4 l{0, 0, 0};
  uint32_t seg = 0;
  if (g < cnt) {
    l.c = cnt - g < kLane ? cnt - g : kLane;
    l.f = *reinterpret_cast<const uint32_t*>(flags + tile0 + g);
    for (int t = 0; t < l.c; ++t) seg = SegAdd32()(seg, (mark[g + t] ? kSeg : 0u) | ((l.f >> (8 * t + 1)) & 1u));
  }
  uint32_t all;
  const uint32_t ex = block_scan(seg, SegAdd32(), s_wave, &all);
  const u64 before = blockIdx.x ? carry[blockIdx.x - 1] & ~kSeg64 : 0;  // runs of the row before the tile
  l.runs = (ex & kSeg) ? (u64)(ex & ~kSeg) : before + ex;
  return l;
}

__global__ __launch_bounds__(kThreads) void k_corrupt_count(u64 n, const u64* __restrict__ row, u64 R, u64 rmax,
                                                            const uint8_t* __restrict__ flags,
                                                            const u64* __restrict__ carry, Pair* __restrict__ tot,
                                                            const u64* __restrict__ res) {
  __shared__ uint8_t s_beg[kTile];
  __shared__ u64 s_q[2];
  __shared__ uint32_t s_wave[kThreads / 64];
  if (res[0]) return;
  const int tid = threadIdx.x;
  const u64 tile0 = (u64)blockIdx.x * kTile;
  const int cnt = n - tile0 < (u64)kTile ? (int)(n - tile0) : kTile;
  *reinterpret_cast<uint32_t*>(s_beg + tid * kLane) = 0;
  tile_rows(row, R, tile0, tile0 + cnt - 1, s_q);
  for (u64 q = s_q[0] + tid; q < s_q[1]; q += kThreads) s_beg[row[q] - tile0] = 1;
  __syncthreads();
  const Lane4 l = lane_runs(flags, tile0, cnt, s_beg, carry, s_wave);
  u64 runs = l.runs;
  uint32_t emit = 0;  // input ids | target ids << 16
  for (int t = 0; t < l.c; ++t) {
    if (s_beg[tid * kLane + t]) runs = 0;
    const bool noise = (l.f >> (8 * t)) & 1u, first = (l.f >> (8 * t + 1)) & 1u;
    runs += first;
    const bool gone = noise && runs <= rmax;  // rank = runs - 1 < Rmax
    emit += (!gone || first ? 1u : 0u) + (gone ? (first ? 2u : 1u) << 16 : 0u);
  }
  uint32_t all;
  block_scan(emit, Add(), s_wave, &all);
  if (tid == 0) tot[blockIdx.x] = Pair{all & 0xFFFFu, all >> 16};
}

// res[1] = T_in, res[2] = T_tgt (base: the inclusive sums of the tiles' pairs; closing: rows x fin).
__global__ void k_corrupt_result(const Pair* __restrict__ base, u64 tiles, u64 closing, u64* __restrict__ res) {
  res[1] = tiles ? base[tiles - 1].in : 0;
  res[2] = (tiles ? base[tiles - 1].tgt : 0) + closing;
}

// One workgroup per tile, and one for n == 0 (the rows' offsets and closing sentinels).  in_src may
// be nullptr.  src0: added to every in_src; in0 / tgt0: added to every offset written to in_row /
// tgt_row (a piece of the host call; its ids go to the piece's own buffers at 0).
__global__ __launch_bounds__(kThreads) void k_corrupt_scatter(
    const int32_t* __restrict__ ids, u64 n, const u64* __restrict__ row, u64 R, CorruptRule rule, uint32_t vec,
    const uint8_t* __restrict__ flags, const u64* __restrict__ carry, const Pair* __restrict__ base, u64 src0, u64 in0,
    u64 tgt0, int32_t* __restrict__ in_ids, int64_t* __restrict__ in_src, int32_t* __restrict__ tgt_ids,
    int64_t* __restrict__ in_row, int64_t* __restrict__ tgt_row, const u64* __restrict__ res) {
  __shared__ unsigned long long s_nb[kTile + 1];       // row_off entries at each position (kTile: at n, last tile)
  __shared__ uint32_t s_in[kTile + 1], s_tg[kTile + 1];  // emitted before the position, within the tile
  __shared__ uint32_t s_j[kTile];                      // corrupted runs of the row up to and with the position
  __shared__ u64 s_q[2];
  __shared__ u64 s_wave64[kThreads / 64];
  __shared__ uint32_t s_wave[kThreads / 64];
  if (res[0]) return;
  const int tid = threadIdx.x;
  const u64 tile0 = (u64)blockIdx.x * kTile;
  const int cnt = n <= tile0 ? 0 : n - tile0 < (u64)kTile ? (int)(n - tile0) : kTile;
  const bool last = blockIdx.x == gridDim.x - 1;
  for (int i = tid; i <= kTile; i += kThreads) s_nb[i] = 0;
  tile_rows(row, R, tile0, last ? ~0ull : tile0 + kTile - 1, s_q);
  const u64 q0 = s_q[0], q1 = s_q[1];
  for (u64 q = q0 + tid; q < q1; q += kThreads) atomicAdd(&s_nb[row[q] - tile0], 1ull);
  __syncthreads();
  const Lane4 l = lane_runs(flags, tile0, cnt, s_nb, carry, s_wave);
  const int g = tid * kLane;
  u64 nb = 0;
  for (int t = 0; t < l.c; ++t) nb += s_nb[g + t];
  u64 nb_all;
  u64 rows_to = q0 + block_scan(nb, Add(), s_wave64, &nb_all);  // row_off entries at or before the token
  u64 runs = l.runs;
  uint32_t emit = 0, kind = 0;  // kind: per token, 1 gone | 2 first
  u64 rank[kLane] = {};
  for (int t = 0; t < l.c; ++t) {
    if (s_nb[g + t]) runs = 0;
    const bool noise = (l.f >> (8 * t)) & 1u, first = (l.f >> (8 * t + 1)) & 1u;
    runs += first;
    const bool gone = noise && runs <= rule.rmax;
    emit += (!gone || first ? 1u : 0u) + (gone ? (first ? 2u : 1u) << 16 : 0u);
    kind |= ((gone ? 1u : 0u) | (first ? 2u : 0u)) << (8 * t);
    rank[t] = runs - 1;
    s_j[g + t] = (uint32_t)(runs < rule.rmax ? runs : rule.rmax);
  }
  uint32_t all;
  const uint32_t ex = block_scan(emit, Add(), s_wave, &all);
  const u64 b_in = blockIdx.x ? base[blockIdx.x - 1].in : 0, b_tg = blockIdx.x ? base[blockIdx.x - 1].tgt : 0;
  uint32_t li = ex & 0xFFFFu, lt = ex >> 16;
  if (l.c) {
    int32_t id[kLane];
    load_ids(ids, tile0 + g, l.c, vec != 0, id);
    for (int t = 0; t < l.c; ++t) {
      rows_to += s_nb[g + t];
      s_in[g + t] = li, s_tg[g + t] = lt;
      const bool gone = (kind >> (8 * t)) & 1u, first = (kind >> (8 * t + 1)) & 1u;
      if (!gone || first) {
        in_ids[b_in + li] = gone ? rule.sentinel(rank[t]) : id[t];
        if (in_src) in_src[b_in + li] = (int64_t)(src0 + tile0 + g + t);
        ++li;
      }
      if (gone) {
        const u64 at = b_tg + lt + (rule.fin ? rows_to - 1 : 0);  // the rows before close with one sentinel each
        if (first) tgt_ids[at] = rule.sentinel(rank[t]);
        tgt_ids[at + (first ? 1 : 0)] = id[t];
        lt += first ? 2u : 1u;
      }
    }
    if (g + l.c == cnt) s_in[cnt] = li, s_tg[cnt] = lt;
  }
  if (cnt == 0 && tid == 0) s_in[0] = 0, s_tg[0] = 0;
  __syncthreads();
  const u64 before = blockIdx.x ? carry[blockIdx.x - 1] & ~kSeg64 : 0;
  for (u64 q = q0 + tid; q < q1; q += kThreads) {
    const u64 p = row[q];
    const int i = (int)(p - tile0);
    in_row[q] = (int64_t)(in0 + b_in + s_in[i]);
    const u64 to = tgt0 + b_tg + s_tg[i] + (rule.fin ? q : 0);
    tgt_row[q] = (int64_t)to;
    if (rule.fin && q) {  // row q - 1 ends here: its closing sentinel, after its J corrupted runs
      u64 J = 0;
      if (row[q - 1] < p) J = i ? s_j[i - 1] : (before < rule.rmax ? before : rule.rmax);
      tgt_ids[to - tgt0 - 1] = rule.sentinel(J);
    }
  }
}

// One call's (or piece's) ids as the passes take them; every pointer on the device.
struct CorruptCall {
  const int32_t* ids;
  u64 n;
  const int64_t* row;  // R + 1 entries
  u64 R;
  CorruptRule rule;
  u64 src0, in0, tgt0;
  int32_t* in_ids;
  int64_t* in_src;
  int32_t* tgt_ids;
  int64_t *in_row, *tgt_row;
};

// The corruption passes' state, allocated on the first corrupt call: the result words, the flags
// and the tiles' words grown to the most ids seen, and the staging of the host path.
struct CorruptState : PassState {
  DeviceWords res;            // [0] a bad row_off, [1] T_in, [2] T_tgt
  PinnedWords host;           // the three; [3], [4]: the offsets {0, n} of a call without row_off
  EventSet<4> ev;
  DeviceBuf<int64_t> one;     // those offsets on the device
  DeviceBuf<uint8_t> flags;   // 1 B per id
  DeviceBuf<u64> agg;         // per tile: the aggregate, then the scanned carry
  DeviceBuf<Pair> tot;        // per tile: the emit counts, then their inclusive sums
  DeviceBuf<uint8_t> tmp;     // hipCUB scan scratch
  DeviceBuf<int32_t> hids, hin, htgt;  // host path: a piece's ids and its two streams
  DeviceBuf<int64_t> hsrc, hrow;       // in_src; the piece's row_off, in_row_off and tgt_row_off (3 x hrow.cap())

  bool reserve(size_t) { return res.ensure(3) && host.ensure(5) && ev.ensure() && one.grow(2); }

  static u64 tiles_of(u64 n) { return (n + kTile - 1) / kTile; }

  bool reserve_ids(size_t n) {
    const size_t tiles = std::max<size_t>(tiles_of(n), 1);
    if (!flags.grow(n + kLane) || !agg.grow(tiles, 2) || !tot.grow(tiles, 2)) return false;
    size_t a = 0, b = 0;
    if (hipcub::DeviceScan::InclusiveScan(nullptr, a, agg.get(), agg.get() + agg.cap(), SegAdd64(), (u64)tiles) !=
            hipSuccess ||
        hipcub::DeviceScan::InclusiveScan(nullptr, b, tot.get(), tot.get() + tot.cap(), PairAdd(), (u64)tiles) !=
            hipSuccess)
      return false;
    return tmp.grow(std::max<size_t>(std::max(a, b), 16));
  }

  // Without a row_off: one row of all ids.
  int one_row(u64 n, hipStream_t st) {
    host[3] = 0, host[4] = n;
    ENC_OK(hipMemcpyAsync(one.get(), host.get() + 3, 16, hipMemcpyHostToDevice, st));
    return 0;
  }

  // The passes up to the counts, which are in `host` when it returns: 0 or -1.  check: row is the
  // caller's and has not been validated.
  int measure(const CorruptCall& c, bool check, hipStream_t st) {
    ENC_OK(hipMemsetAsync(res.get(), 0, 24, st));
    if (check) {
      k_corrupt_rows<<<dim3((unsigned)((c.R + kThreads) / kThreads)), dim3(kThreads), 0, st>>>(c.row, c.R, c.n,
                                                                                                  res.get());
      ENC_OK(hipGetLastError());
    }
    const u64 tiles = tiles_of(c.n);
    u64* const carry = agg.get() + agg.cap();
    Pair* const base = tot.get() + tot.cap();
    const u64* const row = reinterpret_cast<const u64*>(c.row);
    if (tiles) {
      k_corrupt_noise<<<dim3((unsigned)tiles), dim3(kThreads), 0, st>>>(c.ids, c.n, row, c.R, c.rule,
                                                                        aligned16(c.ids) ? 1u : 0u, flags.get(),
                                                                        agg.get(), res.get());
      ENC_OK(hipGetLastError());
      size_t bytes = tmp.cap();
      ENC_OK(hipcub::DeviceScan::InclusiveScan(tmp.get(), bytes, agg.get(), carry, SegAdd64(), tiles, st));
      k_corrupt_count<<<dim3((unsigned)tiles), dim3(kThreads), 0, st>>>(c.n, row, c.R, c.rule.rmax, flags.get(), carry,
                                                                        tot.get(), res.get());
      ENC_OK(hipGetLastError());
      bytes = tmp.cap();
      ENC_OK(hipcub::DeviceScan::InclusiveScan(tmp.get(), bytes, tot.get(), base, PairAdd(), tiles, st));
    }
    k_corrupt_result<<<dim3(1), dim3(1), 0, st>>>(base, tiles, c.rule.fin ? c.R : 0, res.get());
    ENC_OK(hipGetLastError());
    ENC_OK(hipMemcpyAsync(host.get(), res.get(), 24, hipMemcpyDeviceToHost, st));
    ENC_OK(hipStreamSynchronize(st));
    return 0;
  }

  // The outputs, after measure() on the same call: 0 or -1.
  int scatter(const CorruptCall& c, hipStream_t st) {
    const u64 tiles = std::max<u64>(tiles_of(c.n), 1);
    k_corrupt_scatter<<<dim3((unsigned)tiles), dim3(kThreads), 0, st>>>(
        c.ids, c.n, reinterpret_cast<const u64*>(c.row), c.R, c.rule, aligned16(c.ids) ? 1u : 0u, flags.get(),
        agg.get() + agg.cap(), tot.get() + tot.cap(), c.src0, c.in0, c.tgt0, c.in_ids, c.in_src, c.tgt_ids, c.in_row,
        c.tgt_row, res.get());
    ENC_OK(hipGetLastError());
    return 0;
  }

  // Staging of a piece of len ids and m rows.
  bool stage(size_t len, size_t m, bool src) {
    return reserve_ids(len) && hids.grow(std::max<size_t>(len, 1)) && hin.grow(std::max<size_t>(len, 1)) &&
           htgt.grow(2 * len + m) && (!src || hsrc.grow(std::max<size_t>(len, 1))) && hrow.grow(m + 1, 3);
  }
};

}  // namespace

int64_t EncodeDevice::corrupt(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const CorruptOpts& o,
                              int32_t* in_ids, size_t in_cap, int64_t* in_row_off, int64_t* in_src, int32_t* tgt_ids,
                              size_t tgt_cap, int64_t* tgt_row_off, size_t* tgt_n, void* stream, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  if (!tiles_fit(n)) return -1;
  const u64 R = row_off ? rows : 1;
  CorruptCall c{ids, n, row_off, R, rule_of(o, 0), 0, 0, 0, in_ids, in_src, tgt_ids, in_row_off, tgt_row_off};
  return device_call<CorruptState>(
      pass_[kCorrupt], device_, stream ? stream : stream_, "corrupt", R, kernel_ms,
      [&](CorruptState& cs, hipStream_t st, Plan* p) {
        if (!cs.reserve_ids(n)) {
          std::fprintf(stderr, "[ERROR]\t encoder: corrupt allocation failed (%zu ids)\n", n);
          return -1;
        }
        if (!row_off) {
          if (cs.one_row(n, st) < 0) return -1;
          c.row = cs.one.get();
        }
        if (cs.measure(c, row_off != nullptr, st) < 0) return -1;
        if (cs.host[0]) return -6;
        if (tgt_n) *tgt_n = (size_t)cs.host[2];
        *p = Plan{(int64_t)cs.host[1], in_ids && tgt_ids && in_cap >= cs.host[1] && tgt_cap >= cs.host[2], n};
        return 0;
      },
      [&](CorruptState& cs, hipStream_t st) { return cs.scatter(c, st); });
}

// Host ids in pieces of whole rows (piece_end).  A piece is the device passes on its own ids at
// index_base + the index of its first id; its two streams land in the piece's staging at 0 and are
// copied behind the earlier pieces', and its offsets and in_src are written with the piece's bases
// added.  The caller has validated row_off.  Caps that hold the bound (n and 2 n + rows) need one
// round; smaller ones a round of counts first, so that nothing is written when they do not suffice.
int64_t EncodeDevice::corrupt_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows,
                                   const CorruptOpts& o, int32_t* in_ids, size_t in_cap, int64_t* in_row_off,
                                   int64_t* in_src, int32_t* tgt_ids, size_t tgt_cap, int64_t* tgt_row_off,
                                   size_t* tgt_n) {
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  CorruptState& cs = pass_state<CorruptState>(pass_[kCorrupt]);
  if (!cs.reserve(0)) {
    std::fprintf(stderr, "[ERROR]\t encoder: corrupt allocation failed\n");
    return -1;
  }
  hipStream_t st = (hipStream_t)stream_;
  const size_t R = row_off ? rows : 1, piece = piece_ids();
  const HostIn in{ids, n, row_off};
  std::vector<int64_t> local;
  u64 t_in = 0, t_tgt = 0;
  const auto round = [&](bool write) -> int {
    t_in = t_tgt = 0;
    for (size_t r0 = 0; r0 < R;) {
      u64 emitted = 0;
      const size_t r1 = piece_end(&in, 1, R, r0, piece, 0, [](size_t) { return (u64)0; }, &emitted, nullptr);
      const size_t a = row_off ? (size_t)row_off[r0] : 0, len = (row_off ? (size_t)row_off[r1] : n) - a, m = r1 - r0;
      if (!tiles_fit(len) || !cs.stage(len, m, write && in_src)) {
        std::fprintf(stderr, "[ERROR]\t encoder: corrupt staging allocation failed (%zu ids, %zu rows)\n", len, m);
        return -1;
      }
      int64_t *const drow = cs.hrow.get(), *const din_row = drow + cs.hrow.cap(), *const dtgt_row = din_row + cs.hrow.cap();
      if (len) ENC_OK(hipMemcpyAsync(cs.hids.get(), ids + a, len * 4, hipMemcpyHostToDevice, st));
      local.resize(m + 1);
      for (size_t i = 0; i <= m; ++i) local[i] = row_off ? row_off[r0 + i] - (int64_t)a : (int64_t)(i ? n : 0);
      ENC_OK(hipMemcpyAsync(drow, local.data(), (m + 1) * 8, hipMemcpyHostToDevice, st));
      const CorruptCall c{cs.hids.get(), len, drow, m, rule_of(o, a), a, t_in, t_tgt, cs.hin.get(),
                          write && in_src ? cs.hsrc.get() : nullptr, cs.htgt.get(), din_row, dtgt_row};
      if (cs.measure(c, false, st) < 0) return -1;
      const u64 p_in = cs.host[1], p_tgt = cs.host[2];
      if (write) {
        if (cs.scatter(c, st) < 0) return -1;
        if (p_in) ENC_OK(hipMemcpyAsync(in_ids + t_in, cs.hin.get(), p_in * 4, hipMemcpyDeviceToHost, st));
        if (p_in && in_src) ENC_OK(hipMemcpyAsync(in_src + t_in, cs.hsrc.get(), p_in * 8, hipMemcpyDeviceToHost, st));
        if (p_tgt) ENC_OK(hipMemcpyAsync(tgt_ids + t_tgt, cs.htgt.get(), p_tgt * 4, hipMemcpyDeviceToHost, st));
        ENC_OK(hipMemcpyAsync(in_row_off + r0, din_row, (m + 1) * 8, hipMemcpyDeviceToHost, st));
        ENC_OK(hipMemcpyAsync(tgt_row_off + r0, dtgt_row, (m + 1) * 8, hipMemcpyDeviceToHost, st));
        ENC_OK(hipStreamSynchronize(st));
      }
      t_in += p_in, t_tgt += p_tgt;
      r0 = r1;
    }
    return 0;
  };
  const bool write = in_ids && tgt_ids;
  if (!(write && in_cap >= n && tgt_cap >= 2 * (u64)n + R)) {
    if (round(false) < 0) return -1;
    if (tgt_n) *tgt_n = (size_t)t_tgt;
    if (!write || in_cap < t_in || tgt_cap < t_tgt) return (int64_t)t_in;
  }
  if (round(true) < 0) return -1;
  if (tgt_n) *tgt_n = (size_t)t_tgt;
  return (int64_t)t_in;
}

}  // namespace shred
