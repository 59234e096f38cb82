// Exact dedup of whole rows of ids on gfx950: a 64-bit fingerprint of every row, and the first occurrence of
// every fingerprint across the calls since a reset, beside MinHash, dedup, overlap and repeat (C ABI and
// definitions: include/shredword_encode.h, shred_exact_*).  The unit shares the seeded draw and the per-id
// value g of the overlap fingerprint (ngram_print.h), the batch units' wave search (batch_common.h), their
// device-call driver and host piece loop (batch_state.h) and the offset check (encode_common.h).
//
//   k_exact_rows      row_off, and the rows of the call that are compared (a ballot, one atomic per wave), before
//                     anything is written; grp_off goes through k_offsets_check.
//   k_exact_print     the row sums S = sum A^(len-1-j) g(t[j]) as a segmented scan over the flat id stream with
//                     the monoid (P, S), (P1, S1) o (P2, S2) = (P1 P2, S1 P2 + S2), an id entering as (A, g(t)) and
//                     a row start as a flag that drops what lies to its left.  P carries A^len, so no thread ever
//                     raises A to a power.  One workgroup per kExTile = 2304 consecutive ids, whatever the rows
//                     are: a million one-id rows and one row of a million ids load the machine alike.
//     ids             read once, coalesced, into LDS as int32.
//     rows            wave 0 finds the row of the tile's first id and the row_off entries up to its last with two
//                     wave_upper_bound searches; the ends of those rows, relative to the tile, are staged in LDS
//                     (the first kExRows; a tile with more, which takes a thousand empty or short rows, reads the
//                     others from row_off), as k_overlap_tiles does.
//     strips          a thread folds kExStrip = 9 consecutive ids in registers: two mixes for g, a multiply-add
//                     for S, a multiply for P, restarting at a row start.  Nine: a wave's 4-byte LDS reads at a
//                     stride of 9 words fall on banks 9 l mod 64, pairwise distinct over the 64 lanes because 9 is
//                     odd, where strips of 8 would put them 8 deep; 256 x 9 = 2304 ids of 9 KB.  A row that starts
//                     and ends inside a strip is finished there.  Of the rows that end in a strip, only the first
//                     can have started to its left: the thread keeps its (P, S).
//     combine         the strips' (P, S, flag) go through an inclusive scan over the wave by shuffles (six steps,
//                     two multiplies each), the four wave totals through LDS.  A thread's exclusive prefix
//                     finishes its kept row when the row started inside the tile; when it did not, the pair is the
//                     tile's open head.  Per tile the carry arrays get that head (P, S, row) and the tile's total
//                     (P, S, flag): its open tail, or, without a row start, all of it.
//   k_exact_carry     rows that cross tile edges: one workgroup scans the tiles' totals with the same operator,
//                     8 consecutive tiles per thread and 2048 per round, the running prefix kept in registers,
//                     and finishes every tile's head with the prefix to its left.  A row over a thousand tiles
//                     costs what a thousand rows do.  (A decoupled look-back inside k_exact_print was not built:
//                     n / 2304 carries are 0.04 % of the stream.)
//   k_exact_insert    over rows: an empty row gets its F here, without an id being read.  The slot comes from F
//                     (already a mix), linear probing; a free slot is claimed by a 64-bit compare-and-swap of its
//                     key and the row's global index goes in by a 64-bit atomicMin, so `first` does not depend on
//                     scheduling.  With g_in_rows the row goes in a second time under F2.  New keys are summed
//                     over the wave: one atomic.
//   k_exact_resolve   behind the whole insert pass: reads the minimum, writes first, dup and print, counts the
//                     duplicates (a ballot, one atomic per wave) and adds the group counts with one atomic per
//                     run of rows of one group within a wave (a segmented sum by shuffles; a thread finds its
//                     group by a binary search of grp_off).
//
// The table: slots = the power of two >= 2 x capacity, u64 keys (all-ones: free) and u64 smallest global indices
// in two arrays, 16 bytes a slot; at most `capacity` keys, so it is never more than half full and every probe
// ends.  It lives in the pass's state from one shred_exact_reset to the next.
//
// LDS per workgroup of k_exact_print: 9 KB of ids, 4 KB of row ends, 0.1 KB of wave totals: 13.1 KB.  Traffic per
// id: 4 B read, once; per row 16 B of offsets read and 8 B of F written, then two random 16-byte slot accesses
// (atomics on insert) and 17 B of outputs; per tile 48 B of carries.  No matrix instruction fits: 64-bit
// integer multiply-adds, a mix, atomics.  All global indices are 64-bit; a row may hold more than 2^32 ids.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../host/encoder.h"
#include "batch_common.h"
#include "batch_state.h"
#include "encode_common.h"
#include "ngram_print.h"

namespace shred {
namespace {

constexpr int kExStrip = 9;                     // consecutive ids per thread of k_exact_print (EXACT_STRIP)
constexpr int kExTile = kThreads * kExStrip;    // ids per workgroup (EXACT_TILE)
constexpr int kExRows = 1024;                   // row ends staged in LDS
constexpr int kExFar = 1 << 20;                 // a row end past everything the tile holds
constexpr int kExCarryStrip = 8;                // consecutive tiles per thread of k_exact_carry
constexpr u64 kExNone = ~0ull;                  // no row; a free slot's key (kOvFree) and index
static_assert(kExStrip % 2 == 1 && kExTile < kExFar, "odd strips: conflict-free LDS reads");

// The definition's pieces, for the kernels and the asserts below (g is overlap's ov_g).
constexpr __host__ __device__ u64 ex_mult(u64 seed) { return ov_mult(seed, 0); }
constexpr __host__ __device__ u64 ex_print(u64 seed, u64 S, u64 len) { return ov_print(S ^ draw(seed, len, kRow)); }
constexpr __host__ __device__ u64 ex_print2(u64 seed, u64 F, u64 group) { return ov_print(F ^ draw(seed, group, kGroup)); }
// Values of the definition as the tests' numpy reference computes it, under seed 3: the multiplier, the empty
// row, the rows [7] and [7, -1, 5], and the last as a row of group 9.
constexpr u64 ex_three(u64 seed, int32_t a, int32_t b, int32_t c) {
  return ex_print(seed, (ov_g(seed, a) * ex_mult(seed) + ov_g(seed, b)) * ex_mult(seed) + ov_g(seed, c), 3);
}
static_assert(ex_mult(3) == 0x2bb4af56486e8645ull && ex_print(3, 0, 0) == 0xfd0970679625c4f0ull, "exact");
static_assert(ex_print(3, ov_g(3, 7), 1) == 0xedba4ce2cb4e38d2ull && ex_three(3, 7, -1, 5) == 0xb9775c809efaf800ull, "exact");
static_assert(ex_print2(3, ex_three(3, 7, -1, 5), 9) == 0x537ed3aa7b05d282ull, "exact");

// What the kernels know of the state; passed by value.
struct ExRule {
  u64 seed, A, min_len;
};

struct ExTable {
  u64 *key, *idx;
  u64 mask;  // slots - 1
};

// Per tile: the fold of its ids behind its last row start (flag 1) or of all of them (flag 0), and the
// fold of the ids of the row that started before the tile and ends in it (row: kExNone without one).
struct ExCarry {
  u64 *aggP, *aggS, *aggF, *headP, *headS, *headRow;
};

// What a call writes; every pointer but first may be nullptr.
struct ExOut {
  int64_t* first;
  uint8_t* dup;
  u64* print;
  unsigned long long *g_dup_rows, *g_dup_ids, *g_in_rows;
};

// An element of the segmented scan: the fold (P, S) of a run of ids and whether a row starts in the run.
struct Seg {
  u64 P, S;
  int f;
};
constexpr Seg kSegOne{1, 0, 0};
__device__ __forceinline__ Seg seg_op(const Seg& a, const Seg& b) {
  return b.f ? b : Seg{a.P * b.P, a.S * b.P + b.S, a.f};
}
__device__ __forceinline__ Seg seg_up(const Seg& v, int d) {
  return Seg{(u64)__shfl_up((unsigned long long)v.P, d), (u64)__shfl_up((unsigned long long)v.S, d), __shfl_up(v.f, d)};
}

// The exclusive prefix of v over the workgroup's 256 threads, and *total of all of them.  s_w: four entries of
// LDS, free again on return.  Every thread calls it.
__device__ __forceinline__ Seg seg_scan(Seg v, Seg* s_w, Seg* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const Seg o = seg_up(v, d);
    if (lane >= d) v = seg_op(o, v);
  }
  if (lane == 63) s_w[wave] = v;
  Seg ex = seg_up(v, 1);
  if (lane == 0) ex = kSegOne;
  __syncthreads();
  Seg pre = kSegOne, all = kSegOne;
  for (int k = 0; k < kThreads / 64; ++k) {
    if (k < wave) pre = seg_op(pre, s_w[k]);
    all = seg_op(all, s_w[k]);
  }
  __syncthreads();
  *total = all;
  return seg_op(pre, ex);
}

// res[0] = 1 for a bad row_off; res[2] += the rows of at least min_len ids.
__global__ __launch_bounds__(kRowThreads) void k_exact_rows(const int64_t* __restrict__ row, u64 rows, u64 n, u64 min_len,
                                                            u64* __restrict__ res) {
  const u64 i = (u64)blockIdx.x * kRowThreads + threadIdx.x;
  if (i <= rows && offset_bad(row, i, rows, n, true)) res[0] = 1;
  const u64 cmp = __ballot(i < rows && (u64)row[i + 1] - (u64)row[i] >= min_len);
  if ((threadIdx.x & 63) == 0 && cmp) atomicAdd((unsigned long long*)res + 2, (unsigned long long)__popcll(cmp));
}

// Ids [0, n) of the stream, n >= 1; row: rows + 1 good offsets.  F[r] of every non-empty row that ends in
// the tile it started in; the carries of the others.  c.headRow was preset to kExNone.
__global__ __launch_bounds__(kThreads) void k_exact_print(const int32_t* __restrict__ ids, u64 n,
                                                          const int64_t* __restrict__ row, u64 rows, ExRule q,
                                                          u64* __restrict__ F, ExCarry c) {
  __shared__ int32_t s_id[kExTile];
  __shared__ int s_end[kExRows];
  __shared__ u64 s_k[2];
  __shared__ Seg s_w[kThreads / 64];
  const int tid = threadIdx.x;
  const u64 t0 = (u64)blockIdx.x * kExTile;
  const int Tn = (int)(n - t0 < (u64)kExTile ? n - t0 : (u64)kExTile);
  for (int i = tid; i < Tn; i += kThreads) s_id[i] = ids[t0 + (u64)i];
  if (tid < 64) {
    // rows [ks, kend) hold the tile's ids or are empty rows among them: ks is the last k with row[k] <= t0
    // (row[0] = 0 and row[rows] = n > t0, so 0 <= ks < rows), kend the number of entries at or before the last
    // id (<= rows, as row[rows] = n lies past it)
    const u64* E = reinterpret_cast<const u64*>(row);
    const u64 ub = wave_upper_bound(E, 0, rows + 1, t0, tid);
    const u64 ue = wave_upper_bound(E, ub, rows + 1, t0 + (u64)Tn - 1, tid);
    if (tid == 0) s_k[0] = ub - 1, s_k[1] = ue;
  }
  __syncthreads();
  const u64 ks = s_k[0];
  const u64 nrows64 = s_k[1] - ks;  // >= 1; not bounded by the tile: empty rows
  // the end of row ks + i, relative to t0, at most kExFar; i < nrows64, so ks + i + 1 <= rows
  const auto far_end = [&](u64 i) {
    const u64 e = (u64)row[ks + i + 1] - t0;
    return (int)(e < (u64)kExFar ? e : (u64)kExFar);
  };
  const int staged = nrows64 < (u64)kExRows ? (int)nrows64 : kExRows;
  for (int i = tid; i < staged; i += kThreads) s_end[i] = far_end((u64)i);
  __syncthreads();
  const auto end_of = [&](u64 i) { return i < (u64)staged ? s_end[i] : far_end(i); };
  const auto finish = [&](u64 r, u64 S) { F[r] = ex_print(q.seed, S, (u64)row[r + 1] - (u64)row[r]); };

  const int p0 = tid * kExStrip, p1 = p0 + kExStrip < Tn ? p0 + kExStrip : Tn;
  Seg v = kSegOne;
  u64 keptP = 0, keptS = 0, kept = kExNone;  // the first row that ends in the strip, when it began to the left
  if (p0 < Tn) {
    u64 x = 0, y = nrows64 - 1;  // the first row that ends past p0: row nrows64 - 1 ends past Tn - 1
    while (x < y) {
      const u64 mid = (x + y) >> 1;
      if (end_of(mid) > p0) y = mid; else x = mid + 1;
    }
    u64 i = x;
    int e = end_of(x);
    // row i starts where the row before it ends; row ks at or before the tile's first id
    bool fresh = (i ? end_of(i - 1) : (row[ks] == (int64_t)t0 ? 0 : -1)) == p0;
    for (int p = p0; p < p1; ++p) {
      if (p >= e) {
        do e = end_of(++i); while (p >= e);  // ends at the row of Tn - 1 at the latest
        fresh = true;
      }
      if (fresh) v = Seg{1, 0, 1}, fresh = false;
      v.S = v.S * q.A + ov_g(q.seed, s_id[p]);
      v.P *= q.A;
      if (p + 1 == e) {  // row ks + i ends here
        if (v.f) finish(ks + i, v.S);
        else keptP = v.P, keptS = v.S, kept = ks + i;
      }
    }
  }
  Seg all;
  const Seg ex = seg_scan(v, s_w, &all);
  if (kept != kExNone) {
    const u64 S = ex.S * keptP + keptS;
    if (ex.f) {
      finish(kept, S);
    } else {
      c.headP[blockIdx.x] = ex.P * keptP, c.headS[blockIdx.x] = S, c.headRow[blockIdx.x] = kept;
    }
  }
  if (tid == 0) c.aggP[blockIdx.x] = all.P, c.aggS[blockIdx.x] = all.S, c.aggF[blockIdx.x] = (u64)all.f;
}

// One workgroup: F[r] of every row that ends in another tile than it started in.
__global__ __launch_bounds__(kThreads) void k_exact_carry(ExCarry c, u64 tiles, const int64_t* __restrict__ row, ExRule q,
                                                          u64* __restrict__ F) {
  __shared__ Seg s_w[kThreads / 64];
  const auto agg = [&](u64 t) { return Seg{c.aggP[t], c.aggS[t], (int)c.aggF[t]}; };
  Seg run = kSegOne;  // of the tiles before this round
  for (u64 base = 0; base < tiles; base += (u64)kThreads * kExCarryStrip) {
    const u64 t = base + (u64)threadIdx.x * kExCarryStrip;
    Seg v = kSegOne;
    for (int j = 0; j < kExCarryStrip; ++j)
      if (t + j < tiles) v = seg_op(v, agg(t + j));
    Seg all;
    Seg ex = seg_op(run, seg_scan(v, s_w, &all));
    for (int j = 0; j < kExCarryStrip && t + j < tiles; ++j) {
      const u64 r = c.headRow[t + j];
      if (r != kExNone) F[r] = ex_print(q.seed, ex.S * c.headP[t + j] + c.headS[t + j], (u64)row[r + 1] - (u64)row[r]);
      ex = seg_op(ex, agg(t + j));
    }
    run = seg_op(run, all);
  }
}

// The slot of key f, claimed when it was free (*claims counts those).
__device__ __forceinline__ u64 ex_claim(const ExTable& tab, u64 f, u64* claims) {
  u64 slot = f & tab.mask;
  for (;;) {
    u64 cur = __hip_atomic_load(tab.key + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kOvFree && __hip_atomic_compare_exchange_strong(tab.key + slot, &cur, f, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                               __HIP_MEMORY_SCOPE_AGENT)) {
      ++*claims;
      return slot;
    }
    if (cur == f) return slot;  // (on failure cur is the key that won the slot)
    slot = (slot + 1) & tab.mask;
  }
}

// The smallest index under key f, which an insert pass put there.
__device__ __forceinline__ u64 ex_first(const ExTable& tab, u64 f) {
  u64 slot = f & tab.mask;
  for (;;) {
    const u64 cur = tab.key[slot];
    if (cur == f || cur == kOvFree) return tab.idx[slot];
    slot = (slot + 1) & tab.mask;
  }
}

// What the row kernels know of a call or a piece of one: its R rows are the rows r0 .. of the call, which have
// the global indices base + r0 ..; grp (nullptr: no groups) holds the call's G + 1 offsets into its rows, and
// the call's group 0 has the global index gbase.
struct ExRows {
  const int64_t* row;
  u64 R, r0, base;
  const int64_t* grp;
  u64 G, gbase;
  bool in_group;
};

// The group of the call's row r: the one q with grp[q] <= r < grp[q + 1] (groups may be empty).
__device__ __forceinline__ u64 ex_group(const ExRows& w, u64 r) {
  u64 lo = 0, hi = w.G;  // the first q with grp[q + 1] > r; grp[G] = the call's rows > r
  while (lo < hi) {
    const u64 mid = (lo + hi) >> 1;
    if ((u64)w.grp[mid + 1] > r) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// res[3] += the keys that are new.
__global__ __launch_bounds__(kRowThreads) void k_exact_insert(ExRows w, ExRule q, ExTable tab, u64* __restrict__ F,
                                                              u64* __restrict__ res) {
  const u64 r = (u64)blockIdx.x * kRowThreads + threadIdx.x;
  u64 claims = 0;
  if (r < w.R) {
    const u64 len = (u64)w.row[r + 1] - (u64)w.row[r];
    if (!len) F[r] = ex_print(q.seed, 0, 0);
    if (len >= q.min_len) {
      const u64 f = F[r], at = w.base + w.r0 + r;
      atomicMin((unsigned long long*)tab.idx + ex_claim(tab, f, &claims), (unsigned long long)at);
      if (w.in_group) {
        const u64 f2 = ex_print2(q.seed, f, w.gbase + ex_group(w, w.r0 + r));
        atomicMin((unsigned long long*)tab.idx + ex_claim(tab, f2, &claims), (unsigned long long)at);
      }
    }
  }
  claims = ov_sum(claims);
  if ((threadIdx.x & 63) == 0 && claims) atomicAdd((unsigned long long*)res + 3, (unsigned long long)claims);
}

// res[4] += the duplicates.  The group outputs were preset to 0.
__global__ __launch_bounds__(kRowThreads) void k_exact_resolve(ExRows w, ExRule q, ExTable tab, const u64* __restrict__ F,
                                                               ExOut out, u64* __restrict__ res) {
  const u64 r = (u64)blockIdx.x * kRowThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  u64 grp = kExNone, dup = 0, dup_ids = 0, in = 0;
  if (r < w.R) {
    const u64 len = (u64)w.row[r + 1] - (u64)w.row[r], f = F[r], at = w.base + w.r0 + r;
    u64 first = at;
    if (w.grp) grp = ex_group(w, w.r0 + r);
    if (len >= q.min_len) {
      first = ex_first(tab, f);
      dup = first < at;
      if (w.in_group) in = ex_first(tab, ex_print2(q.seed, f, w.gbase + grp)) < at;
    }
    dup_ids = dup ? len : 0;
    out.first[r] = (int64_t)first;
    if (out.dup) out.dup[r] = (uint8_t)dup;
    if (out.print) out.print[r] = f;
  }
  const u64 dups = __ballot(dup != 0);
  if (lane == 0 && dups) atomicAdd((unsigned long long*)res + 4, (unsigned long long)__popcll(dups));
  if (!w.grp) return;
  // the lanes' groups do not decrease: a run's sums gather in its first lane
  for (int d = 1; d < 64; d <<= 1) {
    const u64 og = (u64)__shfl_down((unsigned long long)grp, d);
    const u64 a = (u64)__shfl_down((unsigned long long)dup, d), b = (u64)__shfl_down((unsigned long long)dup_ids, d);
    const u64 e = (u64)__shfl_down((unsigned long long)in, d);
    if (lane + d < 64 && og == grp) dup += a, dup_ids += b, in += e;
  }
  const u64 before = (u64)__shfl_up((unsigned long long)grp, 1);
  if (grp != kExNone && (lane == 0 || before != grp)) {
    if (dup && out.g_dup_rows) atomicAdd(out.g_dup_rows + grp, (unsigned long long)dup);
    if (dup_ids && out.g_dup_ids) atomicAdd(out.g_dup_ids + grp, (unsigned long long)dup_ids);
    if (in && out.g_in_rows) atomicAdd(out.g_in_rows + grp, (unsigned long long)in);
  }
}

u64 ex_tiles(u64 n) { return (n + kExTile - 1) / kExTile; }

// The exact passes' state, allocated on the first exact call: the table and the counters of shred_exact_reset,
// the scratch of a call and the staging of the host calls.
struct ExactState : PassState {
  DeviceWords res;          // [0] a bad row_off, [1] a bad grp_off, [2] compared rows, [3] new keys, [4] duplicates
  PinnedWords host;         // their copy
  EventSet<4> ev;
  OneRow one;               // a call without row_off
  DeviceBuf<u64> tab;       // slots keys, then slots indices
  u64 slots = 0, capacity = 0, distinct = 0, seen = 0, groups_seen = 0;
  ExRule rule{0, 1, 1};
  DeviceBuf<u64> F;         // the rows' fingerprints
  DeviceBuf<u64> carry;     // the six arrays of ExCarry, side by side
  DeviceBuf<int32_t> hids;  // host paths: a piece's ids,
  DeviceBuf<int64_t> hrow;  // its row_off,
  DeviceBuf<int64_t> hrows; // first and print of its rows, side by side,
  DeviceBuf<uint8_t> hdup;  // dup,
  DeviceBuf<int64_t> hgrp;  // and of the whole call grp_off
  DeviceBuf<int64_t> hgout; // and the three group outputs, side by side

  bool reserve(size_t rows) {
    return res.ensure(5) && host.ensure(5) && ev.ensure() && one.ensure() && F.grow(std::max<size_t>(rows, 1));
  }
  ExTable table() const { return ExTable{tab.get(), tab.get() + slots, slots - 1}; }
  ExCarry carries() const {
    u64* const p = carry.get();
    const size_t m = carry.cap();
    return ExCarry{p, p + m, p + 2 * m, p + 3 * m, p + 4 * m, p + 5 * m};
  }
  // Whether `compared` more rows fit, each inserted once or twice.
  bool fits(u64 compared, bool in_group) const {
    return compared <= capacity && distinct <= capacity && compared * (in_group ? 2 : 1) <= capacity - distinct;
  }
};

// The fingerprint, insert and resolve passes on rows whose offsets are good and fit the table; res[3] and res[4]
// were cleared and end up in es.host once st is idle.  0 or -1.
int exact_run(ExactState& es, const int32_t* ids, u64 n, const ExRows& w, const ExOut& out, hipStream_t st) {
  const u64 tiles = ex_tiles(n);
  if (!tiles_fit(n) || !es.carry.grow(std::max<size_t>(tiles, 1), 6)) return -1;
  const dim3 row_grid((unsigned)((w.R + kRowThreads - 1) / kRowThreads));
  if (tiles) {
    const ExCarry c = es.carries();
    ENC_OK(hipMemsetAsync(c.headRow, 0xFF, tiles * 8, st));
    k_exact_print<<<dim3((unsigned)tiles), dim3(kThreads), 0, st>>>(ids, n, w.row, w.R, es.rule, es.F.get(), c);
    ENC_OK(hipGetLastError());
    if (tiles > 1) {
      k_exact_carry<<<dim3(1), dim3(kThreads), 0, st>>>(c, tiles, w.row, es.rule, es.F.get());
      ENC_OK(hipGetLastError());
    }
  }
  k_exact_insert<<<row_grid, dim3(kRowThreads), 0, st>>>(w, es.rule, es.table(), es.F.get(), es.res.get());
  ENC_OK(hipGetLastError());
  k_exact_resolve<<<row_grid, dim3(kRowThreads), 0, st>>>(w, es.rule, es.table(), es.F.get(), out, es.res.get());
  ENC_OK(hipGetLastError());
  ENC_OK(hipMemcpyAsync(es.host.get() + 3, es.res.get() + 3, 16, hipMemcpyDeviceToHost, st));
  return 0;
}

}  // namespace

int EncodeDevice::exact_reset(uint64_t capacity, uint64_t seed, int64_t min_len) {
  if (min_len < 0 || capacity > (1ull << 58)) return -1;
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  ExactState& es = pass_state<ExactState>(pass_[kExact]);
  es.tab.reset();
  es.slots = es.capacity = es.distinct = es.seen = es.groups_seen = 0;
  if (!capacity) return 0;
  u64 slots = 2;
  while (slots < 2 * capacity) slots <<= 1;
  if (!es.tab.grow(slots, 2)) {
    std::fprintf(stderr, "[ERROR]\t encoder: exact table allocation failed (%zu bytes)\n", (size_t)(slots * 16));
    return -1;
  }
  ENC_OK(hipMemsetAsync(es.tab.get(), 0xFF, slots * 16, (hipStream_t)stream_));
  ENC_OK(hipStreamSynchronize((hipStream_t)stream_));
  es.slots = slots, es.capacity = capacity;
  es.rule = ExRule{seed, ex_mult(seed), (u64)min_len};
  return 0;
}

void EncodeDevice::exact_stats(uint64_t* table_bytes, uint64_t* capacity, uint64_t* distinct, uint64_t* seen,
                               uint64_t* groups_seen) const {
  const ExactState* es = static_cast<const ExactState*>(pass_[kExact].get());
  if (table_bytes) *table_bytes = es ? 16 * es->slots : 0;
  if (capacity) *capacity = es ? es->capacity : 0;
  if (distinct) *distinct = es ? es->distinct : 0;
  if (seen) *seen = es ? es->seen : 0;
  if (groups_seen) *groups_seen = es ? es->groups_seen : 0;
}

int64_t EncodeDevice::exact(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const int64_t* grp_off,
                            size_t groups, const ExactOut& o, void* stream, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  ExactState* const have = static_cast<ExactState*>(pass_[kExact].get());
  if (!have || !have->capacity) return -1;  // before a reset
  const u64 R = row_off ? rows : 1;
  if (!R) return 0;
  const bool in_group = o.g_in_rows != nullptr;
  const ExOut out{o.first, o.dup, o.print, (unsigned long long*)o.g_dup_rows, (unsigned long long*)o.g_dup_ids,
                  (unsigned long long*)o.g_in_rows};
  ExRows w{row_off, R, 0, have->seen, grp_off, groups, have->groups_seen, in_group};
  const int64_t r = device_call<ExactState>(
      pass_[kExact], device_, stream ? stream : stream_, "exact", R, kernel_ms,
      [&](ExactState& es, hipStream_t st, Plan* p) {
        if (!row_off && es.one.put(n, st, &w.row) < 0) return -1;
        ENC_OK(hipMemsetAsync(es.res.get(), 0, 40, st));
        k_exact_rows<<<dim3((unsigned)((R + kRowThreads) / kRowThreads)), dim3(kRowThreads), 0, st>>>(
            w.row, R, n, es.rule.min_len, es.res.get());
        ENC_OK(hipGetLastError());
        if (grp_off && check_offsets(grp_off, groups, R, es.res.get() + 1, st) < 0) return -1;
        ENC_OK(hipMemcpyAsync(es.host.get(), es.res.get(), 24, hipMemcpyDeviceToHost, st));
        ENC_OK(hipStreamSynchronize(st));
        if (es.host[0] || es.host[1]) return -6;
        if (!es.fits(es.host[2], in_group)) return -1;
        *p = Plan{0, true, n};
        return 0;
      },
      [&](ExactState& es, hipStream_t st) {
        for (unsigned long long* g : {out.g_dup_rows, out.g_dup_ids, out.g_in_rows})
          if (g && groups) ENC_OK(hipMemsetAsync(g, 0, groups * 8, st));
        return exact_run(es, ids, n, w, out, st);
      });
  if (r < 0) return r;
  have->distinct += have->host[3], have->seen += R, have->groups_seen += grp_off ? groups : 0;
  return (int64_t)have->host[4];
}

// Host rows in pieces of whole rows (host_pieces).  A piece is the device passes on its own rows at their
// global indices; a row's result depends on the rows before it alone, and those are in the table when its
// piece runs, so it does not depend on the piece.  grp_off and the group outputs stay on the device for the
// whole call.  The caller has validated row_off and grp_off.
int64_t EncodeDevice::exact_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const int64_t* grp_off,
                                 size_t groups, const ExactOut& o) {
  ExactState* const have = static_cast<ExactState*>(pass_[kExact].get());
  if (!have || !have->capacity) return -1;  // before a reset
  ExactState& es = *have;
  const u64 R = row_off ? rows : 1;
  if (!R) return 0;
  const bool in_group = o.g_in_rows != nullptr;
  u64 compared = 0;
  for (size_t r = 0; r < R; ++r) compared += (u64)(row_off ? row_off[r + 1] - row_off[r] : (int64_t)n) >= es.rule.min_len;
  if (!es.fits(compared, in_group)) return -1;
  hipStream_t st = (hipStream_t)stream_;
  int64_t* gout[3] = {nullptr, nullptr, nullptr};
  int64_t* const host_gout[3] = {o.g_dup_rows, o.g_dup_ids, o.g_in_rows};
  if (grp_off) {
    DeviceGuard guard;
    ENC_OK(hipSetDevice(device_));
    if (!es.hgrp.grow(groups + 1) || !es.hgout.grow(std::max<size_t>(groups, 1), 3)) return -1;
    ENC_OK(hipMemcpyAsync(es.hgrp.get(), grp_off, (groups + 1) * 8, hipMemcpyHostToDevice, st));
    for (int k = 0; k < 3; ++k) {
      if (!host_gout[k]) continue;
      gout[k] = es.hgout.get() + (size_t)k * es.hgout.cap();
      if (groups) ENC_OK(hipMemsetAsync(gout[k], 0, groups * 8, st));
    }
  }
  const int64_t one[2] = {0, (int64_t)n};
  const HostCall call{"exact", R, 0, 1, {{ids, n, row_off ? row_off : one}}, false, nullptr, 3,
                      {{o.first, 8, 1, 0}, {o.print, 8, 1, 0}, {o.dup, 1, 1, 0}}};
  const u64 seen = es.seen;
  int64_t total = 0;
  const int r = host_pieces(
      device_, st, call, [](size_t) { return (u64)1; },
      [&](const Piece& p, Staged* s) {
        const size_t m = p.r1 - p.r0;
        if (!es.reserve(m) || !es.hids.grow(std::max<size_t>(p.len[0], 1)) || !es.hrow.grow(m + 1) ||
            !es.hrows.grow(m, 2) || !es.hdup.grow(m))
          return false;
        s->ids[0] = es.hids.get(), s->row[0] = es.hrow.get();
        s->out[0] = es.hrows.get(), s->out[1] = es.hrows.get() + es.hrows.cap(), s->out[2] = es.hdup.get();
        return true;
      },
      [&](const Piece& p, const Staged& s) {
        const ExRows w{s.row[0], p.r1 - p.r0, p.r0, seen, grp_off ? es.hgrp.get() : nullptr, groups, es.groups_seen, in_group};
        const ExOut out{s.get<int64_t>(0), s.get<uint8_t>(2), s.get<u64>(1), (unsigned long long*)gout[0],
                        (unsigned long long*)gout[1], (unsigned long long*)gout[2]};
        ENC_OK(hipMemsetAsync(es.res.get() + 3, 0, 16, st));
        if (exact_run(es, s.ids[0], p.len[0], w, out, st) < 0) return -1;
        ENC_OK(hipStreamSynchronize(st));
        es.distinct += es.host[3];
        total += (int64_t)es.host[4];
        return 0;
      });
  if (r < 0) return r;
  for (int k = 0; k < 3; ++k)
    if (gout[k] && groups) ENC_OK(hipMemcpyAsync(host_gout[k], gout[k], groups * 8, hipMemcpyDeviceToHost, st));
  ENC_OK(hipStreamSynchronize(st));
  es.seen += R, es.groups_seen += grp_off ? groups : 0;
  return total;
}

}  // namespace shred
