// Repeated n-gram statistics of rows of ids on gfx950: the Gopher / MassiveText repetition measures, beside
// MinHash, dedup and overlap (C ABI and definitions: include/shredword_encode.h, shred_repeat_*).  The unit
// shares overlap's fingerprint and wave reductions (ngram_print.h), the batch units' wave search
// (batch_common.h), their device-call driver and host piece loop (batch_state.h) and the offset check
// (encode_common.h).
//
// Equality of grams within a row needs a table per row.  Every row's table is a region of one table in
// device memory.  (Two classes that kept the table of a row of up to 256 / 4096 grams in a wave's / a
// workgroup's LDS were built and measured slower on the benchmark corpus than this path alone, 13.0 ms
// against 9.3 ms, and were taken out: DESIGN.md.)
//
//   measure             k_repeat_rows checks row_off and the 32-bit in-row form of every row; two hipCUB sums
//                       over the rows give every row its table region (2 g slots for g grams) and its first
//                       tile; k_repeat_totals gathers the totals, so they reach the host in one copy, and the
//                       host grows the table.
//   k_repeat_tiles<I>   u64 keys, u32 smallest in-row positions, u32 counts.  Row r owns the slots
//                       [E2[r], E2[r] + 2 g): the slot of a fingerprint is E2[r] + mulhi(F, 2 g), probing
//                       wraps inside the region, so rows never meet and no region is more than half full.
//                       One workgroup per 2048 ids of a row (the tile's row is found by a wave search of the
//                       tile sums, a tile never holds two rows), so one row of a million ids loads the machine
//                       as many rows do.  I = true inserts (compare-and-swap claim, atomic add, atomic min);
//                       I = false reads out, with a left halo of w - 1 positions for coverage; strips of 9
//                       positions with the rolling update, masks and doubling as in k_overlap_tiles; a row's
//                       sums take one atomic per wave, its top a 64-bit atomic max of
//                       (count << 32 | inverted first position), so ties resolve as defined whatever the order.
//   k_repeat_init / k_repeat_final   clear the rows' outputs before, unpack their top word behind, and count
//                       the rows with repeats (a ballot and one atomic per wave).
//
// LDS per workgroup: 17 KB g + 9 KB first positions + masks: 27 KB.  Traffic per id: the id is read twice, two
// random 16-byte table accesses (atomics on insert), 9 B written with the token outputs; the table is cleared
// per call over the regions in use (16 B a slot, 32 B an id).  No matrix instruction fits: 64-bit integer
// multiply-adds, a mix, atomics.  All global indices are 64-bit.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

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

constexpr int kRpMaxW = EncodeDevice::kOverlapMaxNgram;
constexpr int kRpTile = 2048;                       // ids of a row per workgroup (overlap's tile)
constexpr int kRpStrip = 9;                         // consecutive positions per thread of k_repeat_tiles
constexpr int kRpPos = kThreads * kRpStrip;         // positions a workgroup can take: the tile and its left halo
constexpr int kRpG = kRpTile + 2 * (kRpMaxW - 1);   // ids a tile reads: both halos
constexpr int kRpWords = kRpPos / 64;               // words of its hit and coverage masks
constexpr uint32_t kRpNone = 0xFFFFFFFFu;           // no gram; above every in-row position
constexpr u64 kRpMaxRow = EncodeDevice::kRepeatMaxRow;  // the longest row whose positions fit 32 bits
static_assert(kRpTile + kRpMaxW - 1 <= kRpPos && kRpPos % 64 == 0 && kRpWords <= 64 && kRpMaxW <= 64,
              "the strips hold the tile and its halo; wave 0 holds the masks a word per lane");

struct RpRule {
  u64 seed, A, Aw;  // Aw = A^w
  int w;
};

struct RpOut {
  int64_t *grams, *distinct, *repeated, *covered, *top_count, *top_pos;
  int64_t* tok_first;  // may be nullptr
  uint8_t* tok_cov;    // may be nullptr
  u64 base;            // of the call's ids in the caller's (a host piece)
};

struct RpTable {
  u64* key;
  uint32_t *pos, *cnt;
};

__host__ __device__ inline u64 rp_grams(u64 len, int w) { return len >= (u64)w ? len - (u64)w + 1 : 0; }

// What the sums read of row_off: entries 0 .. rows, whatever they hold.
struct RpRows {
  const int64_t* row;
  int w;
  __host__ __device__ u64 len(u64 r) const { return (u64)row[r + 1] - (u64)row[r]; }
};
// Entry k of the sums: what row k - 1 adds (the exclusive sum, its total at entry `rows`).
struct RpSlots {
  RpRows rows;
  __host__ __device__ u64 operator()(u64 k) const {
    return k ? 2 * rp_grams(rows.len(k - 1), rows.w) : 0;
  }
};
struct RpTiles {
  RpRows rows;
  __host__ __device__ u64 operator()(u64 k) const {
    return k ? (rows.len(k - 1) + kRpTile - 1) / kRpTile : 0;
  }
};

// res[0] = 1 for a bad row_off, res[1] = 1 for a row past kRpMaxRow ids.
__global__ __launch_bounds__(kRowThreads) void k_repeat_rows(const int64_t* __restrict__ row, u64 rows, u64 n,
                                                             u64* __restrict__ res) {
  const u64 i = (u64)blockIdx.x * kRowThreads + threadIdx.x;
  if (i > rows) return;
  if (offset_bad(row, i, rows, n, true)) res[0] = 1;
  if (i < rows && (u64)row[i + 1] - (u64)row[i] > kRpMaxRow) res[1] = 1;
}

__global__ void k_repeat_totals(const u64* __restrict__ E2, const u64* __restrict__ ET, u64 rows, u64* __restrict__ res) {
  res[5] = E2[rows], res[6] = ET[rows];
}

// The rows' outputs before the tiles add to them.
__global__ __launch_bounds__(kRowThreads) void k_repeat_init(RpRows rows, u64 R, RpOut out) {
  const u64 r = (u64)blockIdx.x * kRowThreads + threadIdx.x;
  if (r >= R) return;
  out.grams[r] = (int64_t)rp_grams(rows.len(r), rows.w);
  out.distinct[r] = out.repeated[r] = out.covered[r] = out.top_count[r] = 0;  // (top_pos: k_repeat_final)
}

// Tile blockIdx.x of the call: ET[r] is row r's first tile, E2[r] its first slot (rows + 1 entries each).
template <bool kInsert>
__global__ __launch_bounds__(kThreads) void k_repeat_tiles(const int32_t* __restrict__ ids, const int64_t* __restrict__ row,
                                                           u64 rows, const u64* __restrict__ E2,
                                                           const u64* __restrict__ ET, RpRule q, RpTable tab, RpOut out) {
  __shared__ u64 s_g[kRpG];
  __shared__ uint32_t s_first[kInsert ? 1 : kRpPos];
  __shared__ u64 s_hit[kRpWords], s_cov[kRpWords];
  __shared__ u64 s_r;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = q.w;
  if (tid < 64) {
    // the last r with ET[r] <= the tile: ET[0] = 0 and ET[rows] = the grid, and a row without tiles repeats
    // its entry, so this is the row that holds the tile
    const u64 ub = wave_upper_bound(ET, 0, rows + 1, (u64)blockIdx.x, tid);
    if (tid == 0) s_r = ub - 1;
  }
  if (tid < kRpWords) s_hit[tid] = 0;
  __syncthreads();
  const u64 r = s_r, a = (u64)row[r], L = (u64)row[r + 1] - a;
  const u64 m = 2 * rp_grams(L, w), base = E2[r];   // the row's region: slots [base, base + m)
  const u64 t0 = ((u64)blockIdx.x - ET[r]) * kRpTile;  // < L
  const int Tn = (int)(L - t0 < (u64)kRpTile ? L - t0 : (u64)kRpTile);
  const int hl = kInsert ? 0 : (int)(t0 < (u64)(w - 1) ? t0 : (u64)(w - 1));
  const u64 b = t0 - (u64)hl;                      // the in-row position of local index 0
  const int np = hl + Tn;                          // positions taken: local [0, np), the tile's own from hl
  const int fill = np + w - 1;                     // g read by them: local [0, fill) <= kRpG
  const u64 have = L - b < (u64)fill ? L - b : (u64)fill;
  for (int i = tid; i < fill; i += kThreads) s_g[i] = (u64)i < have ? ov_g(q.seed, ids[a + b + (u64)i]) : 0;
  __syncthreads();

  const int p0 = tid * kRpStrip, p1 = p0 + kRpStrip < np ? p0 + kRpStrip : np;
  u64 claims = 0, cand = 0;
  if (p0 < np) {
    u64 S = 0;
    for (int k = 0; k < w; ++k) S = S * q.A + s_g[p0 + k];
    for (int p = p0;;) {
      const u64 at = b + (u64)p;
      uint32_t first = kRpNone;
      if (at + (u64)w <= L) {  // the gram lies in the row
        const u64 F = ov_print(S);
        u64 slot = base + __umul64hi(F, m);
        if (kInsert) {
          for (;;) {
            u64 cur = __hip_atomic_load(tab.key + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == kOvFree &&
                __hip_atomic_compare_exchange_strong(tab.key + slot, &cur, F, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)) {
              ++claims;
              break;
            }
            if (cur == F) break;  // (on failure cur is the key that won the slot)
            if (++slot == base + m) slot = base;
          }
          atomicAdd(tab.cnt + slot, 1u);
          atomicMin(tab.pos + slot, (uint32_t)at);
        } else {
          for (;;) {  // the insert pass put F there
            const u64 cur = tab.key[slot];
            if (cur == F || cur == kOvFree) break;
            if (++slot == base + m) slot = base;
          }
          const uint32_t c = tab.cnt[slot];
          first = tab.pos[slot];
          if (c >= 2) atomicOr((unsigned long long*)&s_hit[p >> 6], 1ull << (p & 63));
          const u64 word = (u64)c << 32 | (u64)(kRpNone - first);
          cand = word > cand ? word : cand;
        }
      }
      if (!kInsert) s_first[p] = first;
      if (++p >= p1) break;
      S = S * q.A - q.Aw * s_g[p - 1] + s_g[p - 1 + w];  // p - 1 + w <= np - 2 + w < fill
    }
  }
  if (kInsert) {
    claims = ov_sum(claims);
    if (lane == 0 && claims) atomicAdd((unsigned long long*)out.distinct + r, (unsigned long long)claims);
    return;
  }

  __syncthreads();
  if (tid < 64) {
    u64 c = tid < kRpWords ? s_hit[tid] : 0;
    for (int span = 1; span < w;) {
      const int s = span < w - span ? span : w - span;  // 1 .. 32
      u64 below = (u64)__shfl_up((unsigned long long)c, 1);
      if (tid == 0) below = 0;
      c |= (c << s) | (below >> (64 - s));
      span += s;
    }
    if (tid < kRpWords) s_cov[tid] = c;
  }
  __syncthreads();

  // the tile's own ids: consecutive threads consecutive ids
  u64 rep = 0, cov = 0;
  for (int t = tid; t < Tn; t += kThreads) {
    const int p = hl + t;
    const u64 c = (s_cov[p >> 6] >> (p & 63)) & 1;
    rep += (s_hit[p >> 6] >> (p & 63)) & 1, cov += c;
    if (out.tok_first)
      out.tok_first[a + t0 + (u64)t] = s_first[p] == kRpNone ? -1 : (int64_t)(out.base + a + (u64)s_first[p]);
    if (out.tok_cov) out.tok_cov[a + t0 + (u64)t] = (uint8_t)c;
  }
  rep = ov_sum(rep), cov = ov_sum(cov);
  for (int d = 32; d; d >>= 1) {
    const u64 o = (u64)__shfl_xor((unsigned long long)cand, d);
    cand = o > cand ? o : cand;
  }
  if (lane == 0) {
    if (rep) atomicAdd((unsigned long long*)out.repeated + r, (unsigned long long)rep);
    if (cov) atomicAdd((unsigned long long*)out.covered + r, (unsigned long long)cov);
    if (cand) atomicMax((unsigned long long*)out.top_count + r, (unsigned long long)cand);
  }
}

// The rows' top word unpacked; res[2] += the rows with repeats.
__global__ __launch_bounds__(kRowThreads) void k_repeat_final(RpRows rows, u64 R, RpOut out, u64* __restrict__ res) {
  const u64 r = (u64)blockIdx.x * kRowThreads + threadIdx.x;
  if (r < R) {
    const u64 word = (u64)out.top_count[r];  // 0 without grams
    out.top_count[r] = (int64_t)(word >> 32);
    out.top_pos[r] = word ? (int64_t)(out.base + (u64)rows.row[r] + (u64)(kRpNone - (uint32_t)word)) : -1;
  }
  const u64 some = __ballot(r < R && out.repeated[r] != 0);
  if ((threadIdx.x & 63) == 0 && some) atomicAdd((unsigned long long*)res + 2, (unsigned long long)__popcll(some));
}

// The repeat passes' state, allocated on the first repeat call.
struct RepeatState : PassState {
  DeviceWords res;          // [0] a bad row_off, [1] a row too long, [2] rows with repeats, [5] the rows' slots,
                            // [6] their tiles
  PinnedWords host;         // their copy
  EventSet<4> ev;
  OneRow one;               // a call without row_off
  DeviceBuf<u64> sums;      // E2, and (at cap()) ET: rows + 1 entries each
  DeviceBuf<uint8_t> tmp;   // hipCUB scratch
  DeviceBuf<u64> tab;       // the rows' table: per slot a u64 key, then a u32 position, then a u32 count
  DeviceBuf<int32_t> hids;  // host paths: a piece's ids,
  DeviceBuf<int64_t> hrow;  // its row_off,
  DeviceBuf<int64_t> hrows; // the six outputs of its rows, side by side,
  DeviceBuf<int64_t> hfirst;  // tok_first
  DeviceBuf<uint8_t> hcov;    // and tok_cov

  bool reserve(size_t rows) {
    const size_t m = std::max<size_t>(rows, 1);
    if (!res.ensure(7) || !host.ensure(7) || !ev.ensure() || !one.ensure() || !sums.grow(m + 1, 2))
      return false;
    const RpRows rr{nullptr, 1};
    size_t scan = 0;
    if (hipcub::DeviceScan::InclusiveSum(nullptr, scan, row_iter(RpSlots{rr}), sums.get(), (u64)m + 1) != hipSuccess)
      return false;
    return tmp.grow(std::max<size_t>(scan, 16));
  }
};

// The measure pass on R >= 1 rows; the stream is idle behind it and rs.host holds the words.  0, -1 or -6.
int repeat_measure(RepeatState& rs, u64 n, const int64_t* row, u64 R, const RpRows& rr, hipStream_t st) {
  ENC_OK(hipMemsetAsync(rs.res.get(), 0, 56, st));
  k_repeat_rows<<<dim3((unsigned)((R + kRowThreads) / kRowThreads)), dim3(kRowThreads), 0, st>>>(row, R, n, rs.res.get());
  ENC_OK(hipGetLastError());
  u64* const E2 = rs.sums.get();
  u64* const ET = E2 + rs.sums.cap();
  size_t bytes = rs.tmp.cap();
  ENC_OK(hipcub::DeviceScan::InclusiveSum(rs.tmp.get(), bytes, row_iter(RpSlots{rr}), E2, R + 1, st));
  bytes = rs.tmp.cap();
  ENC_OK(hipcub::DeviceScan::InclusiveSum(rs.tmp.get(), bytes, row_iter(RpTiles{rr}), ET, R + 1, st));
  k_repeat_totals<<<dim3(1), dim3(1), 0, st>>>(E2, ET, R, rs.res.get());
  ENC_OK(hipGetLastError());
  ENC_OK(hipMemcpyAsync(rs.host.get(), rs.res.get(), 56, hipMemcpyDeviceToHost, st));
  ENC_OK(hipStreamSynchronize(st));
  if (rs.host[0]) return -6;
  if (rs.host[1]) return -1;  // as the batch calls answer an entry past int32
  if (rs.host[6] > 0x7FFFFFFFull) return -1;
  if (!rs.tab.grow((size_t)rs.host[5] * 2)) {
    std::fprintf(stderr, "[ERROR]\t encoder: repeat table allocation failed (%zu ids, %zu bytes)\n", (size_t)n,
                 (size_t)rs.host[5] * 16);
    return -1;
  }
  return 0;
}

// The passes behind a good measure; the rows with repeats end up in rs.host[2] once st is idle.  0 or -1.
int repeat_run(RepeatState& rs, const int32_t* ids, const int64_t* row, u64 R, const RpRows& rr, const RpRule& q,
               const RpOut& out, hipStream_t st) {
  const u64 slots = rs.host[5], tiles = rs.host[6];
  const dim3 row_grid((unsigned)((R + kRowThreads - 1) / kRowThreads));
  const u64* const E2 = rs.sums.get();
  const u64* const ET = E2 + rs.sums.cap();
  const RpTable tab{rs.tab.get(), reinterpret_cast<uint32_t*>(rs.tab.get() + slots),
                    reinterpret_cast<uint32_t*>(rs.tab.get() + slots) + slots};
  if (slots) {
    ENC_OK(hipMemsetAsync(tab.key, 0xFF, slots * 12, st));  // keys free, positions above every one
    ENC_OK(hipMemsetAsync(tab.cnt, 0, slots * 4, st));
  }
  k_repeat_init<<<row_grid, dim3(kRowThreads), 0, st>>>(rr, R, out);
  ENC_OK(hipGetLastError());
  if (tiles) {
    k_repeat_tiles<true><<<dim3((unsigned)tiles), dim3(kThreads), 0, st>>>(ids, row, R, E2, ET, q, tab, out);
    ENC_OK(hipGetLastError());
    k_repeat_tiles<false><<<dim3((unsigned)tiles), dim3(kThreads), 0, st>>>(ids, row, R, E2, ET, q, tab, out);
    ENC_OK(hipGetLastError());
  }
  k_repeat_final<<<row_grid, dim3(kRowThreads), 0, st>>>(rr, R, out, rs.res.get());
  ENC_OK(hipGetLastError());
  ENC_OK(hipMemcpyAsync(rs.host.get() + 2, rs.res.get() + 2, 8, hipMemcpyDeviceToHost, st));
  return 0;
}

RpRule repeat_rule(int w, u64 seed) { return RpRule{seed, ov_mult(seed, (u64)w), ov_power(ov_mult(seed, (u64)w), w), w}; }

RpOut repeat_out(const EncodeDevice::RepeatOut& o, u64 base) {
  return RpOut{o.grams, o.distinct, o.repeated, o.covered, o.top_count, o.top_pos, o.tok_first, o.tok_cov, base};
}

}  // namespace

int64_t EncodeDevice::repeat(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, int w, uint64_t seed,
                             const RepeatOut& o, void* stream, double* kernel_ms) {
  const u64 R = row_off ? rows : 1;
  const RpRule q = repeat_rule(w, seed);
  const RpOut out = repeat_out(o, 0);
  RpRows rr{row_off, w};
  RepeatState* state = nullptr;
  const int64_t r = device_call<RepeatState>(
      pass_[kRepeat], device_, stream ? stream : stream_, "repeat", R, kernel_ms,
      [&](RepeatState& rs, hipStream_t st, Plan* p) {
        state = &rs;
        if (!R) return 0;
        if (!row_off && rs.one.put(n, st, &rr.row) < 0) return -1;
        const int bad = repeat_measure(rs, n, rr.row, R, rr, st);
        if (bad < 0) return bad;
        *p = Plan{0, true, n};
        return 0;
      },
      [&](RepeatState& rs, hipStream_t st) { return repeat_run(rs, ids, rr.row, R, rr, q, out, st); });
  return r < 0 || !R ? r : (int64_t)state->host[2];
}

// Host rows in pieces of whole rows (host_pieces).  A piece is the device passes on its own rows; no gram
// crosses a row, so a row's result does not depend on the piece; top_pos and tok_first are rebased by the
// piece's first id, and the per-token outputs, which host_pieces does not know, come back at that id.
int64_t EncodeDevice::repeat_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, int w,
                                  uint64_t seed, const RepeatOut& o) {
  RepeatState& rs = pass_state<RepeatState>(pass_[kRepeat]);
  hipStream_t st = (hipStream_t)stream_;
  const RpRule q = repeat_rule(w, seed);
  const int64_t one[2] = {0, (int64_t)n};
  const HostCall call{"repeat", row_off ? rows : 1, 0, 1, {{ids, n, row_off ? row_off : one}}, false, nullptr, 6,
                      {{o.grams, 8, 1, 0}, {o.distinct, 8, 1, 0}, {o.repeated, 8, 1, 0}, {o.covered, 8, 1, 0},
                       {o.top_count, 8, 1, 0}, {o.top_pos, 8, 1, 0}}};
  int64_t total = 0;
  const int r = host_pieces(
      device_, st, call, [](size_t) { return (u64)1; },
      [&](const Piece& p, Staged* s) {
        const size_t m = p.r1 - p.r0, len = std::max<size_t>(p.len[0], 1);
        if (!tiles_fit(p.len[0]) || !rs.reserve(m) || !rs.hids.grow(len) || !rs.hrow.grow(m + 1) ||
            !rs.hrows.grow(m, 6) || (o.tok_first && !rs.hfirst.grow(len)) || (o.tok_cov && !rs.hcov.grow(len)))
          return false;
        s->ids[0] = rs.hids.get(), s->row[0] = rs.hrow.get();
        for (int k = 0; k < 6; ++k) s->out[k] = rs.hrows.get() + (size_t)k * rs.hrows.cap();
        return true;
      },
      [&](const Piece& p, const Staged& s) {
        const RpRows rr{s.row[0], w};
        const RpOut out{s.get<int64_t>(0), s.get<int64_t>(1), s.get<int64_t>(2), s.get<int64_t>(3), s.get<int64_t>(4),
                        s.get<int64_t>(5), o.tok_first ? rs.hfirst.get() : nullptr,
                        o.tok_cov ? rs.hcov.get() : nullptr, (u64)p.a[0]};
        if (repeat_measure(rs, p.len[0], s.row[0], p.r1 - p.r0, rr, st) < 0) return -1;
        if (repeat_run(rs, s.ids[0], s.row[0], p.r1 - p.r0, rr, q, out, st) < 0) return -1;
        if (o.tok_first && p.len[0])
          ENC_OK(hipMemcpyAsync(o.tok_first + p.a[0], rs.hfirst.get(), p.len[0] * 8, hipMemcpyDeviceToHost, st));
        if (o.tok_cov && p.len[0])
          ENC_OK(hipMemcpyAsync(o.tok_cov + p.a[0], rs.hcov.get(), p.len[0], hipMemcpyDeviceToHost, st));
        ENC_OK(hipStreamSynchronize(st));
        total += (int64_t)rs.host[2];
        return 0;
      });
  return r < 0 ? r : total;
}

}  // namespace shred
