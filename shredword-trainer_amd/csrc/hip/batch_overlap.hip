// n-gram overlap of rows of ids against a held-out reference set on gfx950: benchmark decontamination,
// between "encoded" and "batched" (C ABI and definitions: include/shredword_encode.h, shred_overlap_*).
// The unit shares the batch units' wave search (batch_common.h), their device-call driver and host
// piece loop (batch_state.h), the seeded draw (draw_hash.h) and the offset check (encode_common.h).
//
//   k_offsets_check     (encode_common.h) row_off, before anything is written.
//   k_overlap_tiles<I>  one kernel, two modes: I = true inserts the reference stream's fingerprints into
//                       the table, I = false probes the corpus stream's.  The work is split over the flat
//                       stream, not over rows: one workgroup per kOvTile = 2048 consecutive positions (a
//                       position is the index of a gram's first id), so many short rows and one long row
//                       load the machine alike.
//     ids               the ids of [t0 - hl, t0 + T + w - 1), clipped to the stream, are read once and
//                       g(id) goes to LDS as u64: two mixes per id, not per (position, j).  hl, the
//                       left halo, is w - 1 in probe mode (a hit up to w - 1 positions before the tile
//                       covers tokens of the tile, so those positions are probed again here) and 0 in
//                       insert mode.
//     rows              wave 0 finds the row of the first position and the number of row_off entries up
//                       to the last with two wave_upper_bound searches; the ends of those rows, relative
//                       to the tile, are staged in LDS (the first kOvRows of them; a tile with more, which
//                       takes over a thousand empty or one-id rows in 2048 positions, reads the others
//                       from row_off).  A thread finds the row of its first position by a binary search
//                       there and then walks forward: a gram exists iff it ends before its row does.
//     strips            a thread owns kOvStrip = 9 consecutive positions: S of the first by w multiply-
//                       adds from LDS, then S(k + 1) = A S(k) - A^w g(t[k]) + g(t[k + w]) (A^w comes from
//                       the host), so a position costs 2 + w / 9 multiply-adds and one mix, against
//                       MinHash's w mixes.  Nine, not eight: 256 x 9 = 2304 positions hold the tile and its
//                       halo (2048 + 63), and a wave's 8-byte LDS reads at a stride of 9 words fall on
//                       banks 18 l mod 64, which are pairwise distinct over the 32 lanes of a pass (9 is
//                       odd), where a stride of 8 would put them 4 deep.  So g needs no padding.  (The
//                       layout with strips of 8 and a pad word per strip was not built: the halo would
//                       need a second round of strips.)
//     insert            the slot comes from the fingerprint (already a mix), linear probing; a free
//                       slot is claimed with a 64-bit compare-and-swap of its key and the position goes
//                       into the slot's pos by atomicMin, so P does not depend on scheduling.  Claims
//                       and grams are counted per thread, added over the wave, one atomic per wave.
//     probe             hits set bits of an LDS mask over halo + tile; P goes to LDS.  Wave 0 then turns
//                       the 36 words of the mask into coverage in registers: a word per lane, log2(w)
//                       doubling steps of c |= c << s with the carry from the lane below by shuffle.
//                       Behind it every thread walks its strip again and counts the hits and covered
//                       tokens of the tile's own positions per row, flushed with one atomic add (and an
//                       unsigned atomicMin for `first`, preset to all-ones = -1) when the row changes;
//                       the last run of a wave whose lanes all end in one row is added over the wave
//                       first, so a long row costs a wave one atomic.  tok_ref and tok_cov are written
//                       from LDS, consecutive threads consecutive tokens, for the tile's own positions.
//   k_overlap_count     rows with hits: a ballot and one atomic per wave.
//
// The table: cap = 2^k >= 2 m slots for a reference stream of m ids (it has at most m grams, so it
// is never more than half full and every probe ends), u64 keys (all-ones: free) and u32 smallest
// positions in two arrays, 12 bytes a slot.  A new set is built beside the old one and replaces it
// only when it is complete, so a failed build keeps the previous set.
//
// LDS per workgroup: 17 KB of g, 9 KB of P, 4 KB of row ends, 0.6 KB of masks: 31 KB.  Traffic per
// corpus id: 4 B read, one or two random 8-byte table reads, 9 B written with the token outputs.  No
// matrix instruction fits: 64-bit integer multiply-adds, a mix, atomics.  All global indices are 64-bit.
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

constexpr int kOvTile = 2048;  // positions per workgroup (OVERLAP_TILE)
constexpr int kOvStrip = 9;    // consecutive positions per thread
constexpr int kOvMaxW = EncodeDevice::kOverlapMaxNgram;
constexpr int kOvPos = kThreads * kOvStrip;         // positions a workgroup can take: the tile and its left halo
constexpr int kOvG = kOvTile + 2 * (kOvMaxW - 1);   // ids a tile reads: both halos
constexpr int kOvWords = kOvPos / 64;               // words of the hit and coverage masks
constexpr int kOvRows = 1024;                       // row ends staged in LDS
constexpr int kOvFar = 1 << 20;                     // a row end past everything the tile holds
constexpr uint32_t kOvNone = 0xFFFFFFFFu;           // no reference position: above every one
static_assert(kOvTile + kOvMaxW - 1 <= kOvPos && kOvPos % 64 == 0 && kOvWords <= 64,
              "the strips hold the tile and its halo; wave 0 holds the masks a word per lane");
static_assert(kOvMaxW <= 64, "a doubling step shifts by at most 32 bits");
// (the fingerprint ov_g / ov_mult / ov_print and a free slot's key kOvFree: ngram_print.h)

struct OvTable {
  u64* key;       // nullptr: no reference set, nothing hits
  uint32_t* pos;
  u64 mask;       // cap - 1
};

// What the kernels know of a reference set; passed by value.
struct OvRule {
  u64 seed, A, Aw;  // Aw = A^w
  int w;
};
constexpr OvRule kOvNoRule{0, 1, 1, 1};  // without a reference set: grams of one id, none of which hits

// What a probe writes; every pointer but hits may be nullptr.
struct OvOut {
  unsigned long long *hits, *covered, *first;
  int64_t* tok_ref;
  uint8_t* tok_cov;
  u64 first_base;  // of the call's ids in the caller's (a host piece)
};

// Positions [0, n) of the id stream, n >= 1; row: rows + 1 good offsets.  Insert: ctr[1] += grams,
// ctr[2] += slots claimed.  Probe: out.hits / covered were preset to 0, out.first to all-ones.
template <bool kInsert>
__global__ __launch_bounds__(kThreads) void k_overlap_tiles(const int32_t* __restrict__ ids, u64 n,
                                                            const int64_t* __restrict__ row, u64 rows, OvRule q,
                                                            OvTable tab, OvOut out, u64* __restrict__ ctr) {
  __shared__ u64 s_g[kOvG];
  __shared__ uint32_t s_ref[kInsert ? 1 : kOvPos];
  __shared__ int s_end[kOvRows];
  __shared__ u64 s_hit[kOvWords], s_cov[kOvWords];
  __shared__ u64 s_k[2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = q.w;
  const u64 t0 = (u64)blockIdx.x * kOvTile;
  const int Tn = (int)(n - t0 < (u64)kOvTile ? n - t0 : (u64)kOvTile);
  const int hl = kInsert ? 0 : (int)(t0 < (u64)(w - 1) ? t0 : (u64)(w - 1));
  const u64 b = t0 - (u64)hl;                      // the stream position of local index 0
  const int np = hl + Tn;                          // positions taken: local [0, np), the tile's own from hl
  const int fill = np + w - 1;                     // g read by them: local [0, fill) <= kOvG
  const u64 have = n - b < (u64)fill ? n - b : (u64)fill;  // of which the stream holds these; 0 behind
  for (int i = tid; i < fill; i += kThreads) s_g[i] = (u64)i < have ? ov_g(q.seed, ids[b + (u64)i]) : 0;
  if (tid < kOvWords) s_hit[tid] = 0;
  if (tid < 64) {
    // rows [ks, kend) hold the positions or are empty rows among them: ks is the last k with
    // row[k] <= b (row[0] = 0 and row[rows] = n > b, so 0 <= ks < rows), kend the number of entries at
    // or before the last position (<= rows, as row[rows] = n lies past it)
    const u64* E = reinterpret_cast<const u64*>(row);
    const u64 ub = wave_upper_bound(E, 0, rows + 1, b, tid);
    const u64 ue = wave_upper_bound(E, ub, rows + 1, b + (u64)np - 1, tid);
    if (tid == 0) s_k[0] = ub - 1, s_k[1] = ue;
  }
  __syncthreads();
  const u64 ks = s_k[0];
  const u64 nrows64 = s_k[1] - ks;  // >= 1; not bounded by the tile: empty rows
  // the end of row ks + i, relative to b, at most kOvFar; i < nrows64, so ks + i + 1 <= rows
  const auto far_end = [&](u64 i) {
    const u64 e = (u64)row[ks + i + 1] - b;
    return (int)(e < (u64)kOvFar ? e : (u64)kOvFar);
  };
  const int staged = nrows64 < (u64)kOvRows ? (int)nrows64 : kOvRows;
  for (int i = tid; i < staged; i += kThreads) s_end[i] = far_end((u64)i);
  __syncthreads();
  const auto end_of = [&](u64 i) { return i < (u64)staged ? s_end[i] : far_end(i); };

  const int p0 = tid * kOvStrip, p1 = p0 + kOvStrip < np ? p0 + kOvStrip : np;
  u64 i0 = 0;   // the row of p0 (relative to ks) and its end, kept for the second walk
  int e0 = 0;
  u64 grams = 0, claims = 0;
  if (p0 < np) {
    u64 x = 0, y = nrows64 - 1;  // the first row that ends past p0: row nrows64 - 1 ends past np - 1
    while (x < y) {
      const u64 mid = (x + y) >> 1;
      if (end_of(mid) > p0) y = mid; else x = mid + 1;
    }
    i0 = x, e0 = end_of(x);
    u64 i = i0;
    int e = e0;
    u64 S = 0;
    for (int j = 0; j < w; ++j) S = S * q.A + s_g[p0 + j];
    for (int p = p0;;) {
      while (p >= e) e = end_of(++i);  // ends at the row of np - 1 at the latest
      uint32_t ref = kOvNone;
      if (p + w <= e) {                // the gram lies in its row
        const u64 F = ov_print(S);
        u64 slot = F & tab.mask;
        if (kInsert) {
          ++grams;
          for (;;) {
            u64 cur = __hip_atomic_load(tab.key + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == kOvFree &&
                __hip_atomic_compare_exchange_strong(tab.key + slot, &cur, F, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)) {
              ++claims;
              break;
            }
            if (cur == F) break;  // (on failure cur is the key that won the slot)
            slot = (slot + 1) & tab.mask;
          }
          __hip_atomic_fetch_min(tab.pos + slot, (uint32_t)(b + (u64)p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (tab.key) {
          for (;;) {
            const u64 cur = tab.key[slot];
            if (cur == F) {
              ref = tab.pos[slot];
              atomicOr((unsigned long long*)&s_hit[p >> 6], 1ull << (p & 63));
              break;
            }
            if (cur == kOvFree) break;
            slot = (slot + 1) & tab.mask;
          }
        }
      }
      if (!kInsert) s_ref[p] = ref;
      if (++p >= p1) break;
      S = S * q.A - q.Aw * s_g[p - 1] + s_g[p - 1 + w];  // p - 1 + w <= np - 2 + w < fill
    }
  }
  if (kInsert) {
    grams = ov_sum(grams), claims = ov_sum(claims);
    if (lane == 0 && grams) {
      atomicAdd((unsigned long long*)ctr + 1, (unsigned long long)grams);
      if (claims) atomicAdd((unsigned long long*)ctr + 2, (unsigned long long)claims);
    }
    return;
  }

  __syncthreads();
  if (tid < 64) {
    // coverage = the OR of hit << s over s in [0, w): the span doubles until it is w
    u64 c = tid < kOvWords ? s_hit[tid] : 0;
    for (int L = 1; L < w;) {
      const int s = L < w - L ? L : w - L;  // 1 .. 32
      u64 below = (u64)__shfl_up((unsigned long long)c, 1);
      if (tid == 0) below = 0;
      c |= (c << s) | (below >> (64 - s));
      L += s;
    }
    if (tid < kOvWords) s_cov[tid] = c;
  }
  __syncthreads();

  // the tile's own positions, per row: hits, covered tokens, the first hit
  u64 ph = 0, pc = 0, pf = ~0ull;
  const auto flush = [&](u64 i, u64 h, u64 c, u64 f) {
    if (h) atomicAdd(out.hits + ks + i, (unsigned long long)h);
    if (c && out.covered) atomicAdd(out.covered + ks + i, (unsigned long long)c);
    if (f != ~0ull && out.first) atomicMin(out.first + ks + i, (unsigned long long)f);
  };
  const int o0 = p0 > hl ? p0 : hl;
  const bool own = o0 < p1;
  u64 i = i0;
  if (own) {
    int e = e0;
    for (int p = o0; p < p1; ++p) {
      if (p >= e) {
        flush(i, ph, pc, pf);
        ph = pc = 0, pf = ~0ull;
        while (p >= e) e = end_of(++i);
      }
      const u64 h = (s_hit[p >> 6] >> (p & 63)) & 1;
      ph += h, pc += (s_cov[p >> 6] >> (p & 63)) & 1;
      if (h && pf == ~0ull) pf = out.first_base + b + (u64)p;
    }
  }
  const u64 act = __ballot(own);
  if (act) {
    const u64 lead = (u64)__shfl((unsigned long long)i, __ffsll((unsigned long long)act) - 1);
    if (__all(!own || i == lead)) {  // every lane ends in one row (a lane without positions adds nothing)
      ph = ov_sum(ph), pc = ov_sum(pc), pf = ov_min(pf);
      if (lane == 0) flush(lead, ph, pc, pf);
    } else if (own) {
      flush(i, ph, pc, pf);
    }
  }
  for (int t = tid; t < Tn; t += kThreads) {
    const int p = hl + t;
    if (out.tok_ref) out.tok_ref[t0 + (u64)t] = s_ref[p] == kOvNone ? -1 : (int64_t)s_ref[p];
    if (out.tok_cov) out.tok_cov[t0 + (u64)t] = (uint8_t)((s_cov[p >> 6] >> (p & 63)) & 1);
  }
}

// ctr[0] += the rows of hits[0 .. R) that are not 0.
__global__ __launch_bounds__(kThreads) void k_overlap_count(const unsigned long long* __restrict__ hits, u64 R,
                                                            u64* __restrict__ ctr) {
  const u64 r = (u64)blockIdx.x * kThreads + threadIdx.x;
  const u64 some = __ballot(r < R && hits[r] != 0);
  if ((threadIdx.x & 63) == 0 && some) atomicAdd((unsigned long long*)ctr, (unsigned long long)__popcll(some));
}

unsigned ov_tiles(u64 n) { return (unsigned)((n + kOvTile - 1) / kOvTile); }

// The overlap passes' state, allocated on the first overlap call: the reference set's table, the error
// and result words, and the staging of the host calls.
struct OverlapState : PassState {
  DeviceWords res;       // [0] a bad row_off / rows with hits, [1] reference grams, [2] slots claimed
  PinnedWords host;      // their copy
  EventSet<4> ev;
  OneRow one;            // a call without row_off
  DeviceBuf<u64> tab[2]; // the set in use (cur) and the one being built: cap keys, then cap positions
  int cur = 0;
  bool has = false;      // a reference set is registered
  OvRule rule = kOvNoRule;
  u64 mask = 0, grams = 0, distinct = 0;
  DeviceBuf<int32_t> hids;   // host paths: a piece's ids,
  DeviceBuf<int64_t> hrow;   // its row_off,
  DeviceBuf<int64_t> hrows;  // hits, covered and first of its rows, side by side,
  DeviceBuf<int64_t> href;   // tok_ref
  DeviceBuf<uint8_t> hcov;   // and tok_cov

  bool reserve(size_t) { return res.ensure(3) && host.ensure(3) && ev.ensure() && one.ensure(); }
  OvTable table() const {
    if (!has) return OvTable{nullptr, nullptr, 0};
    return OvTable{tab[cur].get(), reinterpret_cast<uint32_t*>(tab[cur].get() + mask + 1), mask};
  }
  void clear() {
    tab[0].reset(), tab[1].reset();
    has = false, rule = kOvNoRule, mask = grams = distinct = 0;
  }
};

// The probe passes on R rows whose offsets are good: 0 or -1; the rows with hits end up in os.host[0]
// once st is idle.
int overlap_run(OverlapState& os, const int32_t* ids, u64 n, const int64_t* row, u64 R, const OvOut& out,
                hipStream_t st) {
  if (!R) return 0;
  ENC_OK(hipMemsetAsync(os.res.get(), 0, 8, st));
  ENC_OK(hipMemsetAsync(out.hits, 0, R * 8, st));
  if (out.covered) ENC_OK(hipMemsetAsync(out.covered, 0, R * 8, st));
  if (out.first) ENC_OK(hipMemsetAsync(out.first, 0xFF, R * 8, st));
  if (n) {
    k_overlap_tiles<false><<<dim3(ov_tiles(n)), dim3(kThreads), 0, st>>>(ids, n, row, R, os.rule, os.table(), out,
                                                                         os.res.get());
    ENC_OK(hipGetLastError());
  }
  k_overlap_count<<<dim3((unsigned)((R + kThreads - 1) / kThreads)), dim3(kThreads), 0, st>>>(out.hits, R, os.res.get());
  ENC_OK(hipGetLastError());
  ENC_OK(hipMemcpyAsync(os.host.get(), os.res.get(), 8, hipMemcpyDeviceToHost, st));
  return 0;
}

// row_off of a device call on st: *row = the offsets to use; 0, -1 or -6.
int overlap_offsets(OverlapState& os, u64 n, const int64_t* row_off, u64 R, hipStream_t st, const int64_t** row) {
  if (!row_off) return os.one.put(n, st, row);
  ENC_OK(hipMemsetAsync(os.res.get(), 0, 8, st));
  if (check_offsets(row_off, R, n, os.res.get(), st) < 0) return -1;
  ENC_OK(hipMemcpyAsync(os.host.get(), os.res.get(), 8, hipMemcpyDeviceToHost, st));
  ENC_OK(hipStreamSynchronize(st));
  return os.host[0] ? -6 : 0;
}

}  // namespace

int64_t EncodeDevice::overlap_refs(const int32_t* ids, size_t m, const int64_t* row_off, size_t rows, int w,
                                   uint64_t seed, void* stream, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  if (!m) {
    if (pass_[kOverlap]) static_cast<OverlapState&>(*pass_[kOverlap]).clear();
    return 0;
  }
  const u64 R = row_off ? rows : 1;
  const int64_t* row = row_off;
  u64 cap = 2;
  while (cap < 2 * (u64)m) cap <<= 1;
  const OvRule rule{seed, ov_mult(seed, (u64)w), ov_power(ov_mult(seed, (u64)w), w), w};
  OverlapState* state = nullptr;
  const int64_t r = device_call<OverlapState>(
      pass_[kOverlap], device_, stream ? stream : stream_, "overlap reference", R, kernel_ms,
      [&](OverlapState& os, hipStream_t st, Plan* p) {
        state = &os;
        const int bad = overlap_offsets(os, m, row_off, R, st, &row);
        if (bad < 0) return bad;
        if (!os.tab[1 - os.cur].grow(cap + cap / 2)) {
          std::fprintf(stderr, "[ERROR]\t encoder: overlap table allocation failed (%zu ids, %zu bytes)\n", m,
                       (size_t)(cap * 12));
          return -1;
        }
        *p = Plan{0, true, m};
        return 0;
      },
      [&](OverlapState& os, hipStream_t st) {
        u64* const t = os.tab[1 - os.cur].get();
        ENC_OK(hipMemsetAsync(t, 0xFF, (cap + cap / 2) * 8, st));
        ENC_OK(hipMemsetAsync(os.res.get(), 0, 24, st));
        k_overlap_tiles<true><<<dim3(ov_tiles(m)), dim3(kThreads), 0, st>>>(
            ids, m, row, R, rule, OvTable{t, reinterpret_cast<uint32_t*>(t + cap), cap - 1}, OvOut{}, os.res.get());
        ENC_OK(hipGetLastError());
        ENC_OK(hipMemcpyAsync(os.host.get(), os.res.get(), 24, hipMemcpyDeviceToHost, st));
        return 0;
      });
  if (r < 0) return r;
  OverlapState& os = *state;  // the new set is complete: it replaces the old one
  os.tab[os.cur].reset();
  os.cur = 1 - os.cur;
  os.has = true, os.rule = rule, os.mask = cap - 1;
  os.grams = os.host[1], os.distinct = os.host[2];
  return (int64_t)os.grams;
}

int64_t EncodeDevice::overlap_refs_host(const int32_t* ids, size_t m, const int64_t* row_off, size_t rows, int w,
                                        uint64_t seed) {
  if (!m) return overlap_refs(nullptr, 0, nullptr, 0, w, seed, nullptr, nullptr);
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  OverlapState& os = pass_state<OverlapState>(pass_[kOverlap]);
  hipStream_t st = (hipStream_t)stream_;
  if (!os.hids.grow(m) || (row_off && !os.hrow.grow(rows + 1))) {
    std::fprintf(stderr, "[ERROR]\t encoder: overlap reference staging allocation failed (%zu ids, %zu rows)\n", m, rows);
    return -1;
  }
  ENC_OK(hipMemcpyAsync(os.hids.get(), ids, m * 4, hipMemcpyHostToDevice, st));
  if (row_off) ENC_OK(hipMemcpyAsync(os.hrow.get(), row_off, (rows + 1) * 8, hipMemcpyHostToDevice, st));
  return overlap_refs(os.hids.get(), m, row_off ? os.hrow.get() : nullptr, rows, w, seed, nullptr, nullptr);
}

void EncodeDevice::overlap_stats(uint64_t* table_bytes, uint64_t* ref_grams, uint64_t* distinct) const {
  const OverlapState* os = static_cast<const OverlapState*>(pass_[kOverlap].get());
  const bool has = os && os->has;
  if (table_bytes) *table_bytes = has ? 12 * (os->mask + 1) : 0;
  if (ref_grams) *ref_grams = has ? os->grams : 0;
  if (distinct) *distinct = has ? os->distinct : 0;
}

int64_t EncodeDevice::overlap(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, int64_t* hits,
                              int64_t* covered, int64_t* first, int64_t* tok_ref, uint8_t* tok_cov, void* stream,
                              double* kernel_ms) {
  const u64 R = row_off ? rows : 1;
  const int64_t* row = row_off;
  OverlapState* state = nullptr;
  const OvOut out{(unsigned long long*)hits, (unsigned long long*)covered, (unsigned long long*)first, tok_ref, tok_cov, 0};
  const int64_t r = device_call<OverlapState>(
      pass_[kOverlap], device_, stream ? stream : stream_, "overlap", R, kernel_ms,
      [&](OverlapState& os, hipStream_t st, Plan* p) {
        state = &os;
        const int bad = overlap_offsets(os, n, row_off, R, st, &row);
        if (bad < 0) return bad;
        *p = Plan{0, R != 0, n};
        return 0;
      },
      [&](OverlapState& os, hipStream_t st) { return overlap_run(os, ids, n, row, R, out, st); });
  return r < 0 || !R ? r : (int64_t)state->host[0];
}

// Host rows in pieces of whole rows (host_pieces).  A piece is the device passes on its own rows; the
// caller has validated row_off, so no check runs.  No gram crosses a row, so a row's result does not
// depend on the piece; `first` is rebased by the piece's first id, and the per-token outputs, which
// host_pieces does not know, come back at that id behind the passes.
int64_t EncodeDevice::overlap_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, int64_t* hits,
                                   int64_t* covered, int64_t* first, int64_t* tok_ref, uint8_t* tok_cov) {
  OverlapState& os = pass_state<OverlapState>(pass_[kOverlap]);
  hipStream_t st = (hipStream_t)stream_;
  const int64_t one[2] = {0, (int64_t)n};
  const HostCall call{"overlap", row_off ? rows : 1, 0, 1, {{ids, n, row_off ? row_off : one}}, false, nullptr,
                      3,         {{hits, 8, 1, 0}, {covered, 8, 1, 0}, {first, 8, 1, 0}}};
  int64_t total = 0;
  const int r = host_pieces(
      device_, st, call, [](size_t) { return (u64)1; },
      [&](const Piece& p, Staged* s) {
        const size_t m = p.r1 - p.r0, len = std::max<size_t>(p.len[0], 1);
        if (!tiles_fit(p.len[0]) || !os.reserve(m) || !os.hids.grow(len) || !os.hrow.grow(m + 1) ||
            !os.hrows.grow(m, 3) || (tok_ref && !os.href.grow(len)) || (tok_cov && !os.hcov.grow(len)))
          return false;
        s->ids[0] = os.hids.get(), s->row[0] = os.hrow.get();
        for (int k = 0; k < 3; ++k) s->out[k] = os.hrows.get() + (size_t)k * os.hrows.cap();
        return true;
      },
      [&](const Piece& p, const Staged& s) {
        const OvOut out{s.get<unsigned long long>(0), s.get<unsigned long long>(1), s.get<unsigned long long>(2),
                        tok_ref ? os.href.get() : nullptr, tok_cov ? os.hcov.get() : nullptr, (u64)p.a[0]};
        if (overlap_run(os, s.ids[0], p.len[0], s.row[0], p.r1 - p.r0, out, st) < 0) return -1;
        if (tok_ref && p.len[0])
          ENC_OK(hipMemcpyAsync(tok_ref + p.a[0], os.href.get(), p.len[0] * 8, hipMemcpyDeviceToHost, st));
        if (tok_cov && p.len[0])
          ENC_OK(hipMemcpyAsync(tok_cov + p.a[0], os.hcov.get(), p.len[0], hipMemcpyDeviceToHost, st));
        ENC_OK(hipStreamSynchronize(st));
        total += (int64_t)os.host[0];
        return 0;
      });
  return r < 0 ? r : total;
}

}  // namespace shred
