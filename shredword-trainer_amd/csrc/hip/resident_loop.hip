// MI355X (gfx950) whole-chip resident merge loop: k_resident and ResidentLoop (resident_loop.h),
// the host class that plans, launches and talks to it.  Device (bpe_device.hip) chooses between this
// loop, the indexed loop (word_loop.hip) and the launch path, and decides what a collected merge or
// an aborted launch means; hip_common.h holds what the units share.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>

#include "../host/resident_loop.h"
#include "hip_common.h"

namespace shred {

namespace {

// ------------------------------------------------------------------------------------------
// K2+K3 resident: the merge loop as ONE persistent launch with the word table held in LDS.
//
// When the types table fits the chip's LDS (256 CUs x ~100 KB: C2's 17 MB), workgroup w (one
// per CU) copies its contiguous range of tiles and their word weights into LDS once and keeps
// them there for the whole merge loop, so a merge never reads the table from HBM.  The host
// posts each merge in a mailbox in pinned host memory; workgroup 0 (the leader) is the only
// poller of host memory (pollers of one host line serialise over PCIe: 256 of them cost 200 us
// per command on MI355X, one costs ~3 us) and hands the merge to its participants — the owners
// of the merge's candidate tiles from the host tile index, or every workgroup — through one
// 8-byte go word per workgroup on a 128-B line of its own (sc1 store after the sc1 command
// stores and a vmcnt drain; each workgroup polls only its own word).  A participant applies the
// merge to its tiles in LDS exactly as k_merge does to a single-chunk tile, reduces the
// neighbour deltas in an LDS hash, publishes them to its region, and takes a ticket among the
// participants; the last one gathers the regions into the host-visible records and raises the
// host flag, as k_merge's fused completion does.  A STOP command (or a poll time-out) writes the
// tiles back to HBM and ends the launch, so the HBM stream is current whenever the host uses it.
constexpr int kResDeltaW = 1024;         // LDS delta slots per workgroup (spills go to HBM)
constexpr int kResSigBits = 4096;        // per-tile pair signature held in LDS (Bloom, 2 hashes)
constexpr int kResSigWords = kResSigBits / 32;
constexpr uint32_t kResSigRebuild = 192;  // pairs added to a tile's signature before it is rebuilt
constexpr uint32_t kOpMerge = 1, kOpStop = 2, kOpTimeout = 3;

// host command ring, device command ring, per-workgroup queues: at most 10 commands are ever
// outstanding (Device::rollback), so no entry is overwritten before it is read
constexpr uint32_t kResRing = 16;
// Workgroup roles: 0 dispatches the host's commands, 1 completes every merge (gathers the
// participants' records to the host), 2 .. grid-1 own the tiles.
constexpr uint32_t kResGatherWg = 1, kResFirstWorker = 2;
constexpr int kResGatherBatch = 16;  // records per gatherer thread per round trip
constexpr int kResThreadsHbm = 512;  // k_resident block size when the tokens stay in HBM
static_assert(kResDeltaW < (1 << 12) && kResMaxTiles * kWaveTok < (1u << 22), "region header fields (k_resident)");
constexpr uint32_t kOpUnmerge = 4;
// k_resident: not every workgroup became resident within the leader's bound (another kernel or
// process holds CUs); every workgroup leaves without touching the table, the host falls back
constexpr uint32_t kOpAbort = 5;

// One host command (pinned host memory, written by the host; only the leader reads it).
// Every field is an 8-byte granule {seq, value} written by one aligned 8-byte store, so the
// leader reads the whole command in ONE round trip (13 lanes, one granule each) and takes it
// only when every granule carries the command number: no ordering between the host's stores or
// the device's loads is needed.  The command for number s lives in cmd[s % kResRing].
constexpr int kCmdOp = 0, kCmdA = 1, kCmdB = 2, kCmdX = 3, kCmdSlotN = 4, kCmdMask = 5;  // mask: 8 granules
constexpr int kCmdGranules = 13;
struct ResCmd {
  uint64_t g[16];  // g[k] = seq | value << 32
};
struct ResMbox {
  ResCmd cmd[kResRing];
};

// The per-merge device tables and host-visible buffers of one slot (as k_merge's MergeSlot).
struct ResSlot {
  u64* dsum;
  u64* dft;
  uint32_t* dlist;
  uint32_t* dcount;   // [0] touched global slots
  uint32_t* done;     // [8]: participants that published their region (the gatherer resets it)
  DeltaRecord* out;   // host-visible records
  uint32_t* hcount;   // host-visible: [0] records, [1] flag = seq, [2] matched tiles
  u64* hstats;        // host-visible: [0] occurrences, [1] tokens rewritten, [2] device ticks of the merge
  uint32_t* hmlist;   // host-visible matched tiles
  uint32_t* rhdr;     // per-participant regions (as k_merge's)
  u64* rrec;
  uint32_t* rtile;
};

struct ResParams {
  int32_t* tok;
  const uint64_t* tile_off;
  uint32_t* tile_len;
  const uint64_t* weight;
  const uint32_t* wg_tiles;  // grid + 1: workgroup w owns tiles [wg_tiles[w], wg_tiles[w+1])
  const uint32_t* wg_rank;   // grid + 1: ... and the weights of ranks [wg_rank[w], wg_rank[w+1])
  const uint32_t* tile_lofs; // per tile: word offset in its owner's LDS token area (multiple of 4)
  uint32_t tok_words;        // LDS token area (words, multiple of 4, incl. one chunk of read slack)
  uint32_t w_words;          // LDS weight area (u64 entries, even)
  const ResMbox* mbox;
  uint32_t* cmd;             // device command ring: kResRing x 8 words [a, b, X, nparts, slot, op, stamp lo, hi]
  u64* q;                    // per-workgroup queues: kResRing entries each (zeroed before the launch)
  uint32_t* status;          // host-visible: [0] kOpTimeout / kOpAbort when the launch ended itself,
                             //   [2] 1 once every workgroup was seen resident
  uint32_t* arrive;          // workgroups that started (zeroed before the launch)
  uint32_t arrive_polls;     // the leader's bound on waiting for them
  uint32_t seq0;             // first command number of this launch
  uint32_t leader_polls;     // idle leader iterations before the launch ends itself
  uint32_t keys_per_merge, slot_cap;
  uint32_t sig_words;        // LDS signature words per tile (kResSigWords, or a half / quarter of it)
  uint32_t w_global;         // 1: the weights stay in HBM (w_words = 0), read per matched occurrence
  uint32_t region_keys;      // a participant with more LDS delta keys adds them to the global tables
  uint32_t mt_dense;         // more matched tiles than this: the host index marks X in every tile
  uint32_t mt_words;         // the matched tiles go to the host as a bitmap of this many u32 words
  ResSlot sl[ResidentLoop::kSlots];  // merge X uses sl[X % kSlots]
  uint32_t* dbg;      // diagnostic (SHREDWORD_RESIDENT_DEBUG): per workgroup [phase, last seq, pi, T]
  u64* stamps;        // diagnostic: per participant [go seen, work done, loop cycles, -] (s_memrealtime)
};

struct ResDelta {
  uint32_t key[kResDeltaW];
  u64 sum[kResDeltaW];
  u64 ft[kResDeltaW];
  uint32_t spill;
};

// Queue entry: two 8-byte halves, each tagged with this workgroup's entry number (count, 1-based,
// 16 bits); a reader takes the entry when both halves carry the count it expects.
//   half 0: count 16 | pi 8 | op 3 | slot 2 | T 9 | a 20     half 1: count 16 | b 20 | X 20
__device__ __forceinline__ void q_pack(uint32_t cnt, uint32_t pi, uint32_t op, uint32_t slot, uint32_t T, int32_t a,
                                       int32_t b, int32_t X, u64* h0, u64* h1) {
  const u64 c = cnt & 0xFFFFu;
  *h0 = c | ((u64)(pi & 0xFFu) << 16) | ((u64)(op & 7u) << 24) | ((u64)(slot & 3u) << 27) | ((u64)(T & 0x1FFu) << 29) |
        ((u64)((uint32_t)a & 0xFFFFFu) << 38);
  *h1 = c | ((u64)((uint32_t)b & 0xFFFFFu) << 16) | ((u64)((uint32_t)X & 0xFFFFFu) << 36);
}

// sm = the tile signature's bit count - 1 (kResSigBits, or a half / quarter of it when the table
// needs a smaller LDS plan: ResidentLoop::plan)
__device__ __forceinline__ void res_sig_bits(int32_t x, int32_t y, uint32_t* h1, uint32_t* h2, uint32_t sm) {
  uint32_t k = (uint32_t)x * 0x9E3779B1u ^ ((uint32_t)y + 0x7F4A7C15u) * 0x85EBCA77u;
  k ^= k >> 15;
  k *= 0x2C1B3C6Du;
  k ^= k >> 12;
  k *= 0x297A2D39u;
  k ^= k >> 15;
  *h1 = k & sm;
  *h2 = (k >> 16) & sm;
}
__device__ __forceinline__ bool res_sig_test(const uint32_t* sg, int32_t x, int32_t y, uint32_t sm) {
  uint32_t h1, h2;
  res_sig_bits(x, y, &h1, &h2, sm);
  return ((sg[h1 >> 5] >> (h1 & 31)) & 1u) && ((sg[h2 >> 5] >> (h2 & 31)) & 1u);
}
// Rebuilds a tile's LDS signature from its tokens t[0, len) (one wave).
__device__ __forceinline__ void res_sig_build(uint32_t* sg, const int32_t* t, uint32_t len, int lane, uint32_t sm) {
  for (int w = lane; w < (int)((sm + 1) >> 5); w += 64) sg[w] = 0;
  wave_lds_sync();
  for (uint32_t i = (uint32_t)lane; i + 1 < len; i += 64) {
    const int32_t x = t[i], y = t[i + 1];
    if (!is_hdr(x) && !is_hdr(y)) {
      uint32_t h1, h2;
      res_sig_bits(x, y, &h1, &h2, sm);
      atomicOr(&sg[h1 >> 5], 1u << (h1 & 31));
      atomicOr(&sg[h2 >> 5], 1u << (h2 & 31));
    }
  }
  wave_lds_sync();
}


// One wave applies (a, b) -> X to a single-chunk tile held in LDS at tb (live length *len):
// k_merge's per-chunk logic with no carries (the tile is its own first and last chunk).
// Returns the occurrences merged; the tile is compacted in place and *len updated.
// This lane's 16 tokens of a tile (four 16-B loads).
struct TileRegs {
  int4 q[kPer / 4];
};
__device__ __forceinline__ void res_load_tile(const int32_t* tb, int lane, TileRegs* r) {
  const int p0 = lane * kPer;
#pragma unroll
  for (int q = 0; q < kPer / 4; ++q) r->q[q] = *reinterpret_cast<const int4*>(tb + p0 + 4 * q);
}

// The per-launch plan the merge body needs beside the tile: signature mask, and where the word
// weights live (LDS s_w from rank r0, or HBM when the table's weights do not fit LDS).
struct ResPlan {
  uint32_t sm;
  const u64* gw;  // non-null: weights from HBM (indexed by rank)
};

template <bool kWeighted>
__device__ __forceinline__ uint32_t res_merge_body(int32_t* tb, const TileRegs& tr, uint32_t* lenp, uint32_t* sg,
                                                   uint32_t* sgadd, int32_t* st, const u64* s_w, uint32_t r0, int32_t a,
                                                   int32_t b, int32_t X, ResDelta& h, const ResSlot& p,
                                                   uint32_t slot_cap, int lane, u64* n_written, const ResPlan& rp);

template <bool kWeighted>
__device__ __forceinline__ uint32_t res_merge_tile(int32_t* tb, uint32_t* lenp, uint32_t* sg, uint32_t* sgadd, int32_t* st,
                                                   const u64* s_w,
                                                   uint32_t r0, int32_t a, int32_t b, int32_t X, ResDelta& h,
                                                   const ResSlot& p, uint32_t slot_cap, int lane, u64* n_written,
                                                   const ResPlan& rp) {
  if (!res_sig_test(sg, a, b, rp.sm)) return 0;  // the pair cannot be in this tile
  TileRegs tr;
  res_load_tile(tb, lane, &tr);
  return res_merge_body<kWeighted>(tb, tr, lenp, sg, sgadd, st, s_w, r0, a, b, X, h, p, slot_cap, lane, n_written, rp);
}

// The merge of one tile whose 16 tokens per lane are already in registers (tr).
template <bool kWeighted>
__device__ __forceinline__ uint32_t res_merge_body(int32_t* tb, const TileRegs& tr, uint32_t* lenp, uint32_t* sg,
                                                   uint32_t* sgadd, int32_t* st, const u64* s_w, uint32_t r0, int32_t a,
                                                   int32_t b, int32_t X, ResDelta& h, const ResSlot& p,
                                                   uint32_t slot_cap, int lane, u64* n_written, const ResPlan& rp) {
  const uint32_t len = *lenp;
  const int p0 = lane * kPer;
  int32_t v[kPer];
#pragma unroll
  for (int q = 0; q < kPer / 4; ++q) {
    v[4 * q] = tr.q[q].x;
    v[4 * q + 1] = tr.q[q].y;
    v[4 * q + 2] = tr.q[q].z;
    v[4 * q + 3] = tr.q[q].w;
  }
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if ((uint32_t)(p0 + j) >= len) v[j] = kPad;
  int32_t nx = wave_next(v[0]);
  if (lane == 63) nx = kPad;
  bool any = false;
#pragma unroll
  for (int j = 0; j < kPer; ++j) any |= (v[j] == a) & ((j + 1 < kPer ? v[j + 1] : nx) == b);
  if (!__any(any)) return 0;
  const bool same = (a == b);
  const uint32_t cl = len;
#pragma unroll
  for (int j = 0; j < kPer; ++j) st[SK(2 + p0 + j)] = v[j];
  if (lane == 0) {
    st[SK(0)] = kPad;
    st[SK(1)] = kPad;
  }
  if (lane == 63) {
    st[SK(2 + kWaveTok)] = kPad;
    st[SK(3 + kWaveTok)] = kPad;
  }
  wave_lds_sync();
  uint32_t mask = 0;
  if (same) {
    u64 nl = 0;  // last index whose token != a, + 1 (0 = none)
#pragma unroll
    for (int j = 0; j < kPer; ++j)
      if (v[j] != a) nl = (u64)(p0 + j) + 1;
    const u64 inc = wave_scan_max64(nl);
    long long last = (long long)wave_prev64(inc) - 1;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const long long gi = (long long)(p0 + j);
      if (v[j] != a) last = gi;
      else if ((j + 1 < kPer ? v[j + 1] : nx) == a && ((gi - last - 1) & 1) == 0) mask |= 1u << j;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kPer; ++j)
      if (v[j] == a && (j + 1 < kPer ? v[j + 1] : nx) == b) mask |= 1u << j;
  }
  uint32_t prevm = wave_prev(mask);
  if (lane == 0) prevm = 0;
  const uint32_t m_ext = (mask << 2) | ((prevm >> 14) & 3u);  // bit k <-> position p0 - 2 + k
  const uint32_t removed = (m_ext >> 1) & 0xFFFFu;           // bit j <-> match at p0 + j - 1
  const int valid = max(0, min(kPer, (int)cl - p0));
  const uint32_t vmask = valid >= kPer ? 0xFFFFu : ((1u << valid) - 1u);
  const int kc = __popc(~removed & vmask);
  const int nm = __popc(mask);
  uint32_t hmask = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (is_hdr(v[j])) hmask |= 1u << j;
  hmask &= vmask;
  u64 hl = 0;
  if (hmask) {
    const int j = 31 - __clz(hmask);
    hl = ((u64)(p0 + j + 1) << 32) | hdr_rank(st[SK(2 + p0 + j)]);
  }
  const u64 hinc = wave_scan_max64(hl);
  const u64 hdr_ex = wave_prev64(hinc);
  const int cinc = wave_incl_sum(kc | (nm << 16));
  const int ctot = (int)lane_read((uint32_t)cinc, 63);
  const int kc_ex = (cinc - (kc | (nm << 16))) & 0xFFFF;
  const int kept = ctot & 0xFFFF;
  const int matches = ctot >> 16;
  if (mask) {
    const u64 hdr_in = lane == 0 ? 0ull : hdr_ex;
    for (uint32_t mrem = mask; mrem; mrem &= mrem - 1) {
      const int j = __ffs(mrem) - 1;
      const uint32_t hb = hmask & ((2u << j) - 1u);
      u64 hdr = hdr_in;
      if (hb) {
        const int jh = 31 - __clz(hb);
        hdr = ((u64)(p0 + jh + 1) << 32) | hdr_rank(st[SK(2 + p0 + jh)]);
      }
      const uint32_t hidx = (uint32_t)(hdr >> 32) - 1u;
      const uint32_t rank = (uint32_t)hdr;
      const uint32_t gi = p0 + j;
      const u64 w = kWeighted ? (rp.gw ? rp.gw[rank] : s_w[rank - r0]) : 1ull;
      const u64 ftb = ((u64)rank << 32) | ((u64)(gi - hidx - 1u) << 2);
      const bool vl = gi - 1u > hidx;  // a left neighbour inside the word (X if it was just merged)
      const int32_t left = ((m_ext >> j) & 1u) ? X : st[SK(1 + p0 + j)];
      const int32_t right = st[SK(4 + p0 + j)];  // the original token after b
      const bool vr = !is_hdr(right);
      const uint32_t sl = slot_of(left, slot_cap) << 2, sr = slot_of(right, slot_cap) << 2;
      const uint32_t key[4] = {sl | kOldLeft, sl | kNewLeft, sr | kOldRight, sr | kNewRight};
      const bool val[4] = {vl, vl, vr, vr};
      // the four slots are probed together (their CAS round trips overlap), then summed
      uint32_t slot[4];
      bool pend[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        slot[k] = (key[k] * 2654435761u) >> (32 - __builtin_ctz(kResDeltaW));
        pend[k] = val[k];
      }
      for (int probe = 0; probe < 16 && (pend[0] | pend[1] | pend[2] | pend[3]); ++probe) {
        uint32_t prev[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) prev[k] = pend[k] ? atomicCAS(&h.key[slot[k]], kEmpty32, key[k]) : key[k];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (pend[k]) {
            if (prev[k] == kEmpty32 || prev[k] == key[k]) pend[k] = false;
            else slot[k] = (slot[k] + 1) & (kResDeltaW - 1);
          }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!val[k]) continue;
        if (pend[k]) {  // the LDS hash is full around these slots: the global tables take it
          h.spill = 1;
          delta_global(p, key[k], w, ftb | (u64)(k));
        } else {
          atomicAdd(&h.sum[slot[k]], w);
          atomicMin(&h.ft[slot[k]], ftb | (u64)(k));
        }
      }
      // the tile's signature gains the new pairs (a superset stays valid; rebuilt when loose)
      uint32_t h1, h2, h3, h4;
      res_sig_bits(left, X, &h1, &h2, rp.sm);
      res_sig_bits(X, right, &h3, &h4, rp.sm);
      atomicOr(&sg[h1 >> 5], vl ? 1u << (h1 & 31) : 0u);
      atomicOr(&sg[h2 >> 5], vl ? 1u << (h2 & 31) : 0u);
      atomicOr(&sg[h3 >> 5], vr ? 1u << (h3 & 31) : 0u);
      atomicOr(&sg[h4 >> 5], vr ? 1u << (h4 & 31) : 0u);
    }
  }
  wave_lds_sync();  // every neighbour read is done: compact in place
  // branch-free: a dropped position writes this lane's trash word past the staging area
  int o = kc_ex;
  const int trash = kStPad + lane;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const bool keep = j < valid && !((removed >> j) & 1u);
    st[keep ? SK(2 + o) : trash] = ((mask >> j) & 1u) ? X : v[j];
    o += keep ? 1 : 0;
  }
  // a tile whose signature gathered many added pairs since its last build is re-signed below
  const uint32_t added = *sgadd + 2u * (uint32_t)matches;
  const bool rebuild = added > (kResSigRebuild * (rp.sm + 1)) / (uint32_t)kResSigBits;  // scaled with the signature
  if (rebuild)
    for (int w = lane; w < (int)((rp.sm + 1) >> 5); w += 64) sg[w] = 0;
  wave_lds_sync();
  int32_t c[kPer + 1];  // this lane's compacted tokens (kPad past the end) and the next one
#pragma unroll
  for (int j = 0; j <= kPer; ++j) {
    const int32_t t = st[SK(2 + p0 + j)];
    c[j] = p0 + j < kept ? t : kPad;
  }
#pragma unroll
  for (int q = 0; q < kPer / 4; ++q) {
    if (p0 + 4 * q < kept) {
      int4 x;
      x.x = c[4 * q];
      x.y = c[4 * q + 1];
      x.z = c[4 * q + 2];
      x.w = c[4 * q + 3];
      *reinterpret_cast<int4*>(tb + p0 + 4 * q) = x;
    }
  }
  if (lane == 0) *lenp = (uint32_t)kept;
  *n_written += (u64)kept;
  if (rebuild) {
#pragma unroll
    for (int j = 0; j < kPer; ++j) {  // signature of the compacted tile (OR of 0 where no pair)
      uint32_t h1, h2;
      res_sig_bits(c[j], c[j + 1], &h1, &h2, rp.sm);
      const bool pr = !is_hdr(c[j]) && !is_hdr(c[j + 1]);
      atomicOr(&sg[h1 >> 5], pr ? 1u << (h1 & 31) : 0u);
      atomicOr(&sg[h2 >> 5], pr ? 1u << (h2 & 31) : 0u);
    }
  }
  if (lane == 0) *sgadd = rebuild ? 0u : added;
  wave_lds_sync();
  return (uint32_t)matches;
}

// One wave expands every X in a single-chunk tile held in LDS back into (a, b) — the undo of a
// speculative merge that the host did not confirm; the tile's length grows back, within its
// original LDS capacity.  The signature is rebuilt exactly.
__device__ __forceinline__ void res_unmerge_tile(int32_t* tb, uint32_t* lenp, uint32_t* sg, uint32_t* sgadd, int32_t* st,
                                                 int32_t a, int32_t b, int32_t X, int lane, uint32_t sm) {
  const uint32_t len = *lenp;
  const int p0 = lane * kPer;
  int32_t v[kPer];
#pragma unroll
  for (int q = 0; q < kPer / 4; ++q) {
    const int4 x = *reinterpret_cast<const int4*>(tb + p0 + 4 * q);
    v[4 * q] = x.x;
    v[4 * q + 1] = x.y;
    v[4 * q + 2] = x.z;
    v[4 * q + 3] = x.w;
  }
  int nx = 0;  // this lane's X count
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if ((uint32_t)(p0 + j) >= len) v[j] = kPad;
    nx += v[j] == X ? 1 : 0;
  }
  if (!__any(nx != 0)) return;
  const int inc = wave_incl_sum(nx);
  const int total = (int)lane_read((uint32_t)inc, 63);
  const int nlen = (int)len + total;  // <= the tile's LDS capacity: the merge removed these tokens
  int o = p0 + inc - nx;              // this lane's first output position
  const int trash = kStPad + lane;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const bool live = (uint32_t)(p0 + j) < len;
    const bool isx = live && v[j] == X;
    st[live ? SK(o) : trash] = isx ? a : v[j];
    st[isx ? SK(o + 1) : trash] = b;
    o += live ? (isx ? 2 : 1) : 0;
  }
  wave_lds_sync();
  for (int i = lane; i < (int)((sm + 1) >> 5); i += 64) sg[i] = 0;
  int32_t c[kPer + 1];
#pragma unroll
  for (int j = 0; j <= kPer; ++j) {
    const int32_t t = st[SK(p0 + j)];
    c[j] = p0 + j < nlen ? t : kPad;
  }
#pragma unroll
  for (int q = 0; q < kPer / 4; ++q) {
    if (p0 + 4 * q < nlen) {
      int4 x;
      x.x = c[4 * q];
      x.y = c[4 * q + 1];
      x.z = c[4 * q + 2];
      x.w = c[4 * q + 3];
      *reinterpret_cast<int4*>(tb + p0 + 4 * q) = x;
    }
  }
  wave_lds_sync();
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    uint32_t h1, h2;
    res_sig_bits(c[j], c[j + 1], &h1, &h2, sm);
    const bool pr = !is_hdr(c[j]) && !is_hdr(c[j + 1]);
    atomicOr(&sg[h1 >> 5], pr ? 1u << (h1 & 31) : 0u);
    atomicOr(&sg[h2 >> 5], pr ? 1u << (h2 & 31) : 0u);
  }
  if (lane == 0) {
    *lenp = (uint32_t)nlen;
    *sgadd = 0;
  }
  wave_lds_sync();
}

// kLdsTok: the tokens live in LDS (the table fits the chip's LDS); otherwise they stay in HBM
// (read and rewritten in place by their owner workgroup only) and LDS holds the weights and the
// tile signatures, which is what decides which tiles a merge reads at all.
template <bool kWeighted, bool kLdsTok>
__global__ __launch_bounds__(kLdsTok ? 256 : kResThreadsHbm) void k_resident(ResParams p) {
  constexpr int kRT = kLdsTok ? 256 : kResThreadsHbm;  // threads: more waves hide the HBM tile loads
  constexpr int kRW = kRT / 64;
  constexpr int kGB = kLdsTok ? kResGatherBatch : kResGatherBatch / 4;  // gatherer loads in flight per thread
  extern __shared__ __align__(16) int32_t s_dyn[];
  int32_t* s_res = s_dyn;                                     // the tiles' tokens
  u64* s_w = reinterpret_cast<u64*>(s_dyn + p.tok_words);     // the words' weights
  uint32_t* s_sig = reinterpret_cast<uint32_t*>(s_dyn + p.tok_words + 2 * p.w_words);  // per-tile signatures
  const uint32_t sw = p.sig_words;
  const ResPlan rplan{sw * 32u - 1u, p.w_global ? reinterpret_cast<const u64*>(p.weight) : nullptr};
  __shared__ int32_t s_tok[kRW][kStPad + 64];  // + a trash word per lane (branch-free compaction)
  __shared__ ResDelta h;
  __shared__ uint32_t s_len[kResMaxTiles], s_lofs[kResMaxTiles], s_sigadd[kResMaxTiles];
  __shared__ u64 s_toff[kResMaxTiles];
  __shared__ uint32_t s_mt[kResMaxTiles];
  __shared__ uint8_t s_lm[kResMaxTiles];   // per tile: bit X % 8 set when merge X matched there
  __shared__ uint32_t s_qc[kMaxMergeGroups];  // leader: entries written to each workgroup's queue
  __shared__ uint32_t s_nmt, s_nrec, s_nkeys;
  __shared__ uint32_t s_cmd[8];
  __shared__ u64 s_cnt[2];
  __shared__ u64 s_tlead;
  __shared__ u64 s_ts[4];      // diagnostic (stamps): the gatherer's phase ends
  __shared__ uint32_t s_nout;  // the last participant: records written to the host
  __shared__ uint32_t s_pre[kMaxMergeGroups + 1], s_pmt[kMaxMergeGroups + 1];
  __shared__ uint32_t s_wtot[2][kRW];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint32_t G = gridDim.x, me = blockIdx.x;
  const uint32_t t0 = p.wg_tiles[me], nt = p.wg_tiles[me + 1] - t0;
  const uint32_t r0 = p.wg_rank[me], nr = p.wg_rank[me + 1] - r0;
  int32_t* st = s_tok[wid];
  // ---- co-residency: every workgroup counts itself in; the leader dispatches nothing until all
  // have (below), so a launch that is only partly resident aborts instead of hanging
  if (threadIdx.x == 0) __hip_atomic_fetch_add(p.arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  // ---- residency: tiles, weights and signatures into LDS
  for (uint32_t i = threadIdx.x; i < nt; i += kRT) {
    s_len[i] = p.tile_len[t0 + i];
    s_lofs[i] = p.tile_lofs[t0 + i];
    s_toff[i] = p.tile_off[t0 + i];
    s_sigadd[i] = 0;
    s_lm[i] = 0;
  }
  for (uint32_t i = threadIdx.x; i < G; i += kRT) s_qc[i] = 0;
  for (int i = threadIdx.x; i < kResDeltaW; i += kRT) {
    h.key[i] = kEmpty32;
    h.sum[i] = 0;
    h.ft[i] = kEmpty64;
  }
  if (kWeighted)
    for (uint32_t i = threadIdx.x; nr && !p.w_global && i < nr; i += kRT) s_w[i] = p.weight[r0 + i];
  if (threadIdx.x == 0) h.spill = 0;
  __syncthreads();
  auto tile_ptr = [&](uint32_t i) -> int32_t* {
    if constexpr (kLdsTok) return s_res + s_lofs[i];
    else return p.tok + s_toff[i];
  };
  for (uint32_t i = wid; i < nt; i += kRW) {
    if constexpr (kLdsTok) {
      const int32_t* src = p.tok + s_toff[i];
      int32_t* dst = s_res + s_lofs[i];
      const uint32_t n4 = (s_len[i] + 3u) >> 2;
      for (uint32_t q = (uint32_t)lane; q < n4; q += 64)
        *reinterpret_cast<int4*>(dst + 4 * q) = *reinterpret_cast<const int4*>(src + 4 * q);
      wave_lds_sync();
    }
    res_sig_build(s_sig + (size_t)i * sw, tile_ptr(i), s_len[i], lane, rplan.sm);
  }
  __syncthreads();

  uint32_t expect = p.seq0;  // leader: the next host command
  uint32_t idle = 0;         // leader: polls without a command
  uint32_t consumed = 0;     // thread 0: entries taken from this workgroup's queue
  uint32_t exit_op = kOpStop;
  const u64* myq = p.q + (size_t)me * kResRing * 2;
  if (me == 0 && wid == 0) {  // the leader waits (bounded) until every workgroup is resident
    bool all = false;
    for (uint32_t k = 0; k < p.arrive_polls && !all; ++k) {
      all = __hip_atomic_load(p.arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= G;
      if (!all) __builtin_amdgcn_s_sleep(8);
    }
    if (lane == 0) {
      if (all) {
        __hip_atomic_store(p.status + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      } else {  // an abort as the first entry of every queue (the missing workgroups read it when
                // they start, after the host has moved on to another stream)
        for (uint32_t wg = 0; wg < G; ++wg) {
          u64 h0, h1;
          q_pack(1, 0, kOpAbort, 0, G, 0, 0, 0, &h0, &h1);
          u64* e = p.q + (size_t)wg * kResRing * 2;
          __hip_atomic_store(e, h0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(e + 1, h1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __threadfence_system();
        __hip_atomic_store(p.status, kOpAbort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      s_cmd[7] = all ? 1u : 0u;
    }
  }
  __syncthreads();
  if (me == 0 && s_cmd[7] == 0) return;  // aborted: the table was not touched
  for (;;) {
    // ---- the leader hands out the next host command, if one is posted (one poll per pass)
    if (me == 0 && wid == 0) {
      const uint64_t* hc = p.mbox->cmd[expect % kResRing].g;
      // lane k < kCmdGranules reads granule k: the whole command in one round trip
      const u64 gv = lane < kCmdGranules ? __hip_atomic_load(hc + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0ull;
      const bool tagged = lane >= kCmdGranules || (uint32_t)gv == expect;
      const bool ready = __all(tagged);
      const uint32_t val = (uint32_t)(gv >> 32);
      uint32_t op = 0;
      if (ready) {
        op = (uint32_t)__shfl((int)val, kCmdOp, 64);
        idle = 0;
      } else if (++idle >= p.leader_polls) {
        op = kOpTimeout;  // nobody posts any more: every workgroup writes back and leaves
      }
      if (op) {
        const int32_t a = __shfl((int)val, kCmdA, 64), b = __shfl((int)val, kCmdB, 64), X = __shfl((int)val, kCmdX, 64);
        const uint32_t sn = (uint32_t)__shfl((int)val, kCmdSlotN, 64);
        const bool merge_like = ready && (op == kOpMerge || op == kOpUnmerge);
        // lane l covers workgroups 4l .. 4l+3: its mask nibble, participant indices by a wave scan
        const uint32_t mw = (uint32_t)__shfl((int)val, kCmdMask + (lane >> 3), 64);
        uint32_t nib = merge_like ? (mw >> ((lane & 7) * 4)) & 0xFu : 0xFu;
        if (4u * (uint32_t)lane >= G) nib = 0;
        for (int k = 0; k < 4; ++k)
          if (4u * lane + k >= G) nib &= ~(1u << k);
        const uint32_t cnt = __popc(nib);
        const uint32_t incl = wave_scan_add(cnt);
        const uint32_t T = merge_like ? lane_read(incl, 63) : G;
        uint32_t pi = incl - cnt;
        if (lane == 0 && merge_like) {
          uint32_t* dc = p.cmd + ((uint32_t)X % kResRing) * 8;
          __hip_atomic_store(reinterpret_cast<u64*>(dc + 6), (u64)__builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!((nib >> k) & 1u)) continue;
          const uint32_t wg = 4u * lane + k;  // distinct workgroups per lane: the counters need no atomics
          const uint32_t c = ++s_qc[wg];
          u64 h0, h1;
          q_pack(c, pi++, op, sn & 3u, T, a, b, X, &h0, &h1);
          u64* e = p.q + ((size_t)wg * kResRing + ((c - 1) % kResRing)) * 2;
          __hip_atomic_store(e, h0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(e + 1, h1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        ++expect;
      }
      if (lane == 0) s_cmd[7] = op;
    }
    // ---- this workgroup's next queue entry (the leader's workgroup never blocks here)
    if (threadIdx.x == 0) {
      const uint32_t want = (consumed + 1) & 0xFFFFu;
      const u64* e = myq + (consumed % kResRing) * 2;
      u64 h0 = 0, h1 = 0;
      bool got = false;
      for (;;) {
        h0 = __hip_atomic_load(e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        h1 = __hip_atomic_load(e + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        got = (uint32_t)(h0 & 0xFFFFu) == want && (uint32_t)(h1 & 0xFFFFu) == want;
        if (got || me == 0) break;
        __builtin_amdgcn_s_sleep(2);
      }
      if (me == 0 && !got && !s_cmd[7]) __builtin_amdgcn_s_sleep(2);
      s_cmd[0] = got ? (uint32_t)(h0 >> 24) & 7u : 0u;
      if (got) {
        ++consumed;
        s_cmd[1] = (uint32_t)(h0 >> 16) & 0xFFu;
        s_cmd[2] = (uint32_t)(h0 >> 27) & 3u;                     // slot
        s_cmd[6] = (uint32_t)(h0 >> 29) & 0x1FFu;                 // T
        s_cmd[3] = (uint32_t)(h0 >> 38) & 0xFFFFFu;               // a
        s_cmd[4] = (uint32_t)(h1 >> 16) & 0xFFFFFu;               // b
        s_cmd[5] = (uint32_t)(h1 >> 36) & 0xFFFFFu;               // X
      }
      s_nmt = 0;
      s_nrec = 0;
      s_nkeys = 0;
      s_cnt[0] = 0;
      s_cnt[1] = 0;
    }
    __syncthreads();
    const uint32_t op = s_cmd[0];
    if (op == 0) continue;  // the leader's workgroup: nothing queued for it yet
    if (op == kOpAbort) return;  // the launch aborted before any merge: nothing to write back
    if (op != kOpMerge && op != kOpUnmerge) {
      exit_op = op;
      break;
    }
    const uint32_t pi = s_cmd[1], slot = s_cmd[2];
    const int32_t a = (int32_t)s_cmd[3], b = (int32_t)s_cmd[4], X = (int32_t)s_cmd[5];
    const uint32_t T = s_cmd[6];
    if (p.dbg && threadIdx.x == 0) {
      p.dbg[me * 4] = 2;
      p.dbg[me * 4 + 1] = (uint32_t)X;
      p.dbg[me * 4 + 2] = pi;
      p.dbg[me * 4 + 3] = T;
    }
    const uint32_t lm_bit = 1u << ((uint32_t)X & 7u);
    if (op == kOpUnmerge) {  // undo merge X, a wrong guess (the host undoes them newest first)
      for (uint32_t i = wid; i < nt; i += kRW)
        if (s_lm[i] & lm_bit) res_unmerge_tile(tile_ptr(i), &s_len[i], s_sig + (size_t)i * sw, &s_sigadd[i], st,
                                      a, b, X, lane, rplan.sm);
      __syncthreads();
      continue;
    }
    const ResSlot& sl = p.sl[slot];

    // ---- the merge over this workgroup's tiles (wave per tile)
    u64 n_merged = 0, n_written = 0;
    auto note = [&](uint32_t i, uint32_t m) {
      if (lane == 0) s_lm[i] = m ? (s_lm[i] | lm_bit) : (s_lm[i] & ~lm_bit);
      if (m) {
        n_merged += m;
        if (lane == 0) s_mt[atomicAdd(&s_nmt, 1u)] = t0 + i;
      }
    };
    if constexpr (kLdsTok) {
      for (uint32_t i = wid; i < nt; i += kRW) {
        const uint32_t m = res_merge_tile<kWeighted>(tile_ptr(i), &s_len[i], s_sig + (size_t)i * sw,
                                                     &s_sigadd[i], st, s_w, r0, a, b, X, h, sl, p.slot_cap, lane,
                                                     &n_written, rplan);
        note(i, m);
      }
    } else {
      // tokens in HBM: a software pipeline per wave, the next candidate tile's tokens load while
      // this one merges (tiles the signature rules out are only noted)
      auto skip_to = [&](uint32_t i) {
        for (; i < nt; i += kRW) {
          if (res_sig_test(s_sig + (size_t)i * sw, a, b, rplan.sm)) break;
          note(i, 0);
        }
        return i;
      };
      uint32_t i = skip_to(wid);
      TileRegs cur;
      if (i < nt) res_load_tile(tile_ptr(i), lane, &cur);
      while (i < nt) {
        const uint32_t j = skip_to(i + kRW);
        TileRegs nxt;
        if (j < nt) res_load_tile(tile_ptr(j), lane, &nxt);
        const uint32_t m = res_merge_body<kWeighted>(tile_ptr(i), cur, &s_len[i], s_sig + (size_t)i * sw,
                                                     &s_sigadd[i], st, s_w, r0, a, b, X, h, sl, p.slot_cap, lane,
                                                     &n_written, rplan);
        note(i, m);
        cur = nxt;
        i = j;
      }
    }
    if (lane == 0) {
      if (n_merged) atomicAdd(&s_cnt[0], n_merged);
      if (n_written) atomicAdd(&s_cnt[1], n_written);
    }
    __syncthreads();
    // ---- publish this participant's deltas, clearing the LDS hash.  Few keys: a region the
    // gatherer reads and combines.  Many keys (the early merges touch most neighbours in every
    // workgroup): straight into the slot's global tables (device-scope Σ and min, the first
    // toucher lists the key), so the gatherer only reads the combined keys instead of combining
    // every participant's records in one workgroup.
    {
      uint32_t mine = 0;
      for (int i = threadIdx.x; i < kResDeltaW; i += kRT) mine += h.key[i] != kEmpty32 ? 1u : 0u;
      mine = wave_scan_add(mine);
      if (lane == 63 && mine) atomicAdd(&s_nkeys, mine);
      __syncthreads();
      const bool to_global = s_nkeys > p.region_keys;
      u64* rr = sl.rrec + (size_t)pi * kDeltaLdsW * 3;
      for (int i = threadIdx.x; i < kResDeltaW; i += kRT) {
        const uint32_t key = h.key[i];
        if (key == kEmpty32) continue;
        if (to_global) {
          delta_global(sl, key, h.sum[i], h.ft[i]);
        } else {
          const uint32_t k = atomicAdd(&s_nrec, 1u);
          __hip_atomic_store(rr + 3 * k, (u64)key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(rr + 3 * k + 1, h.sum[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(rr + 3 * k + 2, h.ft[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        h.key[i] = kEmpty32;
        h.sum[i] = 0;
        h.ft[i] = kEmpty64;
      }
      if (to_global && threadIdx.x == 0) h.spill = 1;
      const uint32_t nmt = s_nmt;
      for (uint32_t i = threadIdx.x; i < nmt; i += kRT)
        __hip_atomic_store(sl.rtile + (size_t)pi * kResMaxTiles + i, s_mt[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      u64* hd = reinterpret_cast<u64*>(sl.rhdr + (size_t)pi * kRegHdr);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave's region stores (and spills) are done
      __syncthreads();
      // the header: two 8-byte words, each tagged with X, stored last; the gatherer polls them
      // (so no ticket and no second drain: the workgroup goes straight on to its next command)
      //   word 0: X 20 | records 12 | matched tiles 16 | spill 1   word 1: X 20 | merged 22 | written 22
      if (threadIdx.x == 0) {
        const u64 x20 = (u64)(uint32_t)X & 0xFFFFFu;
        const u64 w0 = x20 | ((u64)s_nrec << 20) | ((u64)nmt << 32) | ((u64)(h.spill ? 1u : 0u) << 48);
        const u64 w1 = x20 | ((s_cnt[0] & 0x3FFFFFull) << 20) | ((s_cnt[1] & 0x3FFFFFull) << 42);
        __hip_atomic_store(hd, w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(hd + 1, w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        h.spill = 0;
      }
    }
    if (me != kResGatherWg) continue;
    __syncthreads();
    // ---- the gatherer: gather the regions to the host, raise the slot's flag
    uint32_t n = 0, nm = 0;
    if (threadIdx.x == 0)  // the dispatch stamp (per-merge device time), loaded beside the headers
      s_tlead = __hip_atomic_load(reinterpret_cast<const u64*>(p.cmd + ((uint32_t)X % kResRing) * 8 + 6),
                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    {
      u64 merged = 0, written = 0;
      uint32_t spill = 0, my_nrec = 0, my_nmt = 0;
      if (threadIdx.x == 0) {
        s_cnt[0] = 0;
        s_cnt[1] = 0;
        s_nrec = 0;
        s_nout = 0;
      }
      __syncthreads();
      const uint32_t g = threadIdx.x;
      if (g < T) {  // thread g waits for participant g's header, then takes its counts and resets it
        u64* hd = reinterpret_cast<u64*>(sl.rhdr + (size_t)g * kRegHdr);
        const uint32_t x20 = (uint32_t)X & 0xFFFFFu;
        u64 v0, v1;
        for (;;) {
          v0 = __hip_atomic_load(hd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          v1 = __hip_atomic_load(hd + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (((uint32_t)v0 & 0xFFFFFu) == x20 && ((uint32_t)v1 & 0xFFFFFu) == x20) break;
          __builtin_amdgcn_s_sleep(1);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        my_nrec = (uint32_t)(v0 >> 20) & 0xFFFu;
        my_nmt = (uint32_t)(v0 >> 32) & 0xFFFFu;
        spill = (uint32_t)(v0 >> 48) & 1u;
        merged = (v1 >> 20) & 0x3FFFFFull;
        written = (v1 >> 42) & 0x3FFFFFull;
        __hip_atomic_store(hd, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // drained before the flag
        __hip_atomic_store(hd + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (p.stamps) {  // diagnostic: all regions published
        __syncthreads();
        if (threadIdx.x == 0) s_ts[0] = __builtin_amdgcn_s_memrealtime();
      }
      // per-wave totals first (each participant's counts fit 22 bits): one LDS atomic per wave,
      // not one per participant on the same address
      const uint32_t wm = wave_scan_add((uint32_t)merged), ww = wave_scan_add((uint32_t)written);
      const bool any_spill = __any(spill != 0);
      const uint32_t ir = wave_scan_add(my_nrec), im = wave_scan_add(my_nmt);
      if (lane == 63) {
        if (wm) atomicAdd(&s_cnt[0], (u64)wm);
        if (ww) atomicAdd(&s_cnt[1], (u64)ww);
        if (any_spill) atomicOr(&s_nrec, 1u);
        s_wtot[0][wid] = ir;
        s_wtot[1][wid] = im;
      }
      __syncthreads();
      uint32_t br = 0, bm = 0;
      for (int w = 0; w < wid; ++w) {
        br += s_wtot[0][w];
        bm += s_wtot[1][w];
      }
      if (g < T) {
        s_pre[g] = br + ir - my_nrec;
        s_pmt[g] = bm + im - my_nmt;
      }
      if (g == T - 1) {
        s_pre[T] = br + ir;
        s_pmt[T] = bm + im;
      }
      __syncthreads();
      n = s_pre[T];
      nm = s_pmt[T];
      if (p.stamps && threadIdx.x == 0) s_ts[1] = __builtin_amdgcn_s_memrealtime();
      auto owner = [&](const uint32_t* pre, uint32_t i) {
        uint32_t lo = 0, hi = T;
        while (hi - lo > 1) {
          const uint32_t mid = (lo + hi) >> 1;
          if (pre[mid] <= i) lo = mid;
          else hi = mid;
        }
        return lo;
      };
      for (uint32_t i0 = 0; i0 < n; i0 += kRT * kGB) {
        u64 r[kGB][3];
#pragma unroll
        for (int k = 0; k < kGB; ++k) {
          const uint32_t i = i0 + k * kRT + threadIdx.x;
          if (i < n) {
            const uint32_t o = owner(s_pre, i);
            const u64* src = sl.rrec + ((size_t)o * kDeltaLdsW + (i - s_pre[o])) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) r[k][c] = __hip_atomic_load(src + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
        if (p.stamps && i0 == 0) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __syncthreads();
          if (threadIdx.x == 0) s_ts[2] = __builtin_amdgcn_s_memrealtime();
        }
#pragma unroll
        for (int k = 0; k < kGB; ++k) {  // combine the participants' records per key in the LDS hash
          const uint32_t i = i0 + k * kRT + threadIdx.x;
          if (i >= n) continue;
          const uint32_t key = (uint32_t)r[k][0];
          uint32_t hs = (key * 2654435761u) >> (32 - __builtin_ctz(kResDeltaW));
          bool done = false;
          for (int probe = 0; probe < 16 && !done; ++probe) {
            const uint32_t prev = atomicCAS(&h.key[hs], kEmpty32, key);
            if (prev == kEmpty32 || prev == key) {
              atomicAdd(&h.sum[hs], r[k][1]);
              atomicMin(&h.ft[hs], r[k][2]);
              done = true;
            } else {
              hs = (hs + 1) & (kResDeltaW - 1);
            }
          }
          if (!done) sys_record(sl.out + atomicAdd(&s_nout, 1u), key, r[k][1], r[k][2]);  // the host combines these
        }
      }
      if (p.stamps && threadIdx.x == 0) s_ts[3] = __builtin_amdgcn_s_memrealtime();
      __syncthreads();
      for (int i = threadIdx.x; i < kResDeltaW; i += kRT) {
        const uint32_t key = h.key[i];
        if (key == kEmpty32) continue;
        sys_record(sl.out + atomicAdd(&s_nout, 1u), key, h.sum[i], h.ft[i]);
        h.key[i] = kEmpty32;
        h.sum[i] = 0;
        h.ft[i] = kEmpty64;
      }
      __syncthreads();
      n = s_nout;
      if (nm > p.mt_dense) nm = kAllTiles;  // X is in most tiles: the host marks it everywhere
      if (nm != kAllTiles) {
        // the matched tiles as a bitmap over every tile, built in this workgroup's LDS (the
        // gatherer owns no tiles: its dynamic area is free), so the host takes X's tile set as
        // is instead of sorting a list of up to ntiles / 2 entries
        uint32_t* s_bits = reinterpret_cast<uint32_t*>(s_dyn);
        for (uint32_t i = threadIdx.x; i < p.mt_words; i += kRT) s_bits[i] = 0;
        __syncthreads();
        constexpr int kMB = 8;  // tile ids in flight per thread
        for (uint32_t i0 = 0; i0 < nm; i0 += kRT * kMB) {
          uint32_t t[kMB];
#pragma unroll
          for (int k = 0; k < kMB; ++k) {
            const uint32_t i = i0 + k * kRT + threadIdx.x;
            t[k] = kAllTiles;
            if (i < nm) {
              const uint32_t o = owner(s_pmt, i);
              t[k] = __hip_atomic_load(sl.rtile + (size_t)o * kResMaxTiles + (i - s_pmt[o]), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
          }
#pragma unroll
          for (int k = 0; k < kMB; ++k)
            if (t[k] != kAllTiles) atomicOr(&s_bits[t[k] >> 5], 1u << (t[k] & 31));
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < p.mt_words; i += kRT) sys_store(sl.hmlist + i, s_bits[i]);
      }
      if (s_nrec) {  // spilled deltas in the global tables: all of them follow the records
        __syncthreads();
        if (threadIdx.x == 0) s_cmd[7] = atomicAdd(sl.dcount, 0u);
        __syncthreads();
        const uint32_t ngl = s_cmd[7];
        for (uint32_t i = threadIdx.x; i < ngl; i += kRT) {
          const uint32_t key = atomicOr(&sl.dlist[i], 0u);
          const u64 sum = atomicExch(&sl.dsum[key], 0ull);
          const u64 ft = atomicExch(&sl.dft[key], kEmpty64);
          sys_record(sl.out + n + i, key, sum, ft);
        }
        __syncthreads();
        if (threadIdx.x == 0) atomicExch(sl.dcount, 0u);
        n += ngl;
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      const u64 t_leader = s_tlead;
      sys_store(&sl.hstats[0], s_cnt[0]);
      sys_store(&sl.hstats[1], s_cnt[1]);
      sys_store(&sl.hstats[2], (u64)__builtin_amdgcn_s_memrealtime() - t_leader);
      if (p.stamps) {  // diagnostic: the gatherer's phases, relative to the leader's dispatch
        for (int k = 0; k < 4; ++k) sys_store(&sl.hstats[3 + k], s_ts[k] - t_leader);
        sys_store(&sl.hstats[7], (u64)s_pre[T]);  // records before the combine
        sys_store(&sl.hstats[8], t_leader);        // raw dispatch tick (the host's per-merge log)
      }
      sys_store(&sl.hcount[0], n);
      sys_store(&sl.hcount[2], nm);
      sys_flag(&sl.hcount[1], (uint32_t)X);  // the host clears the flag before posting to the slot
    }
  }
  // ---- STOP (or the leader's time-out): the tiles go back to HBM
  for (uint32_t i = wid; i < nt; i += kRW) {
    const uint32_t len = s_len[i];
    if constexpr (kLdsTok) {
      int32_t* dst = p.tok + s_toff[i];
      const int32_t* src = s_res + s_lofs[i];
      const uint32_t n4 = (len + 3u) >> 2;
      for (uint32_t q = (uint32_t)lane; q < n4; q += 64) {
        int4 x = *reinterpret_cast<const int4*>(src + 4 * q);
        if (4 * q + 1 >= len) x.y = kPad;
        if (4 * q + 2 >= len) x.z = kPad;
        if (4 * q + 3 >= len) x.w = kPad;
        *reinterpret_cast<int4*>(dst + 4 * q) = x;
      }
    }
    if (lane == 0) p.tile_len[t0 + i] = len;
  }
  if (threadIdx.x == 0 && exit_op != kOpStop) {
    __threadfence_system();
    __hip_atomic_store(&p.status[0], exit_op, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace

// ==========================================================================================
// k_resident host side: plan (which workgroup holds which tiles in LDS), launch, post, collect,
// roll back, stop.  See the kernel's comment for the protocol.
ResidentLoop::ResidentLoop(int ordinal, const MergeSlot* slots, uint32_t& seq, const uint32_t& keys_per_merge)
    : ordinal_(ordinal), slot_(slots), seq_(seq), keys_per_merge_(keys_per_merge) {
  if (const char* e = std::getenv("SHREDWORD_RESIDENT_ARRIVE_POLLS")) arrive_polls_ = (uint32_t)std::strtoul(e, nullptr, 10);
  if (const char* e = std::getenv("SHREDWORD_RESIDENT_REGION_KEYS")) region_keys_ = (uint32_t)std::strtoul(e, nullptr, 10);
}

ResidentLoop::~ResidentLoop() {
  free_plan();
  if (mbox_) (void)hipHostFree(mbox_);
  if (status_) (void)hipHostFree(status_);
  for (auto e : ev_)
    if (e) (void)hipEventDestroy((hipEvent_t)e);
}

void ResidentLoop::free_plan() {
  for (void* p : {(void*)wg_tiles_, (void*)wg_rank_, (void*)tile_lofs_, (void*)cmd_, (void*)q_, (void*)dbg_,
                  (void*)stamps_, (void*)arrive_})
    if (p) HIP_OK(hipFree(p));
  wg_tiles_ = wg_rank_ = tile_lofs_ = cmd_ = arrive_ = dbg_ = nullptr;
  q_ = stamps_ = nullptr;
  ok_ = false;
}

void ResidentLoop::plan(const TiledStream& ts, int32_t* tok, const uint64_t* tile_off, uint32_t* tile_len,
                        const uint64_t* weight, int cu_count, size_t* bytes) {
  free_plan();
  tok_ = tok, tile_off_ = tile_off, tile_len_ = tile_len, weight_ = weight;
  ntiles_ = ts.num_tiles();
  if (ntiles_ == 0) return;
  const uint32_t G = (uint32_t)std::min(cu_count, kMaxMergeGroups);
  if (G < kResFirstWorker + 1) return;
  const uint32_t W = G - kResFirstWorker;  // workers 2 .. G-1 (0 dispatches, 1 gathers)
  int max_lds = 0;
  HIP_OK(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ordinal_));
  hipFuncAttributes fa, fh;
  HIP_OK(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_resident<true, true>)));
  HIP_OK(hipFuncGetAttributes(&fh, reinterpret_cast<const void*>(&k_resident<true, false>)));
  // dynamic LDS per workgroup: tokens in LDS (256 threads) / tokens in HBM (kResThreadsHbm threads,
  // more staging); the dynamic region follows the statics unpadded: its 16-B accesses need a 16-B base
  const long budget = (long)max_lds - (long)fa.sharedSizeBytes - 64;
  const long budget_hbm = (long)max_lds - (long)fh.sharedSizeBytes - 64;
  if (budget <= 0 || fa.sharedSizeBytes % 16 != 0 || fh.sharedSizeBytes % 16 != 0) return;
  // per tile: first and last word rank (tiles hold whole words in rank order), LDS words
  const size_t T = ntiles_;
  std::vector<uint32_t> rfirst(T), rlast(T), words(T);
  for (size_t t = 0; t < T; ++t) {
    const uint32_t len = ts.len[t];
    if (len > (uint32_t)kWaveTok || len == 0) return;  // a long word: k_merge handles those
    const int32_t* tk = ts.tok.data() + ts.off[t];
    if (tk[0] >= kHeaderLimit) return;
    rfirst[t] = (uint32_t)(tk[0] - kHeaderBase);
    uint32_t last = rfirst[t];
    for (uint32_t i = 1; i < len; ++i)
      if (tk[i] < kHeaderLimit) last = (uint32_t)(tk[i] - kHeaderBase);
    rlast[t] = last;
    if (t && rfirst[t] != rlast[t - 1] + 1) return;
    words[t] = (len + 3u) & ~3u;
  }
  // The LDS plan, largest first: tokens + weights + 4096-bit signatures in LDS; tokens in HBM;
  // then (big tables: C5 at 100 GB has 68,905 tiles of 4.1 M words) the weights in HBM too, and
  // the signatures halved, then quartered (a looser filter: more tiles scanned per merge).
  // SHREDWORD_RESIDENT_SIG_WORDS / SHREDWORD_RESIDENT_W_GLOBAL force a smaller plan (tests).
  uint32_t sig_min = (uint32_t)kResSigWords / 4;
  uint32_t sig_cap = (uint32_t)kResSigWords;
  if (const char* e = std::getenv("SHREDWORD_RESIDENT_SIG_WORDS")) {
    const uint32_t v = (uint32_t)std::atoi(e);
    if (v == 32 || v == 64 || v == 128) sig_cap = sig_min = v;
  }
  const bool force_wg = std::getenv("SHREDWORD_RESIDENT_W_GLOBAL") != nullptr;
  const bool force_hbm = std::getenv("SHREDWORD_RESIDENT_HBM") != nullptr || force_wg || sig_cap < (uint32_t)kResSigWords;
  std::vector<uint32_t> wg_tiles, wg_rank, lofs;
  uint32_t tok_words = 0, nr_max = 0, sw = 0;
  size_t shm = 0;
  bool lds_tok = false, w_global = false, fit = false;
  for (int plan = 0; plan < 8 && !fit; ++plan) {
    // plan 0: tokens in LDS; 1: tokens in HBM; 2..: weights in HBM, signatures sig_cap >> (plan - 2)
    lds_tok = plan == 0;
    w_global = plan >= 2;
    sw = plan >= 2 ? sig_cap >> (plan - 2) : sig_cap;
    if (sw < sig_min) break;
    if ((lds_tok && force_hbm) || (!w_global && force_wg) || (!w_global && sw != sig_cap)) continue;
    const long bud = lds_tok ? budget : budget_hbm;
    // contiguous ranges balanced by LDS bytes: tile t goes to worker 2 + floor((prefix + cost/2) * W / total)
    auto cost = [&](size_t t) {  // tokens (LDS bytes, or the scan work when they stay in HBM) + weights + signature
      return 4.0 * words[t] + (w_global ? 0.0 : 8.0 * (rlast[t] - rfirst[t] + 1)) + 4.0 * sw;
    };
    double total = 0;
    for (size_t t = 0; t < T; ++t) total += cost(t);
    wg_tiles.assign(G + 1, 0);
    wg_rank.assign(G + 1, 0);
    lofs.assign(T, 0);
    double pre = 0;
    uint32_t w = kResFirstWorker;
    for (size_t t = 0; t < T; ++t) {
      const double c = cost(t);
      uint32_t want = kResFirstWorker + (uint32_t)std::min<double>(W - 1, std::floor((pre + c / 2) * W / total));
      if (want < w) want = w;
      while (w < want) wg_tiles[++w] = (uint32_t)t;
      pre += c;
    }
    while (w < G) wg_tiles[++w] = (uint32_t)T;
    tok_words = 0;
    nr_max = 0;
    uint32_t nt_max = 0;
    wg_ntiles_.assign(G, 0);
    for (uint32_t g = 0; g < G; ++g) {
      const uint32_t a = wg_tiles[g], b = wg_tiles[g + 1];
      wg_ntiles_[g] = b - a;
      nt_max = std::max(nt_max, b - a);
      uint32_t o = 0;
      for (uint32_t t = a; t < b; ++t) {
        lofs[t] = o;
        o += words[t];
      }
      tok_words = std::max(tok_words, o);
      wg_rank[g] = a < b ? rfirst[a] : (a < T ? rfirst[a] : rlast[T - 1] + 1);
      const uint32_t r_end = a < b ? rlast[b - 1] + 1 : wg_rank[g];
      nr_max = std::max(nr_max, r_end - wg_rank[g]);
    }
    wg_rank[G] = rlast[T - 1] + 1;
    if (nt_max > kResMaxTiles) continue;
    tok_words += (uint32_t)kWaveTok;  // every lane reads its 16 tokens of a full chunk from any tile start
    nr_max = w_global ? 0u : (nr_max + 1u) & ~1u;
    if (!lds_tok) tok_words = 0;
    shm = (size_t)tok_words * 4 + (size_t)nr_max * 8 + (size_t)nt_max * sw * 4;
    shm = std::max(shm, 4 * ((T + 31) / 32));  // the gatherer's matched-tile bitmap
    shm = (shm + 15) & ~(size_t)15;
    fit = (long)shm <= bud;
  }
  if (!fit) return;
  lds_tok_ = lds_tok;
  sig_words_ = sw;
  w_global_ = w_global;
  grid_ = G;
  tok_words_ = tok_words;
  w_words_ = nr_max;
  shm_ = shm;
  all_.clear();
  for (uint32_t g = kResFirstWorker; g < G; ++g) all_.push_back(g);
  wg_first_ = wg_tiles;
  wg_tiles_ = dalloc<uint32_t>(G + 1, bytes);
  wg_rank_ = dalloc<uint32_t>(G + 1, bytes);
  tile_lofs_ = dalloc<uint32_t>(T, bytes);
  cmd_ = dalloc<uint32_t>(kResRing * 8, bytes);
  q_ = dalloc<uint64_t>((size_t)G * kResRing * 2, bytes);
  arrive_ = dalloc<uint32_t>(16, bytes);
  HIP_OK(hipMemcpy(wg_tiles_, wg_tiles.data(), (G + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(wg_rank_, wg_rank.data(), (G + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(tile_lofs_, lofs.data(), T * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_OK(hipMemset(cmd_, 0, kResRing * 8 * sizeof(uint32_t)));
  if (std::getenv("SHREDWORD_RESIDENT_DEBUG")) {
    dbg_ = dalloc<uint32_t>((size_t)G * 4, bytes);
    HIP_OK(hipMemset(dbg_, 0, (size_t)G * 16));
  }
  if (std::getenv("SHREDWORD_RESIDENT_STAMPS")) {
    stamps_ = dalloc<uint64_t>((size_t)G * 8, bytes);
    HIP_OK(hipMemset(stamps_, 0, (size_t)G * 64));
  }
  if (!mbox_) {
    const unsigned pin = hipHostMallocMapped | hipHostMallocCoherent;
    HIP_OK(hipHostMalloc(&mbox_, sizeof(ResMbox), pin));
    std::memset(mbox_, 0, sizeof(ResMbox));
    HIP_OK(hipHostGetDevicePointer(&mbox_dev_, mbox_, 0));
    HIP_OK(hipHostMalloc((void**)&status_, 64, pin));
    std::memset(status_, 0, 64);
    HIP_OK(hipHostGetDevicePointer(&status_dev_, status_, 0));
    for (auto& e : ev_) {
      hipEvent_t ev;
      HIP_OK(hipEventCreate(&ev));
      e = ev;
    }
  }
  const void* kfn = lds_tok_ ? reinterpret_cast<const void*>(&k_resident<true, true>)
                             : reinterpret_cast<const void*>(&k_resident<true, false>);
  HIP_OK(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
  int per_cu = 0;  // the persistent grid must be co-resident: at least one workgroup per CU
  HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, lds_tok_ ? 256 : kResThreadsHbm, shm));
  if (per_cu < 1 || (long)per_cu * cu_count < (long)G) return;
  ok_ = true;
  if (std::getenv("SHREDWORD_RESIDENT_REPORT"))
    std::fprintf(stderr, "[RESIDENT] plan: grid %u, %zu B of LDS per workgroup, %d per CU; tokens in %s, weights in %s, "
                 "%u-bit tile signatures\n", G, (size_t)shm, per_cu, lds_tok_ ? "LDS" : "HBM",
                 w_global_ ? "HBM" : "LDS", 32u * sig_words_);
}

void ResidentLoop::start() {
  ResParams rp;
  rp.tok = tok_;
  rp.tile_off = tile_off_;
  rp.tile_len = tile_len_;
  rp.weight = weight_;
  rp.wg_tiles = wg_tiles_;
  rp.wg_rank = wg_rank_;
  rp.tile_lofs = tile_lofs_;
  rp.tok_words = tok_words_;
  rp.w_words = w_words_;
  rp.sig_words = sig_words_;
  rp.w_global = w_global_ ? 1u : 0u;
  rp.mbox = (const ResMbox*)mbox_dev_;
  rp.cmd = cmd_;
  rp.q = reinterpret_cast<u64*>(q_);
  rp.status = (uint32_t*)status_dev_;
  rp.arrive = arrive_;
  rp.arrive_polls = arrive_polls_;
  rp.seq0 = seq_ + 1;
  rp.leader_polls = 1u << 23;  // ~10 s without a command: the launch ends itself (the host relaunches)
  rp.keys_per_merge = keys_per_merge_;
  rp.slot_cap = UINT32_MAX;
  for (int k = 0; k < kSlots; ++k) rp.slot_cap = std::min(rp.slot_cap, slot_[k].cap);
  rp.region_keys = region_keys_;
  rp.mt_dense = (uint32_t)(ntiles_ / 2);
  rp.mt_words = (uint32_t)((ntiles_ + 31) / 32);
  for (int k = 0; k < kSlots; ++k) {
    const MergeSlot& sl = slot_[k];
    ResSlot& r = rp.sl[k];
    r.dsum = U(sl.dsum);
    r.dft = U(sl.dft);
    r.dlist = sl.dlist;
    r.dcount = sl.dcount;
    r.done = sl.dcount + 1;
    r.out = (DeltaRecord*)sl.dev_recs;
    r.hcount = (uint32_t*)sl.dev_count;
    r.hstats = (u64*)((char*)sl.dev_count + 16);
    r.hmlist = (uint32_t*)sl.dev_mlist;
    r.rhdr = sl.rhdr;
    r.rrec = U(sl.rrec);
    r.rtile = sl.rtile;
    // region headers carry the merge id k_resident polls for: none may hold a stale one
    if (sl.rhdr) HIP_OK(hipMemsetAsync(sl.rhdr, 0, (size_t)kMaxMergeGroups * kRegHdr * sizeof(uint32_t), S(stream_)));
  }
  for (int32_t& x : abandoned_) x = -1;
  rp.dbg = dbg_;
  rp.stamps = U(stamps_);
  status_[0] = 0;
  status_[2] = 0;
  HIP_OK(hipMemsetAsync(q_, 0, (size_t)grid_ * kResRing * 2 * sizeof(uint64_t), S(stream_)));
  HIP_OK(hipMemsetAsync(arrive_, 0, sizeof(uint32_t), S(stream_)));
  HIP_OK(hipEventRecord((hipEvent_t)ev_[0], S(stream_)));
  // a plain launch: one workgroup per CU by its LDS footprint, checked against the occupancy
  // query at plan time (plan), so every workgroup is resident together
  if (lds_tok_) k_resident<true, true><<<grid_, 256, shm_, S(stream_)>>>(rp);
  else k_resident<true, false><<<grid_, kResThreadsHbm, shm_, S(stream_)>>>(rp);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord((hipEvent_t)ev_[1], S(stream_)));
  running_ = true;
  merges_ = 0;
  ++launches_;
}

bool ResidentLoop::aborted() const { return __atomic_load_n(&status_[0], __ATOMIC_ACQUIRE) == kOpAbort; }

uint32_t ResidentLoop::post_merge(int slot, int32_t a, int32_t b, int32_t X, const TileIndex* index) {
  const uint32_t seq = post(kOpMerge, a, b, X, slot, index);
  posted_.push_back({X, a, b, seq, slot, (uint32_t)post_parts_[slot].size(), now_seconds()});
  uint32_t visited = 0;
  for (uint32_t o : post_parts_[slot]) visited += wg_ntiles_[o];
  return visited;
}

// Each wrong guess >= X is expanded back where it matched.
int ResidentLoop::rollback(int32_t X) {
  int n = 0;
  for (; !posted_.empty() && posted_.back().X >= X; ++n) {
    const Post rp = posted_.back();
    posted_.pop_back();
    // no wait: every workgroup takes its commands in order, so the undo follows the guess; the
    // slot stays out of use until the guess's completion is seen (pick_slot)
    post(kOpUnmerge, rp.a, rp.b, rp.X, rp.slot);
    abandoned_[rp.slot] = rp.X;
  }
  return n;
}

// Posts one command to the resident launch (relaunching it first if it ended on its time-out).
// Merge and unmerge commands name their participants; a merge's are kept by slot for its undo.
uint32_t ResidentLoop::post(uint32_t op, int32_t a, int32_t b, int32_t X, int slot, const TileIndex* index) {
  if (running_ && __atomic_load_n(&status_[0], __ATOMIC_ACQUIRE) == kOpTimeout) {
    if (!posted_.empty()) fatal("k_resident ended on its time-out with merges in flight");
    HIP_OK(hipStreamSynchronize(S(stream_)));
    running_ = false;
  }
  if (!running_ && op != kOpStop) start();
  uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t np = grid_;
  if (op == kOpMerge) {
    std::vector<uint32_t>& pp = post_parts_[slot];
    if (index) index->owners(a, b, wg_first_, &pp);
    if (!index || pp.empty()) pp = all_;
    slot_[slot].host_count[1] = 0xFFFFFFFFu;  // the merge raises X here
  }
  if (op == kOpMerge || op == kOpUnmerge) {
    const std::vector<uint32_t>& pp = post_parts_[slot];
    for (uint32_t o : pp) mask[o >> 5] |= 1u << (o & 31);
    np = (uint32_t)pp.size();
    if (op == kOpMerge) {  // the gatherer completes every merge
      mask[0] |= 1u << kResGatherWg;
      ++np;
    }
  }
  const uint32_t seq = ++seq_;
  uint64_t* g = static_cast<ResMbox*>(mbox_)->cmd[seq % kResRing].g;
  auto put = [&](int k, uint32_t v) { __atomic_store_n(&g[k], (uint64_t)seq | ((uint64_t)v << 32), __ATOMIC_RELAXED); };
  put(kCmdOp, op);
  put(kCmdA, (uint32_t)a);
  put(kCmdB, (uint32_t)b);
  put(kCmdX, (uint32_t)X);
  put(kCmdSlotN, (uint32_t)slot | (np << 8));
  for (int k = 0; k < 8; ++k) put(kCmdMask + k, mask[k]);
  std::atomic_thread_fence(std::memory_order_release);
  return seq;
}

// A slot for the next resident merge: none with a posted merge, and none whose undone guess has
// not completed yet (its completion still writes the slot and raises the slot's flag with the
// same merge id the next merge may carry).
int ResidentLoop::pick_slot() {
  for (;;) {
    int wait_slot = -1;
    for (int k = 0; k < kSlots; ++k) {
      const int s = (next_slot_ + k) % kSlots;
      bool used = false;
      for (const Post& rp : posted_) used |= rp.slot == s;
      if (used) continue;
      if (abandoned_[s] >= 0) {
        if (__atomic_load_n(slot_[s].host_count + 1, __ATOMIC_ACQUIRE) != (uint32_t)abandoned_[s]) {
          if (wait_slot < 0) wait_slot = s;
          continue;
        }
        abandoned_[s] = -1;
      }
      next_slot_ = (s + 1) % kSlots;
      return s;
    }
    if (wait_slot < 0) fatal("k_resident: no free merge slot");
    if (!wait(slot_[wait_slot], abandoned_[wait_slot])) return -1;  // the launch aborted
  }
}

bool ResidentLoop::wait(const MergeSlot& sl, int32_t X) {
  volatile uint32_t* flag = sl.host_count + 1;
  const double t0 = now_seconds();
  unsigned spins = 0;
  while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != (uint32_t)X) {
    __builtin_ia32_pause();
    if (++spins % 4096 != 0) continue;
    if (aborted()) return false;
    if (__atomic_load_n(&status_[0], __ATOMIC_ACQUIRE) == kOpTimeout)
      fatal("k_resident ended on its time-out before a posted merge completed");
    if (dbg_ && now_seconds() - t0 > 3.0) dump("no flag after 3 s");
    if (now_seconds() - t0 > 120.0) {
      const hipError_t e = hipStreamQuery(S(stream_));
      if (e != hipSuccess && e != hipErrorNotReady) HIP_OK(e);
      if (now_seconds() - t0 > 600.0) fatal("k_resident did not signal completion within 600 s");
    }
  }
  return true;
}

bool ResidentLoop::collect(int32_t X, Collected* c) {
  if (posted_.empty() || posted_.front().X != X) fatal("collect: merge X is not the oldest posted merge");
  const double tw = now_seconds();
  if (!wait(slot_[posted_.front().slot], X)) return false;  // not co-resident: nothing ran
  const Post rp = posted_.front();
  posted_.erase(posted_.begin());
  const MergeSlot& sl = slot_[rp.slot];
  const double t1 = now_seconds();  // host clock: post -> flag seen, and the part of it spent waiting here
  post_flag_us_ += 1e6 * (t1 - rp.t_post);
  host_wait_ += 1e6 * (t1 - tw);
  parts_sum_ += rp.nparts;
  const uint64_t* hs = (const uint64_t*)(sl.host_count + 4);
  lat_us_ += 1e-2 * (double)hs[2];  // s_memrealtime: 100 MHz
  lat_n_ += 1;
  if (stamps_) {
    for (int k = 0; k < 4; ++k) ph_[k] += 1e-2 * (double)hs[3 + k];
    ph_raw_ += (double)hs[7];
    ph_flag_ += 1e-2 * (double)hs[2];
    ph_n_ += 1;
  }
  ++merges_;
  // host_mlist: the gatherer's bitmap (k_resident)
  *c = {sl.host_recs, sl.host_count[0], sl.host_mlist, sl.host_count[2], hs, rp.nparts, rp.t_post, tw, t1};
  return true;
}

// Diagnostic (SHREDWORD_RESIDENT_DEBUG=1): the state of a stuck resident launch, then exit.
void ResidentLoop::dump(const char* why) {
  const uint32_t G = grid_;
  hipStream_t s;
  HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  std::vector<uint32_t> dbg(4 * G), cmd(kResRing * 8);
  std::vector<uint64_t> q((size_t)G * kResRing * 2);
  HIP_OK(hipMemcpyAsync(dbg.data(), dbg_, dbg.size() * 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(cmd.data(), cmd_, cmd.size() * 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(q.data(), q_, q.size() * 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  std::fprintf(stderr, "[RESIDENT] %s: seq_=%u status=%u posted=%zu flags=%u/%u\n", why, seq_, status_[0],
               posted_.size(), slot_[0].host_count[1], slot_[1].host_count[1]);
  for (int k = 2; k < kSlots; ++k) std::fprintf(stderr, "[RESIDENT] flag[%d]=%u\n", k, slot_[k].host_count[1]);
  for (const Post& rp : posted_)
    std::fprintf(stderr, "[RESIDENT]   posted X=%d seq=%u slot=%d np=%u\n", rp.X, rp.seq, rp.slot, rp.nparts);
  for (uint32_t g = 0; g < G; ++g) {
    std::fprintf(stderr, "[RESIDENT] wg %u: phase %u seq %u pi %u T %u | q", g, dbg[4 * g], dbg[4 * g + 1], dbg[4 * g + 2],
                 dbg[4 * g + 3]);
    for (uint32_t k = 0; k < kResRing; ++k) {
      const uint64_t v = q[((size_t)g * kResRing + k) * 2];
      std::fprintf(stderr, " %u:%u", (uint32_t)(v & 0xFFFF), (uint32_t)(v >> 24) & 7u);
    }
    std::fprintf(stderr, "\n");
  }
  std::fflush(stderr);
  std::_Exit(3);
}

uint64_t ResidentLoop::stop(double* ms_out) {
  if (!posted_.empty()) fatal("park: a resident merge was not collected");
  post(kOpStop, 0, 0, 0, 0);
  HIP_OK(hipStreamSynchronize(S(stream_)));
  running_ = false;
  for (int32_t& x : abandoned_) x = -1;  // every command ran
  for (int k = 0; k < kSlots; ++k)  // flags carried merge ids: the launch path compares launch numbers
    if (slot_[k].host_count) slot_[k].host_count[1] = 0xFFFFFFFFu;
  status_[0] = 0;
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, (hipEvent_t)ev_[0], (hipEvent_t)ev_[1]));
  ms_ += ms;
  *ms_out = ms;
  if (merges_ && std::getenv("SHREDWORD_RESIDENT_REPORT")) {
    const double n = (double)merges_;
    std::fprintf(stderr, "[RESIDENT] %llu merges in %.2f ms | host: post->flag %.2f us, waited %.2f us | participants %.1f",
                 (unsigned long long)merges_, ms, post_flag_us_ / n, host_wait_ / n, parts_sum_ / n);
    if (ph_n_)
      std::fprintf(stderr,
                   " | device after dispatch: all published %.2f prefix %.2f loaded %.2f combined %.2f flag %.2f",
                   ph_[0] / ph_n_, ph_[1] / ph_n_, ph_[2] / ph_n_, ph_[3] / ph_n_, ph_flag_ / ph_n_);
    if (ph_n_) std::fprintf(stderr, " | records before combine %.1f", ph_raw_ / ph_n_);
    std::fprintf(stderr, "\n");
  }
  post_flag_us_ = host_wait_ = parts_sum_ = ph_flag_ = ph_raw_ = 0;
  for (double& x : ph_) x = 0;
  ph_n_ = 0;
  return merges_;
}

std::vector<ResidentLoop::Post> ResidentLoop::abandon() {
  std::vector<Post> inflight;
  inflight.swap(posted_);
  running_ = false;
  for (int32_t& x : abandoned_) x = -1;
  return inflight;
}

}  // namespace shred
