// MI355X (gfx950) launch path of the BPE merge loop and the part of the Device class that owns
// the tables and chooses between the merge paths.
//
// Integer-only, HBM/LDS-bound work (no MFMA).  Every kernel walks the tiled token stream of
// device.h with 256-thread workgroups (4 wave64s), 16 consecutive tokens per lane, one 4096-token
// chunk per iteration; a tile longer than one chunk (a word of > 4095 tokens) is walked chunk by
// chunk with carries, so no word length is special.
//
//   k_merge        K2+K3 match (a,b), emit the 4 neighbour deltas per occurrence, rewrite the
//                  chunk compacted in place                      (reference bpe.cpp:259-296)
//   k_collect      K4  touched delta slots -> host records       (FreqChangeMap, bpe.cpp:9-50)
//   k_unmerge      rollback of a chain's unconfirmed merges
//
// Device's other methods: pair_count.hip (K1, K6, probes).  The resident loop (resident_loop.hip)
// and the indexed loop (word_loop.hip) are classes Device drives; hip_common.h holds what the units share.
//
// Deltas are staged in per-workgroup LDS hash tables and spilled to HBM tables
// with 64-bit atomics (sum) and atomicMin (first touch), so the reduction is order-free and the
// result bit-identical run to run.
#include <algorithm>
#include <cstring>
#include <iterator>

#include "../host/device.h"
#include "../host/dist.h"
#include "hip_common.h"

namespace shred {

namespace {

// ------------------------------------------------------------------------------------------
// K2+K3(+K4): merge scan.
//
// Filter: every tile carries a pair signature in HBM — an 8192-bit Bloom filter (two hashes) of
// the adjacent token pairs it holds, a superset of its current pairs.  A workgroup takes windows
// of kWin candidate tiles (the host's candidate list, or every tile); one wave tests their
// signatures with one load per lane and publishes the hit mask in LDS.
// Merge: the 4 waves split the window's hits and walk them kGroup at a time with all first-chunk
// loads in flight: each lane holds 16 consecutive tokens; occurrences, run parity,
// word headers and output offsets are wave-level scans; the 4 neighbour deltas of every
// occurrence go to a workgroup LDS hash; a changed chunk is compacted in LDS, written back in
// place, and (for single-chunk tiles) the tile's signature is rebuilt from the compacted chunk.
// Completion: the last workgroup (per-XCD sharded tickets) turns the touched delta slots into host
// records and raises a host-visible flag, so one launch + one flag wait is a merge's device side.
constexpr uint32_t kFusedCollectMax = 4096;  // beyond this the host launches k_collect
constexpr uint32_t kNeedCollect = 0x80000000u;
constexpr uint32_t kTimingStride = 8;
constexpr uint32_t kInlineTiles = 768;     // candidate tiles that fit the kernel arguments
constexpr int kGroup = 4;                  // tiles walked together per wave (loads in flight)
constexpr uint32_t kWin = 32;              // candidate tiles per workgroup window (filter pass)
constexpr int kMaxChain = 8;               // merges one k_merge launch applies in order
constexpr int kChainShift = Device::kChainShift;  // matched-tile entries: tile | (chain index << 27)
constexpr uint32_t kMtLds = 256;           // matched tiles a workgroup keeps in LDS (more: global list)
[[maybe_unused]] constexpr int kStamps = 18;               // SHRED_STAMPS: entry, init, windows, flush, ticket, collect, flag
#ifdef SHRED_STAMPS
#define STAMP(k) \
  if (threadIdx.x == 0) p.stamps[blockIdx.x * kStamps + (k)] = __builtin_amdgcn_s_memrealtime()
#define STAMP_ONCE(k) \
  if (threadIdx.x == 0 && p.stamps[blockIdx.x * kStamps + (k)] == 0) \
    p.stamps[blockIdx.x * kStamps + (k)] = __builtin_amdgcn_s_memrealtime()
#else
#define STAMP(k)
#define STAMP_ONCE(k)
#endif
static_assert(kMaxChain == Device::kChainMax, "chain length shared with the host");

struct MergeParams {
  int32_t* tok;
  const uint64_t* tile_off;
  uint32_t* tile_len;
  uint32_t ntiles;
  const uint64_t* weight;
  int32_t X0;               // merge i of the chain: (ca[i], cb[i]) -> X0 + i
  int32_t nchain;
  int32_t ca[kMaxChain], cb[kMaxChain];
  uint32_t keys_per_merge;  // delta key of merge i: i * keys_per_merge + (slot << 2 | category)
  uint32_t slot_cap;
  u64* dsum;
  u64* dft;
  uint32_t* dlist;
  uint32_t* dcount;   // [0] touched slots, [1..9] tickets, [10] matched tiles
  u64* stats;         // [0] occurrences merged, [1] tokens rewritten
  uint32_t* done;     // completion tickets: [0..7] per blockIdx % 8 group, [8] top
  DeltaRecord* out;   // records: host-visible, or (multi-GPU) this rank's device bucket
  uint32_t* xhdr;     // multi-GPU: the bucket header ([0] record count | kNeedCollect, [1] k_collect
                      // offset); the flag is then raised by k_xout after the exchange
  uint32_t* hcount;   // host-visible: [0] record count (| kNeedCollect), [1] flag = seq, [2] matched tiles,
                      // [3] first record k_collect writes (kNeedCollect)
  u64* hstats;        // host-visible: [0] occurrences, [1] tokens rewritten
  uint32_t* mlist;    // device: tiles where the merge matched (atomic writes, any XCD)
  uint32_t* mcount;   // device counter for mlist
  uint32_t* hmlist;   // host-visible copy of mlist (-> tiles(X) of the index), by the last workgroup
  uint32_t* sig;      // kSigWords per tile
  uint32_t* rhdr;     // fused: per-workgroup region headers (kRegHdr u32 each)
  u64* rrec;          // fused: per-workgroup records, kDeltaLdsW x 3 u64 each
  uint32_t* rtile;    // fused: per-workgroup matched tiles, kMtLds each
  int filter;         // 1: test tile signatures before loading tiles
  u64* stamps;        // SHRED_STAMPS diagnostic: kStamps s_memrealtime values per workgroup
  uint32_t seq;
  uint32_t nlist;     // 0: every tile is a candidate; else list[0 .. nlist)
  uint32_t list[kInlineTiles];  // candidate tiles (host tile index), passed in the kernel arguments
};

struct DeltaLds {
  uint32_t key[kDeltaLdsW];
  u64 sum[kDeltaLdsW];
  u64 ft[kDeltaLdsW];
  uint32_t spill;  // some delta went to the global tables
};

template <class P>
__device__ __forceinline__ void delta_emit(DeltaLds& h, const P& p, uint32_t key, u64 w, u64 ft) {
  uint32_t s = (key * 2654435761u) >> (32 - __builtin_ctz(kDeltaLdsW));
  for (int probe = 0; probe < 16; ++probe) {
    const uint32_t prev = atomicCAS(&h.key[s], kEmpty32, key);
    if (prev == kEmpty32 || prev == key) {
      atomicAdd(&h.sum[s], w);
      atomicMin(&h.ft[s], ft);
      return;
    }
    s = (s + 1) & (kDeltaLdsW - 1);
  }
  h.spill = 1;
  delta_global(p, key, w, ft);
}

template <bool kWeighted>
__global__ __launch_bounds__(kThreads) void k_merge(MergeParams p) {
  __shared__ int32_t s_tok[kWaves][kStPad];  // [SK(2 + j)] = chunk position j; [SK(0)],[SK(1)] = -2,-1
  __shared__ uint32_t s_sig[kWaves][kSigWords];
  __shared__ DeltaLds h;
  __shared__ uint32_t s_last;
  __shared__ u64 s_cnt[2];
  __shared__ u64 s_hits;
  __shared__ uint32_t s_wt[kWin];  // the window's candidate tiles
  __shared__ uint32_t s_mt[kMtLds];
  __shared__ uint32_t s_nmt, s_nrec;
  __shared__ uint32_t s_pre[kMaxMergeGroups + 1], s_pmt[kMaxMergeGroups + 1];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int32_t* st = s_tok[wid];
  STAMP(0);
#ifdef SHRED_STAMPS
  if (threadIdx.x == 0) p.stamps[blockIdx.x * kStamps + 16] = __builtin_amdgcn_s_memtime();
#endif
  for (int i = threadIdx.x; i < kDeltaLdsW; i += kThreads) {
    h.key[i] = kEmpty32;
    h.sum[i] = 0;
    h.ft[i] = kEmpty64;
  }
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    s_nmt = 0;
    s_nrec = 0;
    h.spill = 0;
  }
  __syncthreads();
  STAMP(1);
  const int p0 = lane * kPer;
  const int nchain = p.nchain;
  u64 n_merged = 0, n_written = 0;  // wave-uniform

  // ---- windows of kWin candidates: filter, then the waves split the hits
  const uint32_t n_cand = p.nlist ? p.nlist : p.ntiles;
  const uint32_t nwin = (n_cand + kWin - 1) / kWin;
  for (uint32_t win = blockIdx.x; win < nwin; win += gridDim.x) {
    if (wid == 0) {
      const uint32_t i = win * kWin + (uint32_t)lane;
      const bool in = (uint32_t)lane < kWin && i < n_cand;
      uint32_t t = in ? i : 0u;
      if (p.nlist) {  // uniform indices: scalar loads of the kernel-argument list
        t = 0;
#pragma unroll
        for (int k = 0; k < (int)kWin; ++k) {
          const uint32_t ik = win * kWin + (uint32_t)k;
          const uint32_t v = ik < n_cand ? p.list[ik] : 0u;
          if (lane == k) t = v;
        }
      }
      if ((uint32_t)lane < kWin) s_wt[lane] = t;
      bool hit = in;
      if (p.filter) {  // may the tile hold any pair of the chain?
        const uint32_t* sg = p.sig + (size_t)t * kSigWords;
        bool any = false;
        for (int cj = 0; cj < nchain; ++cj) {
          uint32_t h1, h2;
          sig_bits(p.ca[cj], p.cb[cj], &h1, &h2);
          const uint32_t w1 = sg[h1 >> 5], w2 = sg[h2 >> 5];
          any |= ((w1 >> (h1 & 31)) & 1u) && ((w2 >> (h2 & 31)) & 1u);
        }
        hit = in && any;
      }
      const u64 m = __ballot(hit);
      if (lane == 0) s_hits = m;
    }
    __syncthreads();
    STAMP_ONCE(8);
    const u64 hits = s_hits;
    // this wave's share: the hits whose rank among the window's hits is wid (mod kWaves)
    const bool mine_b = ((hits >> lane) & 1ull) &&
                        ((uint32_t)__popcll(hits & ((1ull << lane) - 1ull)) & (kWaves - 1)) == (uint32_t)wid;
    u64 mine = __ballot(mine_b);
    while (mine) {
    uint32_t gt[kGroup], gl[kGroup];
    uint64_t go[kGroup];
    int32_t gv[kGroup][kPer];
    int32_t gn[kGroup];
    uint32_t gmask = 0;
    {  // lane k < qn takes the wave's next hit k
      uint32_t qn = 0, pos = 0;
      for (int k = 0; k < kGroup && mine; ++k) {
        const uint32_t j = (uint32_t)__builtin_ctzll(mine);
        mine &= mine - 1;
        if ((uint32_t)lane == (uint32_t)k) pos = j;
        ++qn;
      }
      const uint32_t t = (uint32_t)lane < qn ? s_wt[pos] : 0u;
      const uint64_t o = p.tile_off[t];
      const uint32_t l0 = p.tile_len[t];
      const uint32_t l = (uint32_t)lane < qn ? l0 : 0u;
#pragma unroll
      for (int k = 0; k < kGroup; ++k) {
        gt[k] = (uint32_t)__builtin_amdgcn_readlane((int)t, k);
        gl[k] = (uint32_t)__builtin_amdgcn_readlane((int)l, k);
        go[k] = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(o >> 32), k) << 32) |
                (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)o, k);
      }
    }
    STAMP_ONCE(9);
    // all loads first (a cross-lane shuffle waits for every outstanding load)
    int32_t gm[kGroup];
#pragma unroll
    for (int k = 0; k < kGroup; ++k) {
      const int32_t* gb = p.tok + go[k];
      load_chunk(gb, 0, min((uint32_t)kWaveTok, gl[k]), p0, gv[k]);
      gm[k] = gb[p0 + kPer];  // inside the padded allocation; lane 63's lookahead
    }
#pragma unroll
    for (int k = 0; k < kGroup; ++k) {
      gn[k] = wave_next(gv[k][0]);
      if (lane == 63) gn[k] = (uint32_t)(p0 + kPer) < gl[k] ? gm[k] : kPad;
    }
    for (int cj = 0; cj < nchain; ++cj) {  // a chain merge's pair cannot appear through an earlier one
      const int32_t a = p.ca[cj], b = p.cb[cj];
#pragma unroll
      for (int k = 0; k < kGroup; ++k) {
        bool any = false;
#pragma unroll
        for (int j = 0; j < kPer; ++j) any |= (gv[k][j] == a) & ((j + 1 < kPer ? gv[k][j + 1] : gn[k]) == b);
        if (__any(any)) gmask |= 1u << k;
      }
    }
#pragma unroll
    for (int k = 0; k < kGroup; ++k)
      if (gl[k] > (uint32_t)kWaveTok) gmask |= 1u << k;
    STAMP_ONCE(10);
#pragma unroll 1
    for (int k = 0; k < kGroup; ++k) {
    if (!((gmask >> k) & 1u)) continue;
#define SHRED_SEL(arr) (k == 0 ? arr[0] : k == 1 ? arr[1] : k == 2 ? arr[2] : arr[3])
    const uint32_t tile = SHRED_SEL(gt), len = SHRED_SEL(gl);
    int32_t* base = p.tok + SHRED_SEL(go);
    int32_t v0[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) v0[j] = k == 0 ? gv[0][j] : k == 1 ? gv[1][j] : k == 2 ? gv[2][j] : gv[3][j];
    int32_t nx0 = SHRED_SEL(gn);
#undef SHRED_SEL
    // The chain's merges in order.  A single-chunk tile stays in registers (cur) between merges
    // and is written back once; a longer tile is rewritten in HBM chunk by chunk per merge.
    const bool single = len <= (uint32_t)kWaveTok;
    int32_t cur[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) cur[j] = v0[j];
    int32_t cur_nx = nx0;
    uint32_t cur_len = len;
    bool tdirty = false;
#pragma unroll 1
    for (int cj = 0; cj < nchain; ++cj) {
    const int32_t a = p.ca[cj], b = p.cb[cj], X = p.X0 + cj;
    const bool same = (a == b);
    const uint32_t kofs = (uint32_t)cj * p.keys_per_merge;
    if (!single && tdirty) {  // re-read a long tile rewritten by an earlier merge of the chain
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      load_chunk(base, 0, min((uint32_t)kWaveTok, cur_len), p0, v0);
      nx0 = next_token(base, 0, cur_len, p0, v0[0]);
    }
    const uint32_t tlen = cur_len;
    uint64_t tile_hits = 0;
    long long c_nona = -1;  // last tile index whose token != a (a == b only)
    u64 c_hdr = 0;          // ((index + 1) << 32) | rank of the last header, 0 = none
    bool c_m1 = false, c_m2 = false;
    int32_t c_t1 = kPad, c_t2 = kPad;
    uint32_t c_out = 0;
    bool dirty = false;
    for (uint32_t cs = 0; cs < tlen; cs += kWaveTok) {
      const uint32_t cl = min((uint32_t)kWaveTok, tlen - cs);
      const bool more = cs + cl < tlen;
      int32_t v[kPer];
      int32_t nx;
      if (cs == 0) {
#pragma unroll
        for (int j = 0; j < kPer; ++j) v[j] = single ? cur[j] : v0[j];
        nx = single ? cur_nx : nx0;
      } else {
        load_chunk(base, cs, cl, p0, v);
        nx = next_token(base, cs, tlen, p0, v[0]);
      }
      bool any = false;
#pragma unroll
      for (int j = 0; j < kPer; ++j) any |= (v[j] == a) & ((j + 1 < kPer ? v[j + 1] : nx) == b);
      if (!__any(any) && !dirty && !more) break;  // rest of the tile is unchanged

      // ---- stage the chunk with 2 tokens of left context and 2 of lookahead
#pragma unroll
      for (int j = 0; j < kPer; ++j) st[SK(2 + p0 + j)] = v[j];
      if (lane == 0) {
        st[SK(0)] = c_t2;
        st[SK(1)] = c_t1;
      }
      if (lane == 63) {
        st[SK(2 + kWaveTok)] = (cs + kWaveTok < tlen) ? base[cs + kWaveTok] : kPad;
        st[SK(3 + kWaveTok)] = (cs + kWaveTok + 1 < tlen) ? base[cs + kWaveTok + 1] : kPad;
      }
      wave_lds_sync();
      STAMP_ONCE(12);
      const int32_t last1 = st[SK(2 + cl - 1)];
      const int32_t last2 = st[SK(2 + cl - 2)];  // st[SK(1)] when cl == 1

      // ---- occurrences, greedy left to right (runs of a == b pair up from the run start)
      uint32_t mask = 0;
      long long nona_tot = -1;
      if (same) {
        u64 nl = 0;  // last index whose token != a, + 1 (0 = none)
#pragma unroll
        for (int j = 0; j < kPer; ++j)
          if (v[j] != a) nl = (u64)(cs + p0 + j) + 1;
        const u64 inc = wave_scan_max64(nl);
        nona_tot = (long long)lane_read64(inc, 63) - 1;
        long long last = (long long)wave_prev64(inc) - 1;
        last = last > c_nona ? last : c_nona;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
          const long long gi = (long long)(cs + p0 + j);
          if (v[j] != a) last = gi;
          else if ((j + 1 < kPer ? v[j + 1] : nx) == a && ((gi - last - 1) & 1) == 0) mask |= 1u << j;
        }
      } else {
#pragma unroll
        for (int j = 0; j < kPer; ++j)
          if (v[j] == a && (j + 1 < kPer ? v[j + 1] : nx) == b) mask |= 1u << j;
      }
      uint32_t prevm = wave_prev(mask);
      if (lane == 0) prevm = (c_m1 ? 1u << 15 : 0u) | (c_m2 ? 1u << 14 : 0u);
      const uint32_t m_ext = (mask << 2) | ((prevm >> 14) & 3u);  // bit k <-> position p0 - 2 + k
      const uint32_t removed = (m_ext >> 1) & 0xFFFFu;           // bit j <-> match at p0 + j - 1
      const int valid = max(0, min(kPer, (int)cl - p0));
      const uint32_t vmask = valid >= kPer ? 0xFFFFu : ((1u << valid) - 1u);
      const int kc = __popc(~removed & vmask);
      const int nm = __popc(mask);
      uint32_t hmask = 0;  // word headers among this lane's valid positions
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        if (is_hdr(v[j])) hmask |= 1u << j;
      hmask &= vmask;
      u64 hl = 0;
      if (hmask) {
        const int j = 31 - __clz(hmask);
        hl = ((u64)(cs + p0 + j + 1) << 32) | hdr_rank(st[SK(2 + p0 + j)]);
      }
      const u64 hinc = wave_scan_max64(hl);
      const u64 hdr_ex = wave_prev64(hinc);
      const u64 hdr_tot = lane_read64(hinc, 63);
      const int cinc = wave_incl_sum(kc | (nm << 16));
      const int ctot = (int)lane_read((uint32_t)cinc, 63);
      const int kc_ex = (cinc - (kc | (nm << 16))) & 0xFFFF;
      const int kept = ctot & 0xFFFF;
      const int matches = ctot >> 16;

      // ---- neighbour deltas, 4 per occurrence (bpe.cpp:274-290)
      if (mask) {
        const u64 hdr_in = hdr_ex > c_hdr ? hdr_ex : c_hdr;
        for (uint32_t mrem = mask; mrem; mrem &= mrem - 1) {
          const int j = __ffs(mrem) - 1;
          const uint32_t hb = hmask & ((2u << j) - 1u);  // headers at or before j in this lane
          u64 hdr = hdr_in;
          if (hb) {
            const int jh = 31 - __clz(hb);
            hdr = ((u64)(cs + p0 + jh + 1) << 32) | hdr_rank(st[SK(2 + p0 + jh)]);
          }
          const uint32_t hidx = (uint32_t)(hdr >> 32) - 1u;
          const uint32_t rank = (uint32_t)hdr;
          const uint32_t gi = cs + p0 + j;
          const u64 w = kWeighted ? p.weight[rank] : 1ull;
          const u64 ftb = ((u64)rank << 32) | ((u64)(gi - hidx - 1u) << 2);
          if (gi - 1u > hidx) {  // left neighbour inside the word; X if it was just merged
            const int32_t left = ((m_ext >> j) & 1u) ? X : st[SK(1 + p0 + j)];
            const uint32_t sl = slot_of(left, p.slot_cap) << 2;
            delta_emit(h, p, kofs + (sl | kOldLeft), w, ftb | kOldLeft);
            delta_emit(h, p, kofs + (sl | kNewLeft), w, ftb | kNewLeft);
          }
          const int32_t right = st[SK(4 + p0 + j)];  // original token after b
          if (!is_hdr(right)) {
            const uint32_t sr = slot_of(right, p.slot_cap) << 2;
            delta_emit(h, p, kofs + (sr | kOldRight), w, ftb | kOldRight);
            delta_emit(h, p, kofs + (sr | kNewRight), w, ftb | kNewRight);
          }
        }
      }
      STAMP_ONCE(13);
      const bool write = dirty || matches > 0 || kept != (int)cl;
      if (write) {
        wave_lds_sync();  // every neighbour read is done: compact in place
        int o = kc_ex;
#pragma unroll
        for (int j = 0; j < kPer; ++j)
          if (j < valid && !((removed >> j) & 1u)) st[SK(2 + o++)] = ((mask >> j) & 1u) ? X : v[j];
        wave_lds_sync();
        if (single) {  // the tile lives on in registers: cur <- compacted chunk
#pragma unroll
          for (int j = 0; j < kPer; ++j) cur[j] = p0 + j < kept ? st[SK(2 + p0 + j)] : kPad;
          cur_nx = p0 + kPer < kept ? st[SK(2 + p0 + kPer)] : kPad;
          cur_len = (uint32_t)kept;
          tdirty = true;
        } else {
          for (int j = lane; j < kept; j += 64) base[c_out + j] = st[SK(2 + j)];
        }
        dirty = true;
        n_written += (u64)kept;
        STAMP_ONCE(14);

      }
      n_merged += (u64)matches;
      tile_hits += (u64)matches;
      // ---- carries to the next chunk of this tile
      c_out += (uint32_t)kept;
      c_m1 = (lane_read(mask, (int)((cl - 1) / kPer)) >> ((cl - 1) % kPer)) & 1u;
      c_m2 = cl >= 2 ? ((lane_read(mask, (int)((cl - 2) / kPer)) >> ((cl - 2) % kPer)) & 1u) : c_m1;
      c_t1 = last1;
      c_t2 = last2;
      c_hdr = hdr_tot > c_hdr ? hdr_tot : c_hdr;
      if (same) c_nona = nona_tot > c_nona ? nona_tot : c_nona;
      wave_lds_sync();  // the copy-out reads st before the next chunk overwrites it
    }
    if (!single && dirty) {
      if (lane == 0) p.tile_len[tile] = c_out;
      cur_len = c_out;
      tdirty = true;
    }
    if (tile_hits && lane == 0) {
      const uint32_t ent = tile | ((uint32_t)cj << kChainShift);
      const uint32_t k = atomicAdd(&s_nmt, 1u);
      if (k < kMtLds) s_mt[k] = ent;
      else atomicExch(&p.mlist[atomicAdd(p.mcount, 1u)], ent);
    }
    }  // merges of the chain
    if (single && tdirty) {  // write the tile back once, within its allocation, and re-sign it
      const uint32_t cap = (len + 3u) & ~3u;
#pragma unroll
      for (int q = 0; q < kPer / 4; ++q) {
        if ((uint32_t)(p0 + 4 * q) < cap) {
          int4 o;
          o.x = cur[4 * q];
          o.y = cur[4 * q + 1];
          o.z = cur[4 * q + 2];
          o.w = cur[4 * q + 3];
          *reinterpret_cast<int4*>(base + p0 + 4 * q) = o;
        }
      }
      if (lane == 0) p.tile_len[tile] = cur_len;
      sig_rebuild(s_sig[wid], p.sig + (size_t)tile * kSigWords, cur, cur_nx, lane);
      STAMP_ONCE(15);
    }
    }  // tiles of the group
    STAMP_ONCE(11);
    }  // this wave's hits
    __syncthreads();  // s_hits is rewritten by the next window
  }
  STAMP(2);
  if (lane == 0) {
    if (n_merged) atomicAdd(&s_cnt[0], n_merged);
    if (n_written) atomicAdd(&s_cnt[1], n_written);
  }
  __syncthreads();
  {
    // ---- this workgroup's region: LDS-reduced records, matched tiles and counts, written
    // through (sc1) so the collecting workgroup on any XCD reads them with sc1 loads after the
    // ticket (MI355X_MICROARCH.md, valid forms: sc1 stores, vmcnt drain, atomic ticket)
    u64* rr = p.rrec + (size_t)blockIdx.x * kDeltaLdsW * 3;
    for (int i = threadIdx.x; i < kDeltaLdsW; i += kThreads) {
      if (h.key[i] == kEmpty32) continue;
      const uint32_t k = atomicAdd(&s_nrec, 1u);
      __hip_atomic_store(rr + 3 * k, (u64)h.key[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(rr + 3 * k + 1, h.sum[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(rr + 3 * k + 2, h.ft[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint32_t nmt = min(s_nmt, kMtLds);
    for (uint32_t i = threadIdx.x; i < nmt; i += kThreads)
      __hip_atomic_store(p.rtile + (size_t)blockIdx.x * kMtLds + i, s_mt[i], __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t* hd = p.rhdr + (size_t)blockIdx.x * kRegHdr;
      __hip_atomic_store(hd, s_nrec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(hd + 1, nmt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(hd + 2, h.spill, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(reinterpret_cast<u64*>(hd + 4), s_cnt[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(reinterpret_cast<u64*>(hd + 6), s_cnt[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // ---- completion ticket: every wave drains its stores/atomics first.  One counter for small
  // grids; sharded by blockIdx % 8 above that, so no counter sees more than gridDim/8 arrivals.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  STAMP(3);
  if (threadIdx.x == 0) {
    bool last = false;
    if (gridDim.x <= 32u) {
      last = atomicAdd(&p.done[8], 1u) == gridDim.x - 1u;
    } else {
      const uint32_t g = blockIdx.x & 7u;
      const uint32_t in_group = (gridDim.x - g + 7u) >> 3;
      if (atomicAdd(&p.done[g], 1u) == in_group - 1u) {
        atomicExch(&p.done[g], 0u);
        last = atomicAdd(&p.done[8], 1u) == 7u;
      }
    }
    s_last = last;
  }
  __syncthreads();
  STAMP(4);
#ifdef SHRED_STAMPS
  if (threadIdx.x == 0) p.stamps[blockIdx.x * kStamps + 17] = __builtin_amdgcn_s_memtime();
#endif
  if (!s_last) return;
  const uint32_t G = gridDim.x;
  uint32_t n = 0, nm = 0, base = 0;
  bool need_collect = false;
  {
    // ---- gather the regions: headers, prefix offsets, then records and tiles to the host
    u64 merged = 0, written = 0;
    uint32_t spill = 0;
    if (threadIdx.x == 0) {
      s_cnt[0] = 0;
      s_cnt[1] = 0;
      s_nrec = 0;
    }
    __syncthreads();
    // one header per thread (G <= kThreads), then exclusive prefix sums by wave scans
    uint32_t my_nrec = 0, my_nmt = 0;
    const uint32_t g = threadIdx.x;
    if (g < G) {
      const uint32_t* hd = p.rhdr + (size_t)g * kRegHdr;
      my_nrec = __hip_atomic_load(hd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      my_nmt = __hip_atomic_load(hd + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      spill = __hip_atomic_load(hd + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      merged = __hip_atomic_load(reinterpret_cast<const u64*>(hd + 4), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      written = __hip_atomic_load(reinterpret_cast<const u64*>(hd + 6), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (merged) atomicAdd(&s_cnt[0], merged);
    if (written) atomicAdd(&s_cnt[1], written);
    if (spill) atomicOr(&s_nrec, 1u);
    const uint32_t ir = wave_scan_add(my_nrec), im = wave_scan_add(my_nmt);
    __shared__ uint32_t s_wtot[2][kWaves];
    if (lane == 63) {
      s_wtot[0][wid] = ir;
      s_wtot[1][wid] = im;
    }
    __syncthreads();
    uint32_t br = 0, bm = 0;
    for (int w = 0; w < wid; ++w) {
      br += s_wtot[0][w];
      bm += s_wtot[1][w];
    }
    if (g < G) {
      s_pre[g] = br + ir - my_nrec;
      s_pmt[g] = bm + im - my_nmt;
    }
    if (g == G - 1) {
      s_pre[G] = br + ir;
      s_pmt[G] = bm + im;
    }
    __syncthreads();
    n = s_pre[G];
    nm = s_pmt[G];
    auto owner = [&](const uint32_t* pre, uint32_t i) {  // the workgroup whose range holds i
      uint32_t lo = 0, hi = G;                            // pre[lo] <= i < pre[hi]
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pre[mid] <= i) lo = mid;
        else hi = mid;
      }
      return lo;
    };
    for (uint32_t i0 = 0; i0 < n; i0 += kThreads * 4) {
      u64 r[4][3];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t i = i0 + k * kThreads + threadIdx.x;
        if (i < n) {
          const uint32_t g = owner(s_pre, i);
          const u64* src = p.rrec + ((size_t)g * kDeltaLdsW + (i - s_pre[g])) * 3;
#pragma unroll
          for (int c = 0; c < 3; ++c) r[k][c] = __hip_atomic_load(src + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t i = i0 + k * kThreads + threadIdx.x;
        if (i < n) sys_record(p.out + i, (uint32_t)r[k][0], r[k][1], r[k][2]);
      }
    }
    for (uint32_t i = threadIdx.x; i < nm; i += kThreads) {
      const uint32_t g = owner(s_pmt, i);
      sys_store(p.hmlist + i,
                __hip_atomic_load(p.rtile + (size_t)g * kMtLds + (i - s_pmt[g]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    // workgroups with more matched tiles than their LDS list: the rest is in the global list
    if (threadIdx.x == 0) s_hits = atomicExch(p.mcount, 0u);
    __syncthreads();
    const uint32_t ng = (uint32_t)s_hits;
    for (uint32_t i = threadIdx.x; i < ng; i += kThreads) sys_store(p.hmlist + nm + i, atomicOr(&p.mlist[i], 0u));
    nm += ng;
    if (s_nrec) {  // spilled deltas in the global tables: append them (or leave them to k_collect)
      __syncthreads();
      if (threadIdx.x == 0) s_hits = atomicAdd(p.dcount, 0u);
      __syncthreads();
      const uint32_t ngl = (uint32_t)s_hits;
      base = n;
      if (ngl <= kFusedCollectMax) {
        for (uint32_t i = threadIdx.x; i < ngl; i += kThreads) {
          const uint32_t key = atomicOr(&p.dlist[i], 0u);
          const u64 sum = atomicExch(&p.dsum[key], 0ull);
          const u64 ft = atomicExch(&p.dft[key], kEmpty64);
          sys_record(p.out + n + i, key, sum, ft);
        }
        __syncthreads();
        if (threadIdx.x == 0) atomicExch(p.dcount, 0u);
      } else {
        need_collect = true;
      }
      n += ngl;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  STAMP(5);
  if (threadIdx.x == 0) {
    sys_store(&p.hstats[0], s_cnt[0]);
    sys_store(&p.hstats[1], s_cnt[1]);
    sys_store(&p.hcount[0], need_collect ? (n | kNeedCollect) : n);
    sys_store(&p.hcount[3], base);
    sys_store(&p.hcount[2], nm);
    atomicExch(&p.done[8], 0u);
    STAMP(6);
    if (p.xhdr) {  // multi-GPU: the bucket header; k_xout raises the flag after the exchange
      p.xhdr[0] = need_collect ? (n | kNeedCollect) : n;
      p.xhdr[1] = base;
      __threadfence_system();
    } else {
      sys_flag(&p.hcount[1], p.seq);
    }
    STAMP(7);
  }
}

// Multi-GPU (K4 after the all-gather): the gathered buckets -> one host-visible record list.
// Rank r contributes the records that are valid in its bucket: min(count, bucket) — or, when
// its spilled deltas still wait for k_collect, min(k_collect offset, bucket); the rest goes
// through the host's overflow round.  One workgroup, so the flag follows every host store.
struct XoutParams {
  const uint8_t* recv;  // world buckets of `bucket` bytes: u32 header[8], then records
  uint32_t bucket;
  uint32_t cap;         // records per bucket
  uint32_t world;
  DeltaRecord* out;     // host-visible, world x cap records
  uint32_t* hx;         // host-visible: per rank [count | kNeedCollect, k_collect offset]
  uint32_t* flag;       // host-visible completion flag
  uint32_t seq;
};

__device__ __forceinline__ uint32_t bucket_valid(uint32_t h0, uint32_t h1, uint32_t cap) {
  const uint32_t n = (h0 & kNeedCollect) ? h1 : h0;
  return min(n, cap);
}

__global__ __launch_bounds__(1024) void k_xout(XoutParams p) {
  __shared__ uint32_t s_pre[65];
  if (threadIdx.x == 0) {
    uint32_t acc = 0;
    for (uint32_t r = 0; r < p.world; ++r) {
      const uint32_t* h = reinterpret_cast<const uint32_t*>(p.recv + (size_t)r * p.bucket);
      s_pre[r] = acc;
      acc += bucket_valid(h[0], h[1], p.cap);
    }
    s_pre[p.world] = acc;
  }
  __syncthreads();
  if (threadIdx.x < p.world) {
    const uint32_t* h = reinterpret_cast<const uint32_t*>(p.recv + (size_t)threadIdx.x * p.bucket);
    sys_store(p.hx + 2 * threadIdx.x, h[0]);
    sys_store(p.hx + 2 * threadIdx.x + 1, h[1]);
  }
  for (uint32_t r = 0; r < p.world; ++r) {
    const u64* src = reinterpret_cast<const u64*>(p.recv + (size_t)r * p.bucket + 32);
    const uint32_t nv = s_pre[r + 1] - s_pre[r];
    for (uint32_t i = threadIdx.x; i < nv; i += blockDim.x)
      sys_record(p.out + s_pre[r] + i, (uint32_t)src[3 * i], src[3 * i + 1], src[3 * i + 2]);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) sys_flag(p.flag, p.seq);
}


// K4: touched slots -> records in host-visible memory; clears the slots for the next merge.
__global__ __launch_bounds__(kThreads) void k_collect(uint32_t* dcount, const uint32_t* dlist, u64* dsum, u64* dft,
                                                       DeltaRecord* out) {
  const uint32_t n = *dcount;
  for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
    const uint32_t key = dlist[i];
    DeltaRecord r;
    r.key = key;
    r.pad = 0;
    r.sum = dsum[key];
    r.ft = dft[key];
    out[i] = r;
    dsum[key] = 0;
    dft[key] = kEmpty64;
  }
}

__global__ void k_zero_u32(uint32_t* p) { *p = 0; }

// ------------------------------------------------------------------------------------------
// Rollback of the unconfirmed tail of a merge chain: in every listed tile, each undone merge
// (a,b)->X is expanded back into "a b", newest first, so the tile is exactly as before those
// merges (their X are fresh ids, and their pairs never involve another chain id).  A tile whose
// restored length fits one wave chunk is expanded in registers through LDS, written back once and
// re-signed; a longer one is expanded in place in HBM, chunks walked from the end so a chunk's
// right-shifted output only lands on input already read.  Workgroup 0 also clears the slot
// tables when the chain spilled into them.
struct UnmergeParams {
  int32_t* tok;
  const uint64_t* tile_off;
  uint32_t* tile_len;
  const uint32_t* tiles;  // host-mapped list of the tiles to restore
  uint32_t ntl;
  const uint32_t* ntl_dev;  // if set: the count, written to host memory by the merge itself
  int32_t nundo;          // undo merges ux0 + u, u < nundo
  int32_t ux0;
  int32_t ua[kMaxChain], ub[kMaxChain];
  uint32_t* dcount;
  const uint32_t* dlist;
  u64* dsum;
  u64* dft;
  uint32_t* sig;
};

__global__ __launch_bounds__(kThreads) void k_unmerge(UnmergeParams p) {
  __shared__ uint32_t s_sig[kWaves][kSigWords];
  __shared__ int32_t s_buf[kWaves][kStPad];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int p0 = lane * kPer;
  int32_t* buf = s_buf[wid];
  const uint32_t xlo = (uint32_t)p.ux0, nun = (uint32_t)p.nundo;
  const uint32_t ntl = p.ntl_dev ? *p.ntl_dev : p.ntl;
  for (uint32_t i = blockIdx.x * kWaves + wid; i < ntl; i += gridDim.x * kWaves) {
    const uint32_t tile = p.tiles[i];
    const uint32_t len = p.tile_len[tile];
    int32_t* base = p.tok + p.tile_off[tile];
    int cnt = 0;  // every undone X in the tile: the restored length
    for (uint32_t cs = 0; cs < len; cs += kWaveTok) {
      int32_t v[kPer];
      load_chunk(base, cs, min((uint32_t)kWaveTok, len - cs), p0, v);
#pragma unroll
      for (int j = 0; j < kPer; ++j) cnt += (uint32_t)v[j] - xlo < nun;
    }
    cnt = (int)lane_read((uint32_t)wave_incl_sum(cnt), 63);
    if (cnt == 0) continue;
    const uint32_t final_len = len + (uint32_t)cnt;
    if (final_len <= (uint32_t)kWaveTok) {
      int32_t v[kPer];
      load_chunk(base, 0, len, p0, v);
      uint32_t cl = len;
      for (int u = p.nundo - 1; u >= 0; --u) {
        const int32_t X = p.ux0 + u, a = p.ua[u], b = p.ub[u];
        int c = 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) c += v[j] == X;
        const int inc = wave_incl_sum(c);
        const int ctot = (int)lane_read((uint32_t)inc, 63);
        if (ctot == 0) continue;
        uint32_t o = (uint32_t)p0 + (uint32_t)(inc - c);
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
          if ((uint32_t)(p0 + j) >= cl) continue;
          if (v[j] == X) {
            buf[SK(o)] = a;
            buf[SK(o + 1)] = b;
            o += 2;
          } else {
            buf[SK(o)] = v[j];
            o += 1;
          }
        }
        wave_lds_sync();
        cl += (uint32_t)ctot;
#pragma unroll
        for (int j = 0; j < kPer; ++j) v[j] = (uint32_t)(p0 + j) < cl ? buf[SK(p0 + j)] : kPad;
        wave_lds_sync();
      }
      const uint32_t cap = (cl + 3u) & ~3u;  // within the tile's allocation (>= its original length)
#pragma unroll
      for (int q = 0; q < kPer / 4; ++q) {
        if ((uint32_t)(p0 + 4 * q) < cap) {
          int4 w;
          w.x = v[4 * q];
          w.y = v[4 * q + 1];
          w.z = v[4 * q + 2];
          w.w = v[4 * q + 3];
          *reinterpret_cast<int4*>(base + p0 + 4 * q) = w;
        }
      }
      if (lane == 0) p.tile_len[tile] = cl;
      int32_t nx = wave_next(v[0]);
      if (lane == 63) nx = kPad;
      sig_rebuild(s_sig[wid], p.sig + (size_t)tile * kSigWords, v, nx, lane);
      continue;
    }
    // a tile longer than one chunk (its signature stays all-ones)
    uint32_t tl = len;
    for (int u = p.nundo - 1; u >= 0; --u) {
      const int32_t X = p.ux0 + u, a = p.ua[u], b = p.ub[u];
      if (u != p.nundo - 1) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // our own rewrite
      int total = 0;
      for (uint32_t cs = 0; cs < tl; cs += kWaveTok) {
        int32_t v[kPer];
        load_chunk(base, cs, min((uint32_t)kWaveTok, tl - cs), p0, v);
        int c = 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) c += v[j] == X;
        total += c;
      }
      total = (int)lane_read((uint32_t)wave_incl_sum(total), 63);
      if (total == 0) continue;
      int after = 0;  // X count in the chunks right of the current one
      const uint32_t last_cs = ((tl - 1) / kWaveTok) * kWaveTok;
      for (long long cs = last_cs; cs >= 0; cs -= kWaveTok) {
        const uint32_t cl = min((uint32_t)kWaveTok, tl - (uint32_t)cs);
        int32_t v[kPer];
        load_chunk(base, (uint32_t)cs, cl, p0, v);
        int c = 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) c += v[j] == X;
        const int inc = wave_incl_sum(c);
        const int ctot = (int)lane_read((uint32_t)inc, 63);
        uint32_t o = (uint32_t)cs + (uint32_t)p0 + (uint32_t)(total - after - ctot) + (uint32_t)(inc - c);
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
          if (p0 + j >= (int)cl) continue;
          if (v[j] == X) {
            base[o] = a;
            base[o + 1] = b;
            o += 2;
          } else {
            base[o] = v[j];
            o += 1;
          }
        }
        after += ctot;
      }
      tl += (uint32_t)total;
      if (lane == 0) p.tile_len[tile] = tl;
    }
  }
  if (blockIdx.x == 0) {  // tables left by a spilled chain
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = *p.dcount;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < s_n; i += kThreads) {
      const uint32_t key = p.dlist[i];
      p.dsum[key] = 0;
      p.dft[key] = kEmpty64;
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_n) *p.dcount = 0;
  }
}

// Builds every tile's pair signature from scratch (upload / reset): wave per tile; a tile longer
// than one wave chunk gets an all-ones signature (always a candidate).
__global__ __launch_bounds__(kThreads) void k_sig_build(const int32_t* tok, const uint64_t* tile_off,
                                                         const uint32_t* tile_len, uint32_t ntiles, uint32_t* sig) {
  __shared__ uint32_t s_sig[kWaves][kSigWords];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int p0 = lane * kPer;
  for (uint32_t t = blockIdx.x * kWaves + wid; t < ntiles; t += gridDim.x * kWaves) {
    const uint32_t len = tile_len[t];
    uint32_t* dst = sig + (size_t)t * kSigWords;
    if (len > (uint32_t)kWaveTok) {
      for (int w = lane; w < kSigWords; w += 64) dst[w] = ~0u;
      continue;
    }
    const int32_t* base = tok + tile_off[t];
    int32_t v[kPer];
    load_chunk(base, 0, len, p0, v);
    const int32_t m = base[p0 + kPer];
    int32_t nx = wave_next(v[0]);
    if (lane == 63) nx = (uint32_t)(p0 + kPer) < len ? m : kPad;
    sig_rebuild(s_sig[wid], dst, v, nx, lane);
  }
}

}  // namespace

Device::Device(int device_ordinal) : ordinal_(device_ordinal) {
  HIP_OK(hipSetDevice(ordinal_));
  hipStream_t s;
  HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  stream_ = s;
  res_.set_stream(stream_);
  HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  aux_stream_ = s;
  for (auto& e : ev_) {
    hipEvent_t ev;
    HIP_OK(hipEventCreate(&ev));
    e = ev;
  }
  for (int i = 0; i < kEvPairs; ++i) {
    for (auto& e : mev_[i]) {
      hipEvent_t ev;
      HIP_OK(hipEventCreate(&ev));
      e = ev;
    }
    ev_free_.push_back(i);
  }
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, ordinal_));
  cu_count_ = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  const unsigned pin = hipHostMallocMapped | hipHostMallocCoherent;
  for (MergeSlot& sl : slot_) {
    HIP_OK(hipHostMalloc((void**)&sl.host_count, 128, pin));
    std::memset(sl.host_count, 0, 64);
    HIP_OK(hipHostGetDevicePointer(&sl.dev_count, sl.host_count, 0));
  }
  if (const char* e = std::getenv("SHREDWORD_MERGE_GROUPS")) set_merge_groups(std::atoi(e));
  merge_params_ = new MergeParams();
  unmerge_params_ = new UnmergeParams();
  // diagnostic per-launch log: "C seq X candidates grid 0 merged records" / "R seq X candidates grid 0"
  if (const char* e = std::getenv("SHREDWORD_MERGE_LOG")) merge_log_ = std::fopen(e, "w");
#ifdef SHRED_STAMPS
  HIP_OK(hipMalloc(&stamps_, (size_t)kMaxMergeGroups * 4 * kStamps * sizeof(u64)));
  HIP_OK(hipMemset(stamps_, 0, (size_t)kMaxMergeGroups * 4 * kStamps * sizeof(u64)));
#endif
  if (const char* e = std::getenv("SHREDWORD_TILE_SKIP")) skip_ = std::atoi(e) != 0;
  if (const char* e = std::getenv("SHREDWORD_RESIDENT")) resident_on_ = std::atoi(e) != 0;
  if (const char* e = std::getenv("SHREDWORD_INDEX")) index_on_ = std::atoi(e) != 0;
  if (const char* e = std::getenv("SHREDWORD_HYBRID")) hybrid_ = std::atoi(e) != 0;
  if (const char* e = std::getenv("SHREDWORD_SWITCH_OCC")) switch_occ_ = std::strtoull(e, nullptr, 10);
  int nb = 0;  // resident workgroups of k_merge per CU
  HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(&k_merge<true>), kThreads, 0));
  merge_blocks_per_cu_ = nb > 0 ? nb : 4;
}

// Grid cap of k_merge (tuning).
void Device::set_merge_groups(int groups) { max_groups_ = std::max(1, std::min(kMaxMergeGroups, groups)); }

void Device::set_exchange(const Exchange& x) {
  if (slot_[0].dsum || slot_[1].dsum || slot_[2].dsum || slot_[3].dsum) fatal("set_exchange: merge buffers already exist");
  if (x.world < 1 || x.world > 64 || !x.allgather || x.bucket_records < 1) fatal("set_exchange: bad exchange");
  xchg_ = x;
  exchange_ = true;
}

void Device::free_slot(MergeSlot& s, bool keep_host) {
  for (void* p : {(void*)s.dsum, (void*)s.dft, (void*)s.dlist, (void*)s.dcount})
    if (p) HIP_OK(hipFree(p));
  s.dsum = s.dft = nullptr;
  s.dlist = s.dcount = nullptr;
  if (s.host_recs) HIP_OK(hipHostFree(s.host_recs));
  s.host_recs = nullptr;
  for (void* q : {(void*)s.xsend, (void*)s.xrecv})
    if (q) HIP_OK(hipFree(q));
  s.xsend = s.xrecv = nullptr;
  for (void* q : {(void*)s.host_xrecs, (void*)s.host_xhdr})
    if (q) HIP_OK(hipHostFree(q));
  s.host_xrecs = nullptr;
  s.host_xhdr = nullptr;
  s.cap = 0;
  s.launched = false;
  if (!keep_host) {
    if (s.host_mlist) HIP_OK(hipHostFree(s.host_mlist));
    s.host_mlist = nullptr;
    if (s.host_count) HIP_OK(hipHostFree(s.host_count));
    s.host_count = nullptr;
    if (s.dmlist) HIP_OK(hipFree(s.dmlist));
    s.dmlist = nullptr;
    for (void* q : {(void*)s.rhdr, (void*)s.rrec, (void*)s.rtile})
      if (q) HIP_OK(hipFree(q));
    s.rhdr = nullptr;
    s.rrec = nullptr;
    s.rtile = nullptr;
  }
}

// The streams of aborted resident launches: their missing workgroups may still start once the CUs
// free up, and they read the token table, the weights, the signatures and the resident plan
// before they see the abort.  Every path that frees or reallocates those buffers drains them first.
void Device::drain_retired() {
  for (void* s : retired_streams_) {
    (void)hipStreamSynchronize(S(s));
    (void)hipStreamDestroy(S(s));
  }
  retired_streams_.clear();
}

void Device::free_all() {
  drain_retired();
  void* ptrs[] = {tok_, tok0_, tile_off_, tile_len_, tile_len0_, weight_, sig_};
  for (void* p : ptrs)
    if (p) HIP_OK(hipFree(p));
  sig_ = nullptr;
  tok_ = tok0_ = nullptr;
  tile_off_ = nullptr;
  tile_len_ = tile_len0_ = nullptr;
  weight_ = nullptr;
  for (MergeSlot& s : slot_) free_slot(s, true);
  if (xrecv2_) HIP_OK(hipFree(xrecv2_));
  xrecv2_ = nullptr;
  xrecv2_bytes_ = 0;
  ntiles_ = 0;
  bytes_alloc_ = 0;
  uploaded_ = false;
}

Device::~Device() {
  (void)hipSetDevice(ordinal_);
  if (res_.running() && !res_.in_flight()) park();
  delete wl_;  // ends its launch first
  wl_ = nullptr;
  (void)hipStreamSynchronize(S(stream_));
  drain_retired();  // aborted resident launches: their late workgroups leave first
  res_.free_plan();
  (void)hipStreamSynchronize(S(stream_));
  (void)hipStreamSynchronize(S(aux_stream_));
  free_all();
  for (MergeSlot& s : slot_) free_slot(s, false);
  if (host_ulist_) (void)hipHostFree(host_ulist_);
  delete static_cast<MergeParams*>(merge_params_);
  delete static_cast<UnmergeParams*>(unmerge_params_);
  for (auto e : ev_)
    if (e) (void)hipEventDestroy((hipEvent_t)e);
  for (auto& pr : mev_)
    for (auto e : pr)
      if (e) (void)hipEventDestroy((hipEvent_t)e);
  if (stream_) (void)hipStreamDestroy(S(stream_));
  if (merge_log_) std::fclose(merge_log_);
  if (aux_stream_) (void)hipStreamDestroy(S(aux_stream_));
}

void Device::upload(const TiledStream& ts, Layout layout, const std::vector<uint64_t>& weights, int32_t max_id) {
  const bool report = std::getenv("SHREDWORD_LOAD_REPORT") != nullptr;
  double tph[8];
  tph[0] = now_seconds();
  HIP_OK(hipSetDevice(ordinal_));
  park();
  HIP_OK(hipStreamSynchronize(S(stream_)));
  flush_timing(true);
  free_all();
  layout_ = layout;
  ntiles_ = ts.num_tiles();
  tok_elems_ = ts.elems;
  live_tokens0_ = ts.live;
  live_tokens_est_ = ts.live;
  nentries_ = ts.entries;
  ft_tiles_ = ts.ft_tiles;
  ft_live_tokens_ = 0;
  for (size_t t = 0; t < ft_tiles_; ++t) ft_live_tokens_ += ts.len[t];
  tok_ = dalloc<int32_t>(ts.elems + 4 + kStreamPad, &bytes_alloc_);
  tok0_ = dalloc<int32_t>(ts.elems + 4 + kStreamPad, &bytes_alloc_);
  tile_off_ = dalloc<uint64_t>(ntiles_, &bytes_alloc_);
  tile_len_ = dalloc<uint32_t>(ntiles_, &bytes_alloc_);
  tile_len0_ = dalloc<uint32_t>(ntiles_, &bytes_alloc_);
  HIP_OK(hipMemcpyAsync(tok0_, ts.tok.data(), (ts.elems + 4) * sizeof(int32_t), hipMemcpyHostToDevice, S(stream_)));
  if (ntiles_) {
    HIP_OK(hipMemcpyAsync(tile_off_, ts.off.data(), ntiles_ * sizeof(uint64_t), hipMemcpyHostToDevice, S(stream_)));
    HIP_OK(hipMemcpyAsync(tile_len0_, ts.len.data(), ntiles_ * sizeof(uint32_t), hipMemcpyHostToDevice, S(stream_)));
  }
  if (layout == Layout::kTypes) {
    weight_ = dalloc<uint64_t>(weights.size(), &bytes_alloc_);
    if (!weights.empty())
      HIP_OK(hipMemcpyAsync(weight_, weights.data(), weights.size() * sizeof(uint64_t), hipMemcpyHostToDevice,
                            S(stream_)));
  }
  HIP_OK(hipStreamSynchronize(S(stream_)));
  tph[1] = now_seconds();
  for (MergeSlot& s : slot_) {
    if (s.host_mlist) HIP_OK(hipHostFree(s.host_mlist));
    // one entry per (tile, chain merge) that matched
    HIP_OK(hipHostMalloc((void**)&s.host_mlist, ((size_t)ntiles_ * kChainMax + 1) * sizeof(uint32_t),
                         hipHostMallocMapped | hipHostMallocCoherent));
    HIP_OK(hipHostGetDevicePointer(&s.dev_mlist, s.host_mlist, 0));
    if (s.dmlist) HIP_OK(hipFree(s.dmlist));
    s.dmlist = dalloc<uint32_t>((size_t)ntiles_ * kChainMax + 1, &bytes_alloc_);
    // per-workgroup regions of the fused completion (k_merge)
    if (!s.rhdr) {
      s.rhdr = dalloc<uint32_t>((size_t)kMaxMergeGroups * kRegHdr, &bytes_alloc_);
      s.rrec = dalloc<uint64_t>((size_t)kMaxMergeGroups * kDeltaLdsW * 3, &bytes_alloc_);
      // k_merge's regions hold kMtLds tiles each, k_resident's every tile of its owner
      s.rtile = dalloc<uint32_t>((size_t)kMaxMergeGroups * std::max<uint32_t>(kMtLds, kResMaxTiles), &bytes_alloc_);
    }
  }
  if (host_ulist_) HIP_OK(hipHostFree(host_ulist_));
  HIP_OK(hipHostMalloc((void**)&host_ulist_, (ntiles_ + 1) * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent));
  HIP_OK(hipHostGetDevicePointer(&dev_ulist_, host_ulist_, 0));
  run_count_ = 0;
  run_head_ = 0;
  unmerge_pending_ = false;
  // per-tile pair signatures (built by reset_tokens)
  sig_ = dalloc<uint32_t>(std::max<size_t>(ntiles_, 1) * kSigWords, &bytes_alloc_);
  tph[2] = now_seconds();
  index_.build(ts);
  tph[3] = now_seconds();
  max_id_seen_ = max_id;
  max_id0_ = max_id;
  uploaded_ = true;
  words_stale_ = false;
  wl_pristine_index_ = true;
  if (wl_ && (layout != Layout::kTypes || exchange_ || !index_on_)) {
    delete wl_;
    wl_ = nullptr;
  }
  if (layout == Layout::kTypes && !exchange_ && index_on_) {
    if (!wl_) wl_ = new WordLoop(ordinal_, stream_, unk_);
    if (fin_ >= 0) wl_->set_finalize((uint32_t)fin_);
    if (!wl_->upload(ts, weight_)) {
      delete wl_;
      wl_ = nullptr;
    }
  }
  tph[4] = now_seconds();
  reset_tokens();
  tph[5] = now_seconds();
  if (layout_ == Layout::kTypes) res_.plan(ts, tok_, tile_off_, tile_len_, weight_, cu_count_, &bytes_alloc_);
  else res_.free_plan();
  tph[6] = now_seconds();
  if (report)
    std::fprintf(stderr, "[LOAD] device upload: tables + copies %.1f ms, host-visible slots %.1f ms, tile index %.1f ms, "
                 "word runs + index %.1f ms, reset %.1f ms, resident plan %.1f ms\n", 1e3 * (tph[1] - tph[0]),
                 1e3 * (tph[2] - tph[1]), 1e3 * (tph[3] - tph[2]), 1e3 * (tph[4] - tph[3]), 1e3 * (tph[5] - tph[4]),
                 1e3 * (tph[6] - tph[5]));
}

void Device::set_index(bool on) {
  park();
  index_on_ = on;
}

// Both persistent loops end; the tiles in HBM are current.
void Device::park() {
  index_sync();
  if (!res_.running()) return;
  HIP_OK(hipSetDevice(ordinal_));
  double ms = 0;
  const uint64_t merges = res_.stop(&ms);
  if (timing_ && merges) {  // one launch: its wall time is the merge loop's device time
    times_.merge_ms += ms;
    times_.merge_launches += merges;
    times_.res_ms += ms;
  }
  rebuild_signatures();  // the tiles are back in HBM: their pair signatures for k_merge / k_unmerge
}

// The indexed loop's launch ends and the tile stream catches up with its words (the tile
// kernels — K1, K6, k_merge, downloads — read the tiles).
void Device::index_sync() {
  if (!wl_) return;
  if (wl_->running()) wl_->stop();
  const WordLoopStats& ws = wl_->stats();
  if (timing_ && ws.merges > wl_ms_seen_) {  // the launch's wall time is the merge loop's device time
    times_.merge_launches += ws.merges - wl_ms_seen_;
    times_.merge_ms += ws.kernel_ms - wl_kms_seen_;
  }
  wl_ms_seen_ = ws.merges;
  wl_kms_seen_ = ws.kernel_ms;
  if (wl_->tiles_dirty() && ntiles_) {
    wl_->sync_tiles(tok_, tile_off_, tile_len_);
    rebuild_signatures();
  }
}

// Hybrid: the resident loop ends (its tiles written back) and the indexed loop takes the merged
// words from the tiles and indexes them, all on the device.
void Device::hybrid_switch(int32_t X) {
  const double t0 = now_seconds();
  switch_pending_ = false;
  park();
  idx_phase_ = true;
  if (!wl_ || !wl_->ready()) return;
  wl_->reserve(std::max(X, reserved_max_id_));
  wl_->load_tiles(tok_, tile_off_, tile_len_);
  words_stale_ = false;
  wl_pristine_index_ = false;
  switch_x_ = X;
  switch_ms_ += 1e3 * (now_seconds() - t0);
}

// A tile-path merge ran after the loop's last merge: the loop takes the tiles' words.
void Device::index_refresh() {
  park();
  wl_->load_tiles(tok_, tile_off_, tile_len_);
  words_stale_ = false;
  wl_pristine_index_ = false;
}

void Device::reset_tokens() {
  HIP_OK(hipSetDevice(ordinal_));
  park();
  if (!uploaded_) return;
  for (const MergeSlot& s : slot_)
    if (s.launched) fatal("reset_tokens with a merge in flight");
  HIP_OK(hipMemcpyAsync(tok_, tok0_, (tok_elems_ + 4) * sizeof(int32_t), hipMemcpyDeviceToDevice, S(stream_)));
  if (ntiles_) {
    HIP_OK(hipMemcpyAsync(tile_len_, tile_len0_, ntiles_ * sizeof(uint32_t), hipMemcpyDeviceToDevice, S(stream_)));
    rebuild_signatures();
  }
  live_tokens_est_ = live_tokens0_;
  max_id_seen_ = max_id0_;
  index_.reset();
  idx_phase_ = false;
  switch_pending_ = false;
  sw_n_ = 0;
  if (wl_) {
    if (hybrid_resident_phase()) {  // the switch re-indexes the merged words
      wl_->reset_words();
      words_stale_ = true;
    } else {
      wl_->reset();
      if (!wl_pristine_index_) wl_->rebuild();
      wl_pristine_index_ = true;
      words_stale_ = false;
    }
  }
}

// Every tile's pair signature from its tokens in HBM (k_merge / k_unmerge test them).
void Device::rebuild_signatures() {
  const int grid = (int)std::min<size_t>((ntiles_ + kWaves - 1) / kWaves, (size_t)cu_count_ * 8);
  k_sig_build<<<grid, kThreads, 0, S(stream_)>>>(tok_, tile_off_, tile_len_, (uint32_t)ntiles_, sig_);
  HIP_OK(hipGetLastError());
}

// Sizes one merge slot's tables for ids < need.  Only called for the slot about to be
// launched, which is never the one still in flight, so the other slot's results survive.
void Device::ensure_slots(MergeSlot& s, uint32_t need) {
  if (need <= s.cap && s.dsum) return;
  uint32_t cap = std::max<uint32_t>(s.cap ? s.cap : 4096, 4096);
  while (cap < need) cap *= 2;
  HIP_OK(hipStreamSynchronize(S(stream_)));
  HIP_OK(hipStreamSynchronize(S(aux_stream_)));
  size_t old_bytes = s.dsum ? (size_t)kChainMax * 4 * ((size_t)s.cap + 1) * 20 + 16 + 64 : 0;
  if (s.xsend) {
    const size_t old_rec_cap = (size_t)kChainMax * 4 * ((size_t)s.cap + 1) + (size_t)kMaxMergeGroups * kDeltaLdsW;
    old_bytes += 32 + (xchg_.bucket_records + old_rec_cap) * sizeof(DeltaRecord) + xchg_.world * exchange_bucket_bytes();
  }
  free_slot(s, true);
  bytes_alloc_ -= old_bytes;
  keys_per_merge_ = (uint32_t)(4 * ((size_t)cap + 1));
  const size_t keys = (size_t)kChainMax * keys_per_merge_;  // one key range per chain merge
  s.dsum = dalloc<uint64_t>(keys + 2, &bytes_alloc_);  // + 2 stats words at the end
  s.dft = dalloc<uint64_t>(keys, &bytes_alloc_);
  s.dlist = dalloc<uint32_t>(keys, &bytes_alloc_);
  s.dcount = dalloc<uint32_t>(16, &bytes_alloc_);
  HIP_OK(hipMemsetAsync(s.dsum, 0, (keys + 2) * sizeof(u64), S(stream_)));
  HIP_OK(hipMemsetAsync(s.dft, 0xFF, keys * sizeof(u64), S(stream_)));
  HIP_OK(hipMemsetAsync(s.dcount, 0, 16 * sizeof(uint32_t), S(stream_)));
  // records: the fused completion ships every workgroup's LDS-reduced records (duplicates across
  // workgroups included), at most kMaxMergeGroups x kDeltaLdsW, plus spilled global slots
  const size_t rec_cap = keys + (size_t)kMaxMergeGroups * kDeltaLdsW;
  HIP_OK(hipHostMalloc((void**)&s.host_recs, rec_cap * sizeof(DeltaRecord), hipHostMallocMapped | hipHostMallocCoherent));
  HIP_OK(hipHostGetDevicePointer(&s.dev_recs, s.host_recs, 0));
  if (exchange_) {
    // the bucket header, then room for every record plus one overflow window past the bucket
    const size_t W = (size_t)xchg_.world, cap_x = xchg_.bucket_records;
    s.xsend = dalloc<uint8_t>(32 + (cap_x + rec_cap) * sizeof(DeltaRecord), &bytes_alloc_);
    s.xrecv = dalloc<uint8_t>(W * exchange_bucket_bytes(), &bytes_alloc_);
    HIP_OK(hipHostMalloc((void**)&s.host_xrecs, W * cap_x * sizeof(DeltaRecord), hipHostMallocMapped | hipHostMallocCoherent));
    HIP_OK(hipHostGetDevicePointer(&s.dev_xrecs, s.host_xrecs, 0));
    HIP_OK(hipHostMalloc((void**)&s.host_xhdr, 2 * W * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent));
    HIP_OK(hipHostGetDevicePointer(&s.dev_xhdr, s.host_xhdr, 0));
  }
  s.cap = cap;
  HIP_OK(hipStreamSynchronize(S(stream_)));
}

// Folds completed sampled k_merge launches into times_ (block: wait for all of them).
void Device::flush_timing(bool block) {
  size_t keep = 0;
  for (size_t i = 0; i < ev_pending_.size(); ++i) {
    const PendingEv pe = ev_pending_[i];
    hipEvent_t e1 = (hipEvent_t)mev_[pe.pair][1];
    if (block) {
      HIP_OK(hipEventSynchronize(e1));
    } else {
      const hipError_t q = hipEventQuery(e1);
      if (q == hipErrorNotReady) {
        ev_pending_[keep++] = pe;
        continue;
      }
      HIP_OK(q);
    }
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, (hipEvent_t)mev_[pe.pair][0], e1));
    times_.merge_ms += ms;
    times_.merge_launches += 1;
    times_.merge_bytes += pe.bytes;
    ev_free_.push_back(pe.pair);
  }
  ev_pending_.resize(keep);
}

int Device::device_select(const std::vector<PairCount>& pairs, int32_t X0, int n, uint64_t min_freq,
                          std::vector<SelectedMerge>* out) {
  HIP_OK(hipSetDevice(ordinal_));
  park();
  if (!wl_ || !wl_->ready() || exchange_ || layout_ != Layout::kTypes || !index_on_) return -1;
  if (switch_pending_ || hybrid_resident_phase()) {  // the resident phase ends here (its tiles are current)
    switch_pending_ = false;
    idx_phase_ = true;
    switch_x_ = X0;
    words_stale_ = true;
    wl_->reserve(std::max(X0 + n, reserved_max_id_));  // as hybrid_switch: the id tables before the index
  }
  if (words_stale_) index_refresh();  // the words from the tiles (a tile-path merge, or a reset)
  const int r = wl_->run_select(pairs, X0, (uint32_t)std::max(n, 0), min_freq, out);
  if (r > 0) {
    max_id_seen_ = std::max(max_id_seen_, X0 + r - 1);
    idx_phase_ = true;  // later merges of this train() go to the indexed loop
    wl_pristine_index_ = false;
  }
  return r;
}

bool Device::index_id_room(int32_t max_id) const { return wl_ && (uint32_t)max_id + 2 <= wl_->id_room(); }

// merge_chain's resident branch: one merge (ab[0], ab[1]) -> X0 posted to the launch.
void Device::post_resident_merge(const int32_t* ab, int32_t X0) {
  if (res_.in_flight() >= (size_t)kResSlots) fatal("merge_chain: every resident slot has a merge in flight");
  const int slot = res_.running() && res_.aborted() ? -1 : res_.pick_slot();
  if (slot < 0) {  // the launch aborted (not co-resident): this merge and those in flight go elsewhere
    resident_abort_fallback();
    merge_chain(ab, 1, X0);
    return;
  }
  bool grow = false;
  for (const MergeSlot& s2 : slot_) grow |= !s2.dsum || (uint32_t)X0 + 2 > s2.cap;
  if (grow) {  // the delta tables grow: only between launches
    if (res_.in_flight()) fatal("merge_chain: delta tables too small with a resident merge in flight");
    park();
    for (MergeSlot& s2 : slot_) ensure_slots(s2, (uint32_t)X0 + 2);
    uint32_t cap = 0;
    for (const MergeSlot& s2 : slot_) cap = std::max(cap, s2.cap);
    for (MergeSlot& s2 : slot_) ensure_slots(s2, cap);
  }
  max_id_seen_ = std::max(max_id_seen_, X0);
  visited_tiles_ += res_.post_merge(slot, ab[0], ab[1], X0, skip_ ? &index_ : nullptr);
}

// collect's resident branch: what merge X, seen complete, means for the tile index, the
// statistics and the hybrid switch.
size_t Device::collect_resident(int32_t X, const DeltaRecord** recs) {
  ResidentLoop::Collected c;
  if (!res_.collect(X, &c)) {
    resident_abort_fallback();
    return collect(X, recs);
  }
  const uint64_t* hs = c.hs;
  if (c.n_tiles == kAllTiles) index_.set_all(X);
  else index_.set_tiles_bits(X, c.tiles, c.n_tiles);
  if (res_.stamps() && merge_log_)  // diagnostic: host post / flag-seen clock beside the device's dispatch / flag
    std::fprintf(merge_log_, "S %d %u %.2f %.2f %.2f %llu %llu %zu %u\n", X, c.nparts, 1e6 * c.t_post, 1e6 * c.t_wait,
                 1e6 * c.t_flag, (unsigned long long)hs[8], (unsigned long long)(hs[8] + hs[2]), c.n, c.n_tiles);
  if (timing_) {
    times_.merge_bytes += 4.0 * (double)live_tokens_est_;
    times_.res_bytes += 4.0 * (double)live_tokens_est_;
    times_.res_k3_bytes += 8.0 * (double)hs[1];  // hs[1]: tokens the merge's matched tiles hold after it
    times_.res_merges += 1;
  }
  if (hybrid_ && !idx_phase_ && index_on_ && wl_ && wl_->ready()) {
    // entries merged per merge is far from monotone (a frequent pair of a few common words sits
    // between pairs spread over many words): switch once a whole window of merges stayed small
    sw_win_[sw_n_++ % kSwitchWindow] = hs[0];
    uint64_t mx = 0;
    for (uint64_t v : sw_win_) mx = std::max(mx, v);
    if (sw_n_ >= kSwitchWindow && mx < switch_occ_) switch_pending_ = true;
  }
  live_tokens_est_ -= hs[0];
  records_total_ += c.n;
  records_max_ = std::max<uint64_t>(records_max_, c.n);
  *recs = c.recs;
  return c.n;
}

// The resident launch aborted before dispatching anything (some workgroups never became
// resident: another kernel or process holds CUs).  Resident is off for this device from here on;
// the merges posted to it run again, in order, on the indexed loop (or the launch path).  The
// launch's missing workgroups may start only once those CUs free up, and they hold its stream
// until then, so all further work moves to a fresh stream.
void Device::resident_abort_fallback() {
  const std::vector<ResidentLoop::Post> inflight = res_.abandon();
  res_.disable();
  ++res_aborts_;
  retired_streams_.push_back(stream_);
  hipStream_t s;
  HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  stream_ = s;
  res_.set_stream(stream_);
  if (wl_) wl_->set_stream(stream_);
  if (std::getenv("SHREDWORD_RESIDENT_REPORT"))
    std::fprintf(stderr, "[RESIDENT] launch aborted (not every workgroup resident): %zu merges move to the %s\n",
                 inflight.size(), wl_ && wl_->ready() ? "indexed loop" : "launch path");
  for (const ResidentLoop::Post& rp : inflight) {
    const int32_t ab[2] = {rp.a, rp.b};
    merge_chain(ab, 1, rp.X);
  }
}

void Device::merge_chain(const int32_t* ab, int n, int32_t X0) {
  HIP_OK(hipSetDevice(ordinal_));
  if (n < 1 || n > kChainMax) fatal("merge_chain: bad chain length");
  if (switch_pending_ && n == 1 && run_count_ == 0 && !res_.in_flight()) hybrid_switch(X0);
  if (n == 1 && index_eligible() && run_count_ == 0 && !res_.in_flight()) {  // the indexed loop
    if (words_stale_) index_refresh();
    if (!wl_->in_flight()) wl_->reserve(X0);
    max_id_seen_ = std::max(max_id_seen_, X0);
    wl_->post_merge(ab[0], ab[1], X0);
    return;
  }
  if (wl_) {
    if (wl_->in_flight()) fatal("merge_chain: a tile-path merge while indexed merges are in flight");
    index_sync();
    words_stale_ = true;  // the tile path changes the tiles behind the loop's words
  }
  if (n == 1 && run_count_ == 0 && ntiles_ && resident_eligible() && X0 < (1 << 20)) {  // k_resident (ids: 20 bits)
    post_resident_merge(ab, X0);
    return;
  }
  park();
  if (run_count_ >= 2) fatal("merge_chain: two launches are already in flight");
  ChainRun& run = run_at(run_count_);
  run.slot = (run_head_ + run_count_) & 1;
  MergeSlot& sl = slot_[run.slot];
  if (sl.launched) fatal("merge_chain: the slot is still in flight");
  const int32_t Xn = X0 + n - 1;
  max_id_seen_ = std::max(max_id_seen_, Xn);
  ensure_slots(sl, (uint32_t)Xn + 1);
  run.X0 = X0;
  run.n = n;
  run.collected = 0;
  run.waited = false;
  for (int i = 0; i < 2 * n; ++i) run.ab[i] = ab[i];
  ++run_count_;
  if (!ntiles_ && !exchange_) return;
  sl.seq = ++seq_;
  sl.launched = true;
  if (!ntiles_) {  // an empty shard still joins the exchange, with an empty bucket
    std::memset(sl.host_count, 0, 32);
    HIP_OK(hipMemsetAsync(sl.xsend, 0, 32, S(stream_)));
    exchange_launch(sl);
    return;
  }
  MergeParams& mp = *static_cast<MergeParams*>(merge_params_);
  mp.tok = tok_;
  mp.tile_off = tile_off_;
  mp.tile_len = tile_len_;
  mp.ntiles = (uint32_t)ntiles_;
  mp.weight = weight_;
  mp.X0 = X0;
  mp.nchain = n;
  for (int i = 0; i < n; ++i) {
    mp.ca[i] = ab[2 * i];
    mp.cb[i] = ab[2 * i + 1];
  }
  mp.keys_per_merge = keys_per_merge_;
  mp.slot_cap = sl.cap;
  mp.dsum = U(sl.dsum);
  mp.dft = U(sl.dft);
  mp.dlist = sl.dlist;
  mp.dcount = sl.dcount;
  mp.stats = U(sl.dsum) + (size_t)kChainMax * keys_per_merge_;
  mp.done = sl.dcount + 1;
  mp.out = exchange_ ? (DeltaRecord*)(sl.xsend + 32) : (DeltaRecord*)sl.dev_recs;
  mp.xhdr = exchange_ ? (uint32_t*)sl.xsend : nullptr;
  mp.hcount = (uint32_t*)sl.dev_count;
  mp.hstats = (u64*)((char*)sl.dev_count + 16);
  mp.mlist = sl.dmlist;
  mp.hmlist = (uint32_t*)sl.dev_mlist;
  mp.mcount = sl.dcount + 10;
  mp.seq = sl.seq;
  mp.nlist = 0;
  // tile skipping: the union of the chain's candidate tiles when it is short
  bool use_list = skip_;
  cand_.clear();
  if (n == 1) {
    use_list = use_list && index_.candidates(ab[0], ab[1], &cand_) && cand_.size() <= kInlineTiles;
  }
  for (int i = 0; i < n && n > 1 && use_list; ++i) {
    if (!index_.candidates(ab[2 * i], ab[2 * i + 1], &cand1_)) {
      use_list = false;
      break;
    }
    if (i == 0) {
      cand_.swap(cand1_);
    } else {
      cand2_.clear();
      std::set_union(cand_.begin(), cand_.end(), cand1_.begin(), cand1_.end(), std::back_inserter(cand2_));
      cand_.swap(cand2_);
    }
    if (cand_.size() > kInlineTiles) use_list = false;
  }
  if (use_list && !cand_.empty()) {
    mp.nlist = (uint32_t)cand_.size();
    std::memcpy(mp.list, cand_.data(), cand_.size() * sizeof(uint32_t));
  }
  const size_t n_iter = mp.nlist ? mp.nlist : ntiles_;
  visited_tiles_ += n_iter;
  const size_t groups = (n_iter + kWin - 1) / kWin;  // one filter window per workgroup and pass
  const int grid = (int)std::min<size_t>(groups, (size_t)max_groups_);
  mp.sig = sig_;
  mp.stamps = stamps_;
  mp.rhdr = sl.rhdr;
  mp.rrec = U(sl.rrec);
  mp.rtile = sl.rtile;
  mp.filter = n_iter > 2 * kWin ? 1 : 0;  // short lists: load the tiles straight away
  sl.grid = (uint32_t)grid;
  sl.n_iter = (uint32_t)n_iter;
  // HIP events bracket every kTimingStride-th launch (an unbiased sample of launch durations
  // that keeps event overhead out of the timed loop); they are read back without blocking
  int pair = -1;
  if (timing_ && sl.seq % kTimingStride == 0) {
    flush_timing(false);
    if (!ev_free_.empty()) {
      pair = ev_free_.back();
      ev_free_.pop_back();
      HIP_OK(hipEventRecord((hipEvent_t)mev_[pair][0], S(stream_)));
    }
  }
  if (layout_ == Layout::kStream) k_merge<false><<<grid, kThreads, 0, S(stream_)>>>(mp);
  else k_merge<true><<<grid, kThreads, 0, S(stream_)>>>(mp);
  HIP_OK(hipGetLastError());
  if (pair >= 0) {
    HIP_OK(hipEventRecord((hipEvent_t)mev_[pair][1], S(stream_)));
    // algorithmic bytes of a merge: 4 B per live token, i.e. the scan
    // the reference makes per merge; the signature filter and tile index read far less
    ev_pending_.push_back({pair, 4.0 * (double)live_tokens_est_ * (double)n});
  }
  if (exchange_) exchange_launch(sl);
}

// Queued behind the slot's k_merge: the bucket all-gather over RCCL, then k_xout copies the
// valid records of every rank to the host and raises the slot's flag.  Every rank queues the
// same sequence of exchanges (the host decisions are identical on all ranks).
void Device::exchange_launch(MergeSlot& sl) {
  const size_t bucket = exchange_bucket_bytes();
  xchg_.allgather(xchg_.comm, sl.xsend, sl.xrecv, bucket, stream_);
  XoutParams xp;
  xp.recv = sl.xrecv;
  xp.bucket = (uint32_t)bucket;
  xp.cap = xchg_.bucket_records;
  xp.world = (uint32_t)xchg_.world;
  xp.out = (DeltaRecord*)sl.dev_xrecs;
  xp.hx = (uint32_t*)sl.dev_xhdr;
  xp.flag = (uint32_t*)sl.dev_count + 1;
  xp.seq = sl.seq;
  k_xout<<<1, 1024, 0, S(stream_)>>>(xp);
  HIP_OK(hipGetLastError());
}

// After the slot's flag: every rank's records, concatenated.  A rank whose records did not fit
// its bucket (or whose spilled deltas still need k_collect) sends the remainder in one more
// all-gather, sized by the largest remainder; every rank sees the same headers, so all of them
// take part in that round.
size_t Device::exchange_finish(MergeSlot& sl, const DeltaRecord** recs) {
  const int W = xchg_.world;
  const uint32_t cap = xchg_.bucket_records;
  size_t nvalid = 0, extra_max = 0;
  uint32_t valid[64], total[64];
  for (int r = 0; r < W; ++r) {
    const uint32_t h0 = sl.host_xhdr[2 * r], h1 = sl.host_xhdr[2 * r + 1];
    total[r] = h0 & ~kNeedCollect;
    valid[r] = std::min((h0 & kNeedCollect) ? h1 : h0 & ~kNeedCollect, cap);
    nvalid += valid[r];
    extra_max = std::max<size_t>(extra_max, total[r] - valid[r]);
  }
  *recs = sl.host_xrecs;
  if (extra_max == 0) return nvalid;
  ++x_overflows_;
  const uint32_t me = (uint32_t)xchg_.rank;
  DeltaRecord* mine = (DeltaRecord*)(sl.xsend + 32);
  if (ntiles_ && (sl.host_count[0] & kNeedCollect)) {  // this rank's spilled deltas, behind its records
    k_collect<<<256, kThreads, 0, S(stream_)>>>(sl.dcount, sl.dlist, U(sl.dsum), U(sl.dft), mine + sl.host_count[3]);
    HIP_OK(hipGetLastError());
    k_zero_u32<<<1, 1, 0, S(stream_)>>>(sl.dcount);
    HIP_OK(hipGetLastError());
  }
  const size_t bytes = extra_max * sizeof(DeltaRecord);
  if (xrecv2_bytes_ < bytes * W) {
    HIP_OK(hipStreamSynchronize(S(stream_)));
    if (xrecv2_) HIP_OK(hipFree(xrecv2_));
    xrecv2_bytes_ = bytes * W;
    HIP_OK(hipMalloc((void**)&xrecv2_, xrecv2_bytes_));
  }
  // the send window starts at this rank's first record not yet sent; the slot's send buffer has
  // room for a full window past any valid prefix (see ensure_slots)
  xchg_.allgather(xchg_.comm, mine + valid[me], xrecv2_, bytes, stream_);
  xstage_.resize(bytes * W);
  HIP_OK(hipMemcpyAsync(xstage_.data(), xrecv2_, bytes * W, hipMemcpyDeviceToHost, S(stream_)));
  HIP_OK(hipStreamSynchronize(S(stream_)));
  sl.xall.assign(sl.host_xrecs, sl.host_xrecs + nvalid);
  for (int r = 0; r < W; ++r) {
    const DeltaRecord* src = (const DeltaRecord*)(xstage_.data() + (size_t)r * bytes);
    sl.xall.insert(sl.xall.end(), src, src + (total[r] - valid[r]));
  }
  *recs = sl.xall.data();
  return sl.xall.size();
}

// Spins on the host-visible flag the last workgroup raises (much cheaper than a stream sync).
void Device::wait_flag(const MergeSlot& s) {
  volatile uint32_t* flag = s.host_count + 1;
  const double t0 = now_seconds();
  unsigned spins = 0;
  while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != s.seq) {
    __builtin_ia32_pause();
    if (++spins % 4096 == 0 && now_seconds() - t0 > 120.0) {
      const hipError_t e = hipStreamQuery(S(stream_));
      if (e != hipSuccess && e != hipErrorNotReady) HIP_OK(e);
      if (now_seconds() - t0 > 600.0) fatal("k_merge did not signal completion within 600 s");
    }
  }
}

// Waits for a run's launch and splits its records and matched tiles per merge.
void Device::finish_launch(ChainRun& run_) {
  MergeSlot& sl = slot_[run_.slot];
  run_.waited = true;
  for (int i = 0; i < run_.n; ++i) {
    run_.rp[i] = nullptr;
    run_.tp[i] = nullptr;
    run_.rn[i] = run_.tn[i] = 0;
  }
  if (!ntiles_ && !exchange_) return;
  DeltaRecord* drec = (DeltaRecord*)sl.dev_recs;
  if (sl.launched) {
    wait_flag(sl);
    unmerge_pending_ = false;  // stream order: an earlier k_unmerge has finished
  }
  const bool launched = sl.launched;
  sl.launched = false;
  const u64* hs = (const u64*)(sl.host_count + 4);
  size_t n;
  const uint32_t nm = launched ? sl.host_count[2] : 0;
  const DeltaRecord* all = sl.host_recs;
  if (exchange_) {
    n = exchange_finish(sl, &all);
  } else {
    n = sl.host_count[0];
    if (n & kNeedCollect) {  // too many spilled slots for one workgroup: a wide collect pass
      n &= ~kNeedCollect;
      k_collect<<<256, kThreads, 0, S(aux_stream_)>>>(sl.dcount, sl.dlist, U(sl.dsum), U(sl.dft),
                                                        drec + sl.host_count[3]);
      HIP_OK(hipGetLastError());
      k_zero_u32<<<1, 1, 0, S(aux_stream_)>>>(sl.dcount);
      HIP_OK(hipGetLastError());
      HIP_OK(hipStreamSynchronize(S(aux_stream_)));
    }
  }
  if (run_.n == 1) {  // one merge: its keys and tiles carry no chain index
    run_.rp[0] = all;
    run_.rn[0] = n;
    run_.tp[0] = sl.host_mlist;
    run_.tn[0] = nm;
  } else {
    // records carry chain index * keys_per_merge + key; tiles carry the index in their top bits
    for (int i = 0; i < run_.n; ++i) {
      run_.recs[i].clear();
      run_.tiles[i].clear();
    }
    const DeltaRecord* r = all;
    for (size_t i = 0; i < n; ++i) {
      const uint32_t j = r[i].key / keys_per_merge_;
      if (j >= (uint32_t)run_.n) fatal("k_merge record of a merge outside the chain");
      DeltaRecord d = r[i];
      d.key -= j * keys_per_merge_;
      run_.recs[j].push_back(d);
    }
    for (uint32_t i = 0; i < nm; ++i) {
      const uint32_t e = sl.host_mlist[i];
      const uint32_t j = e >> kChainShift;
      if (j >= (uint32_t)run_.n) fatal("k_merge matched tile of a merge outside the chain");
      run_.tiles[j].push_back(e & ((1u << kChainShift) - 1u));
    }
    for (int i = 0; i < run_.n; ++i) {
      run_.rp[i] = run_.recs[i].data();
      run_.rn[i] = run_.recs[i].size();
      run_.tp[i] = run_.tiles[i].data();
      run_.tn[i] = run_.tiles[i].size();
    }
  }
  if (timing_) flush_timing(false);
  if (launched) live_tokens_est_ -= hs[0];
  records_total_ += n;
  records_max_ = std::max<uint64_t>(records_max_, n);
  if (merge_log_) {
    // ... then this rank's records that left the workgroups' LDS hashes for the global tables
    // (host_count[3]: the LDS records ahead of them, 0 without a spill) and whether they were too
    // many for the fused collect (k_collect ran)
    const uint32_t own = launched ? sl.host_count[0] : 0, lds = launched ? sl.host_count[3] : 0;
    std::fprintf(merge_log_, "C %u %d %u %u %d %llu %zu %u %d", sl.seq, run_.X0, sl.n_iter, sl.grid, run_.n,
                 (unsigned long long)hs[0], n, lds ? (own & ~kNeedCollect) - lds : 0u, (own & kNeedCollect) ? 1 : 0);
#ifdef SHRED_STAMPS
    // per phase: when the last workgroup got there, in us after the first workgroup started
    std::vector<u64> st((size_t)sl.grid * kStamps);
    HIP_OK(hipStreamSynchronize(S(stream_)));
    HIP_OK(hipMemcpy(st.data(), stamps_, st.size() * sizeof(u64), hipMemcpyDeviceToHost));
    u64 t0 = ~0ull;
    for (uint32_t g = 0; g < sl.grid; ++g) t0 = std::min(t0, st[(size_t)g * kStamps]);
    for (int k = 1; k < 8; ++k) {
      u64 mx = 0;
      for (uint32_t g = 0; g < sl.grid; ++g) {
        const u64 v = st[(size_t)g * kStamps + k];
        if (v != 0 && v != ~0ull) mx = std::max(mx, v);
      }
      std::fprintf(merge_log_, " %.2f", mx >= t0 ? (double)(mx - t0) / 100.0 : -1.0);
    }
    // shader clock of workgroup 0 between its start and its ticket (MHz)
    std::fprintf(merge_log_, " %.0f", st[4] > st[0] ? (double)(st[17] - st[16]) / (double)(st[4] - st[0]) * 100.0 : -1.0);
    // workgroup 0's first pass through the window phases, relative to its own start
    for (int k = 8; k < 16; ++k) {
      const u64 v = st[k], s0 = st[0];
      std::fprintf(merge_log_, " %.2f", v >= s0 && v != 0 ? (double)(v - s0) / 100.0 : -1.0);
    }
    HIP_OK(hipMemset(stamps_, 0, st.size() * sizeof(u64)));
#endif
    std::fprintf(merge_log_, "\n");
  }
}

size_t Device::collect(int32_t X, const DeltaRecord** recs) {
  HIP_OK(hipSetDevice(ordinal_));
  last_changes_ = false;
  if (wl_ && wl_->in_flight()) {
    const size_t n = wl_->collect(X, recs);
    last_changes_ = wl_->last_changes();
    records_total_ += n;
    records_max_ = std::max<uint64_t>(records_max_, n);
    return n;
  }
  if (res_.in_flight()) return collect_resident(X, recs);
  if (run_count_ == 0) fatal("collect: no launch in flight");
  ChainRun& run = run_at(0);
  const int j = X - run.X0;
  if (j != run.collected || j >= run.n) fatal("collect: merge X is not the next merge of the oldest launch");
  if (!run.waited) finish_launch(run);
  index_.set_tiles(X, run.tp[j], run.tn[j]);
  ++run.collected;
  *recs = run.rp[j];
  const size_t n = run.rn[j];
  if (run.collected == run.n) {  // the oldest launch is consumed (its record vectors stay valid)
    run_head_ = (run_head_ + 1) & 1;
    --run_count_;
  }
  return n;
}

bool Device::peek(int32_t X, const DeltaRecord** recs, size_t* n) {
  return wl_ && wl_->in_flight() && wl_->peek(X, recs, n);
}

void Device::rollback(int32_t X) {
  HIP_OK(hipSetDevice(ordinal_));
  if (wl_ && wl_->in_flight()) {
    wl_->rollback(X);
    ++rollbacks_;
    return;
  }
  if (res_.in_flight()) {  // resident: each wrong guess is expanded back where it matched
    rollbacks_ += res_.rollback(X);
    return;
  }
  park();
  ++rollbacks_;
  // every uncollected merge >= X, newest launch first
  for (int k = run_count_ - 1; k >= 0; --k) {
    ChainRun& run = run_at(k);
    const int j0 = std::max(X - run.X0, run.collected);
    if (j0 >= run.n) continue;
    if (!run.waited && run.n == 1) {
      // a single merge not waited for: k_unmerge reads its matched tiles and their count from
      // the host memory the merge writes, queued behind it, so the host does not wait at all
      if (ntiles_) unmerge_launch(run, nullptr, 0);
      slot_[run.slot].launched = false;
      run.waited = true;
    } else {
      if (!run.waited) finish_launch(run);
      unmerge_run(run, j0);
    }
    run.n = j0;
  }
  while (run_count_ > 0 && run_at(run_count_ - 1).collected == run_at(run_count_ - 1).n) --run_count_;
}

// k_unmerge for merges j0 .. n-1 of a run (queued on the stream: the host never waits for it).
void Device::unmerge_run(ChainRun& run_, int j0) {
  const int nundo = run_.n - j0;
  if (!ntiles_ || nundo <= 0) return;
  // the tiles where any undone merge matched, once each (one merge lists each tile once)
  ulist_.clear();
  for (int j = j0; j < j0 + nundo; ++j) ulist_.insert(ulist_.end(), run_.tp[j], run_.tp[j] + run_.tn[j]);
  if (nundo > 1) {
    std::sort(ulist_.begin(), ulist_.end());
    ulist_.erase(std::unique(ulist_.begin(), ulist_.end()), ulist_.end());
  }
  MergeSlot& sl = slot_[run_.slot];
  if (merge_log_) std::fprintf(merge_log_, "R %u %d %zu %d\n", sl.seq, run_.X0 + j0, ulist_.size(), nundo);
  if (ulist_.empty()) return;
  // the previous k_unmerge may still read the list: it is ordered before this one on the
  // stream, but the host overwrites the pinned list now, so wait for it first
  if (unmerge_pending_) HIP_OK(hipStreamSynchronize(S(stream_)));
  std::memcpy(host_ulist_, ulist_.data(), ulist_.size() * sizeof(uint32_t));
  unmerge_pending_ = true;
  unmerge_launch(run_, host_ulist_, ulist_.size(), j0);
}

// Queues k_unmerge for merges j0 .. n-1 of a run over `tiles` (host-visible, n_tiles of them),
// or, with tiles == nullptr, over the single merge's own matched-tile list in host memory.
void Device::unmerge_launch(ChainRun& run_, const uint32_t* tiles, size_t n_tiles, int j0) {
  const int nundo = run_.n - j0;
  MergeSlot& sl = slot_[run_.slot];
  UnmergeParams& up = *static_cast<UnmergeParams*>(unmerge_params_);
  up.tok = tok_;
  up.tile_off = tile_off_;
  up.tile_len = tile_len_;
  if (tiles) {
    void* d = nullptr;
    HIP_OK(hipHostGetDevicePointer(&d, const_cast<uint32_t*>(tiles), 0));
    up.tiles = (const uint32_t*)d;
    up.ntl = (uint32_t)n_tiles;
    up.ntl_dev = nullptr;
  } else {
    up.tiles = (const uint32_t*)sl.dev_mlist;
    up.ntl = 0;
    up.ntl_dev = (const uint32_t*)sl.dev_count + 2;
  }
  up.nundo = nundo;
  up.ux0 = run_.X0 + j0;
  for (int j = 0; j < nundo; ++j) {
    up.ua[j] = run_.ab[2 * (j0 + j)];
    up.ub[j] = run_.ab[2 * (j0 + j) + 1];
  }
  up.dcount = sl.dcount;
  up.dlist = sl.dlist;
  up.dsum = U(sl.dsum);
  up.dft = U(sl.dft);
  up.sig = sig_;
  const int grid = tiles ? (int)std::min<size_t>((n_tiles + kWaves - 1) / kWaves, (size_t)kMaxMergeGroups)
                         : kMaxMergeGroups;
  k_unmerge<<<grid, kThreads, 0, S(stream_)>>>(up);
  HIP_OK(hipGetLastError());
}

void Device::download_tokens(std::vector<int32_t>* out) {
  HIP_OK(hipSetDevice(ordinal_));
  park();
  out->clear();
  if (!ntiles_) return;
  std::vector<int32_t> all(tok_elems_ + 4);
  std::vector<uint64_t> off(ntiles_);
  std::vector<uint32_t> lens(ntiles_);
  HIP_OK(hipMemcpyAsync(all.data(), tok_, all.size() * sizeof(int32_t), hipMemcpyDeviceToHost, S(stream_)));
  HIP_OK(hipMemcpyAsync(off.data(), tile_off_, ntiles_ * sizeof(uint64_t), hipMemcpyDeviceToHost, S(stream_)));
  HIP_OK(hipMemcpyAsync(lens.data(), tile_len_, ntiles_ * sizeof(uint32_t), hipMemcpyDeviceToHost, S(stream_)));
  HIP_OK(hipStreamSynchronize(S(stream_)));
  for (size_t t = 0; t < ntiles_; ++t) out->insert(out->end(), all.begin() + off[t], all.begin() + off[t] + lens[t]);
}

// Both slots' delta tables cover ids up to max_id before a launch needs them (a launch holds
// the table pointers, so they cannot grow under it).
void Device::reserve_ids(int32_t max_id) {
  HIP_OK(hipSetDevice(ordinal_));
  reserved_max_id_ = max_id;
  if (index_eligible() && !wl_->in_flight()) wl_->reserve(max_id);
  const uint32_t need = (uint32_t)std::max<int32_t>(max_id, 0) + 2;
  bool grow = false;
  for (const MergeSlot& s : slot_) grow |= !s.dsum || need > s.cap;
  if (!grow) return;
  if (res_.in_flight() || run_count_ > 0) return;  // later: merge_chain grows on demand
  park();
  for (MergeSlot& s : slot_) ensure_slots(s, need);
  // the slots share keys_per_merge_: size them alike
  uint32_t cap = 0;
  for (const MergeSlot& s : slot_) cap = std::max(cap, s.cap);
  for (MergeSlot& s : slot_) ensure_slots(s, cap);
}

}  // namespace shred
