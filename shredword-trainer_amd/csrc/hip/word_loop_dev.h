// What the units of the indexed merge loop (host/word_loop.h) share: word_loop.hip (k_word_loop and
// its host protocol), word_index.hip (the word table and its index), word_select.hip (tiebreak=device
// outside the kernel).  The launch arguments, the run layout, the pool entry, the dstate words, the
// pair table's words and the device helpers of both the loop and the k_sel_* kernels.
#pragma once

#include <algorithm>

#include "hip_common.h"  // first: host/word_loop.h needs host/common.h, which it brings
#include "../host/word_loop.h"

namespace shred {

// (The types a WordLoop member's signature names have linkage: not in the anonymous namespace.)
struct WlCmd {
  // granules (seq | value << 32): op | slot << 8, a, b, X, then the words-of list of max(a, b)
  // when the host knows it (offset, count + 1; 0: look it up), one 64-B line
  u64 g[8];
};

struct WlSlotDev {
  DeltaRecord* recs;  // host-visible
  uint32_t* hdr;      // host-visible: [0] records, [1] flag, [2] listed words, [3] changed words,
                      //   [4..5] occurrences (u64), [6..7] device ticks command -> flag (u64),
                      //   [8..9] ticks command -> list known, [10..11] ticks command -> words merged,
                      //   [12] words whose runs were read, [13] 1: a filtered words-of list,
                      //   [14] run ints read (length + tokens), [15] run ints written back,
                      //   [16..18] stamps (10 ns ticks after the command, thread 0): pool entries
                      //   loaded, first run loaded, first word merged
  uint32_t rec_cap;
};

// A pool entry: the word and a 64-bit filter.  In the words-of list of id M (the words merge M
// changed) the filter holds a bit per (neighbour, side) of M in the word right after merge M:
// nbit(p, 0) for each left neighbour p (X when just produced), nbit(n, 1) for each original
// token n after the pair.  A merge never makes two older ids adjacent, so every adjacency
// (c, M) / (M, d) the word holds later it held right after merge M: a word holding the pair
// now has its bit.  Initial-index entries (exact lists) hold all ones.
struct WEnt {
  u64 e;    // run offset << 32 | groups << 28 | word id (groups: the 16-B groups of the word's run
            // capacity, at most kStripV: a word's run load issues only those, round 6)
  u64 sig;
};

// tiebreak=device (K5 as the selector, WordLoop::run_select): the loop picks its own merges from
// a pair table on the device.  Table: open addressing on the pair key, 16 B a slot -- the key,
// then a word holding the count (low 48 bits) and the slot's frontier position + 1 (high 16
// bits, 0: not in the frontier), so one atomicAdd on the word both counts and tells where the
// LDS copy is (pairs holding unk are never in it).  Frontier: the slots of every pair ranked at or above a threshold
// (count desc, key asc) plus stale ones; each merge takes the best live frontier entry, and pairs
// a merge creates above the threshold join it (only new pairs ever gain: every other count only
// falls).  An empty frontier sends the launch back to the host, which rebuilds it whole-chip.
struct SelParams {
  u64* tab;           // slot h: tab[2h] pair key (kEmpty64 = empty), tab[2h + 1] count | pos + 1 << 48
  u64 pmask;
  uint32_t* fr[2];    // frontier buffers (slots); st[kSelBuf] says which is current
  uint32_t fcap;
  uint32_t* st;       // see kSel* below
  const u64* thr;     // threshold (count, key): every pair ranked at or above it is in the frontier
  u64* out;           // per merge: key, count
  u64* log;           // the launch's pair-count changes (key, signed delta), applied to the table between launches
  u64 log_cap;        //   entries
  int32_t X0;         // id of merge 0 of this training
  uint32_t n_max;     // merges wanted
  u64 min_freq;
  uint32_t fill_max;  // inserts allowed before the table counts as full
  uint32_t probe;     // diagnostic (SHREDWORD_SEL_PROBE): 1 skips the table's HBM updates (timing only: wrong counts)
};

struct WlParams {
  int32_t* wtok;
  const u64* weight;
  WEnt* pool;
  u64 pool_cap;
  const u64* dkey;
  const u64* dval;
  u64 dir_mask;
  u64* lst;          // per id: words-of list, pool offset | count << 32
  uint32_t* lseq;    // per id: the command that made it (~0: none)
  uint32_t id_cap;
  u64* dsum;
  u64* dft;
  uint32_t* dlist;
  uint32_t* dstate;
  uint32_t cap;     // delta slots: ids in [0, cap) have slot id + 1, others (unk) slot 0
  int32_t unk;
  const WlCmd* ring;
  uint32_t* status;  // host-visible: [0] exit op
  uint32_t seq0;
  uint32_t idle_polls;
  uint32_t fin_max;  // K4 on the device: merges with at most this many records leave as ordered changes (0: off)
  uint32_t fin_min;  //   and at least this many (> 0: the small-merge path stays on; its merges leave raw)
  uint32_t prefetch;  // 1: the poller wave reads the next command while the records go out (exact mode)
  // 1: the merge's barriers drain every wave's stores (0: only with spills or K4).  With 0 the
  // word-run (wtok), pool and lst stores of a merge may still be in flight when its flag is raised;
  // that is sound only because nothing reads them before the next command's __syncthreads, which
  // drains them, and the host never reads them while the loop runs.  Any new reader of wtok, pool
  // or lst inside a merge's records phase, or on the host after a flag, needs drain = 1 (K4 sets
  // it: finalize reads the merged words).  tests/test_gpu_parity.py runs both modes.
  uint32_t drain;
  uint32_t fast;      // 1: merges listing <= kWlThreads words take the small-merge path (exact mode)
  WlSlotDev sl[WordLoop::kSlots];
  SelParams sel;  // k_word_loop<true> only
};

namespace {

constexpr int kWlThreads = 512;
constexpr int kStripV = 7;              // 16-B loads per word run: [length][weight lo, hi][25 tokens]
constexpr int kStrip = 4 * kStripV;     // ints per lane in the LDS strip
// A run's header: its live length, then the word's weight (u64, the count of the word) inline, so
// that the run's loads bring it and a scanned word costs no separate weight line (round 6: a third
// of the loop's HBM read requests were those lines)
constexpr uint32_t kRunHdr = 3;
constexpr uint32_t kStripTok = kStrip - kRunHdr;
// Runs are 16-B aligned with a capacity of whole 16-B groups.  (Round 6 measured 128-B aligned
// runs: one L2 line per run load, HBM reads of the loop -30%, but the table grew 2.5x, past what
// the MALL keeps, and the loop got slower; the groups a word needs ride in its pool entries
// instead, see WEnt.)
constexpr uint32_t kRunAlign = 4;  // ints
__host__ __device__ constexpr uint32_t run_cap(uint32_t len) {
  return (kRunHdr + len + kRunAlign - 1u) & ~(kRunAlign - 1u);
}
constexpr uint32_t kRunPad = 4 * kStripV + 4;  // ints past the last run (its 16-B loads may overrun)
// dstate words: [1] pool top, [3] error
constexpr int kStPoolTop = 1, kStError = 3;
// error codes (dstate[kStError], reported by the host)
constexpr uint32_t kErrPool = 1, kErrList = 2, kErrLookup = 4;
constexpr int kGroupShift = 28;
constexpr u64 kWordMask = (1ull << kGroupShift) - 1;
__host__ __device__ __forceinline__ uint32_t ent_groups(u64 e) { return (uint32_t)(e >> kGroupShift) & 0xFu; }

// st words
constexpr int kSelM = 0, kSelNF = 1, kSelBuf = 2, kSelStatus = 3, kSelIns = 4, kSelErr = 5, kSelStats = 6;
constexpr int kSelWords = kSelStats + 2 * 12 + 2;  // st: 6 words, then 12 u64 statistics, then the log's length (u64)
constexpr int kSelLogW = kSelStats + 2 * 12;
// exit status: merges done (target reached / below min_pair_freq), frontier to rebuild, table full
// (the in-kernel fill bound: one more merge's new pairs might not fit; the host grows the table)
constexpr uint32_t kSelDone = 1, kSelRebuild = 2, kSelFull = 3;
// The frontier lives in LDS for the whole launch: each entry's count follows the table's (the
// merge's records add to both; inf[slot] = LDS position + 1), so a select is an LDS scan.  A
// rebuild picks kSelK entries; merges append, and past kSelF - kSelSlack entries the dead ones
// (below the threshold, or merged) are compacted away in LDS.  When more than kSelF - kSelRoom
// stay live the launch ends for a rebuild (a compaction per merge would cost more).
constexpr uint32_t kSelF = 1536, kSelK = 768, kSelRoom = 384, kSelSlack = 96;
constexpr u64 kCntMask = (1ull << 48) - 1;  // the count in a slot's count word; pos + 1 above it
constexpr int kPosShift = 48;

__device__ __forceinline__ u64 pair_key(int32_t a, int32_t b) { return ((u64)(uint32_t)a << 32) | (uint32_t)b; }
__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u64 ld_agent64(const u64* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// tiebreak=device order: larger count first, then the smaller key
__device__ __forceinline__ bool sel_better(u64 c, u64 k, u64 c2, u64 k2) { return c > c2 || (c == c2 && k < k2); }
__device__ __forceinline__ bool sel_at_least(u64 c, u64 k, u64 tc, u64 tk) { return c > tc || (c == tc && k <= tk); }
// The table slot of pair key pk, inserted when absent (~0 when the table is past its probe bound).
// ins / err: counters of inserts and probe overflows (LDS in the loop, global in k_sel_insert).
__device__ __forceinline__ u64 sel_slot(const SelParams& q, u64 pk, uint32_t* ins, uint32_t* err) {
  u64 h = mix64(pk) & q.pmask;
#pragma unroll 1
  for (uint32_t probe = 0; probe < 4096u; ++probe) {
    const u64 cur = ld_agent64(q.tab + 2 * h);
    if (cur == pk) return h;
    if (cur == kEmpty64) {
      const u64 prev = atomicCAS(q.tab + 2 * h, kEmpty64, pk);
      if (prev == kEmpty64) {
        atomicAdd(ins, 1u);
        return h;
      }
      if (prev == pk) return h;
    }
    h = (h + 1) & q.pmask;
  }
  atomicMax(err, 1u);
  return ~0ull;
}
// (the loop's finalize and k_words_to_tiles)
__device__ __forceinline__ uint32_t wave_incl_add(uint32_t x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}

template <class T>
T* wl_alloc(size_t n, size_t* acc) {
  void* p = nullptr;
  HIP_OK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
  *acc += std::max<size_t>(n, 1) * sizeof(T);
  return static_cast<T*>(p);
}

}  // namespace

}  // namespace shred
