// The whole-chip resident merge loop (types layout, one GPU): K2+K3 as ONE persistent launch of
// k_resident with the word table held in LDS (hip/resident_loop.hip has the kernel and protocol).
//
// ResidentLoop is the mechanism: the plan (which workgroup holds which tiles in LDS), the launch, the
// command ring and the slots' flags, the posted queue, and the loop's own diagnostics.  Device
// (device.h) is the policy: which path takes a merge, when the delta tables grow, what an abort
// means for the stream, and what a collected merge does to the tile index and the statistics.
// The loop shares with the launch path the merge slots (Device owns them; the loop reads their
// tables and writes their pinned flags) and the one command / launch sequence counter.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "selector.h"
#include "tiles.h"

namespace shred {

// Device tables and host-visible buffers of a merge launch (k_merge) or a resident merge.
struct MergeSlot {
  uint32_t cap = 0;  // neighbour slots: id+1 for ids < cap, slot 0 for unk outside
  uint64_t* dsum = nullptr;  // kChainMax x 4 (cap + 1) keys + 2 stats words
  uint64_t* dft = nullptr;
  uint32_t* dlist = nullptr;
  uint32_t* dcount = nullptr;  // [0] touched-slot count, [1..9] completion tickets, [10] matched tiles
  DeltaRecord* host_recs = nullptr;  // pinned, device-visible
  void* dev_recs = nullptr;
  uint32_t* host_count = nullptr;    // pinned: [0] records (| need-collect), [1] flag, [2] matched tiles,
  void* dev_count = nullptr;         //         [3] k_collect offset, bytes 16..31: occurrences, tokens
  uint32_t* dmlist = nullptr;        // device: matched tiles beyond a workgroup's LDS list / multi-GPU
  uint32_t* rhdr = nullptr;          // device: per-workgroup regions of the fused completion
  uint64_t* rrec = nullptr;
  uint32_t* rtile = nullptr;
  uint32_t* host_mlist = nullptr;    // pinned: matched tiles (tile | chain index << 27)
  void* dev_mlist = nullptr;
  // multi-GPU: this rank's bucket (32-byte header, then records; records past the bucket
  // stay behind it for the overflow round), the gathered buckets, and their pinned copy
  uint8_t* xsend = nullptr;
  uint8_t* xrecv = nullptr;
  DeltaRecord* host_xrecs = nullptr;  // pinned: world x bucket records, concatenated
  void* dev_xrecs = nullptr;
  uint32_t* host_xhdr = nullptr;      // pinned: per rank [records | need-collect, k_collect offset]
  void* dev_xhdr = nullptr;
  std::vector<DeltaRecord> xall;      // all ranks' records when a bucket overflowed
  uint32_t grid = 0;
  uint32_t n_iter = 0;  // candidate tiles of the launch
  bool launched = false;
  uint32_t seq = 0;
};

constexpr uint32_t kAllTiles = 0xFFFFFFFFu;  // hcount[2]: merge X matched (nearly) every tile

class ResidentLoop {
 public:
  static constexpr int kSlots = 4;  // merges in flight: the current one and the guesses behind it
  struct Post {  // a merge posted to the loop and not yet collected
    int32_t X, a, b;
    uint32_t seq;
    int slot;
    uint32_t nparts;
    double t_post;
  };
  struct Collected {  // a merge seen complete; the pointers are the slot's pinned buffers
    const DeltaRecord* recs;
    size_t n;
    const uint32_t* tiles;  // the gatherer's bitmap of matched tiles, n_tiles bits (kAllTiles: no bitmap)
    uint32_t n_tiles;
    const uint64_t* hs;  // [0] occurrences, [1] tokens of the matched tiles, [2] ticks dispatch -> flag, [3..8] stamps
    uint32_t nparts;
    double t_post, t_wait, t_flag;  // host clock: posted, collect() entered, flag seen
  };

  // slots: the owner's kSlots merge slots.  seq: the counter the launch path shares (a launch takes
  // commands from seq + 1).  keys_per_merge: the delta keys one merge owns in the slots' tables.
  ResidentLoop(int ordinal, const MergeSlot* slots, uint32_t& seq, const uint32_t& keys_per_merge);
  ~ResidentLoop();
  ResidentLoop(const ResidentLoop&) = delete;

  // Partitions the uploaded types table (ts; tok .. weight: its device arrays) over the chip's LDS
  // and uploads the plan; ok() says whether it fits.  Nothing may be running.
  void plan(const TiledStream& ts, int32_t* tok, const uint64_t* tile_off, uint32_t* tile_len, const uint64_t* weight,
            int cu_count, size_t* bytes);
  void free_plan();
  bool ok() const { return ok_; }
  void disable() { ok_ = false; }  // until the next plan()
  bool tokens_in_lds() const { return lds_tok_; }  // else in HBM, LDS holds weights + signatures
  bool stamps() const { return stamps_ != nullptr; }
  void set_stream(void* s) { stream_ = s; }  // later launches go to this stream

  bool running() const { return running_; }  // a k_resident launch is live
  bool aborted() const;  // the live launch gave up: not every workgroup became resident
  size_t in_flight() const { return posted_.size(); }
  // A slot for the next merge (may wait for an undone guess to complete); -1: the launch aborted.
  int pick_slot();
  // Posts (a, b) -> X to `slot` (the launch starts on the first post).  Its participants own the
  // pair's candidate tiles by `index`, or are every worker (nullptr, or no candidates); returns
  // the tiles they hold.
  uint32_t post_merge(int slot, int32_t a, int32_t b, int32_t X, const TileIndex* index);
  // Waits for the oldest posted merge, which must be X.  False: the launch aborted, nothing ran.
  bool collect(int32_t X, Collected* c);
  // Undoes every posted merge with id >= X, newest first (queued; nothing waits); their count.
  int rollback(int32_t X);
  // After aborted(): forgets the launch and hands back the merges in flight, oldest first.
  std::vector<Post> abandon();
  // Ends the launch (nothing in flight; the tiles are back in HBM): its collected merges, *ms its duration.
  uint64_t stop(double* ms);

  uint64_t launches() const { return launches_; }
  double ms() const { return ms_; }  // Σ k_resident launch durations (HIP events)
  // mean dispatch -> host flag time of a merge (device clock), us
  double latency_us() const { return lat_n_ ? lat_us_ / (double)lat_n_ : 0.0; }
  void clear_stats() {
    launches_ = lat_n_ = 0;
    ms_ = lat_us_ = 0;
  }

 private:
  void start();
  uint32_t post(uint32_t op, int32_t a, int32_t b, int32_t X, int slot, const TileIndex* index = nullptr);
  bool wait(const MergeSlot& sl, int32_t X);  // false: the launch aborted
  [[noreturn]] void dump(const char* why);

  int ordinal_;
  const MergeSlot* slot_;
  uint32_t& seq_;  // launch / command sequence number echoed by the device flag
  const uint32_t& keys_per_merge_;
  void* stream_ = nullptr;
  int32_t* tok_ = nullptr;  // the planned table (the owner's device arrays)
  const uint64_t* tile_off_ = nullptr;
  uint32_t* tile_len_ = nullptr;
  const uint64_t* weight_ = nullptr;
  size_t ntiles_ = 0;
  bool ok_ = false;  // the uploaded table fits (plan)
  bool running_ = false, lds_tok_ = true;
  std::vector<Post> posted_;  // oldest first (a merge and the guesses behind it)
  std::vector<uint32_t> post_parts_[kSlots];  // participants of the posted merges, by slot
  int32_t abandoned_[kSlots] = {-1, -1, -1, -1};  // by slot: an undone guess not yet completed
  int next_slot_ = 0;
  uint32_t grid_ = 0, tok_words_ = 0, w_words_ = 0;
  uint32_t sig_words_ = 0;   // LDS signature words per tile in this plan
  bool w_global_ = false;    // the plan reads word weights from HBM
  size_t shm_ = 0;
  uint32_t *wg_tiles_ = nullptr, *wg_rank_ = nullptr;  // device: grid + 1 each
  uint32_t* tile_lofs_ = nullptr;  // device: per tile
  std::vector<uint32_t> wg_ntiles_;
  std::vector<uint32_t> all_;      // every worker workgroup (2 .. grid-1)
  std::vector<uint32_t> wg_first_; // grid + 1: first tile of each workgroup
  void *mbox_ = nullptr, *mbox_dev_ = nullptr;  // pinned host ResMbox (command ring)
  uint32_t* cmd_ = nullptr;        // device command ring
  uint64_t* q_ = nullptr;          // device per-workgroup queues
  uint32_t* arrive_ = nullptr;     // device: workgroups that started
  uint32_t arrive_polls_ = 20000;  // the leader's co-residency bound (~20 ms; env SHREDWORD_RESIDENT_ARRIVE_POLLS)
  uint32_t region_keys_ = 32;      // participants with more delta keys add them to the global tables
                                   // (env SHREDWORD_RESIDENT_REGION_KEYS)
  uint32_t* dbg_ = nullptr;        // device: per-workgroup progress (SHREDWORD_RESIDENT_DEBUG)
  uint64_t* stamps_ = nullptr;     // device: per-participant phase stamps (SHREDWORD_RESIDENT_STAMPS)
  double ph_[4] = {}, ph_flag_ = 0, ph_raw_ = 0;  // diagnostic: the gatherer's phases, flag time, raw records
  uint64_t ph_n_ = 0;
  double host_wait_ = 0, parts_sum_ = 0, post_flag_us_ = 0;
  uint32_t* status_ = nullptr;     // pinned host status
  void* status_dev_ = nullptr;
  void* ev_[2] = {};
  uint64_t launches_ = 0;
  uint64_t merges_ = 0;            // merges collected in the current launch
  double ms_ = 0, lat_us_ = 0;     // Σ launch durations; Σ per-merge dispatch -> flag times (device clock)
  uint64_t lat_n_ = 0;
};

}  // namespace shred
