// MI355X (gfx950) tiebreak=device outside the kernel: the part of WordLoop (host/word_loop.h) that
// keeps the device pair table and its frontier for k_word_loop<true> (word_loop.hip) -- the
// table's initial pairs, growth and logged changes, the frontier's whole-chip rebuild -- and
// run_select, which drives the launches.  SelParams and the kSel* words: word_loop_dev.h.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "word_loop_dev.h"

namespace shred {

namespace {

// ---- tiebreak=device: the frontier's rebuild (whole chip) and the table's initial pairs
constexpr uint32_t kSelBuckets = 65536u + 48u * 256u;  // exact counts below 2^16, 256 per octave above
constexpr uint32_t kSelLds = 16384;                    // buckets counted in LDS per workgroup
__host__ __device__ __forceinline__ uint32_t sel_bucket(u64 c) {
  if (c < 65536) return (uint32_t)c;
  int lg = 63;
  while (!((c >> lg) & 1ull)) --lg;
  return 65536u + (uint32_t)(lg - 16) * 256u + (uint32_t)((c >> (lg - 8)) & 255u);
}
// the smallest count in bucket b
inline u64 sel_bucket_lo(uint32_t b) {
  if (b < 65536u) return b;
  const uint32_t lg = 16u + (b - 65536u) / 256u, mant = (b - 65536u) % 256u;
  return (u64)(256u + mant) << (lg - 8u);
}

__global__ void k_sel_hist(u64* tab, u64 n, u64 minf, uint32_t* hist) {
  __shared__ uint32_t h[kSelLds];
  for (uint32_t i = threadIdx.x; i < kSelLds; i += blockDim.x) h[i] = 0;
  __syncthreads();
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
    const u64 cv = tab[2 * i + 1], c = cv & kCntMask;
    if (cv >> kPosShift) tab[2 * i + 1] = c;  // the last launch's frontier positions are void now
    if (tab[2 * i] == kEmpty64 || c < minf) continue;
    const uint32_t b = sel_bucket(c);
    if (b < kSelLds) atomicAdd(&h[b], 1u);
    else atomicAdd(&hist[b], 1u);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < kSelLds; i += blockDim.x)
    if (h[i]) atomicAdd(&hist[i], h[i]);
}

__global__ void k_sel_collect(const u64* tab, u64 n, u64 minf, uint32_t bstar, uint32_t* out, uint32_t* nout,
                              u64 cap) {
  const int lane = threadIdx.x & 63;
  for (u64 i0 = blockIdx.x * (u64)blockDim.x; i0 < n; i0 += (u64)gridDim.x * blockDim.x) {
    const u64 i = i0 + threadIdx.x;
    bool take = false;
    if (i < n) {
      const u64 c = tab[2 * i + 1] & kCntMask;
      take = tab[2 * i] != kEmpty64 && c >= minf && sel_bucket(c) >= bstar;
    }
    const u64 bl = __ballot(take);
    if (!bl) continue;
    const int lead = __ffsll((long long)bl) - 1;
    uint32_t base = 0;
    if (lane == lead) base = atomicAdd(nout, (uint32_t)__popcll(bl));
    base = __shfl(base, lead, 64);
    const uint32_t pos = base + (uint32_t)__popcll(bl & ((1ull << lane) - 1ull));
    if (take && pos < cap) out[pos] = (uint32_t)i;
  }
}

__global__ void k_sel_gather(const uint32_t* slots, uint32_t n, const u64* tab, u64* key, u64* negc, uint32_t* idx) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    key[i] = tab[2 * (u64)slots[i]];
    negc[i] = ~(tab[2 * (u64)slots[i] + 1] & kCntMask);
    idx[i] = i;
  }
}

// idx: the sorted order; the first n of the collected slots in that order -> the frontier
__global__ void k_sel_pick(const uint32_t* slots, const uint32_t* idx, uint32_t n, uint32_t* fr) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    fr[i] = slots[idx ? idx[i] : i];
}

__global__ void k_sel_insert(const PairCount* pc, uint64_t n, SelParams q) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const u64 h = sel_slot(q, pair_key(pc[i].a, pc[i].b), q.st + kSelIns, q.st + kSelErr);
    if (h != ~0ull) q.tab[2 * h + 1] = pc[i].count & kCntMask;
  }
}

// The launch's logged changes into the table (whole chip, between launches): each a slot
// (inserted when new) and an add; the adds commute, so their order is free.
__global__ void k_sel_apply_log(const u64* log, u64 n, SelParams q) {
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
    const u64 h = sel_slot(q, log[2 * i], q.st + kSelIns, q.st + kSelErr);
    if (h != ~0ull) atomicAdd(q.tab + 2 * h + 1, log[2 * i + 1]);
  }
}

// An empty table: every key kEmpty64, every count word 0.
__global__ void k_sel_clear(u64* tab, u64 n) {
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
    tab[2 * i] = kEmpty64;
    tab[2 * i + 1] = 0;
  }
}

// The live pairs of a table (count > 0), for a bigger one.
__global__ void k_sel_export(const u64* tab, u64 cap, PairCount* out, uint32_t* n) {
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < cap; i += (u64)gridDim.x * blockDim.x) {
    const u64 k = tab[2 * i], c = tab[2 * i + 1] & kCntMask;
    if (k == kEmpty64 || c == 0) continue;
    const uint32_t j = atomicAdd(n, 1u);
    out[j] = PairCount{(int32_t)(uint32_t)(k >> 32), (int32_t)(uint32_t)k, c, 0};
  }
}

}  // namespace

void WordLoop::sel_free() {
  void* ptrs[] = {ptab_, fr_[0], fr_[1], sst_dev_, thr_, sout_, upd_, shist_, scol_};
  for (void* q : ptrs)
    if (q) HIP_OK(hipFree(q));
  ptab_ = thr_ = sout_ = nullptr;
  fr_[0] = fr_[1] = sst_dev_ = upd_ = shist_ = scol_ = nullptr;
  pcap_ = sout_cap_ = upd_cap_ = scol_cap_ = 0;
  fcap_ = 0;
}

// The frontier from the whole table: the kSelK best pairs by (count desc, key asc) among those
// >= min_freq (all of them when few), their slots flagged; the threshold = the last one taken
// (or, when every pair of the counts' top buckets was taken, the lowest count of those buckets).
bool WordLoop::sel_rebuild(uint64_t min_freq) {
  const double t0 = now_seconds();
  hipStream_t s = S(stream_);
  HIP_OK(hipMemsetAsync(shist_, 0, kSelBuckets * sizeof(uint32_t), s));
  k_sel_hist<<<1024, 512, 0, s>>>(ptab_, pcap_, min_freq, shist_);
  HIP_OK(hipGetLastError());
  std::vector<uint32_t> hist(kSelBuckets);
  HIP_OK(hipMemcpyAsync(hist.data(), shist_, kSelBuckets * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  uint64_t acc = 0;
  uint32_t bstar = kSelBuckets;
  for (uint32_t b = kSelBuckets; b-- > 0;) {
    if (!hist[b]) continue;
    acc += hist[b];
    bstar = b;
    if (acc >= kSelK) break;
  }
  uint32_t st[kSelStats] = {};
  HIP_OK(hipMemcpyAsync(st, sst_dev_, sizeof(st), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  u64 thr[2] = {~0ull, 0ull};
  uint32_t nf = 0;
  if (acc > 0) {
    if (acc > scol_cap_) {
      if (scol_) HIP_OK(hipFree(scol_));
      scol_cap_ = std::max<uint64_t>(2 * acc, 1 << 16);
      scol_ = wl_alloc<uint32_t>(scol_cap_ + 1, &bytes_);
    }
    uint32_t* ncol = scol_ + scol_cap_;
    HIP_OK(hipMemsetAsync(ncol, 0, sizeof(uint32_t), s));
    k_sel_collect<<<1024, 512, 0, s>>>(ptab_, pcap_, min_freq, bstar, scol_, ncol, scol_cap_);
    HIP_OK(hipGetLastError());
    uint32_t nc = 0;
    HIP_OK(hipMemcpyAsync(&nc, ncol, sizeof(nc), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (nc != acc) fatal("tiebreak=device: the frontier's collect disagrees with its histogram");
    if (nc <= kSelK) {  // every pair of the top buckets: the threshold is their lowest count
      nf = nc;
      k_sel_pick<<<64, 256, 0, s>>>(scol_, nullptr, nf, fr_[0]);
      HIP_OK(hipGetLastError());
      thr[0] = std::max<u64>(sel_bucket_lo(bstar), min_freq);
      thr[1] = ~0ull;
    } else {  // the top kSelK in (count desc, key asc) order: sort by key, then stably by count
      size_t acc2 = 0;
      u64* key = wl_alloc<u64>(nc, &acc2);
      u64* key2 = wl_alloc<u64>(nc, &acc2);
      u64* negc = wl_alloc<u64>(nc, &acc2);
      u64* negc2 = wl_alloc<u64>(nc, &acc2);
      uint32_t* idx = wl_alloc<uint32_t>(nc, &acc2);
      uint32_t* idx2 = wl_alloc<uint32_t>(nc, &acc2);
      k_sel_gather<<<256, 256, 0, s>>>(scol_, nc, ptab_, key, negc, idx);
      HIP_OK(hipGetLastError());
      size_t tb = 0, tb2 = 0;
      HIP_OK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, key, key2, idx, idx2, (int)nc, 0, 64, s));
      HIP_OK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb2, negc, negc2, idx, idx2, (int)nc, 0, 64, s));
      void* tmp = wl_alloc<uint8_t>(std::max(tb, tb2), &acc2);
      HIP_OK(hipcub::DeviceRadixSort::SortPairs(tmp, tb, key, key2, idx, idx2, (int)nc, 0, 64, s));
      // counts in key order, then a stable sort by ~count
      k_sel_gather<<<256, 256, 0, s>>>(scol_, nc, ptab_, key, negc, idx);  // key/negc of slot order
      HIP_OK(hipGetLastError());
      std::vector<uint32_t> order(nc);
      std::vector<u64> kc(nc), nn(nc);
      HIP_OK(hipMemcpyAsync(order.data(), idx2, nc * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      HIP_OK(hipMemcpyAsync(nn.data(), negc, nc * sizeof(u64), hipMemcpyDeviceToHost, s));
      HIP_OK(hipMemcpyAsync(kc.data(), key, nc * sizeof(u64), hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      // (host) ~count in key order, sorted stably on the device
      std::vector<u64> nk(nc);
      for (uint32_t i = 0; i < nc; ++i) nk[i] = nn[order[i]];
      HIP_OK(hipMemcpyAsync(negc, nk.data(), nc * sizeof(u64), hipMemcpyHostToDevice, s));
      HIP_OK(hipMemcpyAsync(idx, order.data(), nc * sizeof(uint32_t), hipMemcpyHostToDevice, s));
      HIP_OK(hipcub::DeviceRadixSort::SortPairs(tmp, tb2, negc, negc2, idx, idx2, (int)nc, 0, 64, s));
      nf = kSelK;
      k_sel_pick<<<64, 256, 0, s>>>(scol_, idx2, nf, fr_[0]);
      HIP_OK(hipGetLastError());
      uint32_t last = 0;
      HIP_OK(hipMemcpyAsync(&last, idx2 + (nf - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      thr[0] = ~nn[last];
      thr[1] = kc[last];
      for (void* q : {(void*)key, (void*)key2, (void*)negc, (void*)negc2, (void*)idx, (void*)idx2, tmp}) HIP_OK(hipFree(q));
    }
  }
  st[kSelNF] = nf;
  st[kSelBuf] = 0;
  st[kSelStatus] = 0;
  HIP_OK(hipMemcpyAsync(sst_dev_, st, sizeof(st), hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(thr_, thr, sizeof(thr), hipMemcpyHostToDevice, s));
  HIP_OK(hipStreamSynchronize(s));
  sst_.rebuilds += 1;
  sst_.rebuild_ms += 1e3 * (now_seconds() - t0);
  sst_.frontier_max = std::max<uint64_t>(sst_.frontier_max, nf);
  return nf > 0;
}

int WordLoop::run_select(const std::vector<PairCount>& pairs, int32_t X0, uint32_t n_max, uint64_t min_freq,
                         std::vector<SelectedMerge>* out) {
  out->clear();
  if (!ready_ || !posted_.empty()) return -1;
  HIP_OK(hipSetDevice(ordinal_));
  stop();
  if (n_max == 0) return 0;
  reserve(X0 + (int32_t)n_max);
  hipStream_t s = S(stream_);
  // the table: room for the initial pairs and ~64 new pairs a merge (C3 makes 62), 1.5x over;
  // past 3/4 full it is grown 4x between launches.  Round 5, with the table updated from a log
  // per launch: a smaller table is faster -- its rebuild histogram reads fewer slots and its
  // updates stay in L2 / MALL (C3 A/B on one box: 33.5 M slots 57.4-57.5 k merges/s, 8.4 M
  // 59.8-60.1 k, 4.2 M 60.3-60.4 k; profiles/r05_c3_tiebreak_table_ab.txt)
  uint64_t want = 1 << 16;
  while (want < 3 * ((uint64_t)pairs.size() + 64ull * n_max) / 2) want <<= 1;
  if (const char* e = std::getenv("SHREDWORD_SELECT_TABLE_SLOTS")) {  // tests: a table that must grow
    const uint64_t t = std::strtoull(e, nullptr, 10);
    if (t >= 1024) {  // never below what the initial pairs need (they must all fit)
      want = 1024;
      while (want < t || want < 2 * (uint64_t)pairs.size()) want <<= 1;
    }
  }
  if (!fr_[0]) {
    fcap_ = 16384;
    fr_[0] = wl_alloc<uint32_t>(fcap_, &bytes_);
    fr_[1] = wl_alloc<uint32_t>(fcap_, &bytes_);
    sst_dev_ = wl_alloc<uint32_t>(kSelWords, &bytes_);
    thr_ = wl_alloc<u64>(2, &bytes_);
    shist_ = wl_alloc<uint32_t>(kSelBuckets, &bytes_);
  }
  if (2ull * n_max > sout_cap_) {
    if (sout_) HIP_OK(hipFree(sout_));
    sout_cap_ = 2ull * n_max;
    sout_ = wl_alloc<u64>(sout_cap_, &bytes_);
  }
  // the table-change log: many merges' records between two applications (a launch ends early
  // when one more merge might not fit)
  const uint64_t need_log = std::max<uint64_t>(1ull << 22, 16ull * ((uint64_t)cap_ + 2));
  if (need_log > upd_cap_) {
    if (upd_) HIP_OK(hipFree(upd_));
    upd_cap_ = need_log;
    upd_ = wl_alloc<uint32_t>(4 * upd_cap_, &bytes_);  // (key, delta) u64 pairs
  }
  HIP_OK(hipMemsetAsync(sst_dev_, 0, kSelWords * sizeof(uint32_t), s));
  SelParams q{};
  auto table_from = [&](const PairCount* dp, size_t np, uint64_t cap) {  // a fresh table holding dp
    if (cap != pcap_) {
      if (ptab_) HIP_OK(hipFree(ptab_));
      pcap_ = cap;
      ptab_ = wl_alloc<u64>(2 * pcap_, &bytes_);
    }
    k_sel_clear<<<1024, 256, 0, s>>>(ptab_, pcap_);
    HIP_OK(hipGetLastError());
    q.tab = ptab_;
    q.pmask = pcap_ - 1;
    q.fr[0] = fr_[0];
    q.fr[1] = fr_[1];
    q.fcap = fcap_;
    q.st = sst_dev_;
    q.thr = thr_;
    q.out = sout_;
    q.log = reinterpret_cast<u64*>(upd_);
    q.log_cap = upd_cap_;
    q.X0 = X0;
    q.n_max = n_max;
    q.min_freq = min_freq;
    q.fill_max = (uint32_t)std::min<uint64_t>(3 * pcap_ / 4, 0xFFFFFFF0ull);
    if (const char* e = std::getenv("SHREDWORD_SEL_PROBE")) q.probe = (uint32_t)std::atoi(e);
    uint32_t zero = 0;
    HIP_OK(hipMemcpyAsync(sst_dev_ + kSelIns, &zero, sizeof(zero), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(sst_dev_ + kSelErr, &zero, sizeof(zero), hipMemcpyHostToDevice, s));
    if (np) {
      k_sel_insert<<<512, 256, 0, s>>>(dp, np, q);
      HIP_OK(hipGetLastError());
    }
    HIP_OK(hipStreamSynchronize(s));
    uint32_t err = 0;  // a pair that found no slot within the probe bound would be a lost count
    HIP_OK(hipMemcpy(&err, sst_dev_ + kSelErr, sizeof(err), hipMemcpyDeviceToHost));
    if (err) fatal("tiebreak=device: the pair table's initial pairs overran the probe bound");
  };
  {
    size_t acc = 0;
    PairCount* dp = pairs.empty() ? nullptr : wl_alloc<PairCount>(pairs.size(), &acc);
    if (dp) HIP_OK(hipMemcpyAsync(dp, pairs.data(), pairs.size() * sizeof(PairCount), hipMemcpyHostToDevice, s));
    table_from(dp, pairs.size(), want);
    if (dp) HIP_OK(hipFree(dp));
  }
  sst_.table_slots = pcap_;
  uint32_t m = 0;
  if (sel_rebuild(min_freq)) {
    WlParams p{};
    fill_params(&p);  // fast: small merges through the small-merge body (then the pair-table tail)
    p.sel = q;
    dirty_ = true;
    int stalls = 0;
    for (;;) {
      p.seq0 = seq_ + 1;
      launch_kernel(true, p);
      HIP_OK(hipStreamSynchronize(s));
      float ms = 0;
      HIP_OK(hipEventElapsedTime(&ms, (hipEvent_t)ev_[0], (hipEvent_t)ev_[1]));
      sst_.kernel_ms += ms;
      sst_.launches += 1;
      uint32_t st[kSelWords];
      HIP_OK(hipMemcpy(st, sst_dev_, sizeof(st), hipMemcpyDeviceToHost));
      uint32_t ds[8];
      HIP_OK(hipMemcpy(ds, dstate_, sizeof(ds), hipMemcpyDeviceToHost));
      if (ds[kStError]) {
        std::fprintf(stderr, "[ERROR]\t k_word_loop<true>: error code %u\n", ds[kStError]);
        fatal("tiebreak=device merge loop failed");
      }
      if (sel_report_)
        std::fprintf(stderr, "[SELECT] launch %llu: merges %u..%u in %.3f ms (%.2f us/merge), status %u, table %u, "
                     "%u LDS compactions\n", (unsigned long long)sst_.launches, m, st[kSelM], ms,
                     st[kSelM] > m ? 1e3 * ms / (st[kSelM] - m) : 0.0, st[kSelStatus], st[kSelIns], st[kSelBuf]);
      const bool progressed = st[kSelM] != m;
      m = st[kSelM];
      // the launch's logged changes into the table
      const u64 logn = *reinterpret_cast<const u64*>(st + kSelLogW);
      if (logn) {
        const double tl = now_seconds();
        k_sel_apply_log<<<1024, 256, 0, s>>>(reinterpret_cast<const u64*>(upd_), logn, q);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemsetAsync(sst_dev_ + kSelLogW, 0, sizeof(u64), s));
        HIP_OK(hipMemcpyAsync(st + kSelIns, sst_dev_ + kSelIns, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        sst_.log_ms += 1e3 * (now_seconds() - tl);
        sst_.log_entries += logn;
      }
      // a change whose pair found no table slot within the probe bound would be lost: the table
      // would no longer be the corpus's count, so there is nothing exact to grow from
      if (st[kSelErr]) fatal("tiebreak=device: a pair-table update overran the probe bound");
      const uint32_t status = st[kSelStatus];
      if (status == kSelDone) break;
      // a rebuild that merged nothing is not a full table: only kSelFull and the
      // inserts past the bound grow it.  Right after a rebuild the frontier holds entries at or
      // above the threshold, so two such launches in a row would be a loop that cannot progress.
      if (status == kSelRebuild && !progressed) {
        if (++stalls > 1) fatal("tiebreak=device: two launches in a row ended for a rebuild without a merge");
      } else {
        stalls = 0;
      }
      // the table past 3/4 full, or without room for one more merge's new pairs: 4x, live pairs moved
      if (st[kSelIns] > q.fill_max || status == kSelFull) {
        size_t acc = 0;
        PairCount* dp = wl_alloc<PairCount>(pcap_, &acc);
        uint32_t* dn = wl_alloc<uint32_t>(1, &acc);
        HIP_OK(hipMemsetAsync(dn, 0, sizeof(uint32_t), s));
        k_sel_export<<<1024, 256, 0, s>>>(ptab_, pcap_, dp, dn);
        HIP_OK(hipGetLastError());
        uint32_t np = 0;
        HIP_OK(hipMemcpyAsync(&np, dn, sizeof(np), hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        // the exported pairs must survive the old table's release: keep them in their own buffer
        const uint64_t grown = 4 * pcap_;
        u64* old = ptab_;
        ptab_ = nullptr;
        pcap_ = 0;
        table_from(dp, np, grown);
        HIP_OK(hipFree(old));
        HIP_OK(hipFree(dp));
        HIP_OK(hipFree(dn));
        ++sst_.grows;
        p.sel = q;
        if (!sel_rebuild(min_freq)) break;
        continue;
      }
      if (status != kSelRebuild) fatal("tiebreak=device: the merge loop ended without a status");
      if (!sel_rebuild(min_freq)) break;
    }
    uint32_t st[kSelWords];
    HIP_OK(hipMemcpy(st, sst_dev_, sizeof(st), hipMemcpyDeviceToHost));
    const u64* t64 = reinterpret_cast<const u64*>(st + kSelStats);
    sst_.select_us += 1e-2 * (double)t64[0];
    sst_.merge_us += 1e-2 * (double)t64[1];
    sst_.listed += t64[2];
    sst_.changed += t64[3];
    sst_.occurrences += t64[4];
    sst_.new_pairs += t64[5];
    sst_.table_us += 1e-2 * (double)t64[6];
    sst_.rec_us += 1e-2 * (double)t64[8];
    sst_.append_us += 1e-2 * (double)t64[9];
    sst_.tail_us += 1e-2 * (double)t64[10];
    if (sel_report_ && m)
      std::fprintf(stderr, "[SELECT] %u merges: device select %.2f us, merge %.2f us (of it table + frontier %.2f us: "
                   "records %.2f, appends %.2f, tail %.2f) per merge; %llu LDS compactions, %llu listed / %llu changed "
                   "words\n", m, 1e-2 * (double)t64[0] / m, 1e-2 * (double)t64[1] / m, 1e-2 * (double)t64[6] / m,
                   1e-2 * (double)t64[8] / m, 1e-2 * (double)t64[9] / m, 1e-2 * (double)t64[10] / m, (unsigned long long)t64[7],
                   (unsigned long long)t64[2], (unsigned long long)t64[3]);
    sst_.table_pairs = st[kSelIns];
  }
  sst_.table_slots = pcap_;
  sst_.merges += m;
  std::vector<u64> o(2 * (size_t)m);
  if (m) HIP_OK(hipMemcpy(o.data(), sout_, o.size() * sizeof(u64), hipMemcpyDeviceToHost));
  out->resize(m);
  for (uint32_t i = 0; i < m; ++i)
    (*out)[i] = SelectedMerge{(int32_t)(uint32_t)(o[2 * i] >> 32), (int32_t)(uint32_t)o[2 * i], o[2 * i + 1]};
  return (int)m;
}

}  // namespace shred
