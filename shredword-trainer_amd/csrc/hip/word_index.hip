// MI355X (gfx950) word table of the indexed merge loop (word_loop.hip) and its index: the part of
// WordLoop (host/word_loop.h) that uploads, loads and resets the words, indexes their pairs and
// writes them back to the tile stream.  hipCUB sorts and scans, once per load or reset, never per merge.
//   k_wl_pair_counts / k_wl_emit_pairs   every adjacent non-unk pair of every word -> (key, word)
//   k_wl_mark / k_wl_scatter / k_wl_counts / k_wl_dir_init   sorted runs -> pool + directory
//   k_words_to_tiles / k_tiles_to_words  the word table into the tile stream (headers + tokens), and back
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <functional>
#include <thread>
#include <vector>

#include "word_loop_dev.h"

namespace shred {

namespace {

// Initial index, compact (round 6: the sort no longer spans the runs' padding): word w's
// adjacent pairs go to entries base[w] .. base[w] + L - 2 (base: exclusive sum of the words' pair
// counts, k_wl_pair_counts); pairs holding unk emit EMPTY.
__global__ void k_wl_pair_counts(const int32_t* wtok, const uint32_t* woff, uint32_t W, uint32_t* cnt) {
  for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w <= W; w += gridDim.x * blockDim.x) {
    const uint32_t L = w < W ? (uint32_t)wtok[woff[w]] : 0u;
    cnt[w] = L >= 2 ? L - 1 : 0u;
  }
}
__global__ void k_wl_emit_pairs(const int32_t* wtok, const uint32_t* woff, const uint32_t* base, uint32_t W,
                                int32_t unk, u64* key, uint32_t* val) {
  for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < W; w += gridDim.x * blockDim.x) {
    const uint32_t o = woff[w], b = base[w], np = base[w + 1] - b;
    const int32_t* t = wtok + o + kRunHdr;
    for (uint32_t j = 0; j < np; ++j) {
      const int32_t x = t[j], y = t[j + 1];
      key[b + j] = (x != unk && y != unk) ? pair_key(x, y) : kEmpty64;
      val[b + j] = w;
    }
  }
}

// Sorted (key, word) runs: keep the first of equal (key, word) entries; mark the first entry of
// each key.  Word ids are ascending inside a key (stable sort of entries emitted in word order).
__global__ void k_wl_mark(const u64* key, const uint32_t* val, uint64_t n, uint32_t* keep, uint32_t* head) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const u64 k = key[i];
    const bool valid = k != kEmpty64;
    const bool first_key = valid && (i == 0 || key[i - 1] != k);
    keep[i] = valid && (first_key || val[i - 1] != val[i]);
    head[i] = first_key;
  }
}

__global__ void k_wl_scatter(const u64* key, const uint32_t* val, uint64_t n, const uint32_t* keep,
                             const uint32_t* pos, const uint32_t* head, const uint32_t* kidx, const uint32_t* woff,
                             WEnt* pool, u64* ikey, u64* ival) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    if (keep[i]) {
      WEnt ent;
      const uint32_t w = val[i], cap4 = (woff[w + 1] - woff[w]) >> 2;  // the run's 16-B groups
      ent.e = ((u64)woff[w] << 32) | ((u64)min(cap4, (uint32_t)kStripV) << kGroupShift) | w;
      ent.sig = ~0ull;  // an exact list: no filter
      pool[pos[i]] = ent;
    }
    if (head[i]) {
      ikey[kidx[i]] = key[i];
      ival[kidx[i]] = pos[i];  // offset; the count is filled in by k_wl_counts
    }
  }
}

__global__ void k_wl_counts(u64* ival, uint64_t nk, uint64_t total) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nk; i += (uint64_t)gridDim.x * blockDim.x) {
    const u64 o = ival[i] & 0xFFFFFFFFull;
    const u64 e = i + 1 < nk ? (ival[i + 1] & 0xFFFFFFFFull) : total;
    ival[i] = o | ((e - o) << 32);
  }
}

// The initial directory (after a memset of the keys to EMPTY): no key repeats.
__global__ void k_wl_dir_init(const u64* ikey, const u64* ival, uint64_t nk, u64* dkey, u64* dval, u64 mask) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nk; i += (uint64_t)gridDim.x * blockDim.x) {
    const u64 key = ikey[i];
    u64 h = mix64(key) & mask;
    for (;;) {
      const u64 prev = atomicCAS(&dkey[h], kEmpty64, key);
      if (prev == kEmpty64) {
        dval[h] = ival[i];
        break;
      }
      h = (h + 1) & mask;
    }
  }
}

// Each run's header gets its word's weight (ints 1-2), after a host upload of the runs.
__global__ void k_wl_set_weights(int32_t* wtok, const uint32_t* woff, uint32_t W, const u64* weight) {
  for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < W; w += gridDim.x * blockDim.x) {
    const u64 c = weight[w];
    wtok[woff[w] + 1] = (int32_t)(uint32_t)c;
    wtok[woff[w] + 2] = (int32_t)(uint32_t)(c >> 32);
  }
}

// Words -> tiles: a wave per tile writes [header][tokens] for its words in rank order and the
// tile's live length; the old tail up to the previous length becomes padding.
__global__ void k_words_to_tiles(const int32_t* wtok, const uint32_t* woff, const uint32_t* tile_first,
                                 const uint32_t* tile_nw, uint32_t ntiles, int32_t* tok, const uint64_t* tile_off,
                                 uint32_t* tile_len) {
  const int lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (blockDim.x / 64);
  for (uint32_t t = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); t < ntiles; t += waves) {
    int32_t* dst = tok + tile_off[t];
    const uint32_t f = tile_first[t], nw = tile_nw[t];
    uint32_t base = 0;
    for (uint32_t q = 0; q < nw; q += 64) {
      const uint32_t w = f + q + (uint32_t)lane;
      const bool on = q + (uint32_t)lane < nw;
      const int32_t* s = on ? wtok + woff[w] : wtok;
      const uint32_t len = on ? (uint32_t)s[0] : 0u;
      const uint32_t need = on ? len + 1u : 0u;
      const uint32_t incl = wave_incl_add(need);
      if (on) {
        int32_t* d = dst + base + incl - need;
        d[0] = (int32_t)((uint32_t)kHeaderBase + w);
        for (uint32_t j = 0; j < len; ++j) d[1 + j] = s[kRunHdr + j];
      }
      base += __shfl(incl, 63, 64);
    }
    const uint32_t old = tile_len[t];
    for (uint32_t i = base + (uint32_t)lane; i < old; i += 64) dst[i] = INT32_MIN;
    if (lane == 0) tile_len[t] = base;
  }
}

// Tiles -> words (inverse of k_words_to_tiles): a thread per tile walks its entries; each word's
// tokens go to its run after the live length.
__global__ void k_tiles_to_words(const int32_t* tok, const uint64_t* tile_off, const uint32_t* tile_len,
                                 uint32_t ntiles, const uint32_t* woff, int32_t* wtok) {
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < ntiles; t += gridDim.x * blockDim.x) {
    const int32_t* src = tok + tile_off[t];
    const uint32_t n = tile_len[t];
    int32_t* run = nullptr;
    uint32_t len = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const int32_t v = src[i];
      if (v < kHeaderLimit) {
        if (run) run[0] = (int32_t)len;
        const uint32_t w = (uint32_t)(v - kHeaderBase);
        run = wtok + woff[w];
        len = 0;
      } else if (run) {
        run[kRunHdr + len++] = v;
      }
    }
    if (run) run[0] = (int32_t)len;
  }
}

}  // namespace

bool WordLoop::upload(const TiledStream& ts, const uint64_t* d_weight) {
  HIP_OK(hipSetDevice(ordinal_));
  if (running_) stop();
  free_all();
  // the words of the tile stream in rank order (types layout: one entry per distinct word), each
  // as a 16-B aligned run [length][tokens] of round_up(1 + length, 4) ints.  Threads over tile
  // ranges: a sizing pass (words and ints per tile, every header's rank checked against its
  // position), a prefix over the tiles, then each range fills its part of the runs.
  const size_t T = ts.num_tiles();
  const int P = (int)std::max<size_t>(1, std::min<size_t>({16, std::max(1u, std::thread::hardware_concurrency()),
                                                          T / 64 + 1}));
  auto par = [&](const std::function<void(int)>& f) {
    if (P == 1) return f(0);
    std::vector<std::thread> pool;
    for (int k = 0; k < P; ++k) pool.emplace_back(f, k);
    for (auto& th : pool) th.join();
  };
  auto range = [&](int k, size_t* t0, size_t* t1) {
    *t0 = T * (size_t)k / (size_t)P;
    *t1 = T * (size_t)(k + 1) / (size_t)P;
  };
  std::vector<uint32_t> tnw(T, 0), tfirst(T, 0);
  std::vector<uint64_t> tints(T + 1, 0), ttok(T, 0);
  std::vector<int32_t> tr0(T, -1);  // the rank of the tile's first word (-1: none)
  std::vector<char> bad((size_t)P, 0);
  par([&](int k) {
    size_t t0, t1;
    range(k, &t0, &t1);
    for (size_t t = t0; t < t1 && !bad[(size_t)k]; ++t) {
      const int32_t* p = ts.tok.data() + ts.off[t];
      uint32_t nw = 0, wl = 0;
      uint64_t ints = 0, ntk = 0;
      for (uint32_t i = 0; i < ts.len[t]; ++i) {
        if (p[i] < kHeaderLimit) {
          const int32_t r = (int32_t)(uint32_t)(p[i] - kHeaderBase);
          if (nw == 0) tr0[t] = r;
          else if (r != tr0[t] + (int32_t)nw) bad[(size_t)k] = 1;  // ranks not consecutive
          if (nw) ints += run_cap(wl);
          ++nw;
          wl = 0;
        } else {
          if (nw == 0) bad[(size_t)k] = 1;  // tokens before any header
          ++wl;
          ++ntk;
        }
      }
      if (nw) ints += run_cap(wl);
      tnw[t] = nw;
      tints[t] = ints;
      ttok[t] = ntk;
    }
  });
  for (char b : bad)
    if (b) return false;  // not the whole table in rank order: not for this loop
  uint64_t words = 0, ints = 0, ntok = 0;
  for (size_t t = 0; t < T; ++t) {
    if (tnw[t] && tr0[t] != (int32_t)words) return false;
    tfirst[t] = (uint32_t)words;
    const uint64_t n = tints[t];
    tints[t] = ints;
    words += tnw[t];
    ints += n;
    ntok += ttok[t];
  }
  tints[T] = ints;
  if (ints >= 0xFFFFFF00ull) return false;  // offsets are 32-bit
  std::vector<uint32_t> woff(words + 1);
  std::vector<int32_t> wtok(ints + kRunPad, 0);
  par([&](int k) {
    size_t t0, t1;
    range(k, &t0, &t1);
    for (size_t t = t0; t < t1; ++t) {
      const int32_t* p = ts.tok.data() + ts.off[t];
      uint64_t o = tints[t], w = tfirst[t];
      int32_t* len = nullptr;
      for (uint32_t i = 0; i < ts.len[t]; ++i) {
        if (p[i] < kHeaderLimit) {
          if (len) o = (o + kRunAlign - 1u) & ~(uint64_t)(kRunAlign - 1u);
          woff[w++] = (uint32_t)o;
          len = &wtok[o];
          o += kRunHdr;  // (the weight ints are filled on the device: k_wl_set_weights)
        } else {
          wtok[o++] = p[i];
          ++*len;
        }
      }
    }
  });
  woff[words] = (uint32_t)ints;
  nwords_ = (uint32_t)(woff.size() - 1);
  nint_ = ints;
  ntok_ = ntok;
  ntiles_ = (uint32_t)ts.num_tiles();
  if (nwords_ == 0 || nint_ >= (1ull << 31)) return false;  // hipcub sizes are int
  if (nwords_ > kWordMask) return false;  // word ids share the pool entry with the run's groups
  // the pool (below) is addressed with 32-bit offsets (pool top, lst_, directory values)
  if (3 * ntok_ + 4096 >= (1ull << 32)) return false;
  for (uint32_t w = 0; w < nwords_; ++w)
    if (wtok[woff[w]] == 0) return false;  // words are never empty (strtok)
  weight_ = reinterpret_cast<const unsigned long long*>(d_weight);
  woff_h_ = woff;
  wtok_ = wl_alloc<int32_t>(nint_ + kRunPad, &bytes_);
  wtok0_ = wl_alloc<int32_t>(nint_ + kRunPad, &bytes_);
  woff_ = wl_alloc<uint32_t>(nwords_ + 1, &bytes_);
  tile_first_ = wl_alloc<uint32_t>(ntiles_, &bytes_);
  tile_nw_ = wl_alloc<uint32_t>(ntiles_, &bytes_);
  hipStream_t s = S(stream_);
  HIP_OK(hipMemcpyAsync(wtok0_, wtok.data(), (nint_ + kRunPad) * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(woff_, woff.data(), woff.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  k_wl_set_weights<<<(int)std::min<uint32_t>((nwords_ + 255) / 256, 4096), 256, 0, s>>>(wtok0_, woff_, nwords_, weight_);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(tile_first_, tfirst.data(), ntiles_ * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(tile_nw_, tnw.data(), ntiles_ * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(wtok_, wtok0_, (nint_ + kRunPad) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  // pool: the initial index (<= one entry per adjacent pair), the words-of lists (a merge lists
  // the words it shortened: Σ over a run <= Σ (length - 1)) and the pair groups (<= 2 entries
  // per occurrence merged: Σ <= 2 Σ (length - 1)); undone guesses release theirs (each is the
  // last when its undo runs)
  pool_cap_ = 3 * ntok_ + 4096;
  pool_ = wl_alloc<u64>(2 * pool_cap_, &bytes_);  // WEnt: entry + signature
  dstate_ = wl_alloc<uint32_t>(8, &bytes_);
  HIP_OK(hipMemsetAsync(dstate_, 0, 8 * sizeof(uint32_t), s));
  HIP_OK(hipStreamSynchronize(s));
  reserve(kBaseVocab + 1);
  build_index();
  ready_ = true;
  dirty_ = false;
  return true;
}

// The index of the current words: every (pair, word) once, grouped by pair.
void WordLoop::build_index() {
  hipStream_t s = S(stream_);
  size_t acc = 0;
  // the pairs of the current words, compactly: per-word counts, their exclusive sum
  uint32_t* pbase = wl_alloc<uint32_t>((size_t)nwords_ + 2, &acc);
  uint32_t* pcnt = wl_alloc<uint32_t>((size_t)nwords_ + 2, &acc);
  k_wl_pair_counts<<<(int)std::min<uint32_t>((nwords_ + 256) / 256, 4096), 256, 0, s>>>(wtok_, woff_, nwords_, pcnt);
  HIP_OK(hipGetLastError());
  {
    size_t tb = 0;
    HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, pcnt, pbase, (int)nwords_ + 1, s));
    void* t0 = wl_alloc<uint8_t>(tb, &acc);
    HIP_OK(hipcub::DeviceScan::ExclusiveSum(t0, tb, pcnt, pbase, (int)nwords_ + 1, s));
    HIP_OK(hipStreamSynchronize(s));
    HIP_OK(hipFree(t0));
  }
  uint32_t npairs = 0;
  HIP_OK(hipMemcpy(&npairs, pbase + nwords_, sizeof(uint32_t), hipMemcpyDeviceToHost));
  const uint64_t n = std::max<uint64_t>(npairs, 1);
  u64* kin = wl_alloc<u64>(n, &acc);
  u64* kout = wl_alloc<u64>(n, &acc);
  uint32_t* vin = wl_alloc<uint32_t>(n, &acc);
  uint32_t* vout = wl_alloc<uint32_t>(n, &acc);
  uint32_t* keep = wl_alloc<uint32_t>(n + 1, &acc);
  uint32_t* head = wl_alloc<uint32_t>(n + 1, &acc);
  uint32_t* pos = wl_alloc<uint32_t>(n + 1, &acc);
  uint32_t* kidx = wl_alloc<uint32_t>(n + 1, &acc);
  const int grid = 2048;
  if (npairs == 0) {
    HIP_OK(hipMemsetAsync(kin, 0xFF, sizeof(u64), s));
    HIP_OK(hipMemsetAsync(vin, 0, sizeof(uint32_t), s));
  }
  k_wl_emit_pairs<<<grid, 256, 0, s>>>(wtok_, woff_, pbase, nwords_, unk_, kin, vin);
  HIP_OK(hipGetLastError());
  size_t tmp_bytes = 0, tb2 = 0;
  HIP_OK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, kin, kout, vin, vout, (int)n, 0, 64, s));
  HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, keep, pos, (int)n + 1, s));
  tmp_bytes = std::max(tmp_bytes, tb2);
  void* tmp = wl_alloc<uint8_t>(tmp_bytes, &acc);
  HIP_OK(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, kin, kout, vin, vout, (int)n, 0, 64, s));
  HIP_OK(hipMemsetAsync(keep + n, 0, sizeof(uint32_t), s));
  HIP_OK(hipMemsetAsync(head + n, 0, sizeof(uint32_t), s));
  k_wl_mark<<<grid, 256, 0, s>>>(kout, vout, n, keep, head);
  HIP_OK(hipGetLastError());
  HIP_OK(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, keep, pos, (int)n + 1, s));
  HIP_OK(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, head, kidx, (int)n + 1, s));
  uint32_t tot[2] = {0, 0};
  HIP_OK(hipMemcpyAsync(&tot[0], pos + n, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(&tot[1], kidx + n, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  init_pool_n_ = tot[0];
  init_keys_n_ = tot[1];
  if (init_pool_n_ > pool_cap_) fatal("WordLoop: the initial index exceeds the pool");
  if (init_key_) HIP_OK(hipFree(init_key_));
  if (init_val_) HIP_OK(hipFree(init_val_));
  init_key_ = wl_alloc<u64>(init_keys_n_, &bytes_);
  init_val_ = wl_alloc<u64>(init_keys_n_, &bytes_);
  k_wl_scatter<<<grid, 256, 0, s>>>(kout, vout, n, keep, pos, head, kidx, woff_, reinterpret_cast<WEnt*>(pool_),
                                    init_key_, init_val_);
  HIP_OK(hipGetLastError());
  k_wl_counts<<<256, 256, 0, s>>>(init_val_, init_keys_n_, init_pool_n_);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(s));
  for (void* p : {(void*)kin, (void*)kout, (void*)vin, (void*)vout, (void*)keep, (void*)head, (void*)pos, (void*)kidx,
                  tmp, (void*)pbase, (void*)pcnt})
    HIP_OK(hipFree(p));
  // the directory: at most half full
  uint64_t want = 1024;
  while (want < 2 * init_keys_n_) want <<= 1;
  if (want != dir_cap_) {
    if (dkey_) HIP_OK(hipFree(dkey_));
    if (dval_) HIP_OK(hipFree(dval_));
    dir_cap_ = want;
    dkey_ = wl_alloc<u64>(dir_cap_, &bytes_);
    dval_ = wl_alloc<u64>(dir_cap_, &bytes_);
  }
  restore_index();
}

// The directory, the words-of lists and the counters as right after build_index().
void WordLoop::restore_index() {
  hipStream_t s = S(stream_);
  std::fill(lists_.begin(), lists_.end(), 0ull);  // no words-of lists: every merge looks its pair up
  HIP_OK(hipMemsetAsync(dkey_, 0xFF, dir_cap_ * sizeof(u64), s));
  if (init_keys_n_) {
    k_wl_dir_init<<<1024, 256, 0, s>>>(init_key_, init_val_, init_keys_n_, dkey_, dval_, dir_cap_ - 1);
    HIP_OK(hipGetLastError());
  }
  if (lseq_) HIP_OK(hipMemsetAsync(lseq_, 0xFF, id_cap_ * sizeof(uint32_t), s));
  const uint32_t st[8] = {0, (uint32_t)init_pool_n_, 0, 0, 0, 0, 0, 0};
  HIP_OK(hipMemcpyAsync(dstate_, st, sizeof(st), hipMemcpyHostToDevice, s));
  HIP_OK(hipStreamSynchronize(s));
}

bool WordLoop::load_current(const TiledStream& ts) {
  HIP_OK(hipSetDevice(ordinal_));
  if (!ready_ || !posted_.empty()) return false;
  stop();
  std::vector<int32_t> wtok(nint_ + kRunPad, 0);
  uint32_t w = 0;
  bool open = false;
  for (size_t t = 0; t < ts.num_tiles(); ++t) {
    const int32_t* p = ts.tok.data() + ts.off[t];
    for (uint32_t i = 0; i < ts.len[t]; ++i) {
      if (p[i] < kHeaderLimit) {
        if (open) ++w;
        if ((uint32_t)(p[i] - kHeaderBase) != w || w >= nwords_) return false;
        open = true;
      } else {
        if (!open) return false;
        int32_t& len = wtok[woff_h_[w]];
        if (kRunHdr + (uint32_t)len >= woff_h_[w + 1] - woff_h_[w]) return false;  // past the run
        wtok[woff_h_[w] + kRunHdr + (uint32_t)len] = p[i];
        ++len;
      }
    }
  }
  if (!open || w + 1 != nwords_) return false;
  hipStream_t s = S(stream_);
  HIP_OK(hipMemcpyAsync(wtok_, wtok.data(), wtok.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  k_wl_set_weights<<<(int)std::min<uint32_t>((nwords_ + 255) / 256, 4096), 256, 0, s>>>(wtok_, woff_, nwords_, weight_);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(s));
  build_index();
  dirty_ = false;
  return true;
}

void WordLoop::load_tiles(const int32_t* tok, const uint64_t* tile_off, const uint32_t* tile_len) {
  HIP_OK(hipSetDevice(ordinal_));
  if (!ready_) return;
  if (!posted_.empty()) fatal("WordLoop::load_tiles with a merge in flight");
  stop();
  const int grid = (int)std::min<uint32_t>((ntiles_ + 255) / 256, 4096);
  k_tiles_to_words<<<std::max(grid, 1), 256, 0, S(stream_)>>>(tok, tile_off, tile_len, ntiles_, woff_, wtok_);
  HIP_OK(hipGetLastError());
  build_index();
  dirty_ = false;
}

void WordLoop::reset_words() {
  HIP_OK(hipSetDevice(ordinal_));
  if (!ready_) return;
  if (!posted_.empty()) fatal("WordLoop::reset_words with a merge in flight");
  stop();
  HIP_OK(hipMemcpyAsync(wtok_, wtok0_, (nint_ + kRunPad) * sizeof(int32_t), hipMemcpyDeviceToDevice, S(stream_)));
  dirty_ = false;
}

void WordLoop::reset() {
  HIP_OK(hipSetDevice(ordinal_));
  if (!ready_) return;
  if (!posted_.empty()) fatal("WordLoop::reset with a merge in flight");
  stop();
  hipStream_t s = S(stream_);
  HIP_OK(hipMemcpyAsync(wtok_, wtok0_, (nint_ + kRunPad) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  restore_index();
  dirty_ = false;
}

uint64_t WordLoop::pool_used() const {
  uint32_t v = 0;
  if (dstate_) HIP_OK(hipMemcpy(&v, dstate_ + kStPoolTop, sizeof(v), hipMemcpyDeviceToHost));
  return v;
}

void WordLoop::sync_tiles(int32_t* tok, const uint64_t* tile_off, uint32_t* tile_len) {
  if (!dirty_ || !ready_) return;
  if (running_) stop();
  const int grid = (int)std::min<uint32_t>((ntiles_ + 3) / 4, 4096);
  k_words_to_tiles<<<std::max(grid, 1), 256, 0, S(stream_)>>>(wtok_, woff_, tile_first_, tile_nw_, ntiles_, tok,
                                                           tile_off, tile_len);
  HIP_OK(hipGetLastError());
  dirty_ = false;
}

}  // namespace shred
