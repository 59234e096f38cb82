// Special tokens matched in the text on gfx950 (C ABI and the matching rule:
// include/shredword_encode.h, shred_encode_special*).  The passes run around the encoder
// (encode_device.hip) and the span passes (encode_spans.hip) and change none of their kernels.
//
// A special holds no delimiter, so every match lies inside one run of non-delimiter bytes, and
// the rule (leftmost, then longest, no overlap) is a sequential walk of each run on its own.  The
// accepted matches are blanked in a copy of the text; the encoder turns what is left into word
// ids; the two ascending streams (word ids by their byte offsets, matches by position) are merged.
//
//   k_special_scan<false>  one thread per 32-byte span walks the runs that start in it (the
//                   encoder's word walk on the chunk staged in LDS).  At each byte a 256-bit
//                   first-byte set in LDS rejects almost every position; on a hit the specials
//                   with that first byte are compared longest first against the table in LDS (one
//                   word per special + their bytes: <= 17.5 KB, loaded per workgroup from L2).
//                   Counts the span's matches; flags a run past the word limit in force.
//   hipCUB scan     inclusive sum of the per-span counts (runs and their matches are ordered by
//                   position, so the sum is each span's place in the match list).  No match:
//                   the call continues as the plain encode.
//   copy + k_special_scan<true>  the text copied; the same walk writes (position, special) at
//                   the span's place and blanks the match in the copy with ' '.
//   encode()        on the blanked copy: the word ids W.
//   span_passes()   on the blanked copy: the byte offset of every word id.
//   k_special_merge_words / _specials  word id k goes to k + #{matches before its offset}, match j
//                   to j + #{word ids before its position}: per 1024 word ids two binary searches
//                   bound the matches in reach (almost always none or one); per match one binary
//                   search of the offsets.
// starts / line_off of the merged stream are the span passes' on the original text with the
// length table extended by the specials' lengths (the merged ids tile its non-delimiter bytes).
// Traffic per text byte on top of encode + spans, with matches: 2 B of text read (two walks) +
// 2 B copy + 0.5 B of counts, the encoder's 1 B read of the copy, the extra span passes (2 B + 28 B
// x ids / byte) and 4 B x ids / byte x 2 + 8 B x ids / byte (merge: ids read and written, offsets
// read); without a match: 1 B of text read + 0.125 B of counts.
// All global indices are 64-bit; every store is an ordinary vector store.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "../host/encoder.h"
#include "encode_common.h"
#include "encode_words.h"

namespace shred {
namespace {

typedef uint64_t u64;

// The scan table, in 32-bit words: [0, 8) the first-byte set; from word 8 the G + 1 group bounds
// (16 bits each; group g: the specials whose first byte is the g-th set bit, longest first); from
// `ent` one word per special in group order: byte offset | length << 16 | index << 24; from
// `bytes` the specials' bytes.
constexpr int kSetWords = 8;
struct SpecialTab {
  const uint32_t* w;
  uint32_t words, ent, bytes;
};

// The longest special that equals text[p : p + len] with len <= room, or 0.
template <typename T>
__device__ __forceinline__ uint32_t match_at(const T& text, u64 p, u64 room, const uint32_t* tab, uint32_t ent,
                                             uint32_t bytes, uint32_t* idx) {
  const uint32_t c = text[p];
  const uint32_t word = tab[c >> 5], bit = 1u << (c & 31u);
  if (!(word & bit)) return 0;
  uint32_t g = __popc(word & (bit - 1u));
  for (uint32_t i = 0; i < (c >> 5); ++i) g += __popc(tab[i]);
  const uint16_t* grp = reinterpret_cast<const uint16_t*>(tab + kSetWords);
  const uint8_t* sb = reinterpret_cast<const uint8_t*>(tab + bytes);
  for (uint32_t e = grp[g], end = grp[g + 1]; e < end; ++e) {
    const uint32_t v = tab[ent + e];
    const uint32_t len = (v >> 16) & 255u;
    if ((u64)len > room) continue;
    const uint8_t* b = sb + (v & 0xFFFFu);
    uint32_t k = 1;  // byte 0 is the group's
    while (k < len && (uint32_t)b[k] == text[p + k]) ++k;
    if (k == len) {
      *idx = v >> 24;
      return len;
    }
  }
  return 0;
}

// kWrite false: cnt[span] = the matches of the runs starting in the span; *flag |= 1 for a run
// past maxw (kEncMaxWord, or the long-word limit).  kWrite true: the same walk writes its matches from inc[span] - cnt[span] on
// (M entries in all) and blanks them in `masked` (a copy of the text).
template <bool kWrite>
__global__ __launch_bounds__(kThreads) void k_special_scan(const uint8_t* __restrict__ text, u64 n, SpecialTab tab,
                                                           uint32_t* __restrict__ cnt, const u64* __restrict__ inc,
                                                           u64* __restrict__ m_pos, uint32_t* __restrict__ m_idx,
                                                           u64 M, uint8_t* __restrict__ masked,
                                                           u64* __restrict__ flag, u64 maxw) {
  __shared__ uint32_t s_text[kStageBytes / 4];
  extern __shared__ uint32_t s_tab[];
  for (uint32_t i = threadIdx.x; i < tab.words; i += kThreads) s_tab[i] = tab.w[i];
  const TextView tv = stage_chunk(text, n, blockIdx.x, s_text);  // synchronises
  const u64 span = (u64)blockIdx.x * kThreads + threadIdx.x;
  const u64 base = span * kSpan;
  u64 at = 0;
  if (kWrite) at = inc[span] - cnt[span];
  uint32_t c = 0;
  auto run = [&](u64 s, u64 L, int) {
    if (L > maxw) {
      if (!kWrite) atomicOr(reinterpret_cast<unsigned long long*>(flag), 1ull);
      return;
    }
    const u64 end = s + L;
    for (u64 p = s; p < end;) {
      uint32_t idx = 0;
      const uint32_t len = match_at(tv, p, end - p, s_tab, tab.ent, tab.bytes, &idx);
      if (!len) {
        ++p;
        continue;
      }
      if (kWrite && at + c < M) {
        m_pos[at + c] = p;
        m_idx[at + c] = idx;
        for (uint32_t k = 0; k < len; ++k) masked[p + k] = 32;  // p + len <= end <= n
      }
      ++c;
      p += len;
    }
  };
  if (maxw > (u64)kEncMaxWord) for_each_word(tv, n, base, run, text, maxw);
  else for_each_word(tv, n, base, run);
  if (!kWrite) cnt[span] = c;
}

struct Widen {
  __host__ __device__ __forceinline__ u64 operator()(uint32_t v) const { return v; }
};
typedef hipcub::TransformInputIterator<u64, Widen, const uint32_t*> CountIter;

// First j in [lo, hi) with a[j] >= v, or hi.
template <typename A>
__device__ __forceinline__ u64 lower_bound(const A* __restrict__ a, u64 lo, u64 hi, u64 v) {
  while (lo < hi) {
    const u64 mid = lo + ((hi - lo) >> 1);
    if ((u64)a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

constexpr int kMergeThreads = 256;
constexpr int kMergeTile = 4 * kMergeThreads;  // word ids per workgroup

// out[k + #{j : m_pos[j] < wstarts[k]}] = wids[k].  (No token starts where another does.)
__global__ __launch_bounds__(kMergeThreads) void k_special_merge_words(const int32_t* __restrict__ wids,
                                                                       const int64_t* __restrict__ wstarts, u64 Tw,
                                                                       const u64* __restrict__ m_pos, u64 M,
                                                                       int32_t* __restrict__ out) {
  __shared__ u64 s_j[2];
  const u64 k0 = (u64)blockIdx.x * kMergeTile;
  const u64 k1 = k0 + kMergeTile < Tw ? k0 + kMergeTile : Tw;
  if (threadIdx.x == 0) s_j[0] = lower_bound(m_pos, 0, M, (u64)wstarts[k0]);
  if (threadIdx.x == 64) s_j[1] = lower_bound(m_pos, 0, M, (u64)wstarts[k1 - 1]);
  __syncthreads();
  const u64 j0 = s_j[0], j1 = s_j[1];
  for (u64 k = k0 + threadIdx.x; k < k1; k += kMergeThreads)
    out[k + lower_bound(m_pos, j0, j1, (u64)wstarts[k])] = wids[k];
}

// out[j + #{k : wstarts[k] < m_pos[j]}] = first_id + m_idx[j].
__global__ __launch_bounds__(kMergeThreads) void k_special_merge_specials(const int64_t* __restrict__ wstarts, u64 Tw,
                                                                          const u64* __restrict__ m_pos,
                                                                          const uint32_t* __restrict__ m_idx, u64 M,
                                                                          int32_t first_id, int32_t* __restrict__ out) {
  const u64 j = (u64)blockIdx.x * kMergeThreads + threadIdx.x;
  if (j >= M) return;
  out[j + lower_bound(wstarts, 0, Tw, m_pos[j])] = first_id + (int32_t)m_idx[j];
}

// The special passes' state, allocated on the first special call.  Scratch grown to the largest
// call seen: 5 B per text byte (the blanked copy, its word ids) + 12 B per 32-byte span (counts,
// their sums), the scan's scratch.
struct SpecialState : PassState {
  DeviceBuf<uint32_t> tab;          // scan table: first-byte set, groups, entries, bytes
  uint32_t tab_ent = 0, tab_bytes = 0;  // its entry and byte word offsets (its size: tab.cap())
  DeviceBuf<uint8_t> text;          // the text with the accepted matches blanked
  DeviceBuf<int32_t> wids;          // ids of the blanked text's words (as many as text holds bytes)
  DeviceBuf<uint32_t> cnt;          // matches of the runs that start in each 32-byte span
  DeviceBuf<u64> inc;               // their inclusive sum
  DeviceBuf<uint8_t> tmp;           // hipCUB scan scratch
  DeviceBuf<int64_t> wstarts;       // byte offsets of the word ids
  DeviceBuf<u64> mpos;              // match positions, ascending
  DeviceBuf<uint32_t> midx;         // their specials
  DeviceWords flag;                 // a run past the word limit
  PinnedWords host;                 // match total, the flag
  EventSet<4> ev;

  // The scan table of special i = bytes[off[i] .. off[i + 1]).
  bool upload_table(const std::vector<uint8_t>& bytes, const std::vector<uint32_t>& off) {
    const size_t K = off.size() - 1;
    std::vector<uint32_t> order(K);
    std::iota(order.begin(), order.end(), 0u);
    auto len = [&](uint32_t i) { return off[i + 1] - off[i]; };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
      const uint8_t ca = bytes[off[a]], cb = bytes[off[b]];
      return ca != cb ? ca < cb : len(a) != len(b) ? len(a) > len(b) : a < b;
    });
    std::vector<uint32_t> set(kSetWords, 0);
    std::vector<uint16_t> grp;
    for (size_t e = 0; e < K; ++e) {
      const uint8_t c = bytes[off[order[e]]];
      if (!(set[c >> 5] >> (c & 31) & 1u)) grp.push_back((uint16_t)e);
      set[c >> 5] |= 1u << (c & 31);
    }
    grp.push_back((uint16_t)K);
    if (grp.size() & 1) grp.push_back(0);
    const uint32_t ent = kSetWords + (uint32_t)grp.size() / 2, first = ent + (uint32_t)K;
    std::vector<uint32_t> t(first + (bytes.size() + 3) / 4, 0);
    std::copy(set.begin(), set.end(), t.begin());
    for (size_t g = 0; g < grp.size(); ++g) t[kSetWords + g / 2] |= (uint32_t)grp[g] << (16 * (g & 1));
    for (size_t e = 0; e < K; ++e)  // (offsets < 2^14, lengths <= 64, indices < 256)
      t[ent + e] = off[order[e]] | len(order[e]) << 16 | order[e] << 24;
    for (size_t i = 0; i < bytes.size(); ++i) t[first + i / 4] |= (uint32_t)bytes[i] << (8 * (i & 3));
    tab.reset();  // (sized exactly: the kernels stage tab.cap() words in LDS)
    if (!tab.grow(t.size()) || hipMemcpy(tab.get(), t.data(), t.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
      return false;
    tab_ent = ent;
    tab_bytes = first;
    return true;
  }

  bool reserve(size_t n) {
    if (!flag.ensure(1) || !host.ensure(2) || !ev.ensure()) return false;
    const size_t nb = (n + kChunk - 1) / kChunk, cap = nb * kChunk, spans = nb * kThreads;
    if (!text.grow(cap) || !wids.grow(cap) || !cnt.grow(spans) || !inc.grow(spans)) return false;
    size_t need = 0;
    if (hipcub::DeviceScan::InclusiveSum(nullptr, need, CountIter(cnt.get(), Widen()), inc.get(), (u64)spans) !=
        hipSuccess)
      return false;
    return tmp.grow(std::max<size_t>(need, 16));
  }
};

}  // namespace

void EncodeDevice::set_specials(const uint8_t* bytes, const size_t* off, size_t K, int32_t first_id) {
  sx_bytes_.assign(bytes, bytes + (K ? off[K] : 0));
  sx_off_.clear();
  for (size_t i = 0; K && i <= K; ++i) sx_off_.push_back((uint32_t)off[i]);
  sx_first_id_ = first_id;
  sx_dirty_ = true;
  // what was built from the old set: the span passes' length table, the decode vocabulary
  (void)hipSetDevice(device_);
  for (auto& p : pass_)
    if (p) p->specials_changed();
}

int64_t EncodeDevice::encode_special(const uint8_t* text, size_t n, int32_t* out, size_t cap,
                                     const std::vector<int32_t>& lens, void* stream, double* enc_ms,
                                     double* special_ms, uint64_t pos_base) {
  if (enc_ms) *enc_ms = 0;
  if (special_ms) *special_ms = 0;
  if (sx_off_.size() < 2) return encode(text, n, out, cap, stream, enc_ms, pos_base);  // no special registered
  if (n == 0) return 0;
  if (!text || !out) return -1;
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  SpecialState& sx = pass_state<SpecialState>(pass_[kSpecial]);
  if ((sx_dirty_ && !sx.upload_table(sx_bytes_, sx_off_)) || !sx.reserve(n)) {
    std::fprintf(stderr, "[ERROR]\t encoder: special-token scratch allocation failed (%zu bytes)\n", n);
    return -1;
  }
  sx_dirty_ = false;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)stream_;
  const EventSet<4>& ev = sx.ev;
  const u64 nb = (n + kChunk - 1) / kChunk, spans = nb * kThreads;
  const SpecialTab tab{sx.tab.get(), (uint32_t)sx.tab.cap(), sx.tab_ent, sx.tab_bytes};
  const size_t lds = sx.tab.cap() * 4;
  uint32_t* const cnt = sx.cnt.get();
  u64* const inc = sx.inc.get();
  ENC_OK(hipEventRecord(ev[0], st));
  ENC_OK(hipMemsetAsync(sx.flag.get(), 0, 8, st));
  k_special_scan<false><<<dim3((unsigned)nb), dim3(kThreads), lds, st>>>(text, n, tab, cnt, nullptr, nullptr, nullptr,
                                                                         0, nullptr, sx.flag.get(), (u64)max_word());
  ENC_OK(hipGetLastError());
  size_t tmp = sx.tmp.cap();
  ENC_OK(hipcub::DeviceScan::InclusiveSum(sx.tmp.get(), tmp, CountIter(cnt, Widen()), inc, spans, st));
  ENC_OK(hipMemcpyAsync(sx.host.get(), inc + spans - 1, 8, hipMemcpyDeviceToHost, st));
  ENC_OK(hipMemcpyAsync(sx.host.get() + 1, sx.flag.get(), 8, hipMemcpyDeviceToHost, st));
  ENC_OK(hipStreamSynchronize(st));
  if (sx.host[1]) return -3;
  const size_t M = (size_t)sx.host[0];
  if (M == 0) {  // no match: the plain encode
    ENC_OK(hipEventRecord(ev[1], st));
    const int64_t T = encode(text, n, out, cap, stream, enc_ms, pos_base);
    if (T >= 0 && special_ms) ENC_OK(ev.sum_ms(1, special_ms));
    return T;
  }
  if (!sx.mpos.grow(M) || !sx.midx.grow(M)) return -1;
  uint8_t* const masked = sx.text.get();
  int32_t* const wids = sx.wids.get();
  ENC_OK(hipMemcpyAsync(masked, text, n, hipMemcpyDeviceToDevice, st));
  k_special_scan<true><<<dim3((unsigned)nb), dim3(kThreads), lds, st>>>(text, n, tab, cnt, inc, sx.mpos.get(),
                                                                        sx.midx.get(), (u64)M, masked, sx.flag.get(),
                                                                        (u64)max_word());
  ENC_OK(hipGetLastError());
  ENC_OK(hipEventRecord(ev[1], st));
  // (the blanked copy has the text's length, so its offsets are the text's)
  const int64_t Tw = encode(masked, n, wids, sx.wids.cap(), stream, enc_ms, pos_base);
  if (Tw < 0) return Tw;
  ENC_OK(hipSetDevice(device_));  // (encode's guard restored the caller's)
  const size_t T = (size_t)Tw + M;
  if (T > cap) return -2;
  ENC_OK(hipEventRecord(ev[2], st));
  if (Tw) {
    if (!sx.wstarts.grow((size_t)Tw)) return -1;
    size_t nl = 0;
    uint8_t last = 0;
    if (span_passes(masked, n, wids, (size_t)Tw, sx.wstarts.get(), nullptr, 0, 0, 0, false, lens, st, &nl, &last,
                    nullptr) < 0)
      return -1;
    k_special_merge_words<<<dim3((unsigned)(((u64)Tw + kMergeTile - 1) / kMergeTile)), dim3(kMergeThreads), 0, st>>>(
        wids, sx.wstarts.get(), (u64)Tw, sx.mpos.get(), (u64)M, out);
    ENC_OK(hipGetLastError());
  }
  k_special_merge_specials<<<dim3((unsigned)((M + kMergeThreads - 1) / kMergeThreads)), dim3(kMergeThreads), 0, st>>>(
      sx.wstarts.get(), (u64)Tw, sx.mpos.get(), sx.midx.get(), (u64)M, sx_first_id_, out);
  ENC_OK(hipGetLastError());
  ENC_OK(hipEventRecord(ev[3], st));
  ENC_OK(hipStreamSynchronize(st));
  if (special_ms) ENC_OK(ev.sum_ms(2, special_ms));
  return (int64_t)T;
}

}  // namespace shred
