// Masked-LM inputs on gfx950: tokens selected per token or per whole word, replaced by a mask id, a
// random id or themselves, with the labels beside them (C ABI and definitions:
// include/shredword_encode.h, shred_mlm_*).  The passes work on the flat (ids, row_off) pair and use
// none of the other units' kernels; they share the batch units' tile geometry (batch_common.h), their
// device-call driver and piece rule (batch_state.h) and the span passes' token-length table.
//
// A decision is a function of (seed, index, id) alone: d(x, c) = mix(mix(seed + G (x + 1)) ^ c) with
// c = SEL for the selection of unit x and c = ACT for the action of token x, so nothing depends on
// the staging and a piece of the host call is the device call at index_base + its first id.
//
//   k_mlm_rows     one thread per row_off entry: range, order and end points (word 0 of the result
//                  words; ordinary stores, no atomics).  Whole-word mode: it also marks the first
//                  token of every row in the begin bytes (cleared before it);
//   k_mlm_begin    whole-word mode, one workgroup per kTile ids, 4 per lane: begin[k] = 1 iff token k
//                  begins a word (the header's rule: k == 0, a row's first token, a special or a
//                  protected id on either side, or a gap between the end of token k - 1 and starts[k]);
//   hipCUB scan    whole-word mode: inclusive maximum over k of (begin[k] ? k : 0) through a transform
//                  iterator: unit[k] = k', the index at which token k's word begins;
//   k_mlm_apply    one workgroup per kTile ids, 4 per lane (16-byte loads and stores where the
//                  pointers allow, entry by entry where they are only element-aligned): reads ids[k]
//                  (and unit[k]), hashes for the selection and, for a selected token, for the action,
//                  writes out[k] and labels[k].  The selected count: wave reduction, the four waves'
//                  sums through LDS, one atomic per workgroup into word 1 of the result words.  A
//                  workgroup that finds word 0 set writes nothing, so a bad row_off needs no host
//                  round trip before the pass: both words come back in one copy at the end.
//
// The protect list and every other option travel as kernel arguments (MaskRule, by value).
// In place (out == ids): the begin pass and the scan are complete before k_mlm_apply starts (one
// stream), and a lane of k_mlm_apply reads only the ids it then overwrites.
//
// Traffic per id.  Token mode: 4 read (ids) + 8 written (out, labels) = 12 B.  Whole-word mode adds
// 1 written (begin cleared), 4 + 8 + 1 read and 1 written (k_mlm_begin: ids, starts, begin), 1 read
// and 8 written by the scan (its look-back state is per tile, not per id), and 8 read by
// k_mlm_apply (unit): 12 + 32 = 44 B.  Per row 8 B (k_mlm_rows), + 1 B for the row's begin mark.
// All global indices are 64-bit; every store is an ordinary vector store.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../host/encoder.h"
#include "batch_common.h"
#include "batch_state.h"
#include "encode_common.h"

namespace shred {
namespace {

constexpr u64 kGolden = 0x9E3779B97F4A7C15ull;
constexpr u64 kSel = 1ull << 40, kAct = (1ull << 40) + 1;  // above every merge rank (dropout's third input)

__device__ __forceinline__ u64 mix64(u64 x) {  // murmur3's fmix64
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// What the kernels know of a call's options; passed by value, so the protect list is read from the
// kernel arguments.
struct MaskRule {
  u64 seed, base;                 // base: index_base + the index in the call's ids of the pass's first id
  u64 t_sel, t_mask, t_act, rand_vocab;
  int32_t mask_id, ignore_id, sp_lo, sp_hi;
  uint32_t protect_specials, protect_n;
  int32_t protect[EncodeDevice::kMaskMaxProtect];

  __device__ __forceinline__ u64 draw(u64 x, u64 c) const { return mix64(mix64(seed + kGolden * (x + 1)) ^ c); }
  __device__ __forceinline__ bool special(int32_t id) const { return id >= sp_lo && id < sp_hi; }
  __device__ __forceinline__ bool listed(int32_t id) const {
    bool hit = false;
    for (uint32_t i = 0; i < protect_n; ++i) hit |= protect[i] == id;
    return hit;
  }
  // never selected / a word of its own
  __device__ __forceinline__ bool guarded(int32_t id) const { return (protect_specials && special(id)) || listed(id); }
  __device__ __forceinline__ bool alone(int32_t id) const { return special(id) || listed(id); }
};

MaskRule rule_of(const EncodeDevice::MaskOpts& o, u64 first) {
  MaskRule r{o.seed,    o.index_base + first, o.t_sel, o.t_mask, o.t_act, o.rand_vocab, o.mask_id, o.ignore_id,
             o.sp_lo,   o.sp_hi,              o.protect_specials ? 1u : 0u, o.protect_n, {}};
  for (uint32_t i = 0; i < o.protect_n; ++i) r.protect[i] = o.protect[i];
  return r;
}

// begin: nullptr, or n bytes cleared before the launch.
__global__ __launch_bounds__(kThreads) void k_mlm_rows(const int64_t* __restrict__ row, u64 rows, u64 n, int ends,
                                                       uint8_t* __restrict__ begin, u64* __restrict__ res) {
  const u64 r = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (r > rows) return;
  const int64_t v = row[r];
  const int64_t prev = r ? row[r - 1] : 0;
  bool bad = v < 0 || (u64)v > n || prev > v;
  if (ends && ((r == 0 && v != 0) || (r == rows && (u64)v != n))) bad = true;
  if (bad) {
    res[0] = 1;
    return;
  }
  if (begin && r < rows && (u64)v < n) begin[v] = 1;
}

// Four consecutive entries of p at g (cnt of them inside the array).
template <class V, class T>
__device__ __forceinline__ void load4(const T* p, u64 g, int cnt, bool vec, T (&v)[kLane]) {
  if (vec && cnt == kLane) {
    const V w = *reinterpret_cast<const V*>(p + g);
    v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
  } else {
#pragma unroll
    for (int i = 0; i < kLane; ++i) v[i] = i < cnt ? p[g + i] : T(0);
  }
}

__device__ __forceinline__ void store4(int32_t* p, u64 g, int cnt, bool vec, const int32_t (&v)[kLane]) {
  if (vec && cnt == kLane) {
    *reinterpret_cast<int4*>(p + g) = make_int4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < kLane; ++i)
      if (i < cnt) p[g + i] = v[i];
  }
}

// begin: the rows' first tokens marked, n rounded up to kLane bytes allocated; aligned: bit 0 ids,
// bit 1 starts may take 16-byte loads.
__global__ __launch_bounds__(kThreads) void k_mlm_begin(const int32_t* __restrict__ ids,
                                                        const int64_t* __restrict__ starts, u64 n,
                                                        const int32_t* __restrict__ lens, uint32_t limit, MaskRule rule,
                                                        uint32_t aligned, uint8_t* __restrict__ begin) {
  const u64 g = (u64)blockIdx.x * kTile + (u64)threadIdx.x * kLane;
  if (g >= n) return;
  const int cnt = n - g < (u64)kLane ? (int)(n - g) : kLane;
  int32_t id[kLane];
  int64_t st[kLane];
  load4<int4>(ids, g, cnt, (aligned & 1u) != 0, id);
  if ((aligned & 2u) && cnt == kLane) {
    const longlong2 a = *reinterpret_cast<const longlong2*>(starts + g);
    const longlong2 b = *reinterpret_cast<const longlong2*>(starts + g + 2);
    st[0] = a.x, st[1] = a.y, st[2] = b.x, st[3] = b.y;
  } else {
#pragma unroll
    for (int i = 0; i < kLane; ++i) st[i] = i < cnt ? starts[g + i] : 0;
  }
  uint32_t marks = *reinterpret_cast<const uint32_t*>(begin + g);
  int32_t pid = g ? ids[g - 1] : 0;
  int64_t pst = g ? starts[g - 1] : 0;
  bool palone = g ? rule.alone(pid) : true;  // (token 0 begins a word whatever is before it)
#pragma unroll
  for (int i = 0; i < kLane; ++i) {
    const bool me = rule.alone(id[i]);
    const int64_t plen = ((uint32_t)pid >= 256u && (uint32_t)pid < limit) ? (int64_t)lens[pid] : 1;
    if (me || palone || st[i] != pst + plen) marks |= 1u << (8 * i);
    pid = id[i];
    pst = st[i];
    palone = me;
  }
  *reinterpret_cast<uint32_t*>(begin + g) = marks & 0x01010101u;
}

// Element k of the scan: k where a word begins, else 0.
struct BeginAt {
  const uint8_t* begin;
  __host__ __device__ __forceinline__ u64 operator()(u64 k) const { return begin[k] ? k : 0ull; }
};

// aligned: bit 0 ids, bit 1 out, bit 2 labels may take 16-byte accesses.  ids and out may be one
// buffer: a lane reads its four ids before it writes them.
template <bool kWhole>
__global__ __launch_bounds__(kThreads) void k_mlm_apply(const int32_t* ids, u64 n, const u64* __restrict__ unit,
                                                        MaskRule rule, int32_t* out, int32_t* __restrict__ labels,
                                                        uint32_t aligned, u64* res) {
  __shared__ uint32_t s_part[kThreads / 64];
  const int tid = threadIdx.x;
  const u64 g = (u64)blockIdx.x * kTile + (u64)tid * kLane;
  uint32_t selected = 0;
  if (res[0] == 0 && g < n) {  // (word 0: k_mlm_rows found a bad row_off; nothing is written then)
    const int cnt = n - g < (u64)kLane ? (int)(n - g) : kLane;
    int32_t id[kLane], o[kLane], lab[kLane];
    u64 h[kLane];
    load4<int4>(ids, g, cnt, (aligned & 1u) != 0, id);
    if (kWhole) {
      load4<ulonglong4>(unit, g, cnt, true, h);  // unit is the pass's own allocation: aligned
    } else {
#pragma unroll
      for (int i = 0; i < kLane; ++i) h[i] = g + (u64)i;
    }
#pragma unroll
    for (int i = 0; i < kLane; ++i) {
      o[i] = id[i];
      lab[i] = rule.ignore_id;
      if (i < cnt && !rule.guarded(id[i]) && (rule.draw(rule.base + h[i], kSel) >> 32) < rule.t_sel) {
        ++selected;
        lab[i] = id[i];
        const u64 a = rule.draw(rule.base + g + (u64)i, kAct);
        const u64 v = a >> 32;
        if (v < rule.t_mask) {
          o[i] = rule.mask_id;
        } else if (v < rule.t_act) {
          o[i] = (int32_t)(((a & 0xFFFFFFFFull) * rule.rand_vocab) >> 32);
        }
      }
    }
    store4(out, g, cnt, (aligned & 2u) != 0, o);
    store4(labels, g, cnt, (aligned & 4u) != 0, lab);
  }
  for (int d = 32; d > 0; d >>= 1) selected += __shfl_down(selected, d, 64);
  if ((tid & 63) == 0) s_part[tid >> 6] = selected;
  __syncthreads();
  if (tid == 0) {
    uint32_t t = 0;
    for (int i = 0; i < kThreads / 64; ++i) t += s_part[i];
    if (t) atomicAdd(reinterpret_cast<unsigned long long*>(res + 1), (unsigned long long)t);
  }
}

// One call's (or piece's) ids, as the passes take them; every pointer on the device.
struct MaskCall {
  const int32_t* ids;
  u64 n;
  const int64_t* row;  // nullptr: no row pass (one row of all ids, or a piece of token mode)
  u64 rows;
  bool ends;           // check row[0] == 0 and row[rows] == n (a piece's local offsets: no)
  bool whole;
  const int64_t* starts;
  const int32_t* lens;
  uint32_t limit;      // entries of lens
  MaskRule rule;
  int32_t *out, *labels;
};

// The masking passes' state, allocated on the first masking call: the result words, the whole-word
// scratch grown to the most ids seen, and the staging of the host path.
struct MaskState : PassState {
  DeviceWords res;             // [0] a bad row_off, [1] the selected count
  PinnedWords host;            // the two
  EventSet<4> ev;
  DeviceBuf<uint8_t> begin;    // whole-word: 1 B per id
  DeviceBuf<u64> unit;         // whole-word: k' of every id
  DeviceBuf<uint8_t> tmp;      // hipCUB scan scratch
  DeviceBuf<int32_t> hids;     // host path: a piece's ids, out and labels (3 x hids.cap())
  DeviceBuf<int64_t> hrow, hstarts;

  bool reserve(size_t) { return res.ensure(2) && host.ensure(2) && ev.ensure(); }

  bool reserve_words(size_t n) {
    if (!begin.grow(n + kLane) || !unit.grow(std::max<size_t>(n, 1))) return false;
    size_t bytes = 0;
    if (hipcub::DeviceScan::InclusiveScan(nullptr, bytes, row_iter(BeginAt{begin.get()}), unit.get(), hipcub::Max(),
                                          (u64)n) != hipSuccess)
      return false;
    return tmp.grow(std::max<size_t>(bytes, 16));
  }

  // Clears the result words and checks the rows (whole-word mode: marks their first tokens): 0 or -1.
  int check(const MaskCall& c, hipStream_t st) {
    ENC_OK(hipMemsetAsync(res.get(), 0, 16, st));
    if (c.whole && c.n) ENC_OK(hipMemsetAsync(begin.get(), 0, c.n, st));
    if (c.row) {
      k_mlm_rows<<<dim3((unsigned)((c.rows + kThreads) / kThreads)), dim3(kThreads), 0, st>>>(
          c.row, c.rows, c.n, c.ends ? 1 : 0, c.whole && c.n ? begin.get() : nullptr, res.get());
      ENC_OK(hipGetLastError());
    }
    return 0;
  }

  // The passes over the ids, then the result words on their way to `host`: 0 or -1.
  int apply(const MaskCall& c, hipStream_t st) {
    if (c.n) {
      const unsigned tiles = (unsigned)((c.n + kTile - 1) / kTile);
      if (c.whole) {
        k_mlm_begin<<<dim3(tiles), dim3(kThreads), 0, st>>>(c.ids, c.starts, c.n, c.lens, c.limit, c.rule,
                                                            (aligned16(c.ids) ? 1u : 0u) | (aligned16(c.starts) ? 2u : 0u),
                                                            begin.get());
        ENC_OK(hipGetLastError());
        size_t bytes = tmp.cap();
        ENC_OK(hipcub::DeviceScan::InclusiveScan(tmp.get(), bytes, row_iter(BeginAt{begin.get()}), unit.get(),
                                                 hipcub::Max(), c.n, st));
      }
      const uint32_t al = (aligned16(c.ids) ? 1u : 0u) | (aligned16(c.out) ? 2u : 0u) | (aligned16(c.labels) ? 4u : 0u);
      (c.whole ? k_mlm_apply<true> : k_mlm_apply<false>)<<<dim3(tiles), dim3(kThreads), 0, st>>>(
          c.ids, c.n, unit.get(), c.rule, c.out, c.labels, al, res.get());
      ENC_OK(hipGetLastError());
    }
    ENC_OK(hipMemcpyAsync(host.get(), res.get(), 16, hipMemcpyDeviceToHost, st));
    return 0;
  }

  // Staging of a piece of len ids and m rows.
  bool stage(size_t len, size_t m, bool whole) {
    return hids.grow(len, 3) && (!whole || (hrow.grow(m + 1) && hstarts.grow(len) && reserve_words(len)));
  }
};

}  // namespace

int64_t EncodeDevice::mask(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const MaskOpts& o,
                           const int64_t* starts, const std::vector<int32_t>& lens, int32_t* out, int32_t* labels,
                           void* stream, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  const bool whole = o.whole_word && n;
  const int32_t* dlens = whole ? span_lens(lens) : nullptr;
  if (whole && !dlens) {
    std::fprintf(stderr, "[ERROR]\t encoder: mask could not upload the token lengths\n");
    return -1;
  }
  const u64 R = row_off ? rows : 1;
  const MaskCall c{ids, n, row_off, R, true, whole, starts, dlens, (uint32_t)lens.size(), rule_of(o, 0), out, labels};
  const int64_t r = device_call<MaskState>(
      pass_[kMask], device_, stream ? stream : stream_, "mask", R, kernel_ms,
      [&](MaskState& ms, hipStream_t st, Plan* p) {
        if (whole && !ms.reserve_words(n)) {
          std::fprintf(stderr, "[ERROR]\t encoder: mask allocation failed (%zu ids)\n", n);
          return -1;
        }
        *p = Plan{0, true, n};
        return ms.check(c, st);
      },
      [&](MaskState& ms, hipStream_t st) { return ms.apply(c, st); });
  if (r < 0) return r;
  const MaskState& ms = pass_state<MaskState>(pass_[kMask]);
  return ms.host[0] ? -6 : (int64_t)ms.host[1];
}

// Host ids in pieces of whole rows (piece_end).  A piece is the device passes on its own ids at
// index_base + the index of its first id; the caller has validated row_off on the host, so token
// mode stages no offsets, and whole-word mode stages the piece's local ones for the rows' first
// tokens.  The outputs are per id, so the pieces are cut, staged and copied back here.
int64_t EncodeDevice::mask_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const MaskOpts& o,
                                const int64_t* starts, const std::vector<int32_t>& lens, int32_t* out,
                                int32_t* labels) {
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  MaskState& ms = pass_state<MaskState>(pass_[kMask]);
  const bool whole = o.whole_word;
  const int32_t* dlens = whole && n ? span_lens(lens) : nullptr;
  if (!ms.reserve(0) || (whole && n && !dlens)) {
    std::fprintf(stderr, "[ERROR]\t encoder: mask allocation failed\n");
    return -1;
  }
  hipStream_t st = (hipStream_t)stream_;
  const size_t R = row_off ? rows : 1, piece = piece_ids();
  const HostIn in{ids, n, row_off};
  std::vector<int64_t> local;
  u64 selected = 0;
  for (size_t r0 = 0; r0 < R;) {
    u64 emitted = 0;
    const size_t r1 = piece_end(&in, 1, R, r0, piece, 0, [](size_t) { return (u64)0; }, &emitted, nullptr);
    const size_t a = row_off ? (size_t)row_off[r0] : 0, len = (row_off ? (size_t)row_off[r1] : n) - a, m = r1 - r0;
    r0 = r1;
    if (!len) continue;
    if (!tiles_fit(len) || !ms.stage(len, m, whole)) {
      std::fprintf(stderr, "[ERROR]\t encoder: mask staging allocation failed (%zu ids, %zu rows)\n", len, m);
      return -1;
    }
    int32_t *const dids = ms.hids.get(), *const dout = dids + ms.hids.cap(), *const dlab = dout + ms.hids.cap();
    ENC_OK(hipMemcpyAsync(dids, ids + a, len * 4, hipMemcpyHostToDevice, st));
    const bool rows_up = whole && row_off;
    if (whole) ENC_OK(hipMemcpyAsync(ms.hstarts.get(), starts + a, len * 8, hipMemcpyHostToDevice, st));
    if (rows_up) {
      local.resize(m + 1);
      for (size_t i = 0; i <= m; ++i) local[i] = row_off[r1 - m + i] - (int64_t)a;
      ENC_OK(hipMemcpyAsync(ms.hrow.get(), local.data(), (m + 1) * 8, hipMemcpyHostToDevice, st));
    }
    const MaskCall c{dids,  len,   rows_up ? ms.hrow.get() : nullptr, m,   false, whole, whole ? ms.hstarts.get() : nullptr,
                     dlens, (uint32_t)lens.size(), rule_of(o, a),     dout, dlab};
    if (ms.check(c, st) < 0 || ms.apply(c, st) < 0) return -1;
    ENC_OK(hipMemcpyAsync(out + a, dout, len * 4, hipMemcpyDeviceToHost, st));
    ENC_OK(hipMemcpyAsync(labels + a, dlab, len * 4, hipMemcpyDeviceToHost, st));
    ENC_OK(hipStreamSynchronize(st));
    selected += ms.host[1];
  }
  return (int64_t)selected;
}

}  // namespace shred
