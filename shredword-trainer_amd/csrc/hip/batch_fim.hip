// Fill-in-the-middle rows on gfx950 (FIM: a decoder-only model learns infilling): a row is cut into
// prefix, middle and suffix and re-emitted as pre prefix suf suffix mid middle (PSM) or pre suf suffix
// mid prefix middle (SPM) (C ABI and definitions: include/shredword_encode.h, shred_fim_*).  The stream
// comes out in the flat (ids, row_off) format.  The passes share the batch units' tile geometry and
// wave search (batch_common.h), their device-call driver and piece rule (batch_state.h) and the hash of
// the dropout, masked-LM and span-corruption units.
//
// A decision is a function of (seed, row index) alone: d(x, c) = mix(mix(seed + G (x + 1)) ^ c) with
// c = FIM for "the row is transformed", CUT_A and CUT_B for the two cuts and MODE for the order, so
// nothing depends on the staging and a piece of the host call is the device call at row_base + its
// first row.
//
//   k_fim_rows     one thread per row_off entry: range, order and end points (word 0 of the result
//                  words; ordinary stores), then the row's draws, or its triple of `cuts` checked (word
//                  1).  (a, b, mode) go to the info scratch, the row's output length to the scan's input.
//   hipCUB scan    exclusive sum of the output lengths: O[r], the row's offset in the output stream;
//                  O[rows] = T_out.
//   k_fim_result   T_out beside words 0 and 1: one copy of three result words to the host, which
//                  checks them and the cap before anything is written.
//   k_fim_offsets  one thread per row: out_row_off from O, row_info from the info scratch.
//   k_fim_gather   output-centric: one workgroup per kTile output ids, 4 per lane.  The last row that
//                  begins at or before the tile is found with wave_upper_bound on O; then rounds of
//                  kStage rows staged in LDS (offset relative to the tile, source index, a, b, L, mode),
//                  as the pad / pack kernels stage theirs, so a tile of many short rows takes more
//                  rounds.  A lane finds the row of its first position by binary search in LDS and walks
//                  forward; the position's index in its row maps through (a, b, mode, L) to a sentinel
//                  or to one index in ids.  The sources of a row are at most three contiguous runs, so
//                  the lanes of a wave read consecutive ids but for the joins.  16-byte stores of
//                  out_ids and out_src and 4-byte stores of out_seg where the buffers are aligned.
//   k_fim_cuts     character-level cuts (shred_fim_cuts_device): one thread per document draws on the
//                  document's bytes, snaps both cuts back to a UTF-8 character's first byte (at most 3
//                  bytes read per cut) and writes the three piece offsets and the mode.  k_fim_docs
//                  checks doc_off before it, as k_docs_check does.
//
// Traffic per id: 4 B read (ids, k_fim_gather) and 4 B written (out_ids); 8 B more with out_src and 1 B
// more with out_seg.  Per row: 16 B read by k_fim_rows (24 B more with cuts), 24 B (info) and 8 B (the
// length) written, 8 + 8 B through the scan, 8 B (O) read and 8 B (out_row_off) written by
// k_fim_offsets (24 + 24 B more with row_info), and 8 + 8 + 24 B read by the tile that stages the row:
// about 130 B.  Per tile of 1024 output ids one wave search of O.
// All global indices are 64-bit; every global store is an ordinary vector store, and there is no atomic.
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
// beside the span-corruption unit's START and LEN
constexpr u64 kFimC = (1ull << 40) + 4, kCutA = (1ull << 40) + 5, kCutB = (1ull << 40) + 6, kMode = (1ull << 40) + 7;

__device__ __forceinline__ u64 mix64(u64 x) {  // murmur3's fmix64
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// What the kernels know of a call's options; passed by value.
struct FimRule {
  u64 seed, base;  // base: row_base + the index in the call's rows of the pass's first row
  u64 t_fim, t_spm;
  int64_t min_len;
  int32_t sent[3];  // pre_id, suf_id, mid_id

  __device__ __forceinline__ u64 draw(u64 x, u64 c) const { return mix64(mix64(seed + kGolden * (x + 1)) ^ c); }
  // The decisions of row (or document) r of L ids (bytes): -1 not transformed, else the mode, with the cuts.
  __device__ __forceinline__ int64_t decide(u64 r, u64 L, u64* a, u64* b) const {
    const u64 h = base + r;
    *a = *b = 0;
    if ((int64_t)L < min_len || (draw(h, kFimC) >> 32) >= t_fim) return -1;
    const u64 x = ((draw(h, kCutA) >> 32) * (L + 1)) >> 32, y = ((draw(h, kCutB) >> 32) * (L + 1)) >> 32;
    *a = x < y ? x : y, *b = x < y ? y : x;
    return (draw(h, kMode) >> 32) < t_spm ? 1 : 0;
  }
};

FimRule rule_of(const EncodeDevice::FimOpts& o, u64 first) {
  return FimRule{o.seed, o.row_base + first, o.t_fim, o.t_spm, o.min_len, {o.pre_id, o.suf_id, o.mid_id}};
}

// info: 3 int64 per row (a, b, mode, or -1 -1 -1); len: rows + 1 entries, the rows' output lengths and a 0.
__global__ __launch_bounds__(kThreads) void k_fim_rows(const int64_t* __restrict__ row, u64 rows, u64 n, FimRule rule,
                                                       const int64_t* __restrict__ cuts, int64_t* __restrict__ info,
                                                       u64* __restrict__ len, u64* __restrict__ res) {
  const u64 r = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (r > rows) return;
  const int64_t v = row[r];
  const int64_t prev = r ? row[r - 1] : 0;
  if (v < 0 || (u64)v > n || prev > v || (r == 0 && v != 0) || (r == rows && (u64)v != n)) res[0] = 1;
  if (r == rows) {
    len[r] = 0;
    return;
  }
  const int64_t Ls = row[r + 1] - v;
  const u64 L = Ls > 0 ? (u64)Ls : 0;  // a bad row_off: word 0 is set by this row's or the next one's thread
  u64 a = 0, b = 0;
  int64_t mode;
  if (cuts) {
    const int64_t ca = cuts[3 * r], cb = cuts[3 * r + 1], cm = cuts[3 * r + 2];
    mode = -1;
    if (ca == -1 && cb == -1 && cm == -1) {
    } else if (ca < 0 || ca > cb || (u64)cb > L || (cm != 0 && cm != 1)) {
      res[1] = 1;
    } else {
      a = (u64)ca, b = (u64)cb, mode = cm;
    }
  } else {
    mode = rule.decide(r, L, &a, &b);
  }
  info[3 * r] = mode < 0 ? -1 : (int64_t)a;
  info[3 * r + 1] = mode < 0 ? -1 : (int64_t)b;
  info[3 * r + 2] = mode;
  len[r] = L + (mode < 0 ? 0 : 3);
}

__global__ void k_fim_result(const u64* __restrict__ O, u64 rows, u64* __restrict__ res) { res[2] = O[rows]; }

// off0: added to every offset written to out_row (a piece of the host call).  row_info may be nullptr.
__global__ __launch_bounds__(kThreads) void k_fim_offsets(const u64* __restrict__ O, u64 rows, u64 off0,
                                                          const int64_t* __restrict__ info,
                                                          int64_t* __restrict__ out_row,
                                                          int64_t* __restrict__ row_info) {
  const u64 r = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (r > rows) return;
  out_row[r] = (int64_t)(off0 + O[r]);
  if (row_info && r < rows) {
    row_info[3 * r] = info[3 * r];
    row_info[3 * r + 1] = info[3 * r + 1];
    row_info[3 * r + 2] = info[3 * r + 2];
  }
}

// Position `off` of the output row of a row of L ids cut at a <= b: the index in the row that it copies
// and its segment (1 prefix, 2 suffix, 3 middle), or -1 - k for sentinel k (segment 4).  mode: 0 PSM,
// 1 SPM; a row that is not transformed does not come here.
__device__ __forceinline__ int64_t fim_source(u64 off, u64 a, u64 b, u64 L, int mode, uint32_t* seg) {
  const u64 tail = L - b;  // the suffix's ids
  *seg = 4;
  if (off == 0) return -1;
  if (mode == 0) {
    if (off <= a) return *seg = 1, (int64_t)(off - 1);
    if (off == a + 1) return -2;
    if (off < a + 2 + tail) return *seg = 2, (int64_t)(b + (off - a - 2));
    if (off == a + 2 + tail) return -3;
    return *seg = 3, (int64_t)(off - 3 - tail);  // a + (off - (a + 3 + tail))
  }
  if (off == 1) return -2;
  if (off < 2 + tail) return *seg = 2, (int64_t)(b + off - 2);
  if (off == 2 + tail) return -3;
  const u64 q = off - 3 - tail;  // prefix and middle follow each other in the row too
  return *seg = q < a ? 1 : 3, (int64_t)q;
}

// Positions [0, T) of the output stream, O[rows] = T >= 1.  src0: added to every out_src (a piece of
// the host call).  aligned: bit 0 out, bit 1 out_src may take 16-byte stores, bit 2 out_seg 4-byte ones.
__global__ __launch_bounds__(kThreads) void k_fim_gather(const int32_t* __restrict__ ids,
                                                         const int64_t* __restrict__ row, u64 rows,
                                                         const u64* __restrict__ O,
                                                         const int64_t* __restrict__ info, u64 T, FimRule rule,
                                                         u64 src0, int32_t* __restrict__ out,
                                                         int64_t* __restrict__ out_src, uint8_t* __restrict__ out_seg,
                                                         uint32_t aligned) {
  __shared__ int64_t s_rel[kStage + 1];  // O[k] - tile start, at most kTile
  __shared__ u64 s_src[kStage];          // index in ids of the row's first id
  __shared__ u64 s_a[kStage], s_b[kStage], s_len[kStage];
  __shared__ int8_t s_mode[kStage];
  __shared__ u64 s_k;
  const int tid = threadIdx.x;
  const u64 t0 = (u64)blockIdx.x * kTile;
  const int tlen = (int)(T - t0 < (u64)kTile ? T - t0 : (u64)kTile);
  if (tid < 64) {  // the last k with O[k] <= t0 (O[0] = 0): rows that emit nothing before it are passed over
    const u64 ub = wave_upper_bound(O, 0, rows + 1, t0, tid);
    if (tid == 0) s_k = ub - 1;
  }
  __syncthreads();
  u64 ks = s_k;
  const int p0 = tid * kLane;
  int32_t w[kLane];
  int64_t ws[kLane];
  uint32_t wg = 0;
#pragma unroll
  for (int i = 0; i < kLane; ++i) w[i] = 0, ws[i] = -1;
  int cur = 0;
  for (;;) {
    // entries ks .. ks + m - 1 (k == rows: the end, no row), and the offset of entry ks + m
    const int m = (int)(rows + 1 - ks < (u64)kStage ? rows + 1 - ks : (u64)kStage);
    for (int i = tid; i <= m; i += kThreads) {
      const u64 k = ks + (u64)i;
      int64_t rel = kTile;
      if (k <= rows) {
        rel = (int64_t)(O[k] - t0);
        rel = rel > kTile ? (int64_t)kTile : rel;
      }
      s_rel[i] = rel;
      if (i < m) {
        u64 src = 0, a = 0, b = 0, L = 0;
        int64_t mode = -1;
        if (k < rows) {
          src = (u64)row[k], L = (u64)row[k + 1] - src;
          mode = info[3 * k + 2];
          if (mode >= 0) a = (u64)info[3 * k], b = (u64)info[3 * k + 1];
        }
        s_src[i] = src, s_a[i] = a, s_b[i] = b, s_len[i] = L, s_mode[i] = (int8_t)mode;
      }
    }
    __syncthreads();
    // this round resolves the tile's positions [cur, lim): below the offset of the first entry not staged
    const int lim = s_rel[m] < (int64_t)tlen ? (int)s_rel[m] : tlen;
    const int lo = p0 > cur ? p0 : cur, hi = p0 + kLane < lim ? p0 + kLane : lim;
    if (lo < hi) {
      int x = 0, y = m;  // first entry past position lo
      while (x < y) {
        const int mid = (x + y) >> 1;
        if (s_rel[mid] <= (int64_t)lo) x = mid + 1; else y = mid;
      }
      int j = x - 1;  // >= 0: entry 0 starts at or before cur
#pragma unroll
      for (int i = 0; i < kLane; ++i) {
        const int p = p0 + i;
        if (p >= lo && p < hi && j >= 0) {
          while (j + 1 < m && s_rel[j + 1] <= (int64_t)p) ++j;
          const u64 off = (u64)((int64_t)p - s_rel[j]);  // the position's index in its output row
          const int mode = s_mode[j];
          const u64 L = s_len[j];
          if (off < L + (mode < 0 ? 0 : 3)) {  // (always, but for the end entry)
            uint32_t seg = 0;
            const int64_t from = mode < 0 ? (int64_t)off : fim_source(off, s_a[j], s_b[j], L, mode, &seg);
            if (from < 0) {
              w[i] = from == -1 ? rule.sent[0] : from == -2 ? rule.sent[1] : rule.sent[2];
            } else {
              w[i] = ids[s_src[j] + (u64)from];
              ws[i] = (int64_t)(src0 + s_src[j] + (u64)from);
            }
            wg |= seg << (8 * i);
          }
        }
      }
    }
    if (lim >= tlen) break;
    cur = lim;
    ks += (u64)m;
    __syncthreads();
  }
  if (p0 >= tlen) return;
  const u64 g = t0 + (u64)p0;
  const bool full = p0 + kLane <= tlen;
  if (full && (aligned & 1u)) {
    *reinterpret_cast<int4*>(out + g) = make_int4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int i = 0; i < kLane; ++i)
      if (p0 + i < tlen) out[g + i] = w[i];
  }
  if (out_src) {
    if (full && (aligned & 2u)) {
      *reinterpret_cast<longlong2*>(out_src + g) = make_longlong2(ws[0], ws[1]);
      *reinterpret_cast<longlong2*>(out_src + g + 2) = make_longlong2(ws[2], ws[3]);
    } else {
#pragma unroll
      for (int i = 0; i < kLane; ++i)
        if (p0 + i < tlen) out_src[g + i] = ws[i];
    }
  }
  if (out_seg) {
    if (full && (aligned & 4u)) {
      *reinterpret_cast<uint32_t*>(out_seg + g) = wg;
    } else {
#pragma unroll
      for (int i = 0; i < kLane; ++i)
        if (p0 + i < tlen) out_seg[g + i] = (uint8_t)(wg >> (8 * i));
    }
  }
}

// ---- character-level cuts ----

__global__ __launch_bounds__(kThreads) void k_fim_docs(const int64_t* __restrict__ doc_off, u64 docs, u64 n,
                                                       u64* __restrict__ res) {
  const u64 i = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (i > docs) return;
  const int64_t v = doc_off[i];
  bool bad = v < 0 || (u64)v > n || (i == 0 && v != 0) || (i == docs && (u64)v != n);
  if (!bad && i < docs) bad = v > doc_off[i + 1];
  if (bad) res[0] = 1;  // several threads may store at once, on purpose: all store the same value
}

// R >= 1 documents whose doc_off is good (nullptr: one document of n bytes).
__global__ __launch_bounds__(kThreads) void k_fim_cuts(const uint8_t* __restrict__ text, u64 n,
                                                       const int64_t* __restrict__ doc_off, u64 R, FimRule rule,
                                                       int64_t* __restrict__ piece_off, int8_t* __restrict__ doc_mode) {
  const u64 d = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (d > R) return;
  if (d == R) {
    piece_off[3 * R] = (int64_t)n;
    return;
  }
  const u64 s = doc_off ? (u64)doc_off[d] : 0, e = doc_off ? (u64)doc_off[d + 1] : n;
  const u64 B = e - s;
  u64 a, b;
  const int64_t mode = rule.decide(d, B, &a, &b);
  const auto snap = [&](u64 p) {
    for (int step = 0; step < 3 && p > 0 && p < B && (text[s + p] & 0xC0) == 0x80; ++step) --p;
    return p;
  };
  if (mode >= 0) {
    a = snap(a);
    b = snap(b);
    b = b < a ? a : b;
  }
  piece_off[3 * d] = (int64_t)s;
  piece_off[3 * d + 1] = (int64_t)(mode < 0 ? e : s + a);
  piece_off[3 * d + 2] = (int64_t)(mode < 0 ? e : s + b);
  doc_mode[d] = (int8_t)mode;
}

// One call's (or piece's) rows as the passes take them; every pointer on the device.
struct FimCall {
  const int32_t* ids;
  u64 n;
  const int64_t* row;  // R + 1 entries
  u64 R;
  const int64_t* cuts;  // nullptr: drawn
  FimRule rule;
  u64 src0, off0;
  int32_t* out;
  int64_t* out_row;
  int64_t* out_src;
  uint8_t* out_seg;
  int64_t* row_info;
};

// The FIM passes' state, allocated on the first FIM call: the result words, 48 B per row of the
// largest call (info, the output lengths and their scan), and the staging of the host path.
struct FimState : PassState {
  DeviceWords res;         // [0] a bad row_off / doc_off, [1] a bad cuts, [2] T_out
  PinnedWords host;        // the three; [3], [4]: the offsets {0, n} of a call without row_off
  EventSet<4> ev;
  DeviceBuf<int64_t> one;  // those offsets on the device
  DeviceBuf<int64_t> info; // 3 per row
  DeviceBuf<u64> len;      // rows + 1 output lengths, then their exclusive sum O
  DeviceBuf<uint8_t> tmp;  // hipCUB scan scratch
  DeviceBuf<int32_t> hids, hout;        // host path: a piece's ids and its stream
  DeviceBuf<int64_t> hsrc, hrow, hcuts; // out_src; the piece's row_off and out_row_off (2 x hrow.cap()); its cuts
  DeviceBuf<uint8_t> hseg;

  bool words() { return res.ensure(3) && host.ensure(5) && ev.ensure() && one.grow(2); }

  bool reserve(size_t rows) {
    if (!words() || !info.grow(3 * std::max<size_t>(rows, 1)) || !len.grow(rows + 1, 2)) return false;
    size_t bytes = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, len.get(), len.get() + len.cap(), (u64)rows + 1) != hipSuccess)
      return false;
    return tmp.grow(std::max<size_t>(bytes, 16));
  }

  u64* O() const { return len.get() + len.cap(); }

  // Without a row_off: one row of all ids.
  int one_row(u64 n, hipStream_t st) {
    host[3] = 0, host[4] = n;
    ENC_OK(hipMemcpyAsync(one.get(), host.get() + 3, 16, hipMemcpyHostToDevice, st));
    return 0;
  }

  // The passes up to the result words, which are in `host` when it returns: 0 or -1.
  int measure(const FimCall& c, hipStream_t st) {
    ENC_OK(hipMemsetAsync(res.get(), 0, 24, st));
    k_fim_rows<<<dim3((unsigned)((c.R + kThreads) / kThreads)), dim3(kThreads), 0, st>>>(
        c.row, c.R, c.n, c.rule, c.cuts, info.get(), len.get(), res.get());
    ENC_OK(hipGetLastError());
    size_t bytes = tmp.cap();
    ENC_OK(hipcub::DeviceScan::ExclusiveSum(tmp.get(), bytes, len.get(), O(), c.R + 1, st));
    k_fim_result<<<dim3(1), dim3(1), 0, st>>>(O(), c.R, res.get());
    ENC_OK(hipGetLastError());
    ENC_OK(hipMemcpyAsync(host.get(), res.get(), 24, hipMemcpyDeviceToHost, st));
    ENC_OK(hipStreamSynchronize(st));
    return 0;
  }

  // The outputs, after measure() on the same call found T ids and no error: 0 or -1.
  int expand(const FimCall& c, u64 T, hipStream_t st) {
    k_fim_offsets<<<dim3((unsigned)((c.R + kThreads) / kThreads)), dim3(kThreads), 0, st>>>(
        O(), c.R, c.off0, info.get(), c.out_row, c.row_info);
    ENC_OK(hipGetLastError());
    if (!T) return 0;
    const uint32_t aligned = (aligned16(c.out) ? 1u : 0u) | (aligned16(c.out_src) ? 2u : 0u) |
                             ((reinterpret_cast<uintptr_t>(c.out_seg) & 3) == 0 ? 4u : 0u);
    k_fim_gather<<<dim3((unsigned)((T + kTile - 1) / kTile)), dim3(kThreads), 0, st>>>(
        c.ids, c.row, c.R, O(), info.get(), T, c.rule, c.src0, c.out, c.out_src, c.out_seg, aligned);
    ENC_OK(hipGetLastError());
    return 0;
  }

  // Staging of a piece of n ids and m rows.
  bool stage(size_t n, size_t m, bool cuts, bool src, bool seg) {
    const size_t cap = n + 3 * m;
    return reserve(m) && hids.grow(std::max<size_t>(n, 1)) && hout.grow(cap) && hrow.grow(m + 1, 2) &&
           (!cuts || hcuts.grow(3 * m)) && (!src || hsrc.grow(cap)) && (!seg || hseg.grow(cap));
  }
};

}  // namespace

int64_t EncodeDevice::fim(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const FimOpts& o,
                          const int64_t* cuts, int32_t* out_ids, size_t out_cap, int64_t* out_row_off,
                          int64_t* out_src, uint8_t* out_seg, int64_t* row_info, void* stream, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  if (!tiles_fit(n)) return -1;
  const u64 R = row_off ? rows : 1;
  FimCall c{ids, n, row_off, R, cuts, rule_of(o, 0), 0, 0, out_ids, out_row_off, out_src, out_seg, row_info};
  u64 T = 0;
  return device_call<FimState>(
      pass_[kFim], device_, stream ? stream : stream_, "fim", R, kernel_ms,
      [&](FimState& fs, hipStream_t st, Plan* p) {
        if (!row_off) {
          if (fs.one_row(n, st) < 0) return -1;
          c.row = fs.one.get();
        }
        if (fs.measure(c, st) < 0) return -1;
        if (fs.host[0]) return -6;
        if (fs.host[1]) return -8;
        T = fs.host[2];
        *p = Plan{(int64_t)T, out_ids && out_cap >= T, T};
        return 0;
      },
      [&](FimState& fs, hipStream_t st) { return fs.expand(c, T, st); });
}

// Host rows in pieces of whole rows (piece_end).  A piece is the device passes on its own rows at
// row_base + its first row, with its slice of cuts; its stream lands in the piece's staging at 0 and
// is copied behind the earlier pieces', and its offsets and out_src are written with the piece's
// bases added.  The caller has validated row_off and cuts.  A cap that holds the bound (n + 3 rows)
// needs one round; a smaller one a round of counts first, so that nothing is written when it does
// not suffice.
int64_t EncodeDevice::fim_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const FimOpts& o,
                               const int64_t* cuts, int32_t* out_ids, size_t out_cap, int64_t* out_row_off,
                               int64_t* out_src, uint8_t* out_seg, int64_t* row_info) {
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  FimState& fs = pass_state<FimState>(pass_[kFim]);
  if (!fs.words()) {
    std::fprintf(stderr, "[ERROR]\t encoder: fim allocation failed\n");
    return -1;
  }
  hipStream_t st = (hipStream_t)stream_;
  const size_t R = row_off ? rows : 1, piece = piece_ids();
  const HostIn in{ids, n, row_off};
  std::vector<int64_t> local;
  u64 total = 0;
  const auto round = [&](bool write) -> int {
    total = 0;
    for (size_t r0 = 0; r0 < R;) {
      u64 emitted = 0;
      const size_t r1 = piece_end(&in, 1, R, r0, piece, 0, [](size_t) { return (u64)0; }, &emitted, nullptr);
      const size_t a = row_off ? (size_t)row_off[r0] : 0, len = (row_off ? (size_t)row_off[r1] : n) - a, m = r1 - r0;
      if (!tiles_fit(len + 3 * m) || !fs.stage(len, m, cuts != nullptr, write && out_src, write && out_seg)) {
        std::fprintf(stderr, "[ERROR]\t encoder: fim staging allocation failed (%zu ids, %zu rows)\n", len, m);
        return -1;
      }
      int64_t *const drow = fs.hrow.get(), *const dout_row = drow + fs.hrow.cap();
      if (len) ENC_OK(hipMemcpyAsync(fs.hids.get(), ids + a, len * 4, hipMemcpyHostToDevice, st));
      local.resize(m + 1);
      for (size_t i = 0; i <= m; ++i) local[i] = row_off ? row_off[r0 + i] - (int64_t)a : (int64_t)(i ? n : 0);
      ENC_OK(hipMemcpyAsync(drow, local.data(), (m + 1) * 8, hipMemcpyHostToDevice, st));
      if (cuts) ENC_OK(hipMemcpyAsync(fs.hcuts.get(), cuts + 3 * r0, m * 24, hipMemcpyHostToDevice, st));
      const FimCall c{fs.hids.get(), len, drow, m, cuts ? fs.hcuts.get() : nullptr, rule_of(o, r0), a, total,
                      fs.hout.get(), dout_row, write && out_src ? fs.hsrc.get() : nullptr,
                      write && out_seg ? fs.hseg.get() : nullptr, nullptr};
      if (fs.measure(c, st) < 0) return -1;
      const u64 T = fs.host[2];
      if (write) {
        if (fs.expand(c, T, st) < 0) return -1;
        if (T) ENC_OK(hipMemcpyAsync(out_ids + total, fs.hout.get(), T * 4, hipMemcpyDeviceToHost, st));
        if (T && out_src) ENC_OK(hipMemcpyAsync(out_src + total, fs.hsrc.get(), T * 8, hipMemcpyDeviceToHost, st));
        if (T && out_seg) ENC_OK(hipMemcpyAsync(out_seg + total, fs.hseg.get(), T, hipMemcpyDeviceToHost, st));
        ENC_OK(hipMemcpyAsync(out_row_off + r0, dout_row, (m + 1) * 8, hipMemcpyDeviceToHost, st));
        if (row_info) ENC_OK(hipMemcpyAsync(row_info + 3 * r0, fs.info.get(), m * 24, hipMemcpyDeviceToHost, st));
        ENC_OK(hipStreamSynchronize(st));
      }
      total += T;
      r0 = r1;
    }
    return 0;
  };
  if (!(out_ids && out_cap >= n + 3 * (u64)R)) {
    if (round(false) < 0) return -1;
    if (!out_ids || out_cap < total) return (int64_t)total;
  }
  if (round(true) < 0) return -1;
  return (int64_t)total;
}

int EncodeDevice::fim_cuts(const uint8_t* text, size_t n, const int64_t* doc_off, size_t docs, const FimOpts& o,
                           int64_t* piece_off, int8_t* doc_mode, void* stream, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  const u64 R = doc_off ? docs : 1;
  if (!batch_rows_fit(R)) return -1;
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  FimState& fs = pass_state<FimState>(pass_[kFim]);
  if (!fs.words()) {
    std::fprintf(stderr, "[ERROR]\t encoder: fim allocation failed\n");
    return -1;
  }
  hipStream_t st = (hipStream_t)(stream ? stream : stream_);
  const dim3 grid((unsigned)((R + kThreads) / kThreads));
  ENC_OK(hipEventRecord(fs.ev[0], st));
  if (doc_off) {
    ENC_OK(hipMemsetAsync(fs.res.get(), 0, 8, st));
    k_fim_docs<<<grid, dim3(kThreads), 0, st>>>(doc_off, R, n, fs.res.get());
    ENC_OK(hipGetLastError());
    ENC_OK(hipMemcpyAsync(fs.host.get(), fs.res.get(), 8, hipMemcpyDeviceToHost, st));
    ENC_OK(hipStreamSynchronize(st));
    if (fs.host[0]) return -6;
  }
  k_fim_cuts<<<grid, dim3(kThreads), 0, st>>>(text, n, doc_off, R, rule_of(o, 0), piece_off, doc_mode);
  ENC_OK(hipGetLastError());
  ENC_OK(hipEventRecord(fs.ev[1], st));
  ENC_OK(hipStreamSynchronize(st));
  if (kernel_ms) ENC_OK(fs.ev.sum_ms(1, kernel_ms));
  return 0;
}

}  // namespace shred
