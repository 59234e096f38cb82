// Rows of token ids to rectangular model inputs on gfx950: padded batches, packed sequences and
// overlapping windows of long rows (C ABI and definitions: include/shredword_encode.h,
// shred_pad_* / shred_pack_* / shred_window_*).  The passes use
// none of the encoder's or the decoder's kernels.  The pair form (shred_pair_*) is batch_pair.hip;
// what the two units share is batch_common.h (device: tile geometry, the wave search) and
// batch_state.h (host: the length pass, the device-call driver, the host piece loop).
//
// Row r keeps keep_r of its len_r ids (from either end) and emits e_r = add + keep_r ids: an
// optional bos, the kept ids, an optional eos.  E is the exclusive prefix sum of e_r, E[rows] = T.
//
//   k_bat_rows       one thread per row_off entry: range, order and end points, and e_r <= INT32_MAX
//                    (error words, ordinary stores, no atomics);
//   hipCUB scan      pack only: E[0 .. rows] (batch_state.h);
//   hipCUB reduce    pad only: the maximum of e_r (the width needed);
//   k_bat_pad        output-centric: one workgroup per kTile consecutive entries of the flat [rows, W]
//                    array, 4 consecutive entries per lane.  The 64-bit (r, c) split of a lane's first
//                    entry is done once and then walked (++c, a new row's offsets at c == W), so a
//                    lane's entries may straddle rows.  The lane that owns c == 0 writes lengths[r];
//                    the mask bytes come from the same walk.  Pad needs no E and no staging: entry
//                    (r, c) depends on row r alone;
//   k_bat_row_start  pack: row_start[r] = base + E[r];
//   k_bat_pack       stream-centric: one workgroup per kTile stream positions.  Its first row by a
//                    binary search of E: the last r with E[r] <= the tile's first position, which skips
//                    the rows that emit nothing.  Rounds of kStage rows staged in LDS (E relative to the
//                    tile, e_r, the index in ids of the row's emitted id 0); every lane makes 4
//                    consecutive positions: a binary search of the LDS offsets for the row under its
//                    first position, then a forward walk.  A round resolves the positions below the E of
//                    the first row it did not stage, so a tile with more rows than kStage (rows that
//                    emit nothing, rows of one id) takes more rounds, and a row longer than a tile
//                    needs no special case.  Entry `rows` of E is staged as a row that emits nothing:
//                    every position no row covers is padding (pos 0, seg -1).
//
// Traffic per output entry.  Pad at fill f = sum e_r / (rows W): writes 4, reads 4 f (the ids):
// 4 + 4 f bytes, + 1 with the mask; per row 8 (row pass) + 8 (reduce) = 16 B, and each lane reads
// the two offsets of every row it touches through the caches.  Pack: reads 4 (ids), writes 4: 8
// bytes, + 4 each for pos and seg; per row 8 (row pass) + 8 (scan reads row_off) = 16 B, and E is
// written once and read back with row_off by the tiles (24 B per row, through the caches).
//
// Windows (shred_window_*): row r is cut into w_r overlapping windows of at most C = max_len - add
// ids, step = C - stride ids apart; WO is the exclusive prefix sum of w_r, WO[rows] = Wn, and it is
// strictly increasing, since every row has a window.
//
//   k_bat_rows       as above, with keep_max = C: e_r is then the length of row r's first window;
//   hipCUB scan      inclusive sum over k = 0 .. rows of (k ? w_{k-1} : 0): WO[0 .. rows];
//   hipCUB reduce    the maximum of e_r: the longest window (a row's first is its longest);
//   k_bat_row_start  row_win[r] = WO[r];
//   k_bat_window     output-centric like k_bat_pad: one workgroup per kTile consecutive entries of
//                    the flat [Wn, W] array, 4 consecutive entries per lane, the (window, column)
//                    split of a lane's first entry done once and then walked.  The row of the tile's
//                    first window by one search of WO per workgroup (its first wave probes 64
//                    entries a step); then rounds of kStage rows staged in LDS as k_bat_pack stages
//                    them (WO relative to the tile's first window, the index in ids that the row's
//                    window at the tile's first window would start at, the row's end).  A lane finds
//                    the row under its first entry by a binary search of the LDS offsets and walks
//                    forward.  A tile of narrow windows can hold more than kStage rows and takes
//                    more rounds; a row whose windows cover many tiles needs no special case.  The
//                    lane that owns column 0 of a window writes its lengths, win_row and win_src;
//   k_bat_window_meta  W == 0 only (rows that are all empty, nothing added): no lane owns a column,
//                    so one thread per window writes the three.
//
// Window traffic per output entry is pad's: 4 + 4 f bytes at fill f = sum e / (Wn W), + 1 with the
// mask; per window 4 (lengths) + 4 (win_row) + 8 (win_src) = 16 B for those asked for; per row 8
// (row pass) + 8 (scan) + 8 (reduce) reads of row_off, 8 written for WO and 8 for row_win, and the
// tiles read WO and row_off back through the caches.
// All global indices are 64-bit; every store is an ordinary vector store.  Output pointers are
// only element-aligned (tensor views), so the 16-byte (mask: 4-byte) stores have a scalar form.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../host/encoder.h"
#include "batch_common.h"
#include "batch_state.h"
#include "encode_common.h"

namespace shred {
namespace {

// One call's (or piece's) rows, as the kernels take them.
struct BatchCall {
  const int32_t* ids;
  uint64_t n;
  const int64_t* row;  // nullptr: one row of all ids (rows == 1); else rows + 1 entries
  uint64_t rows;
  bool ends;           // check row[0] == 0 and row[rows] == n (a piece's local offsets: no)
  EncodeDevice::BatchOpts o;
  uint64_t base;       // pack: stream offset of the call's first row (ids of the pieces before);
                       // window: index in the call's ids of the piece's first id
  uint64_t row_base;   // index of the call's first row
};

// How a row turns into its emitted row; passed to the kernels and the hipCUB iterators by value.
struct Rows {
  const int64_t* row;  // nullptr: the one row [0, n)
  u64 n;
  u64 keep_max;        // most ids a row keeps: max_len - add, or kNoLimit
  uint32_t bos_n, eos_n, left;
  int32_t bos, eos;
  __host__ __device__ __forceinline__ void bounds(u64 r, u64* a, u64* b) const {
    *a = row ? (u64)row[r] : 0;
    *b = row ? (u64)row[r + 1] : n;
  }
  __host__ __device__ __forceinline__ u64 keep(u64 a, u64 b) const { return b - a < keep_max ? b - a : keep_max; }
  __host__ __device__ __forceinline__ u64 emit(u64 r) const {
    u64 a, b;
    bounds(r, &a, &b);
    return (u64)(bos_n + eos_n) + keep(a, b);
  }
  // e_r, and the index in ids that emitted id j = 0 would have (the bos sits there, if any): emitted
  // id j in [bos_n, e_r - eos_n) is ids[src + j].
  __device__ __forceinline__ void span(u64 r, u64* e, u64* src) const {
    u64 a, b;
    bounds(r, &a, &b);
    const u64 k = keep(a, b);
    *e = (u64)(bos_n + eos_n) + k;
    *src = (left ? b - k : a) - (u64)bos_n;
  }
  __device__ __forceinline__ int32_t id(const int32_t* __restrict__ ids, u64 e, u64 src, u64 j) const {
    return j < (u64)bos_n ? bos : (eos_n && j == e - 1) ? eos : ids[src + j];
  }
};

Rows rows_of(const EncodeDevice::BatchOpts& o, const int64_t* row, u64 n) {
  const uint32_t b = o.has_bos ? 1u : 0u, e = o.has_eos ? 1u : 0u;
  return Rows{row, n, o.max_len ? o.max_len - (b + e) : kNoLimit, b, e, o.trunc_side ? 1u : 0u, o.bos, o.eos};
}

__global__ __launch_bounds__(kThreads) void k_bat_rows(Rows rw, u64 rows, int ends, u64* __restrict__ err) {
  const u64 r = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (r > rows) return;
  const int64_t v = rw.row[r];
  const int64_t prev = r ? rw.row[r - 1] : 0;
  bool bad = v < 0 || (u64)v > rw.n || prev > v;
  if (ends && ((r == 0 && v != 0) || (r == rows && (u64)v != rw.n))) bad = true;
  if (bad) {
    err[0] = 1;
    return;
  }
  if (r && prev >= 0 && (u64)(rw.bos_n + rw.eos_n) + rw.keep((u64)prev, (u64)v) > (u64)INT32_MAX) err[1] = 1;
}

// The row pass of the pad, pack and window calls (0 or -1).
int row_pass(const Rows& rw, const BatchCall& c, u64* err, hipStream_t st) {
  if (!c.row) return rw.emit(0) > (u64)INT32_MAX ? -1 : 0;
  k_bat_rows<<<dim3((unsigned)((c.rows + kThreads) / kThreads)), dim3(kThreads), 0, st>>>(rw, c.rows, c.ends ? 1 : 0,
                                                                                          err);
  ENC_OK(hipGetLastError());
  return 0;
}

// Element k of the scan: the length of emitted row k - 1; element r of the reduction: that of row r.
struct EInput {
  Rows rw;
  __host__ __device__ __forceinline__ u64 operator()(u64 k) const { return k ? rw.emit(k - 1) : 0ull; }
};
struct WInput {
  Rows rw;
  __host__ __device__ __forceinline__ u64 operator()(u64 r) const { return rw.emit(r); }
};

// First k in [lo, hi) with E[k] > v, or hi.
__device__ __forceinline__ u64 upper_bound(const u64* __restrict__ E, u64 lo, u64 hi, u64 v) {
  while (lo < hi) {
    const u64 mid = lo + ((hi - lo) >> 1);
    if (E[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// total = rows * W > 0, W >= every e_r.
template <bool kAligned>
__global__ __launch_bounds__(kThreads) void k_bat_pad(const int32_t* __restrict__ ids, Rows rw, u64 W, u64 total,
                                                      int32_t pad_id, uint32_t pad_left, int32_t* __restrict__ out,
                                                      int32_t* __restrict__ lengths, uint8_t* __restrict__ mask,
                                                      uint32_t mask_aligned) {
  const u64 g = (u64)blockIdx.x * kTile + (u64)threadIdx.x * kLane;
  if (g >= total) return;
  const int cnt = total - g < (u64)kLane ? (int)(total - g) : kLane;
  u64 r = g / W, c = g - r * W;
  u64 e = 0, src = 0, lead = 0;
  bool fresh = true;
  int32_t w[kLane] = {0, 0, 0, 0};
  uint32_t mk = 0;
#pragma unroll
  for (int i = 0; i < kLane; ++i) {
    if (i < cnt) {
      if (fresh) {
        rw.span(r, &e, &src);
        lead = pad_left ? W - e : 0;
        if (c == 0 && lengths) lengths[r] = (int32_t)e;
        fresh = false;
      }
      int32_t v = pad_id;
      if (c >= lead && c - lead < e) {
        v = rw.id(ids, e, src, c - lead);
        mk |= 1u << (8 * i);
      }
      w[i] = v;
      if (++c == W) {
        c = 0;
        ++r;
        fresh = true;
      }
    }
  }
  if (kAligned && cnt == kLane) {
    *reinterpret_cast<int4*>(out + g) = make_int4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int i = 0; i < kLane; ++i)
      if (i < cnt) out[g + i] = w[i];
  }
  if (mask) {
    if (mask_aligned && cnt == kLane) {
      *reinterpret_cast<uint32_t*>(mask + g) = mk;
    } else {
#pragma unroll
      for (int i = 0; i < kLane; ++i)
        if (i < cnt) mask[g + i] = (uint8_t)(mk >> (8 * i));
    }
  }
}

// Positions [0, limit) of the call's stream (E[rows] = T; positions from T on are padding);
// aligned: bit 0 out, bit 1 pos, bit 2 seg may take 16-byte stores.
__global__ __launch_bounds__(kThreads) void k_bat_pack(const int32_t* __restrict__ ids, Rows rw, u64 rows,
                                                       const u64* __restrict__ E, u64 limit, int32_t pad_id,
                                                       u64 row_base, int32_t* __restrict__ out,
                                                       int32_t* __restrict__ pos, int32_t* __restrict__ seg,
                                                       uint32_t aligned) {
  __shared__ int32_t s_rel[kStage + 1];  // E[k] - tile start, clamped to [-INT32_MAX, kTile]
  __shared__ int32_t s_e[kStage];        // e_k (0 for the end entry k == rows)
  __shared__ int64_t s_src[kStage];      // index in ids of the row's emitted id 0
  __shared__ u64 s_k;
  const int tid = threadIdx.x;
  const u64 t0 = (u64)blockIdx.x * kTile;
  const int tlen = (int)(limit - t0 < (u64)kTile ? limit - t0 : (u64)kTile);
  if (tid == 0) {  // the last k with E[k] <= t0 (E[0] = 0); k == rows when the tile is all padding
    const u64 ub = upper_bound(E, 0, rows + 1, t0);
    s_k = ub ? ub - 1 : 0;
  }
  __syncthreads();
  u64 ks = s_k;
  const int p0 = tid * kLane;
  int32_t w[kLane], wp[kLane], ws[kLane];
#pragma unroll
  for (int i = 0; i < kLane; ++i) {
    w[i] = pad_id;
    wp[i] = 0;
    ws[i] = -1;
  }
  int cur = 0;
  for (;;) {
    // entries ks .. ks + m - 1 (k == rows: the end, no row), and the offset of entry ks + m
    const int m = (int)(rows + 1 - ks < (u64)kStage ? rows + 1 - ks : (u64)kStage);
    for (int i = tid; i <= m; i += kThreads) {
      const u64 k = ks + (u64)i;
      int64_t rel = kTile;
      if (k <= rows) {
        rel = (int64_t)(E[k] - t0);
        rel = rel < -(int64_t)INT32_MAX ? -(int64_t)INT32_MAX : rel > kTile ? (int64_t)kTile : rel;
      }
      s_rel[i] = (int32_t)rel;
      if (i < m) {
        u64 e = 0, src = 0;
        if (k < rows) rw.span(k, &e, &src);
        s_e[i] = (int32_t)e;  // <= INT32_MAX (k_bat_rows)
        s_src[i] = (int64_t)src;
      }
    }
    __syncthreads();
    // this round resolves the tile's positions [cur, lim): below the offset of the first entry not staged
    const int lim = s_rel[m] < tlen ? s_rel[m] : tlen;
    const int lo = p0 > cur ? p0 : cur, hi = p0 + kLane < lim ? p0 + kLane : lim;
    if (lo < hi) {
      int a = 0, b = m;  // first entry past position lo
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (s_rel[mid] <= lo) a = mid + 1; else b = mid;
      }
      int j = a - 1;  // >= 0: entry 0 starts at or before cur
#pragma unroll
      for (int i = 0; i < kLane; ++i) {
        const int p = p0 + i;
        if (p >= lo && p < hi && j >= 0) {
          while (j + 1 < m && s_rel[j + 1] <= p) ++j;
          const uint32_t off = (uint32_t)p - (uint32_t)s_rel[j];  // the position's index in its emitted row
          const uint32_t e = (uint32_t)s_e[j];
          if (off < e) {
            w[i] = rw.id(ids, (u64)e, (u64)s_src[j], (u64)off);
            wp[i] = (int32_t)off;
            ws[i] = (int32_t)(row_base + ks + (u64)j);
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
  if (pos) {
    if (full && (aligned & 2u)) {
      *reinterpret_cast<int4*>(pos + g) = make_int4(wp[0], wp[1], wp[2], wp[3]);
    } else {
#pragma unroll
      for (int i = 0; i < kLane; ++i)
        if (p0 + i < tlen) pos[g + i] = wp[i];
    }
  }
  if (seg) {
    if (full && (aligned & 4u)) {
      *reinterpret_cast<int4*>(seg + g) = make_int4(ws[0], ws[1], ws[2], ws[3]);
    } else {
#pragma unroll
      for (int i = 0; i < kLane; ++i)
        if (p0 + i < tlen) seg[g + i] = ws[i];
    }
  }
}

// How a row turns into its windows.  rw.keep_max is C (never kNoLimit), so rw.emit(r) is the length
// of row r's first window; rw.left is 0.
struct Windows {
  Rows rw;
  u64 step;  // C - stride >= 1
  __host__ __device__ __forceinline__ u64 count(u64 r) const {
    u64 a, b;
    rw.bounds(r, &a, &b);
    return window_count(b - a, rw.keep_max, step);
  }
};

Windows windows_of(const EncodeDevice::BatchOpts& o, u64 stride, const int64_t* row, u64 n) {
  const Rows rw = rows_of(o, row, n);
  return Windows{rw, rw.keep_max - stride};
}

// Element k of the scan: the window count of row k - 1.
struct WOInput {
  Windows wn;
  __host__ __device__ __forceinline__ u64 operator()(u64 k) const { return k ? wn.count(k - 1) : 0ull; }
};

// total = Wn * W > 0, W >= every window's length; WO: rows + 1 entries, strictly increasing from 0
// to Wn.  Window w of the call goes to out[w * W ..], lengths[w], win_row[w], win_src[w].
template <bool kAligned>
__global__ __launch_bounds__(kThreads) void k_bat_window(const int32_t* __restrict__ ids, Windows wn, u64 rows,
                                                         const u64* __restrict__ WO, u64 W, u64 total, int32_t pad_id,
                                                         uint32_t pad_left, u64 row_base, u64 id_base,
                                                         int32_t* __restrict__ out, int32_t* __restrict__ lengths,
                                                         uint8_t* __restrict__ mask, uint32_t mask_aligned,
                                                         int32_t* __restrict__ win_row, int64_t* __restrict__ win_src) {
  __shared__ int32_t s_w[kStage + 1];  // WO[k] - the tile's first window, clamped to [-INT32_MAX, kTile + 1]
  __shared__ u64 s_src[kStage];        // index in ids at which the row's window at the tile's first window
                                       // starts (modulo 2^64: rows that begin later lie before their ids)
  __shared__ u64 s_end[kStage];        // the row's end in ids
  __shared__ u64 s_k;
  const int tid = threadIdx.x;
  const u64 t0 = (u64)blockIdx.x * kTile;
  const int tlen = (int)(total - t0 < (u64)kTile ? total - t0 : (u64)kTile);
  const u64 w0 = t0 / W, c0 = t0 - w0 * W;                // the tile's first entry: window, column
  const int wlast = (int)((c0 + (u64)(tlen - 1)) / W);    // its last entry's window, relative to w0
  if (tid < 64) {  // the row of window w0: the last k with WO[k] <= w0 (WO[0] = 0, WO[rows] = Wn > w0)
    const u64 ub = wave_upper_bound(WO, 0, rows + 1, w0, tid);
    if (tid == 0) s_k = ub == 0 ? 0 : ub > rows ? rows - 1 : ub - 1;
  }
  __syncthreads();
  u64 ks = s_k;
  const int p0 = tid * kLane;
  const int cnt = p0 >= tlen ? 0 : tlen - p0 < kLane ? tlen - p0 : kLane;
  const u64 first = c0 + (u64)p0;
  const int wr0 = (int)(first / W);  // the lane's first entry: window relative to w0 (<= kTile), column
  const u64 cl0 = first - (u64)wr0 * W;
  const u64 add = (u64)(wn.rw.bos_n + wn.rw.eos_n);
  int32_t v[kLane] = {pad_id, pad_id, pad_id, pad_id};
  uint32_t mk = 0;
  for (;;) {
    // rows ks .. ks + m - 1, and the offset of row ks + m (k == rows: Wn)
    const int m = (int)(rows - ks < (u64)kStage ? rows - ks : (u64)kStage);
    for (int i = tid; i <= m; i += kThreads) {
      const u64 k = ks + (u64)i;
      const int64_t rel = (int64_t)(WO[k] - w0);
      s_w[i] = (int32_t)(rel < -(int64_t)INT32_MAX ? -(int64_t)INT32_MAX : rel > kTile + 1 ? (int64_t)(kTile + 1) : rel);
      if (i < m) {
        u64 a, b;
        wn.rw.bounds(k, &a, &b);
        s_src[i] = a - (u64)rel * wn.step;
        s_end[i] = b;
      }
    }
    __syncthreads();
    // this round resolves the windows [from, lim) relative to w0: those of the staged rows
    const int from = s_w[0], lim = s_w[m];
    int wr = wr0, j = -1;
    u64 c = cl0, start = 0, e = 0, lead = 0;
    bool fresh = true;
#pragma unroll
    for (int i = 0; i < kLane; ++i) {
      if (i < cnt && wr >= from && wr < lim) {
        if (fresh) {
          if (j < 0) {  // the last staged row that starts at or before window wr
            int a = 0, b = m;
            while (a < b) {
              const int mid = (a + b) >> 1;
              if (s_w[mid] <= wr) a = mid + 1; else b = mid;
            }
            j = a - 1;  // >= 0: s_w[0] = from <= wr
          } else {
            while (j + 1 < m && s_w[j + 1] <= wr) ++j;
          }
          start = s_src[j] + (u64)wr * wn.step;
          const u64 left = s_end[j] - start;
          e = add + (left < wn.rw.keep_max ? left : wn.rw.keep_max);
          lead = pad_left ? W - e : 0;
          fresh = false;
          if (c == 0) {
            const u64 w = w0 + (u64)wr;
            if (lengths) lengths[w] = (int32_t)e;
            if (win_row) win_row[w] = (int32_t)(row_base + ks + (u64)j);
            if (win_src) win_src[w] = (int64_t)(id_base + start);
          }
        }
        if (c >= lead && c - lead < e) {
          v[i] = wn.rw.id(ids, e, start - (u64)wn.rw.bos_n, c - lead);
          mk |= 1u << (8 * i);
        }
      }
      if (++c == W) {
        c = 0;
        ++wr;
        fresh = true;
      }
    }
    if (lim > wlast || ks + (u64)m >= rows) break;
    ks += (u64)m;
    __syncthreads();
  }
  if (cnt == 0) return;
  const u64 g = t0 + (u64)p0;
  if (kAligned && cnt == kLane) {
    *reinterpret_cast<int4*>(out + g) = make_int4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < kLane; ++i)
      if (i < cnt) out[g + i] = v[i];
  }
  if (mask) {
    if (mask_aligned && cnt == kLane) {
      *reinterpret_cast<uint32_t*>(mask + g) = mk;
    } else {
#pragma unroll
      for (int i = 0; i < kLane; ++i)
        if (i < cnt) mask[g + i] = (uint8_t)(mk >> (8 * i));
    }
  }
}

// W == 0: every row is empty and nothing is added, so window r is row r and holds nothing.
__global__ __launch_bounds__(kThreads) void k_bat_window_meta(Rows rw, u64 rows, u64 row_base, u64 id_base,
                                                              int32_t* __restrict__ lengths,
                                                              int32_t* __restrict__ win_row,
                                                              int64_t* __restrict__ win_src) {
  const u64 r = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (r >= rows) return;
  u64 a, b;
  rw.bounds(r, &a, &b);
  if (lengths) lengths[r] = 0;
  if (win_row) win_row[r] = (int32_t)(row_base + r);
  if (win_src) win_src[r] = (int64_t)(id_base + a);
}

// Pad needs no state: entry (r, c) depends on row r alone.
int pad_expand(const BatchCall& c, uint64_t width, int32_t pad_id, int pad_side, int32_t* out, int32_t* lengths,
               uint8_t* mask, hipStream_t st) {
  const u64 total = c.rows * width;
  if (!total) {  // width == 0: every e_r is 0 and no lane owns a column
    if (lengths && c.rows) ENC_OK(hipMemsetAsync(lengths, 0, c.rows * 4, st));
    return 0;
  }
  const Rows rw = rows_of(c.o, c.row, c.n);
  const u64 tiles = (total + kTile - 1) / kTile;
  (aligned16(out) ? k_bat_pad<true> : k_bat_pad<false>)<<<dim3((unsigned)tiles), dim3(kThreads), 0, st>>>(
      c.ids, rw, width, total, pad_id, pad_side ? 1u : 0u, out, lengths, mask,
      (reinterpret_cast<uintptr_t>(mask) & 3) == 0 ? 1u : 0u);
  ENC_OK(hipGetLastError());
  return 0;
}

// The batch passes' state, allocated on the first pad / pack call: the length pass (sum is E) and
// the staging of the pad, pack and window host paths.
struct BatchState : LengthState {
  // host-path staging: ids; row offsets then row_start (2 x hrow.cap()); a piece's int32 outputs:
  // out, then pos / lengths, then seg / win_row (3 x hout.cap()); its mask
  DeviceBuf<int32_t> hids;
  DeviceBuf<int64_t> hrow;
  DeviceBuf<int32_t> hout;
  DeviceBuf<uint8_t> hmask;

  bool reserve(size_t rows) {
    const Rows rw{nullptr, 0, kNoLimit, 0, 0, 0, 0, 0};
    return LengthState::reserve(rows, row_iter(EInput{rw}), row_iter(WInput{rw}));
  }

  // Row checks (when c.row), then E into sum (scan) or the maximum of e_r over c's rows: 0, -1, -6.
  int lengths(const BatchCall& c, bool scan, hipStream_t st, uint64_t* total, uint64_t* widest) {
    const Rows rw = rows_of(c.o, c.row, c.n);
    const auto scan_in = row_iter(EInput{rw});
    const auto max_in = row_iter(WInput{rw});
    return measure(c.rows, [&](u64* err) { return row_pass(rw, c, err, st); }, scan ? &scan_in : nullptr,
                   scan ? nullptr : &max_in, st, total, widest);
  }

  // Stream positions [c.base, c.base + limit) into out / pos / seg (which point at position
  // c.base), pad_id from the rows' end on; row_start[r] = c.base + E[r] for the call's rows.
  int pack_expand(const BatchCall& c, uint64_t limit, int32_t pad_id, int32_t* out, int32_t* pos, int32_t* seg,
                  int64_t* row_start, hipStream_t st) {
    if (row_start) {
      k_bat_row_start<<<dim3((unsigned)((c.rows + kThreads) / kThreads)), dim3(kThreads), 0, st>>>(sum.get(), c.rows,
                                                                                                   c.base, row_start);
      ENC_OK(hipGetLastError());
    }
    if (limit) {
      const Rows rw = rows_of(c.o, c.row, c.n);
      const u64 tiles = (limit + kTile - 1) / kTile;
      const uint32_t al = (aligned16(out) ? 1u : 0u) | (aligned16(pos) ? 2u : 0u) | (aligned16(seg) ? 4u : 0u);
      k_bat_pack<<<dim3((unsigned)tiles), dim3(kThreads), 0, st>>>(c.ids, rw, c.rows, sum.get(), limit, pad_id,
                                                                   c.row_base, out, pos, seg, al);
      ENC_OK(hipGetLastError());
    }
    return 0;
  }

  // Staging of a pad or window piece: its ids and offsets, out (output 0) and two per-row int32
  // arrays (outputs 1 and 3), the mask (output 2).
  bool stage(const Piece& p, bool mask, Staged* s) {
    if (!hids.grow(std::max<size_t>(p.len[0], 1)) || !hrow.grow(p.r1 - p.r0 + 1, 2) ||
        !hout.grow(std::max(p.cells, p.wp), 3) || (mask && !hmask.grow(std::max<size_t>(p.cells, 1))))
      return false;
    s->ids[0] = hids.get();
    s->row[0] = hrow.get();
    s->out[0] = hout.get();
    s->out[1] = hout.get() + hout.cap();
    s->out[2] = hmask.get();
    s->out[3] = hout.get() + 2 * hout.cap();
    return true;
  }
};

// The window passes' state, allocated on the first window call: the length pass (sum is WO); the
// host path stages through BatchState's buffers and hsrc.
struct WindowState : LengthState {
  DeviceBuf<int64_t> hsrc;     // host path: a piece's win_src

  bool reserve(size_t rows) {
    const Rows rw{nullptr, 0, 1, 0, 0, 0, 0, 0};
    return LengthState::reserve(rows, row_iter(WOInput{{rw, 1}}), row_iter(WInput{rw}));
  }

  // Row checks (when c.row), WO into sum and the longest window over c's rows: 0, -1, -6.
  int lengths(const BatchCall& c, const Windows& wn, hipStream_t st, uint64_t* windows, uint64_t* widest) {
    const auto scan_in = row_iter(WOInput{wn});
    const auto max_in = row_iter(WInput{wn.rw});
    return measure(c.rows, [&](u64* err) { return row_pass(wn.rw, c, err, st); }, &scan_in, &max_in, st, windows,
                   widest);
  }

  // The call's windows [0, windows) from sum into out / lengths / mask / win_row / win_src (which
  // point at the call's first window); win_row gets c.row_base added and win_src c.base.
  int expand(const BatchCall& c, const Windows& wn, uint64_t windows, uint64_t width, int32_t pad_id, int pad_side,
             int32_t* out, int32_t* lengths, uint8_t* mask, int32_t* win_row, int64_t* win_src, hipStream_t st) {
    const u64 total = windows * width;
    if (!windows) return 0;
    if (!total) {  // width == 0: every row is empty, window r is row r
      if (lengths || win_row || win_src) {
        k_bat_window_meta<<<dim3((unsigned)((c.rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, st>>>(
            wn.rw, c.rows, c.row_base, c.base, lengths, win_row, win_src);
        ENC_OK(hipGetLastError());
      }
      return 0;
    }
    const u64 tiles = (total + kTile - 1) / kTile;
    (aligned16(out) ? k_bat_window<true> : k_bat_window<false>)<<<dim3((unsigned)tiles), dim3(kThreads), 0, st>>>(
        c.ids, wn, c.rows, sum.get(), width, total, pad_id, pad_side ? 1u : 0u, c.row_base, c.base, out, lengths, mask,
        (reinterpret_cast<uintptr_t>(mask) & 3) == 0 ? 1u : 0u, win_row, win_src);
    ENC_OK(hipGetLastError());
    return 0;
  }
};

}  // namespace

int64_t EncodeDevice::pad(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const BatchOpts& o,
                          size_t width, int32_t pad_id, int pad_side, int32_t* out, size_t cap, int32_t* lengths,
                          uint8_t* mask, void* stream, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  const u64 R = row_off ? rows : 1;
  if (width && R > (u64)INT64_MAX / width) return -1;
  const BatchCall c{ids, n, row_off, R, true, o, 0, 0};
  return device_call<BatchState>(
      pass_[kBatch], device_, stream ? stream : stream_, "batch", R, kernel_ms,
      [&](BatchState& bs, hipStream_t st, Plan* p) {
        u64 total = 0, widest = 0;
        const int r = bs.lengths(c, false, st, &total, &widest);
        *p = Plan{(int64_t)widest, out && width >= widest && cap >= R * width, R * width};
        return r;
      },
      [&](BatchState&, hipStream_t st) { return pad_expand(c, width, pad_id, pad_side, out, lengths, mask, st); });
}

int64_t EncodeDevice::pack(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const BatchOpts& o,
                           size_t seq_len, int32_t pad_id, bool drop_last, int32_t* out, size_t cap, int32_t* pos,
                           int32_t* seg, int64_t* row_start, void* stream, double* kernel_ms) {
  const u64 R = row_off ? rows : 1, L = seq_len;
  const BatchCall c{ids, n, row_off, R, true, o, 0, 0};
  u64 S = 0;
  return device_call<BatchState>(
      pass_[kBatch], device_, stream ? stream : stream_, "batch", R, kernel_ms,
      [&](BatchState& bs, hipStream_t st, Plan* p) {
        u64 total = 0, widest = 0;
        const int r = bs.lengths(c, true, st, &total, &widest);
        if (r < 0) return r;
        S = drop_last ? total / L : total / L + (total % L ? 1 : 0);
        if (S > (u64)INT64_MAX / L) return -1;
        *p = Plan{(int64_t)S, out && cap >= S * L, S * L};
        return 0;
      },
      [&](BatchState& bs, hipStream_t st) { return bs.pack_expand(c, S * L, pad_id, out, pos, seg, row_start, st); });
}

int64_t EncodeDevice::window(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const BatchOpts& o,
                             size_t stride, size_t width, int32_t pad_id, int pad_side, int32_t* out, size_t cap,
                             int32_t* lengths, uint8_t* mask, int32_t* win_row, int64_t* win_src, int64_t* row_win,
                             size_t* widest_out, void* stream, double* kernel_ms) {
  const u64 R = row_off ? rows : 1;
  const BatchCall c{ids, n, row_off, R, true, o, 0, 0};
  const Windows wn = windows_of(o, stride, row_off, n);
  u64 windows = 0, widest = 0;
  const int64_t r = device_call<WindowState>(
      pass_[kWindow], device_, stream ? stream : stream_, "window", R, kernel_ms,
      [&](WindowState& ws, hipStream_t st, Plan* p) {
        const int r = ws.lengths(c, wn, st, &windows, &widest);
        if (r < 0) return r;
        if (windows > (u64)INT64_MAX || (width && windows > (u64)INT64_MAX / width)) return -1;
        *p = Plan{(int64_t)windows, out && width >= widest && cap >= windows * width, windows * width};
        return 0;
      },
      [&](WindowState& ws, hipStream_t st) {
        if (row_win) {
          k_bat_row_start<<<dim3((unsigned)((R + kThreads) / kThreads)), dim3(kThreads), 0, st>>>(ws.sum.get(), R, 0,
                                                                                                  row_win);
          ENC_OK(hipGetLastError());
        }
        return ws.expand(c, wn, windows, width, pad_id, pad_side, out, lengths, mask, win_row, win_src, st);
      });
  if (r >= 0 && widest_out) *widest_out = (size_t)widest;
  return r;
}

// Host rows in pieces of whole rows (host_pieces).  A pad piece is a pad of its own rows into rows
// [r0, r1) of out; the caller has validated row_off and width on the host, so no length pass runs.
int EncodeDevice::pad_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const BatchOpts& o,
                           size_t width, int32_t pad_id, int pad_side, int32_t* out, int32_t* lengths,
                           uint8_t* mask) {
  BatchState& bs = pass_state<BatchState>(pass_[kBatch]);
  hipStream_t st = (hipStream_t)stream_;
  const HostCall call{"batch", row_off ? rows : 1, width, 1, {{ids, n, row_off}}, false, nullptr,
                      3,       {{out, 4, 0, 1}, {lengths, 4, 1, 0}, {mask, 1, 0, 1}}};
  return host_pieces(
      device_, st, call, [](size_t) { return (u64)1; },
      [&](const Piece& p, Staged* s) { return bs.stage(p, mask != nullptr, s); },
      [&](const Piece& p, const Staged& s) {
        const BatchCall c{s.ids[0], p.len[0], row_off ? s.row[0] : nullptr, p.r1 - p.r0, false, o, 0, p.r0};
        return pad_expand(c, width, pad_id, pad_side, s.get<int32_t>(0), s.get<int32_t>(1), s.get<uint8_t>(2), st);
      });
}

// A pack piece runs its own length pass (the caller has validated row_off) and writes its slice of
// the flat stream at the offset of its first row (BatchCall::base), cut at out_len = S * seq_len;
// only the last piece runs on to out_len, which writes the pad tail.  The stream is not a rectangle
// of emitted rows, so the piece's outputs are sized and copied back here.
int EncodeDevice::pack_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const BatchOpts& o,
                            uint64_t out_len, int32_t pad_id, int32_t* out, int32_t* pos, int32_t* seg,
                            int64_t* row_start) {
  const size_t R = row_off ? rows : 1;
  BatchState& bs = pass_state<BatchState>(pass_[kBatch]);
  hipStream_t st = (hipStream_t)stream_;
  const HostCall call{"batch", R, 0, 1, {{ids, n, row_off}}, false, nullptr, 0, {}};
  u64 done = 0;
  if (row_start) row_start[0] = 0;
  return host_pieces(
      device_, st, call, [](size_t) { return (u64)0; },
      [&](const Piece& p, Staged* s) {
        const size_t m = p.r1 - p.r0;
        if (!bs.reserve(m) || !bs.hids.grow(std::max<size_t>(p.len[0], 1)) || !bs.hrow.grow(m + 1, 2)) return false;
        s->ids[0] = bs.hids.get();
        s->row[0] = bs.hrow.get();
        return true;
      },
      [&](const Piece& p, const Staged& s) {
        const size_t m = p.r1 - p.r0;
        const BatchCall c{s.ids[0], p.len[0], row_off ? s.row[0] : nullptr, m, false, o, done, p.r0};
        u64 total = 0, widest = 0;
        if (bs.lengths(c, true, st, &total, &widest) < 0) return -1;
        const u64 end = p.r1 == R ? out_len : std::min(done + total, out_len);
        const u64 limit = end > done ? end - done : 0;
        if (!tiles_fit(limit) || !bs.hout.grow(std::max<size_t>((size_t)limit, 1), 3)) {
          std::fprintf(stderr, "[ERROR]\t encoder: batch staging allocation failed (%zu entries)\n", (size_t)limit);
          return -1;
        }
        int32_t *const dout = bs.hout.get(), *const dpos = dout + bs.hout.cap(), *const dseg = dpos + bs.hout.cap();
        int64_t* dstart = bs.hrow.get() + bs.hrow.cap();
        if (bs.pack_expand(c, limit, pad_id, dout, pos ? dpos : nullptr, seg ? dseg : nullptr,
                           row_start ? dstart : nullptr, st) < 0)
          return -1;
        if (limit) {
          ENC_OK(hipMemcpyAsync(out + done, dout, limit * 4, hipMemcpyDeviceToHost, st));
          if (pos) ENC_OK(hipMemcpyAsync(pos + done, dpos, limit * 4, hipMemcpyDeviceToHost, st));
          if (seg) ENC_OK(hipMemcpyAsync(seg + done, dseg, limit * 4, hipMemcpyDeviceToHost, st));
        }
        if (row_start) ENC_OK(hipMemcpyAsync(row_start + p.r0 + 1, dstart + 1, m * 8, hipMemcpyDeviceToHost, st));
        done += total;
        return 0;
      });
}

// A window piece is the windows of its own rows, written to windows [w0, w1) of the outputs.  The
// caller has validated row_off, width and cap on the host, so no length pass runs: the piece's WO
// is made on the host and uploaded, and row_win is written from it.
int EncodeDevice::window_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const BatchOpts& o,
                              size_t stride, size_t width, int32_t pad_id, int pad_side, int32_t* out,
                              int32_t* lengths, uint8_t* mask, int32_t* win_row, int64_t* win_src, int64_t* row_win) {
  BatchState& bs = pass_state<BatchState>(pass_[kBatch]);
  WindowState& ws = pass_state<WindowState>(pass_[kWindow]);
  hipStream_t st = (hipStream_t)stream_;
  const Windows host = windows_of(o, stride, row_off, n);
  const HostCall call{"window", row_off ? rows : 1, width, 1, {{ids, n, row_off}}, true, row_win, 5,
                      {{out, 4, 0, 1}, {lengths, 4, 1, 0}, {mask, 1, 0, 1}, {win_row, 4, 1, 0}, {win_src, 8, 1, 0}}};
  return host_pieces(
      device_, st, call, [&](size_t r) { return host.count(r); },
      [&](const Piece& p, Staged* s) {
        if (!bs.stage(p, mask != nullptr, s) || !ws.sum.grow(p.r1 - p.r0 + 1) || (win_src && !ws.hsrc.grow(p.wp)))
          return false;
        s->wo = ws.sum.get();
        s->out[4] = ws.hsrc.get();
        return true;
      },
      [&](const Piece& p, const Staged& s) {
        const BatchCall c{s.ids[0], p.len[0], row_off ? s.row[0] : nullptr, p.r1 - p.r0, false, o, p.a[0], p.r0};
        return ws.expand(c, windows_of(o, stride, c.row, c.n), p.wp, width, pad_id, pad_side, s.get<int32_t>(0),
                         s.get<int32_t>(1), s.get<uint8_t>(2), s.get<int32_t>(3), s.get<int64_t>(4), st);
      });
}

}  // namespace shred
