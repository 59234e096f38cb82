// Row pairs to one model input on gfx950: [bos] + kept_a + mid + kept_b + [eos], truncated against
// one budget or with the second row cut into windows (C ABI and definitions:
// include/shredword_encode.h, shred_pair_*).  The rule that turns an example into its emitted rows is
// host/pair_rule.h; the tile geometry and the wave search are batch_common.h's, the kernels this
// unit's own, and the length pass, the device call and the host pieces are batch_state.h's.
//
// Example r has la_r ids of ids_a and lb_r ids of ids_b.  The strategy turns (la_r, lb_r) into ka_r
// kept ids of a and, for strategies 0 .. 2, kb_r kept ids of b (one emitted row), for strategy 3 a
// window capacity C_r = B - ka_r (w_r emitted rows, step_r = C_r - stride apart).  WO is the exclusive
// prefix sum of w_r, WO[rows] = Wn, strictly increasing since every example emits a row.
//
//   k_pair_rows      one thread per entry of the two offset arrays: range, order and end points of
//                    both, and for example r - 1: whether the strategy can make it fit and whether
//                    its e fits an int32 (error words, ordinary stores, no atomics);
//   hipCUB scan      WO[0 .. rows] from w_r, through a transform iterator on the two offset arrays;
//   hipCUB reduce    the maximum over r of the example's longest emitted row (its first);
//   k_bat_row_start  row_win[r] = WO[r];
//   k_bat_pair       output-centric like k_bat_window: one workgroup per kTile consecutive entries
//                    of the flat [Wn, W] array, 4 consecutive entries per lane, the (emitted row,
//                    column) split of a lane's first entry done once and then walked.  The example
//                    of the tile's first emitted row by one search of WO per workgroup (its first
//                    wave probes 64 entries a step); then rounds of kStage examples staged in LDS:
//                    WO relative to the tile's first emitted row, ka and the index in ids_a of the
//                    first kept a id, C_r and step_r, the index in ids_b at which the example's
//                    window at the tile's first emitted row would start, and the end of its b range
//                    (strategies 0 .. 2 stage the kept b ids as one window: C = kb, step = 0).  A
//                    lane finds the example under its first entry by a binary search of the LDS
//                    offsets and walks forward.  A tile of narrow rows can hold more than kStage
//                    examples and takes more rounds; an example whose windows cover many tiles needs
//                    no special case.  The lane that owns column 0 of an emitted row writes its
//                    lengths, win_row, seg_len and seg_src; types and mask come from the same walk;
//   k_bat_pair_meta  W == 0 only (examples that are empty on both sides, nothing added): no lane
//                    owns a column, so one thread per example writes the four.
//
// Traffic per output entry at fill f = sum e / (Wn W): writes 4 (out), reads 4 f (an id of a or of
// b): 4 + 4 f bytes, + 1 each with types and mask; per emitted row 4 (lengths) + 4 (win_row) + 8
// (seg_len) + 16 (seg_src) = 32 B for those asked for; per example 16 (row pass) + 16 (scan) + 16
// (reduce) reads of the two offset arrays, 8 written for WO and 8 for row_win, and the tiles read WO
// and the offsets back through the caches.  Every window of an example reads the same kept a ids
// again: they are counted in f, and come from the caches when the windows share a tile.
// All global indices are 64-bit; every store is an ordinary vector store.  Output pointers are
// only element-aligned (tensor views), so the 16-byte (types, mask: 4-byte) stores have a scalar form.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../host/encoder.h"
#include "../host/pair_rule.h"
#include "batch_common.h"
#include "batch_state.h"
#include "encode_common.h"

namespace shred {
namespace {

// err: [0] a bad offset array, [1] an e past int32, [2] an example that cannot fit.
__global__ __launch_bounds__(kThreads) void k_pair_rows(Pairs pr, u64 rows, u64* __restrict__ err) {
  const u64 r = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (r > rows) return;
  const int64_t va = pr.ra[r], vb = pr.rb[r];
  const int64_t pa = r ? pr.ra[r - 1] : 0, pb = r ? pr.rb[r - 1] : 0;
  bool bad = va < 0 || (u64)va > pr.na || pa > va || vb < 0 || (u64)vb > pr.nb || pb > vb;
  if ((r == 0 && (va != 0 || vb != 0)) || (r == rows && ((u64)va != pr.na || (u64)vb != pr.nb))) bad = true;
  if (bad) {
    err[0] = 1;
    return;
  }
  if (r && pa >= 0 && pb >= 0) {
    u64 ka, kb;
    if (!pr.first((u64)(va - pa), (u64)(vb - pb), &ka, &kb)) {
      err[2] = 1;
    } else if (pr.too_long(ka, kb)) {
      err[1] = 1;
    }
  }
}

// Element k of the scan: the emitted rows of example k - 1; element r of the reduction: its longest.
struct PWOInput {
  Pairs pr;
  __host__ __device__ __forceinline__ u64 operator()(u64 k) const { return k ? pr.count(k - 1) : 0ull; }
};
struct PEInput {
  Pairs pr;
  __host__ __device__ __forceinline__ u64 operator()(u64 r) const { return pr.emit(r); }
};

// total = Wn * W > 0, W >= every emitted row's length; WO: rows + 1 entries, strictly increasing
// from 0 to Wn; every example fits (k_pair_rows, or the host).  Emitted row w of the call goes to
// out[w * W ..], lengths[w], win_row[w], seg_len[2 w ..], seg_src[2 w ..].  bytes_aligned: bit 0
// types, bit 1 mask may take 4-byte stores.
template <bool kAligned>
__global__ __launch_bounds__(kThreads) void k_bat_pair(const int32_t* __restrict__ ids_a,
                                                       const int32_t* __restrict__ ids_b, Pairs pr, u64 rows,
                                                       const u64* __restrict__ WO, u64 W, u64 total, int32_t pad_id,
                                                       uint32_t pad_left, u64 row_base, u64 a_base, u64 b_base,
                                                       int32_t* __restrict__ out, uint8_t* __restrict__ types,
                                                       uint8_t* __restrict__ mask, uint32_t bytes_aligned,
                                                       int32_t* __restrict__ lengths, int32_t* __restrict__ win_row,
                                                       int32_t* __restrict__ seg_len, int64_t* __restrict__ seg_src) {
  __shared__ int32_t s_w[kStage + 1];  // WO[k] - the tile's first emitted row, clamped to [-INT32_MAX, kTile + 1]
  __shared__ uint32_t s_ka[kStage];    // ka (<= INT32_MAX)
  __shared__ uint32_t s_c[kStage];     // C_r (strategies 0 .. 2: kb)
  __shared__ uint32_t s_step[kStage];  // step_r (strategies 0 .. 2: 0)
  __shared__ u64 s_asrc[kStage];       // index in ids_a of the first kept a id
  __shared__ u64 s_bsrc[kStage];       // index in ids_b at which the example's window at the tile's first emitted
                                       // row starts (modulo 2^64: examples that begin later lie before their ids)
  __shared__ u64 s_bend[kStage];       // the end of the example's b range (strategies 0 .. 2: of its kept b ids)
  __shared__ u64 s_k;
  const int tid = threadIdx.x;
  const u64 t0 = (u64)blockIdx.x * kTile;
  const int tlen = (int)(total - t0 < (u64)kTile ? total - t0 : (u64)kTile);
  const u64 w0 = t0 / W, c0 = t0 - w0 * W;                // the tile's first entry: emitted row, column
  const int wlast = (int)((c0 + (u64)(tlen - 1)) / W);    // its last entry's emitted row, relative to w0
  if (tid < 64) {  // the example of row w0: the last k with WO[k] <= w0 (WO[0] = 0, WO[rows] = Wn > w0)
    const u64 ub = wave_upper_bound(WO, 0, rows + 1, w0, tid);
    if (tid == 0) s_k = ub == 0 ? 0 : ub > rows ? rows - 1 : ub - 1;
  }
  __syncthreads();
  u64 ks = s_k;
  const int p0 = tid * kLane;
  const int cnt = p0 >= tlen ? 0 : tlen - p0 < kLane ? tlen - p0 : kLane;
  const u64 first = c0 + (u64)p0;
  const int wr0 = (int)(first / W);  // the lane's first entry: emitted row relative to w0 (<= kTile), column
  const u64 cl0 = first - (u64)wr0 * W;
  const u64 add = pr.add();
  int32_t v[kLane] = {pad_id, pad_id, pad_id, pad_id};
  uint32_t mk = 0, tk = 0;
  for (;;) {
    // examples ks .. ks + m - 1, and the offset of example ks + m (k == rows: Wn)
    const int m = (int)(rows - ks < (u64)kStage ? rows - ks : (u64)kStage);
    for (int i = tid; i <= m; i += kThreads) {
      const u64 k = ks + (u64)i;
      const int64_t rel = (int64_t)(WO[k] - w0);
      s_w[i] = (int32_t)(rel < -(int64_t)INT32_MAX ? -(int64_t)INT32_MAX : rel > kTile + 1 ? (int64_t)(kTile + 1) : rel);
      if (i < m) {
        u64 a0, a1, b0, b1, ka = 0, cb = 0;
        pr.bounds(k, &a0, &a1, &b0, &b1);
        pr.fit(a1 - a0, b1 - b0, &ka, &cb);
        const bool win = pr.strategy == 3;
        const u64 step = win ? cb - pr.stride : 0;
        const u64 bsrc = win || !pr.left ? b0 : b1 - cb;
        s_ka[i] = (uint32_t)ka;
        s_c[i] = (uint32_t)cb;
        s_step[i] = (uint32_t)step;
        s_asrc[i] = pr.left ? a1 - ka : a0;
        s_bsrc[i] = bsrc - (u64)rel * step;
        s_bend[i] = win ? b1 : bsrc + cb;
      }
    }
    __syncthreads();
    // this round resolves the emitted rows [from, lim) relative to w0: those of the staged examples
    const int from = s_w[0], lim = s_w[m];
    int wr = wr0, j = -1;
    u64 c = cl0, asrc = 0, start = 0, ka = 0, kb = 0, e = 0, lead = 0;
    bool fresh = true;
#pragma unroll
    for (int i = 0; i < kLane; ++i) {
      if (i < cnt && wr >= from && wr < lim) {
        if (fresh) {
          if (j < 0) {  // the last staged example that starts at or before emitted row wr
            int a = 0, b = m;
            while (a < b) {
              const int mid = (a + b) >> 1;
              if (s_w[mid] <= wr) a = mid + 1; else b = mid;
            }
            j = a - 1;  // >= 0: s_w[0] = from <= wr
          } else {
            while (j + 1 < m && s_w[j + 1] <= wr) ++j;
          }
          ka = (u64)s_ka[j];
          asrc = s_asrc[j];
          start = s_bsrc[j] + (u64)wr * (u64)s_step[j];
          const u64 left = s_bend[j] - start, C = (u64)s_c[j];
          kb = left < C ? left : C;
          e = add + ka + kb;
          lead = pad_left ? W - e : 0;
          fresh = false;
          if (c == 0) {
            const u64 w = w0 + (u64)wr;
            if (lengths) lengths[w] = (int32_t)e;
            if (win_row) win_row[w] = (int32_t)(row_base + ks + (u64)j);
            if (seg_len) {
              seg_len[2 * w] = (int32_t)ka;
              seg_len[2 * w + 1] = (int32_t)kb;
            }
            if (seg_src) {
              seg_src[2 * w] = (int64_t)(a_base + asrc);
              seg_src[2 * w + 1] = (int64_t)(b_base + start);
            }
          }
        }
        if (c >= lead && c - lead < e) {
          uint32_t ty;
          v[i] = pr.id(ids_a, ids_b, ka, kb, asrc, start, c - lead, &ty);
          mk |= 1u << (8 * i);
          tk |= ty << (8 * i);
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
  if (types) {
    if ((bytes_aligned & 1u) && cnt == kLane) {
      *reinterpret_cast<uint32_t*>(types + g) = tk;
    } else {
#pragma unroll
      for (int i = 0; i < kLane; ++i)
        if (i < cnt) types[g + i] = (uint8_t)(tk >> (8 * i));
    }
  }
  if (mask) {
    if ((bytes_aligned & 2u) && cnt == kLane) {
      *reinterpret_cast<uint32_t*>(mask + g) = mk;
    } else {
#pragma unroll
      for (int i = 0; i < kLane; ++i)
        if (i < cnt) mask[g + i] = (uint8_t)(mk >> (8 * i));
    }
  }
}

// W == 0: every example is empty on both sides and nothing is added, so emitted row r is example r
// and holds nothing.
__global__ __launch_bounds__(kThreads) void k_bat_pair_meta(Pairs pr, u64 rows, u64 row_base, u64 a_base, u64 b_base,
                                                            int32_t* __restrict__ lengths,
                                                            int32_t* __restrict__ win_row,
                                                            int32_t* __restrict__ seg_len,
                                                            int64_t* __restrict__ seg_src) {
  const u64 r = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (r >= rows) return;
  u64 a0, a1, b0, b1;
  pr.bounds(r, &a0, &a1, &b0, &b1);
  if (lengths) lengths[r] = 0;
  if (win_row) win_row[r] = (int32_t)(row_base + r);
  if (seg_len) {
    seg_len[2 * r] = 0;
    seg_len[2 * r + 1] = 0;
  }
  if (seg_src) {
    seg_src[2 * r] = (int64_t)(a_base + a0);
    seg_src[2 * r + 1] = (int64_t)(b_base + b0);
  }
}

// The outputs of a call or of a piece, at its first emitted row.
struct PairOut {
  int32_t* out;
  uint8_t *types, *mask;
  int32_t *lengths, *win_row, *seg_len;
  int64_t* seg_src;
};

// The pair passes' state, allocated on the first pair call: the length pass (sum is WO) and the
// host path's staging.
struct PairState : LengthState {
  // host-path staging: a piece's ids of a and of b; its two local offset arrays (2 x hrow.cap());
  // out; lengths, win_row and the two columns' worth of seg_len (4 x hmeta.cap()); seg_src
  // (2 x hsrc.cap()); types and mask (2 x hbytes.cap())
  DeviceBuf<int32_t> ha, hb;
  DeviceBuf<int64_t> hrow;
  DeviceBuf<int32_t> hout, hmeta;
  DeviceBuf<int64_t> hsrc;
  DeviceBuf<uint8_t> hbytes;

  bool reserve(size_t rows) {
    const Pairs pr{nullptr, nullptr, 0, 0, kNoLimit, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return LengthState::reserve(rows, row_iter(PWOInput{pr}), row_iter(PEInput{pr}));
  }

  // The row pass, WO into sum and the longest emitted row over the call's examples: 0, -1, -6, -7.
  int lengths(const Pairs& pr, u64 rows, hipStream_t st, uint64_t* emitted, uint64_t* widest) {
    const auto scan_in = row_iter(PWOInput{pr});
    const auto max_in = row_iter(PEInput{pr});
    return measure(
        rows,
        [&](u64* err) {
          k_pair_rows<<<dim3((unsigned)((rows + kThreads) / kThreads)), dim3(kThreads), 0, st>>>(pr, rows, err);
          ENC_OK(hipGetLastError());
          return 0;
        },
        &scan_in, &max_in, st, emitted, widest);
  }

  // The emitted rows [0, emitted) of the examples of pr from wo into o; win_row gets row_base added,
  // the two columns of seg_src a_base and b_base.
  int expand(const int32_t* ids_a, const int32_t* ids_b, const Pairs& pr, u64 rows, u64 emitted, u64 width,
             int32_t pad_id, int pad_side, u64 row_base, u64 a_base, u64 b_base, const PairOut& o, hipStream_t st) {
    const u64 total = emitted * width;
    if (!emitted) return 0;
    if (!total) {  // width == 0: every example is empty, emitted row r is example r
      if (o.lengths || o.win_row || o.seg_len || o.seg_src) {
        k_bat_pair_meta<<<dim3((unsigned)((rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, st>>>(
            pr, rows, row_base, a_base, b_base, o.lengths, o.win_row, o.seg_len, o.seg_src);
        ENC_OK(hipGetLastError());
      }
      return 0;
    }
    const u64 tiles = (total + kTile - 1) / kTile;
    const uint32_t al = ((reinterpret_cast<uintptr_t>(o.types) & 3) == 0 ? 1u : 0u) |
                        ((reinterpret_cast<uintptr_t>(o.mask) & 3) == 0 ? 2u : 0u);
    (aligned16(o.out) ? k_bat_pair<true> : k_bat_pair<false>)<<<dim3((unsigned)tiles), dim3(kThreads), 0, st>>>(
        ids_a, ids_b, pr, rows, sum.get(), width, total, pad_id, pad_side ? 1u : 0u, row_base, a_base, b_base, o.out,
        o.types, o.mask, al, o.lengths, o.win_row, o.seg_len, o.seg_src);
    ENC_OK(hipGetLastError());
    return 0;
  }
};

}  // namespace

int64_t EncodeDevice::pair(const int32_t* ids_a, size_t n_a, const int64_t* row_a, const int32_t* ids_b, size_t n_b,
                           const int64_t* row_b, size_t rows, const PairOpts& o, size_t width, int32_t pad_id,
                           int pad_side, int32_t* out, size_t cap, uint8_t* types, uint8_t* mask, int32_t* lengths,
                           int32_t* win_row, int32_t* seg_len, int64_t* seg_src, int64_t* row_win, size_t* widest_out,
                           void* stream, double* kernel_ms) {
  const u64 R = rows;
  const Pairs pr = pairs_of(o, row_a, n_a, row_b, n_b);
  u64 emitted = 0, widest = 0;
  const int64_t r = device_call<PairState>(
      pass_[kPair], device_, stream ? stream : stream_, "pair", R, kernel_ms,
      [&](PairState& ps, hipStream_t st, Plan* p) {
        const int r = ps.lengths(pr, R, st, &emitted, &widest);
        if (r < 0) return r;
        if (emitted > (u64)INT64_MAX || (width && emitted > (u64)INT64_MAX / width)) return -1;
        *p = Plan{(int64_t)emitted, out && width >= widest && cap >= emitted * width, emitted * width};
        return 0;
      },
      [&](PairState& ps, hipStream_t st) {
        if (row_win) {
          k_bat_row_start<<<dim3((unsigned)((R + kThreads) / kThreads)), dim3(kThreads), 0, st>>>(ps.sum.get(), R, 0,
                                                                                                  row_win);
          ENC_OK(hipGetLastError());
        }
        const PairOut po{out, types, mask, lengths, win_row, seg_len, seg_src};
        return ps.expand(ids_a, ids_b, pr, R, emitted, width, pad_id, pad_side, 0, 0, 0, po, st);
      });
  if (r >= 0 && widest_out) *widest_out = (size_t)widest;
  return r;
}

// Host examples, whose offset arrays, fit, Wn, width and cap the caller has settled on the host, so
// no length pass runs on the device.  A piece is the emitted rows of its own examples, written to
// rows [w0, w1) of the outputs; its ids are those of a plus those of b.  The piece's WO is made on
// the host and uploaded, and row_win is written from it.
int EncodeDevice::pair_host(const int32_t* ids_a, size_t n_a, const int64_t* row_a, const int32_t* ids_b, size_t n_b,
                            const int64_t* row_b, size_t rows, const PairOpts& o, size_t width, int32_t pad_id,
                            int pad_side, int32_t* out, uint8_t* types, uint8_t* mask, int32_t* lengths,
                            int32_t* win_row, int32_t* seg_len, int64_t* seg_src, int64_t* row_win) {
  PairState& ps = pass_state<PairState>(pass_[kPair]);
  hipStream_t st = (hipStream_t)stream_;
  const Pairs host = pairs_of(o, row_a, n_a, row_b, n_b);
  const HostCall call{"pair", rows, width, 2, {{ids_a, n_a, row_a}, {ids_b, n_b, row_b}}, true, row_win, 7,
                      {{out, 4, 0, 1}, {types, 1, 0, 1}, {mask, 1, 0, 1}, {lengths, 4, 1, 0}, {win_row, 4, 1, 0},
                       {seg_len, 4, 2, 0}, {seg_src, 8, 2, 0}}};
  return host_pieces(
      device_, st, call, [&](size_t r) { return host.count(r); },
      [&](const Piece& p, Staged* s) {
        const size_t m = p.r1 - p.r0;
        if (!ps.ha.grow(std::max<size_t>(p.len[0], 1)) || !ps.hb.grow(std::max<size_t>(p.len[1], 1)) ||
            !ps.hrow.grow(m + 1, 2) || !ps.sum.grow(m + 1) || !ps.hout.grow(std::max<size_t>(p.cells, 1)) ||
            !ps.hmeta.grow(p.wp, 4) || (seg_src && !ps.hsrc.grow(p.wp, 2)) ||
            ((types || mask) && !ps.hbytes.grow(std::max<size_t>(p.cells, 1), 2)))
          return false;
        *s = Staged{{ps.ha.get(), ps.hb.get()},
                    {ps.hrow.get(), ps.hrow.get() + ps.hrow.cap()},
                    ps.sum.get(),
                    {ps.hout.get(), ps.hbytes.get(), ps.hbytes.get() + ps.hbytes.cap(), ps.hmeta.get(),
                     ps.hmeta.get() + ps.hmeta.cap(), ps.hmeta.get() + 2 * ps.hmeta.cap(), ps.hsrc.get()}};
        return true;
      },
      [&](const Piece& p, const Staged& s) {
        const PairOut po{s.get<int32_t>(0), s.get<uint8_t>(1), s.get<uint8_t>(2), s.get<int32_t>(3),
                         s.get<int32_t>(4), s.get<int32_t>(5), s.get<int64_t>(6)};
        return ps.expand(s.ids[0], s.ids[1], pairs_of(o, s.row[0], p.len[0], s.row[1], p.len[1]), p.r1 - p.r0, p.wp,
                         width, pad_id, pad_side, p.r0, p.a[0], p.a[1], po, st);
      });
}

}  // namespace shred
