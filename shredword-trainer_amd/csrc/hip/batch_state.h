// What the batch units (batch_device.hip, batch_pair.hip) share on the host: the state of a length
// pass, the driver of a device call and the piece loop of a host call.
//
// A length pass runs a row pass over the call's offset arrays (error words), a hipCUB inclusive sum
// over k = 0 .. rows of (k ? x_{k-1} : 0) through a transform iterator (the exclusive prefix sum of
// x with its total at entry rows) and a hipCUB maximum of the rows' longest emitted row through the
// same kind of iterator; the words come back in one copy.
// Included by .hip files only.
#pragma once

#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "batch_common.h"
#include "encode_common.h"

namespace shred {
namespace {

// Iterator over f(0), f(1), ..: what the scan and the reduction read.
template <class F>
using RowIter = hipcub::TransformInputIterator<u64, F, hipcub::CountingInputIterator<u64>>;
template <class F>
RowIter<F> row_iter(const F& f) {
  return RowIter<F>(hipcub::CountingInputIterator<u64>(0), f);
}

// The state of a length pass, allocated on the pass's first call.  Scratch grown to the most rows
// seen: 8 B per row (the prefix sum) and what the scan and the reduction ask for.  The units derive
// theirs from it and add the staging of their host paths.
struct LengthState : PassState {
  DeviceBuf<u64> sum;          // exclusive prefix sum, rows + 1 entries; sum[rows] = the total
  DeviceBuf<uint8_t> tmp;      // hipCUB scan / reduce scratch
  DeviceWords res;             // [0] a bad offset array, [1] an e past int32, [2] an example that cannot fit
                               // (k_pair_rows only: pad, pack and window leave it 0), [3] max e
  PinnedWords host;            // the total, then the four words of res
  EventSet<4> ev;

  // scan_in / max_in: iterators of the kinds measure() will be given (their values are not read).
  template <class ScanIn, class MaxIn>
  bool reserve(size_t rows, ScanIn scan_in, MaxIn max_in) {
    if (!res.ensure(4) || !host.ensure(5) || !ev.ensure() || !sum.grow(rows + 1)) return false;
    size_t scan = 0, red = 0;
    if (hipcub::DeviceScan::InclusiveSum(nullptr, scan, scan_in, sum.get(), (u64)rows + 1) != hipSuccess) return false;
    if (hipcub::DeviceReduce::Max(nullptr, red, max_in, res.get() + 3, (u64)std::max<size_t>(rows, 1)) != hipSuccess)
      return false;
    return tmp.grow(std::max<size_t>(std::max(scan, red), 16));
  }

  // row_pass(err) launches the row pass on st (0 or -1); the sum of scan_in[0 .. rows] into `sum`
  // and the maximum of max_in[0 .. rows) follow, each when its iterator is given.  Returns 0 with
  // the total (0 without a scan) and the maximum, -6, -7 or -1.
  // (The scan and the reduction read entries 0 .. rows of the offset arrays and nothing through
  // them, so they may run on arrays that the row pass finds bad.)
  template <class RowPass, class ScanIn, class MaxIn>
  int measure(u64 rows, RowPass&& row_pass, const ScanIn* scan_in, const MaxIn* max_in, hipStream_t st, u64* total,
              u64* widest) {
    ENC_OK(hipMemsetAsync(res.get(), 0, 32, st));
    if (row_pass(res.get()) < 0) return -1;
    host[0] = 0;
    size_t bytes = tmp.cap();
    if (scan_in) {
      ENC_OK(hipcub::DeviceScan::InclusiveSum(tmp.get(), bytes, *scan_in, sum.get(), rows + 1, st));
      ENC_OK(hipMemcpyAsync(host.get(), sum.get() + rows, 8, hipMemcpyDeviceToHost, st));
    }
    if (max_in && rows) {
      bytes = tmp.cap();
      ENC_OK(hipcub::DeviceReduce::Max(tmp.get(), bytes, *max_in, res.get() + 3, rows, st));
    }
    ENC_OK(hipMemcpyAsync(host.get() + 1, res.get(), 32, hipMemcpyDeviceToHost, st));
    ENC_OK(hipStreamSynchronize(st));
    if (host[1]) return -6;
    if (host[3]) return -7;
    if (host[2]) return -1;
    *total = host[0];
    *widest = host[4];
    return 0;
  }
};

// ---- a device call ----

// What a device call's measure step settles: the call's result, whether the outputs are written
// (out given, wide enough, cap enough) and how many entries that writes.
struct Plan {
  int64_t result;
  bool expand;
  u64 entries;
};

// EncodeDevice::pad / pack / window / pair around what is particular to them: measure(state, st,
// &plan) runs the length pass (0, or the call's error), expand(state, st) writes the outputs (0 or
// -1).  The events around the two are what kernel_ms sums.  S: the pass's state, with reserve(rows).
template <class S, class Measure, class Expand>
int64_t device_call(std::unique_ptr<PassState>& slot, int device, void* stream, const char* what, u64 rows,
                    double* kernel_ms, Measure&& measure, Expand&& expand) {
  if (kernel_ms) *kernel_ms = 0;
  if (!batch_rows_fit(rows)) return -1;
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device));
  S& s = pass_state<S>(slot);
  if (!s.reserve(rows)) {
    std::fprintf(stderr, "[ERROR]\t encoder: %s allocation failed (%zu rows)\n", what, (size_t)rows);
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  const EventSet<4>& ev = s.ev;
  Plan p{0, false, 0};
  ENC_OK(hipEventRecord(ev[0], st));
  const int r = measure(s, st, &p);
  if (r < 0) return r;
  ENC_OK(hipEventRecord(ev[1], st));
  if (p.expand) {
    if (!tiles_fit(p.entries)) return -1;
    ENC_OK(hipEventRecord(ev[2], st));
    if (expand(s, st) < 0) return -1;
    ENC_OK(hipEventRecord(ev[3], st));
  }
  ENC_OK(hipStreamSynchronize(st));
  if (kernel_ms) ENC_OK(ev.sum_ms(p.expand ? 2 : 1, kernel_ms));
  return p.result;
}

// ---- a host call, in pieces of whole rows ----

size_t piece_ids() {
  return std::min(piece_from_env("SHREDWORD_BATCH_PIECE", EncodeDevice::kBatchPiece, 1), size_t(1) << 40);
}

// One (ids, offsets) input of a host call.
struct HostIn {
  const int32_t* ids;
  size_t n;
  const int64_t* row;  // nullptr: one row of all ids
};

// One output of a host call, copied back from the device at the piece's first emitted row: `host`
// (nullptr: not asked for) holds per_row elements of `elem` bytes for every emitted row and
// per_cell for every cell of the [emitted rows, width] rectangle.
struct HostOut {
  void* host;
  size_t elem, per_row, per_cell;
};

// A host call: its inputs, its outputs, and whether its rows emit other than one row each (then a
// piece's WO goes up with it, and row_win, when given, is written from it).
struct HostCall {
  const char* what;
  size_t rows, width;
  int n_in;
  HostIn in[2];
  bool wo;
  int64_t* row_win;
  int n_out;
  HostOut out[7];
};

// Where a piece is staged on the device: filled in by the call's stage callback, once it has grown
// its buffers.  out[k] belongs to HostCall::out[k] (host_pieces clears those not asked for).
struct Staged {
  int32_t* ids[2];
  int64_t* row[2];
  u64* wo;
  void* out[7];
  template <class T>
  T* get(int k) const {
    return static_cast<T*>(out[k]);
  }
};

// A piece: rows [r0, r1), which emit rows [w0, w0 + wp) of the call's; input k's ids [a[k], a[k] + len[k]).
struct Piece {
  size_t r0, r1, w0, wp, cells;
  size_t a[2], len[2];
};

// The rows [r0, r1) of a piece: whole rows while it holds at most `piece` ids (of all inputs
// together), `piece` rows and 4 x piece output entries at count(r) emitted rows of `width` entries
// for row r; at least one row, however long.  *emitted: the piece's emitted rows; wo (when given):
// their exclusive prefix sum over the piece's rows.
template <class Count>
size_t piece_end(const HostIn* in, int n_in, size_t rows, size_t r0, size_t piece, size_t width, Count&& count,
                 u64* emitted, std::vector<u64>* wo) {
  const auto ids_to = [&](size_t r) {
    u64 s = 0;
    for (int k = 0; k < n_in; ++k) s += (u64)(in[k].row[r] - in[k].row[r0]);
    return s;
  };
  if (wo) wo->assign(1, 0);
  *emitted = 0;
  size_t r1 = r0;
  do {
    *emitted += count(r1);
    if (wo) wo->push_back(*emitted);
    ++r1;
  } while (r1 < rows && r1 - r0 < piece && ids_to(r1 + 1) <= (u64)piece && (*emitted + count(r1)) * width <= 4 * (u64)piece);
  return r1;
}

// The piece loop of pad_host / pack_host / window_host / pair_host, whose callers have validated
// the offsets and the sizes on the host.  Per piece: cut it (piece_end; count(r): the rows that row
// r emits); stage(piece, &staged) grows the call's staging and says where the piece goes (false:
// allocation failed); the ids and the offsets rebased to the piece go up, with the piece's WO;
// expand(piece, staged) runs the kernels (0 or -1); every output asked for comes back at the
// piece's offset.
template <class Count, class Stage, class Expand>
int host_pieces(int device, hipStream_t st, const HostCall& c, Count&& count, Stage&& stage, Expand&& expand) {
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device));
  const size_t piece = piece_ids();
  std::vector<int64_t> local[2];
  std::vector<u64> wo;
  size_t w0 = 0;
  if (c.row_win) c.row_win[0] = 0;
  for (size_t r0 = 0; r0 < c.rows;) {
    u64 wp = 0;
    Piece p{r0, 0, w0, 0, 0, {0, 0}, {0, 0}};
    p.r1 = piece_end(c.in, c.n_in, c.rows, r0, piece, c.width, count, &wp, c.wo ? &wo : nullptr);
    p.wp = (size_t)wp;
    p.cells = p.wp * c.width;
    const size_t m = p.r1 - r0;
    for (int k = 0; k < c.n_in; ++k) {
      p.a[k] = c.in[k].row ? (size_t)c.in[k].row[r0] : 0;
      p.len[k] = (c.in[k].row ? (size_t)c.in[k].row[p.r1] : c.in[k].n) - p.a[k];
    }
    Staged s{};
    if (!tiles_fit(p.cells) || !stage(p, &s)) {
      std::fprintf(stderr, "[ERROR]\t encoder: %s staging allocation failed (%zu ids, %zu rows, %zu emitted rows)\n",
                   c.what, p.len[0] + p.len[1], m, p.wp);
      return -1;
    }
    for (int k = 0; k < c.n_in; ++k) {
      if (p.len[k]) ENC_OK(hipMemcpyAsync(s.ids[k], c.in[k].ids + p.a[k], p.len[k] * 4, hipMemcpyHostToDevice, st));
      if (!c.in[k].row) continue;
      local[k].resize(m + 1);
      for (size_t i = 0; i <= m; ++i) local[k][i] = c.in[k].row[r0 + i] - (int64_t)p.a[k];
      ENC_OK(hipMemcpyAsync(s.row[k], local[k].data(), (m + 1) * 8, hipMemcpyHostToDevice, st));
    }
    if (c.wo) ENC_OK(hipMemcpyAsync(s.wo, wo.data(), (m + 1) * 8, hipMemcpyHostToDevice, st));
    for (int k = 0; k < c.n_out; ++k)
      if (!c.out[k].host) s.out[k] = nullptr;
    if (expand(p, s) < 0) return -1;
    for (int k = 0; k < c.n_out; ++k) {
      const HostOut& o = c.out[k];
      const size_t n = o.per_row * p.wp + o.per_cell * p.cells;
      if (o.host && n)
        ENC_OK(hipMemcpyAsync((char*)o.host + (o.per_row * w0 + o.per_cell * w0 * c.width) * o.elem, s.out[k],
                              n * o.elem, hipMemcpyDeviceToHost, st));
    }
    if (c.wo && c.row_win)
      for (size_t i = 1; i <= m; ++i) c.row_win[r0 + i] = (int64_t)(w0 + wo[i]);
    ENC_OK(hipStreamSynchronize(st));
    w0 += p.wp;
    r0 = p.r1;
  }
  return 0;
}

}  // namespace
}  // namespace shred
