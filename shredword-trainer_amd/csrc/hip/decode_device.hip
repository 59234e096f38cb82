// Token ids back to bytes on gfx950, per row (C ABI and definitions: include/shredword_encode.h,
// shred_decode_device / shred_decode_rows).  The passes use none of the encoder's kernels.
//
// With len(k) the byte length of ids[k] (unk_len for an id outside the vocabulary) and P its
// exclusive prefix sum, token k starts at output byte
//   Q[k] = P[k] + #{r >= 1 : row_off[r] <= k}          (the separators of the rows ended before it)
// when every row is followed by a one-byte separator, Q[k] = P[k] without one; Q[n] is the total.
// Output byte p belongs to the last k with Q[k] <= p: it is byte p - Q[k] of that token if
// p - Q[k] < len(k), and a separator otherwise (every byte no token covers is one).  Tokens of
// length 0 (unk_len == 0) repeat a Q value; "the last k" skips them.
//
//   k_dec_check     strict mode only: one workgroup per kChunk ids, flags an id outside the vocabulary;
//   k_dec_rows      one thread per row_off entry: range, order and end points (an error word, no
//                   atomics), and, with a separator, mark[v] = the number of rows that end just
//                   before id v, written by the first row of each run of equal offsets (the run's
//                   end by binary search), so no two threads write one entry;
//   hipCUB scan     inclusive sum over k = 0 .. n of mark[k] + len(k - 1) through a transform
//                   iterator on (ids, tok_off, mark): Q[0 .. n];
//   k_dec_byte_off  one thread per row: byte_off[r] = Q[row_off[r]] - #{r' >= 1 : row_off[r'] <=
//                   row_off[r]} + r  (= P[row_off[r]] + r);
//   k_dec_expand    output-centric: one workgroup per kTile output bytes.  Its first token by a
//                   binary search of Q; rounds of kStage tokens staged in LDS (offset relative to
//                   the tile, arena offset, length; coalesced loads of Q and ids); every lane
//                   makes 16 contiguous output bytes: a binary search of the LDS offsets for the
//                   token under its first byte, then a forward walk; one 16-byte store per lane.
//                   A round resolves the bytes below the Q of the first token it did not stage, so
//                   tiles with more than kStage tokens (short tokens, dropped ids) take more
//                   rounds and a token longer than a tile needs no special case.
// Traffic per output byte at i ids per byte: the scan reads 4 i (ids) and writes 8 i (Q), the
// expansion reads 12 i (Q, ids) and writes 1: 1 + 24 i bytes (7 B at 4 bytes per id), + 8 i with
// rows and a separator (mark cleared and read), + 24 B per row.  The vocabulary (4 B per id +
// its bytes) is read through the caches.
// All global indices are 64-bit; every store is an ordinary vector store.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../host/encoder.h"
#include "encode_common.h"

namespace shred {
namespace {

// One call's (or piece's) arguments, as the kernels take them.
struct DecodeCall {
  const int32_t* ids;
  uint64_t n;
  const int64_t* row;  // nullptr, or rows + 1 entries
  uint64_t rows;
  bool ends;           // check row[0] == 0 and row[rows] == n (a piece's local offsets: no)
  uint32_t tail;       // 1: one separator after the last id (no row_off, the last piece)
  int sep;             // -1 or the byte
  int unk_len;         // -1 strict
  uint64_t unk;        // the replacement's bytes, first in the low byte
  uint64_t base;       // added to every byte offset (bytes of the pieces before)
};

typedef uint64_t u64;

constexpr int kThreads = 256;
constexpr int kChunk = 4096;                      // ids per workgroup of k_dec_check (DECODE_CHUNK)
constexpr int kLaneBytes = 16;
constexpr int kTile = kThreads * kLaneBytes;      // output bytes per workgroup (DECODE_TILE)
constexpr int kStage = 2048;                      // tokens staged in LDS per round
constexpr uint32_t kUnkBase = 0xFFFFFFFFu;        // "arena offset" of an id outside the vocabulary
constexpr int64_t kRelFloor = -(int64_t(1) << 30) - 1;  // further back than any token reaches

__global__ __launch_bounds__(kThreads) void k_dec_check(const int32_t* __restrict__ ids, u64 n, uint32_t vocab,
                                                        u64* __restrict__ err) {
  const u64 cbase = (u64)blockIdx.x * kChunk;
  bool bad = false;
  for (int i = threadIdx.x; i < kChunk; i += kThreads) {
    const u64 k = cbase + (u64)i;
    if (k < n && (uint32_t)ids[k] >= vocab) bad = true;
  }
  if (bad) err[0] = 1;
}

__global__ __launch_bounds__(kThreads) void k_dec_rows(const int64_t* __restrict__ row, u64 rows, u64 n, int ends,
                                                       uint32_t* __restrict__ mark, u64* __restrict__ err) {
  const u64 r = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (r > rows) return;
  const int64_t v = row[r];
  const int64_t prev = r ? row[r - 1] : 0;
  bool bad = v < 0 || (u64)v > n || prev > v;
  if (ends && ((r == 0 && v != 0) || (r == rows && (u64)v != n))) bad = true;
  if (bad) {
    err[1] = 1;
    return;
  }
  if (mark && r >= 1 && (r == 1 || prev != v)) {  // rows r - 1 .. e - 2 end before id v (0 <= v <= n)
    u64 lo = r + 1, hi = rows + 1;
    while (lo < hi) {
      const u64 mid = lo + ((hi - lo) >> 1);
      if (row[mid] <= v) lo = mid + 1; else hi = mid;
    }
    mark[v] = (uint32_t)(lo - r);
  }
}

// Element k of the scan: the separators in front of token k and the length of token k - 1.
struct QInput {
  const int32_t* ids;
  const uint32_t* tok_off;
  const uint32_t* mark;  // nullptr: none
  u64 n;
  uint32_t vocab, unk_len, tail;
  __host__ __device__ __forceinline__ u64 operator()(u64 k) const {
    u64 v = mark ? (u64)mark[k] : 0ull;
    if (k == n) v += tail;
    if (k) {
      const uint32_t id = (uint32_t)ids[k - 1];
      v += id < vocab ? tok_off[id + 1] - tok_off[id] : unk_len;
    }
    return v;
  }
};
typedef hipcub::TransformInputIterator<u64, QInput, hipcub::CountingInputIterator<u64>> QIter;

// First k in [lo, hi) with Q[k] > v, or hi.
__device__ __forceinline__ u64 upper_bound(const u64* __restrict__ Q, u64 lo, u64 hi, u64 v) {
  while (lo < hi) {
    const u64 mid = lo + ((hi - lo) >> 1);
    if (Q[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void k_dec_byte_off(const int64_t* __restrict__ row, u64 rows,
                                                           const u64* __restrict__ Q, int sep, u64 base,
                                                           int64_t* __restrict__ byte_off) {
  const u64 r = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (r > rows) return;
  const int64_t v = row[r];  // validated: 0 <= v <= n, non-decreasing
  u64 o = Q[v];
  if (sep) {                 // Q[v] counts the separators of every row that ends before id v
    u64 lo = 1, hi = rows + 1;
    while (lo < hi) {
      const u64 mid = lo + ((hi - lo) >> 1);
      if (row[mid] <= v) lo = mid + 1; else hi = mid;
    }
    o = o - (lo - 1) + r;
  }
  byte_off[r] = (int64_t)(base + o);
}

__global__ void k_dec_ends(int64_t* __restrict__ byte_off, u64 base, u64 total) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    byte_off[0] = (int64_t)base;
    byte_off[1] = (int64_t)(base + total);
  }
}

template <bool kAligned>
__global__ __launch_bounds__(kThreads) void k_dec_expand(const int32_t* __restrict__ ids, u64 n,
                                                         const u64* __restrict__ Q,
                                                         const uint32_t* __restrict__ tok_off,
                                                         const uint8_t* __restrict__ arena, uint32_t vocab,
                                                         uint32_t unk_len, u64 unk, uint32_t sep,
                                                         uint8_t* __restrict__ out, u64 total) {
  __shared__ int32_t s_rel[kStage + 1];  // Q[k] - tile start, clamped to [kRelFloor, kTile]
  __shared__ uint32_t s_base[kStage];    // arena offset of the token's bytes, or kUnkBase
  __shared__ uint32_t s_len[kStage];
  __shared__ u64 s_k;
  const int tid = threadIdx.x;
  const u64 t0 = (u64)blockIdx.x * kTile;
  const int tlen = (int)(total - t0 < (u64)kTile ? total - t0 : (u64)kTile);
  if (tid == 0) {  // the last k with Q[k] <= t0 (Q[n] = total > t0), or 0 when the tile begins with separators
    const u64 ub = upper_bound(Q, 0, n + 1, t0);
    s_k = ub ? ub - 1 : 0;
  }
  __syncthreads();
  u64 ks = s_k;
  const int p0 = tid * kLaneBytes;
  uint32_t w[kLaneBytes / 4] = {0, 0, 0, 0};
  int cur = 0;
  for (;;) {
    // entries ks .. ks + m - 1 (k == n: the end, no token), and the offset of entry ks + m
    const int m = (int)(n + 1 - ks < (u64)kStage ? n + 1 - ks : (u64)kStage);
    for (int i = tid; i <= m; i += kThreads) {
      const u64 k = ks + (u64)i;
      int64_t rel = kTile;
      if (k <= n) {
        rel = (int64_t)(Q[k] - t0);
        rel = rel < kRelFloor ? kRelFloor : rel > kTile ? (int64_t)kTile : rel;
      }
      s_rel[i] = (int32_t)rel;
      if (i < m) {
        uint32_t b = 0, l = 0;
        if (k < n) {
          const uint32_t id = (uint32_t)ids[k];
          if (id < vocab) {
            b = tok_off[id];
            l = tok_off[id + 1] - b;
          } else {
            b = kUnkBase;
            l = unk_len;
          }
        }
        s_base[i] = b;
        s_len[i] = l;
      }
    }
    __syncthreads();
    // this round resolves the tile's bytes [cur, lim): below the offset of the first entry not staged
    const int lim = s_rel[m] < tlen ? s_rel[m] : tlen;
    const int lo = p0 > cur ? p0 : cur, hi = p0 + kLaneBytes < lim ? p0 + kLaneBytes : lim;
    if (lo < hi) {
      int a = 0, b = m;  // first entry past byte lo
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (s_rel[mid] <= lo) a = mid + 1; else b = mid;
      }
      int j = a - 1;     // -1: separators in front of entry 0
#pragma unroll
      for (int i = 0; i < kLaneBytes; ++i) {
        const int pos = p0 + i;
        if (pos >= lo && pos < hi) {
          while (j + 1 < m && s_rel[j + 1] <= pos) ++j;
          uint32_t byte = sep;
          if (j >= 0) {
            const uint32_t off = (uint32_t)(pos - s_rel[j]);
            if (off < s_len[j]) {
              const uint32_t tb = s_base[j];
              byte = tb == kUnkBase ? (uint32_t)(unk >> (8 * off)) & 255u : (uint32_t)arena[(u64)tb + off];
            }
          }
          w[i >> 2] |= byte << (8 * (i & 3));
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
  if (kAligned && p0 + kLaneBytes <= tlen) {
    *reinterpret_cast<uint4*>(out + g) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int i = 0; i < kLaneBytes; ++i)
      if (p0 + i < tlen) out[g + i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  }
}

// The decode passes' state, allocated on the first decode call: the vocabulary, and scratch grown
// to the largest call seen: 8 B per id (Q), 4 B per id once a call has rows and a separator
// (mark), the scan's scratch.
struct DecodeState : PassState {
  uint32_t vocab = 0;             // 256 + M + the registered specials
  DeviceBuf<uint32_t> tok_off;    // vocab + 1 offsets into arena
  DeviceBuf<uint8_t> arena;       // the bytes of every token
  DeviceBuf<u64> q;               // Q[k]: output offset of token k; Q[n] = the total
  DeviceBuf<uint32_t> mark;       // rows that end just before id k (separators in front of it)
  DeviceBuf<uint8_t> tmp;         // hipCUB scan scratch
  DeviceWords err;                // [0] an id outside the vocabulary, [1] bad row_off
  PinnedWords host;               // total, the two error words
  EventSet<4> ev;
  // host-path staging: ids, row offsets then byte offsets (2 x hrow.cap()), output bytes of a piece
  DeviceBuf<int32_t> hids;
  DeviceBuf<int64_t> hrow;
  DeviceBuf<uint8_t> hout;

  void specials_changed() override {  // the vocabulary holds the specials: rebuilt by the next call
    tok_off.reset();
    arena.reset();
    vocab = 0;
  }

  // n ids, with marks when rows; the vocabulary is the merge list's, then the specials sx_bytes[sx_off[i] ..].
  bool reserve(size_t n, size_t rows, const std::vector<int32_t>& first, const std::vector<int32_t>& second,
               const std::vector<uint8_t>& sx_bytes, const std::vector<uint32_t>& sx_off) {
    if (!tok_off.get()) {
      std::vector<uint32_t> off;
      std::vector<uint8_t> bytes;
      if (!enc_build_arena(first, second, &off, &bytes)) return false;
      for (size_t i = 0; i + 1 < sx_off.size(); ++i) {  // the special tokens: ids 256 + M + i
        bytes.insert(bytes.end(), sx_bytes.begin() + sx_off[i], sx_bytes.begin() + sx_off[i + 1]);
        off.push_back((uint32_t)bytes.size());
      }
      arena.reset();
      if (!arena.grow(bytes.size()) || !tok_off.grow(off.size()) ||
          hipMemcpy(arena.get(), bytes.data(), bytes.size(), hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(tok_off.get(), off.data(), off.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        tok_off.reset();
        return false;
      }
      vocab = (uint32_t)(off.size() - 1);
    }
    if (!err.ensure(2) || !host.ensure(4) || !ev.ensure() || !q.grow(n + 1) || (rows && !mark.grow(n + 1))) return false;
    size_t need = 0;
    QInput in{nullptr, tok_off.get(), nullptr, (u64)n, vocab, 0, 0};
    if (hipcub::DeviceScan::InclusiveSum(nullptr, need, QIter(hipcub::CountingInputIterator<u64>(0), in), q.get(),
                                         (u64)n + 1) != hipSuccess)
      return false;
    return tmp.grow(std::max<size_t>(need, 16));
  }

  // Length passes over c's device ids and row offsets (whose end points are checked when c.ends):
  // Q into q, *total = the bytes needed.  0, -1, -6.
  int lengths(const DecodeCall& c, hipStream_t st, uint64_t* total) {
    const bool marks = c.sep >= 0 && c.row && c.rows;
    ENC_OK(hipMemsetAsync(err.get(), 0, 16, st));
    if (c.unk_len < 0 && c.n) {
      k_dec_check<<<dim3((unsigned)((c.n + kChunk - 1) / kChunk)), dim3(kThreads), 0, st>>>(c.ids, c.n, vocab,
                                                                                            err.get());
      ENC_OK(hipGetLastError());
    }
    if (marks) ENC_OK(hipMemsetAsync(mark.get(), 0, (c.n + 1) * 4, st));
    if (c.row) {
      k_dec_rows<<<dim3((unsigned)((c.rows + kThreads) / kThreads)), dim3(kThreads), 0, st>>>(
          c.row, c.rows, c.n, c.ends ? 1 : 0, marks ? mark.get() : nullptr, err.get());
      ENC_OK(hipGetLastError());
    }
    QInput in{c.ids, tok_off.get(), marks ? mark.get() : nullptr, c.n, vocab,
              c.unk_len > 0 ? (uint32_t)c.unk_len : 0u, c.tail};
    size_t bytes = tmp.cap();
    ENC_OK(hipcub::DeviceScan::InclusiveSum(tmp.get(), bytes, QIter(hipcub::CountingInputIterator<u64>(0), in),
                                            q.get(), c.n + 1, st));
    ENC_OK(hipMemcpyAsync(host.get(), q.get() + c.n, 8, hipMemcpyDeviceToHost, st));
    ENC_OK(hipMemcpyAsync(host.get() + 1, err.get(), 16, hipMemcpyDeviceToHost, st));
    ENC_OK(hipStreamSynchronize(st));
    if (host[2]) return -6;
    if (host[1]) return -1;
    *total = host[0];
    return 0;
  }

  // byte_off (nullptr, or as the header defines it, plus c.base) and the total bytes into out.
  int expand(const DecodeCall& c, uint64_t total, uint8_t* out, int64_t* byte_off, hipStream_t st) {
    if (byte_off) {
      if (c.row)
        k_dec_byte_off<<<dim3((unsigned)((c.rows + kThreads) / kThreads)), dim3(kThreads), 0, st>>>(
            c.row, c.rows, q.get(), c.sep >= 0 ? 1 : 0, c.base, byte_off);
      else
        k_dec_ends<<<dim3(1), dim3(64), 0, st>>>(byte_off, c.base, total);
      ENC_OK(hipGetLastError());
    }
    if (total) {
      const u64 tiles = (total + kTile - 1) / kTile;
      const bool aligned = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
      (aligned ? k_dec_expand<true> : k_dec_expand<false>)<<<dim3((unsigned)tiles), dim3(kThreads), 0, st>>>(
          c.ids, c.n, q.get(), tok_off.get(), arena.get(), vocab, c.unk_len > 0 ? (uint32_t)c.unk_len : 0u, c.unk,
          c.sep >= 0 ? (uint32_t)c.sep : 0u, out, total);
      ENC_OK(hipGetLastError());
    }
    return 0;
  }
};

u64 pack_unk(const uint8_t* unk, int unk_len) {
  u64 v = 0;
  for (int i = 0; i < unk_len; ++i) v |= (u64)unk[i] << (8 * i);
  return v;
}
// Grids are one workgroup per chunk / tile / 256 rows.
bool grids_fit(u64 n, u64 rows) { return n / kChunk < 0x7FFFFFFFull && rows / kThreads < 0x7FFFFFFFull; }
}  // namespace

int64_t EncodeDevice::decode(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, uint8_t* out,
                             size_t cap, int64_t* byte_off, int sep, const uint8_t* unk, int unk_len,
                             const std::vector<int32_t>& first, const std::vector<int32_t>& second, void* stream,
                             double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  if (!grids_fit(n, rows)) return -1;
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  DecodeState& ds = pass_state<DecodeState>(pass_[kDecode]);
  if (!ds.reserve(n, row_off && sep >= 0 ? rows : 0, first, second, sx_bytes_, sx_off_)) {
    std::fprintf(stderr, "[ERROR]\t encoder: decode allocation failed (%zu ids)\n", n);
    return -1;
  }
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)stream_;
  const EventSet<4>& ev = ds.ev;
  const DecodeCall c{ids, n, row_off, rows, true, (!row_off && sep >= 0) ? 1u : 0u, sep, unk_len,
                     pack_unk(unk, unk_len), 0};
  u64 total = 0;
  ENC_OK(hipEventRecord(ev[0], st));
  const int r = ds.lengths(c, st, &total);
  if (r < 0) return r;
  ENC_OK(hipEventRecord(ev[1], st));
  const bool expand = out && total <= cap;
  if (expand) {
    if (total / kTile >= 0x7FFFFFFFull) return -1;
    ENC_OK(hipEventRecord(ev[2], st));
    if (ds.expand(c, total, out, byte_off, st) < 0) return -1;
    ENC_OK(hipEventRecord(ev[3], st));
  }
  ENC_OK(hipStreamSynchronize(st));
  if (kernel_ms) ENC_OK(ev.sum_ms(expand ? 2 : 1, kernel_ms));
  return (int64_t)total;
}

// Host ids in pieces of at most kDecodePiece ids, cut at any id.  Row r ends "before id row_off[r +
// 1]"; a piece [a, b) takes the row ends in (a, b] (the first piece those at 0 too), so the empty
// rows on a cut go to the piece before it, and a row that runs over the cut gets its separator
// from the piece that holds its end.  Each piece's byte offsets get the bytes written before it.
int64_t EncodeDevice::decode_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, uint8_t* out,
                                  int64_t* byte_off, int sep, const uint8_t* unk, int unk_len,
                                  const std::vector<int32_t>& first, const std::vector<int32_t>& second) {
  if (!grids_fit(n, rows)) return -1;
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  const size_t piece = std::min(piece_from_env("SHREDWORD_DECODE_PIECE", kDecodePiece, 1), std::max<size_t>(n, 1));
  DecodeState& ds = pass_state<DecodeState>(pass_[kDecode]);
  hipStream_t st = (hipStream_t)stream_;
  const u64 unk_bytes = pack_unk(unk, unk_len);
  std::vector<int64_t> local;
  size_t a = 0, r_next = 1;
  u64 done = 0;
  if (byte_off) byte_off[0] = 0;
  do {
    const size_t b = std::min(n, a + piece), len = b - a;
    size_t r_end = r_next;
    local.assign(1, 0);
    if (row_off)
      for (; r_end <= rows && (size_t)row_off[r_end] <= b; ++r_end) local.push_back(row_off[r_end] - (int64_t)a);
    const size_t m = r_end - r_next;
    if (!ds.reserve(len, sep >= 0 ? m : 0, first, second, sx_bytes_, sx_off_) || !ds.hids.grow(std::max(len, piece)) ||
        !ds.hrow.grow(m + 1, 2)) {
      std::fprintf(stderr, "[ERROR]\t encoder: decode allocation failed (%zu ids)\n", len);
      return -1;
    }
    int64_t* drow = ds.hrow.get();
    int64_t* dboff = drow + ds.hrow.cap();
    if (len) ENC_OK(hipMemcpyAsync(ds.hids.get(), ids + a, len * 4, hipMemcpyHostToDevice, st));
    if (m) ENC_OK(hipMemcpyAsync(drow, local.data(), (m + 1) * 8, hipMemcpyHostToDevice, st));
    const DecodeCall c{ds.hids.get(), len, m ? drow : nullptr, m, false, (!row_off && sep >= 0 && b == n) ? 1u : 0u,
                       sep, unk_len, unk_bytes, done};
    u64 total = 0;
    if (ds.lengths(c, st, &total) < 0) return -1;  // (the caller has validated ids and row_off)
    if (!ds.hout.grow((size_t)total)) {
      std::fprintf(stderr, "[ERROR]\t encoder: decode staging allocation failed (%zu bytes)\n", (size_t)total);
      return -1;
    }
    if (total / kTile >= 0x7FFFFFFFull) return -1;
    if (ds.expand(c, total, ds.hout.get(), byte_off && m ? dboff : nullptr, st) < 0) return -1;
    if (total) ENC_OK(hipMemcpyAsync(out + done, ds.hout.get(), total, hipMemcpyDeviceToHost, st));
    if (byte_off && m) ENC_OK(hipMemcpyAsync(byte_off + r_next, dboff + 1, m * 8, hipMemcpyDeviceToHost, st));
    ENC_OK(hipStreamSynchronize(st));
    done += total;
    r_next = r_end;
    a = b;
  } while (a < n);
  if (byte_off && !row_off) byte_off[1] = (int64_t)done;
  return (int64_t)done;
}

}  // namespace shred
