// Batches of documents on gfx950: rows cut at given byte offsets (C ABI and the semantics:
// include/shredword_encode.h, shred_encode_docs*).  The passes run around the encoder
// (encode_device.hip, encode_special.hip) and the span passes (encode_spans.hip) and change none
// of their kernels.
//
// A document boundary is a zero-width delimiter, and rows are documents, not lines.  Both follow
// from one copy of the text in which every document is followed by a '\n' and holds none itself:
// the encoder then sees no word, merge or special across a boundary ('\n' is a delimiter and no
// special holds one), and the span passes' lines are exactly the documents.
//
//   k_docs_check    one thread per doc_off entry: first entry 0, last entry n, non-decreasing (an
//                   error word, no atomics); the host reads it before anything else runs.
//   k_docs_expand   the copy, n + docs bytes: document d goes to offset B[d] = doc_off[d] + d, its
//                   '\n' bytes become ' ' (a delimiter too, so the words are unchanged), and one
//                   '\n' follows it at B[d + 1] - 1.  One workgroup per 4096 output bytes, 16 per
//                   thread: two binary searches of B bound the tile's documents [d0, d1] (none when
//                   the tile lies inside one document); their B entries are staged in LDS (up to
//                   1024 documents per tile, else searched in global memory), each thread finds the
//                   document of its first byte there.  16 bytes inside one document: one 16-byte
//                   load at the document's shift (any alignment), '\n' -> ' ' on four words, one
//                   aligned 16-byte store.  16 bytes that meet a boundary: a byte walk that steps
//                   through the documents, then the same store.
//   encode() / encode_special()  on the copy: the ids.
//   span_passes()   on the copy: starts (byte offsets in the copy) and its line offsets, which
//                   are row_off: every document ends in one of the only '\n' bytes the copy has.
//   k_docs_starts   starts[k] -= row of k (the '\n' bytes in front of token k's document): per
//                   1024 ids two binary searches of row_off bound the rows in reach (almost always
//                   one or a few), then one search per id among them.
// Traffic per text byte on top of encode + spans on n + docs bytes: 1 B read + 1 B written by the
// copy, 8 B per document of doc_off read twice (L2), and with starts 16 B x ids / byte (read and
// written) + row_off reads that stay in L2.
// All global indices are 64-bit; every store is an ordinary vector store.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../host/encoder.h"
#include "encode_common.h"

namespace shred {
namespace {

typedef uint64_t u64;

constexpr int kThreads = 256;
constexpr int kLane = 16;                  // output bytes per thread
constexpr int kTile = kThreads * kLane;    // output bytes per workgroup (the span passes' chunk)
constexpr int kStage = 1024;               // documents of a tile whose offsets are staged in LDS
constexpr int kIdTile = 4 * kThreads;      // ids per workgroup of k_docs_starts

// Last d in [lo, hi] with at(d) <= v; the caller guarantees at(lo) <= v.
template <typename At>
__device__ __forceinline__ u64 last_not_above(u64 lo, u64 hi, u64 v, At at) {
  while (lo < hi) {
    const u64 mid = lo + ((hi - lo + 1) >> 1);
    if (at(mid) <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void k_docs_check(const int64_t* __restrict__ doc_off, u64 docs, u64 n,
                                                         u64* __restrict__ flag) {
  const u64 i = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (i > docs) return;
  const int64_t v = doc_off[i];
  bool bad = v < 0 || (u64)v > n || (i == 0 && v != 0) || (i == docs && (u64)v != n);
  if (!bad && i < docs) bad = v > doc_off[i + 1];
  if (bad) *flag = 1;  // several threads may store at once, on purpose: all store the same value
}

// 0x80 in every byte of w that equals '\n'.
__device__ __forceinline__ uint32_t newline_bytes(uint32_t w) {
  const uint32_t x = w ^ 0x0A0A0A0Au;
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// rows >= 1 documents (doc_off == nullptr: one document of n bytes); out holds n + rows bytes
// rounded up to a multiple of kLane.
__global__ __launch_bounds__(kThreads) void k_docs_expand(const uint8_t* __restrict__ text, u64 n,
                                                          const int64_t* __restrict__ doc_off, u64 rows,
                                                          uint8_t* __restrict__ out) {
  __shared__ u64 s_d[2];
  __shared__ u64 s_b[kStage + 1];
  const int tid = threadIdx.x;
  const u64 total = n + rows;
  const u64 t0 = (u64)blockIdx.x * kTile;  // < total: the grid covers total bytes
  const u64 t1 = t0 + kTile < total ? t0 + kTile : total;
  // B[d], d in [0, rows]: where document d starts in the copy; B[rows] = total
  auto B = [&](u64 d) -> u64 { return (doc_off ? (u64)doc_off[d] : (d ? n : 0)) + d; };
  if (tid == 0) s_d[0] = last_not_above(0, rows - 1, t0, B);
  if (tid == 64) s_d[1] = last_not_above(0, rows - 1, t1 - 1, B);
  __syncthreads();
  const u64 d0 = s_d[0], d1 = s_d[1];  // the documents of the tile's first and last byte
  const bool staged = d1 - d0 + 1 <= (u64)kStage;
  if (staged)
    for (u64 i = tid; i <= d1 - d0 + 1; i += kThreads) s_b[i] = B(d0 + i);  // B[d0 .. d1 + 1]
  __syncthreads();
  auto Bt = [&](u64 d) -> u64 { return staged ? s_b[d - d0] : B(d); };
  const u64 o = t0 + (u64)tid * kLane;
  if (o >= total) return;
  u64 d = d0 == d1 ? d0 : last_not_above(d0, d1, o, Bt);
  u64 next = Bt(d + 1);  // one past this document's '\n'
  uint32_t w[4];
  if (o + kLane < next) {  // 16 bytes of one document, its '\n' not among them
    __builtin_memcpy(w, text + (o - d), kLane);
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] ^= (newline_bytes(w[i]) >> 7) * 0x2Au;  // 0x0A -> 0x20
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = 0x20202020u;
    for (int i = 0; i < kLane && o + i < total; ++i) {
      const u64 p = o + i;
      while (p >= next) {  // p < total = B[rows]: stops at a document <= d1
        ++d;
        next = Bt(d + 1);
      }
      uint32_t c = 10;
      if (p != next - 1) {
        c = text[p - d];
        if (c == 10u) c = 32u;
      }
      w[i >> 2] = (w[i >> 2] & ~(255u << (8 * (i & 3)))) | c << (8 * (i & 3));
    }
  }
  *reinterpret_cast<uint4*>(out + o) = make_uint4(w[0], w[1], w[2], w[3]);
}

// starts[k] -= the row of id k: the last r in [0, rows) with row_off[r] <= k (row_off[0] = 0 and
// k < T = row_off[rows], so it exists and is not an empty row).
__global__ __launch_bounds__(kThreads) void k_docs_starts(int64_t* __restrict__ starts, u64 T,
                                                          const int64_t* __restrict__ row_off, u64 rows) {
  __shared__ u64 s_r[2];
  const u64 k0 = (u64)blockIdx.x * kIdTile;
  const u64 k1 = k0 + kIdTile < T ? k0 + kIdTile : T;
  auto R = [&](u64 r) -> u64 { return (u64)row_off[r]; };
  if (threadIdx.x == 0) s_r[0] = last_not_above(0, rows - 1, k0, R);
  if (threadIdx.x == 64) s_r[1] = last_not_above(0, rows - 1, k1 - 1, R);
  __syncthreads();
  const u64 r0 = s_r[0], r1 = s_r[1];
  for (u64 k = k0 + threadIdx.x; k < k1; k += kThreads)
    starts[k] -= (int64_t)(r0 == r1 ? r0 : last_not_above(r0, r1, k, R));
}

// The document passes' state, allocated on the first docs call.  Scratch grown to the largest call
// seen: 1 B per byte of the copy (text bytes + documents).
struct DocsState : PassState {
  DeviceBuf<uint8_t> text;   // the copy: every document followed by a '\n', none inside
  DeviceWords flag;          // bad doc_off
  PinnedWords host;          // the flag
  EventSet<6> ev;            // around the check, the copy, the starts pass
  // host-path staging: a piece's document offsets, row offsets, starts (text and ids: HostStage)
  DeviceBuf<int64_t> hoff, hrow, hstarts;

  bool reserve(size_t total) {
    return flag.ensure(1) && host.ensure(1) && ev.ensure() && text.grow((total + kTile - 1) / kTile * kTile);
  }
};

}  // namespace

int64_t EncodeDevice::encode_docs(const uint8_t* text, size_t n, const int64_t* doc_off, size_t docs, bool specials,
                                  int32_t* out, size_t cap, int64_t* starts, int64_t* row_off, uint64_t start_base,
                                  const std::vector<int32_t>& lens, void* stream, double* kernel_ms,
                                  uint64_t pos_base) {
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = kernel_ms[3] = 0;
  if (!row_off || (n && (!text || !out)) || (!doc_off && docs)) return -1;
  const size_t rows = doc_off ? docs : 1;
  if (rows > SIZE_MAX - n) return -1;
  const size_t total = n + rows;
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  DocsState& dx = pass_state<DocsState>(pass_[kDocs]);
  if (!dx.reserve(total)) {
    std::fprintf(stderr, "[ERROR]\t encoder: document scratch allocation failed (%zu bytes)\n", total);
    return -1;
  }
  uint8_t* const copy = dx.text.get();
  if (!out) {  // n == 0: no id, but the encoder wants a pointer
    out = reinterpret_cast<int32_t*>(copy);
    cap = 0;
  }
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)stream_;
  const EventSet<6>& ev = dx.ev;
  ENC_OK(hipEventRecord(ev[0], st));
  if (doc_off) {
    ENC_OK(hipMemsetAsync(dx.flag.get(), 0, 8, st));
    k_docs_check<<<dim3((unsigned)(((u64)docs + kThreads) / kThreads)), dim3(kThreads), 0, st>>>(doc_off, (u64)docs,
                                                                                               (u64)n, dx.flag.get());
    ENC_OK(hipGetLastError());
    ENC_OK(hipMemcpyAsync(dx.host.get(), dx.flag.get(), 8, hipMemcpyDeviceToHost, st));
    ENC_OK(hipEventRecord(ev[1], st));
    ENC_OK(hipStreamSynchronize(st));
    if (dx.host[0]) return -6;
  } else {
    ENC_OK(hipEventRecord(ev[1], st));
  }
  if (rows == 0) {  // no document (and, as checked, no text): row_off = [0]
    ENC_OK(hipMemsetAsync(row_off, 0, 8, st));
    ENC_OK(hipStreamSynchronize(st));
    return 0;
  }
  ENC_OK(hipEventRecord(ev[2], st));
  k_docs_expand<<<dim3((unsigned)(((u64)total + kTile - 1) / kTile)), dim3(kThreads), 0, st>>>(text, (u64)n, doc_off,
                                                                                             (u64)rows, copy);
  ENC_OK(hipGetLastError());
  ENC_OK(hipEventRecord(ev[3], st));
  double enc_ms = 0, special_ms = 0, span_ms = 0;
  // (dropout's positions are offsets in the copy: shredword_encode.h)
  const int64_t T = specials ? encode_special(copy, total, out, cap, lens, stream, &enc_ms, &special_ms, pos_base)
                             : encode(copy, total, out, cap, stream, &enc_ms, pos_base);
  if (T < 0) return T;
  ENC_OK(hipSetDevice(device_));  // (encode's guard restored the caller's)
  size_t nl = 0;
  uint8_t last = 0;
  // every document ends in one of the copy's '\n' bytes: row_off[1 .. rows] are its line entries
  if (span_passes(copy, total, out, (size_t)T, starts, row_off, rows + 1, start_base, 0, false, lens, st, &nl,
                  &last, &span_ms) < 0)
    return -1;
  ENC_OK(hipMemsetAsync(row_off, 0, 8, st));
  ENC_OK(hipEventRecord(ev[4], st));
  if (starts && T) {
    k_docs_starts<<<dim3((unsigned)(((u64)T + kIdTile - 1) / kIdTile)), dim3(kThreads), 0, st>>>(starts, (u64)T,
                                                                                               row_off, (u64)rows);
    ENC_OK(hipGetLastError());
  }
  ENC_OK(hipEventRecord(ev[5], st));
  ENC_OK(hipStreamSynchronize(st));
  if (kernel_ms) {
    float a = 0, b = 0, c = 0;  // the check, the copy, the starts pass
    ENC_OK(ev.pair_ms(0, &a));
    ENC_OK(ev.pair_ms(1, &b));
    ENC_OK(ev.pair_ms(2, &c));
    kernel_ms[0] = enc_ms;
    kernel_ms[1] = span_ms;
    kernel_ms[2] = special_ms;
    kernel_ms[3] = (double)a + (double)b + (double)c;
    if (std::getenv("SHREDWORD_ENCODE_DEBUG"))
      std::fprintf(stderr, "[DEBUG]\t encoder: document passes: check %.4f ms, copy %.4f ms, starts %.4f ms\n", a, b, c);
  }
  return T;
}

// Host text in pieces of whole documents: a piece takes documents while its copy (their bytes + one
// per document) stays within the piece budget of encode_host; a single longer document is a piece
// of its own.  Each piece's starts get its byte base on the device, its row entries the id count
// of the pieces before it on the host.  The word limit and (when cap is below the text's
// non-delimiter bytes) the id count are settled before any output is written.
int64_t EncodeDevice::encode_docs_host(const uint8_t* text, size_t n, const int64_t* doc_off, size_t docs,
                                       bool specials, int32_t* out, size_t cap, int64_t* starts, int64_t* row_off,
                                       const std::vector<int32_t>& lens) {
  if (!row_off || (n && (!text || !out)) || (!doc_off && docs)) return -1;
  if (doc_off) {
    if (doc_off[0] != 0 || doc_off[docs] < 0 || (uint64_t)doc_off[docs] != n) return -6;
    for (size_t d = 0; d < docs; ++d)
      if (doc_off[d] > doc_off[d + 1]) return -6;
  }
  const size_t rows = doc_off ? docs : 1;
  if (rows == 0) {
    row_off[0] = 0;
    return 0;
  }
  auto doc_begin = [&](size_t d) -> size_t { return doc_off ? (size_t)doc_off[d] : (d ? n : 0); };
  // the word limit after the cut, and an upper bound of the id count
  size_t non_delim = 0;
  for (size_t d = 0; d < rows; ++d) {
    size_t run = 0;
    for (size_t p = doc_begin(d), e = doc_begin(d + 1); p < e; ++p) {
      run = host_is_delim(text[p]) ? 0 : run + 1;
      non_delim += run != 0;
      if (run > max_word()) return -3;
    }
  }
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  const size_t piece = piece_from_env("SHREDWORD_ENCODE_PIECE", kHostPiece, (size_t)kEncMaxWord + 2);
  HostStage& hs = pass_state<HostStage>(pass_[kStage]);
  DocsState& dx = pass_state<DocsState>(pass_[kDocs]);
  hipStream_t st = (hipStream_t)stream_;
  std::vector<int64_t> hoff, hrow;
  // pass 0 (only when cap may be too small): the id count alone; pass 1: the outputs
  for (int pass = cap < non_delim ? 0 : 1; pass < 2; ++pass) {
    size_t d = 0, done = 0;
    while (d < rows) {
      size_t e = d + 1;
      while (e < rows && (doc_begin(e + 1) - doc_begin(d)) + (e + 1 - d) <= piece) ++e;
      const size_t pos = doc_begin(d), len = doc_begin(e) - pos, nd = e - d;
      if (!hs.reserve(std::max<size_t>(len, 1)) || !dx.hoff.grow(nd + 1) || !dx.hrow.grow(nd + 1) ||
          (starts && !dx.hstarts.grow(len))) {
        std::fprintf(stderr, "[ERROR]\t encoder: staging allocation failed (%zu bytes, %zu documents)\n", len, nd);
        return -1;
      }
      if (len) ENC_OK(hipMemcpyAsync(hs.text.get(), text + pos, len, hipMemcpyHostToDevice, st));
      if (doc_off) {
        hoff.resize(nd + 1);
        for (size_t j = 0; j <= nd; ++j) hoff[j] = doc_off[d + j] - (int64_t)pos;
        ENC_OK(hipMemcpyAsync(dx.hoff.get(), hoff.data(), (nd + 1) * 8, hipMemcpyHostToDevice, st));
        ENC_OK(hipStreamSynchronize(st));  // (hoff is pageable and reused)
      }
      const size_t room = pass ? std::min(cap - done, hs.out.cap()) : hs.out.cap();
      const int64_t r = encode_docs(hs.text.get(), len, doc_off ? dx.hoff.get() : nullptr, doc_off ? nd : 0, specials,
                                    hs.out.get(), room, pass && starts ? dx.hstarts.get() : nullptr, dx.hrow.get(),
                                    (uint64_t)pos, lens, nullptr, nullptr, (uint64_t)(pos + d));
      if (r < 0) return r;
      ENC_OK(hipSetDevice(device_));
      const size_t T = (size_t)r;
      if (pass) {
        hrow.resize(nd + 1);
        if (T) ENC_OK(hipMemcpyAsync(out + done, hs.out.get(), T * 4, hipMemcpyDeviceToHost, st));
        if (starts && T) ENC_OK(hipMemcpyAsync(starts + done, dx.hstarts.get(), T * 8, hipMemcpyDeviceToHost, st));
        ENC_OK(hipMemcpyAsync(hrow.data(), dx.hrow.get(), (nd + 1) * 8, hipMemcpyDeviceToHost, st));
        ENC_OK(hipStreamSynchronize(st));
        for (size_t j = 0; j <= nd; ++j) row_off[d + j] = (int64_t)done + hrow[j];
      }
      done += T;
      d = e;
    }
    if (!pass && done > cap) return -2;
  }
  return row_off[rows];
}

}  // namespace shred
