// Token byte offsets and per-line id offsets of an encoded text on gfx950 (C ABI and definitions:
// include/shredword_encode.h, shred_encode_spans*).  The passes run behind the encoder
// (encode_device.hip) on its output and touch none of its kernels.
//
// Ids come out in text order, no token spans a delimiter, and id x covers len(x) source bytes
// (1 below 256, len(first) + len(second) for a merge), so the ids' lengths tile the text's
// non-delimiter bytes in order.  With P[k] the exclusive prefix sum of len(ids[k]) and r(p) the
// number of non-delimiter bytes before byte p, token k starts at the byte of non-delimiter rank
// P[k], and the line after a '\n' at byte p starts at id #{k : P[k] < r(p)}.
//
//   k_span_count    one workgroup per 4096-byte chunk: non-delimiter and '\n' bytes of the chunk
//                   (4 bytes per lane and step, wave64 reduction);
//   hipCUB scans    inclusive sums of both count arrays over the chunks; P over the T ids through
//                   a transform iterator on the length table (4 B x (256 + M), L2-resident);
//   k_span_resolve  one workgroup per chunk: 32-bit non-delimiter / '\n' masks of its 128 spans
//                   (coalesced 4-byte loads -> one nibble pair per load in LDS -> 8 per thread),
//                   block scan of their popcounts, the chunk's id range [k0, k1) by two binary
//                   searches of P against its rank range (a token belongs to the chunk it begins
//                   in); per id: the span by binary search over the LDS scan, then the n-th set
//                   bit of the span's mask, starts[k] stored coalesced over k; per '\n': its
//                   ordinal from the newline scan, the first k in [k0, k1] with P[k] >= r;
//   k_span_ends     line_off[0] = 0, line_off[L] = T.
// Traffic per text byte: 2 B of text + ids/byte x (4 B ids + 8 B P written + 8 B P read + 8 B
// starts) = 2 B + 28 B x ids / byte (9 B at 4 bytes per id), + 8 B per line.
// All global indices are 64-bit; every store is an ordinary vector store.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../host/encoder.h"
#include "encode_common.h"
#include "encode_words.h"  // the encoder's geometry: one thread per 32-byte span, one workgroup per chunk

namespace shred {
namespace {

typedef uint64_t u64;

constexpr int kWords = kChunk / 4;        // 4-byte text words per chunk

// Bits 0-3: bytes of the word outside "\t\r\n "; bits 4-7: bytes equal to '\n'.
__device__ __forceinline__ uint32_t word_nibbles(uint32_t v) {
  uint32_t r = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const uint32_t c = (v >> (8 * b)) & 255u;
    r |= (is_delim(c) ^ 1u) << b | (uint32_t)(c == 10u) << (4 + b);
  }
  return r;
}

// Text word w of the chunk at cbase, bytes past the end read as spaces (a delimiter, no '\n').
template <bool kAligned>
__device__ __forceinline__ uint32_t load_word(const uint8_t* __restrict__ text, u64 n, u64 cbase, int w) {
  const u64 o = cbase + 4 * (u64)w;
  if (o + 4 <= n) {
    if (kAligned) return *reinterpret_cast<const uint32_t*>(text + o);
    return (uint32_t)text[o] | (uint32_t)text[o + 1] << 8 | (uint32_t)text[o + 2] << 16 | (uint32_t)text[o + 3] << 24;
  }
  uint32_t v = 0x20202020u;
  for (int b = 0; b < 4; ++b)
    if (o + b < n) v = (v & ~(255u << (8 * b))) | (uint32_t)text[o + b] << (8 * b);
  return v;
}

template <bool kAligned>
__global__ __launch_bounds__(kThreads) void k_span_count(const uint8_t* __restrict__ text, u64 n,
                                                         u64* __restrict__ nd_cnt, u64* __restrict__ nl_cnt) {
  __shared__ uint32_t s_part[kThreads / 64];
  const int tid = threadIdx.x;
  const u64 cbase = (u64)blockIdx.x * kChunk;
  uint32_t acc = 0;  // non-delimiters | newlines << 16 (each <= 32 per thread)
  for (int w = tid; w < kWords; w += kThreads) {
    const uint32_t nb = word_nibbles(load_word<kAligned>(text, n, cbase, w));
    acc += __popc(nb & 15u) | __popc(nb >> 4) << 16;
  }
  for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d, 64);  // <= 4096 per half: no carry
  if ((tid & 63) == 0) s_part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    uint32_t t = 0;
    for (int i = 0; i < kThreads / 64; ++i) t += s_part[i];
    nd_cnt[blockIdx.x] = t & 0xFFFFu;
    nl_cnt[blockIdx.x] = t >> 16;
  }
}

// Source-byte length of an id: 1 below 256 (a byte's symbol, unk_id included), else the table's.
struct IdLength {
  const int32_t* lens;
  uint32_t limit;  // 256 + M
  __host__ __device__ __forceinline__ u64 operator()(int32_t id) const {
    return ((uint32_t)id >= 256u && (uint32_t)id < limit) ? (u64)lens[id] : 1ull;
  }
};

// First k in [lo, hi) with P[k] >= v, or hi.
__device__ __forceinline__ u64 lower_bound(const u64* __restrict__ P, u64 lo, u64 hi, u64 v) {
  while (lo < hi) {
    const u64 mid = lo + ((hi - lo) >> 1);
    if (P[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Position of the i-th (0-based) set bit of m; i < popc(m).
__device__ __forceinline__ uint32_t select_bit(uint32_t m, uint32_t i) {
  uint32_t pos = 0;
#pragma unroll
  for (int w = 16; w > 0; w >>= 1) {
    const uint32_t c = __popc(m & ((1u << w) - 1u));
    if (i >= c) {
      i -= c;
      m >>= w;
      pos += w;
    }
  }
  return pos;
}

template <bool kAligned>
__global__ __launch_bounds__(kThreads) void k_span_resolve(const uint8_t* __restrict__ text, u64 n,
                                                           const u64* __restrict__ nd_inc, const u64* __restrict__ nl_inc,
                                                           const u64* __restrict__ P, u64 T,
                                                           int64_t* __restrict__ starts, int64_t* __restrict__ line,
                                                           u64 start_base, u64 id_base) {
  __shared__ uint32_t s_nib[kWords / 4];    // one byte per text word: word_nibbles
  __shared__ uint32_t s_mask[kThreads];     // non-delimiter mask of each span
  __shared__ uint32_t s_inc[kThreads];      // inclusive scan of (non-delimiters | newlines << 16)
  __shared__ u64 s_k[2];
  const int tid = threadIdx.x;
  const u64 cbase = (u64)blockIdx.x * kChunk;
  uint8_t* nib = reinterpret_cast<uint8_t*>(s_nib);
  for (int w = tid; w < kWords; w += kThreads) nib[w] = (uint8_t)word_nibbles(load_word<kAligned>(text, n, cbase, w));
  __syncthreads();
  uint32_t nd = 0, nl = 0;  // bit j: byte cbase + 32 tid + j
  {
    const uint32_t a = s_nib[2 * tid], b = s_nib[2 * tid + 1];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t x = (a >> (8 * i)) & 255u, y = (b >> (8 * i)) & 255u;
      nd |= (x & 15u) << (4 * i) | (y & 15u) << (16 + 4 * i);
      nl |= (x >> 4) << (4 * i) | (y >> 4) << (16 + 4 * i);
    }
  }
  const uint32_t mine = __popc(nd) | __popc(nl) << 16;
  s_mask[tid] = nd;
  s_inc[tid] = mine;
  block_inclusive_scan(s_inc, tid);  // each half <= 4096: no carry between them
  const uint32_t total = s_inc[kThreads - 1];
  const uint32_t nd_total = total & 0xFFFFu, nl_total = total >> 16;
  const u64 r1 = nd_inc[blockIdx.x], r0 = r1 - nd_total;  // the chunk's non-delimiter ranks [r0, r1)
  // ids that begin in this chunk: P[k] in [r0, r1).  P[k] >= k bounds both searches from above.
  if (tid == 0) s_k[0] = lower_bound(P, 0, r0 < T ? r0 : T, r0);
  if (tid == 64) s_k[1] = lower_bound(P, 0, r1 < T ? r1 : T, r1);
  __syncthreads();
  const u64 k0 = s_k[0], k1 = s_k[1];
  if (starts) {
    for (u64 k = k0 + tid; k < k1; k += kThreads) {
      const uint32_t r = (uint32_t)(P[k] - r0);  // < nd_total
      const int lo = first_above(s_inc, r, 0xFFFFu);  // the span of the non-delimiter byte of rank r
      const uint32_t m = s_mask[lo];
      const uint32_t before = (s_inc[lo] & 0xFFFFu) - __popc(m);
      const uint32_t i = r - before;
      const uint32_t pos = i < (uint32_t)__popc(m) ? select_bit(m, i) : 0;
      starts[k] = (int64_t)(start_base + cbase + (u64)lo * kSpan + pos);
    }
  }
  if (line && nl) {
    u64 q = nl_inc[blockIdx.x] - nl_total + ((s_inc[tid] >> 16) - (mine >> 16));  // ordinal of this span's first '\n'
    const u64 rs = r0 + ((s_inc[tid] & 0xFFFFu) - (mine & 0xFFFFu));               // rank of the span's first byte
    while (nl) {
      const int j = __ffs(nl) - 1;
      nl &= nl - 1;
      const u64 r = rs + __popc(nd & ((1u << j) - 1u));
      line[q + 1] = (int64_t)(id_base + lower_bound(P, k0, k1, r));
      ++q;
    }
  }
}

__global__ void k_span_ends(int64_t* __restrict__ line, u64 L, u64 T) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    line[L] = (int64_t)T;
    line[0] = 0;  // (L == 0 only for an empty text, where T == 0)
  }
}

typedef hipcub::TransformInputIterator<u64, IdLength, const int32_t*> LengthIter;

// The span passes' state, allocated on the first spans call and grown to the largest call seen:
// 32 B per chunk, 8 B per id, the scans' scratch.
struct SpanState : PassState {
  DeviceBuf<int32_t> lens;      // 256 + M token lengths, then the registered specials'
  DeviceBuf<u64> cnt;           // 4 x chunks: non-delimiter / '\n' counts, their inclusive sums
  DeviceBuf<u64> prefix;        // P[k]: source bytes of the ids before k
  DeviceBuf<uint8_t> tmp;       // hipCUB scan scratch
  PinnedWords host;             // '\n' total, last text byte
  EventSet<4> ev;
  DeviceBuf<int64_t> hstarts, hline;  // host-path staging of the span outputs

  void specials_changed() override { lens.reset(); }

  bool upload_lens(const std::vector<int32_t>& host_lens) {
    if (!lens.get() && (!lens.grow(host_lens.size()) || hipMemcpy(lens.get(), host_lens.data(), host_lens.size() * 4,
                                                                   hipMemcpyHostToDevice) != hipSuccess)) {
      lens.reset();
      return false;
    }
    return true;
  }

  bool reserve(size_t n, size_t T, const std::vector<int32_t>& host_lens) {
    if (!upload_lens(host_lens)) return false;
    const size_t nb = (n + kChunk - 1) / kChunk;
    if (!host.ensure(4) || !ev.ensure() || !cnt.grow(nb, 4) || !prefix.grow(T)) return false;
    size_t a = 0, b = 0;
    if (hipcub::DeviceScan::InclusiveSum(nullptr, a, cnt.get(), cnt.get(), (u64)nb) != hipSuccess) return false;
    if (T && hipcub::DeviceScan::ExclusiveSum(nullptr, b, LengthIter((const int32_t*)nullptr, IdLength{lens.get(), 0}),
                                              prefix.get(), (u64)T) != hipSuccess)
      return false;
    return tmp.grow(std::max<size_t>(std::max(a, b), 16));
  }
};

}  // namespace

const int32_t* EncodeDevice::span_lens(const std::vector<int32_t>& lens) {
  SpanState& sp = pass_state<SpanState>(pass_[kSpans]);
  return sp.upload_lens(lens) ? sp.lens.get() : nullptr;
}

int EncodeDevice::span_passes(const uint8_t* text, size_t n, const int32_t* ids, size_t T, int64_t* starts,
                              int64_t* line, size_t line_cap, uint64_t start_base, uint64_t id_base,
                              bool whole, const std::vector<int32_t>& lens, void* stream, size_t* newlines,
                              uint8_t* last_byte, double* ms) {
  if (ms) *ms = 0;
  if (n == 0) return -1;
  SpanState& sp = pass_state<SpanState>(pass_[kSpans]);
  if (!sp.reserve(n, T, lens)) {
    std::fprintf(stderr, "[ERROR]\t encoder: span scratch allocation failed (%zu bytes, %zu ids)\n", n, T);
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  const EventSet<4>& ev = sp.ev;
  const u64 nb = (n + kChunk - 1) / kChunk;
  const bool aligned = (reinterpret_cast<uintptr_t>(text) & 3) == 0;
  u64 *nd_cnt = sp.cnt.get(), *nl_cnt = nd_cnt + nb, *nd_inc = nd_cnt + 2 * nb, *nl_inc = nd_cnt + 3 * nb;
  ENC_OK(hipEventRecord(ev[0], st));
  (aligned ? k_span_count<true> : k_span_count<false>)<<<dim3((unsigned)nb), dim3(kThreads), 0, st>>>(text, n, nd_cnt,
                                                                                                     nl_cnt);
  ENC_OK(hipGetLastError());
  size_t tmp = sp.tmp.cap();
  ENC_OK(hipcub::DeviceScan::InclusiveSum(sp.tmp.get(), tmp, nd_cnt, nd_inc, nb, st));
  tmp = sp.tmp.cap();
  ENC_OK(hipcub::DeviceScan::InclusiveSum(sp.tmp.get(), tmp, nl_cnt, nl_inc, nb, st));
  sp.host[1] = 0;
  ENC_OK(hipMemcpyAsync(sp.host.get(), nl_inc + nb - 1, 8, hipMemcpyDeviceToHost, st));
  ENC_OK(hipMemcpyAsync(sp.host.get() + 1, text + n - 1, 1, hipMemcpyDeviceToHost, st));
  ENC_OK(hipEventRecord(ev[1], st));
  ENC_OK(hipStreamSynchronize(st));
  const size_t nl = (size_t)sp.host[0];
  *newlines = nl;
  *last_byte = (uint8_t)(sp.host[1] & 255u);
  // the whole text: line[L] follows (k_span_ends); a piece: entries up to line[nl] only
  if (line && line_cap < nl + 1 + (whole && *last_byte != 10)) return -2;
  ENC_OK(hipEventRecord(ev[2], st));
  if (starts || line) {
    if (T) {
      tmp = sp.tmp.cap();
      ENC_OK(hipcub::DeviceScan::ExclusiveSum(sp.tmp.get(), tmp,
                                              LengthIter(ids, IdLength{sp.lens.get(), (uint32_t)lens.size()}),
                                              sp.prefix.get(), (u64)T, st));
    }
    (aligned ? k_span_resolve<true> : k_span_resolve<false>)<<<dim3((unsigned)nb), dim3(kThreads), 0, st>>>(
        text, n, nd_inc, nl_inc, sp.prefix.get(), (u64)T, starts, line, start_base, id_base);
    ENC_OK(hipGetLastError());
  }
  ENC_OK(hipEventRecord(ev[3], st));
  ENC_OK(hipStreamSynchronize(st));
  if (ms) ENC_OK(ev.sum_ms(2, ms));
  return 0;
}

int64_t EncodeDevice::encode_spans(const uint8_t* text, size_t n, int32_t* out, size_t cap, int64_t* starts,
                                   int64_t* line_off, size_t line_cap, size_t* num_lines,
                                   const std::vector<int32_t>& lens, void* stream, double* kernel_ms,
                                   bool specials) {
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0;
  if (kernel_ms && specials) kernel_ms[2] = 0;
  if (num_lines) *num_lines = 0;
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)stream_;
  if (n == 0) {  // L = 0, line_off = [0]
    if (line_off) {
      if (line_cap < 1) return -2;
      ENC_OK(hipMemsetAsync(line_off, 0, 8, st));
      ENC_OK(hipStreamSynchronize(st));
    }
    return 0;
  }
  const int64_t T = specials ? encode_special(text, n, out, cap, lens, stream, kernel_ms, kernel_ms ? kernel_ms + 2 : nullptr)
                             : encode(text, n, out, cap, stream, kernel_ms);
  if (T < 0 || (!starts && !line_off && !num_lines)) return T;
  ENC_OK(hipSetDevice(device_));  // (encode's guard restored the caller's)
  size_t nl = 0;
  uint8_t last = 0;
  double ms = 0;
  const int r = span_passes(text, n, out, (size_t)T, starts, line_off, line_off ? line_cap : 0, 0, 0, true, lens, st,
                            &nl, &last, kernel_ms ? &ms : nullptr);
  const size_t L = nl + (last != 10);
  if (r != -1 && num_lines) *num_lines = L;
  if (r < 0) return r;
  if (line_off) {
    k_span_ends<<<dim3(1), dim3(64), 0, st>>>(line_off, (u64)L, (u64)T);
    ENC_OK(hipGetLastError());
    ENC_OK(hipStreamSynchronize(st));
  }
  if (kernel_ms) kernel_ms[1] = ms;
  return T;
}

// Host text in the pieces of encode_host.  A piece ends after any delimiter, so a line may run
// over several pieces: each piece's starts get its byte base, its line entries the id count and
// the '\n' ordinal carried from the pieces before it, and line_off[L] = T is written at the end.
int64_t EncodeDevice::encode_spans_host(const uint8_t* text, size_t n, int32_t* out, size_t cap, int64_t* starts,
                                        int64_t* line_off, size_t line_cap, size_t* num_lines,
                                        const std::vector<int32_t>& lens, bool specials) {
  if (num_lines) *num_lines = 0;
  if (!specials && !starts && !line_off && !num_lines) return encode_host(text, n, out, cap);
  if (n == 0) {
    if (line_off) {
      if (line_cap < 1) return -2;
      line_off[0] = 0;
    }
    return 0;
  }
  if (!text || !out) return -1;
  const size_t L = count_newlines(text, n) + (text[n - 1] != 10);
  if (num_lines) *num_lines = L;
  if (line_off && line_cap < L + 1) return -2;
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  const size_t piece = std::min(n, piece_from_env("SHREDWORD_ENCODE_PIECE", kHostPiece, (size_t)kEncMaxWord + 2));
  HostStage& hs = pass_state<HostStage>(pass_[kStage]);
  if (!hs.reserve(piece)) {
    std::fprintf(stderr, "[ERROR]\t encoder: staging allocation failed (%zu bytes)\n", piece);
    return -1;
  }
  SpanState& sp = pass_state<SpanState>(pass_[kSpans]);
  uint8_t* dtext = hs.text.get();
  int32_t* dout = hs.out.get();
  hipStream_t st = (hipStream_t)stream_;
  size_t pos = 0, done = 0, lines_done = 0;
  while (pos < n) {
    const size_t len = host_piece_len(text, n, pos, piece, max_word());
    if (len == 0) return -3;
    if (len > hs.text.cap()) {  // a long word that the budget cut is staged whole
      if (!hs.reserve(len)) {
        std::fprintf(stderr, "[ERROR]\t encoder: staging allocation failed (%zu bytes)\n", len);
        return -1;
      }
      dtext = hs.text.get();
      dout = hs.out.get();
    }
    ENC_OK(hipMemcpyAsync(dtext, text + pos, len, hipMemcpyHostToDevice, st));
    const int64_t r = specials ? encode_special(dtext, len, dout, cap - done, lens, nullptr, nullptr, nullptr, (u64)pos)
                               : encode(dtext, len, dout, cap - done, nullptr, nullptr, (u64)pos);
    if (r < 0) return r;
    ENC_OK(hipSetDevice(device_));
    const size_t T = (size_t)r;
    const size_t pnl = line_off ? count_newlines(text + pos, len) : 0;
    if ((starts && !sp.hstarts.grow(T)) || (line_off && !sp.hline.grow(pnl + 1))) {
      std::fprintf(stderr, "[ERROR]\t encoder: staging allocation failed (%zu ids, %zu lines)\n", T, pnl + 1);
      return -1;
    }
    size_t nl = 0;
    uint8_t last = 0;
    // (nothing but the ids wanted: a special call, which has no other host path)
    const int s = !starts && !line_off ? 0
                  : span_passes(dtext, len, dout, T, starts ? sp.hstarts.get() : nullptr,
                                line_off ? sp.hline.get() : nullptr, sp.hline.cap(), (u64)pos, (u64)done, false, lens,
                                st, &nl, &last, nullptr);
    if (s < 0) return -1;  // (-2 cannot happen: the staging holds the piece's own '\n' count + 1)
    if (T) ENC_OK(hipMemcpyAsync(out + done, dout, T * 4, hipMemcpyDeviceToHost, st));
    if (starts && T) ENC_OK(hipMemcpyAsync(starts + done, sp.hstarts.get(), T * 8, hipMemcpyDeviceToHost, st));
    if (line_off && nl)
      ENC_OK(hipMemcpyAsync(line_off + lines_done + 1, sp.hline.get() + 1, nl * 8, hipMemcpyDeviceToHost, st));
    ENC_OK(hipStreamSynchronize(st));
    done += T;
    lines_done += nl;
    pos += len;
  }
  if (line_off) {
    line_off[0] = 0;
    line_off[L] = (int64_t)done;
  }
  return (int64_t)done;
}

}  // namespace shred
