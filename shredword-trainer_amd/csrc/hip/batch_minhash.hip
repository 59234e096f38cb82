// MinHash signatures and LSH band keys of rows of ids on gfx950, for near-duplicate removal between
// "encoded" and "batched" (C ABI and definitions: include/shredword_encode.h, shred_minhash_*).  The
// passes share the batch units' wave search (batch_common.h), their device-call driver and host piece
// loop (batch_state.h) and the seeded draw (draw_hash.h).
//
// A row's signature is a function of (seed, K, w) and the row's ids alone, so a piece of the host
// call is the device call on its own rows.
//
//   k_offsets_check  (encode_common.h) row_off, before anything is written.
//   memset           sig to 0xFF bytes: the signature of a row without shingles, and the identity of min.
//   k_minhash_tiles  the work is split over the flat id stream, not over rows: one workgroup per
//                    kMhTile consecutive shingle positions (a position is the index of a shingle's
//                    first id), so many short rows and one long row load the machine alike.  The rows
//                    that begin in the tile, and the one that holds its first position, are found with
//                    two wave_upper_bound searches of row_off and staged kStage at a time in LDS: the
//                    range of positions that start a shingle of the row ([s, e - w + 1), or [s, s + 1)
//                    for a row shorter than w), clamped to the tile.  Per round of staged rows:
//                      phase 1  one position per thread per step: the row of the position by binary
//                               search in LDS, the w ids from the tile's ids in LDS (loaded once, with
//                               the halo of w - 1 ids past the tile's edge), the mix chain, x to LDS.
//                               Positions that start no shingle are never read back, so no marker.
//                      phase 2  lanes own permutations: lane l of wave block q holds a_i, b_i (drawn
//                               once per thread) and a running minimum for i = 64 q + l (and i + 256
//                               when K > 256).  All lanes of a wave read the same x from LDS, a
//                               broadcast, four positions per 16-byte read; per position and
//                               permutation one 64 x 32 multiply-add and one unsigned minimum.  With
//                               K <= 128 (64) the waves that K does not need take the other half
//                               (quarters) of the tile's positions.  At the end of each staged row's
//                               range a lane writes its minimum to sig[r K + i]: consecutive lanes,
//                               consecutive words.  atomicMin, unless the row's whole range lies in
//                               this wave's share of this tile: then nobody else holds a part of the
//                               row and the lane stores.
//   k_minhash_bands  one thread per (row, band): R = K / B consecutive words of the finished sig
//                    through the mix chain, one 8-byte key out.  Threads read R x 4 B runs that lie
//                    side by side, so a wave's reads cover one contiguous stretch of sig.
//
// LDS per workgroup: 8 KB of x, 8.25 KB of ids, 8 KB of staged rows: 24.3 KB, six workgroups per CU.
// Work per position: w + 1 mix (phase 1) and K multiply-add-min (phase 2); traffic per id: 4 B read,
// and per row 16 B read per tile that holds a part of it and 4 K B written (8 B more per band key).
// No matrix instruction fits: the inner step is a 64-bit integer multiply-add and an unsigned minimum.
// All global indices are 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../host/encoder.h"
#include "batch_common.h"
#include "batch_state.h"
#include "draw_hash.h"
#include "encode_common.h"

namespace shred {
namespace {

constexpr int kMhTile = 2048;  // shingle positions per workgroup (MINHASH_TILE)
constexpr int kMhWaves = kThreads / 64;
constexpr int kMhWhole = 0x100;  // in s_c: the row's whole range of shingle starts lies in this tile
static_assert(EncodeDevice::kMinhashMaxShingle < kMhWhole && EncodeDevice::kMinhashMaxPerm <= 2 * kThreads,
              "a shingle's id count shares a word with the flag; a thread carries at most two permutations");

// The definition's pieces, for the kernels and the asserts below.
constexpr __host__ __device__ u64 mh_start(u64 seed, u64 c) { return draw(seed, c, kMhShingle); }
constexpr __host__ __device__ u64 mh_a(u64 seed, u64 i) { return draw(seed, i, kMhA) | 1; }
constexpr __host__ __device__ u64 mh_b(u64 seed, u64 i) { return draw(seed, i, kMhB); }
constexpr __host__ __device__ uint32_t mh_value(u64 a, u64 b, uint32_t x) { return (uint32_t)((a * (u64)x + b) >> 32); }

// Values of the definition as the tests' numpy reference computes it: the one-id row [7] under seed 3
// (w = 1), permutations 0 and 511, and its key as band 0 of one word.
constexpr uint32_t kMhX7 = (uint32_t)(fmix64(mh_start(3, 1) ^ 7) >> 32);
static_assert(mh_value(mh_a(3, 0), mh_b(3, 0), kMhX7) == 0xfdd551deu, "minhash");
static_assert(mh_value(mh_a(3, 511), mh_b(3, 511), kMhX7) == 0x3edb57aau, "minhash");
static_assert(fmix64(draw(3, 0, kMhBand) ^ 0xfdd551deull) == 0x25205c6200e80766ull, "minhash");

// What the kernels know of a call's options; passed by value.
struct MhRule {
  u64 seed, h0;  // h0 = h_0 of a shingle of w ids
  int K, w, B;
  int cover;     // waves that together hold permutations 0 .. min(K, 256) - 1: 1, 2 or 4
};

MhRule rule_of(const EncodeDevice::MinhashOpts& o) {
  const int cover = o.K <= 64 ? 1 : o.K <= 128 ? 2 : kMhWaves;
  return MhRule{o.seed, mh_start(o.seed, (u64)o.w), o.K, o.w, o.B, cover};
}

// Positions [0, n) of the id stream, n >= 1; row: rows + 1 good offsets.  sig was preset to 0xFF bytes.
// P: permutations per thread, 2 when K > 256.
template <int P>
__global__ __launch_bounds__(kThreads) void k_minhash_tiles(const int32_t* __restrict__ ids, u64 n,
                                                            const int64_t* __restrict__ row, u64 rows, MhRule rule,
                                                            uint32_t* __restrict__ sig) {
  __shared__ __attribute__((aligned(16))) uint32_t s_x[kMhTile];
  __shared__ uint32_t s_ids[kMhTile + EncodeDevice::kMinhashMaxShingle];
  // per staged row, relative to the tile and clamped to [0, T]: its first id, its shingle starts [vlo, vhi)
  __shared__ int s_beg[kStage], s_vlo[kStage], s_vhi[kStage];
  __shared__ int s_c[kStage];  // ids per shingle of the row (w, or the length of a shorter row) | kMhWhole
  __shared__ int s_lim;
  __shared__ u64 s_k[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u64 t0 = (u64)blockIdx.x * kMhTile;
  const int T = (int)(n - t0 < (u64)kMhTile ? n - t0 : (u64)kMhTile);
  const int w = rule.w, K = rule.K;
  const auto rel = [&](u64 v) { return v <= t0 ? 0 : v - t0 >= (u64)T ? T : (int)(v - t0); };

  // the tile's ids and the halo: a shingle that starts in the tile ends at most w - 1 ids past it
  const int have = (int)(n - t0 < (u64)(kMhTile + w - 1) ? n - t0 : (u64)(kMhTile + w - 1));
  for (int q = tid; q < have; q += kThreads) s_ids[q] = (uint32_t)ids[t0 + q];
  if (tid < 64) {
    // rows [ks, kend) hold the tile's positions or are empty rows among them: ks is the last k with
    // row[k] <= t0 (row[0] = 0 and row[rows] = n > t0, so 0 <= ks < rows), kend the number of entries
    // at or before the tile's last position (<= rows)
    const u64* E = reinterpret_cast<const u64*>(row);
    const u64 ub = wave_upper_bound(E, 0, rows + 1, t0, tid);
    const u64 ue = wave_upper_bound(E, ub, rows + 1, t0 + (u64)T - 1, tid);
    if (tid == 0) s_k[0] = ub - 1, s_k[1] = ue;
  }

  // this thread's permutations, and this wave's share of the tile's positions
  const int cover = rule.cover, sub = kMhTile / (kMhWaves / cover);
  const int sub_lo = (wave / cover) * sub, sub_hi = sub_lo + sub;
  int perm[P];
  u64 a[P], b[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    perm[j] = (wave % cover) * 64 + lane + j * kThreads;
    a[j] = mh_a(rule.seed, (u64)perm[j]);
    b[j] = mh_b(rule.seed, (u64)perm[j]);
  }
  __syncthreads();
  u64 ks = s_k[0];
  const u64 kend = s_k[1];
  int cur = 0;
  for (;;) {
    const int m = (int)(kend - ks < (u64)kStage ? kend - ks : (u64)kStage);
    for (int i = tid; i < m; i += kThreads) {
      const u64 s = (u64)row[ks + (u64)i], e = (u64)row[ks + (u64)i + 1];
      const u64 len = e - s, c = len < (u64)w ? len : (u64)w;
      const u64 ve = len ? e - c + 1 : s;  // the row's shingles start at [s, ve)
      s_beg[i] = s_vlo[i] = rel(s);
      s_vhi[i] = rel(ve);
      s_c[i] = (int)c | (s >= t0 && ve <= t0 + (u64)T ? kMhWhole : 0);
    }
    if (tid == 0) s_lim = ks + (u64)m < kend ? rel((u64)row[ks + (u64)m]) : T;
    __syncthreads();
    // this round resolves the tile's positions [cur, lim): below the first id of the first row not staged
    const int lim = s_lim;
    for (int p = cur + tid; p < lim; p += kThreads) {
      int x = 0, y = m;  // first staged row that begins past p
      while (x < y) {
        const int mid = (x + y) >> 1;
        if (s_beg[mid] <= p) x = mid + 1; else y = mid;
      }
      const int i = x - 1;  // >= 0: row 0 of the round begins at or before cur; the last of equal begins is not empty
      if (i >= 0 && p >= s_vlo[i] && p < s_vhi[i]) {
        const int c = s_c[i] & (kMhWhole - 1);
        u64 h = c == w ? rule.h0 : mh_start(rule.seed, (u64)c);
        for (int j = 0; j < c; ++j) h = fmix64(h ^ (u64)s_ids[p + j]);  // p + c <= the row's end - t0 <= have
        s_x[p] = (uint32_t)(h >> 32);
      }
    }
    __syncthreads();
    for (int i = 0; i < m; ++i) {
      const int vlo = s_vlo[i], vhi = s_vhi[i];
      const int lo = vlo > sub_lo ? vlo : sub_lo, hi = vhi < sub_hi ? vhi : sub_hi;
      if (lo >= hi) continue;  // (the same for every lane of the wave)
      uint32_t mn[P];
#pragma unroll
      for (int j = 0; j < P; ++j) mn[j] = 0xFFFFFFFFu;
      const auto take = [&](uint32_t x) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const uint32_t v = mh_value(a[j], b[j], x);
          mn[j] = v < mn[j] ? v : mn[j];
        }
      };
      int p = lo;
      for (; p < hi && (p & 3); ++p) take(s_x[p]);
      for (; p + 4 <= hi; p += 4) {
        uint32_t v[4];  // p is a multiple of 4 and s_x is 16-byte aligned: one 16-byte LDS read
        __builtin_memcpy(v, __builtin_assume_aligned(s_x + p, 16), 16);
        take(v[0]), take(v[1]), take(v[2]), take(v[3]);
      }
      for (; p < hi; ++p) take(s_x[p]);
      // nobody else holds a part of the row when all its shingle starts are in this wave's share of this tile
      const bool whole = (s_c[i] & kMhWhole) && vlo >= sub_lo && vhi <= sub_hi;
      uint32_t* const out = sig + (ks + (u64)i) * (u64)K;
#pragma unroll
      for (int j = 0; j < P; ++j) {
        if (perm[j] >= K) continue;
        if (whole) out[perm[j]] = mn[j]; else atomicMin(out + perm[j], mn[j]);
      }
    }
    if (lim >= T) break;
    cur = lim;
    ks += (u64)m;
    __syncthreads();
  }
}

// cells = rows x B keys; band j of row r reads sig[r K + j R .. + R), which is sig[(r B + j) R ..).
__global__ __launch_bounds__(kThreads) void k_minhash_bands(const uint32_t* __restrict__ sig, u64 cells, MhRule rule,
                                                            u64* __restrict__ keys) {
  const u64 t = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (t >= cells) return;
  const int R = rule.K / rule.B;
  const uint32_t* const s = sig + t * (u64)R;
  u64 g = draw(rule.seed, t % (u64)rule.B, kMhBand);
  for (int k = 0; k < R; ++k) g = fmix64(g ^ (u64)s[k]);
  keys[t] = g;
}

// The passes on R rows whose offsets are good: 0 or -1.  keys: nullptr without bands.
int minhash_run(const int32_t* ids, u64 n, const int64_t* row, u64 R, const MhRule& rule, uint32_t* sig, u64* keys,
                hipStream_t st) {
  if (!R) return 0;
  ENC_OK(hipMemsetAsync(sig, 0xFF, R * (u64)rule.K * 4, st));
  if (n) {
    const dim3 grid((unsigned)((n + kMhTile - 1) / kMhTile));
    (rule.K > kThreads ? k_minhash_tiles<2> : k_minhash_tiles<1>)<<<grid, dim3(kThreads), 0, st>>>(ids, n, row, R, rule,
                                                                                                    sig);
    ENC_OK(hipGetLastError());
  }
  if (keys) {
    const u64 cells = R * (u64)rule.B;
    k_minhash_bands<<<dim3((unsigned)((cells + kThreads - 1) / kThreads)), dim3(kThreads), 0, st>>>(sig, cells, rule,
                                                                                                   keys);
    ENC_OK(hipGetLastError());
  }
  return 0;
}

// The MinHash passes' state, allocated on the first MinHash call: the error word of the offset check
// and the staging of the host path.
struct MinhashState : PassState {
  DeviceWords res;   // [0] a bad row_off
  PinnedWords host;
  EventSet<4> ev;
  OneRow one;        // a call without row_off
  DeviceBuf<int32_t> hids;   // host path: a piece's ids,
  DeviceBuf<int64_t> hrow;   // its row_off,
  DeviceBuf<uint32_t> hsig;  // its signatures
  DeviceBuf<u64> hkey;       // and its band keys

  bool reserve(size_t) { return res.ensure(1) && host.ensure(1) && ev.ensure() && one.ensure(); }
};

}  // namespace

int64_t EncodeDevice::minhash(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const MinhashOpts& o,
                              uint32_t* sig, uint64_t* keys, void* stream, double* kernel_ms) {
  const u64 R = row_off ? rows : 1;
  const int64_t* row = row_off;
  return device_call<MinhashState>(
      pass_[kMinhash], device_, stream ? stream : stream_, "minhash", R, kernel_ms,
      [&](MinhashState& ms, hipStream_t st, Plan* p) {
        if (!row_off) {
          if (ms.one.put(n, st, &row) < 0) return -1;
        } else {
          ENC_OK(hipMemsetAsync(ms.res.get(), 0, 8, st));
          if (check_offsets(row_off, R, n, ms.res.get(), st) < 0) return -1;
          ENC_OK(hipMemcpyAsync(ms.host.get(), ms.res.get(), 8, hipMemcpyDeviceToHost, st));
          ENC_OK(hipStreamSynchronize(st));
          if (ms.host[0]) return -6;
        }
        *p = Plan{(int64_t)R, true, n};
        return 0;
      },
      [&](MinhashState&, hipStream_t st) { return minhash_run(ids, n, row, R, rule_of(o), sig, keys, st); });
}

// Host rows in pieces of whole rows (host_pieces).  A piece is the device passes on its own rows; the
// caller has validated row_off, so no check runs.  A row's signature does not depend on the piece.
int EncodeDevice::minhash_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const MinhashOpts& o,
                               uint32_t* sig, uint64_t* keys) {
  MinhashState& ms = pass_state<MinhashState>(pass_[kMinhash]);
  hipStream_t st = (hipStream_t)stream_;
  const int64_t one[2] = {0, (int64_t)n};
  const size_t K = (size_t)o.K, B = (size_t)o.B;
  const HostCall call{"minhash", row_off ? rows : 1, 0, 1, {{ids, n, row_off ? row_off : one}}, false, nullptr,
                      2,         {{sig, 4, K, 0}, {keys, 8, B, 0}}};
  return host_pieces(
      device_, st, call, [](size_t) { return (u64)1; },
      [&](const Piece& p, Staged* s) {
        const size_t m = p.r1 - p.r0;
        if (!tiles_fit(p.len[0]) || !ms.reserve(m) || !ms.hids.grow(std::max<size_t>(p.len[0], 1)) ||
            !ms.hrow.grow(m + 1) || !ms.hsig.grow(m * K) || (keys && !ms.hkey.grow(m * B)))
          return false;
        s->ids[0] = ms.hids.get(), s->row[0] = ms.hrow.get();
        s->out[0] = ms.hsig.get(), s->out[1] = ms.hkey.get();
        return true;
      },
      [&](const Piece& p, const Staged& s) {
        return minhash_run(s.ids[0], p.len[0], s.row[0], p.r1 - p.r0, rule_of(o), s.get<uint32_t>(0), s.get<u64>(1), st);
      });
}

}  // namespace shred
