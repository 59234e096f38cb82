// MI355X (gfx950) counting and probe kernels and the Device methods (device.h) that launch them.
// They walk the tiled token stream as bpe_device.hip's kernels do (hip_common.h).
//
//   k_pair_count   K1  weighted pair histogram + first touch     (reference bpe.cpp:187-206)
//   k_pair_dense / k_pair_hist   K1 while every id is a byte: dense tables, LDS histograms
//   k_token_freq   K6  final weighted token histogram            (reference bpe.cpp:409-415)
//   k_hbm_read / k_hbm_copy / k_occupy   bandwidth probes, co-residency diagnostic
//
// Pair counts are staged in per-workgroup LDS hash tables and spilled to HBM tables with 64-bit
// atomics (sum) and atomicMin (first touch), so the reduction is order-free and the result
// bit-identical run to run.
#ifndef SHRED_DENSE_TOK
#define SHRED_DENSE_TOK 32768
#endif

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <type_traits>

#include "../host/device.h"
#include "../host/dist.h"
#include "hip_common.h"

namespace shred {

namespace {

constexpr int kPairLds = 2048;           // per-workgroup pair-count staging slots

// ------------------------------------------------------------------------------------------
// K1: pair count
struct CountParams {
  const int32_t* tok;
  const uint64_t* tile_off;
  const uint32_t* tile_len;
  uint32_t ntiles;
  const uint64_t* weight;
  int32_t unk;
  u64* tkey;
  u64* tcnt;
  u64* tft;
  u64 tmask;
  uint32_t* overflow;
};

struct PairLds {
  u64 key[kPairLds];
  u64 cnt[kPairLds];
  u64 ft[kPairLds];
};

__device__ __forceinline__ void pair_global(const CountParams& p, u64 key, u64 c, u64 ft) {
  u64 s = mix64(key) & p.tmask;
  for (u64 probe = 0; probe <= p.tmask; ++probe) {
    const u64 prev = atomicCAS(&p.tkey[s], kEmpty64, key);
    if (prev == kEmpty64 || prev == key) {
      atomicAdd(&p.tcnt[s], c);
      atomicMin(&p.tft[s], ft);
      return;
    }
    s = (s + 1) & p.tmask;
  }
  atomicOr(p.overflow, 1u);
}

__device__ __forceinline__ void pair_emit(PairLds& h, const CountParams& p, u64 key, u64 c, u64 ft) {
  uint32_t s = (uint32_t)(mix64(key) >> 53);  // 11 bits
  for (int probe = 0; probe < 16; ++probe) {
    const u64 prev = atomicCAS(&h.key[s], kEmpty64, key);
    if (prev == kEmpty64 || prev == key) {
      atomicAdd(&h.cnt[s], c);
      atomicMin(&h.ft[s], ft);
      return;
    }
    s = (s + 1) & (kPairLds - 1);
  }
  pair_global(p, key, c, ft);
}

template <bool kWeighted>
__global__ __launch_bounds__(kThreads) void k_pair_count(CountParams p) {
  __shared__ PairLds h;
  __shared__ ScanLds s_scan;
  const int tid = threadIdx.x;
  for (int i = tid; i < kPairLds; i += kThreads) {
    h.key[i] = kEmpty64;
    h.cnt[i] = 0;
    h.ft[i] = kEmpty64;
  }
  __syncthreads();
  const int p0 = tid * kPer;
  for (uint32_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const uint32_t len = p.tile_len[tile];
    const int32_t* base = p.tok + p.tile_off[tile];
    u64 c_hdr = 0;
    for (uint32_t cs = 0; cs < len; cs += kChunk) {
      const uint32_t cl = min((uint32_t)kChunk, len - cs);
      int32_t v[kPer];
      load_chunk(base, cs, cl, p0, v);
      const int32_t nx = next_token(base, cs, len, p0, v[0]);
      u64 hl = 0;
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        if (is_hdr(v[j]) && p0 + j < (int)cl) hl = ((u64)(cs + p0 + j + 1) << 32) | hdr_rank(v[j]);
      u64 hdr_ex, hdr_tot;
      int cx, ct;
      block_scan_hdr_cnt(hl, 0, s_scan, &hdr_ex, &cx, &hdr_tot, &ct);
      u64 hdr = hdr_ex > c_hdr ? hdr_ex : c_hdr;
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const int32_t x = v[j];
        const int32_t y = j + 1 < kPer ? v[j + 1] : nx;
        if (is_hdr(x)) {
          if (p0 + j < (int)cl) hdr = ((u64)(cs + p0 + j + 1) << 32) | hdr_rank(x);
          continue;
        }
        if (is_hdr(y) || x == p.unk || y == p.unk) continue;
        const uint32_t hidx = (uint32_t)(hdr >> 32) - 1u;
        const uint32_t rank = (uint32_t)hdr;
        const u64 w = kWeighted ? p.weight[rank] : 1ull;
        const u64 key = ((u64)(uint32_t)x << 32) | (uint32_t)y;
        pair_emit(h, p, key, w, ((u64)rank << 32) | (u64)(cs + p0 + j - hidx - 1u));
      }
      c_hdr = hdr_tot > c_hdr ? hdr_tot : c_hdr;
    }
  }
  __syncthreads();
  for (int i = tid; i < kPairLds; i += kThreads)
    if (h.key[i] != kEmpty64) pair_global(p, h.key[i], h.cnt[i], h.ft[i]);
}

__global__ __launch_bounds__(kThreads) void k_pair_collect(const u64* tkey, const u64* tcnt, const u64* tft, u64 cap,
                                                            PairCount* out, uint32_t out_cap, uint32_t* n) {
  for (u64 i = (u64)blockIdx.x * kThreads + threadIdx.x; i < cap; i += (u64)gridDim.x * kThreads) {
    const u64 k = tkey[i];
    if (k == kEmpty64) continue;
    PairCount pc;
    pc.a = (int32_t)(uint32_t)(k >> 32);
    pc.b = (int32_t)(uint32_t)k;
    pc.count = tcnt[i];
    pc.ft = tft[i];
    const uint32_t i_out = atomicAdd(n + 1, 1u);
    if (i_out < out_cap) out[i_out] = pc;
    else atomicOr(n, 2u);
  }
}

// ------------------------------------------------------------------------------------------
// K1 when every id is a byte (the initial count: ids < 256, unk skipped): a dense 256 x 256
// table.  One wave per tile (16 tokens per lane, DPP header scan), 512-thread workgroups for
// memory-level parallelism, a 4096-slot LDS pair hash per workgroup (first touch updated only
// when smaller), spills and the final flush go straight to the dense HBM table (no probing).
constexpr int kDenseThreads = 512;
constexpr int kDenseWaves = kDenseThreads / 64;
constexpr int kDenseLds = 4096;
constexpr uint32_t kDensePairs = 256u * 256u;

struct DenseCountParams {
  const int32_t* tok;
  const uint64_t* tile_off;
  const uint32_t* tile_len;
  uint32_t ntiles;
  const uint64_t* weight;
  int32_t unk;
  u64* cnt;  // kDensePairs, zeroed
  u64* ft;   // kDensePairs, all ones
};

// Counts are u64 for weighted (types) tiles and u32 for unweighted (stream) ones: a workgroup
// never sees 2^32 occurrences, and 32-bit LDS atomics are the cheaper ones.
template <class C>
struct DenseLds {
  uint32_t key[kDenseLds];
  C cnt[kDenseLds];
  u64 ft[kDenseLds];
};

template <class C>
__device__ __forceinline__ void dense_emit(DenseLds<C>& h, const DenseCountParams& p, uint32_t key, C w, u64 ft) {
  uint32_t s = (key * 2654435761u) >> (32 - 12);
  for (int probe = 0; probe < 8; ++probe) {
    uint32_t k = h.key[s];
    if (k == kEmpty32) {
      k = atomicCAS(&h.key[s], kEmpty32, key);
      if (k == kEmpty32) k = key;
    }
    if (k == key) {
      atomicAdd(&h.cnt[s], w);
      if (ft < h.ft[s]) atomicMin(&h.ft[s], ft);
      return;
    }
    s = (s + 1) & (kDenseLds - 1);
  }
  atomicAdd(&p.cnt[key], (u64)w);
  atomicMin(&p.ft[key], ft);
}

template <bool kWeighted>
__global__ __launch_bounds__(kDenseThreads) void k_pair_dense(DenseCountParams p) {
  typedef typename std::conditional<kWeighted, u64, uint32_t>::type C;
  __shared__ DenseLds<C> h;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int p0 = lane * kPer;
  for (int i = threadIdx.x; i < kDenseLds; i += kDenseThreads) {
    h.key[i] = kEmpty32;
    h.cnt[i] = 0;
    h.ft[i] = kEmpty64;
  }
  __syncthreads();
  for (uint32_t t = blockIdx.x * kDenseWaves + wid; t < p.ntiles; t += gridDim.x * kDenseWaves) {
    const uint32_t len = p.tile_len[t];
    const int32_t* base = p.tok + p.tile_off[t];
    u64 c_hdr = 0;  // ((index + 1) << 32) | rank of the last header so far
    for (uint32_t cs = 0; cs < len; cs += kWaveTok) {
      const uint32_t cl = min((uint32_t)kWaveTok, len - cs);
      int32_t v[kPer];
      load_chunk(base, cs, cl, p0, v);
      const int32_t nx = next_token(base, cs, len, p0, v[0]);
      uint32_t hmask = 0;
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        if (is_hdr(v[j]) && p0 + j < (int)cl) hmask |= 1u << j;
      u64 hl = 0;
      if (hmask) {
        const int j = 31 - __clz(hmask);
        hl = ((u64)(cs + p0 + j + 1) << 32) | hdr_rank(v[j]);
      }
      const u64 hinc = wave_scan_max64(hl);
      u64 hdr = wave_prev64(hinc);
      hdr = hdr > c_hdr ? hdr : c_hdr;
      uint32_t w_rank = ~0u;
      C w = 1;
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const int32_t x = v[j];
        const int32_t y = j + 1 < kPer ? v[j + 1] : nx;
        if (is_hdr(x)) {
          hdr = ((u64)(cs + p0 + j + 1) << 32) | hdr_rank(x);
          continue;
        }
        if (is_hdr(y) || x == p.unk || y == p.unk) continue;
        const uint32_t hidx = (uint32_t)(hdr >> 32) - 1u;
        const uint32_t rank = (uint32_t)hdr;
        if (kWeighted && rank != w_rank) {
          w = (C)p.weight[rank];
          w_rank = rank;
        }
        const uint32_t key = ((uint32_t)x << 8) | (uint32_t)y;
        dense_emit(h, p, key, w, ((u64)rank << 32) | (u64)(cs + p0 + j - hidx - 1u));
      }
      const u64 htot = lane_read64(hinc, 63);
      c_hdr = htot > c_hdr ? htot : c_hdr;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kDenseLds; i += kDenseThreads) {
    const uint32_t k = h.key[i];
    if (k == kEmpty32) continue;
    atomicAdd(&p.cnt[k], (u64)h.cnt[i]);
    atomicMin(&p.ft[k], h.ft[i]);
  }
}

// Dense table -> PairCount list (pairs with a count).
__global__ __launch_bounds__(kThreads) void k_pair_dense_collect(const u64* cnt, const u64* ft, PairCount* out,
                                                                  uint32_t* n) {
  for (uint32_t k = blockIdx.x * kThreads + threadIdx.x; k < kDensePairs; k += gridDim.x * kThreads) {
    if (ft[k] == kEmpty64) continue;
    PairCount pc;
    pc.a = (int32_t)(k >> 8);
    pc.b = (int32_t)(k & 255u);
    pc.count = cnt[k];
    pc.ft = ft[k];
    out[atomicAdd(n, 1u)] = pc;
  }
}

// K5 check (debug): the largest count of a collected pair list, and (a, b)'s count.
__global__ __launch_bounds__(kThreads) void k_pair_max(const PairCount* pc, uint32_t n, int32_t a, int32_t b, u64* r) {
  u64 mx = 0;
  for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
    const PairCount p = pc[i];
    mx = p.count > mx ? p.count : mx;
    if (p.a == a && p.b == b) r[1] = p.count;  // one entry per pair: a single writer
  }
  for (int o = 32; o > 0; o >>= 1) {
    const u64 v = (u64)__shfl_xor((unsigned long long)mx, o);
    mx = v > mx ? v : mx;
  }
  if ((threadIdx.x & 63) == 0 && mx) atomicMax(reinterpret_cast<unsigned long long*>(r), (unsigned long long)mx);
}

// ------------------------------------------------------------------------------------------
// K1 bulk (stream layout, every id a byte): pair counts only, over the tiles past the ft tiles
// (the first occurrence of every type is packed into tiles [0, ft_tiles), where k_pair_dense
// takes first touch; every other occurrence repeats a type, so only its counts matter).
//
// One 1024-thread workgroup per CU keeps the whole 256 x 256 table in LDS as packed 16-bit
// counters (two pairs per dword, 128 KiB): a pair occurrence is one ds_add_rtn_u32 at a fixed
// address, no hashing, no probing, nothing in HBM until the end.  A counter never wraps: the one
// atomic that takes a half from 0x7FFF to 0x8000 (exactly one per crossing, increments are 1)
// moves 0x8000 to the HBM table and takes it back off the half; meanwhile at most 16 K other
// increments can land, so a half stays below 0xC000 and never carries into its neighbour.
// Each lane streams 2 tiles x 16 tokens per iteration (8 x 16 B loads in flight), and the final
// flush adds the non-zero halves to the HBM table (one u64 atomic per pair per workgroup).
#ifndef SHRED_HIST_CO
#define SHRED_HIST_CO 1
#endif
#ifndef SHRED_HIST_MODE
#define SHRED_HIST_MODE 0  // diagnostic 1: no LDS atomics (read ceiling of the access pattern)
#endif
constexpr int kHistThreads = 1024;
constexpr int kHistWaves = kHistThreads / 64;
constexpr int kHistWords = kDensePairs / 2;

// One pair occurrence (x, y) per element: add 1 to its 16-bit half; `old` gets the dword before
// the add.  Branch-free so that a lane's 16 atomics issue back to back behind one wait: an
// inactive element adds 0 to a per-lane dummy word past the table (distinct banks).
__device__ __forceinline__ void hist_add(uint32_t* h, int32_t x, int32_t y, int32_t unk, int lane, uint32_t& key,
                                         uint32_t& old, bool& on, uint32_t& sink) {
  // bitwise, not &&: short-circuit evaluation compiles to a branch per element
  on = (bool)((unsigned)(x >= kHeaderLimit) & (unsigned)(y >= kHeaderLimit) & (unsigned)(x != unk) &
              (unsigned)(y != unk));
  key = ((uint32_t)x << 8) | ((uint32_t)y & 255u);
#if SHRED_HIST_MODE == 1
  old = 0;
  if (on) sink += key;
#else
  const uint32_t a = on ? key >> 1 : (uint32_t)(kHistWords + lane);
  const uint32_t inc = on ? ((key & 1u) ? 0x10000u : 1u) : 0u;
  old = __hip_atomic_fetch_add(&h[a], inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
}
__device__ __forceinline__ void hist_fix(uint32_t* h, uint32_t key, uint32_t old, bool on, u64* cnt) {
  const uint32_t half = (key & 1u) ? (old >> 16) : (old & 0xFFFFu);
  if (on && half == 0x7FFFu) {
    atomicSub(&h[key >> 1], (key & 1u) ? 0x80000000u : 0x8000u);
    atomicAdd(&cnt[key], (u64)0x8000);
  }
}

// 16 tokens per lane, lane-contiguous (load_chunk order): pairs (v[j], v[j+1]), then (v[15], nx).
__device__ __forceinline__ void hist_tile(uint32_t* h, const int32_t (&v)[kPer], int32_t nx, int32_t unk, u64* cnt,
                                          uint32_t& sink) {
  uint32_t old[kPer], key[kPer];
  bool on[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    hist_add(h, v[j], j + 1 < kPer ? v[j + 1] : nx, unk, threadIdx.x & 63, key[j], old[j], on[j], sink);
#pragma unroll
  for (int j = 0; j < kPer; ++j) hist_fix(h, key[j], old[j], on[j], cnt);
}

// Coalesced order for a tile of <= 1024 tokens: quad k of lane l holds tokens 256 k + 4 l .. +3,
// so each 16-B load instruction reads 1 KiB contiguous.  The token after a quad is lane l+1's
// first of the same quad (DPP), or for lane 63 lane 0's first of quad k+1.
__device__ __forceinline__ void load_tile_co(const int32_t* base, uint32_t len, int lane, int32_t (&v)[kPer]) {
  const int4* q = reinterpret_cast<const int4*>(base) + lane;
  int4 x[kPer / 4];
#pragma unroll
  for (int k = 0; k < kPer / 4; ++k) x[k] = q[64 * k];
#pragma unroll
  for (int k = 0; k < kPer / 4; ++k) {
    const int p = 256 * k + 4 * lane;
    v[4 * k] = p < (int)len ? x[k].x : kPad;
    v[4 * k + 1] = p + 1 < (int)len ? x[k].y : kPad;
    v[4 * k + 2] = p + 2 < (int)len ? x[k].z : kPad;
    v[4 * k + 3] = p + 3 < (int)len ? x[k].w : kPad;
  }
}
__device__ __forceinline__ void hist_tile_co(uint32_t* h, const int32_t (&v)[kPer], int lane, int32_t unk, u64* cnt,
                                             uint32_t& sink) {
  uint32_t old[kPer], key[kPer];
  bool on[kPer];
#pragma unroll
  for (int k = 0; k < kPer / 4; ++k) {
    int32_t nx = wave_next(v[4 * k]);
    if (lane == 63) nx = k + 1 < kPer / 4 ? (int32_t)lane_read((uint32_t)v[4 * k + 4], 0) : kPad;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = 4 * k + e;
      hist_add(h, v[j], e < 3 ? v[j + 1] : nx, unk, lane, key[j], old[j], on[j], sink);
    }
  }
#pragma unroll
  for (int j = 0; j < kPer; ++j) hist_fix(h, key[j], old[j], on[j], cnt);
}

__global__ __launch_bounds__(kHistThreads) void k_pair_hist(const int32_t* tok, const uint64_t* tile_off,
                                                             const uint32_t* tile_len, uint32_t t0, uint32_t t1,
                                                             int32_t unk, u64* cnt) {
  __shared__ uint32_t h[kHistWords + 64];  // + per-lane dummy words
  for (int i = threadIdx.x; i < kHistWords + 64; i += kHistThreads) h[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int p0 = lane * kPer;
  const uint32_t stride = gridDim.x * kHistWaves;
  uint32_t sink = 0;
  for (uint32_t t = t0 + blockIdx.x * kHistWaves + wid; t < t1; t += 2 * stride) {
    const uint32_t u = t + stride;
    const bool two = u < t1;
    const uint32_t lt = tile_len[t], lu = two ? tile_len[u] : 0u;
    const int32_t* bt = tok + tile_off[t];
    const int32_t* bu = tok + (two ? tile_off[u] : tile_off[t]);
    if (lt <= (uint32_t)kWaveTok && lu <= (uint32_t)kWaveTok) {
      // both tiles are one wave chunk: all 8 loads in flight together
      int32_t va[kPer], vb[kPer];
#if SHRED_HIST_CO
      load_tile_co(bt, lt, lane, va);
      load_tile_co(bu, lu, lane, vb);
      hist_tile_co(h, va, lane, unk, cnt, sink);
      hist_tile_co(h, vb, lane, unk, cnt, sink);
#else
      load_chunk(bt, 0, lt, p0, va);
      load_chunk(bu, 0, lu, p0, vb);
      const int32_t na = next_token(bt, 0, lt, p0, va[0]);
      const int32_t nb = next_token(bu, 0, lu, p0, vb[0]);
      hist_tile(h, va, na, unk, cnt, sink);
      hist_tile(h, vb, nb, unk, cnt, sink);
#endif
      continue;
    }
    for (int k = 0; k < 2; ++k) {  // a tile holding one long word: chunk by chunk
      const uint32_t len = k ? lu : lt;
      const int32_t* base = k ? bu : bt;
      for (uint32_t cs = 0; cs < len; cs += kWaveTok) {
        int32_t v[kPer];
        load_chunk(base, cs, min((uint32_t)kWaveTok, len - cs), p0, v);
        hist_tile(h, v, next_token(base, cs, len, p0, v[0]), unk, cnt, sink);
      }
    }
  }
#if SHRED_HIST_MODE == 1
  if (sink == 0x12345678u) h[0] = sink;  // keeps the loads alive in the diagnostic build
#endif
  __syncthreads();
  for (int i = threadIdx.x; i < kHistWords; i += kHistThreads) {
    const uint32_t w = h[i];
    if (w & 0xFFFFu) atomicAdd(&cnt[2 * i], (u64)(w & 0xFFFFu));
    if (w >> 16) atomicAdd(&cnt[2 * i + 1], (u64)(w >> 16));
  }
}

// ------------------------------------------------------------------------------------------
// K6: final token histogram over ids [0, T) (the unk count lands on unk_id when it is in range)
template <bool kWeighted>
__global__ __launch_bounds__(kThreads) void k_token_freq(const int32_t* tok, const uint64_t* tile_off,
                                                          const uint32_t* tile_len, uint32_t ntiles,
                                                          const uint64_t* weight, uint32_t T, u64* freq) {
  __shared__ ScanLds s_scan;
  const int p0 = threadIdx.x * kPer;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t len = tile_len[tile];
    const int32_t* base = tok + tile_off[tile];
    u64 c_hdr = 0;
    for (uint32_t cs = 0; cs < len; cs += kChunk) {
      const uint32_t cl = min((uint32_t)kChunk, len - cs);
      int32_t v[kPer];
      load_chunk(base, cs, cl, p0, v);
      u64 hl = 0;
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        if (is_hdr(v[j]) && p0 + j < (int)cl) hl = ((u64)(cs + p0 + j + 1) << 32) | hdr_rank(v[j]);
      u64 hdr_ex, hdr_tot;
      int cx, ct;
      block_scan_hdr_cnt(hl, 0, s_scan, &hdr_ex, &cx, &hdr_tot, &ct);
      u64 hdr = hdr_ex > c_hdr ? hdr_ex : c_hdr;
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        if (is_hdr(v[j])) {
          if (p0 + j < (int)cl) hdr = ((u64)(cs + p0 + j + 1) << 32) | hdr_rank(v[j]);
          continue;
        }
        if ((uint32_t)v[j] >= T) continue;
        atomicAdd(&freq[v[j]], kWeighted ? weight[(uint32_t)hdr] : 1ull);
      }
      c_hdr = hdr_tot > c_hdr ? hdr_tot : c_hdr;
    }
  }
}

__global__ void k_sum_len(const uint32_t* tile_len, uint32_t n, u64* out) {
  u64 s = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) s += tile_len[i];
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(out, s);
}

// Achievable-bandwidth probes (the measured ceiling beside the nominal 8 TB/s):
// a pure streaming read (4 x 16 B per lane in flight, xor-reduced so nothing is elided) and a
// streaming copy, both grid-stride over 16-B vectors with a few workgroups per CU.
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_hbm_read(const v4u* __restrict__ src, size_t n16, uint32_t* out) {
  v4u acc = {0, 0, 0, 0};
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n16; i += 4 * stride) {
    const v4u a = __builtin_nontemporal_load(src + i), b = __builtin_nontemporal_load(src + i + stride);
    const v4u c = __builtin_nontemporal_load(src + i + 2 * stride), d = __builtin_nontemporal_load(src + i + 3 * stride);
    acc ^= a ^ b ^ c ^ d;
  }
  for (; i < n16; i += stride) acc ^= src[i];
  const uint32_t x = acc.x ^ acc.y ^ acc.z ^ acc.w;
  if (x == 0x9e3779b9u) out[blockIdx.x] = x;  // practically never taken; keeps the loads live
}

__global__ __launch_bounds__(256) void k_hbm_copy(const v4u* __restrict__ src, v4u* __restrict__ dst, size_t n16) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + stride < n16; i += 2 * stride) {
    const v4u a = __builtin_nontemporal_load(src + i), b = __builtin_nontemporal_load(src + i + stride);
    __builtin_nontemporal_store(a, dst + i);
    __builtin_nontemporal_store(b, dst + i + stride);
  }
  for (; i < n16; i += stride) dst[i] = src[i];
}

}  // namespace

// ==========================================================================================
// Diagnostic (tests of k_resident's co-residency check): workgroups of 1024 threads that fill
// every wave slot of all CUs but `free_cus`, spinning on their own stream until the host raises a
// flag or `max_seconds` pass (every wave reaches one of the two exits).  Each workgroup marks
// itself started.
__global__ __launch_bounds__(1024) void k_occupy(const uint32_t* release, uint32_t* started, uint64_t max_ticks) {
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0) __hip_atomic_store(started + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  for (;;) {
    if (__hip_atomic_load(release, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) break;
    if (__builtin_amdgcn_s_memrealtime() - t0 > max_ticks) break;
    __builtin_amdgcn_s_sleep(64);
  }
}

struct Occupier {
  int ordinal;
  hipStream_t stream;
  uint32_t* host;  // pinned: [0] release flag, [1..] started marks
  void* dev;
  uint32_t groups;
};

void* Device::occupy(int ordinal, int free_cus, double max_seconds) {
  if (max_seconds <= 0 || hipSetDevice(ordinal) != hipSuccess) return nullptr;
  hipDeviceProp_t pr;
  HIP_OK(hipGetDeviceProperties(&pr, ordinal));
  const int per_cu = std::max(1, pr.maxThreadsPerMultiProcessor / 1024);
  const int groups = per_cu * (pr.multiProcessorCount - free_cus);
  const size_t lds = 0;
  if (groups < 1) return nullptr;
  Occupier* o = new Occupier{ordinal, nullptr, nullptr, nullptr, (uint32_t)groups};
  HIP_OK(hipStreamCreateWithFlags(&o->stream, hipStreamNonBlocking));
  const unsigned pin = hipHostMallocMapped | hipHostMallocCoherent;
  HIP_OK(hipHostMalloc((void**)&o->host, (size_t)(groups + 1) * sizeof(uint32_t), pin));
  std::memset(o->host, 0, (size_t)(groups + 1) * sizeof(uint32_t));
  HIP_OK(hipHostGetDevicePointer(&o->dev, o->host, 0));
  uint32_t* d = static_cast<uint32_t*>(o->dev);
  k_occupy<<<groups, 1024, lds, o->stream>>>(d, d + 1, (uint64_t)(max_seconds * 1e8));
  HIP_OK(hipGetLastError());
  const double t0 = now_seconds();  // until every workgroup runs (or 10 s)
  for (;;) {
    uint32_t n = 0;
    for (int g = 0; g < groups; ++g) n += __atomic_load_n(&o->host[1 + g], __ATOMIC_ACQUIRE);
    if (n == (uint32_t)groups || now_seconds() - t0 > 10.0) {
      if (std::getenv("SHREDWORD_RESIDENT_REPORT"))
 std::fprintf(stderr, "[OCCUPY] %u of %d workgroups (1024 threads, %d per CU) running after %.1f ms\n", n, groups, per_cu,
                     1e3 * (now_seconds() - t0));
      break;
    }
    std::this_thread::sleep_for(std::chrono::microseconds(100));
  }
  return o;
}

void Device::release(void* handle) {
  Occupier* o = static_cast<Occupier*>(handle);
  if (!o) return;
  (void)hipSetDevice(o->ordinal);
  __atomic_store_n(&o->host[0], 1u, __ATOMIC_RELEASE);
  (void)hipStreamSynchronize(o->stream);
  (void)hipStreamDestroy(o->stream);
  (void)hipHostFree(o->host);
  delete o;
}

int Device::hbm_probe(int ordinal, size_t bytes, int reps, double* read_gbps, double* copy_gbps) {
  std::string why;
  if (!available(&why) || bytes < (1u << 20) || reps < 1) return -1;
  HIP_OK(hipSetDevice(ordinal));
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, ordinal));
  const int cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  const size_t n16 = bytes / 16;
  v4u *a = nullptr, *b = nullptr;
  uint32_t* sink = nullptr;
  if (hipMalloc(&a, n16 * 16) != hipSuccess) return -1;
  if (hipMalloc(&b, n16 * 16) != hipSuccess) {
    HIP_OK(hipFree(a));
    return -1;
  }
  const int grid = cus * 8;
  HIP_OK(hipMalloc(&sink, grid * sizeof(uint32_t)));
  hipStream_t s;
  HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  HIP_OK(hipMemsetAsync(a, 0x5a, n16 * 16, s));
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  float ms = 0;
  for (int w = 0; w < 2; ++w) k_hbm_read<<<grid, 256, 0, s>>>(a, n16, sink);
  HIP_OK(hipEventRecord(e0, s));
  for (int r = 0; r < reps; ++r) k_hbm_read<<<grid, 256, 0, s>>>(a, n16, sink);
  HIP_OK(hipEventRecord(e1, s));
  HIP_OK(hipEventSynchronize(e1));
  HIP_OK(hipEventElapsedTime(&ms, e0, e1));
  if (read_gbps) *read_gbps = (double)n16 * 16 * reps / (ms * 1e-3) / 1e9;
  for (int w = 0; w < 2; ++w) k_hbm_copy<<<grid, 256, 0, s>>>(a, b, n16);
  HIP_OK(hipEventRecord(e0, s));
  for (int r = 0; r < reps; ++r) k_hbm_copy<<<grid, 256, 0, s>>>(a, b, n16);
  HIP_OK(hipEventRecord(e1, s));
  HIP_OK(hipEventSynchronize(e1));
  HIP_OK(hipEventElapsedTime(&ms, e0, e1));
  if (copy_gbps) *copy_gbps = 2.0 * (double)n16 * 16 * reps / (ms * 1e-3) / 1e9;
  HIP_OK(hipEventDestroy(e0));
  HIP_OK(hipEventDestroy(e1));
  HIP_OK(hipStreamDestroy(s));
  HIP_OK(hipFree(a));
  HIP_OK(hipFree(b));
  HIP_OK(hipFree(sink));
  return 0;
}

bool Device::available(std::string* why) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) {
    if (why) *why = e != hipSuccess ? std::string("hipGetDeviceCount: ") + hipGetErrorString(e) : "no HIP device";
    return false;
  }
  return true;
}

uint64_t Device::live_tokens() {
  HIP_OK(hipSetDevice(ordinal_));
  park();
  if (!ntiles_) return 0;
  u64* d = dalloc<u64>(1, &bytes_alloc_);
  HIP_OK(hipMemsetAsync(d, 0, sizeof(u64), S(stream_)));
  k_sum_len<<<64, 256, 0, S(stream_)>>>(tile_len_, (uint32_t)ntiles_, d);
  u64 h = 0;
  HIP_OK(hipMemcpyAsync(&h, d, sizeof(u64), hipMemcpyDeviceToHost, S(stream_)));
  HIP_OK(hipStreamSynchronize(S(stream_)));
  HIP_OK(hipFree(d));
  bytes_alloc_ -= sizeof(u64);
  return h;
}

void Device::count_pairs(int32_t unk_id, std::vector<PairCount>* out) {
  HIP_OK(hipSetDevice(ordinal_));
  park();
  out->clear();
  if (!ntiles_) {
    if (xchg_.world > 1) dist_merge_pairs(out);
    return;
  }
  const uint64_t live = live_tokens();
  if (max_id_seen_ < kBaseVocab) {  // every id in the stream is a byte or unk (skipped)
    count_pairs_dense(unk_id, live, out);
    if (xchg_.world > 1) dist_merge_pairs(out);
    return;
  }
  // distinct pairs <= live tokens and <= (ids in play)^2
  const uint64_t ids = (uint64_t)std::max<int32_t>(max_id_seen_, kBaseVocab) + 2;
  uint64_t bound = std::min<uint64_t>(live, ids * ids);
  uint64_t cap = 1024;
  while (cap < 2 * bound && cap < (1ull << 27)) cap *= 2;
  size_t acc = 0;
  u64* tkey = dalloc<u64>(cap, &acc);
  u64* tcnt = dalloc<u64>(cap, &acc);
  u64* tft = dalloc<u64>(cap, &acc);
  uint32_t* flags = dalloc<uint32_t>(2, &acc);
  HIP_OK(hipMemsetAsync(tkey, 0xFF, cap * sizeof(u64), S(stream_)));
  HIP_OK(hipMemsetAsync(tcnt, 0, cap * sizeof(u64), S(stream_)));
  HIP_OK(hipMemsetAsync(tft, 0xFF, cap * sizeof(u64), S(stream_)));
  HIP_OK(hipMemsetAsync(flags, 0, 2 * sizeof(uint32_t), S(stream_)));
  CountParams cp{tok_, tile_off_, tile_len_, (uint32_t)ntiles_, weight_, unk_id, tkey, tcnt, tft, cap - 1, flags};
  const int grid = (int)std::min<size_t>(ntiles_, (size_t)cu_count_ * 2);
  if (timing_) HIP_OK(hipEventRecord((hipEvent_t)ev_[2], S(stream_)));
  if (layout_ == Layout::kStream) k_pair_count<false><<<grid, kThreads, 0, S(stream_)>>>(cp);
  else k_pair_count<true><<<grid, kThreads, 0, S(stream_)>>>(cp);
  HIP_OK(hipGetLastError());
  if (timing_) HIP_OK(hipEventRecord((hipEvent_t)ev_[3], S(stream_)));
  const uint32_t out_cap = (uint32_t)std::min<uint64_t>(cap, bound + 1);
  PairCount* dout = dalloc<PairCount>(out_cap, &acc);
  k_pair_collect<<<512, kThreads, 0, S(stream_)>>>(tkey, tcnt, tft, cap, dout, out_cap, flags);
  HIP_OK(hipGetLastError());
  uint32_t hflags[2];
  HIP_OK(hipMemcpyAsync(hflags, flags, sizeof(hflags), hipMemcpyDeviceToHost, S(stream_)));
  HIP_OK(hipStreamSynchronize(S(stream_)));
  if (hflags[0]) fatal("pair table overflow in k_pair_count / k_pair_collect");
  if (pmq_) {
    reduce_pair_max(dout, hflags[1]);
  } else {
    out->resize(hflags[1]);
    if (hflags[1])
      HIP_OK(hipMemcpy(out->data(), dout, hflags[1] * sizeof(PairCount), hipMemcpyDeviceToHost));
  }
  if (timing_) {
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, (hipEvent_t)ev_[2], (hipEvent_t)ev_[3]));
    times_.count_ms += ms;
    times_.count_launches += 1;
    // 4 B per token and per word header (the boundary), 8 B weight per word in the types
    // layout, 12 B of tile descriptor per tile
    times_.count_bytes += 4.0 * (double)live + 12.0 * (double)ntiles_ +
                          (layout_ == Layout::kTypes ? 8.0 * (double)nentries_ : 0.0);
  }
  for (void* p : {(void*)tkey, (void*)tcnt, (void*)tft, (void*)flags, (void*)dout}) HIP_OK(hipFree(p));
  if (xchg_.world > 1) dist_merge_pairs(out);
}

// K1 with every id a byte: dense tables, no hashing in HBM.
void Device::count_pairs_dense(int32_t unk_id, uint64_t live, std::vector<PairCount>* out) {
  size_t acc = 0;
  u64* cnt = dalloc<u64>(kDensePairs, &acc);
  u64* ft = dalloc<u64>(kDensePairs, &acc);
  uint32_t* n = dalloc<uint32_t>(1, &acc);
  PairCount* dout = dalloc<PairCount>(kDensePairs, &acc);
  HIP_OK(hipMemsetAsync(cnt, 0, kDensePairs * sizeof(u64), S(stream_)));
  HIP_OK(hipMemsetAsync(ft, 0xFF, kDensePairs * sizeof(u64), S(stream_)));
  HIP_OK(hipMemsetAsync(n, 0, sizeof(uint32_t), S(stream_)));
  // stream layout: first touch (and counts) from the ft tiles, counts alone from the rest
  const size_t ft_tiles = layout_ == Layout::kStream ? ft_tiles_ : ntiles_;
  DenseCountParams dp{tok_, tile_off_, tile_len_, (uint32_t)ft_tiles, weight_, unk_id, cnt, ft};
  int per_cu = 0;
  HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(&k_pair_dense<true>),
                                                      kDenseThreads, 0));
  // >= SHRED_DENSE_TOK tokens per workgroup: each one flushes its LDS table with HBM atomics
  const uint64_t ft_live = ft_tiles == ntiles_ ? live : ft_live_tokens_;
  const size_t by_tokens = (size_t)(ft_live / SHRED_DENSE_TOK) + 1;
  const int grid = (int)std::min<size_t>(std::min<size_t>((ft_tiles + kDenseWaves - 1) / kDenseWaves, by_tokens),
                                         (size_t)cu_count_ * (size_t)std::max(1, per_cu));
  if (timing_) HIP_OK(hipEventRecord((hipEvent_t)ev_[2], S(stream_)));
  if (ft_tiles > 0) {
    if (layout_ == Layout::kStream) k_pair_dense<false><<<grid, kDenseThreads, 0, S(stream_)>>>(dp);
    else k_pair_dense<true><<<grid, kDenseThreads, 0, S(stream_)>>>(dp);
    HIP_OK(hipGetLastError());
  }
  const bool bulk = ft_tiles < ntiles_;
  if (bulk) {
    if (timing_) HIP_OK(hipEventRecord((hipEvent_t)ev_[4], S(stream_)));
    const size_t hist_grid = std::min<size_t>((ntiles_ - ft_tiles + kHistWaves - 1) / kHistWaves, (size_t)cu_count_);
    k_pair_hist<<<(int)hist_grid, kHistThreads, 0, S(stream_)>>>(tok_, tile_off_, tile_len_, (uint32_t)ft_tiles,
                                                                (uint32_t)ntiles_, unk_id, cnt);
    HIP_OK(hipGetLastError());
  }
  if (timing_) HIP_OK(hipEventRecord((hipEvent_t)ev_[3], S(stream_)));
  k_pair_dense_collect<<<64, kThreads, 0, S(stream_)>>>(cnt, ft, dout, n);
  HIP_OK(hipGetLastError());
  uint32_t hn = 0;
  HIP_OK(hipMemcpyAsync(&hn, n, sizeof(uint32_t), hipMemcpyDeviceToHost, S(stream_)));
  HIP_OK(hipStreamSynchronize(S(stream_)));
  if (pmq_) {
    reduce_pair_max(dout, hn);
  } else {
    out->resize(hn);
    if (hn) HIP_OK(hipMemcpy(out->data(), dout, hn * sizeof(PairCount), hipMemcpyDeviceToHost));
  }
  if (timing_) {
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, (hipEvent_t)ev_[2], (hipEvent_t)ev_[3]));
    times_.count_ms += ms;
    times_.count_launches += 1;
    // 4 B per token and per word header (the boundary), 8 B weight per word in the types
    // layout, 12 B of tile descriptor per tile
    times_.count_bytes += 4.0 * (double)live + 12.0 * (double)ntiles_ +
                          (layout_ == Layout::kTypes ? 8.0 * (double)nentries_ : 0.0);
    if (bulk) {  // k_pair_hist alone: 4 B per token (headers = word boundaries) + 12 B per tile
      HIP_OK(hipEventElapsedTime(&ms, (hipEvent_t)ev_[4], (hipEvent_t)ev_[3]));
      times_.hist_ms += ms;
      times_.hist_launches += 1;
      times_.hist_bytes += 4.0 * (double)(live - ft_live) + 12.0 * (double)(ntiles_ - ft_tiles);
    }
  }
  for (void* q : {(void*)cnt, (void*)ft, (void*)n, (void*)dout}) HIP_OK(hipFree(q));
}

void Device::reduce_pair_max(const PairCount* dout, uint32_t n) {
  size_t acc = 0;
  u64* r = dalloc<u64>(2, &acc);
  HIP_OK(hipMemsetAsync(r, 0, 2 * sizeof(u64), S(stream_)));
  if (n) k_pair_max<<<(int)std::min<uint32_t>((n + kThreads - 1) / kThreads, 1024), kThreads, 0, S(stream_)>>>(
      dout, n, pmq_->a, pmq_->b, r);
  HIP_OK(hipGetLastError());
  u64 h[2];
  HIP_OK(hipMemcpyAsync(h, r, sizeof(h), hipMemcpyDeviceToHost, S(stream_)));
  HIP_OK(hipStreamSynchronize(S(stream_)));
  HIP_OK(hipFree(r));
  pmq_->max_freq = h[0];
  pmq_->ab_freq = h[1];
}

// K5 check: one rank reduces its fresh K1 histogram on the device; under RCCL the ranks' lists
// are merged first (a pair's count is a sum over ranks), then reduced on the host.
void Device::pair_max(int32_t unk_id, int32_t a, int32_t b, uint64_t* max_freq, uint64_t* ab_freq) {
  if (xchg_.world > 1) {
    Backend::pair_max(unk_id, a, b, max_freq, ab_freq);
    return;
  }
  PairMaxQuery q{a, b, 0, 0};
  pmq_ = &q;
  std::vector<PairCount> none;
  count_pairs(unk_id, &none);
  pmq_ = nullptr;
  *max_freq = q.max_freq;
  *ab_freq = q.ab_freq;
}

void Device::token_freq(size_t T, std::vector<uint64_t>* freq) {
  HIP_OK(hipSetDevice(ordinal_));
  park();
  freq->assign(T, 0);
  if (!ntiles_ || !T) {
    if (xchg_.world > 1) dist_allreduce_host(freq->data(), T, false);
    return;
  }
  size_t acc = 0;
  u64* d = dalloc<u64>(T, &acc);
  HIP_OK(hipMemsetAsync(d, 0, T * sizeof(u64), S(stream_)));
  const int grid = (int)std::min<size_t>(ntiles_, (size_t)cu_count_ * 4);
  if (layout_ == Layout::kStream)
    k_token_freq<false><<<grid, kThreads, 0, S(stream_)>>>(tok_, tile_off_, tile_len_, (uint32_t)ntiles_, weight_, (uint32_t)T, d);
  else
    k_token_freq<true><<<grid, kThreads, 0, S(stream_)>>>(tok_, tile_off_, tile_len_, (uint32_t)ntiles_, weight_, (uint32_t)T, d);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(freq->data(), d, T * sizeof(u64), hipMemcpyDeviceToHost, S(stream_)));
  HIP_OK(hipStreamSynchronize(S(stream_)));
  HIP_OK(hipFree(d));
  if (xchg_.world > 1) dist_allreduce_host(freq->data(), T, false);
}

}  // namespace shred
