// Helpers every HIP unit of the trainer shares: error check, host-visible stores, DPP wave
// primitives, and the pieces of the tiled token stream (device.h) that more than one unit walks.
// Included by .hip files only (csrc/host/*.h stay free of HIP types); everything here is inline
// or in the anonymous namespace, so no unit exports any of it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../host/common.h"

#ifndef SHRED_MAX_GROUPS
#define SHRED_MAX_GROUPS 256
#endif
#ifndef SHRED_DELTA_LDS
#define SHRED_DELTA_LDS 2048
#endif
#ifndef SHRED_SIG_BITS
#define SHRED_SIG_BITS 8192
#endif

namespace shred {

#define HIP_OK(expr)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) {                                                                 \
      std::fprintf(stderr, "[ERROR]\t HIP %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), \
                   __FILE__, __LINE__);                                                     \
      std::fflush(stderr);                                                                  \
      std::abort();                                                                         \
    }                                                                                       \
  } while (0)

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 16;
constexpr int kChunk = kThreads * kPer;  // 4096 tokens = 16 KiB per chunk
constexpr uint32_t kEmpty32 = 0xFFFFFFFFu;
constexpr unsigned long long kEmpty64 = ~0ull;
constexpr int32_t kPad = INT32_MIN;      // beyond the tile; also looks like a header
constexpr size_t kStreamPad = kChunk + 64;  // elements allocated past the stream (whole-chunk reads)

typedef unsigned long long u64;

__device__ __forceinline__ bool is_hdr(int32_t t) { return t < kHeaderLimit; }
__device__ __forceinline__ uint32_t hdr_rank(int32_t t) { return (uint32_t)(t - kHeaderBase); }

__device__ __forceinline__ u64 mix64(u64 k) {
  k ^= k >> 33;
  k *= 0xFF51AFD7ED558CCDull;
  k ^= k >> 33;
  k *= 0xC4CEB9FE1A85EC53ull;
  k ^= k >> 33;
  return k;
}

// Host-visible writes.  Plain stores, published by one system-scope release (L2 write-back)
// before the flag: measured on MI355X, write-through system stores (sc0 sc1, SHRED_SYS_STORES)
// are one small PCIe write each and made a merge 2-8x slower, while a flag behind plain stores
// without the release let the host read stale records.
#ifdef SHRED_SYS_STORES
__device__ __forceinline__ void sys_store(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void sys_store(unsigned long long* p, unsigned long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
#else
__device__ __forceinline__ void sys_store(uint32_t* p, uint32_t v) { *p = v; }
__device__ __forceinline__ void sys_store(unsigned long long* p, unsigned long long v) { *p = v; }
#endif
// Raises a host-visible flag after this lane's (and, behind a barrier, its workgroup's) writes.
__device__ __forceinline__ void sys_flag(uint32_t* flag, uint32_t v) {
#ifdef SHRED_SYS_STORES
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#else
  __threadfence_system();
  __hip_atomic_store(flag, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
#endif
}
__device__ __forceinline__ void sys_record(void* rec, uint32_t key, unsigned long long sum, unsigned long long ft) {
  unsigned long long* r = static_cast<unsigned long long*>(rec);
  sys_store(r, (unsigned long long)key);
  sys_store(r + 1, sum);
  sys_store(r + 2, ft);
}

// One exclusive block scan of a packed header key (max) and a counter (sum) over 256 lanes.
struct ScanLds {
  u64 hdr[4];
  int cnt[4];
};

__device__ __forceinline__ void block_scan_hdr_cnt(u64 hdr, int cnt, ScanLds& s, u64* hdr_excl, int* cnt_excl,
                                                   u64* hdr_tot, int* cnt_tot) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  u64 h = hdr;
  int c = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    u64 hy = __shfl_up(h, d, 64);
    int cy = __shfl_up(c, d, 64);
    if (lane >= d) {
      h = hy > h ? hy : h;
      c += cy;
    }
  }
  if (lane == 63) {
    s.hdr[w] = h;
    s.cnt[w] = c;
  }
  __syncthreads();
  u64 hp = 0;
  int cp = 0;
  for (int i = 0; i < w; ++i) {
    hp = s.hdr[i] > hp ? s.hdr[i] : hp;
    cp += s.cnt[i];
  }
  u64 ht = 0;
  int ct = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ht = s.hdr[i] > ht ? s.hdr[i] : ht;
    ct += s.cnt[i];
  }
  u64 hx = __shfl_up(h, 1, 64);
  int cx = __shfl_up(c, 1, 64);
  if (lane == 0) {
    hx = 0;
    cx = 0;
  }
  *hdr_excl = hx > hp ? hx : hp;
  *cnt_excl = cx + cp;
  *hdr_tot = ht;
  *cnt_tot = ct;
  __syncthreads();
}

// ---- wave-level data movement on DPP (gfx9 row / wave shifts and row broadcasts): a few cycles
// each instead of an LDS round trip per __shfl (ds_bpermute).
template <int kCtrl, int kRowMask = 0xf, bool kBound = true>
__device__ __forceinline__ uint32_t dpp32(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, kCtrl, kRowMask, 0xf, kBound);
}
template <int kCtrl, int kRowMask = 0xf, bool kBound = true>
__device__ __forceinline__ u64 dpp64(u64 x) {
  const uint32_t lo = dpp32<kCtrl, kRowMask, kBound>((uint32_t)x);
  const uint32_t hi = dpp32<kCtrl, kRowMask, kBound>((uint32_t)(x >> 32));
  return ((u64)hi << 32) | lo;
}
constexpr int kDppWaveShl1 = 0x130;  // lane i <- lane i + 1 (lane 63 <- 0)
constexpr int kDppWaveShr1 = 0x138;  // lane i <- lane i - 1 (lane 0 <- 0)
__device__ __forceinline__ int32_t wave_next(int32_t x) { return (int32_t)dpp32<kDppWaveShl1>((uint32_t)x); }
__device__ __forceinline__ uint32_t wave_prev(uint32_t x) { return dpp32<kDppWaveShr1>(x); }
__device__ __forceinline__ u64 wave_prev64(u64 x) { return dpp64<kDppWaveShr1>(x); }

// Inclusive wave scans (sum / max, identity 0): row shifts 1, 2, 4, 8, then row broadcasts 15, 31.
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t x) {
  x += dpp32<0x111>(x);
  x += dpp32<0x112>(x);
  x += dpp32<0x114>(x);
  x += dpp32<0x118>(x);
  x += dpp32<0x142, 0xa, false>(x);
  x += dpp32<0x143, 0xc, false>(x);
  return x;
}
__device__ __forceinline__ u64 max64(u64 a, u64 b) { return a > b ? a : b; }
__device__ __forceinline__ u64 wave_scan_max64(u64 x) {
  x = max64(x, dpp64<0x111>(x));
  x = max64(x, dpp64<0x112>(x));
  x = max64(x, dpp64<0x114>(x));
  x = max64(x, dpp64<0x118>(x));
  x = max64(x, dpp64<0x142, 0xa, false>(x));
  x = max64(x, dpp64<0x143, 0xc, false>(x));
  return x;
}
__device__ __forceinline__ uint32_t lane_read(uint32_t x, int lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)x, lane);
}
__device__ __forceinline__ u64 lane_read64(u64 x, int lane) {
  return ((u64)lane_read((uint32_t)(x >> 32), lane) << 32) | lane_read((uint32_t)x, lane);
}

// Sum over the wave (every lane active), read back from lane 63 as a scalar.
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) { return lane_read(wave_scan_add(x), 63); }

// Loads this lane's 16 tokens of chunk [cs, cs+cl) (kPad beyond cl) as four unconditional
// 16-byte loads: tiles start 16-byte aligned and the stream is padded by kStreamPad elements, so
// reading a whole chunk from any tile start stays inside the allocation.  Branch-free, all four
// loads are in flight together (a bounds-checked form compiled to one wait per quad).
__device__ __forceinline__ void load_chunk(const int32_t* base, uint32_t cs, uint32_t cl, int p0, int32_t (&v)[kPer]) {
  const int4* q = reinterpret_cast<const int4*>(base + cs + p0);
  int4 x[kPer / 4];
#pragma unroll
  for (int k = 0; k < kPer / 4; ++k) x[k] = q[k];
#pragma unroll
  for (int k = 0; k < kPer / 4; ++k) {
    v[4 * k] = p0 + 4 * k < (int)cl ? x[k].x : kPad;
    v[4 * k + 1] = p0 + 4 * k + 1 < (int)cl ? x[k].y : kPad;
    v[4 * k + 2] = p0 + 4 * k + 2 < (int)cl ? x[k].z : kPad;
    v[4 * k + 3] = p0 + 4 * k + 3 < (int)cl ? x[k].w : kPad;
  }
}

// Token following this lane's 16 (from the next lane, or from memory at a wave edge).
__device__ __forceinline__ int32_t next_token(const int32_t* base, uint32_t cs, uint32_t len, int p0, int32_t v0) {
  int32_t nx = wave_next(v0);
  const int32_t m = base[cs + p0 + kPer];  // inside the padded allocation; used by lane 63 only
  if ((threadIdx.x & 63) == 63) nx = (cs + p0 + kPer < len) ? m : kPad;
  return nx;
}

// ---- what k_merge (bpe_device.hip) and k_resident (resident_loop.hip) share: the wave chunk and
// its LDS staging, the per-workgroup record regions, the per-tile pair signature, the delta tables.
constexpr int kWaveTok = 64 * kPer;  // 1024 tokens per wave chunk
constexpr int kWaves = kThreads / 64;
constexpr int kDeltaLdsW = SHRED_DELTA_LDS;
// LDS staging index skew: lane l touches positions 16 l + j together, which unskewed all fall in
// two of the 32 banks; i + i / 16 gives a stride of 17 words, conflict-free.
__device__ __forceinline__ int SK(int i) { return i + (i >> 4); }
constexpr int kStPad = kWaveTok + 8 + (kWaveTok + 8) / 16 + 1;
constexpr int kMaxMergeGroups = SHRED_MAX_GROUPS;
constexpr int kSigBits = SHRED_SIG_BITS;   // per-tile pair signature
constexpr int kSigWords = kSigBits / 32;
constexpr int kRegHdr = 8;                 // region header: nrec, nmt, spill, pad, merged (2), written (2)
static_assert(kSigWords % 256 == 0 || kSigWords == 64 || kSigWords == 128, "signature written as 16 B per lane");

// The two signature bits of pair (x, y).
__device__ __forceinline__ void sig_bits(int32_t x, int32_t y, uint32_t* h1, uint32_t* h2) {
  uint32_t k = (uint32_t)x * 0x9E3779B1u ^ ((uint32_t)y + 0x7F4A7C15u) * 0x85EBCA77u;
  k ^= k >> 15;
  k *= 0x2C1B3C6Du;
  k ^= k >> 12;
  k *= 0x297A2D39u;
  k ^= k >> 15;
  *h1 = k & (kSigBits - 1);
  *h2 = (k >> 16) & (kSigBits - 1);
}

__device__ __forceinline__ void sig_add(uint32_t* s, int32_t x, int32_t y) {
  uint32_t h1, h2;
  sig_bits(x, y, &h1, &h2);
  atomicOr(&s[h1 >> 5], 1u << (h1 & 31));
  atomicOr(&s[h2 >> 5], 1u << (h2 & 31));
}

// Writes a wave's LDS signature to the tile's HBM signature (16 B per lane per pass).
__device__ __forceinline__ void sig_store(uint32_t* dst, const uint32_t* s, int lane) {
  for (int w = lane * 4; w < kSigWords; w += 256) {
    uint4 v;
    v.x = s[w];
    v.y = s[w + 1];
    v.z = s[w + 2];
    v.w = s[w + 3];
    *reinterpret_cast<uint4*>(dst + w) = v;
  }
}

__device__ __forceinline__ void sig_clear(uint32_t* s, int lane) {
  for (int w = lane; w < kSigWords; w += 64) s[w] = 0;
}

// Orders this wave's LDS accesses across lanes (LDS executes one wave's ops in order; this
// keeps the compiler from moving them and drains lgkmcnt).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// Rebuilds a single-chunk tile's signature from its tokens v (this lane's 16, kPad beyond) and
// the token after them (nx); longer tiles keep an all-ones signature.
__device__ __forceinline__ void sig_rebuild(uint32_t* s_sig, uint32_t* dst, const int32_t (&v)[kPer], int32_t nx,
                                            int lane) {
  sig_clear(s_sig, lane);
  wave_lds_sync();
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int32_t x = v[j], y = j + 1 < kPer ? v[j + 1] : nx;
    if (!is_hdr(x) && !is_hdr(y)) sig_add(s_sig, x, y);
  }
  wave_lds_sync();
  sig_store(dst, s_sig, lane);
}

template <class P>
__device__ __forceinline__ void delta_global(const P& p, uint32_t key, u64 w, u64 ft) {
  atomicAdd(&p.dsum[key], w);
  const u64 old = atomicMin(&p.dft[key], ft);
  if (old == kEmpty64) {  // exactly one toucher sees MAX
    atomicExch(&p.dlist[atomicAdd(p.dcount, 1u)], key);
  }
}

__device__ __forceinline__ uint32_t slot_of(int32_t id, uint32_t cap) {
  return (uint32_t)id < cap ? (uint32_t)id + 1u : 0u;
}

__device__ __forceinline__ int wave_incl_sum(int x) { return (int)wave_scan_add((uint32_t)x); }

constexpr uint32_t kResMaxTiles = 320;  // tiles one k_resident workgroup may own (C5 at 100 GB: 271)

inline hipStream_t S(void* s) { return (hipStream_t)s; }
inline u64* U(uint64_t* p) { return reinterpret_cast<u64*>(p); }

template <class T>
T* dalloc(size_t n, size_t* acc) {
  void* p = nullptr;
  if (n == 0) n = 1;
  HIP_OK(hipMalloc(&p, n * sizeof(T)));
  *acc += n * sizeof(T);
  return (T*)p;
}

}  // namespace

}  // namespace shred
