// Near-duplicate clusters and a keep mask from MinHash signatures and LSH band keys on gfx950: the step
// behind batch_minhash.hip (C ABI and definitions: include/shredword_encode.h, shred_dedup_*).  Bucket by
// 64-bit key, verify each row against its bucket's first row, take the connected components.  The unit
// shares the device resources and the pass state of encode_common.h, the batch units' workgroup and
// grid limit (batch_common.h) and fmix64 (draw_hash.h).  Its result is known only after its last pass
// and it has no pieces, so the batch units' device_call and host_pieces (batch_state.h) do not fit it.
//
//   k_dedup_init    parent[r] = r, the four counters to 0.
//   per group of g bands (g: what fits the table budget, or SHREDWORD_DEDUP_GROUP):
//     memset          the group's tables to 0xFF bytes: every slot free, every rep "none".
//     k_dedup_insert  one thread per cell (r, j) of the group.  Band j has an open-addressing table of
//                     cap = 2^k >= 2 R slots, keys (u64) and reps (u32) in two arrays.  The slot comes
//                     from fmix64(key), linear probing; a free slot is claimed with a 64-bit
//                     compare-and-swap of its key, and the row index goes into the slot's rep by
//                     atomicMin.  A band holds at most R distinct keys, so a table is never more than
//                     half full and every probe ends.  All 64 bits of 0xFF..FF mark a free slot, so a
//                     cell whose key is that value takes one side word per band instead of a slot.
//     k_dedup_link    one thread per cell again, behind the kernel boundary: rep(r, j) by the same
//                     probe.  A lane whose rep != r holds an edge.  Every lane first runs find on both
//                     ends, in parallel, and drops its edge when they share a root: a real duplicate
//                     pair meets in many bands, and all but its first meeting end here without a byte
//                     of sig read.  With min_equal == 0 the lanes that are left unite, still in
//                     parallel.  Otherwise the wave takes the edges left (a ballot) in rounds of
//                     64 / W at once: W = the power of two >= the units of a signature row (16-byte
//                     units when sig is 16-byte aligned and K % 4 == 0, else words), at most 64, lanes
//                     per edge.  The lanes of a group get the edge by shuffle, run find again (same
//                     addresses: one broadcast read; the edges of earlier rounds may have joined the
//                     ends), read both rows side by side, count equal columns, add the counts over the
//                     group with W - 1 xor shuffles, and the group's first lane unites when the count
//                     reaches min_equal.
//                     Cell t of a group is (row t / g, band t % g): a wave reads its keys in one stretch and
//                     its probes go to all g tables.  The band-major order (one band's table hot in the
//                     cache, keys read 8 B out of every 128 B) measured 1.3 to 1.6 times slower at the
//                     benchmark shape; SHREDWORD_DEDUP_ORDER=band still selects it, and
//                     SHREDWORD_DEDUP_LANES=wave takes W = 64, for measurements.
//   k_dedup_labels  behind the last group: label[r] = find(r), keep[r] = (label[r] == r), the roots
//                   counted by a ballot and one atomic add per wave.
//
// The union-find is lock-free on uint32 parent[R].  parent[x] <= x always: unite swings the larger
// root's parent from itself to the smaller root with a compare-and-swap and starts over from the new
// roots when it loses; find halves paths with relaxed stores of a grandparent, which only ever
// replace a non-root's parent by another of its ancestors.  So every chain descends and ends, a
// component's root is its smallest row, and label and keep do not depend on the order in which the
// edges arrive, on the grouping of the bands or on the cell order.  (Which edges the same-root tests
// drop does depend on it; the components do not: a dropped edge joins two rows already joined.)
//
// Scratch: 4 R (parent) + 12 g cap + 512 (tables) bytes, cap < 4 R.  Work is linear in R x B; traffic
// per cell: 8 B of key twice, two or three random 8 B / 4 B table accesses, and per verified edge 8 K B.
// No matrix instruction fits: 64-bit compares, atomics, popcounts.  All global indices are 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../host/encoder.h"
#include "batch_common.h"
#include "draw_hash.h"
#include "encode_common.h"

namespace shred {
namespace {

constexpr u64 kDdFree = ~0ull;            // a free slot's key
constexpr uint32_t kDdNone = 0xFFFFFFFFu; // a rep nobody has written: above every row index
constexpr u64 kDdBudget = u64(256) << 20; // bytes of tables a group of bands may take (at least one band)
constexpr int kDdSide = 128;              // side words: one per band of a group
static_assert(EncodeDevice::kDedupMaxBands <= kDdSide && EncodeDevice::kDedupMaxRows < kDdNone, "dedup");

// What the kernels know of a call; passed by value.
struct DdRule {
  u64 R;
  int K, B, min_equal;
  int b0, g;        // the group: bands [b0, b0 + g)
  u64 mask;         // cap - 1
  bool band_major;  // cell t is (t % R, t / R), else (t / g, t % g)
  bool vec;         // sig rows are 16-byte aligned: units of four words
  int units, W;     // units per signature row; lanes per edge, a power of two in [1, 64]
};

// The group's tables: g arrays of cap keys, g arrays of cap reps, kDdSide side words.
struct DdTables {
  u64* key;
  uint32_t* rep;
  uint32_t* side;
};

__device__ __forceinline__ uint32_t ld(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's tree, halving the path on the way.  Every index read from parent is a row index.
__device__ __forceinline__ uint32_t dd_find(uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = ld(parent + x);
    if (p == x) return x;
    const uint32_t gp = ld(parent + p);
    if (gp != p) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = gp;
  }
}

// Joins the trees of a and b: the larger root goes under the smaller.
__device__ __forceinline__ void dd_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = dd_find(parent, a);
    b = dd_find(parent, b);
    if (a == b) return;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    uint32_t expect = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expect, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return;
  }
}

// Cell t of the group -> its row and its band within the group.
__device__ __forceinline__ void dd_cell(const DdRule& q, u64 t, u64* r, int* j) {
  if (q.band_major) {
    *j = (int)(t / q.R);
    *r = t - (u64)*j * q.R;
  } else {
    *r = t / (u64)q.g;
    *j = (int)(t - *r * (u64)q.g);
  }
}

__global__ __launch_bounds__(kThreads) void k_dedup_init(uint32_t* __restrict__ parent, u64 R, u64* __restrict__ ctr) {
  const u64 r = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (r < R) parent[r] = (uint32_t)r;
  if (r < 4) ctr[r] = 0;
}

__global__ __launch_bounds__(kThreads) void k_dedup_insert(const u64* __restrict__ keys, DdRule q, DdTables tab) {
  const u64 t = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (t >= q.R * (u64)q.g) return;
  u64 r;
  int j;
  dd_cell(q, t, &r, &j);
  const u64 key = keys[r * (u64)q.B + (u64)(q.b0 + j)];
  if (key == kDdFree) {
    __hip_atomic_fetch_min(tab.side + j, (uint32_t)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  u64* const tk = tab.key + (u64)j * (q.mask + 1);
  u64 slot = fmix64(key) & q.mask;
  for (;;) {
    u64 cur = __hip_atomic_load(tk + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kDdFree &&
        __hip_atomic_compare_exchange_strong(tk + slot, &cur, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      break;         // claimed (on failure cur is the key that won the slot)
    if (cur == key) break;
    slot = (slot + 1) & q.mask;
  }
  __hip_atomic_fetch_min(tab.rep + (u64)j * (q.mask + 1) + slot, (uint32_t)r, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
}

// ctr: [1] edges (cells with rep != r), [2] edges dropped by a same-root test, [3] edges accepted.
__global__ __launch_bounds__(kThreads) void k_dedup_link(const u64* __restrict__ keys, const uint32_t* __restrict__ sig,
                                                         DdRule q, DdTables tab, uint32_t* __restrict__ parent,
                                                         u64* __restrict__ ctr) {
  const u64 t = (u64)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  uint32_t r32 = 0, rep = 0;
  bool edge = false;
  if (t < q.R * (u64)q.g) {  // (no lane leaves: the wave's ballots and shuffles below take all 64)
    u64 r;
    int j;
    dd_cell(q, t, &r, &j);
    r32 = rep = (uint32_t)r;
    const u64 key = keys[r * (u64)q.B + (u64)(q.b0 + j)];
    if (key == kDdFree) {
      rep = tab.side[j];
    } else {
      const u64* const tk = tab.key + (u64)j * (q.mask + 1);
      u64 slot = fmix64(key) & q.mask;
      for (;;) {
        const u64 cur = tk[slot];
        if (cur == key) {
          rep = tab.rep[(u64)j * (q.mask + 1) + slot];
          break;
        }
        if (cur == kDdFree) break;  // (k_dedup_insert has put every key of the group in)
        slot = (slot + 1) & q.mask;
      }
    }
    edge = rep < r32;
  }
  const u64 edges = __ballot(edge);
  if (!edges) return;
  edge = edge && dd_find(parent, r32) != dd_find(parent, rep);
  u64 todo = __ballot(edge);
  uint32_t dropped = (uint32_t)__popcll(edges & ~todo), accepted = 0;
  if (q.min_equal == 0) {
    if (edge) dd_unite(parent, r32, rep);
    accepted = (uint32_t)__popcll(todo);
  } else {
    const int W = q.W, grp = lane / W, gl = lane % W, per = 64 / W;
    while (todo) {
      u64 m = todo;  // this group's edge: the grp-th of those left
      for (int i = 0; i < grp; ++i) m &= m - 1;
      const bool has = m != 0;
      const int src = has ? __ffsll((unsigned long long)m) - 1 : 0;
      const uint32_t a = (uint32_t)__shfl((int)r32, src), b = (uint32_t)__shfl((int)rep, src);
      const bool open = has && dd_find(parent, a) != dd_find(parent, b);
      int c = 0;
      if (open) {
        const uint32_t* const x = sig + (u64)a * (u64)q.K;
        const uint32_t* const y = sig + (u64)b * (u64)q.K;
        if (q.vec) {
          for (int u = gl; u < q.units; u += W) {
            const uint4 v = reinterpret_cast<const uint4*>(x)[u], w = reinterpret_cast<const uint4*>(y)[u];
            c += (v.x == w.x) + (v.y == w.y) + (v.z == w.z) + (v.w == w.w);
          }
        } else {
          for (int u = gl; u < q.units; u += W) c += x[u] == y[u];
        }
      }
      for (int d = W >> 1; d; d >>= 1) c += __shfl_xor(c, d);  // stays inside the group: W-aligned, W = 2^k
      const bool first = has && gl == 0, join = first && open && c >= q.min_equal;
      if (join) dd_unite(parent, a, b);
      dropped += (uint32_t)__popcll(__ballot(first && !open));
      accepted += (uint32_t)__popcll(__ballot(join));
      for (int i = 0; i < per && todo; ++i) todo &= todo - 1;
    }
  }
  if (lane == 0) {
    atomicAdd((unsigned long long*)ctr + 1, (unsigned long long)__popcll(edges));
    if (dropped) atomicAdd((unsigned long long*)ctr + 2, (unsigned long long)dropped);
    if (accepted) atomicAdd((unsigned long long*)ctr + 3, (unsigned long long)accepted);
  }
}

// ctr[0]: the roots.  keep: nullptr when not asked for.
__global__ __launch_bounds__(kThreads) void k_dedup_labels(uint32_t* __restrict__ parent, u64 R, int64_t* __restrict__ label,
                                                           uint8_t* __restrict__ keep, u64* __restrict__ ctr) {
  const u64 r = (u64)blockIdx.x * kThreads + threadIdx.x;
  bool root = false;
  if (r < R) {
    const uint32_t l = dd_find(parent, (uint32_t)r);
    root = l == (uint32_t)r;
    label[r] = (int64_t)l;
    if (keep) keep[r] = root;
  }
  const u64 roots = __ballot(root);
  if ((threadIdx.x & 63) == 0 && roots) atomicAdd((unsigned long long*)ctr, (unsigned long long)__popcll(roots));
}

// The dedup passes' state, allocated on the first dedup call: the union-find, one group's tables, the
// counters and the staging of the host call.
struct DedupState : PassState {
  DeviceBuf<uint32_t> parent;
  DeviceBuf<u64> tab;  // per group: g cap keys, g cap reps (two to a word), the side words
  DeviceWords ctr;     // [0] components, [1 .. 3] k_dedup_link's
  PinnedWords host;
  EventSet<2> ev;
  DeviceBuf<u64> hkeys;       // host path: the keys,
  DeviceBuf<uint32_t> hsig;   // the signatures (when they are read),
  DeviceBuf<int64_t> hlabel;  // the labels
  DeviceBuf<uint8_t> hkeep;   // and the keep mask
  u64 last[4] = {};           // dedup_stats: of the last call
};

unsigned dd_grid(u64 n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// The passes on device arrays, R >= 1.  Returns the number of components or -1.
int64_t dedup_run(DedupState& ds, const uint32_t* sig, const u64* keys, u64 R, const EncodeDevice::DedupOpts& o,
                  int64_t* label, uint8_t* keep, hipStream_t st, double* kernel_ms) {
  u64 cap = 2;
  while (cap < 2 * R) cap <<= 1;
  const u64 fit = std::max<u64>(kDdBudget / (12 * cap), 1);
  const int g = (int)std::min<u64>({fit, (u64)o.B, (u64)piece_from_env("SHREDWORD_DEDUP_GROUP", (size_t)o.B, 1)});
  const u64 slots = (u64)g * cap, words = slots + slots / 2 + kDdSide / 2;
  if (!tiles_fit(R * (u64)g) || !ds.ctr.ensure(4) || !ds.host.ensure(4) || !ds.ev.ensure() || !ds.parent.grow(R) ||
      !ds.tab.grow(words)) {
    std::fprintf(stderr, "[ERROR]\t encoder: dedup allocation failed (%zu rows, %d bands at a time, %zu table bytes)\n",
                 (size_t)R, g, (size_t)(words * 8));
    return -1;
  }
  DdRule q{};
  q.R = R, q.K = o.K, q.B = o.B, q.min_equal = o.min_equal, q.mask = cap - 1;
  const char* order = std::getenv("SHREDWORD_DEDUP_ORDER");  // measurement switches
  const char* lanes = std::getenv("SHREDWORD_DEDUP_LANES");
  q.band_major = order && !std::strcmp(order, "band");  // row-major by default: the faster of the two
  q.vec = o.min_equal > 0 && aligned16(sig) && o.K % 4 == 0;
  q.units = q.vec ? o.K / 4 : o.K;
  q.W = 1;
  while (q.W < 64 && q.W < q.units) q.W <<= 1;
  if (lanes && !std::strcmp(lanes, "wave")) q.W = 64;
  const DdTables tab{ds.tab.get(), reinterpret_cast<uint32_t*>(ds.tab.get() + slots),
                     reinterpret_cast<uint32_t*>(ds.tab.get() + slots + slots / 2)};
  ENC_OK(hipEventRecord(ds.ev[0], st));
  k_dedup_init<<<dim3(dd_grid(R)), dim3(kThreads), 0, st>>>(ds.parent.get(), R, ds.ctr.get());
  ENC_OK(hipGetLastError());
  for (int b0 = 0; b0 < o.B; b0 += g) {
    q.b0 = b0, q.g = std::min(g, o.B - b0);
    const dim3 grid(dd_grid(R * (u64)q.g));
    ENC_OK(hipMemsetAsync(ds.tab.get(), 0xFF, words * 8, st));
    k_dedup_insert<<<grid, dim3(kThreads), 0, st>>>(keys, q, tab);
    ENC_OK(hipGetLastError());
    k_dedup_link<<<grid, dim3(kThreads), 0, st>>>(keys, sig, q, tab, ds.parent.get(), ds.ctr.get());
    ENC_OK(hipGetLastError());
  }
  k_dedup_labels<<<dim3(dd_grid(R)), dim3(kThreads), 0, st>>>(ds.parent.get(), R, label, keep, ds.ctr.get());
  ENC_OK(hipGetLastError());
  ENC_OK(hipEventRecord(ds.ev[1], st));
  ENC_OK(hipMemcpyAsync(ds.host.get(), ds.ctr.get(), 32, hipMemcpyDeviceToHost, st));
  ENC_OK(hipStreamSynchronize(st));
  double ms = 0;
  ENC_OK(ds.ev.sum_ms(1, &ms));
  if (kernel_ms) *kernel_ms = ms;
  ds.last[0] = 4 * (u64)ds.parent.cap() + 8 * (u64)ds.tab.cap();
  for (int i = 1; i < 4; ++i) ds.last[i] = ds.host[i];
  if (std::getenv("SHREDWORD_ENCODE_DEBUG"))
    std::fprintf(stderr,
                 "[DEBUG]\t encoder: dedup passes: %.4f ms, %d bands at a time, %s-major, %d lanes per edge, edges %llu, "
                 "dropped by the same-root tests %llu, accepted %llu, components %llu\n",
                 ms, g, q.band_major ? "band" : "row", q.W, (unsigned long long)ds.host[1],
                 (unsigned long long)ds.host[2], (unsigned long long)ds.host[3], (unsigned long long)ds.host[0]);
  return (int64_t)ds.host[0];
}

}  // namespace

int64_t EncodeDevice::dedup(const uint32_t* sig, const uint64_t* keys, size_t rows, const DedupOpts& o, int64_t* label,
                            uint8_t* keep, void* stream, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  return dedup_run(pass_state<DedupState>(pass_[kDedup]), sig, keys, rows, o, label, keep,
                   (hipStream_t)(stream ? stream : stream_), kernel_ms);
}

void EncodeDevice::dedup_stats(uint64_t* scratch_bytes, uint64_t* edges, uint64_t* dropped, uint64_t* accepted) const {
  const DedupState* ds = static_cast<const DedupState*>(pass_[kDedup].get());
  uint64_t* const out[4] = {scratch_bytes, edges, dropped, accepted};
  for (int i = 0; i < 4; ++i)
    if (out[i]) *out[i] = ds ? ds->last[i] : 0;
}

// Clustering is global, so the host call has no pieces: keys (and sig when it is read) go up whole, the
// passes run once, label and keep come back.
int64_t EncodeDevice::dedup_host(const uint32_t* sig, const uint64_t* keys, size_t rows, const DedupOpts& o,
                                 int64_t* label, uint8_t* keep) {
  DeviceGuard guard;
  ENC_OK(hipSetDevice(device_));
  DedupState& ds = pass_state<DedupState>(pass_[kDedup]);
  hipStream_t st = (hipStream_t)stream_;
  const size_t nk = rows * (size_t)o.B, ns = o.min_equal > 0 ? rows * (size_t)o.K : 0;
  if (!ds.hkeys.grow(nk) || !ds.hsig.grow(std::max<size_t>(ns, 1)) || !ds.hlabel.grow(rows) || !ds.hkeep.grow(rows)) {
    std::fprintf(stderr, "[ERROR]\t encoder: dedup staging allocation failed (%zu rows, %zu bytes of keys and signatures)\n",
                 rows, nk * 8 + ns * 4);
    return -1;
  }
  ENC_OK(hipMemcpyAsync(ds.hkeys.get(), keys, nk * 8, hipMemcpyHostToDevice, st));
  if (ns) ENC_OK(hipMemcpyAsync(ds.hsig.get(), sig, ns * 4, hipMemcpyHostToDevice, st));
  const int64_t count = dedup_run(ds, ds.hsig.get(), ds.hkeys.get(), rows, o, ds.hlabel.get(),
                                  keep ? ds.hkeep.get() : nullptr, st, nullptr);
  if (count < 0) return -1;
  ENC_OK(hipMemcpyAsync(label, ds.hlabel.get(), rows * 8, hipMemcpyDeviceToHost, st));
  if (keep) ENC_OK(hipMemcpyAsync(keep, ds.hkeep.get(), rows, hipMemcpyDeviceToHost, st));
  ENC_OK(hipStreamSynchronize(st));
  return count;
}

}  // namespace shred
