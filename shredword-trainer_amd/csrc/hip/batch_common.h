// What the batch units (batch_device.hip, batch_pair.hip) share on the device: the tile geometry of
// their output-centric kernels, the search of a prefix sum by one wave, the kernel that writes a
// prefix sum out as int64, and the limit of their grids.  The host side they share is batch_state.h.
// Included by .hip files only.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "encode_common.h"

namespace shred {
namespace {

typedef uint64_t u64;

constexpr int kThreads = 256;
constexpr int kLane = 4;                   // int32 entries per lane: one 16-byte store
constexpr int kTile = kThreads * kLane;    // output entries per workgroup (BATCH_TILE)
constexpr int kStage = 512;                // rows staged in LDS per round (BATCH_STAGE)

// (not every unit writes a prefix sum out)
[[maybe_unused]] __global__ __launch_bounds__(kThreads) void k_bat_row_start(const u64* __restrict__ E, u64 rows, u64 base,
                                                            int64_t* __restrict__ row_start) {
  const u64 r = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (r <= rows) row_start[r] = (int64_t)(base + E[r]);
}

// upper_bound by the 64 lanes of one wave (all active): a step probes 64 entries spread over
// [lo, hi), so a search of 2^24 entries takes 4 rounds of loads instead of 24.
__device__ __forceinline__ u64 wave_upper_bound(const u64* __restrict__ E, u64 lo, u64 hi, u64 v, int lane) {
  while (lo < hi) {
    const u64 gap = (hi - lo) / 64 + 1;
    const u64 k = lo + (u64)lane * gap;
    // E does not decrease: the lanes that see an entry <= v are the first `le`
    const u64 le = (u64)__popcll(__ballot(k < hi && E[k] <= v));
    if (le == 0) {
      hi = lo;
    } else {
      const u64 next = lo + le * gap;
      lo += (le - 1) * gap + 1;
      hi = next < hi ? next : hi;
    }
  }
  return lo;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Grids are one workgroup per tile (per 256 rows: batch_rows_fit, host/encoder.h).
static_assert(kThreads == (int)kBatchRowsPerGroup, "batch_rows_fit assumes the row kernels' workgroup");
bool tiles_fit(u64 entries) { return entries / kTile < 0x7FFFFFFFull; }

}  // namespace
}  // namespace shred
