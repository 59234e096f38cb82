// How an example of the pair form (shred_pair_*) turns into its emitted rows: what the strategy
// keeps of each side, how many rows it emits and how long the longest is.  One rule for the host's
// length pass (encoder.cpp, on host offset arrays) and for the kernels and hipCUB iterators of
// batch_pair.hip, which take it by value.
#pragma once

#include <cstdint>

#include "encoder.h"

#ifdef __HIPCC__
#define SHRED_HD __host__ __device__ __forceinline__
#else
#define SHRED_HD inline __attribute__((always_inline))
#endif

namespace shred {

struct Pairs {
  const int64_t* ra;   // rows + 1 entries each
  const int64_t* rb;
  uint64_t na, nb;
  uint64_t B;               // kept ids per emitted row: max_len - add, or kNoLimit
  uint64_t max_a, stride;   // strategy 3 (max_a 0: all of a)
  uint32_t strategy, left, bos_n, mid_n, eos_n;
  int32_t bos, mid0, mid1, eos;

  SHRED_HD uint64_t add() const { return (uint64_t)(bos_n + mid_n + eos_n); }
  SHRED_HD void bounds(uint64_t r, uint64_t* a0, uint64_t* a1, uint64_t* b0, uint64_t* b1) const {
    *a0 = (uint64_t)ra[r];
    *a1 = (uint64_t)ra[r + 1];
    *b0 = (uint64_t)rb[r];
    *b1 = (uint64_t)rb[r + 1];
  }
  // ka and cb: kb for strategies 0 .. 2, the window capacity C for strategy 3.  False: the example
  // cannot be made to fit (nothing is set).
  SHRED_HD bool fit(uint64_t la, uint64_t lb, uint64_t* ka, uint64_t* cb) const {
    if (strategy == 0) {
      if (lb <= B && la <= B - lb) {  // la + lb <= B
        *ka = la;
        *cb = lb;
      } else if ((la < lb ? la : lb) <= B / 2) {  // the shorter stays whole
        *ka = la <= lb ? la : B - lb;
        *cb = la <= lb ? B - la : lb;
      } else {
        *ka = B - B / 2;
        *cb = B / 2;
      }
      return true;
    }
    if (strategy == 1) {
      if (lb > B) return false;
      *ka = la < B - lb ? la : B - lb;
      *cb = lb;
      return true;
    }
    if (strategy == 2) {
      if (la > B) return false;
      *ka = la;
      *cb = lb < B - la ? lb : B - la;
      return true;
    }
    const uint64_t k = max_a && max_a < la ? max_a : la;
    if (k > B || B - k <= stride) return false;
    *ka = k;
    *cb = B - k;
    return true;
  }
  // w_r (1 for an example that cannot fit: the call fails before the value is used).
  SHRED_HD uint64_t count(uint64_t r) const {
    if (strategy != 3) return 1;
    uint64_t a0, a1, b0, b1, ka, C;
    bounds(r, &a0, &a1, &b0, &b1);
    return fit(a1 - a0, b1 - b0, &ka, &C) ? window_count(b1 - b0, C, C - stride) : 1;
  }
  // ka and the kb of the example's first (its longest) emitted row.
  SHRED_HD bool first(uint64_t la, uint64_t lb, uint64_t* ka, uint64_t* kb) const {
    if (!fit(la, lb, ka, kb)) return false;
    if (strategy == 3 && lb < *kb) *kb = lb;
    return true;
  }
  // Whether a first row of ka and kb kept ids has more than INT32_MAX ids.
  SHRED_HD bool too_long(uint64_t ka, uint64_t kb) const {
    return ka > (uint64_t)INT32_MAX || kb > (uint64_t)INT32_MAX || add() + ka + kb > (uint64_t)INT32_MAX;
  }
  // The largest e of example r (0 for one that cannot fit).
  SHRED_HD uint64_t emit(uint64_t r) const {
    uint64_t a0, a1, b0, b1, ka, kb;
    bounds(r, &a0, &a1, &b0, &b1);
    return first(a1 - a0, b1 - b0, &ka, &kb) ? add() + ka + kb : 0;
  }
#ifdef __HIPCC__
  // Emitted id j of a row of e = add + ka + kb ids, and its token type.
  __device__ __forceinline__ int32_t id(const int32_t* __restrict__ ids_a, const int32_t* __restrict__ ids_b,
                                        uint64_t ka, uint64_t kb, uint64_t asrc, uint64_t bsrc, uint64_t j,
                                        uint32_t* type) const {
    *type = 0;
    if (j < (uint64_t)bos_n) return bos;
    j -= (uint64_t)bos_n;
    if (j < ka) return ids_a[asrc + j];
    j -= ka;
    if (j < (uint64_t)mid_n) return j ? mid1 : mid0;
    j -= (uint64_t)mid_n;
    *type = 1;
    return j < kb ? ids_b[bsrc + j] : eos;
  }
#endif
};

inline Pairs pairs_of(const EncodeDevice::PairOpts& o, const int64_t* ra, uint64_t na, const int64_t* rb,
                      uint64_t nb) {
  const uint32_t b = o.has_bos ? 1u : 0u, e = o.has_eos ? 1u : 0u;
  return Pairs{ra, rb, na, nb, o.max_len ? o.max_len - (b + o.mid_n + e) : kNoLimit, o.max_a, o.stride,
               (uint32_t)o.strategy, o.trunc_side ? 1u : 0u, b, o.mid_n, e, o.bos, o.mid[0], o.mid[1], o.eos};
}

}  // namespace shred

#undef SHRED_HD
