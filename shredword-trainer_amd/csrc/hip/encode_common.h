// What the encoder units (encode_device.hip, encode_spans.hip, encode_special.hip, ...) share on the
// host side: the error macro, the device guard, the device resources every pass's state is built
// from, and the piece rules of the host paths.
// Included by .hip files only.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../host/encoder.h"

// An encoder call reports a HIP error and returns -1 (the trainer's HIP_OK aborts instead).
#define ENC_OK(expr)                                                                            \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) {                                                                     \
      std::fprintf(stderr, "[ERROR]\t encoder: %s: %s\n", #expr, hipGetErrorString(e_));        \
      return -1;                                                                                \
    }                                                                                           \
  } while (0)

namespace shred {
namespace {

// Restores the caller's current device when an encoder call returns.
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// ---- device resources: each owns what it allocates and frees it when its pass state dies ----

struct NoCopy {
  NoCopy() = default;
  NoCopy(const NoCopy&) = delete;
  NoCopy& operator=(const NoCopy&) = delete;
};

// Grow-only device buffer.  grow(count) keeps a buffer that holds count elements and replaces a
// smaller one (the contents are lost); `arrays` > 1 allocates that many arrays of cap() elements
// side by side, the second at get() + cap().  A failed grow leaves the buffer empty.
template <class T>
class DeviceBuf : NoCopy {
 public:
  ~DeviceBuf() { reset(); }
  bool grow(size_t count, size_t arrays = 1) {
    if (count <= cap_) return true;
    reset();
    if (hipMalloc(&p_, count * arrays * sizeof(T)) != hipSuccess) {
      p_ = nullptr;
      return false;
    }
    cap_ = count;
    return true;
  }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  T* get() const { return p_; }
  size_t cap() const { return cap_; }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// A few 64-bit words of device memory (flags, error and result words), allocated once.
class DeviceWords : NoCopy {
 public:
  ~DeviceWords() {
    if (p_) (void)hipFree(p_);
  }
  bool ensure(size_t words) {
    if (p_) return true;
    if (hipMalloc(&p_, words * 8) == hipSuccess) return true;
    p_ = nullptr;
    return false;
  }
  uint64_t* get() const { return p_; }

 private:
  uint64_t* p_ = nullptr;
};

// The same in pinned host memory: where a call's result words are copied for the host to read.
class PinnedWords : NoCopy {
 public:
  ~PinnedWords() {
    if (p_) (void)hipHostFree(p_);
  }
  bool ensure(size_t words) {
    if (p_) return true;
    if (hipHostMalloc(&p_, words * 8, hipHostMallocDefault) == hipSuccess) return true;
    p_ = nullptr;
    return false;
  }
  uint64_t* get() const { return p_; }
  uint64_t& operator[](size_t i) const { return p_[i]; }

 private:
  uint64_t* p_ = nullptr;
};

// N events, recorded in pairs (2 i, 2 i + 1) around the timed regions of a call.
template <int N>
class EventSet : NoCopy {
 public:
  ~EventSet() {
    for (hipEvent_t e : ev_)
      if (e) (void)hipEventDestroy(e);
  }
  bool ensure() {
    for (hipEvent_t& e : ev_) {
      if (e) continue;
      if (hipEventCreate(&e) != hipSuccess) {
        e = nullptr;
        return false;
      }
    }
    return true;
  }
  hipEvent_t operator[](int i) const { return ev_[i]; }
  // Device time of pair i; of the first `pairs` pairs together.
  hipError_t pair_ms(int i, float* ms) const { return hipEventElapsedTime(ms, ev_[2 * i], ev_[2 * i + 1]); }
  hipError_t sum_ms(int pairs, double* ms) const {
    *ms = 0;
    for (int i = 0; i < pairs; ++i) {
      float t = 0;
      const hipError_t e = pair_ms(i, &t);
      if (e != hipSuccess) return e;
      *ms += (double)t;
    }
    return hipSuccess;
  }

 private:
  hipEvent_t ev_[N] = {};
};

// The pass's state behind one of EncodeDevice's slots, created on the pass's first call.
template <class S>
S& pass_state(std::unique_ptr<PassState>& slot) {
  if (!slot) slot.reset(new S());
  return static_cast<S&>(*slot);
}

// Staging of the host paths that encode text (encode_host, encode_spans_host, encode_docs_host):
// a piece's text and its ids on the device.
struct HostStage : PassState {
  DeviceBuf<uint8_t> text;
  DeviceBuf<int32_t> out;  // as many ids as text holds bytes
  bool reserve(size_t n) {
    if (text.grow(n) && out.grow(n)) return true;
    text.reset();
    out.reset();
    return false;
  }
};

// ---- pieces of the host paths ----

// The piece size of a host path: `def`, or the environment's (tests: small pieces), at least `minimum`.
inline size_t piece_from_env(const char* name, size_t def, size_t minimum) {
  const char* e = std::getenv(name);
  return e ? std::max<size_t>((size_t)std::strtoull(e, nullptr, 10), minimum) : def;
}

// The host's spelling of encode_words.h's is_delim (which is device code).
inline bool host_is_delim(uint8_t c) { return c == 9 || c == 10 || c == 13 || c == 32; }

// Length of the text piece at pos: at most `piece` bytes, ending just after its last delimiter
// (words never straddle two pieces, so the ids are those of one call); 0 = a word past the limit
// maxw.  With maxw == kEncMaxWord that is "no delimiter in the last kEncMaxWord + 1 bytes".  With a
// larger maxw (long-word mode) a budget that falls inside a longer word extends the piece forward
// to that word's end: the word is staged whole (pos is never inside a word).
inline size_t host_piece_len(const uint8_t* text, size_t n, size_t pos, size_t piece,
                             size_t maxw = (size_t)kEncMaxWord) {
  size_t len = std::min(piece, n - pos);
  if (pos + len < n) {
    size_t k = len;
    const size_t lo = len > (size_t)kEncMaxWord + 1 ? len - (size_t)kEncMaxWord - 1 : 0;
    while (k > lo && !host_is_delim(text[pos + k - 1])) --k;
    if (k == lo) {
      if (maxw <= (size_t)kEncMaxWord) return 0;
      while (k > 0 && len - k <= maxw && !host_is_delim(text[pos + k - 1])) --k;  // the word starts at pos + k
      size_t e = len;
      while (pos + e < n && e - k <= maxw && !host_is_delim(text[pos + e])) ++e;
      return e - k > maxw ? 0 : e;
    }
    len = k;
  }
  return len;
}

inline size_t count_newlines(const uint8_t* p, size_t n) {
  size_t c = 0;
  for (size_t i = 0; i < n; ++i) c += p[i] == 10;
  return c;
}

}  // namespace
}  // namespace shred
