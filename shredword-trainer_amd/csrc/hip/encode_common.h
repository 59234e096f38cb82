// What the encoder units (encode_device.hip, encode_spans.hip, encode_special.hip, ...) share on the
// host side.
// Included by .hip files only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdio>

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

}  // namespace
}  // namespace shred
