// The seeded draw of the dropout, masked-LM, span-corruption, fill-in-the-middle, MinHash, overlap and exact-dedup units:
//     d(x, c) = mix(mix(seed + G (x + 1)) ^ c)      (mix: murmur3's fmix64, arithmetic mod 2^64)
// x is a position or a row index, c says which decision of that x is drawn (bits 63..32 of d).
// Included by .hip files only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace shred {
namespace {

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;  // G

constexpr __host__ __device__ uint64_t fmix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

constexpr __host__ __device__ uint64_t draw(uint64_t seed, uint64_t x, uint64_t c) {
  return fmix64(fmix64(seed + kGolden * (x + 1)) ^ c);
}

// What c may be.  BPE-dropout passes the candidate's merge rank, which is below 2^32; every other
// decision has a constant here, above every merge rank, so that one seed given to several units
// (and to dropout) draws each decision independently.  A new unit adds its constants at the end.
enum Domain : uint64_t {
  kSel = 1ull << 40,  // masked-LM: unit x is selected
  kAct,               // masked-LM: what becomes of the selected token x
  kStart,             // span corruption: a span starts at x
  kLen,               // span corruption: its length
  kFimC,              // fill-in-the-middle: row x is transformed
  kCutA,              // fill-in-the-middle: its two cuts
  kCutB,
  kMode,              // fill-in-the-middle: PSM or SPM
  kMhShingle,         // MinHash: where the hash chain of a shingle of x ids starts
  kMhA,               // MinHash: multiplier and
  kMhB,               //          addend of permutation x
  kMhBand,            // MinHash: where the hash chain of band x starts
  kNgram,             // n-gram overlap: g(x), what id x adds to a fingerprint
  kMult,              // n-gram overlap: the multiplier of grams of x ids (exact dedup: x = 0)
  kRow,               // exact dedup: what a row of x ids adds to its sum
  kGroup              // exact dedup: what group x adds to a row's fingerprint
};
// (strictly increasing, so pairwise distinct)
static_assert(kSel >= 1ull << 40 && kAct == kSel + 1 && kStart == kAct + 1 && kLen == kStart + 1 &&
                  kFimC == kLen + 1 && kCutA == kFimC + 1 && kCutB == kCutA + 1 && kMode == kCutB + 1 &&
                  kMhShingle == kMode + 1 && kMhA == kMhShingle + 1 && kMhB == kMhA + 1 && kMhBand == kMhB + 1 &&
                  kNgram == kMhBand + 1 && kMult == kNgram + 1 && kRow == kMult + 1 && kGroup == kRow + 1,
              "the domain constants are (1 << 40) + 0 .. 15 (include/shredword_encode.h)");

// Values of the definition as the tests' Python reference computes it; the second wraps mod 2^64
// in seed + G (x + 1), the third is a dropout draw (c: a rank).
static_assert(draw(0, 0, kSel) == 0xf9293adfa22bb94eull, "draw");
static_assert(draw(0xFFFFFFFFFFFFFFFFull, 0x8000000000003039ull, kLen) == 0xf67eb8c521d928feull, "draw");
static_assert(draw(0x0123456789ABCDEFull, 41, 7) == 0x1b5bc2cbc1de4a8dull, "draw");

}  // namespace
}  // namespace shred
