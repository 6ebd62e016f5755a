// Temporal denoising of a served picture from the ring's history: one definition of the arithmetic,
// shared by the CPU implementation (denoise.cpp) and the gfx950 kernel (gpu_denoise.hip), so both
// produce the same bytes. docs/DENOISE.md has the reasoning. Integers only; every intermediate fits
// a u32 (the bounds are stated where they arise).
//
// For K packed BGR24 frames F_0 .. F_{K-1} of one size w x h (1 <= w, h <= 65535; F_0 the newest,
// 1 <= K <= 8) and the parameters
//   level     T, 1..64 luma levels (default 8): the noise floor
//   strength  S, 0..256 (default 256)
//   luma      Y_k = motion::luma(B, G, R) of frame k, 0..255
//   distance  for k >= 1 and pixel p: d_k(p) = sum over the 3 x 3 neighbourhood q of p of
//             |Y_0(q) - Y_k(q)|, coordinates clamped to the picture (edge replication): 0..2295
//   weight    s = d_k * 16 / (9 * T) (floor): the mean absolute difference in 1/16 of T;
//             w_k = 16 for s <= 16, 0 for s >= 32, else 32 - s; then w_k = (w_k * S) >> 8.
//             w_0 = 16 always. An earlier frame counts fully while its mean absolute luma
//             difference around p is at most T, not at all from 2 T upward, linearly in between.
//   pixel     W = sum w_k (16..128); every channel c: out[c] = (sum_k w_k * F_k[c] + W / 2) / W
//             (the sum is at most 128 * 255 + 64 = 32704).
//
// The kernel divides by multiplying: n / D = (n * ceil(2^32 / D)) >> 32 is exact while
// n * (D * ceil(2^32 / D) - 2^32) < 2^32, and that error term is below D. For s: n = 16 d <= 36720,
// D = 9 T <= 576; for the pixel: n <= 32704, D = W <= 128: both products stay below 2^25.
// csrc/tests/denoise_selftest.cpp checks every d, T, W and every n exhaustively.
//
// Fixed properties (closed forms of tests/test_denoise.py and csrc/tests/denoise_selftest.cpp):
//   * K = 1 is the identity, byte for byte: W = 16, out = (16 c + 8) / 16 = c.
//   * S = 0 is the identity: every w_k = 0 for k >= 1.
//   * K identical frames give the identity: d = 0, w = 16 (S = 256), out = (W c + W / 2) / W = c;
//     for any S the weighted mean of equal values is that value.
//   * an earlier frame whose luma differs by more than 2 T everywhere has d > 18 T, s >= 32, w = 0.
//   * two one-colour frames with |Y_a - Y_b| <= T: d <= 9 T, s <= 16, w = 16, out = (a + b + 1) / 2.
//   * every output channel lies between the minimum and maximum of that channel over the K frames
//     (a weighted mean, rounded to nearest, of integers in that range).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "motion.h"

namespace vep::denoise {

constexpr int kMaxSide = motion::kMaxSide;
constexpr int kMaxFrames = 8;
constexpr int kMinLevel = 1, kMaxLevel = 64;
constexpr int kMaxStrength = 256;
constexpr uint32_t kFull = 16;                  // the weight of a frame that counts fully
constexpr uint32_t kMaxDistance = 9 * 255;      // 2295
constexpr uint32_t kMaxWeightSum = kFull * kMaxFrames;  // 128
constexpr uint32_t kMaxChannelSum = kMaxWeightSum * 255 + kMaxWeightSum / 2;
static_assert(kMaxDistance * 16 < (1u << 16) && 9 * kMaxLevel < (1 << 10), "16 d and 9 T are small");
static_assert(uint64_t(kMaxDistance) * 16 * (9 * kMaxLevel) < (uint64_t(1) << 32), "the reciprocal of 9 T is exact over 16 d");
static_assert(uint64_t(kMaxChannelSum) * kMaxWeightSum < (uint64_t(1) << 32), "the reciprocal of W is exact over a channel sum");
static_assert(kFull * kMaxStrength >> 8 == kFull, "strength 256 keeps a full weight");

struct Params {
  int frames = 4, level = 8, strength = 256;  // frames: how many a serving read asks the ring for, 2..8
};
// Throws unless frames is 2..8 (a serving read's request), level 1..64, strength 0..256.
void check_params(const Params& p);

// ceil(2^32 / D) for 2 <= D: the multiplier of div_by().
VEP_MOTION_HD constexpr uint32_t reciprocal(uint32_t divisor) {
  return uint32_t(((uint64_t(1) << 32) + divisor - 1) / divisor);
}
// n / D by its reciprocal (exact in the ranges above).
VEP_MOTION_HD inline uint32_t div_by(uint32_t n, uint32_t recip) { return uint32_t((uint64_t(n) * recip) >> 32); }

// w_k from s = 16 d / (9 T).
VEP_MOTION_HD inline uint32_t weight_of(uint32_t s, uint32_t strength) {
  const uint32_t w = s <= 16u ? 16u : (s >= 32u ? 0u : 32u - s);
  return (w * strength) >> 8;
}
// The definition, and the kernel's form with recip9t = reciprocal(9 T).
VEP_MOTION_HD inline uint32_t weight(uint32_t d, uint32_t level, uint32_t strength) {
  return weight_of(d * 16u / (9u * level), strength);
}
VEP_MOTION_HD inline uint32_t weight_fast(uint32_t d, uint32_t recip9t, uint32_t strength) {
  return weight_of(div_by(d * 16u, recip9t), strength);
}
// out[c] from the channel's weighted sum and W.
VEP_MOTION_HD inline uint32_t mean(uint32_t sum, uint32_t wsum) { return (sum + wsum / 2u) / wsum; }

// reciprocal(W) for W = 0 .. 128 (entries below 16 are never used): the kernel's table.
struct WeightSumTable {
  uint32_t r[kMaxWeightSum + 1];
};
constexpr WeightSumTable weight_sum_table() {
  WeightSumTable t{};
  for (uint32_t w = 0; w <= kMaxWeightSum; ++w) t.r[w] = w < 2 ? 0u : reciprocal(w);
  return t;
}

// One picture's job as the host states it: K sources, each `src_bytes[k]` long, and a destination.
struct Job {
  const uint8_t* src[kMaxFrames] = {};
  size_t src_bytes[kMaxFrames] = {};
  uint32_t src_pitch[kMaxFrames] = {};
  uint8_t* dst = nullptr;
  size_t dst_bytes = 0;
  uint32_t dst_pitch = 0;
  int w = 0, h = 0, frames = 0, level = 0, strength = 0;
};
// Throws unless 1 <= frames <= 8, level and strength are in range, the size is 1..65535, every
// row of every source and of the destination lies inside its memory, and the destination overlaps
// no source (out of place only: a source is never written). Sources may overlap or repeat.
void check_job(const Job& j);

// The K frames (src[k]: h rows of src_pitch[k] bytes, newest first) denoised into dst. Checked.
void denoise_cpu(const Job& j);

}  // namespace vep::denoise
