// Dehazing of fog, haze and smoke by the dark-channel prior: one definition of the arithmetic,
// shared by the CPU implementation (dehaze.cpp) and the gfx950 kernels (gpu_dehaze.hip), so both
// produce the same bytes. docs/DEHAZE.md has the reasoning. Integers only; every width is stated
// with its bound where it arises.
//
// For a packed BGR24 picture of w x h (16 <= w, h <= 65535, w * h <= 2^24) and the parameters
//   patch     odd, 3..31 (default 15): the window of the dark channel, r = patch / 2
//   omega     0..256 in 1/256 (default 243: 0.95): how much of the veil is taken off
//   t0        51..1024 in 1/1024 (default 102: 0.1): the floor of the transmission
//   radius    1..16 cells (default 8): the box of the guided filter
//   strength  0..256 (default 256): the blend with the input
//
// 1. air light
//   m(x)      min(B, G, R)
//   D(x)      min of m over the patch x patch window around x, clipped to the picture
//   table     256 bins over D of {count, sum B, sum G, sum R}, u32: w h <= 2^24 keeps a sum below
//             2^24 * 255 < 2^32, so the order of accumulation does not matter
//   walk      from bin 255 down, WHOLE bins, until count n >= max(1, w h / 1000)
//   A_c       max(1, (sum_c + n / 2) / n)   (2^24 * 255 + 2^23 < 2^32). The floor of 1 is all the
//             division below needs, and it keeps a picture of one colour unchanged.
// 2. raw transmission
//   norm_c[v] min(255, (255 v + A_c / 2) / A_c), three tables of bytes: I_c / A_c in 1/255, capped at 1
//   N(x)      min_c norm_c[I_c(x)];  Dn(x) the same windowed minimum of N, a byte
//   t_raw     1024 - (4 omega Dn + 127) / 255, in 1/1024: 0..1024   (4 * 256 * 255 + 127 < 2^19)
// 3. refinement: a guided filter (guide: luma) on cells of 4 x 4 pixels, the right and bottom ones
//    partial, cw = ceil(w / 4) by ch = ceil(h / 4) of them
//   cell      over its n true pixels (1..16): Yc = (4 sum Y + n / 2) / n, 0..1020 (luma in 1/4
//             levels), Tc = (sum t_raw + n / 2) / n, 0..1024; stored as Yc | Tc << 16
//   box       over the cells within `radius` of the cell on both axes, clipped to the plane, K <= 33^2
//             of them: S_Y, S_T, S_YT, S_YY as u32 (1089 * 1020 * 1024 < 2^31)
//   a, b      in 1/1024 (kCoeffBits = 10), i64 arithmetic, floor division (fdiv):
//               num = K S_YT - S_Y S_T,  den = K S_YY - S_Y^2 + kEps K^2   (kEps = 1024: (32/1020)^2)
//               a = fdiv(1024 num + den / 2, den)          |a| <= 8 * 1024, since |cov| <=
//                   sqrt(var_Y var_T), var_T <= 512^2 and sqrt(v) / (v + eps) <= 1 / (2 sqrt(eps)) = 1/64
//               b = fdiv(1024 S_T - a S_Y + K / 2, K)      |b| <= 1024 * 1024 + 8192 * 1020 + 1 < 2^24
//   mean      box sums of a (i32: 1089 * 8192) and b (i64: 1089 * 2^24 > 2^31), then
//             mean_a = fdiv(S_a + K / 2, K), mean_b likewise: the same bounds as a and b
// 4. recovery
//   axis      pixel x lies between the centres of cells i0 and i1 = min(i0 + 1, n - 1) with weight
//             wx (in 1/8) of i1: u = 2 x - 3; u < 0: i0 = 0, wx = 0; else i0 = u / 8, wx = u % 8; and
//             i0 >= n - 1: i0 = i1 = n - 1, wx = 0 (clamped edges; a partial cell counts as whole)
//   t         with A, B the weighted sums of the four cells' mean_a, mean_b (weights sum to 64):
//             t = clamp((A * 4 Y + B + 2^15) >> 16, t0, 1024)   (|A * 4 Y| <= 2^19 * 1020, |B| <=
//             2^30: the sum stays below 2^31; the shift is arithmetic: floor)
//   J_c       A_c + (((I_c - A_c) * recip[t] + 2048) >> 12), clamped to 0..255, with
//             recip[t] = (2^22 + t / 2) / t <= 82241 (t >= 51), so 255 * recip < 2^25; recip[1024] = 4096
//   out       (I_c (256 - strength) + J_c strength + 128) >> 8
//
// Fixed properties (closed forms of tests/test_dehaze.py and csrc/tests/dehaze_selftest.cpp):
//   * strength = 0 is the identity, byte for byte.
//   * a picture of ONE colour comes out unchanged: A = I (a channel of 0 has A_c = 1 and
//     J_c = 1 + a negative number, clamped to 0), so I - A = 0. For the same reason I = A
//     everywhere comes out unchanged.
//   * |J_c - A_c| <= |I_c - A_c| * 1024 / t0 + 1: t0 bounds the gain.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "motion.h"

namespace vep::dehaze {

constexpr int kMinSide = 16, kMaxSide = motion::kMaxSide;
constexpr uint64_t kMaxPixels = uint64_t(1) << 24;
constexpr int kMinPatch = 3, kMaxPatch = 31;
constexpr int kMaxOmega = 256;
constexpr int kTOne = 1024, kMinT0 = 51;
constexpr int kMinRadius = 1, kMaxRadius = 16;
constexpr int kMaxStrength = 256;
constexpr int kBins = 256;
constexpr int kTableWords = kBins * 4;  // {count, sum B, sum G, sum R} per bin
constexpr int kAirWords = 4 + 3 * kBins / 4;  // {A_b, A_g, A_r, n}, then norm_b, norm_g, norm_r as bytes
constexpr int kCell = 4;
constexpr int kCoeffBits = 10;
constexpr int64_t kEps = 1024;
constexpr uint64_t kMaxBox = uint64_t(2 * kMaxRadius + 1) * (2 * kMaxRadius + 1);
static_assert(kMaxPixels * 255 + kMaxPixels / 2 < (uint64_t(1) << 32), "a bin's sum and its rounding fit a u32");
static_assert(kMaxBox * 1020 * 1024 < (uint64_t(1) << 31), "the box sums fit a u32");
static_assert(kMaxBox * (8u << kCoeffBits) < (uint64_t(1) << 31), "the box sum of a fits an i32");
static_assert((uint64_t(64) * (8u << kCoeffBits)) * 1020 + (uint64_t(64) << 24) + 32768 < (uint64_t(1) << 31), "t fits an i32");
static_assert(uint64_t(255) * ((uint64_t(1) << 22) / kMinT0 + 1) + 2048 < (uint64_t(1) << 31), "the recovery fits an i32");

struct Params {
  int patch = 15, omega = 243, t0 = 102, radius = 8, strength = 256;
};
// Throws unless patch is odd and 3..31, omega 0..256, t0 51..1024, radius 1..16, strength 0..256.
void check_params(const Params& p);

VEP_MOTION_HD inline uint32_t cells(uint32_t side) { return (side + kCell - 1) / kCell; }
VEP_MOTION_HD inline uint32_t min3(uint32_t a, uint32_t b, uint32_t c) {
  const uint32_t m = a < b ? a : b;
  return m < c ? m : c;
}
VEP_MOTION_HD inline uint32_t air_target(uint32_t w, uint32_t h) {
  const uint32_t n = w * h / 1000u;
  return n ? n : 1u;
}
VEP_MOTION_HD inline uint32_t air_of(uint32_t sum, uint32_t n) {
  const uint32_t a = (sum + n / 2u) / n;
  return a ? a : 1u;
}
VEP_MOTION_HD inline uint32_t norm_of(uint32_t v, uint32_t a) {
  const uint32_t q = (255u * v + a / 2u) / a;
  return q < 255u ? q : 255u;
}
VEP_MOTION_HD inline uint32_t t_raw(uint32_t omega, uint32_t dn) { return uint32_t(kTOne) - (4u * omega * dn + 127u) / 255u; }
VEP_MOTION_HD inline uint32_t cell_value(uint32_t sum_y, uint32_t sum_t, uint32_t n) {
  return (4u * sum_y + n / 2u) / n | ((sum_t + n / 2u) / n) << 16;
}
// Floor division, d > 0.
VEP_MOTION_HD inline int64_t fdiv(int64_t n, int64_t d) {
  const int64_t q = n / d;
  return n % d < 0 ? q - 1 : q;
}
// The cells of the box around cell c along a side of n cells: lo .. hi.
VEP_MOTION_HD inline void box_span(uint32_t c, uint32_t n, uint32_t radius, uint32_t& lo, uint32_t& hi) {
  lo = c > radius ? c - radius : 0u;
  hi = c + radius < n ? c + radius : n - 1u;
}
VEP_MOTION_HD inline void coeffs(uint32_t sy, uint32_t st, uint32_t syt, uint32_t syy, uint32_t k, int32_t& a, int32_t& b) {
  const int64_t K = int64_t(k);
  const int64_t num = K * int64_t(syt) - int64_t(sy) * int64_t(st);
  const int64_t den = K * int64_t(syy) - int64_t(sy) * int64_t(sy) + kEps * K * K;
  a = int32_t(fdiv(num * (int64_t(1) << kCoeffBits) + den / 2, den));
  b = int32_t(fdiv(int64_t(st) * (int64_t(1) << kCoeffBits) - int64_t(a) * int64_t(sy) + K / 2, K));
}
VEP_MOTION_HD inline int32_t box_mean(int64_t s, uint32_t k) { return int32_t(fdiv(s + int64_t(k / 2u), int64_t(k))); }
VEP_MOTION_HD inline void axis(uint32_t x, uint32_t n, uint32_t& i0, uint32_t& i1, uint32_t& wx) {
  i0 = i1 = wx = 0;
  if (2u * x >= 3u) {
    const uint32_t u = 2u * x - 3u;
    i0 = u >> 3;
    wx = u & 7u;
    i1 = i0 + 1u < n ? i0 + 1u : n - 1u;
  }
  if (i0 >= n - 1u) {
    i0 = i1 = n - 1u;
    wx = 0;
  }
}
VEP_MOTION_HD inline int32_t lerp4(int32_t c00, int32_t c01, int32_t c10, int32_t c11, uint32_t wx, uint32_t wy) {
  return int32_t((8u - wx) * (8u - wy)) * c00 + int32_t(wx * (8u - wy)) * c01 + int32_t((8u - wx) * wy) * c10 +
         int32_t(wx * wy) * c11;
}
VEP_MOTION_HD inline uint32_t transmission(int32_t a64, int32_t b64, uint32_t y, uint32_t t0) {
  const int32_t t = (a64 * int32_t(4u * y) + b64 + 32768) >> 16;  // (arithmetic shift: floor)
  return uint32_t(t < int32_t(t0) ? int32_t(t0) : (t > kTOne ? kTOne : t));
}
VEP_MOTION_HD inline uint32_t recip_of(uint32_t t) { return ((1u << 22) + t / 2u) / t; }
VEP_MOTION_HD inline uint32_t recovered(uint32_t i, uint32_t a, uint32_t recip, uint32_t strength) {
  int32_t j = int32_t(a) + (((int32_t(i) - int32_t(a)) * int32_t(recip) + 2048) >> 12);
  j = j < 0 ? 0 : (j > 255 ? 255 : j);
  return (i * (256u - strength) + uint32_t(j) * strength + 128u) >> 8;
}

// One picture's job as the host states it: the picture, the output and the five scratch planes
// with the sizes of their memory (elements).
struct Job {
  const uint8_t* src = nullptr;
  size_t src_bytes = 0;
  uint32_t src_pitch = 0;
  uint8_t* dst = nullptr;
  size_t dst_bytes = 0;
  uint32_t dst_pitch = 0;
  int w = 0, h = 0;
  Params p;
  uint32_t* table = nullptr;  // kTableWords
  uint32_t* air = nullptr;    // kAirWords
  uint32_t* cell = nullptr;   // ch x cw
  int32_t* ab = nullptr;      // ch x cw x {a, b}
  int32_t* mean = nullptr;    // ch x cw x {mean_a, mean_b}
  size_t table_words = 0, air_words = 0, cell_words = 0, ab_words = 0, mean_words = 0;
};
// Throws unless the parameters are in range, both sides are 16..65535 with w h <= 2^24, every row
// of the source and of the destination lies inside its memory, the two are the same picture (equal
// pitches: in place) or apart, every plane is 8-byte aligned, large enough, and apart from the
// others and from both pictures.
void check_job(const Job& j);
// The five planes of a w x h picture carved from one 8-byte aligned buffer of plane_words(w, h)
// u32: table, air, ab, mean, cell, in this order.
size_t plane_words(int w, int h);
void carve_planes(Job& j, uint32_t* words);

// The passes on the host, on a checked job's planes. apply_cpu is the only one that writes dst.
void table_cpu(const Job& j);   // 1: D and the table
void air_cpu(const Job& j);     // 1: the walk, A and the norm tables
void cells_cpu(const Job& j);   // 2 and the cell means of 3
void coeff_cpu(const Job& j);   // 3: a and b
void smooth_cpu(const Job& j);  // 3: mean_a and mean_b
void apply_cpu(const Job& j);   // 4
// All six, checked.
void run_cpu(const Job& j);
// All six with planes of its own; air (3 values, may be null) receives A.
void dehaze_cpu(const uint8_t* src, size_t src_pitch, uint8_t* dst, size_t dst_pitch, int w, int h, const Params& p,
                uint32_t* air = nullptr);

}  // namespace vep::dehaze
