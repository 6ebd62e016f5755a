// Area-average downscale and the camera wall: one definition of the arithmetic and the geometry,
// shared by the CPU implementation (scale.cpp) and the gfx950 kernel (gpu_scale.hip), so both
// produce the same bytes. docs/WALL.md has the reasoning.
//
// Resampling a source of sw x sh to ow x oh (1 <= ow <= sw, 1 <= oh <= sh), exact in integers:
// on an axis of sw * ow units, source column i covers [i * ow, (i + 1) * ow) and output column j
// covers [j * sw, (j + 1) * sw); wx(j, i) is the length of their overlap, so the weights of one
// output column sum to sw. Rows are the same with sh and oh. For each of B, G, R:
//   out(j, k) = (sum_r sum_i wy(k, r) * wx(j, i) * src(r, i) + (sw * sh) / 2) / (sw * sh)
// in integer division: no intermediate rounding, no float, no clamp (the result is in 0..255 by
// construction). ow == sw && oh == sh is the identity; at integer ratios the result is the
// round-half-up mean of the block.
//
// The sum of one output sample is at most 255 * sw * sh: it fits 32 bits while
// sw * sh <= kNarrowArea (4K fits, 4113 x 4096 does not). round_div32 rounds without adding the
// half to the sum, which would overflow from sw * sh = 16,810,049 on already.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VEP_SCALE_HD __host__ __device__
#else
#define VEP_SCALE_HD
#endif

namespace vep::scale {

constexpr int kMaxSide = 65535;            // of a source, an output, a tile and a canvas
constexpr uint32_t kNarrowArea = 16843009; // 255 * kNarrowArea == 2^32 - 1
constexpr uint8_t kBackground = 16;        // B = G = R of everything that is not picture

// First and last source index overlapping output index j (s source samples, o outputs).
VEP_SCALE_HD inline uint32_t span_lo(uint32_t j, uint32_t s, uint32_t o) { return j * s / o; }
VEP_SCALE_HD inline uint32_t span_hi(uint32_t j, uint32_t s, uint32_t o) { return ((j + 1) * s - 1) / o; }
// Overlap of source sample i with output j; i in [span_lo, span_hi] gives 1..o.
VEP_SCALE_HD inline uint32_t weight(uint32_t j, uint32_t i, uint32_t s, uint32_t o) {
  const uint32_t a = i * o > j * s ? i * o : j * s;
  const uint32_t b = (i + 1) * o < (j + 1) * s ? (i + 1) * o : (j + 1) * s;
  return b - a;
}
VEP_SCALE_HD inline bool narrow(uint32_t sw, uint32_t sh) { return uint64_t(sw) * sh <= kNarrowArea; }
// (sum + den / 2) / den for sum <= 255 * den
VEP_SCALE_HD inline uint32_t round_div32(uint32_t sum, uint32_t den) {
  const uint32_t q = sum / den, r = sum - q * den;
  return q + (r + den / 2 >= den ? 1u : 0u);
}
VEP_SCALE_HD inline uint32_t round_div64(uint64_t sum, uint64_t den) { return uint32_t((sum + den / 2) / den); }
// the one that fits the accumulator's type
VEP_SCALE_HD inline uint32_t round_div(uint32_t sum, uint32_t den) { return round_div32(sum, den); }
VEP_SCALE_HD inline uint32_t round_div(uint64_t sum, uint64_t den) { return round_div64(sum, den); }

// Fit sw x sh into a box of bw x bh keeping the aspect ratio, never enlarging. A side of the box
// that is not given counts as kMaxSide.
struct Size {
  int w, h;
};
inline Size fit(int sw, int sh, int bw, int bh) {
  if (bw <= 0) bw = kMaxSide;
  if (bh <= 0) bh = kMaxSide;
  if (bw >= sw && bh >= sh) return {sw, sh};
  auto other = [](int64_t a, int64_t b, int64_t o, int64_t cap) {  // b scaled by o / a, rounded
    int64_t v = (2 * b * o + a) / (2 * a);
    return int(v < 1 ? 1 : (v > cap ? cap : v));
  };
  if (int64_t(sw) * bh >= int64_t(sh) * bw) {
    const int ow = bw < sw ? bw : sw;
    return {ow, other(sw, sh, ow, bh < sh ? bh : sh)};
  }
  const int oh = bh < sh ? bh : sh;
  return {other(sh, sw, oh, bw < sw ? bw : sw), oh};
}

// Wall of n tiles: cols (0 = ceil(sqrt(n))) x rows cells of tw x th.
struct Wall {
  int cols, rows, w, h;
};
inline Wall wall(int n, int cols, int tw, int th) {
  if (cols <= 0) {
    cols = 1;
    while (cols * cols < n) ++cols;
  }
  const int rows = (n + cols - 1) / cols;
  return {cols, rows, cols * tw, rows * th};
}
// Tile t's picture in the canvas: fitted into its cell and centred.
struct Placement {
  int x, y, w, h;
};
inline Placement place(int t, int cols, int tw, int th, int sw, int sh) {
  const Size f = fit(sw, sh, tw, th);
  return {(t % cols) * tw + (tw - f.w) / 2, (t / cols) * th + (th - f.h) / 2, f.w, f.h};
}

// One tile of compose_cpu: a packed BGR24 picture, or null (background only).
struct Tile {
  const uint8_t* src = nullptr;
  int sw = 0, sh = 0;
  size_t pitch = 0;
};

// dst (oh rows of dst_pitch bytes) = src (sh rows of src_pitch bytes) resampled as above.
void area_cpu(const uint8_t* src, int sw, int sh, size_t src_pitch, uint8_t* dst, size_t dst_pitch, int ow,
              int oh);
// canvas (wall(n, cols, tw, th), rows of canvas_pitch bytes) = background + every tile's picture.
void compose_cpu(const Tile* tiles, int n, int cols, int tw, int th, uint8_t* canvas, size_t canvas_pitch);

}  // namespace vep::scale
