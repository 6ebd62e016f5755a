// Contrast enhancement of dark scenes, contrast-limited adaptive histogram equalisation (CLAHE) on
// luma: one definition of the arithmetic, shared by the CPU implementation (clahe.cpp) and the
// gfx950 kernels (gpu_clahe.hip), so both produce the same bytes. docs/ENHANCE.md has the
// reasoning. Integers only; every intermediate fits a u32 (the bounds are stated where they arise).
//
// For a packed BGR24 picture of w x h (1 <= w, h <= 65535) and the parameters
//   tile      32..256, a multiple of 8 (default 128)
//   clip16    the clip limit in 1/16 of the mean bin height, 16..4096 (default 32: 2.0 x)
//   strength  0..256 (default 256)
//   luma      Y = motion::luma(B, G, R), 0..255
//   grid      cells of tile x tile pixels, cols = ceil(w / tile), rows = ceil(h / tile), the right
//             and bottom tiles partial. With rw = w - (cols - 1) * tile the last column is THIN when
//             cols > 1 and 2 * rw < tile; thin rows likewise.
//   group     a thin column's tiles and their left neighbours share one histogram and one LUT (the
//             same for rows; the corner is a group of four): a sliver of a few pixels with a LUT of
//             its own would show as a stripe at the picture's edge. group_of() names a tile's group
//             by its first tile. A group is less than 1.5 tiles wide and high: n < 384^2 = 147,456.
//   LUT       of a group with histogram h[256] over its n pixels:
//               L      = max(1, clip16 * n / 4096)                  (4096 * 147,456 < 2^32)
//               E      = sum max(0, h[v] - L),  h'[v] = min(h[v], L)
//               q, r   = E / 256, E % 256
//               h''[v] = h'[v] + q + (((v + 1) * r >> 8) > (v * r >> 8))   exactly r extras, evenly
//                        spaced; one pass, no second clip; sum h'' = n
//               c[v]   = h''[0] + .. + h''[v]
//               m[v]   = (c[v] * 255 + n / 2) / n                   (147,456 * 255 + n / 2 < 2^32)
//               lut[v] = (v * (256 - strength) + m[v] * strength + 128) >> 8
//             The LUT is monotone and lut[255] = 255 (c[255] = n).
//   pixel     along x with u = 2 * x + 1 - tile: u < 0: i0 = i1 = 0, ax = 0; else i0 = u / (2 * tile),
//             ax = (u - i0 * 2 * tile) * 128 / tile (0..255), i1 = min(i0 + 1, cols - 1); and
//             i0 >= cols - 1: i0 = i1 = cols - 1, ax = 0. The y axis gives j0, j1, ay the same way.
//             With a, b, c, d the LUT values at Y of the tiles (i0,j0), (i1,j0), (i0,j1), (i1,j1):
//               Y' = ((256-ax)*(256-ay)*a + ax*(256-ay)*b + (256-ax)*ay*c + ax*ay*d + 32768) >> 16
//             (the weights sum to 65536, so the sum is at most 65536 * 255 + 32768 < 2^32), and
//             every channel becomes clamp(ch + (Y' - Y), 0, 255). The shift is ADDITIVE: B - Y and
//             R - Y are untouched, nothing divides, and chroma noise of dark areas is not amplified
//             as a multiplicative gain Y' / Y would.
//
// Fixed properties (closed forms of tests/test_clahe.py and csrc/tests/clahe_selftest.cpp):
//   * strength = 0 is the identity, byte for byte: lut[v] = (256 v + 128) >> 8 = v, so Y' = Y.
//   * clip16 = 4096 never clips: L = n >= every h[v], E = 0: plain adaptive equalisation.
//   * a picture of ONE colour, luma v0, moves every channel by at most one_colour_bound(): there
//     h[v0] = n, so c[v0] lies within 1 of (v0 + 1) * (n - L) / 256 + L, m[v0] within 1/2 + 255 / n
//     of 255 * c[v0] / n, and 255 * ((v0 + 1) * (1 - L/n) / 256 + L/n) - v0 lies in
//     [0, 1 + 255 * L / n). Hence |m[v0] - v0| < 2 + 255 * L / n; the strength fold and the blend
//     (a weighted mean of four such values) stay inside that.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "motion.h"

namespace vep::clahe {

constexpr int kMaxSide = motion::kMaxSide;
constexpr int kMinTile = 32, kMaxTile = 256;
constexpr int kMinClip16 = 16, kMaxClip16 = 4096;
constexpr int kMaxStrength = 256;
constexpr int kBins = 256;
// pixels of the largest group: less than 1.5 tiles on each side
constexpr uint64_t kMaxGroup = uint64_t(kMaxTile + kMaxTile / 2) * (kMaxTile + kMaxTile / 2);
static_assert(uint64_t(kMaxClip16) * kMaxGroup < (uint64_t(1) << 32), "clip16 * n fits a u32");
static_assert(kMaxGroup * 255 + kMaxGroup / 2 < (uint64_t(1) << 32), "c[v] * 255 + n / 2 fits a u32");
static_assert(uint64_t(65536) * 255 + 32768 < (uint64_t(1) << 32), "the blend fits a u32");
static_assert(uint64_t(256) * 255 < (uint64_t(1) << 32) && 2 * kMaxSide + 1 < (int64_t(1) << 31), "extras and u fit");

struct Params {
  int tile = 128, clip16 = 32, strength = 256;
};
// Throws unless tile is 32..256 and a multiple of 8, clip16 16..4096, strength 0..256.
void check_params(const Params& p);

using motion::cells;
// Whether the last of `n` cells along a side of `side` pixels is thin.
VEP_MOTION_HD inline bool thin(uint32_t side, uint32_t tile, uint32_t n) { return n > 1 && 2 * (side - (n - 1) * tile) < tile; }
// The first cell of cell i's group along a side, and the group's pixels along it.
VEP_MOTION_HD inline uint32_t group_of(uint32_t i, uint32_t side, uint32_t tile, uint32_t n) {
  return thin(side, tile, n) && i == n - 1 ? n - 2 : i;
}
VEP_MOTION_HD inline uint32_t group_span(uint32_t g, uint32_t side, uint32_t tile, uint32_t n) {
  if (thin(side, tile, n) && g == n - 2) return side - g * tile;  // tile + the thin rest
  return g == n - 1 ? side - g * tile : tile;
}

VEP_MOTION_HD inline uint32_t clip_limit(uint32_t clip16, uint32_t n) {
  const uint32_t l = clip16 * n / 4096u;
  return l ? l : 1u;
}
// h''[v] from h[v] and the excess E of the whole histogram.
VEP_MOTION_HD inline uint32_t redistributed(uint32_t hv, uint32_t v, uint32_t limit, uint32_t excess) {
  const uint32_t q = excess >> 8, r = excess & 255u;
  return (hv < limit ? hv : limit) + q + ((((v + 1u) * r) >> 8) > ((v * r) >> 8) ? 1u : 0u);
}
// lut[v] from c[v].
VEP_MOTION_HD inline uint32_t lut_value(uint32_t v, uint32_t cv, uint32_t n, uint32_t strength) {
  const uint32_t m = (cv * 255u + n / 2u) / n;
  return (v * (256u - strength) + m * strength + 128u) >> 8;
}

// Index and weight of pixel x along a side of n cells: the two cells i0, i1 and i1's weight a (0..255).
VEP_MOTION_HD inline void axis(uint32_t x, uint32_t tile, uint32_t n, uint32_t& i0, uint32_t& i1, uint32_t& a) {
  const int32_t u = int32_t(2u * x + 1u) - int32_t(tile);
  i0 = i1 = a = 0;
  if (u >= 0) {
    i0 = uint32_t(u) / (2u * tile);
    a = (uint32_t(u) - i0 * 2u * tile) * 128u / tile;
    i1 = i0 + 1u < n ? i0 + 1u : n - 1u;
  }
  if (i0 >= n - 1u) {
    i0 = i1 = n - 1u;
    a = 0;
  }
}
VEP_MOTION_HD inline uint32_t blend(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t ax, uint32_t ay) {
  return ((256u - ax) * (256u - ay) * a + ax * (256u - ay) * b + (256u - ax) * ay * c + ax * ay * d + 32768u) >> 16;
}
VEP_MOTION_HD inline uint32_t shifted(uint32_t ch, uint32_t y_new, uint32_t y) {
  const int32_t v = int32_t(ch) + int32_t(y_new) - int32_t(y);
  return uint32_t(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// The most a channel of a one-colour picture moves: 2 + ceil(255 * L / n) over a group of n pixels
// (derived above; the smallest group of a picture gives the largest value).
inline uint32_t one_colour_bound(uint32_t clip16, uint32_t n) {
  return 2u + uint32_t((uint64_t(255) * clip_limit(clip16, n) + n - 1) / n);
}

// The LUT of one group: hist[256] over n = sum hist pixels -> lut[256]. Throws unless n is that sum.
void lut_of_group(const uint32_t* hist, uint32_t n, int clip16, int strength, uint8_t* lut);

// The three passes on the host; src / dst are h rows of their pitch, hist is rows x cols x 256 u32
// (one histogram per TILE, every bin written), lut rows x cols x 256 u8 (a tile holds its group's
// LUT). apply_cpu works in place (dst == src with equal pitches) or out of place.
void hist_cpu(const uint8_t* src, int w, int h, size_t src_pitch, int tile, uint32_t* hist);
void luts_cpu(const uint32_t* hist, int w, int h, const Params& p, uint8_t* lut);
void apply_cpu(const uint8_t* src, size_t src_pitch, uint8_t* dst, size_t dst_pitch, int w, int h, int tile,
               const uint8_t* lut);
// All three, with planes of its own.
void enhance_cpu(const uint8_t* src, size_t src_pitch, uint8_t* dst, size_t dst_pitch, int w, int h, const Params& p);

}  // namespace vep::clahe
