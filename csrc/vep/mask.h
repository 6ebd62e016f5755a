// Per-camera privacy masks (fill, pixelate): one definition of the arithmetic, shared by the CPU
// implementation (mask.cpp) and the gfx950 kernel (gpu_mask.hip), so both produce the same bytes.
// docs/PRIVACY.md has the reasoning. Integers only.
//
// A mask is a rectangle in 1/10000 of the picture's width and height (0 <= x0 < x1 <= 10000,
// likewise y), so it survives a resolution change. to_pixels() rounds it OUTWARD to pixels:
//   px0 = x0 * W / 10000, px1 = (x1 * W + 9999) / 10000, the same for y (integer division);
// the pixel rect is never empty and never leaves the picture.
//   fill      every pixel of the rect becomes (b, g, r)
//   pixelate  blocks of B x B pixels (B 4..128) anchored at (px0, py0), the right and bottom ones
//             partial; per channel every pixel of a block becomes (sum + n / 2) / n, n the block's
//             pixel count, sum over its pixels (<= 255 * 128 * 128 < 2^32)
// A camera has at most kMaxMasks masks, applied in list order, each on the picture as the earlier
// ones left it. levels() gives mask k the level 1 + (the largest level of the earlier masks whose
// pixel rects intersect it), 0 when none does: masks of one level are disjoint, and applying the
// levels in ascending order equals applying the list in order.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VEP_MASK_HD __host__ __device__
#else
#define VEP_MASK_HD
#endif

namespace vep::mask {

constexpr int kMaxMasks = 8;
constexpr int kUnit = 10000;  // a coordinate's full scale
constexpr int kMinBlock = 4, kMaxBlock = 128;
constexpr int kDefaultBlock = 16;  // a design choice, not a measured one
constexpr int kMaxSide = 65535;
enum Mode : int { kFill = 0, kPixelate = 1 };

struct Mask {
  int x0 = 0, y0 = 0, x1 = kUnit, y1 = kUnit;  // 1/10000 of the width / height
  int mode = kPixelate;
  int block = kDefaultBlock;  // pixelate only
  int b = 0, g = 0, r = 0;    // fill only
};
struct Rect {
  int x0, y0, x1, y1;  // pixels, x1 / y1 exclusive
};

static_assert(int64_t(kMaxSide) * kUnit + (kUnit - 1) < (int64_t(1) << 31), "to_pixels stays in 32 bits");
static_assert(uint64_t(255) * kMaxBlock * kMaxBlock + kMaxBlock * kMaxBlock / 2 < (uint64_t(1) << 32),
              "a block's sum fits a u32");

// One axis: [a, b) in 1/10000 of n pixels -> pixels, rounded outward, never empty, inside 0..n.
VEP_MASK_HD inline void axis_pixels(int n, int a, int b, int& p0, int& p1) {
  p0 = a * n / kUnit;
  p1 = (b * n + (kUnit - 1)) / kUnit;
  if (p1 > n) p1 = n;
  if (p0 > n - 1) p0 = n - 1;
  if (p0 < 0) p0 = 0;
  if (p1 <= p0) p1 = p0 + 1;
}
VEP_MASK_HD inline Rect to_pixels(int w, int h, const Mask& m) {
  Rect r{0, 0, 1, 1};
  axis_pixels(w, m.x0, m.x1, r.x0, r.x1);
  axis_pixels(h, m.y0, m.y1, r.y0, r.y1);
  return r;
}
// The value of a block's channel out of its sum and its pixel count.
VEP_MASK_HD inline uint32_t block_value(uint32_t sum, uint32_t n) { return (sum + n / 2) / n; }
VEP_MASK_HD inline bool intersects(const Rect& a, const Rect& b) {
  return a.x0 < b.x1 && b.x0 < a.x1 && a.y0 < b.y1 && b.y0 < a.y1;
}

// Throws unless the mask (the list) is valid: coordinates, mode, block 4..128, colour 0..255, at
// most kMaxMasks masks.
void check_mask(const Mask& m);
void check_list(const Mask* m, int n);
// out[k] = the level of mask k of a w x h picture (see above); n <= kMaxMasks. Returns the
// number of levels (0 for an empty list).
int levels(int w, int h, const Mask* m, int n, int* out);

// The list applied in order, in place, to a packed BGR24 picture of h rows of `pitch` bytes.
void apply_cpu(uint8_t* bgr, size_t pitch, int w, int h, const Mask* m, int n);

}  // namespace vep::mask
