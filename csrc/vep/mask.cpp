// CPU implementation of mask.h: the CPU backend's path and the byte-exact twin of the kernel.
#include "mask.h"

#include <algorithm>

#include "common.h"

namespace vep::mask {

void check_mask(const Mask& m) {
  VEP_CHECK(m.x0 >= 0 && m.x0 < m.x1 && m.x1 <= kUnit, "mask: need 0 <= x0 < x1 <= 10000");
  VEP_CHECK(m.y0 >= 0 && m.y0 < m.y1 && m.y1 <= kUnit, "mask: need 0 <= y0 < y1 <= 10000");
  VEP_CHECK(m.mode == kFill || m.mode == kPixelate, "mask: mode must be fill or pixelate");
  VEP_CHECK(m.block >= kMinBlock && m.block <= kMaxBlock, "mask: block must be 4..128");
  VEP_CHECK(m.b >= 0 && m.b <= 255 && m.g >= 0 && m.g <= 255 && m.r >= 0 && m.r <= 255,
            "mask: colour components must be 0..255");
}

void check_list(const Mask* m, int n) {
  VEP_CHECK(n >= 0 && n <= kMaxMasks, "mask: at most 8 masks per camera");
  VEP_CHECK(n == 0 || m, "mask: null list");
  for (int k = 0; k < n; ++k) check_mask(m[k]);
}

int levels(int w, int h, const Mask* m, int n, int* out) {
  VEP_CHECK(w >= 1 && h >= 1 && w <= kMaxSide && h <= kMaxSide, "mask: picture size must be 1..65535");
  check_list(m, n);
  Rect r[kMaxMasks];
  int top = 0;
  for (int k = 0; k < n; ++k) {
    r[k] = to_pixels(w, h, m[k]);
    int lv = 0;
    for (int e = 0; e < k; ++e)
      if (intersects(r[e], r[k])) lv = std::max(lv, out[e] + 1);
    out[k] = lv;
    top = std::max(top, lv + 1);
  }
  return top;
}

void apply_cpu(uint8_t* bgr, size_t pitch, int w, int h, const Mask* m, int n) {
  VEP_CHECK(bgr, "mask: null picture");
  VEP_CHECK(w >= 1 && h >= 1 && w <= kMaxSide && h <= kMaxSide, "mask: picture size must be 1..65535");
  VEP_CHECK(pitch >= size_t(w) * 3, "mask: pitch shorter than a row");
  check_list(m, n);
  for (int k = 0; k < n; ++k) {
    const Rect r = to_pixels(w, h, m[k]);
    if (m[k].mode == kFill) {
      const uint8_t c[3] = {uint8_t(m[k].b), uint8_t(m[k].g), uint8_t(m[k].r)};
      for (int y = r.y0; y < r.y1; ++y) {
        uint8_t* p = bgr + size_t(y) * pitch + size_t(r.x0) * 3;
        for (int x = r.x0; x < r.x1; ++x, p += 3) p[0] = c[0], p[1] = c[1], p[2] = c[2];
      }
      continue;
    }
    const int B = m[k].block;
    for (int by = r.y0; by < r.y1; by += B) {
      const int ey = std::min(by + B, r.y1);
      for (int bx = r.x0; bx < r.x1; bx += B) {
        const int ex = std::min(bx + B, r.x1);
        uint32_t sum[3] = {0, 0, 0};
        for (int y = by; y < ey; ++y) {
          const uint8_t* p = bgr + size_t(y) * pitch + size_t(bx) * 3;
          for (int x = bx; x < ex; ++x, p += 3) sum[0] += p[0], sum[1] += p[1], sum[2] += p[2];
        }
        const uint32_t cnt = uint32_t(ex - bx) * uint32_t(ey - by);
        const uint8_t c[3] = {uint8_t(block_value(sum[0], cnt)), uint8_t(block_value(sum[1], cnt)),
                              uint8_t(block_value(sum[2], cnt))};
        for (int y = by; y < ey; ++y) {
          uint8_t* p = bgr + size_t(y) * pitch + size_t(bx) * 3;
          for (int x = bx; x < ex; ++x, p += 3) p[0] = c[0], p[1] = c[1], p[2] = c[2];
        }
      }
    }
  }
}

}  // namespace vep::mask
