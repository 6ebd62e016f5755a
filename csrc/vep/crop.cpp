// CPU implementation of crop.h: the CPU backend's path and the byte-exact twin of the kernel.
#include "crop.h"

#include <algorithm>
#include <vector>

#include "common.h"

namespace vep::crop {

void check_box(const Box& b) {
  VEP_CHECK(b.x0 >= 0 && b.x0 < b.x1 && b.x1 <= kUnit, "crop: need 0 <= x0 < x1 <= 10000");
  VEP_CHECK(b.y0 >= 0 && b.y0 < b.y1 && b.y1 <= kUnit, "crop: need 0 <= y0 < y1 <= 10000");
}

void check_list(const Box* b, int n) {
  VEP_CHECK(n >= 0 && n <= kMaxBoxes, "crop: at most 64 boxes per picture");
  VEP_CHECK(n == 0 || b, "crop: null list");
  for (int k = 0; k < n; ++k) check_box(b[k]);
}

void check_output(int ow, int oh, int fit, const Pad& pad) {
  VEP_CHECK(ow >= 1 && ow <= kMaxOut && oh >= 1 && oh <= kMaxOut, "crop: width and height must be 1..4096");
  VEP_CHECK(fit == kStretch || fit == kLetterbox, "crop: fit must be stretch or letterbox");
  VEP_CHECK(pad.b >= 0 && pad.b <= 255 && pad.g >= 0 && pad.g <= 255 && pad.r >= 0 && pad.r <= 255,
            "crop: pad colour components must be 0..255");
}

namespace {

// One rect resampled into its fitted rectangle of one output picture.
void resample(const uint8_t* src, size_t pitch, const mask::Rect& r, uint8_t* out, int ow, const Placement& p) {
  const uint32_t sw = uint32_t(r.x1 - r.x0), sh = uint32_t(r.y1 - r.y0), fw = uint32_t(p.w), fh = uint32_t(p.h);
  const uint64_t d = uint64_t(den(sw, fw)) * den(sh, fh);
  std::vector<Taps> tx(fw);
  for (uint32_t j = 0; j < fw; ++j) tx[j] = taps(j, sw, fw);
  // the horizontal sums of a source row, kept for the output rows that share it (enlarging: two
  // rows serve several output rows)
  std::vector<uint32_t> rows[2];
  int64_t held[2] = {-1, -1};
  auto hrow = [&](uint32_t y) -> const uint32_t* {
    const int s = int(y & 1u);
    if (held[s] == int64_t(y)) return rows[s].data();
    rows[s].resize(size_t(fw) * 3);
    const uint8_t* row = src + size_t(uint32_t(r.y0) + y) * pitch + size_t(r.x0) * 3;
    for (uint32_t j = 0; j < fw; ++j) {
      uint32_t h0 = 0, h1 = 0, h2 = 0;  // <= 255 * Dx
      for (uint32_t i = tx[j].lo; i <= tx[j].hi; ++i) {
        const uint32_t w = weight_of(tx[j], i);
        const uint8_t* q = row + size_t(i) * 3;
        h0 += w * q[0];
        h1 += w * q[1];
        h2 += w * q[2];
      }
      rows[s][size_t(j) * 3] = h0;
      rows[s][size_t(j) * 3 + 1] = h1;
      rows[s][size_t(j) * 3 + 2] = h2;
    }
    held[s] = int64_t(y);
    return rows[s].data();
  };
  std::vector<uint64_t> acc(size_t(fw) * 3);
  for (uint32_t k = 0; k < fh; ++k) {
    const Taps ty = taps(k, sh, fh);
    std::fill(acc.begin(), acc.end(), uint64_t(0));
    for (uint32_t y = ty.lo; y <= ty.hi; ++y) {
      const uint64_t wy = weight_of(ty, y);
      const uint32_t* h = hrow(y);
      for (size_t x = 0; x < acc.size(); ++x) acc[x] += wy * h[x];
    }
    uint8_t* o = out + (size_t(uint32_t(p.y) + k) * size_t(ow) + size_t(p.x)) * 3;
    for (size_t x = 0; x < acc.size(); ++x) o[x] = uint8_t(scale::round_div64(acc[x], d));
  }
}

}  // namespace

void apply_cpu(const uint8_t* src, size_t pitch, int w, int h, const Box* boxes, int n, uint8_t* out, int ow, int oh,
               int fit, const Pad& pad) {
  VEP_CHECK(src, "crop: null picture");
  VEP_CHECK(w >= 1 && h >= 1 && w <= kMaxSide && h <= kMaxSide, "crop: picture size must be 1..65535");
  VEP_CHECK(pitch >= size_t(w) * 3, "crop: pitch shorter than a row");
  check_list(boxes, n);
  check_output(ow, oh, fit, pad);
  VEP_CHECK(n == 0 || out, "crop: null output");
  const size_t one = size_t(ow) * size_t(oh) * 3;
  for (int k = 0; k < n; ++k) {
    const mask::Rect r = to_pixels(w, h, boxes[k]);
    const Placement p = fitted(r.x1 - r.x0, r.y1 - r.y0, ow, oh, fit);
    uint8_t* o = out + size_t(k) * one;
    if (p.w != ow || p.h != oh)
      for (size_t x = 0; x < one; x += 3) o[x] = uint8_t(pad.b), o[x + 1] = uint8_t(pad.g), o[x + 2] = uint8_t(pad.r);
    resample(src, pitch, r, o, ow, p);
  }
}

}  // namespace vep::crop
