// CPU implementation of clahe.h: the CPU backend's path and the byte-exact twin of the kernels.
#include "clahe.h"

#include <algorithm>
#include <vector>

#include "common.h"

namespace vep::clahe {

void check_params(const Params& p) {
  VEP_CHECK(p.tile >= kMinTile && p.tile <= kMaxTile && p.tile % 8 == 0, "enhance: tile must be 32..256 and a multiple of 8");
  VEP_CHECK(p.clip16 >= kMinClip16 && p.clip16 <= kMaxClip16, "enhance: clip must be 1.0..256.0");
  VEP_CHECK(p.strength >= 0 && p.strength <= kMaxStrength, "enhance: strength must be 0..1");
}

static void check_picture(const void* a, const void* b, int w, int h) {
  VEP_CHECK(a && b, "enhance: null picture or plane");
  VEP_CHECK(w >= 1 && h >= 1 && w <= kMaxSide && h <= kMaxSide, "enhance: picture size must be 1..65535");
}

void lut_of_group(const uint32_t* hist, uint32_t n, int clip16, int strength, uint8_t* lut) {
  VEP_CHECK(hist && lut && n >= 1 && n <= kMaxGroup, "enhance: a group has 1..147456 pixels");
  check_params(Params{kMinTile, clip16, strength});
  const uint32_t limit = clip_limit(uint32_t(clip16), n);
  uint32_t excess = 0;
  uint64_t total = 0;
  for (int v = 0; v < kBins; ++v) {
    excess += hist[v] > limit ? hist[v] - limit : 0u;
    total += hist[v];
  }
  VEP_CHECK(total == n, "enhance: the histogram must sum to n");  // (the u32 bounds of clahe.h rest on it)
  uint32_t c = 0;
  for (uint32_t v = 0; v < uint32_t(kBins); ++v) {
    c += redistributed(hist[v], v, limit, excess);
    lut[v] = uint8_t(lut_value(v, c, n, uint32_t(strength)));
  }
}

void hist_cpu(const uint8_t* src, int w, int h, size_t src_pitch, int tile, uint32_t* hist) {
  check_picture(src, hist, w, h);
  check_params(Params{tile, kMinClip16, 0});
  VEP_CHECK(src_pitch >= size_t(w) * 3, "enhance: pitch shorter than a row");
  const uint32_t cols = cells(uint32_t(w), uint32_t(tile)), rows = cells(uint32_t(h), uint32_t(tile));
  std::fill(hist, hist + size_t(cols) * rows * kBins, uint32_t(0));
  for (int y = 0; y < h; ++y) {
    const uint8_t* p = src + size_t(y) * src_pitch;
    uint32_t* row = hist + size_t(y / tile) * cols * kBins;
    for (int x = 0; x < w; ++x, p += 3) ++row[size_t(x / tile) * kBins + motion::luma(p[0], p[1], p[2])];
  }
}

void luts_cpu(const uint32_t* hist, int w, int h, const Params& p, uint8_t* lut) {
  check_picture(hist, lut, w, h);
  check_params(p);
  const uint32_t tile = uint32_t(p.tile), cols = cells(uint32_t(w), tile), rows = cells(uint32_t(h), tile);
  for (uint32_t j = 0; j < rows; ++j)
    for (uint32_t i = 0; i < cols; ++i) {
      const uint32_t gi = group_of(i, uint32_t(w), tile, cols), gj = group_of(j, uint32_t(h), tile, rows);
      uint8_t* out = lut + (size_t(j) * cols + i) * kBins;
      if (gi != i || gj != j) continue;  // (filled from its group's first tile below)
      const uint32_t gw = group_span(gi, uint32_t(w), tile, cols), gh = group_span(gj, uint32_t(h), tile, rows);
      uint32_t sum[kBins] = {};
      for (uint32_t jj = gj; jj < rows && group_of(jj, uint32_t(h), tile, rows) == gj; ++jj)
        for (uint32_t ii = gi; ii < cols && group_of(ii, uint32_t(w), tile, cols) == gi; ++ii)
          for (int v = 0; v < kBins; ++v) sum[v] += hist[(size_t(jj) * cols + ii) * kBins + size_t(v)];
      lut_of_group(sum, gw * gh, p.clip16, p.strength, out);
    }
  for (uint32_t j = 0; j < rows; ++j)
    for (uint32_t i = 0; i < cols; ++i) {
      const uint32_t gi = group_of(i, uint32_t(w), tile, cols), gj = group_of(j, uint32_t(h), tile, rows);
      if (gi != i || gj != j)
        std::copy_n(lut + (size_t(gj) * cols + gi) * kBins, size_t(kBins), lut + (size_t(j) * cols + i) * kBins);
    }
}

void apply_cpu(const uint8_t* src, size_t src_pitch, uint8_t* dst, size_t dst_pitch, int w, int h, int tile,
               const uint8_t* lut) {
  check_picture(src, dst, w, h);
  VEP_CHECK(lut, "enhance: null picture or plane");
  check_params(Params{tile, kMinClip16, 0});
  VEP_CHECK(src_pitch >= size_t(w) * 3 && dst_pitch >= size_t(w) * 3, "enhance: pitch shorter than a row");
  VEP_CHECK(src != dst || src_pitch == dst_pitch, "enhance: in place needs equal pitches");
  const uint32_t cols = cells(uint32_t(w), uint32_t(tile)), rows = cells(uint32_t(h), uint32_t(tile));
  struct Col {
    uint32_t i0, i1, a;
  };
  std::vector<Col> cx((size_t(w)));
  for (int x = 0; x < w; ++x) axis(uint32_t(x), uint32_t(tile), cols, cx[size_t(x)].i0, cx[size_t(x)].i1, cx[size_t(x)].a);
  for (int y = 0; y < h; ++y) {
    uint32_t j0, j1, ay;
    axis(uint32_t(y), uint32_t(tile), rows, j0, j1, ay);
    const uint8_t* top = lut + size_t(j0) * cols * kBins;
    const uint8_t* bot = lut + size_t(j1) * cols * kBins;
    const uint8_t* p = src + size_t(y) * src_pitch;
    uint8_t* q = dst + size_t(y) * dst_pitch;
    for (int x = 0; x < w; ++x, p += 3, q += 3) {
      const Col& c = cx[size_t(x)];
      const uint32_t Y = motion::luma(p[0], p[1], p[2]);
      const size_t a0 = size_t(c.i0) * kBins + Y, a1 = size_t(c.i1) * kBins + Y;
      const uint32_t y_new = blend(top[a0], top[a1], bot[a0], bot[a1], c.a, ay);
      q[0] = uint8_t(shifted(p[0], y_new, Y));
      q[1] = uint8_t(shifted(p[1], y_new, Y));
      q[2] = uint8_t(shifted(p[2], y_new, Y));
    }
  }
}

void enhance_cpu(const uint8_t* src, size_t src_pitch, uint8_t* dst, size_t dst_pitch, int w, int h, const Params& p) {
  check_picture(src, dst, w, h);
  check_params(p);
  const size_t tiles = size_t(cells(uint32_t(w), uint32_t(p.tile))) * cells(uint32_t(h), uint32_t(p.tile));
  std::vector<uint32_t> hist(tiles * kBins);
  std::vector<uint8_t> lut(tiles * kBins);
  hist_cpu(src, w, h, src_pitch, p.tile, hist.data());
  luts_cpu(hist.data(), w, h, p, lut.data());
  apply_cpu(src, src_pitch, dst, dst_pitch, w, h, p.tile, lut.data());
}

}  // namespace vep::clahe
