// CPU implementation of tamper.h: the CPU backend's path and the byte-exact twin of the kernel.
#include "tamper.h"

#include <algorithm>

#include "common.h"

namespace vep::tamper {

void check_cell(int cell) { VEP_CHECK(cell >= kMinCell && cell <= kMaxCell, "tamper: cell must be 8..128"); }

void check_params(const Params& p) {
  check_cell(p.cell);
  VEP_CHECK(p.dark_level >= 0 && p.dark_level <= 255, "tamper: dark_level must be 0..255");
  VEP_CHECK(p.bright_level >= 0 && p.bright_level <= 255, "tamper: bright_level must be 0..255");
  VEP_CHECK(p.spread_min >= 0 && p.spread_min <= 255, "tamper: spread_min must be 0..255");
  VEP_CHECK(p.focus_percent >= 0 && p.focus_percent <= 100, "tamper: focus_percent must be 0..100");
  VEP_CHECK(p.shift_level >= 0 && p.shift_level <= 255, "tamper: shift_level must be 0..255");
  VEP_CHECK(p.shift_percent >= 1 && p.shift_percent <= 100, "tamper: shift_percent must be 1..100");
}

Summary summarize(const uint32_t* hist, const uint32_t* sum_y, const uint32_t* energy, int w, int h, const Params& p,
                  const Reference* ref) {
  VEP_CHECK(hist && sum_y && energy, "tamper: null histogram or grid");
  VEP_CHECK(w >= 1 && h >= 1 && w <= kMaxSide && h <= kMaxSide, "tamper: picture size must be 1..65535");
  check_params(p);
  const int cell = p.cell;
  const int cols = int(cells(uint32_t(w), uint32_t(cell))), rows = int(cells(uint32_t(h), uint32_t(cell)));
  if (ref && (ref->w != w || ref->h != h || ref->cell != cell || ref->sum_y.size() != size_t(cols) * rows)) ref = nullptr;
  Summary s;
  s.n = uint64_t(w) * uint64_t(h);
  s.cells = cols * rows;
  s.has_reference = ref != nullptr;
  for (int gy = 0; gy < rows; ++gy) {
    const int ch = std::min(cell, h - gy * cell);
    for (int gx = 0; gx < cols; ++gx) {
      const int cw = std::min(cell, w - gx * cell);
      const size_t at = size_t(gy) * cols + gx;
      s.mean_sum += sum_y[at];
      s.energy_total += energy[at];
      s.pairs_total += pairs_of(uint32_t(cw), uint32_t(ch));
      if (ref) {
        const int64_t d = int64_t(sum_y[at]) - int64_t(ref->sum_y[at]);
        if (uint64_t(d < 0 ? -d : d) > uint64_t(p.shift_level) * uint64_t(cw) * uint64_t(ch)) ++s.shifted;
      }
    }
  }
  auto percentile = [&](uint64_t k) {
    uint64_t cum = 0;
    for (int v = 0; v < kBins; ++v) {
      cum += hist[v];
      if (cum * 100 >= k * s.n) return v;
    }
    return kBins - 1;  // (a histogram that does not sum to n)
  };
  s.p5 = percentile(5);
  s.p95 = percentile(95);
  s.dark = s.mean_sum <= uint64_t(p.dark_level) * s.n;
  s.bright = s.mean_sum >= uint64_t(p.bright_level) * s.n;
  s.flat = s.p95 - s.p5 < p.spread_min;
  if (ref) {
    s.defocused = p.focus_percent > 0 && s.energy_total * 100 < uint64_t(p.focus_percent) * ref->energy_total;
    s.moved = uint64_t(s.shifted) * 100 >= uint64_t(p.shift_percent) * uint64_t(s.cells);
  }
  s.tampered = s.dark || s.bright || s.flat || s.defocused || s.moved;
  return s;
}

void stats_cpu(const uint8_t* src, int w, int h, size_t src_pitch, int cell, uint32_t* hist, uint32_t* sum_y,
               uint32_t* energy) {
  VEP_CHECK(src && hist && sum_y && energy, "tamper: null picture, histogram or grid");
  VEP_CHECK(w >= 1 && h >= 1 && w <= kMaxSide && h <= kMaxSide, "tamper: picture size must be 1..65535");
  check_cell(cell);
  VEP_CHECK(src_pitch >= size_t(w) * 3, "tamper: pitch shorter than a row");
  const uint32_t cols = cells(uint32_t(w), uint32_t(cell)), rows = cells(uint32_t(h), uint32_t(cell));
  std::fill(hist, hist + kBins, uint32_t(0));
  std::fill(sum_y, sum_y + size_t(cols) * rows, uint32_t(0));
  std::fill(energy, energy + size_t(cols) * rows, uint32_t(0));
  std::vector<uint8_t> lum[2] = {std::vector<uint8_t>(size_t(w)), std::vector<uint8_t>(size_t(w))};
  auto lumas = [&](int y, std::vector<uint8_t>& out) {
    const uint8_t* p = src + size_t(y) * src_pitch;
    for (int x = 0; x < w; ++x, p += 3) out[size_t(x)] = uint8_t(motion::luma(p[0], p[1], p[2]));
  };
  lumas(0, lum[0]);
  for (int y = 0; y < h; ++y) {
    const uint8_t* cur = lum[y & 1].data();
    const uint8_t* below = nullptr;  // the row a vertical pair ends in, where it lies in the same cell
    if (y + 1 < h) {
      lumas(y + 1, lum[(y + 1) & 1]);
      if ((y + 1) % cell != 0) below = lum[(y + 1) & 1].data();
    }
    const size_t row = size_t(y / cell) * cols;
    for (int x = 0; x < w; ++x) {
      const uint32_t Y = cur[x];
      const size_t at = row + size_t(x / cell);
      ++hist[Y];
      sum_y[at] += Y;
      if (x + 1 < w && (x + 1) % cell != 0) energy[at] += sq_diff(cur[x + 1], Y);
      if (below) energy[at] += sq_diff(below[x], Y);
    }
  }
}

}  // namespace vep::tamper
