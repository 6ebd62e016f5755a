// CPU implementation of motion.h: the CPU backend's path and the byte-exact twin of the kernel.
#include "motion.h"

#include <algorithm>

#include "common.h"

namespace vep::motion {

void check_update_params(int cell, int threshold, int learn_shift) {
  VEP_CHECK(cell >= kMinCell && cell <= kMaxCell, "motion: cell must be 4..256");
  VEP_CHECK(threshold >= 0 && threshold <= kMaxThreshold, "motion: threshold must be 0..255");
  VEP_CHECK(learn_shift >= 0 && learn_shift <= kMaxLearnShift, "motion: learn_shift must be 0..8");
}

void check_params(const Params& p) {
  check_update_params(p.cell, p.threshold, p.learn_shift);
  VEP_CHECK(p.cell_percent >= 1 && p.cell_percent <= 100, "motion: cell_percent must be 1..100");
  VEP_CHECK(p.min_cells >= 1, "motion: min_cells must be >= 1");
}

Summary summarize(const uint32_t* counts, int w, int h, int cell, int cell_percent, int min_cells) {
  VEP_CHECK(counts, "motion: null counts");
  VEP_CHECK(w >= 1 && h >= 1 && w <= kMaxSide && h <= kMaxSide, "motion: picture size must be 1..65535");
  VEP_CHECK(cell >= kMinCell && cell <= kMaxCell, "motion: cell must be 4..256");
  VEP_CHECK(cell_percent >= 1 && cell_percent <= 100, "motion: cell_percent must be 1..100");
  VEP_CHECK(min_cells >= 1, "motion: min_cells must be >= 1");
  const int cols = int(cells(uint32_t(w), uint32_t(cell))), rows = int(cells(uint32_t(h), uint32_t(cell)));
  Summary s;
  int x0 = cols, y0 = rows, x1 = -1, y1 = -1;  // active cells: inclusive bounds
  for (int gy = 0; gy < rows; ++gy) {
    const int ch = std::min(cell, h - gy * cell);
    for (int gx = 0; gx < cols; ++gx) {
      const int cw = std::min(cell, w - gx * cell);
      const uint64_t n = counts[size_t(gy) * cols + gx];
      s.changed += n;
      if (n * 100 < uint64_t(cw) * ch * uint64_t(cell_percent)) continue;
      ++s.active;
      x0 = std::min(x0, gx);
      y0 = std::min(y0, gy);
      x1 = std::max(x1, gx);
      y1 = std::max(y1, gy);
    }
  }
  if (s.active) {
    s.has_box = true;
    s.x = x0 * cell;
    s.y = y0 * cell;
    s.w = std::min(w, (x1 + 1) * cell) - s.x;
    s.h = std::min(h, (y1 + 1) * cell) - s.y;
  }
  s.motion = s.active >= min_cells;
  return s;
}

void update_cpu(const uint8_t* src, int w, int h, size_t src_pitch, const uint16_t* bg_in, uint16_t* bg_out,
                size_t bg_pitch_samples, int cell, int threshold, int learn_shift, uint32_t* counts) {
  VEP_CHECK(src && bg_out && counts, "motion: null picture, background or counts");
  VEP_CHECK(w >= 1 && h >= 1 && w <= kMaxSide && h <= kMaxSide, "motion: picture size must be 1..65535");
  check_update_params(cell, threshold, learn_shift);
  VEP_CHECK(src_pitch >= size_t(w) * 3 && bg_pitch_samples >= size_t(w), "motion: pitch shorter than a row");
  VEP_CHECK(bg_in != bg_out, "motion: the background is updated out of place");
  const uint32_t cols = cells(uint32_t(w), uint32_t(cell)), rows = cells(uint32_t(h), uint32_t(cell));
  std::fill(counts, counts + size_t(cols) * rows, uint32_t(0));
  for (int y = 0; y < h; ++y) {
    const uint8_t* p = src + size_t(y) * src_pitch;
    uint16_t* out = bg_out + size_t(y) * bg_pitch_samples;
    if (!bg_in) {
      for (int x = 0; x < w; ++x, p += 3) out[x] = uint16_t(prime(luma(p[0], p[1], p[2])));
      continue;
    }
    const uint16_t* in = bg_in + size_t(y) * bg_pitch_samples;
    uint32_t* row = counts + size_t(y / cell) * cols;
    for (int x = 0; x < w; ++x, p += 3) {
      const uint32_t Y = luma(p[0], p[1], p[2]), bg = in[x];
      if (changed(Y, ref_of(bg), uint32_t(threshold))) ++row[x / cell];
      out[x] = uint16_t(update(bg, Y, uint32_t(learn_shift)));
    }
  }
}

}  // namespace vep::motion
