// Per-camera tamper detection (dark, bright, flat, defocused, moved): one definition of the
// arithmetic, shared by the CPU implementation (tamper.cpp) and the gfx950 kernel
// (gpu_tamper.hip), so both produce the same bytes. docs/TAMPER.md has the reasoning. Integers only.
//
// For a packed BGR24 picture of w x h (1 <= w, h <= 65535):
//   luma       Y = motion::luma(B, G, R), 0..255
//   histogram  hist[v] = pixels with Y == v (u32: 65535^2 < 2^32, so one bin holds a whole picture)
//   grid       cells of cell x cell pixels (cell 8..128), cols = ceil(w / cell), rows = ceil(h / cell),
//              the right and bottom cells partial; two u32 planes of rows x cols
//   sum_y      the sum of Y over the cell's pixels (<= 128^2 * 255)
//   energy     the squared-gradient focus measure over the pixel pairs INSIDE the cell:
//                (Y[x+1,y] - Y[x,y])^2  for x + 1 < w and (x + 1) % cell != 0, plus
//                (Y[x,y+1] - Y[x,y])^2  for y + 1 < h and (y + 1) % cell != 0
//              A cell of true size cw x ch has (cw - 1) * ch + cw * (ch - 1) pairs, so at cell = 128
//              the largest value is 2 * 128 * 127 * 65025 = 2,114,092,800 < 2^31: this bound is why
//              cell stops at 128. No pair crosses a cell boundary.
// The summary (host only, 64-bit sums) turns the three results into flags: see summarize().
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "motion.h"

namespace vep::tamper {

constexpr int kMaxSide = motion::kMaxSide;
constexpr int kMinCell = 8, kMaxCell = 128;
constexpr int kBins = 256;

// The squared difference of two lumas.
VEP_MOTION_HD inline uint32_t sq_diff(uint32_t a, uint32_t b) {
  const int32_t d = int32_t(a) - int32_t(b);
  return uint32_t(d * d);
}
// pairs inside a cell of true size cw x ch
VEP_MOTION_HD inline uint32_t pairs_of(uint32_t cw, uint32_t ch) { return (cw - 1) * ch + cw * (ch - 1); }
using motion::cells;

// Every cell in 8..128: the largest sum_y and the largest energy fit a u32.
constexpr bool cells_fit() {
  for (uint64_t cell = uint64_t(kMinCell); cell <= uint64_t(kMaxCell); ++cell) {
    if (cell * cell * 255u >= (uint64_t(1) << 32)) return false;
    if (2u * cell * (cell - 1) * 65025u >= (uint64_t(1) << 32)) return false;
  }
  return true;
}
static_assert(cells_fit(), "a cell's sum_y and energy must fit a u32");
static_assert(uint64_t(kMaxSide) * kMaxSide < (uint64_t(1) << 32), "one histogram bin holds a whole picture");

// The parameters hold for the whole hub. The defaults are design choices, not measured thresholds.
struct Params {
  int cell = 32;            // 8..128
  int dark_level = 32;      // 0..255: dark when the mean luma is <= this
  int bright_level = 224;   // 0..255: bright when the mean luma is >= this
  int spread_min = 24;      // 0..255: flat when p95 - p5 < this
  int focus_percent = 50;   // 0..100: defocused when energy < this share of the reference's, 0 = off
  int shift_level = 24;     // 0..255: a cell is shifted when its mean luma moved by more than this
  int shift_percent = 50;   // 1..100: moved when this share of the cells is shifted
};
// Throws unless every parameter is in its range.
void check_cell(int cell);
void check_params(const Params& p);

// The grid of a frame that an operator declared normal. Valid only for the same w, h and cell.
struct Reference {
  int w = 0, h = 0, cell = 0;
  std::vector<uint32_t> sum_y;  // rows x cols
  uint64_t energy_total = 0;
};

struct Summary {
  uint64_t n = 0;             // w * h
  uint64_t mean_sum = 0;      // sum of sum_y; the mean luma is mean_sum / n
  int p5 = 0, p95 = 0;        // p(k): the smallest v with cum(v) * 100 >= k * n
  uint64_t energy_total = 0, pairs_total = 0;  // sharpness = energy_total / pairs_total
  bool has_reference = false;
  int cells = 0, shifted = 0;  // cells with |sum_y - ref_sum_y| > shift_level * pixels_in_cell
  bool dark = false, bright = false, flat = false, defocused = false, moved = false;
  bool tampered = false;      // the OR of the five
};
// hist[256], sum_y and energy (rows x cols each) -> what a client asks about. ref: null, or a
// reference, which is ignored (has_reference false) unless its w, h and cell are the picture's.
Summary summarize(const uint32_t* hist, const uint32_t* sum_y, const uint32_t* energy, int w, int h, const Params& p,
                  const Reference* ref);

// One evaluation on the host: src (h rows of src_pitch bytes) into hist[256] and the two planes
// (cells(h) x cells(w) each); every bin and every cell is written.
void stats_cpu(const uint8_t* src, int w, int h, size_t src_pitch, int cell, uint32_t* hist, uint32_t* sum_y,
               uint32_t* energy);

}  // namespace vep::tamper
