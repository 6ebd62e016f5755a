// Per-camera motion detection: one definition of the arithmetic, shared by the CPU implementation
// (motion.cpp) and the gfx950 kernel (gpu_motion.hip), so both produce the same bytes.
// docs/MOTION.md has the reasoning. Integers only.
//
// For a packed BGR24 picture of w x h (1 <= w, h <= 65535):
//   luma        Y = (29 * B + 150 * G + 77 * R + 128) >> 8      (the weights sum to 256: 0..255,
//                                                                a grey pixel v, v, v has Y == v)
//   background  one u16 per pixel in 8.8 fixed point, 0..65280; ref = (bg + 128) >> 8
//   changed     |Y - ref| > threshold, with ref from the background BEFORE the update
//   update      bg' = bg + (((Y << 8) - bg) >> learn_shift), the difference signed and the shift
//               arithmetic (a floor division): bg' lies between bg and Y << 8, so it stays in
//               0..65280. learn_shift 0 makes the background the previous evaluated frame.
//   priming     without a background: bg' = Y << 8 and nothing counts as changed
//   grid        cells of cell x cell pixels, cols = ceil(w / cell), rows = ceil(h / cell), the
//               right and bottom cells partial; counts[gy * cols + gx] = changed pixels of the cell
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VEP_MOTION_HD __host__ __device__
#else
#define VEP_MOTION_HD
#endif

namespace vep::motion {

constexpr int kMaxSide = 65535;
constexpr int kMinCell = 4, kMaxCell = 256;
constexpr int kMaxThreshold = 255;
constexpr int kMaxLearnShift = 8;

VEP_MOTION_HD inline uint32_t luma(uint32_t b, uint32_t g, uint32_t r) {
  return (29u * b + 150u * g + 77u * r + 128u) >> 8;
}
VEP_MOTION_HD inline uint32_t prime(uint32_t y) { return y << 8; }
VEP_MOTION_HD inline uint32_t ref_of(uint32_t bg) { return (bg + 128u) >> 8; }
VEP_MOTION_HD inline bool changed(uint32_t y, uint32_t ref, uint32_t threshold) {
  const int32_t d = int32_t(y) - int32_t(ref);
  return uint32_t(d < 0 ? -d : d) > threshold;
}
VEP_MOTION_HD inline uint32_t update(uint32_t bg, uint32_t y, uint32_t learn_shift) {
  const int32_t d = int32_t(y << 8) - int32_t(bg);
  return uint32_t(int32_t(bg) + (d >> learn_shift));  // (arithmetic shift: floor)
}

// cells along a side of n pixels
VEP_MOTION_HD inline uint32_t cells(uint32_t n, uint32_t cell) { return (n + cell - 1) / cell; }
// samples per row of a background plane: rows start 16-byte aligned
VEP_MOTION_HD inline uint32_t pitch_for(uint32_t w) { return (w + 7u) & ~7u; }

struct Params {
  int cell = 16, threshold = 24, learn_shift = 4;  // the update
  int cell_percent = 25, min_cells = 1;            // the summary
};
// Throws unless every parameter is in its range: cell 4..256, threshold 0..255, learn_shift 0..8,
// cell_percent 1..100, min_cells >= 1.
void check_update_params(int cell, int threshold, int learn_shift);
void check_params(const Params& p);

// counts -> what a client asks about.
struct Summary {
  uint64_t changed = 0;  // sum of the counts
  int active = 0;        // cells with count * 100 >= pixels_in_cell * cell_percent (true size of a partial cell)
  bool has_box = false;  // the pixel rectangle bounding the active cells, clipped to the picture
  int x = 0, y = 0, w = 0, h = 0;
  bool motion = false;   // active >= min_cells
};
Summary summarize(const uint32_t* counts, int w, int h, int cell, int cell_percent, int min_cells);

// One evaluation on the host: src (h rows of src_pitch bytes) against bg_in (null: prime) into
// bg_out (both h rows of bg_pitch_samples u16; padding samples are not written) and counts
// (cells(h) x cells(w), every cell written). bg_in == bg_out is not allowed.
void update_cpu(const uint8_t* src, int w, int h, size_t src_pitch, const uint16_t* bg_in, uint16_t* bg_out,
                size_t bg_pitch_samples, int cell, int threshold, int learn_shift, uint32_t* counts);

}  // namespace vep::motion
