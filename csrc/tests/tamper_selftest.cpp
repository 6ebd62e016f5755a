// Stand-alone check of the CPU tamper detector (vep/tamper.cpp) for sanitizer builds
// (`make asan-tamper`: AddressSanitizer + UndefinedBehaviorSanitizer on the host). Every picture,
// plane and histogram lives in a heap buffer of exactly its size, so a read or write past a row,
// a plane or the 256 bins is a report. Shapes: one partial cell, partial right and bottom cells,
// an exact grid, cells of 12 and 20 pixels, single rows and columns, a cell wider than the picture;
// noise, and the closed forms (uniform grey, the 128 x 128 checkerboard at cell 128, stripes, an
// edge on a cell boundary), each compared with a per-pixel restatement that visits every pair of
// neighbours and asks whether both ends lie in one cell; once more with a pitch wider than the
// row. The summary runs on every result. Exit status 0 and no sanitizer report = pass.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "vep/tamper.h"

using namespace vep;

static int failures = 0;

static void check(bool ok, const char* what, int w, int h, int cell) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s (%dx%d cell %d)\n", what, w, h, cell);
  ++failures;
}

static uint32_t seed = 9753;
static uint8_t rnd() {
  seed = seed * 1664525u + 1013904223u;
  return uint8_t(seed >> 24);
}

static int64_t luma_at(const uint8_t* src, size_t pitch, int x, int y) {
  const uint8_t* p = src + size_t(y) * pitch + size_t(x) * 3;
  return (29 * int64_t(p[0]) + 150 * int64_t(p[1]) + 77 * int64_t(p[2]) + 128) / 256;
}

// the text of docs/TAMPER.md §1, pair by pair
static void restate(const uint8_t* src, size_t pitch, int w, int h, int cell, std::vector<uint64_t>& hist,
                    std::vector<uint64_t>& sum_y, std::vector<uint64_t>& energy) {
  const int cols = (w + cell - 1) / cell, rows = (h + cell - 1) / cell;
  hist.assign(256, 0);
  sum_y.assign(size_t(cols) * rows, 0);
  energy.assign(size_t(cols) * rows, 0);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const int64_t Y = luma_at(src, pitch, x, y);
      const size_t at = size_t(y / cell) * cols + x / cell;
      ++hist[size_t(Y)];
      sum_y[at] += uint64_t(Y);
      if (x + 1 < w && (x + 1) / cell == x / cell) {
        const int64_t d = luma_at(src, pitch, x + 1, y) - Y;
        energy[at] += uint64_t(d * d);
      }
      if (y + 1 < h && (y + 1) / cell == y / cell) {
        const int64_t d = luma_at(src, pitch, x, y + 1) - Y;
        energy[at] += uint64_t(d * d);
      }
    }
}

enum Kind { kNoise, kGrey, kChecker, kVStripes, kHStripes, kBoundaryEdge };

static uint8_t level(Kind kind, int x, int y, int cell) {
  switch (kind) {
    case kGrey: return 77;
    case kChecker: return uint8_t(((x + y) & 1) * 255);
    case kVStripes: return uint8_t((x & 1) * 255);
    case kHStripes: return uint8_t((y & 1) * 255);
    case kBoundaryEdge: return x < cell ? 10 : 240;
    default: return 0;
  }
}

// -> the energy summed over the grid
static uint64_t run(Kind kind, int w, int h, int cell, size_t extra_pitch = 0) {
  const size_t pitch = size_t(w) * 3 + extra_pitch;
  const size_t n = pitch * size_t(h - 1) + size_t(w) * 3;  // exactly: the last row has no padding
  const size_t cells = size_t(tamper::cells(uint32_t(w), uint32_t(cell))) * tamper::cells(uint32_t(h), uint32_t(cell));
  std::unique_ptr<uint8_t[]> src(new uint8_t[n]);
  for (size_t i = 0; i < n; ++i) src[i] = rnd();
  if (kind != kNoise)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) std::memset(src.get() + size_t(y) * pitch + size_t(x) * 3, level(kind, x, y, cell), 3);
  std::unique_ptr<uint32_t[]> hist(new uint32_t[256]), sum_y(new uint32_t[cells]), energy(new uint32_t[cells]);
  std::memset(hist.get(), 0xa5, 256 * sizeof(uint32_t));  // every bin and every cell must be written
  std::memset(sum_y.get(), 0xa5, cells * sizeof(uint32_t));
  std::memset(energy.get(), 0xa5, cells * sizeof(uint32_t));
  tamper::stats_cpu(src.get(), w, h, pitch, cell, hist.get(), sum_y.get(), energy.get());
  std::vector<uint64_t> wh, ws, we;
  restate(src.get(), pitch, w, h, cell, wh, ws, we);
  bool same = true;
  uint64_t total = 0, pixels = 0;
  for (size_t i = 0; i < 256; ++i) {
    same = same && hist[i] == wh[i];
    pixels += hist[i];
  }
  check(same, "histogram", w, h, cell);
  check(pixels == uint64_t(w) * uint64_t(h), "histogram total", w, h, cell);
  same = true;
  for (size_t i = 0; i < cells; ++i) {
    same = same && sum_y[i] == ws[i] && energy[i] == we[i];
    total += energy[i];
  }
  check(same, "grid planes", w, h, cell);
  tamper::Params p;
  p.cell = cell;
  tamper::Reference ref;
  ref.w = w;
  ref.h = h;
  ref.cell = cell;
  ref.sum_y.assign(sum_y.get(), sum_y.get() + cells);
  ref.energy_total = total;
  const tamper::Summary s = tamper::summarize(hist.get(), sum_y.get(), energy.get(), w, h, p, &ref);
  check(s.has_reference && s.shifted == 0 && !s.moved && !s.defocused && s.energy_total == total, "summary", w, h, cell);
  ref.w = w + 1;  // another size: the reference is ignored
  check(!tamper::summarize(hist.get(), sum_y.get(), energy.get(), w, h, p, &ref).has_reference, "dropped reference", w, h,
        cell);
  return total;
}

int main() {
  const int shapes[][3] = {{7, 5, 8},     {17, 9, 8},   {33, 17, 16}, {64, 48, 16}, {50, 30, 12}, {50, 30, 20},
                           {200, 120, 32}, {1, 9, 8},    {9, 1, 8},    {300, 3, 128}, {1, 1, 8},    {130, 129, 128}};
  for (const auto& s : shapes) {
    run(kNoise, s[0], s[1], s[2]);
    run(kNoise, s[0], s[1], s[2], 5);
    check(run(kGrey, s[0], s[1], s[2]) == 0, "uniform grey has no energy", s[0], s[1], s[2]);
    run(kChecker, s[0], s[1], s[2]);
  }
  check(run(kChecker, 128, 128, 128) == 2114092800ull, "the largest cell value", 128, 128, 128);
  check(run(kVStripes, 64, 48, 16) == uint64_t(15 * 4 * 48) * 65025, "vertical stripes: horizontal pairs only", 64, 48, 16);
  check(run(kHStripes, 64, 48, 16) == uint64_t(15 * 3 * 64) * 65025, "horizontal stripes: vertical pairs only", 64, 48, 16);
  check(run(kBoundaryEdge, 32, 16, 16) == 0, "an edge on the cell boundary", 32, 16, 16);
  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::puts("tamper_selftest ok");
  return 0;
}
