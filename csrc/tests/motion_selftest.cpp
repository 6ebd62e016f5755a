// Stand-alone check of the CPU motion detector (vep/motion.cpp) for sanitizer builds
// (`make asan-motion`: AddressSanitizer + UndefinedBehaviorSanitizer on the host). Every picture,
// background and grid lives in a heap buffer of exactly its size, so a read or write past a row,
// a plane or the grid is a report. Shapes: one partial cell, partial right and bottom cells, an
// exact grid, single rows and columns, a cell wider than the picture. Each is primed and then
// evaluated at shifts 0, 4 and 8 and compared with a per-pixel restatement (a division that
// floors by hand instead of a shift, the cell found per pixel); once more with a background pitch
// wider than the row, whose padding must keep its sentinel. Exit status 0 and no sanitizer
// report = pass.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "vep/motion.h"

using namespace vep;

static int failures = 0;

static void check(bool ok, const char* what, int w, int h, int cell, int shift) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s (%dx%d cell %d shift %d)\n", what, w, h, cell, shift);
  ++failures;
}

static uint32_t seed = 4321;
static uint8_t rnd() {
  seed = seed * 1664525u + 1013904223u;
  return uint8_t(seed >> 24);
}

static int64_t floor_div(int64_t a, int64_t b) {  // b > 0
  int64_t q = a / b;
  if (a % b != 0 && a < 0) --q;
  return q;
}

// the text of docs/MOTION.md §1, pixel by pixel
static void restate(const uint8_t* src, int w, int h, const uint16_t* bg, int cell, int threshold, int shift,
                    std::vector<uint32_t>& counts, std::vector<uint16_t>& out) {
  const int cols = (w + cell - 1) / cell, rows = (h + cell - 1) / cell;
  counts.assign(size_t(cols) * rows, 0);
  out.assign(size_t(w) * h, 0);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const uint8_t* p = src + (size_t(y) * w + x) * 3;
      const int64_t Y = (29 * int64_t(p[0]) + 150 * int64_t(p[1]) + 77 * int64_t(p[2]) + 128) / 256;
      if (!bg) {
        out[size_t(y) * w + x] = uint16_t(Y * 256);
        continue;
      }
      const int64_t b = bg[size_t(y) * w + x], ref = (b + 128) / 256;
      const int64_t diff = Y > ref ? Y - ref : ref - Y;
      if (diff > threshold) ++counts[size_t(y / cell) * cols + x / cell];
      out[size_t(y) * w + x] = uint16_t(b + floor_div(Y * 256 - b, int64_t(1) << shift));
    }
}

static void run(int w, int h, int cell) {
  const size_t n = size_t(w) * h * 3, m = size_t(w) * h;
  const size_t cells = size_t(motion::cells(uint32_t(w), uint32_t(cell))) * motion::cells(uint32_t(h), uint32_t(cell));
  std::unique_ptr<uint8_t[]> a(new uint8_t[n]), b(new uint8_t[n]);
  for (size_t i = 0; i < n; ++i) {
    a[i] = rnd();
    b[i] = rnd();
  }
  std::unique_ptr<uint16_t[]> bg0(new uint16_t[m]), bg1(new uint16_t[m]);
  std::unique_ptr<uint32_t[]> counts(new uint32_t[cells]);
  std::vector<uint32_t> wc;
  std::vector<uint16_t> w0, w1;
  for (size_t i = 0; i < cells; ++i) counts[i] = 77;
  motion::update_cpu(a.get(), w, h, size_t(w) * 3, nullptr, bg0.get(), size_t(w), cell, 24, 4, counts.get());
  restate(a.get(), w, h, nullptr, cell, 24, 4, wc, w0);
  bool ok = true;
  for (size_t i = 0; i < cells; ++i) ok = ok && counts[i] == 0;
  for (size_t i = 0; i < m; ++i) ok = ok && bg0[i] == w0[i];
  check(ok, "priming", w, h, cell, 4);
  const int shifts[] = {0, 4, 8};
  for (int shift : shifts) {
    motion::update_cpu(b.get(), w, h, size_t(w) * 3, bg0.get(), bg1.get(), size_t(w), cell, 24, shift, counts.get());
    restate(b.get(), w, h, w0.data(), cell, 24, shift, wc, w1);
    ok = true;
    for (size_t i = 0; i < cells; ++i) ok = ok && counts[i] == wc[i];
    check(ok, "counts equal the per-pixel restatement", w, h, cell, shift);
    ok = true;
    for (size_t i = 0; i < m; ++i) ok = ok && bg1[i] == w1[i] && bg1[i] <= 65280;
    check(ok, "background equals the per-pixel restatement", w, h, cell, shift);
  }
  // padded planes: pitch_for(w) + 8 samples a row, in buffers of exactly h rows
  const size_t pitch = size_t(motion::pitch_for(uint32_t(w))) + 8;
  std::unique_ptr<uint16_t[]> p0(new uint16_t[pitch * h]), p1(new uint16_t[pitch * h]);
  for (size_t i = 0; i < pitch * h; ++i) p0[i] = p1[i] = 0xABCD;
  motion::update_cpu(a.get(), w, h, size_t(w) * 3, nullptr, p0.get(), pitch, cell, 24, 4, counts.get());
  motion::update_cpu(b.get(), w, h, size_t(w) * 3, p0.get(), p1.get(), pitch, cell, 24, 8, counts.get());
  ok = true;
  for (int y = 0; y < h; ++y) {
    for (int x = 0; x < w; ++x) ok = ok && p0[y * pitch + x] == w0[size_t(y) * w + x] && p1[y * pitch + x] == w1[size_t(y) * w + x];
    for (size_t x = size_t(w); x < pitch; ++x) ok = ok && p0[y * pitch + x] == 0xABCD && p1[y * pitch + x] == 0xABCD;
  }
  for (size_t i = 0; i < cells; ++i) ok = ok && counts[i] == wc[i];
  check(ok, "padded pitch: same samples, padding untouched", w, h, cell, 8);
  std::printf("motion %5dx%-5d cell %3d ok\n", w, h, cell);
}

static void edges() {
  // the threshold is exclusive, 255 never fires, shift 0 is frame differencing
  const int w = 9, h = 5, cell = 4;
  const size_t m = size_t(w) * h, cells = 3 * 2;
  auto grey = [&](uint8_t v) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[m * 3]);
    for (size_t i = 0; i < m * 3; ++i) p[i] = v;
    return p;
  };
  std::unique_ptr<uint16_t[]> bg0(new uint16_t[m]), bg1(new uint16_t[m]);
  std::unique_ptr<uint32_t[]> counts(new uint32_t[cells]);
  auto total = [&] {
    uint64_t s = 0;
    for (size_t i = 0; i < cells; ++i) s += counts[i];
    return s;
  };
  const int ts[] = {0, 24, 254};
  for (int t : ts) {
    const int base = t == 254 ? 0 : 100;
    motion::update_cpu(grey(uint8_t(base)).get(), w, h, size_t(w) * 3, nullptr, bg0.get(), size_t(w), cell, t, 0, counts.get());
    motion::update_cpu(grey(uint8_t(base + t)).get(), w, h, size_t(w) * 3, bg0.get(), bg1.get(), size_t(w), cell, t, 0, counts.get());
    check(total() == 0, "a difference of exactly the threshold is no change", w, h, cell, t);
    motion::update_cpu(grey(uint8_t(base + t + 1)).get(), w, h, size_t(w) * 3, bg0.get(), bg1.get(), size_t(w), cell, t, 0, counts.get());
    check(total() == m && bg1[0] == uint16_t((base + t + 1) << 8), "one above the threshold changes every pixel", w, h, cell, t);
  }
  motion::update_cpu(grey(0).get(), w, h, size_t(w) * 3, nullptr, bg0.get(), size_t(w), cell, 255, 0, counts.get());
  motion::update_cpu(grey(255).get(), w, h, size_t(w) * 3, bg0.get(), bg1.get(), size_t(w), cell, 255, 0, counts.get());
  check(total() == 0 && bg1[m - 1] == 65280, "threshold 255 never fires", w, h, cell, 255);
  // the summary of a grid with a partial corner cell
  uint32_t grid[6] = {0, 0, 0, 0, 0, 1};  // the corner cell is 1 x 1 pixel: one changed pixel is 100 %
  const motion::Summary s = motion::summarize(grid, w, h, cell, 100, 1);
  check(s.changed == 1 && s.active == 1 && s.has_box && s.x == 8 && s.y == 4 && s.w == 1 && s.h == 1 && s.motion,
        "summary of a partial cell", w, h, cell, 0);
  std::puts("motion edges ok");
}

int main() {
  const int shapes[][3] = {{7, 5, 8}, {17, 9, 8}, {33, 17, 16}, {64, 48, 16}, {200, 120, 32}, {1, 9, 4}, {9, 1, 4}, {300, 3, 256}};
  for (const auto& s : shapes) run(s[0], s[1], s[2]);
  edges();
  // bad arguments throw, they do not read or write out of bounds
  const int bad[][5] = {{0, 4, 8, 24, 4}, {4, 65536, 8, 24, 4}, {4, 4, 3, 24, 4}, {4, 4, 257, 24, 4},
                        {4, 4, 8, -1, 4}, {4, 4, 8, 256, 4}, {4, 4, 8, 24, -1}, {4, 4, 8, 24, 9}};
  for (const auto& b : bad) {
    try {
      uint8_t px[48] = {};
      uint16_t bg[16] = {};
      uint32_t c[1] = {};
      motion::update_cpu(px, b[0], b[1], 12, nullptr, bg, 4, b[2], b[3], b[4], c);
      check(false, "bad argument rejected", b[0], b[1], b[2], b[4]);
    } catch (const std::exception&) {
    }
  }
  try {
    uint8_t px[48] = {};
    uint16_t bg[16] = {};
    uint32_t c[1] = {};
    motion::update_cpu(px, 4, 4, 12, bg, bg, 4, 8, 24, 4, c);
    check(false, "in-place update rejected", 4, 4, 8, 4);
  } catch (const std::exception&) {
  }
  if (failures) return 1;
  std::puts("motion_selftest ok");
  return 0;
}
