// Stand-alone check of the CPU contrast enhancement (vep/clahe.cpp) for sanitizer builds (`make
// asan-clahe`: AddressSanitizer + UndefinedBehaviorSanitizer on the host). Every picture lives in a
// heap buffer of exactly its size, so a read or write past a row or the picture is a report, and so
// is an overflow of the arithmetic. Pictures 1x1, 7x9, thin and not-thin last tiles on each axis, a
// side below half a tile, 700x300 and 65535x2, once more with a pitch wider than a row; tiles 32,
// 40, 128 and 256; the extreme clips and strengths; random, dark and one-colour content. The
// arithmetic itself is held to tests/clahe_oracle.py by tests/test_clahe.py; here the header's
// closed forms are asserted: in place equals out of place, the source is not written, strength 0
// is the identity, one colour moves within the derived bound, no clip gives the rounded
// distribution. Exit status 0 and no sanitizer report = pass.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "vep/clahe.h"

using namespace vep;

static int failures = 0;
static long compared = 0;

static void check(bool ok, const char* what, int a = 0, int b = 0, int c = 0, int d = 0) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s (%d %d %d %d)\n", what, a, b, c, d);
  ++failures;
}

static uint32_t seed = 4711;
static uint32_t rnd() {
  seed = seed * 1664525u + 1013904223u;
  return seed >> 8;
}

static void run(int w, int h, size_t pitch, const clahe::Params& p, int kind) {
  const size_t bytes = size_t(h - 1) * pitch + size_t(w) * 3;
  std::unique_ptr<uint8_t[]> src(new uint8_t[bytes]), orig(new uint8_t[bytes]), dst(new uint8_t[bytes]);
  for (size_t i = 0; i < bytes; ++i) src[i] = uint8_t(kind == 0 ? rnd() : (kind == 1 ? rnd() % 40 : 77));
  std::memcpy(orig.get(), src.get(), bytes);
  std::memset(dst.get(), 0, bytes);
  clahe::enhance_cpu(src.get(), pitch, dst.get(), pitch, w, h, p);
  check(std::memcmp(src.get(), orig.get(), bytes) == 0, "the source is not written", w, h);
  clahe::enhance_cpu(src.get(), pitch, src.get(), pitch, w, h, p);  // in place
  // The largest bound over the picture's groups (clahe.h): a flat picture moves within it.
  const uint32_t tile = uint32_t(p.tile), cols = clahe::cells(uint32_t(w), tile), rows = clahe::cells(uint32_t(h), tile);
  uint32_t bound = 0;
  for (uint32_t j = 0; j < rows; ++j)
    for (uint32_t i = 0; i < cols; ++i) {
      const uint32_t n = clahe::group_span(clahe::group_of(i, uint32_t(w), tile, cols), uint32_t(w), tile, cols) *
                         clahe::group_span(clahe::group_of(j, uint32_t(h), tile, rows), uint32_t(h), tile, rows);
      const uint32_t b = clahe::one_colour_bound(uint32_t(p.clip16), n);
      bound = b > bound ? b : bound;
    }
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w * 3; ++x, ++compared) {
      const size_t at = size_t(y) * pitch + size_t(x);
      check(src[at] == dst[at], "in place equals out of place", w, h, x, y);
      if (p.strength == 0) check(dst[at] == orig[at], "strength 0 is the identity", w, h, x, y);
      if (kind == 2) {
        const int moved = int(dst[at]) - int(orig[at]);
        check(moved <= int(bound) && -moved <= int(bound), "one colour moves within the bound", w, h, moved, int(bound));
      }
    }
}

int main() {
  const int pics[][2] = {{1, 1}, {7, 9}, {100, 70}, {112, 80}, {10, 100}, {200, 9}, {300, 150}, {700, 300}, {65535, 2}};
  const clahe::Params params[] = {{32, 32, 256}, {40, 16, 128}, {128, 32, 256}, {256, 4096, 256}, {32, 4096, 0}, {64, 16, 1}};
  for (const auto& s : pics)
    for (const clahe::Params& p : params)
      for (int kind = 0; kind < 3; ++kind) {
        run(s[0], s[1], size_t(s[0]) * 3, p, kind);
        run(s[0], s[1], size_t(s[0]) * 3 + 7, p, kind);
      }
  // clip16 4096 never clips: the LUT is the rounded cumulative distribution
  uint32_t hist[256] = {};
  uint32_t n = 0;
  for (uint32_t& b : hist) n += b = rnd() % 300;
  uint8_t lut[256];
  clahe::lut_of_group(hist, n, 4096, 256, lut);
  uint64_t c = 0;
  for (int v = 0; v < 256; ++v) {
    c += hist[v];
    check(lut[v] == (c * 255 + n / 2) / n, "no clip: the rounded distribution", v);
  }
  check(lut[255] == 255, "lut[255] is 255");
  int refused = 0;
  const clahe::Params bad[] = {{24, 32, 256}, {36, 32, 256}, {264, 32, 256}, {32, 15, 256}, {32, 4097, 256}, {32, 32, 257}, {32, 32, -1}};
  for (const clahe::Params& p : bad) {
    try {
      clahe::check_params(p);
    } catch (const std::exception&) {
      ++refused;
    }
  }
  try {
    clahe::lut_of_group(hist, n + 1, 32, 256, lut);  // n is not the histogram's sum
  } catch (const std::exception&) {
    ++refused;
  }
  check(refused == 8, "bad parameters and a histogram that does not sum to n are refused", refused);
  std::printf("clahe selftest: %ld bytes compared, %d failures\n", compared, failures);
  return failures ? 1 : 0;
}
