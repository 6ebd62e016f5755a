// Stand-alone check of the CPU scaler (vep/scale.cpp) for sanitizer builds (`make asan-scale`:
// AddressSanitizer + UndefinedBehaviorSanitizer on the host). Every picture lives in a heap
// buffer of exactly its size, so a read or write past a row or past the picture is a report.
// Shapes: identity, integer and non-integer ratios, one output sample, single-row and
// single-column sources, 1080p to a wall tile, and the two sizes around the 32-bit bound of the
// accumulator (all-255 pictures: the largest sums there are). Small shapes are compared with a
// per-unit integration (every unit of the sw * ow axis visited on its own); walls with pitches
// wider than their rows, empty tiles and bars. Exit status 0 and no sanitizer report = pass.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "vep/scale.h"

using namespace vep;

static int failures = 0;

static void check(bool ok, const char* what, int sw, int sh, int ow, int oh) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s (%dx%d -> %dx%d)\n", what, sw, sh, ow, oh);
  ++failures;
}

// out(j, k) by visiting every unit square of the (sw * ow) x (sh * oh) plane
static std::vector<uint8_t> brute(const uint8_t* src, int sw, int sh, int ow, int oh) {
  std::vector<uint8_t> out(size_t(ow) * oh * 3);
  const uint64_t den = uint64_t(sw) * sh;
  for (int k = 0; k < oh; ++k)
    for (int j = 0; j < ow; ++j)
      for (int c = 0; c < 3; ++c) {
        uint64_t sum = 0;
        for (int y = k * sh; y < (k + 1) * sh; ++y)
          for (int x = j * sw; x < (j + 1) * sw; ++x) sum += src[(size_t(y / oh) * sw + size_t(x / ow)) * 3 + c];
        // (a unit square weighs 1, so a source sample's squares add up to wy * wx)
        out[(size_t(k) * ow + j) * 3 + c] = uint8_t((sum + den / 2) / den);
      }
  return out;
}

static uint32_t seed = 12345;
static uint8_t rnd() {
  seed = seed * 1664525u + 1013904223u;
  return uint8_t(seed >> 24);
}

static void run(int sw, int sh, int ow, int oh, bool compare) {
  const size_t n = size_t(sw) * sh * 3, m = size_t(ow) * oh * 3;
  std::unique_ptr<uint8_t[]> src(new uint8_t[n]), dst(new uint8_t[m]);
  for (int kind = 0; kind < 3; ++kind) {
    for (size_t i = 0; i < n; ++i) src[i] = kind == 0 ? rnd() : kind == 1 ? 255 : uint8_t(((i / 3) % sw + (i / 3) / sw) & 1 ? 255 : 0);
    scale::area_cpu(src.get(), sw, sh, size_t(sw) * 3, dst.get(), size_t(ow) * 3, ow, oh);
    if (kind == 1) {
      bool white = true;
      for (size_t i = 0; i < m; ++i) white = white && dst[i] == 255;
      check(white, "all-255 stays 255", sw, sh, ow, oh);
    }
    if (ow == sw && oh == sh) {
      bool same = true;
      for (size_t i = 0; i < m; ++i) same = same && dst[i] == src[i];
      check(same, "identity", sw, sh, ow, oh);
    }
    if (compare) {
      const std::vector<uint8_t> want = brute(src.get(), sw, sh, ow, oh);
      bool same = true;
      for (size_t i = 0; i < m; ++i) same = same && dst[i] == want[i];
      check(same, "equals the per-unit integration", sw, sh, ow, oh);
    }
  }
  std::printf("area %5dx%-5d -> %4dx%-4d ok\n", sw, sh, ow, oh);
}

static void wall() {
  // five tiles of three sizes, one empty, in 3 x 2 cells of 31 x 18; the canvas has a pitch of
  // its own and is exactly rows * pitch bytes
  const int sizes[5][2] = {{64, 36}, {200, 120}, {0, 0}, {64, 48}, {64, 36}};
  std::vector<std::unique_ptr<uint8_t[]>> px;
  std::vector<scale::Tile> tiles(5);
  for (int t = 0; t < 5; ++t) {
    const int w = sizes[t][0], h = sizes[t][1];
    px.emplace_back(w ? new uint8_t[size_t(w) * h * 3] : nullptr);
    if (!w) continue;
    for (size_t i = 0; i < size_t(w) * h * 3; ++i) px.back()[i] = rnd();
    tiles[size_t(t)].src = px.back().get();
    tiles[size_t(t)].sw = w;
    tiles[size_t(t)].sh = h;
    tiles[size_t(t)].pitch = size_t(w) * 3;
  }
  const scale::Wall g = scale::wall(5, 0, 31, 18);
  check(g.cols == 3 && g.rows == 2 && g.w == 93 && g.h == 36, "wall geometry", 5, 0, 31, 18);
  const size_t pitch = size_t(g.w) * 3 + 5;
  std::unique_ptr<uint8_t[]> canvas(new uint8_t[pitch * g.h]);
  for (size_t i = 0; i < pitch * g.h; ++i) canvas[i] = 200;
  scale::compose_cpu(tiles.data(), 5, 0, 31, 18, canvas.get(), pitch);
  bool ok = true;
  for (int y = 0; y < g.h; ++y) {
    for (size_t x = size_t(g.w) * 3; x < pitch; ++x) ok = ok && canvas[y * pitch + x] == 200;  // padding untouched
    for (int x = 62 * 3; x < 93 * 3; ++x) ok = ok && canvas[y * pitch + x] == scale::kBackground;  // empty cells
  }
  const scale::Placement p = scale::place(3, 3, 31, 18, 64, 48);
  check(p.x == 3 && p.y == 18 && p.w == 24 && p.h == 18, "4:3 in a 16:9 cell", 64, 48, 31, 18);
  for (int y = 18; y < 36; ++y)
    for (int x = 0; x < 9; ++x) ok = ok && canvas[y * pitch + x] == scale::kBackground;  // the left bar
  check(ok, "bars, empty cells and padding", 5, 0, 31, 18);
  std::puts("wall 5 tiles ok");
}

int main() {
  const int small[][4] = {{7, 5, 7, 5},     {48, 32, 8, 8}, {64, 48, 1, 1}, {17, 9, 5, 4}, {33, 17, 32, 16},
                          {200, 120, 199, 119}, {1, 9, 1, 4},   {9, 1, 4, 1}};
  for (const auto& s : small) run(s[0], s[1], s[2], s[3], s[0] < 200);  // (200 x 120: 568 M unit squares)
  run(1920, 1080, 320, 180, false);
  run(4112, 4096, 8, 8, false);  // 255 * sw * sh = 2^32 - 65536 * 255 ...
  run(4113, 4096, 8, 8, false);  // ... and above 2^32
  wall();
  // fit: the cases the text names
  auto fits = [](int sw, int sh, int bw, int bh, int w, int h) {
    const scale::Size f = scale::fit(sw, sh, bw, bh);
    check(f.w == w && f.h == h, "fit", sw, sh, bw, bh);
  };
  fits(1920, 1080, 320, 180, 320, 180);
  fits(1920, 1080, 320, 65535, 320, 180);
  fits(1920, 1080, 65535, 180, 320, 180);
  fits(1920, 1080, 0, 0, 1920, 1080);
  fits(640, 480, 320, 180, 240, 180);
  fits(65535, 1, 100, 100, 100, 1);
  // bad arguments throw, they do not read or write out of bounds
  const int bad[][4] = {{4, 4, 5, 4}, {4, 4, 4, 5}, {4, 4, 0, 4}, {4, 4, 4, 0}, {0, 4, 1, 1}, {65536, 1, 1, 1}};
  for (const auto& b : bad) {
    try {
      uint8_t one[3] = {};
      scale::area_cpu(one, b[0], b[1], size_t(b[0] > 0 ? b[0] : 1) * 3, one, 3, b[2], b[3]);
      check(false, "bad size rejected", b[0], b[1], b[2], b[3]);
    } catch (const std::exception&) {
    }
  }
  if (failures) return 1;
  std::puts("scale_selftest ok");
  return 0;
}
