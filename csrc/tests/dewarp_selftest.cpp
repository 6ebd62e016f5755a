// Stand-alone check of the CPU views (vep/dewarp.cpp) for sanitizer builds (`make asan-dewarp`:
// AddressSanitizer + UndefinedBehaviorSanitizer on the host). Every picture, mesh and output lives
// in a heap buffer of exactly its size, so a read or write past a row, the picture, the mesh or the
// view is a report, and so is a signed overflow of the position arithmetic. Pictures 1x1, 17x9,
// 200x120 and 8192x2, once more with a pitch wider than a row; outputs 1x1, 15x16, 17x17, 65x33 and
// 4096x1; meshes: identity, a half-pixel shift, everything outside, INT32_MIN / INT32_MAX garbage
// and random words. Each result is compared with a per-pixel restatement in 64-bit arithmetic
// written from the text of dewarp.h; identity must return the picture. Exit status 0 and no
// sanitizer report = pass.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "vep/dewarp.h"

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

static int64_t clampi(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
static int64_t floor_shift(int64_t v, int n) { return v >= 0 ? v >> n : -((-v + (int64_t(1) << n) - 1) >> n); }

// One output byte from the text of dewarp.h, in 64 bits and with divisions spelled as floors.
static uint8_t restate(const uint8_t* src, size_t pitch, int w, int h, const int32_t* mesh, int ow, int j, int k, int ch,
                       const crop::Pad& pad) {
  const int mw = (ow + 7) / 8 + 1, m = j / 8, n = k / 8;
  const int64_t a = j % 8, b = k % 8;
  int64_t p[2];
  for (int c = 0; c < 2; ++c) {
    auto node = [&](int mm, int nn) {
      return clampi(mesh[(size_t(nn) * size_t(mw) + size_t(mm)) * 2 + size_t(c)], -8192 * 256, 2 * 8192 * 256 - 1);
    };
    const int64_t s = (8 - a) * (8 - b) * node(m, n) + a * (8 - b) * node(m + 1, n) + (8 - a) * b * node(m, n + 1) +
                      a * b * node(m + 1, n + 1);
    p[c] = floor_shift(s + 32, 6);
  }
  if (p[0] < -128 || p[0] >= int64_t(w) * 256 - 128 || p[1] < -128 || p[1] >= int64_t(h) * 256 - 128)
    return uint8_t(ch == 0 ? pad.b : (ch == 1 ? pad.g : pad.r));
  const int64_t ix = floor_shift(p[0], 8), iy = floor_shift(p[1], 8), fx = p[0] - ix * 256, fy = p[1] - iy * 256;
  const int64_t x0 = clampi(ix, 0, w - 1), x1 = clampi(ix + 1, 0, w - 1), y0 = clampi(iy, 0, h - 1), y1 = clampi(iy + 1, 0, h - 1);
  auto px = [&](int64_t y, int64_t x) { return int64_t(src[size_t(y) * pitch + size_t(x) * 3 + size_t(ch)]); };
  return uint8_t(((256 - fx) * (256 - fy) * px(y0, x0) + fx * (256 - fy) * px(y0, x1) + (256 - fx) * fy * px(y1, x0) +
                  fx * fy * px(y1, x1) + 32768) >> 16);
}

static void run(int w, int h, size_t pitch, int ow, int oh, int kind) {
  std::unique_ptr<uint8_t[]> src(new uint8_t[size_t(h - 1) * pitch + size_t(w) * 3]);
  for (size_t i = 0; i < size_t(h - 1) * pitch + size_t(w) * 3; ++i) src[i] = uint8_t(rnd());
  const int mw = dewarp::mesh_w(ow), mh = dewarp::mesh_h(oh);
  std::unique_ptr<int32_t[]> mesh(new int32_t[size_t(mw) * size_t(mh) * 2]);
  for (int n = 0; n < mh; ++n)
    for (int m = 0; m < mw; ++m) {
      int32_t* q = &mesh[(size_t(n) * size_t(mw) + size_t(m)) * 2];
      switch (kind) {
        case 0: q[0] = m * 8 * 256, q[1] = n * 8 * 256; break;
        case 1: q[0] = m * 8 * 256 - 128, q[1] = n * 8 * 256 + 128; break;
        case 2: q[0] = -100000, q[1] = n * 8 * 256; break;
        case 3: q[0] = (rnd() & 1) ? INT32_MIN : INT32_MAX, q[1] = (rnd() & 1) ? INT32_MAX : INT32_MIN; break;
        default: q[0] = int32_t(rnd() % uint32_t(w * 512)) - w * 128, q[1] = int32_t(rnd() % uint32_t(h * 512)) - h * 128;
      }
    }
  const crop::Pad pad{1, 2, 3};
  std::unique_ptr<uint8_t[]> out(new uint8_t[size_t(ow) * size_t(oh) * 3]);
  dewarp::apply_cpu(src.get(), pitch, w, h, mesh.get(), ow, oh, pad, out.get());
  for (int k = 0; k < oh; ++k)
    for (int j = 0; j < ow; ++j)
      for (int ch = 0; ch < 3; ++ch, ++compared)
        check(out[(size_t(k) * size_t(ow) + size_t(j)) * 3 + size_t(ch)] == restate(src.get(), pitch, w, h, mesh.get(), ow, j, k, ch, pad),
              "byte", w, ow, j, k);
  if (kind == 0 && ow == w && oh == h && pitch == size_t(w) * 3)
    check(std::memcmp(out.get(), src.get(), size_t(w) * size_t(h) * 3) == 0, "identity", w, h);
}

int main() {
  const int pics[][2] = {{1, 1}, {17, 9}, {200, 120}, {8192, 2}};
  const int outs[][2] = {{1, 1}, {7, 8}, {15, 16}, {17, 17}, {65, 33}, {4096, 1}, {17, 9}, {200, 120}};
  for (const auto& p : pics)
    for (const auto& o : outs)
      for (int kind = 0; kind < 5; ++kind) {
        run(p[0], p[1], size_t(p[0]) * 3, o[0], o[1], kind);
        run(p[0], p[1], size_t(p[0]) * 3 + 7, o[0], o[1], kind);
      }
  bool threw = false;
  try {
    uint8_t px[3] = {0, 0, 0};
    int32_t mesh[8] = {};
    dewarp::apply_cpu(px, 3, 8193, 1, mesh, 1, 1, crop::Pad{0, 0, 0}, px);
  } catch (const std::exception&) {
    threw = true;
  }
  check(threw, "a picture above 8192 is refused");
  std::printf("dewarp selftest: %ld bytes compared, %d failures\n", compared, failures);
  return failures ? 1 : 0;
}
