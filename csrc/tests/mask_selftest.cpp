// Stand-alone check of the CPU privacy masks (vep/mask.cpp) for sanitizer builds (`make asan-mask`:
// AddressSanitizer + UndefinedBehaviorSanitizer on the host). Every picture lives in a heap buffer
// of exactly its size, so a read or write past a row or the picture is a report. Shapes: the edge
// pictures (7x5, 17x9, 1x9, 9x1, 64x48, 300x260 at block 128, 9000x3), each with the whole picture,
// one pixel, rects at every x offset modulo 4, a rect smaller than a block, edges and corners, in
// both modes; each compared with a per-pixel restatement (which block a pixel lies in, that block's
// sum and count in 64 bits); once more with a pitch wider than the row, whose padding must stay
// untouched. Then the closed forms: outward rounding, idempotence, the uniform picture, the
// checkerboard's 128, list order and levels, and every invalid list. Exit status 0 and no
// sanitizer report = pass.
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <utility>
#include <vector>

#include "vep/common.h"
#include "vep/mask.h"

using namespace vep;

static int failures = 0;

static void check(bool ok, const char* what, int w = 0, int h = 0, int k = 0) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s (%dx%d case %d)\n", what, w, h, k);
  ++failures;
}

static uint32_t seed = 24680;
static uint8_t rnd() {
  seed = seed * 1664525u + 1013904223u;
  return uint8_t(seed >> 24);
}

// A mask whose pixel rect on a w x h picture is [x0, x1) x [y0, y1), where one exists.
static bool rect_mask(int w, int h, int x0, int y0, int x1, int y1, mask::Mask& m) {
  auto lo = [](int p, int n) { return int((int64_t(p) * 10000 + n - 1) / n); };
  auto hi = [](int p, int n) { return int(int64_t(p) * 10000 / n); };
  m.x0 = lo(x0, w), m.y0 = lo(y0, h), m.x1 = hi(x1, w), m.y1 = hi(y1, h);
  if (m.x0 >= m.x1 || m.y0 >= m.y1) return false;
  const mask::Rect r = mask::to_pixels(w, h, m);
  return r.x0 == x0 && r.y0 == y0 && r.x1 == x1 && r.y1 == y1;
}

// the text of docs/PRIVACY.md §1, pixel by pixel
static void restate(std::vector<uint8_t>& pic, size_t pitch, int w, int h, const mask::Mask& m) {
  const int px0 = int(int64_t(m.x0) * w / 10000), px1 = int((int64_t(m.x1) * w + 9999) / 10000);
  const int py0 = int(int64_t(m.y0) * h / 10000), py1 = int((int64_t(m.y1) * h + 9999) / 10000);
  const std::vector<uint8_t> in = pic;
  std::map<std::pair<int, int>, std::array<uint8_t, 3>> seen;  // a block's values, worked out at its first pixel
  for (int y = py0; y < py1; ++y)
    for (int x = px0; x < px1; ++x) {
      std::array<uint8_t, 3> v;
      if (m.mode == mask::kFill) {
        v = {uint8_t(m.b), uint8_t(m.g), uint8_t(m.r)};
      } else {
        const int bx = px0 + (x - px0) / m.block * m.block, by = py0 + (y - py0) / m.block * m.block;
        auto it = seen.find({bx, by});
        if (it == seen.end()) {
          for (int c = 0; c < 3; ++c) {
            uint64_t sum = 0, n = 0;
            for (int yy = by; yy < by + m.block && yy < py1; ++yy)
              for (int xx = bx; xx < bx + m.block && xx < px1; ++xx) sum += in[size_t(yy) * pitch + size_t(xx) * 3 + c], ++n;
            v[size_t(c)] = uint8_t((sum + n / 2) / n);
          }
          seen[{bx, by}] = v;
        } else {
          v = it->second;
        }
      }
      for (int c = 0; c < 3; ++c) pic[size_t(y) * pitch + size_t(x) * 3 + c] = v[size_t(c)];
    }
}

static void run_case(int w, int h, size_t pitch, const std::vector<mask::Mask>& ms, int k) {
  const size_t bytes = size_t(h - 1) * pitch + size_t(w) * 3;  // exactly the rows: the last one has no padding
  std::unique_ptr<uint8_t[]> buf(new uint8_t[bytes]);
  for (size_t i = 0; i < bytes; ++i) buf[i] = rnd();
  std::vector<uint8_t> want(buf.get(), buf.get() + bytes);
  for (const mask::Mask& m : ms) restate(want, pitch, w, h, m);
  mask::apply_cpu(buf.get(), pitch, w, h, ms.data(), int(ms.size()));
  check(std::memcmp(buf.get(), want.data(), bytes) == 0, "twin differs from the restatement", w, h, k);
}

static void shapes() {
  const int sizes[][3] = {{7, 5, 4}, {17, 9, 4}, {1, 9, 16}, {9, 1, 16}, {64, 48, 16}, {300, 260, 128}, {9000, 3, 128}, {9000, 3, 4}};
  for (const auto& s : sizes) {
    const int w = s[0], h = s[1], B = s[2];
    std::vector<std::vector<int>> rects = {{0, 0, w, h}, {w / 2, h / 2, w / 2 + 1, h / 2 + 1}, {w - 1, h - 1, w, h}, {0, 0, 1, 1},
                                           {2, 1, 5, 4}};
    for (int x0 : {1, 2, 3})
      for (int wd : {1, 2, 3, 4, 5, 21}) rects.push_back({x0, 1, x0 + wd, h < 7 ? h : 7});
    const int qx = w / 3 > 0 ? w / 3 : 1, qy = h / 3 > 0 ? h / 3 : 1;
    for (const auto& r : std::vector<std::vector<int>>{{0, qy, qx, h - qy}, {w - qx, qy, w, h - qy}, {qx, 0, w - qx, qy},
                                                       {qx, h - qy, w - qx, h}, {0, 0, qx, qy}, {w - qx, 0, w, qy},
                                                       {0, h - qy, qx, h}, {w - qx, h - qy, w, h}})
      rects.push_back(r);
    int k = 0;
    for (const auto& r : rects) {
      ++k;
      if (!(0 <= r[0] && r[0] < r[2] && r[2] <= w && 0 <= r[1] && r[1] < r[3] && r[3] <= h)) continue;
      mask::Mask m;
      if (!rect_mask(w, h, r[0], r[1], r[2], r[3], m)) continue;
      for (int mode : {int(mask::kFill), int(mask::kPixelate)}) {
        m.mode = mode;
        m.block = B;
        m.b = 3, m.g = 130, m.r = 255;
        run_case(w, h, size_t(w) * 3, {m}, k);
        run_case(w, h, size_t(w) * 3 + 5, {m}, k);  // a pitch wider than the row
      }
    }
  }
  // 1080p once, three masks of two levels
  mask::Mask a, b, c;
  b.x0 = 2000, b.y0 = 3000, b.x1 = 7001, b.y1 = 9999, b.block = 48;
  c.x0 = 6000, c.y0 = 0, c.x1 = 10000, c.y1 = 4000, c.mode = mask::kFill, c.g = 77;
  run_case(1920, 1080, 1920 * 3, {a, b, c}, 0);
}

static bool throws(const std::vector<mask::Mask>& ms) {
  try {
    mask::check_list(ms.data(), int(ms.size()));
  } catch (const Error&) {
    return true;
  }
  return false;
}

static void closed_forms() {
  mask::Mask m;
  m.x0 = 1, m.y0 = 1, m.x1 = 9999, m.y1 = 9999;
  mask::Rect r = mask::to_pixels(1920, 1080, m);
  check(r.x0 == 0 && r.y0 == 0 && r.x1 == 1920 && r.y1 == 1080, "outward rounding");
  m.x0 = 5000, m.x1 = 5001, m.y0 = 9999, m.y1 = 10000;
  r = mask::to_pixels(1920, 1080, m);
  check(r.x0 == 960 && r.x1 == 961 && r.y0 == 1079 && r.y1 == 1080, "a rect narrower than a pixel is one pixel");
  for (int w : {1, 2, 3, 7, 1920, 9999, 10001, 65535})
    for (int x0 : {0, 1, 3333, 9999})
      for (int x1 : {x0 + 1, 10000}) {
        mask::Mask q;
        q.x0 = x0, q.x1 = x1;
        r = mask::to_pixels(w, 5, q);
        check(0 <= r.x0 && r.x0 < r.x1 && r.x1 <= w, "rect empty or outside the picture", w, 5, x0);
        check(int64_t(r.x0) * 10000 <= int64_t(x0) * w && int64_t(r.x1) * 10000 >= int64_t(x1) * w, "rounding not outward", w, 5,
              x0);
      }
  // idempotence, the uniform picture, the checkerboard
  const int w = 61, h = 45;
  std::vector<uint8_t> p(size_t(w) * h * 3), once, twice;
  for (auto& v : p) v = rnd();
  mask::Mask pix;
  check(rect_mask(w, h, 3, 2, 58, 41, pix), "rect_mask");
  pix.block = 8;
  once = p;
  mask::apply_cpu(once.data(), size_t(w) * 3, w, h, &pix, 1);
  twice = once;
  mask::apply_cpu(twice.data(), size_t(w) * 3, w, h, &pix, 1);
  check(once == twice && once != p, "pixelate is idempotent");
  std::vector<uint8_t> u(size_t(w) * h * 3, 97), u2 = u;
  mask::apply_cpu(u2.data(), size_t(w) * 3, w, h, &pix, 1);
  check(u == u2, "a uniform picture is unchanged");
  std::vector<uint8_t> ck(size_t(64) * 48 * 3);
  for (int y = 0; y < 48; ++y)
    for (int x = 0; x < 64; ++x)
      for (int c = 0; c < 3; ++c) ck[(size_t(y) * 64 + x) * 3 + c] = ((x + y) & 1) ? 255 : 0;
  mask::Mask cm;
  check(rect_mask(64, 48, 8, 4, 56, 44, cm), "rect_mask");
  cm.block = 8;
  mask::apply_cpu(ck.data(), 64 * 3, 64, 48, &cm, 1);
  bool all128 = true;
  for (int y = 4; y < 44; ++y)
    for (int x = 8; x < 56; ++x)
      for (int c = 0; c < 3; ++c) all128 = all128 && ck[(size_t(y) * 64 + x) * 3 + c] == 128;
  check(all128 && ck[0] == 0 && ck[3] == 255, "the checkerboard gives 128 (127.5 rounds up)");
  // list order and levels
  mask::Mask f, q;
  check(rect_mask(80, 60, 10, 10, 50, 40, f) && rect_mask(80, 60, 30, 20, 70, 55, q), "rect_mask");
  f.mode = mask::kFill, f.b = 255;
  std::vector<uint8_t> a(size_t(80) * 60 * 3), b;
  for (auto& v : a) v = rnd();
  b = a;
  const mask::Mask fq[2] = {f, q}, qf[2] = {q, f};
  mask::apply_cpu(a.data(), 240, 80, 60, fq, 2);
  mask::apply_cpu(b.data(), 240, 80, 60, qf, 2);
  check(a != b, "the order of overlapping masks matters");
  int lv[mask::kMaxMasks];
  check(mask::levels(80, 60, fq, 2, lv) == 2 && lv[0] == 0 && lv[1] == 1, "levels of two overlapping masks");
  mask::Mask far;
  check(rect_mask(80, 60, 70, 55, 80, 60, far), "rect_mask");
  const mask::Mask three[3] = {f, far, q};
  check(mask::levels(80, 60, three, 3, lv) == 2 && lv[0] == 0 && lv[1] == 0 && lv[2] == 1, "touching rects are disjoint");
  check(mask::levels(80, 60, nullptr, 0, lv) == 0, "no masks, no levels");
  // invalid lists
  const mask::Mask good;
  check(!throws({good}) && !throws({}), "a valid list");
  check(throws(std::vector<mask::Mask>(9, good)), "9 masks");
  auto bad = [&](auto set) {
    mask::Mask x = good;
    set(x);
    return throws({x});
  };
  check(bad([](mask::Mask& x) { x.x0 = x.x1; }), "x0 >= x1");
  check(bad([](mask::Mask& x) { x.y0 = 10000; }), "y0 >= y1");
  check(bad([](mask::Mask& x) { x.x1 = 10001; }), "a coordinate above 10000");
  check(bad([](mask::Mask& x) { x.x0 = -1; }), "a negative coordinate");
  check(bad([](mask::Mask& x) { x.block = 3; }), "block 3");
  check(bad([](mask::Mask& x) { x.block = 129; }), "block 129");
  check(bad([](mask::Mask& x) { x.mode = 2; }), "an unknown mode");
  check(bad([](mask::Mask& x) { x.r = 256; }), "a colour above 255");
}

int main() {
  shapes();
  closed_forms();
  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("mask_selftest: ok\n");
  return 0;
}
