// Stand-alone check of the CPU crops (vep/crop.cpp) for sanitizer builds (`make asan-crop`:
// AddressSanitizer + UndefinedBehaviorSanitizer on the host). Every picture and every output lives
// in a heap buffer of exactly its size, so a read or write past a row, past the picture or past a
// crop's own output is a report. Shapes: the pictures 7x5, 17x9, 1x9, 9x1, 64x48 and 200x120; the
// whole picture, one pixel, rects that start at x = 1, 2, 3, 5 with widths 1..8, 21 and 37, every
// edge and corner; outputs 1x1, 3x3, 7x5, 16x16, 112x112, 224x224, the rect's size +- 1 on each
// axis and 4096x1; both fits and two pad colours; all once more with a pitch wider than a row.
// Each result is compared with a per-pixel restatement (dense weight rows written from the text
// of crop.h, not from its Taps). Then the closed forms and the 64-bit accumulator on a 9000x3
// picture. Exit status 0 and no sanitizer report = pass.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <exception>
#include <memory>
#include <vector>

#include "vep/crop.h"

using namespace vep;

static int failures = 0;
static long compared = 0;

static void check(bool ok, const char* what, int a = 0, int b = 0, int c = 0, int d = 0) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s (%d %d %d %d)\n", what, a, b, c, d);
  ++failures;
}

static uint32_t seed = 4711;
static uint8_t rnd() {
  seed = seed * 1664525u + 1013904223u;
  return uint8_t(seed >> 24);
}

// The weights of output j over the s source samples, and the denominator: the text of crop.h.
static std::vector<int64_t> weights(int j, int s, int o, int64_t& den) {
  std::vector<int64_t> w(size_t(s), 0);
  if (o <= s) {
    den = s;
    for (int i = 0; i < s; ++i) {
      const int64_t a = std::max<int64_t>(int64_t(i) * o, int64_t(j) * s);
      const int64_t b = std::min<int64_t>(int64_t(i + 1) * o, int64_t(j + 1) * s);
      if (b > a) w[size_t(i)] = b - a;
    }
    return w;
  }
  den = 2 * int64_t(o);
  const int64_t t = int64_t(2 * j + 1) * s - o;
  if (t <= 0) {
    w[0] = den;
    return w;
  }
  const int64_t i0 = t / den, f = t % den;
  if (i0 >= s - 1) {
    w[size_t(s - 1)] = den;
    return w;
  }
  w[size_t(i0)] = den - f;
  w[size_t(i0 + 1)] = f;
  return w;
}

// The box whose pixel rect in a w x h picture is [a, b) x [c, d) (w, h <= 5000).
static crop::Box box_of(int w, int h, int a, int c, int b, int d) {
  crop::Box x;
  x.x0 = (a * crop::kUnit + w - 1) / w;
  x.x1 = b * crop::kUnit / w;
  x.y0 = (c * crop::kUnit + h - 1) / h;
  x.y1 = d * crop::kUnit / h;
  const mask::Rect r = crop::to_pixels(w, h, x);
  check(r.x0 == a && r.x1 == b && r.y0 == c && r.y1 == d, "box_of gives the rect", a, c, b, d);
  return x;
}

struct Picture {
  int w, h;
  size_t pitch;
  std::unique_ptr<uint8_t[]> px;  // exactly (h - 1) * pitch + w * 3 bytes
  const uint8_t* at(int x, int y) const { return px.get() + size_t(y) * pitch + size_t(x) * 3; }
};
static Picture picture(int w, int h, size_t extra, int kind) {
  Picture p{w, h, size_t(w) * 3 + extra, nullptr};
  const size_t n = size_t(h - 1) * p.pitch + size_t(w) * 3;
  p.px.reset(new uint8_t[n]);
  for (size_t i = 0; i < n; ++i) p.px[i] = kind == 0 ? rnd() : uint8_t(kind);
  return p;
}

// One box into a buffer of exactly ow * oh * 3 bytes, compared with the restatement when cheap.
static void one(const Picture& p, const crop::Box& b, int ow, int oh, int fit, const crop::Pad& pad) {
  const size_t m = size_t(ow) * oh * 3;
  std::unique_ptr<uint8_t[]> out(new uint8_t[m]);
  crop::apply_cpu(p.px.get(), p.pitch, p.w, p.h, &b, 1, out.get(), ow, oh, fit, pad);
  const mask::Rect r = crop::to_pixels(p.w, p.h, b);
  const int sw = r.x1 - r.x0, sh = r.y1 - r.y0;
  int fx = 0, fy = 0, fw = ow, fh = oh;
  if (fit == crop::kLetterbox) {  // the text of crop.h
    if (int64_t(sw) * oh >= int64_t(sh) * ow) {
      fh = int(std::min<int64_t>(oh, std::max<int64_t>(1, (2 * int64_t(sh) * ow + sw) / (2 * sw))));
    } else {
      fw = int(std::min<int64_t>(ow, std::max<int64_t>(1, (2 * int64_t(sw) * oh + sh) / (2 * sh))));
    }
    fx = (ow - fw) / 2;
    fy = (oh - fh) / 2;
  }
  if (int64_t(sw) * sh * fw * fh > 40000000) return;  // (memory safety only)
  std::vector<std::vector<int64_t>> wx, wy;
  int64_t dx = 0, dy = 0;
  for (int j = 0; j < fw; ++j) wx.push_back(weights(j, sw, fw, dx));
  for (int k = 0; k < fh; ++k) wy.push_back(weights(k, sh, fh, dy));
  const int padc[3] = {pad.b, pad.g, pad.r};
  bool same = true;
  for (int y = 0; y < oh; ++y)
    for (int x = 0; x < ow; ++x)
      for (int c = 0; c < 3; ++c) {
        int64_t want = padc[c];
        if (x >= fx && x < fx + fw && y >= fy && y < fy + fh) {
          int64_t sum = 0;
          for (int rr = 0; rr < sh; ++rr) {
            const int64_t a = wy[size_t(y - fy)][size_t(rr)];
            if (!a) continue;
            for (int i = 0; i < sw; ++i) sum += a * wx[size_t(x - fx)][size_t(i)] * p.at(r.x0 + i, r.y0 + rr)[c];
          }
          want = (sum + dx * dy / 2) / (dx * dy);
        }
        same = same && out[(size_t(y) * ow + x) * 3 + c] == want;
      }
  check(same, "equals the per-pixel restatement", sw, sh, ow, oh);
  ++compared;
}

static void shapes(size_t extra) {
  const int pics[][2] = {{7, 5}, {17, 9}, {1, 9}, {9, 1}, {64, 48}, {200, 120}};
  const crop::Pad grey, odd{1, 2, 250};
  for (const auto& s : pics) {
    const int w = s[0], h = s[1];
    const Picture p = picture(w, h, extra, 0);
    std::vector<crop::Box> boxes;
    boxes.push_back(crop::Box{});  // the whole picture
    boxes.push_back(box_of(w, h, w / 2, h / 2, w / 2 + 1, h / 2 + 1));  // one pixel
    for (int x0 : {1, 2, 3, 5})
      for (int bw : {1, 2, 3, 4, 5, 6, 7, 8, 21, 37})
        if (x0 + bw <= w) boxes.push_back(box_of(w, h, x0, h > 2 ? 1 : 0, x0 + bw, h > 2 ? h - 1 : h));
    // edges and corners
    const int ew = std::max(1, w / 3), eh = std::max(1, h / 3);
    for (int cx : {0, w - ew})
      for (int cy : {0, h - eh}) boxes.push_back(box_of(w, h, cx, cy, cx + ew, cy + eh));
    boxes.push_back(box_of(w, h, 0, 0, w, eh));
    boxes.push_back(box_of(w, h, 0, h - eh, w, h));
    boxes.push_back(box_of(w, h, 0, 0, ew, h));
    boxes.push_back(box_of(w, h, w - ew, 0, w, h));
    for (size_t bi = 0; bi < boxes.size(); ++bi) {
      const mask::Rect r = crop::to_pixels(w, h, boxes[bi]);
      const int sw = r.x1 - r.x0, sh = r.y1 - r.y0;
      std::vector<std::pair<int, int>> outs = {{1, 1}, {3, 3}, {7, 5}, {16, 16}, {sw + 1, sh}, {sw, sh + 1},
                                               {sw + 1, sh + 1}, {sw, sh}};
      if (sw > 1) outs.push_back({sw - 1, sh});
      if (sh > 1) outs.push_back({sw, sh - 1});
      if (bi < 2 || bi % 7 == 0) {
        outs.push_back({112, 112});
        outs.push_back({224, 224});
      }
      for (const auto& o : outs) {
        one(p, boxes[bi], o.first, o.second, crop::kStretch, grey);
        one(p, boxes[bi], o.first, o.second, crop::kLetterbox, bi & 1 ? odd : grey);
      }
    }
    one(p, boxes[1], 4096, 1, crop::kStretch, grey);
    std::printf("crops of %3dx%-3d pitch +%zu ok (%zu boxes)\n", w, h, extra, boxes.size());
  }
}

static std::vector<uint8_t> crop_of(const std::vector<uint8_t>& src, int w, int h, const crop::Box& b, int ow, int oh,
                                    int fit = crop::kStretch) {
  std::unique_ptr<uint8_t[]> in(new uint8_t[src.size()]);
  std::copy(src.begin(), src.end(), in.get());
  std::unique_ptr<uint8_t[]> out(new uint8_t[size_t(ow) * oh * 3]);
  crop::apply_cpu(in.get(), size_t(w) * 3, w, h, &b, 1, out.get(), ow, oh, fit, crop::Pad{});
  return std::vector<uint8_t>(out.get(), out.get() + size_t(ow) * oh * 3);
}

static void closed_forms() {
  // identity: the bytes come back
  std::vector<uint8_t> p(size_t(64) * 48 * 3);
  for (auto& v : p) v = rnd();
  check(crop_of(p, 64, 48, crop::Box{}, 64, 48) == p, "identity");
  // a uniform picture stays uniform at any size
  std::vector<uint8_t> u(size_t(17) * 9 * 3, 201);
  for (const auto& o : {std::pair<int, int>{1, 1}, {5, 30}, {224, 224}, {16, 9}, {18, 8}}) {
    const std::vector<uint8_t> got = crop_of(u, 17, 9, crop::Box{}, o.first, o.second);
    check(std::all_of(got.begin(), got.end(), [](uint8_t v) { return v == 201; }), "uniform stays uniform", o.first,
          o.second);
  }
  // [0, 255] enlarged to 4: the weights 8 0 | 6 2 | 2 6 | 0 8 of 8
  const std::vector<uint8_t> two = {0, 0, 0, 255, 255, 255};
  const std::vector<uint8_t> four = crop_of(two, 2, 1, crop::Box{}, 4, 1);
  const uint8_t want4[4] = {0, 64, 191, 255};
  for (int j = 0; j < 4; ++j) check(four[size_t(j) * 3] == want4[j] && four[size_t(j) * 3 + 2] == want4[j], "[0, 255] -> 4", j);
  // an integer-ratio reduce is the round-half-up block mean
  std::vector<uint8_t> q(size_t(12) * 8 * 3);
  for (auto& v : q) v = rnd();
  const std::vector<uint8_t> r = crop_of(q, 12, 8, crop::Box{}, 4, 2);
  bool mean = true;
  for (int k = 0; k < 2; ++k)
    for (int j = 0; j < 4; ++j)
      for (int c = 0; c < 3; ++c) {
        uint32_t s = 0;
        for (int y = 0; y < 4; ++y)
          for (int x = 0; x < 3; ++x) s += q[(size_t(k * 4 + y) * 12 + size_t(j * 3 + x)) * 3 + c];
        mean = mean && r[(size_t(k) * 4 + j) * 3 + c] == (s + 6) / 12;
      }
  check(mean, "integer ratio = block mean");
  // one pixel enlarged to 4096 x 1 is constant
  const std::vector<uint8_t> px = {7, 99, 250};
  const std::vector<uint8_t> line = crop_of(px, 1, 1, crop::Box{}, 4096, 1);
  bool flat = true;
  for (size_t j = 0; j < 4096; ++j) flat = flat && line[j * 3] == 7 && line[j * 3 + 1] == 99 && line[j * 3 + 2] == 250;
  check(flat, "one pixel -> 4096 x 1");
  // letterbox: 2:1 in a square, bars of the pad colour above and below
  const crop::Placement f = crop::fitted(100, 50, 64, 64, crop::kLetterbox);
  check(f.x == 0 && f.y == 16 && f.w == 64 && f.h == 32, "letterbox placement", f.x, f.y, f.w, f.h);
  const crop::Placement g = crop::fitted(1, 4096, 4096, 1, crop::kLetterbox);
  check(g.w == 1 && g.h == 1 && g.x == 2047 && g.y == 0, "letterbox never empty", g.x, g.y, g.w, g.h);
  // the taps' extremes: weights sum to D, indices inside the source
  const int ends[][2] = {{1, 4096}, {65535, 1}, {65535, 4096}, {4095, 4096}, {4096, 4095}};
  for (const auto& e : ends) {
    bool ok = true;
    for (int j = 0; j < e[1]; ++j) {
      const crop::Taps t = crop::taps(uint32_t(j), uint32_t(e[0]), uint32_t(e[1]));
      uint64_t sum = 0;
      for (uint32_t i = t.lo; i <= t.hi; ++i) sum += crop::weight_of(t, i);
      ok = ok && t.lo <= t.hi && t.hi < uint32_t(e[0]) && sum == crop::den(uint32_t(e[0]), uint32_t(e[1]));
    }
    check(ok, "taps sum to D inside the source", e[0], e[1]);
  }
}

static void wide() {
  // Dx * Dy = 9000 * 2048 > kNarrowArea: x reduces, y enlarges, all-255 (the largest sums there are)
  check(!crop::narrow(crop::den(9000, 10), crop::den(3, 1024)), "9000x3 -> 10x1024 is the wide path");
  const Picture p = picture(9000, 3, 0, 255);
  std::unique_ptr<uint8_t[]> out(new uint8_t[size_t(10) * 1024 * 3]);
  const crop::Box whole;
  crop::apply_cpu(p.px.get(), p.pitch, 9000, 3, &whole, 1, out.get(), 10, 1024, crop::kStretch, crop::Pad{});
  bool white = true;
  for (size_t i = 0; i < size_t(10) * 1024 * 3; ++i) white = white && out[i] == 255;
  check(white, "all-255 stays 255 in 64 bits");
  const Picture n = picture(9000, 3, 5, 0);
  one(n, whole, 10, 64, crop::kStretch, crop::Pad{});
}

template <class F>
static void rejects(const char* what, F&& f) {
  try {
    f();
    check(false, what);
  } catch (const std::exception&) {
  }
}

int main() {
  shapes(0);
  shapes(7);
  closed_forms();
  wide();
  // several boxes land one after the other
  {
    const Picture p = picture(64, 48, 0, 0);
    crop::Box b[3] = {crop::Box{}, box_of(64, 48, 3, 1, 40, 30), box_of(64, 48, 63, 47, 64, 48)};
    std::unique_ptr<uint8_t[]> all(new uint8_t[size_t(3) * 20 * 10 * 3]), single(new uint8_t[size_t(20) * 10 * 3]);
    crop::apply_cpu(p.px.get(), p.pitch, 64, 48, b, 3, all.get(), 20, 10, crop::kLetterbox, crop::Pad{});
    for (int k = 0; k < 3; ++k) {
      crop::apply_cpu(p.px.get(), p.pitch, 64, 48, b + k, 1, single.get(), 20, 10, crop::kLetterbox, crop::Pad{});
      check(std::equal(single.get(), single.get() + 600, all.get() + size_t(k) * 600), "box k of a list", k);
    }
  }
  // bad arguments throw, they do not read or write out of bounds
  uint8_t px[3] = {}, out[3] = {};
  const crop::Box whole;
  const crop::Pad pad;
  auto run = [&](const crop::Box& b, int n, int ow, int oh, int fit, const crop::Pad& c, int w = 1, int h = 1) {
    crop::apply_cpu(px, 3, w, h, &b, n, out, ow, oh, fit, c);
  };
  rejects("x0 == x1", [&] { run(crop::Box{5, 0, 5, 10}, 1, 1, 1, 0, pad); });
  rejects("x1 > 10000", [&] { run(crop::Box{0, 0, 10001, 10}, 1, 1, 1, 0, pad); });
  rejects("y0 < 0", [&] { run(crop::Box{0, -1, 10, 10}, 1, 1, 1, 0, pad); });
  rejects("65 boxes", [&] { run(whole, 65, 1, 1, 0, pad); });
  rejects("width 0", [&] { run(whole, 1, 0, 1, 0, pad); });
  rejects("height 4097", [&] { run(whole, 1, 1, 4097, 0, pad); });
  rejects("fit 2", [&] { run(whole, 1, 1, 1, 2, pad); });
  rejects("pad 256", [&] { run(whole, 1, 1, 1, 0, crop::Pad{0, 256, 0}); });
  rejects("picture 0 wide", [&] { run(whole, 1, 1, 1, 0, pad, 0, 1); });
  rejects("short pitch", [&] { crop::apply_cpu(px, 2, 1, 1, &whole, 1, out, 1, 1, 0, pad); });
  if (failures) return 1;
  std::printf("crop_selftest: ok (%ld crops compared)\n", compared);
  return 0;
}
