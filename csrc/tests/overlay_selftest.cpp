// Stand-alone check of the CPU on-screen display (vep/overlay.cpp) for sanitizer builds
// (`make asan-overlay`: AddressSanitizer + UndefinedBehaviorSanitizer on the host). Every picture
// lives in a heap buffer of exactly its size, so a read or write past a row or the picture is a
// report. Shapes: the edge pictures (1x1, 7x5, 17x9, 64x16, 65x17, 200x120), each with boxes
// (outlines, fills, labels above, inside and off the right edge), texts at every corner and past
// every edge at scales 1, 3 and 8, translucent overlaps and a 256-primitive list; each compared,
// out of place and in place, with a per-pixel restatement of docs/OVERLAY.md section 1 (for every
// pixel: fold the blend over the primitives that cover it, in list order); once more with a pitch
// wider than the row, whose padding must stay untouched. Then the refusals. Exit status 0, no
// sanitizer report and "overlay_selftest: ok" = pass.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "vep/common.h"
#include "vep/overlay.h"

using namespace vep;

static int failures = 0;

static void check(bool ok, const char* what, int w = 0, int h = 0, int k = 0) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s (%dx%d case %d)\n", what, w, h, k);
  ++failures;
}

static uint32_t seed = 97531;
static uint8_t rnd() {
  seed = seed * 1664525u + 1013904223u;
  return uint8_t(seed >> 24);
}

static overlay::Item box(int x0, int y0, int x1, int y1, int t, int alpha, const char* label, int fill = 0) {
  overlay::Item it;
  it.kind = overlay::kBox;
  it.x0 = x0, it.y0 = y0, it.x1 = x1, it.y1 = y1;
  it.b = 30, it.g = 200, it.r = 90, it.alpha = alpha;
  it.thickness = t;
  it.fill = fill;
  it.text = label;
  return it;
}

static overlay::Item text(int x, int y, int scale, int alpha, const char* s, int bg_alpha = -1) {
  overlay::Item it;
  it.kind = overlay::kTextItem;
  it.x0 = x, it.y0 = y;
  it.b = 250, it.g = 240, it.r = 10, it.alpha = alpha;
  it.scale = scale;
  it.text = s;
  if (bg_alpha >= 0) it.has_bg = 1, it.bg_b = 5, it.bg_g = 6, it.bg_r = 7, it.bg_alpha = bg_alpha;
  return it;
}

// docs/OVERLAY.md section 1, pixel by pixel: is (px, py) covered by primitive p?
static bool covered(const overlay::Prim& p, const std::string& pool, int px, int py, int w, int h) {
  if (px < 0 || py < 0 || px >= w || py >= h) return false;
  if (p.k == 0) return px >= p.x0 && px < p.x1 && py >= p.y0 && py < p.y1;
  const int k = p.k, dx = px - int(p.x0), dy = py - int(p.y0);
  if (dx < 0 || dy < 0 || dx >= 6 * k * int(p.len) || dy >= 8 * k) return false;
  const int glyph = uint8_t(pool[size_t(p.off) + size_t(dx / (6 * k))]) - 0x20;
  return (overlay::font_byte(uint32_t(glyph * 8 + dy / k)) >> ((dx / k) % 6)) & 1;
}

static void run_case(int w, int h, size_t pitch, const std::vector<overlay::Item>& items, int k) {
  const overlay::Meta meta{123456, int64_t(90) * 1790000000123};
  const overlay::Expanded e = overlay::expand(items.data(), int(items.size()), w, h, "cam", meta);
  const uint8_t* pool = reinterpret_cast<const uint8_t*>(e.text.data());
  const size_t bytes = size_t(h - 1) * pitch + size_t(w) * 3;  // exactly the rows: the last one has no padding
  std::unique_ptr<uint8_t[]> src(new uint8_t[bytes]), dst(new uint8_t[bytes]), want(new uint8_t[bytes]);
  for (size_t i = 0; i < bytes; ++i) src[i] = rnd();
  std::memset(dst.get(), 0xA5, bytes);
  std::memset(want.get(), 0xA5, bytes);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x)
      for (int c = 0; c < 3; ++c) {
        uint32_t v = src[size_t(y) * pitch + size_t(x) * 3 + size_t(c)];
        for (const overlay::Prim& p : e.prims)
          if (covered(p, e.text, x, y, w, h)) {
            const uint32_t col = (p.bgra >> (8 * c)) & 255u, a = p.bgra >> 24;
            v = (v * (255 - a) + col * a + 127) / 255;
          }
        want[size_t(y) * pitch + size_t(x) * 3 + size_t(c)] = uint8_t(v);
      }
  overlay::apply_cpu(src.get(), pitch, dst.get(), pitch, w, h, e.prims.data(), int(e.prims.size()), pool, e.text.size());
  check(std::memcmp(dst.get(), want.get(), bytes) == 0, "out of place differs from the restatement", w, h, k);
  // in place: the pixels as above, the padding as the source had it
  for (int y = 0; y + 1 < h; ++y)
    std::memcpy(want.get() + size_t(y) * pitch + size_t(w) * 3, src.get() + size_t(y) * pitch + size_t(w) * 3,
                pitch - size_t(w) * 3);
  overlay::apply_cpu(src.get(), pitch, src.get(), pitch, w, h, e.prims.data(), int(e.prims.size()), pool, e.text.size());
  check(std::memcmp(src.get(), want.get(), bytes) == 0, "in place differs from the restatement", w, h, k);
}

template <class F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const Error&) {
    return true;
  }
  return false;
}

int main() {
  const int sizes[][2] = {{1, 1}, {7, 5}, {17, 9}, {64, 16}, {65, 17}, {200, 120}};
  std::vector<std::vector<overlay::Item>> lists;
  lists.push_back({});
  lists.push_back({box(0, 0, 10000, 10000, 0, 200, "", 1)});
  lists.push_back({box(0, 0, 7000, 6000, 0, 100, "", 1), box(3000, 2000, 10000, 9000, 0, 180, "", 1),
                   box(1000, 4000, 9000, 10000, 0, 33, "", 1)});
  lists.push_back({box(500, 500, 9500, 9500, 0, 120, "person 87%"), box(2000, 0, 6000, 5000, 3, 255, "top {seq}"),
                   box(8000, 6000, 10000, 10000, 32, 200, "runs off the right edge"), box(4999, 4999, 5000, 5000, 1, 255, "")});
  for (int scale : {1, 3, 8})  // every corner, and past every edge
    lists.push_back({text(0, 0, scale, 255, "corner", 140), text(9700, 4000, scale, 210, "right edge"),
                     text(2000, 9800, scale, 255, "bottom edge", 255), text(10000, 10000, scale, 255, "outside", 9),
                     text(9990, 9990, scale, 77, "last pixel"), text(300, 2000, scale, 255, "{name} {time} ~!@#$%^&*()_+|"),
                     text(10000, 0, scale, 255, "x", 1), text(0, 10000, scale, 255, "y", 1)});
  {
    std::vector<overlay::Item> dense;  // 42 labelled outlines and two texts on a background: 256 primitives at 200 x 120
    for (int i = 0; i < 42; ++i)
      dense.push_back(box(100 + 1400 * (i % 7), 1200 + 1450 * (i / 7), 700 + 1400 * (i % 7), 2000 + 1450 * (i / 7), 1,
                          255 - 3 * i, std::to_string(i).c_str()));
    dense.push_back(text(50, 50, 1, 255, "{name} {time}", 128));
    dense.push_back(text(5000, 9000, 2, 255, "seq {seq}", 60));
    check(overlay::expand(dense.data(), int(dense.size()), 200, 120, "cam", overlay::Meta{}).prims.size() == 256,
          "the dense list expands to 256 primitives");
    lists.push_back(dense);
    dense.push_back(box(0, 0, 1, 1, 0, 255, ""));
    check(throws([&] { overlay::expand(dense.data(), int(dense.size()), 200, 120, "cam", overlay::Meta{}); }),
          "257 primitives are refused");
  }
  int k = 0;
  for (const auto& sz : sizes)
    for (const auto& items : lists) {
      const int w = sz[0], h = sz[1];
      run_case(w, h, size_t(w) * 3, items, k);
      run_case(w, h, size_t(w) * 3 + 13, items, k);
      ++k;
    }
  // closed forms
  check(overlay::blend(77, 200, 255) == 200 && overlay::blend(77, 200, 0) == 77, "blend identities");
  check(overlay::auto_k(1) == 1 && overlay::auto_k(539) == 1 && overlay::auto_k(540) == 2 && overlay::auto_k(1080) == 4 &&
            overlay::auto_k(4320) == 8,
        "auto scale");
  check(overlay::time_text(int64_t(90) * 1790000000123) == "2026-09-21 14:13:20.123", "time text");
  check(overlay::final_text(std::string(65, 'x'), "", overlay::Meta{}).size() == 64, "text is cut at 64 bytes");
  check(overlay::final_text("a\x80", "", overlay::Meta{}) == "a?", "a byte 0x80 becomes ?");
  // refusals
  const overlay::Item good = box(0, 0, 5000, 5000, 0, 255, "");
  auto bad = [&](auto&& change) {
    overlay::Item it = good;
    change(it);
    return throws([&] { overlay::check_item(it); });
  };
  check(bad([](overlay::Item& i) { i.x0 = -1; }) && bad([](overlay::Item& i) { i.x1 = 10001; }) &&
            bad([](overlay::Item& i) { i.y0 = 5000; }) && bad([](overlay::Item& i) { i.alpha = 256; }) &&
            bad([](overlay::Item& i) { i.r = -1; }) && bad([](overlay::Item& i) { i.thickness = 33; }) &&
            bad([](overlay::Item& i) { i.fill = 2; }) && bad([](overlay::Item& i) { i.kind = 2; }) &&
            bad([](overlay::Item& i) { i.text = std::string(257, 'x'); }) &&
            bad([](overlay::Item& i) { i.kind = overlay::kTextItem, i.scale = 9; }) &&
            bad([](overlay::Item& i) { i.kind = overlay::kTextItem, i.x0 = 10001; }) &&
            bad([](overlay::Item& i) { i.kind = overlay::kTextItem, i.bg_alpha = -1; }),
        "invalid items are refused");
  std::vector<overlay::Item> many(65, good);
  check(throws([&] { overlay::check_list(many.data(), 65); }), "65 items are refused");
  check(throws([&] { overlay::expand(&good, 1, 0, 5, "", overlay::Meta{}); }), "an empty picture is refused");
  {
    overlay::Prim p{0, 0, 8, 4, 0, 0, 0, 0};
    uint8_t pic[3 * 7 * 5] = {};
    check(throws([&] { overlay::apply_cpu(pic, 21, pic, 21, 7, 5, &p, 1, nullptr, 0); }), "a fill outside the picture is refused");
    overlay::Prim t{0, 0, 6, 5, 0, 3, 1, 1};
    check(throws([&] { overlay::apply_cpu(pic, 21, pic, 21, 7, 5, &t, 1, reinterpret_cast<const uint8_t*>("abc"), 3); }),
          "a text outside the pool is refused");
    const uint8_t raw[1] = {0x80};
    overlay::Prim u{0, 0, 6, 5, 0, 0, 1, 1};
    check(throws([&] { overlay::apply_cpu(pic, 21, pic, 21, 7, 5, &u, 1, raw, 1); }), "an unprintable pool is refused");
  }
  if (failures) {
    std::fprintf(stderr, "overlay_selftest: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("overlay_selftest: ok\n");
  return 0;
}
