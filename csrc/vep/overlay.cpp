// CPU implementation of overlay.h: the expansion of items into primitives (the one both backends
// use), the CPU backend's drawing path and the byte-exact twin of the kernel.
#include "overlay.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "common.h"

namespace vep::overlay {

namespace {

bool byte_ok(int v) { return v >= 0 && v <= 255; }

struct FontTable {
  uint8_t operator[](uint32_t i) const { return font_byte(i); }
};

uint32_t word_of(int b, int g, int r, int a) { return uint32_t(b) | uint32_t(g) << 8 | uint32_t(r) << 16 | uint32_t(a) << 24; }

// [x0, x1) x [y0, y1) clipped to the picture; nothing is added when nothing is left.
void add_fill(std::vector<Prim>& out, int x0, int y0, int x1, int y1, int w, int h, uint32_t bgra) {
  x0 = std::max(x0, 0);
  y0 = std::max(y0, 0);
  x1 = std::min(x1, w);
  y1 = std::min(y1, h);
  if (x0 >= x1 || y0 >= y1) return;
  out.push_back(Prim{uint16_t(x0), uint16_t(y0), uint16_t(x1), uint16_t(y1), bgra, 0, 0, 0});
}

void add_text(Expanded& e, int ox, int oy, int k, const std::string& s, int w, int h, uint32_t bgra) {
  const int len = int(s.size());
  Prim p{};
  p.x0 = uint16_t(ox);
  p.y0 = uint16_t(oy);
  p.x1 = uint16_t(std::min(ox + kGlyphW * k * len, w));
  p.y1 = uint16_t(std::min(oy + kGlyphH * k, h));
  p.bgra = bgra;
  p.off = uint16_t(e.text.size());
  p.len = uint8_t(len);
  p.k = uint8_t(k);
  e.text += s;
  e.prims.push_back(p);
}

}  // namespace

void check_item(const Item& it) {
  VEP_CHECK(it.kind == kBox || it.kind == kTextItem, "overlay: an item is a box or a text");
  VEP_CHECK(byte_ok(it.b) && byte_ok(it.g) && byte_ok(it.r), "overlay: colour components must be 0..255");
  VEP_CHECK(byte_ok(it.alpha), "overlay: alpha must be 0..255");
  VEP_CHECK(it.text.size() <= size_t(kMaxRawText), "overlay: a text has at most 256 bytes");
  if (it.kind == kBox) {
    VEP_CHECK(it.x0 >= 0 && it.x0 < it.x1 && it.x1 <= kUnit, "overlay: a box needs 0 <= x0 < x1 <= 10000");
    VEP_CHECK(it.y0 >= 0 && it.y0 < it.y1 && it.y1 <= kUnit, "overlay: a box needs 0 <= y0 < y1 <= 10000");
    VEP_CHECK(it.thickness >= 0 && it.thickness <= kMaxThickness, "overlay: thickness must be 1..32, or 0 for auto");
    VEP_CHECK(it.fill == 0 || it.fill == 1, "overlay: fill must be true or false");
  } else {
    VEP_CHECK(it.x0 >= 0 && it.x0 <= kUnit && it.y0 >= 0 && it.y0 <= kUnit, "overlay: a text needs 0 <= x, y <= 10000");
    VEP_CHECK(it.scale >= 0 && it.scale <= kMaxScale, "overlay: scale must be 1..8, or 0 for auto");
    VEP_CHECK(it.has_bg == 0 || it.has_bg == 1, "overlay: bg must be a colour or absent");
    VEP_CHECK(byte_ok(it.bg_b) && byte_ok(it.bg_g) && byte_ok(it.bg_r), "overlay: bg components must be 0..255");
    VEP_CHECK(byte_ok(it.bg_alpha), "overlay: bg_alpha must be 0..255");
  }
}

void check_list(const Item* it, int n) {
  VEP_CHECK(n >= 0 && n <= kMaxItems, "overlay: at most 64 items per picture");
  VEP_CHECK(n == 0 || it, "overlay: null list");
  for (int k = 0; k < n; ++k) check_item(it[k]);
}

std::string time_text(int64_t timestamp) {
  constexpr int64_t kLastMs = 253402300799999;  // 9999-12-31 23:59:59.999
  int64_t ms = timestamp < 0 ? 0 : timestamp / 90;
  ms = std::min(ms, kLastMs);
  const int64_t days = ms / 86400000, in_day = ms % 86400000;
  // days since 1970-01-01 -> civil date (the proleptic Gregorian calendar, eras of 400 years
  // starting on March 1st)
  const int64_t z = days + 719468, era = z / 146097, doe = z - era * 146097;
  const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100), mp = (5 * doy + 2) / 153;
  const int64_t d = doy - (153 * mp + 2) / 5 + 1, m = mp < 10 ? mp + 3 : mp - 9;
  const int64_t y = yoe + era * 400 + (m <= 2 ? 1 : 0);
  char buf[40];
  std::snprintf(buf, sizeof buf, "%04d-%02d-%02d %02d:%02d:%02d.%03d", int(y), int(m), int(d), int(in_day / 3600000),
                int(in_day / 60000 % 60), int(in_day / 1000 % 60), int(in_day % 1000));
  return buf;
}

std::string final_text(const std::string& raw, const std::string& name, const Meta& meta) {
  std::string s;
  for (size_t i = 0; i < raw.size();) {
    if (raw.compare(i, 6, "{name}") == 0) {
      s += name;
      i += 6;
    } else if (raw.compare(i, 5, "{seq}") == 0) {
      s += std::to_string(meta.seq);
      i += 5;
    } else if (raw.compare(i, 6, "{time}") == 0) {
      s += time_text(meta.timestamp);
      i += 6;
    } else {
      s += raw[i++];
    }
  }
  if (s.size() > size_t(kMaxText)) s.resize(size_t(kMaxText));
  for (char& c : s)
    if (uint8_t(c) < 0x20 || uint8_t(c) > 0x7E) c = '?';
  return s;
}

Expanded expand(const Item* items, int n, int w, int h, const std::string& name, const Meta& meta) {
  VEP_CHECK(w >= 1 && h >= 1 && w <= kMaxSide && h <= kMaxSide, "overlay: picture size must be 1..65535");
  check_list(items, n);
  Expanded e;
  const int ak = auto_k(h);
  for (int i = 0; i < n; ++i) {
    const Item& it = items[i];
    const std::string s = final_text(it.text, name, meta);
    const int len = int(s.size());
    if (it.kind == kBox) {
      mask::Mask m;
      m.x0 = it.x0, m.y0 = it.y0, m.x1 = it.x1, m.y1 = it.y1;
      const mask::Rect R = mask::to_pixels(w, h, m);
      const uint32_t c = word_of(it.b, it.g, it.r, it.alpha);
      const int t = it.thickness ? it.thickness : ak;
      if (it.fill || 2 * t >= std::min(R.x1 - R.x0, R.y1 - R.y0)) {
        add_fill(e.prims, R.x0, R.y0, R.x1, R.y1, w, h, c);
      } else {
        add_fill(e.prims, R.x0, R.y0, R.x1, R.y0 + t, w, h, c);
        add_fill(e.prims, R.x0, R.y1 - t, R.x1, R.y1, w, h, c);
        add_fill(e.prims, R.x0, R.y0 + t, R.x0 + t, R.y1 - t, w, h, c);
        add_fill(e.prims, R.x1 - t, R.y0 + t, R.x1, R.y1 - t, w, h, c);
      }
      if (len) {
        const int sw = kGlyphW * ak * len + ak, sh = 9 * ak, sx = R.x0;
        const int sy = R.y0 - sh >= 0 ? R.y0 - sh : R.y0;
        add_fill(e.prims, sx, sy, sx + sw, sy + sh, w, h, c);
        const int ink = 2 * it.r + 5 * it.g + it.b < 1024 ? 255 : 0;
        add_text(e, sx + ak, sy + ak, ak, s, w, h, word_of(ink, ink, ink, 255));
      }
    } else if (len) {
      const int k = it.scale ? it.scale : ak;
      const int ox = it.x0 * w / kUnit, oy = it.y0 * h / kUnit;
      if (it.has_bg)
        add_fill(e.prims, ox - k, oy - k, ox + kGlyphW * k * len, oy + kGlyphH * k, w, h,
                 word_of(it.bg_b, it.bg_g, it.bg_r, it.bg_alpha));
      add_text(e, ox, oy, k, s, w, h, word_of(it.b, it.g, it.r, it.alpha));
    }
    VEP_CHECK(e.prims.size() <= size_t(kMaxPrims), "overlay: the list expands to more than 256 primitives");
  }
  return e;
}

void check_prims(const Prim* p, int n, const uint8_t* text, size_t text_len, int w, int h) {
  VEP_CHECK(w >= 1 && h >= 1 && w <= kMaxSide && h <= kMaxSide, "overlay: picture size must be 1..65535");
  VEP_CHECK(n >= 0 && n <= kMaxPrims, "overlay: at most 256 primitives per picture");
  VEP_CHECK(n == 0 || p, "overlay: null primitives");
  VEP_CHECK(text_len <= size_t(kMaxPool) && (text_len == 0 || text), "overlay: text pool missing or too large");
  for (size_t i = 0; i < text_len; ++i) VEP_CHECK(text[i] >= 0x20 && text[i] <= 0x7E, "overlay: unprintable byte in the pool");
  for (int i = 0; i < n; ++i) {
    const Prim& q = p[i];
    VEP_CHECK(int(q.x1) <= w && int(q.y1) <= h, "overlay: primitive outside the picture");
    if (q.k == 0) {
      VEP_CHECK(q.x0 < q.x1 && q.y0 < q.y1, "overlay: empty fill");
      continue;
    }
    VEP_CHECK(q.k <= kMaxScale && q.len >= 1 && q.len <= kMaxText, "overlay: text scale or length out of range");
    VEP_CHECK(size_t(q.off) + q.len <= text_len, "overlay: text outside the pool");
    // the clipped end never lies past the run's cells (what bounds the glyph and row indices)
    VEP_CHECK(int(q.x1) <= int(q.x0) + kGlyphW * q.k * q.len && int(q.y1) <= int(q.y0) + kGlyphH * q.k,
              "overlay: text end past its cells");
  }
}

void apply_cpu(const uint8_t* src, size_t src_pitch, uint8_t* dst, size_t dst_pitch, int w, int h, const Prim* prims,
               int n, const uint8_t* text, size_t text_len) {
  VEP_CHECK(src && dst, "overlay: null picture");
  check_prims(prims, n, text, text_len, w, h);
  const size_t row = size_t(w) * 3;
  VEP_CHECK(src_pitch >= row && dst_pitch >= row, "overlay: pitch shorter than a row");
  if (dst != src) {
    for (int y = 0; y < h; ++y) std::memcpy(dst + size_t(y) * dst_pitch, src + size_t(y) * src_pitch, row);
  } else {
    VEP_CHECK(src_pitch == dst_pitch, "overlay: in place needs equal pitches");
  }
  // Primitive by primitive on the picture as the earlier ones left it: per pixel that is the fold
  // of blend over the primitives covering it, in list order.
  const FontTable font;
  for (int i = 0; i < n; ++i) {
    const Prim& p = prims[i];
    const uint32_t c[3] = {p.bgra & 255u, (p.bgra >> 8) & 255u, (p.bgra >> 16) & 255u}, a = p.bgra >> 24;
    for (int y = p.y0; y < int(p.y1); ++y) {
      uint8_t* q = dst + size_t(y) * dst_pitch + size_t(p.x0) * 3;
      for (int x = p.x0; x < int(p.x1); ++x, q += 3) {
        if (p.k && !covers(p, x, y, font, text)) continue;
        q[0] = uint8_t(blend(q[0], c[0], a));
        q[1] = uint8_t(blend(q[1], c[1], a));
        q[2] = uint8_t(blend(q[2], c[2], a));
      }
    }
  }
}

}  // namespace vep::overlay
