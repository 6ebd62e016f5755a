// CPU implementation of dehaze.h: the CPU backend's path and the byte-exact twin of the kernels.
#include "dehaze.h"

#include <algorithm>
#include <vector>

#include "common.h"

namespace vep::dehaze {

void check_params(const Params& p) {
  VEP_CHECK(p.patch >= kMinPatch && p.patch <= kMaxPatch && p.patch % 2 == 1, "dehaze: patch must be odd and 3..31");
  VEP_CHECK(p.omega >= 0 && p.omega <= kMaxOmega, "dehaze: omega must be 0..1");
  VEP_CHECK(p.t0 >= kMinT0 && p.t0 <= kTOne, "dehaze: t0 must be 0.05..1");
  VEP_CHECK(p.radius >= kMinRadius && p.radius <= kMaxRadius, "dehaze: radius must be 1..16");
  VEP_CHECK(p.strength >= 0 && p.strength <= kMaxStrength, "dehaze: strength must be 0..1");
}

void check_job(const Job& j) {
  check_params(j.p);
  VEP_CHECK(j.w >= kMinSide && j.h >= kMinSide && j.w <= kMaxSide && j.h <= kMaxSide && uint64_t(j.w) * uint64_t(j.h) <= kMaxPixels,
            "dehaze: both sides must be 16..65535 and the picture at most 2^24 pixels");
  // Twin and kernels read rows 0 .. h - 1 of the source, bytes 0 .. 3 w - 1 of each (windows are
  // clipped to the picture), and write the same of the destination: inside the spans below.
  const uint64_t row = uint64_t(j.w) * 3, h = uint64_t(j.h);
  VEP_CHECK(j.src && j.dst, "dehaze: null picture");
  VEP_CHECK(uint64_t(j.src_pitch) >= row && uint64_t(j.dst_pitch) >= row, "dehaze: pitch shorter than a row");
  const uint64_t src_span = (h - 1) * j.src_pitch + row, dst_span = (h - 1) * j.dst_pitch + row;
  VEP_CHECK(src_span <= j.src_bytes, "dehaze: picture rows outside the picture's memory");
  VEP_CHECK(dst_span <= j.dst_bytes, "dehaze: output rows outside the output's memory");
  // The table pass touches kTableWords words, the air pass kAirWords, and every cell pass cells
  // (cy, cx) with cy < ch and cx < cw (boxes and the recovery's four cells are clamped to that).
  const uint64_t ncell = uint64_t(cells(uint32_t(j.w))) * cells(uint32_t(j.h));
  VEP_CHECK(j.table && j.air && j.cell && j.ab && j.mean, "dehaze: null plane");
  VEP_CHECK(j.table_words >= size_t(kTableWords) && j.air_words >= size_t(kAirWords) && j.cell_words >= ncell &&
                j.ab_words >= 2 * ncell && j.mean_words >= 2 * ncell,
            "dehaze: a plane is too small for the picture");
  const uintptr_t at[7] = {reinterpret_cast<uintptr_t>(j.table), reinterpret_cast<uintptr_t>(j.air),
                           reinterpret_cast<uintptr_t>(j.cell),  reinterpret_cast<uintptr_t>(j.ab),
                           reinterpret_cast<uintptr_t>(j.mean),  reinterpret_cast<uintptr_t>(j.src),
                           reinterpret_cast<uintptr_t>(j.dst)};
  const uint64_t len[7] = {uint64_t(kTableWords) * 4, uint64_t(kAirWords) * 4, ncell * 4, ncell * 8, ncell * 8, src_span, dst_span};
  for (int k = 0; k < 5; ++k) VEP_CHECK(at[k] % 8 == 0, "dehaze: the planes must be 8-byte aligned");
  for (int a = 0; a < 7; ++a)
    for (int b = a + 1; b < 7; ++b) {
      if (a == 5 && at[5] == at[6]) {
        VEP_CHECK(j.src_pitch == j.dst_pitch, "dehaze: in place needs equal pitches");
        continue;
      }
      VEP_CHECK(at[a] + len[a] <= at[b] || at[b] + len[b] <= at[a], "dehaze: pictures and planes overlap");
    }
}

size_t plane_words(int w, int h) {
  const size_t ncell = size_t(cells(uint32_t(w))) * cells(uint32_t(h));
  return (size_t(kTableWords) + kAirWords + 5 * ncell + 1) & ~size_t(1);
}

void carve_planes(Job& j, uint32_t* words) {
  static_assert((kTableWords + kAirWords) % 2 == 0, "the planes behind the tables stay 8-byte aligned");
  const size_t ncell = size_t(cells(uint32_t(j.w))) * cells(uint32_t(j.h));
  j.table = words;
  j.table_words = kTableWords;
  j.air = words += kTableWords;
  j.air_words = kAirWords;
  j.ab = reinterpret_cast<int32_t*>(words += kAirWords);
  j.ab_words = 2 * ncell;
  j.mean = reinterpret_cast<int32_t*>(words += 2 * ncell);
  j.mean_words = 2 * ncell;
  j.cell = words += 2 * ncell;
  j.cell_words = ncell;
}

namespace {

// out[y][x] = min of v over the patch window around (x, y), clipped: rows first, then columns.
void window_min(const std::vector<uint8_t>& v, int w, int h, int r, std::vector<uint8_t>& out) {
  std::vector<uint8_t> rows(v.size());
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      uint8_t m = 255;
      for (int k = std::max(0, x - r); k <= std::min(w - 1, x + r); ++k) m = std::min(m, v[size_t(y) * w + k]);
      rows[size_t(y) * w + x] = m;
    }
  out.resize(v.size());
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      uint8_t m = 255;
      for (int k = std::max(0, y - r); k <= std::min(h - 1, y + r); ++k) m = std::min(m, rows[size_t(k) * w + x]);
      out[size_t(y) * w + x] = m;
    }
}

}  // namespace

void table_cpu(const Job& j) {
  const int w = j.w, h = j.h;
  std::vector<uint8_t> m(size_t(w) * h), d;
  for (int y = 0; y < h; ++y) {
    const uint8_t* p = j.src + size_t(y) * j.src_pitch;
    for (int x = 0; x < w; ++x, p += 3) m[size_t(y) * w + x] = uint8_t(min3(p[0], p[1], p[2]));
  }
  window_min(m, w, h, j.p.patch / 2, d);
  std::fill(j.table, j.table + kTableWords, uint32_t(0));
  for (int y = 0; y < h; ++y) {
    const uint8_t* p = j.src + size_t(y) * j.src_pitch;
    for (int x = 0; x < w; ++x, p += 3) {
      uint32_t* bin = j.table + size_t(d[size_t(y) * w + x]) * 4;
      bin[0] += 1;
      bin[1] += p[0];
      bin[2] += p[1];
      bin[3] += p[2];
    }
  }
}

void air_cpu(const Job& j) {
  const uint32_t target = air_target(uint32_t(j.w), uint32_t(j.h));
  uint32_t n = 0, s[3] = {0, 0, 0};
  for (int v = kBins - 1; v >= 0 && n < target; --v) {
    const uint32_t* bin = j.table + size_t(v) * 4;
    n += bin[0];
    for (int c = 0; c < 3; ++c) s[c] += bin[1 + c];
  }
  VEP_CHECK(n >= 1, "dehaze: the table is empty");
  uint8_t* norm = reinterpret_cast<uint8_t*>(j.air + 4);
  for (int c = 0; c < 3; ++c) {
    j.air[c] = air_of(s[c], n);
    for (int v = 0; v < kBins; ++v) norm[c * kBins + v] = uint8_t(norm_of(uint32_t(v), j.air[c]));
  }
  j.air[3] = n;
}

void cells_cpu(const Job& j) {
  const int w = j.w, h = j.h;
  const uint8_t* norm = reinterpret_cast<const uint8_t*>(j.air + 4);
  std::vector<uint8_t> nn(size_t(w) * h), dn;
  for (int y = 0; y < h; ++y) {
    const uint8_t* p = j.src + size_t(y) * j.src_pitch;
    for (int x = 0; x < w; ++x, p += 3)
      nn[size_t(y) * w + x] = uint8_t(min3(norm[p[0]], norm[kBins + p[1]], norm[2 * kBins + p[2]]));
  }
  window_min(nn, w, h, j.p.patch / 2, dn);
  const int cw = int(cells(uint32_t(w))), ch = int(cells(uint32_t(h)));
  for (int cy = 0; cy < ch; ++cy)
    for (int cx = 0; cx < cw; ++cx) {
      uint32_t sy = 0, st = 0, n = 0;
      for (int y = cy * kCell; y < std::min(h, (cy + 1) * kCell); ++y) {
        const uint8_t* p = j.src + size_t(y) * j.src_pitch + size_t(cx) * kCell * 3;
        for (int x = cx * kCell; x < std::min(w, (cx + 1) * kCell); ++x, p += 3, ++n) {
          sy += motion::luma(p[0], p[1], p[2]);
          st += t_raw(uint32_t(j.p.omega), dn[size_t(y) * w + x]);
        }
      }
      j.cell[size_t(cy) * cw + cx] = cell_value(sy, st, n);
    }
}

void coeff_cpu(const Job& j) {
  const uint32_t cw = cells(uint32_t(j.w)), ch = cells(uint32_t(j.h)), r = uint32_t(j.p.radius);
  for (uint32_t cy = 0; cy < ch; ++cy)
    for (uint32_t cx = 0; cx < cw; ++cx) {
      uint32_t x0, x1, y0, y1, sy = 0, st = 0, syt = 0, syy = 0;
      box_span(cx, cw, r, x0, x1);
      box_span(cy, ch, r, y0, y1);
      for (uint32_t y = y0; y <= y1; ++y)
        for (uint32_t x = x0; x <= x1; ++x) {
          const uint32_t c = j.cell[size_t(y) * cw + x], yc = c & 0xffffu, tc = c >> 16;
          sy += yc;
          st += tc;
          syt += yc * tc;
          syy += yc * yc;
        }
      int32_t* o = j.ab + (size_t(cy) * cw + cx) * 2;
      coeffs(sy, st, syt, syy, (x1 - x0 + 1) * (y1 - y0 + 1), o[0], o[1]);
    }
}

void smooth_cpu(const Job& j) {
  const uint32_t cw = cells(uint32_t(j.w)), ch = cells(uint32_t(j.h)), r = uint32_t(j.p.radius);
  for (uint32_t cy = 0; cy < ch; ++cy)
    for (uint32_t cx = 0; cx < cw; ++cx) {
      uint32_t x0, x1, y0, y1;
      box_span(cx, cw, r, x0, x1);
      box_span(cy, ch, r, y0, y1);
      int64_t sa = 0, sb = 0;
      for (uint32_t y = y0; y <= y1; ++y)
        for (uint32_t x = x0; x <= x1; ++x) {
          sa += j.ab[(size_t(y) * cw + x) * 2];
          sb += j.ab[(size_t(y) * cw + x) * 2 + 1];
        }
      const uint32_t k = (x1 - x0 + 1) * (y1 - y0 + 1);
      j.mean[(size_t(cy) * cw + cx) * 2] = box_mean(sa, k);
      j.mean[(size_t(cy) * cw + cx) * 2 + 1] = box_mean(sb, k);
    }
}

void apply_cpu(const Job& j) {
  const uint32_t cw = cells(uint32_t(j.w)), ch = cells(uint32_t(j.h));
  const uint32_t t0 = uint32_t(j.p.t0), strength = uint32_t(j.p.strength);
  std::vector<uint32_t> recip(size_t(kTOne) + 1, 0u);
  for (uint32_t t = t0; t <= uint32_t(kTOne); ++t) recip[t] = recip_of(t);
  for (int y = 0; y < j.h; ++y) {
    uint32_t j0, j1, wy;
    axis(uint32_t(y), ch, j0, j1, wy);
    const int32_t* top = j.mean + size_t(j0) * cw * 2;
    const int32_t* bot = j.mean + size_t(j1) * cw * 2;
    const uint8_t* p = j.src + size_t(y) * j.src_pitch;
    uint8_t* q = j.dst + size_t(y) * j.dst_pitch;
    for (int x = 0; x < j.w; ++x, p += 3, q += 3) {
      uint32_t i0, i1, wx;
      axis(uint32_t(x), cw, i0, i1, wx);
      const int32_t a64 = lerp4(top[i0 * 2], top[i1 * 2], bot[i0 * 2], bot[i1 * 2], wx, wy);
      const int32_t b64 = lerp4(top[i0 * 2 + 1], top[i1 * 2 + 1], bot[i0 * 2 + 1], bot[i1 * 2 + 1], wx, wy);
      const uint32_t rc = recip[transmission(a64, b64, motion::luma(p[0], p[1], p[2]), t0)];
      for (int c = 0; c < 3; ++c) q[c] = uint8_t(recovered(p[c], j.air[c], rc, strength));
    }
  }
}

void run_cpu(const Job& j) {
  check_job(j);
  table_cpu(j);
  air_cpu(j);
  cells_cpu(j);
  coeff_cpu(j);
  smooth_cpu(j);
  apply_cpu(j);
}

void dehaze_cpu(const uint8_t* src, size_t src_pitch, uint8_t* dst, size_t dst_pitch, int w, int h, const Params& p,
                uint32_t* air) {
  VEP_CHECK(w >= kMinSide && h >= kMinSide && w <= kMaxSide && h <= kMaxSide, "dehaze: both sides must be 16..65535");
  VEP_CHECK(src_pitch <= 0xffffffffu && dst_pitch <= 0xffffffffu, "dehaze: pitch too large");
  std::vector<uint64_t> planes(plane_words(w, h) / 2);  // (8-byte aligned)
  Job j;
  j.src = src;
  j.src_pitch = uint32_t(src_pitch);
  j.src_bytes = size_t(h - 1) * src_pitch + size_t(w) * 3;
  j.dst = dst;
  j.dst_pitch = uint32_t(dst_pitch);
  j.dst_bytes = size_t(h - 1) * dst_pitch + size_t(w) * 3;
  j.w = w;
  j.h = h;
  j.p = p;
  carve_planes(j, reinterpret_cast<uint32_t*>(planes.data()));
  run_cpu(j);
  if (air)
    for (int c = 0; c < 3; ++c) air[c] = j.air[c];
}

}  // namespace vep::dehaze
