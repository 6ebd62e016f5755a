// CPU implementation of scale.h: the CPU backend's path and the byte-exact twin of the kernel.
#include "scale.h"

#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"

namespace vep::scale {

void area_cpu(const uint8_t* src, int sw, int sh, size_t src_pitch, uint8_t* dst, size_t dst_pitch, int ow,
              int oh) {
  VEP_CHECK(src && dst, "scale: null picture");
  VEP_CHECK(sw >= 1 && sh >= 1 && sw <= kMaxSide && sh <= kMaxSide, "scale: source size out of range");
  VEP_CHECK(ow >= 1 && oh >= 1 && ow <= sw && oh <= sh, "scale: output must be 1..source size (no upscaling)");
  VEP_CHECK(src_pitch >= size_t(sw) * 3 && dst_pitch >= size_t(ow) * 3, "scale: pitch shorter than a row");
  const uint32_t usw = uint32_t(sw), ush = uint32_t(sh), uow = uint32_t(ow), uoh = uint32_t(oh);
  const uint64_t den = uint64_t(usw) * ush;
  const size_t n = size_t(ow) * 3;
  std::vector<uint64_t> acc(n);
  std::vector<uint32_t> lo(n / 3), hi(n / 3);
  for (uint32_t j = 0; j < uow; ++j) {
    lo[j] = span_lo(j, usw, uow);
    hi[j] = span_hi(j, usw, uow);
  }
  for (uint32_t k = 0; k < uoh; ++k) {
    std::fill(acc.begin(), acc.end(), uint64_t(0));
    const uint32_t r1 = span_hi(k, ush, uoh);
    for (uint32_t r = span_lo(k, ush, uoh); r <= r1; ++r) {
      const uint8_t* row = src + size_t(r) * src_pitch;
      const uint64_t wy = weight(k, r, ush, uoh);
      for (uint32_t j = 0; j < uow; ++j) {
        uint32_t h0 = 0, h1 = 0, h2 = 0;  // <= 255 * sw
        for (uint32_t i = lo[j]; i <= hi[j]; ++i) {
          const uint32_t wx = weight(j, i, usw, uow);
          const uint8_t* p = row + size_t(i) * 3;
          h0 += wx * p[0];
          h1 += wx * p[1];
          h2 += wx * p[2];
        }
        acc[size_t(j) * 3] += wy * h0;
        acc[size_t(j) * 3 + 1] += wy * h1;
        acc[size_t(j) * 3 + 2] += wy * h2;
      }
    }
    uint8_t* out = dst + size_t(k) * dst_pitch;
    for (size_t x = 0; x < n; ++x) out[x] = uint8_t(round_div64(acc[x], den));
  }
}

void compose_cpu(const Tile* tiles, int n, int cols, int tw, int th, uint8_t* canvas, size_t canvas_pitch) {
  VEP_CHECK(canvas && n >= 1 && (tiles || n == 0), "wall: null canvas or no tiles");
  VEP_CHECK(tw >= 1 && th >= 1 && tw <= kMaxSide && th <= kMaxSide, "wall: tile size must be 1..65535");
  VEP_CHECK(cols >= 0 && cols <= kMaxSide, "wall: cols out of range");
  const Wall g = wall(n, cols, tw, th);
  VEP_CHECK(int64_t(g.cols) * tw <= kMaxSide && int64_t(g.rows) * th <= kMaxSide, "wall: canvas larger than 65535");
  VEP_CHECK(canvas_pitch >= size_t(g.w) * 3, "wall: pitch shorter than a row");
  for (int y = 0; y < g.h; ++y) std::memset(canvas + size_t(y) * canvas_pitch, kBackground, size_t(g.w) * 3);
  for (int t = 0; t < n; ++t) {
    const Tile& tl = tiles[t];
    if (!tl.src) continue;
    const Placement p = place(t, g.cols, tw, th, tl.sw, tl.sh);
    area_cpu(tl.src, tl.sw, tl.sh, tl.pitch, canvas + size_t(p.y) * canvas_pitch + size_t(p.x) * 3, canvas_pitch, p.w,
             p.h);
  }
}

}  // namespace vep::scale
