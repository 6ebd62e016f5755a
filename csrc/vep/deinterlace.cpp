// CPU implementation of deinterlace.h: the CPU backend's path and the byte-exact twin of the kernel.
#include "deinterlace.h"

#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"

namespace vep::deinterlace {

void check_params(const Params& p) {
  VEP_CHECK(p.order == kTff || p.order == kBff, "deinterlace: order must be tff or bff");
  VEP_CHECK(p.temporal == 0 || p.temporal == 1, "deinterlace: temporal must be 0 or 1");
}

void check_job(const Job& j) {
  check_params(j.p);
  VEP_CHECK(j.w >= kMinSide && j.h >= kMinSide && j.w <= kMaxSide && j.h <= kMaxSide,
            "deinterlace: both sides of the picture must be 4..65535");
  // Twin and kernel read rows 0 .. h - 1 of every source, bytes 0 .. 3 w - 1 of each (the halo is
  // clamped in the indices), and write the same of the destination: inside the spans below.
  const uint64_t row = uint64_t(j.w) * 3, h = uint64_t(j.h);
  VEP_CHECK(j.dst && uint64_t(j.dst_pitch) >= row, "deinterlace: null output or pitch shorter than a row");
  const uint64_t dst_span = (h - 1) * j.dst_pitch + row;
  VEP_CHECK(dst_span <= j.dst_bytes, "deinterlace: output rows outside the output's memory");
  const uintptr_t o = reinterpret_cast<uintptr_t>(j.dst);
  auto source = [&](const uint8_t* p, uint32_t pitch, size_t bytes) {
    VEP_CHECK(p && uint64_t(pitch) >= row, "deinterlace: null frame or pitch shorter than a row");
    const uint64_t span = (h - 1) * pitch + row;
    VEP_CHECK(span <= bytes, "deinterlace: frame rows outside the frame's memory");
    const uintptr_t s = reinterpret_cast<uintptr_t>(p);
    VEP_CHECK(s + span <= o || o + dst_span <= s, "deinterlace: the output overlaps a frame");
  };
  source(j.newer, j.newer_pitch, j.newer_bytes);
  if (j.older) {
    VEP_CHECK(j.older_w == j.w && j.older_h == j.h, "deinterlace: the previous frame must have the size of the newest");
    source(j.older, j.older_pitch, j.older_bytes);
  }
}

void deinterlace_cpu(const Job& j) {
  check_job(j);
  const int w = j.w, h = j.h, parity = j.p.order;
  const bool temporal = temporal_of(j);
  auto lumas = [&](const uint8_t* src, uint32_t pitch, std::vector<uint8_t>& y) {
    y.resize(size_t(w) * size_t(h));
    for (int r = 0; r < h; ++r) {
      const uint8_t* p = src + size_t(r) * pitch;
      for (int x = 0; x < w; ++x, p += 3) y[size_t(r) * size_t(w) + size_t(x)] = uint8_t(motion::luma(p[0], p[1], p[2]));
    }
  };
  std::vector<uint8_t> yf, yg;
  lumas(j.newer, j.newer_pitch, yf);
  if (temporal) lumas(j.older, j.older_pitch, yg);
  for (int y = 0; y < h; ++y) {
    const uint8_t* f = j.newer + size_t(y) * j.newer_pitch;
    uint8_t* q = j.dst + size_t(y) * j.dst_pitch;
    if ((y & 1) == parity) {
      std::memcpy(q, f, size_t(w) * 3);
      continue;
    }
    const int up = row_up(y), dn = row_dn(y, h);
    const uint8_t* fu = j.newer + size_t(up) * j.newer_pitch;
    const uint8_t* fd = j.newer + size_t(dn) * j.newer_pitch;
    const uint8_t* yu = yf.data() + size_t(up) * size_t(w);
    const uint8_t* yd = yf.data() + size_t(dn) * size_t(w);
    auto col = [&](int x) { return size_t(std::clamp(x, 0, w - 1)); };
    auto score = [&](int x, int d) {
      uint32_t s = 0;
      for (int k = -1; k <= 1; ++k) s += absdiff(yu[col(x + k + d)], yd[col(x + k - d)]);
      return s;
    };
    for (int x = 0; x < w; ++x) {
      const int d = direction(score(x, -2), score(x, -1), score(x, 0), score(x, 1), score(x, 2));
      const uint8_t* a = fu + col(x + d) * 3;
      const uint8_t* b = fd + col(x - d) * 3;
      uint32_t out[3] = {predict(a[0], b[0]), predict(a[1], b[1]), predict(a[2], b[2])};
      if (temporal) {
        auto moved = [&](int r) {
          const size_t at = size_t(r) * size_t(w) + size_t(x);
          return absdiff(yg[at], yf[at]);
        };
        const uint32_t diff = motion_of(moved(y), moved(up), moved(dn));
        const uint8_t* g = j.older + size_t(y) * j.older_pitch + size_t(x) * 3;
        for (int c = 0; c < 3; ++c) out[c] = bound(out[c], g[c], f[size_t(x) * 3 + size_t(c)], diff);
      }
      for (int c = 0; c < 3; ++c) q[size_t(x) * 3 + size_t(c)] = uint8_t(out[c]);
    }
  }
}

}  // namespace vep::deinterlace
