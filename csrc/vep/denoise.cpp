// CPU implementation of denoise.h: the CPU backend's path and the byte-exact twin of the kernel.
#include "denoise.h"

#include <algorithm>
#include <vector>

#include "common.h"

namespace vep::denoise {

void check_params(const Params& p) {
  VEP_CHECK(p.frames >= 2 && p.frames <= kMaxFrames, "denoise: frames must be 2..8");
  VEP_CHECK(p.level >= kMinLevel && p.level <= kMaxLevel, "denoise: level must be 1..64");
  VEP_CHECK(p.strength >= 0 && p.strength <= kMaxStrength, "denoise: strength must be 0..1");
}

void check_job(const Job& j) {
  VEP_CHECK(j.frames >= 1 && j.frames <= kMaxFrames, "denoise: 1..8 frames expected");
  VEP_CHECK(j.level >= kMinLevel && j.level <= kMaxLevel, "denoise: level must be 1..64");
  VEP_CHECK(j.strength >= 0 && j.strength <= kMaxStrength, "denoise: strength must be 0..1");
  VEP_CHECK(j.w >= 1 && j.h >= 1 && j.w <= kMaxSide && j.h <= kMaxSide, "denoise: picture size must be 1..65535");
  // Twin and kernel read rows 0 .. h - 1 of every source, bytes 0 .. 3 w - 1 of each (the halo is
  // clamped in the indices), and write the same of the destination: inside the spans below.
  const uint64_t row = uint64_t(j.w) * 3, h = uint64_t(j.h);
  VEP_CHECK(j.dst && uint64_t(j.dst_pitch) >= row, "denoise: null output or pitch shorter than a row");
  const uint64_t dst_span = (h - 1) * j.dst_pitch + row;
  VEP_CHECK(dst_span <= j.dst_bytes, "denoise: output rows outside the output's memory");
  const uintptr_t o = reinterpret_cast<uintptr_t>(j.dst);
  for (int k = 0; k < j.frames; ++k) {
    VEP_CHECK(j.src[k] && uint64_t(j.src_pitch[k]) >= row, "denoise: null frame or pitch shorter than a row");
    const uint64_t span = (h - 1) * j.src_pitch[k] + row;
    VEP_CHECK(span <= j.src_bytes[k], "denoise: frame rows outside the frame's memory");
    const uintptr_t s = reinterpret_cast<uintptr_t>(j.src[k]);
    VEP_CHECK(s + span <= o || o + dst_span <= s, "denoise: the output overlaps a frame");
  }
}

void denoise_cpu(const Job& j) {
  check_job(j);
  const int w = j.w, h = j.h, K = j.frames;
  const size_t n = size_t(w) * size_t(h);
  auto lumas = [&](int k, std::vector<uint8_t>& y) {
    y.resize(n);
    for (int r = 0; r < h; ++r) {
      const uint8_t* p = j.src[k] + size_t(r) * j.src_pitch[k];
      for (int x = 0; x < w; ++x, p += 3) y[size_t(r) * size_t(w) + size_t(x)] = uint8_t(motion::luma(p[0], p[1], p[2]));
    }
  };
  std::vector<uint8_t> y0, yk;
  lumas(0, y0);
  // per pixel: the three channel sums and W, started with the newest frame at full weight
  std::vector<uint32_t> acc(n * 4);
  for (int r = 0; r < h; ++r) {
    const uint8_t* p = j.src[0] + size_t(r) * j.src_pitch[0];
    uint32_t* a = acc.data() + size_t(r) * size_t(w) * 4;
    for (int x = 0; x < w; ++x, p += 3, a += 4) {
      a[0] = kFull * p[0];
      a[1] = kFull * p[1];
      a[2] = kFull * p[2];
      a[3] = kFull;
    }
  }
  std::vector<uint16_t> hs(n);  // three-sums of |Y_0 - Y_k| along the row
  for (int k = 1; k < K; ++k) {
    lumas(k, yk);
    auto ad = [&](int r, int x) {
      const size_t at = size_t(r) * size_t(w) + size_t(std::clamp(x, 0, w - 1));
      return uint32_t(y0[at] > yk[at] ? y0[at] - yk[at] : yk[at] - y0[at]);
    };
    for (int r = 0; r < h; ++r)
      for (int x = 0; x < w; ++x) hs[size_t(r) * size_t(w) + size_t(x)] = uint16_t(ad(r, x - 1) + ad(r, x) + ad(r, x + 1));
    for (int r = 0; r < h; ++r) {
      const uint16_t* up = hs.data() + size_t(std::max(r - 1, 0)) * size_t(w);
      const uint16_t* mid = hs.data() + size_t(r) * size_t(w);
      const uint16_t* down = hs.data() + size_t(std::min(r + 1, h - 1)) * size_t(w);
      const uint8_t* p = j.src[k] + size_t(r) * j.src_pitch[k];
      uint32_t* a = acc.data() + size_t(r) * size_t(w) * 4;
      for (int x = 0; x < w; ++x, p += 3, a += 4) {
        const uint32_t wk = weight(uint32_t(up[x]) + mid[x] + down[x], uint32_t(j.level), uint32_t(j.strength));
        a[0] += wk * p[0];
        a[1] += wk * p[1];
        a[2] += wk * p[2];
        a[3] += wk;
      }
    }
  }
  for (int r = 0; r < h; ++r) {
    uint8_t* q = j.dst + size_t(r) * j.dst_pitch;
    const uint32_t* a = acc.data() + size_t(r) * size_t(w) * 4;
    for (int x = 0; x < w; ++x, q += 3, a += 4) {
      q[0] = uint8_t(mean(a[0], a[3]));
      q[1] = uint8_t(mean(a[1], a[3]));
      q[2] = uint8_t(mean(a[2], a[3]));
    }
  }
}

}  // namespace vep::denoise
