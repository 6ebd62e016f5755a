// CPU implementation of orient.h: the CPU backend's path and the byte-exact twin of the kernel.
#include "orient.h"

#include <cstring>

#include "common.h"

namespace vep::orient {

void check_job(const Job& j) {
  VEP_CHECK(j.op >= 0 && j.op <= (kT | kMX | kMY), "orient: rotate must be 0, 90, 180 or 270 and flip none, h or v");
  VEP_CHECK(j.w >= 1 && j.h >= 1 && j.w <= kMaxSide && j.h <= kMaxSide, "orient: both sides of the picture must be 1..65535");
  // Twin and kernel read rows 0 .. h - 1 of the source, bytes 0 .. 3 w - 1 of each, and write rows
  // 0 .. oh - 1 of the destination, bytes 0 .. 3 ow - 1 of each: inside the spans below.
  const uint64_t row = uint64_t(j.w) * 3, orow = uint64_t(out_w(j.op, j.w, j.h)) * 3;
  const uint64_t h = uint64_t(j.h), oh = uint64_t(out_h(j.op, j.w, j.h));
  VEP_CHECK(j.src && uint64_t(j.src_pitch) >= row, "orient: null picture or pitch shorter than a row");
  VEP_CHECK(j.dst && uint64_t(j.dst_pitch) >= orow, "orient: null output or pitch shorter than a row");
  const uint64_t src_span = (h - 1) * j.src_pitch + row, dst_span = (oh - 1) * j.dst_pitch + orow;
  VEP_CHECK(src_span <= j.src_bytes, "orient: picture rows outside the picture's memory");
  VEP_CHECK(dst_span <= j.dst_bytes, "orient: output rows outside the output's memory");
  const uintptr_t s = reinterpret_cast<uintptr_t>(j.src), o = reinterpret_cast<uintptr_t>(j.dst);
  VEP_CHECK(s + src_span <= o || o + dst_span <= s, "orient: the output overlaps the picture");
}

void apply_cpu(const Job& j) {
  check_job(j);
  const int ow = out_w(j.op, j.w, j.h), oh = out_h(j.op, j.w, j.h);
  for (int oy = 0; oy < oh; ++oy) {
    uint8_t* q = j.dst + size_t(oy) * j.dst_pitch;
    if (!(j.op & (kT | kMX))) {  // a row as it is
      int sx, sy;
      source_of(j.op, ow, oh, 0, oy, sx, sy);
      std::memcpy(q, j.src + size_t(sy) * j.src_pitch, size_t(ow) * 3);
      continue;
    }
    for (int ox = 0; ox < ow; ++ox, q += 3) {
      int sx, sy;
      source_of(j.op, ow, oh, ox, oy, sx, sy);
      const uint8_t* p = j.src + size_t(sy) * j.src_pitch + size_t(sx) * 3;
      q[0] = p[0];
      q[1] = p[1];
      q[2] = p[2];
    }
  }
}

}  // namespace vep::orient
