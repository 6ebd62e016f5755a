// CPU implementation of dewarp.h: the CPU backend's path and the byte-exact twin of the kernel.
#include "dewarp.h"

#include "common.h"

namespace vep::dewarp {

void check_source(int w, int h) {
  VEP_CHECK(w >= 1 && h >= 1 && w <= kMaxSrc && h <= kMaxSrc, "view: picture size must be 1..8192");
}

void check_output(int ow, int oh, const crop::Pad& pad) {
  VEP_CHECK(ow >= 1 && ow <= kMaxOut && oh >= 1 && oh <= kMaxOut, "view: width and height must be 1..4096");
  VEP_CHECK(pad.b >= 0 && pad.b <= 255 && pad.g >= 0 && pad.g <= 255 && pad.r >= 0 && pad.r <= 255,
            "view: pad colour components must be 0..255");
}

void apply_cpu(const uint8_t* src, size_t pitch, int w, int h, const int32_t* mesh, int ow, int oh, const crop::Pad& pad,
               uint8_t* out) {
  VEP_CHECK(src && mesh && out, "view: null picture, mesh or output");
  check_source(w, h);
  VEP_CHECK(pitch >= size_t(w) * 3, "view: pitch shorter than a row");
  check_output(ow, oh, pad);
  const int mw = mesh_w(ow);
  for (int k = 0; k < oh; ++k) {
    const int n = k >> kCellShift, b = k & (kCell - 1);
    uint8_t* o = out + size_t(k) * size_t(ow) * 3;
    for (int j = 0; j < ow; ++j, o += 3) {
      const int m = j >> kCellShift, a = j & (kCell - 1);
      const Pos p = position(node(mesh, mw, m, n), node(mesh, mw, m + 1, n), node(mesh, mw, m, n + 1),
                             node(mesh, mw, m + 1, n + 1), a, b);
      if (outside(p.x, w) || outside(p.y, h)) {
        o[0] = uint8_t(pad.b), o[1] = uint8_t(pad.g), o[2] = uint8_t(pad.r);
        continue;
      }
      const Tap tx = tap(p.x, w), ty = tap(p.y, h);
      const uint8_t* r0 = src + size_t(ty.i0) * pitch;
      const uint8_t* r1 = src + size_t(ty.i1) * pitch;
      for (int c = 0; c < 3; ++c)
        o[c] = blend(tx.f, ty.f, r0[tx.i0 * 3 + c], r0[tx.i1 * 3 + c], r1[tx.i0 * 3 + c], r1[tx.i1 * 3 + c]);
    }
  }
}

}  // namespace vep::dewarp
