// Remapped views of a picture (fisheye dewarp, lens undistortion, any per-pixel mapping): one
// definition of the arithmetic, shared by the CPU implementation (dewarp.cpp) and the gfx950
// kernel (gpu_dewarp.hip), so both produce the same bytes. docs/DEWARP.md has the reasoning.
// Integers only.
//
// A remap is a MESH: plain data. The output is ow x oh (1 .. kMaxOut each), the source picture at
// most kMaxSrc on a side. Nodes lie every kCell output pixels: mw = cells(ow) + 1 by
// mh = cells(oh) + 1 row-major int32 pairs (sx, sy); node (m, n) is the source position of the
// centre of output pixel (kCell m, kCell n), whether or not that pixel exists, in 1/256 of a source
// pixel, 0 the centre of source pixel 0. A mesh is untrusted: node() clamps every coordinate it
// loads to [kNodeLo, kNodeHi), so no content overflows what follows, and the taps are clamped, so
// no content makes either implementation read outside the picture.
//
// kCell is 8: at 16 the interpolated position of a 185 degree fisheye's panorama is off by half a
// source pixel, at 8 by an eighth (docs/DEWARP.md section 6).
//
// Output pixel (j, k): cell (j >> 3, k >> 3), a = j & 7, b = k & 7, per coordinate
//   S = (8 - a)(8 - b) N00 + a (8 - b) N10 + (8 - a) b N01 + a b N11          weights sum to 64
//   P = (S + 32) >> 6                                                         floor; 1/256 px
// |S| <= 64 * 2^22 = 2^28. A convex combination, and the rounding keeps integers inside the
// nodes' [min, max]: position() never leaves the bounding box of its four nodes.
//
// Sampling: the pixel is OUTSIDE (pad colour) when Px < -128 || Px >= 256 w - 128, likewise y.
// Otherwise ix = Px >> 8, fx = Px & 255, taps clamp(ix, 0, w - 1) and clamp(ix + 1, 0, w - 1),
// likewise y, and each of B, G, R is
//   ((256 - fx)(256 - fy) p00 + fx (256 - fy) p10 + (256 - fx) fy p01 + fx fy p11 + 32768) >> 16
// one rounding, no float; the sum is at most 255 * 65536 + 32768: 32 bits.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "crop.h"

namespace vep::dewarp {

constexpr int kCell = 8, kCellShift = 3;
constexpr int kMaxOut = crop::kMaxOut;
constexpr int kMaxSrc = 8192;
constexpr int32_t kNodeLo = -kMaxSrc * 256, kNodeHi = 2 * kMaxSrc * 256;  // [lo, hi)
constexpr int kMaxMeshPairs = ((kMaxOut + kCell - 1) / kCell + 1) * ((kMaxOut + kCell - 1) / kCell + 1);

static_assert(kCell == 1 << kCellShift, "cell shift");
static_assert(int64_t(kCell) * kCell * kNodeHi + kCell * kCell / 2 < (int64_t(1) << 31) &&
                  int64_t(kCell) * kCell * kNodeLo > -(int64_t(1) << 31),
              "the weighted node sum and its rounding term fit int32");
static_assert(int64_t(kMaxSrc) * 256 < kNodeHi, "every position of the picture can be named");
static_assert(uint64_t(255) * 65536 + 32768 < (uint64_t(1) << 32), "a sample's weighted sum fits a u32");
static_assert(size_t(kMaxMeshPairs) * 8 <= 2057 * 1024, "a mesh is at most 2057 KB");

VEP_MASK_HD inline int cells(int o) { return (o + kCell - 1) >> kCellShift; }
VEP_MASK_HD inline int mesh_w(int ow) { return cells(ow) + 1; }
VEP_MASK_HD inline int mesh_h(int oh) { return cells(oh) + 1; }

struct Pos {
  int32_t x, y;  // 1/256 px
};

VEP_MASK_HD inline int32_t clamp_coord(int32_t v) { return v < kNodeLo ? kNodeLo : (v >= kNodeHi ? kNodeHi - 1 : v); }
// Node (m, n) of a mesh of mw nodes a row: the one place a mesh is loaded from.
template <class Ptr>
VEP_MASK_HD inline Pos node(Ptr mesh, int mw, int m, int n) {
  const size_t at = (size_t(n) * size_t(mw) + size_t(m)) * 2;
  return {clamp_coord(mesh[at]), clamp_coord(mesh[at + 1])};
}

VEP_MASK_HD inline int32_t lerp(int32_t n00, int32_t n10, int32_t n01, int32_t n11, int a, int b) {
  const int32_t s = (kCell - a) * (kCell - b) * n00 + a * (kCell - b) * n10 + (kCell - a) * b * n01 + a * b * n11;
  return (s + kCell * kCell / 2) >> (2 * kCellShift);  // arithmetic shift: floor
}
// The source position of the pixel at (a, b) inside the cell whose nodes are n00 .. n11.
VEP_MASK_HD inline Pos position(const Pos& n00, const Pos& n10, const Pos& n01, const Pos& n11, int a, int b) {
  return {lerp(n00.x, n10.x, n01.x, n11.x, a, b), lerp(n00.y, n10.y, n01.y, n11.y, a, b)};
}

// One axis of a position in a picture of s samples.
VEP_MASK_HD inline bool outside(int32_t p, int s) { return p < -128 || p >= s * 256 - 128; }
struct Tap {
  int i0, i1;   // clamped sample indices
  uint32_t f;   // weight of i1 over 256
};
VEP_MASK_HD inline Tap tap(int32_t p, int s) {  // !outside(p, s)
  const int i = p >> 8;
  return {i < 0 ? 0 : i, i + 1 > s - 1 ? s - 1 : i + 1, uint32_t(p & 255)};
}
VEP_MASK_HD inline uint8_t blend(uint32_t fx, uint32_t fy, uint32_t p00, uint32_t p10, uint32_t p01, uint32_t p11) {
  return uint8_t(((256 - fx) * (256 - fy) * p00 + fx * (256 - fy) * p10 + (256 - fx) * fy * p01 + fx * fy * p11 + 32768) >> 16);
}

// Throws unless the picture size (the output size, the pad colour) is valid.
void check_source(int w, int h);
void check_output(int ow, int oh, const crop::Pad& pad);

// out = the packed BGR24 view of oh x ow: the packed BGR24 picture src (h rows of `pitch` bytes)
// sampled through the mesh of mesh_w(ow) x mesh_h(oh) pairs, as above.
void apply_cpu(const uint8_t* src, size_t pitch, int w, int h, const int32_t* mesh, int ow, int oh, const crop::Pad& pad,
               uint8_t* out);

}  // namespace vep::dewarp
