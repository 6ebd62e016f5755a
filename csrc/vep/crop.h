// Crops of a picture, cut and resized: one definition of the arithmetic, shared by the CPU
// implementation (crop.cpp) and the gfx950 kernel (gpu_crop.hip), so both produce the same bytes.
// docs/CROPS.md has the reasoning. Integers only.
//
// A box is a rectangle in 1/10000 of the picture's width and height (0 <= x0 < x1 <= 10000,
// likewise y); mask::to_pixels rounds it OUTWARD to the pixel rect sw x sh, never empty, never
// outside the picture. Every tap below is an index inside that rect.
//
// One axis, source extent s, output extent o (1 <= o <= kMaxOut): output index j has taps (i, w)
// over the fixed denominator D = den(s, o), its weights summing to D.
//   reduce,  o <= s  D = s: scale.h's area average, i in span_lo(j) .. span_hi(j) with weight();
//   enlarge, o > s   D = 2o: bilinear with half-pixel centres and clamped edges. t = (2j + 1) s - o;
//                    t <= 0: (0, 2o). Otherwise i0 = t / 2o, f = t % 2o; i0 >= s - 1: (s - 1, 2o),
//                    else (i0, 2o - f) and (i0 + 1, f). Products stay below 2^31 (8191 * 65535).
// Either way the taps of j are the consecutive indices lo .. hi, and only the two ends differ from
// a common inner weight (reduce: o; enlarge has no inner tap): Taps below.
//
// Two axes, each of B, G, R:
//   out(j, k) = (sum_r sum_i wy(k, r) * wx(j, i) * src(r, i) + Dx * Dy / 2) / (Dx * Dy)
// one rounding at the end, no float, no clamp. The axes are independent: one may reduce while the
// other enlarges. The sum fits 32 bits while Dx * Dy <= scale::kNarrowArea.
//
// Fit: stretch fills the ow x oh output with the rect; letterbox keeps the aspect (fitted()),
// centres the picture and makes every other pixel the pad colour.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "mask.h"
#include "scale.h"

namespace vep::crop {

constexpr int kMaxBoxes = 64;  // per picture
constexpr int kMaxOut = 4096;  // of an output side
constexpr int kMaxSide = mask::kMaxSide;
constexpr int kUnit = mask::kUnit;
constexpr uint8_t kPad = 114;  // B = G = R of the default pad colour (the project's letterbox default)
enum Fit : int { kStretch = 0, kLetterbox = 1 };

static_assert(int64_t(2 * kMaxOut - 1) * kMaxSide < (int64_t(1) << 31), "(2j + 1) * s stays in 32 bits");
static_assert(uint64_t(255) * (2 * kMaxOut) < (uint64_t(1) << 32) && uint64_t(255) * kMaxSide < (uint64_t(1) << 32),
              "a row's weighted sum fits a u32");

struct Box {
  int x0 = 0, y0 = 0, x1 = kUnit, y1 = kUnit;  // 1/10000 of the width / height
};

VEP_MASK_HD inline mask::Rect to_pixels(int w, int h, const Box& b) {
  mask::Rect r{0, 0, 1, 1};
  mask::axis_pixels(w, b.x0, b.x1, r.x0, r.x1);
  mask::axis_pixels(h, b.y0, b.y1, r.y0, r.y1);
  return r;
}

// The denominator of an axis.
VEP_MASK_HD inline uint32_t den(uint32_t s, uint32_t o) { return o <= s ? s : 2 * o; }
VEP_MASK_HD inline bool narrow(uint32_t dx, uint32_t dy) { return uint64_t(dx) * dy <= scale::kNarrowArea; }

// The taps of one output index: source indices lo .. hi, weighing w_lo at lo, w_hi at hi (hi > lo
// only) and w_mid between them.
struct Taps {
  uint32_t lo, hi, w_lo, w_hi, w_mid;
};
VEP_MASK_HD inline Taps taps(uint32_t j, uint32_t s, uint32_t o) {
  Taps t;
  if (o <= s) {
    t.lo = scale::span_lo(j, s, o);
    t.hi = scale::span_hi(j, s, o);
    t.w_lo = scale::weight(j, t.lo, s, o);
    t.w_hi = scale::weight(j, t.hi, s, o);
    t.w_mid = o;
    return t;
  }
  const int32_t c = int32_t((2 * j + 1) * s) - int32_t(o);
  t.w_mid = 0;
  if (c <= 0) {
    t.lo = t.hi = 0;
    t.w_lo = t.w_hi = 2 * o;
    return t;
  }
  const uint32_t i0 = uint32_t(c) / (2 * o), f = uint32_t(c) % (2 * o);
  if (i0 >= s - 1) {
    t.lo = t.hi = s - 1;
    t.w_lo = t.w_hi = 2 * o;
    return t;
  }
  t.lo = i0;
  t.hi = i0 + 1;
  t.w_lo = 2 * o - f;
  t.w_hi = f;
  return t;
}
VEP_MASK_HD inline uint32_t weight_of(const Taps& t, uint32_t i) { return i == t.lo ? t.w_lo : (i == t.hi ? t.w_hi : t.w_mid); }

// Where the resampled rect lies in the ow x oh output: all of it (stretch), or fitted and centred.
struct Placement {
  int x, y, w, h;
};
VEP_MASK_HD inline Placement fitted(int sw, int sh, int ow, int oh, int fit) {
  if (fit != kLetterbox) return {0, 0, ow, oh};
  int fw, fh;
  if (int64_t(sw) * oh >= int64_t(sh) * ow) {
    fw = ow;
    const int64_t v = (2 * int64_t(sh) * ow + sw) / (2 * int64_t(sw));
    fh = int(v < 1 ? 1 : (v > oh ? oh : v));
  } else {
    fh = oh;
    const int64_t v = (2 * int64_t(sw) * oh + sh) / (2 * int64_t(sh));
    fw = int(v < 1 ? 1 : (v > ow ? ow : v));
  }
  return {(ow - fw) / 2, (oh - fh) / 2, fw, fh};
}

struct Pad {
  int b = kPad, g = kPad, r = kPad;
};

// Throws unless the box (the list, the output size, the fit, the pad colour) is valid.
void check_box(const Box& b);
void check_list(const Box* b, int n);
void check_output(int ow, int oh, int fit, const Pad& pad);

// out = n packed BGR24 pictures of oh x ow, one after the other: box k of the packed BGR24 picture
// src (h rows of `pitch` bytes) resampled as above.
void apply_cpu(const uint8_t* src, size_t pitch, int w, int h, const Box* boxes, int n, uint8_t* out, int ow, int oh,
               int fit, const Pad& pad);

}  // namespace vep::crop
