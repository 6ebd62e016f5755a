// Upright pictures of cameras mounted sideways, upside down or behind a mirror: quarter turns and
// mirrors of a packed BGR24 picture. One definition of the index arithmetic, shared by the CPU
// implementation (orient.cpp) and the gfx950 kernel (gpu_orient.hip), so both produce the same
// bytes. docs/ORIENT.md has the reasoning. Pixels are only moved: there is no arithmetic on them.
//
// A request is `rotate` in {0, 90, 180, 270} degrees clockwise FOLLOWED BY `flip` in {none, h, v}
// (h mirrors left-right, v top-bottom, both on the rotated picture). It becomes three bits:
//   T   the output's rows run along the source's columns (a transposition)
//   MX  the output's columns are walked backwards
//   MY  the output's rows are walked backwards
// For a source of w x h (sides 1..65535):
//   size   ow x oh = (T ? h : w) x (T ? w : h)
//   map    ax = MX ? ow - 1 - ox : ox,  ay = MY ? oh - 1 - oy : oy,
//          (sx, sy) = T ? (ay, ax) : (ax, ay),  out(oy, ox) = src(sy, sx), all three bytes.
//   rotate 90: T MX.  180: MX MY.  270: T MY.  flip h toggles MX, flip v toggles MY.
//
// Closed forms (asserted below or in csrc/tests/orient_selftest.cpp and tests/test_orient.py):
//   * the map is a bijection of the ow x oh output onto the w x h source: ax and ay are
//     involutions of 0 .. ow - 1 and 0 .. oh - 1, and the swap exchanges two ranges of equal size.
//   * composition. Write an op as the map on coordinates "mirror, then maybe swap". Applying op a
//     to a picture and op b to the result gives the op compose(a, b):
//       T  = Ta ^ Tb
//       MX = MXb ^ (Tb ? MYa : MXa)
//       MY = MYb ^ (Tb ? MXa : MYa)
//     (b's mirrors act on b's output axes; behind b's swap a's mirrors meet the other axis).
//   * rotate 90 four times is the identity: T MX -> MX MY -> T MY -> 0 under compose.
//   * rotate 180 equals flip h followed by flip v: MX then MY, no swap, gives MX MY.
//   * the eight ops are the symmetry group of the square; of(rotate, flip) reaches each of them
//     (12 requests, 4 of them twice: rotate 180 + h == v, 180 + v == h, and the two diagonals).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "motion.h"
#include "scale.h"

namespace vep::orient {

constexpr int kMaxSide = scale::kMaxSide;

enum Bits : int { kT = 1, kMX = 2, kMY = 4 };
enum Flip : int { kNone = 0, kH = 1, kV = 2 };

// The op of a request, or -1 where rotate is no quarter turn or flip none of the three.
VEP_MOTION_HD constexpr int of(int rotate, int flip) {
  int op = rotate == 0 ? 0 : rotate == 90 ? (kT | kMX) : rotate == 180 ? (kMX | kMY) : rotate == 270 ? (kT | kMY) : -1;
  if (op < 0 || flip < kNone || flip > kV) return -1;
  return op ^ (flip == kH ? kMX : flip == kV ? kMY : 0);
}
// Op a applied first, op b to its result.
VEP_MOTION_HD constexpr int compose(int a, int b) {
  const int ta = a & kT, tb = b & kT;
  const int mxa = (a & kMX) != 0, mya = (a & kMY) != 0;
  const int mx = ((b & kMX) != 0) ^ (tb ? mya : mxa), my = ((b & kMY) != 0) ^ (tb ? mxa : mya);
  return (ta ^ tb) | (mx ? kMX : 0) | (my ? kMY : 0);
}
constexpr int kR90 = of(90, kNone);
static_assert(compose(compose(compose(kR90, kR90), kR90), kR90) == 0, "four quarter turns are the identity");
static_assert(compose(kR90, kR90) == of(180, kNone) && compose(of(180, kNone), kR90) == of(270, kNone), "quarter turns add up");
static_assert(compose(of(0, kH), of(0, kV)) == of(180, kNone), "180 is h followed by v");
static_assert(compose(kR90, of(0, kH)) == of(90, kH) && compose(of(270, kNone), of(0, kV)) == of(270, kV), "flip follows rotate");

VEP_MOTION_HD inline int out_w(int op, int w, int h) { return op & kT ? h : w; }
VEP_MOTION_HD inline int out_h(int op, int w, int h) { return op & kT ? w : h; }
// The source pixel (sx, sy) of the output pixel (ox, oy) of an ow x oh output.
VEP_MOTION_HD inline void source_of(int op, int ow, int oh, int ox, int oy, int& sx, int& sy) {
  const int ax = op & kMX ? ow - 1 - ox : ox, ay = op & kMY ? oh - 1 - oy : oy;
  sx = op & kT ? ay : ax;
  sy = op & kT ? ax : ay;
}

// One picture's job as the host states it: the source of w x h, the destination of out_w x out_h,
// each with the bytes of its memory.
struct Job {
  const uint8_t* src = nullptr;
  uint8_t* dst = nullptr;
  size_t src_bytes = 0, dst_bytes = 0;
  uint32_t src_pitch = 0, dst_pitch = 0;
  int w = 0, h = 0;
  int op = 0;  // Bits
};
// Throws unless op is 0..7, both sides are 1..65535, every row of the source and of the ow x oh
// destination lies inside its memory, and the two do not overlap (out of place only: a source,
// which may be a ring slot, is never written).
void check_job(const Job& j);
// The source oriented into dst. Checked.
void apply_cpu(const Job& j);

}  // namespace vep::orient
