// Motion-adaptive deinterlacing of a served picture from the ring's newest two frames: one
// definition of the arithmetic, shared by the CPU implementation (deinterlace.cpp) and the gfx950
// kernel (gpu_deinterlace.hip), so both produce the same bytes. docs/DEINTERLACE.md has the
// reasoning. Integers only; every intermediate fits 16 bits (the bounds are stated where they arise).
//
// A woven frame F (packed BGR24, w x h, 4 <= w, h <= 65535) holds two fields half a frame interval
// apart on alternating rows. With p the parity of the EARLIER field (order tff: p = 0, the even
// rows; bff: p = 1) the output shows the scene at the time of that field:
//   kept rows     y % 2 == p: copied from F.
//   missing rows  y % 2 != p: rebuilt. up = y - 1 (y + 1 at y == 0), dn = y + 1 (y - 1 at
//                 y == h - 1): rows of the kept field. Columns are clamped to 0 .. w - 1 in the
//                 indices; Y is motion::luma, 0..255.
//     direction   score(j) = sum over k in {-1, 0, 1} of |Y_F(up, x + k + j) - Y_F(dn, x + k - j)|,
//                 0..765. best = score(0) - 1 (-1..764), j* = 0; score(-1) < best takes -1, and only
//                 then a still smaller score(-2) takes -2; the same for +1, then +2, against the
//                 best so far (direction() below: the five scores decide, in whatever order they
//                 were formed).
//     spatial     pred_c = (F_c(up, x + j*) + F_c(dn, x - j*)) >> 1 per channel: 0..255.
//     temporal    with the previous frame G of the same size (and Params::temporal): the fields half
//                 an interval before and after the kept one are G's and F's own rows of parity
//                 1 - p, so  d_c = (G_c(y, x) + F_c(y, x)) >> 1                          0..255
//                            t0  = |Y_G(y, x) - Y_F(y, x)|                               0..255
//                            t1  = (|Y_G(up, x) - Y_F(up, x)| + |Y_G(dn, x) - Y_F(dn, x)|) >> 1
//                            diff = max(t0 >> 1, t1)                                     0..255
//                            out_c = clamp(pred_c, d_c - diff, d_c + diff)               -255..510
//                 the yadif filter without its spatial interlacing check (rows y +- 2), made
//                 causal. Without G, or with temporal 0: out_c = pred_c.
//
// Fixed properties (closed forms of tests/test_deinterlace.py and csrc/tests/deinterlace_selftest.cpp):
//   * kept rows always equal F.
//   * where F and G agree on rows up, y and dn at column x, the output pixel is F(y, x): t0 = t1 = 0,
//     diff = 0, d_c = F_c(y, x), and the clamp to [d_c, d_c] returns it. A static scene keeps its
//     woven frame bit for bit, at full vertical resolution.
//   * the result is 0..255 with no final clamp: pred_c is, so a lower bound is only taken where it
//     exceeds pred_c >= 0 and is itself at most d_c <= 255; the upper bound likewise.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "motion.h"
#include "scale.h"

namespace vep::deinterlace {

constexpr int kMinSide = 4;
constexpr int kMaxSide = scale::kMaxSide;
constexpr int kMaxDirection = 2;              // |j| of the edge-directed prediction
constexpr int kReach = kMaxDirection + 1;     // columns left and right of x that a score reads
constexpr uint32_t kMaxScore = 3 * 255;

enum Order : int { kTff = 0, kBff = 1 };  // the parity of the earlier field

struct Params {
  int order = kTff;
  int temporal = 1;
};
// Throws unless order is kTff or kBff and temporal 0 or 1.
void check_params(const Params& p);

VEP_MOTION_HD inline uint32_t absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }
// The rows of the kept field above and below the missing row y of a picture of h rows.
VEP_MOTION_HD inline int row_up(int y) { return y == 0 ? 1 : y - 1; }
VEP_MOTION_HD inline int row_dn(int y, int h) { return y == h - 1 ? y - 1 : y + 1; }
// j* from score(-2), score(-1), score(0), score(1), score(2).
VEP_MOTION_HD inline int direction(uint32_t sm2, uint32_t sm1, uint32_t s0, uint32_t sp1, uint32_t sp2) {
  int best = int(s0) - 1, j = 0;
  if (int(sm1) < best) {
    best = int(sm1), j = -1;
    if (int(sm2) < best) best = int(sm2), j = -2;
  }
  if (int(sp1) < best) {
    best = int(sp1), j = 1;
    if (int(sp2) < best) j = 2;
  }
  return j;
}
VEP_MOTION_HD inline uint32_t predict(uint32_t up, uint32_t dn) { return (up + dn) >> 1; }
// diff from |Y_G - Y_F| at (y, x), (up, x) and (dn, x).
VEP_MOTION_HD inline uint32_t motion_of(uint32_t at_y, uint32_t at_up, uint32_t at_dn) {
  const uint32_t t0 = at_y >> 1, t1 = (at_up + at_dn) >> 1;
  return t0 > t1 ? t0 : t1;
}
// out_c from pred_c, G_c(y, x), F_c(y, x) and diff.
VEP_MOTION_HD inline uint32_t bound(uint32_t pred, uint32_t g, uint32_t f, uint32_t diff) {
  const int d = int((g + f) >> 1), lo = d - int(diff), hi = d + int(diff), v = int(pred);
  return uint32_t(v < lo ? lo : (v > hi ? hi : v));
}

// One picture's job as the host states it: the newest frame, the previous one (null: spatial
// only) and a destination, each with the bytes of its memory.
struct Job {
  const uint8_t* newer = nullptr;
  const uint8_t* older = nullptr;
  uint8_t* dst = nullptr;
  size_t newer_bytes = 0, older_bytes = 0, dst_bytes = 0;
  uint32_t newer_pitch = 0, older_pitch = 0, dst_pitch = 0;
  int w = 0, h = 0;
  int older_w = 0, older_h = 0;  // with `older`: must be w and h
  Params p;
};
// Throws unless the parameters are valid, both sides are 4..65535, the previous frame (if any)
// has the size of the newest, every row of every picture lies inside its memory, and the
// destination overlaps no source (out of place only: a source is never written).
void check_job(const Job& j);
// Whether the job's temporal bound runs: a previous frame is given and Params::temporal is set.
inline bool temporal_of(const Job& j) { return j.older && j.p.temporal; }

// The woven frame deinterlaced into dst. Checked.
void deinterlace_cpu(const Job& j);

}  // namespace vep::deinterlace
