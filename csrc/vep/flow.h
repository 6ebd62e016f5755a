// Per-camera motion vectors by exhaustive block matching: one definition of the arithmetic, shared
// by the CPU implementation (flow.cpp) and the gfx950 kernels (gpu_flow.hip), so both produce the
// same bytes. docs/FLOW.md has the reasoning. Integers only; every intermediate fits a u32.
//
// For two packed BGR24 pictures of one size w x h (1 <= w, h <= 65535): F_0, the newest, and F_g,
// the frame `gap` frames before it in the ring:
//   luma plane  Y = motion::luma. With decimate d in {1, 2, 4}: w' = w / d, h' = h / d (floor, the
//               trailing pixels unused), L[y][x] = (sum of the d x d lumas + d * d / 2) >> (2 log2 d)
//   blocks      8 x 8 samples of L: cols = w' / 8, rows = h' / 8 (floor). Only whole blocks are
//               matched; a picture too small for one block has an empty grid
//   candidates  (vx, vy), |vx|, |vy| <= R (range, 1..15): the block of L_0 at (x0, y0) against L_g
//               at (x0 - vx, y0 - vy), so the vector says how the content moved from the earlier
//               frame to the newest. A candidate counts only if its displaced block lies wholly
//               inside L_g: decided from coordinates, never from data. (0, 0) always counts
//   cost        SAD = sum over the 64 samples of |L_0 - L_g|, at most 16320
//   choice      the valid candidate with the smallest
//               key = SAD << 15 | (|vx| + |vy|) << 10 | (vy + R) << 5 | (vx + R)
//               (|vx| + |vy| <= 30 and vy + R, vx + R <= 30 fit five bits each; the key is below
//               2^29). Ties go to the shorter vector, then to the smaller vy, then the smaller vx; a
//               flat or unchanged block reports (0, 0)
//   record      8 bytes a block, row-major: i8 vx, i8 vy, u16 best, u16 zero (the SAD at (0, 0)), u16 0
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "motion.h"

namespace vep::flow {

constexpr int kMaxSide = motion::kMaxSide;
constexpr int kBlock = 8;
constexpr int kMinRange = 1, kMaxRange = 15;
constexpr int kMinGap = 1, kMaxGap = 7;
constexpr uint32_t kMaxSad = 64 * 255;  // 16320
constexpr uint32_t kInvalidKey = 0xFFFFFFFFu;
static_assert(kMaxSad < (1u << 14) && 2 * kMaxRange < 32, "the key's fields hold their values");

struct Params {
  int decimate = 2, range = 7, gap = 1;                  // the match
  int min_gain = 4, min_blocks = 4, global_percent = 60;  // the summary
};
// Throws unless decimate is 1, 2 or 4, range 1..15, gap 1..7, min_gain 0..255, min_blocks >= 1 and
// global_percent 1..100.
void check_match_params(int decimate, int range);
void check_params(const Params& p);

VEP_MOTION_HD inline uint32_t log2_of(uint32_t d) { return d == 4u ? 2u : (d == 2u ? 1u : 0u); }
// A sample of L from the sum of its d x d lumas.
VEP_MOTION_HD inline uint32_t sample(uint32_t sum, uint32_t d) { return (sum + d * d / 2u) >> (2u * log2_of(d)); }
// samples along a side of n pixels, whole blocks along a side of n samples
VEP_MOTION_HD inline uint32_t plane_side(uint32_t n, uint32_t d) { return n / d; }
VEP_MOTION_HD inline uint32_t blocks(uint32_t n) { return n / uint32_t(kBlock); }
// bytes between the rows of a plane of pw samples: rows start 16-byte aligned
VEP_MOTION_HD inline uint32_t plane_pitch(uint32_t pw) { return (pw + 15u) & ~15u; }

VEP_MOTION_HD inline uint32_t key(uint32_t sad, int vx, int vy, int range) {
  const uint32_t len = uint32_t(vx < 0 ? -vx : vx) + uint32_t(vy < 0 ? -vy : vy);
  return sad << 15 | len << 10 | uint32_t(vy + range) << 5 | uint32_t(vx + range);
}
// Whether the block at (x0, y0) displaced by (-vx, -vy) lies inside a plane of pw x ph.
VEP_MOTION_HD inline bool valid(int x0, int y0, int vx, int vy, int pw, int ph) {
  const int x = x0 - vx, y = y0 - vy;
  return x >= 0 && y >= 0 && x + kBlock <= pw && y + kBlock <= ph;
}

struct Record {
  int8_t vx, vy;
  uint16_t best, zero, pad;
};
static_assert(sizeof(Record) == 8, "Record layout");
VEP_MOTION_HD inline Record record_of(uint32_t k, uint32_t zero, int range) {
  return Record{int8_t(int(k & 31u) - range), int8_t(int((k >> 5) & 31u) - range), uint16_t(k >> 15), uint16_t(zero), 0};
}

// One picture's job as the host states it: the two frames, the two planes they become and the
// records. Planes and records are the caller's scratch; every row of a plane is plane_pitch bytes.
struct Job {
  const uint8_t* src[2] = {};  // newest, earlier
  size_t src_bytes[2] = {};
  uint32_t src_pitch[2] = {};
  uint8_t* plane[2] = {};
  size_t plane_bytes[2] = {};
  Record* records = nullptr;
  size_t record_count = 0;
  int w = 0, h = 0, decimate = 0, range = 0;
};
// Throws unless the parameters are in range, the size is 1..65535, every row of both sources lies
// inside its memory, both planes hold h' rows of plane_pitch(w') bytes at a 16-byte aligned address,
// the records hold rows x cols entries at an 8-byte aligned address, and no output overlaps
// anything else of the job.
void check_job(const Job& j);

// L of one frame: h' rows of plane_pitch bytes, w' samples written in each (padding untouched).
void luma_plane_cpu(const uint8_t* src, int w, int h, size_t src_pitch, int decimate, uint8_t* plane, size_t plane_pitch);
// The records of L_0 against L_g, both pw x ph in rows of `pitch` bytes: blocks(ph) x blocks(pw).
void match_cpu(const uint8_t* l0, const uint8_t* lg, int pw, int ph, size_t pitch, int range, Record* records);
// Both steps of a checked job.
void flow_cpu(const Job& j);

// records -> what a client asks about.
struct Summary {
  int moving = 0;              // blocks with (vx, vy) != (0, 0) and zero - best >= 64 * min_gain
  int sum_vx = 0, sum_vy = 0;  // over the moving blocks, in samples of L
  int dirs[8] = {};            // E, SE, S, SW, W, NW, N, NE (picture coordinates, y down)
  bool has_box = false;        // the pixel rectangle bounding the moving blocks
  int x = 0, y = 0, w = 0, h = 0;
  bool motion = false;         // moving >= min_blocks
  int global_vx = 0, global_vy = 0, global_count = 0, global_percent = 0;  // the most frequent vector of all blocks
  bool camera_moved = false;   // it is not (0, 0) and count * 100 >= blocks * global_percent
};
// The direction bin of a vector other than (0, 0): horizontal when 12 |vy| < 5 |vx|, vertical when
// 12 |vx| < 5 |vy|, diagonal otherwise (the boundary is tan 22.6 degrees).
VEP_MOTION_HD inline int direction(int vx, int vy) {
  const int a = vx < 0 ? -vx : vx, b = vy < 0 ? -vy : vy;
  if (12 * b < 5 * a) return vx > 0 ? 0 : 4;
  if (12 * a < 5 * b) return vy > 0 ? 2 : 6;
  return vy > 0 ? (vx > 0 ? 1 : 3) : (vx > 0 ? 7 : 5);
}
Summary summarize(const Record* records, int cols, int rows, int decimate, int min_gain, int min_blocks, int global_percent);

}  // namespace vep::flow
