// Per-camera moving-object boxes: frame differencing, a morphological cleanup and 8-connected
// components. One definition of the arithmetic, shared by the CPU implementation (objects.cpp) and
// the gfx950 kernels (gpu_objects.hip), so both produce the same bytes. docs/OBJECTS.md has the
// reasoning. Integers only.
//
// For two packed BGR24 pictures of one size w x h (1 <= w, h <= 65535): F_0, the newest, and F_g,
// the frame `gap` frames before it in the ring:
//   luma planes L_0, L_g: flow.h's (motion::luma, decimated by d in {1, 2, 4} with flow::sample,
//               w' = w / d, h' = h / d, rows flow::plane_pitch(w') bytes apart)
//   raw mask    M0[y][x] = |L_0 - L_g| > threshold (0..255)
//   cleanup     every step maps a w' x h' mask to a w' x h' mask, samples outside the plane being
//               background: if open is 1 a 3 x 3 erosion and then a 3 x 3 dilation; then a square
//               dilation of radius grow (0..3). The result is M
//   packed mask h' rows of mask_words(w') u64: bit x & 63 of word x >> 6 is M[y][x]; the bits past
//               w' are 0
//   components  of M under 8-connectivity. A component's label is the smallest raster index
//               y * w' + x of its samples. Label plane: w' * h' u32, row after row without padding,
//               kBackground where M is 0
//   records     one per component of area >= min_area (4..65535), 24 bytes: label, area and the box
//               x0, y0, x1, y1 in plane samples, x1 and y1 exclusive. capacity() bounds their number.
//               The twin writes them sorted by label; the kernels in any order
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "flow.h"

namespace vep::objects {

constexpr int kMaxSide = flow::kMaxSide;
constexpr int kMinGap = 1, kMaxGap = 7;
constexpr int kMaxGrow = 3;
constexpr int kHalo = 2 + kMaxGrow;  // how far a raw sample reaches through the cleanup
constexpr int kMinArea = 4, kMaxArea = 65535;
constexpr int kMaxObjects = 1024;
constexpr uint32_t kBackground = 0xFFFFFFFFu;

struct Params {
  int decimate = 2, threshold = 24, gap = 1, open = 1, grow = 1, min_area = 64;  // the labelling
  int max_objects = 32;                                                          // the summary
};
// Throws unless decimate is 1, 2 or 4, threshold 0..255, open 0 or 1, grow 0..3, min_area 4..65535,
// gap 1..7 and max_objects 1..1024.
void check_label_params(int decimate, int threshold, int open, int grow, int min_area);
void check_params(const Params& p);

struct Record {
  uint32_t label, area, x0, y0, x1, y1;
};
static_assert(sizeof(Record) == 24, "Record layout");

VEP_MOTION_HD inline uint32_t mask_words(uint32_t pw) { return (pw + 63u) >> 6; }
// The most components of area >= min_area a plane of pw x ph holds: they are disjoint.
VEP_MOTION_HD inline uint64_t capacity(uint32_t pw, uint32_t ph, uint32_t min_area) { return uint64_t(pw) * ph / min_area; }
VEP_MOTION_HD inline bool raw(uint32_t a, uint32_t b, uint32_t threshold) { return (a > b ? a - b : b - a) > threshold; }

// One picture's job as the host states it. Planes, mask, labels, area, records and count are the
// caller's scratch; `area` is working memory whose content afterwards is unspecified.
struct Job {
  const uint8_t* src[2] = {};  // newest, earlier
  size_t src_bytes[2] = {};
  uint32_t src_pitch[2] = {};
  uint8_t* plane[2] = {};
  size_t plane_bytes[2] = {};
  uint64_t* mask = nullptr;
  size_t mask_count = 0;  // u64 words
  uint32_t* labels = nullptr;
  uint32_t* area = nullptr;
  size_t sample_count = 0;  // u32 words of labels and of area, each
  Record* records = nullptr;
  size_t record_count = 0;
  uint32_t* count = nullptr;  // the records written
  int w = 0, h = 0, decimate = 0, threshold = 0, open = 0, grow = 0, min_area = 0;
};
// Throws unless the parameters are in range, the size is 1..65535, every row of both sources lies
// inside its memory, both planes hold h' rows of plane_pitch(w') bytes at a 16-byte aligned address,
// the mask holds h' * mask_words(w') words at an 8-byte aligned address, labels and area w' * h'
// words each, the records capacity(w', h', min_area) entries, count is a word of its own, and no
// output overlaps anything else of the job.
void check_job(const Job& j);

// M of two planes of pw x ph in rows of `pitch` bytes, packed.
void mask_cpu(const uint8_t* l0, const uint8_t* lg, int pw, int ph, size_t pitch, int threshold, int open, int grow, uint64_t* mask);
// Label plane and records (sorted by label) of a packed mask; returns the number of records.
// `area` is scratch of pw * ph words.
uint32_t label_cpu(const uint64_t* mask, int pw, int ph, int min_area, uint32_t* labels, uint32_t* area, Record* records);
// Every step of a checked job.
void objects_cpu(const Job& j);

// sorted records -> what a client asks about. Boxes in full-resolution pixels, clipped to w x h.
struct Object {
  uint32_t label = 0, area = 0;  // area in plane samples
  int x = 0, y = 0, w = 0, h = 0;
};
struct Summary {
  int count = 0;                // records
  std::vector<Object> objects;  // the max_objects largest by area (ties: the smaller label), largest first
  bool truncated = false;       // count > max_objects
  uint64_t area = 0;            // of all records, in plane samples
  bool has_box = false;         // the union of all records' boxes
  int x = 0, y = 0, w = 0, h = 0;
  bool motion = false;          // count >= 1
};
Summary summarize(const Record* sorted, size_t n, int decimate, int max_objects, int w, int h);

}  // namespace vep::objects
