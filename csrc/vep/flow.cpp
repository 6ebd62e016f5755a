// CPU implementation of flow.h: the CPU backend's path and the byte-exact twin of the kernels.
#include "flow.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "common.h"

namespace vep::flow {

void check_match_params(int decimate, int range) {
  VEP_CHECK(decimate == 1 || decimate == 2 || decimate == 4, "flow: decimate must be 1, 2 or 4");
  VEP_CHECK(range >= kMinRange && range <= kMaxRange, "flow: range must be 1..15");
}

void check_params(const Params& p) {
  check_match_params(p.decimate, p.range);
  VEP_CHECK(p.gap >= kMinGap && p.gap <= kMaxGap, "flow: gap must be 1..7");
  VEP_CHECK(p.min_gain >= 0 && p.min_gain <= 255, "flow: min_gain must be 0..255");
  VEP_CHECK(p.min_blocks >= 1, "flow: min_blocks must be 1 or more");
  VEP_CHECK(p.global_percent >= 1 && p.global_percent <= 100, "flow: global_percent must be 1..100");
}

void check_job(const Job& j) {
  check_match_params(j.decimate, j.range);
  VEP_CHECK(j.w >= 1 && j.h >= 1 && j.w <= kMaxSide && j.h <= kMaxSide, "flow: picture size must be 1..65535");
  // Twin and kernels read rows 0 .. h' d - 1 of both sources, bytes 0 .. 3 w' d - 1 of each, write
  // and read rows 0 .. h' - 1 of both planes, whole (pitch bytes: the match kernel loads aligned
  // vectors), and write rows x cols records: inside the spans below.
  const uint64_t row = uint64_t(j.w) * 3, h = uint64_t(j.h);
  const uint32_t pw = plane_side(uint32_t(j.w), uint32_t(j.decimate)), ph = plane_side(uint32_t(j.h), uint32_t(j.decimate));
  const uint64_t plane_span = uint64_t(plane_pitch(pw)) * ph, rec_span = uint64_t(blocks(pw)) * blocks(ph) * sizeof(Record);
  struct Span {
    uintptr_t at;
    uint64_t n;
  };
  Span in[2], out[3];
  for (int k = 0; k < 2; ++k) {
    VEP_CHECK(j.src[k] && uint64_t(j.src_pitch[k]) >= row, "flow: null frame or pitch shorter than a row");
    const uint64_t span = (h - 1) * j.src_pitch[k] + row;
    VEP_CHECK(span <= j.src_bytes[k], "flow: frame rows outside the frame's memory");
    in[k] = {reinterpret_cast<uintptr_t>(j.src[k]), span};
    VEP_CHECK(j.plane[k] && (reinterpret_cast<uintptr_t>(j.plane[k]) & 15u) == 0, "flow: null or unaligned luma plane");
    VEP_CHECK(plane_span <= j.plane_bytes[k], "flow: luma plane too small");
    out[k] = {reinterpret_cast<uintptr_t>(j.plane[k]), plane_span};
  }
  VEP_CHECK(j.records && (reinterpret_cast<uintptr_t>(j.records) & 7u) == 0, "flow: null or unaligned records");
  VEP_CHECK(rec_span <= uint64_t(j.record_count) * sizeof(Record), "flow: record buffer too small");
  out[2] = {reinterpret_cast<uintptr_t>(j.records), rec_span};
  auto apart = [](const Span& a, const Span& b) { return a.n == 0 || b.n == 0 || a.at + a.n <= b.at || b.at + b.n <= a.at; };
  for (int a = 0; a < 3; ++a) {
    for (int k = 0; k < 2; ++k) VEP_CHECK(apart(out[a], in[k]), "flow: an output overlaps a frame");
    for (int b = a + 1; b < 3; ++b) VEP_CHECK(apart(out[a], out[b]), "flow: the outputs overlap");
  }
}

void luma_plane_cpu(const uint8_t* src, int w, int h, size_t src_pitch, int decimate, uint8_t* plane, size_t pitch) {
  const int d = decimate, pw = w / d, ph = h / d;
  for (int y = 0; y < ph; ++y)
    for (int x = 0; x < pw; ++x) {
      uint32_t sum = 0;
      for (int dy = 0; dy < d; ++dy) {
        const uint8_t* p = src + size_t(y * d + dy) * src_pitch + size_t(x) * size_t(d) * 3;
        for (int dx = 0; dx < d; ++dx, p += 3) sum += motion::luma(p[0], p[1], p[2]);
      }
      plane[size_t(y) * pitch + size_t(x)] = uint8_t(sample(sum, uint32_t(d)));
    }
}

void match_cpu(const uint8_t* l0, const uint8_t* lg, int pw, int ph, size_t pitch, int range, Record* records) {
  const int cols = pw / kBlock, rows = ph / kBlock;
  for (int by = 0; by < rows; ++by)
    for (int bx = 0; bx < cols; ++bx) {
      const int x0 = bx * kBlock, y0 = by * kBlock;
      uint32_t best = kInvalidKey, zero = 0;
      for (int vy = -range; vy <= range; ++vy)
        for (int vx = -range; vx <= range; ++vx) {
          if (!valid(x0, y0, vx, vy, pw, ph)) continue;
          uint32_t sad = 0;
          for (int r = 0; r < kBlock; ++r) {
            const uint8_t* a = l0 + size_t(y0 + r) * pitch + size_t(x0);
            const uint8_t* b = lg + size_t(y0 - vy + r) * pitch + size_t(x0 - vx);
            for (int c = 0; c < kBlock; ++c) sad += uint32_t(std::abs(int(a[c]) - int(b[c])));
          }
          if (vx == 0 && vy == 0) zero = sad;
          best = std::min(best, key(sad, vx, vy, range));
        }
      records[size_t(by) * size_t(cols) + size_t(bx)] = record_of(best, zero, range);
    }
}

void flow_cpu(const Job& j) {
  check_job(j);
  const int pw = j.w / j.decimate, ph = j.h / j.decimate;
  const size_t pitch = plane_pitch(uint32_t(pw));
  for (int k = 0; k < 2; ++k) luma_plane_cpu(j.src[k], j.w, j.h, j.src_pitch[k], j.decimate, j.plane[k], pitch);
  match_cpu(j.plane[0], j.plane[1], pw, ph, pitch, j.range, j.records);
}

Summary summarize(const Record* records, int cols, int rows, int decimate, int min_gain, int min_blocks, int global_percent) {
  Summary s;
  const int n = cols * rows, side = 2 * kMaxRange + 1, px = kBlock * decimate;
  std::vector<int> votes(size_t(side) * size_t(side), 0);
  int bx0 = cols, by0 = rows, bx1 = -1, by1 = -1;
  for (int i = 0; i < n; ++i) {
    const Record& r = records[i];
    VEP_CHECK(std::abs(int(r.vx)) <= kMaxRange && std::abs(int(r.vy)) <= kMaxRange, "flow: a record's vector is out of range");
    ++votes[size_t(r.vy + kMaxRange) * size_t(side) + size_t(r.vx + kMaxRange)];
    if ((r.vx == 0 && r.vy == 0) || int(r.zero) - int(r.best) < 64 * min_gain) continue;
    ++s.moving;
    s.sum_vx += r.vx;
    s.sum_vy += r.vy;
    ++s.dirs[direction(r.vx, r.vy)];
    bx0 = std::min(bx0, i % cols);
    bx1 = std::max(bx1, i % cols);
    by0 = std::min(by0, i / cols);
    by1 = std::max(by1, i / cols);
  }
  if (s.moving) {
    s.has_box = true;
    s.x = bx0 * px;
    s.y = by0 * px;
    s.w = (bx1 - bx0 + 1) * px;
    s.h = (by1 - by0 + 1) * px;
  }
  s.motion = s.moving >= min_blocks;
  // the most frequent vector; ties in the key's order: the shorter, then the smaller vy, then vx
  uint32_t best_order = 0;
  for (int vy = -kMaxRange; vy <= kMaxRange; ++vy)
    for (int vx = -kMaxRange; vx <= kMaxRange; ++vx) {
      const int c = votes[size_t(vy + kMaxRange) * size_t(side) + size_t(vx + kMaxRange)];
      const uint32_t order = key(0, vx, vy, kMaxRange);
      if (c > s.global_count || (c == s.global_count && c > 0 && order < best_order)) {
        s.global_count = c;
        s.global_vx = vx;
        s.global_vy = vy;
        best_order = order;
      }
    }
  if (n > 0) {
    s.global_percent = s.global_count * 100 / n;
    s.camera_moved = (s.global_vx != 0 || s.global_vy != 0) && int64_t(s.global_count) * 100 >= int64_t(n) * global_percent;
  }
  return s;
}

}  // namespace vep::flow
