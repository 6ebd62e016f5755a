// CPU implementation of objects.h: the CPU backend's path and the byte-exact twin of the kernels.
#include "objects.h"

#include <algorithm>

#include "common.h"

namespace vep::objects {

void check_label_params(int decimate, int threshold, int open, int grow, int min_area) {
  VEP_CHECK(decimate == 1 || decimate == 2 || decimate == 4, "objects: decimate must be 1, 2 or 4");
  VEP_CHECK(threshold >= 0 && threshold <= 255, "objects: threshold must be 0..255");
  VEP_CHECK(open == 0 || open == 1, "objects: open must be 0 or 1");
  VEP_CHECK(grow >= 0 && grow <= kMaxGrow, "objects: grow must be 0..3");
  VEP_CHECK(min_area >= kMinArea && min_area <= kMaxArea, "objects: min_area must be 4..65535");
}

void check_params(const Params& p) {
  check_label_params(p.decimate, p.threshold, p.open, p.grow, p.min_area);
  VEP_CHECK(p.gap >= kMinGap && p.gap <= kMaxGap, "objects: gap must be 1..7");
  VEP_CHECK(p.max_objects >= 1 && p.max_objects <= kMaxObjects, "objects: max_objects must be 1..1024");
}

void check_job(const Job& j) {
  check_label_params(j.decimate, j.threshold, j.open, j.grow, j.min_area);
  VEP_CHECK(j.w >= 1 && j.h >= 1 && j.w <= kMaxSide && j.h <= kMaxSide, "objects: picture size must be 1..65535");
  // Twin and kernels read rows 0 .. h' d - 1 of both sources, bytes 0 .. 3 w' d - 1 of each, write
  // and read rows 0 .. h' - 1 of both planes, h' * mask_words(w') mask words, w' * h' words of
  // labels and of area, at most capacity() records and the count: inside the spans below.
  const uint64_t row = uint64_t(j.w) * 3, h = uint64_t(j.h);
  const uint32_t pw = flow::plane_side(uint32_t(j.w), uint32_t(j.decimate)), ph = flow::plane_side(uint32_t(j.h), uint32_t(j.decimate));
  const uint64_t samples = uint64_t(pw) * ph;
  struct Span {
    uintptr_t at;
    uint64_t n;
  };
  Span in[2], out[7];
  const uint64_t plane_span = uint64_t(flow::plane_pitch(pw)) * ph;
  for (int k = 0; k < 2; ++k) {
    VEP_CHECK(j.src[k] && uint64_t(j.src_pitch[k]) >= row, "objects: null frame or pitch shorter than a row");
    const uint64_t span = (h - 1) * j.src_pitch[k] + row;
    VEP_CHECK(span <= j.src_bytes[k], "objects: frame rows outside the frame's memory");
    in[k] = {reinterpret_cast<uintptr_t>(j.src[k]), span};
    VEP_CHECK(j.plane[k] && (reinterpret_cast<uintptr_t>(j.plane[k]) & 15u) == 0, "objects: null or unaligned luma plane");
    VEP_CHECK(plane_span <= j.plane_bytes[k], "objects: luma plane too small");
    out[k] = {reinterpret_cast<uintptr_t>(j.plane[k]), plane_span};
  }
  VEP_CHECK(j.mask && (reinterpret_cast<uintptr_t>(j.mask) & 7u) == 0, "objects: null or unaligned mask");
  VEP_CHECK(uint64_t(mask_words(pw)) * ph <= j.mask_count, "objects: mask too small");
  out[2] = {reinterpret_cast<uintptr_t>(j.mask), uint64_t(mask_words(pw)) * ph * 8};
  VEP_CHECK(j.labels && j.area && ((reinterpret_cast<uintptr_t>(j.labels) | reinterpret_cast<uintptr_t>(j.area)) & 3u) == 0,
            "objects: null or unaligned label or area plane");
  VEP_CHECK(samples <= j.sample_count, "objects: label and area planes too small");
  out[3] = {reinterpret_cast<uintptr_t>(j.labels), samples * 4};
  out[4] = {reinterpret_cast<uintptr_t>(j.area), samples * 4};
  const uint64_t cap = capacity(pw, ph, uint32_t(j.min_area));
  VEP_CHECK(j.records && (reinterpret_cast<uintptr_t>(j.records) & 3u) == 0, "objects: null or unaligned records");
  VEP_CHECK(cap <= j.record_count, "objects: record buffer below the capacity bound");
  out[5] = {reinterpret_cast<uintptr_t>(j.records), cap * sizeof(Record)};
  VEP_CHECK(j.count && (reinterpret_cast<uintptr_t>(j.count) & 3u) == 0, "objects: null or unaligned count");
  out[6] = {reinterpret_cast<uintptr_t>(j.count), 4};
  auto apart = [](const Span& a, const Span& b) { return a.n == 0 || b.n == 0 || a.at + a.n <= b.at || b.at + b.n <= a.at; };
  for (int a = 0; a < 7; ++a) {
    for (int k = 0; k < 2; ++k) VEP_CHECK(apart(out[a], in[k]), "objects: an output overlaps a frame");
    for (int b = a + 1; b < 7; ++b) VEP_CHECK(apart(out[a], out[b]), "objects: the outputs overlap");
  }
}

namespace {

// One step of the cleanup on a byte mask: erosion (all of the square set) or dilation (any),
// samples outside the plane background.
void morph(const std::vector<uint8_t>& in, std::vector<uint8_t>& out, int pw, int ph, int radius, bool erode) {
  for (int y = 0; y < ph; ++y)
    for (int x = 0; x < pw; ++x) {
      bool all = true, any = false;
      for (int dy = -radius; dy <= radius; ++dy)
        for (int dx = -radius; dx <= radius; ++dx) {
          const int yy = y + dy, xx = x + dx;
          const bool v = yy >= 0 && yy < ph && xx >= 0 && xx < pw && in[size_t(yy) * size_t(pw) + size_t(xx)];
          all = all && v;
          any = any || v;
        }
      out[size_t(y) * size_t(pw) + size_t(x)] = erode ? all : any;
    }
}

}  // namespace

void mask_cpu(const uint8_t* l0, const uint8_t* lg, int pw, int ph, size_t pitch, int threshold, int open, int grow, uint64_t* mask) {
  std::vector<uint8_t> a(size_t(pw) * size_t(ph)), b(a.size());
  for (int y = 0; y < ph; ++y)
    for (int x = 0; x < pw; ++x)
      a[size_t(y) * size_t(pw) + size_t(x)] = raw(l0[size_t(y) * pitch + size_t(x)], lg[size_t(y) * pitch + size_t(x)], uint32_t(threshold));
  if (open) {
    morph(a, b, pw, ph, 1, true);
    morph(b, a, pw, ph, 1, false);
  }
  if (grow) {
    morph(a, b, pw, ph, grow, false);
    a.swap(b);
  }
  const size_t words = mask_words(uint32_t(pw));
  std::fill(mask, mask + words * size_t(ph), uint64_t(0));
  for (int y = 0; y < ph; ++y)
    for (int x = 0; x < pw; ++x)
      if (a[size_t(y) * size_t(pw) + size_t(x)]) mask[size_t(y) * words + size_t(x >> 6)] |= uint64_t(1) << (x & 63);
}

uint32_t label_cpu(const uint64_t* mask, int pw, int ph, int min_area, uint32_t* labels, uint32_t* area, Record* records) {
  const size_t words = mask_words(uint32_t(pw)), n = size_t(pw) * size_t(ph);
  auto set = [&](int x, int y) { return (mask[size_t(y) * words + size_t(x >> 6)] >> (x & 63) & 1u) != 0; };
  std::fill(labels, labels + n, kBackground);
  std::fill(area, area + n, 0u);
  std::vector<uint32_t> stack;
  uint32_t count = 0;
  // A flood fill from every sample not yet reached, in raster order: its seed is the smallest index
  // of its component, and the records come out sorted by label.
  for (int sy = 0; sy < ph; ++sy)
    for (int sx = 0; sx < pw; ++sx) {
      const uint32_t seed = uint32_t(sy) * uint32_t(pw) + uint32_t(sx);
      if (!set(sx, sy) || labels[seed] != kBackground) continue;
      Record r{seed, 0, uint32_t(sx), uint32_t(sy), uint32_t(sx) + 1, uint32_t(sy) + 1};
      labels[seed] = seed;
      stack.assign(1, seed);
      while (!stack.empty()) {
        const uint32_t i = stack.back();
        stack.pop_back();
        const int y = int(i / uint32_t(pw)), x = int(i % uint32_t(pw));
        ++r.area;
        r.x0 = std::min(r.x0, uint32_t(x));
        r.y0 = std::min(r.y0, uint32_t(y));
        r.x1 = std::max(r.x1, uint32_t(x) + 1);
        r.y1 = std::max(r.y1, uint32_t(y) + 1);
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const int yy = y + dy, xx = x + dx;
            if (yy < 0 || yy >= ph || xx < 0 || xx >= pw || !set(xx, yy)) continue;
            const uint32_t k = uint32_t(yy) * uint32_t(pw) + uint32_t(xx);
            if (labels[k] != kBackground) continue;
            labels[k] = seed;
            stack.push_back(k);
          }
      }
      area[seed] = r.area;
      if (r.area >= uint32_t(min_area)) records[count++] = r;  // (count < capacity: the components are disjoint)
    }
  return count;
}

void objects_cpu(const Job& j) {
  check_job(j);
  const int pw = j.w / j.decimate, ph = j.h / j.decimate;
  const size_t pitch = flow::plane_pitch(uint32_t(pw));
  for (int k = 0; k < 2; ++k) flow::luma_plane_cpu(j.src[k], j.w, j.h, j.src_pitch[k], j.decimate, j.plane[k], pitch);
  mask_cpu(j.plane[0], j.plane[1], pw, ph, pitch, j.threshold, j.open, j.grow, j.mask);
  *j.count = label_cpu(j.mask, pw, ph, j.min_area, j.labels, j.area, j.records);
}

Summary summarize(const Record* sorted, size_t n, int decimate, int max_objects, int w, int h) {
  Summary s;
  s.count = int(n);
  s.motion = n >= 1;
  s.truncated = n > size_t(max_objects);
  std::vector<const Record*> by_area(n);
  uint32_t x0 = kBackground, y0 = kBackground, x1 = 0, y1 = 0;
  for (size_t i = 0; i < n; ++i) {
    const Record& r = sorted[i];
    VEP_CHECK(r.x0 < r.x1 && r.y0 < r.y1 && (i == 0 || sorted[i - 1].label < r.label), "objects: a record is malformed or out of order");
    by_area[i] = &r;
    s.area += r.area;
    x0 = std::min(x0, r.x0);
    y0 = std::min(y0, r.y0);
    x1 = std::max(x1, r.x1);
    y1 = std::max(y1, r.y1);
  }
  auto px = [&](uint32_t lo, uint32_t hi, int side, int& at, int& len) {
    at = int(std::min<uint64_t>(uint64_t(lo) * uint64_t(decimate), uint64_t(side)));
    len = int(std::min<uint64_t>(uint64_t(hi) * uint64_t(decimate), uint64_t(side))) - at;
  };
  if (n) {
    s.has_box = true;
    px(x0, x1, w, s.x, s.w);
    px(y0, y1, h, s.y, s.h);
  }
  const size_t top = std::min(n, size_t(max_objects));
  std::partial_sort(by_area.begin(), by_area.begin() + std::ptrdiff_t(top), by_area.end(),
                    [](const Record* a, const Record* b) { return a->area != b->area ? a->area > b->area : a->label < b->label; });
  for (size_t i = 0; i < top; ++i) {
    Object o;
    o.label = by_area[i]->label;
    o.area = by_area[i]->area;
    px(by_area[i]->x0, by_area[i]->x1, w, o.x, o.w);
    px(by_area[i]->y0, by_area[i]->y1, h, o.y, o.h);
    s.objects.push_back(o);
  }
  return s;
}

}  // namespace vep::objects
