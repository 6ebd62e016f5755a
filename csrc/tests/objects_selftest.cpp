// Stand-alone check of the moving-object boxes' CPU twin (vep/objects.h), host only: hand-made
// pictures whose components are known, the job check's refusals, the capacity bound and the
// summary. `make objects-selftest` links it against the objects csrc/build.py made; `make
// asan-objects` builds it from sources under AddressSanitizer + UndefinedBehaviorSanitizer. Exit
// status 0 and no sanitizer report = pass.
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "vep/common.h"
#include "vep/objects.h"

using namespace vep;

static int failures = 0;

#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #cond); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

// A job on buffers of exactly the sizes check_job asks for (so the sanitizer sees any byte past them).
struct Case {
  int w, h, d, min_area;
  std::vector<u8> newer, older, planes;
  std::vector<u64> mask;
  std::vector<u32> labels, area;
  std::vector<objects::Record> records;
  u32 count = 77;
  objects::Job j;
  Case(int w_, int h_, int d_, int min_area_, int threshold, int open, int grow) : w(w_), h(h_), d(d_), min_area(min_area_) {
    const u32 pw = u32(w / d), ph = u32(h / d);
    newer.assign(size_t(w) * size_t(h) * 3, 0);
    older.assign(newer.size(), 0);
    const size_t half = size_t(flow::plane_pitch(pw)) * ph;
    planes.assign(2 * half + 16, 0);
    mask.assign(size_t(objects::mask_words(pw)) * ph + 1, 0);
    labels.assign(size_t(pw) * ph + 1, 0);
    area.assign(size_t(pw) * ph + 1, 0);
    records.assign(size_t(objects::capacity(pw, ph, u32(min_area))) + 1, objects::Record{});
    u8* base = planes.data() + ((16 - (reinterpret_cast<uintptr_t>(planes.data()) & 15u)) & 15u);
    j.src[0] = newer.data();
    j.src[1] = older.data();
    for (int k = 0; k < 2; ++k) {
      j.src_bytes[k] = newer.size();
      j.src_pitch[k] = u32(w) * 3;
      j.plane[k] = base + size_t(k) * half;
      j.plane_bytes[k] = half;
    }
    j.mask = mask.data();
    j.mask_count = mask.size() - 1;
    j.labels = labels.data();
    j.area = area.data();
    j.sample_count = size_t(pw) * ph;
    j.records = records.data();
    j.record_count = records.size() - 1;
    j.count = &count;
    j.w = w;
    j.h = h;
    j.decimate = d;
    j.threshold = threshold;
    j.open = open;
    j.grow = grow;
    j.min_area = min_area;
  }
  void set(int x, int y) { std::memset(newer.data() + (size_t(y) * size_t(w) + size_t(x)) * 3, 255, 3); }
  u32 label(int x, int y) const { return labels[size_t(y) * size_t(w / d) + size_t(x)]; }
};

static bool same(const objects::Record& r, u32 label, u32 area, u32 x0, u32 y0, u32 x1, u32 y1) {
  return r.label == label && r.area == area && r.x0 == x0 && r.y0 == y0 && r.x1 == x1 && r.y1 == y1;
}

static void twin() {
  {  // two squares that touch only diagonally are one component; a third apart is another; a speck is dropped
    Case c(20, 10, 1, 4, 0, 0, 0);
    for (int y = 0; y < 2; ++y)
      for (int x = 0; x < 2; ++x) {
        c.set(3 + x, 1 + y);
        c.set(5 + x, 3 + y);
        c.set(12 + x, 6 + y);
      }
    c.set(19, 9);
    objects::objects_cpu(c.j);
    CHECK(c.count == 2 && same(c.records[0], 23, 8, 3, 1, 7, 5) && same(c.records[1], 132, 4, 12, 6, 14, 8));
    CHECK(c.label(6, 4) == 23 && c.label(13, 7) == 132 && c.label(19, 9) == 199 && c.label(0, 0) == objects::kBackground);
    CHECK(c.mask[1] == (u64(3) << 3) && c.mask[3] == (u64(3) << 5) && c.mask[9] == (u64(1) << 19));
  }
  {  // the opening removes the speck and keeps the 3 x 3 square at the border (what lies outside the
     // plane is background, so the erosion leaves its centre alone); grow 1 makes it 5 x 5, clipped to 4 x 5
    Case c(16, 8, 1, 4, 0, 1, 1);
    for (int y = 0; y < 3; ++y)
      for (int x = 0; x < 3; ++x) c.set(x, 4 + y);
    c.set(10, 2);
    objects::objects_cpu(c.j);
    CHECK(c.count == 1 && same(c.records[0], 48, 20, 0, 3, 4, 8));
  }
  {  // a full plane at the capacity bound: 2 x 2 samples of 2 x 2 pixels, min_area 4
    Case c(5, 4, 2, 4, 254, 0, 0);
    for (int y = 0; y < 4; ++y)
      for (int x = 0; x < 4; ++x) c.set(x, y);
    CHECK(objects::capacity(2, 2, 4) == 1);
    objects::objects_cpu(c.j);
    CHECK(c.count == 1 && same(c.records[0], 0, 4, 0, 0, 2, 2) && c.records[1].area == 0);
    c.j.threshold = 255;  // nothing differs by more than 255
    objects::objects_cpu(c.j);
    CHECK(c.count == 0 && c.mask[0] == 0 && c.label(1, 1) == objects::kBackground);
  }
  {  // isolated 2 x 2 blocks on a stride of three: the most records there can be, below the bound
    Case c(65, 33, 1, 4, 0, 0, 0);
    for (int y = 0; y < 33; ++y)
      for (int x = 0; x < 65; ++x)
        if (x % 3 < 2 && y % 3 < 2) c.set(x, y);
    objects::objects_cpu(c.j);
    CHECK(c.count == 22 * 11 && u64(c.count) <= objects::capacity(65, 33, 4));
    for (u32 k = 1; k < c.count; ++k) CHECK(c.records[k - 1].label < c.records[k].label && c.records[k].area == 4);
  }
}

static bool refused(const std::function<void(Case&)>& spoil) {
  Case c(20, 10, 2, 4, 24, 1, 1);
  spoil(c);
  try {
    objects::check_job(c.j);
  } catch (const Error&) {
    return true;
  }
  return false;
}

static void refusals() {
  CHECK(!refused([](Case&) {}));
  CHECK(refused([](Case& c) { c.j.decimate = 3; }));
  CHECK(refused([](Case& c) { c.j.threshold = 256; }));
  CHECK(refused([](Case& c) { c.j.open = 2; }));
  CHECK(refused([](Case& c) { c.j.grow = 4; }));
  CHECK(refused([](Case& c) { c.j.min_area = 3; }));
  CHECK(refused([](Case& c) { c.j.w = 0; }));
  CHECK(refused([](Case& c) { c.j.src_pitch[1] = 59; }));
  CHECK(refused([](Case& c) { c.j.src_bytes[0] -= 1; }));
  CHECK(refused([](Case& c) { c.j.plane[0] += 1; }));
  CHECK(refused([](Case& c) { c.j.plane_bytes[1] -= 1; }));
  CHECK(refused([](Case& c) { c.j.mask_count -= 1; }));
  CHECK(refused([](Case& c) { c.j.sample_count -= 1; }));
  CHECK(refused([](Case& c) { c.j.record_count -= 1; }));  // below the capacity bound
  CHECK(refused([](Case& c) { c.j.count = nullptr; }));
  CHECK(refused([](Case& c) { c.j.area = c.j.labels + 1; }));
  CHECK(refused([](Case& c) { c.j.count = &c.j.labels[3]; }));
  CHECK(refused([](Case& c) { c.j.plane[1] = c.j.plane[0]; }));
  CHECK(refused([](Case& c) { c.j.labels = reinterpret_cast<u32*>(c.newer.data()); }));
}

static void summary() {
  const objects::Record r[3] = {{5, 10, 1, 1, 4, 3}, {9, 30, 8, 2, 12, 9}, {20, 10, 30, 30, 32, 33}};
  const objects::Summary s = objects::summarize(r, 3, 2, 2, 63, 65);
  CHECK(s.count == 3 && s.truncated && s.motion && s.area == 50 && s.objects.size() == 2);
  CHECK(s.objects[0].label == 9 && s.objects[1].label == 5 && s.objects[0].x == 16 && s.objects[0].w == 8);
  CHECK(s.has_box && s.x == 2 && s.y == 2 && s.w == 61 && s.h == 63);  // clipped to 63 x 65
  const objects::Summary none = objects::summarize(r, 0, 2, 2, 63, 65);
  CHECK(none.count == 0 && !none.motion && !none.has_box && none.objects.empty());
  bool threw = false;
  const objects::Record bad[2] = {r[1], r[0]};
  try {
    objects::summarize(bad, 2, 2, 2, 63, 65);
  } catch (const Error&) {
    threw = true;
  }
  CHECK(threw);
}

int main() {
  twin();
  refusals();
  summary();
  if (failures) {
    std::fprintf(stderr, "objects_selftest: %d failures\n", failures);
    return 1;
  }
  std::printf("objects_selftest ok\n");
  return 0;
}
