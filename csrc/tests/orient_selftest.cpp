// Stand-alone check of the CPU orientation (vep/orient.cpp) for sanitizer builds (`make
// asan-orient`: AddressSanitizer + UndefinedBehaviorSanitizer on the host). Source and destination
// live in heap buffers of exactly their size, so a read or write past a row or the picture is a
// report. Pictures 1x1, 1x7, 7x1, 5x3, 67x19 and 65535x2, once more with pitches wider than a row;
// all eight ops. Every output pixel is held to the header's map, the map is seen to be a bijection,
// the composition table is held to applying two ops one after the other, and check_job is seen to
// refuse what the kernel must never be given. Exit status 0 and no sanitizer report = pass.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "vep/orient.h"

using namespace vep;

static int failures = 0;
static long compared = 0;

static void check(bool ok, const char* what, int a = 0, int b = 0, int c = 0, int d = 0) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s (%d %d %d %d)\n", what, a, b, c, d);
  ++failures;
}

template <class F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const std::exception&) {
    return true;
  }
  return false;
}

struct Picture {
  int w, h;
  size_t pitch, bytes;
  std::unique_ptr<uint8_t[]> p;
  Picture(int w_, int h_, size_t extra) : w(w_), h(h_), pitch(size_t(w_) * 3 + extra), bytes(size_t(h_ - 1) * pitch + size_t(w_) * 3), p(new uint8_t[bytes]) {
    std::memset(p.get(), 0, bytes);
  }
};

static orient::Job job_of(const Picture& s, Picture& d, int op) {
  orient::Job j;
  j.src = s.p.get();
  j.dst = d.p.get();
  j.src_bytes = s.bytes;
  j.dst_bytes = d.bytes;
  j.src_pitch = uint32_t(s.pitch);
  j.dst_pitch = uint32_t(d.pitch);
  j.w = s.w;
  j.h = s.h;
  j.op = op;
  return j;
}

static Picture apply(const Picture& s, int op, size_t extra) {
  Picture d(orient::out_w(op, s.w, s.h), orient::out_h(op, s.w, s.h), extra);
  orient::apply_cpu(job_of(s, d, op));
  return d;
}

static bool same(const Picture& a, const Picture& b) {
  if (a.w != b.w || a.h != b.h) return false;
  for (int y = 0; y < a.h; ++y)
    if (std::memcmp(a.p.get() + size_t(y) * a.pitch, b.p.get() + size_t(y) * b.pitch, size_t(a.w) * 3)) return false;
  return true;
}

static void run(int w, int h, size_t extra) {
  Picture s(w, h, extra);
  uint32_t seed = uint32_t(w * 131 + h);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w * 3; ++x) s.p[size_t(y) * s.pitch + size_t(x)] = uint8_t((seed = seed * 1664525u + 1013904223u) >> 24);
  for (int op = 0; op < 8; ++op) {
    const Picture d = apply(s, op, extra ? extra + 2 : 0);
    check(d.w == (op & orient::kT ? h : w) && d.h == (op & orient::kT ? w : h), "output size", w, h, op);
    std::vector<uint8_t> hit(size_t(w) * size_t(h), 0);
    for (int oy = 0; oy < d.h; ++oy)
      for (int ox = 0; ox < d.w; ++ox) {
        int sx, sy;
        orient::source_of(op, d.w, d.h, ox, oy, sx, sy);
        const bool inside = sx >= 0 && sx < w && sy >= 0 && sy < h;
        check(inside, "the map stays inside the source", w, h, op);
        if (!inside) continue;
        ++hit[size_t(sy) * size_t(w) + size_t(sx)];
        check(std::memcmp(d.p.get() + size_t(oy) * d.pitch + size_t(ox) * 3, s.p.get() + size_t(sy) * s.pitch + size_t(sx) * 3, 3) == 0,
              "out(oy, ox) == src(sy, sx)", w, h, op, ox);
        ++compared;
      }
    for (uint8_t n : hit) check(n == 1, "the map is a bijection", w, h, op, n);
    if (w > 4096) continue;  // (the composition on the small pictures)
    for (int b = 0; b < 8; ++b) check(same(apply(d, b, 0), apply(s, orient::compose(op, b), 0)), "compose(a, b) is a, then b", w, h, op, b);
  }
}

int main() {
  // every request reaches a group element, and all eight are reached
  int seen = 0;
  for (int rotate : {0, 90, 180, 270})
    for (int flip : {orient::kNone, orient::kH, orient::kV}) {
      const int op = orient::of(rotate, flip);
      check(op >= 0 && op < 8, "a request is an op", rotate, flip);
      seen |= 1 << op;
    }
  check(seen == 0xff, "all eight ops are reachable", seen);
  check(orient::of(45, 0) < 0 && orient::of(-90, 0) < 0 && orient::of(90, 3) < 0 && orient::of(0, -1) < 0, "bad requests are none");
  int op = 0;
  for (int k = 0; k < 4; ++k) op = orient::compose(op, orient::of(90, orient::kNone));
  check(op == 0, "rotate 90 four times is the identity");
  check(orient::compose(orient::of(0, orient::kH), orient::of(0, orient::kV)) == orient::of(180, orient::kNone), "180 is h then v");
  for (int a = 0; a < 8; ++a) {
    int inverse = 0;
    for (int b = 0; b < 8; ++b) inverse += orient::compose(a, b) == 0;
    check(inverse == 1 && orient::compose(a, 0) == a && orient::compose(0, a) == a, "a group: identity and inverses", a);
  }
  for (const auto& s : {std::pair<int, int>{1, 1}, {1, 7}, {7, 1}, {5, 3}, {67, 19}, {65535, 2}})
    for (size_t extra : {size_t(0), size_t(7)}) run(s.first, s.second, extra);

  uint8_t buf[2][5 * 3 * 3] = {};
  orient::Job good;
  good.src = buf[0];
  good.dst = buf[1];
  good.src_bytes = good.dst_bytes = 45;
  good.src_pitch = 15;
  good.dst_pitch = 9;
  good.w = 5;
  good.h = 3;
  good.op = orient::of(90, orient::kNone);
  check(!throws([&] { orient::check_job(good); }), "a good job passes");
  auto refused = [&](const char* what, auto&& change) {
    orient::Job j = good;
    change(j);
    check(throws([&] { orient::check_job(j); }), what);
  };
  refused("side 0", [](orient::Job& j) { j.w = 0; });
  refused("side 65536", [](orient::Job& j) { j.h = 65536; });
  refused("op 8", [](orient::Job& j) { j.op = 8; });
  refused("short source pitch", [](orient::Job& j) { j.src_pitch = 14; });
  refused("short destination pitch: the output's rows are 3 pixels", [](orient::Job& j) { j.dst_pitch = 8; });
  refused("short source", [](orient::Job& j) { j.src_bytes = 44; });
  refused("short destination", [](orient::Job& j) { j.dst_bytes = 44; });
  refused("a destination sized for the source's shape", [](orient::Job& j) { j.dst_pitch = 15; });  // 5 rows of 15 > 45
  refused("null output", [](orient::Job& j) { j.dst = nullptr; });
  refused("null picture", [](orient::Job& j) { j.src = nullptr; });
  refused("in place", [](orient::Job& j) { j.dst = const_cast<uint8_t*>(j.src); });
  refused("overlap by one byte", [](orient::Job& j) { j.dst = const_cast<uint8_t*>(j.src) + 44; });

  std::printf("orient selftest: %ld pixels compared, %d failures\n", compared, failures);
  return failures ? 1 : 0;
}
