// Stand-alone check of the CPU deinterlacer (vep/deinterlace.cpp) for sanitizer builds (`make
// asan-deinterlace`: AddressSanitizer + UndefinedBehaviorSanitizer on the host). Every frame lives in
// a heap buffer of exactly its size, so a read or write past a row or the picture is a report, and
// so is an overflow of the arithmetic. Pictures 4x4, 5x7, 64x16, 67x19, 130x35 and 65535x4, once more
// with a pitch wider than a row; both orders; with and without the previous frame. The arithmetic
// itself is held to tests/deinterlace_oracle.py by tests/test_deinterlace.py; here the header's
// closed forms are asserted and check_job is seen to refuse what the kernel must never be given.
// Exit status 0 and no sanitizer report = pass.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <utility>

#include "vep/deinterlace.h"

using namespace vep;

static int failures = 0;
static long compared = 0;

static void check(bool ok, const char* what, int a = 0, int b = 0, int c = 0, int d = 0) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s (%d %d %d %d)\n", what, a, b, c, d);
  ++failures;
}

static uint32_t seed = 4711;
static uint32_t rnd() {
  seed = seed * 1664525u + 1013904223u;
  return seed >> 8;
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

static deinterlace::Job job_of(int w, int h, size_t pitch, size_t bytes, const uint8_t* f, const uint8_t* g, uint8_t* dst, int order) {
  deinterlace::Job j;
  j.newer = f;
  j.older = g;
  j.dst = dst;
  j.newer_bytes = j.older_bytes = j.dst_bytes = bytes;
  j.newer_pitch = j.older_pitch = j.dst_pitch = uint32_t(pitch);
  j.w = j.older_w = w;
  j.h = j.older_h = h;
  j.p.order = order;
  return j;
}

static void run(int w, int h, size_t pitch, int order) {
  const size_t bytes = size_t(h - 1) * pitch + size_t(w) * 3, row = size_t(w) * 3;
  std::unique_ptr<uint8_t[]> f(new uint8_t[bytes]), g(new uint8_t[bytes]), dst(new uint8_t[bytes]);
  for (size_t i = 0; i < bytes; ++i) f[i] = uint8_t(rnd()), g[i] = uint8_t(rnd());
  // G agrees with F on the left half of every row: there the output must be F's
  const int same = w / 2;
  for (int y = 0; y < h; ++y) std::memcpy(g.get() + size_t(y) * pitch, f.get() + size_t(y) * pitch, size_t(same) * 3);
  for (int mode = 0; mode < 3; ++mode) {  // 0: with G; 1: without; 2: G == F
    std::memset(dst.get(), 0, bytes);
    const uint8_t* older = mode == 0 ? g.get() : (mode == 1 ? nullptr : f.get());
    deinterlace::deinterlace_cpu(job_of(w, h, pitch, bytes, f.get(), older, dst.get(), order));
    for (int y = 0; y < h; ++y) {
      const uint8_t* a = f.get() + size_t(y) * pitch;
      const uint8_t* o = dst.get() + size_t(y) * pitch;
      const size_t must = (y & 1) == order || mode == 2 ? row : (mode == 0 ? size_t(same) * 3 : 0);
      check(std::memcmp(a, o, must) == 0, "kept rows, and pixels where F and G agree, equal F", w, h, y, mode);
      ++compared;
    }
  }
  // temporal 0 with a previous frame is the spatial prediction alone
  std::unique_ptr<uint8_t[]> lone(new uint8_t[bytes]);
  std::memset(lone.get(), 0, bytes);
  std::memset(dst.get(), 0, bytes);
  deinterlace::Job j = job_of(w, h, pitch, bytes, f.get(), g.get(), dst.get(), order);
  j.p.temporal = 0;
  deinterlace::deinterlace_cpu(j);
  deinterlace::deinterlace_cpu(job_of(w, h, pitch, bytes, f.get(), nullptr, lone.get(), order));
  for (int y = 0; y < h; ++y)
    check(std::memcmp(dst.get() + size_t(y) * pitch, lone.get() + size_t(y) * pitch, row) == 0, "temporal 0 is spatial only", w, h, y);
}

int main() {
  // the cascade: ties keep 0, -2 only behind -1, +1 against the best so far
  check(deinterlace::direction(0, 5, 5, 5, 0) == 0, "a tie keeps direction 0");
  check(deinterlace::direction(0, 5, 6, 5, 0) == 0, "score - 1: one less is not enough");
  check(deinterlace::direction(9, 4, 6, 9, 9) == -1 && deinterlace::direction(3, 4, 6, 9, 9) == -2, "-1, then -2");
  check(deinterlace::direction(0, 6, 6, 4, 9) == 1 && deinterlace::direction(0, 6, 6, 4, 3) == 2, "-2 only behind -1");
  check(deinterlace::direction(9, 3, 6, 3, 0) == -1 && deinterlace::direction(9, 3, 6, 2, 9) == 1, "+1 against the best so far");
  // the bound's whole range: inside 0..255 without a clamp, and the identity where diff is 0
  for (uint32_t pred = 0; pred < 256; pred += 5)
    for (uint32_t g = 0; g < 256; g += 3)
      for (uint32_t f = 0; f < 256; f += 7)
        for (uint32_t diff = 0; diff < 256; diff += 15) {
          const uint32_t v = deinterlace::bound(pred, g, f, diff);
          check(v <= 255u, "bound stays a byte", int(pred), int(g), int(f), int(diff));
          if (diff == 0) check(v == ((g + f) >> 1), "diff 0 returns d", int(pred), int(g), int(f));
        }
  for (int order = 0; order < 2; ++order)
    for (const auto& s : {std::pair<int, int>{4, 4}, {5, 7}, {64, 16}, {67, 19}, {130, 35}, {65535, 4}, {4, 4099}})
      for (size_t extra : {size_t(0), size_t(7)}) run(s.first, s.second, size_t(s.first) * 3 + extra, order);

  uint8_t buf[3][4 * 4 * 3] = {};
  const deinterlace::Job good = job_of(4, 4, 12, 48, buf[0], buf[1], buf[2], 0);
  check(!throws([&] { deinterlace::check_job(good); }), "a good job passes");
  auto refused = [&](const char* what, auto&& change) {
    deinterlace::Job j = good;
    change(j);
    check(throws([&] { deinterlace::check_job(j); }), what);
  };
  refused("side 3", [](deinterlace::Job& j) { j.w = j.older_w = 3; });
  refused("side 65536", [](deinterlace::Job& j) { j.h = j.older_h = 65536; });
  refused("a previous frame of another size", [](deinterlace::Job& j) { j.older_h = 6; });
  refused("short pitch", [](deinterlace::Job& j) { j.newer_pitch = 11; });
  refused("short memory", [](deinterlace::Job& j) { j.older_bytes = 47; });
  refused("short output", [](deinterlace::Job& j) { j.dst_bytes = 47; });
  refused("null output", [](deinterlace::Job& j) { j.dst = nullptr; });
  refused("null frame", [](deinterlace::Job& j) { j.newer = nullptr; });
  refused("in place", [](deinterlace::Job& j) { j.dst = const_cast<uint8_t*>(j.newer); });
  refused("output over the previous frame", [](deinterlace::Job& j) { j.dst = const_cast<uint8_t*>(j.older) + 12; });
  refused("order 2", [](deinterlace::Job& j) { j.p.order = 2; });
  refused("temporal 2", [](deinterlace::Job& j) { j.p.temporal = 2; });

  std::printf("deinterlace selftest: %ld rows compared, %d failures\n", compared, failures);
  return failures ? 1 : 0;
}
