// Stand-alone check of the CPU dehazing (vep/dehaze.cpp) for sanitizer builds (`make asan-dehaze`:
// AddressSanitizer + UndefinedBehaviorSanitizer on the host). Every picture lives in a heap buffer
// of exactly its size, so a read or write past a row or the picture is a report, and so is an
// overflow of the arithmetic. Pictures 16x16 (the window larger than the picture), partial cells and
// tiles, 700x300 and 65535x16, once more with a pitch wider than a row; the extreme parameters;
// random, extreme (0 / 255) and one-colour content. The arithmetic itself is held to
// tests/dehaze_oracle.py by tests/test_dehaze.py; here the header's closed forms and the job check
// are asserted. Exit status 0 and no sanitizer report = pass.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "vep/dehaze.h"

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

static void run(int w, int h, size_t pitch, const dehaze::Params& p, int kind) {
  const size_t bytes = size_t(h - 1) * pitch + size_t(w) * 3;
  std::unique_ptr<uint8_t[]> src(new uint8_t[bytes]), orig(new uint8_t[bytes]), dst(new uint8_t[bytes]);
  for (size_t i = 0; i < bytes; ++i) src[i] = uint8_t(kind == 0 ? rnd() : (kind == 1 ? (rnd() & 1 ? 255 : 0) : 77));
  std::memcpy(orig.get(), src.get(), bytes);
  std::memset(dst.get(), 0, bytes);
  uint32_t air[3];
  dehaze::dehaze_cpu(src.get(), pitch, dst.get(), pitch, w, h, p, air);
  check(std::memcmp(src.get(), orig.get(), bytes) == 0, "the source is not written", w, h);
  dehaze::dehaze_cpu(src.get(), pitch, src.get(), pitch, w, h, p);  // in place
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w * 3; ++x, ++compared) {
      const size_t at = size_t(y) * pitch + size_t(x);
      check(src[at] == dst[at], "in place equals out of place", w, h, x, y);
      if (p.strength == 0 || kind == 2) check(dst[at] == orig[at], "strength 0 and one colour are the identity", w, h, x, y);
      const int a = int(air[x % 3]), gain = (abs(int(orig[at]) - a) * 1024) / p.t0 + 1;
      if (p.strength == 256) check(abs(int(dst[at]) - a) <= gain, "t0 bounds the gain", w, h, x, y);
    }
}

int main() {
  const int pics[][2] = {{16, 16}, {67, 19}, {130, 34}, {257, 65}, {700, 300}, {65535, 16}};
  const dehaze::Params params[] = {{15, 243, 102, 8, 256}, {3, 256, 51, 1, 256}, {31, 0, 1024, 16, 128}, {31, 256, 51, 16, 0}};
  for (const auto& s : pics)
    for (const dehaze::Params& p : params)
      for (int kind = 0; kind < 3; ++kind) {
        if (s[0] > 1000 && (kind || p.patch != 15)) continue;  // (the widest picture once)
        run(s[0], s[1], size_t(s[0]) * 3, p, kind);
        run(s[0], s[1], size_t(s[0]) * 3 + 7, p, kind);
      }
  // the job check: parameters, sizes, spans, planes
  const int w = 40, h = 24;
  std::vector<uint8_t> a(size_t(w) * 3 * h), b(a.size());
  std::vector<uint64_t> planes(dehaze::plane_words(w, h) / 2);
  auto job = [&]() {
    dehaze::Job j;
    j.src = a.data();
    j.dst = b.data();
    j.src_bytes = j.dst_bytes = a.size();
    j.src_pitch = j.dst_pitch = uint32_t(w) * 3;
    j.w = w;
    j.h = h;
    dehaze::carve_planes(j, reinterpret_cast<uint32_t*>(planes.data()));
    return j;
  };
  int refused = 0, total = 0;
  auto refuse = [&](const dehaze::Job& j) {
    ++total;
    try {
      dehaze::check_job(j);
    } catch (const std::exception&) {
      ++refused;
    }
  };
  dehaze::check_job(job());  // the good one passes
  for (const dehaze::Params& p : {dehaze::Params{4, 243, 102, 8, 256}, dehaze::Params{33, 243, 102, 8, 256},
                                  dehaze::Params{15, 257, 102, 8, 256}, dehaze::Params{15, 243, 50, 8, 256},
                                  dehaze::Params{15, 243, 102, 0, 256}, dehaze::Params{15, 243, 102, 17, 256},
                                  dehaze::Params{15, 243, 102, 8, -1}}) {
    dehaze::Job j = job();
    j.p = p;
    refuse(j);
  }
  dehaze::Job j = job();
  j.w = 15;
  refuse(j);
  j = job(), j.src_bytes -= 1, refuse(j);
  j = job(), j.dst_bytes -= 1, refuse(j);
  j = job(), j.dst_pitch -= 1, refuse(j);
  j = job(), j.cell_words -= 1, refuse(j);
  j = job(), j.mean = j.ab, refuse(j);
  j = job(), j.dst = a.data() + 3, refuse(j);
  j = job(), j.table = reinterpret_cast<uint32_t*>(a.data()), refuse(j);
  j = job(), j.air += 1, refuse(j);
  j = job(), j.w = 4096, j.h = 4097, refuse(j);
  check(refused == total, "every bad job is refused", refused, total);
  std::printf("dehaze selftest: %ld bytes compared, %d failures\n", compared, failures);
  return failures ? 1 : 0;
}
