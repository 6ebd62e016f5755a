// Stand-alone check of the CPU JPEG encoder (vep/jpeg.cpp) for sanitizer builds (`make
// asan-jpeg`: AddressSanitizer + UndefinedBehaviorSanitizer on the host): the inputs that drive
// the encoder to its limits — the largest coefficient categories and the clamps (1-pixel
// checkerboard), byte stuffing and the worst-case segment size (noise), EOB-only blocks
// (constant), edge replication in both directions (1x1, 17x9) — at the ends of the quality range.
// Exit status 0 and no sanitizer report = pass.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "vep/jpeg.h"

using namespace vep;

static int failures = 0;

static void check(bool ok, const char* what, int w, int h, int q) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s (%dx%d q%d)\n", what, w, h, q);
  ++failures;
}

static void run(const char* name, const std::vector<uint8_t>& px, int w, int h) {
  for (int q : {1, 50, 100}) {
    const std::string a = jpeg::encode_cpu(px.data(), w, h, q);
    const std::string b = jpeg::encode_cpu(px.data(), w, h, q);
    const std::string head = jpeg::header(w, h, q);
    const int n = jpeg::intervals(jpeg::mcus_x(w) * jpeg::mcus_y(h));
    check(a == b, "deterministic", w, h, q);
    check(a.size() > head.size() + 2 && a.compare(0, head.size(), head) == 0, "starts with the header", w, h, q);
    check(uint8_t(a[a.size() - 2]) == 0xff && uint8_t(a.back()) == 0xd9, "ends with EOI", w, h, q);
    check(a.size() <= head.size() + size_t(n) * (jpeg::kSegmentCap + 2), "within the proven worst case", w, h, q);
    int rst = 0;  // RSTm markers in order, none missing
    for (size_t i = head.size(); i + 1 < a.size(); ++i)
      if (uint8_t(a[i]) == 0xff && uint8_t(a[i + 1]) >= 0xd0 && uint8_t(a[i + 1]) <= 0xd7) {
        check(uint8_t(a[i + 1]) == jpeg::rst_marker(rst), "RSTm order", w, h, q);
        ++rst;
      }
    check(rst == n - 1, "one RSTm between intervals", w, h, q);
    std::printf("%-14s %4dx%-4d q%-3d %7zu bytes, %d intervals\n", name, w, h, q, a.size(), n);
  }
}

int main() {
  uint32_t s = 12345;
  auto rnd = [&] {
    s = s * 1664525u + 1013904223u;
    return uint8_t(s >> 24);
  };
  for (auto [w, h] : {std::pair<int, int>{64, 48}, {17, 9}, {1, 1}, {200, 120}}) {
    std::vector<uint8_t> px(size_t(w) * h * 3);
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x)
        for (int c = 0; c < 3; ++c) px[(size_t(y) * w + x) * 3 + c] = ((x + y) & 1) ? 255 : 0;
    run("checkerboard", px, w, h);
    for (auto& v : px) v = rnd();
    run("noise", px, w, h);
    for (auto& v : px) v = 77;
    run("constant", px, w, h);
    for (size_t i = 0; i < px.size(); ++i) px[i] = (i / 3) % 2 ? 255 : 0;  // columns (or rows) of 0 / 255
    run("stripes", px, w, h);
  }
  // bad arguments throw, they do not read or write out of bounds
  for (int q : {0, 101}) {
    try {
      std::vector<uint8_t> px(3);
      jpeg::encode_cpu(px.data(), 1, 1, q);
      check(false, "quality out of range rejected", 1, 1, q);
    } catch (const std::exception&) {
    }
  }
  if (failures) return 1;
  std::puts("jpeg_selftest ok");
  return 0;
}
