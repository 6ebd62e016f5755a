// Stand-alone check of the CPU temporal denoise (vep/denoise.cpp) for sanitizer builds (`make
// asan-denoise`: AddressSanitizer + UndefinedBehaviorSanitizer on the host). Every frame lives in a
// heap buffer of exactly its size, so a read or write past a row or the picture is a report, and so
// is an overflow of the arithmetic. Pictures 1x1, 1x7, 2x2, 9x9, 65x33, 129x17 and 65535x1, once
// more with a pitch wider than a row; K 1, 2, 3 and 8; the extreme levels and strengths; random,
// noisy and one-colour content. The arithmetic itself is held to tests/denoise_oracle.py by
// tests/test_denoise.py; here the header's closed forms are asserted, the reciprocals that replace
// the kernel's two divisions are proved exact over their whole ranges, and check_job is seen to
// refuse what the kernel must never be given. Exit status 0 and no sanitizer report = pass.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "vep/denoise.h"

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

// kind 0: random frames; 1: one base picture plus noise of up to 4 * level; 2: identical frames.
static void run(int w, int h, size_t pitch, int frames, int level, int strength, int kind) {
  const size_t bytes = size_t(h - 1) * pitch + size_t(w) * 3;
  std::vector<std::unique_ptr<uint8_t[]>> src;
  std::unique_ptr<uint8_t[]> base(new uint8_t[bytes]), dst(new uint8_t[bytes]), lone(new uint8_t[bytes]);
  for (size_t i = 0; i < bytes; ++i) base[i] = uint8_t(rnd());
  denoise::Job j;
  j.frames = frames;
  for (int k = 0; k < frames; ++k) {
    src.emplace_back(new uint8_t[bytes]);
    for (size_t i = 0; i < bytes; ++i) {
      const int noise = kind == 1 ? int(rnd() % uint32_t(8 * level + 1)) - 4 * level : 0;
      const int v = kind == 0 ? int(rnd() & 255u) : int(base[i]) + noise;
      src.back()[i] = uint8_t(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
    j.src[k] = src.back().get();
    j.src_bytes[k] = bytes;
    j.src_pitch[k] = uint32_t(pitch);
  }
  std::memset(dst.get(), 0, bytes);
  j.dst = dst.get();
  j.dst_bytes = bytes;
  j.dst_pitch = uint32_t(pitch);
  j.w = w;
  j.h = h;
  j.level = level;
  j.strength = strength;
  denoise::denoise_cpu(j);
  denoise::Job one = j;  // K = 1
  one.frames = 1;
  one.dst = lone.get();
  denoise::denoise_cpu(one);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w * 3; ++x, ++compared) {
      const size_t at = size_t(y) * pitch + size_t(x);
      check(lone[at] == src[0][at], "K = 1 is the identity", w, h, x, y);
      if (strength == 0 || kind == 2) check(dst[at] == src[0][at], "strength 0 and identical frames are the identity", w, h, x, y);
      uint8_t lo = 255, hi = 0;
      for (int k = 0; k < frames; ++k) {
        lo = src[size_t(k)][at] < lo ? src[size_t(k)][at] : lo;
        hi = src[size_t(k)][at] > hi ? src[size_t(k)][at] : hi;
      }
      check(dst[at] >= lo && dst[at] <= hi, "the output lies between the frames' minimum and maximum", w, h, x, y);
    }
}

int main() {
  const int pics[][2] = {{1, 1}, {1, 7}, {2, 2}, {9, 9}, {65, 33}, {129, 17}, {65535, 1}};
  const int params[][3] = {{1, 1, 256}, {2, 8, 256}, {3, 64, 128}, {8, 8, 256}, {8, 1, 1}, {4, 24, 0}};  // K, T, S
  for (const auto& s : pics)
    for (const auto& p : params)
      for (int kind = 0; kind < 3; ++kind) {
        run(s[0], s[1], size_t(s[0]) * 3, p[0], p[1], p[2], kind);
        run(s[0], s[1], size_t(s[0]) * 3 + 7, p[0], p[1], p[2], kind);
      }
  // Two one-colour frames within T of each other: the rounded mean. Further apart than 2 T: the newest alone.
  {
    const int w = 5, h = 4;
    std::vector<uint8_t> a(size_t(w * h * 3)), b(a.size()), c(a.size()), out(a.size());
    for (size_t i = 0; i < a.size(); i += 3) {
      a[i] = 10, a[i + 1] = 100, a[i + 2] = 201;  // luma 120
      b[i] = 13, b[i + 1] = 107, b[i + 2] = 196;  // luma 123
      c[i] = 30, c[i + 1] = 120, c[i + 2] = 221;  // luma 140
    }
    denoise::Job j;
    j.frames = 2;
    j.src[0] = a.data();
    j.src[1] = b.data();
    j.src_bytes[0] = j.src_bytes[1] = j.dst_bytes = a.size();
    j.src_pitch[0] = j.src_pitch[1] = j.dst_pitch = uint32_t(w) * 3;
    j.dst = out.data();
    j.w = w;
    j.h = h;
    j.level = 8;
    j.strength = 256;
    denoise::denoise_cpu(j);
    for (size_t i = 0; i < out.size(); i += 3)
      check(out[i] == 12 && out[i + 1] == 104 && out[i + 2] == 199, "within T: the rounded mean", int(i));
    j.src[1] = c.data();
    denoise::denoise_cpu(j);
    check(out == a, "further apart than 2 T: contributes nothing");
    // check_job: what the kernel must never be given
    const denoise::Job good = j;
    check(!throws([&] { denoise::check_job(good); }), "a good job passes");
    auto refused = [&](const char* what, auto&& spoil) {
      denoise::Job bad = good;
      spoil(bad);
      check(throws([&] { denoise::check_job(bad); }), what);
    };
    refused("the destination is a source", [&](denoise::Job& x) { x.dst = a.data(); });
    refused("the destination overlaps a source's end", [&](denoise::Job& x) { x.dst = c.data() + c.size() - 1, x.dst_bytes = a.size(); });
    refused("a pitch past the frame's memory", [&](denoise::Job& x) { x.src_pitch[1] = uint32_t(w) * 3 + 1; });
    refused("a pitch shorter than a row", [&](denoise::Job& x) { x.src_pitch[0] = uint32_t(w) * 3 - 1; });
    refused("K = 9", [&](denoise::Job& x) { x.frames = 9; });
    refused("T = 0", [&](denoise::Job& x) { x.level = 0; });
    refused("S = 257", [&](denoise::Job& x) { x.strength = 257; });
  }
  // The kernel's divisions by their reciprocals, over the whole ranges: every d and T, every
  // strength's weight; every W and every channel sum it can meet.
  for (uint32_t t = denoise::kMinLevel; t <= uint32_t(denoise::kMaxLevel); ++t) {
    const uint32_t r = denoise::reciprocal(9 * t);
    for (uint32_t d = 0; d <= denoise::kMaxDistance; ++d) {
      check(denoise::div_by(d * 16, r) == d * 16 / (9 * t), "16 d / 9 T by its reciprocal", int(d), int(t));
      for (uint32_t s : {0u, 1u, 128u, 255u, 256u})
        check(denoise::weight_fast(d, r, s) == denoise::weight(d, t, s), "the weight by the reciprocal", int(d), int(t), int(s));
    }
  }
  constexpr denoise::WeightSumTable table = denoise::weight_sum_table();
  for (uint32_t w = denoise::kFull; w <= denoise::kMaxWeightSum; ++w)
    for (uint32_t n = 0; n <= w * 255; ++n)
      check(denoise::div_by(n + w / 2, table.r[w]) == denoise::mean(n, w), "(sum + W / 2) / W by the table", int(n), int(w));
  std::printf("denoise selftest: %ld bytes compared, %d failures\n", compared, failures);
  return failures ? 1 : 0;
}
