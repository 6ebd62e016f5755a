// Baseline JPEG stream of the frame server: one definition of the format and of every piece of
// arithmetic, shared by the CPU encoder (jpeg.cpp) and the gfx950 kernels (gpu_jpeg.hip), so both
// produce the same bytes. docs/JPEG.md has the reasoning.
//
// Stream: JFIF 1.01, baseline sequential DCT (SOF0), 8 bit, three components, 4:2:0 (Y 2x2,
// Cb 1x1, Cr 1x1), 16x16 MCUs in raster order, blocks per MCU: Y00 Y01 Y10 Y11 Cb Cr.
//
// Colour (BGR24 -> full-range BT.601 YCbCr, the JFIF definition), 16.16 fixed point:
//   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//   Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
//   Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
// (>> of a negative value is an arithmetic shift everywhere below). Every result is in 0..255
// without a clamp. A chroma sample is the rounded mean of the 2x2 converted samples,
// (a + b + c + d + 2) >> 2. Samples past the right / bottom edge replicate the last column / row
// (before conversion, so the mean of replicated samples is the sample).
//
// FDCT of the level-shifted (-128) samples, integer, separable, with the orthonormal DCT-II
// matrix scaled by 2^13 (kDct):
//   rows:    t[y][u] = (sum_x kDct[u][x] * p[y][x] + 512) >> 10      (3 fraction bits)
//   columns: d[v][u] =  sum_y kDct[v][y] * t[y][u]                   (16 fraction bits)
// |t| <= 4017 and |d| < 2^27, so everything fits 32 bits. Quantiser: round half away from zero,
//   q = sign(d) * ((|d| + (Q << 15)) / (Q << 16))
// then AC clamped to +-1023, and the DC difference to +-2047 (the predictor follows the clamped
// value, as a decoder does), so every value has a Huffman code.
//
// Quantisation tables: Annex K.1 / K.2 scaled by the IJG rule (quant_entry). Huffman tables:
// Annex K.3. Restart interval kRestartInterval MCUs: DC prediction restarts and the bit stream is
// padded with 1-bits to a byte at the end of every interval; RSTm (m cycling 0..7) separates
// intervals. A 0x00 byte follows every 0xFF byte of entropy data.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VEP_JPEG_HD __host__ __device__
#else
#define VEP_JPEG_HD
#endif

namespace vep::jpeg {

// MCUs per restart interval. 3 gives a 1080p picture (8160 MCUs) 2720 independently coded
// intervals for the GPU's entropy pass at ~2.5 bytes of marker and padding each.
constexpr int kRestartInterval = 3;
constexpr int kMcu = 16;
constexpr int kBlocksPerMcu = 6;
constexpr int kCoefsPerMcu = kBlocksPerMcu * 64;

// Worst case of one interval's entropy bytes. Every coefficient position costs at most 26 bits
// (longest AC code 16 + 10 value bits; a ZRL code covers 16 positions, EOB at least one; DC: at
// most 9 + 11), so a block is at most 64 * 26 bits = 208 bytes whole, an MCU 1248, and byte
// stuffing at most doubles that. Padding fills the last byte, it never adds one to this bound.
constexpr int kMaxBlockBytes = 64 * 26 / 8;
constexpr int kSegmentCap = kRestartInterval * kBlocksPerMcu * kMaxBlockBytes * 2;
static_assert(kSegmentCap == 7488 && kSegmentCap % 16 == 0, "segment capacity");

constexpr uint8_t kLumaQuant[64] = {
    16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
    14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
    18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kChromaQuant[64] = {
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
    99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// zigzag index -> natural (row-major) position
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// round(2^13 * c(u) / 2 * cos((2x + 1) u pi / 16)), c(0) = 1 / sqrt(2), c(u > 0) = 1
constexpr int16_t kDct[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},
                                {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                                {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784},
                                {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                                {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896},
                                {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                                {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567},
                                {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};

// Annex K.3 Huffman specifications: codes per length 1..16, then the symbols in code order.
constexpr uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// Encoder tables derived from the specifications (Annex C): entry [symbol] = length << 16 | code,
// 0 for a symbol without a code. Layout of the 4 tables as one array (HuffTables::e): DC luma at
// kHuffDcLuma, DC chroma, AC luma, AC chroma.
constexpr int kHuffDcLuma = 0, kHuffDcChroma = 16, kHuffAcLuma = 32, kHuffAcChroma = 32 + 256;
constexpr int kHuffEntries = 32 + 2 * 256;
struct HuffTables {
  uint32_t e[kHuffEntries];
};
constexpr void fill_huff(uint32_t* e, const uint8_t* bits, const uint8_t* vals) {
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i) e[vals[k++]] = uint32_t(len) << 16 | code++;
    code <<= 1;
  }
}
constexpr HuffTables make_huff() {
  HuffTables t{};
  fill_huff(t.e + kHuffDcLuma, kDcLumaBits, kDcVals);
  fill_huff(t.e + kHuffDcChroma, kDcChromaBits, kDcVals);
  fill_huff(t.e + kHuffAcLuma, kAcLumaBits, kAcLumaVals);
  fill_huff(t.e + kHuffAcChroma, kAcChromaBits, kAcChromaVals);
  return t;
}
constexpr HuffTables kHuff = make_huff();

// IJG quality rule: `quality` 1..100 -> one quantiser entry.
VEP_JPEG_HD inline int quant_entry(int base, int quality) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int v = (base * scale + 50) / 100;
  return v < 1 ? 1 : (v > 255 ? 255 : v);
}

VEP_JPEG_HD inline int mcus_x(int w) { return (w + kMcu - 1) / kMcu; }
VEP_JPEG_HD inline int mcus_y(int h) { return (h + kMcu - 1) / kMcu; }
VEP_JPEG_HD inline int intervals(int mcus) { return (mcus + kRestartInterval - 1) / kRestartInterval; }

// second byte of the marker after interval i (not the last): RSTm, m cycling 0..7
VEP_JPEG_HD inline int rst_marker(int i) { return 0xd0 + (i & 7); }

VEP_JPEG_HD inline void bgr_to_ycc(int b, int g, int r, int* y, int* cb, int* cr) {
  *y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  *cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  *cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// One output of a DCT pass over 8 values `stride` apart, before its shift. `dct` points to
// kDct (or a copy of it) as 64 consecutive entries.
template <class C, class P>
VEP_JPEG_HD inline int dct_dot(const C* dct, int u, const P* p, int stride) {
  int s = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) s += int(dct[u * 8 + k]) * int(p[k * stride]);
  return s;
}
VEP_JPEG_HD inline int dct_round1(int s) { return (s + 512) >> 10; }
// d: column pass output (16 fraction bits); q: quantiser entry 1..255
VEP_JPEG_HD inline int quantise(int d, int q, bool ac) {
  const uint32_t a = uint32_t(d < 0 ? -d : d);
  int v = int((a + (uint32_t(q) << 15)) / (uint32_t(q) << 16));
  if (ac && v > 1023) v = 1023;
  return d < 0 ? -v : v;
}

// Bit writer over a byte sink (`void put(uint8_t)`), with byte stuffing.
template <class Sink>
struct BitWriter {
  Sink& sink;
  uint64_t acc = 0;
  int nb = 0;
  VEP_JPEG_HD explicit BitWriter(Sink& s) : sink(s) {}
  // len <= 32 bits of `code`, most significant first
  VEP_JPEG_HD void put(uint32_t code, int len) {
    acc = (acc << len) | code;
    nb += len;
    while (nb >= 8) {
      const uint8_t b = uint8_t(acc >> (nb - 8));
      sink.put(b);
      if (b == 0xff) sink.put(0);
      nb -= 8;
    }
  }
  VEP_JPEG_HD void flush() {
    if (nb) put((1u << (8 - nb)) - 1, 8 - nb);
  }
};

// Huffman-code one block. `c` gives its 64 zigzag coefficients (c[k]) and the mask of its nonzero
// AC coefficients (c.ac_mask(): bit k, k = 1..63), so the coder visits the nonzero ones only and
// takes the zero runs from their positions. `pred` is the component's DC predictor; dc / ac point
// to the component's tables (HuffTables entries).
template <class Block, class Tab, class Sink>
VEP_JPEG_HD inline void encode_block(const Block& c, int* pred, const Tab* dc, const Tab* ac, BitWriter<Sink>& bw) {
  int diff = int(c[0]) - *pred;
  diff = diff < -2047 ? -2047 : (diff > 2047 ? 2047 : diff);
  *pred += diff;
  {
    const uint32_t a = uint32_t(diff < 0 ? -diff : diff);
    const int s = a ? 32 - __builtin_clz(a) : 0;
    const uint32_t e = dc[s];
    const uint32_t bits = uint32_t(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1);
    bw.put((e & 0xffff) << s | bits, int(e >> 16) + s);
  }
  uint64_t mask = c.ac_mask();
  int prev = 0;
  while (mask) {
    const int k = __builtin_ctzll(mask);
    mask &= mask - 1;
    int run = k - prev - 1;
    prev = k;
    while (run > 15) {
      const uint32_t z = ac[0xf0];
      bw.put(z & 0xffff, int(z >> 16));
      run -= 16;
    }
    const int v = int(c[k]);
    const uint32_t a = uint32_t(v < 0 ? -v : v);
    const int s = 32 - __builtin_clz(a);
    const uint32_t e = ac[run << 4 | s];
    const uint32_t bits = uint32_t(v < 0 ? v - 1 : v) & ((1u << s) - 1);
    bw.put((e & 0xffff) << s | bits, int(e >> 16) + s);
  }
  if (prev != 63) {
    const uint32_t z = ac[0];
    bw.put(z & 0xffff, int(z >> 16));
  }
}

// One restart interval: `n` MCUs, block i of the interval from blocks.block(i), then the padding.
template <class Blocks, class Tab, class Sink>
VEP_JPEG_HD inline void encode_interval(const Blocks& blocks, int n, const Tab* huff, Sink& sink) {
  BitWriter<Sink> bw(sink);
  int pred[3] = {0, 0, 0};
  for (int m = 0; m < n; ++m) {
#pragma unroll
    for (int b = 0; b < kBlocksPerMcu; ++b) {
      const int comp = b < 4 ? 0 : b - 3;
      encode_block(blocks.block(m * kBlocksPerMcu + b), &pred[comp], huff + (comp ? kHuffDcChroma : kHuffDcLuma),
                   huff + (comp ? kHuffAcChroma : kHuffAcLuma), bw);
    }
  }
  bw.flush();
}

// Blocks in host memory: 64 consecutive zigzag coefficients each.
struct HostBlock {
  const int16_t* p;
  int operator[](int k) const { return p[k]; }
  uint64_t ac_mask() const {
    uint64_t m = 0;
    for (int k = 1; k < 64; ++k) m |= uint64_t(p[k] != 0) << k;
    return m;
  }
};
struct HostBlocks {
  const int16_t* p;
  HostBlock block(int i) const { return HostBlock{p + size_t(i) * 64}; }
};

// ---- host side (jpeg.cpp) ----

// Everything up to and including the SOS header of a w x h picture at `quality` 1..100.
std::string header(int w, int h, int quality);
// Append interval `index` of `count` and what follows it: 0xFF and its RSTm marker, or EOI
// after the last one. (The GPU path joins its segments on the device by the same rule and ends
// with append_segment of an empty last piece.)
void append_segment(std::string& out, const uint8_t* seg, size_t len, int index, int count);
// The whole stream of a packed BGR24 picture (w, h >= 1; quality 1..100): the no-GPU backend's
// encoder and the oracle of the kernels.
std::string encode_cpu(const uint8_t* bgr, int w, int h, int quality);

}  // namespace vep::jpeg
