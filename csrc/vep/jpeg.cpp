// CPU JPEG encoder: the no-GPU backend's encoder and the oracle of gpu_jpeg.hip. The format and
// the arithmetic are jpeg.h's; this file adds the header writer and the segment join the GPU
// path uses as well.
#include "jpeg.h"

#include <algorithm>
#include <vector>

#include "common.h"

namespace vep::jpeg {

namespace {

void put16(std::string& s, int v) {
  s.push_back(char(v >> 8));
  s.push_back(char(v & 0xff));
}

void put_dht(std::string& s, int tc_th, const uint8_t* bits, const uint8_t* vals) {
  int n = 0;
  for (int i = 0; i < 16; ++i) n += bits[i];
  s.push_back(char(0xff));
  s.push_back(char(0xc4));
  put16(s, 2 + 1 + 16 + n);
  s.push_back(char(tc_th));
  s.append(reinterpret_cast<const char*>(bits), 16);
  s.append(reinterpret_cast<const char*>(vals), size_t(n));
}

struct VecSink {
  std::vector<uint8_t>& v;
  void put(uint8_t b) { v.push_back(b); }
};

}  // namespace

std::string header(int w, int h, int quality) {
  VEP_CHECK(w >= 1 && h >= 1 && w <= 65535 && h <= 65535, "jpeg: picture size out of range");
  VEP_CHECK(quality >= 1 && quality <= 100, "jpeg: quality must be 1..100");
  std::string s;
  s.reserve(640);
  s.append("\xff\xd8", 2);                                      // SOI
  s.append("\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00", 18);  // APP0: JFIF 1.01, 1:1
  s.append("\xff\xdb", 2);                                      // DQT: both tables, 8 bit, zigzag order
  put16(s, 2 + 2 * 65);
  for (int t = 0; t < 2; ++t) {
    s.push_back(char(t));
    for (int k = 0; k < 64; ++k) s.push_back(char(quant_entry((t ? kChromaQuant : kLumaQuant)[kZigzag[k]], quality)));
  }
  s.append("\xff\xc0", 2);  // SOF0
  put16(s, 8 + 3 * 3);
  s.push_back(8);
  put16(s, h);
  put16(s, w);
  s.push_back(3);
  s.append("\x01\x22\x00\x02\x11\x01\x03\x11\x01", 9);  // Y 2x2 table 0; Cb, Cr 1x1 table 1
  put_dht(s, 0x00, kDcLumaBits, kDcVals);
  put_dht(s, 0x10, kAcLumaBits, kAcLumaVals);
  put_dht(s, 0x01, kDcChromaBits, kDcVals);
  put_dht(s, 0x11, kAcChromaBits, kAcChromaVals);
  s.append("\xff\xdd\x00\x04", 4);  // DRI
  put16(s, kRestartInterval);
  s.append("\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00", 14);  // SOS
  return s;
}

void append_segment(std::string& out, const uint8_t* seg, size_t len, int index, int count) {
  out.append(reinterpret_cast<const char*>(seg), len);
  out.push_back(char(0xff));
  out.push_back(char(index + 1 < count ? rst_marker(index) : 0xd9));
}

// One MCU: 16x16 samples at (mx, my) with edge replication -> 6 blocks of zigzag coefficients.
static void transform_mcu(const uint8_t* bgr, int w, int h, int mx, int my, const uint8_t q[2][64], int16_t* out) {
  int16_t px[kBlocksPerMcu][64];
  int cb[kMcu][kMcu], cr[kMcu][kMcu];
  for (int y = 0; y < kMcu; ++y) {
    const int sy = std::min(my * kMcu + y, h - 1);
    for (int x = 0; x < kMcu; ++x) {
      const int sx = std::min(mx * kMcu + x, w - 1);
      const uint8_t* p = bgr + (size_t(sy) * size_t(w) + size_t(sx)) * 3;
      int Y;
      bgr_to_ycc(p[0], p[1], p[2], &Y, &cb[y][x], &cr[y][x]);
      px[(y >> 3) * 2 + (x >> 3)][(y & 7) * 8 + (x & 7)] = int16_t(Y - 128);
    }
  }
  for (int y = 0; y < 8; ++y)
    for (int x = 0; x < 8; ++x) {
      px[4][y * 8 + x] =
          int16_t(((cb[2 * y][2 * x] + cb[2 * y][2 * x + 1] + cb[2 * y + 1][2 * x] + cb[2 * y + 1][2 * x + 1] + 2) >> 2) - 128);
      px[5][y * 8 + x] =
          int16_t(((cr[2 * y][2 * x] + cr[2 * y][2 * x + 1] + cr[2 * y + 1][2 * x] + cr[2 * y + 1][2 * x + 1] + 2) >> 2) - 128);
    }
  for (int b = 0; b < kBlocksPerMcu; ++b) {
    int t[64];
    for (int y = 0; y < 8; ++y)
      for (int u = 0; u < 8; ++u) t[y * 8 + u] = dct_round1(dct_dot(&kDct[0][0], u, px[b] + y * 8, 1));
    int16_t nat[64];
    for (int v = 0; v < 8; ++v)
      for (int u = 0; u < 8; ++u)
        nat[v * 8 + u] = int16_t(quantise(dct_dot(&kDct[0][0], v, t + u, 8), q[b >= 4][v * 8 + u], (v | u) != 0));
    for (int k = 0; k < 64; ++k) out[b * 64 + k] = nat[kZigzag[k]];
  }
}

std::string encode_cpu(const uint8_t* bgr, int w, int h, int quality) {
  std::string out = header(w, h, quality);
  VEP_CHECK(bgr, "jpeg: null picture");
  uint8_t q[2][64];
  for (int k = 0; k < 64; ++k) {
    q[0][k] = uint8_t(quant_entry(kLumaQuant[k], quality));
    q[1][k] = uint8_t(quant_entry(kChromaQuant[k], quality));
  }
  const int mw = mcus_x(w), mcus = mw * mcus_y(h), n = intervals(mcus);
  std::vector<int16_t> coefs(size_t(kRestartInterval) * kCoefsPerMcu);
  std::vector<uint8_t> seg;
  seg.reserve(kSegmentCap);
  out.reserve(out.size() + size_t(mcus) * 96);
  for (int i = 0; i < n; ++i) {
    const int m0 = i * kRestartInterval, cnt = std::min(kRestartInterval, mcus - m0);
    for (int m = 0; m < cnt; ++m) transform_mcu(bgr, w, h, (m0 + m) % mw, (m0 + m) / mw, q, coefs.data() + size_t(m) * kCoefsPerMcu);
    seg.clear();
    VecSink sink{seg};
    encode_interval(HostBlocks{coefs.data()}, cnt, kHuff.e, sink);
    append_segment(out, seg.data(), seg.size(), i, n);
  }
  return out;
}

}  // namespace vep::jpeg
