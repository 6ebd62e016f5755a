// gfx950 (CDNA4) baseline JPEG encoder of the frame server. See gpu.h for the contracts and
// jpeg.h for the stream format and the arithmetic, which the CPU encoder (jpeg.cpp) shares: both
// produce the same bytes.
//
// Decomposition (one picture, four launches on one stream):
//  * jpeg_transform_kernel — one 256-thread workgroup per 16x16 MCU, one thread per sample:
//    load with edge replication, convert to YCbCr, stage the six 8x8 blocks in LDS, two DCT
//    passes over LDS (one output per thread and step, 8-term dot products), quantise, and write
//    the MCU's 384 zigzag coefficients as one contiguous 768-byte row.
//  * jpeg_entropy_kernel — restart intervals are independent, so a lane Huffman-codes one
//    interval (jpeg::encode_interval, the code the CPU encoder runs) into the interval's own
//    segment, with the four code tables staged in LDS. A lane fetches a block with eight
//    16-byte loads in flight together, parks it in its own LDS column ([k][lane], so the
//    wave's accesses to one k fall on distinct banks) and keeps the mask of the nonzero
//    coefficients; the coder then visits only those. (With one 2-byte global load per
//    coefficient, each waited for, the kernel took 427 us instead of 285 us for a noisy 1080p
//    frame.) It is the encoder's longest kernel and bound by a lane's own chain of dependent
//    instructions, about 0.5 us per coded coefficient, not by bytes, stores or divergence:
//    storing four bytes at a time and running 16 lanes per wave both left it at 290 us
//    (docs/JPEG.md). More lanes per interval is what would shorten it.
//  * jpeg_scan_kernel — one workgroup: exclusive prefix sum of the segments' lengths (+ 2 for
//    each RSTm marker) -> offsets in the joined stream and its total size.
//  * jpeg_gather_kernel — one wave per interval copies the segment to its offset and appends the
//    marker.
// The host (jpeg_pool.cpp) then copies only the joined stream's bytes.
#define VEP_KERNEL_SOURCE 1  // descriptors' pointers are global-address-space here (gpu.h)
#include <algorithm>

#include "gpu.h"
#include "jpeg.h"

namespace vep::gpu {

namespace {

__global__ __launch_bounds__(256) void jpeg_transform_kernel(const JpegDesc d) {
  __shared__ int16_t px[jpeg::kBlocksPerMcu * 64];   // level-shifted samples, block-major
  __shared__ uint8_t cbf[256], crf[256];             // full-resolution chroma of the MCU
  __shared__ int t[jpeg::kBlocksPerMcu * 64];        // row pass
  __shared__ int16_t zz[jpeg::kBlocksPerMcu * 64];   // quantised, zigzag order
  __shared__ uint8_t q[2 * 64];                      // luma, chroma quantisers (natural order)
  __shared__ uint8_t izz[64];                        // natural position -> zigzag index
  __shared__ int16_t dct[64];
  const int tid = threadIdx.x;
  const int mcu = blockIdx.x;
  const int mx = mcu % d.mcus_x, my = mcu / d.mcus_x;
  if (tid < 128) q[tid] = uint8_t(jpeg::quant_entry(tid < 64 ? jpeg::kLumaQuant[tid] : jpeg::kChromaQuant[tid - 64], d.quality));
  if (tid < 64) {
    izz[jpeg::kZigzag[tid]] = uint8_t(tid);
    dct[tid] = jpeg::kDct[tid >> 3][tid & 7];
  }
  {
    const int y = tid >> 4, x = tid & 15;
    const int sy = min(my * jpeg::kMcu + y, d.h - 1), sx = min(mx * jpeg::kMcu + x, d.w - 1);
    const VEP_DEV u8* p = d.bgr + (size_t(sy) * size_t(d.w) + size_t(sx)) * 3;
    int Y, cb, cr;
    jpeg::bgr_to_ycc(p[0], p[1], p[2], &Y, &cb, &cr);
    px[((y >> 3) * 2 + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7)] = int16_t(Y - 128);
    cbf[tid] = uint8_t(cb);
    crf[tid] = uint8_t(cr);
  }
  __syncthreads();
  if (tid < 128) {
    const uint8_t* c = tid < 64 ? cbf : crf;
    const int k = tid & 63, cy = k >> 3, cx = k & 7;
    const int a = (2 * cy) * 16 + 2 * cx;
    px[(4 + (tid >> 6)) * 64 + k] = int16_t(((c[a] + c[a + 1] + c[a + 16] + c[a + 17] + 2) >> 2) - 128);
  }
  __syncthreads();
  for (int i = tid; i < jpeg::kCoefsPerMcu; i += 256) {  // rows: t[b][y][u]
    const int u = i & 7;
    t[i] = jpeg::dct_round1(jpeg::dct_dot(dct, u, px + (i & ~7), 1));
  }
  __syncthreads();
  for (int i = tid; i < jpeg::kCoefsPerMcu; i += 256) {  // columns: d[b][v][u], quantised
    const int b = i >> 6, v = (i >> 3) & 7, u = i & 7;
    const int val = jpeg::dct_dot(dct, v, t + b * 64 + u, 8);
    zz[b * 64 + izz[i & 63]] = int16_t(jpeg::quantise(val, q[(b >= 4 ? 64 : 0) + (i & 63)], (i & 63) != 0));
  }
  __syncthreads();
  VEP_DEV i16* out = d.coefs + size_t(mcu) * jpeg::kCoefsPerMcu;
  for (int i = tid; i < jpeg::kCoefsPerMcu; i += 256) out[i] = zz[i];
}

// Byte sink of one interval's segment: never stores outside it.
struct SegmentSink {
  VEP_DEV u8* p;
  u32 pos = 0;
  bool overflow = false;
  __device__ void put(uint8_t b) {
    if (pos < u32(jpeg::kSegmentCap))
      p[pos] = b;
    else
      overflow = true;
    ++pos;
  }
};

// The interval's blocks for jpeg::encode_interval: block(i) stages block i in the lane's LDS
// column (coefficient k at col[k * 64]).
struct LdsBlock {
  const int16_t* col;
  uint64_t mask;
  __device__ int operator[](int k) const { return col[k * 64]; }
  __device__ uint64_t ac_mask() const { return mask; }
};
struct LdsBlocks {
  const VEP_DEV i16* coefs;  // the interval's first block (16-byte aligned, as every block)
  int16_t* col;
  __device__ LdsBlock block(int i) const {
    const VEP_DEV uint4* src = reinterpret_cast<const VEP_DEV uint4*>(coefs + size_t(i) * 64);
    uint4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = src[j];
    uint64_t mask = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int16_t val = int16_t((e & 1) ? w[e >> 1] >> 16 : w[e >> 1] & 0xffff);
        col[(j * 8 + e) * 64] = val;
        mask |= uint64_t(val != 0) << (j * 8 + e);
      }
    }
    return LdsBlock{col, mask & ~uint64_t(1)};
  }
};

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const JpegDesc d) {
  __shared__ uint32_t huff[jpeg::kHuffEntries];
  __shared__ int16_t stage[64 * 64];
  for (int i = threadIdx.x; i < jpeg::kHuffEntries; i += 64) huff[i] = jpeg::kHuff.e[i];
  __syncthreads();
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= d.intervals) return;
  const int m0 = i * jpeg::kRestartInterval;
  const int n = min(jpeg::kRestartInterval, d.mcus - m0);
  SegmentSink sink{d.seg + size_t(i) * jpeg::kSegmentCap};
  const LdsBlocks blocks{d.coefs + size_t(m0) * jpeg::kCoefsPerMcu, stage + threadIdx.x};
  jpeg::encode_interval(blocks, n, huff, sink);
  if (sink.overflow) {
    d.status[0] = 1;
    sink.pos = 0;
  }
  d.len[i] = sink.pos;
}

constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void jpeg_scan_kernel(const JpegDesc d) {
  __shared__ u32 part[kScanThreads];
  const int tid = threadIdx.x;
  const int n = d.intervals;
  const int per = (n + kScanThreads - 1) / kScanThreads;
  const int lo = min(tid * per, n), hi = min(lo + per, n);
  u32 sum = 0;
  for (int i = lo; i < hi; ++i) sum += d.len[i] + (i + 1 < n ? 2u : 0u);
  part[tid] = sum;
  __syncthreads();
  for (int step = 1; step < kScanThreads; step <<= 1) {  // inclusive scan of the partial sums
    const u32 add = tid >= step ? part[tid - step] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  u32 run = part[tid] - sum;
  for (int i = lo; i < hi; ++i) {
    d.off[i] = run;
    run += d.len[i] + (i + 1 < n ? 2u : 0u);
  }
  if (tid == kScanThreads - 1) {
    d.status[1] = part[tid];
    if (part[tid] > d.out_cap) d.status[2] = 1;
  }
}

__global__ __launch_bounds__(256) void jpeg_gather_kernel(const JpegDesc d) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= d.intervals) return;
  const u32 len = d.len[i], off = d.off[i];
  const u32 total = len + (i + 1 < d.intervals ? 2u : 0u);
  if (len > u32(jpeg::kSegmentCap) || off > d.out_cap || total > d.out_cap - off) return;  // (status[2] is set)
  const VEP_DEV u8* src = d.seg + size_t(i) * jpeg::kSegmentCap;
  VEP_DEV u8* dst = d.out + off;
  for (u32 j = lane; j < len; j += 64) dst[j] = src[j];
  if (lane < 2 && total != len) dst[len + lane] = lane ? uint8_t(jpeg::rst_marker(i)) : uint8_t(0xff);
}

}  // namespace

void launch_jpeg_transform(const JpegDesc& d, hipStream_t s) {
  hipLaunchKernelGGL(jpeg_transform_kernel, dim3(d.mcus), dim3(256), 0, s, d);
}
void launch_jpeg_entropy(const JpegDesc& d, hipStream_t s) {
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((d.intervals + 63) / 64), dim3(64), 0, s, d);
}
void launch_jpeg_scan(const JpegDesc& d, hipStream_t s) {
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, d);
}
void launch_jpeg_gather(const JpegDesc& d, hipStream_t s) {
  hipLaunchKernelGGL(jpeg_gather_kernel, dim3((d.intervals + 3) / 4), dim3(256), 0, s, d);
}

}  // namespace vep::gpu
