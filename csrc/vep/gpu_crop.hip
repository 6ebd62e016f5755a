// gfx950 (CDNA4) crops of a picture, cut and resized. See gpu.h for the contract and crop.h for the
// arithmetic, which the CPU implementation (crop.cpp) shares: both produce the same bytes.
//
// One launch covers every crop of every picture of a request: blockIdx.y is the descriptor (one
// box of one picture), blockIdx.x below `fill_base` a tile of its fitted rectangle, at or above it
// a row of its output to fill with the pad colour wherever the picture does not cover it.
//
// A tile is kTileW x kTileH output pixels: a wave owns every fourth row of it, a lane one column,
// so a thread computes up to kRows output pixels. Both axes run on one tap definition
// (crop::Taps: consecutive source indices, only the two ends weighing differently), so reducing,
// enlarging and any mix of the two are the same code:
//  * the source rows of the tile's footprint are staged in LDS (gpu_stage.h: 16-byte loads from
//    aligned addresses, byte heads and tails, nothing outside the rect's own bytes is read), as
//    many rows per barrier as fit; a footprint wider than the buffer goes in segments of kSegPix
//    pixels, one row at a time;
//  * a thread sums a staged row horizontally for its column ONCE (sum <= 255 * Dx: 32 bits) and
//    adds it, weighed, to each of its output rows that has the row among its taps. Reducing, that
//    is the scale kernel's streaming read (a source row serves one or two output rows);
//    enlarging, the footprint is small, one staging serves the whole tile and a source row feeds
//    several output rows;
//  * the accumulators are 32 bits while 255 * Dx * Dy fits and 64 bits above (crop::narrow); one
//    rounding at the end, no float.
// The tile's bytes are then put together in LDS, every byte at its global address modulo 16, and
// written row by row: 16-byte stores to 16-byte aligned addresses, the unaligned head and tail of
// a row byte by byte (crop k of a packed [n, H, W, 3] tensor starts at any byte address). Bytes
// outside the tile's own rows are NOT WRITTEN AT ALL.
//
// check_crop() proves on the host that every read lies inside the picture and every write inside
// the crop's own output.
#define VEP_KERNEL_SOURCE 1  // descriptors' pointers are global-address-space here (gpu.h)
#include <algorithm>

#include "crop.h"
#include "gpu.h"
#include "gpu_stage.h"

namespace vep::gpu {

namespace {

constexpr u32 kThreads = stage::kThreads;
constexpr u32 kLdsBytes = 24576;
// pixels of one staged segment: 3 bytes each + up to 15 bytes of misalignment fit the buffer
constexpr u32 kSegPix = (kLdsBytes - 16) / 3;
static_assert(kSegPix * 3 + 15 <= kLdsBytes, "segment fits LDS");
constexpr u32 kTileW = 64;                   // a wave spans a tile's row
constexpr u32 kWaves = kThreads / kTileW;    // 4
constexpr u32 kRows = 4;                     // output rows of one thread
constexpr u32 kTileH = kWaves * kRows;       // 16
constexpr u32 kOutCap = kTileW * 3 + 16;     // a tile row in LDS: its bytes + up to 15 of misalignment
static_assert(kOutCap % 16 == 0, "tile rows keep their alignment");
static_assert(kTileH * ((kTileW * 3 >> 4) + 1) <= kThreads, "one 16-byte vector of the tile per thread");

__host__ __device__ inline u32 tiles_x(u32 fw) { return (fw + kTileW - 1) / kTileW; }
__host__ __device__ inline u32 tiles_of(u32 fw, u32 fh) { return tiles_x(fw) * ((fh + kTileH - 1) / kTileH); }

template <typename Acc>
__device__ __forceinline__ void crop_tile(const CropDesc& d, u32 j0, u32 j1, u32 k0, u32 k1, u8* lds, u8* olds) {
  // (every field is read into a register once: the descriptor itself stays in global memory)
  const u32 sw = u32(d.x1 - d.x0), sh = u32(d.y1 - d.y0), fw = d.fw, fh = d.fh, ow = d.ow;
  const u32 src_pitch = d.src_pitch;
  const VEP_DEV u8* src = d.src + u64(u32(d.y0)) * src_pitch + u64(u32(d.x0)) * 3;  // the rect's origin
  // the tile's footprint (taps are monotone in the output index)
  const u32 ia = crop::taps(j0, sw, fw).lo, ib = crop::taps(j1 - 1, sw, fw).hi;
  const u32 ra = crop::taps(k0, sh, fh).lo, rz = crop::taps(k1 - 1, sh, fh).hi;
  const u32 npix = ib - ia + 1;
  const bool fits = npix <= kSegPix;
  const u32 rowcap = fits ? ((npix * 3 + 15 + 15) & ~15u) : kLdsBytes;
  const u32 rpp = fits ? kLdsBytes / rowcap : 1;  // rows staged per barrier
  const u32 c = threadIdx.x & (kTileW - 1), q = threadIdx.x / kTileW;
  const u32 j = j0 + c;
  const bool active = j < j1;
  crop::Taps tx = {1, 0, 0, 0, 0};
  if (active) tx = crop::taps(j, sw, fw);
  // the taps of the thread's output rows k0 + q + m * kWaves; lo > hi: no such row
  u32 ylo[kRows], yhi[kRows], ywlo[kRows], ywhi[kRows];
  const u32 ywmid = fh <= sh ? fh : 0;
  Acc acc[kRows][3];
#pragma unroll
  for (u32 m = 0; m < kRows; ++m) {
    const u32 k = k0 + q + m * kWaves;
    ylo[m] = 1;
    yhi[m] = ywlo[m] = ywhi[m] = 0;
    if (active && k < k1) {
      const crop::Taps t = crop::taps(k, sh, fh);
      ylo[m] = t.lo;
      yhi[m] = t.hi;
      ywlo[m] = t.w_lo;
      ywhi[m] = t.w_hi;
    }
    acc[m][0] = acc[m][1] = acc[m][2] = 0;
  }
  u32 h0 = 0, h1 = 0, h2 = 0;
  for (u32 rb = ra; rb <= rz; rb += rpp) {
    const u32 nr = min(rpp, rz - rb + 1);
    for (u32 is = ia; is <= ib; is += kSegPix) {
      const u32 ie = min(is + kSegPix, ib + 1);  // exclusive
      stage::stage_rows(src, src_pitch, rb, nr, is, (ie - is) * 3, rowcap, lds);
      __syncthreads();
      if (active) {
        const u32 a = max(tx.lo + 1, is), b = min(tx.hi, ie);  // inner samples [a, b) of this segment
        const bool has_lo = tx.lo >= is && tx.lo < ie, has_hi = tx.hi != tx.lo && tx.hi >= is && tx.hi < ie;
        for (u32 rr = 0; rr < nr; ++rr) {
          const u32 r = rb + rr;
          bool need = false;
#pragma unroll
          for (u32 m = 0; m < kRows; ++m) need = need || (r >= ylo[m] && r <= yhi[m]);
          if (!need) continue;  // (the same answer in every segment of the row)
          const VEP_DEV u8* g = src + u64(r) * src_pitch + u64(is) * 3;
          const u32 row_off = rr * rowcap + (u32(reinterpret_cast<uintptr_t>(g)) & 15u);
          const u8* l = lds + row_off;
          if (a < b) {
            u32 s0 = 0, s1 = 0, s2 = 0;
            stage::sum_samples(lds, row_off + (a - is) * 3, b - a, s0, s1, s2);
            h0 += tx.w_mid * s0;
            h1 += tx.w_mid * s1;
            h2 += tx.w_mid * s2;
          }
          if (has_lo) {
            const u8* p = l + (tx.lo - is) * 3;
            h0 += tx.w_lo * p[0];
            h1 += tx.w_lo * p[1];
            h2 += tx.w_lo * p[2];
          }
          if (has_hi) {
            const u8* p = l + (tx.hi - is) * 3;
            h0 += tx.w_hi * p[0];
            h1 += tx.w_hi * p[1];
            h2 += tx.w_hi * p[2];
          }
          if (ie == ib + 1) {  // the row is complete
#pragma unroll
            for (u32 m = 0; m < kRows; ++m) {
              if (r >= ylo[m] && r <= yhi[m]) {
                const Acc wy = r == ylo[m] ? ywlo[m] : (r == yhi[m] ? ywhi[m] : ywmid);
                acc[m][0] += wy * h0;
                acc[m][1] += wy * h1;
                acc[m][2] += wy * h2;
              }
            }
            h0 = h1 = h2 = 0;
          }
        }
      }
      __syncthreads();
    }
  }
  // The tile's bytes in LDS: row rr's at rr * kOutCap + (their global address modulo 16).
  VEP_DEV u8* dst = d.dst;
  const u32 fx = d.fx, fy = d.fy;
  auto row_ptr = [&](u32 rr) -> VEP_DEV u8* { return dst + (u64(fy + k0 + rr) * ow + fx + j0) * 3; };
  const u32 dx = crop::den(sw, fw), dy = crop::den(sh, fh);
#pragma unroll
  for (u32 m = 0; m < kRows; ++m) {
    const u32 rr = q + m * kWaves;
    if (!active || k0 + rr >= k1) continue;
    u32 o0, o1, o2;
    if constexpr (sizeof(Acc) == 4) {
      const u32 den = dx * dy;
      o0 = scale::round_div32(acc[m][0], den);
      o1 = scale::round_div32(acc[m][1], den);
      o2 = scale::round_div32(acc[m][2], den);
    } else {
      const u64 den = u64(dx) * dy;
      o0 = scale::round_div64(acc[m][0], den);
      o1 = scale::round_div64(acc[m][1], den);
      o2 = scale::round_div64(acc[m][2], den);
    }
    u8* o = olds + rr * kOutCap + (u32(reinterpret_cast<u64>(row_ptr(rr))) & 15u) + c * 3;
    o[0] = u8(o0);
    o[1] = u8(o1);
    o[2] = u8(o2);
  }
  __syncthreads();
  // The rows go out: whole 16-byte vectors at aligned addresses, one per thread ...
  const u32 nrow = k1 - k0, nbytes = (j1 - j0) * 3;
  const u32 t = threadIdx.x;
  const u32 vpr = (nbytes >> 4) + 1;  // upper bound of a row's 16-byte vectors
  if (t < nrow * vpr) {
    const u32 rr = t / vpr, v = t - rr * vpr;
    VEP_DEV u8* gp = row_ptr(rr);
    const u32 mis = u32(reinterpret_cast<u64>(gp)) & 15u;
    const u32 head = min(nbytes, (16u - mis) & 15u);
    if (v < ((nbytes - head) >> 4)) {
      const u32 o = head + v * 16;  // o + 16 <= nbytes
      *reinterpret_cast<VEP_DEV uint4*>(gp + o) = *reinterpret_cast<const uint4*>(olds + rr * kOutCap + mis + o);
    }
  }
  // ... and a row's head and tail byte by byte: 32 byte slots per row, 8 rows per step
  for (u32 rr = t >> 5; rr < nrow; rr += kThreads / 32) {
    const u32 slot = t & 31u;
    VEP_DEV u8* gp = row_ptr(rr);
    const u32 mis = u32(reinterpret_cast<u64>(gp)) & 15u;
    const u32 head = min(nbytes, (16u - mis) & 15u);
    const u32 body = ((nbytes - head) >> 4) << 4;
    u32 o;
    if (slot < 16) {
      if (slot >= head) continue;
      o = slot;
    } else {
      if (slot - 16 >= nbytes - head - body) continue;
      o = head + body + (slot - 16);
    }
    gp[o] = olds[rr * kOutCap + mis + o];
  }
}

__global__ __launch_bounds__(kThreads) void crop_kernel(const CropDesc* __restrict__ descs, u32 fill_base) {
  __shared__ __attribute__((aligned(16))) u8 lds[kLdsBytes + 16];  // (+ 16: sum_samples' dword reads)
  __shared__ __attribute__((aligned(16))) u8 olds[kTileH * kOutCap];
  const CropDesc& d = descs[blockIdx.y];
  const u32 bx = blockIdx.x;
  const u32 ow = d.ow, oh = d.oh, fw = d.fw, fh = d.fh;
  if (bx >= fill_base) {
    // padding: one row of the output, every byte outside the picture's rectangle
    const u32 y = bx - fill_base;
    if (y >= oh || (fw == ow && fh == oh)) return;
    const u32 fx = d.fx, fy = d.fy, pad = d.pad_bgr;
    const bool pic_row = y >= fy && y < fy + fh;
    VEP_DEV u8* row = d.dst + u64(y) * ow * 3;
    const u32 n = ow * 3, pa = fx * 3, pb = pa + fw * 3;
    for (u32 b = threadIdx.x; b < n; b += kThreads)
      if (!(pic_row && b >= pa && b < pb)) row[b] = u8(pad >> (8 * (b % 3)));
    return;
  }
  if (bx >= tiles_of(fw, fh)) return;
  const u32 ntx = tiles_x(fw);
  const u32 tk = bx / ntx, tj = bx - tk * ntx;
  const u32 j0 = tj * kTileW, j1 = min(fw, j0 + kTileW);
  const u32 k0 = tk * kTileH, k1 = min(fh, k0 + kTileH);
  if (crop::narrow(crop::den(u32(d.x1 - d.x0), fw), crop::den(u32(d.y1 - d.y0), fh)))
    crop_tile<u32>(d, j0, j1, k0, k1, lds, olds);
  else
    crop_tile<u64>(d, j0, j1, k0, k1, lds, olds);
}

}  // namespace

void check_crop(const CropDesc& d, size_t src_bytes, size_t dst_bytes) {
  VEP_CHECK(d.src && d.dst, "crop: null picture or output");
  VEP_CHECK(d.pw >= 1 && d.ph >= 1 && d.pw <= crop::kMaxSide && d.ph <= crop::kMaxSide,
            "crop: picture size must be 1..65535");
  const u64 w = u64(d.pw), h = u64(d.ph);
  VEP_CHECK(u64(d.src_pitch) >= w * 3, "crop: pitch shorter than a row");
  VEP_CHECK((h - 1) * d.src_pitch + w * 3 <= src_bytes, "crop: picture rows outside the picture's memory");
  VEP_CHECK(d.x0 >= 0 && d.x0 < d.x1 && d.x1 <= d.pw && d.y0 >= 0 && d.y0 < d.y1 && d.y1 <= d.ph,
            "crop: rect empty or outside the picture");
  VEP_CHECK(d.ow >= 1 && d.oh >= 1 && d.ow <= crop::kMaxOut && d.oh <= crop::kMaxOut,
            "crop: width and height must be 1..4096");
  VEP_CHECK(d.fw >= 1 && d.fh >= 1 && u32(d.fx) + d.fw <= d.ow && u32(d.fy) + d.fh <= d.oh,
            "crop: fitted rectangle empty or outside the output");
  VEP_CHECK(u64(d.ow) * d.oh * 3 <= dst_bytes, "crop: output larger than its memory");
  VEP_CHECK(d.pad_bgr <= 0xFFFFFFu, "crop: pad colour out of range");
}

void launch_crop(const CropDesc* d_descs, const CropDesc* h_descs, int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= 65535, "crop: at most 65535 crops per launch");
  u32 tiles = 0, rows = 0;
  for (int i = 0; i < n; ++i) {
    const CropDesc& d = h_descs[i];
    tiles = std::max(tiles, tiles_of(d.fw, d.fh));
    if (d.fw != d.ow || d.fh != d.oh) rows = std::max(rows, u32(d.oh));
  }
  hipLaunchKernelGGL(crop_kernel, dim3(tiles + rows, u32(n)), dim3(kThreads), 0, s, d_descs, tiles);
  VEP_HIP(hipGetLastError());
}

}  // namespace vep::gpu
