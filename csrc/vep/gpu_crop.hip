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
//  * the source rows of the tile's footprint are staged in LDS (stage::stage_rows: nothing outside
//    the rect's own bytes is read), as many rows per barrier as fit; a footprint wider than the
//    buffer goes in segments of kSegPix pixels, one row at a time;
//  * a thread sums a staged row horizontally for its column ONCE (stage::sum_weighted, which the
//    scale kernel shares; sum <= 255 * Dx: 32 bits) and
//    adds it, weighed, to each of its output rows that has the row among its taps. Reducing, that
//    is the scale kernel's streaming read (a source row serves one or two output rows);
//    enlarging, the footprint is small, one staging serves the whole tile and a source row feeds
//    several output rows;
//  * the accumulators are 32 bits while 255 * Dx * Dy fits and 64 bits above (crop::narrow); one
//    rounding at the end, no float.
// The tile's bytes are then put together in LDS, every byte at its global address modulo 16, and
// written with stage::store_rows (crop k of a packed [n, H, W, 3] tensor starts at any byte
// address). Bytes outside the tile's own rows are NOT WRITTEN AT ALL. The tile's geometry, the
// staging and the store live in gpu_stage.h, which the overlay kernel (gpu_overlay.hip) shares.
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

using stage::kLdsBytes;
using stage::kSegPix;
using stage::kThreads;
// the tile: kRows output rows of one thread
using stage::kRows;
using stage::kTileH;
using stage::kTileW;
using stage::kWaves;
using stage::tiles_of;
using stage::tiles_x;
constexpr u32 kOutCap = stage::kTileRowCap;

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
  const u32 rowcap = fits ? stage::rowcap_of(npix) : kLdsBytes;
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
        for (u32 rr = 0; rr < nr; ++rr) {
          const u32 r = rb + rr;
          bool need = false;
#pragma unroll
          for (u32 m = 0; m < kRows; ++m) need = need || (r >= ylo[m] && r <= yhi[m]);
          if (!need) continue;  // (the same answer in every segment of the row)
          const VEP_DEV u8* g = src + u64(r) * src_pitch + u64(is) * 3;
          const u32 row_off = rr * rowcap + (u32(reinterpret_cast<uintptr_t>(g)) & 15u);
          stage::sum_weighted(lds, row_off, is, ie, tx.lo, tx.hi, tx.w_lo, tx.w_mid, tx.w_hi, h0, h1, h2);
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
  const Acc den = Acc(crop::den(sw, fw)) * crop::den(sh, fh);
#pragma unroll
  for (u32 m = 0; m < kRows; ++m) {
    const u32 rr = q + m * kWaves;
    if (!active || k0 + rr >= k1) continue;
    u8* o = olds + rr * kOutCap + (u32(reinterpret_cast<u64>(row_ptr(rr))) & 15u) + c * 3;
    o[0] = u8(scale::round_div(acc[m][0], den));
    o[1] = u8(scale::round_div(acc[m][1], den));
    o[2] = u8(scale::round_div(acc[m][2], den));
  }
  __syncthreads();
  stage::store_rows(row_ptr(0), ow * 3, k1 - k0, (j1 - j0) * 3, kOutCap, olds);
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
