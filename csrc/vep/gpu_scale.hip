// gfx950 (CDNA4) area-average downscale and camera wall. See gpu.h for the contract and scale.h
// for the arithmetic, which the CPU implementation (scale.cpp) shares: both produce the same
// bytes.
//
// One launch covers every tile: blockIdx.y is the tile, blockIdx.x below `fill_base` a block of
// its picture, at or above it a row of its cell to fill with background.
//
// A picture block owns one output row and a chunk of at most 256 output columns, one thread per
// output pixel. The source is a pure streaming read (1080p -> 320x180: 36 source pixels per
// output pixel), so the block stages the source rows of its footprint in LDS (stage::stage_rows),
// several rows per barrier when they fit. Each thread then reduces its pixel's footprint
// horizontally out of LDS (stage::sum_weighted with the wx weights: ow for every sample but the
// two at the ends, so the inner loop only adds; sum <= 255 * sw: 32 bits) and accumulates the rows
// vertically in registers (wy weights), in 32 bits while 255 * sw * sh fits and in 64 bits above
// (scale::narrow). A footprint wider than the LDS buffer is staged in segments of kSegPix pixels,
// one row at a time. The staging, the buffer's size and the weighted sum live in gpu_stage.h,
// which the crop kernel (gpu_crop.hip) shares.
//
// Every store is checked against the tile's cell (or the picture's own rectangle when the tile
// has no cell); check_scale() proves on the host that those lie inside the canvas.
#define VEP_KERNEL_SOURCE 1  // descriptors' pointers are global-address-space here (gpu.h)
#include <algorithm>

#include "gpu.h"
#include "gpu_stage.h"
#include "scale.h"

namespace vep::gpu {

namespace {

using stage::kLdsBytes;
using stage::kSegPix;
using stage::kThreads;

__device__ __forceinline__ u32 chunks_of(u32 ow) { return (ow + kThreads - 1) / kThreads; }

template <typename Acc>
__device__ __forceinline__ void scale_block(const ScaleDesc& d, u32 k, u32 j0, u32 j1, u8* lds) {
  // (every field is read into a register once: the descriptor itself stays in global memory)
  const VEP_DEV u8* src = d.src;
  const u32 src_pitch = d.src_pitch;
  const u32 sw = u32(d.sw), sh = u32(d.sh), ow = u32(d.ow), oh = u32(d.oh);
  const u32 ia = scale::span_lo(j0, sw, ow), ib = scale::span_hi(j1 - 1, sw, ow);
  const u32 r0 = scale::span_lo(k, sh, oh), r1 = scale::span_hi(k, sh, oh);
  const u32 npix = ib - ia + 1;
  const bool fits = npix <= kSegPix;
  const u32 rowcap = fits ? stage::rowcap_of(npix) : kLdsBytes;
  const u32 rpp = fits ? kLdsBytes / rowcap : 1;  // rows staged per barrier
  const u32 j = j0 + threadIdx.x;
  const bool active = j < j1;
  // Only the two ends of a footprint overlap the output pixel in part; every sample between
  // them weighs ow, so the inner loop only adds.
  u32 lo = 0, hi = 0, w_lo = 0, w_hi = 0;
  if (active) {
    lo = scale::span_lo(j, sw, ow);
    hi = scale::span_hi(j, sw, ow);
    w_lo = scale::weight(j, lo, sw, ow);
    w_hi = scale::weight(j, hi, sw, ow);
  }
  Acc a0 = 0, a1 = 0, a2 = 0;
  u32 h0 = 0, h1 = 0, h2 = 0;
  for (u32 rb = r0; rb <= r1; rb += rpp) {
    const u32 nr = min(rpp, r1 - rb + 1);
    for (u32 is = ia; is <= ib; is += kSegPix) {
      const u32 ie = min(is + kSegPix, ib + 1);  // exclusive
      stage::stage_rows(src, src_pitch, rb, nr, is, (ie - is) * 3, rowcap, lds);
      __syncthreads();
      if (active) {
        for (u32 rr = 0; rr < nr; ++rr) {
          const VEP_DEV u8* g = src + u64(rb + rr) * src_pitch + u64(is) * 3;
          const u32 row_off = rr * rowcap + (u32(reinterpret_cast<uintptr_t>(g)) & 15u);
          stage::sum_weighted(lds, row_off, is, ie, lo, hi, w_lo, ow, w_hi, h0, h1, h2);
          if (ie == ib + 1) {  // the row is complete
            const Acc wy = scale::weight(k, rb + rr, sh, oh);
            a0 += wy * h0;
            a1 += wy * h1;
            a2 += wy * h2;
            h0 = h1 = h2 = 0;
          }
        }
      }
      __syncthreads();
    }
  }
  if (!active) return;
  const i32 x = d.dx + i32(j), y = d.dy + i32(k);
  if (d.cw > 0 && d.ch > 0 && (x < d.cx || x >= d.cx + d.cw || y < d.cy || y >= d.cy + d.ch)) return;
  const Acc den = Acc(sw) * sh;
  VEP_DEV u8* q = d.dst + u64(y) * d.dst_pitch + u64(x) * 3;
  q[0] = u8(scale::round_div(a0, den));
  q[1] = u8(scale::round_div(a1, den));
  q[2] = u8(scale::round_div(a2, den));
}

__global__ __launch_bounds__(kThreads) void scale_kernel(const ScaleDesc* __restrict__ descs, u32 fill_base) {
  __shared__ __attribute__((aligned(16))) u8 lds[kLdsBytes + 16];  // (+ 16: scale_block's dword reads)
  const ScaleDesc& d = descs[blockIdx.y];
  const u32 bx = blockIdx.x;
  if (bx >= fill_base) {
    // background: one row of the cell, every byte outside the picture's rectangle
    const u32 fy = bx - fill_base;
    if (d.cw <= 0 || d.ch <= 0 || fy >= u32(d.ch)) return;
    const i32 y = d.cy + i32(fy);
    const bool pic_row = d.src && y >= d.dy && y < d.dy + d.oh;
    VEP_DEV u8* row = d.dst + u64(y) * d.dst_pitch + u64(d.cx) * 3;
    const u32 n = u32(d.cw) * 3;
    const u32 pa = u32(d.dx - d.cx) * 3, pb = pa + u32(d.ow) * 3;  // (check_scale: dx >= cx)
    for (u32 b = threadIdx.x; b < n; b += kThreads)
      if (!(pic_row && b >= pa && b < pb)) row[b] = scale::kBackground;
    return;
  }
  if (!d.src) return;
  const u32 nch = chunks_of(u32(d.ow));
  if (bx >= nch * u32(d.oh)) return;
  const u32 k = bx / nch, c = bx - k * nch;
  const u32 cwid = (u32(d.ow) + nch - 1) / nch;
  const u32 j0 = c * cwid, j1 = min(u32(d.ow), j0 + cwid);
  if (j0 >= j1) return;
  if (scale::narrow(u32(d.sw), u32(d.sh)))
    scale_block<u32>(d, k, j0, j1, lds);
  else
    scale_block<u64>(d, k, j0, j1, lds);
}

}  // namespace

void check_scale(const ScaleDesc& d, int canvas_w, int canvas_h) {
  VEP_CHECK(d.dst, "scale: null canvas");
  VEP_CHECK(canvas_w >= 1 && canvas_h >= 1 && canvas_w <= scale::kMaxSide && canvas_h <= scale::kMaxSide,
            "scale: canvas size must be 1..65535");
  VEP_CHECK(u64(d.dst_pitch) >= u64(canvas_w) * 3, "scale: canvas pitch shorter than a row");
  const bool cell = d.cw > 0 && d.ch > 0;
  VEP_CHECK(d.cw >= 0 && d.ch >= 0 && (d.cw > 0) == (d.ch > 0), "scale: bad cell");
  if (cell)
    VEP_CHECK(d.cx >= 0 && d.cy >= 0 && d.cx <= canvas_w - d.cw && d.cy <= canvas_h - d.ch,
              "scale: cell outside the canvas");
  if (!d.src) return;
  VEP_CHECK(d.sw >= 1 && d.sh >= 1 && d.sw <= scale::kMaxSide && d.sh <= scale::kMaxSide,
            "scale: source size out of range");
  VEP_CHECK(d.ow >= 1 && d.oh >= 1 && d.ow <= d.sw && d.oh <= d.sh,
            "scale: output must be 1..source size (no upscaling)");
  VEP_CHECK(u64(d.src_pitch) >= u64(d.sw) * 3, "scale: source pitch shorter than a row");
  if (cell)
    VEP_CHECK(d.dx >= d.cx && d.dy >= d.cy && d.dx <= d.cx + d.cw - d.ow && d.dy <= d.cy + d.ch - d.oh,
              "scale: picture outside its cell");
  else
    VEP_CHECK(d.dx >= 0 && d.dy >= 0 && d.dx <= canvas_w - d.ow && d.dy <= canvas_h - d.oh,
              "scale: picture outside the canvas");
}

void launch_scale(const ScaleDesc* d_descs, const ScaleDesc* h_descs, int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= 65535, "scale: at most 65535 tiles per launch");
  u64 blocks = 0;
  u32 rows = 0;
  for (int i = 0; i < n; ++i) {
    const ScaleDesc& d = h_descs[i];
    if (d.src) blocks = std::max(blocks, u64((u32(d.ow) + kThreads - 1) / kThreads) * u32(d.oh));
    if (d.cw > 0 && d.ch > 0) rows = std::max(rows, u32(d.ch));
  }
  if (blocks + rows == 0) return;
  VEP_CHECK(blocks + rows < (u64(1) << 31), "scale: launch too large");
  hipLaunchKernelGGL(scale_kernel, dim3(u32(blocks) + rows, u32(n)), dim3(kThreads), 0, s, d_descs, u32(blocks));
  VEP_HIP(hipGetLastError());
}

}  // namespace vep::gpu
