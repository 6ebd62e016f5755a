// gfx950 (CDNA4) temporal denoising of a served picture from its camera's history. See gpu.h for
// the contract and denoise.h for the arithmetic, which the CPU implementation (denoise.cpp) shares:
// both produce the same bytes. ONE launch for every picture of a request: blockIdx.y is the
// picture, blockIdx.x a 64 x 16 tile of it (a block past its own picture's tiles exits). 8-bit
// differences and small integer weights: there is no matrix-instruction work here.
//
// A block stages its tile with a halo of one pixel, 18 rows of 66 pixels, clipped to the picture
// (stage::stage_rows: any address and pitch, no byte outside a row's own bytes is read); the halo
// outside the picture is clamped in the INDICES. A wave owns four consecutive rows of the tile and a
// lane one column of them, so a lane needs the luma differences of six rows: its four and the one
// above and below.
//
//   newest frame   staged once. A lane keeps the six lumas of its column in registers, and one more
//                  for the wave's halo columns (below); its four pixels start the accumulators: three
//                  channel sums and W per pixel, in registers for the whole kernel.
//   earlier frame  the lane forms |Y_0 - Y_k| for its six rows. The three-sum along the row takes
//                  the two neighbours' values by wave shuffles; what lanes 0 and 63 lack, the halo
//                  columns left and right of the tile, is computed once per wave by lanes 0 .. 11
//                  (six rows, two sides) and broadcast. The three-sums are added down the column
//                  in registers, the weight follows (the division by 9 T is a multiplication by
//                  its reciprocal, denoise.h), and the frame's four pixels, already in registers
//                  from the luma, are folded in. No LDS plane of differences and no barrier
//                  inside a frame.
//   pipeline       two staging buffers. The loads of frame k + 1 are issued (stage_rows into the
//                  other buffer) before the arithmetic on frame k, and ONE barrier per frame
//                  separates them from their use: while a wave waits for its loads, the block's
//                  other waves compute on frame k.
//   output         (sum + W / 2) / W by a table of reciprocals in LDS (denoise.h proves it exact), into
//                  LDS at the DESTINATION address modulo 16, out with stage::store_rows: no byte
//                  outside the destination's rows is written. Out of place only.
//
// LDS: 2 x 4032 staging + 3328 output + 516 table = 11,908 bytes a block.
#define VEP_KERNEL_SOURCE 1  // descriptors' pointers are global-address-space here (gpu.h)
#include <algorithm>

#include "denoise.h"
#include "gpu.h"
#include "gpu_stage.h"

namespace vep::gpu {

namespace {

using stage::kRows;
using stage::kThreads;
using stage::kTileH;
using stage::kTileW;
using stage::kWaves;
constexpr u32 kHaloW = kTileW + 2, kHaloH = kTileH + 2;  // 66 x 18
constexpr u32 kInCap = stage::rowcap_of(kHaloW);        // 224: a staged row
constexpr u32 kInBytes = kHaloH * kInCap;               // 4032
constexpr u32 kOutCap = stage::kTileRowCap;
constexpr u32 kLaneRows = kRows + 2;                    // a lane's rows with the one above and below
constexpr u32 kTable = denoise::kMaxWeightSum + 1;
static_assert(kTileW == 64, "a wave spans a tile's row: the shuffles below");
static_assert(kWaves * kRows == kTileH, "a wave owns kRows consecutive rows");
static_assert(2 * kLaneRows <= 64, "the halo columns of a wave's rows have a lane each");
static_assert((kHaloH - 1) * kInCap + 15 + kHaloW * 3 <= kInBytes, "the staged tile fits its buffer");
static_assert(kTable <= kThreads, "one table entry per thread");

__device__ const denoise::WeightSumTable kRecipW = denoise::weight_sum_table();

__global__ __launch_bounds__(kThreads) void denoise_kernel(const DenoiseDesc* __restrict__ descs) {
  __shared__ __attribute__((aligned(16))) u8 in[2][kInBytes];
  __shared__ __attribute__((aligned(16))) u8 outb[kTileH * kOutCap];
  __shared__ u32 recip_w[kTable];
  const DenoiseDesc& d = descs[blockIdx.y];
  const u32 w = u32(d.w), h = u32(d.h);
  const u32 bx = blockIdx.x;
  if (bx >= stage::tiles_of(w, h)) return;
  const u32 ntx = stage::tiles_x(w);
  const u32 tk = bx / ntx, tj = bx - tk * ntx;
  const u32 j0 = tj * kTileW, j1 = min(w, j0 + kTileW);
  const u32 k0 = tk * kTileH, k1 = min(h, k0 + kTileH);
  // the staged window: the tile and its halo, clipped to the picture
  const u32 xs = j0 ? j0 - 1 : 0, xe = min(w, j1 + 1);
  const u32 ys = k0 ? k0 - 1 : 0, ye = min(h, k1 + 1);
  const u32 nr = ye - ys, nin = (xe - xs) * 3;
  const u32 frames = u32(d.frames), strength = u32(d.strength), recip9t = d.recip9t;
  const u32 t = threadIdx.x;
  if (t < kTable) recip_w[t] = kRecipW.r[t];
  stage::stage_rows(d.src[0], d.src_pitch[0], ys, nr, xs, nin, kInCap, in[0]);
  if (frames > 1) stage::stage_rows(d.src[1], d.src_pitch[1], ys, nr, xs, nin, kInCap, in[1]);
  __syncthreads();

  // The lane's column and six rows, clamped to the picture (so every lane of every wave reads staged
  // bytes, and the shuffles below run in all of them), as offsets into the staged window.
  const u32 c = t & (kTileW - 1), q = t / kTileW;
  const u32 px = min(j0 + c, w - 1) - xs;
  u32 row[kLaneRows];
#pragma unroll
  for (u32 i = 0; i < kLaneRows; ++i) row[i] = u32(min(max(int(k0 + q * kRows + i) - 1, 0), int(h - 1))) - ys;
  // The wave's halo columns: lane l < 12 serves row l % 6 of the left (l < 6) or right side.
  const u32 ei = c % kLaneRows;
  const u32 erow = u32(min(max(int(k0 + q * kRows + ei) - 1, 0), int(h - 1))) - ys;
  const u32 epx = ((c / kLaneRows) & 1u ? min(j0 + kTileW, w - 1) : xs) - xs;  // (xs is clamp(j0 - 1))
  // a staged pixel of the frame at `sp`: its row's bytes keep their address modulo 16
  auto pixel = [&](const u8* buf, const VEP_DEV u8* sp, u32 pitch, u32 r, u32 x) -> const u8* {
    const u32 mis = (u32(reinterpret_cast<uintptr_t>(sp)) + (ys + r) * pitch + xs * 3) & 15u;
    return buf + r * kInCap + mis + x * 3;
  };

  u32 y0[kLaneRows], y0e;
  u32 acc[kRows][4];
  {
    const VEP_DEV u8* sp = d.src[0];
    const u32 pitch = d.src_pitch[0];
#pragma unroll
    for (u32 i = 0; i < kLaneRows; ++i) {
      const u8* p = pixel(in[0], sp, pitch, row[i], px);
      const u32 b0 = p[0], b1 = p[1], b2 = p[2];
      y0[i] = motion::luma(b0, b1, b2);
      if (i >= 1 && i <= kRows) {
        acc[i - 1][0] = denoise::kFull * b0;
        acc[i - 1][1] = denoise::kFull * b1;
        acc[i - 1][2] = denoise::kFull * b2;
        acc[i - 1][3] = denoise::kFull;
      }
    }
    const u8* p = pixel(in[0], sp, pitch, erow, epx);
    y0e = motion::luma(p[0], p[1], p[2]);
  }
  __syncthreads();  // (frame 2 is staged over the newest frame)

  for (u32 k = 1; k < frames; ++k) {
    const u8* cur = in[k & 1u];
    // the loads of the next frame first: into the buffer whose frame every wave has finished
    if (k + 1 < frames) stage::stage_rows(d.src[k + 1], d.src_pitch[k + 1], ys, nr, xs, nin, kInCap, in[(k + 1) & 1u]);
    const VEP_DEV u8* sp = d.src[k];
    const u32 pitch = d.src_pitch[k];
    u32 ad[kLaneRows], f[kRows][3];
#pragma unroll
    for (u32 i = 0; i < kLaneRows; ++i) {
      const u8* p = pixel(cur, sp, pitch, row[i], px);
      const u32 b0 = p[0], b1 = p[1], b2 = p[2];
      const u32 y = motion::luma(b0, b1, b2);
      ad[i] = y > y0[i] ? y - y0[i] : y0[i] - y;
      if (i >= 1 && i <= kRows) {
        f[i - 1][0] = b0;
        f[i - 1][1] = b1;
        f[i - 1][2] = b2;
      }
    }
    const u8* p = pixel(cur, sp, pitch, erow, epx);
    const u32 ye_ = motion::luma(p[0], p[1], p[2]);
    const u32 ade = ye_ > y0e ? ye_ - y0e : y0e - ye_;
    u32 hs[kLaneRows];  // three-sums along the row
#pragma unroll
    for (u32 i = 0; i < kLaneRows; ++i) {
      const u32 left = u32(__shfl_up(int(ad[i]), 1)), right = u32(__shfl_down(int(ad[i]), 1));
      const u32 halo_l = u32(__shfl(int(ade), int(i))), halo_r = u32(__shfl(int(ade), int(kLaneRows + i)));
      hs[i] = (c == 0 ? halo_l : left) + ad[i] + (c == kTileW - 1 ? halo_r : right);
    }
#pragma unroll
    for (u32 m = 0; m < kRows; ++m) {
      const u32 wk = denoise::weight_fast(hs[m] + hs[m + 1] + hs[m + 2], recip9t, strength);
      acc[m][0] += wk * f[m][0];
      acc[m][1] += wk * f[m][1];
      acc[m][2] += wk * f[m][2];
      acc[m][3] += wk;
    }
    __syncthreads();  // (the next frame is staged; this one's buffer is free)
  }

  VEP_DEV u8* out0 = d.dst + u64(k0) * d.dst_pitch + u64(j0) * 3;  // the tile's origin in the destination
  const u32 dst_pitch = d.dst_pitch, nrow = k1 - k0, nout = (j1 - j0) * 3;
  if (j0 + c < j1) {
#pragma unroll
    for (u32 m = 0; m < kRows; ++m) {
      const u32 rr = q * kRows + m;
      if (rr >= nrow) continue;
      const u32 ws = acc[m][3], rw = recip_w[ws], half = ws >> 1;
      u8* o = outb + rr * kOutCap + (u32(reinterpret_cast<uintptr_t>(out0 + u64(rr) * dst_pitch)) & 15u) + c * 3;
      o[0] = u8(denoise::div_by(acc[m][0] + half, rw));
      o[1] = u8(denoise::div_by(acc[m][1] + half, rw));
      o[2] = u8(denoise::div_by(acc[m][2] + half, rw));
    }
  }
  __syncthreads();
  stage::store_rows(out0, dst_pitch, nrow, nout, kOutCap, outb);
}

}  // namespace

void launch_denoise(const DenoiseDesc* d_descs, const DenoiseDesc* h_descs, int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= 65535, "denoise: at most 65535 pictures per launch");
  u64 blocks = 0;
  for (int i = 0; i < n; ++i) blocks = std::max(blocks, u64(stage::tiles_of(u32(h_descs[i].w), u32(h_descs[i].h))));
  VEP_CHECK(blocks >= 1 && blocks < (u64(1) << 31), "denoise: launch too large");
  hipLaunchKernelGGL(denoise_kernel, dim3(u32(blocks), u32(n)), dim3(kThreads), 0, s, d_descs);
  VEP_HIP(hipGetLastError());
}

}  // namespace vep::gpu
