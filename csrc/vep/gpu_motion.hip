// gfx950 (CDNA4) motion detection. See gpu.h for the contract and motion.h for the arithmetic,
// which the CPU implementation (motion.cpp) shares: both produce the same bytes.
//
// One launch covers every picture: blockIdx.y is the picture, blockIdx.x a block of it (a block
// past its own picture's work exits).
//
// A block owns whole cells: one row of the cell grid (`cell` pixel rows) and a chunk of its
// columns. A chunk is a multiple of lcm(cell, 8) pixels wide, so it starts at a cell boundary and
// at a 16-byte boundary of the background rows (8 u16 samples). The kernel is a pure stream: per
// pixel 3 bytes of source and 2 of background in, 2 of background out. The block stages the source
// rows of a pass in LDS (stage::stage_rows, gpu_stage.h: a byte keeps its address modulo 16). A
// thread then takes groups of 8 pixels: 24 source bytes out of aligned LDS dwords, one 16-byte
// background vector in and one out. The chunk geometry and the groups' lumas are the tamper
// kernel's too and live in gpu_cells.h. The group's changed pixels are added to the block's
// per-cell counters in LDS (integer atomics: the sum does not depend on the order), and when the
// block's rows are done every cell of the block is written once by a plain store, zeros
// included. Nothing in global memory is written twice or by two blocks.
//
// check_motion() proves on the host that every access lies inside the source rows, the two
// background planes and the counts array.
#define VEP_KERNEL_SOURCE 1  // descriptors' pointers are global-address-space here (gpu.h)
#include <algorithm>

#include "gpu.h"
#include "gpu_cells.h"
#include "motion.h"

namespace vep::gpu {

namespace {

using cells::chunk_of;
using stage::kLdsBytes;
using stage::kThreads;
constexpr u32 kMaxItems = 4;    // 8-pixel groups of a thread per pass
constexpr u32 kMaxCells = cells::kChunkPix / u32(motion::kMinCell);  // cells of a chunk
// Every cell in 4..256: a chunk has at most kMaxCells cells, a pass of one row has at most
// kThreads * kMaxItems groups, and a row of the widest chunk fits the staging buffer.
static_assert(cells::chunks_fit(u32(motion::kMinCell), u32(motion::kMaxCell), kMaxCells, kThreads * kMaxItems, 1),
              "chunk geometry");

__global__ __launch_bounds__(kThreads) void motion_kernel(const MotionDesc* __restrict__ descs) {
  __shared__ __attribute__((aligned(16))) u8 lds[kLdsBytes + 16];  // (+ 16: the groups' dword reads)
  __shared__ u32 cnt[kMaxCells];
  const MotionDesc& d = descs[blockIdx.y];
  // (every field is read into a register once: the descriptor itself stays in global memory)
  const u32 w = u32(d.w), h = u32(d.h), cell = u32(d.cell);
  const u32 chunk = chunk_of(cell);
  const u32 nch = (w + chunk - 1) / chunk;
  const u32 bx = blockIdx.x;
  if (bx >= nch * motion::cells(h, cell)) return;
  const VEP_DEV u8* src = d.src;
  const VEP_DEV u16* bg_in = d.bg_in;
  VEP_DEV u16* bg_out = d.bg_out;
  const u32 src_pitch = d.src_pitch, bg_pitch = d.bg_pitch;
  const u32 threshold = u32(d.threshold), learn_shift = u32(d.learn_shift);
  const u32 gy = bx / nch, c = bx - gy * nch;
  const u32 x0 = c * chunk, x1 = min(w, x0 + chunk);     // the block's pixel columns
  const u32 y0 = gy * cell, y1 = min(h, y0 + cell);      // and rows
  const u32 cw = x1 - x0, nbytes = cw * 3;
  const u32 gpr = (cw + 7) >> 3;                         // 8-pixel groups per row
  const u32 rowcap = stage::rowcap_of(cw);
  const u32 rpp = min(kLdsBytes / rowcap, kThreads * kMaxItems / gpr);  // rows per pass, >= 1 (chunks_fit)
  const u32 ncell = (cw + cell - 1) / cell;
  const u32 t = threadIdx.x;
  for (u32 i = t; i < ncell; i += kThreads) cnt[i] = 0;  // (the first pass's barrier orders this)
  const bool primed = bg_in != nullptr;
  for (u32 rb = y0; rb < y1; rb += rpp) {
    const u32 nr = min(rpp, y1 - rb);
    const u32 total = nr * gpr;
    stage::stage_rows(src, src_pitch, rb, nr, x0, nbytes, rowcap, lds);
    uint4 b[kMaxItems];
#pragma unroll
    for (u32 k = 0; k < kMaxItems; ++k) {
      const u32 item = t + k * kThreads;
      b[k] = uint4{0, 0, 0, 0};
      if (primed && item < total) {
        const u32 rr = item / gpr, g = item - rr * gpr;
        // (the last group of a row may read padding samples: inside the row's pitch)
        b[k] = *reinterpret_cast<const VEP_DEV uint4*>(bg_in + u64(rb + rr) * bg_pitch + x0 + g * 8);
      }
    }
    __syncthreads();
#pragma unroll
    for (u32 k = 0; k < kMaxItems; ++k) {
      const u32 item = t + k * kThreads;
      if (item >= total) continue;
      const u32 rr = item / gpr, g = item - rr * gpr;
      const u32 px = x0 + g * 8, n = min(8u, x1 - px);
      const VEP_DEV u8* grow = src + u64(rb + rr) * src_pitch + u64(x0) * 3;
      const u32 off = rr * rowcap + (u32(reinterpret_cast<uintptr_t>(grow)) & 15u) + g * 24;
      u32 y[8];
      cells::lumas<false>(lds, off, n, y);
      const u32 bw[4] = {b[k].x, b[k].y, b[k].z, b[k].w};
      u32 o[8];
      u32 ci = (px - x0) / cell, rem = (px - x0) - ci * cell, run = 0;
#pragma unroll
      for (u32 i = 0; i < 8; ++i) {
        if (primed) {
          const u32 bg = (bw[i >> 1] >> ((i & 1u) * 16)) & 0xffffu;
          o[i] = motion::update(bg, y[i], learn_shift);
          if (i < n) {
            run += motion::changed(y[i], motion::ref_of(bg), threshold) ? 1u : 0u;
            if (++rem == cell) {  // the group crosses into the next cell
              if (run) atomicAdd(&cnt[ci], run);
              ++ci;
              rem = 0;
              run = 0;
            }
          }
        } else {
          o[i] = motion::prime(y[i]);
        }
      }
      if (run) atomicAdd(&cnt[ci], run);
      VEP_DEV u16* out = bg_out + u64(rb + rr) * bg_pitch + px;
      if (n == 8) {
        *reinterpret_cast<VEP_DEV uint4*>(out) =
            uint4{o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16)};
      } else {
        // (never the padding samples)
#pragma unroll
        for (u32 i = 0; i < 8; ++i)
          if (i < n) out[i] = u16(o[i]);
      }
    }
    __syncthreads();
  }
  VEP_DEV u32* counts = d.counts + u64(gy) * motion::cells(w, cell) + x0 / cell;
  for (u32 i = t; i < ncell; i += kThreads) counts[i] = cnt[i];
}

}  // namespace

void check_motion(const MotionDesc& d, size_t src_bytes, size_t bg_samples, size_t count_cells) {
  VEP_CHECK(d.src && d.bg_out && d.counts, "motion: null source, background or counts");
  VEP_CHECK(d.w >= 1 && d.h >= 1 && d.w <= motion::kMaxSide && d.h <= motion::kMaxSide,
            "motion: picture size must be 1..65535");
  motion::check_update_params(d.cell, d.threshold, d.learn_shift);
  const u64 w = u64(d.w), h = u64(d.h);
  VEP_CHECK(u64(d.src_pitch) >= w * 3, "motion: source pitch shorter than a row");
  VEP_CHECK((h - 1) * d.src_pitch + w * 3 <= src_bytes, "motion: source rows outside the source");
  // a row's vectors cover samples 0 .. pitch_for(w) (loads; stores stop at w)
  VEP_CHECK(d.bg_pitch % 8 == 0 && d.bg_pitch >= motion::pitch_for(u32(d.w)),
            "motion: background pitch must be a multiple of 8 samples and hold a row");
  VEP_CHECK(h * d.bg_pitch <= bg_samples, "motion: background rows outside the plane");
  const uintptr_t in = reinterpret_cast<uintptr_t>(d.bg_in), out = reinterpret_cast<uintptr_t>(d.bg_out);
  VEP_CHECK(in % 16 == 0 && out % 16 == 0, "motion: background planes must be 16-byte aligned");
  const u64 plane = bg_samples * sizeof(u16);
  VEP_CHECK(!d.bg_in || in + plane <= out || out + plane <= in, "motion: the background planes overlap");
  VEP_CHECK(reinterpret_cast<uintptr_t>(d.counts) % 4 == 0, "motion: counts must be 4-byte aligned");
  VEP_CHECK(u64(motion::cells(u32(d.w), u32(d.cell))) * motion::cells(u32(d.h), u32(d.cell)) <= count_cells,
            "motion: the grid does not fit the counts array");
}

void launch_motion(const MotionDesc* d_descs, const MotionDesc* h_descs, int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= 65535, "motion: at most 65535 pictures per launch");
  u64 blocks = 0;
  for (int i = 0; i < n; ++i) {
    const MotionDesc& d = h_descs[i];
    const u32 chunk = chunk_of(u32(d.cell));
    blocks = std::max(blocks, u64((u32(d.w) + chunk - 1) / chunk) * motion::cells(u32(d.h), u32(d.cell)));
  }
  VEP_CHECK(blocks >= 1 && blocks < (u64(1) << 31), "motion: launch too large");
  hipLaunchKernelGGL(motion_kernel, dim3(u32(blocks), u32(n)), dim3(kThreads), 0, s, d_descs);
  VEP_HIP(hipGetLastError());
}

}  // namespace vep::gpu
