// What the two kernels on a cell grid share (motion, gpu_motion.hip; tamper, gpu_tamper.hip): the
// chunk of cell columns a block owns, the proof that every chunk fits a kernel's limits, and the
// lumas of a group of 8 pixels out of staged rows (gpu_stage.h). Kernel sources only.
#pragma once

#include "gpu_stage.h"
#include "motion.h"

namespace vep::gpu::cells {

constexpr u32 kChunkPix = 512;  // a chunk is at most this wide, or one lcm(cell, 8) where that is wider

// Pixels of a chunk: the largest multiple of lcm(cell, 8) that is <= kChunkPix, at least one. So a
// chunk starts at a cell boundary and at a multiple of 8 pixels.
__host__ __device__ constexpr u32 chunk_of(u32 cell) {
  const u32 low = cell & (0u - cell);
  const u32 unit = cell / (low < 8u ? low : 8u) * 8u;  // lcm(cell, 8)
  return unit >= kChunkPix ? unit : kChunkPix / unit * unit;
}
// Every cell in lo..hi: a chunk is whole cells and whole groups of 8 pixels, at most max_cells of
// the one and max_groups of the other, and min_rows rows of it fit the staging buffer.
constexpr bool chunks_fit(u32 lo, u32 hi, u32 max_cells, u32 max_groups, u32 min_rows) {
  for (u32 cell = lo; cell <= hi; ++cell) {
    const u32 chunk = chunk_of(cell);
    if (chunk % cell || chunk % 8u) return false;
    if (chunk / cell > max_cells) return false;
    if (chunk / 8u > max_groups) return false;
    if (stage::kLdsBytes / stage::rowcap_of(chunk) < min_rows) return false;
  }
  return true;
}

// Lumas of four pixels out of their 12 bytes B G R B | G R B G | R B G R.
__device__ __forceinline__ void luma4(u32 r0, u32 r1, u32 r2, u32& y0, u32& y1, u32& y2, u32& y3) {
  y0 = motion::luma(r0 & 255u, (r0 >> 8) & 255u, (r0 >> 16) & 255u);
  y1 = motion::luma(r0 >> 24, r1 & 255u, (r1 >> 8) & 255u);
  y2 = motion::luma((r1 >> 16) & 255u, r1 >> 24, r2 & 255u);
  y3 = motion::luma((r2 >> 8) & 255u, (r2 >> 16) & 255u, r2 >> 24);
}

// The lumas of the n <= 8 pixels of a group at LDS offset `off`; pixels past n are 0. With
// kNinth, y[8] is the next pixel's (only meaningful where that pixel is staged: the caller masks
// it).
template <bool kNinth>
__device__ __forceinline__ void lumas(const u8* lds, u32 off, u32 n, u32 (&y)[kNinth ? 9 : 8]) {
  if (n == 8) {
    // 24 (27) bytes out of seven (eight) aligned LDS dwords, realigned. The last dwords may lie
    // up to 4 (8) bytes past the row: inside the buffer's padding.
    const u32 sh = off & 3u;
    const u32* q = reinterpret_cast<const u32*>(lds + (off & ~3u));
    const u32 d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = q[4], d5 = q[5], d6 = q[6];
    luma4(__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
          __builtin_amdgcn_alignbyte(d3, d2, sh), y[0], y[1], y[2], y[3]);
    luma4(__builtin_amdgcn_alignbyte(d4, d3, sh), __builtin_amdgcn_alignbyte(d5, d4, sh),
          __builtin_amdgcn_alignbyte(d6, d5, sh), y[4], y[5], y[6], y[7]);
    if constexpr (kNinth) {
      const u32 r = __builtin_amdgcn_alignbyte(q[7], d6, sh);
      y[8] = motion::luma(r & 255u, (r >> 8) & 255u, (r >> 16) & 255u);
    }
  } else {
    // the partial group at the picture's right edge: only its own bytes
#pragma unroll
    for (u32 i = 0; i < 8; ++i) {
      y[i] = 0;
      if (i < n) {
        const u8* p = lds + off + i * 3;
        y[i] = motion::luma(p[0], p[1], p[2]);
      }
    }
    if constexpr (kNinth) y[8] = 0;
  }
}

}  // namespace vep::gpu::cells
