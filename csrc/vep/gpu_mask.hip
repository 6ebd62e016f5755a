// gfx950 (CDNA4) privacy masks. See gpu.h for the contract and mask.h for the arithmetic, which the
// CPU implementation (mask.cpp) shares: both produce the same bytes.
//
// One launch covers the masks of one level of every picture of a batch: blockIdx.y is the
// descriptor (a descriptor of another level exits), blockIdx.x a workgroup of its rect (one past
// the rect's work exits). Masks of one level of one picture are disjoint (mask::levels), and kernel
// boundaries on the stream order the levels.
//
// A workgroup owns whole blocks: a strip of `block` pixel rows of the rect (fill: 16 rows) and a
// chunk of its columns, a whole number of blocks and at most 512 pixels wide, so a chunk starts at
// a block boundary. A block's pixels are read and written by that workgroup alone, so working in
// place is race-free.
//
// Pixelate, pass 1: a thread owns one column of 4 pixels of the chunk and every nseg-th row of the
// strip. It reads the 12 bytes of a row out of three or four ALIGNED dwords, realigned in
// registers (a rect starts at any byte offset modulo 4); a dword that does not lie wholly inside
// the picture is put together from the picture's own bytes one by one, so nothing outside the
// picture is read. A column of 4 pixels lies in at most two blocks (block >= 4), split at a
// position that is fixed per thread; the per-channel sums of the two blocks stay in registers over
// the rows and reach the workgroup's LDS counters once, by integer atomics (the sum does not
// depend on the order). One thread per block and channel then computes mask::block_value.
//
// Pass 2 (both modes) writes the strip's rows: 16-byte stores to 16-byte aligned addresses, the
// value of every byte looked up by its pixel's block and its channel, and the unaligned head and
// tail of every row byte by byte (the split of a row is stage::split_row, gpu_stage.h, which the
// staging kernels share; the bytes are generated here, not copied, so the store itself is this
// kernel's own). Bytes outside the rect are NOT WRITTEN AT ALL: a byte that
// shares a dword or a 16-byte vector with the rect belongs to the bytewise head or tail of its
// neighbour, never to a wide store. No float is involved anywhere.
//
// check_mask() proves on the host that every access lies inside the picture.
#define VEP_KERNEL_SOURCE 1  // descriptors' pointers are global-address-space here (gpu.h)
#include <algorithm>

#include "gpu.h"
#include "gpu_stage.h"
#include "mask.h"

namespace vep::gpu {

namespace {

using stage::kThreads;
constexpr u32 kChunkPix = 512;  // a chunk is at most this wide
constexpr u32 kFillRows = 16;   // rows of a fill strip
constexpr u32 kMaxBlocks = kChunkPix / u32(mask::kMinBlock);  // blocks of a chunk
constexpr u32 kNoBlock = 0x7fffffffu;  // fill: every pixel of the chunk is in "block" 0
static_assert(kChunkPix >= u32(mask::kMaxBlock), "a chunk holds at least one block");
static_assert(kChunkPix / 4 * 2 <= kThreads, "every column of 4 pixels has at least two row segments");

// Rows of a strip and pixels of a chunk.
__host__ __device__ inline u32 strip_rows(i32 mode, u32 block) { return mode == mask::kPixelate ? block : kFillRows; }
__host__ __device__ inline u32 chunk_pix(i32 mode, u32 block) {
  return mode == mask::kPixelate ? kChunkPix / block * block : kChunkPix;
}
__host__ __device__ inline u32 groups_of(const MaskDesc& d) {
  const u32 sr = strip_rows(d.mode, u32(d.block)), cp = chunk_pix(d.mode, u32(d.block));
  return ((u32(d.x1 - d.x0) + cp - 1) / cp) * ((u32(d.y1 - d.y0) + sr - 1) / sr);
}

// The aligned dword at q, of which only the bytes inside [lo, hi) are read (the others are 0).
__device__ __forceinline__ u32 dword_inside(u64 q, u64 lo, u64 hi) {
  if (q >= lo && q + 4 <= hi) return *reinterpret_cast<const VEP_DEV u32*>(q);
  u32 v = 0;
#pragma unroll
  for (u32 i = 0; i < 4; ++i)
    if (q + i >= lo && q + i < hi) v |= u32(*reinterpret_cast<const VEP_DEV u8*>(q + i)) << (8 * i);
  return v;
}

__global__ __launch_bounds__(kThreads) void mask_kernel(const MaskDesc* __restrict__ descs, int level) {
  __shared__ u32 sums[kMaxBlocks * 3];
  __shared__ u32 vals[kMaxBlocks * 3];
  const MaskDesc& d = descs[blockIdx.y];
  if (d.level != level) return;
  // (every field is read into a register once: the descriptor itself stays in global memory)
  const i32 mode = d.mode;
  const u32 B = u32(d.block);
  const u32 rx0 = u32(d.x0), ry0 = u32(d.y0), rx1 = u32(d.x1), ry1 = u32(d.y1);
  const u32 sr = strip_rows(mode, B), cp = chunk_pix(mode, B);
  const u32 nch = (rx1 - rx0 + cp - 1) / cp, nst = (ry1 - ry0 + sr - 1) / sr;
  const u32 bx = blockIdx.x;
  if (bx >= nch * nst) return;
  VEP_DEV u8* dst = d.dst;
  const u32 pitch = d.pitch;
  const u64 lo = reinterpret_cast<u64>(dst);
  const u64 hi = lo + u64(u32(d.h) - 1) * pitch + u64(u32(d.w)) * 3;  // the picture's bytes
  const u32 fill = d.bgr;
  const u32 st = bx / nch, c = bx - st * nch;
  const u32 cx0 = rx0 + c * cp, cx1 = min(rx1, cx0 + cp);  // the workgroup's pixel columns
  const u32 sy0 = ry0 + st * sr, sy1 = min(ry1, sy0 + sr);  // and rows
  const u32 cw = cx1 - cx0, nr = sy1 - sy0, nbytes = cw * 3;
  const u32 bdiv = mode == mask::kPixelate ? B : kNoBlock;
  const u32 nblk = mode == mask::kPixelate ? (cw + B - 1) / B : 1u;  // <= kMaxBlocks
  const u32 t = threadIdx.x;
  if (mode == mask::kPixelate) {
    for (u32 i = t; i < nblk * 3; i += kThreads) sums[i] = 0;
    __syncthreads();
    const u32 ngrp = (cw + 3) >> 2;       // columns of 4 pixels, <= kThreads / 2
    const u32 nseg = kThreads / ngrp;     // row segments
    const u32 s = t / ngrp, g = t - s * ngrp;
    if (s < nseg) {
      const u32 p0 = g * 4, n = min(4u, cw - p0);
      // The column's pixels i < split lie in block bi, the others in block bi + 1.
      const u32 bi = p0 / B;
      const u32 split = min(4u, B - (p0 - bi * B));
      u32 sa0 = 0, sa1 = 0, sa2 = 0, sb0 = 0, sb1 = 0, sb2 = 0;
      for (u32 row = sy0 + s; row < sy1; row += nseg) {
        const u64 a = lo + u64(row) * pitch + u64(cx0 + p0) * 3;
        const u32 sh = u32(a) & 3u;
        const u64 q = a - sh;
        // 12 bytes B G R B | G R B G | R B G R out of aligned dwords. Dwords past the column's own
        // bytes are not needed (n < 4) or not read (outside the picture).
        const u32 d0 = dword_inside(q, lo, hi);
        const u32 d1 = (n * 3 + sh > 4) ? dword_inside(q + 4, lo, hi) : 0u;
        const u32 d2 = (n * 3 + sh > 8) ? dword_inside(q + 8, lo, hi) : 0u;
        const u32 d3 = (n * 3 + sh > 12) ? dword_inside(q + 12, lo, hi) : 0u;
        const u32 r0 = __builtin_amdgcn_alignbyte(d1, d0, sh), r1 = __builtin_amdgcn_alignbyte(d2, d1, sh),
                  r2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
        const u32 pb[4] = {r0 & 255u, r0 >> 24, (r1 >> 16) & 255u, (r2 >> 8) & 255u};
        const u32 pg[4] = {(r0 >> 8) & 255u, r1 & 255u, r1 >> 24, (r2 >> 16) & 255u};
        const u32 pr[4] = {(r0 >> 16) & 255u, (r1 >> 8) & 255u, r2 & 255u, r2 >> 24};
#pragma unroll
        for (u32 i = 0; i < 4; ++i) {
          if (i >= n) continue;
          if (i < split) {
            sa0 += pb[i];
            sa1 += pg[i];
            sa2 += pr[i];
          } else {
            sb0 += pb[i];
            sb1 += pg[i];
            sb2 += pr[i];
          }
        }
      }
      // the column's two blocks; the second one exists where the column has pixels past the split
      atomicAdd(&sums[bi * 3 + 0], sa0);
      atomicAdd(&sums[bi * 3 + 1], sa1);
      atomicAdd(&sums[bi * 3 + 2], sa2);
      if (split < n) {
        atomicAdd(&sums[bi * 3 + 3], sb0);
        atomicAdd(&sums[bi * 3 + 4], sb1);
        atomicAdd(&sums[bi * 3 + 5], sb2);
      }
    }
    __syncthreads();
    for (u32 i = t; i < nblk * 3; i += kThreads) {
      const u32 b = i / 3;
      const u32 bw = min(B, cw - b * B);
      vals[i] = mask::block_value(sums[i], bw * nr);
    }
  } else if (t < 3) {
    vals[t] = (fill >> (8 * t)) & 255u;
  }
  __syncthreads();
  // Pass 2: the strip's rows. Row rr's bytes start at row_ptr(rr); the bytes before its first and
  // after its last whole 16-byte vector go byte by byte (stage::split_row).
  auto row_ptr = [&](u32 rr) -> VEP_DEV u8* { return dst + u64(sy0 + rr) * pitch + u64(cx0) * 3; };
  const u32 vpr = (nbytes >> 4) + 1;  // upper bound of a row's 16-byte vectors
  const u32 total = nr * vpr;
  for (u32 item = t; item < total; item += kThreads) {
    const u32 rr = item / vpr, v = item - rr * vpr;
    VEP_DEV u8* gp = row_ptr(rr);
    const stage::RowSplit r = stage::split_row(gp, nbytes);
    if (v >= r.nvec) continue;
    const u32 o = r.head + v * 16;  // o + 16 <= nbytes
    u32 p = o / 3, ch = o - p * 3;
    u32 blk = p / bdiv, rem = p - blk * bdiv;
    u32 w4[4];
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
      u32 x = 0;
#pragma unroll
      for (u32 i = 0; i < 4; ++i) {
        x |= vals[blk * 3 + ch] << (8 * i);
        if (++ch == 3) {
          ch = 0;
          if (++rem == bdiv) {
            rem = 0;
            ++blk;
          }
        }
      }
      w4[k] = x;
    }
    uint4 out;
    out.x = w4[0];
    out.y = w4[1];
    out.z = w4[2];
    out.w = w4[3];
    *reinterpret_cast<VEP_DEV uint4*>(gp + o) = out;
  }
  // 32 byte slots per row (16 of the head, 16 of the tail), 8 rows per step
  for (u32 rr = t >> 5; rr < nr; rr += kThreads / 32) {
    VEP_DEV u8* gp = row_ptr(rr);
    u32 o;
    if (!stage::edge_byte(stage::split_row(gp, nbytes), nbytes, t & 31u, o)) continue;
    const u32 p = o / 3, ch = o - p * 3;
    gp[o] = u8(vals[(p / bdiv) * 3 + ch]);
  }
}

}  // namespace

void check_mask(const MaskDesc& d, size_t dst_bytes) {
  VEP_CHECK(d.dst, "mask: null picture");
  VEP_CHECK(d.w >= 1 && d.h >= 1 && d.w <= mask::kMaxSide && d.h <= mask::kMaxSide,
            "mask: picture size must be 1..65535");
  const u64 w = u64(d.w), h = u64(d.h);
  VEP_CHECK(u64(d.pitch) >= w * 3, "mask: pitch shorter than a row");
  VEP_CHECK((h - 1) * d.pitch + w * 3 <= dst_bytes, "mask: picture rows outside the picture's memory");
  VEP_CHECK(d.x0 >= 0 && d.x0 < d.x1 && d.x1 <= d.w && d.y0 >= 0 && d.y0 < d.y1 && d.y1 <= d.h,
            "mask: rect empty or outside the picture");
  VEP_CHECK(d.mode == mask::kFill || d.mode == mask::kPixelate, "mask: unknown mode");
  VEP_CHECK(d.block >= mask::kMinBlock && d.block <= mask::kMaxBlock, "mask: block must be 4..128");
  VEP_CHECK(d.bgr <= 0xFFFFFFu, "mask: colour out of range");
  VEP_CHECK(d.level >= 0 && d.level < mask::kMaxMasks, "mask: level out of range");
}

void launch_mask(const MaskDesc* d_descs, const MaskDesc* h_descs, int n, int level, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= 65535, "mask: at most 65535 descriptors per launch");
  u64 blocks = 0;
  for (int i = 0; i < n; ++i)
    if (h_descs[i].level == level) blocks = std::max(blocks, u64(groups_of(h_descs[i])));
  if (!blocks) return;
  VEP_CHECK(blocks < (u64(1) << 31), "mask: launch too large");
  hipLaunchKernelGGL(mask_kernel, dim3(u32(blocks), u32(n)), dim3(kThreads), 0, s, d_descs, level);
  VEP_HIP(hipGetLastError());
}

}  // namespace vep::gpu
