// Staging rows of a packed BGR24 picture in LDS, summing samples out of them and storing rows
// back: the part the scale kernel (gpu_scale.hip), the crop kernel (gpu_crop.hip) and the overlay
// kernel (gpu_overlay.hip) share. Kernel sources only
// (VEP_KERNEL_SOURCE, 256 threads a workgroup).
//
// Packed BGR rows start at any byte address, so a row segment is staged with 16-byte loads from
// 16-byte aligned addresses and its unaligned head and tail byte by byte; nothing outside the
// segment's own bytes is read. A byte keeps its address modulo 16 in LDS, so the LDS stores are
// aligned too.
#pragma once

#include "gpu.h"

namespace vep::gpu::stage {

constexpr u32 kThreads = 256;

// Rows rb .. rb + nr of the source, pixels [is, is + nbytes / 3), into LDS: row rr at
// rr * rowcap + (its address modulo 16).
__device__ __forceinline__ void stage_rows(const VEP_DEV u8* src, u32 src_pitch, u32 rb, u32 nr, u32 is,
                                           u32 nbytes, u32 rowcap, u8* lds) {
  const u32 t = threadIdx.x;
  const u32 vpr = (nbytes >> 4) + 1;  // upper bound of a row's 16-byte vectors
  const u32 total = nr * vpr;
  // Every load of a pass is issued before the first LDS store, so a pass costs one memory
  // latency: the thread's head / tail byte, then up to six vectors (1080p -> 320x180 stages its
  // six rows of 2.9 KB in one pass).
  auto edge = [&](u32 rr, u8& x) -> u32 {  // a byte of row rr's unaligned head or tail
    const u32 slot = t & 31u;
    const VEP_DEV u8* g = src + u64(rb + rr) * src_pitch + u64(is) * 3;
    const u32 mis = u32(reinterpret_cast<uintptr_t>(g)) & 15u;
    const u32 head = min(nbytes, (16u - mis) & 15u);
    const u32 body = ((nbytes - head) >> 4) << 4;
    u32 o;
    if (slot < 16) {
      if (slot >= head) return ~0u;
      o = slot;
    } else {
      if (slot - 16 >= nbytes - head - body) return ~0u;
      o = head + body + (slot - 16);
    }
    x = g[o];
    return rr * rowcap + mis + o;
  };
  auto fetch = [&](u32 item, uint4& x) -> u32 {  // -> LDS offset, ~0u: no vector
    if (item >= total) return ~0u;
    const u32 rr = item / vpr, v = item - rr * vpr;
    const VEP_DEV u8* g = src + u64(rb + rr) * src_pitch + u64(is) * 3;
    const u32 mis = u32(reinterpret_cast<uintptr_t>(g)) & 15u;
    const u32 head = min(nbytes, (16u - mis) & 15u);
    if (v >= ((nbytes - head) >> 4)) return ~0u;
    x = *reinterpret_cast<const VEP_DEV uint4*>(g + head + v * 16);
    return rr * rowcap + mis + head + v * 16;
  };
  u8 e = 0;
  const u32 e_at = (t >> 5) < nr ? edge(t >> 5, e) : ~0u;  // 32 byte slots per row, 8 rows per step
  for (u32 base = t; base < total; base += kThreads * 6) {
    uint4 x0 = {}, x1 = {}, x2 = {}, x3 = {}, x4 = {}, x5 = {};
    const u32 at0 = fetch(base, x0), at1 = fetch(base + kThreads, x1), at2 = fetch(base + 2 * kThreads, x2),
              at3 = fetch(base + 3 * kThreads, x3), at4 = fetch(base + 4 * kThreads, x4),
              at5 = fetch(base + 5 * kThreads, x5);
    if (at0 != ~0u) *reinterpret_cast<uint4*>(lds + at0) = x0;
    if (at1 != ~0u) *reinterpret_cast<uint4*>(lds + at1) = x1;
    if (at2 != ~0u) *reinterpret_cast<uint4*>(lds + at2) = x2;
    if (at3 != ~0u) *reinterpret_cast<uint4*>(lds + at3) = x3;
    if (at4 != ~0u) *reinterpret_cast<uint4*>(lds + at4) = x4;
    if (at5 != ~0u) *reinterpret_cast<uint4*>(lds + at5) = x5;
  }
  if (e_at != ~0u) lds[e_at] = e;
  for (u32 rr = (t >> 5) + kThreads / 32; rr < nr; rr += kThreads / 32) {
    const u32 at = edge(rr, e);
    if (at != ~0u) lds[at] = e;
  }
}

// The other direction: nrow rows of nbytes bytes out of LDS (row rr at rr * rowcap + (its global
// address modulo 16), as stage_rows leaves them) to dst + rr * pitch. 16-byte stores to 16-byte
// aligned addresses, a row's unaligned head and tail byte by byte: no byte outside the rows' own
// bytes is written. One vector per thread: nrow * ((nbytes >> 4) + 1) <= kThreads.
__device__ __forceinline__ void store_rows(VEP_DEV u8* dst, u32 pitch, u32 nrow, u32 nbytes, u32 rowcap, const u8* lds) {
  const u32 t = threadIdx.x;
  const u32 vpr = (nbytes >> 4) + 1;  // upper bound of a row's 16-byte vectors
  if (t < nrow * vpr) {
    const u32 rr = t / vpr, v = t - rr * vpr;
    VEP_DEV u8* gp = dst + u64(rr) * pitch;
    const u32 mis = u32(reinterpret_cast<uintptr_t>(gp)) & 15u;
    const u32 head = min(nbytes, (16u - mis) & 15u);
    if (v < ((nbytes - head) >> 4)) {
      const u32 o = head + v * 16;  // o + 16 <= nbytes
      *reinterpret_cast<VEP_DEV uint4*>(gp + o) = *reinterpret_cast<const uint4*>(lds + rr * rowcap + mis + o);
    }
  }
  for (u32 rr = t >> 5; rr < nrow; rr += kThreads / 32) {  // 32 byte slots per row, 8 rows per step
    const u32 slot = t & 31u;
    VEP_DEV u8* gp = dst + u64(rr) * pitch;
    const u32 mis = u32(reinterpret_cast<uintptr_t>(gp)) & 15u;
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
    gp[o] = lds[rr * rowcap + mis + o];
  }
}

// s0 / s1 / s2 += the B / G / R of the n samples that start at byte `off` of the LDS buffer.
__device__ __forceinline__ void sum_samples(const u8* lds, u32 off, u32 n, u32& s0, u32& s1, u32& s2) {
  u32 i = 0;
  if (n >= 4) {
    // Four whole samples at a time: their 12 bytes come out of aligned LDS dwords (a third of the
    // byte reads, which bound the kernels), realigned to B G R B | G R B G | R B G R. The last
    // dword may lie up to 4 bytes past the samples: inside the buffer's padding.
    const u32 sh = off & 3u;
    const u32* w = reinterpret_cast<const u32*>(lds + (off & ~3u));
    u32 d0 = w[0];
    for (; i + 4 <= n; i += 4, w += 3) {
      const u32 d1 = w[1], d2 = w[2], d3 = w[3];
      const u32 r0 = __builtin_amdgcn_alignbyte(d1, d0, sh), r1 = __builtin_amdgcn_alignbyte(d2, d1, sh),
                r2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
      s0 += (r0 & 255u) + (r0 >> 24) + ((r1 >> 16) & 255u) + ((r2 >> 8) & 255u);
      s1 += ((r0 >> 8) & 255u) + (r1 & 255u) + (r1 >> 24) + ((r2 >> 16) & 255u);
      s2 += ((r0 >> 16) & 255u) + ((r1 >> 8) & 255u) + (r2 & 255u) + (r2 >> 24);
      d0 = d3;
    }
  }
  for (; i < n; ++i) {
    const u8* p = lds + off + i * 3;
    s0 += p[0];
    s1 += p[1];
    s2 += p[2];
  }
}

}  // namespace vep::gpu::stage
