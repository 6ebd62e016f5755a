// What the kernels on packed BGR24 pictures share: staging rows in LDS, storing rows back out of
// it, the split of a row into aligned vectors and byte ends that both rest on (the mask kernel,
// gpu_mask.hip, uses the split alone), the weighted sum of a staged row segment (scale and crop
// kernels) and the 64 x 16 tile of the crop and overlay kernels. Kernel sources only
// (VEP_KERNEL_SOURCE, 256 threads a workgroup).
//
// Packed BGR rows start at any byte address, so a row segment is staged with 16-byte loads from
// 16-byte aligned addresses and its unaligned head and tail byte by byte; nothing outside the
// segment's own bytes is read. A byte keeps its address modulo 16 in LDS, so the LDS stores are
// aligned too. Rows go out the same way: no byte outside a row's own bytes is written.
#pragma once

#include "gpu.h"

namespace vep::gpu::stage {

constexpr u32 kThreads = 256;
constexpr u32 kLdsBytes = 24576;  // the staging buffer (kernels declare 16 more: the dword reads below)
// pixels of one staged segment: 3 bytes each + up to 15 bytes of misalignment fit the buffer
constexpr u32 kSegPix = (kLdsBytes - 16) / 3;
static_assert(kSegPix * 3 + 15 <= kLdsBytes, "segment fits LDS");
// bytes between staged rows of npix pixels: a row + up to 15 bytes of misalignment, 16-byte aligned
__host__ __device__ constexpr u32 rowcap_of(u32 npix) { return (npix * 3 + 15 + 15) & ~15u; }

// The tile of the crop and overlay kernels: a wave owns every fourth row of it, a lane one column.
constexpr u32 kTileW = 64;                   // a wave spans a tile's row
constexpr u32 kWaves = kThreads / kTileW;    // 4
constexpr u32 kRows = 4;                     // pixels of one thread
constexpr u32 kTileH = kWaves * kRows;       // 16
constexpr u32 kTileRowCap = kTileW * 3 + 16; // a tile row in LDS: its bytes + up to 15 of misalignment
static_assert(kTileRowCap % 16 == 0, "tile rows keep their alignment");
static_assert(kTileH * ((kTileW * 3 >> 4) + 1) <= kThreads, "one 16-byte vector of the tile per thread");
__host__ __device__ inline u32 tiles_x(u32 w) { return (w + kTileW - 1) / kTileW; }
__host__ __device__ inline u32 tiles_of(u32 w, u32 h) { return tiles_x(w) * ((h + kTileH - 1) / kTileH); }

// A row of nbytes bytes at g: `head` bytes up to the first 16-byte aligned address, then nvec
// whole 16-byte vectors, then a tail of fewer than 16 bytes. mis is g modulo 16.
struct RowSplit {
  u32 mis, head, nvec;
};
__device__ __forceinline__ RowSplit split_row(const VEP_DEV u8* g, u32 nbytes) {
  const u32 mis = u32(reinterpret_cast<uintptr_t>(g)) & 15u;
  const u32 head = min(nbytes, (16u - mis) & 15u);
  return {mis, head, (nbytes - head) >> 4};
}
// The row's bytes that no vector covers, by slot: slots 0..15 are the head's, 16..31 the tail's.
// -> false: the slot is empty; o: the byte's offset in the row.
__device__ __forceinline__ bool edge_byte(const RowSplit& r, u32 nbytes, u32 slot, u32& o) {
  const u32 body = r.nvec << 4;
  if (slot < 16) {
    if (slot >= r.head) return false;
    o = slot;
  } else {
    if (slot - 16 >= nbytes - r.head - body) return false;
    o = r.head + body + (slot - 16);
  }
  return true;
}

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
    const VEP_DEV u8* g = src + u64(rb + rr) * src_pitch + u64(is) * 3;
    const RowSplit r = split_row(g, nbytes);
    u32 o;
    if (!edge_byte(r, nbytes, t & 31u, o)) return ~0u;
    x = g[o];
    return rr * rowcap + r.mis + o;
  };
  auto fetch = [&](u32 item, uint4& x) -> u32 {  // -> LDS offset, ~0u: no vector
    if (item >= total) return ~0u;
    const u32 rr = item / vpr, v = item - rr * vpr;
    const VEP_DEV u8* g = src + u64(rb + rr) * src_pitch + u64(is) * 3;
    const RowSplit r = split_row(g, nbytes);
    if (v >= r.nvec) return ~0u;
    x = *reinterpret_cast<const VEP_DEV uint4*>(g + r.head + v * 16);
    return rr * rowcap + r.mis + r.head + v * 16;
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
// address modulo 16), as stage_rows leaves them) to dst + rr * pitch. One vector per thread:
// nrow * ((nbytes >> 4) + 1) <= kThreads.
__device__ __forceinline__ void store_rows(VEP_DEV u8* dst, u32 pitch, u32 nrow, u32 nbytes, u32 rowcap, const u8* lds) {
  const u32 t = threadIdx.x;
  const u32 vpr = (nbytes >> 4) + 1;  // upper bound of a row's 16-byte vectors
  if (t < nrow * vpr) {
    const u32 rr = t / vpr, v = t - rr * vpr;
    VEP_DEV u8* gp = dst + u64(rr) * pitch;
    const RowSplit r = split_row(gp, nbytes);
    if (v < r.nvec) {
      const u32 o = r.head + v * 16;  // o + 16 <= nbytes
      *reinterpret_cast<VEP_DEV uint4*>(gp + o) = *reinterpret_cast<const uint4*>(lds + rr * rowcap + r.mis + o);
    }
  }
  for (u32 rr = t >> 5; rr < nrow; rr += kThreads / 32) {  // 32 byte slots per row, 8 rows per step
    VEP_DEV u8* gp = dst + u64(rr) * pitch;
    const RowSplit r = split_row(gp, nbytes);
    u32 o;
    if (edge_byte(r, nbytes, t & 31u, o)) gp[o] = lds[rr * rowcap + r.mis + o];
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

// h0 / h1 / h2 += the weighted B / G / R sum of a row's samples lo .. hi, as far as they lie in
// the staged segment [is, ie) whose first byte is at row_off of the LDS buffer: w_lo times sample
// lo, w_mid times every sample between the two ends, w_hi times sample hi (where hi != lo). Only
// the ends weigh differently, so the inner run only adds.
__device__ __forceinline__ void sum_weighted(const u8* lds, u32 row_off, u32 is, u32 ie, u32 lo, u32 hi, u32 w_lo,
                                             u32 w_mid, u32 w_hi, u32& h0, u32& h1, u32& h2) {
  const u32 a = max(lo + 1, is), b = min(hi, ie);  // inner samples [a, b) of this segment
  u32 s0 = 0, s1 = 0, s2 = 0;
  if (a < b) sum_samples(lds, row_off + (a - is) * 3, b - a, s0, s1, s2);
  h0 += w_mid * s0;
  h1 += w_mid * s1;
  h2 += w_mid * s2;
  if (lo >= is && lo < ie) {
    const u8* p = lds + row_off + (lo - is) * 3;
    h0 += w_lo * p[0];
    h1 += w_lo * p[1];
    h2 += w_lo * p[2];
  }
  if (hi != lo && hi >= is && hi < ie) {
    const u8* p = lds + row_off + (hi - is) * 3;
    h0 += w_hi * p[0];
    h1 += w_hi * p[1];
    h2 += w_hi * p[2];
  }
}

}  // namespace vep::gpu::stage
