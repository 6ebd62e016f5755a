// gfx950 (CDNA4) on-screen display: primitives (rects and text runs) blended onto packed BGR24
// pictures. See gpu.h for the contract and overlay.h for the arithmetic, which the CPU
// implementation (overlay.cpp) shares: both produce the same bytes.
//
// One launch covers every picture of a request: blockIdx.y is the descriptor (one picture),
// blockIdx.x a tile of kTileW x kTileH pixels of it. A workgroup of 256 threads (four wave64s):
//  * binning: overlay::kMaxPrims equals the thread count, so thread p tests primitive p's
//    rectangle against the tile; four wave ballots give the 256-bit set of the tile in LDS. An
//    empty set ends the workgroup at once when the picture is drawn in place;
//  * the tile's bytes are staged in LDS (stage::stage_rows: nothing outside the tile's own bytes
//    is read), and, when a TEXT is in the set, the font and the picture's text pool beside them;
//  * a wave owns every fourth row of the tile, a lane one column, so a thread holds four pixels
//    in registers. The workgroup walks the set bits in ascending order; the loop is uniform (the
//    set goes through readfirstlane), so a primitive's 16 bytes are one wave-uniform load. Each
//    thread tests coverage (a TEXT's column part once for its four rows) and blends. A pixel is
//    read once and written once, however many primitives cover it, and the list order is the
//    loop order: no second launch, unlike the mask kernel's levels;
//  * the pixels go back to LDS at their DESTINATION address modulo 16 and out with
//    stage::store_rows. The tile's geometry, the staging and the store live in gpu_stage.h, which
//    the crop kernel (gpu_crop.hip) shares.
// A tile's bytes are read and written by its workgroup alone, so drawing in place is race-free.
// No byte outside the picture's rows is read, none outside a tile is written by that tile.
//
// check_overlay() proves on the host that every row lies inside its buffer and every primitive
// inside the picture and the pool.
#define VEP_KERNEL_SOURCE 1  // descriptors' pointers are global-address-space here (gpu.h)
#include <algorithm>

#include "gpu.h"
#include "gpu_stage.h"
#include "overlay.h"

namespace vep::gpu {

namespace {

using stage::kThreads;
static_assert(kThreads == u32(overlay::kMaxPrims), "thread p bins primitive p");
// the tile (gpu_stage.h, which the crop kernel shares)
using stage::kRows;
using stage::kTileH;
using stage::kTileW;
using stage::kWaves;
using stage::tiles_of;
using stage::tiles_x;
constexpr u32 kRowCap = stage::kTileRowCap;
constexpr u32 kFontLds = (u32(overlay::kFontBytes) + 15u) & ~15u;

__device__ __forceinline__ overlay::Prim unpack(const uint4& r) {
  overlay::Prim p;
  p.x0 = u16(r.x);
  p.y0 = u16(r.x >> 16);
  p.x1 = u16(r.y);
  p.y1 = u16(r.y >> 16);
  p.bgra = r.z;
  p.off = u16(r.w);
  p.len = u8(r.w >> 16);
  p.k = u8(r.w >> 24);
  return p;
}

__global__ __launch_bounds__(kThreads) void overlay_kernel(const OverlayDesc* __restrict__ descs) {
  __shared__ __attribute__((aligned(16))) u8 in[kTileH * kRowCap];
  __shared__ __attribute__((aligned(16))) u8 outb[kTileH * kRowCap];
  __shared__ __attribute__((aligned(16))) u8 font[kFontLds];
  __shared__ __attribute__((aligned(16))) u8 text[overlay::kMaxPool];
  __shared__ u64 hit[kWaves], hit_text[kWaves];
  const OverlayDesc& d = descs[blockIdx.y];
  const u32 w = u32(d.w), h = u32(d.h);
  const u32 bx = blockIdx.x;
  if (bx >= tiles_of(w, h)) return;
  const u32 ntx = tiles_x(w);
  const u32 tk = bx / ntx, tj = bx - tk * ntx;
  const u32 j0 = tj * kTileW, j1 = min(w, j0 + kTileW);
  const u32 k0 = tk * kTileH, k1 = min(h, k0 + kTileH);
  const u32 t = threadIdx.x;
  const VEP_DEV uint4* prims = reinterpret_cast<const VEP_DEV uint4*>(d.prims);
  // binning: thread p, primitive p
  bool mine = false, mine_text = false;
  if (t < d.nprims) {
    const overlay::Prim p = unpack(prims[t]);
    mine = p.x0 < j1 && p.x1 > j0 && p.y0 < k1 && p.y1 > k0;
    mine_text = mine && p.k != 0;
  }
  const u64 b = __ballot(mine), bt = __ballot(mine_text);
  if ((t & 63u) == 0) {
    hit[t >> 6] = b;
    hit_text[t >> 6] = bt;
  }
  __syncthreads();
  const bool any = (hit[0] | hit[1] | hit[2] | hit[3]) != 0;
  const bool any_text = (hit_text[0] | hit_text[1] | hit_text[2] | hit_text[3]) != 0;
  const VEP_DEV u8* src = d.src;
  VEP_DEV u8* dst = d.dst;
  const u32 src_pitch = d.src_pitch, dst_pitch = d.dst_pitch;
  if (!any && src == dst) return;  // nothing to draw and nothing to copy
  const u32 nrow = k1 - k0, nbytes = (j1 - j0) * 3;
  stage::stage_rows(src, src_pitch, k0, nrow, j0, nbytes, kRowCap, in);
  if (any_text) {
    for (u32 i = t; i < u32(overlay::kFontBytes); i += kThreads) font[i] = overlay::font_byte(i);
    const VEP_DEV u8* pool = d.text;
    const u32 n = min(d.text_len, u32(overlay::kMaxPool));
    for (u32 i = t; i < n; i += kThreads) text[i] = pool[i];
  }
  __syncthreads();
  // the thread's pixels: column c of rows q + m * kWaves
  const u32 c = t & (kTileW - 1), q = t / kTileW;
  const int px = int(j0 + c);
  const bool active = j0 + c < j1;
  u32 v[kRows][3];
#pragma unroll
  for (u32 m = 0; m < kRows; ++m) {
    const u32 rr = q + m * kWaves;
    const VEP_DEV u8* g = src + u64(k0 + rr) * src_pitch + u64(j0) * 3;
    const u8* p = in + rr * kRowCap + (u32(reinterpret_cast<uintptr_t>(g)) & 15u) + c * 3;
    v[m][0] = p[0];
    v[m][1] = p[1];
    v[m][2] = p[2];
  }
  if (any) {
#pragma unroll 1
    for (u32 g4 = 0; g4 < kWaves; ++g4) {
      const u64 bits = hit[g4];
      u32 lo = __builtin_amdgcn_readfirstlane(u32(bits)), hi = __builtin_amdgcn_readfirstlane(u32(bits >> 32));
      while (lo | hi) {
        u32 i;
        if (lo) {
          i = u32(__builtin_ctz(lo));
          lo &= lo - 1;
        } else {
          i = 32u + u32(__builtin_ctz(hi));
          hi &= hi - 1;
        }
        const overlay::Prim p = unpack(prims[g4 * 64 + i]);
        if (!active || px < int(p.x0) || px >= int(p.x1)) continue;
        const u32 cb = p.bgra & 255u, cg = (p.bgra >> 8) & 255u, cr = (p.bgra >> 16) & 255u, a = p.bgra >> 24;
        const u32 column = p.k ? overlay::text_column(p, px, text) : 0u;
#pragma unroll
        for (u32 m = 0; m < kRows; ++m) {
          const int py = int(k0 + q + m * kWaves);
          if (py < int(p.y0) || py >= int(p.y1)) continue;  // (p.y1 <= h: rows past the picture never pass)
          if (p.k && !overlay::text_row(p, py, column, font)) continue;
          v[m][0] = overlay::blend(v[m][0], cb, a);
          v[m][1] = overlay::blend(v[m][1], cg, a);
          v[m][2] = overlay::blend(v[m][2], cr, a);
        }
      }
    }
  }
  VEP_DEV u8* out0 = dst + u64(k0) * dst_pitch + u64(j0) * 3;  // the tile's origin in the destination
#pragma unroll
  for (u32 m = 0; m < kRows; ++m) {
    const u32 rr = q + m * kWaves;
    if (!active || rr >= nrow) continue;
    u8* o = outb + rr * kRowCap + (u32(reinterpret_cast<uintptr_t>(out0 + u64(rr) * dst_pitch)) & 15u) + c * 3;
    o[0] = u8(v[m][0]);
    o[1] = u8(v[m][1]);
    o[2] = u8(v[m][2]);
  }
  __syncthreads();
  stage::store_rows(out0, dst_pitch, nrow, nbytes, kRowCap, outb);
}

}  // namespace

void check_overlay(const OverlayDesc& d, size_t src_bytes, size_t dst_bytes, const overlay::Prim* h_prims,
                   const u8* h_text) {
  VEP_CHECK(d.src && d.dst, "overlay: null picture");
  VEP_CHECK(d.w >= 1 && d.h >= 1 && d.w <= overlay::kMaxSide && d.h <= overlay::kMaxSide,
            "overlay: picture size must be 1..65535");
  const u64 row = u64(d.w) * 3, h = u64(d.h);
  VEP_CHECK(u64(d.src_pitch) >= row && u64(d.dst_pitch) >= row, "overlay: pitch shorter than a row");
  const u64 src_span = (h - 1) * d.src_pitch + row, dst_span = (h - 1) * d.dst_pitch + row;
  VEP_CHECK(src_span <= src_bytes, "overlay: picture rows outside the picture's memory");
  VEP_CHECK(dst_span <= dst_bytes, "overlay: output rows outside the output's memory");
  const uintptr_t s = reinterpret_cast<uintptr_t>(d.src), o = reinterpret_cast<uintptr_t>(d.dst);
  if (s == o)
    VEP_CHECK(d.src_pitch == d.dst_pitch, "overlay: in place needs equal pitches");
  else
    VEP_CHECK(s + src_span <= o || o + dst_span <= s, "overlay: picture and output overlap");
  VEP_CHECK(d.nprims <= u32(overlay::kMaxPrims), "overlay: at most 256 primitives per picture");
  VEP_CHECK(d.nprims == 0 || (d.prims && reinterpret_cast<uintptr_t>(d.prims) % 16 == 0),
            "overlay: primitives missing or not 16-byte aligned");
  VEP_CHECK(d.text_len == 0 || d.text, "overlay: text pool missing");
  overlay::check_prims(h_prims, int(d.nprims), h_text, d.text_len, d.w, d.h);
}

void launch_overlay(const OverlayDesc* d_descs, const OverlayDesc* h_descs, int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= 65535, "overlay: at most 65535 pictures per launch");
  u32 tiles = 0;
  for (int i = 0; i < n; ++i) tiles = std::max(tiles, tiles_of(u32(h_descs[i].w), u32(h_descs[i].h)));
  hipLaunchKernelGGL(overlay_kernel, dim3(tiles, u32(n)), dim3(kThreads), 0, s, d_descs);
  VEP_HIP(hipGetLastError());
}

}  // namespace vep::gpu
