// gfx950 (CDNA4) remapped views of a picture (fisheye dewarp, lens undistortion). See gpu.h for
// the contract and dewarp.h for the arithmetic, which the CPU implementation (dewarp.cpp) shares:
// both produce the same bytes.
//
// One launch covers every (picture, view) pair of a request: blockIdx.y is the descriptor,
// blockIdx.x a tile of its output. A tile is kTileW x kTileH output pixels (gpu_stage.h): a wave
// owns every fourth row of it, a lane one column, so a thread computes up to kRows pixels. A
// dewarp is a per-pixel 2-D gather, so unlike the crop kernel nothing is summed along an axis; what
// the tile shares is its FOOTPRINT:
//  * the tile spans up to 8 x 2 mesh cells, so at most 9 x 3 nodes, clipped to the cells that hold
//    its pixels. 27 threads load them (dewarp::node, the clamp included) into LDS once;
//  * a pixel's position is a convex combination of its cell's nodes, rounded inside their
//    [min, max], so the bounding box of the tile's nodes, widened by the one extra tap and clamped
//    to the picture, contains every byte the tile can read. Every thread derives the same box from
//    the same LDS words, so the cases below are uniform over the workgroup:
//      pad     the box lies wholly outside the picture on one axis: no source load at all;
//      staged  the box fits the staging buffer: its rows go into LDS with stage::stage_rows
//              (16-byte vector loads, nothing outside the rows' own bytes) and all four taps of
//              every pixel come out of LDS. Neighbouring pixels share three of their four taps and
//              a global gather would fetch every tap as a byte load of its own;
//      global  the box does not fit (strong minification, the seam of a panorama), or it is no
//              larger than kDirectW x kDirectH, about the tile itself (an undistortion at native
//              size): there a wave's row of pixels reads one or two runs of neighbouring bytes,
//              the cache lines staging would fetch, and staging only adds an LDS round trip and a
//              barrier. The taps come straight from global memory, with the same clamps.
//    VEP_DEWARP_GLOBAL_ONLY compiles the staged case out (tools/bench_dewarp.py measures both).
// The tile's bytes are then put together in LDS, every byte at its global address modulo 16, and
// written with stage::store_rows (a view of a packed [n, H, W, 3] tensor starts at any byte
// address). Bytes outside the tile's own rows are NOT WRITTEN AT ALL.
//
// check_dewarp() proves on the host that the picture, the mesh and the output lie inside their
// memory; with the clamps that is every access of the kernel.
#define VEP_KERNEL_SOURCE 1  // descriptors' pointers are global-address-space here (gpu.h)
#include <algorithm>

#include "dewarp.h"
#include "gpu.h"
#include "gpu_stage.h"

namespace vep::gpu {

namespace {

using stage::kLdsBytes;
using stage::kRows;
using stage::kSegPix;
using stage::kThreads;
using stage::kTileH;
using stage::kTileW;
using stage::kWaves;
using stage::tiles_of;
using stage::tiles_x;
constexpr u32 kOutCap = stage::kTileRowCap;
constexpr int kNodeCols = int(kTileW) / dewarp::kCell + 1, kNodeRows = int(kTileH) / dewarp::kCell + 1;  // 9 x 3
static_assert(kTileW % dewarp::kCell == 0 && kTileH % dewarp::kCell == 0, "a tile is whole cells wide and high");
static_assert(kNodeCols * kNodeRows <= int(kThreads), "a thread a node");
constexpr u32 kDirectW = kTileW + kTileW / 8, kDirectH = kTileH + kTileH / 2;  // 72 x 24 source pixels

__global__ __launch_bounds__(kThreads) void dewarp_kernel(const DewarpDesc* __restrict__ descs) {
  __shared__ __attribute__((aligned(16))) u8 lds[kLdsBytes];
  __shared__ __attribute__((aligned(16))) u8 olds[kTileH * kOutCap];
  __shared__ dewarp::Pos nodes[kNodeRows][kNodeCols];
  const DewarpDesc& d = descs[blockIdx.y];
  const u32 ow = d.ow, oh = d.oh;
  if (blockIdx.x >= tiles_of(ow, oh)) return;
  const u32 ntx = tiles_x(ow);
  const u32 tk = blockIdx.x / ntx, tj = blockIdx.x - tk * ntx;
  const u32 j0 = tj * kTileW, j1 = min(ow, j0 + kTileW);
  const u32 k0 = tk * kTileH, k1 = min(oh, k0 + kTileH);
  const int w = d.pw, h = d.ph;
  const u32 pad = d.pad_bgr;
  // the nodes of the cells that hold pixels of the tile: columns m0 .. m0 + ncols - 1, rows n0 .. n0 + nrows - 1
  const int m0 = int(j0) >> dewarp::kCellShift, n0 = int(k0) >> dewarp::kCellShift;
  const int ncols = (int(j1 - 1) >> dewarp::kCellShift) - m0 + 2, nrows = (int(k1 - 1) >> dewarp::kCellShift) - n0 + 2;
  const u32 t = threadIdx.x;
  if (t < u32(nrows * ncols)) {
    const int r = int(t) / ncols, c = int(t) - r * ncols;
    nodes[r][c] = dewarp::node(d.mesh, dewarp::mesh_w(int(ow)), m0 + c, n0 + r);
  }
  __syncthreads();
  int xa = nodes[0][0].x, xb = xa, ya = nodes[0][0].y, yb = ya;  // the nodes' bounding box, 1/256 px
  for (int c = 0; c < ncols; ++c)
    for (int r = 0; r < nrows; ++r) {
      const dewarp::Pos p = nodes[r][c];
      xa = min(xa, p.x), xb = max(xb, p.x), ya = min(ya, p.y), yb = max(yb, p.y);
    }
  VEP_DEV u8* dst = d.dst;
  auto row_ptr = [&](u32 rr) -> VEP_DEV u8* { return dst + (u64(k0 + rr) * ow + j0) * 3; };
  const u32 c = t & (kTileW - 1), q = t / kTileW;
  const u32 j = j0 + c;
  const bool active = j < j1;
  auto put = [&](u32 rr, u32 b0, u32 b1, u32 b2) {
    u8* o = olds + rr * kOutCap + (u32(reinterpret_cast<u64>(row_ptr(rr))) & 15u) + c * 3;
    o[0] = u8(b0), o[1] = u8(b1), o[2] = u8(b2);
  };
  // every position of the tile lies in the box: left of, right of, above or below the picture
  const bool all_pad = xb < -128 || xa >= w * 256 - 128 || yb < -128 || ya >= h * 256 - 128;
  if (all_pad) {
#pragma unroll
    for (u32 m = 0; m < kRows; ++m) {
      const u32 rr = q + m * kWaves;
      if (active && k0 + rr < k1) put(rr, pad & 255u, (pad >> 8) & 255u, (pad >> 16) & 255u);
    }
  } else {
    // the taps of every pixel inside the picture lie in columns ia .. ib of rows ra .. rz
    const u32 ia = u32(max(0, min(w - 1, xa >> 8))), ib = u32(max(0, min(w - 1, (xb >> 8) + 1)));
    const u32 ra = u32(max(0, min(h - 1, ya >> 8))), rz = u32(max(0, min(h - 1, (yb >> 8) + 1)));
    const u32 npix = ib - ia + 1, nrow = rz - ra + 1;
    const u32 rowcap = stage::rowcap_of(min(npix, kSegPix));
#ifdef VEP_DEWARP_GLOBAL_ONLY
    const bool staged = false;
#else
    const bool staged = npix <= kSegPix && u64(nrow) * rowcap <= kLdsBytes && (npix > kDirectW || nrow > kDirectH);
#endif
    const VEP_DEV u8* src = d.src;
    const u32 src_pitch = d.src_pitch;
    if (staged) {
      stage::stage_rows(src, src_pitch, ra, nrow, ia, npix * 3, rowcap, lds);
      __syncthreads();
    }
    if (active) {
      const int mc = (int(j) >> dewarp::kCellShift) - m0, a = int(j) & (dewarp::kCell - 1);
      const u32 base = u32(reinterpret_cast<uintptr_t>(src)) + ia * 3;  // (modulo 16 is all that is used)
#pragma unroll
      for (u32 m = 0; m < kRows; ++m) {
        const u32 rr = q + m * kWaves;  // k0 is a multiple of kCell: cell row rr >> kCellShift of the tile
        if (k0 + rr >= k1) continue;
        const int nr = int(rr) >> dewarp::kCellShift;
        const dewarp::Pos p = dewarp::position(nodes[nr][mc], nodes[nr][mc + 1], nodes[nr + 1][mc], nodes[nr + 1][mc + 1], a,
                                               int(rr) & (dewarp::kCell - 1));
        if (dewarp::outside(p.x, w) || dewarp::outside(p.y, h)) {
          put(rr, pad & 255u, (pad >> 8) & 255u, (pad >> 16) & 255u);
          continue;
        }
        const dewarp::Tap tx = dewarp::tap(p.x, w), ty = dewarp::tap(p.y, h);
        u32 p00[3], p10[3], p01[3], p11[3];
        if (staged) {
          // row r of the footprint lies at (r - ra) * rowcap + (its first byte's address modulo 16)
          const u8* r0 = lds + (u32(ty.i0) - ra) * rowcap + ((base + u32(ty.i0) * src_pitch) & 15u);
          const u8* r1 = lds + (u32(ty.i1) - ra) * rowcap + ((base + u32(ty.i1) * src_pitch) & 15u);
          const u32 o0 = (u32(tx.i0) - ia) * 3, o1 = (u32(tx.i1) - ia) * 3;
#pragma unroll
          for (u32 ch = 0; ch < 3; ++ch) p00[ch] = r0[o0 + ch], p10[ch] = r0[o1 + ch], p01[ch] = r1[o0 + ch], p11[ch] = r1[o1 + ch];
        } else {
          const VEP_DEV u8* r0 = src + u64(u32(ty.i0)) * src_pitch;
          const VEP_DEV u8* r1 = src + u64(u32(ty.i1)) * src_pitch;
          const u32 o0 = u32(tx.i0) * 3, o1 = u32(tx.i1) * 3;
#pragma unroll
          for (u32 ch = 0; ch < 3; ++ch) p00[ch] = r0[o0 + ch], p10[ch] = r0[o1 + ch], p01[ch] = r1[o0 + ch], p11[ch] = r1[o1 + ch];
        }
        put(rr, dewarp::blend(tx.f, ty.f, p00[0], p10[0], p01[0], p11[0]),
            dewarp::blend(tx.f, ty.f, p00[1], p10[1], p01[1], p11[1]),
            dewarp::blend(tx.f, ty.f, p00[2], p10[2], p01[2], p11[2]));
      }
    }
  }
  __syncthreads();
  stage::store_rows(row_ptr(0), ow * 3, k1 - k0, (j1 - j0) * 3, kOutCap, olds);
}

}  // namespace

void check_dewarp(const DewarpDesc& d, size_t src_bytes, size_t mesh_pairs, size_t dst_bytes) {
  VEP_CHECK(d.src && d.dst && d.mesh, "view: null picture, mesh or output");
  VEP_CHECK(d.pw >= 1 && d.ph >= 1 && d.pw <= dewarp::kMaxSrc && d.ph <= dewarp::kMaxSrc,
            "view: picture size must be 1..8192");
  const u64 w = u64(d.pw), h = u64(d.ph);
  VEP_CHECK(u64(d.src_pitch) >= w * 3, "view: pitch shorter than a row");
  VEP_CHECK((h - 1) * d.src_pitch + w * 3 <= src_bytes, "view: picture rows outside the picture's memory");
  VEP_CHECK(d.ow >= 1 && d.oh >= 1 && d.ow <= dewarp::kMaxOut && d.oh <= dewarp::kMaxOut,
            "view: width and height must be 1..4096");
  VEP_CHECK(u64(dewarp::mesh_w(d.ow)) * u64(dewarp::mesh_h(d.oh)) <= mesh_pairs, "view: mesh smaller than the output needs");
  VEP_CHECK(u64(d.ow) * d.oh * 3 <= dst_bytes, "view: output larger than its memory");
  VEP_CHECK(d.pad_bgr <= 0xFFFFFFu, "view: pad colour out of range");
}

void launch_dewarp(const DewarpDesc* d_descs, const DewarpDesc* h_descs, int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= 65535, "view: at most 65535 views per launch");
  u32 tiles = 0;
  for (int i = 0; i < n; ++i) tiles = std::max(tiles, tiles_of(h_descs[i].ow, h_descs[i].oh));
  hipLaunchKernelGGL(dewarp_kernel, dim3(tiles, u32(n)), dim3(kThreads), 0, s, d_descs);
  VEP_HIP(hipGetLastError());
}

}  // namespace vep::gpu
