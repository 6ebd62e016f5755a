// gfx950 (CDNA4) motion-adaptive deinterlacing of a served picture. See gpu.h for the contract and
// deinterlace.h for the arithmetic, which the CPU implementation (deinterlace.cpp) shares: both
// produce the same bytes. ONE launch for every picture of a request: blockIdx.y is the picture,
// blockIdx.x a 64 x 16 tile of it (a block past its own picture's tiles exits). 8-bit differences,
// comparisons and one halving: there is no matrix-instruction work here.
//
//   newest frame   F is staged with its halo, one row above and below the tile and three columns
//                  left and right (direction +-2 with the three-tap score reaches x +- 3), 18 rows
//                  of 70 pixels, clipped to the picture (stage::stage_rows: any address and pitch,
//                  no byte outside a row's own bytes is read).
//   previous frame G is staged narrowly: the tile's own 64 columns with the same row halo. Its loads
//                  are issued right behind F's barrier, ahead of the arithmetic on F's luma, so
//                  while a wave waits for them the block's other waves compute lumas. A descriptor
//                  with a null G skips it and everything temporal (a batch may mix both cases).
//   luma once      the luma of every staged pixel of F goes into a byte plane of 18 x 70 (pitch 72),
//                  the column clamp of the picture's edges folded into the plane, so the scores
//                  index it unclamped. With G a second plane of 18 x 64 receives |Y_G - Y_F|, all
//                  the temporal bound needs of G's luma.
//   missing rows   only 8 of a tile's 16 rows need arithmetic. A wave owns four consecutive rows, two
//                  missing and two kept, and a lane one column of them: no wave idles on kept rows.
//                  For a missing pixel the lane takes the 7 luma bytes x - 3 .. x + 3 of the rows
//                  above and below out of three aligned LDS dwords each (v_alignbyte), cuts the five
//                  three-byte windows of either row, and forms each score with ONE packed 8-bit SAD
//                  (v_sad_u8, the fourth byte shifted out): 5 SADs for 15 absolute differences.
//                  The scalar form of the same scores takes 15 subtractions, 15 absolute values
//                  and 10 additions on 14 byte reads; the packed form was kept (docs/DEINTERLACE.md).
//                  Kept rows go from the staged bytes to the output buffer as a copy.
//   output         into LDS at the DESTINATION address modulo 16, out with stage::store_rows: no
//                  byte outside the destination's rows is written. Out of place only.
//
// LDS: 4320 (F) + 3744 (G) + 1296 (luma) + 1152 (differences) + 3328 (output) = 13,840 bytes a
// block. Barriers: four (F staged; lumas; differences; output), three without G.
#define VEP_KERNEL_SOURCE 1  // descriptors' pointers are global-address-space here (gpu.h)
#include <algorithm>

#include "deinterlace.h"
#include "gpu.h"
#include "gpu_stage.h"

namespace vep::gpu {

namespace {

using stage::kRows;
using stage::kThreads;
using stage::kTileH;
using stage::kTileW;
constexpr u32 kReach = u32(deinterlace::kReach);          // 3
constexpr u32 kHaloW = kTileW + 2 * kReach, kHaloH = kTileH + 2;  // 70 x 18
constexpr u32 kFCap = stage::rowcap_of(kHaloW);           // 240: a staged row of F
constexpr u32 kFBytes = kHaloH * kFCap;                   // 4320
constexpr u32 kGCap = stage::kTileRowCap;                 // 208: a staged row of G
constexpr u32 kGBytes = kHaloH * kGCap;                   // 3744
constexpr u32 kYPitch = 72;                               // a row of the luma plane: 70 bytes in whole dwords
constexpr u32 kOutCap = stage::kTileRowCap;
static_assert(kTileW == 64 && kRows == 4, "a wave owns four rows of the tile, a lane one column");
static_assert(kYPitch % 4 == 0 && kYPitch >= kHaloW, "the luma rows are read as aligned dwords");
static_assert(((kTileW - 1) >> 2) * 4 + 12 <= kYPitch, "the three dwords of the last lane lie in its row");
static_assert((kHaloH - 1) * kFCap + 15 + kHaloW * 3 <= kFBytes, "the staged tile of F fits its buffer");
static_assert((kHaloH - 1) * kGCap + 15 + kTileW * 3 <= kGBytes, "the staged tile of G fits its buffer");

// The three luma bytes at byte offset o (0..4) of the eight in hi:lo, in the upper three bytes of
// the result (the low byte is zero, in every window alike: it adds nothing to a SAD).
__device__ __forceinline__ u32 window(u32 lo, u32 hi, u32 o) {
  return (o < 4 ? __builtin_amdgcn_alignbyte(hi, lo, o) : hi) << 8;
}

__global__ __launch_bounds__(kThreads) void deinterlace_kernel(const DeinterlaceDesc* __restrict__ descs) {
  __shared__ __attribute__((aligned(16))) u8 fin[kFBytes];
  __shared__ __attribute__((aligned(16))) u8 gin[kGBytes];
  __shared__ __attribute__((aligned(16))) u8 yf[kHaloH * kYPitch];
  __shared__ __attribute__((aligned(16))) u8 dif[kHaloH * kTileW];
  __shared__ __attribute__((aligned(16))) u8 outb[kTileH * kOutCap];
  const DeinterlaceDesc& d = descs[blockIdx.y];
  const u32 w = u32(d.w), h = u32(d.h);
  const u32 bx = blockIdx.x;
  if (bx >= stage::tiles_of(w, h)) return;
  const u32 ntx = stage::tiles_x(w);
  const u32 tk = bx / ntx, tj = bx - tk * ntx;
  const u32 j0 = tj * kTileW, j1 = min(w, j0 + kTileW);
  const u32 k0 = tk * kTileH, k1 = min(h, k0 + kTileH);
  // the staged window of F: the tile and its halo, clipped to the picture; G: the tile's columns
  const u32 xs = j0 >= kReach ? j0 - kReach : 0, xe = min(w, j1 + kReach);
  const u32 ys = k0 ? k0 - 1 : 0, ye = min(h, k1 + 1);
  const u32 nr = ye - ys;
  const VEP_DEV u8* fsrc = d.newer;
  const VEP_DEV u8* gsrc = d.older;
  const u32 fpitch = d.newer_pitch, gpitch = d.older_pitch;
  const bool temporal = gsrc != nullptr;
  const u32 parity = u32(d.parity);
  const u32 t = threadIdx.x;
  // a staged pixel: its row's bytes keep their address modulo 16
  auto fpix = [&](u32 r, u32 x) -> const u8* {  // row r - ys, column x of the picture
    const u32 mis = (u32(reinterpret_cast<uintptr_t>(fsrc)) + (ys + r) * fpitch + xs * 3) & 15u;
    return fin + r * kFCap + mis + (x - xs) * 3;
  };
  auto gpix = [&](u32 r, u32 x) -> const u8* {
    const u32 mis = (u32(reinterpret_cast<uintptr_t>(gsrc)) + (ys + r) * gpitch + j0 * 3) & 15u;
    return gin + r * kGCap + mis + (x - j0) * 3;
  };

  stage::stage_rows(fsrc, fpitch, ys, nr, xs, (xe - xs) * 3, kFCap, fin);
  __syncthreads();
  if (temporal) stage::stage_rows(gsrc, gpitch, ys, nr, j0, (j1 - j0) * 3, kGCap, gin);
  // Y_F of the staged rows: plane column pc is the picture's column j0 - 3 + pc, clamped.
  for (u32 i = t; i < nr * kHaloW; i += kThreads) {
    const u32 r = i / kHaloW, pc = i - r * kHaloW;
    const u32 x = u32(min(max(int(j0 + pc) - int(kReach), 0), int(w - 1)));
    const u8* p = fpix(r, x);
    yf[r * kYPitch + pc] = u8(motion::luma(p[0], p[1], p[2]));
  }
  __syncthreads();
  if (temporal) {
    for (u32 i = t; i < nr * kTileW; i += kThreads) {
      const u32 r = i / kTileW, c = i - r * kTileW;
      const u32 x = min(j0 + c, w - 1);  // (a column past a partial tile repeats the last one: staged bytes)
      const u8* p = gpix(r, x);
      dif[i] = u8(deinterlace::absdiff(motion::luma(p[0], p[1], p[2]), yf[r * kYPitch + (x - j0) + kReach]));
    }
    __syncthreads();
  }

  VEP_DEV u8* out0 = d.dst + u64(k0) * d.dst_pitch + u64(j0) * 3;  // the tile's origin in the destination
  const u32 dst_pitch = d.dst_pitch, nrow = k1 - k0, nout = (j1 - j0) * 3;
  const u32 c = t & (kTileW - 1), q = t / kTileW;
  if (j0 + c < j1) {
    const u32 x = j0 + c;
#pragma unroll
    for (u32 m = 0; m < kRows; ++m) {
      const u32 rr = q * kRows + m;  // the row of the tile; k0 is even, so its parity is the picture row's
      if (rr >= nrow) continue;
      const u32 y = k0 + rr;
      u8* o = outb + rr * kOutCap + (u32(reinterpret_cast<uintptr_t>(out0 + u64(rr) * dst_pitch)) & 15u) + c * 3;
      const u8* f = fpix(y - ys, x);
      if ((y & 1u) == parity) {
        o[0] = f[0];
        o[1] = f[1];
        o[2] = f[2];
        continue;
      }
      const u32 up = u32(deinterlace::row_up(int(y))) - ys, dn = u32(deinterlace::row_dn(int(y), int(h))) - ys;
      // plane bytes c .. c + 6 are the columns x - 3 .. x + 3: out of aligned dwords c / 4 .. c / 4 + 2
      const u32* ur = reinterpret_cast<const u32*>(yf + up * kYPitch) + (c >> 2);
      const u32* dr = reinterpret_cast<const u32*>(yf + dn * kYPitch) + (c >> 2);
      const u32 sh = c & 3u;
      const u32 u0 = ur[0], u1 = ur[1], u2 = ur[2], d0 = dr[0], d1 = dr[1], d2 = dr[2];
      const u32 ulo = __builtin_amdgcn_alignbyte(u1, u0, sh), uhi = __builtin_amdgcn_alignbyte(u2, u1, sh);
      const u32 dlo = __builtin_amdgcn_alignbyte(d1, d0, sh), dhi = __builtin_amdgcn_alignbyte(d2, d1, sh);
      // score(j): the window of `up` around x + j (offset j + 2) against that of `dn` around x - j
      u32 s[5];
#pragma unroll
      for (u32 k = 0; k < 5; ++k) s[k] = __builtin_amdgcn_sad_u8(window(ulo, uhi, k), window(dlo, dhi, 4 - k), 0u);
      const int dir = deinterlace::direction(s[0], s[1], s[2], s[3], s[4]);
      const u32 xa = u32(min(max(int(x) + dir, 0), int(w - 1))), xb = u32(min(max(int(x) - dir, 0), int(w - 1)));
      const u8* a = fpix(up, xa);
      const u8* b = fpix(dn, xb);
      u32 v0 = deinterlace::predict(a[0], b[0]), v1 = deinterlace::predict(a[1], b[1]), v2 = deinterlace::predict(a[2], b[2]);
      if (temporal) {
        const u32 diff = deinterlace::motion_of(dif[(y - ys) * kTileW + c], dif[up * kTileW + c], dif[dn * kTileW + c]);
        const u8* g = gpix(y - ys, x);
        v0 = deinterlace::bound(v0, g[0], f[0], diff);
        v1 = deinterlace::bound(v1, g[1], f[1], diff);
        v2 = deinterlace::bound(v2, g[2], f[2], diff);
      }
      o[0] = u8(v0);
      o[1] = u8(v1);
      o[2] = u8(v2);
    }
  }
  __syncthreads();
  stage::store_rows(out0, dst_pitch, nrow, nout, kOutCap, outb);
}

}  // namespace

void launch_deinterlace(const DeinterlaceDesc* d_descs, const DeinterlaceDesc* h_descs, int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= 65535, "deinterlace: at most 65535 pictures per launch");
  u64 blocks = 0;
  for (int i = 0; i < n; ++i) blocks = std::max(blocks, u64(stage::tiles_of(u32(h_descs[i].w), u32(h_descs[i].h))));
  VEP_CHECK(blocks >= 1 && blocks < (u64(1) << 31), "deinterlace: launch too large");
  hipLaunchKernelGGL(deinterlace_kernel, dim3(u32(blocks), u32(n)), dim3(kThreads), 0, s, d_descs);
  VEP_HIP(hipGetLastError());
}

}  // namespace vep::gpu
