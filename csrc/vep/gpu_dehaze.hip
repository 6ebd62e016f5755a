// gfx950 (CDNA4) dehazing by the dark-channel prior. See gpu.h for the contract and dehaze.h for
// the arithmetic, which the CPU implementation (dehaze.cpp) shares: both produce the same bytes,
// planes included. Seven launches, each ONE launch for every picture of a request: blockIdx.y is
// the picture, blockIdx.x a block of it (a block past its own picture's work exits). Byte minima,
// integer box sums and table lookups: there is no matrix-instruction work here.
//
// 0. dehaze_clear_kernel zeroes the 1024 words of every picture's table (the dark kernel adds to it).
// 1. dehaze_dark_kernel<false>: the 64 x 16 tile of gpu_stage.h with a halo of r = patch / 2 <= 15
//    pixels, clipped to the picture, staged with stage::stage_rows (up to 46 rows of 94 pixels). A
//    byte plane of the window takes min(B, G, R), 255 outside the picture (neutral for a minimum).
//    The windowed minimum is separable. ROWS: a thread owns four neighbouring outputs of a plane
//    row, reads the 2 r + 4 bytes they depend on as up to nine aligned LDS dwords, takes the
//    minimum of the bytes 3 .. 2 r that all four share ONCE and adds each output's three own bytes:
//    2 r + 10 minima for four outputs instead of 8 r, and a quarter of the LDS reads. COLUMNS: a
//    thread owns the same four columns of one tile row and walks 2 r + 1 dwords of the row minima.
//    Its four pixels then go into the block's 256 x 4 table in LDS (equal neighbours merged into
//    one add), and the non-empty bins leave by global atomics once per block.
// 2. dehaze_air_kernel: one block per picture, thread i holds bin 255 - i: an inclusive scan of the
//    counts (shuffles inside the wave, LDS across the four) says which bins the walk from 255
//    takes, their sums are reduced the same way, and thread v writes entry v of the three
//    normalisation tables.
// 3. dehaze_dark_kernel<true>: the same body; the plane takes min_c norm_c[I_c] through the tables
//    in LDS, and the four pixels' t_raw and luma are summed over the cell's four rows by two
//    shuffles (a wave owns four tile rows: one row of cells), divided by the cell's true count.
// 4. dehaze_coeff_kernel, 5. dehaze_smooth_kernel: tiles of 32 x 32 cells with a halo of `radius`
//    <= 16, zero outside the plane; row sums of the box into LDS, then column sums of those, the
//    true count K from the clipped spans, and the i64 divisions of dehaze::coeffs / box_mean. Two
//    launches: the second box needs its neighbours' a and b.
// 6. dehaze_apply_kernel: the 64 x 16 tile. Its pixels lie between at most 18 x 6 cell centres,
//    whose mean_a / mean_b are staged in LDS beside the reciprocal table of t0 .. 1024 (computed by
//    the block: four divisions a thread). A wave owns every fourth row, a lane one column; the
//    pixels go to LDS at their DESTINATION address modulo 16 and out with stage::store_rows. A
//    tile's bytes are read and written by its block alone, so in place is race-free.
//
// LDS of the dark kernel: 46 x 304 + 16 staging, 46 x 96 plane, 46 x 64 row minima, 4 KB table
// (768 bytes of norm tables in the second instantiation): 25.5 KB, six blocks (24 waves) a CU.
#define VEP_KERNEL_SOURCE 1  // descriptors' pointers are global-address-space here (gpu.h)
#include <algorithm>

#include "dehaze.h"
#include "gpu.h"
#include "gpu_stage.h"

namespace vep::gpu {

namespace {

using stage::kRows;
using stage::kThreads;
using stage::kTileH;
using stage::kTileW;
using stage::kWaves;
constexpr u32 kBins = u32(dehaze::kBins);
constexpr u32 kHalo = u32(dehaze::kMaxPatch) / 2;            // 15
constexpr u32 kWinW = kTileW + 2 * kHalo;                    // 94
constexpr u32 kWinH = kTileH + 2 * kHalo;                    // 46
constexpr u32 kWinCap = stage::rowcap_of(kWinW);             // 304
constexpr u32 kPlaneW = (kWinW + 3) & ~3u;                   // 96: rows of whole dwords
constexpr u32 kRowCap = stage::kTileRowCap;
constexpr u32 kBoxTile = 32;                                 // cells of a coefficient tile's side
constexpr u32 kBoxWin = kBoxTile + 2 * u32(dehaze::kMaxRadius);  // 64
constexpr u32 kMeanCols = (2 * (kTileW - 1) + 7) / 8 + 2;    // 18: first index grows by <= 16, the second adds one
constexpr u32 kMeanRows = (2 * (kTileH - 1) + 7) / 8 + 2;    // 6
static_assert(kThreads == kBins && kThreads == 256 && kTileW == 64 && kTileH == 16, "one thread per bin and per four pixels");
static_assert(kMeanCols == 18 && kMeanRows == 6, "cell window of an apply tile");
static_assert((2 * kHalo + 7) / 4 <= 9 && kTileW / 4 - 1 + 9 <= kPlaneW / 4, "the row pass reads inside a plane row");

__device__ __forceinline__ u32 block_box_tiles(u32 cw, u32 ch) {
  return ((cw + kBoxTile - 1) / kBoxTile) * ((ch + kBoxTile - 1) / kBoxTile);
}

__global__ __launch_bounds__(kThreads) void dehaze_clear_kernel(const DehazeDesc* __restrict__ descs) {
  descs[blockIdx.y].table[blockIdx.x * kThreads + threadIdx.x] = 0;  // grid.x = kTableWords / kThreads
}

template <bool kCells>
__global__ __launch_bounds__(kThreads) void dehaze_dark_kernel(const DehazeDesc* __restrict__ descs) {
  __shared__ __attribute__((aligned(16))) u8 in[kWinH * kWinCap + 16];
  __shared__ u32 plane32[kWinH * kPlaneW / 4];
  __shared__ u32 rowmin32[kWinH * kTileW / 4];
  __shared__ u32 tab[kCells ? 3 * kBins / 4 : 4 * kBins];
  const DehazeDesc& d = descs[blockIdx.y];
  const u32 w = u32(d.w), h = u32(d.h), r = u32(d.patch) >> 1;
  const u32 bx = blockIdx.x;
  if (bx >= stage::tiles_of(w, h)) return;
  const u32 ntx = stage::tiles_x(w);
  const u32 tk = bx / ntx, tj = bx - tk * ntx;
  const u32 j0 = tj * kTileW, j1 = min(w, j0 + kTileW);
  const u32 k0 = tk * kTileH, k1 = min(h, k0 + kTileH);
  const u32 nrow = k1 - k0;
  // the window, clipped to the picture: columns sx0 .. sx1, rows sy0 .. sy1
  const u32 sx0 = j0 > r ? j0 - r : 0u, sx1 = min(w, j1 + r);
  const u32 sy0 = k0 > r ? k0 - r : 0u, sy1 = min(h, k1 + r);
  const VEP_DEV u8* src = d.src;
  const u32 src_pitch = d.src_pitch;
  const u32 t = threadIdx.x;
  stage::stage_rows(src, src_pitch, sy0, sy1 - sy0, sx0, (sx1 - sx0) * 3, kWinCap, in);
  if (kCells) {
    if (t < 3 * kBins / 4) tab[t] = d.air[4 + t];
  } else {
    for (u32 i = t; i < 4 * kBins; i += kThreads) tab[i] = 0;
  }
  __syncthreads();
  const u32 base_mis = u32(reinterpret_cast<uintptr_t>(src)) + sx0 * 3;  // (only its low 4 bits are used)
  // the staged bytes of pixel (x, y), sx0 <= x < sx1 and sy0 <= y < sy1
  auto pixel = [&](u32 x, u32 y) { return in + (y - sy0) * kWinCap + ((base_mis + y * src_pitch) & 15u) + (x - sx0) * 3; };
  const u8* norm = reinterpret_cast<const u8*>(tab);
  u8* plane = reinterpret_cast<u8*>(plane32);
  // plane (py, px) is pixel (j0 + px - r, k0 + py - r)
  for (u32 idx = t; idx < kWinH * kPlaneW; idx += kThreads) {
    const u32 py = idx / kPlaneW, px = idx - py * kPlaneW;
    const u32 x = j0 + px - r, y = k0 + py - r;  // (wraps below zero: then >= sx1 / sy1)
    u32 v = 255u;
    if (x >= sx0 && x < sx1 && y >= sy0 && y < sy1) {
      const u8* p = pixel(x, y);
      v = kCells ? dehaze::min3(norm[p[0]], norm[kBins + p[1]], norm[2 * kBins + p[2]]) : dehaze::min3(p[0], p[1], p[2]);
    }
    plane[idx] = u8(v);
  }
  __syncthreads();
  // rows: output (py, 4 xg + i) is the minimum of plane bytes 4 xg + i .. 4 xg + i + 2 r of row py
  const u32 ndw = (2 * r + 7) >> 2;
  for (u32 item = t; item < (nrow + 2 * r) * (kTileW / 4); item += kThreads) {
    const u32 py = item >> 4, xg = item & 15u;
    const u32* at = plane32 + py * (kPlaneW / 4) + xg;
    u32 wd[9];
#pragma unroll
    for (u32 k = 0; k < 9; ++k) wd[k] = k < ndw ? at[k] : ~0u;
    u32 core = 255u, e1 = 255u, e2 = 255u, e3 = 255u;
#pragma unroll
    for (u32 k = 3; k < 2 * kHalo + 4; ++k) {
      const u32 v = (wd[k >> 2] >> ((k & 3u) * 8u)) & 255u;
      core = k <= 2 * r ? min(core, v) : core;
      e1 = k == 2 * r + 1 ? v : e1;
      e2 = k == 2 * r + 2 ? v : e2;
      e3 = k == 2 * r + 3 ? v : e3;
    }
    const u32 b0 = wd[0] & 255u, b1 = (wd[0] >> 8) & 255u, b2 = (wd[0] >> 16) & 255u;
    const u32 o0 = min(core, dehaze::min3(b0, b1, b2)), o1 = min(core, dehaze::min3(b1, b2, e1)),
              o2 = min(core, dehaze::min3(b2, e1, e2)), o3 = min(core, dehaze::min3(e1, e2, e3));
    rowmin32[py * (kTileW / 4) + xg] = o0 | o1 << 8 | o2 << 16 | o3 << 24;
  }
  __syncthreads();
  // columns: the thread's four pixels (j0 + 4 xg + i, k0 + ry)
  const u32 xg = t & 15u, ry = t >> 4;
  u32 m[4] = {255u, 255u, 255u, 255u};
  if (ry < nrow) {
#pragma unroll
    for (u32 k = 0; k < 2 * kHalo + 1; ++k)
      if (k <= 2 * r) {
        const u32 v = rowmin32[(ry + k) * (kTileW / 4) + xg];
#pragma unroll
        for (u32 i = 0; i < 4; ++i) m[i] = min(m[i], (v >> (8u * i)) & 255u);
      }
  }
  const u32 x0 = j0 + 4 * xg, y = k0 + ry;
  const u32 npx = ry < nrow && x0 < j1 ? min(4u, j1 - x0) : 0u;
  if (!kCells) {
    u32 prev = 0, cnt = 0, s0 = 0, s1 = 0, s2 = 0;
    auto flush = [&]() {
      if (!cnt) return;
      atomicAdd(&tab[prev * 4], cnt);
      atomicAdd(&tab[prev * 4 + 1], s0);
      atomicAdd(&tab[prev * 4 + 2], s1);
      atomicAdd(&tab[prev * 4 + 3], s2);
    };
#pragma unroll
    for (u32 i = 0; i < 4; ++i)
      if (i < npx) {
        const u8* p = pixel(x0 + i, y);
        if (m[i] != prev) {
          flush();
          prev = m[i];
          cnt = s0 = s1 = s2 = 0;
        }
        ++cnt;
        s0 += p[0];
        s1 += p[1];
        s2 += p[2];
      }
    flush();
    __syncthreads();
    if (tab[t * 4]) {
      VEP_DEV u32* out = d.table + t * 4;
#pragma unroll
      for (u32 c = 0; c < 4; ++c) atomicAdd((u32*)(out + c), tab[t * 4 + c]);
    }
  } else {
    u32 sy = 0, st = 0;
#pragma unroll
    for (u32 i = 0; i < 4; ++i)
      if (i < npx) {
        const u8* p = pixel(x0 + i, y);
        sy += motion::luma(p[0], p[1], p[2]);
        st += dehaze::t_raw(u32(d.omega), m[i]);
      }
    // a wave owns tile rows 4 wave .. 4 wave + 3: lanes l, l + 16, l + 32, l + 48 share a cell
    u32 n = npx;
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      sy += u32(__shfl_xor(int(sy), off));
      st += u32(__shfl_xor(int(st), off));
      n += u32(__shfl_xor(int(n), off));
    }
    if ((t & 63u) < 16u && n) d.cell[u64((k0 >> 2) + (t >> 6)) * dehaze::cells(w) + (j0 >> 2) + xg] = dehaze::cell_value(sy, st, n);
  }
}

__global__ __launch_bounds__(kThreads) void dehaze_air_kernel(const DehazeDesc* __restrict__ descs) {
  __shared__ u32 ends[kWaves], part[kWaves][4];
  const DehazeDesc& d = descs[blockIdx.x];
  const u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6, v = kBins - 1 - t;
  const VEP_DEV u32* bin = d.table + v * 4;
  const u32 cnt = bin[0];
  u32 incl = cnt;
#pragma unroll
  for (u32 off = 1; off < 64; off <<= 1) {
    const u32 o = u32(__shfl_up(int(incl), off));
    if (lane >= off) incl += o;
  }
  if (lane == 63) ends[wave] = incl;
  __syncthreads();
  for (u32 k = 0; k < wave; ++k) incl += ends[k];
  // the walk takes bin v while the count of the bins above it is short of the target
  const bool take = incl - cnt < dehaze::air_target(u32(d.w), u32(d.h));
  u32 s[4] = {take ? cnt : 0u, take ? bin[1] : 0u, take ? bin[2] : 0u, take ? bin[3] : 0u};
#pragma unroll
  for (u32 c = 0; c < 4; ++c) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s[c] += u32(__shfl_xor(int(s[c]), off));
    if (lane == 0) part[wave][c] = s[c];
  }
  __syncthreads();
  const u32 n = part[0][0] + part[1][0] + part[2][0] + part[3][0];  // >= 1: the table holds w h >= target pixels
  VEP_DEV u8* norm = reinterpret_cast<VEP_DEV u8*>(d.air + 4);
#pragma unroll
  for (u32 c = 0; c < 3; ++c) {
    const u32 a = dehaze::air_of(part[0][c + 1] + part[1][c + 1] + part[2][c + 1] + part[3][c + 1], n);
    norm[c * kBins + t] = u8(dehaze::norm_of(t, a));
    if (t == 0) d.air[c] = a;
  }
  if (t == 0) d.air[3] = n;
}

// The window of a box tile: cell (ox + ix - radius, oy + iy - radius) for ix, iy < side, through
// `load` (zero outside the plane) into in[iy * kBoxWin + ix].
template <class T, class Load>
__device__ __forceinline__ void stage_cells(u32 ox, u32 oy, u32 radius, u32 cw, u32 ch, T* in, Load&& load) {
  const u32 side = kBoxTile + 2 * radius;
  for (u32 idx = threadIdx.x; idx < side * side; idx += kThreads) {
    const u32 iy = idx / side, ix = idx - iy * side;
    const u32 cx = ox + ix - radius, cy = oy + iy - radius;  // (wraps below zero: then >= cw / ch)
    in[iy * kBoxWin + ix] = cx < cw && cy < ch ? load(u64(cy) * cw + cx) : T{};
  }
}
// The true count of the box around cell (cx, cy).
__device__ __forceinline__ u32 box_count(u32 cx, u32 cy, u32 cw, u32 ch, u32 radius) {
  u32 x0, x1, y0, y1;
  dehaze::box_span(cx, cw, radius, x0, x1);
  dehaze::box_span(cy, ch, radius, y0, y1);
  return (x1 - x0 + 1) * (y1 - y0 + 1);
}

__global__ __launch_bounds__(kThreads) void dehaze_coeff_kernel(const DehazeDesc* __restrict__ descs) {
  __shared__ u32 in[kBoxWin * kBoxWin];
  __shared__ uint4 hs[kBoxWin * kBoxTile];
  const DehazeDesc& d = descs[blockIdx.y];
  const u32 cw = dehaze::cells(u32(d.w)), ch = dehaze::cells(u32(d.h)), radius = u32(d.radius);
  const u32 bx = blockIdx.x;
  if (bx >= block_box_tiles(cw, ch)) return;
  const u32 ntx = (cw + kBoxTile - 1) / kBoxTile;
  const u32 ty = bx / ntx, ox = (bx - ty * ntx) * kBoxTile, oy = ty * kBoxTile;
  const VEP_DEV u32* cell = d.cell;
  stage_cells(ox, oy, radius, cw, ch, in, [&](u64 at) { return cell[at]; });
  __syncthreads();
  const u32 t = threadIdx.x, side = kBoxTile + 2 * radius;
  for (u32 item = t; item < side * kBoxTile; item += kThreads) {
    const u32 iy = item >> 5, ix = item & 31u;
    uint4 s = {0, 0, 0, 0};
    for (u32 k = 0; k <= 2 * radius; ++k) {
      const u32 c = in[iy * kBoxWin + ix + k], yc = c & 0xffffu, tc = c >> 16;
      s.x += yc;
      s.y += tc;
      s.z += yc * tc;
      s.w += yc * yc;
    }
    hs[item] = s;
  }
  __syncthreads();
  for (u32 item = t; item < kBoxTile * kBoxTile; item += kThreads) {
    const u32 iy = item >> 5, ix = item & 31u, cx = ox + ix, cy = oy + iy;
    if (cx >= cw || cy >= ch) continue;
    uint4 s = {0, 0, 0, 0};
    for (u32 k = 0; k <= 2 * radius; ++k) {
      const uint4 v = hs[(iy + k) * kBoxTile + ix];
      s.x += v.x;
      s.y += v.y;
      s.z += v.z;
      s.w += v.w;
    }
    int32_t a, b;
    dehaze::coeffs(s.x, s.y, s.z, s.w, box_count(cx, cy, cw, ch, radius), a, b);
    d.ab[u64(cy) * cw + cx] = make_int2(a, b);
  }
}

__global__ __launch_bounds__(kThreads) void dehaze_smooth_kernel(const DehazeDesc* __restrict__ descs) {
  __shared__ int2 in[kBoxWin * kBoxWin];
  __shared__ int2 hs[kBoxWin * kBoxTile];
  const DehazeDesc& d = descs[blockIdx.y];
  const u32 cw = dehaze::cells(u32(d.w)), ch = dehaze::cells(u32(d.h)), radius = u32(d.radius);
  const u32 bx = blockIdx.x;
  if (bx >= block_box_tiles(cw, ch)) return;
  const u32 ntx = (cw + kBoxTile - 1) / kBoxTile;
  const u32 ty = bx / ntx, ox = (bx - ty * ntx) * kBoxTile, oy = ty * kBoxTile;
  const VEP_DEV int2* ab = d.ab;
  stage_cells(ox, oy, radius, cw, ch, in, [&](u64 at) { return ab[at]; });
  __syncthreads();
  const u32 t = threadIdx.x, side = kBoxTile + 2 * radius;
  for (u32 item = t; item < side * kBoxTile; item += kThreads) {
    const u32 iy = item >> 5, ix = item & 31u;
    int2 s = {0, 0};  // (33 * 2^24 < 2^31: a row's sum of b fits)
    for (u32 k = 0; k <= 2 * radius; ++k) {
      const int2 v = in[iy * kBoxWin + ix + k];
      s.x += v.x;
      s.y += v.y;
    }
    hs[item] = s;
  }
  __syncthreads();
  for (u32 item = t; item < kBoxTile * kBoxTile; item += kThreads) {
    const u32 iy = item >> 5, ix = item & 31u, cx = ox + ix, cy = oy + iy;
    if (cx >= cw || cy >= ch) continue;
    int64_t sa = 0, sb = 0;
    for (u32 k = 0; k <= 2 * radius; ++k) {
      const int2 v = hs[(iy + k) * kBoxTile + ix];
      sa += v.x;
      sb += v.y;
    }
    const u32 n = box_count(cx, cy, cw, ch, radius);
    d.mean[u64(cy) * cw + cx] = make_int2(dehaze::box_mean(sa, n), dehaze::box_mean(sb, n));
  }
}

__global__ __launch_bounds__(kThreads) void dehaze_apply_kernel(const DehazeDesc* __restrict__ descs) {
  __shared__ __attribute__((aligned(16))) u8 in[kTileH * kRowCap];
  __shared__ __attribute__((aligned(16))) u8 outb[kTileH * kRowCap];
  __shared__ u32 recip[dehaze::kTOne + 1];
  __shared__ int2 mc[kMeanRows * kMeanCols];
  const DehazeDesc& d = descs[blockIdx.y];
  const u32 w = u32(d.w), h = u32(d.h), t0 = u32(d.t0), strength = u32(d.strength);
  const u32 bx = blockIdx.x;
  if (bx >= stage::tiles_of(w, h)) return;
  const u32 ntx = stage::tiles_x(w);
  const u32 tk = bx / ntx, tj = bx - tk * ntx;
  const u32 j0 = tj * kTileW, j1 = min(w, j0 + kTileW);
  const u32 k0 = tk * kTileH, k1 = min(h, k0 + kTileH);
  const u32 cw = dehaze::cells(w), ch = dehaze::cells(h);
  const u32 t = threadIdx.x;
  // the window of cells: columns ilo .. ihi (at most kMeanCols), rows jlo .. jhi (at most kMeanRows)
  u32 ilo, ihi, jlo, jhi, x_, a_;
  dehaze::axis(j0, cw, ilo, x_, a_);
  dehaze::axis(j1 - 1, cw, x_, ihi, a_);
  dehaze::axis(k0, ch, jlo, x_, a_);
  dehaze::axis(k1 - 1, ch, x_, jhi, a_);
  const u32 nci = ihi - ilo + 1, nc = nci * (jhi - jlo + 1);
  const VEP_DEV int2* mean = d.mean;
  if (t < nc) {
    const u32 lj = t / nci, li = t - lj * nci;
    mc[lj * kMeanCols + li] = mean[u64(jlo + lj) * cw + ilo + li];
  }
  for (u32 tt = t; tt <= u32(dehaze::kTOne); tt += kThreads) recip[tt] = tt >= t0 ? dehaze::recip_of(tt) : 0u;
  const u32 air0 = d.air[0], air1 = d.air[1], air2 = d.air[2];
  const VEP_DEV u8* src = d.src;
  VEP_DEV u8* dst = d.dst;
  const u32 src_pitch = d.src_pitch, dst_pitch = d.dst_pitch;
  const u32 nrow = k1 - k0, nbytes = (j1 - j0) * 3;
  stage::stage_rows(src, src_pitch, k0, nrow, j0, nbytes, kRowCap, in);
  __syncthreads();
  // the thread's pixels: column c of rows q + m * kWaves
  const u32 c = t & (kTileW - 1), q = t / kTileW;
  VEP_DEV u8* out0 = dst + u64(k0) * dst_pitch + u64(j0) * 3;  // the tile's origin in the destination
  if (j0 + c < j1) {
    u32 i0, i1, wx;
    dehaze::axis(j0 + c, cw, i0, i1, wx);
    i0 -= ilo;
    i1 -= ilo;
#pragma unroll
    for (u32 m = 0; m < kRows; ++m) {
      const u32 rr = q + m * kWaves;
      if (rr >= nrow) continue;
      u32 jj0, jj1, wy;
      dehaze::axis(k0 + rr, ch, jj0, jj1, wy);
      const int2* top = mc + (jj0 - jlo) * kMeanCols;
      const int2* bot = mc + (jj1 - jlo) * kMeanCols;
      const VEP_DEV u8* g = src + u64(k0 + rr) * src_pitch + u64(j0) * 3;
      const u8* p = in + rr * kRowCap + (u32(reinterpret_cast<uintptr_t>(g)) & 15u) + c * 3;
      const u32 b0 = p[0], b1 = p[1], b2 = p[2];
      const int32_t a64 = dehaze::lerp4(top[i0].x, top[i1].x, bot[i0].x, bot[i1].x, wx, wy);
      const int32_t b64 = dehaze::lerp4(top[i0].y, top[i1].y, bot[i0].y, bot[i1].y, wx, wy);
      const u32 rc = recip[dehaze::transmission(a64, b64, motion::luma(b0, b1, b2), t0)];
      u8* o = outb + rr * kRowCap + (u32(reinterpret_cast<uintptr_t>(out0 + u64(rr) * dst_pitch)) & 15u) + c * 3;
      o[0] = u8(dehaze::recovered(b0, air0, rc, strength));
      o[1] = u8(dehaze::recovered(b1, air1, rc, strength));
      o[2] = u8(dehaze::recovered(b2, air2, rc, strength));
    }
  }
  __syncthreads();
  stage::store_rows(out0, dst_pitch, nrow, nbytes, kRowCap, outb);
}

}  // namespace

void launch_dehaze(const DehazeDesc* d_descs, const DehazeDesc* h_descs, int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= 65535, "dehaze: at most 65535 pictures per launch");
  u32 tiles = 0, boxes = 0;
  for (int i = 0; i < n; ++i) {
    const u32 w = u32(h_descs[i].w), h = u32(h_descs[i].h), cw = dehaze::cells(w), ch = dehaze::cells(h);
    tiles = std::max(tiles, stage::tiles_of(w, h));  // (w h <= 2^24: at most 2^14 tiles)
    boxes = std::max(boxes, ((cw + kBoxTile - 1) / kBoxTile) * ((ch + kBoxTile - 1) / kBoxTile));
  }
  VEP_CHECK(tiles >= 1 && boxes >= 1, "dehaze: empty launch");
  const dim3 block(kThreads), per_tile(tiles, u32(n)), per_box(boxes, u32(n));
  hipLaunchKernelGGL(dehaze_clear_kernel, dim3(u32(dehaze::kTableWords) / kThreads, u32(n)), block, 0, s, d_descs);
  hipLaunchKernelGGL(dehaze_dark_kernel<false>, per_tile, block, 0, s, d_descs);
  hipLaunchKernelGGL(dehaze_air_kernel, dim3(u32(n)), block, 0, s, d_descs);
  hipLaunchKernelGGL(dehaze_dark_kernel<true>, per_tile, block, 0, s, d_descs);
  hipLaunchKernelGGL(dehaze_coeff_kernel, per_box, block, 0, s, d_descs);
  hipLaunchKernelGGL(dehaze_smooth_kernel, per_box, block, 0, s, d_descs);
  hipLaunchKernelGGL(dehaze_apply_kernel, per_tile, block, 0, s, d_descs);
  VEP_HIP(hipGetLastError());
}

}  // namespace vep::gpu
