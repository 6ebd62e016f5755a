// gfx950 (CDNA4) contrast enhancement: contrast-limited adaptive histogram equalisation on luma.
// See gpu.h for the contract and clahe.h for the arithmetic, which the CPU implementation
// (clahe.cpp) shares: both produce the same bytes. Three kernels, each ONE launch for every picture
// of a request: blockIdx.y is the picture, blockIdx.x a block of it (a block past its own picture's
// work exits). Integer table lookups and 8-bit blends: there is no matrix-instruction work here.
//
// 1. clahe_hist_kernel: per-tile luma histograms. A block owns one row of the tile grid (`tile`
//    pixel rows) and a chunk of its columns (cells::chunk_of: whole tiles, at most 16 of them and at
//    most 512 pixels), so every pixel of a tile is seen by ONE block: the tile's 256 bins leave by
//    plain stores, there are no global atomics and nothing is zeroed before the launch. The block
//    stages its rows in LDS pass by pass (stage::stage_rows) beside the 16 tile histograms (16 KB).
//    A thread owns a column of 8 pixels (cells::lumas) and a segment of every pass's rows; tile is
//    a multiple of 8 and a chunk starts at a tile boundary, so a column lies in one tile and adds
//    into one LDS histogram. The worst case is the one-colour picture, every lane on one bin:
//    equal neighbours among a row's 8 lumas are merged into one add, and when every active lane of
//    a wave holds one value the wave votes and the first lane of each run of lanes that share a
//    tile adds the run's pixel count (at tile 128: 4 adds a wave and row, on 4 different
//    histograms, instead of 64 on 4 addresses).
// 2. clahe_lut_kernel: one block per tile, one thread per bin. The bin sums its group's histograms
//    (1, 2 or 4 tiles: clahe.h's thin rule), clips, the excess is reduced inside the waves by
//    shuffles and across the four waves through LDS, the bin takes its share back, an inclusive
//    scan runs inside the wave and across the waves through LDS, and the scaled, strength-folded
//    byte is stored. Tiles of one group compute the same LUT twice: the apply pass then needs no
//    indirection.
// 3. clahe_apply_kernel: the 64 x 16 tile of gpu_stage.h. Along x the first LUT index of 64
//    consecutive pixels grows by at most ceil(63 / 32) = 2 and the second is one more, so a tile
//    touches at most 4 LUT columns, and likewise 3 LUT rows (kLutCols, kLutRows: asserted below);
//    those 12 LUTs, 3 KB, are staged in LDS as dwords. The tile's BGR rows are staged
//    (stage::stage_rows), a wave owns every fourth row and a lane one column: luma, four LDS byte
//    lookups, the blend, the additive shift with its clamp; the pixels go to LDS at their
//    DESTINATION address modulo 16 and out with stage::store_rows. A tile's bytes are read and
//    written by its block alone, so in place is race-free; out of place the source is never written.
//
// check_clahe() proves on the host that every access of the three kernels lies inside the source,
// the destination and the two planes, and that those do not overlap.
#define VEP_KERNEL_SOURCE 1  // descriptors' pointers are global-address-space here (gpu.h)
#include <algorithm>

#include "clahe.h"
#include "gpu.h"
#include "gpu_cells.h"

namespace vep::gpu {

namespace {

using cells::chunk_of;
using stage::kLdsBytes;
using stage::kRows;
using stage::kThreads;
using stage::kTileH;
using stage::kTileW;
using stage::kWaves;
constexpr u32 kBins = u32(clahe::kBins);
constexpr u32 kMaxTiles = cells::kChunkPix / u32(clahe::kMinTile);  // tiles of a chunk: 16
// Every tile in 32..256: a chunk is whole tiles, at most kMaxTiles of them, at most kThreads
// columns of 8 pixels, and at least one row of the widest chunk fits the staging buffer.
static_assert(cells::chunks_fit(u32(clahe::kMinTile), u32(clahe::kMaxTile), kMaxTiles, kThreads, 1), "chunk geometry");
static_assert(clahe::kMinTile % 8 == 0, "a column of 8 pixels lies in one tile");
static_assert(kThreads == kBins, "one thread per bin");

// The LUTs a 64 x 16 tile touches: floor((a + d) / T) - floor(a / T) <= ceil(d / T), so the first
// index grows by at most ceil((side - 1) / tile) over a side, and the second index adds one.
constexpr u32 kLutCols = (kTileW - 1 + u32(clahe::kMinTile) - 1) / u32(clahe::kMinTile) + 2;  // 4
constexpr u32 kLutRows = (kTileH - 1 + u32(clahe::kMinTile) - 1) / u32(clahe::kMinTile) + 2;  // 3
static_assert(kLutCols == 4 && kLutRows == 3, "LUT window of an apply tile");
constexpr u32 kRowCap = stage::kTileRowCap;

__global__ __launch_bounds__(kThreads) void clahe_hist_kernel(const ClaheDesc* __restrict__ descs) {
  __shared__ __attribute__((aligned(16))) u8 lds[kLdsBytes + 16];  // (+ 16: the columns' dword reads)
  __shared__ u32 hh[kMaxTiles * kBins];
  const ClaheDesc& d = descs[blockIdx.y];
  const u32 w = u32(d.w), h = u32(d.h), tile = u32(d.tile);
  const u32 chunk = chunk_of(tile);
  const u32 nch = (w + chunk - 1) / chunk;
  const u32 bx = blockIdx.x;
  if (bx >= nch * clahe::cells(h, tile)) return;
  const VEP_DEV u8* src = d.src;
  const u32 src_pitch = d.src_pitch;
  const u32 gy = bx / nch, c = bx - gy * nch;
  const u32 x0 = c * chunk, x1 = min(w, x0 + chunk);  // the block's pixel columns
  const u32 y0 = gy * tile, y1 = min(h, y0 + tile);   // and rows
  const u32 cw = x1 - x0, nbytes = cw * 3;
  const u32 gpr = (cw + 7) >> 3;                      // columns of 8 pixels, <= kThreads (chunks_fit)
  const u32 rowcap = stage::rowcap_of(cw);
  const u32 rpp = kLdsBytes / rowcap;                 // rows staged per pass, >= 1 (chunks_fit)
  const u32 ntile = (cw + tile - 1) / tile;           // <= kMaxTiles (chunks_fit)
  const u32 t = threadIdx.x, lane = t & 63u;
  // The thread's column g and its segment s of every pass's rows; threads past the last whole
  // segment stay idle.
  const u32 nseg_max = kThreads / gpr;
  const u32 s = t / gpr, g = t - s * gpr;
  const bool col = s < nseg_max;
  const u32 px = x0 + g * 8, n = min(8u, x1 - px);
  const u32 tpl = tile >> 3;  // columns of a tile
  const u32 ci = g / tpl;     // the column's tile, < ntile
  u32* mine = hh + ci * kBins;
  // The run of the vote: the lanes from this one on that lie in the same wave, segment and tile.
  const u32 run_len = min(min((ci + 1) * tpl, gpr) - g, 64u - lane);
  const bool leader = lane == 0 || g == ci * tpl;
  const u32 run_pix = min(x1, px + run_len * 8) - px;
  const u32 base_mis = u32(reinterpret_cast<uintptr_t>(src)) + x0 * 3;  // (only its low 4 bits are used)
  // (the first pass's barrier orders these)
  for (u32 i = t; i < ntile * kBins; i += kThreads) hh[i] = 0;
  for (u32 rb = y0; rb < y1;) {
    const u32 ns = min(rpp, y1 - rb);  // rows staged, all owned
    stage::stage_rows(src, src_pitch, rb, ns, x0, nbytes, rowcap, lds);
    __syncthreads();
    const u32 nseg = min(nseg_max, ns), rps = (ns + nseg - 1) / nseg;
    const u32 r0 = s * rps, r1 = col ? min(r0 + rps, ns) : 0;  // the thread's rows of this pass
    for (u32 k = 0; k < rps; ++k) {  // (uniform: the waves vote below)
      const u32 rr = r0 + k;
      const bool act = rr < r1;
      u32 y[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      bool single = true;  // the column's pixels of this row share one luma
      if (act) {
        const u32 mis = (base_mis + (rb + rr) * src_pitch) & 15u;
        cells::lumas<false>(lds, rr * rowcap + mis + g * 24, n, y);
#pragma unroll
        for (u32 i = 1; i < 8; ++i) single = single && (i >= n || y[i] == y[0]);
      }
      const u64 live = __ballot(act);
      if (!live) continue;
      const u32 first = u32(__ffsll(static_cast<long long>(live))) - 1u;
      const u32 v0 = u32(__shfl(int(y[0]), int(first)));
      if (__all(!act || (single && y[0] == v0))) {
        // one luma in the whole wave (the dark scene's flat wall): one add per run of a tile's lanes
        // (a run lies in one segment, so its lanes are active together)
        if (act && leader) atomicAdd(&mine[v0], run_pix);
      } else if (act) {
        u32 prev = y[0], cnt = 1;  // equal neighbours merged
#pragma unroll
        for (u32 i = 1; i < 8; ++i)
          if (i < n) {
            if (y[i] == prev) {
              ++cnt;
            } else {
              atomicAdd(&mine[prev], cnt);
              prev = y[i];
              cnt = 1;
            }
          }
        atomicAdd(&mine[prev], cnt);
      }
    }
    rb += ns;
    __syncthreads();  // (the next pass's staging overwrites the rows just read; the last: hh is whole)
  }
  // the block's tiles lie side by side in the plane: tile (gy, x0 / tile + i) for i < ntile
  VEP_DEV u32* out = d.hist + (u64(gy) * clahe::cells(w, tile) + x0 / tile) * kBins;
  for (u32 i = t; i < ntile * kBins; i += kThreads) out[i] = hh[i];
}

__global__ __launch_bounds__(kThreads) void clahe_lut_kernel(const ClaheDesc* __restrict__ descs) {
  __shared__ u32 part[kWaves], ends[kWaves];
  const ClaheDesc& d = descs[blockIdx.y];
  const u32 w = u32(d.w), h = u32(d.h), tile = u32(d.tile);
  const u32 cols = clahe::cells(w, tile), rows = clahe::cells(h, tile);
  const u32 bx = blockIdx.x;
  if (bx >= cols * rows) return;
  const u32 j = bx / cols, i = bx - j * cols;
  const u32 gi = clahe::group_of(i, w, tile, cols), gj = clahe::group_of(j, h, tile, rows);
  const u32 n = clahe::group_span(gi, w, tile, cols) * clahe::group_span(gj, h, tile, rows);
  // the group's tiles: gi .. i_end x gj .. j_end (the thin last column / row joins its neighbour)
  const u32 i_end = clahe::thin(w, tile, cols) && gi == cols - 2 ? cols : gi + 1;
  const u32 j_end = clahe::thin(h, tile, rows) && gj == rows - 2 ? rows : gj + 1;
  const u32 v = threadIdx.x, lane = v & 63u, wave = v >> 6;
  const VEP_DEV u32* hist = d.hist;
  u32 hv = 0;
  for (u32 jj = gj; jj < j_end; ++jj)
    for (u32 ii = gi; ii < i_end; ++ii) hv += hist[(u64(jj) * cols + ii) * kBins + v];
  const u32 limit = clahe::clip_limit(u32(d.clip16), n);
  u32 ex = hv > limit ? hv - limit : 0u;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) ex += u32(__shfl_xor(int(ex), off));
  if (lane == 0) part[wave] = ex;
  __syncthreads();
  const u32 excess = part[0] + part[1] + part[2] + part[3];
  u32 cv = clahe::redistributed(hv, v, limit, excess);
#pragma unroll
  for (u32 off = 1; off < 64; off <<= 1) {
    const u32 o = u32(__shfl_up(int(cv), off));
    if (lane >= off) cv += o;
  }
  if (lane == 63) ends[wave] = cv;
  __syncthreads();
  for (u32 k = 0; k < wave; ++k) cv += ends[k];
  d.lut[u64(bx) * kBins + v] = u8(clahe::lut_value(v, cv, n, u32(d.strength)));
}

__global__ __launch_bounds__(kThreads) void clahe_apply_kernel(const ClaheDesc* __restrict__ descs) {
  __shared__ __attribute__((aligned(16))) u8 in[kTileH * kRowCap];
  __shared__ __attribute__((aligned(16))) u8 outb[kTileH * kRowCap];
  __shared__ u32 luts[kLutRows * kLutCols * (kBins / 4)];
  const ClaheDesc& d = descs[blockIdx.y];
  const u32 w = u32(d.w), h = u32(d.h), tile = u32(d.tile);
  const u32 bx = blockIdx.x;
  if (bx >= stage::tiles_of(w, h)) return;
  const u32 ntx = stage::tiles_x(w);
  const u32 tk = bx / ntx, tj = bx - tk * ntx;
  const u32 j0 = tj * kTileW, j1 = min(w, j0 + kTileW);
  const u32 k0 = tk * kTileH, k1 = min(h, k0 + kTileH);
  const u32 cols = clahe::cells(w, tile), rows = clahe::cells(h, tile);
  const u32 t = threadIdx.x;
  // the window of LUTs: columns ilo .. ihi (at most kLutCols), rows jlo .. jhi (at most kLutRows)
  u32 ilo, ihi, jlo, jhi, x_, a_;
  clahe::axis(j0, tile, cols, ilo, x_, a_);
  clahe::axis(j1 - 1, tile, cols, x_, ihi, a_);
  clahe::axis(k0, tile, rows, jlo, x_, a_);
  clahe::axis(k1 - 1, tile, rows, x_, jhi, a_);
  const u32 nci = ihi - ilo + 1, nl = nci * (jhi - jlo + 1);
  const VEP_DEV u32* lut32 = reinterpret_cast<const VEP_DEV u32*>(d.lut);  // (4-byte aligned: check_clahe)
  for (u32 idx = t; idx < nl * (kBins / 4); idx += kThreads) {
    const u32 l = idx >> 6, word = idx & 63u;
    const u32 lj = l / nci, li = l - lj * nci;
    luts[(lj * kLutCols + li) * (kBins / 4) + word] = lut32[(u64(jlo + lj) * cols + ilo + li) * (kBins / 4) + word];
  }
  const VEP_DEV u8* src = d.src;
  VEP_DEV u8* dst = d.dst;
  const u32 src_pitch = d.src_pitch, dst_pitch = d.dst_pitch;
  const u32 nrow = k1 - k0, nbytes = (j1 - j0) * 3;
  stage::stage_rows(src, src_pitch, k0, nrow, j0, nbytes, kRowCap, in);
  __syncthreads();
  // the thread's pixels: column c of rows q + m * kWaves
  const u32 c = t & (kTileW - 1), q = t / kTileW;
  const bool active = j0 + c < j1;
  VEP_DEV u8* out0 = dst + u64(k0) * dst_pitch + u64(j0) * 3;  // the tile's origin in the destination
  if (active) {
    u32 i0, i1, ax;
    clahe::axis(j0 + c, tile, cols, i0, i1, ax);
    const u8* lb = reinterpret_cast<const u8*>(luts);
    const u32 at0 = (i0 - ilo) * kBins, at1 = (i1 - ilo) * kBins;
#pragma unroll
    for (u32 m = 0; m < kRows; ++m) {
      const u32 rr = q + m * kWaves;
      if (rr >= nrow) continue;
      u32 jj0, jj1, ay;
      clahe::axis(k0 + rr, tile, rows, jj0, jj1, ay);
      const VEP_DEV u8* g = src + u64(k0 + rr) * src_pitch + u64(j0) * 3;
      const u8* p = in + rr * kRowCap + (u32(reinterpret_cast<uintptr_t>(g)) & 15u) + c * 3;
      const u32 b0 = p[0], b1 = p[1], b2 = p[2];
      const u32 y = motion::luma(b0, b1, b2);
      const u8* top = lb + (jj0 - jlo) * kLutCols * kBins + y;
      const u8* bot = lb + (jj1 - jlo) * kLutCols * kBins + y;
      const u32 y_new = clahe::blend(top[at0], top[at1], bot[at0], bot[at1], ax, ay);
      u8* o = outb + rr * kRowCap + (u32(reinterpret_cast<uintptr_t>(out0 + u64(rr) * dst_pitch)) & 15u) + c * 3;
      o[0] = u8(clahe::shifted(b0, y_new, y));
      o[1] = u8(clahe::shifted(b1, y_new, y));
      o[2] = u8(clahe::shifted(b2, y_new, y));
    }
  }
  __syncthreads();
  stage::store_rows(out0, dst_pitch, nrow, nbytes, kRowCap, outb);
}

}  // namespace

size_t clahe_tiles(int w, int h, int tile) {
  return size_t(clahe::cells(u32(w), u32(tile))) * clahe::cells(u32(h), u32(tile));
}

void check_clahe(const ClaheDesc& d, size_t src_bytes, size_t dst_bytes, size_t hist_words, size_t lut_bytes) {
  VEP_CHECK(d.src && d.dst && d.hist && d.lut, "enhance: null picture or plane");
  VEP_CHECK(d.w >= 1 && d.h >= 1 && d.w <= clahe::kMaxSide && d.h <= clahe::kMaxSide,
            "enhance: picture size must be 1..65535");
  clahe::check_params(clahe::Params{d.tile, d.clip16, d.strength});
  // The histogram kernel reads rows y0 .. y1 <= h of columns x0 .. x1 <= w and the apply kernel the
  // rows and columns of its tiles, clipped to the picture: inside the spans below.
  const u64 row = u64(d.w) * 3, h = u64(d.h);
  VEP_CHECK(u64(d.src_pitch) >= row && u64(d.dst_pitch) >= row, "enhance: pitch shorter than a row");
  const u64 src_span = (h - 1) * d.src_pitch + row, dst_span = (h - 1) * d.dst_pitch + row;
  VEP_CHECK(src_span <= src_bytes, "enhance: picture rows outside the picture's memory");
  VEP_CHECK(dst_span <= dst_bytes, "enhance: output rows outside the output's memory");
  // A histogram block writes the tiles (gy, x0 / tile + i), i < ceil((x1 - x0) / tile), of a chunk
  // that starts at a tile boundary: tiles of the grid. The LUT kernel reads and writes tile bx <
  // cols * rows and its group's tiles, which group_of keeps below cols and rows; the apply kernel
  // reads the LUTs of axis(), which are < cols and < rows.
  const u64 tiles = clahe_tiles(d.w, d.h, d.tile), hb = tiles * clahe::kBins * sizeof(u32), lb = tiles * clahe::kBins;
  VEP_CHECK(tiles * clahe::kBins <= hist_words && lb <= lut_bytes, "enhance: the grid does not fit the planes");
  const uintptr_t s = reinterpret_cast<uintptr_t>(d.src), o = reinterpret_cast<uintptr_t>(d.dst),
                  hs = reinterpret_cast<uintptr_t>(d.hist), ls = reinterpret_cast<uintptr_t>(d.lut);
  VEP_CHECK(hs % 4 == 0 && ls % 4 == 0, "enhance: the planes must be 4-byte aligned");
  auto apart = [](uintptr_t a, u64 an, uintptr_t b, u64 bn) { return a + an <= b || b + bn <= a; };
  if (s == o)
    VEP_CHECK(d.src_pitch == d.dst_pitch, "enhance: in place needs equal pitches");
  else
    VEP_CHECK(apart(s, src_span, o, dst_span), "enhance: picture and output overlap");
  VEP_CHECK(apart(hs, hb, ls, lb) && apart(hs, hb, s, src_span) && apart(hs, hb, o, dst_span) &&
                apart(ls, lb, s, src_span) && apart(ls, lb, o, dst_span),
            "enhance: the planes overlap each other or a picture");
}

void launch_clahe(const ClaheDesc* d_descs, const ClaheDesc* h_descs, int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= 65535, "enhance: at most 65535 pictures per launch");
  u64 hist_blocks = 0, lut_blocks = 0, apply_blocks = 0;
  for (int i = 0; i < n; ++i) {
    const ClaheDesc& d = h_descs[i];
    const u32 w = u32(d.w), h = u32(d.h), tile = u32(d.tile), chunk = chunk_of(tile);
    hist_blocks = std::max(hist_blocks, u64((w + chunk - 1) / chunk) * clahe::cells(h, tile));
    lut_blocks = std::max(lut_blocks, u64(clahe_tiles(d.w, d.h, d.tile)));
    apply_blocks = std::max(apply_blocks, u64(stage::tiles_of(w, h)));
  }
  VEP_CHECK(hist_blocks >= 1 && lut_blocks < (u64(1) << 31) && apply_blocks < (u64(1) << 31), "enhance: launch too large");
  hipLaunchKernelGGL(clahe_hist_kernel, dim3(u32(hist_blocks), u32(n)), dim3(kThreads), 0, s, d_descs);
  hipLaunchKernelGGL(clahe_lut_kernel, dim3(u32(lut_blocks), u32(n)), dim3(kThreads), 0, s, d_descs);
  hipLaunchKernelGGL(clahe_apply_kernel, dim3(u32(apply_blocks), u32(n)), dim3(kThreads), 0, s, d_descs);
  VEP_HIP(hipGetLastError());
}

}  // namespace vep::gpu
