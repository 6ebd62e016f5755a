// gfx950 (CDNA4) tamper detection. See gpu.h for the contract and tamper.h for the arithmetic,
// which the CPU implementation (tamper.cpp) shares: both produce the same bytes.
//
// One launch covers every picture: blockIdx.y is the picture, blockIdx.x a block of it (a block
// past its own picture's work exits).
//
// A block owns whole cells, as in the motion kernel: one row of the cell grid (`cell` pixel rows)
// and a chunk of its columns, a multiple of lcm(cell, 8) pixels wide, so a chunk starts at a cell
// boundary. No pixel pair of the energy crosses a cell boundary, so a block needs nothing from
// another block's cells. The block stages the source rows of a pass in LDS (stage::stage_rows,
// gpu_stage.h: a byte keeps its address modulo 16). The chunk geometry and the lumas of 8 pixels
// out of the staged rows are the motion kernel's too and live in gpu_cells.h.
//
// A thread owns one column of 8 pixels of the chunk for the block's whole life, and in every pass
// a segment of the pass's rows, which it walks downwards: it computes the 8 lumas of a row and the
// next pixel's (9 lumas out of eight aligned LDS dwords), and keeps them in registers as the
// current row while it computes the row below. The horizontal pairs come from the current row,
// the vertical pairs from the two rows; no luma goes through memory. A column of 8 pixels lies in
// at most two cells (cell >= 8), split at a position that is fixed per thread, so the sums and
// energies of the two cells are accumulated in registers over all rows and passes and reach the
// block's per-cell LDS counters once, at the end (integer atomics: the sum does not depend on the
// order). A pass stages one row more than it owns, the first row of the next pass, so the
// vertical pair of a pass's last row has its second luma (passes overlap by one row; the last
// pass of a cell row owns all its rows); the same holds between segments, whose threads compute
// the first row of the next segment once more.
//
// The block's 256-bin histogram lives in LDS. Its worst case is the uniform picture, every lane
// on one bin: equal neighbouring lumas of a row's 8 pixels are merged into one add, and when
// every active lane of a wave holds one value the wave votes and a single lane adds its count.
// When the block's rows are done every cell of the block is written once by a plain store, and
// the block's histogram is merged into the picture's by at most one global integer atomic add per
// non-zero bin; the picture's histogram is zeroed on the same stream before the launch. Integer
// sums do not depend on the order, so the result does not depend on scheduling. No float is
// involved anywhere.
//
// check_tamper() proves on the host that every access lies inside the source rows, the two grid
// planes and the histogram.
#define VEP_KERNEL_SOURCE 1  // descriptors' pointers are global-address-space here (gpu.h)
#include <algorithm>

#include "gpu.h"
#include "gpu_cells.h"
#include "tamper.h"

namespace vep::gpu {

namespace {

using cells::chunk_of;
using stage::kLdsBytes;
using stage::kThreads;
constexpr u32 kMaxCells = cells::kChunkPix / u32(tamper::kMinCell);  // cells of a chunk
// Every cell in 8..128: a chunk has at most kMaxCells cells and at most kThreads columns of 8
// pixels, and at least two rows of the widest chunk fit the staging buffer (a pass that is not
// the last owns one row less than it stages).
static_assert(cells::chunks_fit(u32(tamper::kMinCell), u32(tamper::kMaxCell), kMaxCells, kThreads, 2), "chunk geometry");

__global__ __launch_bounds__(kThreads) void tamper_kernel(const TamperDesc* __restrict__ descs) {
  __shared__ __attribute__((aligned(16))) u8 lds[kLdsBytes + 16];  // (+ 16: the columns' dword reads)
  __shared__ u32 hh[tamper::kBins];
  __shared__ u32 cs[kMaxCells], en[kMaxCells];
  const TamperDesc& d = descs[blockIdx.y];
  // (every field is read into a register once: the descriptor itself stays in global memory)
  const u32 w = u32(d.w), h = u32(d.h), cell = u32(d.cell);
  const u32 chunk = chunk_of(cell);
  const u32 nch = (w + chunk - 1) / chunk;
  const u32 bx = blockIdx.x;
  if (bx >= nch * tamper::cells(h, cell)) return;
  const VEP_DEV u8* src = d.src;
  const u32 src_pitch = d.src_pitch;
  const u32 gy = bx / nch, c = bx - gy * nch;
  const u32 x0 = c * chunk, x1 = min(w, x0 + chunk);  // the block's pixel columns
  const u32 y0 = gy * cell, y1 = min(h, y0 + cell);   // and rows
  const u32 cw = x1 - x0, nbytes = cw * 3;
  const u32 gpr = (cw + 7) >> 3;                      // columns of 8 pixels, <= kThreads (chunks_fit)
  const u32 rowcap = stage::rowcap_of(cw);
  const u32 rpp = kLdsBytes / rowcap;                 // rows staged per pass, >= 2 (chunks_fit)
  const u32 ncell = (cw + cell - 1) / cell;
  const u32 t = threadIdx.x;
  // The thread's column g and its segment s of every pass's rows; threads past the last whole
  // segment stay idle.
  const u32 nseg_max = kThreads / gpr;
  const u32 s = t / gpr, g = t - s * gpr;
  const bool col = s < nseg_max;
  const u32 px = x0 + g * 8, n = min(8u, x1 - px);
  // The column's pixels i < split lie in cell ci, the others in cell ci + 1.
  const u32 ci = (px - x0) / cell;
  const u32 to_edge = cell - ((px - x0) - ci * cell);  // pixels from px to the cell's right edge
  const u32 split = min(8u, to_edge);
  // bit i: the horizontal pair of pixel i counts (its right neighbour exists and is in the same cell)
  u32 hmask = 0;
#pragma unroll
  for (u32 i = 0; i < 8; ++i)
    if (i < n && px + i + 1 < w && i + 1 != to_edge) hmask |= 1u << i;
  const u32 base_mis = u32(reinterpret_cast<uintptr_t>(src)) + x0 * 3;  // (only its low 4 bits are used)
  u32 sum0 = 0, sum1 = 0, en0 = 0, en1 = 0;
  // (the first pass's barrier orders these)
  for (u32 i = t; i < ncell; i += kThreads) cs[i] = en[i] = 0;
  for (u32 i = t; i < u32(tamper::kBins); i += kThreads) hh[i] = 0;
  for (u32 rb = y0; rb < y1;) {
    const u32 ns = min(rpp, y1 - rb);            // rows staged
    const u32 nr = rb + ns == y1 ? ns : ns - 1;  // rows owned: the last staged row opens the next pass
    stage::stage_rows(src, src_pitch, rb, ns, x0, nbytes, rowcap, lds);
    __syncthreads();
    const u32 nseg = min(nseg_max, nr), rps = (nr + nseg - 1) / nseg;
    const u32 r0 = s * rps, r1 = col ? min(r0 + rps, nr) : 0;  // the thread's rows of this pass
    auto lumas = [&](u32 rr, u32 (&y)[9]) {
      const u32 mis = (base_mis + (rb + rr) * src_pitch) & 15u;
      cells::lumas<true>(lds, rr * rowcap + mis + g * 24, n, y);
    };
    u32 cur[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (r0 < r1) lumas(r0, cur);
    for (u32 k = 0; k < rps; ++k) {  // (uniform: the waves vote below)
      const u32 rr = r0 + k;
      const bool act = rr < r1;
      const bool vert = act && rb + rr + 1 < y1;  // the row below lies in the same cells, and is staged
      u32 nxt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      if (vert) lumas(rr + 1, nxt);
      bool single = true;  // the column's pixels of this row share one luma
      if (act) {
        u32 sa = 0, sb = 0, ea = 0, eb = 0;
#pragma unroll
        for (u32 i = 0; i < 8; ++i) {
          u32 e = (hmask >> i) & 1u ? tamper::sq_diff(cur[i + 1], cur[i]) : 0u;
          if (vert && i < n) e += tamper::sq_diff(nxt[i], cur[i]);
          single = single && (i >= n || cur[i] == cur[0]);
          if (i < split) {
            sa += cur[i];  // (pixels past n are 0)
            ea += e;
          } else {
            sb += cur[i];
            eb += e;
          }
        }
        sum0 += sa;
        sum1 += sb;
        en0 += ea;
        en1 += eb;
      }
      // The histogram of the row.
      const u64 live = __ballot(act);
      if (live) {
        const u32 first = u32(__ffsll(static_cast<long long>(live))) - 1u;
        const u32 v0 = u32(__shfl(int(cur[0]), int(first)));
        if (__all(!act || (single && cur[0] == v0))) {
          // one luma in the whole wave (the covered lens): one add for its full columns
          const u64 full = __ballot(act && n == 8);
          if (act && n < 8) atomicAdd(&hh[v0], n);
          if ((t & 63u) == first && full) atomicAdd(&hh[v0], 8u * u32(__popcll(full)));
        } else if (act) {
          u32 prev = cur[0], cnt = 1;  // equal neighbours merged
#pragma unroll
          for (u32 i = 1; i < 8; ++i)
            if (i < n) {
              if (cur[i] == prev) {
                ++cnt;
              } else {
                atomicAdd(&hh[prev], cnt);
                prev = cur[i];
                cnt = 1;
              }
            }
          atomicAdd(&hh[prev], cnt);
        }
      }
      if (act) {
#pragma unroll
        for (u32 i = 0; i < 9; ++i) cur[i] = nxt[i];
      }
    }
    rb += nr;
    __syncthreads();  // (the next pass's staging overwrites the rows just read)
  }
  // the column's two cells; the second one exists where it got anything
  if (sum0) atomicAdd(&cs[ci], sum0);
  if (en0) atomicAdd(&en[ci], en0);
  if (sum1) atomicAdd(&cs[ci + 1], sum1);
  if (en1) atomicAdd(&en[ci + 1], en1);
  __syncthreads();
  const u64 at = u64(gy) * tamper::cells(w, cell) + x0 / cell;
  VEP_DEV u32* sum_y = d.sum_y + at;
  VEP_DEV u32* energy = d.energy + at;
  for (u32 i = t; i < ncell; i += kThreads) {
    sum_y[i] = cs[i];
    energy[i] = en[i];
  }
  VEP_DEV u32* hist = d.hist;
  for (u32 i = t; i < u32(tamper::kBins); i += kThreads) {
    const u32 v = hh[i];
    if (v) atomicAdd(&hist[i], v);
  }
}

}  // namespace

void check_tamper(const TamperDesc& d, size_t src_bytes, size_t grid_cells) {
  VEP_CHECK(d.src && d.hist && d.sum_y && d.energy, "tamper: null source, histogram or grid");
  VEP_CHECK(d.w >= 1 && d.h >= 1 && d.w <= tamper::kMaxSide && d.h <= tamper::kMaxSide,
            "tamper: picture size must be 1..65535");
  tamper::check_cell(d.cell);
  const u64 w = u64(d.w), h = u64(d.h);
  VEP_CHECK(u64(d.src_pitch) >= w * 3, "tamper: source pitch shorter than a row");
  VEP_CHECK((h - 1) * d.src_pitch + w * 3 <= src_bytes, "tamper: source rows outside the source");
  const u64 cells = u64(tamper::cells(u32(d.w), u32(d.cell))) * tamper::cells(u32(d.h), u32(d.cell));
  VEP_CHECK(cells <= grid_cells, "tamper: the grid does not fit the planes");
  const uintptr_t hs = reinterpret_cast<uintptr_t>(d.hist), ss = reinterpret_cast<uintptr_t>(d.sum_y),
                  es = reinterpret_cast<uintptr_t>(d.energy);
  VEP_CHECK(hs % 4 == 0 && ss % 4 == 0 && es % 4 == 0, "tamper: histogram and grid planes must be 4-byte aligned");
  const u64 hb = u64(tamper::kBins) * sizeof(u32), gb = u64(grid_cells) * sizeof(u32);
  auto apart = [](uintptr_t a, u64 an, uintptr_t b, u64 bn) { return a + an <= b || b + bn <= a; };
  VEP_CHECK(apart(hs, hb, ss, gb) && apart(hs, hb, es, gb) && apart(ss, gb, es, gb),
            "tamper: the histogram and the grid planes overlap");
}

void launch_tamper(const TamperDesc* d_descs, const TamperDesc* h_descs, int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= 65535, "tamper: at most 65535 pictures per launch");
  u64 blocks = 0;
  for (int i = 0; i < n; ++i) {
    const TamperDesc& d = h_descs[i];
    const u32 chunk = chunk_of(u32(d.cell));
    blocks = std::max(blocks, u64((u32(d.w) + chunk - 1) / chunk) * tamper::cells(u32(d.h), u32(d.cell)));
  }
  VEP_CHECK(blocks >= 1 && blocks < (u64(1) << 31), "tamper: launch too large");
  hipLaunchKernelGGL(tamper_kernel, dim3(u32(blocks), u32(n)), dim3(kThreads), 0, s, d_descs);
  VEP_HIP(hipGetLastError());
}

}  // namespace vep::gpu
