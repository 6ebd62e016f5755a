// gfx950 (CDNA4) quarter turns and mirrors of a served picture. See gpu.h for the contract and
// orient.h for the index arithmetic, which the CPU implementation (orient.cpp) shares: both produce
// the same bytes. ONE launch for every picture of a request: blockIdx.y is the picture, blockIdx.x
// a 64 x 64 tile of its OUTPUT (a block past its own picture's tiles exits). Pixels are moved, never
// computed on: there is no matrix-instruction work here.
//
// ONE kernel with a branch per descriptor (uniform in a block) between the row-preserving and the
// transposing ops, on one square tile for both: a batch may mix ops, staging and storing are the
// same code for all eight, and a second kernel would only save the row-preserving ops LDS they do
// not lack (docs/ORIENT.md).
//
//   source     the tile's 64 x 64 output pixels map to a rectangle of the source (orient.h: mirrored
//              ranges, swapped for T), clipped to the picture. Its rows, up to 64 of up to 192
//              bytes, are staged with stage::stage_rows: whole 16-byte vectors along rows, any
//              address and pitch, no byte outside a row's own bytes is read.
//   re-order   a lane assembles FOUR output pixels = three dwords. A quarter wave (16 lanes) owns
//              one output row of the tile, a wave four rows, the block 16 rows a pass, four passes.
//     T = 0    the four pixels are 12 consecutive bytes of one staged row: four aligned LDS dwords,
//              three v_alignbyte. With MX the pixel order is reversed, not the byte order (BGR stays
//              BGR): B3G3R3B2 | G2R2B1G1 | R1B0G0R0 out of B0G0R0B1 | G1R1B2G2 | R2B3G3R3 with four
//              v_perm.
//     T = 1    the four pixels are one column of four consecutive staged rows. Each is cut out of
//              its two aligned dwords with v_alignbyte, then p0 | p1 << 24, p1 >> 8 | p2 << 16,
//              p2 >> 16 | p3 << 8. The strided side is this LDS read, and its banks follow from
//              the staged pitch: stage_rows keeps a byte's global address modulo 16, so the pitch
//              is a multiple of 16 bytes; it is 208 = 52 dwords = 4 * 13. Rows r and r + 1 are 52 =
//              20 (mod 32) banks apart, so eight consecutive rows fall on the eight banks 0, 4 ..
//              28 (+ the column) and row r + 8 on row r's again: NO pitch that is a multiple of 16
//              bytes gives more than eight. A lane that read its rows 4g, 4g + 1 .. in turn would
//              put the quarter wave's 16 lanes on two banks in every read (4g + i is i or i + 4
//              modulo 8). So lane g reads its four rows in the order rotated by (g >> 1) & 3: in
//              one read the 16 lanes meet rows 4g + ((i + (g >> 1)) & 3), every class modulo 8
//              twice, and the wave's four quarters read four neighbouring columns, 3 bytes apart,
//              which fill the three banks between two classes or share a dword (a broadcast).
//              About two lanes a bank: what a 64-lane dword read costs on 32 banks anyway. The
//              registers are put back in order with twelve v_cndmask. (Reasoned, not measured.)
//   output     the three dwords go into LDS at the DESTINATION row's address modulo 16. Where
//              that is no multiple of 4 they are shifted across four aligned dwords; the bytes
//              that a lane lacks for its first dword come from its left neighbour's last (one
//              16-lane shuffle), so every aligned dword is written by exactly one lane, whole.
//              Rows leave with stage::store_rows, 16 at a time: whole 16-byte vectors along rows,
//              no byte outside a destination row's own bytes is written. Out of place only.
//
// Partial tiles are clipped in the indices: lanes past the last group of four or the last row
// read the last valid one and write nothing; the pixels of a last group past the row's end are
// staged bytes or padding that store_rows never sends. A 1 x N picture is N tiles' first column.
// LDS: 16 + 13,312 + 16 (staged, padded for the dword reads at either end) + 13,312 (output) =
// 26,656 bytes a block. Barriers: two.
#define VEP_KERNEL_SOURCE 1  // descriptors' pointers are global-address-space here (gpu.h)
#include <algorithm>

#include "gpu.h"
#include "gpu_stage.h"
#include "orient.h"

namespace vep::gpu {

namespace {

using stage::kThreads;
constexpr u32 kTile = 64;                      // pixels a side
constexpr u32 kCap = stage::rowcap_of(kTile);  // 208: a staged row, and an output row
constexpr u32 kPad = 16;                       // in front of and behind the staged rows
constexpr u32 kInBytes = kPad + kTile * kCap + kPad;
constexpr u32 kOutBytes = kTile * kCap;
constexpr u32 kPassRows = kThreads / (kTile / 4);  // 16: rows of one pass, and of one store_rows
static_assert(kCap == 208 && (kCap / 4) % 8 == 4, "the bank arithmetic above: 52 dwords, 4 * odd");
static_assert(kPassRows * ((kTile * 3 >> 4) + 1) <= kThreads, "store_rows: one vector per thread");
// the lowest dword read lies 9 bytes (three pixels of a mirrored last group) in front of row 0
static_assert(kPad >= 12, "front padding");
// the highest: row 63 at misalignment 15, the 16 bytes from the dword of byte 12 * 15, or the 8 from that of pixel 63
static_assert(kPad + (kTile - 1) * kCap + 15 + 12 * (kTile / 4 - 1) + 16 <= kInBytes, "back padding, rows");
static_assert(kPad + (kTile - 1) * kCap + 15 + 3 * (kTile - 1) + 8 <= kInBytes, "back padding, columns");
// an output row's four shifted dwords stay inside its own 208 bytes
static_assert(((15 + 12 * (kTile / 4 - 1)) & ~3u) + 16 <= kCap, "output row");

__device__ __forceinline__ u32 pick(u32 rot, u32 a, u32 b, u32 c, u32 d) {
  return rot == 0 ? a : (rot == 1 ? b : (rot == 2 ? c : d));
}

__global__ __launch_bounds__(kThreads) void orient_kernel(const OrientDesc* __restrict__ descs) {
  __shared__ __attribute__((aligned(16))) u8 inb[kInBytes];
  __shared__ __attribute__((aligned(16))) u8 outb[kOutBytes];
  const OrientDesc& d = descs[blockIdx.y];
  const u32 op = u32(d.op);
  const bool swap = op & orient::kT, mx = op & orient::kMX, my = op & orient::kMY;
  const u32 w = u32(d.w), h = u32(d.h), ow = swap ? h : w, oh = swap ? w : h;
  const u32 ntx = (ow + kTile - 1) / kTile, nty = (oh + kTile - 1) / kTile;
  const u32 bx = blockIdx.x;
  if (bx >= ntx * nty) return;
  const u32 tk = bx / ntx, tj = bx - tk * ntx;
  const u32 j0 = tj * kTile, j1 = min(ow, j0 + kTile);
  const u32 k0 = tk * kTile, k1 = min(oh, k0 + kTile);
  const u32 ncol = j1 - j0, nrow = k1 - k0;
  // the tile's columns and rows in mirrored coordinates (ax, ay of orient.h), then the source's
  const u32 a0 = mx ? ow - j1 : j0, a1 = mx ? ow - j0 : j1;
  const u32 b0 = my ? oh - k1 : k0, b1 = my ? oh - k0 : k1;
  const u32 xs = swap ? b0 : a0, xe = swap ? b1 : a1;
  const u32 ys = swap ? a0 : b0, ye = swap ? a1 : b1;
  const VEP_DEV u8* src = d.src;
  const u32 spitch = d.src_pitch, dpitch = d.dst_pitch;
  const u32 sbase = u32(reinterpret_cast<uintptr_t>(src)) + xs * 3;
  // byte `col - xs` pixels into staged row r (of the picture: ys + r); col may lie up to three
  // pixels outside the staged columns (the padding)
  auto at = [&](u32 r, int col) -> u32 {
    return u32(int(kPad + r * kCap + ((sbase + (ys + r) * spitch) & 15u)) + (col - int(xs)) * 3);
  };

  stage::stage_rows(src, spitch, ys, ye - ys, xs, (xe - xs) * 3, kCap, inb + kPad);
  __syncthreads();

  VEP_DEV u8* out0 = d.dst + u64(k0) * dpitch + u64(j0) * 3;  // the tile's origin in the destination
  const u32 dbase = u32(reinterpret_cast<uintptr_t>(out0));
  const u32 t = threadIdx.x, g = t & 15u, q = t >> 4;
  const u32 gl = (ncol - 1) >> 2, gc = min(g, gl);  // the last group of four that holds a pixel
  const u32 rot = (g >> 1) & 3u;
  for (u32 rb = 0; rb < nrow; rb += kPassRows) {
    const u32 rr = rb + q;
    const u32 oy = k0 + min(rr, nrow - 1);
    const u32 ay = my ? oh - 1 - oy : oy;
    const u32 ox0 = j0 + 4 * gc;
    u32 r0, r1, r2;
    if (!swap) {
      // source columns ox0 .. ox0 + 3, or mirrored ow - 4 - ox0 .. ow - 1 - ox0: 12 bytes of row ay
      const u32 a = at(ay - ys, mx ? int(ow) - 4 - int(ox0) : int(ox0)), sh = a & 3u;
      const u32* wp = reinterpret_cast<const u32*>(inb + (a & ~3u));
      const u32 d0 = wp[0], d1 = wp[1], d2 = wp[2], d3 = wp[3];
      r0 = __builtin_amdgcn_alignbyte(d1, d0, sh);
      r1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
      r2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
      if (mx) {  // B0G0R0B1 G1R1B2G2 R2B3G3R3 -> B3G3R3B2 G2R2B1G1 R1B0G0R0 (selector 0..3: second operand)
        const u32 x = __builtin_amdgcn_perm(r2, r0, 0x00000304u);  // R2 B1 . .
        const u32 o0 = __builtin_amdgcn_perm(r2, r1, 0x02070605u);
        const u32 o1 = __builtin_amdgcn_perm(x, r1, 0x00050403u);
        const u32 o2 = __builtin_amdgcn_perm(r1, r0, 0x02010005u);
        r0 = o0, r1 = o1, r2 = o2;
      }
    } else {
      // source column ay, rows ax(ox0) .. ax(ox0 + 3), read in the lane's rotated order
      u32 p[4];
#pragma unroll
      for (u32 i = 0; i < 4; ++i) {
        const u32 ox = min(ox0 + ((i + rot) & 3u), j1 - 1);
        const u32 ax = mx ? ow - 1 - ox : ox;
        const u32 a = at(ax - ys, int(ay));
        const u32* wp = reinterpret_cast<const u32*>(inb + (a & ~3u));
        p[i] = __builtin_amdgcn_alignbyte(wp[1], wp[0], a & 3u) & 0xffffffu;
      }
      // p[i] is pixel (i + rot) & 3: pixel k is p[(k - rot) & 3]
      const u32 p0 = pick(rot, p[0], p[3], p[2], p[1]), p1 = pick(rot, p[1], p[0], p[3], p[2]);
      const u32 p2 = pick(rot, p[2], p[1], p[0], p[3]), p3 = pick(rot, p[3], p[2], p[1], p[0]);
      r0 = p0 | (p1 << 24);
      r1 = (p1 >> 8) | (p2 << 16);
      r2 = (p2 >> 16) | (p3 << 8);
    }
    // (every lane takes part: the loop and the branch are uniform in the block)
    const u32 left = __shfl_up(r2, 1u, 16);
    if (rr < nrow && g <= gl) {
      const u32 a = rr * kCap + ((dbase + rr * dpitch) & 15u) + 12 * g, sh = a & 3u;
      u32* wq = reinterpret_cast<u32*>(outb + (a & ~3u));
      if (sh) {
        const u32 n = 4 - sh;  // the lane's 12 bytes start `sh` bytes into wq[0]
        wq[0] = __builtin_amdgcn_alignbyte(r0, left, n);
        wq[1] = __builtin_amdgcn_alignbyte(r1, r0, n);
        wq[2] = __builtin_amdgcn_alignbyte(r2, r1, n);
        if (g == gl) wq[3] = __builtin_amdgcn_alignbyte(0u, r2, n);
      } else {
        wq[0] = r0;
        wq[1] = r1;
        wq[2] = r2;
      }
    }
  }
  __syncthreads();
  for (u32 rb = 0; rb < nrow; rb += kPassRows)
    stage::store_rows(out0 + u64(rb) * dpitch, dpitch, min(kPassRows, nrow - rb), ncol * 3, kCap, outb + rb * kCap);
}

}  // namespace

void launch_orient(const OrientDesc* d_descs, const OrientDesc* h_descs, int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= 65535, "orient: at most 65535 pictures per launch");
  u64 blocks = 0;
  for (int i = 0; i < n; ++i) {
    const u64 tx = (u64(u32(h_descs[i].w)) + kTile - 1) / kTile, ty = (u64(u32(h_descs[i].h)) + kTile - 1) / kTile;
    blocks = std::max(blocks, tx * ty);  // (the same for the output: a transposition swaps the two)
  }
  VEP_CHECK(blocks >= 1 && blocks < (u64(1) << 31), "orient: launch too large");
  hipLaunchKernelGGL(orient_kernel, dim3(u32(blocks), u32(n)), dim3(kThreads), 0, s, d_descs);
  VEP_HIP(hipGetLastError());
}

}  // namespace vep::gpu
