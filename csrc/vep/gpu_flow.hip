// gfx950 (CDNA4) motion vectors by exhaustive block matching. See gpu.h for the contract and flow.h
// for the arithmetic, which the CPU implementation (flow.cpp) shares: both produce the same bytes.
// TWO launches for every picture of a request; blockIdx.y is the picture (a block past its own
// picture's tiles exits). Sums of absolute differences of bytes: no matrix-instruction work here,
// the packed SAD instruction v_qsad_pk_u16_u8 does it.
//
// flow_luma_kernel   blockIdx.z is the frame (newest, earlier), blockIdx.x a tile of 16 source rows
//                    by 64 d source pixels, which become 16 / d rows of 64 samples of L. The rows
//                    are staged with stage::stage_rows (any address and pitch, no byte outside a
//                    row's own bytes is read); a lane owns one column of L and 4 / d of its rows
//                    and forms each d x d sum in registers. A separate kernel, so that a source
//                    pixel is converted once and not once per overlapping search window.
//                    LDS: 16 rows x 784 bytes (d = 4) = 12,544 bytes a block.
//
// flow_match_kernel  a block of 256 threads owns a tile of 8 x 4 blocks, 64 x 32 samples of L_0.
//   staging   the tile of L_0 (32 rows of 64 bytes) and the window of L_g: the tile with a halo of
//             R rows above and below and 16 columns left and right, clipped to the plane (bytes
//             outside it are never loaded; what stays unwritten in LDS is read only by candidates
//             that the geometry has ruled out). Plane rows are 16-byte aligned and the window
//             starts at tile origin - 16, so both come in as aligned 16-byte vectors, and a
//             window byte x sits at LDS byte x - (origin - 16): dwords stay dwords.
//   split     a wave owns one row of 8 blocks and takes them one after another; the block's 16
//             dwords sit in registers (LDS broadcast reads). The candidates of a block are split
//             over the lanes: G = R / 4 + (R + 3) / 4 + 1 aligned groups of four vx (four
//             neighbouring window bytes), consecutive lanes owning consecutive groups, and
//             P = 64 / G lanes per group, each walking N = ceil((2 R + 1) / P) consecutive vy
//             (N is 1..4: the kernel's template parameter). R = 7: 4 groups x 15 lanes x 1 vy;
//             R = 15: 8 groups x 8 lanes x 4 vy. Lanes and slots that the odd 2 R + 1 leaves over
//             are masked (key 0xFFFFFFFF) and take part in every shuffle.
//   SAD       a lane reads the N + 7 window rows of its N vertical candidates once, three dwords
//             each; v_qsad_pk_u16_u8 forms the four horizontally adjacent candidates' 4-byte SADs
//             at once from 8 window bytes against 4 block bytes, accumulated in packed u16 (16320
//             fits): 16 of them per four candidates, no realignment.
//   choice    keys from coordinates (flow::key, flow::valid), the lane's minimum in a register, the
//             block's minimum by six xor-shuffles, the SAD at (0, 0) by one shuffle from the lane
//             that owns it; lane 0 writes the 8-byte record with one vector store.
//   Every loop bound is a function of R and the tile; nothing depends on data.
//   LDS: 2048 (L_0) + 65 rows x 100 bytes (window: 32 + 2 x 15 rows and 3 that the N - 1 unused
//   slots of a lane may reach above it), 16-byte aligned = 8,560 bytes a block.
#define VEP_KERNEL_SOURCE 1  // descriptors' pointers are global-address-space here (gpu.h)
#include <algorithm>

#include "flow.h"
#include "gpu.h"
#include "gpu_stage.h"

namespace vep::gpu {

namespace {

using stage::kThreads;
constexpr u32 kLumaCols = 64;     // samples of L a luma tile is wide
constexpr u32 kLumaSrcRows = 16;  // source rows it stages
constexpr u32 kLumaBytes = kLumaSrcRows * stage::rowcap_of(kLumaCols * 4);  // 12,544
static_assert(kThreads == 4 * kLumaCols, "a lane owns a column of L, a wave a quarter of the tile's rows");
static_assert((kLumaSrcRows - 1) * stage::rowcap_of(kLumaCols * 4) + 15 + kLumaCols * 4 * 3 <= kLumaBytes, "the staged rows fit");
static_assert(kLumaSrcRows * ((kLumaCols * 4 * 3 >> 4) + 1) <= kThreads * 6, "stage_rows: one pass");

__host__ __device__ inline u32 luma_tiles(u32 pw, u32 ph, u32 dec) {
  const u32 trows = kLumaSrcRows / dec;
  return ((pw + kLumaCols - 1) / kLumaCols) * ((ph + trows - 1) / trows);
}

__global__ __launch_bounds__(kThreads) void flow_luma_kernel(const FlowDesc* __restrict__ descs) {
  __shared__ __attribute__((aligned(16))) u8 in[kLumaBytes];
  const FlowDesc& d = descs[blockIdx.y];
  const u32 f = blockIdx.z;
  const u32 pw = u32(d.pw), ph = u32(d.ph), dec = u32(d.decimate);
  const u32 bx = blockIdx.x;
  if (bx >= luma_tiles(pw, ph, dec)) return;
  const u32 trows = kLumaSrcRows / dec, ntx = (pw + kLumaCols - 1) / kLumaCols;
  const u32 tk = bx / ntx, tj = bx - tk * ntx;
  const u32 j0 = tj * kLumaCols, j1 = min(pw, j0 + kLumaCols);  // samples of L
  const u32 k0 = tk * trows, k1 = min(ph, k0 + trows);
  const VEP_DEV u8* src = d.src[f];
  const u32 pitch = d.src_pitch[f], rowcap = stage::rowcap_of(kLumaCols * dec);
  // source rows k0 d .. k1 d, pixels j0 d .. j1 d: inside d h' x d w', so inside the picture
  stage::stage_rows(src, pitch, k0 * dec, (k1 - k0) * dec, j0 * dec, (j1 - j0) * dec * 3, rowcap, in);
  __syncthreads();
  const u32 t = threadIdx.x, c = t & (kLumaCols - 1), q = t / kLumaCols, per = trows / 4;
  if (j0 + c >= j1) return;
  VEP_DEV u8* plane = d.plane[f];
  for (u32 m = 0; m < per; ++m) {
    const u32 r = q * per + m;
    if (k0 + r >= k1) break;
    u32 sum = 0;
    for (u32 dy = 0; dy < dec; ++dy) {
      const u32 rr = r * dec + dy;
      // (a staged row keeps its address modulo 16; only those four bits of the sum matter)
      const u32 mis = (u32(reinterpret_cast<uintptr_t>(src)) + (k0 * dec + rr) * pitch + j0 * dec * 3) & 15u;
      const u8* p = in + rr * rowcap + mis + c * dec * 3;
      for (u32 dx = 0; dx < dec; ++dx, p += 3) sum += motion::luma(p[0], p[1], p[2]);
    }
    plane[u64(k0 + r) * d.plane_pitch + j0 + c] = u8(flow::sample(sum, dec));
  }
}

constexpr u32 kTileBX = 8, kTileBY = 4;               // blocks of a tile
constexpr u32 kTileW = kTileBX * flow::kBlock;        // 64 samples
constexpr u32 kTileH = kTileBY * flow::kBlock;        // 32
constexpr u32 kHaloX = 16;                            // window columns left and right of the tile
constexpr u32 kWinVecs = (kTileW + 2 * kHaloX) / 16;  // 6 vectors a window row
constexpr u32 kWinStride = kTileW + 2 * kHaloX + 4;   // 100 bytes: 25 dwords, odd
constexpr u32 kMaxN = 4;
constexpr u32 kWinRows = kTileH + 2 * flow::kMaxRange + (kMaxN - 1);  // 65
static_assert(kThreads / 64 == kTileBY && kTileW == 64, "a wave owns a row of the tile's blocks");
static_assert(kHaloX >= u32(flow::kMaxRange) + 1 && kHaloX % 16 == 0, "the halo holds every aligned group of four vx");
static_assert(kWinStride % 4 == 0, "window rows start on dwords");

__host__ __device__ inline u32 match_tiles(u32 pw, u32 ph) {
  return ((flow::blocks(pw) + kTileBX - 1) / kTileBX) * ((flow::blocks(ph) + kTileBY - 1) / kTileBY);
}
// The split of a block's candidates over a wave (header): groups of four vx, lanes per group.
__host__ __device__ inline u32 groups_of(u32 range) { return range / 4 + (range + 3) / 4 + 1; }
__host__ __device__ inline u32 slots_of(u32 range) {
  const u32 p = 64 / groups_of(range);
  return (2 * range + 1 + p - 1) / p;
}

template <u32 N>
__global__ __launch_bounds__(kThreads) void flow_match_kernel(const FlowDesc* __restrict__ descs) {
  __shared__ __attribute__((aligned(16))) u8 l0[kTileH * kTileW];
  __shared__ __attribute__((aligned(16))) u8 win[kWinRows * kWinStride];
  const FlowDesc& d = descs[blockIdx.y];
  const int pw = d.pw, ph = d.ph, R = d.range;
  const u32 bx = blockIdx.x;
  if (bx >= match_tiles(u32(pw), u32(ph))) return;
  const u32 cols = flow::blocks(u32(pw)), rows = flow::blocks(u32(ph));
  const u32 ntx = (cols + kTileBX - 1) / kTileBX;
  const u32 ty = bx / ntx, tx = bx - ty * ntx;
  const int x0t = int(tx * kTileW), y0t = int(ty * kTileH);
  const u32 t = threadIdx.x, pitch = d.plane_pitch;
  // Aligned vectors of plane rows: a vector that starts inside the plane ends inside its pitch.
  if (t < kTileH * (kTileW / 16)) {
    const u32 r = t / (kTileW / 16), v = t % (kTileW / 16);
    const int x = x0t + int(v * 16), y = y0t + int(r);
    if (x < pw && y < ph)
      *reinterpret_cast<uint4*>(l0 + r * kTileW + v * 16) =
          *reinterpret_cast<const VEP_DEV uint4*>(d.plane[0] + u64(y) * pitch + u32(x));
  }
  const u32 nwr = kTileH + 2 * u32(R);  // window rows: LDS row kMaxN - 1 + wr is plane row y0t - R + wr
  for (u32 item = t; item < nwr * kWinVecs; item += kThreads) {
    const u32 wr = item / kWinVecs, v = item - wr * kWinVecs;
    const int x = x0t - int(kHaloX) + int(v * 16), y = y0t - R + int(wr);
    if (x < 0 || x >= pw || y < 0 || y >= ph) continue;
    const uint4 val = *reinterpret_cast<const VEP_DEV uint4*>(d.plane[1] + u64(y) * pitch + u32(x));
    u32* o = reinterpret_cast<u32*>(win + (kMaxN - 1 + wr) * kWinStride + v * 16);
    o[0] = val.x;
    o[1] = val.y;
    o[2] = val.z;
    o[3] = val.w;
  }
  __syncthreads();

  const u32 q = t >> 6, lane = t & 63u;
  const u32 by = ty * kTileBY + q;
  if (by >= rows) return;  // (the whole wave)
  const u32 G = groups_of(u32(R)), P = 64 / G;
  const int gmin = -int((u32(R) + 3) / 4);
  const u32 g = lane % G;
  u32 p = lane / G;
  const bool active = p < P && p * N <= 2 * u32(R);  // the lane has a slot with vy <= R
  if (!active) p = 0;                                // (it reads where lane p = 0 reads)
  const int vy0 = -R + int(p * N), vx0 = -4 * (int(g) + gmin);  // slot i: vy0 + i; candidate k: vx0 - k
  // LDS row of window row j of the lane, 0 <= j < N + 7: at least 0 (p N <= 2 R), at most 2 R + 34
  const u32 rowbase = kMaxN - 1 + q * 8 + 2 * u32(R) - p * N - (N - 1);
  const u32 zero_lane = (u32(R) / N) * G + u32(-gmin), zero_slot = u32(R) % N;  // the owner of (0, 0)
  const int y0 = int(by) * flow::kBlock;

  for (u32 b = 0; b < kTileBX; ++b) {
    const u32 bxg = tx * kTileBX + b;
    if (bxg >= cols) break;  // (the whole wave)
    u32 blk[8][2];
#pragma unroll
    for (u32 r = 0; r < 8; ++r) {
      const u32* pr = reinterpret_cast<const u32*>(l0 + (q * 8 + r) * kTileW + b * 8);
      blk[r][0] = pr[0];
      blk[r][1] = pr[1];
    }
    u64 acc[N];
#pragma unroll
    for (u32 i = 0; i < N; ++i) acc[i] = 0;
    // window byte of candidate k = 0: x0 - vx0 - (x0t - 16) = 16 + 8 b + 4 (g + gmin), 0 .. 84
    const u8* wcol = win + (rowbase * kWinStride + u32(int(kHaloX + b * 8) - vx0));
#pragma unroll
    for (u32 j = 0; j < N + 7; ++j) {
      const u32* wp = reinterpret_cast<const u32*>(wcol + j * kWinStride);
      const u32 w0 = wp[0], w1 = wp[1], w2 = wp[2];
      const u64 w01 = u64(w0) | u64(w1) << 32, w12 = u64(w1) | u64(w2) << 32;
#pragma unroll
      for (u32 i = 0; i < N; ++i) {
        const int r = int(j) - int(N - 1 - i);  // the block row that slot i meets in window row j
        if (r < 0 || r >= 8) continue;
        acc[i] = __builtin_amdgcn_qsad_pk_u16_u8(w01, blk[r][0], acc[i]);
        acc[i] = __builtin_amdgcn_qsad_pk_u16_u8(w12, blk[r][1], acc[i]);
      }
    }
    const int x0 = int(bxg) * flow::kBlock;
    u32 best = flow::kInvalidKey, zl = 0;
#pragma unroll
    for (u32 i = 0; i < N; ++i) {
      const int vy = vy0 + int(i);
      if (i == zero_slot) zl = u32(acc[i]) & 0xFFFFu;
#pragma unroll
      for (u32 k = 0; k < 4; ++k) {
        const int vx = vx0 - int(k);
        const u32 sad = u32(acc[i] >> (16 * k)) & 0xFFFFu;
        const bool ok = active && vy <= R && vx >= -R && vx <= R && flow::valid(x0, y0, vx, vy, pw, ph);
        best = min(best, ok ? flow::key(sad, vx, vy, R) : flow::kInvalidKey);
      }
    }
    const u32 zero = u32(__shfl(int(zl), int(zero_lane)));
#pragma unroll
    for (int m = 32; m; m >>= 1) best = min(best, u32(__shfl_xor(int(best), m)));
    if (lane == 0) {
      const flow::Record rec = flow::record_of(best, zero, R);
      d.records[u64(by) * cols + bxg] =
          make_uint2(u32(u8(rec.vx)) | u32(u8(rec.vy)) << 8 | u32(rec.best) << 16, u32(rec.zero));
    }
  }
}

}  // namespace

bool launch_flow_luma(const FlowDesc* d_descs, const FlowDesc* h_descs, int n, int decimate, hipStream_t s) {
  u64 luma = 0;
  for (int i = 0; i < n; ++i) {
    const FlowDesc& d = h_descs[i];
    VEP_CHECK(d.decimate == decimate, "flow: the pictures of a launch share decimate");
    luma = std::max(luma, u64(luma_tiles(u32(d.pw), u32(d.ph), u32(decimate))));
  }
  VEP_CHECK(n <= 65535 && luma < (u64(1) << 31), "flow: launch too large");
  if (n <= 0 || luma == 0) return false;  // no picture holds a sample of L: nothing to convert
  hipLaunchKernelGGL(flow_luma_kernel, dim3(u32(luma), u32(n), 2), dim3(kThreads), 0, s, d_descs);
  VEP_HIP(hipGetLastError());
  return true;
}

void launch_flow(const FlowDesc* d_descs, const FlowDesc* h_descs, int n, int decimate, int range, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= 65535, "flow: at most 65535 pictures per launch");
  flow::check_match_params(decimate, range);
  u64 match = 0;
  for (int i = 0; i < n; ++i) {
    const FlowDesc& d = h_descs[i];
    VEP_CHECK(d.decimate == decimate && d.range == range, "flow: the pictures of a launch share decimate and range");
    match = std::max(match, u64(match_tiles(u32(d.pw), u32(d.ph))));
  }
  VEP_CHECK(match < (u64(1) << 31), "flow: launch too large");
  if (!launch_flow_luma(d_descs, h_descs, n, decimate, s)) return;  // (then there is no block to match either)
  if (match == 0) return;
  const dim3 grid{u32(match), u32(n), 1};
  switch (slots_of(u32(range))) {
    case 1: hipLaunchKernelGGL(flow_match_kernel<1>, grid, dim3(kThreads), 0, s, d_descs); break;
    case 2: hipLaunchKernelGGL(flow_match_kernel<2>, grid, dim3(kThreads), 0, s, d_descs); break;
    case 3: hipLaunchKernelGGL(flow_match_kernel<3>, grid, dim3(kThreads), 0, s, d_descs); break;
    default: hipLaunchKernelGGL(flow_match_kernel<4>, grid, dim3(kThreads), 0, s, d_descs); break;
  }
  VEP_HIP(hipGetLastError());
}

}  // namespace vep::gpu
