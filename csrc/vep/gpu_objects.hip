// gfx950 (CDNA4) moving-object boxes: a frame-difference mask, its cleanup, and 8-connected
// components by a data-dependent union-find. See gpu.h for the contract and objects.h for the
// arithmetic, which the CPU implementation (objects.cpp) shares: both produce the same bytes (the
// records in any order). The two luma planes come from flow_luma_kernel (gpu_flow.hip) unchanged.
// FIVE launches for every picture of a request; blockIdx.y is the picture, blockIdx.x a tile (a
// block past its own picture's tiles exits). Bit operations and integer atomics: no
// matrix-instruction work here.
//
// The tile is 64 x 32 samples of the plane. 64 wide, because a wave's ballot turns one row of 64
// comparisons into one u64 and the packed mask's words are then whole tile rows; 32 high, because
// 2048 samples are eight a thread, their union-find parents fill 8 KB of LDS and a tile-local index
// fits eleven bits. The parent of a node is always a smaller or the same raster index, in LDS and in
// the label plane alike; a root is its own parent.
//
// objects_mask_kernel   threshold, cleanup and the labelling inside a tile.
//   threshold  the tile and a halo of objects::kHalo = 5 samples (what an open and a grow of 3 can
//              reach; the fixed halo covers every parameter set): the 42 rows' centre words by one
//              ballot a row, the ten halo columns by LDS atomicOr. Samples outside the plane are 0.
//   cleanup    a row is a 74-bit word (unsigned __int128) in LDS; a thread owns a row. Every step is
//              a horizontal pass (shifts of the own row) and a vertical pass (the rows above and
//              below), ANDs for the erosion, ORs for the dilations, then an AND with the plane's
//              extent, so that what lies outside the plane is background for the next step. What the
//              missing rows and columns beyond the halo spoil stays within 1 + 1 + 3 = 5 samples of
//              the halo's rim and never reaches the tile. The centre words are the packed mask
//              (written once) and go on in LDS.
//   labelling  every foreground sample starts with the first sample of its row run as its parent
//              (bit arithmetic on the row word: no loop). Links to the row above are then made only
//              where they can matter: at the first sample of every stretch where both rows are set,
//              and diagonally from a run's first or last sample when the sample straight above is
//              clear. A thread owns eight columns of one row pair and unites through LDS atomicMin.
//              Then every sample finds its root and writes it as a global raster index; the area
//              plane of the tile is cleared and block 0 clears the picture's count.
// objects_seam_kernel   for every foreground sample of a tile's top row and left column: unite it
//              with its up to three neighbours across the seam in the label plane (atomicMin on
//              global memory); diagonals and corners count. A neighbour whose link follows from
//              another (the diagonals beside a set sample straight across) is skipped.
// objects_count_kernel  a tile's samples still point at their tile-local roots, so the tile counts
//              per local root in LDS; each local root then finds its global root once, adds its
//              count there (one global atomic a local component) and points at it directly.
// objects_slot_kernel   a root whose area reaches min_area takes a record slot from the picture's
//              counter, writes label and area and an empty box, and leaves the slot number in its
//              area word (kBackground: no record).
// objects_box_kernel    per local root again: the columns and rows its samples occupy as a u64 and
//              a u32 of LDS bits (atomicOr); each local component then issues four global
//              atomicMin/Max on its record's box, and every sample of the tile gets its global root.
//
// Termination: find() moves to a strictly smaller index until it meets a root; a failed atomicMin in
// unite() returns a parent smaller than the node it was tried on, and the pair's sum falls with
// every retry. No thread waits for another. All atomics are on integers, so the label plane, the
// areas and the boxes do not depend on the order; only the records' slots do.
// LDS: mask kernel 672 + 168 + 2 x 672 + 264 + 8192 = 10,640 bytes; count 8 KB; box 32 KB.
#define VEP_KERNEL_SOURCE 1  // descriptors' pointers are global-address-space here (gpu.h)
#include <algorithm>

#include "gpu.h"
#include "gpu_stage.h"
#include "objects.h"

namespace vep::gpu {

namespace {

using stage::kThreads;
using u128 = unsigned __int128;
constexpr u32 kTW = 64, kTH = 32, kTile = kTW * kTH, kPer = kTile / kThreads;
constexpr u32 kHalo = u32(objects::kHalo), kRows = kTH + 2 * kHalo, kSide = 2 * kHalo;
constexpr u32 kBg = objects::kBackground;
static_assert(kThreads == 256 && kPer == 8 && kThreads / 8 == kTH, "a thread owns eight columns of a row pair");
static_assert(kTW + 2 * kHalo <= 128 && kRows <= kThreads, "a row with its halo fits a 128-bit word, a thread owns a row");

__host__ __device__ inline u32 tiles_of(u32 pw, u32 ph) { return ((pw + kTW - 1) / kTW) * ((ph + kTH - 1) / kTH); }

// The origin of the block's tile; false for a block past the picture's tiles.
__device__ inline bool tile_of(const ObjectsDesc& d, u32& x0, u32& y0) {
  const u32 pw = u32(d.pw), ph = u32(d.ph);
  if (blockIdx.x >= tiles_of(pw, ph)) return false;
  const u32 ntx = (pw + kTW - 1) / kTW, ty = blockIdx.x / ntx;
  x0 = (blockIdx.x - ty * ntx) * kTW;
  y0 = ty * kTH;
  return true;
}

// ---- union-find in LDS -----------------------------------------------------------------------------
__device__ inline u32 find_lds(const u32* par, u32 i) {
  for (;;) {
    const u32 p = *reinterpret_cast<const volatile u32*>(par + i);
    if (p == i) return i;
    i = p;  // p < i
  }
}
__device__ inline void unite_lds(u32* par, u32 a, u32 b) {
  for (;;) {
    a = find_lds(par, a);
    b = find_lds(par, b);
    if (a == b) return;
    if (a < b) {
      const u32 s = a;
      a = b;
      b = s;
    }
    const u32 old = atomicMin(&par[a], b);
    if (old == a) return;  // a was a root and now points at b
    a = old;               // someone linked a first: unite what it pointed at (old < a) with b
  }
}

// ---- union-find in the label plane ---------------------------------------------------------------
__device__ inline u32 load(const VEP_DEV u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline u32 find_global(const VEP_DEV u32* lab, u32 i) {
  for (;;) {
    const u32 p = load(lab + i);
    if (p == i) return i;
    i = p;  // p < i: a foreground sample's parent is a foreground sample of a smaller index
  }
}
__device__ inline void unite_global(VEP_DEV u32* lab, u32 a, u32 b) {
  for (;;) {
    a = find_global(lab, a);
    b = find_global(lab, b);
    if (a == b) return;
    if (a < b) {
      const u32 s = a;
      a = b;
      b = s;
    }
    const u32 old = __hip_atomic_fetch_min(lab + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;  // (as in unite_lds; if b < old the word now holds b, and old is united with b here)
  }
}

// The tile-local slot a sample counts under: its parent p (at most its own index) when p lies in
// the tile, else its own slot (it was a local root whose parent now lies in an earlier tile).
__device__ inline u32 slot_of(u32 p, u32 idx, u32 x0, u32 y0, u32 pw) {
  const u32 py = p / pw, px = p - py * pw;
  return (py >= y0 && px >= x0 && px < x0 + kTW) ? (py - y0) * kTW + (px - x0) : idx;
}

__global__ __launch_bounds__(kThreads) void objects_mask_kernel(const ObjectsDesc* __restrict__ descs) {
  __shared__ u64 ctr[kRows];
  __shared__ u32 side[kRows];
  __shared__ u128 ra[kRows], rb[kRows];
  __shared__ u64 cm[kTH + 1];  // cm[r + 1]: row r of the tile; cm[0] = 0, the tile has no row above
  __shared__ u32 par[kTile];
  const ObjectsDesc& d = descs[blockIdx.y];
  const u32 t = threadIdx.x;
  if (blockIdx.x == 0 && t == 0) *d.count = 0;
  u32 x0, y0;
  if (!tile_of(d, x0, y0)) return;
  const i32 pw = d.pw, ph = d.ph;
  const u32 thr = u32(d.threshold), pitch = d.plane_pitch;
  const VEP_DEV u8* l0 = d.plane[0];
  const VEP_DEV u8* lg = d.plane[1];
  if (t < kRows) side[t] = 0;
  __syncthreads();
  const u32 q = t >> 6, lane = t & 63u;
  for (u32 r = q; r < kRows; r += kThreads / 64) {  // (the same trips for every lane of a wave)
    const i32 y = i32(y0 + r) - i32(kHalo), x = i32(x0 + lane);
    bool bit = false;
    if (y >= 0 && y < ph && x < pw) {
      const u64 at = u64(u32(y)) * pitch + u32(x);
      bit = objects::raw(l0[at], lg[at], thr);
    }
    const u64 word = __ballot(bit);
    if (lane == 0) ctr[r] = word;
  }
  for (u32 item = t; item < kRows * kSide; item += kThreads) {
    const u32 r = item / kSide, c = item - r * kSide;
    const i32 y = i32(y0 + r) - i32(kHalo);
    const i32 x = c < kHalo ? i32(x0 + c) - i32(kHalo) : i32(x0 + kTW + c - kHalo);
    if (y < 0 || y >= ph || x < 0 || x >= pw) continue;
    const u64 at = u64(u32(y)) * pitch + u32(x);
    if (objects::raw(l0[at], lg[at], thr)) atomicOr(&side[r], 1u << c);
  }
  __syncthreads();
  // bit j of a row is column x0 - kHalo + j
  u128 valid = 0;
  if (t < kRows) {
    const i32 y = i32(y0 + t) - i32(kHalo);
    if (y >= 0 && y < ph) {
      const u32 lo = x0 == 0 ? kHalo : 0u, hi = min(kTW + 2 * kHalo, u32(pw) - x0 + kHalo);
      valid = ((u128(1) << hi) - 1) & ~((u128(1) << lo) - 1);
    }
    ra[t] = u128(side[t] & ((1u << kHalo) - 1u)) | u128(ctr[t]) << kHalo | u128(side[t] >> kHalo) << (kHalo + kTW);
  }
  __syncthreads();
  auto step = [&](u32 radius, bool erode) {  // ra -> ra, every thread of the block takes part
    if (t < kRows) {
      const u128 m = ra[t];
      u128 acc = m;
      for (u32 k = 1; k <= radius; ++k) acc = erode ? (acc & (m << k) & (m >> k)) : (acc | (m << k) | (m >> k));
      rb[t] = acc;
    }
    __syncthreads();
    if (t < kRows) {
      u128 acc = rb[t];
      for (u32 k = 1; k <= radius; ++k) {
        const u128 up = t >= k ? rb[t - k] : u128(0), dn = t + k < kRows ? rb[t + k] : u128(0);
        acc = erode ? (acc & up & dn) : (acc | up | dn);
      }
      ra[t] = acc & valid;
    }
    __syncthreads();
  };
  if (d.open) {
    step(1, true);
    step(1, false);
  }
  if (d.grow) step(u32(d.grow), false);
  if (t < kTH) {
    const u64 w = u64(ra[t + kHalo] >> kHalo);
    cm[t + 1] = w;
    if (y0 + t < u32(ph)) d.mask[u64(y0 + t) * d.words + (x0 >> 6)] = w;
  }
  if (t == kTH) cm[0] = 0;
  __syncthreads();
  // row runs: a sample's parent is the first sample of its run
  for (u32 k = 0; k < kPer; ++k) {
    const u32 idx = t + k * kThreads, r = idx >> 6, x = idx & 63u;
    const u64 c = cm[r + 1];
    if (!(c >> x & 1u)) continue;
    const u64 zeros = ~c & ((u64(1) << x) - 1u);
    par[idx] = r * kTW + (zeros ? 64u - u32(__clzll(static_cast<long long>(zeros))) : 0u);
  }
  __syncthreads();
  {  // links to the row above
    const u32 r = t >> 3, sh = (t & 7u) * 8u;
    if (r >= 1) {
      const u64 u = cm[r], c = cm[r + 1];
      const u64 up = c & u & ~((c << 1) & (u << 1));      // the first sample of a stretch set in both rows
      const u64 ul = c & ~(c << 1) & (u << 1) & ~u;       // a run's first sample under a clear one: up-left (x >= 1)
      const u64 ur = c & ~(c >> 1) & (u >> 1) & ~u;       // a run's last sample under a clear one: up-right (x <= 62)
      for (u32 b = u32(up >> sh) & 0xFFu; b; b &= b - 1u) {
        const u32 x = sh + u32(__ffs(int(b))) - 1u;
        unite_lds(par, r * kTW + x, (r - 1) * kTW + x);
      }
      for (u32 b = u32(ul >> sh) & 0xFFu; b; b &= b - 1u) {
        const u32 x = sh + u32(__ffs(int(b))) - 1u;
        unite_lds(par, r * kTW + x, (r - 1) * kTW + x - 1u);
      }
      for (u32 b = u32(ur >> sh) & 0xFFu; b; b &= b - 1u) {
        const u32 x = sh + u32(__ffs(int(b))) - 1u;
        unite_lds(par, r * kTW + x, (r - 1) * kTW + x + 1u);
      }
    }
  }
  __syncthreads();
  for (u32 k = 0; k < kPer; ++k) {
    const u32 idx = t + k * kThreads, r = idx >> 6, x = idx & 63u;
    if (y0 + r >= u32(ph) || x0 + x >= u32(pw)) continue;
    const u32 i = (y0 + r) * u32(pw) + x0 + x;
    u32 label = kBg;
    if (cm[r + 1] >> x & 1u) {
      const u32 root = find_lds(par, idx);
      label = (y0 + (root >> 6)) * u32(pw) + x0 + (root & 63u);
    }
    d.labels[i] = label;
    d.area[i] = 0;
  }
}

// 128 threads: 0..63 the tile's top row, 64..95 its left column.
__global__ __launch_bounds__(128) void objects_seam_kernel(const ObjectsDesc* __restrict__ descs) {
  const ObjectsDesc& d = descs[blockIdx.y];
  u32 x0, y0;
  if (!tile_of(d, x0, y0)) return;
  const u32 pw = u32(d.pw), ph = u32(d.ph), t = threadIdx.x;
  VEP_DEV u32* lab = d.labels;
  if (t < kTW) {
    const u32 x = x0 + t, y = y0;
    if (y == 0 || x >= pw) return;
    const u32 i = y * pw + x, above = i - pw;
    if (load(lab + i) == kBg) return;
    if (load(lab + above) != kBg) {
      unite_global(lab, i, above);
    } else {
      if (x > 0 && load(lab + above - 1) != kBg) unite_global(lab, i, above - 1);
      if (x + 1 < pw && load(lab + above + 1) != kBg) unite_global(lab, i, above + 1);
    }
  } else if (t < kTW + kTH) {
    const u32 x = x0, y = y0 + (t - kTW);
    if (x == 0 || y >= ph) return;
    const u32 i = y * pw + x, left = i - 1;
    if (load(lab + i) == kBg) return;
    if (load(lab + left) != kBg) {
      unite_global(lab, i, left);
    } else {
      if (y > 0 && load(lab + left - pw) != kBg) unite_global(lab, i, left - pw);
      if (y + 1 < ph && load(lab + left + pw) != kBg) unite_global(lab, i, left + pw);
    }
  }
}

__global__ __launch_bounds__(kThreads) void objects_count_kernel(const ObjectsDesc* __restrict__ descs) {
  __shared__ u32 cnt[kTile];
  const ObjectsDesc& d = descs[blockIdx.y];
  u32 x0, y0;
  if (!tile_of(d, x0, y0)) return;
  const u32 pw = u32(d.pw), ph = u32(d.ph), t = threadIdx.x;
  VEP_DEV u32* lab = d.labels;
  for (u32 k = 0; k < kPer; ++k) cnt[t + k * kThreads] = 0;
  __syncthreads();
  for (u32 k = 0; k < kPer; ++k) {
    const u32 idx = t + k * kThreads, r = idx >> 6, x = idx & 63u;
    if (y0 + r >= ph || x0 + x >= pw) continue;
    const u32 p = lab[(y0 + r) * pw + x0 + x];  // (of this tile: only this block writes it, below)
    if (p != kBg) atomicAdd(&cnt[slot_of(p, idx, x0, y0, pw)], 1u);
  }
  __syncthreads();
  for (u32 k = 0; k < kPer; ++k) {
    const u32 idx = t + k * kThreads, c = cnt[idx];
    if (!c) continue;  // (a slot that counted lies inside the plane)
    const u32 i = (y0 + (idx >> 6)) * pw + x0 + (idx & 63u);
    const u32 root = find_global(lab, i);
    __hip_atomic_fetch_add(d.area + root, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // (a shorter path for everyone; other blocks that pass here read the old parent or the root)
    if (root != i) __hip_atomic_store(lab + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(kThreads) void objects_slot_kernel(const ObjectsDesc* __restrict__ descs) {
  const ObjectsDesc& d = descs[blockIdx.y];
  u32 x0, y0;
  if (!tile_of(d, x0, y0)) return;
  const u32 pw = u32(d.pw), ph = u32(d.ph), t = threadIdx.x;
  for (u32 k = 0; k < kPer; ++k) {
    const u32 idx = t + k * kThreads, r = idx >> 6, x = idx & 63u;
    if (y0 + r >= ph || x0 + x >= pw) continue;
    const u32 i = (y0 + r) * pw + x0 + x;
    if (d.labels[i] != i) continue;
    const u32 a = d.area[i];
    u32 slot = kBg;
    if (a >= u32(d.min_area)) {
      slot = __hip_atomic_fetch_add(d.count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (slot < d.capacity) {  // (always: the components are disjoint)
        VEP_DEV u32* rec = d.records + u64(slot) * 6u;
        rec[0] = i;
        rec[1] = a;
        rec[2] = kBg;
        rec[3] = kBg;
        rec[4] = 0;
        rec[5] = 0;
      } else {
        slot = kBg;
      }
    }
    d.area[i] = slot;
  }
}

__global__ __launch_bounds__(kThreads) void objects_box_kernel(const ObjectsDesc* __restrict__ descs) {
  __shared__ u64 cols[kTile];
  __shared__ u32 rows[kTile];
  __shared__ u32 groot[kTile];
  const ObjectsDesc& d = descs[blockIdx.y];
  u32 x0, y0;
  if (!tile_of(d, x0, y0)) return;
  const u32 pw = u32(d.pw), ph = u32(d.ph), t = threadIdx.x;
  VEP_DEV u32* lab = d.labels;
  for (u32 k = 0; k < kPer; ++k) {
    cols[t + k * kThreads] = 0;
    rows[t + k * kThreads] = 0;
  }
  __syncthreads();
  u32 slots[kPer];
#pragma unroll
  for (u32 k = 0; k < kPer; ++k) {
    const u32 idx = t + k * kThreads, r = idx >> 6, x = idx & 63u;
    slots[k] = kBg;
    if (y0 + r >= ph || x0 + x >= pw) continue;
    const u32 p = lab[(y0 + r) * pw + x0 + x];
    if (p == kBg) continue;
    const u32 s = slot_of(p, idx, x0, y0, pw);
    slots[k] = s;
    atomicOr(reinterpret_cast<unsigned long long*>(&cols[s]), 1ull << x);
    atomicOr(&rows[s], 1u << r);
  }
  __syncthreads();
  for (u32 k = 0; k < kPer; ++k) {
    const u32 idx = t + k * kThreads, rw = rows[idx];
    if (!rw) continue;
    const u32 i = (y0 + (idx >> 6)) * pw + x0 + (idx & 63u);
    const u32 root = find_global(lab, i);  // (one step: the count kernel left the slots pointing at their roots)
    groot[idx] = root;
    const u32 slot = d.area[root];
    if (slot >= d.capacity) continue;  // kBackground: below min_area
    const u64 cw = cols[idx];
    VEP_DEV u32* rec = d.records + u64(slot) * 6u;
    __hip_atomic_fetch_min(rec + 2, x0 + u32(__ffsll(static_cast<long long>(cw))) - 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_min(rec + 3, y0 + u32(__ffs(int(rw))) - 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(rec + 4, x0 + 64u - u32(__clzll(static_cast<long long>(cw))), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(rec + 5, y0 + 32u - u32(__clz(int(rw))), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
#pragma unroll
  for (u32 k = 0; k < kPer; ++k) {
    if (slots[k] == kBg) continue;
    const u32 idx = t + k * kThreads;
    lab[(y0 + (idx >> 6)) * pw + x0 + (idx & 63u)] = groot[slots[k]];
  }
}

}  // namespace

void launch_objects(const ObjectsDesc* d_descs, const ObjectsDesc* h_descs, int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= 65535, "objects: at most 65535 pictures per launch");
  u64 tiles = 1;  // (at least one block a picture: it clears the count)
  for (int i = 0; i < n; ++i) tiles = std::max(tiles, u64(tiles_of(u32(h_descs[i].pw), u32(h_descs[i].ph))));
  VEP_CHECK(tiles < (u64(1) << 31), "objects: launch too large");
  const dim3 grid{u32(tiles), u32(n), 1};
  hipLaunchKernelGGL(objects_mask_kernel, grid, dim3(kThreads), 0, s, d_descs);
  hipLaunchKernelGGL(objects_seam_kernel, grid, dim3(128), 0, s, d_descs);
  hipLaunchKernelGGL(objects_count_kernel, grid, dim3(kThreads), 0, s, d_descs);
  hipLaunchKernelGGL(objects_slot_kernel, grid, dim3(kThreads), 0, s, d_descs);
  hipLaunchKernelGGL(objects_box_kernel, grid, dim3(kThreads), 0, s, d_descs);
  VEP_HIP(hipGetLastError());
}

}  // namespace vep::gpu
