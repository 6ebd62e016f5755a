// gfx950 device layer: memory, streams and the batched HIP kernels of the data plane.
//
// Kernels (gpu_kernels.hip):
//  * decode_convert — fused I_PCM macroblock reconstruction into the per-camera NV12 reference
//    surface + BT.601 NV12->BGR24 conversion into the camera's HBM ring slot. One launch per
//    worker step covers every camera of the GPU (block -> (camera, 8x2-MB tile)).
//    Replaces libavcodec reconstruction + libswscale (read_image.py:87,94).
//  * letterbox — NV12 surface -> letterboxed model input (HWC u8 and/or normalised CHW
//    fp16/bf16/fp32), batched over cameras.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "mask.h"
#include "overlay.h"
#include "scratch.h"

namespace vep::gpu {

// Device-side view of the descriptors' buffer pointers in the kernel sources (which define
// VEP_KERNEL_SOURCE): the global address space. Kernels then issue global_load / global_store
// (counted by vmcnt only) instead of flat accesses, which also count against lgkmcnt and so tie
// every LDS or scalar-load wait to outstanding global traffic. Same size and layout as the
// plain pointers the host code fills in.
#if defined(__HIP_DEVICE_COMPILE__) && defined(VEP_KERNEL_SOURCE)
#define VEP_DEV __attribute__((address_space(1)))
#else
#define VEP_DEV
#endif

#define VEP_HIP(expr)                                                                    \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess)                                                                \
      throw ::vep::Error(std::string("HIP error ") + hipGetErrorString(_e) + " at " +     \
                         __FILE__ + ":" + std::to_string(__LINE__) + ": " #expr);        \
  } while (0)

int device_count();  // 0 when no GPU / no driver
bool rocdecode_available();  // VCN backend library present (backend.cpp)

// One camera-frame of a batched decode_convert launch (lives in device memory).
struct DecodeDesc {
  VEP_DEV u8* y;              // NV12 luma plane, pitch = wmbs*16
  VEP_DEV u8* uv;             // NV12 interleaved chroma plane, pitch = wmbs*16
  VEP_DEV u8* bgr;            // output slot: out_h x out_w x 3 (packed BGR24); may be null
  // Coded-MB bitmask (bit mb of word mb/32) + exclusive per-word popcount prefix: the payload
  // slot of a coded MB is prefix[w] + popc(mask[w] & below(mb)), slots in raster order.
  // null mask = no update (pure conversion). 2 bits/MB of H2D instead of a 32-bit map.
  const VEP_DEV u32* mask;
  const VEP_DEV u32* prefix;
  const VEP_DEV u32* offsets;  // per coded MB (raster order): byte offset of its 384 samples in payload
  const VEP_DEV u8* payload;   // the slices' bytes as received (samples read in place, unaligned)
  const VEP_DEV u64* ptrs;     // direct mode (non-null): per coded MB, device address of its samples in
                       // pinned host memory — read over PCIe; offsets/payload unused
  i32 wmbs, hmbs;
  i32 out_w, out_h;
  i32 crop_left, crop_top;
  i32 tile_begin;     // exclusive prefix sum of tiles over the batch
  i32 tiles_x;
  // Speculatively placed blocks (PictureInfo::spec_lo/hi): payload slots [chk_lo, chk_hi) must
  // be preceded by the 2 header bytes chk_pat (little-endian); a mismatch sets *err (pinned
  // host memory) and the worker drops the frame.
  i32 chk_lo, chk_hi;
  u32 chk_pat;
  VEP_DEV u32* err;
};
constexpr int kTileMbW = 8, kTileMbH = 2;  // 256 threads: 32 pixel rows x 8 MB columns
inline int tiles_for(int wmbs, int hmbs) {
  return ((wmbs + kTileMbW - 1) / kTileMbW) * ((hmbs + kTileMbH - 1) / kTileMbH);
}

void launch_decode_convert(const DecodeDesc* d_descs, int n, int total_tiles, hipStream_t s);
// Single-frame variant: descriptor passed by value (op API on caller-owned buffers).
void launch_decode_convert_one(const DecodeDesc& d, hipStream_t s);

// One picture of a batched surface_to_bgr launch (device memory): a reconstructed DPB surface of
// any supported sample format -> packed BGR24, bit-exact with cpu_nv12_to_bgr (codec.h) including
// narrow_surface: samples above 8 bits are rounded to 8 in registers, 4:2:2 chroma rows are
// averaged in pairs before that. Nothing is staged: no 8-bit scratch copy, no LDS. The frame
// history path (runtime.h) converts the outputs a multi-picture job releases with it, between
// reconstruction rounds, while their surfaces are intact.
struct SurfaceBgrDesc {
  const VEP_DEV u8* y;   // luma plane: u8 samples (bit_depth 8) or u16 (9..10), 16-byte aligned
  const VEP_DEV u8* uv;  // interleaved chroma plane: coded_h / 2 rows (4:2:0) or coded_h rows (4:2:2)
  VEP_DEV u8* bgr;       // out_h x out_w x 3
  i32 pitch;             // samples per plane row (multiple of 16)
  i32 coded_w, coded_h;  // multiples of 16
  i32 bit_depth;         // 8..10
  i32 chroma_format;     // 1 = 4:2:0, 2 = 4:2:2
  i32 crop_left, crop_top;
  i32 out_w, out_h;
  i32 tile_begin;        // exclusive prefix sum of tiles over the batch
};
// (tiles of 128 x 32 samples: tiles_for(coded_w / 16, coded_h / 16))
void launch_surface_to_bgr(const SurfaceBgrDesc* d_descs, int n, int total_tiles, hipStream_t s);
void launch_surface_to_bgr_one(const SurfaceBgrDesc& d, hipStream_t s);
// Throws unless the descriptor's geometry keeps every access of the kernel inside the planes
// and the output (the launches above do not check).
void check_surface_bgr(const SurfaceBgrDesc& d);

// Gather: copy byte ranges from device-accessible (pinned, mapped) host memory into device
// memory over PCIe — one workgroup per chunk, 16-byte loads per lane. Replaces a host memcpy
// into staging + SDMA copy when the slice bytes already live in the pinned ingest pool.
struct GatherChunk {
  const VEP_DEV u8* src;  // device address of pinned host memory (any alignment)
  VEP_DEV u8* dst;        // device memory, 16-byte aligned
  u32 len;
  u32 pad;
};
constexpr u32 kGatherChunk = 32u << 10;
void launch_gather(const GatherChunk* d_chunks, int n, hipStream_t s);

// ---- general H.265 reconstruction (gpu_hevc.hip; records from hevc::Decoder, hevc_kern.h) ----
// One picture of a batched reconstruction round (device memory). DPB slot k of the camera
// lives at y + k * slot_y / uv + k * slot_uv (NV12, pitch = `stride` samples; slot sizes in
// bytes: Main10 pictures have u16 samples).
constexpr int kHevcWide = 16;
struct HevcDesc {
  VEP_DEV u8* y;
  VEP_DEV u8* uv;
  u64 slot_y, slot_uv;
  i32 stride, width, height;
  i32 log2ctb, wctb, hctb;
  i32 target;
  i32 cb_qp_offset, cr_qp_offset;
  i32 flags;             // bit 0 deblock, bit 1 SAO, bit 2 samples not loop-filtered (pcm_map),
                         // bit 3 SAO does not cross tile boundaries, bit 4 (kHevcWide) u16 samples
  i32 bd_y, bd_c;        // sample bit depths (8; Main10: up to 10, with kHevcWide)
  const VEP_DEV void* pus;       // hevc::GpuPu[npu]
  const VEP_DEV void* tus;       // hevc::GpuTu (level-sorted)
  const VEP_DEV i16* coefs;
  const VEP_DEV u8* pcm;
  const VEP_DEV u8* bs_v;
  const VEP_DEV u8* bs_h;
  const VEP_DEV signed char* qp;
  const VEP_DEV u8* pcm_map;
  const VEP_DEV u16* ctb_slice;
  const VEP_DEV void* slices;    // hevc::GpuSlice
  const VEP_DEV void* sao;       // hevc::GpuSao per CTB
  VEP_DEV u8* sao_y;             // device scratch: the deblocked picture (SAO input)
  VEP_DEV u8* sao_uv;
  const VEP_DEV void* wp;        // hevc::GpuWp (explicit weighted prediction, GpuPu::wp - 1)
  const VEP_DEV u16* ctb_tile;   // tile id per CTB
  VEP_DEV u32* err;              // the job's error word (bit 1: a dependency wait timed out)
  // Intra edge exchange (hevc_tu_queue_kernel): the camera's words, tagged with this round's
  // epoch, holding the right column / bottom row samples of every intra transform block.
  VEP_DEV u64* xg;
  i32 xg_h;              // coded height of the exchange's luma plane (width = stride)
  u32 epoch;             // tag of this round's words (never 0)
  i32 npu, pu_begin;     // exclusive prefix of PUs over the round
  i32 blk_begin;         // exclusive prefix of 4x4 blocks over the round
  // Polling backoff of a wave waiting on an edge word: it sleeps 256 cycles, then twice as long
  // after every miss, up to nap_max x 256 cycles (1: a fixed 256-cycle poll). Waves far ahead of
  // the wavefront then stop loading L2 with polls the producers' stores compete with.
  u32 nap_max;
  u32 pad_;
};
// Exchange words of a stride x h picture: luma columns (x % 4 == 3) and rows (y % 4 == 3), then
// the same for Cb and Cr. 3/4 word per luma sample.
inline size_t hevc_xg_words(int stride, int h) { return size_t(stride) * size_t(h) * 3 / 4; }
// Transform blocks tus[first .. first + count) of descs[desc], at tickets begin .. begin + count
// of their launch (intra queue: level-major, so a block's producers hold lower tickets).
struct HevcTuRange {
  i32 desc, first, count, begin;
};
// Motion compensation of every prediction block of the round (one workgroup per block).
void launch_hevc_mc(const HevcDesc* d_descs, int n, int total_pus, hipStream_t s);
// Independent transform blocks (level 0: inter residual + PCM; or the blocks of one intra level
// at tickets base .. base + count of the queue's ranges), one wave per block.
void launch_hevc_tu(const HevcDesc* d_descs, const HevcTuRange* d_ranges, int nranges, int base, int count,
                    hipStream_t s);
// Intra transform blocks at tickets base .. base + count (every intra level of the round, or a
// window of consecutive levels) in ONE launch: waves take tickets in level order from ctr[0]
// (zero at launch) — persistent waves until the queue is empty, or (windows) one ticket per wave
// — so every block a wave waits on was claimed by a running wave, whatever the dispatch order.
// A block reads the reference samples other intra blocks of the round write (GpuTu::pend) from
// their epoch-tagged edge words (HevcDesc::xg), polled until current, and publishes its own
// right column / bottom row the same way.
void launch_hevc_tu_queue(const HevcDesc* d_descs, const HevcTuRange* d_ranges, int nranges, int base, int count,
                          u32* ctr, bool persistent, hipStream_t s);
// Intra transform blocks, one workgroup per picture: d_pics[k] = {desc, first, count} names
// picture k's intra blocks tus[first .. first + count) (level-major); the workgroup's waves take
// them in order from an LDS counter, so every dependency wait stays inside one workgroup.
void launch_hevc_tu_pics(const HevcDesc* d_descs, const HevcTuRange* d_pics, int npics, hipStream_t s);
// Deblocking of every vertical (dir 0) or horizontal (dir 1) edge of the round, one thread per
// 4-line edge segment; then SAO (copy of the deblocked picture, one thread per sample).
void launch_hevc_deblock(const HevcDesc* d_descs, int n, int total_blocks, int dir, hipStream_t s);
void launch_hevc_sao(const HevcDesc* d_descs, int n, int total_blocks, hipStream_t s);
// Main10 output: u16 NV12 planes (n luma samples, n / 2 chroma) -> 8-bit NV12 (round to nearest,
// saturating), the form the BGR24 conversion and the letterbox read.
// 8-bit NV12 copy of a published slot (w x h luma): samples above 8 bits rounded to nearest
// (bd > 8: u16 planes), 4:2:2 chroma rows averaged in pairs (cf 2: an NV16 chroma plane of h rows)
// — the same result as narrow_surface (codec.h).
void launch_narrow(const void* y, const void* uv, u8* y8, u8* uv8, int w, int h, int bd, int cf, hipStream_t s);
// H.264 field pairs (frame slot in field-separated layout: top field rows, then bottom) -> the
// interleaved 8-bit NV12 frames (pitch bytes per row, `height` luma rows), one launch for the
// `n` descriptors of a batch (grid y = descriptor).
struct WeaveDesc {
  const VEP_DEV u8* y;
  const VEP_DEV u8* uv;
  VEP_DEV u8* y8;
  VEP_DEV u8* uv8;
  i32 pitch, height;
};
void launch_weave(const WeaveDesc* d_descs, int n, int max_pitch, int max_height, hipStream_t s);

// ---- general H.264 reconstruction (gpu_avc.hip; records from avc::Decoder, avc.h) ----------
// One picture of a batched reconstruction round (device memory). DPB slot k of the camera
// lives at y + k * slot_y / uv + k * slot_uv (NV12, pitch = wmbs * 16).
struct AvcDesc {
  const VEP_DEV void* mbs;     // avc::MbRec[wmbs * hmbs]
  const VEP_DEV i16* coefs;    // dequantised 4x4 blocks (16 x i16) / I_PCM samples
  const VEP_DEV i16* mvs;      // 32 x i16 per list per inter MB
  const VEP_DEV void* wps;     // avc::WpEntry pool (weighted prediction)
  VEP_DEV u8* y;
  VEP_DEV u8* uv;
  u64 slot_y, slot_uv;
  i32 wmbs, hmbs;
  i32 target;          // DPB slot reconstructed into
  i32 constrained;     // constrained_intra_pred_flag
  i32 mb_begin;        // exclusive prefix of MBs over the round (inter kernel block -> picture)
  i32 field;           // 0 frame; 1 / 2 top / bottom field picture (slots are fields, parity = slot & 1)
  VEP_DEV u32* err;            // pinned flag: wavefront timeout (frame dropped)
  VEP_DEV void* dbk;           // device scratch: AvcDbkInfo[wmbs * hmbs] (avc_bs_kernel -> deblock)
  VEP_DEV i16* res;            // device scratch: kAvcResSamples per intra MB with residual (MbRec::res
                       // slot; avc_inter_kernel -> avc_intra_kernel)
  VEP_DEV u64* prof;           // optional (VEP_AVC_PROF=1): kAvcProfSlots clock64() phase accumulators
  i32 bd;              // sample bit depth: 8 (u8 surfaces), 9 / 10 (High 10: u16 surfaces,
                       // slot_y / slot_uv in bytes; intra + deblocking in avc_hbd_kernel)
  i32 qp_bias, qpc_bias;  // MbRec::qp / qpc bias (QpBdOffsetY / C)
  i32 cf;              // chroma format: 1 (or 0: grey chroma) 4:2:0, 2 = 4:2:2 (NV16 slots; intra +
                       // deblocking in avc_hbd_kernel)
  // pool sizes (i16 coefficients, intra residual slots): the High 10 / 4:2:2 paths bound-check
  // every picture / pool access against them and report a violation in *err (bits 8..15)
  // instead of touching memory outside
  u32 ncoef, nres;
  i32 intra_mbs;       // intra MBs of the picture (avc_hbd_kernel skips its intra pass without)
  i32 deblock;         // any MB filtered (avc_hbd_kernel skips its loop-filter pass without)
  VEP_DEV u64* xg;             // device scratch: exchange between the wavefront workgroups, kAvcXgWords
                       // tagged words per MB of every workgroup's last row (intra wavefront:
                       // words 0..7, zeroed by avc_inter_kernel; deblocking: all, zeroed by
                       // avc_bs_kernel)
};
// Phase accumulators of the wavefront kernels (summed over waves): intra wait / load / luma /
// chroma / store+publish / MBs, deblock wait / load / filter / store+publish / MBs.
constexpr int kAvcProfSlots = 20;  // + [11] intra residual pass, [12..15] avc_hbd_kernel: intra
                                   // pass / loop-filter pass / barrier cycles (per workgroup),
                                   // pictures; [16..19] its loop filter per MB (wave 0): tile
                                   // load / edges / store cycles, MBs
// Residual samples of one intra MB: 256 luma (raster) + 2 x 64 chroma, as i16.
constexpr int kAvcResSamples = 512;  // slot stride: 256 luma + 2 x 64 chroma (4:2:2: 2 x 128)
// Per-MB loop-filter inputs, computed in parallel ahead of the deblocking wavefront.
struct AvcDbkInfo {
  u32 bs[4];      // 32 x 4-bit bS: nibble dir * 16 + edge * 4 + segment (0 = edge not filtered)
  u8 alpha[9], beta[9];  // [left, top, internal] for luma, Cb, Cr (component * 3 + edge kind)
  u8 tc0[9][3];   // tC0 for bS 1..3, same order
  u8 any;         // any bS != 0
  u8 pad[1];
};
static_assert(sizeof(AvcDbkInfo) == 64, "AvcDbkInfo layout");
// The deblocking wavefront runs kAvcDbkWgRows MB rows per workgroup (two per wave64), several
// workgroups per picture; a workgroup's last row hands its final bottom samples to the next
// workgroup through `xg`: 16 luma + 8 NV12 chroma u32 words per MB, each tagged (high half) with
// 2 once final (1 = columns 12..15 still to be filtered by the next MB's left edge).
constexpr int kAvcDbkWgRows = 8;
constexpr int kAvcXgWords = 24;
inline int avc_dbk_groups(int hmbs) { return (hmbs + kAvcDbkWgRows - 1) / kAvcDbkWgRows; }
inline size_t avc_xg_bytes(int wmbs, int hmbs) {
  return size_t(avc_dbk_groups(hmbs) - 1) * size_t(wmbs) * kAvcXgWords * sizeof(u64);
}
constexpr int kAvcMaxRows = 512;  // MB rows per picture the wavefront kernels support (8K)
constexpr int kAvcMaxCols = 512;  // MB columns
// Inter / skip / I_PCM macroblocks of every picture of the round (and intra MBs' residuals): one
// wave64 per MB, four per workgroup.
void launch_avc_inter(const AvcDesc* d_descs, int n, int total_mbs, hipStream_t s);
// Intra 4x4 / 16x16 macroblocks in a wavefront: avc_dbk_groups(hmbs) workgroups of
// kAvcDbkWgRows wave64s (one row each) per picture; rows synchronised through LDS counters
// inside a workgroup and tagged exchange words (AvcDesc::xg) between workgroups.
void launch_avc_intra(const AvcDesc* d_descs, int n, int max_hmbs, hipStream_t s);
// Boundary strengths + edge thresholds of every MB of the round (fully parallel), then the
// deblocking wavefront over them: avc_dbk_groups(hmbs) workgroups of kAvcDbkWgRows / 2 wave64s
// per picture, spread over the XCDs picture-wise (a picture's workgroups share one L2).
void launch_avc_bs(const AvcDesc* d_descs, int n, int total_mbs, hipStream_t s);
// packed: bit 0 vertical edges with word / half-word LDS accesses (VEP_DBK_PACKED=0: a byte per
// sample); bit 1 a wave sync after every edge instead of one per direction (VEP_DBK_SYNC=1)
void launch_avc_deblock(const AvcDesc* d_descs, int n, int max_hmbs, hipStream_t s, int packed = 1);
// High 10 pictures of the round (AvcDesc::bd > 8; the 8-bit wavefronts skip them): intra
// prediction, then (dbk: after launch_avc_bs) the loop filter. gpu_avc_hbd.hip
// variants: bit 0 High 10 4:2:0, bit 1 8-bit 4:2:2, bit 2 High 10 4:2:2 pictures present
void launch_avc_hbd(const AvcDesc* d_descs, int n, bool intra, bool dbk, int variants, hipStream_t s);

// ---- per-request scratch of the serving ops below ---------------------------------------------
// Every op keeps its scratch in a ScratchPool of sets (scratch.h states the contract: up to
// kScratch sets per pool, one per request in flight, leased for a scope). A Worker owns one pool
// per op; the ops on caller-owned tensors use one process-wide pool per device. A set is built
// from the grow-only buffers and the event below, and is used with its device bound to the
// calling thread: acquire, `reserve` room for the request, fill the host descriptors, `run`.
//
// Grow-only buffer of T, in device memory or (kPinned) in pinned host memory. It never shrinks.
template <class T, bool kPinned>
struct GrowBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  GrowBuf() = default;
  GrowBuf(const GrowBuf&) = delete;
  GrowBuf& operator=(const GrowBuf&) = delete;
  ~GrowBuf() {
    if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
  }
  // Room for n elements. Nothing happens when cap >= n; otherwise the old buffer is freed and
  // max(n, floor) elements are allocated. cap is set only after the allocation succeeded, so a
  // buffer whose growth threw is empty and grows again on the next call.
  void reserve(size_t n, size_t floor = 0) {
    if (cap >= n) return;
    if (p) VEP_HIP(kPinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
    const size_t want = std::max(n, floor);
    void* q = nullptr;
    VEP_HIP(kPinned ? hipHostMalloc(&q, want * sizeof(T), hipHostMallocDefault) : hipMalloc(&q, want * sizeof(T)));
    p = static_cast<T*>(q);
    cap = want;
  }
};
template <class T>
using DevBuf = GrowBuf<T, false>;
template <class T>
using PinBuf = GrowBuf<T, true>;

// A set's event, created on first use; waiters sleep (several server threads wait at once).
struct SetEvent {
  hipEvent_t ev = nullptr;
  SetEvent() = default;
  SetEvent(const SetEvent&) = delete;
  SetEvent& operator=(const SetEvent&) = delete;
  ~SetEvent() {
    if (ev) (void)hipEventDestroy(ev);
  }
  void ensure() {
    if (!ev) VEP_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming | hipEventBlockingSync));
  }
  operator hipEvent_t() const { return ev; }
};

// The part every batched op shares: its descriptor array on the device and in pinned host memory
// (the caller fills h_descs.p[0..n), `run` copies them up), and the event `run` records last.
constexpr size_t kDescFloor = 64;
template <class Desc>
struct DescSet {
  DevBuf<Desc> d_descs;
  PinBuf<Desc> h_descs;
  SetEvent ev;
  void reserve_descs(int n) {
    ev.ensure();
    d_descs.reserve(size_t(n), kDescFloor);
    h_descs.reserve(size_t(n), kDescFloor);
  }
  bool holds(int n) const { return size_t(n) <= d_descs.cap && size_t(n) <= h_descs.cap; }
  void upload_descs(int n, hipStream_t s) {
    VEP_HIP(hipMemcpyAsync(d_descs.p, h_descs.p, size_t(n) * sizeof(Desc), hipMemcpyHostToDevice, s));
  }
};

// ---- baseline JPEG encoder (gpu_jpeg.hip; stream format and arithmetic: jpeg.h) -------------
// One BGR24 picture -> the entropy-coded part of its JPEG stream, byte-identical with
// jpeg::encode_cpu, in four launches: transform (one workgroup per 16x16 MCU), entropy (one lane
// per restart interval, into the interval's own segment), scan (offsets of the segments in the
// joined stream) and gather (segments + RSTm markers -> `out`).
struct JpegDesc {
  const VEP_DEV u8* bgr;  // h x w x 3, packed
  i32 w, h, quality;
  i32 mcus_x, mcus;       // MCU columns, MCUs of the picture
  i32 intervals;          // restart intervals: ceil(mcus / jpeg::kRestartInterval)
  VEP_DEV i16* coefs;     // device scratch: mcus x 6 x 64 quantised zigzag coefficients
  VEP_DEV u8* seg;        // device scratch: interval i's bytes at seg + i * jpeg::kSegmentCap (the
                          // proven worst case; every store is bound-checked all the same)
  VEP_DEV u32* len;       // device scratch: bytes of every interval's segment
  VEP_DEV u32* off;       // device scratch: offset of every interval in `out`
  VEP_DEV u8* out;        // device scratch: the joined stream (no header, no EOI)
  u32 out_cap;
  // pinned words: [0] != 0: a segment overflowed, [1] bytes of the joined stream, [2] != 0: the
  // joined stream does not fit out_cap. The caller zeroes them; nothing is written outside the
  // buffers in either case.
  VEP_DEV u32* status;
};
void launch_jpeg_transform(const JpegDesc& d, hipStream_t s);
void launch_jpeg_entropy(const JpegDesc& d, hipStream_t s);
void launch_jpeg_scan(const JpegDesc& d, hipStream_t s);
void launch_jpeg_gather(const JpegDesc& d, hipStream_t s);

// Encoder scratch of one device (pool contract: above).
struct JpegSet {
  DevBuf<u8> dev;      // coefficients | segments | joined stream | lengths | offsets
  PinBuf<u32> status;  // JpegDesc::status
  PinBuf<u8> host;     // the joined stream's D2H destination
  SetEvent ev;
};
class JpegPool : public ScratchPool<JpegSet> {
 public:
  // The JPEG stream of the device picture d_bgr (h x w x 3) at `quality` 1..100, encoded on
  // stream `s` (waits for it). False when the kernels reported an overflow: the caller encodes
  // with jpeg::encode_cpu instead.
  bool encode(const u8* d_bgr, int w, int h, int quality, hipStream_t s, std::string& out);
};

// ---- area-average downscale and the camera wall (gpu_scale.hip; arithmetic: scale.h) ---------
// One tile of a batched scale launch (device memory): a packed BGR24 source resampled to
// ow x oh at (dx, dy) of a canvas, byte-identical with scale::area_cpu, and the tile's cell
// filled with scale::kBackground wherever the picture does not cover it. Tiles of one launch may
// have different source sizes.
struct ScaleDesc {
  const VEP_DEV u8* src;  // sh rows of src_pitch bytes; null: the tile draws background only
  VEP_DEV u8* dst;        // canvas origin, rows of dst_pitch bytes
  u32 src_pitch, dst_pitch;
  i32 sw, sh;
  i32 dx, dy, ow, oh;     // the picture's rectangle in the canvas
  // The cell: filled with background outside the picture, and the bound of every store of the
  // tile. A zero-size cell means no fill; the picture's own rectangle then bounds the stores.
  i32 cx, cy, cw, ch;
};
static_assert(sizeof(ScaleDesc) == 64, "ScaleDesc layout");
// Throws unless the kernel can run the descriptor without touching memory outside the source
// picture and outside a canvas of canvas_w x canvas_h (the launch below does not check).
void check_scale(const ScaleDesc& d, int canvas_w, int canvas_h);
// One launch for the n tiles: grid = (blocks of the largest tile + rows of the tallest cell) x
// tiles. h_descs is the host copy of d_descs (the grid is sized from it).
void launch_scale(const ScaleDesc* d_descs, const ScaleDesc* h_descs, int n, hipStream_t s);

// Scale scratch of one device (pool contract: above): descriptors, a canvas and a pinned buffer
// for host tiles on their way into the canvas and for D2H results, both of the exact size asked.
struct ScaleSet : DescSet<ScaleDesc> {
  DevBuf<u8> canvas;
  PinBuf<u8> upload;
  void reserve(size_t canvas_bytes, int ndescs, size_t upload_bytes);
  // Copies the first n host descriptors up, launches them on `s` and records the event (no
  // wait). A caller that enqueues more on `s` for this request records the event again after it.
  void run(int n, hipStream_t s);
};
using ScalePool = ScratchPool<ScaleSet>;

// ---- motion detection (gpu_motion.hip; arithmetic: motion.h) ----------------------------------
// One picture of a batched motion launch (device memory): a packed BGR24 source compared with
// the background plane bg_in and folded into bg_out, changed pixels counted per cell,
// byte-identical with motion::update_cpu. Pictures of one launch may differ in size and
// parameters.
struct MotionDesc {
  const VEP_DEV u8* src;      // h rows of src_pitch bytes
  const VEP_DEV u16* bg_in;   // h rows of bg_pitch samples, 16-byte aligned; null: prime
  VEP_DEV u16* bg_out;        // the same layout; padding samples are never written
  VEP_DEV u32* counts;        // motion::cells(h) x motion::cells(w), every cell written once
  u32 src_pitch;              // bytes
  u32 bg_pitch;               // samples, a multiple of 8 (motion::pitch_for)
  i32 w, h;
  i32 cell, threshold, learn_shift;
  u32 pad_;
};
static_assert(sizeof(MotionDesc) == 64, "MotionDesc layout");
// Throws unless the kernel can run the descriptor without touching memory outside a source of
// src_bytes, background planes of bg_samples u16 each and a counts array of count_cells u32
// (the launch below does not check).
void check_motion(const MotionDesc& d, size_t src_bytes, size_t bg_samples, size_t count_cells);
// One launch for the n pictures: grid = (blocks of the largest picture) x pictures. h_descs is the
// host copy of d_descs (the grid is sized from it).
void launch_motion(const MotionDesc* d_descs, const MotionDesc* h_descs, int n, hipStream_t s);
// The descriptor of one picture: the packed w x h picture at src (src_bytes long, rows of w * 3
// bytes), planes of bg_samples u16 each in rows of bg_pitch samples (bg_in null: prime) and a
// counts array of count_cells u32; checked.
MotionDesc make_motion_desc(const u8* src, size_t src_bytes, int w, int h, const u16* bg_in, u16* bg_out, u32 bg_pitch,
                            size_t bg_samples, u32* counts, size_t count_cells, int cell, int threshold,
                            int learn_shift);

// Motion scratch of one device (pool contract: above): descriptors and a counts buffer.
constexpr size_t kResultFloor = 16384;  // words: motion counts, tamper results
struct MotionSet : DescSet<MotionDesc> {
  DevBuf<u32> d_counts;  // the grids of a request, one after another
  PinBuf<u32> h_counts;  // their copy on the host
  void reserve(int ndescs, size_t count_cells);
  // Copies the first n host descriptors up, launches them on `s`, then copies the first
  // count_cells cells down into h_counts (0: the counts are the caller's own buffers) and records
  // the event (no wait).
  void run(int n, size_t count_cells, hipStream_t s);
};
using MotionPool = ScratchPool<MotionSet>;

// ---- tamper detection (gpu_tamper.hip; arithmetic: tamper.h) -----------------------------------
// One picture of a batched tamper launch (device memory): the luma histogram, the per-cell luma
// sums and the per-cell squared-gradient energy of a packed BGR24 source, byte-identical with
// tamper::stats_cpu. Pictures of one launch may differ in size and cell.
struct TamperDesc {
  const VEP_DEV u8* src;   // h rows of src_pitch bytes
  VEP_DEV u32* hist;       // 256 bins, ZERO before the launch: blocks add their partial histograms
  VEP_DEV u32* sum_y;      // tamper::cells(h) x tamper::cells(w), every cell written once
  VEP_DEV u32* energy;     // the same layout
  u32 src_pitch;           // bytes
  i32 w, h;
  i32 cell;
  u32 pad_[4];
};
static_assert(sizeof(TamperDesc) == 64, "TamperDesc layout");
// Throws unless the kernel can run the descriptor without touching memory outside a source of
// src_bytes, two grid planes of grid_cells u32 each and a histogram of 256 u32, all three 4-byte
// aligned and apart from each other (the launch below does not check).
void check_tamper(const TamperDesc& d, size_t src_bytes, size_t grid_cells);
// One launch for the n pictures: grid = (blocks of the largest picture) x pictures. h_descs is the
// host copy of d_descs (the grid is sized from it). The histograms are zeroed by the caller, on `s`.
void launch_tamper(const TamperDesc* d_descs, const TamperDesc* h_descs, int n, hipStream_t s);
// The descriptor of one picture: the packed w x h picture at src (src_bytes long, rows of w * 3
// bytes), a histogram of 256 u32 and two grid planes of grid_cells u32 each; checked.
TamperDesc make_tamper_desc(const u8* src, size_t src_bytes, int w, int h, u32* hist, u32* sum_y, u32* energy,
                            size_t grid_cells, int cell);

// Tamper scratch of one device (pool contract: above): descriptors and a results buffer. A
// request's results are the histograms of all its pictures first (zeroed by one memset), then
// each picture's two planes.
struct TamperSet : DescSet<TamperDesc> {
  DevBuf<u32> d_res;
  PinBuf<u32> h_res;  // its copy on the host
  void reserve(int ndescs, size_t res_words);
  // Copies the first n host descriptors up, zeroes the first hist_words words of d_res, launches
  // on `s`, then copies the first res_words words down into h_res and records the event (no
  // wait). hist_words = res_words = 0: the results are the caller's own buffers, with the
  // histograms zeroed on `s` already.
  void run(int n, size_t hist_words, size_t res_words, hipStream_t s);
};
using TamperPool = ScratchPool<TamperSet>;

// ---- privacy masks (gpu_mask.hip; arithmetic: mask.h) ------------------------------------------
// One mask of one picture of a batched mask launch (device memory): the pixel rect x0..x1 x y0..y1
// of a packed BGR24 picture is filled or pixelated IN PLACE, byte-identical with mask::apply_cpu.
// A launch runs the descriptors of one level (mask::levels); pictures may differ in size.
struct MaskDesc {
  VEP_DEV u8* dst;    // h rows of pitch bytes (any alignment)
  u32 pitch;          // bytes
  i32 w, h;
  i32 x0, y0, x1, y1; // mask::to_pixels: 0 <= x0 < x1 <= w, 0 <= y0 < y1 <= h
  i32 mode;           // mask::Mode
  i32 block;          // pixelate: 4..128
  u32 bgr;            // fill: b | g << 8 | r << 16
  i32 level;          // 0 .. mask::kMaxMasks - 1
  u32 pad_[3];
};
static_assert(sizeof(MaskDesc) == 64, "MaskDesc layout");
// Throws unless the kernel can run the descriptor without touching memory outside a picture of
// dst_bytes (the launch below does not check).
void check_mask(const MaskDesc& d, size_t dst_bytes);
// One launch for the descriptors of `level` among the n: grid = (workgroups of the largest such
// mask) x n; the others' workgroups exit. h_descs is the host copy of d_descs (the grid is sized
// from it). Nothing is launched when no descriptor has the level. Levels are ordered by calling
// this in ascending level on one stream.
void launch_mask(const MaskDesc* d_descs, const MaskDesc* h_descs, int n, int level, hipStream_t s);
// The descriptors of one picture's list: out[k] for mask k of m[0..n) (n <= mask::kMaxMasks) on
// the packed w x h picture at dst, dst_bytes long; pixel rects and levels from mask.h, each
// descriptor checked. Returns the number of levels.
int fill_mask_descs(MaskDesc* out, u8* dst, size_t dst_bytes, int w, int h, const mask::Mask* m, int n);

// Mask descriptors of one device (pool contract: above).
struct MaskSet : DescSet<MaskDesc> {
  void reserve(int ndescs) { reserve_descs(ndescs); }
  // Copies the first n host descriptors up, launches their levels in ascending order on `s` and
  // records the event (no wait).
  void run(int n, hipStream_t s);
};
using MaskPool = ScratchPool<MaskSet>;

// ---- crops (gpu_crop.hip; arithmetic: crop.h) --------------------------------------------------
// One box of one picture of a batched crop launch (device memory): the pixel rect x0..x1 x y0..y1
// of a packed BGR24 picture resampled (reduced, enlarged or both, crop.h) into the rectangle
// fw x fh at (fx, fy) of its own packed ow x oh output, every other pixel of the output the pad
// colour; byte-identical with crop::apply_cpu. Pictures, rects and fitted rectangles of one launch
// may all differ; the outputs of one launch must not overlap.
struct CropDesc {
  const VEP_DEV u8* src;  // ph rows of src_pitch bytes (any alignment)
  VEP_DEV u8* dst;        // this crop's own output: oh rows of ow * 3 bytes, packed (any alignment)
  u32 src_pitch;          // bytes
  i32 pw, ph;             // the picture
  i32 x0, y0, x1, y1;     // crop::to_pixels: 0 <= x0 < x1 <= pw, 0 <= y0 < y1 <= ph
  u16 ow, oh;             // 1 .. crop::kMaxOut
  u16 fx, fy, fw, fh;     // crop::fitted: the picture's rectangle in the output
  u32 pad_bgr;            // b | g << 8 | r << 16
  u32 pad_;
};
static_assert(sizeof(CropDesc) == 64, "CropDesc layout");
// Throws unless the kernel can run the descriptor without reading outside a picture of src_bytes
// and without writing outside the crop's own oh * ow * 3 bytes, of which dst_bytes are there (the
// launch below does not check).
void check_crop(const CropDesc& d, size_t src_bytes, size_t dst_bytes);
// One launch for the n crops: grid = (tiles of the largest fitted rectangle + rows of the tallest
// padded output) x crops. h_descs is the host copy of d_descs (the grid is sized from it).
void launch_crop(const CropDesc* d_descs, const CropDesc* h_descs, int n, hipStream_t s);
// The descriptor of one box: the w x h picture at src (src_bytes long, rows of w * 3 bytes) into
// the ow x oh output at dst (dst_bytes long); pixel rect and fitted rectangle from crop.h, checked.
CropDesc make_crop_desc(const u8* src, size_t src_bytes, int w, int h, const mask::Rect& rect, u8* dst,
                        size_t dst_bytes, int ow, int oh, int fit, u32 pad_bgr);

// Crop scratch of one device (pool contract: above): descriptors, the outputs of a request one
// after the other, and their copy on the host.
struct CropSet : DescSet<CropDesc> {
  DevBuf<u8> out;
  PinBuf<u8> host;
  void reserve(int ndescs, size_t out_bytes, size_t host_bytes);
  // Copies the first n host descriptors up, launches them on `s`, then copies the first
  // down_bytes of `out` into `host` (0: nothing comes down) and records the event (no wait).
  void run(int n, size_t down_bytes, hipStream_t s);
};
using CropPool = ScratchPool<CropSet>;

// ---- on-screen display (gpu_overlay.hip; arithmetic: overlay.h) --------------------------------
// One picture of a batched overlay launch (device memory): the packed BGR24 picture at src with
// its primitives drawn on, written to dst, byte-identical with overlay::apply_cpu. dst == src (and
// equal pitches): in place; otherwise copy and draw, and the two must not overlap. Pictures of one
// launch may differ in size; their destinations must not overlap.
struct OverlayDesc {
  const VEP_DEV u8* src;    // h rows of src_pitch bytes (any alignment)
  VEP_DEV u8* dst;          // h rows of dst_pitch bytes (any alignment)
  const VEP_DEV overlay::Prim* prims;  // the picture's nprims primitives, 16-byte aligned
  const VEP_DEV u8* text;   // the picture's text pool, text_len bytes of 0x20..0x7E
  u32 src_pitch, dst_pitch;  // bytes
  i32 w, h;
  u32 nprims;               // 0 .. overlay::kMaxPrims
  u32 text_len;             // 0 .. overlay::kMaxPool
  u32 pad_[2];
};
static_assert(sizeof(OverlayDesc) == 64, "OverlayDesc layout");
// Throws unless the kernel can run the descriptor without reading outside a source of src_bytes
// and without writing outside a destination of dst_bytes, with every primitive inside the picture
// and every text inside the pool (h_prims / h_text: the host copies of prims / text). The launch
// below does not check.
void check_overlay(const OverlayDesc& d, size_t src_bytes, size_t dst_bytes, const overlay::Prim* h_prims,
                   const u8* h_text);
// One launch for the n pictures: grid = (tiles of the largest picture) x pictures. h_descs is the
// host copy of d_descs (the grid is sized from it).
void launch_overlay(const OverlayDesc* d_descs, const OverlayDesc* h_descs, int n, hipStream_t s);

// Overlay scratch of one device (pool contract: above): descriptors, the primitives and the text
// pools of a request's pictures one after the other (device and pinned), and a picture buffer for
// the out-of-place copy of a frame.
struct OverlaySet : DescSet<OverlayDesc> {
  DevBuf<overlay::Prim> d_prims;
  PinBuf<overlay::Prim> h_prims;
  DevBuf<u8> d_text;
  PinBuf<u8> h_text;
  DevBuf<u8> picture;
  void reserve(int ndescs, size_t nprims, size_t text_bytes, size_t picture_bytes);
  // Descriptor k of the request: the picture at src drawn to dst with e's primitives, which are
  // appended to the set's host arrays at prim_at / text_at (both advanced). Checked.
  void put(int k, const u8* src, size_t src_bytes, u32 src_pitch, u8* dst, size_t dst_bytes, u32 dst_pitch, int w, int h,
           const overlay::Expanded& e, size_t& prim_at, size_t& text_at);
  // Copies the first n host descriptors, nprims primitives and text_bytes of text up, launches on
  // `s` and records the event (no wait).
  void run(int n, size_t nprims, size_t text_bytes, hipStream_t s);
};
using OverlayPool = ScratchPool<OverlaySet>;

enum ChwDtype : int { kChwNone = 0, kChwF16 = 1, kChwBF16 = 2, kChwF32 = 3 };

struct LetterboxDesc {
  const VEP_DEV u8* y;
  const VEP_DEV u8* uv;
  i32 pitch;
  i32 src_w, src_h, crop_left, crop_top;
  VEP_DEV u8* out_hwc;      // S*S*3 BGR u8, or null
  VEP_DEV void* out_chw;    // 3*S*S RGB normalised, or null
  i32 nw, nh, pad_x, pad_y;
  float rx, ry;     // src/dst scale per axis
};
enum LetterboxFormat : int {
  kLbBGR = 0,   // out_hwc = S*S*3 packed BGR (+ optional normalised CHW)
  kLbNV12 = 1,  // out_hwc = S*S*3/2 NV12 (Y plane then interleaved UV): half the bytes on xGMI
};
struct LetterboxParams {
  i32 size;          // S
  i32 chw_dtype;     // ChwDtype
  float mean[3];     // RGB
  float inv_std[3];  // RGB
  u8 pad_value;
  i32 format = kLbBGR;
};
// even = true keeps the fitted size and padding on chroma-sample boundaries (NV12 output)
void fill_letterbox_geometry(LetterboxDesc& d, int size, bool even = false);
inline size_t letterbox_bytes(int size, int format) {
  return format == kLbNV12 ? size_t(size) * size * 3 / 2 : size_t(size) * size * 3;
}
// Consumer side: NV12 letterboxed batch [n][S*S*3/2] -> normalised RGB CHW [n][3][S][S].
void launch_nv12_to_chw(const u8* in, void* out, int n, int size, int chw_dtype,
                        const float mean[3], const float inv_std[3], hipStream_t s);
void launch_letterbox(const LetterboxDesc* d_descs, int n, const LetterboxParams& p,
                      hipStream_t s);
void launch_letterbox_one(const LetterboxDesc& d, const LetterboxParams& p, hipStream_t s);
// Throws unless the descriptor and the parameters describe a launch the kernels can run: planes
// and an output present, a positive window that starts inside the pitch, a known format and CHW
// dtype, S a positive multiple of 8 (the launches above do not check; the plane heights are the
// caller's to check, the descriptor does not carry them).
void check_letterbox(const LetterboxDesc& d, const LetterboxParams& p);

}  // namespace vep::gpu
