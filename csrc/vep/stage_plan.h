// The layout of one batch in a stage's pinned + device buffer pair, decided once from the batch's
// jobs: which regions the buffer holds and where, how their bytes get there (host copy tasks,
// gather chunks), and the per-round bookkeeping of the reconstruction launches. Pure host
// arithmetic: no HIP call, no Camera. Worker::launch_gpu (runtime.cpp) reserves plan.need bytes,
// stages and describes into the regions and enqueues from the rounds.
//
// Layout, in offset order:
//   [decode | letterbox | weave | history descriptors]
//   [per job: coded-MB mask, prefix, offset or pointer table]
//   [H.264, per round: every picture's records, then the round's AvcDesc array]
//   [H.265, per round: every picture's records, then the round's HevcDesc array, TU ranges,
//    queue-window ticket counters, per-picture queues]
//   [gather chunks]                                   <- header_bytes: the H2D copy carries this
//   [per job: slice segments (staged when pageable)]  <- payload
//   [H.264, per picture: loop-filter inputs, intra residuals, deblock exchange]  <- device only
// Sizes are padded to 256 bytes, to 16 inside the index tables and the payload; the header, the
// payload and the scratch each start on a 256-byte line. An offset is therefore a multiple of
// 256 until the first index table and of 16 after it (Entry::align says which).
#pragma once

#include <vector>

#include "gpu.h"
#include "hostmem.h"
#include "runtime.h"

namespace vep {

constexpr size_t kPackChunk = size_t(1) << 20;  // bytes per host copy task

struct StagePlan {
  enum Kind : u8 {
    kBuilt,    // descriptors and tables the host writes into the pinned half
    kRecord,   // a source array: copied into the pinned half, or gathered when it lies in pinned memory
    kPayload,  // a slice segment: staged only when pageable
    kScratch,  // device only, never copied
  };
  struct Region {  // what a descriptor needs of a registered region
    size_t off = 0, bytes = 0;
  };
  struct Entry {
    Kind kind;
    size_t off, bytes;  // the data
    size_t room;        // bytes reserved (padded; 0 for an empty H.264 array)
    size_t align;       // off is a multiple of this
    const u8* src;      // record / payload: the host bytes
    const u8* dev;      // their device address when the GPU can read them in place, else null
    bool copy;          // the pack threads copy src to the pinned half at off
    bool gather;        // the gather kernel pulls dev (null: the staged copy) to the device half at off
  };
  struct CopyTask {
    const u8* src;
    size_t dst, len;  // dst: offset in the pinned half
  };
  struct Chunk {
    const u8* src;  // device address; null: the pinned half at dst (a staged segment)
    size_t dst;     // offset in the device half
    u32 len;
  };
  struct Settings {
    bool direct = true;  // decode_convert reads the slices in host memory (else: gathered first)
    int tu_window = 0;   // Worker's H.265 TU schedule (hevc_tu_window_)
  };

  struct Job {
    Region mask, prefix, table;  // coded-MB bitmask, per-word prefix, per-MB offsets (u32) or pointers (u64)
    size_t payload = 0;          // where the job's segments start (DecodeDesc::payload)
    std::vector<size_t> seg_rel;      // per segment: offset from `payload`
    std::vector<const u8*> seg_dev;   // per segment: device address in place, null = staged at payload + seg_rel
  };
  struct AvcPic {
    const avc::Picture* p;
    int job;
    Region mbs, coefs, mvs, wps;  // records
    Region dbk, res, xg;          // scratch
  };
  struct HevcPic {
    const hevc::GpuPicture* p;
    int job;
    Region pus, tus, coefs, pcm, bs_v, bs_h, qp, pcm_map, ctb_slice, slices, sao, wp, ctb_tile;
  };
  // Frame history: the outputs with a ring slot, in the order of the round that releases them;
  // one surface_to_bgr launch after each such round, before the next may reuse their surfaces.
  struct HistOut {
    int job, out;
    int tile_begin;  // exclusive prefix of tiles over its round
  };
  struct HistSpan {
    int first = 0, count = 0, tiles = 0;
  };
  struct Span {
    int first, count;  // tickets
  };
  struct AvcRound {  // round r = the r-th picture of every job that has one
    std::vector<int> pics;  // indices into avc
    Region descs;
    int mbs = 0, max_h = 0;
    bool intra = false, dbk = false, narrow = false;
    int variants = 0;  // High 10 / 4:2:2 pictures by kind (launch_avc_hbd)
    HistSpan hist;
  };
  struct HevcRound {
    std::vector<int> pics;  // indices into hevc
    Region descs, ranges, counters, picq;
    // level 0 (inter residual + PCM, independent blocks): one range per picture, one wide launch.
    // Intra levels >= 1 after them: one ticket queue for the whole round, level-major (a block's
    // producers are at lower levels, so they hold lower tickets).
    std::vector<gpu::HevcTuRange> tu_ranges;
    int l0_ranges = 0, l0_blocks = 0, intra_ranges = 0, intra_blocks = 0;
    std::vector<Span> levels;   // per intra level (tu_window == 0: one launch each)
    std::vector<Span> windows;  // tu_window > 0: consecutive levels, one queue launch and counter each
    std::vector<gpu::HevcTuRange> pic_queues;  // tu_window < 0: {desc, first intra block, blocks} per picture
    int pus = 0, blks = 0;  // prediction units, 4x4 blocks
    bool dbk = false, sao = false;
    HistSpan hist;
  };

  // Throws (VEP_CHECK) when a picture does not fit the kernels or its job.
  StagePlan(const std::vector<DecodeJob>& jobs, const Settings& s);

  Settings set;
  std::vector<Entry> entries;  // every region, in offset order
  size_t need = 0;             // bytes of the stage buffer pair
  size_t header_bytes = 0;     // the part the H2D copy carries
  Region decode, letterbox, weave, history, gather;
  std::vector<int> outs;       // jobs that publish a frame (the others only reconstruct)
  std::vector<Job> jobs;
  std::vector<AvcPic> avc;
  std::vector<HevcPic> hevc;
  std::vector<AvcRound> avc_rounds;
  std::vector<HevcRound> hevc_rounds;
  std::vector<HistOut> hist;
  std::vector<CopyTask> tasks;
  std::vector<Chunk> chunks;
  size_t planned_chunks = 0;  // what the gather region was sized for (== chunks.size())
  u64 bytes_gathered = 0, bytes_staged = 0, bytes_inplace = 0;  // records pulled; segments copied / read in place

 private:
  // `bytes` of `src` at the next offset; the reserved size is max(bytes, floor) padded to `pad`.
  // pull (records): gathered by the GPU when the array lies in pinned memory, else always copied.
  Region add(Kind kind, const void* src, size_t bytes, size_t pad = 256, size_t floor = 0, bool pull = true);
  void seal();  // the next region starts on a 256-byte line
  void plan_avc(const std::vector<DecodeJob>& jobs);
  void plan_hevc(const std::vector<DecodeJob>& jobs);
  void plan_history(const std::vector<DecodeJob>& jobs);
  void plan_transfers();
  size_t align_ = 256;
};

}  // namespace vep
