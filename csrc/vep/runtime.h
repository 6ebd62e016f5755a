// Data-plane runtime: per-camera HBM frame rings, lazy-decode camera state and the per-GPU
// worker that batches every camera's decode into one HIP launch.
//
// Reference parity:
//  * FrameRing replaces the Redis stream `XADD <device> MAXLEN n` / `XREAD` frame cache
//    (python/read_image.py:121, server/grpcapi/grpc_api.go:186-231).
//  * Camera's control atomics replace the Redis keys `last_access_time_<dev>`
//    {last_query, proxy_rtmp} and `is_key_frame_only_<dev>`.
//  * Camera::on_access_unit implements the lazy decode / keyframe-only / GOP catch-up rules of
//    rtsp_to_rtmp.py:94-160 and read_image.py:57-128.
#pragma once

#include <condition_variable>
#include <deque>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <thread>

#include "avc.h"
#include "codec.h"
#include "crop.h"
#include "overlay.h"
#include "hevc_dec.h"
#include "hevc_kern.h"
#include "hostplan.h"
#include "ioloop.h"
#include "gpu.h"
#include "motion.h"
#include "mask.h"
#include "tamper.h"
#include "pool.h"
#include "vcn.h"

namespace vep {

// VideoFrame metadata (proto/video_streaming.proto VideoFrame; read_image.py:99-117).
struct FrameMeta {
  i64 width = 0, height = 0;
  i64 timestamp = 0, pts = 0, dts = 0;
  i64 packet = 0, keyframe = 0;  // index in GOP, GOP counter
  bool is_keyframe = false, is_corrupt = false;
  char frame_type = '?';
  double time_base = 1.0 / 90000.0;
  i64 seq = 0;            // ring publish counter (per-client cursor, XREAD lastId analog)
  i64 decoded_us = 0;     // monotonic time the frame became readable
  i64 arrival_ms = 0;     // packet arrival wall clock
};

// Device (or host) memory owner. id < 0 selects the CPU backend.
class Device {
 public:
  explicit Device(int id);
  ~Device();
  bool gpu() const { return id_ >= 0; }
  int id() const { return id_; }
  void* alloc(size_t n);
  void free(void* p);
  void* alloc_pinned(size_t n);
  void free_pinned(void* p);
  void bind() const;  // hipSetDevice on the calling thread

 private:
  int id_;
};

// Ring of N decoded BGR24 frames for one camera, seqlock-published.
class FrameRing {
 public:
  // history: the H newest committed frames stay readable (range()); 0 = only the newest one
  FrameRing(Device& dev, int slots, int width, int height, int history = 0);
  ~FrameRing();
  int slots() const { return int(slots_.size()); }
  int history() const { return hist_; }
  int width() const { return w_; }
  int height() const { return h_; }
  size_t slot_bytes() const { return size_t(w_) * h_ * 3; }
  u8* slot_ptr(int i) const { return base_ + size_t(i) * slot_bytes(); }
  // writer side (single writer: the worker thread)
  // With a history, begin_write never returns one of the H newest committed slots; try_write is
  // the same for a frame that may be given up: -1 when no slot is free.
  int begin_write();
  int try_write();
  void commit(int slot, FrameMeta meta);
  // Release a slot from begin_write() without publishing (frame dropped after a failed check).
  void abort(int slot);
  // Every committed frame stops being readable (the camera's privacy masks changed): latest, range
  // and still_valid fail for them, so a reader in the middle of a copy retries or gets nothing.
  // published() keeps counting; slots being written are left to their writer.
  void invalidate();
  // reader side: newest committed frame with seq > after (false if none)
  bool latest(i64 after, FrameMeta* meta, int* slot) const;
  // The newest max_count committed frames with seq > after_seq (XRANGE / XREVRANGE analog):
  // ascending, contiguous in seq and ending at the newest frame. Returns how many.
  int range(i64 after_seq, int max_count, std::vector<std::pair<FrameMeta, int>>& out) const;
  // true if `slot` still holds the frame with publish counter `seq`
  bool still_valid(int slot, i64 seq) const;
  i64 published() const { return published_.load(std::memory_order_acquire); }
  // Block until a frame with seq > after is published (XREAD ... BLOCK analog).
  bool wait_newer(i64 after, int timeout_ms) const;

 private:
  mutable std::condition_variable cv_;
  struct Slot {
    std::atomic<u64> version{0};  // odd while being written
    FrameMeta meta;
  };
  Device& dev_;
  int w_, h_;
  u8* base_ = nullptr;
  std::vector<std::unique_ptr<Slot>> slots_;
  mutable std::mutex meta_mu_;
  std::atomic<int> latest_{-1};
  std::atomic<i64> published_{0};
  int next_ = 0;
  int hist_ = 0;
  int pick_free() const;  // history rule (meta_mu_ held): -1 when none
};

// What read_motion answers about one frame (motion.h has the arithmetic).
struct MotionResult {
  i64 seq = 0;                 // the frame evaluated
  int width = 0, height = 0;
  int cell = 0, cols = 0, rows = 0, threshold = 0;
  bool primed = false;         // false: the frame only initialised the background
  motion::Summary summary;
  std::vector<u32> counts;     // rows x cols
};

// A camera's motion state: the background model (two planes, ping-pong) and the last answer.
// Allocated on the first evaluation, freed with the camera and by Worker::motion_reset.
struct MotionState {
  std::mutex mu;               // one evaluation of the camera at a time
  u16* bg[2] = {nullptr, nullptr};  // device (CPU backend: host) planes of `samples` u16 each
  size_t samples = 0;
  int w = 0, h = 0;            // the picture size the planes hold
  int cur = 0;                 // bg[cur] is the model
  bool have_bg = false;
  bool removed = false;        // the camera left its worker: nothing is allocated any more
  u64 gen = 0;                 // Worker::set_motion_params generation the model was built under
  std::weak_ptr<FrameRing> ring;  // the ring `seq` counts in (a resolution change starts a new one)
  i64 seq = 0;                 // the frame last evaluated, 0: none
  MotionResult result;         // its answer
};

// What read_tamper answers about one frame (tamper.h has the arithmetic).
struct TamperResult {
  i64 seq = 0;                 // the frame evaluated
  int width = 0, height = 0;
  int cell = 0, cols = 0, rows = 0;
  tamper::Summary summary;
  std::vector<u32> hist;       // 256
  std::vector<u32> sum_y, energy;  // rows x cols each
};

// A camera's tamper state: the last answer and the optional reference grid (host memory, not
// persisted). Nothing lives on the device.
struct TamperState {
  std::mutex mu;               // one evaluation of the camera at a time
  u64 gen = 0;                 // Worker::set_tamper_params generation the answer was built under
  std::weak_ptr<FrameRing> ring;  // the ring `seq` counts in (a resolution change starts a new one)
  i64 seq = 0;                 // the frame last evaluated, 0: none
  TamperResult result;         // its answer
  bool have_ref = false;
  tamper::Reference ref;       // the grid of the frame an operator declared normal
};

// One picture that left the reorder buffer during a job (frame history, Camera::history): a
// job of several pictures publishes each of them, not only the newest.
struct JobOutput {
  int slot = -1;          // DPB slot
  bool fields = false;    // H.264 field pair (avc::OutFrame::fields)
  PictureInfo pic;
  FrameMeta meta;
  // Index of the job's picture (DecodeJob::avc / ::hevc) whose decoding released it: its surface
  // is intact until the NEXT picture reconstructs, so it is converted right after this one's
  // reconstruction round.
  int released_by = 0;
  i64 rasl_of = -1;       // H.265: a RASL picture of the CRA with this tag
  int ring_slot = -1;     // worker (prepare): the ring slot it is converted into, -1 = skipped
};

struct DecodeJob {
  int cam = -1;
  MbUpdate upd;                        // PCM / skip fast path (collapsible)
  std::vector<avc::PicturePtr> avc;    // general H.264 path: pictures in decoding order
  std::vector<hevc::GpuPicturePtr> hevc;  // general H.265 path: reconstruction records
  int hevc_slots = 0;                  // DPB surfaces the H.265 pictures use
  PictureInfo pic;                     // the published frame's picture (sizes of the surfaces)
  FrameMeta meta;
  bool refresh = false;  // IDR: every MB is covered
  bool keyframe_only = false;  // from a keyframe-only camera (one picture per GOP)

  // General path: DPB slot of the newest picture that left the reorder buffer in this job (it is
  // converted and published), -1 when every picture of the job is still waiting for output
  // (B-frame reordering): the job then only reconstructs.
  int out_slot = -1;
  bool out_fields = false;  // H.264 field pair: out_slot holds two fields (avc::OutFrame::fields)
  // (slot, pts) of the pictures a keyframe's job dropped from the backlog it replaced
  // (merge_job): the reorder buffer may still output them from later jobs; they are not published
  std::vector<std::pair<int, i64>> dropped;
  // H.265: decode tags of CRA pictures such a job restarted from. Their RASL pictures predict from
  // pictures before the CRA, possibly dropped ones: they are not published either.
  std::vector<i64> poisoned_cra;
  i64 out_rasl_of = -1;  // H.265: the output picture is a RASL picture of the CRA with this tag
  // Cameras with a frame history: every output of the job in output order (the last one is the
  // out_slot / pic / meta picture above, which keeps its end-of-batch conversion). Empty for
  // cameras without a history, fast-path and VCN jobs.
  std::vector<JobOutput> outputs;
  // the outputs converted by the history path: all but the newest (which out_slot describes)
  size_t history_outputs() const { return outputs.size() - (out_slot >= 0 && !outputs.empty() ? 1 : 0); }
  // VCN backend (vcn.h): a picture decoded by the video core; the worker copies its planes into
  // the camera's surface, then converts / letterboxes / publishes it like any other frame.
  vcn::FramePtr ext;
  bool general() const { return !avc.empty() || !hevc.empty(); }
  bool has_output() const { return !general() || out_slot >= 0; }
  // (H.265: the DPB slots plus one scratch surface, the SAO input copy)
  int dpb_slots() const { return !avc.empty() ? avc.back()->dpb_slots : (!hevc.empty() ? hevc_slots + 1 : 1); }
  // bytes per sample of the camera's surfaces: 2 for Main10 pictures (u16 samples), else 1
  // (High 10 H.264 / Main10 H.265: u16 samples at the stream's bit depth)
  int bit_depth() const {
    if (!avc.empty()) return avc.back()->bd;
    if (!hevc.empty()) return std::max(hevc.back()->bd_y, hevc.back()->bd_c);
    return 8;
  }
  int bytes_per_sample() const { return bit_depth() > 8 ? 2 : 1; }
  int chroma_format() const { return !avc.empty() && avc.back()->cf == 2 ? 2 : 1; }
  int target() const { return general() ? out_slot : 0; }
};

// Fold `job` into the not-yet-launched job `p` of the same camera (GOP catch-up collapse).
void merge_job(DecodeJob& p, DecodeJob&& job);

class Worker;
struct StagePlan;  // stage_plan.h

// Bounded log ring (docker json-file analog, rtsp_process_manager.go:72-75; Info returns 100).
class LogRing {
 public:
  void add(bool err, std::string line);
  std::string dump(bool err, size_t last = 100) const;

 private:
  mutable std::mutex mu_;
  std::deque<std::string> out_, err_;
};

// Camera data-plane state (one per registered RTSP process).
class Camera {
 public:
  Camera(Worker& w, int index, std::string name, int ring_slots, int history = 0);
  // Frame history depth H: the ring keeps the H newest frames readable and a job of several
  // pictures publishes its last H outputs (0: only the newest frame, as the reference's
  // buffer.in_memory: 1).
  int history() const { return history_; }
  const std::string& name() const { return name_; }
  int index() const { return index_; }
  // WorkerOptions::backpressure: wait (bounded) until the worker took this camera's queued job
  void wait_reconstruction();

  // --- control (atomics; replaces Redis control keys) ---
  std::atomic<i64> last_query_ms{0};   // 0 = never queried ("no last_query" in the hash)
  std::atomic<bool> keyframe_only{false};
  std::atomic<bool> proxy_rtmp{false};
  std::atomic<i64> idle_cutoff_ms{10000};  // rtsp_to_rtmp.py:144-145

  // --- ingest entry point (called from the camera's network thread) ---
  // Returns true if the AU triggered a decode submission.
  bool on_access_unit(const AuPtr& au);
  // Force-decode (used by bench/tests): parse au and submit regardless of query state.
  void decode_now(const AuPtr& au);
  // Same as decode_now but hands the job back (bench driver batches jobs itself).
  bool make_job(const AuPtr& au, DecodeJob& job);

  // --- stats ---
  // decoded = frames published to the ring; pictures = pictures reconstructed (general path: a
  // picture can be reconstructed in one job and output by a later one)
  std::atomic<u64> packets{0}, decoded{0}, skipped{0}, errors{0}, bytes_in{0}, pictures{0}, shed{0};
  // outputs of multi-picture jobs the history did not take: older than its depth, no free ring
  // slot, or a job outside the multi-output path (field pairs)
  std::atomic<u64> history_skipped{0};
  // packet arrival -> frame published (ms) histogram, upper bounds kLatBucketsMs (+inf last)
  static constexpr int kLatBuckets = 12;
  static constexpr double kLatBucketsMs[kLatBuckets - 1] = {1, 2, 5, 10, 20, 35, 50, 100, 250, 500, 1000};
  std::atomic<u64> lat_hist[kLatBuckets] = {};
  std::atomic<u64> lat_sum_ms{0};
  std::atomic<i64> last_packet_ms{0};
  LogRing logs;

  // The ring is replaced on a resolution change: readers hold their own reference.
  std::shared_ptr<FrameRing> ring() const { return std::atomic_load(&ring_); }
  void set_ring(std::shared_ptr<FrameRing> r) { std::atomic_store(&ring_, std::move(r)); }
  StreamParser& parser() { return parser_; }
  // true once the stream left the I_PCM / P_Skip fast path (general H.264 / H.265 decoder in use)
  bool general_decoder() const { return full_ || hevc_full_; }
  // decoder backend serving this camera: "vcn" (rocDecode) or "native" (CPU parse + gfx950)
  const char* backend() const { return use_vcn_ ? "vcn" : "native"; }
  std::mutex& gop_mutex() { return mu_; }
  std::vector<AuPtr> gop_snapshot();   // current GOP packets (for RTMP flush / archive)

  // worker-owned GPU state
  struct Surface {
    int wmbs = 0, hmbs = 0;
    int slots = 1;                 // DPB surfaces (general H.264 path); slot k at y + k * bytes
    int bps = 1;                   // bytes per sample: 2 = u16 samples (HEVC Main10, H.264 High 10)
    int bd = 8;                    // sample bit depth
    int cf = 1;                    // chroma format: 2 = 4:2:2 (NV16: full-height chroma plane)
    u8* y = nullptr;
    u8* uv = nullptr;
    // bps 2 or 4:2:2: the 8-bit NV12 copy of the picture being published (what the BGR
    // conversion and the letterbox read; written by gpu::launch_narrow)
    u8* y8 = nullptr;
    u8* uv8 = nullptr;
    // H.265 intra edge exchange (gpu::hevc_xg_words of the coded picture) and its round epoch
    u64* hevc_xg = nullptr;
    size_t hevc_xg_words = 0;
    u32 hevc_epoch = 0;
    size_t slot_y() const { return size_t(wmbs) * 16 * hmbs * 16 * size_t(bps); }
    size_t slot_uv() const { return cf == 2 ? slot_y() : slot_y() / 2; }
    bool narrowed() const { return bps == 2 || cf == 2; }  // published through y8 / uv8
    std::vector<HostSurface> host;  // CPU backend: one per slot
    std::vector<HostSurface> fields;  // CPU backend, H.264 field pictures: one per field slot
  } surface;
  std::shared_ptr<FrameRing> ring_;  // written by the worker via set_ring(); read via ring()
  // DPB slot and pts of the newest published picture (Worker::read_surface; -1: none / a field
  // pair). Worker thread, under the worker's camera lock.
  int out_surface_slot = -1;
  i64 out_surface_pts = 0;
  int ring_slots_cfg;

 private:
  friend class Worker;
  friend bool stale_output(Camera& c, const DecodeJob& j, bool check);
  friend bool stale_picture(Camera& c, int slot, i64 pts, i64 rasl_of);
  bool build_job(DecodeJob& job, size_t from, size_t to, bool refresh);
  bool build_vcn_job(DecodeJob& job, size_t from, size_t to);
  Worker& w_;
  int index_;
  std::string name_;
  int history_ = 0;
  std::mutex mu_;
  std::vector<AuPtr> gop_;
  size_t decoded_upto_ = 0;  // gop_[0, decoded_upto_) are reconstructed on the surface
  bool broken_ = false;      // worker thread: a published frame failed its check; drop until IDR
  // Worker thread: DecodeJob::dropped / poisoned_cra of recent jobs. A dropped picture leaves the
  // reorder buffer at most once (its entry is erased when it does); entries also expire after
  // kStaleJobs of the camera's jobs, so a pts that repeats later (looped source, reconnect, wrap)
  // is not suppressed for good.
  static constexpr u64 kStaleJobs = 64;
  struct StaleOut {
    int slot;
    i64 pts;
    u64 until;
  };
  std::vector<StaleOut> stale_;
  std::vector<std::pair<i64, u64>> bad_cra_;  // (CRA tag, expiry)
  u64 jobs_seen_ = 0;
  i64 keyframes_ = 0;
  StreamParser parser_;
  avc::Decoder avc_;
  bool full_ = false;
  // General H.265 path: the CPU parses into reconstruction records (hevc_dec.h records mode);
  // the worker reconstructs them on the GPU (gpu_hevc.hip) or with the CPU mirror.
  bool hevc_full_ = false;
  hevc::Decoder hevc_;
  // VCN backend: one rocDecode session per camera, created on the first keyframe
  bool use_vcn_ = false;
  std::unique_ptr<vcn::Session> vcn_;
  u64 fault_after_ = 0;  // VEP_FAULT_CAMERA: crash on this access unit (0 = never)

 public:
  // motion detection (Worker::read_motion): frames evaluated, and those of them with motion.
  // (Last in the class: the members the ingest and publish paths touch keep their places.)
  std::atomic<u64> motion_evaluations{0}, motion_frames{0};
  MotionState motion;
  // tamper detection (Worker::read_tamper): frames evaluated, and those of them flagged. (Last,
  // after motion's members, for the same reason.)
  std::atomic<u64> tamper_evaluations{0}, tamper_frames{0};
  TamperState tamper;
  // privacy masks (Worker::set_privacy_masks; last again). The list and its generation change
  // under the worker's camera lock only; a frame converted under an older generation is never
  // committed (Worker::publish).
  std::vector<mask::Mask> masks;
  u64 mask_gen = 0;
  std::atomic<u64> masked_frames{0};  // committed frames that had at least one mask
  std::atomic<u64> mask_dropped{0};   // frames given up because the list changed while they were in flight
};

struct WorkerOptions {
  int device = 0;             // -1 = CPU backend
  int letterbox_size = 0;     // 0 = no consumer batch
  int letterbox_format = 0;   // gpu::LetterboxFormat (BGR HWC or NV12)
  int chw_dtype = 0;          // gpu::ChwDtype for the normalised CHW consumer tensor
  float mean[3] = {0.f, 0.f, 0.f};
  float std[3] = {1.f, 1.f, 1.f};
  int max_cameras = 256;
  int pack_threads = 4;       // host threads packing MB payloads into pinned staging
  bool direct_reads = true;   // decode kernel reads slice bytes from host memory (else gather)
  // Independent GPU pipelines ("lanes"): camera c always runs on lane c % lanes, each lane with
  // its own stream and staging. A keyframe's long intra wavefront then delays only its lane's
  // cameras instead of the whole tick. 0 = VEP_LANES or the default.
  int lanes = 0;
  // Batches in flight per lane (staging buffers): launch_async blocks only when its lane still
  // runs the batch from `stages` launches ago. 0 = VEP_STAGES or the default.
  int stages = 0;
  // Batches a lane's launcher thread may have queued behind its in-flight ones (several lanes):
  // how far the other lanes can run ahead of one held up by a slow batch. 0 = VEP_LANE_QUEUE or
  // the default.
  int queue = 0;
  bool lane_threads = false;  // one launcher thread per lane (also VEP_LANE_THREADS=1)
  // Decoder backend: kDecoderNative (CPU parse + gfx950 reconstruction), kDecoderVcn (rocDecode
  // on the video core; fails when librocdecode is missing) or kDecoderAuto (VCN when present).
  int decoder = 0;
  // Keyframe-only coalescing: while every pending job is a keyframe-only camera's picture, the
  // worker waits up to this long (from the first one) for more before launching, so one
  // latency-bound intra + deblocking wavefront launch serves several pictures. Such cameras
  // show one frame per GOP, so the wait is invisible to their clients. -1 = VEP_KF_WINDOW_US or
  // the default; 0 = off.
  int kf_window_us = -1;
  // CPU backend only (sanitizer runs): serve through the pinned serve-buffer pool with chunked
  // copies, as the GPU path's D2H does, so its concurrency (the pool's leases, chunk
  // hand-off) runs under ThreadSanitizer without a GPU. Also VEP_MOCK_SERVE=1.
  bool mock_serve = false;
  // CPU backend: the reference's per-frame copy chain after the BGR24 conversion
  // (read_image.py:97 `img.tobytes()` + :119 `SerializeToString()`): each published frame is
  // copied into a bytes buffer and then into a serialized VideoFrame message. Used by the bench's
  // reference-equivalent CPU run (bench.py), off otherwise.
  bool ref_copies = false;
  // Lossless ingest also waits for reconstruction: a camera's parse strand waits (up to 2 s)
  // until the worker has taken the camera's queued job before parsing its next access unit, so a
  // reconstruction-bound backend back-pressures the socket instead of parsing pictures a GOP
  // catch-up later drops (the reference decodes only what it shows). Used by the bench's
  // reference-equivalent CPU run.
  bool backpressure = false;
  // Host domain (hostplan.h): the CPUs this worker's host threads run on and its ingest pool
  // sizes. parse_threads 0 = none: the worker's threads are not pinned and its cameras share the
  // process-wide ingest services.
  HostDomain domain;
};
enum DecoderBackend : int { kDecoderNative = 0, kDecoderVcn = 1, kDecoderAuto = 2 };

class Worker {
 public:
  explicit Worker(const WorkerOptions& o);
  ~Worker();
  Device& device() { return dev_; }
  const WorkerOptions& options() const { return opt_; }
  const HostDomain& host_domain() const { return opt_.domain; }
  // Ingest services (socket loops, parse strands, fan-out) of this worker's host domain, created
  // with its first IngestSession and released with the last; the process-wide services when the
  // worker has no host domain.
  std::shared_ptr<IngestServices> ingest_services();
  // Parse strands of the live ingest services (0 when none are running).
  int ingest_parse_threads();

  // history: frames kept readable for read_history (0 = only the newest, as before). The ring
  // then gets at least history_ring_slots(history) slots.
  int add_camera(const std::string& name, int ring_slots, int history = 0);
  int history_ring_slots(int history) const;
  void remove_camera(int idx);
  // Shared ownership: a reader (gRPC thread) keeps the camera alive across remove_camera().
  std::shared_ptr<Camera> camera(int idx);
  std::shared_ptr<Camera> find(const std::string& name);
  int num_cameras() const;

  // Live mode: a background thread drains submitted jobs in batches.
  void start();
  void stop();
  void submit(DecodeJob&& job);  // merges with a not-yet-launched job of the same camera

  // Synchronous batched decode (bench / tests). Jobs are consumed.
  void run_batch(std::vector<DecodeJob>& jobs);
  // Asynchronous pipeline (per lane `stages()` batches in flight, one staging buffer each; with
  // one lane the H2D runs on a copy stream overlapping the previous batch's kernels).
  // launch_async returns once the batch is enqueued; its frames are published by a later
  // launch_async (when its staging buffer is reused) or by complete_all().
  void launch_async(std::vector<DecodeJob>& jobs);
  void complete_all();
  // Wait until every submitted job is published.
  void flush();

  // Serving: copy the newest frame with seq > after into dst (host). Returns false if none.
  // dst_pinned: dst is page-locked (register_host) -> one DMA straight into it, no staging.
  bool read_latest(int cam, i64 after, FrameMeta* meta, u8* dst, size_t cap);
  bool read_latest(FrameRing& ring, i64 after, FrameMeta* meta, u8* dst, size_t cap, bool dst_pinned = false);
  // The newest frame with seq > after as a JPEG stream (jpeg.h) at `quality` 1..100. On a GPU the
  // frame is encoded where it lies, in its HBM ring slot, on the serving stream, and only the
  // compressed bytes are copied; the CPU backend runs jpeg::encode_cpu on the host ring. A slot
  // the writer reused during the encode is encoded again from the newer frame, as read_latest
  // does for its copy. False if there is no such frame.
  // width / height (0 = not given): the frame is first fitted into that box (scale::fit, never
  // enlarged) and downscaled by area averaging (scale.h) into pooled device scratch, on the
  // serving stream as well. With both 0 the path and the bytes are as without them.
  bool read_latest_jpeg(int cam, i64 after, int quality, FrameMeta* meta, std::string& out, int width = 0,
                        int height = 0);
  // The same scaled picture as packed BGR24 in host memory (dst is resized to ow * oh * 3; only
  // those bytes are copied off the GPU); meta->width / height are the scaled size.
  bool read_latest_scaled(int cam, i64 after, int width, int height, FrameMeta* meta, std::vector<u8>& dst);
  // One picture of several cameras: a wall of scale::wall(n, cols, tw, th) cells, tile t showing
  // the newest frame of camera cams[t] fitted into its cell and centred, background elsewhere,
  // as a JPEG stream. One scale launch fills the canvas from the ring slots; tiles whose slot the
  // writer reused meanwhile are scaled again (up to four rounds). seqs_out[t] is the seq shown, 0
  // for a tile drawn as background: camera index < 0 or unknown, no ring, no frame, or still
  // inconsistent. foreign[t].data (non-null) is an already scaled host BGR24 tile (a camera of
  // another worker, seq as given) copied into its cell instead. Only descriptors and foreign
  // tiles go up, only compressed bytes come down.
  struct ForeignTile {
    const u8* data = nullptr;  // h rows of w * 3 bytes, w <= tw, h <= th
    int w = 0, h = 0;
    i64 seq = 0;
  };
  void read_wall_jpeg(const std::vector<int>& cams, int cols, int tw, int th, int quality,
                      const std::vector<ForeignTile>& foreign, std::vector<i64>& seqs_out, std::string& out);
  // On-screen display (overlay.h, docs/OVERLAY.md). read_latest_jpeg with `items` drawn on the
  // picture that is encoded: at native size the slot is copied and drawn into pooled scratch in
  // one launch, scaled the items are drawn in place on the scaled picture, both on the serving
  // stream with the encoder chained behind, inside the consistent read. Placeholders ({name},
  // {seq}, {time}) are replaced from the meta of the frame actually picked. The ring slot is never
  // written.
  bool read_overlay_jpeg(int cam, i64 after, int quality, const std::vector<overlay::Item>& items,
                         const std::string& name, FrameMeta* meta, std::string& out, int width = 0, int height = 0);
  // read_wall_jpeg with labels[t] (non-empty) drawn at the top-left corner of every tile that
  // shows a frame, as a text at auto scale for the tile's height over black at alpha 160, clipped
  // to the tile's cell: one in-place launch on the composed canvas. At most
  // overlay::kMaxPrims / 2 tiles may carry a label.
  void read_wall_jpeg_labelled(const std::vector<int>& cams, int cols, int tw, int th, int quality,
                               const std::vector<ForeignTile>& foreign, const std::vector<std::string>& labels,
                               std::vector<i64>& seqs_out, std::string& out);
  // Overlay requests answered and the primitives they drew, since the worker started.
  std::pair<u64, u64> overlay_counts() const { return {overlay_requests_.load(), overlay_prims_.load()}; }
  // Motion detection (motion.h, docs/MOTION.md): did the newest frame with seq > after differ from
  // the camera's background model? The frame is evaluated where it lies, in its ring slot, on the
  // serving stream (CPU backend: motion::update_cpu on the host ring), from the model plane into
  // the other one; only the counts grid comes down. The planes are swapped once the slot proved
  // unchanged (still_valid), so a torn frame never reaches the model; a reused slot is evaluated
  // again from the newer frame, up to four times. A frame is evaluated once: later calls at the
  // same seq get the stored answer. False if there is no such frame.
  bool read_motion(int cam, i64 after, MotionResult& out);
  // The newest frame of several cameras, every camera that needs an evaluation in ONE launch.
  // ok[k] is false for an unknown index, a camera without a ring or a frame, or one still
  // inconsistent after the fourth round.
  void read_motion_many(const std::vector<int>& cams, std::vector<MotionResult>& out, std::vector<char>& ok);
  // Parameters are per worker (the models depend on them): validates and resets every model.
  void set_motion_params(const motion::Params& p);
  motion::Params motion_params();
  // Frees the camera's model: its next evaluation primes again.
  void motion_reset(int cam);
  // Tamper detection (tamper.h, docs/TAMPER.md): is the newest frame with seq > after dark, bright,
  // flat, or, against the camera's reference, defocused or moved? The frame is evaluated where it
  // lies, in its ring slot, on the serving stream (CPU backend: tamper::stats_cpu on the host
  // ring); the histogram and the two grid planes come down and tamper::summarize runs on the host.
  // An answer is stored once the slot proved unchanged (still_valid); a reused slot is evaluated
  // again from the newer frame, up to four times. A frame is evaluated once: later calls at the
  // same seq get the stored answer. False if there is no such frame.
  bool read_tamper(int cam, i64 after, TamperResult& out);
  // The newest frame of several cameras, every camera that needs an evaluation in ONE launch.
  // ok[k] is false for an unknown index, a camera without a ring or a frame, or one still
  // inconsistent after the fourth round.
  void read_tamper_many(const std::vector<int>& cams, std::vector<TamperResult>& out, std::vector<char>& ok);
  // Parameters are per worker: validates, resets every stored answer and drops the references
  // whose cell changed.
  void set_tamper_params(const tamper::Params& p);
  tamper::Params tamper_params();
  // Declares the camera's newest frame normal: evaluates it if needed and stores its grid as the
  // reference (the stored answer is summarised again against it). False when there is no frame.
  bool tamper_set_reference(int cam);
  // Drops the camera's reference and its stored answer.
  void tamper_reset(int cam);
  // Privacy masks (mask.h, docs/PRIVACY.md): the camera's list, applied in its ring slot after the
  // BGR24 conversion and before the commit, so no consumer of the ring sees an unmasked pixel of a
  // masked region. set_privacy_masks throws on an invalid list; an empty list clears. A change
  // makes the camera's committed frames unreadable (FrameRing::invalidate), gives up the frames in
  // flight when they complete, and resets the camera's motion model and tamper state.
  void set_privacy_masks(int cam, const std::vector<mask::Mask>& masks);
  std::vector<mask::Mask> privacy_masks(int cam);
  // Crops (crop.h, docs/CROPS.md): the boxes of a frame, cut and resized to ow x oh where the frame
  // lies, in its ring slot, on the serving stream (CPU backend: crop::apply_cpu on the host ring);
  // only the crops come down, n packed BGR24 pictures one after the other in dst. seq == 0: the
  // newest frame with seq > after; seq > 0: that very frame (a detector's boxes belong to the
  // frame it saw), found in the camera's history, no answer once it has left the ring. A slot the
  // writer reused (or a mask change invalidated) meanwhile is read again, up to four times, and
  // what was produced from it is never returned. Crops read the ring slot, so they show the
  // camera's privacy masks. Throws on an invalid list, size, fit or pad colour.
  bool read_crops(int cam, i64 after, i64 seq, const std::vector<crop::Box>& boxes, int ow, int oh, int fit,
                  const crop::Pad& pad, FrameMeta* meta, std::vector<u8>& dst);
  // Several cameras (a camera may repeat): the crops of every request in ONE launch a round.
  struct CropRequest {
    int cam = -1;
    i64 after = 0, seq = 0;
    std::vector<crop::Box> boxes;
    bool ok = false;   // out: false for an unknown camera, no ring, no such frame, still inconsistent
    FrameMeta meta;    // out
    std::vector<u8> data;  // out: boxes.size() * oh * ow * 3 bytes
  };
  void read_crops_many(std::vector<CropRequest>& reqs, int ow, int oh, int fit, const crop::Pad& pad);
  // One crop as a JPEG stream: the encoder is chained onto the crop on the device, only the
  // compressed bytes come down.
  bool read_crop_jpeg(int cam, i64 after, i64 seq, const crop::Box& box, int ow, int oh, int fit, const crop::Pad& pad,
                      int quality, FrameMeta* meta, std::string& out);
  void set_wall_max_tiles(int n);
  int wall_max_tiles() const { return wall_max_tiles_.load(); }
  // Frame history: the newest max_count (0 = the camera's depth) frames with seq > after, copied
  // to host memory, ascending and contiguous in seq, ending at the newest frame. A frame the
  // writer reused during the read is dropped together with everything older.
  struct HistoryFrame {
    FrameMeta meta;
    std::unique_ptr<u8[]> data;
    size_t bytes = 0;
  };
  std::vector<HistoryFrame> read_history(int cam, i64 after, int max_count);
  // Several rings' newest frames at once (the frame bus pump): every copy into page-locked
  // destinations is queued on the serving stream before one wait; others go one by one.
  struct ReadReq {
    FrameRing* ring = nullptr;
    i64 after = 0;
    u8* dst = nullptr;
    size_t cap = 0;
    bool pinned = false;
    FrameMeta meta;  // out
    bool ok = false; // out
  };
  void read_latest_many(std::vector<ReadReq>& reqs);
  // Called after every frame a camera commits to its ring: (camera index, sequence). Runs on the
  // publishing thread with the camera table locked: must be cheap and must not call back in.
  void set_publish_hook(std::function<void(int, i64)> f);
  // Page-lock caller memory (e.g. a shared-memory segment another process maps) for direct
  // D2H. False on the CPU backend or when the driver refuses the range.
  bool register_host(void* p, size_t n);
  void unregister_host(void* p);

  // Consumer batch (letterbox): device pointers of [max_cameras, S, S, 3] u8 and CHW tensor.
  // Point the consumer batch at caller-owned device buffers (e.g. torch tensors that feed an
  // RCCL all-gather); row r belongs to camera index r. Takes effect from the next batch.
  void set_consumer_buffers(u8* hwc, void* chw, int rows);
  u8* consumer_hwc() const { return cons_hwc_; }
  // Consistent copy of consumer rows [0, rows) into dst (device memory on the GPU): ordered after
  // every letterbox write already enqueued on any lane and before any later one, without a host
  // wait. `stream` is the caller's (e.g. torch's current stream, so a collective enqueued next on
  // it reads whole rows: no row is half one frame, half the next); 0 = wait on the host. Reading
  // the live rows instead races the lanes' next letterbox writes. Returns the bytes copied.
  size_t snapshot_consumer(void* dst, size_t cap, int rows, hipStream_t stream);
  u64 snapshots() const { return snap_gen_.load(); }
  void* consumer_chw() const { return cons_chw_; }
  hipStream_t compute_stream() const { return stream_; }  // lane 0
  int lanes() const { return int(lanes_.size()); }
  // batches in flight per lane: a launch publishes the batch from this many launches ago
  int stages() const { return stages_; }
  // batches launch_async may have handed over but not yet published, per lane
  int inflight() const { return stages_ + (threaded_ ? queue_ : 0); }
  // Every launch_async() with work gets a sequence number (launch_seq() after it returns).
  // With several lanes each lane has its own launcher thread, so a batch's frames are published
  // asynchronously: wait_published(s) blocks until every batch with sequence <= s is published.
  u64 launch_seq() const { return launch_seq_.load(); }
  void wait_published(u64 seq);
  u64 batches() const { return batches_.load(); }
  // slice bytes the GPU read in place from pinned AU blocks vs. staged by a host memcpy
  u64 bytes_inplace() const { return pinned_bytes_inplace_.load(); }
  u64 records_gathered() const { return records_gathered_.load(); }  // record bytes the GPU pulled
  int kf_window_us() const { return kf_window_us_; }
  u64 bytes_staged() const { return pinned_bytes_staged_.load(); }
  // frames committed to camera rings (what a client can read) / frames a batch produced but the
  // worker did not publish (GPU check failure, wavefront timeout, camera waiting for a keyframe
  // after an error, camera removed)
  u64 frames() const { return frames_.load(); }
  u64 dropped() const { return dropped_.load(); }
  // outputs not published because their reconstruction was shed with a merged backlog (load
  // shedding at a keyframe, merge_job) or predicts from such a picture (RASL of a shed CRA)
  u64 shed() const { return shed_.load(); }
  u64 merged() const { return merged_.load(); }  // batches merged into an earlier one (lane launchers)
  // Lane launcher threads leave queued batches queued while held (tests: a deterministic queue
  // for merge_queued; a drain still launches them).
  void hold_lanes(bool hold);
  u64 pictures() const { return pictures_.load(); }  // pictures reconstructed
  // GPU time of the batches (first event to last, per lane; the busiest lane's total)
  double gpu_ms_total() const;
  // clock64() phase accumulators of the wavefront kernels (VEP_AVC_PROF=1; gpu::kAvcProfSlots)
  std::vector<u64> avc_profile();

 private:
  struct MaskSnap {  // a camera's privacy masks as a batch saw them
    u64 gen = 0;
    int n = 0;
    mask::Mask m[mask::kMaxMasks];
  };
  // A stage's buffer pair: a pinned half the host fills and a device half of the same size. The
  // pinned half is registered with hostmem, so the GPU can also read staged bytes in place.
  struct StagePair {
    u8* h = nullptr;
    u8* d = nullptr;
    const u8* h_dev = nullptr;  // device address of h
    size_t cap = 0;
    StagePair() = default;
    StagePair(const StagePair&) = delete;
    StagePair& operator=(const StagePair&) = delete;
    ~StagePair() { release(); }
    void reserve(size_t need);  // grow-only, to max(need + need / 2, 4 MiB)
    void release();
  };
  struct Stage {  // one pinned + device staging pair and the batch that uses it
    StagePair buf;
    hipEvent_t copied = nullptr, e0 = nullptr, e1 = nullptr;
    std::vector<DecodeJob> jobs;
    std::vector<int> slots;
    u64 seq = 0;               // launch sequence of the batch (merged batches: the first ...
    u64 seq_last = 0;          // ... to the last, consecutive in the lane's `unpublished`)
    u8* cons_hwc = nullptr;    // consumer batch at launch time (set_consumer_buffers may move on)
    void* cons_chw = nullptr;
    int cons_rows = 0;
    bool active = false;
    gpu::PinBuf<u32> err;      // per-job check flags (written by the kernels)
    u32* err_dev = nullptr;    // their device address
    // privacy masks: per job the camera's list and generation at launch; the batch's descriptors
    // (pinned + device, grown to the largest batch seen)
    std::vector<MaskSnap> mask_snap;
    gpu::PinBuf<gpu::MaskDesc> mask_h;
    gpu::DevBuf<gpu::MaskDesc> mask_d;
  };
  // What reserve / describe hand to enqueue besides the plan.
  struct Described {
    std::vector<u32> hevc_epoch;  // per StagePlan::hevc picture: its round's tag in the camera's exchange
    int tiles = 0;                // conversion tiles of the batch
    int nweave = 0, weave_pitch = 0, weave_h = 0;
    int nmask = 0, mask_levels = 0;
  };
  void loop();
  void ensure_surface(Camera& c, const PictureInfo& pi, int slots, int bd = 8, bool weave = false, int cf = 1);
  struct Batch {
    std::vector<DecodeJob> jobs;
    std::vector<int> slots;
    u64 seq = 0, seq_last = 0;
    u8* cons_hwc = nullptr;
    void* cons_chw = nullptr;
    int cons_rows = 0;
  };
  struct Lane {
    hipStream_t stream = nullptr;  // lane 0 uses Worker::stream_
    hipStream_t copy = nullptr;    // H2D of the next batch's MB data while this one decodes
    std::vector<Stage> stage;      // ring of staging buffers (Worker::stages() deep)
    int next = 0;                  // the stage reused next (the oldest in-flight batch)
    std::atomic<double> gpu_ms{0}; // cumulative batch time on this lane
    // launcher thread (several lanes): batches handed over by launch_async
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Batch> q;
    bool busy = false, drain = false, stop = false;
    std::deque<u64> unpublished;   // sequences given to this lane, not yet published (pub_mu_)
    u64 snap_seen = 0;             // consumer snapshots this lane's stream already waits for
    hipEvent_t snap_mark = nullptr;  // recorded by snapshot_consumer: the lane's enqueued work
  };
  void prepare(std::vector<DecodeJob>& jobs, std::vector<int>& slots);
  // One batch on a lane: plan, reserve, stage, describe, enqueue (runtime.cpp, in this order).
  void launch_gpu(Lane& ln, Stage& st);
  void check_plan(const StagePlan& pl, const Stage& st);
  void reserve_stage(const StagePlan& pl, Stage& st, Described& ds);
  void stage_batch(const StagePlan& pl, Stage& st);
  void describe_outputs(const StagePlan& pl, Stage& st, Described& ds);
  void describe_history(const StagePlan& pl, Stage& st);
  void describe_avc_round(const StagePlan& pl, size_t r, Stage& st);
  void describe_hevc_round(const StagePlan& pl, size_t r, Stage& st, const Described& ds);
  void describe_masks(Stage& st, Described& ds);
  void enqueue(const StagePlan& pl, Lane& ln, Stage& st, const Described& ds);
  void lane_loop(Lane& ln);
  void merge_queued(Lane& ln, Batch& b);
  void launch_on(Lane& ln, Batch&& b);  // reuse the lane's oldest stage for batch b
  void drain_lanes();
  void run_cpu(std::vector<DecodeJob>& jobs, std::vector<int>& slots, std::vector<u32>& err,
               const MaskSnap* snaps = nullptr);
  // err[i] != 0: job i failed its speculative-header check (dropped, camera waits for the
  // next keyframe)
  // snaps (one per job, or null): the masks the batch was converted under; a job whose camera's
  // list has changed since is not committed
  void publish(std::vector<DecodeJob>& jobs, std::vector<int>& slots, const u32* err = nullptr,
               const MaskSnap* snaps = nullptr);
  // The jobs' cameras' masks now (takes the camera lock). False: no camera of the batch has any.
  bool snapshot_masks(const std::vector<DecodeJob>& jobs, std::vector<MaskSnap>& out);
  void complete(Lane& ln, Stage& st);
  void complete_locked();
  void copy_slot(FrameRing& ring, int slot, u8* dst);  // one ring slot -> host memory
  void reserve_history(Camera& c, DecodeJob& j);       // ring slots of a job's earlier outputs
  WorkerOptions opt_;
  Device dev_;
  hipStream_t stream_ = nullptr, copy_stream_ = nullptr, serve_stream_ = nullptr;
  mutable std::mutex cams_mu_;
  std::vector<std::shared_ptr<Camera>> cams_;
  std::vector<std::unique_ptr<Lane>> lanes_;
  int stages_ = 2;
  bool threaded_ = false;        // one launcher thread per lane
  int queue_ = 0;                // lane queue depth (threaded)
  std::atomic<bool> hold_{false};
  int merge_jobs_ = 0;           // lane launcher: merge queued batches up to this many jobs (0: off)
  std::atomic<u64> launch_seq_{0};
  std::mutex pub_mu_;
  std::condition_variable pub_cv_;
  std::exception_ptr lane_err_;  // first error of a lane thread, rethrown to the launcher
  std::unique_ptr<ThreadPool> pack_pool_;
  // CPU backend: reconstruction + conversion of a batch's cameras in parallel (the reference runs
  // one decoder per camera container); the host domain's CPU share threads
  std::unique_ptr<ThreadPool> cpu_pool_;
  void run_cpu_job(std::vector<DecodeJob>& jobs, std::vector<int>& slots, std::vector<u32>& err, size_t i,
                   const MaskSnap* snap = nullptr);

 public:
  // host-side launch path timers (µs, cumulative): where a batch's CPU time goes (summed over
  // lane threads)
  struct Timers_ {
    double prepare = 0, index = 0, copy = 0, enqueue = 0, wait = 0;
  };
  using Timers = Timers_;
  Timers timers;

 private:
  void add_time(double Timers_::*f, double us);
  // Serving: a pool of pinned host buffers, one per in-flight read_latest(), so concurrent
  // requests DMA in parallel instead of queueing on one buffer. Each read streams the slot in
  // kServeChunks pieces: the host copy of chunk k overlaps the DMA of chunk k+1.
  static constexpr int kServeBufs = 8;
  static constexpr int kServeChunks = 4;
  struct ServeBuf {  // a set of the pool below (scratch.h), leased for one copy
    Device* dev = nullptr;  // owner of h
    u8* h = nullptr;
    size_t cap = 0;
    gpu::SetEvent ev[kServeChunks];  // one per chunk (GPU only)
    ~ServeBuf();
    void reserve(Device& d, size_t n);  // grow-only pinned room for n bytes; the events on first use
  };
  // (by pointer: ~Worker destroys the sets before the serving stream, with the device alive)
  using ServePool = ScratchPool<ServeBuf, kServeBufs>;
  std::unique_ptr<ServePool> serve_pool_ = std::make_unique<ServePool>();
  gpu::JpegPool jpeg_pool_;  // encoder scratch of read_latest_jpeg, one set per request in flight
  gpu::ScalePool scale_pool_;  // canvas + descriptors of the scaled / wall reads, likewise
  std::atomic<int> wall_max_tiles_{64};  // serving.wall_max_tiles
  // Encode a device picture on the serving stream (host encoder if the kernels report an overflow).
  void encode_device(const u8* d_bgr, int w, int h, int quality, std::string& out);
  // ring slot -> ow x oh at the origin of set's canvas, on the serving stream (no wait)
  void scale_slot(gpu::ScaleSet& set, const FrameRing& ring, int slot, int ow, int oh);
  template <class Consume>  // the scaled read of read_latest_scaled and read_latest_jpeg (serve.cpp)
  bool read_scaled(int cam, i64 after, int width, int height, bool download, FrameMeta* meta, Consume&& consume);
  u8* cons_hwc_ = nullptr;
  void* cons_chw_ = nullptr;
  // consumer snapshots: exclusive while a snapshot is enqueued, shared while a lane enqueues a
  // batch (its letterbox writes must come after the last snapshot's copy)
  std::shared_mutex cons_gate_;
  hipEvent_t snap_ev_ = nullptr;
  std::atomic<u64> snap_gen_{0};
  bool owns_cons_ = true;
  int cons_rows_ = 0;
  // live queue
  std::mutex q_mu_;
  std::condition_variable q_cv_, idle_cv_, taken_cv_;
  std::vector<DecodeJob> pending_;
  int kf_window_us_ = 0;
  // H.265 intra transform blocks: 0 = one launch per dependency level; k > 0 = one queue launch
  // per window of k consecutive levels (kAllLevels: the whole round in one launch)
  int hevc_tu_window_ = 0;
  u32 hevc_tu_nap_ = 16;  // HevcDesc::nap_max (VEP_HEVC_TU_NAP)
  // lanes wait for a stage's batch by polling its event with sleeps (VEP_SPIN_WAIT=1:
  // hipEventSynchronize, which spins a core in the HSA runtime)
  bool polite_wait_ = true;
  bool mock_serve_ = false;  // WorkerOptions::mock_serve

 public:
  u64 ref_copy_bytes() const { return ref_copy_bytes_.load(); }  // WorkerOptions::ref_copies output
  // until no queued (not yet taken) job of camera `cam` or timeout_ms passed
  void wait_camera_taken(int cam, int timeout_ms);
  // Debug / test readback of the DPB surface holding camera `cam`'s newest published picture, at
  // its full sample depth (u16 planes above 8 bits; NV16 chroma for 4:2:2) and coded size: what
  // the reconstruction wrote before the 8-bit narrowing for BGR24. False when none (or a field
  // pair). Call with the camera idle (after decode_now / flush): later jobs reuse the slot.
  bool read_surface(int cam, HostSurface& out, i64* pts);

 private:
  std::atomic<u64> ref_copy_bytes_{0};
  bool running_ = false, stop_ = false, busy_ = false;
  std::thread th_;
  std::mutex svc_mu_;
  std::weak_ptr<IngestServices> svc_;  // ingest_services()
  std::mutex launch_mu_;
  std::shared_ptr<std::function<void(int, i64)>> publish_hook_;  // (atomic_load / atomic_store)
  std::atomic<u64> batches_{0}, frames_{0}, dropped_{0}, pictures_{0}, shed_{0}, merged_{0};
  std::atomic<u64> pinned_bytes_inplace_{0}, pinned_bytes_staged_{0}, records_gathered_{0};
  std::mutex timers_mu_;
  bool direct_reads_ = false;
  u64* avc_prof_ = nullptr;
  int dbk_packed_ = 1;  // VEP_DBK_PACKED=0: the deblocking filter's byte-wise vertical edges (A/B)

 public:
  bool direct_reads() const { return direct_reads_; }
  // cameras decode through rocDecode / VCN (WorkerOptions::decoder)
  bool vcn() const { return vcn_; }

 private:
  bool vcn_ = false;
  // motion detection (last in the class, as in Camera)
  gpu::MotionPool motion_pool_;  // descriptors + counts of the motion reads, one set per request in flight
  std::mutex motion_mu_;         // motion_params_ / motion_gen_
  motion::Params motion_params_;
  u64 motion_gen_ = 1;
  struct MotionOp;  // the motion reads as an op of read_consistent_rounds (ring_read.h, serve.cpp)
  void motion_free(MotionState& st);  // (st.mu held)
  // tamper detection (after motion's members)
  gpu::TamperPool tamper_pool_;  // descriptors + results of the tamper reads, one set per request in flight
  std::mutex tamper_mu_;         // tamper_params_ / tamper_gen_
  tamper::Params tamper_params_;
  u64 tamper_gen_ = 1;
  struct TamperOp;  // likewise
  // crops (after tamper's members)
  gpu::CropPool crop_pool_;  // descriptors + outputs of the crop reads, one set per request in flight
  struct CropOp;  // likewise
  // on-screen display (after the crops' members)
  gpu::OverlayPool overlay_pool_;  // descriptors, primitives, text and a picture, one set per request in flight
  std::atomic<u64> overlay_requests_{0}, overlay_prims_{0};
  void wall_jpeg(const std::vector<int>& cams, int cols, int tw, int th, int quality,
                 const std::vector<ForeignTile>& foreign, const std::vector<std::string>* labels,
                 std::vector<i64>& seqs_out, std::string& out);
};

// Protobuf wire encoding of chrys.cloud.videostreaming.v1beta1.VideoFrame
// (field numbers from proto/video_streaming.proto). `data` bytes are supplied separately so
// the payload can be DMA'd straight into the output buffer: returns (prefix, suffix).
std::pair<std::string, std::string> encode_video_frame(const FrameMeta& m, size_t data_len,
                                                       const std::string& device_id);
// Upper bound of the suffix (fields after `data`) encode_video_frame produces for device_id.
inline size_t video_frame_suffix_max(const std::string& device_id) {
  return 7 * 11 + 2 * 2 + 3 + 9 + 48 + 12 + device_id.size();
}

}  // namespace vep
