// Data-plane runtime implementation. See runtime.h.
#include "runtime.h"

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <csignal>
#include <cstdio>
#include <map>
#include <thread>

#include "color.h"
#include "stage_plan.h"
#include "trace.h"

namespace vep {

// ------------------------------------------------------------------------------------ Device

Device::Device(int id) : id_(id) {
  if (id_ >= 0) {
    int n = gpu::device_count();
    VEP_CHECK(id_ < n, "GPU " + std::to_string(id_) + " not present (" + std::to_string(n) +
                           " visible)");
    bind();
  }
}
Device::~Device() = default;

void Device::bind() const {
  if (id_ >= 0) VEP_HIP(hipSetDevice(id_));
}

void* Device::alloc(size_t n) {
  n = std::max<size_t>(n, 256);
  if (!gpu()) {
    void* p = std::aligned_alloc(256, (n + 255) & ~size_t(255));
    VEP_CHECK(p, "host alloc failed");
    return p;
  }
  void* p = nullptr;
  VEP_HIP(hipMalloc(&p, n));
  return p;
}
void Device::free(void* p) {
  if (!p) return;
  if (!gpu()) std::free(p);
  else (void)hipFree(p);
}
void* Device::alloc_pinned(size_t n) {
  n = std::max<size_t>(n, 256);
  if (!gpu()) return alloc(n);
  void* p = nullptr;
  VEP_HIP(hipHostMalloc(&p, n, hipHostMallocDefault));
  return p;
}
void Device::free_pinned(void* p) {
  if (!p) return;
  if (!gpu()) std::free(p);
  else (void)hipHostFree(p);
}

// --------------------------------------------------------------------------------- FrameRing

FrameRing::FrameRing(Device& dev, int slots, int width, int height, int history)
    : dev_(dev), w_(width), h_(height), hist_(std::max(0, history)) {
  VEP_CHECK(slots >= 1 && slots <= 4096, "ring slots out of range");
  VEP_CHECK(hist_ == 0 || slots > hist_, "ring too small for its history");
  base_ = static_cast<u8*>(dev_.alloc(slot_bytes() * size_t(slots)));
  for (int i = 0; i < slots; ++i) slots_.emplace_back(std::make_unique<Slot>());
}
FrameRing::~FrameRing() { dev_.free(base_); }

// History rule: the first slot from next_ that is neither being written nor one of the hist_
// newest committed frames (seq > published - hist_).
int FrameRing::pick_free() const {
  const int n = int(slots_.size());
  const i64 keep_above = published_.load() - hist_;
  for (int k = 0; k < n; ++k) {
    const int c = (next_ + k) % n;
    const Slot& sl = *slots_[size_t(c)];
    const u64 v = sl.version.load();
    if (v & 1) continue;
    if (v != 0 && sl.meta.seq > 0 && sl.meta.seq > keep_above) continue;  // (v 0: never written)
    return c;
  }
  return -1;
}

int FrameRing::try_write() {
  std::lock_guard<std::mutex> g(meta_mu_);
  const int s = pick_free();
  if (s < 0) return -1;
  next_ = (s + 1) % int(slots_.size());
  slots_[size_t(s)]->version.fetch_add(1, std::memory_order_acq_rel);  // odd: being written
  slots_[size_t(s)]->meta.seq = 0;  // (range() must not take it for its old frame if the write is aborted)
  return s;
}

int FrameRing::begin_write() {
  if (hist_ > 0) {  // (the ring is sized so that a slot is free: Worker::history_ring_slots)
    const int s = try_write();
    if (s >= 0) return s;
  }
  std::lock_guard<std::mutex> g(meta_mu_);
  // never overwrite the newest committed frame or a slot an in-flight batch is writing
  const int n = int(slots_.size());
  int s = next_;
  for (int k = 0; k < n; ++k) {
    const int c = (next_ + k) % n;
    if ((n == 1 || c != latest_.load()) && !(slots_[c]->version.load() & 1)) {
      s = c;
      break;
    }
  }
  next_ = (s + 1) % n;
  slots_[s]->version.fetch_add(1, std::memory_order_acq_rel);  // odd: being written
  if (hist_ > 0) slots_[s]->meta.seq = 0;
  return s;
}

int FrameRing::range(i64 after_seq, int max_count, std::vector<std::pair<FrameMeta, int>>& out) const {
  out.clear();
  if (max_count <= 0) return 0;
  std::lock_guard<std::mutex> g(meta_mu_);
  const i64 newest = published_.load();
  // seq s (newest, newest - 1, ...) lives in at most one stable slot; stop at the first gap
  for (i64 s = newest; s > std::max<i64>(after_seq, 0) && int(out.size()) < max_count; --s) {
    int hit = -1;
    for (size_t k = 0; k < slots_.size(); ++k)
      if (!(slots_[k]->version.load() & 1) && slots_[k]->meta.seq == s) hit = int(k);
    if (hit < 0) break;
    out.emplace_back(slots_[size_t(hit)]->meta, hit);
  }
  std::reverse(out.begin(), out.end());
  return int(out.size());
}

void FrameRing::commit(int slot, FrameMeta meta) {
  {
    std::lock_guard<std::mutex> g(meta_mu_);
    meta.seq = published_.load() + 1;
    slots_[slot]->meta = meta;
    slots_[slot]->version.fetch_add(1, std::memory_order_acq_rel);  // even: stable
    latest_.store(slot, std::memory_order_release);
    published_.store(meta.seq, std::memory_order_release);
  }
  cv_.notify_all();
}

void FrameRing::abort(int slot) {
  std::lock_guard<std::mutex> g(meta_mu_);
  if (slots_[slot]->version.load() & 1) slots_[slot]->version.fetch_add(1, std::memory_order_acq_rel);
}

void FrameRing::invalidate() {
  std::lock_guard<std::mutex> g(meta_mu_);
  latest_.store(-1, std::memory_order_release);
  for (auto& sl : slots_)
    if (!(sl->version.load() & 1)) sl->meta.seq = 0;  // (0: no frame; pick_free takes such a slot as free)
}

bool FrameRing::wait_newer(i64 after, int timeout_ms) const {
  std::unique_lock<std::mutex> g(meta_mu_);
  return cv_.wait_for(g, std::chrono::milliseconds(timeout_ms),
                      [&] { return published_.load() > after; });
}

bool FrameRing::latest(i64 after, FrameMeta* meta, int* slot) const {
  std::lock_guard<std::mutex> g(meta_mu_);
  int s = latest_.load();
  if (s < 0) return false;
  const Slot& sl = *slots_[s];
  if ((sl.version.load() & 1) || sl.meta.seq <= after) return false;
  *meta = sl.meta;
  *slot = s;
  return true;
}

bool FrameRing::still_valid(int slot, i64 seq) const {
  std::lock_guard<std::mutex> g(meta_mu_);
  const Slot& sl = *slots_[slot];
  return !(sl.version.load() & 1) && sl.meta.seq == seq;
}

// ----------------------------------------------------------------------------------- LogRing

void LogRing::add(bool err, std::string line) {
  std::lock_guard<std::mutex> g(mu_);
  auto& q = err ? err_ : out_;
  q.push_back(std::move(line));
  while (q.size() > 1000) q.pop_front();
}

std::string LogRing::dump(bool err, size_t last) const {
  std::lock_guard<std::mutex> g(mu_);
  const auto& q = err ? err_ : out_;
  std::string s;
  size_t start = q.size() > last ? q.size() - last : 0;
  for (size_t i = start; i < q.size(); ++i) {
    s += q[i];
    s += '\n';
  }
  return s;
}

// ------------------------------------------------------------------------------------ Camera

Camera::Camera(Worker& w, int index, std::string name, int ring_slots, int history)
    : ring_slots_cfg(ring_slots), w_(w), index_(index), name_(std::move(name)), history_(history), use_vcn_(w.vcn()) {
  // (H.265: the outputs a picture's start releases keep their surfaces until it is reconstructed)
  hevc_.set_pin_outputs(history_ > 0);
  // Fault injection (tests of per-camera-group containment): VEP_FAULT_CAMERA=<name>[:<n>] makes
  // this camera's n-th access unit (default 1) crash the process inside its parse, as a bug in
  // the bitstream parser hit by a hostile stream would.
  if (const char* f = std::getenv("VEP_FAULT_CAMERA")) {
    const std::string spec(f);
    const size_t colon = spec.rfind(':');
    const std::string who = colon == std::string::npos ? spec : spec.substr(0, colon);
    if (who == name_) fault_after_ = colon == std::string::npos ? 1 : std::max<u64>(1, std::strtoull(f + colon + 1, nullptr, 10));
  }
}

std::vector<AuPtr> Camera::gop_snapshot() {
  std::lock_guard<std::mutex> g(mu_);
  return gop_;
}

// VCN backend: the AUs go to the camera's rocDecode session; the newest picture that reached
// display order is published (older ones of a catch-up run are released at once, as the native
// path collapses them).
bool Camera::build_vcn_job(DecodeJob& job, size_t from, size_t to) {
  job.cam = index_;
  job.refresh = true;  // a complete picture: the surface is rewritten whole
  vcn::FramePtr out;
  try {
    if (!vcn_) {
      const int dev = w_.device().gpu() ? w_.device().id() : 0;
      vcn_ = std::make_unique<vcn::Session>(gop_[from]->codec, dev);
      logs.add(false, std::string("VCN decoder session opened (") + vcn::library() + ")");
    }
    const bool key_only = keyframe_only.load() && to - from == 1 && gop_[from]->keyframe;
    for (size_t i = from; i < to; ++i) {
      std::vector<vcn::FramePtr> fs = vcn_->decode(*gop_[i], i64(i));
      if (!fs.empty()) out = fs.back();
    }
    if (key_only) {  // nothing else of the GOP is decoded: drain the reorder queue
      std::vector<vcn::FramePtr> fs = vcn_->flush();
      if (!fs.empty()) out = fs.back();
    }
  } catch (const std::exception& e) {
    errors.fetch_add(1);
    logs.add(true, std::string("VCN decode failed: ") + e.what());
    decoded_upto_ = gop_.size();  // wait for the next keyframe
    if (vcn_) {
      try {
        vcn_->flush();
      } catch (const std::exception&) {
        vcn_.reset();  // a fresh session at the next keyframe
      }
    }
    return false;
  }
  decoded_upto_ = to;
  if (!out) return false;  // reordering: nothing reached display order yet
  job.ext = out;
  PictureInfo& pi = job.pic;
  pi = PictureInfo{};
  pi.width = out->width;
  pi.height = out->height;
  pi.coded_width = (out->width + 15) & ~15;
  pi.coded_height = (out->height + 15) & ~15;
  pi.pict_type = out->type;
  pi.idr = out->keyframe;
  FrameMeta& m = job.meta;
  m.width = out->width;
  m.height = out->height;
  m.pts = out->pts;
  m.dts = out->dts;
  m.timestamp = out->pts;
  m.packet = out->tag;
  m.keyframe = keyframes_;
  m.is_keyframe = out->keyframe;
  m.is_corrupt = out->corrupt;
  m.frame_type = out->type;
  m.arrival_ms = gop_[to - 1]->arrival_ms;
  return true;
}

bool Camera::build_job(DecodeJob& job, size_t from, size_t to, bool refresh) {
  job.keyframe_only = keyframe_only.load(std::memory_order_relaxed);
  if (use_vcn_) return build_vcn_job(job, from, to);
  job.cam = index_;
  job.refresh = refresh;
  const AccessUnit* last = nullptr;
  try {
    if (!full_ && !hevc_full_) {
      try {
        for (size_t i = from; i < to; ++i) {
          // single-AU jobs may take the header-free I-slice walk: the worker verifies the
          // skipped headers on the GPU (or CPU) before it publishes the frame
          job.pic = parser_.parse(*gop_[i], job.upd, to - from == 1);
          job.upd.keep.push_back(gop_[i]);  // MB samples are referenced in place
          last = gop_[i].get();
        }
      } catch (const UnsupportedStream& e) {
        if (!gop_[0]->keyframe) throw;
        // The stream uses syntax beyond the I_PCM / P_Skip fast path: switch this camera to the
        // general decoder for good and rebuild the job from the GOP's keyframe (the general
        // decoder needs the whole reference history of the GOP).
        const bool h264 = gop_[from]->codec == Codec::kH264;
        (h264 ? full_ : hevc_full_) = true;
        logs.add(false, std::string(h264 ? "general H.264" : "general H.265") + " decoder enabled (" + e.what() + ")");
        job.upd = MbUpdate{};
        from = 0;
        job.refresh = true;
      }
    }
    if (hevc_full_) {
      hevc_.set_gpu_mode(true);
      hevc::FramePtr of;
      const bool key_only = keyframe_only.load() && to - from == 1 && gop_[from]->keyframe;
      for (size_t i = from; i < to; ++i) {
        std::vector<hevc::FramePtr> outs = hevc_.decode(*gop_[i], i64(i));
        if (key_only) {  // nothing else of the GOP is decoded: take the picture out right away
          std::vector<hevc::FramePtr> rest = hevc_.flush();
          outs.insert(outs.end(), rest.begin(), rest.end());
        }
        for (auto& p : hevc_.take_gpu_pictures()) job.hevc.push_back(std::move(p));
        if (!outs.empty()) of = outs.back();
        last = gop_[i].get();
        if (history_ > 0)  // every output, with the job picture that released it
          for (const hevc::FramePtr& f : outs) {
            JobOutput o;
            o.slot = f->slot;
            o.released_by = std::max(0, int(job.hevc.size()) - 1);
            o.rasl_of = f->rasl_of;
            o.pic.width = f->width;
            o.pic.height = f->height;
            o.pic.crop_left = f->crop_left;
            o.pic.crop_top = f->crop_top;
            o.pic.pict_type = f->type;
            o.pic.idr = f->keyframe;
            FrameMeta& m = o.meta;
            m.width = f->width;
            m.height = f->height;
            m.pts = f->pts;
            m.dts = f->dts;
            m.timestamp = f->pts;
            m.packet = f->tag;
            m.keyframe = keyframes_;
            m.is_keyframe = f->keyframe;
            m.frame_type = f->type;
            m.arrival_ms = last->arrival_ms;
            job.outputs.push_back(std::move(o));
          }
      }
      decoded_upto_ = to;
      if (job.hevc.empty()) return false;
      for (const auto& p : job.hevc)  // (a size change starts a new coded video sequence)
        VEP_CHECK(p->width == job.hevc.back()->width && p->height == job.hevc.back()->height,
                  "HEVC: pictures of different sizes in one decode job");
      job.hevc_slots = hevc_.gpu_slots();
      const hevc::GpuPicture& gp = *job.hevc.back();
      PictureInfo& pi = job.pic;
      pi = PictureInfo{};
      pi.coded_width = (gp.width + 15) & ~15;  // surfaces keep the 16-aligned pitch of the convert kernels
      pi.coded_height = (gp.height + 15) & ~15;
      pi.width = of ? of->width : gp.width;
      pi.height = of ? of->height : gp.height;
      job.out_slot = of ? of->slot : -1;
      job.out_rasl_of = of ? of->rasl_of : -1;
      if (!of) return true;  // reordering: reconstruct only, nothing leaves the DPB yet
      pi.crop_left = of->crop_left;
      pi.crop_top = of->crop_top;
      pi.pict_type = of->type;
      pi.idr = of->keyframe;
      FrameMeta& m = job.meta;
      m.width = of->width;
      m.height = of->height;
      m.pts = of->pts;
      m.dts = of->dts;
      m.timestamp = of->pts;
      m.packet = of->tag;
      m.keyframe = keyframes_;
      m.is_keyframe = of->keyframe;
      m.is_corrupt = false;
      m.frame_type = of->type;
      m.arrival_ms = last->arrival_ms;
      for (JobOutput& o : job.outputs) {
        o.pic.coded_width = pi.coded_width;
        o.pic.coded_height = pi.coded_height;
      }
      if (!job.outputs.empty()) {  // (the newest one is the picture pic / meta describe)
        job.outputs.back().pic = job.pic;
        job.outputs.back().meta = job.meta;
      }
      return true;
    }
    if (full_) {
      for (size_t i = from; i < to; ++i) {
        size_t nal = 0;  // (a field pair may come as one access unit: one picture per field)
        do {
          job.avc.push_back(avc_.parse(*gop_[i], i64(i), &nal));
          if (history_ > 0)  // every output, with the job picture that released it
            for (const avc::OutFrame& f : job.avc.back()->outputs) {
              JobOutput o;
              o.slot = f.slot;
              o.fields = f.fields;
              o.released_by = int(job.avc.size()) - 1;
              o.pic = f.info;
              FrameMeta& m = o.meta;
              m.width = f.info.width;
              m.height = f.info.height;
              m.pts = f.au.pts;
              m.dts = f.au.dts;
              m.timestamp = f.au.pts;
              m.packet = f.au.tag;
              m.keyframe = keyframes_;
              m.is_keyframe = f.au.keyframe;
              m.is_corrupt = f.au.corrupt;
              m.frame_type = f.info.pict_type;
              m.arrival_ms = gop_[i]->arrival_ms;
              job.outputs.push_back(std::move(o));
            }
        } while (nal < gop_[i]->nals.size());
        last = gop_[i].get();
      }
      job.pic = job.avc.back()->info;
      // the newest picture that left the reorder buffer during this job is the one published
      const avc::OutFrame* of = nullptr;
      for (const auto& p : job.avc)
        if (!p->outputs.empty()) of = &p->outputs.back();
      job.out_slot = of ? of->slot : -1;
      job.out_fields = of && of->fields;
      if (of) {
        job.pic = of->info;
        FrameMeta& m = job.meta;
        m.width = of->info.width;
        m.height = of->info.height;
        m.pts = of->au.pts;
        m.dts = of->au.dts;
        m.timestamp = of->au.pts;
        m.packet = of->au.tag;
        m.keyframe = keyframes_;
        m.is_keyframe = of->au.keyframe;
        m.is_corrupt = of->au.corrupt;
        m.frame_type = of->info.pict_type;
        m.arrival_ms = last->arrival_ms;  // latency: from the packet that completed the output
        if (!job.outputs.empty()) job.outputs.back().meta = job.meta;
        decoded_upto_ = to;
        return true;
      }
    }
  } catch (const std::exception& e) {
    errors.fetch_add(1);
    logs.add(true, std::string("failed to decode packet: ") + e.what());
    if (full_) avc_.reset_references();
    decoded_upto_ = gop_.size();  // give up on this GOP; wait for the next keyframe
    return false;
  }
  FrameMeta& m = job.meta;
  m.width = job.pic.width;
  m.height = job.pic.height;
  m.pts = last->pts;
  m.dts = last->dts;
  m.timestamp = last->pts;  // int(frame.time * time_base.denominator) with tb = 1/90000
  m.packet = i64(to - 1);
  m.keyframe = keyframes_;
  m.is_keyframe = last->keyframe;
  m.is_corrupt = last->corrupt;
  m.frame_type = job.pic.pict_type;
  m.arrival_ms = last->arrival_ms;
  decoded_upto_ = to;
  return true;
}

bool Camera::on_access_unit(const AuPtr& au) {
  DecodeJob job;
  {
    std::lock_guard<std::mutex> g(mu_);
    const u64 np = packets.fetch_add(1, std::memory_order_relaxed) + 1;
    if (fault_after_ && np >= fault_after_) {  // (VEP_FAULT_CAMERA, see the constructor)
      std::fprintf(stderr, "vep: injected fault in camera %s's parse (access unit %llu)\n", name_.c_str(),
                   static_cast<unsigned long long>(np));
      std::fflush(stderr);
      std::raise(SIGSEGV);
    }
    bytes_in.fetch_add(au->bytes(), std::memory_order_relaxed);
    last_packet_ms.store(au->arrival_ms ? au->arrival_ms : now_ms());
    if (au->keyframe) {
      gop_.clear();
      decoded_upto_ = 0;
      ++keyframes_;
    }
    if (gop_.empty() && !au->keyframe) {  // rtsp_to_rtmp.py:111-114 "skipping, since not a keyframe"
      skipped.fetch_add(1, std::memory_order_relaxed);
      if (parser_.has_sps() == false) parser_.absorb_parameter_sets(*au);
      return false;
    }
    gop_.push_back(au);
    const i64 lq = last_query_ms.load();
    if (lq == 0) return false;                            // no last_query yet
    if (now_ms() - lq >= idle_cutoff_ms.load()) return false;  // idle > 10 s: stop decoding
    size_t to = gop_.size();
    if (keyframe_only.load()) {
      if (decoded_upto_ > 0) return false;  // keyframe already reconstructed
      to = 1;
    }
    if (decoded_upto_ >= to) return false;
    const size_t from = decoded_upto_;
    if (!build_job(job, from, to, from == 0 && gop_[0]->keyframe)) return false;
  }
  w_.submit(std::move(job));
  return true;
}

void Camera::decode_now(const AuPtr& au) {
  DecodeJob job;
  if (make_job(au, job)) w_.submit(std::move(job));
}

bool Camera::make_job(const AuPtr& au, DecodeJob& job) {
  {
    std::lock_guard<std::mutex> g(mu_);
    packets.fetch_add(1, std::memory_order_relaxed);
    bytes_in.fetch_add(au->bytes(), std::memory_order_relaxed);
    if (au->keyframe) {
      gop_.clear();
      decoded_upto_ = 0;
      ++keyframes_;
    }
    if (gop_.empty() && !au->keyframe) return false;
    gop_.push_back(au);
    size_t from = decoded_upto_, to = gop_.size();
    return build_job(job, from, to, from == 0);
  }
}

// ------------------------------------------------------------------------------------ Worker

// Lanes per GPU worker (WorkerOptions::lanes): lane streams + the serving stream fit the
// default 4 hardware queues per process.
constexpr int kDefaultLanes = 3;
// Batches in flight per lane: one slow batch (a keyframe's intra wavefront) then blocks the
// launching thread only after the other lanes have this many batches queued.
constexpr int kDefaultStages = 3;
// Batches queued per lane launcher thread behind the in-flight ones.
constexpr int kDefaultLaneQueue = 2;
constexpr int kDefaultLaneMergeJobs = 64;  // jobs per merged lane launch (lane launcher threads)
constexpr int kDefaultKfWindowUs = 16000;  // keyframe-only coalescing window (see WorkerOptions)
constexpr int kAllLevels = 1 << 20;        // (a window holding every level of a round)
// H.265 intra transform blocks: one launch per intra level (kernel boundaries order the levels;
// no wave ever polls). kAllLevels (VEP_HEVC_TU_QUEUE=1) = one persistent ticket-queue launch per
// round (waves take blocks in level order and poll their neighbours' edge words), k = windows of
// k levels, -1 = one workgroup per picture. Round 6, GPU-side ceiling of 8 x 4K H.265 (--source
// records, three alternated runs, profiles/r6/hevc_tu/): per-level 2,199 / 2,183 / 2,187
// pictures/s, GPU 91-93 ms per step; queue 2,087 / 2,068 / 2,052, 94-99 ms; per-picture 353-362.
// The queue's ~150x fewer launches do not pay for its polling (84% of its wave-cycles waiting,
// round 5 counters), so per-level launches are the default again.
constexpr int kDefaultTuWindow = 0;

Worker::Worker(const WorkerOptions& o) : opt_(o), dev_(o.device) {
  mock_serve_ = !dev_.gpu() && (opt_.mock_serve || (std::getenv("VEP_MOCK_SERVE") && std::getenv("VEP_MOCK_SERVE")[0] == '1'));
  if (opt_.decoder == kDecoderVcn)
    VEP_CHECK(vcn::available(), "decoder backend 'vcn' requested but rocDecode is unavailable: " + vcn::load_error());
  vcn_ = opt_.decoder == kDecoderVcn || (opt_.decoder == kDecoderAuto && vcn::available());
  if (dev_.gpu()) {
    dev_.bind();
    int nl = opt_.lanes;
    if (nl <= 0) {
      const char* le = std::getenv("VEP_LANES");
      nl = le ? std::atoi(le) : kDefaultLanes;
    }
    nl = std::clamp(nl, 1, 16);
    for (int g = 0; g < nl; ++g) lanes_.push_back(std::make_unique<Lane>());
    // Launcher thread per lane: opt-in (measured no steadier than the single launching thread
    // at the default 3 lanes, whose batches are bound by per-picture wavefront latency).
    const char* lt = std::getenv("VEP_LANE_THREADS");
    threaded_ = nl > 1 && (opt_.lane_threads || (lt && lt[0] == '1'));
    int nq = opt_.queue;
    if (nq <= 0) {
      const char* qe = std::getenv("VEP_LANE_QUEUE");
      nq = qe ? std::atoi(qe) : kDefaultLaneQueue;
    }
    queue_ = std::clamp(nq, 1, 16);
    // lane launchers merge queued batches (merge_queued); VEP_LANE_MERGE = job cap, 0 = off
    const char* me = std::getenv("VEP_LANE_MERGE");
    merge_jobs_ = std::clamp(me ? std::atoi(me) : kDefaultLaneMergeJobs, 0, 4096);
    int kw = opt_.kf_window_us;
    if (kw < 0) {
      const char* ke = std::getenv("VEP_KF_WINDOW_US");
      kw = ke ? std::atoi(ke) : kDefaultKfWindowUs;
    }
    kf_window_us_ = std::clamp(kw, 0, 100000);
    // H.265 intra transform blocks: one launch per level (VEP_HEVC_TU_QUEUE=0), one queue launch
    // per round (=1), or one queue launch per window of k levels (VEP_HEVC_TU_WINDOW=k)
    polite_wait_ = !(std::getenv("VEP_SPIN_WAIT") && std::getenv("VEP_SPIN_WAIT")[0] == '1');
    hevc_tu_window_ = kDefaultTuWindow;
    if (const char* tq = std::getenv("VEP_HEVC_TU_QUEUE")) hevc_tu_window_ = tq[0] == '1' ? kAllLevels : 0;
    if (const char* tw = std::getenv("VEP_HEVC_TU_WINDOW")) hevc_tu_window_ = std::clamp(std::atoi(tw), -1, kAllLevels);
    // (queue waits: longest polling nap, x 256 cycles; 1 = round 4's fixed poll)
    if (const char* tn = std::getenv("VEP_HEVC_TU_NAP")) hevc_tu_nap_ = u32(std::clamp(std::atoi(tn), 1, 256));
    int ns = opt_.stages;
    if (ns <= 0) {
      const char* se = std::getenv("VEP_STAGES");
      ns = se ? std::atoi(se) : kDefaultStages;
    }
    stages_ = std::clamp(ns, 2, 8);
    // Streams map onto the process's few hardware queues (GPU_MAX_HW_QUEUES): create only the
    // ones in use, serving first so its D2H never queues behind a lane's kernels.
    VEP_HIP(hipStreamCreateWithFlags(&serve_stream_, hipStreamNonBlocking));
    VEP_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    if (lanes_.size() == 1) {
      // The copy stream's gather kernel is PCIe-latency bound and must keep its waves resident
      // while the previous batch's decode kernel floods the CUs: give it dispatch priority.
      int prio_lo = 0, prio_hi = 0;
      VEP_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
      VEP_HIP(hipStreamCreateWithPriority(&copy_stream_, hipStreamNonBlocking, prio_hi));
    }
    for (size_t g = 0; g < lanes_.size(); ++g) {
      Lane& ln = *lanes_[g];
      if (g == 0) ln.stream = stream_;
      else VEP_HIP(hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
      // VEP_LANE_COPY=1 (several lanes): each lane gets its own copy stream, so a batch's MB
      // records / coefficients cross PCIe while the lane's previous batch is still decoding
      // (3 lanes use 7 streams, within the 8 hardware queues bench.py / the package ask for).
      // Otherwise (the default) the copy goes on the lane's own stream: measured faster on
      // 32x1080p (10.7k vs 7.5k fps/GPU, gpurun sweep), cause not yet profiled.
      const char* lc = std::getenv("VEP_LANE_COPY");
      if (lanes_.size() > 1 && lc && std::atoi(lc) == 1)
        VEP_HIP(hipStreamCreateWithFlags(&ln.copy, hipStreamNonBlocking));
      ln.stage = std::vector<Stage>(size_t(stages_));  // (a Stage owns its buffers: not movable)
      for (Stage& st : ln.stage) {
        VEP_HIP(hipEventCreateWithFlags(&st.copied, hipEventDisableTiming));
        VEP_HIP(hipEventCreate(&st.e0));
        // waiters sleep instead of spinning: several lane threads wait at once and share the
        // CPUs with the parse threads
        VEP_HIP(hipEventCreateWithFlags(&st.e1, threaded_ ? hipEventBlockingSync : hipEventDefault));
      }
    }
    hostmem::enable_pool();  // AUs finalised from here on are GPU-readable in place
    const char* ap = std::getenv("VEP_AVC_PROF");
    if (ap && ap[0] == '1') {
      avc_prof_ = static_cast<u64*>(dev_.alloc(gpu::kAvcProfSlots * sizeof(u64)));
      VEP_HIP(hipMemset(avc_prof_, 0, gpu::kAvcProfSlots * sizeof(u64)));
    }
    const char* dp = std::getenv("VEP_DBK_PACKED");
    const char* ds = std::getenv("VEP_DBK_SYNC");  // 1: a wave sync after every edge (A/B)
    const char* dg = std::getenv("VEP_DBK_REGS");  // 0: round 4's per-edge LDS lines (A/B)
    dbk_packed_ = ((dp && dp[0] == '0') ? 0 : 1) | ((ds && ds[0] == '1') ? 2 : 0) | ((dg && dg[0] == '0') ? 0 : 4);
    const char* dr = std::getenv("VEP_DIRECT_READS");
    direct_reads_ = opt_.direct_reads && !(dr && dr[0] == '0');
  }
  if (opt_.pack_threads > 0 && !threaded_) pack_pool_ = std::make_unique<ThreadPool>(opt_.pack_threads, domain_thread_init(opt_.domain, nullptr));
  if (!dev_.gpu()) {
    const int n = opt_.domain.cpu_share > 0 ? opt_.domain.cpu_share : std::max(1, int(std::thread::hardware_concurrency()) / 2);
    if (n > 1) cpu_pool_ = std::make_unique<ThreadPool>(n, domain_thread_init(opt_.domain, nullptr));
  }
  if (threaded_)
    for (auto& lp : lanes_) {
      Lane* ln = lp.get();
      ln->th = std::thread([this, ln] {
        name_thread("vep-lane");
        pin_current_thread(opt_.domain.cpus);
        lane_loop(*ln);
      });
    }
  cams_.reserve(size_t(opt_.max_cameras));
  if (opt_.letterbox_size > 0) {
    const size_t S = size_t(opt_.letterbox_size);
    (void)S;
    cons_hwc_ = static_cast<u8*>(dev_.alloc(
        size_t(opt_.max_cameras) * gpu::letterbox_bytes(opt_.letterbox_size, opt_.letterbox_format)));
    size_t es = opt_.chw_dtype == gpu::kChwF32 ? 4 : 2;
    if (opt_.chw_dtype != gpu::kChwNone)
      cons_chw_ = dev_.alloc(size_t(opt_.max_cameras) * 3 * S * S * es);
    cons_rows_ = opt_.max_cameras;
  }
}

void Worker::set_consumer_buffers(u8* hwc, void* chw, int rows) {
  std::lock_guard<std::mutex> lg(launch_mu_);
  VEP_CHECK(opt_.letterbox_size > 0, "worker was built without a letterbox consumer batch");
  if (owns_cons_) {
    if (dev_.gpu()) {
      dev_.bind();
      complete_locked();  // batches in flight still write the worker-owned buffers
    }
    dev_.free(cons_hwc_);
    dev_.free(cons_chw_);
  }
  owns_cons_ = false;
  cons_hwc_ = hwc;
  cons_chw_ = chw;
  cons_rows_ = rows;
}

Worker::~Worker() {
  stop();
  try {
    complete_all();
  } catch (...) {
  }
  std::lock_guard<std::mutex> g(cams_mu_);
  for (auto& c : cams_) {
    if (!c) continue;
    dev_.free(c->surface.y);
    dev_.free(c->surface.uv);
    dev_.free(c->surface.y8);
    dev_.free(c->surface.uv8);
    dev_.free(c->surface.hevc_xg);
    dev_.free(c->motion.bg[0]);
    dev_.free(c->motion.bg[1]);
    c->motion.bg[0] = c->motion.bg[1] = nullptr;
    c->set_ring(nullptr);
  }
  if (owns_cons_) {
    dev_.free(cons_hwc_);
    dev_.free(cons_chw_);
  }
  for (auto& lp : lanes_) {
    Lane& ln = *lp;
    {
      std::lock_guard<std::mutex> g(ln.mu);
      ln.stop = true;
    }
    ln.cv.notify_all();
    if (ln.th.joinable()) ln.th.join();
  }
  for (auto& lp : lanes_) {
    Lane& ln = *lp;
    for (Stage& st : ln.stage) {
      if (st.copied) (void)hipEventDestroy(st.copied);
      if (st.e0) (void)hipEventDestroy(st.e0);
      if (st.e1) (void)hipEventDestroy(st.e1);
    }
    ln.stage.clear();  // (their buffers go here: lanes drained, device bound, streams still alive)
    if (ln.stream && ln.stream != stream_) (void)hipStreamDestroy(ln.stream);
    if (ln.copy) (void)hipStreamDestroy(ln.copy);
    if (ln.snap_mark) (void)hipEventDestroy(ln.snap_mark);
  }
  if (snap_ev_) (void)hipEventDestroy(snap_ev_);
  serve_pool_.reset();  // (its buffers and events go here: device alive, serving stream not yet destroyed)
  dev_.free(avc_prof_);
  if (stream_) (void)hipStreamDestroy(stream_);
  if (copy_stream_) (void)hipStreamDestroy(copy_stream_);
  if (serve_stream_) (void)hipStreamDestroy(serve_stream_);
}

// Ring slots of a camera with history depth H. A batch holds up to H slots of the camera while
// it is in flight (H - 1 history outputs and the newest frame), F = inflight() (+ 1 with lane
// threads: the batch being launched) batches can be in flight when the next one reserves its
// slots, and the H newest committed frames are never written: H * (F + 2) slots, so a reservation
// always finds a free one. At 1920x1080 BGR24 (6.2 MB a slot), H = 5 and the default 3 stages
// that is 25 slots, 155 MB of HBM per camera (CPU backend, F = 0: 10 slots of host memory).
int Worker::history_ring_slots(int history) const {
  if (history <= 0) return 0;
  const int f = dev_.gpu() ? inflight() + (threaded_ ? 1 : 0) : 0;
  return history * (f + 2);
}

int Worker::add_camera(const std::string& name, int ring_slots, int history) {
  VEP_CHECK(history >= 0 && history <= 64, "camera history depth out of range (0..64)");
  ring_slots = std::max(ring_slots, history_ring_slots(history));
  std::lock_guard<std::mutex> g(cams_mu_);
  for (auto& c : cams_)
    VEP_CHECK(!c || c->name() != name, "camera already registered: " + name);
  int idx = -1;
  for (size_t i = 0; i < cams_.size(); ++i)
    if (!cams_[i]) { idx = int(i); break; }
  if (idx < 0) {
    VEP_CHECK(int(cams_.size()) < opt_.max_cameras, "worker camera capacity exhausted");
    idx = int(cams_.size());
    cams_.emplace_back();
  }
  // `stages` batches may be in flight on the GPU (+ the lane thread's queue and the batch it is
  // launching): keep one more slot so the newest committed frame stays readable meanwhile
  const int min_slots = dev_.gpu() ? inflight() + (threaded_ ? 2 : 1) : 1;
  cams_[size_t(idx)] = std::make_shared<Camera>(*this, idx, name, std::max(min_slots, ring_slots), history);
  return idx;
}

void Worker::remove_camera(int idx) {
  flush();
  complete_all();
  std::lock_guard<std::mutex> lg(launch_mu_);
  std::lock_guard<std::mutex> g(cams_mu_);
  VEP_CHECK(idx >= 0 && idx < int(cams_.size()) && cams_[size_t(idx)], "no such camera");
  auto& c = cams_[size_t(idx)];
  dev_.free(c->surface.y);
  dev_.free(c->surface.uv);
  dev_.free(c->surface.y8);
  dev_.free(c->surface.uv8);
  dev_.free(c->surface.hevc_xg);
  {
    std::lock_guard<std::mutex> mg(c->motion.mu);
    motion_free(c->motion);
    c->motion.removed = true;  // (a reader that still holds the camera allocates nothing)
  }
  c.reset();
}

std::shared_ptr<IngestServices> Worker::ingest_services() {
  std::lock_guard<std::mutex> g(svc_mu_);
  if (auto s = svc_.lock()) return s;
  auto s = opt_.domain.parse_threads > 0 ? std::make_shared<IngestServices>(opt_.domain) : IngestServices::acquire();
  svc_ = s;
  return s;
}

int Worker::ingest_parse_threads() {
  std::lock_guard<std::mutex> g(svc_mu_);
  auto s = svc_.lock();
  return s ? s->parse_threads : 0;
}

std::shared_ptr<Camera> Worker::camera(int idx) {
  std::lock_guard<std::mutex> g(cams_mu_);
  if (idx < 0 || idx >= int(cams_.size())) return nullptr;
  return cams_[size_t(idx)];
}

std::shared_ptr<Camera> Worker::find(const std::string& name) {
  std::lock_guard<std::mutex> g(cams_mu_);
  for (auto& c : cams_)
    if (c && c->name() == name) return c;
  return nullptr;
}

int Worker::num_cameras() const {
  std::lock_guard<std::mutex> g(cams_mu_);
  int n = 0;
  for (auto& c : cams_) n += c ? 1 : 0;
  return n;
}

void Worker::start() {
  std::lock_guard<std::mutex> g(q_mu_);
  if (running_) return;
  running_ = true;
  stop_ = false;
  th_ = std::thread([this] {
    name_thread("vep-worker");
    pin_current_thread(opt_.domain.cpus);
    loop();
  });
}

void Worker::stop() {
  {
    std::lock_guard<std::mutex> g(q_mu_);
    if (!running_) return;
    stop_ = true;
  }
  q_cv_.notify_all();
  taken_cv_.notify_all();
  if (th_.joinable()) th_.join();
  std::lock_guard<std::mutex> g(q_mu_);
  running_ = false;
}

static void fold_update(MbUpdate& into, const MbUpdate& from) {
  VEP_CHECK(into.width_mbs == from.width_mbs && into.height_mbs == from.height_mbs,
            "fold size mismatch");
  for (int mb = 0; mb < from.mbs(); ++mb) {
    int s = from.slot[size_t(mb)];
    if (s < 0) continue;
    into.set_in(mb, from.block(s), u32(into.segs.size()) + from.slot_seg[size_t(s)]);
  }
  into.segs.insert(into.segs.end(), from.segs.begin(), from.segs.end());
  into.keep.insert(into.keep.end(), from.keep.begin(), from.keep.end());
  into.own.insert(into.own.end(), from.own.begin(), from.own.end());
  into.frames += from.frames;
}

// Whether one of the job's own pictures reconstructs DPB slot `slot`.
static bool reconstructs_slot(const DecodeJob& j, int slot) {
  for (const auto& p : j.avc)
    if ((p->structure ? p->target / 2 : p->target) == slot) return true;
  for (const auto& p : j.hevc)
    if (p->target == slot) return true;
  return false;
}
// Whether one of the job's own pictures reconstructs its output slot.
static bool reconstructs_output(const DecodeJob& j) { return reconstructs_slot(j, j.out_slot); }

void merge_job(DecodeJob& p, DecodeJob&& job) {
  VEP_CHECK(p.cam == job.cam, "merge_job: different cameras");
  // collapse into the not-yet-launched job: latest writer wins per macroblock (fast path);
  // general-path pictures are appended (each references the previous ones)
  if (job.general() && p.general() && job.refresh) {
    // A backlog that reaches a keyframe restarts from it (load shedding: the queued pictures are
    // dropped). The keyframe bumps the previous GOP's pictures out of the reorder buffer; when the
    // frame it would publish is one of those, its reconstruction was in the dropped job, so the
    // merged job only reconstructs (the keyframe's picture is published by a later job).
    // (H.265 open GOPs: the RASL pictures of a CRA predict from the previous GOP, whose dropped
    // pictures are never reconstructed; they are not published either)
    std::vector<std::pair<int, i64>> dropped = std::move(p.dropped);
    std::vector<i64> poisoned = std::move(p.poisoned_cra);
    for (const auto& pic : p.avc) dropped.emplace_back(pic->structure ? pic->target / 2 : pic->target, pic->au.pts);
    for (const auto& pic : p.hevc) dropped.emplace_back(pic->target, pic->pts);
    const bool lost = !p.hevc.empty();
    p = std::move(job);
    if (lost)
      for (const auto& pic : p.hevc)
        if (pic->cra) poisoned.push_back(pic->tag);
    p.dropped.insert(p.dropped.begin(), dropped.begin(), dropped.end());
    p.poisoned_cra.insert(p.poisoned_cra.begin(), poisoned.begin(), poisoned.end());
    if (p.out_slot >= 0 && !reconstructs_output(p)) {
      p.out_slot = -1;
      p.out_fields = false;
    }
    // (history: the same rule for every output of the kept job)
    p.outputs.erase(std::remove_if(p.outputs.begin(), p.outputs.end(),
                                   [&](const JobOutput& o) { return !reconstructs_slot(p, o.slot); }),
                    p.outputs.end());
  } else if (job.general() && p.general()) {
    const int base = int(!p.avc.empty() ? p.avc.size() : p.hevc.size());  // job's pictures follow p's
    for (JobOutput& o : job.outputs) {
      o.released_by += base;
      p.outputs.push_back(std::move(o));
    }
    p.avc.insert(p.avc.end(), job.avc.begin(), job.avc.end());
    p.hevc.insert(p.hevc.end(), job.hevc.begin(), job.hevc.end());
    p.hevc_slots = std::max(p.hevc_slots, job.hevc_slots);
    if (job.out_slot >= 0 || p.out_slot < 0) {  // the newer output wins; none keeps the older
      p.pic = job.pic;
      p.meta = job.meta;
      p.out_slot = job.out_slot;
      p.out_fields = job.out_fields;
      p.out_rasl_of = job.out_rasl_of;
    }
    p.dropped.insert(p.dropped.end(), job.dropped.begin(), job.dropped.end());
    p.poisoned_cra.insert(p.poisoned_cra.end(), job.poisoned_cra.begin(), job.poisoned_cra.end());
  } else if (job.refresh || job.general() != p.general() || p.upd.width_mbs != job.upd.width_mbs ||
             p.upd.height_mbs != job.upd.height_mbs) {
    p = std::move(job);
  } else {
    fold_update(p.upd, job.upd);
    p.pic = job.pic;
    p.meta = job.meta;
  }
}

void Worker::submit(DecodeJob&& job) {
  {
    std::lock_guard<std::mutex> g(q_mu_);
    for (auto& p : pending_) {
      if (p.cam != job.cam) continue;
      merge_job(p, std::move(job));
      q_cv_.notify_one();
      return;
    }
    pending_.push_back(std::move(job));
  }
  q_cv_.notify_one();
}

void Worker::wait_camera_taken(int cam, int timeout_ms) {
  std::unique_lock<std::mutex> g(q_mu_);
  taken_cv_.wait_for(g, std::chrono::milliseconds(timeout_ms), [&] {
    if (stop_) return true;
    for (const DecodeJob& p : pending_)
      if (p.cam == cam) return false;
    return true;
  });
}

bool Worker::read_surface(int cam, HostSurface& out, i64* pts) {
  std::shared_ptr<Camera> c;
  int slot;
  {
    std::lock_guard<std::mutex> g(cams_mu_);
    if (cam < 0 || size_t(cam) >= cams_.size() || !cams_[size_t(cam)]) return false;
    c = cams_[size_t(cam)];
    slot = c->out_surface_slot;
    if (pts) *pts = c->out_surface_pts;
  }
  if (slot < 0) return false;
  const Camera::Surface& sf = c->surface;
  if (!dev_.gpu()) {
    if (size_t(slot) >= sf.host.size()) return false;
    out = sf.host[size_t(slot)];
    return true;
  }
  if (!sf.y || slot >= sf.slots) return false;
  out.alloc(sf.wmbs * 16, sf.hmbs * 16, sf.bd, sf.cf);
  void* dy = out.wide() ? static_cast<void*>(out.y16.data()) : static_cast<void*>(out.y.data());
  void* duv = out.wide() ? static_cast<void*>(out.uv16.data()) : static_cast<void*>(out.uv.data());
  VEP_CHECK(sf.slot_y() == size_t(out.coded_w) * size_t(out.coded_h) * size_t(sf.bps), "surface size mismatch");
  dev_.bind();
  VEP_HIP(hipDeviceSynchronize());  // (the picture's reconstruction ran on a lane stream)
  VEP_HIP(hipMemcpy(dy, sf.y + size_t(slot) * sf.slot_y(), sf.slot_y(), hipMemcpyDeviceToHost));
  VEP_HIP(hipMemcpy(duv, sf.uv + size_t(slot) * sf.slot_uv(), sf.slot_uv(), hipMemcpyDeviceToHost));
  return true;
}

void Camera::wait_reconstruction() {
  if (w_.options().backpressure) w_.wait_camera_taken(index_, 2000);
}

void Worker::flush() {
  {
    std::unique_lock<std::mutex> g(q_mu_);
    if (running_) {
      idle_cv_.wait(g, [this] { return pending_.empty() && !busy_; });
      return;
    }
  }
  complete_all();
}

void Worker::loop() {
  dev_.bind();
  std::vector<DecodeJob> batch;
  for (;;) {
    {
      std::unique_lock<std::mutex> g(q_mu_);
      q_cv_.wait(g, [this] { return stop_ || !pending_.empty(); });
      if (stop_ && pending_.empty()) break;
      if (kf_window_us_ > 0) {  // keyframe-only pictures: gather a few per wavefront launch
        auto all_kf = [this] {
          for (const DecodeJob& j : pending_)
            if (!j.keyframe_only) return false;
          return true;
        };
        const size_t enough = 8 * lanes_.size();
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(kf_window_us_);
        while (!stop_ && pending_.size() < enough && all_kf())
          if (q_cv_.wait_until(g, deadline) == std::cv_status::timeout) break;
      }
      batch.swap(pending_);
      busy_ = true;
    }
    taken_cv_.notify_all();
    try {
      launch_async(batch);
    } catch (const std::exception& e) {
      for (auto& j : batch)
        if (auto c = camera(j.cam)) {
          c->errors.fetch_add(1);
          c->logs.add(true, std::string("decode batch failed: ") + e.what());
        }
    }
    batch.clear();
    {
      std::lock_guard<std::mutex> g(q_mu_);
      if (!pending_.empty()) continue;  // keep the pipeline full while work keeps arriving
    }
    try {
      complete_all();
    } catch (const std::exception&) {
    }
    {
      std::lock_guard<std::mutex> g(q_mu_);
      if (pending_.empty()) busy_ = false;
    }
    idle_cv_.notify_all();
  }
  try {
    complete_all();
  } catch (const std::exception&) {
  }
}

void Worker::ensure_surface(Camera& c, const PictureInfo& pi, int slots, int bd, bool weave, int cf) {
  const int bps = bd > 8 ? 2 : 1;
  const int wmbs = pi.coded_width / 16, hmbs = pi.coded_height / 16;
  auto& s = c.surface;
  // the 8-bit frame the conversion reads when the slot is not one (Main10; a woven field pair)
  auto scratch8 = [&] {
    if (!dev_.gpu() || s.y8) return;
    const size_t y8 = size_t(s.wmbs) * 16 * s.hmbs * 16;
    s.y8 = static_cast<u8*>(dev_.alloc(y8));
    s.uv8 = static_cast<u8*>(dev_.alloc(y8 / 2));
  };
  if (s.wmbs == wmbs && s.hmbs == hmbs && s.slots >= slots && s.bd == bd && s.cf == cf && c.ring_ &&
      c.ring_->width() == pi.width && c.ring_->height() == pi.height) {
    if (weave) scratch8();  // (only ever added: no batch in flight reads a missing scratch)
    return;
  }
  dev_.free(s.y);
  dev_.free(s.uv);
  dev_.free(s.y8);
  dev_.free(s.uv8);
  s.y = s.uv = s.y8 = s.uv8 = nullptr;
  s.wmbs = wmbs;
  s.hmbs = hmbs;
  s.slots = std::max(1, slots);
  s.bps = bps;
  s.bd = bd;
  s.cf = cf;
  const size_t ysz = s.slot_y() * size_t(s.slots);
  if (dev_.gpu()) {
    s.y = static_cast<u8*>(dev_.alloc(ysz));
    const size_t uvsz = s.slot_uv() * size_t(s.slots);
    s.uv = static_cast<u8*>(dev_.alloc(uvsz));
    if (bps == 2) {  // Main10 / High 10: u16 samples at the depth's black / grey
      VEP_HIP(hipMemsetD16Async(reinterpret_cast<hipDeviceptr_t>(s.y), u16(16 << (bd - 8)), ysz / 2, stream_));
      VEP_HIP(hipMemsetD16Async(reinterpret_cast<hipDeviceptr_t>(s.uv), u16(128 << (bd - 8)), uvsz / 2, stream_));
      scratch8();
    } else {
      if (weave || cf == 2) scratch8();
      VEP_HIP(hipMemsetAsync(s.y, 16, ysz, stream_));
      VEP_HIP(hipMemsetAsync(s.uv, 128, uvsz, stream_));
    }
    // the camera's lane may be another stream: the fill must land before its first kernel
    if (lanes_.size() > 1) VEP_HIP(hipStreamSynchronize(stream_));
  } else {
    s.host.assign(size_t(s.slots), HostSurface{});
    for (auto& h : s.host) h.alloc(wmbs * 16, hmbs * 16, bd, cf);
  }
  c.set_ring(std::make_shared<FrameRing>(dev_, c.ring_slots_cfg, pi.width, pi.height, c.history()));
}

static inline size_t al(size_t x, size_t a = 256) { return (x + a - 1) & ~(a - 1); }

// CPU mirror of letterbox_nv12_kernel (same float math, same rounding).
static void cpu_letterbox_nv12(const HostSurface& s, const gpu::LetterboxDesc& d, int S, u8 pad) {
  const u8 pad_y = u8(std::lround(16.0 + pad * 219.0 / 255.0));
  auto axis = [](int o, int p, float r, int src, int& i0, int& i1, float& l) {
    const float v = std::max((float(o - p) + 0.5f) * r - 0.5f, 0.f);
    i0 = int(v);
    i1 = i0 + (i0 < src - 1 ? 1 : 0);
    l = v - float(i0);
  };
  auto lerp = [](const u8* p, int pitch, int step, int x0, int x1, int y0, int y1, float lx, float ly) {
    const float a = p[size_t(y0) * pitch + x0 * step], b = p[size_t(y0) * pitch + x1 * step];
    const float c = p[size_t(y1) * pitch + x0 * step], e = p[size_t(y1) * pitch + x1 * step];
    return (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * c + lx * e);
  };
  const int pitch = s.coded_w;
  const u8* Y = s.y.data() + size_t(d.crop_top) * pitch + d.crop_left;
  for (int oy = 0; oy < S; ++oy)
    for (int ox = 0; ox < S; ++ox) {
      u8 v = pad_y;
      if (oy >= d.pad_y && oy < d.pad_y + d.nh && ox >= d.pad_x && ox < d.pad_x + d.nw) {
        int x0, x1, y0, y1;
        float lx, ly;
        axis(oy, d.pad_y, d.ry, d.src_h, y0, y1, ly);
        axis(ox, d.pad_x, d.rx, d.src_w, x0, x1, lx);
        v = u8(std::min(lerp(Y, pitch, 1, x0, x1, y0, y1, lx, ly) + 0.5f, 255.f));
      }
      d.out_hwc[size_t(oy) * S + ox] = v;
    }
  const u8* UV = s.uv.data() + size_t(d.crop_top / 2) * pitch + (d.crop_left & ~1);
  const int px = d.pad_x / 2, py = d.pad_y / 2, nwc = d.nw / 2, nhc = d.nh / 2;
  const int sw = (d.src_w + 1) / 2, sh = (d.src_h + 1) / 2;
  u8* out = d.out_hwc + size_t(S) * S;
  for (int cy = 0; cy < S / 2; ++cy)
    for (int cx = 0; cx < S / 2; ++cx) {
      u8 u = 128, w = 128;
      if (cy >= py && cy < py + nhc && cx >= px && cx < px + nwc) {
        int x0, x1, y0, y1;
        float lx, ly;
        axis(cy, py, d.ry, sh, y0, y1, ly);
        axis(cx, px, d.rx, sw, x0, x1, lx);
        u = u8(std::min(lerp(UV, pitch, 2, x0, x1, y0, y1, lx, ly) + 0.5f, 255.f));
        w = u8(std::min(lerp(UV + 1, pitch, 2, x0, x1, y0, y1, lx, ly) + 0.5f, 255.f));
      }
      out[size_t(cy) * S + 2 * cx] = u;
      out[size_t(cy) * S + 2 * cx + 1] = w;
    }
}

// float -> bfloat16 bits, round to nearest even (the kernels' f32_to_bf16).
static inline u16 cpu_f32_to_bf16(float f) {
  u32 u;
  std::memcpy(&u, &f, 4);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return u16(u >> 16);
}

// float -> IEEE half bits, round to nearest even (what the kernels' _Float16 cast does).
static inline u16 cpu_f32_to_f16(float f) {
  u32 u;
  std::memcpy(&u, &f, 4);
  const u32 sign = (u >> 16) & 0x8000u;
  u &= 0x7FFFFFFFu;
  u32 o;
  if (u >= (143u << 23)) {  // >= 65536, infinity or NaN
    o = u > (255u << 23) ? 0x7E00u : 0x7C00u;
  } else if (u < (113u << 23)) {  // below 2^-14: a half subnormal; the float add rounds it
    const u32 magic = 126u << 23;  // 0.5f: its ulp is 2^-24, the half subnormal step
    float a, m;
    std::memcpy(&a, &u, 4);
    std::memcpy(&m, &magic, 4);
    a += m;
    std::memcpy(&o, &a, 4);
    o -= magic;
  } else {
    const u32 odd = (u >> 13) & 1u;
    u += (u32(15 - 127) << 23) + 0xFFFu + odd;  // rebias; a mantissa carry rounds up to infinity
    o = u >> 13;
  }
  return u16(sign | o);
}

static void cpu_letterbox(const HostSurface& s, const gpu::LetterboxDesc& d,
                          const gpu::LetterboxParams& p) {
  const int S = p.size;
  for (int oy = 0; oy < S; ++oy) {
    for (int ox = 0; ox < S; ++ox) {
      float v[3];
      bool in = oy >= d.pad_y && oy < d.pad_y + d.nh && ox >= d.pad_x && ox < d.pad_x + d.nw;
      if (!in) {
        v[0] = v[1] = v[2] = float(p.pad_value);
      } else {
        float sy = std::max((float(oy - d.pad_y) + 0.5f) * d.ry - 0.5f, 0.f);
        float sx = std::max((float(ox - d.pad_x) + 0.5f) * d.rx - 0.5f, 0.f);
        int y0 = int(sy), x0 = int(sx);
        int y1 = y0 + (y0 < d.src_h - 1 ? 1 : 0), x1 = x0 + (x0 < d.src_w - 1 ? 1 : 0);
        float ly = sy - float(y0), lx = sx - float(x0);
        auto px = [&](int x, int y, float* o) {
          x += d.crop_left;
          y += d.crop_top;
          const u8* c = &s.uv[size_t(y >> 1) * s.coded_w + (x & ~1)];
          u8 b, g, r;
          yuv_to_bgr(s.y[size_t(y) * s.coded_w + x], c[0], c[1], &b, &g, &r);
          o[0] = b;
          o[1] = g;
          o[2] = r;
        };
        float a[3], b[3], c[3], e[3];
        px(x0, y0, a);
        px(x1, y0, b);
        px(x0, y1, c);
        px(x1, y1, e);
        float w00 = (1.f - ly) * (1.f - lx), w01 = (1.f - ly) * lx, w10 = ly * (1.f - lx),
              w11 = ly * lx;
        for (int k = 0; k < 3; ++k) v[k] = w00 * a[k] + w01 * b[k] + w10 * c[k] + w11 * e[k];
      }
      size_t pix = size_t(oy) * S + ox;
      if (d.out_hwc)
        for (int k = 0; k < 3; ++k)
          d.out_hwc[pix * 3 + k] = u8(std::min(std::max(v[k] + 0.5f, 0.f), 255.f));
      if (d.out_chw && p.chw_dtype != gpu::kChwNone) {
        const size_t plane = size_t(S) * S;
        for (int k = 0; k < 3; ++k) {  // RGB planes from BGR values
          const float c = (v[2 - k] * (1.f / 255.f) - p.mean[k]) * p.inv_std[k];
          if (p.chw_dtype == gpu::kChwF32)
            static_cast<float*>(d.out_chw)[k * plane + pix] = c;
          else
            static_cast<u16*>(d.out_chw)[k * plane + pix] =
                p.chw_dtype == gpu::kChwF16 ? cpu_f32_to_f16(c) : cpu_f32_to_bf16(c);
        }
      }
    }
  }
}

// Drop jobs of vanished cameras, (re)allocate surfaces/rings, reserve ring slots.
void Worker::prepare(std::vector<DecodeJob>& jobs, std::vector<int>& slots) {
  bool resize = false;
  {
    std::lock_guard<std::mutex> g(cams_mu_);
    jobs.erase(std::remove_if(jobs.begin(), jobs.end(),
                              [&](const DecodeJob& j) {
                                return j.cam < 0 || j.cam >= int(cams_.size()) ||
                                       !cams_[size_t(j.cam)];
                              }),
               jobs.end());
    for (auto& j : jobs) {
      Camera& c = *cams_[size_t(j.cam)];
      const bool have = c.ring_ != nullptr;
      if (have && (c.surface.wmbs * 16 != j.pic.coded_width ||
                   c.surface.hmbs * 16 != j.pic.coded_height || c.ring_->width() != j.pic.width ||
                   c.ring_->height() != j.pic.height || c.surface.slots < j.dpb_slots() ||
                   c.surface.bd != j.bit_depth() || c.surface.cf != j.chroma_format()))
        resize = true;
    }
  }
  if (resize) complete_locked();  // never free a surface an in-flight batch still writes
  std::lock_guard<std::mutex> g(cams_mu_);
  slots.resize(jobs.size());
  for (size_t i = 0; i < jobs.size(); ++i) {
    Camera& c = *cams_[size_t(jobs[i].cam)];
    bool weave = jobs[i].out_fields;
    for (const auto& p : jobs[i].avc) weave |= p->structure != 0;
    ensure_surface(c, jobs[i].pic, jobs[i].dpb_slots(), jobs[i].bit_depth(), weave, jobs[i].chroma_format());
    if (!jobs[i].outputs.empty()) reserve_history(c, jobs[i]);
    slots[i] = jobs[i].has_output() ? c.ring_->begin_write() : -1;
  }
}

// Frame history: ring slots for the job's outputs before the newest one. The last
// min(H, outputs) outputs of the job are kept (the newest takes its slot as ever); the others,
// and those of a job outside the multi-output path (field pictures), count as history_skipped.
// Slots go to the newest outputs first, so when the ring has none left the older ones are dropped.
void Worker::reserve_history(Camera& c, DecodeJob& j) {
  const size_t nh = j.history_outputs();
  const Camera::Surface& sf = c.surface;
  bool eligible = c.history() > 0 && !j.out_fields && !j.ext;
  for (const auto& p : j.avc) eligible &= p->structure == 0;
  for (const JobOutput& o : j.outputs) eligible &= !o.fields;
  const size_t room = size_t(std::max(0, c.history() - (j.out_slot >= 0 ? 1 : 0)));
  const size_t keep = eligible ? std::min(nh, room) : 0;
  const int npics = int(!j.avc.empty() ? j.avc.size() : j.hevc.size());
  const int dpb = j.hevc.empty() ? j.dpb_slots() : j.hevc_slots;
  size_t taken = 0;
  for (size_t k = nh; k-- > nh - keep;) {
    JobOutput& o = j.outputs[k];
    // only pictures of the surfaces' and the ring's geometry (the conversion is not bounds-checked)
    const bool fits = o.slot >= 0 && o.slot < dpb && o.slot < sf.slots && o.released_by >= 0 && o.released_by < npics &&
                      o.pic.coded_width == sf.wmbs * 16 && o.pic.coded_height == sf.hmbs * 16 &&
                      o.pic.width == c.ring_->width() && o.pic.height == c.ring_->height() && o.pic.crop_left >= 0 &&
                      o.pic.crop_top >= 0 && o.pic.crop_left + o.pic.width <= o.pic.coded_width &&
                      o.pic.crop_top + o.pic.height <= o.pic.coded_height;
    if (!fits) continue;
    o.ring_slot = c.ring_->try_write();
    if (o.ring_slot < 0) break;
    ++taken;
  }
  if (nh > taken) c.history_skipped.fetch_add(nh - taken, std::memory_order_relaxed);
}

namespace {

// Coded-MB bitmask + per-word exclusive prefix, and the raster-order table of sample blocks:
// table[k] = where(segment, byte offset inside it) of the k-th coded MB's samples.
// O(coded MBs), not O(picture MBs): a P frame touches a few hundred of 8,160 MBs.
template <class T, class Where>
void build_index(const MbUpdate& u, u32* mask, u32* prefix, T* table, Where where) {
  const int words = (u.mbs() + 31) / 32;
  std::memset(mask, 0, size_t(words) * sizeof(u32));
  const std::vector<i32>* list = &u.coded;
  std::vector<i32> sorted;
  if (!std::is_sorted(u.coded.begin(), u.coded.end())) {  // GOP collapse re-ordered slots
    sorted = u.coded;
    std::sort(sorted.begin(), sorted.end());
    list = &sorted;
  }
  size_t k = 0;
  for (i32 mb : *list) {
    mask[mb >> 5] |= 1u << (mb & 31);
    const int s = u.slot[size_t(mb)];
    const u32 g = u.slot_seg[size_t(s)];
    table[k++] = where(g, size_t(u.block(s) - u.segs[g].base));
  }
  u32 run = 0;
  for (int w = 0; w < words; ++w) {
    prefix[w] = run;
    run += u32(__builtin_popcount(mask[w]));
  }
}

}  // namespace

void Worker::StagePair::reserve(size_t need) {
  if (need <= cap) return;
  release();
  const size_t want = std::max(need + need / 2, size_t(4) << 20);
  void* p = nullptr;
  VEP_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
  h = static_cast<u8*>(p);
  VEP_HIP(hipMalloc(&p, want));
  d = static_cast<u8*>(p);
  void* hd = nullptr;
  if (hipHostGetDevicePointer(&hd, h, 0) != hipSuccess) hd = h;
  h_dev = static_cast<const u8*>(hd);
  hostmem::register_range(h, want, h_dev);
  cap = want;  // (only now: a pair whose growth threw is empty and grows again)
}

void Worker::StagePair::release() {
  if (cap) hostmem::unregister_range(h);
  cap = 0;
  if (d) (void)hipFree(d);
  if (h) (void)hipHostFree(h);
  h = d = nullptr;
  h_dev = nullptr;
}

// One batch on a lane. Slice bytes stay in host memory: pinned AU blocks as received (hostmem.h),
// or the stage's pinned half for pageable AUs (one host memcpy). Two ways to the GPU:
//  * direct (default): decode_convert reads each block straight over PCIe from its host address
//    (per-MB 64-bit pointer table) — no device copy of the payload at all;
//  * gather: a gather kernel first pulls the slices into the device half, and the kernel reads
//    per-MB offsets into that copy.
// stage_plan.h has the layout of the buffer pair.
void Worker::launch_gpu(Lane& ln, Stage& st) {
  const StagePlan pl(st.jobs, {direct_reads_, hevc_tu_window_});
  check_plan(pl, st);
  Described ds;
  const i64 t_res0 = mono_us();
  reserve_stage(pl, st, ds);
  const i64 t_res = mono_us() - t_res0;  // (counted as enqueue time, where its parts always were)
  stage_batch(pl, st);
  const i64 t_enq0 = mono_us();
  describe_outputs(pl, st, ds);
  describe_history(pl, st);
  for (size_t r = 0; r < pl.avc_rounds.size(); ++r) describe_avc_round(pl, r, st);
  for (size_t r = 0; r < pl.hevc_rounds.size(); ++r) describe_hevc_round(pl, r, st, ds);
  describe_masks(st, ds);
  enqueue(pl, ln, st, ds);
  add_time(&Timers::enqueue, double(mono_us() - t_enq0 + t_res));
}

// The checks of a batch that need its cameras' surfaces and rings (StagePlan makes those that
// need only the jobs).
void Worker::check_plan(const StagePlan& pl, const Stage& st) {
  auto surface = [&](int job) -> const Camera::Surface& { return cams_[size_t(st.jobs[size_t(job)].cam)]->surface; };
  for (int i : pl.outs) {
    const DecodeJob& j = st.jobs[size_t(i)];
    const Camera::Surface& sf = surface(i);
    if (j.out_fields)
      VEP_CHECK(sf.y8 && sf.bps == 1 && sf.hmbs % 2 == 0, "field pair output without its weave scratch");
    if (opt_.letterbox_size > 0) VEP_CHECK(j.cam < st.cons_rows, "camera index exceeds consumer batch rows");
  }
  for (const StagePlan::AvcPic& a : pl.avc)
    VEP_CHECK(surface(a.job).bd == a.p->bd && surface(a.job).cf == a.p->cf,
              "H.264: picture bit depth / chroma format differs from the camera's surfaces");
  for (const StagePlan::HevcPic& a : pl.hevc) {
    VEP_CHECK(surface(a.job).bps == (a.p->wide() ? 2 : 1), "HEVC: picture bit depth differs from the camera's surfaces");
    VEP_CHECK(surface(a.job).slots > st.jobs[size_t(a.job)].hevc_slots, "camera surfaces lack the SAO scratch slot");
  }
  for (const StagePlan::HistOut& h : pl.hist) {  // (the plan counted its tiles from the picture's coded size)
    const DecodeJob& j = st.jobs[size_t(h.job)];
    const JobOutput& o = j.outputs[size_t(h.out)];
    const Camera::Surface& sf = surface(h.job);
    const FrameRing& ring = *cams_[size_t(j.cam)]->ring_;
    VEP_CHECK(o.slot < sf.slots && o.pic.width == ring.width() && o.pic.height == ring.height() &&
                  o.pic.coded_width == sf.wmbs * 16 && o.pic.coded_height == sf.hmbs * 16,
              "history output does not match the camera's surfaces");
  }
  for (const DecodeJob& j : st.jobs) {
    if (!j.ext) continue;
    const Camera::Surface& sf = cams_[size_t(j.cam)]->surface;
    VEP_CHECK(j.ext->width <= sf.wmbs * 16 && j.ext->height <= sf.hmbs * 16, "VCN picture exceeds the camera surface");
  }
}

// Every allocation of the batch, and nothing later: the buffer pair, the error words (cleared),
// the mask descriptors (under the lists the cameras have now: publish() commits a slot only if
// its camera's list is still that one) and each H.265 camera's intra edge exchange.
void Worker::reserve_stage(const StagePlan& pl, Stage& st, Described& ds) {
  const size_t n = st.jobs.size();
  st.buf.reserve(pl.need);  // (the stage's previous batch is complete: nothing reads the old buffers)
  if (st.err.cap < n) {
    st.err.reserve(n, 64);
    void* ed = nullptr;
    if (hipHostGetDevicePointer(&ed, st.err.p, 0) != hipSuccess) ed = st.err.p;
    st.err_dev = static_cast<u32*>(ed);
  }
  std::memset(st.err.p, 0, n * sizeof(u32));
  if (snapshot_masks(st.jobs, st.mask_snap)) {
    size_t nd = 0;
    for (size_t i = 0; i < n; ++i) {
      size_t slots_of = st.jobs[i].has_output() ? 1 : 0;
      for (const JobOutput& o : st.jobs[i].outputs) slots_of += o.ring_slot >= 0 ? 1 : 0;
      nd += slots_of * size_t(st.mask_snap[i].n);
    }
    VEP_CHECK(nd <= 65535, "mask descriptors miscounted");
    if (nd > 0) {
      st.mask_h.reserve(nd, 256);
      st.mask_d.reserve(nd, 256);
    }
    ds.nmask = int(nd);
  }
  // the cameras' intra edge exchanges (zeroed once: epochs start at 1), one epoch per round
  ds.hevc_epoch.resize(pl.hevc.size());
  for (const StagePlan::HevcRound& rd : pl.hevc_rounds) {
    for (int k : rd.pics) {
      Camera::Surface& sf = cams_[size_t(st.jobs[size_t(pl.hevc[size_t(k)].job)].cam)]->surface;
      const size_t words = gpu::hevc_xg_words(sf.wmbs * 16, sf.hmbs * 16);
      if (sf.hevc_xg_words < words) {
        dev_.free(sf.hevc_xg);
        sf.hevc_xg = static_cast<u64*>(dev_.alloc(words * sizeof(u64)));
        VEP_HIP(hipMemset(sf.hevc_xg, 0, words * sizeof(u64)));
        sf.hevc_xg_words = words;
        sf.hevc_epoch = 0;
      }
      if (++sf.hevc_epoch == 0) {  // (after 2^32 rounds) never reuse a tag still in the words
        VEP_HIP(hipMemset(sf.hevc_xg, 0, words * sizeof(u64)));
        sf.hevc_epoch = 1;
      }
      ds.hevc_epoch[size_t(k)] = sf.hevc_epoch;
    }
  }
}

// The pinned half's bulk: gather chunks, then (pack threads) per job the coded-MB bitmask,
// prefix and per-MB offsets or pointers, then the copies of records and pageable segments.
void Worker::stage_batch(const StagePlan& pl, Stage& st) {
  const std::vector<DecodeJob>& jobs = st.jobs;
  const int n = int(jobs.size());
  u8* const h = st.buf.h;
  auto* gc = reinterpret_cast<gpu::GatherChunk*>(h + pl.gather.off);
  for (size_t k = 0; k < pl.chunks.size(); ++k) {
    const StagePlan::Chunk& c = pl.chunks[k];
    gc[k] = {c.src ? c.src : st.buf.h_dev + c.dst, st.buf.d + c.dst, c.len, 0};
  }
  records_gathered_ += pl.bytes_gathered;
  pinned_bytes_staged_ += pl.bytes_staged;
  pinned_bytes_inplace_ += pl.bytes_inplace;
  auto index = [&](int i) {
    const StagePlan::Job& jp = pl.jobs[size_t(i)];
    auto* mask = reinterpret_cast<u32*>(h + jp.mask.off);
    auto* prefix = reinterpret_cast<u32*>(h + jp.prefix.off);
    const MbUpdate& u = jobs[size_t(i)].upd;
    if (pl.set.direct) {  // per MB the device address of its samples in host memory (AU block or pinned half)
      const u8* staged = st.buf.h_dev + jp.payload;
      build_index(u, mask, prefix, reinterpret_cast<u64*>(h + jp.table.off), [&](u32 g, size_t o) {
        return reinterpret_cast<u64>((jp.seg_dev[g] ? jp.seg_dev[g] : staged + jp.seg_rel[g]) + o);
      });
    } else {  // per MB the offset of its samples in the device copy of the job's payload
      build_index(u, mask, prefix, reinterpret_cast<u32*>(h + jp.table.off),
                  [&](u32 g, size_t o) { return u32(jp.seg_rel[g] + o); });
    }
  };
  const i64 t_index0 = mono_us();
  {
    trace::Range tr("vep.index");
    if (pack_pool_ && n > 1) pack_pool_->parallel_for(n, index);
    else for (int i = 0; i < n; ++i) index(i);
  }
  const i64 t_copy0 = mono_us();
  add_time(&Timers::index, double(t_copy0 - t_index0));
  const auto& tasks = pl.tasks;
  auto copy = [&](int t) { std::memcpy(h + tasks[size_t(t)].dst, tasks[size_t(t)].src, tasks[size_t(t)].len); };
  if (pack_pool_ && tasks.size() > 1) pack_pool_->parallel_for(int(tasks.size()), copy);
  else for (int t = 0; t < int(tasks.size()); ++t) copy(t);
  add_time(&Timers::copy, double(mono_us() - t_copy0));
}

// Conversion, letterbox and weave descriptors, only for jobs that publish a frame (a general-path
// job whose pictures all wait in the reorder buffer only reconstructs).
void Worker::describe_outputs(const StagePlan& pl, Stage& st, Described& ds) {
  u8* const dv = st.buf.d;
  auto* hd = reinterpret_cast<gpu::DecodeDesc*>(st.buf.h + pl.decode.off);
  auto* hl = reinterpret_cast<gpu::LetterboxDesc*>(st.buf.h + pl.letterbox.off);
  auto* hw = reinterpret_cast<gpu::WeaveDesc*>(st.buf.h + pl.weave.off);
  for (size_t k = 0; k < pl.outs.size(); ++k) {
    const int i = pl.outs[k];
    const DecodeJob& j = st.jobs[size_t(i)];
    const StagePlan::Job& jp = pl.jobs[size_t(i)];
    const Camera* c = cams_[size_t(j.cam)].get();
    const Camera::Surface& sf = c->surface;
    gpu::DecodeDesc& d = hd[k];
    const size_t tgt = size_t(j.target());
    if (j.out_fields) {  // field pair: woven into the 8-bit scratch first (launch_weave)
      gpu::WeaveDesc& w = hw[ds.nweave++];
      w.y = sf.y + tgt * sf.slot_y();
      w.uv = sf.uv + tgt * sf.slot_uv();
      w.y8 = sf.y8;
      w.uv8 = sf.uv8;
      w.pitch = sf.wmbs * 16;
      w.height = sf.hmbs * 16;
      ds.weave_pitch = std::max(ds.weave_pitch, w.pitch);
      ds.weave_h = std::max(ds.weave_h, w.height);
    }
    if (sf.narrowed() || j.out_fields) {  // Main10 / 4:2:2 / field pair: convert / letterbox the
                                          // 8-bit frame (launch_narrow / launch_weave)
      d.y = sf.y8;
      d.uv = sf.uv8;
    } else {
      d.y = sf.y + tgt * sf.slot_y();
      d.uv = sf.uv + tgt * sf.slot_uv();
    }
    d.bgr = c->ring_->slot_ptr(st.slots[size_t(i)]);
    d.mask = reinterpret_cast<const u32*>(dv + jp.mask.off);
    d.prefix = reinterpret_cast<const u32*>(dv + jp.prefix.off);
    if (pl.set.direct) {
      d.ptrs = reinterpret_cast<const u64*>(dv + jp.table.off);
      d.offsets = nullptr;
      d.payload = nullptr;
    } else {
      d.ptrs = nullptr;
      d.offsets = reinterpret_cast<const u32*>(dv + jp.table.off);
      d.payload = dv + jp.payload;
    }
    const bool whole = j.general() || j.ext;  // the slot already holds the picture
    d.wmbs = whole ? j.pic.coded_width / 16 : j.upd.width_mbs;
    d.hmbs = whole ? j.pic.coded_height / 16 : j.upd.height_mbs;
    if (whole) d.mask = d.prefix = nullptr;  // pure conversion of the reconstructed slot
    d.out_w = j.pic.width;
    d.out_h = j.pic.height;
    d.crop_left = j.pic.crop_left;
    d.crop_top = j.pic.crop_top;
    d.tiles_x = (d.wmbs + gpu::kTileMbW - 1) / gpu::kTileMbW;
    d.tile_begin = ds.tiles;
    d.chk_lo = j.pic.spec_lo;
    d.chk_hi = j.pic.spec_hi;
    d.chk_pat = 0x000Du;  // I_PCM header bytes 0D 00
    d.err = st.err_dev + i;
    ds.tiles += gpu::tiles_for(d.wmbs, d.hmbs);
    if (opt_.letterbox_size > 0) {
      gpu::LetterboxDesc& l = hl[k];
      const size_t S = size_t(opt_.letterbox_size);
      l.y = d.y;
      l.uv = d.uv;
      l.pitch = d.wmbs * 16;
      l.src_w = j.pic.width;
      l.src_h = j.pic.height;
      l.crop_left = j.pic.crop_left;
      l.crop_top = j.pic.crop_top;
      l.out_hwc = st.cons_hwc ? st.cons_hwc + size_t(j.cam) * gpu::letterbox_bytes(int(S), opt_.letterbox_format)
                            : nullptr;
      const size_t es = opt_.chw_dtype == gpu::kChwF32 ? 4 : 2;
      l.out_chw = st.cons_chw ? static_cast<u8*>(st.cons_chw) + size_t(j.cam) * 3 * S * S * es
                            : nullptr;
      gpu::fill_letterbox_geometry(l, opt_.letterbox_size, opt_.letterbox_format == gpu::kLbNV12);
    }
  }
}

// History conversions, in round order (StagePlan::hist).
void Worker::describe_history(const StagePlan& pl, Stage& st) {
  auto* hs = reinterpret_cast<gpu::SurfaceBgrDesc*>(st.buf.h + pl.history.off);
  for (size_t k = 0; k < pl.hist.size(); ++k) {
    const DecodeJob& j = st.jobs[size_t(pl.hist[k].job)];
    const JobOutput& o = j.outputs[size_t(pl.hist[k].out)];
    const Camera* c = cams_[size_t(j.cam)].get();
    const Camera::Surface& sf = c->surface;
    gpu::SurfaceBgrDesc& d = hs[k];
    d = gpu::SurfaceBgrDesc{};
    d.y = sf.y + size_t(o.slot) * sf.slot_y();
    d.uv = sf.uv + size_t(o.slot) * sf.slot_uv();
    d.bgr = c->ring_->slot_ptr(o.ring_slot);
    d.pitch = d.coded_w = sf.wmbs * 16;
    d.coded_h = sf.hmbs * 16;
    d.bit_depth = sf.bd;
    d.chroma_format = sf.cf;
    d.crop_left = o.pic.crop_left;
    d.crop_top = o.pic.crop_top;
    d.out_w = o.pic.width;
    d.out_h = o.pic.height;
    d.tile_begin = pl.hist[k].tile_begin;
    gpu::check_surface_bgr(d);
  }
}

void Worker::describe_avc_round(const StagePlan& pl, size_t r, Stage& st) {
  const StagePlan::AvcRound& rd = pl.avc_rounds[r];
  u8* const dv = st.buf.d;
  auto* ad = reinterpret_cast<gpu::AvcDesc*>(st.buf.h + rd.descs.off);
  int mbs = 0;
  for (size_t k = 0; k < rd.pics.size(); ++k) {
    const StagePlan::AvcPic& a = pl.avc[size_t(rd.pics[k])];
    const Camera::Surface& sf = cams_[size_t(st.jobs[size_t(a.job)].cam)]->surface;
    gpu::AvcDesc& g = ad[k];
    g = gpu::AvcDesc{};
    g.mbs = dv + a.mbs.off;
    g.coefs = reinterpret_cast<const i16*>(dv + a.coefs.off);
    g.mvs = reinterpret_cast<const i16*>(dv + a.mvs.off);
    g.wps = dv + a.wps.off;
    g.y = sf.y;
    g.uv = sf.uv;
    // field pictures address field slots: half a frame slot each (top field rows, then bottom)
    const size_t per = a.p->structure ? 2 : 1;
    g.slot_y = sf.slot_y() / per;
    g.slot_uv = sf.slot_uv() / per;
    g.wmbs = a.p->wmbs;
    g.hmbs = a.p->hmbs;
    g.target = a.p->target;
    g.constrained = a.p->constrained_intra ? 1 : 0;
    g.mb_begin = mbs;
    g.field = a.p->structure;
    g.err = st.err_dev + a.job;
    g.dbk = dv + a.dbk.off;
    g.res = reinterpret_cast<i16*>(dv + a.res.off);
    g.xg = reinterpret_cast<u64*>(dv + a.xg.off);
    g.prof = avc_prof_;
    g.bd = a.p->bd;
    g.qp_bias = a.p->qp_bias;
    g.qpc_bias = a.p->qpc_bias;
    g.cf = a.p->cf;
    g.ncoef = u32(a.p->coefs.size());
    g.nres = u32(a.p->intra_res);
    g.intra_mbs = a.p->intra_mbs;
    g.deblock = a.p->deblock ? 1 : 0;
    mbs += a.p->nmbs();
  }
}

// An H.265 round's descriptors, TU ranges, zeroed ticket counters and per-picture queues.
void Worker::describe_hevc_round(const StagePlan& pl, size_t r, Stage& st, const Described& ds) {
  const StagePlan::HevcRound& rd = pl.hevc_rounds[r];
  u8* const dv = st.buf.d;
  auto* hd = reinterpret_cast<gpu::HevcDesc*>(st.buf.h + rd.descs.off);
  int pus = 0, blks = 0;
  for (size_t k = 0; k < rd.pics.size(); ++k) {
    const StagePlan::HevcPic& a = pl.hevc[size_t(rd.pics[k])];
    const hevc::GpuPicture& p = *a.p;
    const DecodeJob& j = st.jobs[size_t(a.job)];
    const Camera::Surface& sf = cams_[size_t(j.cam)]->surface;
    gpu::HevcDesc& g = hd[k];
    g = gpu::HevcDesc{};
    g.y = sf.y;
    g.uv = sf.uv;
    g.slot_y = sf.slot_y();
    g.slot_uv = sf.slot_uv();
    g.stride = sf.wmbs * 16;
    g.width = p.width;
    g.height = p.height;
    g.log2ctb = p.log2ctb;
    g.wctb = p.wctb;
    g.hctb = p.hctb;
    g.target = p.target;
    g.cb_qp_offset = p.cb_qp_offset;
    g.cr_qp_offset = p.cr_qp_offset;
    g.flags = (p.deblock ? 1 : 0) | (p.sao ? 2 : 0) | (p.pcm_nofilter ? 4 : 0) | (p.tiles_block_sao ? 8 : 0) |
              (p.wide() ? gpu::kHevcWide : 0);
    g.bd_y = p.bd_y;
    g.bd_c = p.bd_c;
    g.pus = dv + a.pus.off;
    g.tus = dv + a.tus.off;
    g.coefs = reinterpret_cast<const i16*>(dv + a.coefs.off);
    g.pcm = dv + a.pcm.off;
    g.bs_v = dv + a.bs_v.off;
    g.bs_h = dv + a.bs_h.off;
    g.qp = reinterpret_cast<const signed char*>(dv + a.qp.off);
    g.pcm_map = dv + a.pcm_map.off;
    g.ctb_slice = reinterpret_cast<const u16*>(dv + a.ctb_slice.off);
    g.slices = dv + a.slices.off;
    g.sao = dv + a.sao.off;
    g.wp = dv + a.wp.off;
    g.ctb_tile = reinterpret_cast<const u16*>(dv + a.ctb_tile.off);
    const size_t scratch = size_t(j.hevc_slots);  // the extra surface after the DPB slots
    g.sao_y = sf.y + scratch * sf.slot_y();
    g.sao_uv = sf.uv + scratch * sf.slot_uv();
    g.err = st.err_dev + a.job;
    g.xg = hevc_tu_window_ == 0 ? nullptr : sf.hevc_xg;  // (per-level launches read the picture)
    g.xg_h = sf.hmbs * 16;
    g.epoch = ds.hevc_epoch[size_t(rd.pics[k])];
    g.nap_max = hevc_tu_nap_;
    g.npu = int(p.pus.size());
    g.pu_begin = pus;
    g.blk_begin = blks;
    pus += g.npu;
    blks += p.w4() * p.h4();
  }
  if (!rd.tu_ranges.empty())
    std::memcpy(st.buf.h + rd.ranges.off, rd.tu_ranges.data(), rd.tu_ranges.size() * sizeof(gpu::HevcTuRange));
  std::memset(st.buf.h + rd.counters.off, 0, std::max<size_t>(rd.windows.size(), 1) * sizeof(u32));
  if (!rd.pic_queues.empty())
    std::memcpy(st.buf.h + rd.picq.off, rd.pic_queues.data(), rd.pic_queues.size() * sizeof(gpu::HevcTuRange));
}

// Privacy masks: every ring slot this batch converts into (the newest frame's and the earlier
// outputs') gets its camera's masks, under the lists snapshot in reserve_stage.
void Worker::describe_masks(Stage& st, Described& ds) {
  if (ds.nmask == 0) return;
  size_t k = 0;
  auto add = [&](const Camera& c, const MaskSnap& ms, int slot, int w, int h) {
    VEP_CHECK(w == c.ring_->width() && h == c.ring_->height(), "masked output does not match the camera's ring");
    ds.mask_levels = std::max(ds.mask_levels, gpu::fill_mask_descs(st.mask_h.p + k, c.ring_->slot_ptr(slot),
                                                                   c.ring_->slot_bytes(), w, h, ms.m, ms.n));
    k += size_t(ms.n);
  };
  for (size_t i = 0; i < st.jobs.size(); ++i) {
    const DecodeJob& j = st.jobs[i];
    const MaskSnap& ms = st.mask_snap[i];
    if (ms.n == 0) continue;
    const Camera& c = *cams_[size_t(j.cam)];
    for (const JobOutput& o : j.outputs)
      if (o.ring_slot >= 0) add(c, ms, o.ring_slot, o.pic.width, o.pic.height);
    if (j.has_output()) add(c, ms, st.slots[i], j.pic.width, j.pic.height);
  }
  VEP_CHECK(k == size_t(ds.nmask), "mask descriptors miscounted");
}

// THE RULE: from the first call below that puts work on a stream, nothing follows but HIP enqueue
// calls and kernel launches: no VEP_CHECK on batch contents, no allocation, no synchronous
// memset. launch_on gives a batch's ring slots back when launch_gpu throws, and kernels already
// on the stream would go on writing into them; so whatever can refuse a batch (StagePlan,
// check_plan, reserve_stage, the describe steps) has run by now, and only a failing HIP call can
// still throw here.
void Worker::enqueue(const StagePlan& pl, Lane& ln, Stage& st, const Described& ds) {
  const hipStream_t cs = ln.stream;
  const std::vector<DecodeJob>& jobs = st.jobs;
  u8* const dv = st.buf.d;
  const auto* chunks = reinterpret_cast<const gpu::GatherChunk*>(dv + pl.gather.off);
  const int nchunks = int(pl.chunks.size());
  // H2D on the copy stream overlaps the previous batch's kernels on the compute stream: the
  // small header region by SDMA, the slice payload by the gather kernel (PCIe reads).
  // With several lanes the copy goes on the lane's own stream instead: it then waits for the
  // lane's previous kernels, while the other lanes keep the GPU busy, and no lane ever waits
  // on a queue another lane shares.
  // (the stage's previous batch has completed, launch_on: the device half is free)
  const hipStream_t hs = ln.copy ? ln.copy : lanes_.size() > 1 ? cs : copy_stream_;
  if (hs == cs) VEP_HIP(hipEventRecord(st.e0, cs));
  VEP_HIP(hipMemcpyAsync(dv, st.buf.h, pl.header_bytes, hipMemcpyHostToDevice, hs));
  if (nchunks) gpu::launch_gather(chunks, nchunks, hs);
  if (hs != cs) {
    VEP_HIP(hipEventRecord(st.copied, hs));
    VEP_HIP(hipStreamWaitEvent(cs, st.copied, 0));
    VEP_HIP(hipEventRecord(st.e0, cs));
  }
  auto convert_history = [&](const StagePlan::HistSpan& hs) {  // the outputs a round's pictures released
    if (hs.count > 0)
      gpu::launch_surface_to_bgr(reinterpret_cast<const gpu::SurfaceBgrDesc*>(dv + pl.history.off) + hs.first, hs.count,
                                 hs.tiles, cs);
  };
  for (const StagePlan::AvcRound& rd : pl.avc_rounds) {
    const auto* ad = reinterpret_cast<const gpu::AvcDesc*>(dv + rd.descs.off);
    const int np = int(rd.pics.size());
    gpu::launch_avc_inter(ad, np, rd.mbs, cs);
    if (rd.intra && rd.narrow) gpu::launch_avc_intra(ad, np, rd.max_h, cs);
    if (rd.dbk) {
      gpu::launch_avc_bs(ad, np, rd.mbs, cs);
      if (rd.narrow) gpu::launch_avc_deblock(ad, np, rd.max_h, cs, dbk_packed_);
    }
    if (rd.variants) gpu::launch_avc_hbd(ad, np, rd.intra, rd.dbk, rd.variants, cs);  // (High 10 / 4:2:2 pictures)
    convert_history(rd.hist);
  }
  for (const StagePlan::HevcRound& rd : pl.hevc_rounds) {
    const auto* hd = reinterpret_cast<const gpu::HevcDesc*>(dv + rd.descs.off);
    const auto* hr = reinterpret_cast<const gpu::HevcTuRange*>(dv + rd.ranges.off);
    const int np = int(rd.pics.size());
    gpu::launch_hevc_mc(hd, np, rd.pus, cs);
    gpu::launch_hevc_tu(hd, hr, rd.l0_ranges, 0, rd.l0_blocks, cs);
    if (hevc_tu_window_ < 0) {  // one workgroup per picture: every dependency wait inside it
      gpu::launch_hevc_tu_pics(hd, reinterpret_cast<const gpu::HevcTuRange*>(dv + rd.picq.off), int(rd.pic_queues.size()),
                               cs);
    } else if (hevc_tu_window_ == 0) {  // one launch per intra level (kernel boundaries order the levels)
      for (const StagePlan::Span& lv : rd.levels)
        gpu::launch_hevc_tu(hd, hr + rd.l0_ranges, rd.intra_ranges, lv.first, lv.count, cs);
    } else {  // one queue launch per window of levels, in level order on the stream
      auto* ctr = reinterpret_cast<u32*>(dv + rd.counters.off);
      // (a window of bounded depth runs one wave per block, each taking its block from the
      // window's ticket counter; the whole round keeps the persistent ticket queue)
      const bool persistent = hevc_tu_window_ >= kAllLevels;
      for (size_t k = 0; k < rd.windows.size(); ++k)
        gpu::launch_hevc_tu_queue(hd, hr + rd.l0_ranges, rd.intra_ranges, rd.windows[k].first, rd.windows[k].count,
                                  ctr + k, persistent, cs);
    }
    if (rd.dbk) {
      gpu::launch_hevc_deblock(hd, np, rd.blks, 0, cs);
      gpu::launch_hevc_deblock(hd, np, rd.blks, 1, cs);
    }
    if (rd.sao) gpu::launch_hevc_sao(hd, np, rd.blks, cs);
    convert_history(rd.hist);
  }
  // VCN pictures: the video core's surfaces -> the cameras' NV12 surfaces (device copies on the
  // lane stream, ordered before the conversion; the surfaces return to rocDecode when the batch
  // completes and its jobs are dropped)
  for (const DecodeJob& j : jobs) {
    if (!j.ext) continue;
    const Camera::Surface& sf = cams_[size_t(j.cam)]->surface;
    const vcn::Frame& f = *j.ext;
    const size_t pitch = size_t(sf.wmbs) * 16;
    VEP_HIP(hipMemcpy2DAsync(sf.y, pitch, f.y, f.pitch_y, size_t(f.width), size_t(f.height), hipMemcpyDefault, cs));
    VEP_HIP(hipMemcpy2DAsync(sf.uv, pitch, f.uv, f.pitch_uv, size_t(f.width), size_t(f.height / 2), hipMemcpyDefault, cs));
  }
  gpu::launch_weave(reinterpret_cast<const gpu::WeaveDesc*>(dv + pl.weave.off), ds.nweave, ds.weave_pitch, ds.weave_h, cs);
  for (int i : pl.outs) {  // Main10 pictures: the published slot's 8-bit NV12 copy
    const DecodeJob& j = jobs[size_t(i)];
    const Camera::Surface& sf = cams_[size_t(j.cam)]->surface;
    const size_t tgt = size_t(j.target());
    if (!sf.narrowed()) continue;
    gpu::launch_narrow(sf.y + tgt * sf.slot_y(), sf.uv + tgt * sf.slot_uv(), sf.y8, sf.uv8, sf.wmbs * 16,
                       sf.hmbs * 16, sf.bd, sf.cf, cs);
  }
  const int nout = int(pl.outs.size());
  gpu::launch_decode_convert(reinterpret_cast<const gpu::DecodeDesc*>(dv + pl.decode.off), nout, ds.tiles, cs);
  if (opt_.letterbox_size > 0) {
    gpu::LetterboxParams p{};
    p.size = opt_.letterbox_size;
    p.chw_dtype = opt_.chw_dtype;
    for (int k = 0; k < 3; ++k) {
      p.mean[k] = opt_.mean[k];
      p.inv_std[k] = 1.f / opt_.std[k];
    }
    p.pad_value = 114;
    p.format = opt_.letterbox_format;
    gpu::launch_letterbox(reinterpret_cast<const gpu::LetterboxDesc*>(dv + pl.letterbox.off), nout, p, cs);
  }
  // the masks go last on the lane's stream: in place, behind the conversions
  if (ds.nmask > 0) {
    VEP_HIP(hipMemcpyAsync(st.mask_d.p, st.mask_h.p, size_t(ds.nmask) * sizeof(gpu::MaskDesc), hipMemcpyHostToDevice, cs));
    for (int level = 0; level < ds.mask_levels; ++level)
      gpu::launch_mask(st.mask_d.p, st.mask_h.p, ds.nmask, level, cs);
  }
  VEP_HIP(hipEventRecord(st.e1, cs));
}

bool Worker::snapshot_masks(const std::vector<DecodeJob>& jobs, std::vector<MaskSnap>& out) {
  out.resize(jobs.size());
  bool any = false;
  std::lock_guard<std::mutex> g(cams_mu_);
  for (size_t i = 0; i < jobs.size(); ++i) {
    MaskSnap& ms = out[i];
    const auto& cp = cams_[size_t(jobs[i].cam)];
    ms.gen = cp ? cp->mask_gen : 0;
    ms.n = cp ? int(std::min(cp->masks.size(), size_t(mask::kMaxMasks))) : 0;
    for (int k = 0; k < ms.n; ++k) ms.m[k] = cp->masks[size_t(k)];
    any = any || ms.n > 0;
  }
  return any;
}

void Worker::set_privacy_masks(int cam, const std::vector<mask::Mask>& masks) {
  VEP_CHECK(masks.size() <= size_t(mask::kMaxMasks), "mask: at most 8 masks per camera");
  mask::check_list(masks.data(), int(masks.size()));
  {
    std::lock_guard<std::mutex> g(cams_mu_);
    VEP_CHECK(cam >= 0 && size_t(cam) < cams_.size() && cams_[size_t(cam)], "no such camera");
    Camera& c = *cams_[size_t(cam)];
    c.masks = masks;
    ++c.mask_gen;
    // Fail closed: what was published under the old list is no longer readable, and publish()
    // gives up what is in flight (it compares generations under this lock).
    if (c.ring_) c.ring_->invalidate();
  }
  // the detectors' state was learned on other pixels
  motion_reset(cam);
  tamper_reset(cam);
}

std::vector<mask::Mask> Worker::privacy_masks(int cam) {
  std::lock_guard<std::mutex> g(cams_mu_);
  VEP_CHECK(cam >= 0 && size_t(cam) < cams_.size() && cams_[size_t(cam)], "no such camera");
  return cams_[size_t(cam)]->masks;
}

void Worker::run_cpu(std::vector<DecodeJob>& jobs, std::vector<int>& slots,
                     std::vector<u32>& err, const MaskSnap* snaps) {
  err.assign(jobs.size(), 0);
  // one task per camera (a camera's jobs stay in order: they share its surfaces)
  std::vector<std::vector<size_t>> groups;
  std::map<int, size_t> of;
  for (size_t i = 0; i < jobs.size(); ++i) {
    auto it = of.find(jobs[i].cam);
    if (it == of.end()) {
      of[jobs[i].cam] = groups.size();
      groups.push_back({i});
    } else {
      groups[it->second].push_back(i);
    }
  }
  auto run = [&](int g) {
    for (size_t i : groups[size_t(g)]) run_cpu_job(jobs, slots, err, i, snaps ? snaps + i : nullptr);
  };
  if (cpu_pool_ && groups.size() > 1) cpu_pool_->parallel_for(int(groups.size()), run);
  else
    for (int g = 0; g < int(groups.size()); ++g) run(g);
}

void Worker::run_cpu_job(std::vector<DecodeJob>& jobs, std::vector<int>& slots, std::vector<u32>& err, size_t i,
                         const MaskSnap* snap) {
  {
    Camera& c = *cams_[size_t(jobs[i].cam)];
    auto apply_masks = [&](u8* bgr, int w, int h) {  // the slot just converted, before anyone reads it
      if (snap && snap->n > 0) mask::apply_cpu(bgr, size_t(w) * 3, w, h, snap->m, snap->n);
    };
    const PictureInfo& pi = jobs[i].pic;
    for (int sl = pi.spec_lo; sl < pi.spec_hi && !err[i]; ++sl) {  // speculative headers
      const u8* b = jobs[i].upd.block(sl);
      err[i] = (b[-2] != 0x0D || b[-1] != 0x00) ? 1u : 0u;
    }
    if (err[i]) return;
    if (jobs[i].ext) {  // VCN picture (host-visible planes on the CPU backend)
      const vcn::Frame& f = *jobs[i].ext;
      HostSurface& hs = c.surface.host[0];
      VEP_CHECK(f.width <= hs.coded_w && f.height <= hs.coded_h, "VCN picture exceeds the camera surface");
      for (int r = 0; r < f.height; ++r)
        std::memcpy(&hs.y[size_t(r) * size_t(hs.coded_w)], f.y + size_t(r) * f.pitch_y, size_t(f.width));
      for (int r = 0; r < f.height / 2; ++r)
        std::memcpy(&hs.uv[size_t(r) * size_t(hs.coded_w)], f.uv + size_t(r) * f.pitch_uv, size_t(f.width));
    } else if (jobs[i].general()) {
      // frame history: the outputs picture k released are converted before picture k + 1 may
      // reuse their surfaces (cpu_nv12_to_bgr narrows u16 / 4:2:2 surfaces itself)
      auto convert_history = [&](size_t k) {
        for (const JobOutput& o : jobs[i].outputs)
          if (o.ring_slot >= 0 && size_t(o.released_by) == k) {
            cpu_nv12_to_bgr(c.surface.host[size_t(o.slot)], o.pic.crop_left, o.pic.crop_top, o.pic.width, o.pic.height,
                            c.ring_->slot_ptr(o.ring_slot));
            apply_masks(c.ring_->slot_ptr(o.ring_slot), o.pic.width, o.pic.height);
          }
      };
      for (size_t k = 0; k < jobs[i].avc.size(); ++k) {
        const auto& pic = jobs[i].avc[k];
        if (!pic->structure) {
          avc::cpu_reconstruct(*pic, c.surface.host);
          convert_history(k);
          continue;
        }
        auto& F = c.surface.fields;  // field slots (half-height surfaces)
        if (F.size() < size_t(pic->dpb_slots)) F.resize(size_t(pic->dpb_slots));
        for (auto& h : F)
          if (h.coded_w != pic->wmbs * 16 || h.coded_h != pic->hmbs * 16 || h.bd != pic->bd || h.cf != pic->cf)
            h.alloc(pic->wmbs * 16, pic->hmbs * 16, pic->bd, pic->cf);
        avc::cpu_reconstruct(*pic, F);
      }
      for (size_t k = 0; k < jobs[i].hevc.size(); ++k) {
        hevc::cpu_execute(*jobs[i].hevc[k], c.surface.host);
        convert_history(k);
      }
    } else {
      cpu_apply_update(jobs[i].upd, c.surface.host[0]);
    }
    if (!jobs[i].has_output()) return;
    HostSurface narrow;  // Main10: the 8-bit copy the conversion and the letterbox read
    HostSurface woven;   // a field pair's frame
    if (jobs[i].out_fields) {
      const size_t t = size_t(jobs[i].target());
      VEP_CHECK(2 * t + 1 < c.surface.fields.size(), "field pair output without its fields");
      avc::weave_fields(c.surface.fields[2 * t], c.surface.fields[2 * t + 1], woven);
    }
    const HostSurface& out = jobs[i].out_fields ? woven : c.surface.host[size_t(jobs[i].target())];
    const bool conv = out.wide() || out.cf == 2;
    if (conv) narrow_surface(out, narrow);
    const HostSurface& src = conv ? narrow : out;
    cpu_nv12_to_bgr(src, jobs[i].pic.crop_left, jobs[i].pic.crop_top,
                    jobs[i].pic.width, jobs[i].pic.height, c.ring_->slot_ptr(slots[i]));
    apply_masks(c.ring_->slot_ptr(slots[i]), jobs[i].pic.width, jobs[i].pic.height);
    if (opt_.ref_copies) {  // read_image.py:97 tobytes() + :119 SerializeToString()
      const size_t n = size_t(jobs[i].pic.width) * size_t(jobs[i].pic.height) * 3;
      std::vector<u8> bytes(c.ring_->slot_ptr(slots[i]), c.ring_->slot_ptr(slots[i]) + n);
      FrameMeta m{};
      m.width = jobs[i].pic.width;
      m.height = jobs[i].pic.height;
      m.pts = jobs[i].meta.pts;
      const auto pre_suf = encode_video_frame(m, n, c.name());
      std::string msg;
      msg.reserve(pre_suf.first.size() + n + pre_suf.second.size());
      msg += pre_suf.first;
      msg.append(reinterpret_cast<const char*>(bytes.data()), n);
      msg += pre_suf.second;
      ref_copy_bytes_.fetch_add(msg.size(), std::memory_order_relaxed);
    }
    if (opt_.letterbox_size > 0) {
      gpu::LetterboxDesc l{};
      const size_t S = size_t(opt_.letterbox_size);
      l.src_w = jobs[i].pic.width;
      l.src_h = jobs[i].pic.height;
      l.crop_left = jobs[i].pic.crop_left;
      l.crop_top = jobs[i].pic.crop_top;
      const bool nv12 = opt_.letterbox_format == gpu::kLbNV12;
      l.out_hwc = cons_hwc_ ? cons_hwc_ + size_t(jobs[i].cam) *
                                              gpu::letterbox_bytes(int(S), opt_.letterbox_format)
                            : nullptr;
      const size_t es = opt_.chw_dtype == gpu::kChwF32 ? 4 : 2;
      l.out_chw = (cons_chw_ && opt_.chw_dtype != gpu::kChwNone)
                      ? static_cast<u8*>(cons_chw_) + size_t(jobs[i].cam) * 3 * S * S * es
                      : nullptr;
      gpu::fill_letterbox_geometry(l, opt_.letterbox_size, nv12);
      if (nv12) {
        cpu_letterbox_nv12(src, l, opt_.letterbox_size, 114);
        return;
      }
      gpu::LetterboxParams p{};
      p.size = opt_.letterbox_size;
      p.chw_dtype = opt_.chw_dtype;
      for (int k = 0; k < 3; ++k) {
        p.mean[k] = opt_.mean[k];
        p.inv_std[k] = 1.f / opt_.std[k];
      }
      p.pad_value = 114;
      cpu_letterbox(src, l, p);
    }
  }
}

// Worker thread, per finished job of a camera: records the job's dropped pictures / poisoned
// CRAs and tells whether its output is one of the recorded stale pictures (each is output once:
// the entry is erased) or a RASL picture of a poisoned CRA.
bool stale_output(Camera& c, const DecodeJob& j, bool check) {
  const u64 now = ++c.jobs_seen_;
  for (const auto& d : j.dropped) c.stale_.push_back({d.first, d.second, now + Camera::kStaleJobs});
  for (i64 tag : j.poisoned_cra) c.bad_cra_.emplace_back(tag, now + Camera::kStaleJobs);
  c.stale_.erase(std::remove_if(c.stale_.begin(), c.stale_.end(), [&](const Camera::StaleOut& s) { return s.until < now; }),
                 c.stale_.end());
  c.bad_cra_.erase(std::remove_if(c.bad_cra_.begin(), c.bad_cra_.end(), [&](const auto& b) { return b.second < now; }),
                   c.bad_cra_.end());
  if (c.stale_.size() > 64) c.stale_.erase(c.stale_.begin(), c.stale_.end() - 64);
  if (!check) return false;
  return stale_picture(c, j.out_slot, j.meta.pts, j.out_rasl_of);
}

// Whether the output (slot, pts) is one of the camera's recorded stale pictures (erased: each is
// output once) or a RASL picture of a poisoned CRA.
bool stale_picture(Camera& c, int slot, i64 pts, i64 rasl_of) {
  for (auto it = c.stale_.begin(); it != c.stale_.end(); ++it)
    if (it->slot == slot && it->pts == pts) {
      c.stale_.erase(it);
      return true;
    }
  if (rasl_of >= 0)
    for (const auto& b : c.bad_cra_)
      if (b.first == rasl_of) return true;
  return false;
}

void Worker::publish(std::vector<DecodeJob>& jobs, std::vector<int>& slots, const u32* err, const MaskSnap* snaps) {
  trace::Range tr("vep.publish");
  const i64 t = mono_us();
  const i64 wall = now_ms();
  std::lock_guard<std::mutex> g(cams_mu_);
  for (size_t i = 0; i < jobs.size(); ++i) {
    auto& cp = cams_[size_t(jobs[i].cam)];
    const bool out = jobs[i].has_output();
    if (!cp || !cp->ring_) {
      if (out) dropped_.fetch_add(1, std::memory_order_relaxed);
      continue;
    }
    if (!(err && err[i]) && !cp->broken_) {
      // decoded frames (a field pair counts once: its second field)
      u64 np = jobs[i].general() ? jobs[i].hevc.size() : 1;
      for (const auto& p : jobs[i].avc) np += !p->structure || p->second_field;
      pictures_.fetch_add(np, std::memory_order_relaxed);
      cp->pictures.fetch_add(np, std::memory_order_relaxed);
    }
    const bool stale = stale_output(*cp, jobs[i], out && jobs[i].general());
    // Privacy masks, fail closed: a frame converted under another list than the camera's current
    // one is not committed (set_privacy_masks bumps mask_gen under this lock).
    const bool mask_stale = snaps && snaps[i].gen != cp->mask_gen;
    const bool masked = snaps && snaps[i].n > 0;
    auto mask_drop = [&](int slot) {
      cp->ring_->abort(slot);
      cp->mask_dropped.fetch_add(1, std::memory_order_relaxed);
      dropped_.fetch_add(1, std::memory_order_relaxed);
    };
    // Frame history: the job's earlier outputs, oldest first, each under the rules of the newest
    // one below: none from a failed job or while the camera waits for a keyframe (a refresh job's
    // own pictures excepted), none that is stale. The hook fires once per job (here only when the
    // newest frame is not committed below).
    bool hist_committed = false;
    for (JobOutput& o : jobs[i].outputs) {
      if (o.ring_slot < 0) continue;
      const bool ok = !(err && err[i]) && (!cp->broken_ || (jobs[i].refresh && reconstructs_slot(jobs[i], o.slot)));
      if (!ok) {
        cp->ring_->abort(o.ring_slot);
        dropped_.fetch_add(1, std::memory_order_relaxed);
      } else if (stale_picture(*cp, o.slot, o.meta.pts, o.rasl_of)) {
        cp->ring_->abort(o.ring_slot);
        shed_.fetch_add(1, std::memory_order_relaxed);
        cp->shed.fetch_add(1, std::memory_order_relaxed);
      } else if (mask_stale) {
        mask_drop(o.ring_slot);
      } else {
        o.meta.decoded_us = t;
        cp->ring_->commit(o.ring_slot, o.meta);
        if (masked) cp->masked_frames.fetch_add(1, std::memory_order_relaxed);
        cp->decoded.fetch_add(1, std::memory_order_relaxed);
        frames_.fetch_add(1, std::memory_order_relaxed);
        hist_committed = true;
      }
      o.ring_slot = -1;
    }
    struct HookOnce {  // (the paths below that do not commit the newest frame leave through here)
      Worker& w;
      Camera& c;
      int cam;
      bool armed;
      ~HookOnce() {
        if (!armed) return;
        if (auto hook = std::atomic_load(&w.publish_hook_)) (*hook)(cam, c.ring_->published());
      }
    } hook_once{*this, *cp, jobs[i].cam, hist_committed};
    if (!out) {  // reconstruction only (its pictures wait in the reorder buffer)
      if (err && err[i]) {
        cp->errors.fetch_add(1, std::memory_order_relaxed);
        cp->logs.add(true, "GPU reconstruction wavefront timed out; waiting for the next keyframe");
        cp->broken_ = true;
      } else if (jobs[i].refresh) {
        cp->broken_ = false;  // a keyframe reconstructed (its picture is published later)
      }
      continue;
    }
    if (err && err[i]) {
      dropped_.fetch_add(1, std::memory_order_relaxed);
      cp->errors.fetch_add(1, std::memory_order_relaxed);
      // err bit 0: a speculatively placed I_PCM block failed its header check (decode_convert);
      // bit 1: a reconstruction wavefront timed out waiting for a neighbour (gpu_avc.hip)
      if (err[i] & 2u)
        cp->logs.add(true, "GPU reconstruction wavefront timed out; frame dropped, waiting for the next keyframe");
      if (err[i] & 0xFF00u) {  // (gpu_avc.hip / gpu_avc_hbd.hip bound checks)
        char b[96];
        std::snprintf(b, sizeof b, "GPU reconstruction bound check failed (0x%x); frame dropped", err[i]);
        cp->logs.add(true, b);
        std::fprintf(stderr, "vep: camera %s: %s\n", cp->name().c_str(), b);
      } else if (err[i] & ~2u) {
        cp->logs.add(true, "corrupt keyframe: I_PCM header check failed; waiting for the next keyframe");
      }
      cp->broken_ = true;
      cp->ring_->abort(slots[i]);
      continue;
    }
    if (cp->broken_) {  // surfaces are garbage until a keyframe rewrites every MB
      if (!jobs[i].refresh) {
        cp->ring_->abort(slots[i]);
        dropped_.fetch_add(1, std::memory_order_relaxed);
        continue;
      }
      cp->broken_ = false;
    }
    if (stale) {  // its reconstruction was dropped with a backlog (or predicts from one): a stale surface
      cp->ring_->abort(slots[i]);
      shed_.fetch_add(1, std::memory_order_relaxed);
      cp->shed.fetch_add(1, std::memory_order_relaxed);
      continue;
    }
    if (mask_stale) {
      mask_drop(slots[i]);
      continue;
    }
    jobs[i].meta.decoded_us = t;
    if (jobs[i].meta.arrival_ms > 0) {
      const i64 lat = std::max<i64>(0, wall - jobs[i].meta.arrival_ms);
      int b = 0;
      while (b < Camera::kLatBuckets - 1 && double(lat) > Camera::kLatBucketsMs[b]) ++b;
      cp->lat_hist[b].fetch_add(1, std::memory_order_relaxed);
      cp->lat_sum_ms.fetch_add(u64(lat), std::memory_order_relaxed);
    }
    cp->ring_->commit(slots[i], jobs[i].meta);
    if (masked) cp->masked_frames.fetch_add(1, std::memory_order_relaxed);
    cp->out_surface_slot = jobs[i].general() && !jobs[i].out_fields ? jobs[i].target() : -1;
    cp->out_surface_pts = jobs[i].meta.pts;
    cp->decoded.fetch_add(1, std::memory_order_relaxed);
    frames_.fetch_add(1, std::memory_order_relaxed);
    hook_once.armed = false;
    if (auto hook = std::atomic_load(&publish_hook_)) (*hook)(jobs[i].cam, cp->ring_->published());
  }
  batches_.fetch_add(1);
}

void Worker::set_publish_hook(std::function<void(int, i64)> f) {
  std::shared_ptr<std::function<void(int, i64)>> h;
  if (f) h = std::make_shared<std::function<void(int, i64)>>(std::move(f));
  std::lock_guard<std::mutex> g(cams_mu_);  // (publish holds it: no hook call is in flight after this)
  std::atomic_store(&publish_hook_, h);
}

double Worker::gpu_ms_total() const {
  double m = 0;
  for (const auto& lp : lanes_) m = std::max(m, lp->gpu_ms.load());
  return m;
}

void Worker::add_time(double Timers::*f, double us) {
  std::lock_guard<std::mutex> g(timers_mu_);
  timers.*f += us;
}

// Wait for a batch's completion event without spinning a CPU core. hipEventSynchronize busy-polls
// the HSA completion signal (rdtsc loop in libhsa-runtime64) even for hipEventBlockingSync events
// for a while before it sleeps: in the host profile of the headline that spin was 17% of the
// process's CPU samples, taken from the parse threads. A lane only needs to notice its stage is
// free within a fraction of a batch (~5 ms), so it polls the event and sleeps between polls.
static void wait_event_polite(hipEvent_t e) {
  for (int i = 0;; ++i) {
    const hipError_t r = hipEventQuery(e);
    if (r == hipSuccess) return;
    if (r != hipErrorNotReady) VEP_HIP(r);
    if (i < 2) std::this_thread::yield();
    else std::this_thread::sleep_for(std::chrono::microseconds(40));
  }
}

void Worker::complete(Lane& ln, Stage& st) {
  if (!st.active) return;
  st.active = false;
  const i64 t0 = mono_us();
  {
    trace::Range tr("vep.wait_gpu");
    if (polite_wait_) wait_event_polite(st.e1);
    else VEP_HIP(hipEventSynchronize(st.e1));
  }
  add_time(&Timers::wait, double(mono_us() - t0));
  float ms = 0;
  if (hipEventElapsedTime(&ms, st.e0, st.e1) == hipSuccess) ln.gpu_ms.store(ln.gpu_ms.load() + ms);
  publish(st.jobs, st.slots, st.err.p, st.mask_snap.size() == st.jobs.size() ? st.mask_snap.data() : nullptr);
  st.jobs.clear();
  st.slots.clear();
  {
    std::lock_guard<std::mutex> g(pub_mu_);
    while (!ln.unpublished.empty() && ln.unpublished.front() >= st.seq && ln.unpublished.front() <= st.seq_last)
      ln.unpublished.pop_front();
  }
  pub_cv_.notify_all();
}

void Worker::launch_on(Lane& ln, Batch&& b) {
  Stage& st = ln.stage[size_t(ln.next)];
  ln.next = (ln.next + 1) % int(ln.stage.size());
  complete(ln, st);  // this lane's oldest batch (`stages` launches ago): its staging is reused
  st.jobs.swap(b.jobs);
  st.slots.swap(b.slots);
  st.seq = b.seq;
  st.seq_last = std::max(b.seq, b.seq_last);
  st.cons_hwc = b.cons_hwc;
  st.cons_chw = b.cons_chw;
  st.cons_rows = b.cons_rows;
  try {
    std::shared_lock<std::shared_mutex> gate(cons_gate_);
    const u64 sg = snap_gen_.load();
    if (ln.snap_seen != sg) {  // this batch's letterbox writes wait for the last snapshot's copy
      VEP_HIP(hipStreamWaitEvent(ln.stream, snap_ev_, 0));
      ln.snap_seen = sg;
    }
    launch_gpu(ln, st);
  } catch (...) {
    // the batch is dropped: give its ring slots back and count it as published
    {
      std::lock_guard<std::mutex> g(cams_mu_);
      for (size_t i = 0; i < st.jobs.size(); ++i) {
        auto& cp = cams_[size_t(st.jobs[i].cam)];
        if (cp && cp->ring_ && st.slots[i] >= 0) cp->ring_->abort(st.slots[i]);
        for (JobOutput& o : st.jobs[i].outputs)
          if (cp && cp->ring_ && o.ring_slot >= 0) cp->ring_->abort(o.ring_slot);
      }
      for (const auto& j : st.jobs) dropped_.fetch_add(j.has_output() ? 1 : 0, std::memory_order_relaxed);
    }
    st.jobs.clear();
    st.slots.clear();
    {
      std::lock_guard<std::mutex> g(pub_mu_);
      while (!ln.unpublished.empty() && ln.unpublished.front() >= st.seq && ln.unpublished.front() <= st.seq_last)
        ln.unpublished.pop_front();
    }
    pub_cv_.notify_all();
    throw;
  }
  st.active = true;
}

// Batches that queued behind this lane's in-flight ones (ln.mu held) join `b`: one launch per
// kernel for all of them. The wavefront kernels (intra, deblock) take about the same time for
// one picture as for many (a picture's latency is its MB-row chain, and a launch of one picture
// fills a few CUs of 256), and the batches would run back to back on the lane's stream anyway,
// so merging turns queueing into parallel work without holding anything back: nothing waits
// for a merge, only what is already waiting is merged. A camera appears at most once per launch
// (its pictures inside one job are rounds; two jobs of one camera in one launch would put
// dependent pictures in the same round), so the merge stops at a batch that repeats a camera,
// at a different consumer batch, or at merge_jobs_ jobs.
void Worker::merge_queued(Lane& ln, Batch& b) {
  if (merge_jobs_ <= 0) return;
  while (!ln.q.empty()) {
    Batch& n = ln.q.front();
    if (n.cons_hwc != b.cons_hwc || n.cons_chw != b.cons_chw || n.cons_rows != b.cons_rows) break;
    if (int(b.jobs.size() + n.jobs.size()) > merge_jobs_) break;
    bool repeat = false;
    for (const DecodeJob& j : n.jobs) {
      for (const DecodeJob& k : b.jobs)
        if (k.cam == j.cam) {
          repeat = true;
          break;
        }
      if (repeat) break;
    }
    if (repeat) break;
    for (size_t i = 0; i < n.jobs.size(); ++i) {
      b.jobs.push_back(std::move(n.jobs[i]));
      b.slots.push_back(n.slots[i]);
    }
    b.seq_last = std::max(n.seq, n.seq_last);
    ln.q.pop_front();
    merged_.fetch_add(1, std::memory_order_relaxed);
  }
}

// Launcher thread of one lane: launches the batches handed over by launch_async, each after
// its staging buffer's previous batch is complete and published, so a lane waiting on a slow
// batch (a keyframe's intra wavefront) never holds back the other lanes.
void Worker::lane_loop(Lane& ln) {
  dev_.bind();
  auto keep_error = [&] {
    std::lock_guard<std::mutex> g(pub_mu_);
    if (!lane_err_) lane_err_ = std::current_exception();
  };
  std::unique_lock<std::mutex> lk(ln.mu);
  for (;;) {
    ln.cv.wait(lk, [&] { return ln.stop || ln.drain || (!ln.q.empty() && !hold_.load()); });
    if (!ln.q.empty() && (!hold_.load() || ln.drain || ln.stop)) {
      Batch b = std::move(ln.q.front());
      ln.q.pop_front();
      merge_queued(ln, b);
      ln.busy = true;
      lk.unlock();
      ln.cv.notify_all();  // room for the next batch
      try {
        launch_on(ln, std::move(b));
      } catch (...) {
        keep_error();
      }
      lk.lock();
      ln.busy = false;
      ln.cv.notify_all();
      continue;
    }
    if (ln.drain) {
      lk.unlock();
      try {
        for (size_t k = 0; k < ln.stage.size(); ++k)
          complete(ln, ln.stage[(size_t(ln.next) + k) % ln.stage.size()]);
      } catch (...) {
        keep_error();
      }
      lk.lock();
      ln.drain = false;
      ln.cv.notify_all();
      continue;
    }
    if (ln.stop) return;
  }
}

void Worker::hold_lanes(bool hold) {
  hold_.store(hold);
  for (auto& lp : lanes_) {
    std::lock_guard<std::mutex> g(lp->mu);  // (a launcher between its predicate check and its wait)
  }
  for (auto& lp : lanes_) lp->cv.notify_all();
}

void Worker::drain_lanes() {
  for (auto& lp : lanes_) {
    std::lock_guard<std::mutex> g(lp->mu);
    lp->drain = true;
  }
  for (auto& lp : lanes_) lp->cv.notify_all();
  for (auto& lp : lanes_) {
    Lane& ln = *lp;
    std::unique_lock<std::mutex> lk(ln.mu);
    ln.cv.wait(lk, [&] { return !ln.drain && ln.q.empty() && !ln.busy; });
  }
  std::exception_ptr e;
  {
    std::lock_guard<std::mutex> g(pub_mu_);
    std::swap(e, lane_err_);
  }
  if (e) std::rethrow_exception(e);
}

void Worker::complete_locked() {
  if (threaded_) {
    drain_lanes();
    return;
  }
  // oldest first: Lane::next names the stage that will be reused next, i.e. the oldest batch
  for (auto& lp : lanes_)
    for (size_t k = 0; k < lp->stage.size(); ++k)
      complete(*lp, lp->stage[(size_t(lp->next) + k) % lp->stage.size()]);
}

void Worker::complete_all() {
  std::lock_guard<std::mutex> lg(launch_mu_);
  if (dev_.gpu()) dev_.bind();
  complete_locked();
}

void Worker::wait_published(u64 seq) {
  std::unique_lock<std::mutex> g(pub_mu_);
  pub_cv_.wait(g, [&] {
    for (const auto& lp : lanes_)
      if (!lp->unpublished.empty() && lp->unpublished.front() <= seq) return false;
    return true;
  });
}

void Worker::launch_async(std::vector<DecodeJob>& jobs) {
  trace::Range tr("vep.launch_async");
  if (jobs.empty()) return;
  std::lock_guard<std::mutex> lg(launch_mu_);
  dev_.bind();
  std::vector<int> slots;
  const i64 t0 = mono_us();
  prepare(jobs, slots);
  add_time(&Timers::prepare, double(mono_us() - t0));
  if (jobs.empty()) return;
  if (!dev_.gpu()) {
    std::vector<u32> err;
    std::vector<MaskSnap> snaps;
    snapshot_masks(jobs, snaps);
    run_cpu(jobs, slots, err, snaps.data());
    publish(jobs, slots, err.data(), snaps.data());
    jobs.clear();
    return;
  }
  const size_t nl = lanes_.size();
  std::vector<std::vector<DecodeJob>> lj(nl);
  std::vector<std::vector<int>> ls(nl);
  for (size_t i = 0; i < jobs.size(); ++i) {
    const size_t g = size_t(jobs[i].cam) % nl;  // a camera's surfaces are ordered by its lane
    lj[g].push_back(std::move(jobs[i]));
    ls[g].push_back(slots[i]);
  }
  jobs.clear();
  const u64 seq = ++launch_seq_;
  for (size_t g = 0; g < nl; ++g) {
    if (lj[g].empty()) continue;
    Lane& ln = *lanes_[g];
    {
      std::lock_guard<std::mutex> pg(pub_mu_);
      ln.unpublished.push_back(seq);
    }
    Batch b{std::move(lj[g]), std::move(ls[g]), seq, seq, cons_hwc_, cons_chw_, cons_rows_};
    if (!threaded_) {
      launch_on(ln, std::move(b));
      continue;
    }
    std::unique_lock<std::mutex> lk(ln.mu);
    ln.cv.wait(lk, [&] { return int(ln.q.size()) < queue_; });  // bounded per-lane backlog
    ln.q.push_back(std::move(b));
    lk.unlock();
    ln.cv.notify_all();
  }
  if (threaded_) {
    std::exception_ptr e;
    {
      std::lock_guard<std::mutex> g(pub_mu_);
      std::swap(e, lane_err_);
    }
    if (e) std::rethrow_exception(e);
  }
}

std::vector<u64> Worker::avc_profile() {
  std::vector<u64> v(gpu::kAvcProfSlots, 0);
  if (!avc_prof_) return v;
  complete_all();
  VEP_HIP(hipMemcpy(v.data(), avc_prof_, v.size() * sizeof(u64), hipMemcpyDeviceToHost));
  return v;
}

void Worker::run_batch(std::vector<DecodeJob>& jobs) {
  launch_async(jobs);
  complete_all();
}

size_t Worker::snapshot_consumer(void* dst, size_t cap, int rows, hipStream_t stream) {
  VEP_CHECK(opt_.letterbox_size > 0 && cons_hwc_, "consumer batch disabled (letterbox_size is 0)");
  rows = std::clamp(rows, 0, cons_rows_);
  const size_t n = size_t(rows) * gpu::letterbox_bytes(opt_.letterbox_size, opt_.letterbox_format);
  VEP_CHECK(cap >= n, "snapshot_consumer destination too small");
  if (!n) return 0;
  if (!dev_.gpu()) {  // CPU backend: rows are written by launch_async (under launch_mu_)
    std::lock_guard<std::mutex> g(launch_mu_);
    std::memcpy(dst, cons_hwc_, n);
    snap_gen_.fetch_add(1);
    return n;
  }
  std::unique_lock<std::shared_mutex> gate(cons_gate_);  // no lane enqueues meanwhile
  dev_.bind();
  if (!snap_ev_) {
    VEP_HIP(hipEventCreateWithFlags(&snap_ev_, hipEventDisableTiming));
    for (auto& lp : lanes_) VEP_HIP(hipEventCreateWithFlags(&lp->snap_mark, hipEventDisableTiming));
  }
  const hipStream_t s = stream ? stream : serve_stream_;
  for (auto& lp : lanes_) {  // after every letterbox write enqueued so far
    VEP_HIP(hipEventRecord(lp->snap_mark, lp->stream));
    VEP_HIP(hipStreamWaitEvent(s, lp->snap_mark, 0));
  }
  VEP_HIP(hipMemcpyAsync(dst, cons_hwc_, n, hipMemcpyDeviceToDevice, s));
  VEP_HIP(hipEventRecord(snap_ev_, s));  // ... and before any later one (launch_on waits on it)
  snap_gen_.fetch_add(1);
  if (!stream) VEP_HIP(hipStreamSynchronize(s));
  return n;
}

}  // namespace vep
