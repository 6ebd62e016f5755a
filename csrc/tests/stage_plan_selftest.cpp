// Stand-alone check of the stage plan's invariants (vep/stage_plan.h), host only: real jobs from
// the synthetic encoders, built by the cameras of a CPU-backend Worker (device -1), are planned
// and every batch's layout, transfers and rounds are checked. `make plan-selftest` links it
// against the objects csrc/build.py made (default CPU suite); `make asan-plan` builds it from
// sources under AddressSanitizer + UndefinedBehaviorSanitizer. Exit status 0 and no sanitizer
// report = pass.
#include <algorithm>
#include <cstdio>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "vep/runtime.h"
#include "vep/stage_plan.h"
#include "vep/synth.h"

using namespace vep;

static int failures = 0;
static std::string batch_name;

static void check(bool ok, const char* what) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s: %s\n", batch_name.c_str(), what);
  ++failures;
}

constexpr int kWholeRound = 1 << 20;  // the window that holds every level of a round

static void check_plan(const std::vector<DecodeJob>& jobs, const StagePlan& pl) {
  using E = StagePlan::Entry;
  // regions: inside the buffer, aligned, disjoint, in their section
  size_t payload_end = pl.header_bytes, first_scratch = pl.need;
  for (const E& e : pl.entries) {
    check(e.off + e.room <= pl.need && e.bytes <= e.room, "a region lies outside [0, need)");
    check(e.align >= 16 && e.off % e.align == 0 && e.off % 16 == 0, "a region's offset is not aligned");
    if (e.kind == StagePlan::kPayload) payload_end = std::max(payload_end, e.off + e.room);
    if (e.kind == StagePlan::kScratch) first_scratch = std::min(first_scratch, e.off);
  }
  check(pl.header_bytes % 256 == 0 && pl.need % 256 == 0 && pl.header_bytes <= pl.need, "section bounds");
  for (const E& e : pl.entries) {
    if (e.kind == StagePlan::kBuilt || e.kind == StagePlan::kRecord)
      check(e.off + e.room <= pl.header_bytes, "a built / record region is not carried by the header copy");
    if (e.kind == StagePlan::kPayload)
      check(e.off >= pl.header_bytes && e.off + e.room <= first_scratch, "payload outside its section");
    if (e.kind == StagePlan::kScratch) check(e.off >= payload_end, "scratch below the payload");
    check((e.kind == StagePlan::kBuilt || e.kind == StagePlan::kScratch) ? !e.copy && !e.gather && !e.src : true,
          "a built / scratch region has a transfer");
  }
  std::vector<std::pair<size_t, size_t>> spans;
  for (const E& e : pl.entries)
    if (e.room > 0) spans.push_back({e.off, e.off + e.room});
  std::sort(spans.begin(), spans.end());
  for (size_t k = 1; k < spans.size(); ++k) check(spans[k].first >= spans[k - 1].second, "two regions overlap");
  // transfers: the tasks / chunks of a region tile it exactly, in region order
  size_t t = 0, c = 0;
  u64 gathered = 0;
  for (const E& e : pl.entries) {
    if (e.copy) {
      check(e.src != nullptr || e.bytes == 0, "a copied region without source");
      for (size_t o = 0; o < e.bytes;) {
        if (t >= pl.tasks.size()) {
          check(false, "copy tasks end inside a region");
          break;
        }
        const StagePlan::CopyTask& k = pl.tasks[t++];
        check(k.dst == e.off + o && k.src == e.src + o && k.len > 0 && k.len <= kPackChunk && o + k.len <= e.bytes,
              "a copy task does not continue its region");
        o += std::max<size_t>(k.len, 1);
      }
    }
    if (e.gather) {
      check(e.kind == StagePlan::kPayload || e.dev != nullptr, "a gathered record without device address");
      for (size_t o = 0; o < e.bytes;) {
        if (c >= pl.chunks.size()) {
          check(false, "gather chunks end inside a region");
          break;
        }
        const StagePlan::Chunk& k = pl.chunks[c++];
        check(k.dst == e.off + o && k.src == (e.dev ? e.dev + o : nullptr) && k.len > 0 && k.len <= gpu::kGatherChunk &&
                  o + k.len <= e.bytes,
              "a gather chunk does not continue its region");
        o += std::max<size_t>(k.len, 1);
      }
      if (e.kind == StagePlan::kRecord) gathered += e.bytes;
    }
    check(!(e.copy && e.gather) || e.kind == StagePlan::kPayload, "a record both copied and gathered");
    if (e.kind == StagePlan::kPayload) check(e.copy == (e.dev == nullptr) && e.gather == !pl.set.direct, "payload policy");
  }
  check(t == pl.tasks.size(), "copy tasks outside every region");
  check(c == pl.chunks.size() && pl.chunks.size() == pl.planned_chunks, "planned chunk count differs from the chunks");
  check(pl.gather.bytes == pl.planned_chunks * sizeof(gpu::GatherChunk), "gather region size");
  check(gathered == pl.bytes_gathered, "gathered byte count");
  // rounds: round r lists exactly the pictures of the jobs with more than r pictures, in job order
  size_t navc = 0, nhevc = 0;
  for (size_t r = 0; r < pl.avc_rounds.size(); ++r) {
    size_t k = 0;
    for (size_t i = 0; i < jobs.size(); ++i) {
      if (jobs[i].avc.size() <= r) continue;
      const bool ok = k < pl.avc_rounds[r].pics.size() && pl.avc[size_t(pl.avc_rounds[r].pics[k])].job == int(i) &&
                      pl.avc[size_t(pl.avc_rounds[r].pics[k])].p == jobs[i].avc[r].get();
      check(ok, "an H.264 round misses a picture");
      ++k;
    }
    check(k == pl.avc_rounds[r].pics.size() && k > 0, "an H.264 round lists a foreign picture");
    check(pl.avc_rounds[r].descs.bytes == k * sizeof(gpu::AvcDesc), "AvcDesc array size");
    navc += k;
  }
  for (size_t r = 0; r < pl.hevc_rounds.size(); ++r) {
    const StagePlan::HevcRound& rd = pl.hevc_rounds[r];
    size_t k = 0;
    int l0 = 0, intra = 0;
    for (size_t i = 0; i < jobs.size(); ++i) {
      if (jobs[i].hevc.size() <= r) continue;
      const bool ok = k < rd.pics.size() && pl.hevc[size_t(rd.pics[k])].job == int(i) &&
                      pl.hevc[size_t(rd.pics[k])].p == jobs[i].hevc[r].get();
      check(ok, "an H.265 round misses a picture");
      const hevc::GpuPicture& p = *jobs[i].hevc[r];
      if (p.level_begin.size() >= 2) {
        l0 += int(p.level_begin[1] - p.level_begin[0]);
        intra += int(p.tus.size()) - int(p.level_begin[1]);
      }
      ++k;
    }
    check(k == rd.pics.size() && k > 0, "an H.265 round lists a foreign picture");
    check(rd.l0_blocks == l0 && rd.intra_blocks == intra, "TU blocks of a round");
    check(int(rd.tu_ranges.size()) == rd.l0_ranges + rd.intra_ranges, "TU range count");
    int next = 0, sum = 0;  // intra tickets: the ranges, the levels and the windows each cover 0 .. intra_blocks once
    for (int q = rd.l0_ranges; q < int(rd.tu_ranges.size()); ++q) {
      check(rd.tu_ranges[size_t(q)].begin == next && rd.tu_ranges[size_t(q)].count > 0, "intra ranges are not consecutive");
      next += rd.tu_ranges[size_t(q)].count;
    }
    check(next == rd.intra_blocks, "intra ranges do not cover the tickets");
    for (const StagePlan::Span& s : rd.levels) {
      check(s.first == sum, "levels are not consecutive");
      sum += s.count;
    }
    check(sum == rd.intra_blocks, "levels do not cover the tickets");
    sum = 0;
    for (const StagePlan::Span& s : rd.windows) {
      check(s.first == sum && s.count > 0, "windows are not consecutive");
      sum += s.count;
    }
    check(pl.set.tu_window > 0 ? sum == rd.intra_blocks : rd.windows.empty(), "windows do not cover the tickets");
    if (pl.set.tu_window >= kWholeRound) check(rd.windows.size() <= 1, "the whole-round window is one launch");
    sum = 0;
    for (const gpu::HevcTuRange& q : rd.pic_queues) sum += q.count;
    check(pl.set.tu_window < 0 ? sum == rd.intra_blocks : rd.pic_queues.empty(), "picture queues do not cover the blocks");
    check(rd.counters.bytes == rd.windows.size() * sizeof(u32), "ticket counter region");
    nhevc += k;
  }
  check(navc == pl.avc.size() && nhevc == pl.hevc.size(), "a picture outside every round");
  // history: every output with a ring slot in exactly one round, the one that releases it
  std::set<std::pair<int, int>> seen;
  int next = 0;
  auto span = [&](const StagePlan::HistSpan& hs, bool avc, size_t r) {
    if (hs.count == 0) return;
    check(hs.first == next, "history spans are not consecutive");
    int tiles = 0;
    for (int k = hs.first; k < hs.first + hs.count && k < int(pl.hist.size()); ++k) {
      const StagePlan::HistOut& h = pl.hist[size_t(k)];
      const DecodeJob& j = jobs[size_t(h.job)];
      const JobOutput& o = j.outputs[size_t(h.out)];
      check(o.ring_slot >= 0 && size_t(o.released_by) == r && j.avc.empty() != avc, "a history output in a foreign round");
      check(seen.insert({h.job, h.out}).second, "a history output twice");
      check(h.tile_begin == tiles, "history tile prefix");
      tiles += gpu::tiles_for(o.pic.coded_width / 16, o.pic.coded_height / 16);
    }
    check(tiles == hs.tiles, "history tiles of a round");
    next += hs.count;
  };
  for (size_t r = 0; r < pl.avc_rounds.size(); ++r) span(pl.avc_rounds[r].hist, true, r);
  for (size_t r = 0; r < pl.hevc_rounds.size(); ++r) span(pl.hevc_rounds[r].hist, false, r);
  size_t want = 0;
  for (const DecodeJob& j : jobs)
    for (const JobOutput& o : j.outputs) want += o.ring_slot >= 0 ? 1 : 0;
  check(size_t(next) == pl.hist.size() && seen.size() == want && pl.hist.size() == want, "a history output in no round");
  check(pl.history.bytes == want * sizeof(gpu::SurfaceBgrDesc), "history region size");
  check(pl.outs.size() == size_t(std::count_if(jobs.begin(), jobs.end(), [](const DecodeJob& j) { return j.has_output(); })),
        "output list");
}

static void plan_and_check(const char* name, const std::vector<DecodeJob>& jobs, bool direct, int window) {
  batch_name = std::string(name) + (direct ? " direct" : " gather") + " window " + std::to_string(window);
  const StagePlan pl(jobs, {direct, window});
  check_plan(jobs, pl);
}

// One camera and its stream: job(n) = the next n access units as one (catch-up) job, its history
// outputs given ring slots as Worker::prepare would.
struct Source {
  Source(Worker& w, const SynthConfig& cfg, const char* name, int history)
      : enc(cfg), cam(w.camera(w.add_camera(name, 4, history))) {}
  DecodeJob job(int n) {
    DecodeJob j;
    for (int k = 0; k < n; ++k) {
      DecodeJob one;
      if (!cam->make_job(enc.next(), one)) {
        std::fprintf(stderr, "FAIL %s: no job from an access unit\n", cam->name().c_str());
        ++failures;
        continue;
      }
      if (j.cam < 0) j = std::move(one);
      else merge_job(j, std::move(one));
    }
    for (size_t k = 0; k < j.history_outputs(); ++k) j.outputs[k].ring_slot = int(k);
    return j;
  }
  SynthH264 enc;
  std::shared_ptr<Camera> cam;
};

static SynthConfig fast_cfg(int w, int h, double motion) {
  SynthConfig c;
  c.width = w;
  c.height = h;
  c.gop = 64;
  c.motion = motion;
  return c;
}

static SynthConfig general_cfg(const char* profile, int w, int h, Codec codec) {
  SynthConfig c;
  c.width = w;
  c.height = h;
  c.gop = 64;
  c.compressed = true;
  c.profile = profile;
  c.bframes = 2;
  c.codec = codec;
  return c;
}

int main() {
  WorkerOptions o;
  o.device = -1;
  o.max_cameras = 16;
  Worker w(o);
  Source fast(w, fast_cfg(176, 144, 0.05), "fast", 0);
  Source still(w, fast_cfg(176, 144, 0.0), "still", 0);
  Source high(w, general_cfg("high", 320, 240, Codec::kH264), "high", 3);
  Source base(w, general_cfg("baseline", 176, 144, Codec::kH264), "base", 0);
  Source hintra(w, general_cfg("baseline", 416, 240, Codec::kH265), "hintra", 0);
  Source hinter(w, general_cfg("baseline", 416, 240, Codec::kH265), "hinter", 0);

  std::vector<DecodeJob> a, b, c, d;
  a.push_back(fast.job(1));  // (a) one fast-path job: the keyframe
  still.job(1);
  b.push_back(still.job(1));  // (b) a P picture without a coded macroblock
  batch_name = "setup";
  check(!a[0].general() && a[0].upd.nslots > 0 && !a[0].upd.segs.empty(), "(a) is not a fast-path keyframe");
  check(!b[0].general() && b[0].upd.nslots == 0, "(b) has coded macroblocks");
  high.job(1);
  c.push_back(high.job(5));  // (c) an IBBP catch-up of five pictures next to a one-picture job
  c.push_back(base.job(1));
  check(c[0].avc.size() == 5 && c[1].avc.size() == 1, "(c) does not hold 5 + 1 pictures");
  check(c[0].history_outputs() > 0, "(c) has no history output");
  hinter.job(1);
  d.push_back(hintra.job(1));  // (d) an intra picture (several TU levels) next to an inter-only one
  d.push_back(hinter.job(1));
  check(d[0].hevc.size() == 1 && d[0].hevc[0]->level_begin.size() > 3, "(d) has no intra levels");
  check(d[1].hevc.size() == 1 && d[1].hevc[0]->level_begin.size() <= 2, "(d) has no inter-only picture");
  check(d[0].hevc[0]->width % 64 != 0 || d[0].hevc[0]->height % 64 != 0, "(d) has no partial last CTB");

  plan_and_check("a", a, true, 8);
  plan_and_check("b", b, true, 8);
  plan_and_check("c", c, true, 8);
  for (int window : {-1, 0, 3, kWholeRound}) plan_and_check("d", d, true, window);

  {  // (f) batch (c) with the H.264 record arrays in registered memory: the gathered branch
    std::vector<const u8*> ranges;
    auto reg = [&](const void* p, size_t n) {
      if (n == 0) return;
      hostmem::register_range(static_cast<const u8*>(p), n, static_cast<const u8*>(p));
      ranges.push_back(static_cast<const u8*>(p));
    };
    for (const DecodeJob& j : c)
      for (const auto& p : j.avc) {
        reg(p->mbs.data(), p->mbs.size() * sizeof(avc::MbRec));
        reg(p->coefs.data(), p->coefs.size() * sizeof(i16));
        reg(p->mvs.data(), p->mvs.size() * sizeof(i16));
        reg(p->wps.data(), p->wps.size() * sizeof(avc::WpEntry));
      }
    batch_name = "f";
    const StagePlan pl(c, {true, 8});
    check(pl.bytes_gathered > 0 && !pl.chunks.empty() && pl.tasks.empty(), "(f) does not gather its records");
    check_plan(c, pl);
    for (const u8* p : ranges) hostmem::unregister_range(p);
  }

  std::vector<DecodeJob> e;  // (e) everything in one batch
  for (auto* v : {&a, &b, &c, &d})
    for (DecodeJob& j : *v) e.push_back(std::move(j));
  plan_and_check("e", e, true, 8);
  plan_and_check("e", e, false, 8);

  if (failures) {
    std::fprintf(stderr, "stage_plan_selftest: %d failures\n", failures);
    return 1;
  }
  std::printf("stage_plan_selftest ok\n");
  return 0;
}
