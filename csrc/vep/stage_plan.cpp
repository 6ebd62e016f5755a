// Stage plan: see stage_plan.h.
#include "stage_plan.h"

#include <algorithm>

namespace vep {

namespace {

size_t al(size_t x, size_t a = 256) { return (x + a - 1) & ~(a - 1); }
size_t chunks_of(size_t len) { return (len + gpu::kGatherChunk - 1) / gpu::kGatherChunk; }
template <class V>
size_t bytes_of(const V& v) {
  return v.size() * sizeof(*v.data());
}

}  // namespace

StagePlan::Region StagePlan::add(Kind kind, const void* src, size_t bytes, size_t pad, size_t floor, bool pull) {
  Entry e{kind, need, bytes, al(std::max(bytes, floor), pad), align_, static_cast<const u8*>(src), nullptr, false, false};
  switch (kind) {
    case kRecord:  // pull: the GPU gathers an array that lies in pinned memory (H.264: hostmem::pinned_vector)
      e.dev = pull && bytes > 0 ? hostmem::device_address(e.src, bytes) : nullptr;
      e.gather = e.dev != nullptr;
      e.copy = !e.gather;
      break;
    case kPayload:  // read in place when pinned; additionally gathered without direct reads
      e.dev = hostmem::device_address(e.src, bytes);
      e.copy = e.dev == nullptr;
      e.gather = !set.direct;
      break;
    default:
      break;
  }
  if (e.gather && kind == kRecord) planned_chunks += chunks_of(bytes);
  need += e.room;
  align_ = std::min(align_, pad);
  entries.push_back(e);
  return {e.off, bytes};
}

void StagePlan::seal() {
  need = al(need);
  align_ = 256;
}

StagePlan::StagePlan(const std::vector<DecodeJob>& jv, const Settings& s) : set(s) {
  const size_t n = jv.size();
  if (!set.direct)  // (the gather region precedes the payload it describes)
    for (const DecodeJob& j : jv)
      for (const auto& sg : j.upd.segs) planned_chunks += chunks_of(sg.len);
  for (size_t i = 0; i < n; ++i)
    if (jv[i].has_output()) outs.push_back(int(i));
  size_t nhist = 0, nregions = 5 + 3 * n;  // (one allocation for the region list)
  for (const DecodeJob& j : jv) {
    for (const JobOutput& o : j.outputs) nhist += o.ring_slot >= 0 ? 1 : 0;
    nregions += 8 * j.avc.size() + 17 * j.hevc.size() + j.upd.segs.size();
  }
  entries.reserve(nregions);
  decode = add(kBuilt, nullptr, sizeof(gpu::DecodeDesc) * n);
  letterbox = add(kBuilt, nullptr, sizeof(gpu::LetterboxDesc) * n);
  weave = add(kBuilt, nullptr, sizeof(gpu::WeaveDesc) * n);  // field pairs
  history = add(kBuilt, nullptr, sizeof(gpu::SurfaceBgrDesc) * nhist);
  jobs.resize(n);
  const size_t ent = set.direct ? sizeof(u64) : sizeof(u32);
  for (size_t i = 0; i < n; ++i) {
    const size_t words = size_t(jv[i].upd.mbs() + 31) / 32;
    jobs[i].mask = add(kBuilt, nullptr, words * sizeof(u32), 16);
    jobs[i].prefix = add(kBuilt, nullptr, words * sizeof(u32), 16);
    jobs[i].table = add(kBuilt, nullptr, size_t(jv[i].upd.nslots) * ent, 16);
  }
  plan_avc(jv);
  plan_hevc(jv);
  plan_history(jv);
  // pinned records (+ every slice segment without direct reads)
  gather = add(kBuilt, nullptr, sizeof(gpu::GatherChunk) * planned_chunks, 256, sizeof(gpu::GatherChunk));
  seal();
  header_bytes = need;
  for (size_t i = 0; i < n; ++i) {
    Job& jp = jobs[i];
    jp.payload = need;
    for (const auto& sg : jv[i].upd.segs) {
      const Region r = add(kPayload, sg.base, sg.len, 16);
      jp.seg_rel.push_back(r.off - jp.payload);
      jp.seg_dev.push_back(entries.back().dev);
      (entries.back().copy ? bytes_staged : bytes_inplace) += u64(sg.len);
    }
  }
  seal();
  for (AvcPic& a : avc) {
    a.dbk = add(kScratch, nullptr, size_t(a.p->nmbs()) * sizeof(gpu::AvcDbkInfo));  // per-MB loop-filter inputs
    // intra MBs' residual samples (inter kernel -> intra wavefront)
    a.res = add(kScratch, nullptr, size_t(a.p->intra_res) * gpu::kAvcResSamples * sizeof(i16));
    a.xg = add(kScratch, nullptr, gpu::avc_xg_bytes(a.p->wmbs, a.p->hmbs));  // deblock exchange between workgroups
  }
  seal();
  plan_transfers();
}

// General H.264 pictures: MB records, coefficient blocks, motion vectors and prediction weights
// of every picture, plus one AvcDesc array per reconstruction round.
void StagePlan::plan_avc(const std::vector<DecodeJob>& jv) {
  size_t rounds = 0;
  for (const DecodeJob& j : jv) rounds = std::max(rounds, j.avc.size());
  avc_rounds.resize(rounds);
  for (size_t r = 0; r < rounds; ++r) {
    AvcRound& rd = avc_rounds[r];
    for (size_t i = 0; i < jv.size(); ++i) {
      if (jv[i].avc.size() <= r) continue;
      const avc::Picture& p = *jv[i].avc[r];
      VEP_CHECK(p.hmbs <= gpu::kAvcMaxRows && p.wmbs <= gpu::kAvcMaxCols,
                "picture too large for the wavefront kernels");
      VEP_CHECK(p.wmbs * 16 == jv[i].pic.coded_width &&
                    p.hmbs * 16 * (p.structure ? 2 : 1) == jv[i].pic.coded_height,  // (a field: half)
                "picture size differs from the camera's surfaces");
      AvcPic a{&p, int(i), {}, {}, {}, {}, {}, {}, {}};
      a.mbs = add(kRecord, p.mbs.data(), bytes_of(p.mbs));
      a.coefs = add(kRecord, p.coefs.data(), bytes_of(p.coefs));
      a.mvs = add(kRecord, p.mvs.data(), bytes_of(p.mvs));
      a.wps = add(kRecord, p.wps.data(), bytes_of(p.wps));
      rd.pics.push_back(int(avc.size()));
      avc.push_back(a);
      rd.mbs += p.nmbs();
      rd.max_h = std::max(rd.max_h, p.hmbs);
      rd.intra |= p.intra_mbs > 0;
      rd.dbk |= p.deblock;
      if (p.bd > 8 || p.cf == 2) rd.variants |= p.cf != 2 ? 1 : (p.bd > 8 ? 4 : 2);
      else rd.narrow = true;
    }
    rd.descs = add(kBuilt, nullptr, rd.pics.size() * sizeof(gpu::AvcDesc));
  }
}

// General H.265 pictures: reconstruction records of every picture; per round one HevcDesc array,
// the TU ranges, the queue windows' ticket counters and the per-picture queues.
void StagePlan::plan_hevc(const std::vector<DecodeJob>& jv) {
  size_t rounds = 0;
  for (const DecodeJob& j : jv) rounds = std::max(rounds, j.hevc.size());
  hevc_rounds.resize(rounds);
  for (size_t r = 0; r < rounds; ++r) {
    HevcRound& rd = hevc_rounds[r];
    int maxl = 0;
    for (size_t i = 0; i < jv.size(); ++i) {
      if (jv[i].hevc.size() <= r) continue;
      const hevc::GpuPicture& p = *jv[i].hevc[r];
      VEP_CHECK(((p.width + 15) & ~15) == jv[i].pic.coded_width && ((p.height + 15) & ~15) == jv[i].pic.coded_height,
                "picture size differs from the camera's surfaces");
      HevcPic a{&p, int(i), {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}};
      // (always copied; an empty array keeps 16 bytes, so its descriptor holds a valid address)
      auto add_copied = [&](const void* src, size_t bytes) { return add(kRecord, src, bytes, 256, 16, false); };
      a.pus = add_copied(p.pus.data(), bytes_of(p.pus));
      a.tus = add_copied(p.tus.data(), bytes_of(p.tus));
      a.coefs = add_copied(p.coefs.data(), bytes_of(p.coefs));
      a.pcm = add_copied(p.pcm.data(), bytes_of(p.pcm));
      a.bs_v = add_copied(p.bs_v.data(), bytes_of(p.bs_v));
      a.bs_h = add_copied(p.bs_h.data(), bytes_of(p.bs_h));
      a.qp = add_copied(p.qp.data(), bytes_of(p.qp));
      a.pcm_map = add_copied(p.pcm_map.data(), bytes_of(p.pcm_map));
      a.ctb_slice = add_copied(p.ctb_slice.data(), bytes_of(p.ctb_slice));
      a.slices = add_copied(p.slices.data(), bytes_of(p.slices));
      a.sao = add_copied(p.sao_params.data(), bytes_of(p.sao_params));
      a.wp = add_copied(p.wp.data(), bytes_of(p.wp));
      a.ctb_tile = add_copied(p.ctb_tile.data(), bytes_of(p.ctb_tile));
      maxl = std::max(maxl, int(p.level_begin.size()) - 1);
      rd.pics.push_back(int(hevc.size()));
      hevc.push_back(a);
      rd.pus += int(p.pus.size());
      rd.blks += p.w4() * p.h4();
      rd.dbk |= p.deblock;
      rd.sao |= p.sao;
    }
    rd.descs = add(kBuilt, nullptr, rd.pics.size() * sizeof(gpu::HevcDesc));
    int tickets = 0;
    for (int l = 0; l < maxl; ++l) {
      if (l > 0) rd.levels.push_back({tickets, 0});
      for (size_t k = 0; k < rd.pics.size(); ++k) {
        const hevc::GpuPicture& p = *hevc[size_t(rd.pics[k])].p;
        if (int(p.level_begin.size()) - 1 <= l) continue;
        const int b = int(p.level_begin[size_t(l)]), e = int(p.level_begin[size_t(l) + 1]);
        if (e <= b) continue;
        if (l == 0) {
          rd.tu_ranges.push_back({int(k), b, e - b, rd.l0_blocks});
          rd.l0_ranges += 1;
          rd.l0_blocks += e - b;
        } else {
          rd.tu_ranges.push_back({int(k), b, e - b, tickets});
          rd.intra_ranges += 1;
          tickets += e - b;
          rd.levels.back().count += e - b;
        }
      }
    }
    rd.intra_blocks = tickets;
    if (set.tu_window < 0) {  // one workgroup per picture with intra blocks
      for (size_t k = 0; k < rd.pics.size(); ++k) {
        const hevc::GpuPicture& p = *hevc[size_t(rd.pics[k])].p;
        if (p.level_begin.size() < 3) continue;  // (levels 0 .. L-1 plus the end: intra needs L >= 2)
        const int b = int(p.level_begin[1]), e = int(p.tus.size());
        if (e > b) rd.pic_queues.push_back({int(k), b, e - b, 0});
      }
    }
    if (set.tu_window > 0) {  // consecutive levels, tu_window per launch
      const auto& lv = rd.levels;
      for (size_t l = 0; l < lv.size(); l += size_t(set.tu_window)) {
        const size_t e = std::min(lv.size(), l + size_t(set.tu_window));
        const int first = lv[l].first, last = lv[e - 1].first + lv[e - 1].count;
        if (last > first) rd.windows.push_back({first, last - first});
      }
    }
    rd.ranges = add(kBuilt, nullptr, bytes_of(rd.tu_ranges), 256, sizeof(gpu::HevcTuRange));
    rd.counters = add(kBuilt, nullptr, rd.windows.size() * sizeof(u32), 256, sizeof(u32));  // (zero in the upload)
    rd.picq = add(kBuilt, nullptr, bytes_of(rd.pic_queues), 256, sizeof(gpu::HevcTuRange));
  }
}

// The history outputs in round order: the H.264 rounds run first, then the H.265 rounds.
void StagePlan::plan_history(const std::vector<DecodeJob>& jv) {
  struct Key {
    size_t round;
    HistOut h;
  };
  std::vector<Key> keys;
  for (size_t i = 0; i < jv.size(); ++i) {
    const DecodeJob& j = jv[i];
    for (size_t k = 0; k < j.outputs.size(); ++k) {
      const JobOutput& o = j.outputs[k];
      if (o.ring_slot < 0) continue;
      VEP_CHECK(o.released_by >= 0 && o.released_by < int(j.avc.empty() ? j.hevc.size() : j.avc.size()),
                "history output released by a picture outside its job");
      keys.push_back({size_t(o.released_by) + (j.avc.empty() ? avc_rounds.size() : 0), {int(i), int(k), 0}});
    }
  }
  std::stable_sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) { return a.round < b.round; });
  for (const Key& k : keys) {
    HistSpan& hs = k.round < avc_rounds.size() ? avc_rounds[k.round].hist : hevc_rounds[k.round - avc_rounds.size()].hist;
    if (hs.count == 0) hs.first = int(hist.size());
    const PictureInfo& pi = jv[size_t(k.h.job)].outputs[size_t(k.h.out)].pic;
    hist.push_back({k.h.job, k.h.out, hs.tiles});
    hs.count += 1;
    hs.tiles += gpu::tiles_for(pi.coded_width / 16, pi.coded_height / 16);
  }
}

// The one place that turns regions into transfers: kPackChunk pieces for the pack threads,
// gpu::kGatherChunk pieces for the gather kernel.
void StagePlan::plan_transfers() {
  for (const Entry& e : entries) {
    if (e.copy)
      for (size_t o = 0; o < e.bytes; o += kPackChunk)
        tasks.push_back({e.src + o, e.off + o, std::min(kPackChunk, e.bytes - o)});
    if (e.gather) {
      for (size_t o = 0; o < e.bytes; o += gpu::kGatherChunk)
        chunks.push_back({e.dev ? e.dev + o : nullptr, e.off + o, u32(std::min<size_t>(gpu::kGatherChunk, e.bytes - o))});
      if (e.kind == kRecord) bytes_gathered += u64(e.bytes);
    }
  }
  VEP_CHECK(chunks.size() == planned_chunks, "gather chunk count mismatch");
}

}  // namespace vep
