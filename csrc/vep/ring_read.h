// The consistent-read rule of a FrameRing, stated once for every serving read (serve.cpp). No HIP
// call in here: csrc/tests/serve_selftest.cpp drives both loops on host rings with stub ops.
//
// A ring slot is read without holding the writer up, so a read is only good once it is over:
//   pick   ring.latest(after, &meta, &slot)   the newest committed frame, none: no answer
//          (pick_frame with seq > 0: that very frame, while the ring's history still holds it);
//   produce something from the slot           a copy, a picture, a launch's results;
//   check  ring.still_valid(slot, meta.seq)   true: the slot held that frame all the while.
// A slot the writer reused meanwhile (or that FrameRing::invalidate took away) is read again from
// the then newest frame, kReadAttempts times in all; after that there is no answer. What was
// produced from a reused slot is never served and never reaches a model.
#pragma once

#include <algorithm>
#include <vector>

#include "runtime.h"

namespace vep {

constexpr int kReadAttempts = 4;

// The pick: seq == 0 the newest frame with seq > after; seq > 0 the frame with that seq (and
// seq > after), found in the history the ring keeps (FrameRing::range). A frame no longer in the
// ring is no answer.
inline bool pick_frame(const FrameRing& ring, i64 after, i64 seq, FrameMeta* meta, int* slot) {
  if (seq <= 0) return ring.latest(after, meta, slot);
  if (seq <= after) return false;
  std::vector<std::pair<FrameMeta, int>> have;  // ascending, contiguous, ending at the newest frame
  ring.range(seq - 1, std::max(1, ring.history()), have);
  if (have.empty() || have.front().first.seq != seq) return false;
  *meta = have.front().first;
  *slot = have.front().second;
  return true;
}

// One ring: produce(slot, *meta) runs on the picked frame (pick_frame(after, seq)) until a run
// proved consistent. False (produce not called) when there is no such frame, and after
// kReadAttempts runs that all saw their slot reused. What produce throws propagates.
template <class Produce>
bool read_consistent(const FrameRing& ring, i64 after, i64 seq, FrameMeta* meta, Produce&& produce) {
  for (int attempt = 0; attempt < kReadAttempts; ++attempt) {
    int slot;
    if (!pick_frame(ring, after, seq, meta, &slot)) return false;
    produce(slot, *meta);
    if (ring.still_valid(slot, meta->seq)) return true;
  }
  return false;
}
// The newest frame with seq > after.
template <class Produce>
bool read_consistent(const FrameRing& ring, i64 after, FrameMeta* meta, Produce&& produce) {
  return read_consistent(ring, after, 0, meta, produce);
}

// Several slots of one ring (the temporal denoise, denoise.h): the rule above over all of them.
//   pick   ring.range(after, frames)   the newest min(frames, available) frames with seq > after,
//          contiguous in seq and ending at the newest; none: no answer. Fewer than asked for
//          (start-up, or just after FrameRing::invalidate) means fewer are used;
//   produce(have, *meta) from all of them   have[0] is the newest, *meta its meta;
//   check  ring.still_valid for EVERY one of those slots.
// One reused slot spoils the read: it starts again from the then newest frames, kReadAttempts
// times in all. After invalidate() no earlier frame is readable, so what a privacy-mask change
// withdrew is never blended into a later picture. *used: how many frames the good read used.
// any_earlier (the deinterlacer, deinterlace.h): `after` decides only whether the newest frame
// answers; the earlier frames are picked whatever `after` is, so a client that polls with the last
// seq it saw still gets the frame before the newest (as FramesEntry below).
template <class Produce>
bool read_consistent_frames(const FrameRing& ring, i64 after, int frames, FrameMeta* meta, int* used, Produce&& produce,
                            bool any_earlier = false) {
  std::vector<std::pair<FrameMeta, int>> have;
  for (int attempt = 0; attempt < kReadAttempts; ++attempt) {
    if (ring.range(any_earlier ? 0 : after, frames, have) < 1 || have.back().first.seq <= after) return false;
    std::reverse(have.begin(), have.end());  // newest first
    *meta = have.front().first;
    produce(have, *meta);
    bool good = true;
    for (const auto& f : have) good = good && ring.still_valid(f.second, f.first.seq);
    if (good) {
      *used = int(have.size());
      return true;
    }
  }
  return false;
}

// One ring of a batched read; an op's entry type derives from it.
struct ReadEntry {
  std::shared_ptr<FrameRing> ring;
  i64 after = 0;
  i64 seq = 0;           // > 0: that very frame (pick_frame)
  FrameMeta meta;        // of the frame picked last
  int slot = -1;
  bool pending = false;  // set by the caller: needs (another) round
  bool ok = false;       // answered, from a stored result or a committed round
};

// One ring of a batched read over several slots (the block matching, flow.h): the entry asks for
// `frames` frames and gets the ring's newest min(frames, available), newest first. `after` decides
// only whether the newest frame answers (its seq > after); the EARLIER frames are picked whatever
// `after` is, since what the op makes of them is stored per newest seq for every caller, and a
// caller polling with the last seq it saw must get what a caller with after = 0 gets. (Unlike
// read_consistent_frames, whose `after` also bounds the earlier frames.) meta and slot are those of
// the newest.
struct FramesEntry : ReadEntry {
  int frames = 1;
  std::vector<std::pair<FrameMeta, int>> have;
};

// The pick and the check of an entry of the rounds below: one slot, or every slot of `have`.
inline bool pick_entry(ReadEntry& e) { return pick_frame(*e.ring, e.after, e.seq, &e.meta, &e.slot); }
inline bool entry_valid(const ReadEntry& e) { return e.ring->still_valid(e.slot, e.meta.seq); }
inline bool pick_entry(FramesEntry& e) {
  if (e.ring->range(0, e.frames, e.have) < 1 || e.have.back().first.seq <= e.after) return false;
  std::reverse(e.have.begin(), e.have.end());
  e.meta = e.have.front().first;
  e.slot = e.have.front().second;
  return true;
}
inline bool entry_valid(const FramesEntry& e) {
  bool good = true;
  for (const auto& f : e.have) good = good && e.ring->still_valid(f.second, f.first.seq);
  return good;
}

// Several rings, one launch a round. Up to kReadAttempts rounds; in each, every pending entry
// picks its frame or frames (pick_entry; none: dropped, not ok) and the op either answers it from a stored
// result (op.stored(e) true: ok, never run) or plans it (op.plan(e)); op.run(todo) then produces
// for all planned entries at once, and op.commit(e) is called for those whose slot, or every one
// of whose slots (FramesEntry), proved unchanged (ok). The others go into the next round; an entry still pending after the last round
// ends not ok and is never committed.
template <class Entry, class Op>
void read_consistent_rounds(std::vector<Entry>& entries, Op& op) {
  std::vector<Entry*> todo;
  for (int round = 0; round < kReadAttempts; ++round) {
    todo.clear();
    for (Entry& e : entries) {
      if (!e.pending) continue;
      if (!pick_entry(e)) {
        e.pending = false;
      } else if (op.stored(e)) {
        e.ok = true;
        e.pending = false;
      } else {
        op.plan(e);
        todo.push_back(&e);
      }
    }
    if (todo.empty()) return;
    op.run(todo);
    for (Entry* e : todo) {
      if (!entry_valid(*e)) continue;  // redone from the newer frame
      op.commit(*e);
      e->ok = true;
      e->pending = false;
    }
  }
}

// A request over a list of cameras that may repeat: evaluate(evs) sees every distinct camera
// once, in ascending index (Eval::cam, Eval::after set), and each position of the request gets a
// copy of its camera's Eval::result, ok[t] = 0 where Eval::ok is false.
template <class Eval, class Result, class Evaluate>
void read_each_once(const std::vector<int>& cams, i64 after, std::vector<Result>& out, std::vector<char>& ok,
                    Evaluate&& evaluate) {
  std::vector<int> order(cams);
  std::sort(order.begin(), order.end());
  order.erase(std::unique(order.begin(), order.end()), order.end());
  std::vector<Eval> evs(order.size());
  for (size_t k = 0; k < order.size(); ++k) {
    evs[k].cam = order[k];
    evs[k].after = after;
  }
  evaluate(evs);
  out.assign(cams.size(), Result{});
  ok.assign(cams.size(), 0);
  for (size_t t = 0; t < cams.size(); ++t) {
    const size_t k = size_t(std::lower_bound(order.begin(), order.end(), cams[t]) - order.begin());
    if (!evs[k].ok) continue;
    out[t] = evs[k].result;
    ok[t] = 1;
  }
}

}  // namespace vep
