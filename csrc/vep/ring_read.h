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

// Several rings, one launch a round. Up to kReadAttempts rounds; in each, every pending entry
// picks its frame (pick_frame; none: dropped, not ok) and the op either answers it from a stored
// result (op.stored(e) true: ok, never run) or plans it (op.plan(e)); op.run(todo) then produces
// for all planned entries at once, and op.commit(e) is called for those whose slot proved
// unchanged (ok). The others go into the next round; an entry still pending after the last round
// ends not ok and is never committed.
template <class Entry, class Op>
void read_consistent_rounds(std::vector<Entry>& entries, Op& op) {
  std::vector<Entry*> todo;
  for (int round = 0; round < kReadAttempts; ++round) {
    todo.clear();
    for (Entry& e : entries) {
      if (!e.pending) continue;
      if (!pick_frame(*e.ring, e.after, e.seq, &e.meta, &e.slot)) {
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
      if (!e->ring->still_valid(e->slot, e->meta.seq)) continue;  // redone from the newer frame
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
