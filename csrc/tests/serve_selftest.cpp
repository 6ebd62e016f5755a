// Stand-alone check of the serving reads' consistent-read rule (vep/ring_read.h), host only: the
// produce step (or a stub op's run step) rewrites or invalidates the ring itself, so the retry
// runs deterministically. Rings of 2 slots of 16x8 BGR24 (384 bytes), one fill byte per frame; a
// CPU-backend Worker (device -1) for the stored-answer case. `make serve-selftest` links it
// against the objects csrc/build.py made (default CPU suite); `make asan-serve` builds it from
// sources under AddressSanitizer + UndefinedBehaviorSanitizer. Exit status 0 and no sanitizer
// report = pass.
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <vector>

#include "vep/ring_read.h"
#include "vep/runtime.h"

using namespace vep;

static int failures = 0;

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #cond);          \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

constexpr int kW = 16, kH = 8;

static std::shared_ptr<FrameRing> make_ring(Device& dev) { return std::make_shared<FrameRing>(dev, 2, kW, kH); }

// One frame of `fill` bytes (also its pts); returns its seq.
static i64 publish(FrameRing& r, u8 fill) {
  const int s = r.begin_write();
  std::memset(r.slot_ptr(s), fill, r.slot_bytes());
  FrameMeta m;
  m.pts = fill;
  r.commit(s, m);
  return r.published();
}
// Two frames: on a 2-slot ring the second one takes the slot that held the newest frame before.
static i64 rewrite(FrameRing& r, u8 fill) {
  publish(r, u8(fill - 1));
  return publish(r, fill);
}

// produce of the single-ring cases: keeps the slot's bytes and the seqs it saw.
struct Keeper {
  FrameRing& ring;
  std::vector<u8> kept;
  std::vector<i64> seen;
  void operator()(int slot, const FrameMeta& m) {
    seen.push_back(m.seq);
    kept.assign(ring.slot_ptr(slot), ring.slot_ptr(slot) + ring.slot_bytes());
  }
  bool all(u8 fill) const {
    for (u8 b : kept)
      if (b != fill) return false;
    return kept.size() == size_t(kW) * kH * 3;
  }
};

static void single_ring(Device& dev) {
  FrameMeta meta;
  {  // no committed frame, and after >= the newest seq: false, produce never called
    auto r = make_ring(dev);
    Keeper k{*r};
    CHECK(!read_consistent(*r, 0, &meta, k) && k.seen.empty());
    CHECK(publish(*r, 10) == 1);
    CHECK(!read_consistent(*r, 1, &meta, k) && !read_consistent(*r, 5, &meta, k) && k.seen.empty());
    // a stable ring: one call, that frame's meta
    CHECK(read_consistent(*r, 0, &meta, k));
    CHECK(k.seen == std::vector<i64>{1} && meta.seq == 1 && meta.pts == 10 && k.all(10));
  }
  for (int how = 0; how < 2; ++how) {  // the slot is taken away once during produce
    auto r = make_ring(dev);
    publish(*r, 10);
    Keeper k{*r};
    i64 newer = 0;
    const bool ok = read_consistent(*r, 0, &meta, [&](int slot, const FrameMeta& m) {
      k(slot, m);
      if (k.seen.size() > 1) return;
      if (how == 0) {
        newer = rewrite(*r, 30);  // commit, commit again into the slot being read
        CHECK(r->begin_write() != slot);  // (and a write in progress elsewhere changes nothing)
      } else {
        r->invalidate();
        newer = publish(*r, 30);
      }
    });
    CHECK(ok && k.seen.size() == 2 && k.seen[0] == 1 && k.seen[1] == newer && newer > 1);
    CHECK(meta.seq == newer && meta.pts == 30 && k.all(30));
  }
  {  // rewritten during every call: kReadAttempts calls, no answer
    auto r = make_ring(dev);
    publish(*r, 10);
    Keeper k{*r};
    u8 fill = 20;
    CHECK(!read_consistent(*r, 0, &meta, [&](int slot, const FrameMeta& m) {
      k(slot, m);
      rewrite(*r, fill += 2);
    }));
    CHECK(int(k.seen.size()) == kReadAttempts);
  }
  {  // what produce throws reaches the caller
    auto r = make_ring(dev);
    publish(*r, 10);
    int calls = 0;
    bool caught = false;
    try {
      read_consistent(*r, 0, &meta, [&](int, const FrameMeta&) {
        ++calls;
        throw std::runtime_error("produce");
      });
    } catch (const std::runtime_error&) {
      caught = true;
    }
    CHECK(caught && calls == 1);
  }
}

// ---- the batched rounds with a stub op ----------------------------------------------------------

struct StubEntry : ReadEntry {
  int id = 0;
  int planned = 0, committed = 0;
  i64 committed_seq = 0;
};
struct StubOp {
  std::map<int, i64> answers;               // id -> the seq a stored answer exists for
  std::vector<std::vector<int>> rounds;     // the ids of every run's todo list
  std::vector<StubEntry>* entries = nullptr;
  std::vector<int> rewrite_in_run;          // ids whose ring is rewritten by every run ...
  int rewrite_rounds = kReadAttempts;       // ... of the first so many rounds
  u8 fill = 100;
  bool stored(StubEntry& e) {
    auto it = answers.find(e.id);
    return it != answers.end() && it->second == e.meta.seq;
  }
  void plan(StubEntry& e) { ++e.planned; }
  void run(std::vector<StubEntry*>& todo) {
    std::vector<int> ids;
    for (StubEntry* e : todo) ids.push_back(e->id);
    rounds.push_back(ids);
    if (int(rounds.size()) > rewrite_rounds) return;
    for (int id : rewrite_in_run) rewrite(*(*entries)[size_t(id)].ring, fill += 2);
  }
  void commit(StubEntry& e) {
    ++e.committed;
    e.committed_seq = e.meta.seq;
  }
};

static std::vector<StubEntry> stub_entries(Device& dev, int n) {
  std::vector<StubEntry> es((size_t(n)));
  for (int k = 0; k < n; ++k) {
    es[size_t(k)].id = k;
    es[size_t(k)].ring = make_ring(dev);
    es[size_t(k)].pending = true;
  }
  return es;
}

static void batched(Device& dev) {
  {  // three rings, entry 1's rewritten by round 0's run: only it runs again
    std::vector<StubEntry> es = stub_entries(dev, 3);
    for (StubEntry& e : es) publish(*e.ring, u8(10 + e.id));
    StubOp op;
    op.entries = &es;
    op.rewrite_in_run = {1};
    op.rewrite_rounds = 1;
    read_consistent_rounds(es, op);
    CHECK(op.rounds.size() == 2 && op.rounds[0] == (std::vector<int>{0, 1, 2}) && op.rounds[1] == std::vector<int>{1});
    for (const StubEntry& e : es) CHECK(e.ok && !e.pending && e.committed == 1);
    CHECK(es[0].committed_seq == 1 && es[2].committed_seq == 1 && es[0].planned == 1 && es[2].planned == 1);
    CHECK(es[1].committed_seq == 3 && es[1].meta.seq == 3 && es[1].planned == 2);
  }
  {  // a stored answer for the newest seq: ok, never planned or run; no frame: dropped, not ok
    std::vector<StubEntry> es = stub_entries(dev, 2);
    publish(*es[0].ring, 10);
    StubOp op;
    op.entries = &es;
    op.answers[0] = 1;
    read_consistent_rounds(es, op);
    CHECK(es[0].ok && !es[0].pending && es[0].planned == 0 && es[0].committed == 0);
    CHECK(!es[1].ok && !es[1].pending && es[1].planned == 0);
    CHECK(op.rounds.empty());
  }
  {  // rewritten in all rounds: not ok, never committed, run kReadAttempts times
    std::vector<StubEntry> es = stub_entries(dev, 2);
    for (StubEntry& e : es) publish(*e.ring, u8(10 + e.id));
    StubOp op;
    op.entries = &es;
    op.rewrite_in_run = {1};
    read_consistent_rounds(es, op);
    CHECK(int(op.rounds.size()) == kReadAttempts && !es[1].ok && es[1].committed == 0 && es[1].planned == kReadAttempts);
    CHECK(es[0].ok && es[0].committed == 1 && es[0].planned == 1);
  }
}

static void each_once() {
  struct Eval {
    int cam = -1;
    i64 after = 0;
    bool ok = false;
    int result = 0;
  };
  std::vector<int> seen, out;
  std::vector<char> ok;
  read_each_once<Eval>({3, 1, 3, 7}, 5, out, ok, [&](std::vector<Eval>& evs) {
    for (Eval& e : evs) {
      seen.push_back(e.cam);
      CHECK(e.after == 5);
      e.ok = e.cam != 7;  // (7: an unknown camera)
      e.result = e.cam * 10;
    }
  });
  CHECK(seen == (std::vector<int>{1, 3, 7}));
  CHECK(out.size() == 4 && out[0] == 30 && out[2] == out[0] && out[1] == 10);
  CHECK(ok == (std::vector<char>{1, 1, 1, 0}) && out[3] == 0);
}

// One evaluation per frame: a second read at the same seq gets the stored answer.
static void stored_answers() {
  WorkerOptions o;
  o.device = -1;
  o.max_cameras = 4;
  Worker w(o);
  const int cam = w.add_camera("c", 2);
  std::shared_ptr<Camera> c = w.camera(cam);
  c->set_ring(make_ring(w.device()));
  motion::Params mp;
  mp.cell = 4;
  w.set_motion_params(mp);
  tamper::Params tp;
  tp.cell = 8;
  w.set_tamper_params(tp);
  publish(*c->ring(), 90);
  MotionResult m1, m2;
  CHECK(w.read_motion(cam, 0, m1) && w.read_motion(cam, 0, m2));
  CHECK(m1.seq == 1 && m2.seq == 1 && m1.cols == 4 && m1.rows == 2 && m1.counts == m2.counts && m1.primed == m2.primed);
  CHECK(c->motion_evaluations.load() == 1);
  MotionResult m3;
  CHECK(!w.read_motion(cam, 1, m3) && c->motion_evaluations.load() == 1);
  TamperResult t1, t2;
  CHECK(w.read_tamper(cam, 0, t1) && c->tamper_evaluations.load() == 1 && !t1.summary.has_reference);
  CHECK(w.tamper_set_reference(cam) && c->tamper_evaluations.load() == 1);  // on the stored answer
  CHECK(w.read_tamper(cam, 0, t2) && c->tamper_evaluations.load() == 1);
  CHECK(t2.seq == 1 && t2.summary.has_reference && t2.hist == t1.hist && t2.sum_y == t1.sum_y);
  publish(*c->ring(), 91);
  CHECK(w.tamper_set_reference(cam) && c->tamper_evaluations.load() == 2);  // on a fresh one
  CHECK(w.read_tamper(cam, 0, t2) && t2.seq == 2 && t2.summary.has_reference && c->tamper_evaluations.load() == 2);
}

int main() {
  Device dev(-1);
  single_ring(dev);
  batched(dev);
  each_once();
  stored_answers();
  if (failures) {
    std::fprintf(stderr, "serve_selftest: %d failures\n", failures);
    return 1;
  }
  std::printf("serve_selftest ok\n");
  return 0;
}
