// Stand-alone check of the block matching's packed key (vep/flow.h) and of the multi-slot rounds of
// the consistent-read rule (vep/ring_read.h, FramesEntry), host only: a stub op's run step rewrites
// a ring itself, so the retry runs deterministically. Rings of 4 slots that keep 2 frames of 16x8
// BGR24. `make flow-selftest` links it against the objects csrc/build.py made; `make asan-flow`
// builds it from sources under AddressSanitizer + UndefinedBehaviorSanitizer. Exit status 0 and no
// sanitizer report = pass.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <tuple>
#include <vector>

#include "vep/flow.h"
#include "vep/ring_read.h"
#include "vep/runtime.h"

using namespace vep;

static int failures = 0;

#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #cond); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

// The key orders candidates by SAD, then by |vx| + |vy|, then by vy, then by vx; and decodes.
static void key_order() {
  for (int R = flow::kMinRange; R <= flow::kMaxRange; ++R) {
    using Cand = std::tuple<u32, int, int, int>;  // sad, length, vy, vx
    const u32 sads[] = {0, 1, 63, flow::kMaxSad};
    for (int vy = -R; vy <= R; ++vy)
      for (int vx = -R; vx <= R; ++vx)
        for (u32 sad : sads) {
          const u32 k = flow::key(sad, vx, vy, R);
          CHECK(k != flow::kInvalidKey && k < (1u << 29));
          const flow::Record rec = flow::record_of(k, 7, R);
          CHECK(rec.vx == vx && rec.vy == vy && rec.best == sad && rec.zero == 7 && rec.pad == 0);
          // against its neighbours in every field: the keys compare as the tuples do
          const Cand a{sad, std::abs(vx) + std::abs(vy), vy, vx};
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx)
              for (u32 other : sads) {
                const int ux = vx + dx, uy = vy + dy;
                if (ux < -R || ux > R || uy < -R || uy > R) continue;
                const Cand b{other, std::abs(ux) + std::abs(uy), uy, ux};
                CHECK((k < flow::key(other, ux, uy, R)) == (a < b));
              }
        }
    CHECK(flow::valid(8, 8, R > 8 ? 8 : R, -R, 16 + R, 16 + R) && !flow::valid(0, 0, 1, 0, 64, 64) && flow::valid(0, 0, 0, 0, 8, 8));
  }
}

// ---- the multi-slot rounds with a stub op ---------------------------------------------------------

constexpr int kW = 16, kH = 8;

static i64 publish(FrameRing& r, u8 fill) {
  const int s = r.begin_write();
  std::memset(r.slot_ptr(s), fill, r.slot_bytes());
  FrameMeta m;
  m.pts = fill;
  r.commit(s, m);
  return r.published();
}

struct StubEntry : FramesEntry {
  int id = 0, planned = 0, committed = 0;
  std::vector<i64> committed_seqs;
};
struct StubOp {
  std::vector<std::vector<int>> rounds;  // the ids of every run's todo list
  std::vector<StubEntry>* entries = nullptr;
  int victim = -1;         // the entry whose ring every run of the first `spoil_rounds` rounds ...
  int spoil_rounds = 0;
  int publishes = 1;       // ... publishes so many frames into: 1 reuses no slot a reader holds but
                           // moves the history on, so the OLDER of the two slots stops being valid
  u8 fill = 100;
  bool stored(StubEntry&) { return false; }
  void plan(StubEntry& e) { ++e.planned; }
  void run(std::vector<StubEntry*>& todo) {
    std::vector<int> ids;
    for (StubEntry* e : todo) ids.push_back(e->id);
    rounds.push_back(ids);
    if (int(rounds.size()) > spoil_rounds) return;
    // four slots keep two frames: three more frames are sure to reuse the older frame's slot
    for (int k = 0; k < publishes; ++k) publish(*(*entries)[size_t(victim)].ring, fill += 1);
  }
  void commit(StubEntry& e) {
    ++e.committed;
    e.committed_seqs.clear();
    for (const auto& f : e.have) e.committed_seqs.push_back(f.first.seq);
  }
};

static std::vector<StubEntry> stub_entries(Device& dev, int n) {
  std::vector<StubEntry> es((size_t(n)));
  for (int k = 0; k < n; ++k) {
    es[size_t(k)].id = k;
    es[size_t(k)].ring = std::make_shared<FrameRing>(dev, 4, kW, kH, 2);
    es[size_t(k)].frames = 2;
    es[size_t(k)].pending = true;
    publish(*es[size_t(k)].ring, u8(10 + k));
    publish(*es[size_t(k)].ring, u8(20 + k));
  }
  return es;
}

static void rounds(Device& dev) {
  {  // three rings; the slot of entry 1's OLDER frame is reused during round 0: only it runs again
    std::vector<StubEntry> es = stub_entries(dev, 3);
    StubOp op;
    op.entries = &es;
    op.victim = 1;
    op.spoil_rounds = 1;
    op.publishes = 3;
    read_consistent_rounds(es, op);
    CHECK(op.rounds.size() == 2 && op.rounds[0] == (std::vector<int>{0, 1, 2}) && op.rounds[1] == std::vector<int>{1});
    for (const StubEntry& e : es) CHECK(e.ok && !e.pending && e.committed == 1 && e.have.size() == 2);
    CHECK(es[0].committed_seqs == (std::vector<i64>{2, 1}) && es[2].committed_seqs == (std::vector<i64>{2, 1}));
    CHECK(es[1].committed_seqs == (std::vector<i64>{5, 4}) && es[1].meta.seq == 5 && es[1].planned == 2);
  }
  {  // spoiled in every round: never committed, kReadAttempts runs; the other entry is answered once
    std::vector<StubEntry> es = stub_entries(dev, 2);
    StubOp op;
    op.entries = &es;
    op.victim = 1;
    op.spoil_rounds = kReadAttempts;
    op.publishes = 3;
    read_consistent_rounds(es, op);
    CHECK(int(op.rounds.size()) == kReadAttempts && !es[1].ok && es[1].committed == 0 && es[1].planned == kReadAttempts);
    CHECK(es[0].ok && es[0].committed == 1 && es[0].planned == 1);
  }
  {  // `after` bounds the newest frame only: newest - 1 still gets both frames, newest gets no answer
    std::vector<StubEntry> es = stub_entries(dev, 2);
    es[0].after = 1;
    es[1].after = 2;
    StubOp op;
    op.entries = &es;
    read_consistent_rounds(es, op);
    CHECK(es[0].ok && es[0].committed == 1 && es[0].committed_seqs == (std::vector<i64>{2, 1}) && es[0].meta.seq == 2);
    CHECK(!es[1].ok && !es[1].pending && es[1].planned == 0 && op.rounds == (std::vector<std::vector<int>>{{0}}));
  }
  {  // after invalidate() the earlier frame is not readable: the next read has the new frame alone
    std::vector<StubEntry> es = stub_entries(dev, 1);
    es[0].ring->invalidate();
    StubOp op;
    op.entries = &es;
    read_consistent_rounds(es, op);
    CHECK(!es[0].ok && op.rounds.empty());
    publish(*es[0].ring, 50);
    es[0].pending = true;
    read_consistent_rounds(es, op);
    CHECK(es[0].ok && es[0].committed_seqs == std::vector<i64>{3});
  }
}

int main() {
  Device dev(-1);
  key_order();
  rounds(dev);
  if (failures) {
    std::fprintf(stderr, "flow_selftest: %d failures\n", failures);
    return 1;
  }
  std::printf("flow_selftest ok\n");
  return 0;
}
