// Stand-alone check of the scratch pool's locking (vep/scratch.h), host only: no HIP in it, so it
// runs anywhere and under the host sanitizers (`make tsan-scratch`, `make asan-scratch`, and
// un-instrumented in the default suite: `make scratch-selftest`). The set is a fake that counts
// its constructions and carries an owner flag; its buffer restates the grow-only reserve of
// gpu::GrowBuf on the heap and counts growths. Exit status 0 and no sanitizer report = pass.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <stdexcept>
#include <thread>
#include <utility>
#include <vector>

#include "vep/scratch.h"

static int failures = 0;

static void check(bool ok, const char* what) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s\n", what);
  ++failures;
}

static std::atomic<int> constructed{0};
static std::atomic<int> growths{0};

struct FakeBuf {  // the reserve contract of gpu::GrowBuf
  char* p = nullptr;
  size_t cap = 0;
  ~FakeBuf() { std::free(p); }
  void reserve(size_t n, size_t floor = 0) {
    if (cap >= n) return;
    std::free(p);
    p = nullptr;
    cap = 0;
    const size_t want = n > floor ? n : floor;
    p = static_cast<char*>(std::malloc(want));
    if (!p) throw std::bad_alloc();
    cap = want;
    ++growths;
  }
};

struct FakeSet {
  FakeSet() { ++constructed; }
  std::atomic<int> owner{0};  // 1 while a thread holds the set
  int plain = 0;              // unsynchronised on purpose: a set shared by two threads is a race
  FakeBuf buf;
};

constexpr int kMax = 4;
using Pool = vep::ScratchPool<FakeSet, kMax>;

// 1-3: more threads than sets; never more than kMax sets or live leases, never a shared set
static void hammer() {
  Pool pool;
  constructed = 0;
  std::atomic<int> live{0}, max_live{0}, shared{0}, over{0};
  std::vector<std::thread> th;
  for (int t = 0; t < 16; ++t)
    th.emplace_back([&] {
      for (int i = 0; i < 4000; ++i) {
        Pool::Lease l = pool.acquire();
        const int now = ++live;
        int seen = max_live.load();
        while (now > seen && !max_live.compare_exchange_weak(seen, now)) {
        }
        if (l->owner.exchange(1) != 0) ++shared;
        if (constructed.load() > kMax) ++over;
        ++l->plain;
        (*l).buf.reserve(64 + size_t(i % 3), 64);
        l.get()->owner.store(0);
        --live;
      }
    });
  for (std::thread& t : th) t.join();
  check(constructed.load() <= kMax && over.load() == 0, "more than kMax sets constructed");
  check(max_live.load() <= kMax, "more than kMax leases live at once");
  check(shared.load() == 0, "a set was held by two threads");
  check(live.load() == 0, "a lease outlived its scope");
}

// 4: a throw while a lease is held returns the set
static void throwing() {
  Pool pool;
  constructed = 0;
  FakeSet* first = nullptr;
  try {
    Pool::Lease l = pool.acquire();
    first = l.get();
    throw std::runtime_error("request failed");
  } catch (const std::runtime_error&) {
  }
  Pool::Lease l = pool.acquire();
  check(l.get() == first, "the set of a failed request was not the next one handed out");
  check(constructed.load() == 1, "a failed request cost a set");
}

// 5: a moved-from lease releases nothing
static void moving() {
  Pool pool;
  constructed = 0;
  {
    Pool::Lease a = pool.acquire();
    FakeSet* s = a.get();
    Pool::Lease b = std::move(a);
    check(a.get() == nullptr && b.get() == s, "move construction");
    Pool::Lease c;
    c = std::move(b);
    check(b.get() == nullptr && c.get() == s, "move assignment");
  }
  // were the set released twice, it would sit in the free list twice and go to two holders
  Pool::Lease x = pool.acquire();
  Pool::Lease y = pool.acquire();
  check(x.get() != y.get(), "a moved-from lease released its set again");
  check(constructed.load() == 2, "sets after the moves");
}

// 6: with every set held, acquire waits until one is dropped
static void waiting() {
  Pool pool;
  constructed = 0;
  std::vector<Pool::Lease> held;
  for (int i = 0; i < kMax; ++i) held.push_back(pool.acquire());
  std::atomic<bool> started{false}, got{false};
  std::thread waiter([&] {
    started = true;
    Pool::Lease l = pool.acquire();
    got = true;
  });
  while (!started) std::this_thread::yield();
  std::this_thread::sleep_for(std::chrono::milliseconds(20));
  check(!got.load(), "acquire returned with every set held");
  check(constructed.load() == kMax, "a set beyond kMax was constructed for the waiter");
  held.pop_back();
  waiter.join();
  check(got.load(), "the waiter did not get the dropped set");
  check(constructed.load() == kMax, "sets after the wait");
}

// 7: steady state allocates nothing
static void steady() {
  Pool pool;
  constructed = 0;
  for (int i = 0; i < 8; ++i) pool.acquire()->buf.reserve(100, 64);  // (one set: each lease ends at once)
  growths = 0;
  for (int i = 0; i < 1000; ++i) {
    Pool::Lease l = pool.acquire();
    l->buf.reserve(100, 64);
    l->buf.reserve(10, 64);  // a smaller request: never shrinks
  }
  check(growths.load() == 0, "steady state grew a buffer");
  check(constructed.load() == 1, "sequential requests used more than one set");
  {
    Pool::Lease l = pool.acquire();
    l->buf.reserve(1, 64);
    check(l->buf.cap == 100, "capacity after smaller requests");
    l->buf.reserve(101, 64);
    check(l->buf.cap == 101 && growths.load() == 1, "growth past the capacity");
  }
  FakeBuf b;
  b.reserve(1, 64);
  check(b.cap == 64, "the floor");
  b.reserve(0);
  check(b.cap == 64, "reserve(0)");
}

int main() {
  hammer();
  throwing();
  moving();
  waiting();
  steady();
  if (failures) {
    std::fprintf(stderr, "scratch_selftest: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("scratch_selftest ok\n");
  return 0;
}
