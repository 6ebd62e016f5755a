// Bounded pool of scratch sets, one per request in flight (host only: no HIP in here, so the
// locking runs under ThreadSanitizer on any machine, csrc/tests/scratch_selftest.cpp).
//
// The pool contract, stated once for every GPU op that keeps per-request scratch (gpu.h):
//  * up to kMax sets, created lazily: a set is made only when none is free and fewer than kMax
//    exist; otherwise acquire() waits for one to come back;
//  * a set is held by one caller at a time, through a Lease; the lease's destructor returns the
//    set and wakes one waiter, so a set comes back on every path out of a scope, a throw included;
//  * a set keeps what it has grown to (its buffers never shrink), so steady state allocates
//    nothing; the pool itself never frees a set before it is destroyed.
#pragma once

#include <condition_variable>
#include <memory>
#include <mutex>
#include <vector>

namespace vep {

template <class Set, int kMax = 4>
class ScratchPool {
 public:
  static constexpr int kScratch = kMax;

  class Lease {
   public:
    Lease() = default;
    Lease(Lease&& o) noexcept : pool_(o.pool_), set_(o.set_) { o.set_ = nullptr; }
    Lease& operator=(Lease&& o) noexcept {
      if (this != &o) {
        reset();
        pool_ = o.pool_;
        set_ = o.set_;
        o.set_ = nullptr;
      }
      return *this;
    }
    Lease(const Lease&) = delete;
    Lease& operator=(const Lease&) = delete;
    ~Lease() { reset(); }
    Set* get() const { return set_; }
    Set* operator->() const { return set_; }
    Set& operator*() const { return *set_; }

   private:
    friend class ScratchPool;
    Lease(ScratchPool* pool, Set* set) : pool_(pool), set_(set) {}
    void reset() {
      if (set_) pool_->release(set_);
      set_ = nullptr;
    }
    ScratchPool* pool_ = nullptr;
    Set* set_ = nullptr;  // null: moved from, holds nothing
  };

  ScratchPool() = default;
  ScratchPool(const ScratchPool&) = delete;
  ScratchPool& operator=(const ScratchPool&) = delete;

  Lease acquire() {  // a free set (waits for one)
    std::unique_lock<std::mutex> g(mu_);
    if (free_.empty() && all_.size() < size_t(kMax)) {
      all_.push_back(std::make_unique<Set>());
      free_.push_back(all_.back().get());
    }
    cv_.wait(g, [&] { return !free_.empty(); });
    Set* s = free_.back();
    free_.pop_back();
    return Lease(this, s);
  }

 private:
  void release(Set* s) {
    {
      std::lock_guard<std::mutex> g(mu_);
      free_.push_back(s);
    }
    cv_.notify_one();
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<std::unique_ptr<Set>> all_;
  std::vector<Set*> free_;
};

}  // namespace vep
