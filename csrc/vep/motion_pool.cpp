// Host side of the GPU motion detector: the scratch pool (kernel: gpu_motion.hip).
#include <algorithm>

#include "gpu.h"

namespace vep::gpu {

MotionPool::Set::~Set() {
  if (d_descs) (void)hipFree(d_descs);
  if (h_descs) (void)hipHostFree(h_descs);
  if (d_counts) (void)hipFree(d_counts);
  if (h_counts) (void)hipHostFree(h_counts);
  if (ev) (void)hipEventDestroy(ev);
}

MotionPool::MotionPool() = default;
MotionPool::~MotionPool() = default;

MotionPool::Set* MotionPool::acquire(int ndescs, size_t count_cells) {
  Set* s;
  {
    std::unique_lock<std::mutex> g(mu_);
    if (free_.empty() && all_.size() < size_t(kScratch)) {
      all_.push_back(std::make_unique<Set>());
      free_.push_back(all_.back().get());
    }
    cv_.wait(g, [&] { return !free_.empty(); });
    s = free_.back();
    free_.pop_back();
  }
  try {
    if (!s->ev) VEP_HIP(hipEventCreateWithFlags(&s->ev, hipEventDisableTiming | hipEventBlockingSync));
    if (s->desc_cap < ndescs) {  // first use, or a larger request
      if (s->d_descs) VEP_HIP(hipFree(s->d_descs));
      s->d_descs = nullptr;
      if (s->h_descs) VEP_HIP(hipHostFree(s->h_descs));
      s->h_descs = nullptr;
      s->desc_cap = 0;
      const int cap = std::max(ndescs, 64);
      VEP_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_descs), size_t(cap) * sizeof(MotionDesc)));
      VEP_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->h_descs), size_t(cap) * sizeof(MotionDesc),
                            hipHostMallocDefault));
      s->desc_cap = cap;
    }
    if (s->counts_cap < count_cells) {
      if (s->d_counts) VEP_HIP(hipFree(s->d_counts));
      s->d_counts = nullptr;
      if (s->h_counts) VEP_HIP(hipHostFree(s->h_counts));
      s->h_counts = nullptr;
      s->counts_cap = 0;
      const size_t cap = std::max(count_cells, size_t(16384));
      VEP_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_counts), cap * sizeof(u32)));
      VEP_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->h_counts), cap * sizeof(u32), hipHostMallocDefault));
      s->counts_cap = cap;
    }
  } catch (...) {
    release(s);
    throw;
  }
  return s;
}

void MotionPool::release(Set* s) {
  {
    std::lock_guard<std::mutex> g(mu_);
    free_.push_back(s);
  }
  cv_.notify_one();
}

void MotionPool::run(Set& set, int n, size_t count_cells, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= set.desc_cap && count_cells <= set.counts_cap, "motion: more work than the set holds");
  VEP_HIP(hipMemcpyAsync(set.d_descs, set.h_descs, size_t(n) * sizeof(MotionDesc), hipMemcpyHostToDevice, s));
  launch_motion(set.d_descs, set.h_descs, n, s);
  if (count_cells)  // (0: the counts are the caller's own buffers)
    VEP_HIP(hipMemcpyAsync(set.h_counts, set.d_counts, count_cells * sizeof(u32), hipMemcpyDeviceToHost, s));
  VEP_HIP(hipEventRecord(set.ev, s));
}

}  // namespace vep::gpu
