// Host side of the GPU tamper detector: the scratch pool (kernel: gpu_tamper.hip).
#include <algorithm>

#include "gpu.h"

namespace vep::gpu {

TamperPool::Set::~Set() {
  if (d_descs) (void)hipFree(d_descs);
  if (h_descs) (void)hipHostFree(h_descs);
  if (d_res) (void)hipFree(d_res);
  if (h_res) (void)hipHostFree(h_res);
  if (ev) (void)hipEventDestroy(ev);
}

TamperPool::TamperPool() = default;
TamperPool::~TamperPool() = default;

TamperPool::Set* TamperPool::acquire(int ndescs, size_t res_words) {
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
      VEP_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_descs), size_t(cap) * sizeof(TamperDesc)));
      VEP_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->h_descs), size_t(cap) * sizeof(TamperDesc),
                            hipHostMallocDefault));
      s->desc_cap = cap;
    }
    if (s->res_cap < res_words) {
      if (s->d_res) VEP_HIP(hipFree(s->d_res));
      s->d_res = nullptr;
      if (s->h_res) VEP_HIP(hipHostFree(s->h_res));
      s->h_res = nullptr;
      s->res_cap = 0;
      const size_t cap = std::max(res_words, size_t(16384));
      VEP_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_res), cap * sizeof(u32)));
      VEP_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->h_res), cap * sizeof(u32), hipHostMallocDefault));
      s->res_cap = cap;
    }
  } catch (...) {
    release(s);
    throw;
  }
  return s;
}

void TamperPool::release(Set* s) {
  {
    std::lock_guard<std::mutex> g(mu_);
    free_.push_back(s);
  }
  cv_.notify_one();
}

void TamperPool::run(Set& set, int n, size_t hist_words, size_t res_words, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= set.desc_cap && hist_words <= res_words && res_words <= set.res_cap,
            "tamper: more work than the set holds");
  VEP_HIP(hipMemcpyAsync(set.d_descs, set.h_descs, size_t(n) * sizeof(TamperDesc), hipMemcpyHostToDevice, s));
  if (hist_words) VEP_HIP(hipMemsetAsync(set.d_res, 0, hist_words * sizeof(u32), s));
  launch_tamper(set.d_descs, set.h_descs, n, s);
  if (res_words)  // (0: the results are the caller's own buffers)
    VEP_HIP(hipMemcpyAsync(set.h_res, set.d_res, res_words * sizeof(u32), hipMemcpyDeviceToHost, s));
  VEP_HIP(hipEventRecord(set.ev, s));
}

}  // namespace vep::gpu
