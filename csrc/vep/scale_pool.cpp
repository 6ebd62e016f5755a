// Host side of the GPU scaler: the scratch pool (kernel: gpu_scale.hip).
#include <algorithm>

#include "gpu.h"

namespace vep::gpu {

ScalePool::Set::~Set() {
  if (canvas) (void)hipFree(canvas);
  if (d_descs) (void)hipFree(d_descs);
  if (h_descs) (void)hipHostFree(h_descs);
  if (upload) (void)hipHostFree(upload);
  if (ev) (void)hipEventDestroy(ev);
}

ScalePool::ScalePool() = default;
ScalePool::~ScalePool() = default;

ScalePool::Set* ScalePool::acquire(size_t canvas_bytes, int ndescs, size_t upload_bytes) {
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
    if (s->canvas_cap < canvas_bytes) {  // first use, or a larger canvas
      if (s->canvas) VEP_HIP(hipFree(s->canvas));
      s->canvas = nullptr;
      s->canvas_cap = 0;
      VEP_HIP(hipMalloc(reinterpret_cast<void**>(&s->canvas), canvas_bytes));
      s->canvas_cap = canvas_bytes;
    }
    if (s->desc_cap < ndescs) {
      if (s->d_descs) VEP_HIP(hipFree(s->d_descs));
      s->d_descs = nullptr;
      if (s->h_descs) VEP_HIP(hipHostFree(s->h_descs));
      s->h_descs = nullptr;
      s->desc_cap = 0;
      const int cap = std::max(ndescs, 64);
      VEP_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_descs), size_t(cap) * sizeof(ScaleDesc)));
      VEP_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->h_descs), size_t(cap) * sizeof(ScaleDesc),
                            hipHostMallocDefault));
      s->desc_cap = cap;
    }
    if (s->upload_cap < upload_bytes) {
      if (s->upload) VEP_HIP(hipHostFree(s->upload));
      s->upload = nullptr;
      s->upload_cap = 0;
      VEP_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->upload), upload_bytes, hipHostMallocDefault));
      s->upload_cap = upload_bytes;
    }
  } catch (...) {
    release(s);
    throw;
  }
  return s;
}

void ScalePool::release(Set* s) {
  {
    std::lock_guard<std::mutex> g(mu_);
    free_.push_back(s);
  }
  cv_.notify_one();
}

void ScalePool::run(Set& set, int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= set.desc_cap, "scale: more descriptors than the set holds");
  VEP_HIP(hipMemcpyAsync(set.d_descs, set.h_descs, size_t(n) * sizeof(ScaleDesc), hipMemcpyHostToDevice, s));
  launch_scale(set.d_descs, set.h_descs, n, s);
}

}  // namespace vep::gpu
