// Host side of the GPU privacy masks: the descriptor pool (kernel: gpu_mask.hip).
#include <algorithm>

#include "gpu.h"
#include "mask.h"

namespace vep::gpu {

MaskPool::Set::~Set() {
  if (d_descs) (void)hipFree(d_descs);
  if (h_descs) (void)hipHostFree(h_descs);
  if (ev) (void)hipEventDestroy(ev);
}

MaskPool::MaskPool() = default;
MaskPool::~MaskPool() = default;

MaskPool::Set* MaskPool::acquire(int ndescs) {
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
      VEP_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_descs), size_t(cap) * sizeof(MaskDesc)));
      VEP_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->h_descs), size_t(cap) * sizeof(MaskDesc),
                            hipHostMallocDefault));
      s->desc_cap = cap;
    }
  } catch (...) {
    release(s);
    throw;
  }
  return s;
}

void MaskPool::release(Set* s) {
  {
    std::lock_guard<std::mutex> g(mu_);
    free_.push_back(s);
  }
  cv_.notify_one();
}

int fill_mask_descs(MaskDesc* out, u8* dst, size_t dst_bytes, int w, int h, const mask::Mask* m, int n) {
  int lv[mask::kMaxMasks];
  const int top = mask::levels(w, h, m, n, lv);  // (checks the size and the list)
  for (int k = 0; k < n; ++k) {
    const mask::Rect r = mask::to_pixels(w, h, m[k]);
    MaskDesc d{};
    d.dst = dst;
    d.pitch = u32(w) * 3;
    d.w = w;
    d.h = h;
    d.x0 = r.x0;
    d.y0 = r.y0;
    d.x1 = r.x1;
    d.y1 = r.y1;
    d.mode = m[k].mode;
    d.block = m[k].block;
    d.bgr = u32(m[k].b) | u32(m[k].g) << 8 | u32(m[k].r) << 16;
    d.level = lv[k];
    check_mask(d, dst_bytes);
    out[k] = d;
  }
  return top;
}

void MaskPool::run(Set& set, int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(n <= set.desc_cap, "mask: more work than the set holds");
  VEP_HIP(hipMemcpyAsync(set.d_descs, set.h_descs, size_t(n) * sizeof(MaskDesc), hipMemcpyHostToDevice, s));
  for (int level = 0; level < mask::kMaxMasks; ++level) launch_mask(set.d_descs, set.h_descs, n, level, s);
  VEP_HIP(hipEventRecord(set.ev, s));
}

}  // namespace vep::gpu
