// Host side of the GPU JPEG encoder: the scratch pool and the launch sequence of one picture
// (kernels: gpu_jpeg.hip).
#include <algorithm>

#include "gpu.h"
#include "jpeg.h"

namespace vep::gpu {

// ------------------------------------------------------------------------------- scratch pool

struct JpegPool::Scratch {
  u8* dev = nullptr;       // coefficients | segments | joined stream | lengths | offsets
  size_t dev_cap = 0;
  u32* status = nullptr;   // pinned: JpegDesc::status
  u8* host = nullptr;      // pinned: the joined stream's D2H destination
  size_t host_cap = 0;
  hipEvent_t ev = nullptr;
  ~Scratch() {
    if (dev) (void)hipFree(dev);
    if (status) (void)hipHostFree(status);
    if (host) (void)hipHostFree(host);
    if (ev) (void)hipEventDestroy(ev);
  }
};

JpegPool::JpegPool() = default;
JpegPool::~JpegPool() = default;

JpegPool::Scratch* JpegPool::acquire() {
  std::unique_lock<std::mutex> g(mu_);
  if (free_.empty() && all_.size() < size_t(kScratch)) {
    all_.push_back(std::make_unique<Scratch>());
    free_.push_back(all_.back().get());
  }
  cv_.wait(g, [&] { return !free_.empty(); });
  Scratch* sc = free_.back();
  free_.pop_back();
  return sc;
}

void JpegPool::release(Scratch* sc) {
  {
    std::lock_guard<std::mutex> g(mu_);
    free_.push_back(sc);
  }
  cv_.notify_one();
}

static size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

bool JpegPool::encode(const u8* d_bgr, int w, int h, int quality, hipStream_t s, std::string& out) {
  VEP_CHECK(d_bgr, "jpeg: null picture");
  std::string head = jpeg::header(w, h, quality);  // (validates the size and the quality)
  JpegDesc d{};
  d.bgr = d_bgr;
  d.w = w;
  d.h = h;
  d.quality = quality;
  d.mcus_x = jpeg::mcus_x(w);
  d.mcus = d.mcus_x * jpeg::mcus_y(h);
  d.intervals = jpeg::intervals(d.mcus);
  const size_t coef_bytes = align256(size_t(d.mcus) * jpeg::kCoefsPerMcu * sizeof(i16));
  const size_t seg_bytes = align256(size_t(d.intervals) * jpeg::kSegmentCap);
  const size_t out_bytes = align256(size_t(d.intervals) * (jpeg::kSegmentCap + 2));
  const size_t idx_bytes = align256(size_t(d.intervals) * sizeof(u32));
  VEP_CHECK(out_bytes < (size_t(1) << 31), "jpeg: picture too large for the GPU encoder");
  const size_t need = coef_bytes + seg_bytes + out_bytes + 2 * idx_bytes;
  Scratch* sc = acquire();
  bool ok = false;
  try {
    if (!sc->ev) {
      VEP_HIP(hipEventCreateWithFlags(&sc->ev, hipEventDisableTiming | hipEventBlockingSync));
      VEP_HIP(hipHostMalloc(reinterpret_cast<void**>(&sc->status), 64, hipHostMallocDefault));
    }
    if (sc->dev_cap < need) {  // first use, or a larger picture
      if (sc->dev) VEP_HIP(hipFree(sc->dev));
      sc->dev = nullptr;
      sc->dev_cap = 0;
      VEP_HIP(hipMalloc(reinterpret_cast<void**>(&sc->dev), need));
      sc->dev_cap = need;
    }
    u8* p = sc->dev;
    d.coefs = reinterpret_cast<i16*>(p);
    p += coef_bytes;
    d.seg = p;
    p += seg_bytes;
    d.out = p;
    p += out_bytes;
    d.len = reinterpret_cast<u32*>(p);
    p += idx_bytes;
    d.off = reinterpret_cast<u32*>(p);
    d.out_cap = u32(out_bytes);
    d.status = sc->status;
    sc->status[0] = sc->status[1] = sc->status[2] = 0;
    launch_jpeg_transform(d, s);
    launch_jpeg_entropy(d, s);
    launch_jpeg_scan(d, s);
    launch_jpeg_gather(d, s);
    VEP_HIP(hipGetLastError());
    VEP_HIP(hipEventRecord(sc->ev, s));
    VEP_HIP(hipEventSynchronize(sc->ev));
    const u32 total = sc->status[1];
    if (!sc->status[0] && !sc->status[2] && total <= d.out_cap) {
      if (sc->host_cap < total) {
        if (sc->host) VEP_HIP(hipHostFree(sc->host));
        sc->host = nullptr;
        sc->host_cap = 0;
        const size_t cap = std::max<size_t>(size_t(total) * 2, size_t(1) << 20);
        VEP_HIP(hipHostMalloc(reinterpret_cast<void**>(&sc->host), cap, hipHostMallocDefault));
        sc->host_cap = cap;
      }
      if (total) {
        VEP_HIP(hipMemcpyAsync(sc->host, d.out, total, hipMemcpyDeviceToHost, s));
        VEP_HIP(hipEventRecord(sc->ev, s));
        VEP_HIP(hipEventSynchronize(sc->ev));
      }
      out = std::move(head);
      out.reserve(out.size() + total + 2);
      jpeg::append_segment(out, sc->host, total, d.intervals - 1, d.intervals);
      ok = true;
    }
  } catch (...) {
    release(sc);
    throw;
  }
  release(sc);
  return ok;
}

}  // namespace vep::gpu
