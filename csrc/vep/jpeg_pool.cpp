// Host side of the GPU JPEG encoder: the launch sequence of one picture on a pooled scratch set
// (kernels: gpu_jpeg.hip).
#include <algorithm>

#include "gpu.h"
#include "jpeg.h"

namespace vep::gpu {

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
  Lease sc = acquire();
  sc->ev.ensure();
  sc->status.reserve(16, 16);
  sc->dev.reserve(need);  // first use, or a larger picture
  u8* p = sc->dev.p;
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
  u32* status = sc->status.p;
  d.status = status;
  status[0] = status[1] = status[2] = 0;
  launch_jpeg_transform(d, s);
  launch_jpeg_entropy(d, s);
  launch_jpeg_scan(d, s);
  launch_jpeg_gather(d, s);
  VEP_HIP(hipGetLastError());
  VEP_HIP(hipEventRecord(sc->ev, s));
  VEP_HIP(hipEventSynchronize(sc->ev));
  const u32 total = status[1];
  if (status[0] || status[2] || total > d.out_cap) return false;
  sc->host.reserve(total, std::max<size_t>(size_t(total) * 2, size_t(1) << 20));
  if (total) {
    VEP_HIP(hipMemcpyAsync(sc->host.p, d.out, total, hipMemcpyDeviceToHost, s));
    VEP_HIP(hipEventRecord(sc->ev, s));
    VEP_HIP(hipEventSynchronize(sc->ev));
  }
  out = std::move(head);
  out.reserve(out.size() + total + 2);
  jpeg::append_segment(out, sc->host.p, total, d.intervals - 1, d.intervals);
  return true;
}

}  // namespace vep::gpu
