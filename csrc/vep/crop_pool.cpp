// Host side of the GPU crops: the descriptor of a box and the scratch set (kernel: gpu_crop.hip).
#include "crop.h"
#include "gpu.h"

namespace vep::gpu {

CropDesc make_crop_desc(const u8* src, size_t src_bytes, int w, int h, const mask::Rect& rect, u8* dst,
                        size_t dst_bytes, int ow, int oh, int fit, u32 pad_bgr) {
  VEP_CHECK(ow >= 1 && oh >= 1 && ow <= crop::kMaxOut && oh <= crop::kMaxOut, "crop: width and height must be 1..4096");
  VEP_CHECK(rect.x0 < rect.x1 && rect.y0 < rect.y1, "crop: empty rect");
  const crop::Placement p = crop::fitted(rect.x1 - rect.x0, rect.y1 - rect.y0, ow, oh, fit);
  CropDesc d{};
  d.src = src;
  d.dst = dst;
  d.src_pitch = u32(w) * 3;
  d.pw = w;
  d.ph = h;
  d.x0 = rect.x0;
  d.y0 = rect.y0;
  d.x1 = rect.x1;
  d.y1 = rect.y1;
  d.ow = u16(ow);
  d.oh = u16(oh);
  d.fx = u16(p.x);
  d.fy = u16(p.y);
  d.fw = u16(p.w);
  d.fh = u16(p.h);
  d.pad_bgr = pad_bgr;
  check_crop(d, src_bytes, dst_bytes);
  return d;
}

void CropSet::reserve(int ndescs, size_t out_bytes, size_t host_bytes) {
  reserve_descs(ndescs);
  out.reserve(out_bytes);
  host.reserve(host_bytes);
}

void CropSet::run(int n, size_t down_bytes, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(holds(n), "crop: more descriptors than the set holds");
  VEP_CHECK(down_bytes <= out.cap && down_bytes <= host.cap, "crop: more bytes than the set holds");
  upload_descs(n, s);
  launch_crop(d_descs.p, h_descs.p, n, s);
  if (down_bytes) VEP_HIP(hipMemcpyAsync(host.p, out.p, down_bytes, hipMemcpyDeviceToHost, s));
  VEP_HIP(hipEventRecord(ev, s));
}

}  // namespace vep::gpu
