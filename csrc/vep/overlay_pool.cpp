// Host side of the GPU overlay: the scratch set and a picture's descriptor (kernel: gpu_overlay.hip).
#include <cstring>

#include "gpu.h"
#include "overlay.h"

namespace vep::gpu {

void OverlaySet::reserve(int ndescs, size_t nprims, size_t text_bytes, size_t picture_bytes) {
  reserve_descs(ndescs);
  d_prims.reserve(nprims, size_t(overlay::kMaxPrims));
  h_prims.reserve(nprims, size_t(overlay::kMaxPrims));
  d_text.reserve(text_bytes, size_t(overlay::kMaxPool));
  h_text.reserve(text_bytes, size_t(overlay::kMaxPool));
  picture.reserve(picture_bytes);
}

void OverlaySet::put(int k, const u8* src, size_t src_bytes, u32 src_pitch, u8* dst, size_t dst_bytes, u32 dst_pitch,
                     int w, int h, const overlay::Expanded& e, size_t& prim_at, size_t& text_at) {
  const size_t np = e.prims.size(), nt = e.text.size();
  VEP_CHECK(holds(k + 1) && prim_at + np <= h_prims.cap && prim_at + np <= d_prims.cap && text_at + nt <= h_text.cap &&
                text_at + nt <= d_text.cap,
            "overlay: more than the set holds");
  if (np) std::memcpy(h_prims.p + prim_at, e.prims.data(), np * sizeof(overlay::Prim));
  if (nt) std::memcpy(h_text.p + text_at, e.text.data(), nt);
  OverlayDesc d{};
  d.src = src;
  d.dst = dst;
  d.prims = d_prims.p + prim_at;
  d.text = d_text.p + text_at;
  d.src_pitch = src_pitch;
  d.dst_pitch = dst_pitch;
  d.w = w;
  d.h = h;
  d.nprims = u32(np);
  d.text_len = u32(nt);
  check_overlay(d, src_bytes, dst_bytes, h_prims.p + prim_at, h_text.p + text_at);
  h_descs.p[k] = d;
  prim_at += np;
  text_at += nt;
}

void OverlaySet::run(int n, size_t nprims, size_t text_bytes, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(holds(n) && nprims <= d_prims.cap && nprims <= h_prims.cap && text_bytes <= d_text.cap &&
                text_bytes <= h_text.cap,
            "overlay: more than the set holds");
  upload_descs(n, s);
  if (nprims)
    VEP_HIP(hipMemcpyAsync(d_prims.p, h_prims.p, nprims * sizeof(overlay::Prim), hipMemcpyHostToDevice, s));
  if (text_bytes) VEP_HIP(hipMemcpyAsync(d_text.p, h_text.p, text_bytes, hipMemcpyHostToDevice, s));
  launch_overlay(d_descs.p, h_descs.p, n, s);
  VEP_HIP(hipEventRecord(ev, s));
}

}  // namespace vep::gpu
