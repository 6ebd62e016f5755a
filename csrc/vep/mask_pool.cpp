// Host side of the GPU privacy masks: the descriptor set (kernel: gpu_mask.hip).
#include "gpu.h"
#include "mask.h"

namespace vep::gpu {

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

void MaskSet::run(int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(holds(n), "mask: more work than the set holds");
  upload_descs(n, s);
  for (int level = 0; level < mask::kMaxMasks; ++level) launch_mask(d_descs.p, h_descs.p, n, level, s);
  VEP_HIP(hipEventRecord(ev, s));
}

}  // namespace vep::gpu
