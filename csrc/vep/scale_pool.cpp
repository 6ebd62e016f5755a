// Host side of the GPU scaler: the scratch set (kernel: gpu_scale.hip).
#include "gpu.h"

namespace vep::gpu {

void ScaleSet::reserve(size_t canvas_bytes, int ndescs, size_t upload_bytes) {
  ev.ensure();
  canvas.reserve(canvas_bytes);
  reserve_descs(ndescs);
  upload.reserve(upload_bytes);
}

void ScaleSet::run(int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(holds(n), "scale: more descriptors than the set holds");
  upload_descs(n, s);
  launch_scale(d_descs.p, h_descs.p, n, s);
  VEP_HIP(hipEventRecord(ev, s));
}

}  // namespace vep::gpu
