// Host side of the GPU motion detector: the scratch set (kernel: gpu_motion.hip).
#include "gpu.h"

namespace vep::gpu {

void MotionSet::reserve(int ndescs, size_t count_cells) {
  reserve_descs(ndescs);
  d_counts.reserve(count_cells, kResultFloor);
  h_counts.reserve(count_cells, kResultFloor);
}

void MotionSet::run(int n, size_t count_cells, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(holds(n) && count_cells <= d_counts.cap && count_cells <= h_counts.cap,
            "motion: more work than the set holds");
  upload_descs(n, s);
  launch_motion(d_descs.p, h_descs.p, n, s);
  if (count_cells)  // (0: the counts are the caller's own buffers)
    VEP_HIP(hipMemcpyAsync(h_counts.p, d_counts.p, count_cells * sizeof(u32), hipMemcpyDeviceToHost, s));
  VEP_HIP(hipEventRecord(ev, s));
}

}  // namespace vep::gpu
