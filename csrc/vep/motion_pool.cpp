// Host side of the GPU motion detector: the descriptor of a picture and the scratch set (kernel:
// gpu_motion.hip).
#include "gpu.h"

namespace vep::gpu {

MotionDesc make_motion_desc(const u8* src, size_t src_bytes, int w, int h, const u16* bg_in, u16* bg_out, u32 bg_pitch,
                            size_t bg_samples, u32* counts, size_t count_cells, int cell, int threshold,
                            int learn_shift) {
  MotionDesc d{};
  d.src = src;
  d.src_pitch = u32(w) * 3;
  d.bg_in = bg_in;
  d.bg_out = bg_out;
  d.bg_pitch = bg_pitch;
  d.counts = counts;
  d.w = w;
  d.h = h;
  d.cell = cell;
  d.threshold = threshold;
  d.learn_shift = learn_shift;
  check_motion(d, src_bytes, bg_samples, count_cells);
  return d;
}

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
