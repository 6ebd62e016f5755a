// Host side of the GPU tamper detector: the descriptor of a picture and the scratch set (kernel:
// gpu_tamper.hip).
#include "gpu.h"

namespace vep::gpu {

TamperDesc make_tamper_desc(const u8* src, size_t src_bytes, int w, int h, u32* hist, u32* sum_y, u32* energy,
                            size_t grid_cells, int cell) {
  TamperDesc d{};
  d.src = src;
  d.src_pitch = u32(w) * 3;
  d.hist = hist;
  d.sum_y = sum_y;
  d.energy = energy;
  d.w = w;
  d.h = h;
  d.cell = cell;
  check_tamper(d, src_bytes, grid_cells);
  return d;
}

void TamperSet::reserve(int ndescs, size_t res_words) {
  reserve_descs(ndescs);
  d_res.reserve(res_words, kResultFloor);
  h_res.reserve(res_words, kResultFloor);
}

void TamperSet::run(int n, size_t hist_words, size_t res_words, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(holds(n) && hist_words <= res_words && res_words <= d_res.cap && res_words <= h_res.cap,
            "tamper: more work than the set holds");
  upload_descs(n, s);
  if (hist_words) VEP_HIP(hipMemsetAsync(d_res.p, 0, hist_words * sizeof(u32), s));
  launch_tamper(d_descs.p, h_descs.p, n, s);
  if (res_words)  // (0: the results are the caller's own buffers)
    VEP_HIP(hipMemcpyAsync(h_res.p, d_res.p, res_words * sizeof(u32), hipMemcpyDeviceToHost, s));
  VEP_HIP(hipEventRecord(ev, s));
}

}  // namespace vep::gpu
