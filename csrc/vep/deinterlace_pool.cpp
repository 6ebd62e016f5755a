// Host side of the GPU deinterlacing: the scratch set (kernel: gpu_deinterlace.hip).
#include "deinterlace.h"
#include "gpu.h"

namespace vep::gpu {

DeinterlaceDesc check_deinterlace(const deinterlace::Job& j) {
  deinterlace::check_job(j);
  // The kernel stages the rows and columns of a tile and its halo, clipped to the picture, of
  // either source, and stores the rows and columns of its tiles, clipped likewise: the spans
  // check_job has proved.
  DeinterlaceDesc d{};
  d.newer = j.newer;
  d.newer_pitch = j.newer_pitch;
  if (deinterlace::temporal_of(j)) {
    d.older = j.older;
    d.older_pitch = j.older_pitch;
  }
  d.dst = j.dst;
  d.dst_pitch = j.dst_pitch;
  d.w = j.w;
  d.h = j.h;
  d.parity = j.p.order;
  return d;
}

void DeinterlaceSet::reserve(int ndescs, size_t picture_bytes, size_t host_bytes) {
  reserve_descs(ndescs);
  picture.reserve(picture_bytes);
  host.reserve(host_bytes);
}

void DeinterlaceSet::put(int k, const deinterlace::Job& j) {
  VEP_CHECK(k >= 0 && holds(k + 1), "deinterlace: more descriptors than the set holds");
  h_descs.p[k] = check_deinterlace(j);
}

void DeinterlaceSet::run(int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(holds(n), "deinterlace: more descriptors than the set holds");
  upload_descs(n, s);
  launch_deinterlace(d_descs.p, h_descs.p, n, s);
  VEP_HIP(hipEventRecord(ev, s));
}

}  // namespace vep::gpu
