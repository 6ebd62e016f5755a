// Host side of the GPU orientation: the scratch set (kernel: gpu_orient.hip).
#include "gpu.h"
#include "orient.h"

namespace vep::gpu {

OrientDesc check_orient(const orient::Job& j) {
  orient::check_job(j);
  // The kernel stages the source rows and columns that a tile of the output maps to, clipped to
  // the picture, and stores the rows and columns of its tiles, clipped likewise: the spans
  // check_job has proved.
  OrientDesc d{};
  d.src = j.src;
  d.src_pitch = j.src_pitch;
  d.dst = j.dst;
  d.dst_pitch = j.dst_pitch;
  d.w = j.w;
  d.h = j.h;
  d.op = j.op;
  return d;
}

void OrientSet::reserve(int ndescs, size_t picture_bytes, size_t host_bytes) {
  reserve_descs(ndescs);
  picture.reserve(picture_bytes);
  host.reserve(host_bytes);
}

void OrientSet::put(int k, const orient::Job& j) {
  VEP_CHECK(k >= 0 && holds(k + 1), "orient: more descriptors than the set holds");
  h_descs.p[k] = check_orient(j);
}

void OrientSet::run(int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(holds(n), "orient: more descriptors than the set holds");
  upload_descs(n, s);
  launch_orient(d_descs.p, h_descs.p, n, s);
  VEP_HIP(hipEventRecord(ev, s));
}

}  // namespace vep::gpu
