// Host side of the GPU dehazing: the scratch set (kernels: gpu_dehaze.hip).
#include "dehaze.h"
#include "gpu.h"

namespace vep::gpu {

DehazeDesc check_dehaze(const dehaze::Job& j) {
  dehaze::check_job(j);
  DehazeDesc d{};
  d.src = j.src;
  d.dst = j.dst;
  d.table = j.table;
  d.air = j.air;
  d.cell = j.cell;
  d.ab = reinterpret_cast<int2*>(j.ab);
  d.mean = reinterpret_cast<int2*>(j.mean);
  d.src_pitch = j.src_pitch;
  d.dst_pitch = j.dst_pitch;
  d.w = j.w;
  d.h = j.h;
  d.patch = j.p.patch;
  d.omega = j.p.omega;
  d.t0 = j.p.t0;
  d.radius = j.p.radius;
  d.strength = j.p.strength;
  return d;
}

size_t DehazeSet::plane_words(int w, int h) { return dehaze::plane_words(w, h) / 2; }

void DehazeSet::reserve(int ndescs, size_t words, size_t picture_bytes, size_t host_bytes) {
  reserve_descs(ndescs);
  planes.reserve(words, kResultFloor);
  picture.reserve(picture_bytes);
  host.reserve(host_bytes);
  h_air.reserve(4);
}

const u32* DehazeSet::put(int k, const u8* src, size_t src_bytes, u32 src_pitch, u8* dst, size_t dst_bytes, u32 dst_pitch,
                          int w, int h, const dehaze::Params& p, size_t& plane_at) {
  VEP_CHECK(k >= 0 && holds(k + 1), "dehaze: more descriptors than the set holds");
  VEP_CHECK(w >= dehaze::kMinSide && h >= dehaze::kMinSide && w <= dehaze::kMaxSide && h <= dehaze::kMaxSide,
            "dehaze: both sides must be 16..65535");
  const size_t words = plane_words(w, h);
  VEP_CHECK(plane_at + words <= planes.cap, "dehaze: more planes than the set holds");
  dehaze::Job j;
  j.src = src;
  j.src_bytes = src_bytes;
  j.src_pitch = src_pitch;
  j.dst = dst;
  j.dst_bytes = dst_bytes;
  j.dst_pitch = dst_pitch;
  j.w = w;
  j.h = h;
  j.p = p;
  dehaze::carve_planes(j, reinterpret_cast<u32*>(planes.p + plane_at));
  h_descs.p[k] = check_dehaze(j);
  plane_at += words;
  return j.air;
}

void DehazeSet::run(int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(holds(n), "dehaze: more descriptors than the set holds");
  upload_descs(n, s);
  launch_dehaze(d_descs.p, h_descs.p, n, s);
  VEP_HIP(hipEventRecord(ev, s));
}

}  // namespace vep::gpu
