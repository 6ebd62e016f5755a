// Host side of the GPU temporal denoising: the scratch set (kernel: gpu_denoise.hip).
#include "denoise.h"
#include "gpu.h"

namespace vep::gpu {

DenoiseDesc check_denoise(const denoise::Job& j) {
  denoise::check_job(j);
  // The kernel stages the rows and columns of a tile and its halo, clipped to the picture, of
  // every source, and stores the rows and columns of its tiles, clipped likewise: the spans
  // check_job has proved.
  DenoiseDesc d{};
  for (int k = 0; k < j.frames; ++k) {
    d.src[k] = j.src[k];
    d.src_pitch[k] = j.src_pitch[k];
  }
  d.dst = j.dst;
  d.dst_pitch = j.dst_pitch;
  d.w = j.w;
  d.h = j.h;
  d.frames = j.frames;
  d.level = j.level;
  d.strength = j.strength;
  d.recip9t = denoise::reciprocal(9u * u32(j.level));
  return d;
}

void DenoiseSet::reserve(int ndescs, size_t picture_bytes, size_t host_bytes) {
  reserve_descs(ndescs);
  picture.reserve(picture_bytes);
  host.reserve(host_bytes);
}

void DenoiseSet::put(int k, const denoise::Job& j) {
  VEP_CHECK(k >= 0 && holds(k + 1), "denoise: more descriptors than the set holds");
  h_descs.p[k] = check_denoise(j);
}

void DenoiseSet::run(int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(holds(n), "denoise: more descriptors than the set holds");
  upload_descs(n, s);
  launch_denoise(d_descs.p, h_descs.p, n, s);
  VEP_HIP(hipEventRecord(ev, s));
}

}  // namespace vep::gpu
