// Host side of the GPU views: the descriptor of a view and the scratch set (kernel: gpu_dewarp.hip).
#include "dewarp.h"
#include "gpu.h"

namespace vep::gpu {

DewarpDesc make_dewarp_desc(const u8* src, size_t src_bytes, int w, int h, const i32* mesh, size_t mesh_pairs, u8* dst,
                            size_t dst_bytes, int ow, int oh, u32 pad_bgr) {
  VEP_CHECK(ow >= 1 && oh >= 1 && ow <= dewarp::kMaxOut && oh <= dewarp::kMaxOut, "view: width and height must be 1..4096");
  VEP_CHECK(w >= 1 && h >= 1 && w <= dewarp::kMaxSrc && h <= dewarp::kMaxSrc, "view: picture size must be 1..8192");
  DewarpDesc d{};
  d.src = src;
  d.dst = dst;
  d.mesh = mesh;
  d.src_pitch = u32(w) * 3;
  d.pw = w;
  d.ph = h;
  d.ow = u16(ow);
  d.oh = u16(oh);
  d.pad_bgr = pad_bgr;
  check_dewarp(d, src_bytes, mesh_pairs, dst_bytes);
  return d;
}

void DewarpSet::reserve(int ndescs, size_t mesh_words, size_t out_bytes, size_t host_bytes) {
  reserve_descs(ndescs);
  d_mesh.reserve(mesh_words);
  h_mesh.reserve(mesh_words);
  out.reserve(out_bytes);
  host.reserve(host_bytes);
}

void DewarpSet::run(int n, size_t mesh_words, size_t down_bytes, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(holds(n), "view: more descriptors than the set holds");
  VEP_CHECK(mesh_words <= d_mesh.cap && mesh_words <= h_mesh.cap, "view: more mesh words than the set holds");
  VEP_CHECK(down_bytes <= out.cap && down_bytes <= host.cap, "view: more bytes than the set holds");
  upload_descs(n, s);
  if (mesh_words) VEP_HIP(hipMemcpyAsync(d_mesh.p, h_mesh.p, mesh_words * sizeof(i32), hipMemcpyHostToDevice, s));
  launch_dewarp(d_descs.p, h_descs.p, n, s);
  if (down_bytes) VEP_HIP(hipMemcpyAsync(host.p, out.p, down_bytes, hipMemcpyDeviceToHost, s));
  VEP_HIP(hipEventRecord(ev, s));
}

}  // namespace vep::gpu
