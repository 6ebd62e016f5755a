// Host side of the GPU contrast enhancement: the scratch set (kernels: gpu_clahe.hip).
#include "clahe.h"
#include "gpu.h"

namespace vep::gpu {

void ClaheSet::reserve(int ndescs, size_t tiles, size_t picture_bytes, size_t host_bytes) {
  reserve_descs(ndescs);
  hist.reserve(tiles * clahe::kBins, kResultFloor);
  lut.reserve(tiles * clahe::kBins, kResultFloor);
  picture.reserve(picture_bytes);
  host.reserve(host_bytes);
}

void ClaheSet::put(int k, const u8* src, size_t src_bytes, u32 src_pitch, u8* dst, size_t dst_bytes, u32 dst_pitch, int w,
                   int h, const clahe::Params& p, size_t& tile_at) {
  VEP_CHECK(k >= 0 && holds(k + 1), "enhance: more descriptors than the set holds");
  clahe::check_params(p);
  VEP_CHECK(w >= 1 && h >= 1 && w <= clahe::kMaxSide && h <= clahe::kMaxSide, "enhance: picture size must be 1..65535");
  const size_t tiles = clahe_tiles(w, h, p.tile), words = tiles * clahe::kBins;
  VEP_CHECK((tile_at + tiles) * clahe::kBins <= hist.cap && (tile_at + tiles) * clahe::kBins <= lut.cap,
            "enhance: more tiles than the set holds");
  ClaheDesc d{};
  d.src = src;
  d.dst = dst;
  d.hist = hist.p + tile_at * clahe::kBins;
  d.lut = lut.p + tile_at * clahe::kBins;
  d.src_pitch = src_pitch;
  d.dst_pitch = dst_pitch;
  d.w = w;
  d.h = h;
  d.tile = p.tile;
  d.clip16 = p.clip16;
  d.strength = p.strength;
  check_clahe(d, src_bytes, dst_bytes, words, words);
  h_descs.p[k] = d;
  tile_at += tiles;
}

void ClaheSet::run(int n, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(holds(n), "enhance: more descriptors than the set holds");
  upload_descs(n, s);
  launch_clahe(d_descs.p, h_descs.p, n, s);
  VEP_HIP(hipEventRecord(ev, s));
}

}  // namespace vep::gpu
