// Host side of the GPU block matching: the checked descriptor and the scratch set (kernels:
// gpu_flow.hip).
#include "flow.h"
#include "gpu.h"

namespace vep::gpu {

FlowDesc check_flow(const flow::Job& j) {
  flow::check_job(j);
  // The luma kernel stages the rows and columns of its tiles, clipped to the d w' x d h' pixels the
  // planes are made of, and stores w' bytes of every plane row; the match kernel loads aligned
  // 16-byte vectors of the planes' rows (inside their pitch) and stores one record a block: the
  // spans check_job has proved.
  FlowDesc d{};
  const u32 pw = flow::plane_side(u32(j.w), u32(j.decimate)), ph = flow::plane_side(u32(j.h), u32(j.decimate));
  for (int k = 0; k < 2; ++k) {
    d.src[k] = j.src[k];
    d.src_pitch[k] = j.src_pitch[k];
    d.plane[k] = j.plane[k];
  }
  d.records = reinterpret_cast<uint2*>(j.records);
  d.plane_pitch = flow::plane_pitch(pw);
  d.w = j.w;
  d.h = j.h;
  d.pw = i32(pw);
  d.ph = i32(ph);
  d.decimate = j.decimate;
  d.range = j.range;
  return d;
}

size_t FlowSet::plane_bytes(int w, int h, int decimate) {
  const u32 pw = flow::plane_side(u32(w), u32(decimate)), ph = flow::plane_side(u32(h), u32(decimate));
  return 2 * ((size_t(flow::plane_pitch(pw)) * ph + 255) & ~size_t(255));
}

void FlowSet::reserve(int ndescs, size_t plane_bytes, size_t records) {
  reserve_descs(ndescs);
  // (never empty: a picture too small for one block still names a plane and a record address)
  planes.reserve(std::max<size_t>(plane_bytes, 256));
  d_records.reserve(std::max<size_t>(records, 1), kDescFloor);
  h_records.reserve(std::max<size_t>(records, 1), kDescFloor);
}

void FlowSet::put(int k, const u8* newer, const u8* older, size_t src_bytes, u32 pitch_newer, u32 pitch_older, int w, int h,
                  int decimate, int range, size_t& plane_at, size_t& record_at, flow::Record* records, size_t record_count) {
  VEP_CHECK(k >= 0 && holds(k + 1), "flow: more descriptors than the set holds");
  flow::check_match_params(decimate, range);
  VEP_CHECK(w >= 1 && h >= 1 && w <= flow::kMaxSide && h <= flow::kMaxSide, "flow: picture size must be 1..65535");
  const size_t half = plane_bytes(w, h, decimate) / 2;
  const size_t blocks = size_t(flow::blocks(flow::plane_side(u32(w), u32(decimate)))) *
                        flow::blocks(flow::plane_side(u32(h), u32(decimate)));
  VEP_CHECK(plane_at + 2 * half <= planes.cap, "flow: more planes than the set holds");
  flow::Job j;
  j.src[0] = newer;
  j.src[1] = older;
  j.src_bytes[0] = j.src_bytes[1] = src_bytes;
  j.src_pitch[0] = pitch_newer;
  j.src_pitch[1] = pitch_older;
  // (an empty plane still gets an aligned, non-null address inside or at the end of the buffer)
  j.plane[0] = planes.p + plane_at;
  j.plane[1] = planes.p + plane_at + half;
  j.plane_bytes[0] = j.plane_bytes[1] = half;
  if (records) {
    j.records = records;
    j.record_count = record_count;
  } else {
    VEP_CHECK(record_at + blocks <= d_records.cap, "flow: more records than the set holds");
    j.records = d_records.p + record_at;
    j.record_count = blocks;
  }
  j.w = w;
  j.h = h;
  j.decimate = decimate;
  j.range = range;
  h_descs.p[k] = check_flow(j);
  plane_at += 2 * half;
  record_at += blocks;
}

void FlowSet::run(int n, int decimate, int range, size_t records, hipStream_t s) {
  if (n <= 0) return;
  VEP_CHECK(holds(n) && records <= h_records.cap && records <= d_records.cap, "flow: more than the set holds");
  upload_descs(n, s);
  launch_flow(d_descs.p, h_descs.p, n, decimate, range, s);
  if (records)
    VEP_HIP(hipMemcpyAsync(h_records.p, d_records.p, records * sizeof(flow::Record), hipMemcpyDeviceToHost, s));
  VEP_HIP(hipEventRecord(ev, s));
}

}  // namespace vep::gpu
