// Host side of the GPU moving-object boxes: the checked descriptors and the scratch set (kernels:
// gpu_objects.hip, and gpu_flow.hip's luma kernel).
#include <algorithm>

#include "gpu.h"
#include "objects.h"

namespace vep::gpu {

ObjectsJobDescs check_objects(const objects::Job& j) {
  objects::check_job(j);
  // The luma kernel stages the rows and columns of its tiles, clipped to the d w' x d h' pixels the
  // planes are made of, and stores w' bytes of every plane row. The mask kernel loads single bytes of
  // both planes at (x, y) inside w' x h', stores the words of rows below h' (a row's words cover
  // ceil(w' / 64) tiles) and the label and area words of samples inside w' x h'; the later kernels
  // touch label and area words at indices below w' h' only (a parent is a sample's index), records
  // at slots below the capacity, and the count: the spans check_job has proved.
  const u32 pw = flow::plane_side(u32(j.w), u32(j.decimate)), ph = flow::plane_side(u32(j.h), u32(j.decimate));
  const u64 cap = objects::capacity(pw, ph, u32(j.min_area));
  VEP_CHECK(cap <= (u64(1) << 30), "objects: too many records");
  ObjectsJobDescs out{};
  FlowDesc& f = out.luma;
  ObjectsDesc& d = out.objects;
  for (int k = 0; k < 2; ++k) {
    f.src[k] = j.src[k];
    f.src_pitch[k] = j.src_pitch[k];
    f.plane[k] = j.plane[k];
    d.plane[k] = j.plane[k];
  }
  f.records = nullptr;  // (the match kernel is not launched)
  f.plane_pitch = d.plane_pitch = flow::plane_pitch(pw);
  f.w = j.w;
  f.h = j.h;
  f.pw = d.pw = i32(pw);
  f.ph = d.ph = i32(ph);
  f.decimate = j.decimate;
  f.range = flow::kMinRange;
  d.mask = j.mask;
  d.labels = j.labels;
  d.area = j.area;
  d.records = reinterpret_cast<u32*>(j.records);
  d.count = j.count;
  d.words = objects::mask_words(pw);
  d.capacity = u32(cap);
  d.threshold = j.threshold;
  d.open = j.open;
  d.grow = j.grow;
  d.min_area = j.min_area;
  return out;
}

namespace {
size_t round256(size_t n) { return (n + 255) & ~size_t(255); }
struct Layout {
  size_t half, mask, plane;  // bytes of one luma plane, of the mask, of the label (or area) plane
  size_t total() const { return 2 * half + mask + 2 * plane; }
};
Layout layout_of(int w, int h, int decimate) {
  const u32 pw = flow::plane_side(u32(w), u32(decimate)), ph = flow::plane_side(u32(h), u32(decimate));
  return {round256(size_t(flow::plane_pitch(pw)) * ph), round256(size_t(objects::mask_words(pw)) * ph * 8),
          round256(size_t(pw) * ph * 4)};
}
}  // namespace

size_t ObjectsSet::scratch_bytes(int w, int h, int decimate) { return layout_of(w, h, decimate).total(); }

size_t ObjectsSet::capacity(int w, int h, int decimate, int min_area) {
  return size_t(objects::capacity(flow::plane_side(u32(w), u32(decimate)), flow::plane_side(u32(h), u32(decimate)), u32(min_area)));
}

void ObjectsSet::reserve(int ndescs, size_t bytes, size_t records) {
  reserve_descs(ndescs);
  d_luma.reserve(size_t(ndescs), kDescFloor);
  h_luma.reserve(size_t(ndescs), kDescFloor);
  d_counts.reserve(size_t(ndescs), kDescFloor);
  h_counts.reserve(size_t(ndescs), kDescFloor);
  // (never empty: an empty plane still names addresses)
  scratch.reserve(std::max<size_t>(bytes, 256));
  d_records.reserve(std::max<size_t>(records, 1), kDescFloor);
  h_records.reserve(std::max<size_t>(records, 1), kDescFloor);
}

void ObjectsSet::put(int k, const u8* newer, const u8* older, size_t src_bytes, u32 pitch_newer, u32 pitch_older, int w, int h,
                     const objects::Params& p, size_t& scratch_at, size_t& record_at) {
  VEP_CHECK(k >= 0 && holds(k + 1) && size_t(k) < h_luma.cap && size_t(k) < d_counts.cap, "objects: more descriptors than the set holds");
  objects::check_label_params(p.decimate, p.threshold, p.open, p.grow, p.min_area);
  VEP_CHECK(w >= 1 && h >= 1 && w <= objects::kMaxSide && h <= objects::kMaxSide, "objects: picture size must be 1..65535");
  const Layout l = layout_of(w, h, p.decimate);
  const size_t cap = capacity(w, h, p.decimate, p.min_area);
  VEP_CHECK(scratch_at + l.total() <= scratch.cap && record_at + cap <= d_records.cap, "objects: more scratch than the set holds");
  objects::Job j;
  j.src[0] = newer;
  j.src[1] = older;
  j.src_bytes[0] = j.src_bytes[1] = src_bytes;
  j.src_pitch[0] = pitch_newer;
  j.src_pitch[1] = pitch_older;
  u8* at = scratch.p + scratch_at;
  j.plane[0] = at;
  j.plane[1] = at + l.half;
  j.plane_bytes[0] = j.plane_bytes[1] = l.half;
  j.mask = reinterpret_cast<u64*>(at + 2 * l.half);
  j.mask_count = l.mask / 8;
  j.labels = reinterpret_cast<u32*>(at + 2 * l.half + l.mask);
  j.area = reinterpret_cast<u32*>(at + 2 * l.half + l.mask + l.plane);
  j.sample_count = l.plane / 4;
  j.records = d_records.p + record_at;
  j.record_count = cap;
  j.count = d_counts.p + k;
  j.w = w;
  j.h = h;
  j.decimate = p.decimate;
  j.threshold = p.threshold;
  j.open = p.open;
  j.grow = p.grow;
  j.min_area = p.min_area;
  const ObjectsJobDescs d = check_objects(j);
  h_luma.p[k] = d.luma;
  h_descs.p[k] = d.objects;
  scratch_at += l.total();
  record_at += cap;
}

void ObjectsSet::run(int n, int decimate, hipStream_t s, bool own_counts) {
  if (n <= 0) return;
  VEP_CHECK(holds(n) && size_t(n) <= h_luma.cap && size_t(n) <= h_counts.cap, "objects: more than the set holds");
  upload_descs(n, s);
  VEP_HIP(hipMemcpyAsync(d_luma.p, h_luma.p, size_t(n) * sizeof(FlowDesc), hipMemcpyHostToDevice, s));
  launch_flow_luma(d_luma.p, h_luma.p, n, decimate, s);
  launch_objects(d_descs.p, h_descs.p, n, s);
  if (own_counts) VEP_HIP(hipMemcpyAsync(h_counts.p, d_counts.p, size_t(n) * sizeof(u32), hipMemcpyDeviceToHost, s));
  VEP_HIP(hipEventRecord(ev, s));
}

void ObjectsSet::fetch(int n, hipStream_t s, std::vector<size_t>& at) {
  at.assign(size_t(std::max(n, 0)) + 1, 0);
  bool any = false;
  for (int k = 0; k < n; ++k) {
    const u32 c = h_counts.p[k];
    VEP_CHECK(c <= h_descs.p[k].capacity, "objects: a count above the capacity bound");
    at[size_t(k) + 1] = at[size_t(k)] + c;
    if (!c) continue;
    VEP_CHECK(at[size_t(k) + 1] <= h_records.cap, "objects: more records than the set holds");
    VEP_HIP(hipMemcpyAsync(h_records.p + at[size_t(k)], h_descs.p[k].records, size_t(c) * sizeof(objects::Record),
                           hipMemcpyDeviceToHost, s));
    any = true;
  }
  if (!any) return;
  VEP_HIP(hipEventRecord(ev, s));
  VEP_HIP(hipEventSynchronize(ev));
  for (int k = 0; k < n; ++k)
    std::sort(h_records.p + at[size_t(k)], h_records.p + at[size_t(k) + 1],
              [](const objects::Record& a, const objects::Record& b) { return a.label < b.label; });
}

}  // namespace vep::gpu
