// What more than one binding file needs, once: conversions between the data plane's types and the
// Python objects they cross the boundary as.
#pragma once
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "bind_ext.h"
#include "vep/crop.h"
#include "vep/overlay.h"
#include "vep/runtime.h"

namespace py = pybind11;
using namespace vep;

// The sides of a picture, 1..65535 each; the caller raises, with its own exception type and message.
inline bool picture_size_ok(py::ssize_t w, py::ssize_t h) { return w >= 1 && h >= 1 && w <= 65535 && h <= 65535; }
static_assert(motion::kMaxSide == 65535 && mask::kMaxSide == 65535, "picture_size_ok states every op's limit");
// An (H, W, 3) array of such sides.
inline bool is_bgr_picture(const py::array& a) {
  return a.ndim() == 3 && a.shape(2) == 3 && picture_size_ok(a.shape(1), a.shape(0));
}
// Per-channel mean and std (inverse: 1 / std) as the kernels take them; a list that has not 3 entries: 0 and 1.
inline void fill_mean_std(const std::vector<float>& mean, const std::vector<float>& stdv, float* m, float* s, bool inverse) {
  for (int k = 0; k < 3; ++k) {
    m[k] = mean.size() == 3 ? mean[size_t(k)] : 0.f;
    s[k] = stdv.size() == 3 ? stdv[size_t(k)] : 1.f;
    if (inverse) s[k] = 1.f / s[k];
  }
}

inline py::bytes to_bytes(const u8* p, size_t n) {
  return py::bytes(reinterpret_cast<const char*>(p), n);
}

// (y, uv) coded NV12 planes of a surface: uint8, or uint16 for high bit depth (HEVC Main10,
// H.264 High 10); 4:2:2 (NV16): the uv plane has coded_h rows
inline py::tuple surface_planes(const HostSurface& p) {
  auto planes_of = [&](const auto& sy, const auto& suv) -> py::tuple {
    using T = std::decay_t<decltype(sy[0])>;
    py::array_t<T> y({p.coded_h, p.coded_w}), uv({p.chroma_rows(), p.coded_w});
    std::memcpy(y.mutable_data(), sy.data(), sy.size() * sizeof(T));
    std::memcpy(uv.mutable_data(), suv.data(), suv.size() * sizeof(T));
    return py::make_tuple(y, uv);
  };
  return p.wide() ? planes_of(p.y16, p.uv16) : planes_of(p.y, p.uv);
}

inline py::dict meta_dict(const FrameMeta& m) {
  py::dict d;
  d["width"] = m.width;
  d["height"] = m.height;
  d["timestamp"] = m.timestamp;
  d["pts"] = m.pts;
  d["dts"] = m.dts;
  d["packet"] = m.packet;
  d["keyframe"] = m.keyframe;
  d["is_keyframe"] = m.is_keyframe;
  d["is_corrupt"] = m.is_corrupt;
  d["frame_type"] = std::string(1, m.frame_type);
  d["time_base"] = m.time_base;
  d["seq"] = m.seq;
  d["decoded_us"] = m.decoded_us;
  d["arrival_ms"] = m.arrival_ms;
  return d;
}

inline py::dict pic_dict(const PictureInfo& p) {
  py::dict d;
  d["width"] = p.width;
  d["height"] = p.height;
  d["coded_width"] = p.coded_width;
  d["coded_height"] = p.coded_height;
  d["pict_type"] = std::string(1, p.pict_type);
  d["idr"] = p.idr;
  d["frame_num"] = p.frame_num;
  d["coded_mbs"] = p.coded_mbs;
  d["fps"] = p.fps;
  return d;
}

inline py::dict domain_dict(const HostDomain& d) {
  py::dict o;
  o["device"] = d.device;
  o["index"] = d.index;
  o["numa_node"] = d.numa_node;
  o["pci_bus_id"] = d.pci_bus_id;
  o["cpus"] = d.cpus;
  o["cpulist"] = format_cpulist(d.cpus);
  o["cpu_share"] = d.cpu_share;
  o["parse_threads"] = d.parse_threads;
  o["io_threads"] = d.io_threads;
  o["source"] = d.source;
  return o;
}

inline HostDomain domain_from(const py::dict& o) {
  HostDomain d;
  auto get_i = [&](const char* k, int dflt) { return o.contains(k) ? o[k].cast<int>() : dflt; };
  d.device = get_i("device", -1);
  d.index = get_i("index", 0);
  d.numa_node = get_i("numa_node", -1);
  if (o.contains("pci_bus_id")) d.pci_bus_id = o["pci_bus_id"].cast<std::string>();
  if (o.contains("cpus")) d.cpus = o["cpus"].cast<std::vector<int>>();
  d.cpu_share = get_i("cpu_share", int(d.cpus.size()));
  d.parse_threads = get_i("parse_threads", 0);
  d.io_threads = get_i("io_threads", 1);
  if (o.contains("source")) d.source = o["source"].cast<std::string>();
  return d;
}

// Callers bind the result to a local (`auto cp = cam_ref(w, i)`) when the camera must outlive
// a GIL-released section; short accessors use cam_of.
inline std::shared_ptr<Camera> cam_ref(Worker& w, int idx) {
  std::shared_ptr<Camera> c = w.camera(idx);
  if (!c) throw py::index_error("no camera with index " + std::to_string(idx));
  return c;
}
inline Camera& cam_of(Worker& w, int idx) { return *cam_ref(w, idx); }

inline py::dict summary_dict(const motion::Summary& s) {
  py::dict d;
  d["changed"] = s.changed;
  d["active"] = s.active;
  if (s.has_box)
    d["box"] = py::make_tuple(s.x, s.y, s.w, s.h);
  else
    d["box"] = py::none();
  d["motion"] = s.motion;
  return d;
}

inline py::dict tamper_summary_dict(const tamper::Summary& s) {
  py::dict d;
  d["mean"] = s.n ? double(s.mean_sum) / double(s.n) : 0.0;
  d["mean_sum"] = s.mean_sum;
  d["p5"] = s.p5;
  d["p95"] = s.p95;
  d["energy_total"] = s.energy_total;
  d["pairs_total"] = s.pairs_total;
  d["sharpness"] = s.pairs_total ? double(s.energy_total) / double(s.pairs_total) : 0.0;
  d["has_reference"] = s.has_reference;
  d["cells"] = s.cells;
  d["shifted"] = s.shifted;
  d["dark"] = s.dark;
  d["bright"] = s.bright;
  d["flat"] = s.flat;
  d["defocused"] = s.defocused;
  d["moved"] = s.moved;
  d["tampered"] = s.tampered;
  py::list causes;
  if (s.dark) causes.append("dark");
  if (s.bright) causes.append("bright");
  if (s.flat) causes.append("flat");
  if (s.defocused) causes.append("defocused");
  if (s.moved) causes.append("moved");
  d["causes"] = causes;
  return d;
}

inline py::array_t<uint32_t> u32_array(const std::vector<u32>& v, py::ssize_t rows, py::ssize_t cols) {
  py::array_t<uint32_t> a = rows < 0 ? py::array_t<uint32_t>(py::ssize_t(v.size())) : py::array_t<uint32_t>({rows, cols});
  std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(uint32_t));
  return a;
}

inline py::dict tamper_dict(const TamperResult& r) {
  py::dict d = tamper_summary_dict(r.summary);
  d["seq"] = r.seq;
  d["width"] = r.width;
  d["height"] = r.height;
  d["cell"] = r.cell;
  d["cols"] = r.cols;
  d["rows"] = r.rows;
  d["hist"] = u32_array(r.hist, -1, 0);
  d["sum_y"] = u32_array(r.sum_y, r.rows, r.cols);
  d["energy"] = u32_array(r.energy, r.rows, r.cols);
  return d;
}

// Privacy masks cross the boundary as tuples (x0, y0, x1, y1, mode, block, b, g, r) of ints; an
// invalid list is a ValueError.
using MaskTuple = std::tuple<int, int, int, int, int, int, int, int, int>;
inline std::vector<mask::Mask> masks_of(const std::vector<MaskTuple>& v) {
  std::vector<mask::Mask> out;
  for (const MaskTuple& t : v) {
    mask::Mask m;
    std::tie(m.x0, m.y0, m.x1, m.y1, m.mode, m.block, m.b, m.g, m.r) = t;
    out.push_back(m);
  }
  try {
    VEP_CHECK(out.size() <= size_t(mask::kMaxMasks), "mask: at most 8 masks per camera");
    mask::check_list(out.data(), int(out.size()));
  } catch (const Error& e) {
    throw py::value_error(e.what());
  }
  return out;
}
inline std::vector<MaskTuple> mask_tuples(const std::vector<mask::Mask>& v) {
  std::vector<MaskTuple> out;
  for (const mask::Mask& m : v) out.emplace_back(m.x0, m.y0, m.x1, m.y1, m.mode, m.block, m.b, m.g, m.r);
  return out;
}

// Crop boxes cross the boundary as tuples (x0, y0, x1, y1) of ints, a pad colour as (b, g, r); an
// invalid list, output size, fit or colour is a ValueError.
using BoxTuple = std::tuple<int, int, int, int>;
using PadTuple = std::tuple<int, int, int>;
inline std::vector<crop::Box> boxes_of(const std::vector<BoxTuple>& v) {
  std::vector<crop::Box> out;
  for (const BoxTuple& t : v) {
    crop::Box b;
    std::tie(b.x0, b.y0, b.x1, b.y1) = t;
    out.push_back(b);
  }
  try {
    VEP_CHECK(out.size() <= size_t(crop::kMaxBoxes), "crop: at most 64 boxes per picture");
    crop::check_list(out.data(), int(out.size()));
  } catch (const Error& e) {
    throw py::value_error(e.what());
  }
  return out;
}
inline crop::Pad crop_output_of(int ow, int oh, int fit, const PadTuple& pad) {
  crop::Pad p;
  std::tie(p.b, p.g, p.r) = pad;
  try {
    crop::check_output(ow, oh, fit, p);
  } catch (const Error& e) {
    throw py::value_error(e.what());
  }
  return p;
}
// (n, oh, ow, 3) over the bytes of px, which the array takes over: no second copy of the crops
inline py::array_t<uint8_t> crops_array(std::vector<u8>& px, size_t n, int ow, int oh) {
  const std::vector<py::ssize_t> shape = {py::ssize_t(n), py::ssize_t(oh), py::ssize_t(ow), py::ssize_t(3)};
  if (px.empty()) return py::array_t<uint8_t>(shape);
  auto* keep = new std::vector<u8>(std::move(px));
  py::capsule owner(keep, [](void* p) { delete static_cast<std::vector<u8>*>(p); });
  return py::array_t<uint8_t>(shape, keep->data(), owner);
}

// Overlay items (vep/overlay.h) cross the boundary as tuples (kind, x0, y0, x1, y1, b, g, r, alpha,
// thickness, fill, scale, has_bg, bg_b, bg_g, bg_r, bg_alpha, text) of ints and one bytes (a text
// item's origin is (x0, y0)); an invalid list is a ValueError.
using ItemTuple = std::tuple<int, int, int, int, int, int, int, int, int, int, int, int, int, int, int, int, int, py::bytes>;
inline std::vector<overlay::Item> items_of(const std::vector<ItemTuple>& v) {
  std::vector<overlay::Item> out;
  for (const ItemTuple& t : v) {
    overlay::Item it;
    py::bytes text;
    std::tie(it.kind, it.x0, it.y0, it.x1, it.y1, it.b, it.g, it.r, it.alpha, it.thickness, it.fill, it.scale, it.has_bg,
             it.bg_b, it.bg_g, it.bg_r, it.bg_alpha, text) = t;
    it.text = std::string(text);
    out.push_back(std::move(it));
  }
  try {
    VEP_CHECK(out.size() <= size_t(overlay::kMaxItems), "overlay: at most 64 items per picture");
    overlay::check_list(out.data(), int(out.size()));
  } catch (const Error& e) {
    throw py::value_error(e.what());
  }
  return out;
}
inline overlay::Meta overlay_meta_of(const py::object& meta) {
  overlay::Meta m;
  if (meta.is_none()) return m;
  py::dict d = meta.cast<py::dict>();
  if (d.contains("seq")) m.seq = d["seq"].cast<i64>();
  if (d.contains("timestamp")) m.timestamp = d["timestamp"].cast<i64>();
  return m;
}
// The expansion of a list on a w x h picture; what expand refuses is a ValueError.
inline overlay::Expanded overlay_expand_of(const std::vector<overlay::Item>& items, int w, int h, const std::string& name,
                                           const overlay::Meta& meta) {
  try {
    return overlay::expand(items.data(), int(items.size()), w, h, name, meta);
  } catch (const Error& e) {
    throw py::value_error(e.what());
  }
}

inline tamper::Params tamper_params_of(int cell, int dark_level, int bright_level, int spread_min, int focus_percent,
                                       int shift_level, int shift_percent) {
  tamper::Params p;
  p.cell = cell;
  p.dark_level = dark_level;
  p.bright_level = bright_level;
  p.spread_min = spread_min;
  p.focus_percent = focus_percent;
  p.shift_level = shift_level;
  p.shift_percent = shift_percent;
  tamper::check_params(p);
  return p;
}

inline py::dict tamper_params_dict(const tamper::Params& p) {
  py::dict d;
  d["cell"] = p.cell;
  d["dark_level"] = p.dark_level;
  d["bright_level"] = p.bright_level;
  d["spread_min"] = p.spread_min;
  d["focus_percent"] = p.focus_percent;
  d["shift_level"] = p.shift_level;
  d["shift_percent"] = p.shift_percent;
  return d;
}

inline py::dict motion_dict(const MotionResult& r) {
  py::dict d = summary_dict(r.summary);
  d["seq"] = r.seq;
  d["width"] = r.width;
  d["height"] = r.height;
  d["cell"] = r.cell;
  d["cols"] = r.cols;
  d["rows"] = r.rows;
  d["threshold"] = r.threshold;
  d["primed"] = r.primed;
  d["counts"] = u32_array(r.counts, r.rows, r.cols);
  return d;
}
