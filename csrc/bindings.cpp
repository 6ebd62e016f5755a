// pybind11 bindings of the vep native data plane (module `video_edge_ai_proxy_amd._vep`).
// Every call that can block (decode, D2H, network) releases the GIL.
#include <malloc.h>

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "vep/hostprof.h"
#include "vep/avc.h"
#include "vep/avc_cavlc.h"
#include "vep/avc_recon.h"
#include "vep/bench_driver.h"
#include "vep/cabac.h"
#include "vep/codec.h"
#include "vep/crop.h"
#include "vep/overlay.h"
#include "vep/gpu.h"
#include "vep/h264.h"
#include "vep/hevc_ctu.h"
#include "vep/hevc_dec.h"
#include "vep/hevc_kern.h"
#include "vep/jpeg.h"
#include "vep/scale.h"
#include "bind_ext.h"
#include "vep/runtime.h"
#include "vep/synth.h"

namespace py = pybind11;
using namespace vep;

// Scratch of the ops on caller-owned device buffers: one process-wide pool per device and op,
// created under a lock on first use, never freed, then used without the lock.
template <class Pool>
static Pool& pool_of_current_device() {
  static std::mutex mu;
  static std::map<int, Pool*>* pools = new std::map<int, Pool*>();  // (never freed)
  int dev = 0;
  VEP_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> g(mu);
  Pool*& slot = (*pools)[dev];
  if (!slot) slot = new Pool();
  return *slot;
}

static py::bytes to_bytes(const u8* p, size_t n) {
  return py::bytes(reinterpret_cast<const char*>(p), n);
}

// (y, uv) coded NV12 planes of a surface: uint8, or uint16 for high bit depth (HEVC Main10,
// H.264 High 10); 4:2:2 (NV16): the uv plane has coded_h rows
static py::tuple surface_planes(const HostSurface& p) {
  if (p.wide()) {
    py::array_t<uint16_t> y({p.coded_h, p.coded_w});
    py::array_t<uint16_t> uv({p.chroma_rows(), p.coded_w});
    std::memcpy(y.mutable_data(), p.y16.data(), p.y16.size() * 2);
    std::memcpy(uv.mutable_data(), p.uv16.data(), p.uv16.size() * 2);
    return py::make_tuple(y, uv);
  }
  py::array_t<uint8_t> y({p.coded_h, p.coded_w});
  py::array_t<uint8_t> uv({p.chroma_rows(), p.coded_w});
  std::memcpy(y.mutable_data(), p.y.data(), p.y.size());
  std::memcpy(uv.mutable_data(), p.uv.data(), p.uv.size());
  return py::make_tuple(y, uv);
}

static py::dict meta_dict(const FrameMeta& m) {
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

// Worst case of a VideoFrame's trailer (everything after the pixel data): 7 varint fields
// (<= 11 B each), 2 bools, frame_type, time_base, shape, device_id.
static py::dict pic_dict(const PictureInfo& p) {
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

// Callers bind the result to a local (`auto cp = cam_ref(w, i)`) when the camera must outlive
// a GIL-released section; short accessors use cam_of.
static py::dict domain_dict(const HostDomain& d) {
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

static HostDomain domain_from(const py::dict& o) {
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

static std::shared_ptr<Camera> cam_ref(Worker& w, int idx) {
  std::shared_ptr<Camera> c = w.camera(idx);
  if (!c) throw py::index_error("no camera with index " + std::to_string(idx));
  return c;
}
static Camera& cam_of(Worker& w, int idx) { return *cam_ref(w, idx); }

static py::dict summary_dict(const motion::Summary& s) {
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

static py::dict tamper_summary_dict(const tamper::Summary& s) {
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

static py::array_t<uint32_t> u32_array(const std::vector<u32>& v, py::ssize_t rows, py::ssize_t cols) {
  py::array_t<uint32_t> a = rows < 0 ? py::array_t<uint32_t>(py::ssize_t(v.size())) : py::array_t<uint32_t>({rows, cols});
  std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(uint32_t));
  return a;
}

static py::dict tamper_dict(const TamperResult& r) {
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
static std::vector<mask::Mask> masks_of(const std::vector<MaskTuple>& v) {
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
static std::vector<MaskTuple> mask_tuples(const std::vector<mask::Mask>& v) {
  std::vector<MaskTuple> out;
  for (const mask::Mask& m : v) out.emplace_back(m.x0, m.y0, m.x1, m.y1, m.mode, m.block, m.b, m.g, m.r);
  return out;
}

// Crop boxes cross the boundary as tuples (x0, y0, x1, y1) of ints, a pad colour as (b, g, r); an
// invalid list, output size, fit or colour is a ValueError.
using BoxTuple = std::tuple<int, int, int, int>;
using PadTuple = std::tuple<int, int, int>;
static std::vector<crop::Box> boxes_of(const std::vector<BoxTuple>& v) {
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
static crop::Pad crop_output_of(int ow, int oh, int fit, const PadTuple& pad) {
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
static py::array_t<uint8_t> crops_array(std::vector<u8>& px, size_t n, int ow, int oh) {
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
static std::vector<overlay::Item> items_of(const std::vector<ItemTuple>& v) {
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
static overlay::Meta overlay_meta_of(const py::object& meta) {
  overlay::Meta m;
  if (meta.is_none()) return m;
  py::dict d = meta.cast<py::dict>();
  if (d.contains("seq")) m.seq = d["seq"].cast<i64>();
  if (d.contains("timestamp")) m.timestamp = d["timestamp"].cast<i64>();
  return m;
}
// The expansion of a list on a w x h picture; what expand refuses is a ValueError.
static overlay::Expanded overlay_expand_of(const std::vector<overlay::Item>& items, int w, int h, const std::string& name,
                                           const overlay::Meta& meta) {
  try {
    return overlay::expand(items.data(), int(items.size()), w, h, name, meta);
  } catch (const Error& e) {
    throw py::value_error(e.what());
  }
}

static tamper::Params tamper_params_of(int cell, int dark_level, int bright_level, int spread_min, int focus_percent,
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

static py::dict tamper_params_dict(const tamper::Params& p) {
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

static py::dict motion_dict(const MotionResult& r) {
  py::dict d = summary_dict(r.summary);
  d["seq"] = r.seq;
  d["width"] = r.width;
  d["height"] = r.height;
  d["cell"] = r.cell;
  d["cols"] = r.cols;
  d["rows"] = r.rows;
  d["threshold"] = r.threshold;
  d["primed"] = r.primed;
  py::array_t<uint32_t> counts({py::ssize_t(r.rows), py::ssize_t(r.cols)});
  std::memcpy(counts.mutable_data(), r.counts.data(), r.counts.size() * sizeof(uint32_t));
  d["counts"] = counts;
  return d;
}

// Stateful oracle: parse + CPU reconstruct a sequence of AUs, return the final BGR picture.
// Streams inside the I_PCM / P_Skip subset take the fast-path parser; anything else switches to
// the general H.264 decoder (avc.h) for good, like a Camera does.
struct CpuDecoder {
  StreamParser parser;
  MbUpdate upd;
  HostSurface surf;
  PictureInfo last;
  avc::Decoder avc;
  std::vector<HostSurface> slots;
  bool general = false;
  int target = 0;
  int coded = 0;
  bool fields_out = false;  // the newest output is a field pair (woven into `woven`)
  HostSurface woven;
  mutable HostSurface weave_tmp;
  const HostSurface& out() const { return general ? (fields_out ? woven : slots[size_t(target)]) : surf; }
  // samples of an output frame (a field pair: its two field slots woven)
  const HostSurface& frame_of(const avc::OutFrame& f) const {
    if (!f.fields) return slots[size_t(f.slot)];
    avc::weave_fields(slots[2 * size_t(f.slot)], slots[2 * size_t(f.slot) + 1], weave_tmp);
    return weave_tmp;
  }
  py::object decode(const AccessUnit& au) {
    bool no_output = false;
    {
      py::gil_scoped_release nogil;
      bool done = false;
      if (!general) {
        try {
          upd.clear_payload();  // `au` outlives this call: src pointers into it are safe
          last = parser.parse(au, upd);
          if (surf.coded_w != last.coded_width || surf.coded_h != last.coded_height)
            surf.alloc(last.coded_width, last.coded_height);
          cpu_apply_update(upd, surf);
          coded = upd.nslots;
          done = true;
        } catch (const UnsupportedStream&) {
          if (au.codec != Codec::kH264) throw;
          general = true;
        }
      }
      std::vector<avc::OutFrame> outs;
      size_t nal = 0;  // (a field pair may come as one access unit: one picture per field)
      while (!done) {
        avc::PicturePtr pic = avc.parse(au, 0, &nal);
        done = nal >= au.nals.size();
        if (slots.size() < size_t(pic->dpb_slots)) slots.resize(size_t(pic->dpb_slots));
        for (auto& h : slots)
          if (h.coded_w != pic->wmbs * 16 || h.coded_h != pic->hmbs * 16 || h.bd != pic->bd || h.cf != pic->cf)
            h.alloc(pic->wmbs * 16, pic->hmbs * 16, pic->bd, pic->cf);
        avc::cpu_reconstruct(*pic, slots);
        coded = pic->info.coded_mbs;
        pictures.push_back(pic->info);
        for (const avc::MbRec& m : pic->mbs) {
          ++kinds[m.kind];
          if (m.flags & avc::kMbT8x8) ++t8x8;
          if (m.flags & avc::kMbWp) ++weighted;
          if (m.kind <= avc::kInter) {
            bool bi = false, l1only = false;
            for (int k = 0; k < 4; ++k) {
              bi |= m.ref[k] != 0xFF && m.ref1[k] != 0xFF;
              l1only |= m.ref[k] == 0xFF && m.ref1[k] != 0xFF;
            }
            bipred += bi;
            list1_only += l1only;
          }
        }
        outs.insert(outs.end(), pic->outputs.begin(), pic->outputs.end());
        if (!done) continue;
        // B-frame reordering: the newest frame that left the reorder buffer, if any
        pending_outputs = outs;
        no_output = outs.empty();
        if (!no_output) {
          last = outs.back().info;
          target = outs.back().slot;
          fields_out = outs.back().fields;
          if (fields_out) woven = frame_of(outs.back());
          last_poc = outs.back().poc;
          last_pts = outs.back().au.pts;
        }
      }
    }
    if (no_output) return py::none();
    py::array_t<uint8_t> o({last.height, last.width, 3});
    cpu_nv12_to_bgr(out(), last.crop_left, last.crop_top, last.width, last.height, o.mutable_data());
    return o;
  }
  // Every frame that left the reorder buffer with the last decode() (or, after flush_frames(),
  // at end of stream): [(pts, (Y, UV) coded NV12 planes)] in output order.
  py::list frames_of(const std::vector<avc::OutFrame>& fs) const {
    py::list l;
    for (const auto& f : fs) {
      const HostSurface& s = frame_of(f);
      l.append(py::make_tuple(f.au.pts, surface_planes(s)));
    }
    return l;
  }
  // Frames still in the reorder buffer (end of stream), oldest first.
  py::list flush() {
    py::list out_list;
    for (const auto& f : avc.flush_output()) {
      py::array_t<uint8_t> o({f.info.height, f.info.width, 3});
      cpu_nv12_to_bgr(frame_of(f), f.info.crop_left, f.info.crop_top, f.info.width, f.info.height,
                      o.mutable_data());
      out_list.append(o);
    }
    return out_list;
  }
  std::vector<PictureInfo> pictures;      // every decoded picture (decoding order)
  // macroblock statistics over every decoded picture (coverage checks)
  u64 kinds[6] = {0, 0, 0, 0, 0, 0};
  u64 t8x8 = 0, weighted = 0, bipred = 0, list1_only = 0;
  std::vector<avc::OutFrame> pending_outputs;  // outputs of the last decode() (output order)
  int last_poc = 0;
  i64 last_pts = 0;
};

PYBIND11_MODULE(_vep, m) {
  m.doc() = "vep native data plane (gfx950 HIP kernels, H.264 subset decoder, RTSP/RTP, muxers)";
  py::register_exception<Error>(m, "NativeError");
  py::register_exception<UnsupportedStream>(m, "UnsupportedStream");

  m.def("device_count", &gpu::device_count);
  // Frame servers and clients allocate a new multi-MB buffer per frame: glibc would mmap each
  // one and the first touch of its pages then costs more than the copy itself. Keep such blocks
  // in the (per-thread) heaps instead, so freed frame buffers are reused without page faults.
  // The arenas are capped (M_ARENA_MAX): with hundreds of handler threads, per-thread arenas each
  // keeping freed frames plus the trim threshold would grow the resident set without bound.
  m.def("tune_malloc_for_frames", [](int mmap_threshold_mb, int arenas) {
    const int thr = std::max(1, mmap_threshold_mb) << 20;
    return mallopt(M_MMAP_THRESHOLD, thr) == 1 && mallopt(M_TRIM_THRESHOLD, 4 * thr) == 1 &&
           mallopt(M_TOP_PAD, thr) == 1 && (arenas <= 0 || mallopt(M_ARENA_MAX, arenas) == 1);
  }, py::arg("mmap_threshold_mb") = 64, py::arg("arenas") = 8);

  py::class_<SynthConfig>(m, "SynthConfig")
      .def(py::init<>())
      .def_readwrite("width", &SynthConfig::width)
      .def_readwrite("height", &SynthConfig::height)
      .def_readwrite("fps", &SynthConfig::fps)
      .def_readwrite("gop", &SynthConfig::gop)
      .def_readwrite("motion", &SynthConfig::motion)
      .def_readwrite("seed", &SynthConfig::seed)
      .def_readwrite("slices", &SynthConfig::slices)
      .def_readwrite("zero_samples", &SynthConfig::zero_samples)
      .def_readwrite("idr_phase", &SynthConfig::idr_phase)
      .def_readwrite("merge_cands", &SynthConfig::merge_cands)
      .def_readwrite("compressed", &SynthConfig::compressed)
      .def_readwrite("qp", &SynthConfig::qp)
      .def_readwrite("refs", &SynthConfig::refs)
      .def_readwrite("objects", &SynthConfig::objects)
      .def_readwrite("deblock_idc", &SynthConfig::deblock_idc)
      .def_readwrite("coverage", &SynthConfig::coverage)
      .def_readwrite("noise", &SynthConfig::noise)
      .def_readwrite("temporal_noise", &SynthConfig::temporal_noise)
      .def_readwrite("profile", &SynthConfig::profile)
      .def_readwrite("bframes", &SynthConfig::bframes)
      .def_readwrite("cabac", &SynthConfig::cabac)
      .def_readwrite("weighted_p", &SynthConfig::weighted_p)
      .def_readwrite("weighted_b", &SynthConfig::weighted_b)
      .def_readwrite("direct_spatial", &SynthConfig::direct_spatial)
      .def_readwrite("tile_cols", &SynthConfig::tile_cols)
      .def_readwrite("tile_rows", &SynthConfig::tile_rows)
      .def_readwrite("wpp", &SynthConfig::wpp)
      .def_readwrite("segments", &SynthConfig::segments)
      .def_readwrite("scaling_lists", &SynthConfig::scaling_lists)
      .def_readwrite("long_term", &SynthConfig::long_term)
      .def_readwrite("open_gop", &SynthConfig::open_gop)
      .def_readwrite("lossless", &SynthConfig::lossless)
      .def_readwrite("bit_depth", &SynthConfig::bit_depth)
      .def_readwrite("chroma_format", &SynthConfig::chroma_format)
      .def_readwrite("interlaced", &SynthConfig::interlaced)
      .def_readwrite("mono", &SynthConfig::mono)
      .def_property(
          "codec", [](const SynthConfig& c) { return c.codec == Codec::kH265 ? "h265" : "h264"; },
          [](SynthConfig& c, const std::string& v) {
            if (v == "h264" || v == "avc") c.codec = Codec::kH264;
            else if (v == "h265" || v == "hevc") c.codec = Codec::kH265;
            else throw Error("codec must be h264 or h265");
          });

  py::class_<AccessUnit, std::shared_ptr<AccessUnit>>(m, "AccessUnit")
      .def(py::init<>())
      .def_property_readonly("codec", [](const AccessUnit& a) { return int(a.codec); })
      .def_readwrite("pts", &AccessUnit::pts)
      .def_readwrite("dts", &AccessUnit::dts)
      .def_readwrite("duration", &AccessUnit::duration)
      .def_readwrite("keyframe", &AccessUnit::keyframe)
      .def_readwrite("corrupt", &AccessUnit::corrupt)
      .def_readwrite("arrival_ms", &AccessUnit::arrival_ms)
      .def_readwrite("seq", &AccessUnit::seq)
      .def_property_readonly("size", &AccessUnit::bytes)
      .def("pin", &AccessUnit::pin)
      .def_property_readonly("pinned", &AccessUnit::pinned)
      .def("nals",
           [](const AccessUnit& a) {
             py::list l;
             for (size_t i = 0; i < a.nals.size(); ++i) l.append(to_bytes(a.nal(i), a.nal_size(i)));
             return l;
           })
      .def("annexb",
           [](const AccessUnit& a) {
             std::string s;
             for (size_t i = 0; i < a.nals.size(); ++i) {
               s.append("\x00\x00\x00\x01", 4);
               s.append(reinterpret_cast<const char*>(a.nal(i)), a.nal_size(i));
             }
             return py::bytes(s);
           })
      .def_static(
          "from_nals",
          [](const std::vector<std::string>& nals, i64 pts, i64 dts, bool key, int codec) {
            auto a = std::make_shared<AccessUnit>();
            a->codec = Codec(codec);
            for (auto& n : nals) a->add_nal(reinterpret_cast<const u8*>(n.data()), n.size());
            a->pts = pts;
            a->dts = dts;
            a->keyframe = key;
            a->arrival_ms = now_ms();
            return a;
          },
          py::arg("nals"), py::arg("pts") = 0, py::arg("dts") = 0, py::arg("keyframe") = false,
          py::arg("codec") = 0);

  py::class_<SynthH264>(m, "SynthH264")
      .def(py::init<const SynthConfig&>())
      .def("next", [](SynthH264& s) { return std::shared_ptr<AccessUnit>(s.next()); },
           py::call_guard<py::gil_scoped_release>())
      .def("picture", [](const SynthH264& s) { return surface_planes(s.picture()); })
      .def_property_readonly("sps_nal", [](const SynthH264& s) { return to_bytes(s.sps_nal().data(), s.sps_nal().size()); })
      .def_property_readonly("pps_nal", [](const SynthH264& s) { return to_bytes(s.pps_nal().data(), s.pps_nal().size()); })
      .def_property_readonly("vps_nal", [](const SynthH264& s) { return to_bytes(s.vps_nal().data(), s.vps_nal().size()); })
      .def_property_readonly("frame_index", &SynthH264::frame_index)
      .def_property_readonly("last_pts", &SynthH264::last_pts);
  m.attr("SynthEncoder") = m.attr("SynthH264");

  auto surface_tuple = [](const HostSurface& p) { return surface_planes(p); };

  py::class_<avc::AvcHighConfig>(m, "AvcHighConfig")
      .def(py::init<>())
      .def_readwrite("width", &avc::AvcHighConfig::width)
      .def_readwrite("height", &avc::AvcHighConfig::height)
      .def_readwrite("fps", &avc::AvcHighConfig::fps)
      .def_readwrite("gop", &avc::AvcHighConfig::gop)
      .def_readwrite("idr_phase", &avc::AvcHighConfig::idr_phase)
      .def_readwrite("bframes", &avc::AvcHighConfig::bframes)
      .def_readwrite("pyramid", &avc::AvcHighConfig::pyramid)
      .def_readwrite("refs", &avc::AvcHighConfig::refs)
      .def_readwrite("qp", &avc::AvcHighConfig::qp)
      .def_readwrite("bit_depth", &avc::AvcHighConfig::bit_depth)
      .def_readwrite("chroma_format", &avc::AvcHighConfig::chroma_format)
      .def_readwrite("cabac", &avc::AvcHighConfig::cabac)
      .def_readwrite("t8x8", &avc::AvcHighConfig::t8x8)
      .def_readwrite("weighted_p", &avc::AvcHighConfig::weighted_p)
      .def_readwrite("weighted_b", &avc::AvcHighConfig::weighted_b)
      .def_readwrite("direct_spatial", &avc::AvcHighConfig::direct_spatial)
      .def_readwrite("scaling", &avc::AvcHighConfig::scaling)
      .def_readwrite("slices", &avc::AvcHighConfig::slices)
      .def_readwrite("deblock_idc", &avc::AvcHighConfig::deblock_idc)
      .def_readwrite("chroma_qp_offset", &avc::AvcHighConfig::chroma_qp_offset)
      .def_readwrite("second_chroma_qp_offset", &avc::AvcHighConfig::second_chroma_qp_offset)
      .def_readwrite("coverage", &avc::AvcHighConfig::coverage)
      .def_readwrite("interlaced", &avc::AvcHighConfig::interlaced)
      .def_readwrite("mono", &avc::AvcHighConfig::mono)
      .def_readwrite("fields", &avc::AvcHighConfig::fields)
      .def_readwrite("marking", &avc::AvcHighConfig::marking)
      .def_readwrite("objects", &avc::AvcHighConfig::objects)
      .def_readwrite("noise", &avc::AvcHighConfig::noise)
      .def_readwrite("temporal_noise", &avc::AvcHighConfig::temporal_noise)
      .def_readwrite("seed", &avc::AvcHighConfig::seed);
  py::class_<avc::AvcHighEncoder>(m, "AvcHighEncoder")
      .def(py::init<const avc::AvcHighConfig&>())
      .def("next", &avc::AvcHighEncoder::next, py::call_guard<py::gil_scoped_release>())
      .def("picture", [surface_tuple](const avc::AvcHighEncoder& e) { return surface_tuple(e.reconstruction()); })
      .def("source", [surface_tuple](const avc::AvcHighEncoder& e) { return surface_tuple(e.source()); })
      .def_property_readonly("last_pts", &avc::AvcHighEncoder::last_pts)
      .def_property_readonly("last_type", [](const avc::AvcHighEncoder& e) { return std::string(1, e.last_type()); })
      .def_property_readonly("last_display_index", &avc::AvcHighEncoder::last_display_index)
      .def_property_readonly("sps_nal", [](const avc::AvcHighEncoder& e) { return to_bytes(e.sps_nal().data(), e.sps_nal().size()); })
      .def_property_readonly("pps_nal", [](const avc::AvcHighEncoder& e) { return to_bytes(e.pps_nal().data(), e.pps_nal().size()); });

  py::class_<hevc::HevcEncConfig>(m, "HevcEncConfig")
      .def(py::init<>())
      .def_readwrite("width", &hevc::HevcEncConfig::width)
      .def_readwrite("height", &hevc::HevcEncConfig::height)
      .def_readwrite("fps", &hevc::HevcEncConfig::fps)
      .def_readwrite("gop", &hevc::HevcEncConfig::gop)
      .def_readwrite("idr_phase", &hevc::HevcEncConfig::idr_phase)
      .def_readwrite("bframes", &hevc::HevcEncConfig::bframes)
      .def_readwrite("qp", &hevc::HevcEncConfig::qp)
      .def_readwrite("log2_ctb", &hevc::HevcEncConfig::log2_ctb)
      .def_readwrite("log2_min_cb", &hevc::HevcEncConfig::log2_min_cb)
      .def_readwrite("amp", &hevc::HevcEncConfig::amp)
      .def_readwrite("sao", &hevc::HevcEncConfig::sao)
      .def_readwrite("deblock", &hevc::HevcEncConfig::deblock)
      .def_readwrite("tskip", &hevc::HevcEncConfig::tskip)
      .def_readwrite("sign_hiding", &hevc::HevcEncConfig::sign_hiding)
      .def_readwrite("cu_qp_delta", &hevc::HevcEncConfig::cu_qp_delta)
      .def_readwrite("pcm", &hevc::HevcEncConfig::pcm)
      .def_readwrite("tmvp", &hevc::HevcEncConfig::tmvp)
      .def_readwrite("slices", &hevc::HevcEncConfig::slices)
      .def_readwrite("tile_cols", &hevc::HevcEncConfig::tile_cols)
      .def_readwrite("tile_rows", &hevc::HevcEncConfig::tile_rows)
      .def_readwrite("wpp", &hevc::HevcEncConfig::wpp)
      .def_readwrite("segments", &hevc::HevcEncConfig::segments)
      .def_readwrite("scaling_lists", &hevc::HevcEncConfig::scaling_lists)
      .def_readwrite("weighted", &hevc::HevcEncConfig::weighted)
      .def_readwrite("long_term", &hevc::HevcEncConfig::long_term)
      .def_readwrite("open_gop", &hevc::HevcEncConfig::open_gop)
      .def_readwrite("lossless", &hevc::HevcEncConfig::lossless)
      .def_readwrite("bit_depth", &hevc::HevcEncConfig::bit_depth)
      .def_readwrite("coverage", &hevc::HevcEncConfig::coverage)
      .def_readwrite("objects", &hevc::HevcEncConfig::objects)
      .def_readwrite("noise", &hevc::HevcEncConfig::noise)
      .def_readwrite("temporal_noise", &hevc::HevcEncConfig::temporal_noise)
      .def_readwrite("seed", &hevc::HevcEncConfig::seed);
  py::class_<hevc::HevcEncoder>(m, "HevcEncoder")
      .def(py::init<const hevc::HevcEncConfig&>())
      .def("next", &hevc::HevcEncoder::next, py::call_guard<py::gil_scoped_release>())
      .def("picture", [surface_tuple](const hevc::HevcEncoder& e) { return surface_tuple(e.reconstruction()); })
      .def("source", [surface_tuple](const hevc::HevcEncoder& e) { return surface_tuple(e.source()); })
      .def_property_readonly("last_pts", &hevc::HevcEncoder::last_pts)
      .def_property_readonly("last_type", [](const hevc::HevcEncoder& e) { return std::string(1, e.last_type()); })
      .def_property_readonly("vps_nal", [](const hevc::HevcEncoder& e) { return to_bytes(e.vps_nal().data(), e.vps_nal().size()); })
      .def_property_readonly("sps_nal", [](const hevc::HevcEncoder& e) { return to_bytes(e.sps_nal().data(), e.sps_nal().size()); })
      .def_property_readonly("pps_nal", [](const hevc::HevcEncoder& e) { return to_bytes(e.pps_nal().data(), e.pps_nal().size()); });
  // General H.265 Main decoder (CPU): decode() / flush() return the frames leaving the output
  // queue as [(pts, poc, type, (Y, UV) coded NV12 planes)] in output order.
  py::class_<hevc::Decoder>(m, "HevcDecoder")
      .def(py::init<>())
      .def("decode",
           [surface_tuple](hevc::Decoder& d, const AccessUnit& au) {
             std::vector<hevc::FramePtr> fs;
             {
               py::gil_scoped_release nogil;
               fs = d.decode(au, 0);
             }
             py::list l;
             for (const auto& f : fs) l.append(py::make_tuple(f->pts, f->poc, std::string(1, f->type), surface_tuple(f->s)));
             return l;
           })
      .def("flush",
           [surface_tuple](hevc::Decoder& d) {
             py::list l;
             for (const auto& f : d.flush()) l.append(py::make_tuple(f->pts, f->poc, std::string(1, f->type), surface_tuple(f->s)));
             return l;
           })
      .def_property_readonly("stats", [](const hevc::Decoder& d) {
        py::dict s;
        s["intra"] = d.stats.intra;
        s["inter"] = d.stats.inter;
        s["skip"] = d.stats.skip;
        s["pcm"] = d.stats.pcm;
        s["merge"] = d.stats.merge;
        s["bi"] = d.stats.bi;
        s["tskip"] = d.stats.tskip;
        s["amp"] = d.stats.amp;
        return s;
      });

  // General H.265 decoder in records mode + the CPU mirror of the GPU reconstruction (tests):
  // same outputs as HevcDecoder, reconstructed from the GPU work lists.
  struct HevcRecords {
    hevc::Decoder d;
    std::vector<HostSurface> slots;
    u64 pictures = 0, pus = 0, tus = 0, intra_tus = 0, max_level = 0, exchange_violations = 0;
    bool execute = true;  // false: parse only (records are counted, not executed: parse timing)
    explicit HevcRecords(bool ex = true) : execute(ex) { d.set_gpu_mode(true); }
    py::list frames(const std::vector<hevc::FramePtr>& fs) {
      py::list l;
      for (const auto& f : fs) {
        const HostSurface& s = slots[size_t(f->slot)];
        const int W = f->width + f->crop_left, H = f->height + f->crop_top;
        (void)W;
        (void)H;
        const int cw = s.coded_w, ch = s.coded_h;
        (void)ch;
        // the coded picture (the decoder's surfaces are coded_w x coded_h, slots are 16-aligned)
        const int pw = coded_w_, ph = coded_h_;
        py::tuple planes;
        if (s.wide()) {  // Main10: uint16 planes
          py::array_t<uint16_t> y({ph, pw});
          py::array_t<uint16_t> uv({ph / 2, pw});
          for (int r = 0; r < ph; ++r) std::memcpy(y.mutable_data() + size_t(r) * pw, &s.y16[size_t(r) * cw], size_t(pw) * 2);
          for (int r = 0; r < ph / 2; ++r)
            std::memcpy(uv.mutable_data() + size_t(r) * pw, &s.uv16[size_t(r) * cw], size_t(pw) * 2);
          planes = py::make_tuple(y, uv);
        } else {
          py::array_t<uint8_t> y({ph, pw});
          py::array_t<uint8_t> uv({ph / 2, pw});
          for (int r = 0; r < ph; ++r) std::memcpy(y.mutable_data() + size_t(r) * pw, &s.y[size_t(r) * cw], size_t(pw));
          for (int r = 0; r < ph / 2; ++r)
            std::memcpy(uv.mutable_data() + size_t(r) * pw, &s.uv[size_t(r) * cw], size_t(pw));
          planes = py::make_tuple(y, uv);
        }
        l.append(py::make_tuple(f->pts, f->poc, std::string(1, f->type), planes, f->slot));
      }
      return l;
    }
    void run(std::vector<std::shared_ptr<hevc::GpuPicture>> ps) {
      for (auto& p : ps) {
        coded_w_ = p->width;
        coded_h_ = p->height;
        const int sw = (p->width + 15) & ~15, sh = (p->height + 15) & ~15;
        if (slots.size() < size_t(d.gpu_slots())) slots.resize(size_t(d.gpu_slots()));
        const int bd = std::max(p->bd_y, p->bd_c);
        for (auto& h : slots)
          if (h.coded_w != sw || h.coded_h != sh || h.bd != bd) h.alloc(sw, sh, bd);
        if (execute) hevc::cpu_execute(*p, slots);
        ++pictures;
        pus += p->pus.size();
        tus += p->tus.size();
        for (const auto& t : p->tus) intra_tus += (t.flags & hevc::kTuIntra) ? 1 : 0;
        exchange_violations += hevc::exchange_violations(*p);
        auto h = [](const void* d, size_t n) {  // FNV-1a of a record array (tests: records equality)
          u64 x = 1469598103934665603ull;
          for (size_t i = 0; i < n; ++i) x = (x ^ static_cast<const u8*>(d)[i]) * 1099511628211ull;
          return x;
        };
        last_qp.assign(p->qp.begin(), p->qp.end());
        last_digest = {h(p->pus.data(), p->pus.size() * sizeof(hevc::GpuPu)),
                       h(p->tus.data(), p->tus.size() * sizeof(hevc::GpuTu)),
                       h(p->coefs.data(), p->coefs.size() * 2), h(p->pcm.data(), p->pcm.size()),
                       h(p->bs_v.data(), p->bs_v.size()), h(p->bs_h.data(), p->bs_h.size()),
                       h(p->qp.data(), p->qp.size()), h(p->wp.data(), p->wp.size() * sizeof(hevc::GpuWp)),
                       h(p->sao_params.data(), p->sao_params.size() * sizeof(hevc::GpuSao))};
        max_level = std::max<u64>(max_level, p->level_begin.empty() ? 0 : p->level_begin.size() - 1);
      }
    }
    int coded_w_ = 0, coded_h_ = 0;
    std::vector<u64> last_digest;  // pus, tus, coefs, pcm, bs_v, bs_h, qp, wp, sao of the last picture
    std::vector<signed char> last_qp;       // QpY per 4x4 block of the last picture
  };
  py::class_<HevcRecords>(m, "HevcRecordsDecoder")
      .def(py::init<bool>(), py::arg("execute") = true)
      .def_property_readonly("parallel_units", [](const HevcRecords& r) { return r.d.parallel_units(); })
      .def_property_readonly("last_digest", [](const HevcRecords& r) { return r.last_digest; })
      .def_property_readonly("last_qp", [](const HevcRecords& r) { return std::vector<int>(r.last_qp.begin(), r.last_qp.end()); })
      .def("decode",
           [](HevcRecords& r, const AccessUnit& au) {
             std::vector<hevc::FramePtr> fs;
             {
               py::gil_scoped_release nogil;
               fs = r.d.decode(au, 0);
               r.run(r.d.take_gpu_pictures());
             }
             return r.frames(fs);
           })
      .def("flush",
           [](HevcRecords& r) {
             auto fs = r.d.flush();
             r.run(r.d.take_gpu_pictures());
             return r.frames(fs);
           })
      .def_property_readonly("stats", [](const HevcRecords& r) {
        py::dict s;
        s["pictures"] = r.pictures;
        s["pus"] = r.pus;
        s["tus"] = r.tus;
        s["intra_tus"] = r.intra_tus;
        s["max_levels"] = r.max_level;
        s["exchange_violations"] = r.exchange_violations;
        s["slots"] = r.d.gpu_slots();
        return s;
      });

  py::class_<CpuDecoder>(m, "CpuDecoder")
      .def(py::init<>())
      .def("decode", &CpuDecoder::decode)
      .def("flush", &CpuDecoder::flush)
      .def("frames", [](CpuDecoder& d) { return d.general ? d.frames_of(d.pending_outputs) : py::list(); })
      .def("flush_frames", [](CpuDecoder& d) { return d.frames_of(d.avc.flush_output()); })
      .def_property_readonly("last_poc", [](const CpuDecoder& d) { return d.last_poc; })
      .def_property_readonly("last_pts", [](const CpuDecoder& d) { return d.last_pts; })
      .def_property_readonly("mb_stats", [](const CpuDecoder& d) {
        py::dict r;
        const char* names[6] = {"skip", "inter", "i4x4", "i16x16", "pcm", "i8x8"};
        for (int k = 0; k < 6; ++k) r[names[k]] = d.kinds[k];
        r["t8x8"] = d.t8x8;
        r["weighted"] = d.weighted;
        r["bipred"] = d.bipred;
        r["list1_only"] = d.list1_only;
        std::string types;
        for (const auto& p : d.pictures) types += p.pict_type;
        r["types"] = types;
        return r;
      })
      .def_property_readonly("outputs_last", [](const CpuDecoder& d) { return int(d.pending_outputs.size()); })
      .def_property_readonly("info", [](const CpuDecoder& d) { return pic_dict(d.last); })
      .def_property_readonly("coded_mbs", [](const CpuDecoder& d) { return d.coded; })
      .def_property_readonly("pictures_decoded", [](const CpuDecoder& d) { return d.pictures.size(); })
      .def_property_readonly("marking_stats", [](const CpuDecoder& d) {
        py::dict s;
        for (int k = 1; k <= 6; ++k) s[py::str("mmco" + std::to_string(k))] = d.avc.mmco_ops[k];
        s["list_mods"] = d.avc.list_mods;
        s["long_term_marked"] = d.avc.long_term_marked;
        s["redundant_slices_skipped"] = d.avc.redundant_slices_skipped;
        return s;
      })
      .def_property_readonly("general", [](const CpuDecoder& d) { return d.general; })
      .def_property_readonly("parallel_slices", [](const CpuDecoder& d) { return d.avc.parallel_slices_run(); })
      .def("surface", [](const CpuDecoder& d) {
        const HostSurface& s = d.out();
        py::array_t<uint8_t> y({s.coded_h, s.coded_w});
        py::array_t<uint8_t> uv({s.coded_h / 2, s.coded_w});
        std::memcpy(y.mutable_data(), s.y.data(), s.y.size());
        std::memcpy(uv.mutable_data(), s.uv.data(), s.uv.size());
        return py::make_tuple(y, uv);
      });

  // Reconstruction primitives of avc_recon.h (shared by the CPU decoder, the gfx950 kernels and
  // the encoders), exposed one by one for tests/test_spec_oracle.py, which checks them against
  // independent implementations written from the H.264 text.
  auto rc = m.def_submodule("recon", "H.264 reconstruction primitives (avc_recon.h)");
  rc.def("idct4", [](std::vector<int> d) {
    VEP_CHECK(d.size() == 16, "16 coefficients");
    i16 c[16];
    for (int k = 0; k < 16; ++k) c[k] = i16(d[size_t(k)]);
    std::vector<int> r(16);
    avc::idct4x4(c, r.data());
    return r;
  });
  rc.def("idct8", [](std::vector<int> d) {
    VEP_CHECK(d.size() == 64, "64 coefficients");
    i16 c[64];
    for (int k = 0; k < 64; ++k) c[k] = i16(d[size_t(k)]);
    std::vector<int> r(64);
    avc::idct8x8(c, r.data());
    return r;
  });
  rc.def("dequant4", [](int c, int qp, int i, int j) { return avc::dequant4x4(c, qp, i, j); });
  // top = p[-1..7, -1] (9, top-right already substituted), left = p[-1, 0..3]
  rc.def("intra4x4", [](std::vector<int> top, std::vector<int> left, bool has_top, bool has_left, int mode, int bd) {
    VEP_CHECK(top.size() == 9 && left.size() == 4, "9 top + 4 left samples");
    avc::Intra4Nb n{};
    for (int k = 0; k < 9; ++k) n.t[k] = top[size_t(k)];
    for (int k = 0; k < 4; ++k) n.l[k] = left[size_t(k)];
    n.has_top = has_top;
    n.has_left = has_left;
    std::vector<int> r(16);
    for (int y = 0; y < 4; ++y)
      for (int x = 0; x < 4; ++x) r[size_t(y * 4 + x)] = avc::intra4x4_pred(n, mode, x, y, bd);
    return r;
  }, py::arg("top"), py::arg("left"), py::arg("has_top"), py::arg("has_left"), py::arg("mode"), py::arg("bd") = 8);
  // top = p[-1..15, -1] (17, top-right substituted), left = p[-1, 0..7]: reference filtering +
  // prediction
  rc.def("intra8x8", [](std::vector<int> top, std::vector<int> left, bool has_top, bool has_left, bool has_tl,
                        int mode, int bd) {
    VEP_CHECK(top.size() == 17 && left.size() == 8, "17 top + 8 left samples");
    int f[25];
    avc::intra8x8_filter([&](int x) { return top[size_t(x + 1)]; }, [&](int y) { return left[size_t(y)]; },
                         has_top, has_left, has_tl, f);
    std::vector<int> r(64);
    for (int y = 0; y < 8; ++y)
      for (int x = 0; x < 8; ++x) r[size_t(y * 8 + x)] = avc::intra8x8_pred(f, has_top, has_left, mode, x, y, bd);
    return r;
  }, py::arg("top"), py::arg("left"), py::arg("has_top"), py::arg("has_left"), py::arg("has_tl"), py::arg("mode"),
     py::arg("bd") = 8);
  rc.def("intra16x16", [](std::vector<int> top, std::vector<int> left, bool has_top, bool has_left, int mode, int bd) {
    VEP_CHECK(top.size() == 17 && left.size() == 16, "17 top + 16 left samples");
    avc::Intra16Nb n{};
    for (int k = 0; k < 17; ++k) n.top[k] = top[size_t(k)];
    for (int k = 0; k < 16; ++k) n.left[k] = left[size_t(k)];
    n.has_top = has_top;
    n.has_left = has_left;
    n.has_tl = has_top && has_left;
    const avc::PredConst k = avc::intra16x16_const(n, mode, bd);
    std::vector<int> r(256);
    for (int y = 0; y < 16; ++y)
      for (int x = 0; x < 16; ++x) r[size_t(y * 16 + x)] = avc::intra16x16_pred(n, k, mode, x, y, bd);
    return r;
  }, py::arg("top"), py::arg("left"), py::arg("has_top"), py::arg("has_left"), py::arg("mode"), py::arg("bd") = 8);
  // (cf 2: 4:2:2, 16 left samples, 8x16 prediction)
  rc.def("intra_chroma", [](std::vector<int> top, std::vector<int> left, bool has_top, bool has_left, int mode, int bd,
                            int cf) {
    const int ch = cf == 2 ? 16 : 8;
    VEP_CHECK(top.size() == 9 && left.size() == size_t(ch), "9 top + 8 (4:2:2: 16) left samples");
    avc::IntraChromaNb n{};
    for (int k = 0; k < 9; ++k) n.top[k] = top[size_t(k)];
    for (int k = 0; k < ch; ++k) n.left[k] = left[size_t(k)];
    n.has_top = has_top;
    n.has_left = has_left;
    n.has_tl = has_top && has_left;
    const avc::PredConst k = mode == 3 ? avc::chroma_plane_const(n, cf) : avc::PredConst{0, 0, 0, 0};
    std::vector<int> r(size_t(8 * ch));
    for (int y = 0; y < ch; ++y)
      for (int x = 0; x < 8; ++x) r[size_t(y * 8 + x)] = avc::chroma_pred(n, k, mode, x, y, bd, cf);
    return r;
  }, py::arg("top"), py::arg("left"), py::arg("has_top"), py::arg("has_left"), py::arg("mode"), py::arg("bd") = 8,
     py::arg("cf") = 1);
  // 4:2:2 chroma DC: 8 levels (parsing order) -> dcC per chroma block (raster, 2 wide)
  rc.def("chroma422_dc", [](std::vector<int> lv, int qpdc, int ls) {
    VEP_CHECK(lv.size() == 8, "8 levels");
    std::vector<int> r(8);
    avc::chroma422_dc(lv.data(), qpdc, ls, r.data());
    return r;
  });
  rc.def("luma_qpel", [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> plane, int xi, int yi,
                         int fx, int fy) {
    VEP_CHECK(plane.ndim() == 2, "2-D plane");
    const int h = int(plane.shape(0)), w = int(plane.shape(1));
    return avc::luma_qpel(plane.data(), w, w, h, xi, yi, fx, fy);
  });
  rc.def("chroma_epel", [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> uv, int c, int xi,
                           int yi, int fx, int fy) {
    VEP_CHECK(uv.ndim() == 2 && uv.shape(1) % 2 == 0, "interleaved UV plane");
    const int h = int(uv.shape(0)), pitch = int(uv.shape(1));
    return avc::chroma_epel(uv.data(), pitch, pitch / 2, h, c, xi, yi, fx, fy);
  });
  // High 10 planes: u16 samples at bit depth bd
  rc.def("luma_qpel16", [](py::array_t<uint16_t, py::array::c_style | py::array::forcecast> plane, int xi, int yi,
                           int fx, int fy, int bd) {
    VEP_CHECK(plane.ndim() == 2, "2-D plane");
    const int h = int(plane.shape(0)), w = int(plane.shape(1));
    return avc::luma_qpel(plane.data(), w, w, h, xi, yi, fx, fy, bd);
  });
  rc.def("chroma_epel16", [](py::array_t<uint16_t, py::array::c_style | py::array::forcecast> uv, int c, int xi,
                             int yi, int fx, int fy) {
    VEP_CHECK(uv.ndim() == 2 && uv.shape(1) % 2 == 0, "interleaved UV plane");
    const int h = int(uv.shape(0)), pitch = int(uv.shape(1));
    return avc::chroma_epel(uv.data(), pitch, pitch / 2, h, c, xi, yi, fx, fy);
  });
  rc.def("edge_params", [](int qp_p, int qp_q, int off_a, int off_b, int bd) {
    const avc::EdgeParams e = avc::edge_params(qp_p, qp_q, off_a, off_b, bd);
    return py::make_tuple(e.alpha, e.beta, std::vector<int>{e.tc0[0], e.tc0[1], e.tc0[2]});
  }, py::arg("qp_p"), py::arg("qp_q"), py::arg("off_a"), py::arg("off_b"), py::arg("bd") = 8);
  // QPC of Table 8-15 from QPY (QpBdOffsetC: High 10 QPs below 0)
  rc.def("chroma_qp_bd", [](int qpy, int offset, int qpbd_c) { return avc::chroma_qp_bd(qpy, offset, qpbd_c); });
  // one sample line across an edge: p = p0..p3, q = q0..q3 -> filtered (p, q)
  // (unified: filter_samples_u, the one-stream luma / chroma form of the GPU High 10 / 4:2:2 filter)
  rc.def("filter_line", [](std::vector<int> p, std::vector<int> q, int bs, int alpha, int beta, int tc0,
                           bool chroma, int bd, bool unified) {
    VEP_CHECK(p.size() == 4 && q.size() == 4, "4 + 4 samples");
    if (unified) avc::filter_samples_u(p.data(), q.data(), bs, alpha, beta, tc0, chroma, bd);
    else avc::filter_samples(p.data(), q.data(), bs, alpha, beta, tc0, chroma, bd);
    return py::make_tuple(p, q);
  }, py::arg("p"), py::arg("q"), py::arg("bs"), py::arg("alpha"), py::arg("beta"), py::arg("tc0"),
     py::arg("chroma"), py::arg("bd") = 8, py::arg("unified") = false);

  m.def("cavlc_roundtrip", [](int nc, int max_coeff, const std::vector<int>& c) {
    // write_residual_block -> read_residual_block (table self-consistency, tests only)
    VEP_CHECK(int(c.size()) == max_coeff, "coefficient count mismatch");
    BitWriter bw;
    avc::write_residual_block(bw, nc, max_coeff, c.data());
    bw.u1(1);
    bw.align_zero();
    avc::Bits br(bw.buf().data(), bw.buf().size());
    std::vector<int> out(16, 0);
    const int total = avc::read_residual_block(br, nc, max_coeff, out.data());
    out.resize(size_t(max_coeff));
    return py::make_tuple(out, total);
  });
  m.def("avc_source_luma", [](const SynthH264& s) {
    const HostSurface& p = s.source();
    py::array_t<uint8_t> y({p.coded_h, p.coded_w});
    std::memcpy(y.mutable_data(), p.y.data(), p.y.size());
    return y;
  });
  m.def("parse_sps", [](const std::string& nal) {
    std::vector<u8> r(nal.size());
    size_t n = ebsp_to_rbsp(reinterpret_cast<const u8*>(nal.data()), nal.size(), r.data());
    h264::Sps s = h264::parse_sps(r.data(), n);
    py::dict d;
    d["profile_idc"] = s.profile_idc;
    d["level_idc"] = s.level_idc;
    d["width"] = s.width();
    d["height"] = s.height();
    d["coded_width"] = s.coded_width();
    d["coded_height"] = s.coded_height();
    d["fps"] = s.fps();
    d["poc_type"] = s.poc_type;
    d["max_num_ref_frames"] = s.max_num_ref_frames;
    d["chroma_format_idc"] = s.chroma_format_idc;
    d["bit_depth_luma"] = s.bit_depth_luma;
    d["bit_depth_chroma"] = s.bit_depth_chroma;
    return d;
  });
  m.def("parse_hevc_sps", [](const std::string& nal) {
    std::vector<u8> r(nal.size());
    size_t n = ebsp_to_rbsp(reinterpret_cast<const u8*>(nal.data()), nal.size(), r.data());
    hevc::Sps s = hevc::parse_sps(r.data(), n);
    py::dict d;
    d["profile_idc"] = s.ptl.profile_idc;
    d["level_idc"] = s.ptl.level_idc;
    d["width"] = s.out_width();
    d["height"] = s.out_height();
    d["coded_width"] = s.width;
    d["coded_height"] = s.height;
    d["fps"] = s.fps();
    d["ctb_size"] = s.ctb_size();
    d["pcm"] = s.pcm;
    d["num_short_term_rps"] = int(s.st_rps.size());
    d["scaling_list"] = s.scaling_list;
    d["scaling_list_data"] = s.scaling_list_data;
    d["long_term_refs"] = s.long_term_refs;
    d["num_long_term_ref_pics_sps"] = s.num_long_term_ref_pics_sps;
    return d;
  });
  auto hevc_rbsp = [](const std::string& nal) {
    std::vector<u8> r(nal.size());
    r.resize(ebsp_to_rbsp(reinterpret_cast<const u8*>(nal.data()), nal.size(), r.data()));
    return r;
  };
  m.def("parse_hevc_pps", [hevc_rbsp](const std::string& nal) {
    const std::vector<u8> r = hevc_rbsp(nal);
    hevc::Pps p = hevc::parse_pps(r.data(), r.size());
    py::dict d;
    d["tiles"] = p.tiles;
    d["tile_cols"] = p.tile_cols;
    d["tile_rows"] = p.tile_rows;
    d["uniform_spacing"] = p.uniform_spacing;
    d["loop_filter_across_tiles"] = p.loop_filter_across_tiles;
    d["entropy_coding_sync"] = p.entropy_coding_sync;
    d["dependent_slice_segments"] = p.dependent_slice_segments;
    d["weighted_pred"] = p.weighted_pred;
    d["weighted_bipred"] = p.weighted_bipred;
    d["transquant_bypass"] = p.transquant_bypass;
    d["scaling_list"] = p.scaling_list;
    return d;
  });
  // ScalingFactor matrix (raster n x n, n = 4 << size_id) of the default lists, or of the lists an
  // SPS / PPS carries (the PPS ones win, as in decoding).
  m.def("hevc_scaling_factors", [hevc_rbsp](int size_id, int matrix_id, py::object sps_nal, py::object pps_nal) {
    VEP_CHECK(size_id >= 0 && size_id < 4 && matrix_id >= 0 && matrix_id < 6, "bad sizeId / matrixId");
    hevc::ScalingList sl;
    if (!sps_nal.is_none()) {
      const std::vector<u8> r = hevc_rbsp(sps_nal.cast<std::string>());
      sl = hevc::parse_sps(r.data(), r.size()).sl;
    }
    if (!pps_nal.is_none()) {
      const std::vector<u8> r = hevc_rbsp(pps_nal.cast<std::string>());
      hevc::Pps p = hevc::parse_pps(r.data(), r.size());
      if (p.scaling_list) sl = p.sl;
    }
    const int n = 4 << size_id;
    std::vector<u8> f(size_t(n) * n);
    sl.factors(size_id, matrix_id, f.data());
    return std::vector<int>(f.begin(), f.end());
  }, py::arg("size_id"), py::arg("matrix_id"), py::arg("sps_nal") = py::none(), py::arg("pps_nal") = py::none());
  // Slice segment header fields of an escaped slice NAL: entry point offsets and the byte offset
  // of slice_segment_data() within the escaped NAL.
  m.def("hevc_slice_entry_points", [hevc_rbsp](const std::string& nal, const std::string& sps_nal,
                                               const std::string& pps_nal) {
    const std::vector<u8> rs = hevc_rbsp(sps_nal), rp = hevc_rbsp(pps_nal), r = hevc_rbsp(nal);
    const hevc::Sps sps = hevc::parse_sps(rs.data(), rs.size());
    const hevc::Pps pps = hevc::parse_pps(rp.data(), rp.size());
    const hevc::SliceHeader prev;  // (a dependent segment's slice fields are not needed here)
    const hevc::SliceHeader sh = hevc::parse_slice_header(r.data(), r.size(), sps, pps, &prev);
    // RBSP offset -> escaped offset: count the emulation prevention bytes before it
    size_t ebsp = 0, rbsp = 0;
    int zeros = 0;
    const u8* p = reinterpret_cast<const u8*>(nal.data());
    while (rbsp < sh.data_bytepos && ebsp < nal.size()) {
      const u8 b = p[ebsp++];
      if (zeros >= 2 && b == 3) {
        zeros = 0;
        continue;
      }
      ++rbsp;
      zeros = b == 0 ? zeros + 1 : 0;
    }
    py::dict d;
    d["entry_points"] = std::vector<u32>(sh.entry_points.begin(), sh.entry_points.end());
    d["data_offset_ebsp"] = ebsp;
    d["dependent"] = sh.dependent;
    d["segment_address"] = sh.segment_address;
    return d;
  });
  // Record-size statistics of H.264 access units parsed in records mode (the bytes the GPU pulls
  // over PCIe per picture): macroblocks, coefficient-pool entries (sparse groups: mask words +
  // values), non-zero coefficients, motion-vector entries.
  // Sparse coefficient records against the dense blocks they encode: random blocks (any density,
  // int16 extremes, 4x4 and 8x8 transforms, any coded pattern) through store_mb -> expand_coefs
  // (H.264, avc_recon.h) and through hk_sparse_store -> hk_sparse_expand for every H.265 TB size
  // (hevc_kern.h). Returns (H.264 mismatches, H.265 mismatches).
  m.def("sparse_coef_fuzz", [](u64 seed, int trials) {
    u64 x = seed * 0x9E3779B97F4A7C15ull + 1;
    auto rnd = [&]() {
      x ^= x << 13;
      x ^= x >> 7;
      x ^= x << 17;
      return x;
    };
    auto val = [&](int density) -> i16 {  // non-zero with probability density / 16
      if (int(rnd() & 15) >= density) return 0;
      const int r = int(rnd() % 8);
      if (r == 0) return i16(-32768);
      if (r == 1) return i16(32767);
      const int v = int(rnd() % 64) - 32;
      return i16(v ? v : 1);
    };
    int bad_avc = 0, bad_hevc = 0;
    for (int t = 0; t < trials; ++t) {
      const int dens = int(rnd() % 17);
      avc::MbResidual res;
      res.t8 = rnd() & 1;
      i16 want[avc::kDenseCoefs] = {};
      if (res.t8) {
        for (int q = 0; q < 4; ++q) {
          const bool coded = rnd() & 1;
          for (int i = 0; i < 64; ++i) want[64 * q + i] = res.b8[q][i] = coded ? val(dens) : 0;
          if (coded) res.luma |= u16(0x33u << ((q & 1) * 2 + (q >> 1) * 8));
        }
      } else {
        for (int b = 0; b < 16; ++b) {
          const bool coded = rnd() & 1;
          for (int i = 0; i < 16; ++i) want[16 * b + i] = res.blk[b][i] = coded ? val(dens) : 0;
          if (coded) res.luma |= u16(1u << b);
        }
      }
      for (int k = 0; k < 8; ++k) {
        const bool coded = rnd() & 1;
        for (int i = 0; i < 16; ++i) want[256 + 16 * k + i] = res.blk[16 + k][i] = coded ? val(dens) : 0;
        if (coded) res.chroma |= u8(1u << k);
      }
      avc::Picture pic;
      pic.wmbs = pic.hmbs = 1;
      pic.mbs.resize(1);
      avc::MbRec rec{};
      rec.kind = res.t8 ? avc::kI8x8 : avc::kI16x16;
      rec.flags = res.t8 ? u8(avc::kMbT8x8) : u8(0);
      avc::MbState s;
      avc::store_mb(pic, 0, rec, s, &res, nullptr);
      i16 got[avc::kDenseCoefs];
      avc::expand_coefs(pic.coefs.data(), pic.mbs[0], got);
      bad_avc += std::memcmp(got, want, sizeof got) != 0 ||
                 pic.coefs.size() != size_t(avc::coef_words(pic.mbs[0])) + avc::coef_values(pic.coefs.data(), pic.mbs[0]);
      // H.265: one TB per size, positions listed in random order
      for (int log2 = 2; log2 <= 5; ++log2) {
        const int nn = 1 << (2 * log2);
        std::vector<i16> dense(size_t(nn), 0), val_list, out(size_t(nn + nn / 16)), back(static_cast<size_t>(nn));
        std::vector<u16> pos;
        for (int k = 0; k < nn; ++k)
          if ((dense[size_t(k)] = val(dens))) pos.push_back(u16(k));
        for (size_t i = pos.size(); i > 1; --i) std::swap(pos[i - 1], pos[size_t(rnd() % i)]);
        for (u16 k : pos) val_list.push_back(dense[k]);
        const int n = hevc::hk_sparse_store(log2, pos.data(), val_list.data(), int(pos.size()), out.data());
        hevc::hk_sparse_expand(out.data(), log2, back.data());
        bad_hevc += back != dense || n != hevc::hk_sparse_words(log2) + int(pos.size());
      }
    }
    return std::make_pair(bad_avc, bad_hevc);
  });
  // Parse-only timing of an access-unit sequence (the host cost per picture; tools/bench).
  m.def("avc_parse_seconds", [](const std::vector<std::shared_ptr<AccessUnit>>& aus, int reps) {
    py::gil_scoped_release r;
    double best = 1e30;
    for (int k = 0; k < std::max(1, reps); ++k) {
      avc::Decoder dec;
      const i64 t0 = mono_us();
      for (const auto& au : aus) {
        size_t nal = 0;
        do dec.parse(*au, 0, &nal);
        while (nal < au->nals.size());
      }
      best = std::min(best, double(mono_us() - t0) * 1e-6);
    }
    return best;
  }, py::arg("aus"), py::arg("reps") = 3);
  m.def("avc_record_stats", [](const std::vector<std::shared_ptr<AccessUnit>>& aus) {
    py::gil_scoped_release r;
    avc::Decoder dec;
    u64 mbs = 0, coefs = 0, nz = 0, mvs = 0, pics = 0;
    for (const auto& au : aus) {
      auto p = dec.parse(*au);
      if (!p) continue;
      ++pics;
      mbs += p->mbs.size();
      coefs += p->coefs.size();
      mvs += p->mvs.size();
      for (const avc::MbRec& m : p->mbs)
        if (m.kind != avc::kIPcm) nz += avc::coef_values(p->coefs.data(), m);
    }
    py::gil_scoped_acquire g;
    py::dict d;
    d["pictures"] = pics;
    d["mbs"] = mbs;
    d["coefs"] = coefs;
    d["nonzero"] = nz;
    d["mvs"] = mvs;
    return d;
  });
  // Same for H.265 access units (records mode): pictures, transform blocks, coefficient-pool
  // entries (sparse: mask words + stored values per coded block), non-zero entries, prediction
  // blocks.
  m.def("hevc_record_stats", [](const std::vector<std::shared_ptr<AccessUnit>>& aus) {
    py::gil_scoped_release r;
    hevc::Decoder dec;
    dec.set_gpu_mode(true);
    u64 pics = 0, tus = 0, coefs = 0, nz = 0, pus = 0;
    for (const auto& au : aus) {
      dec.decode(*au);
      for (const auto& p : dec.take_gpu_pictures()) {
        ++pics;
        tus += p->tus.size();
        pus += p->pus.size();
        coefs += p->coefs.size();
        for (i16 c : p->coefs) nz += c != 0;
      }
    }
    py::gil_scoped_acquire g;
    py::dict d;
    d["pictures"] = pics;
    d["tus"] = tus;
    d["coefs"] = coefs;
    d["nonzero"] = nz;
    d["pus"] = pus;
    return d;
  });
  // Intra_8x8 tap forms (intra8x8_pred_tap / intra8x8_filter_tap, the GPU kernel's branch-free
  // form) against the direct formulas (intra8x8_pred_g / intra8x8_filter_at) on random samples:
  // every mode but DC, every sample position, every availability combination. Returns the
  // number of mismatching samples.
  m.def("avc_intra8x8_tap_check", [](u64 seed, int trials) {
    u64 st = seed * 0x9E3779B97F4A7C15ull + 7;
    auto rnd = [&]() {
      st ^= st << 13;
      st ^= st >> 7;
      st ^= st << 17;
      return int(st & 255);
    };
    int bad = 0;
    for (int t = 0; t < trials; ++t) {
      int s[25];
      for (int k = 0; k < 25; ++k) s[k] = (t & 3) == 0 ? (rnd() & 1) * 255 : rnd();  // extremes too
      auto T = [&](int i) { return s[1 + i]; };
      auto L = [&](int j) { return j < 0 ? s[0] : s[17 + j]; };
      for (int mode = 0; mode < 9; ++mode) {
        if (mode == 2) continue;
        for (int y = 0; y < 8; ++y)
          for (int x = 0; x < 8; ++x) {
            const u32 tw = avc::intra8x8_pred_tap(mode, x, y);
            const int got = avc::eval_tap8(tw, s[tw & 31], s[(tw >> 5) & 31], s[(tw >> 10) & 31]);
            bad += got != avc::intra8x8_pred_g(T, L, true, true, mode, x, y);
          }
      }
      for (int av = 0; av < 8; ++av) {
        const bool top = av & 1, left = av & 2, tl = av & 4;
        for (int k = 0; k < 25; ++k) {
          const u32 tw = avc::intra8x8_filter_tap(top, left, tl, k);
          const int got =
              (tw & avc::kTap8Const) ? 128 : avc::eval_tap8(tw, s[tw & 31], s[(tw >> 5) & 31], s[(tw >> 10) & 31]);
          bad += got != avc::intra8x8_filter_at(T, [&](int j) { return s[17 + j]; }, top, left, tl, k);
        }
      }
    }
    return bad;
  });
  // Random-bin CABAC engine round trip (context-coded with skewed and flipping statistics,
  // bypass, terminate-0 and a final terminate-1 flush). Returns (ok, coded_bytes).
  m.def("cabac_roundtrip", [](u64 seed, int n, int qp) {
    u64 st = seed * 0x9E3779B97F4A7C15ull + 1;
    auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    const size_t nn = static_cast<size_t>(n);
    std::vector<u8> kind(nn), ctx(nn), bin(nn);
    for (int i = 0; i < n; ++i) {
      u64 r = rnd();
      kind[size_t(i)] = u8((r & 15) == 0 ? 1 : ((r & 63) == 1 ? 2 : 0));  // 0 ctx, 1 bypass, 2 term0
      ctx[size_t(i)] = u8((r >> 8) % 4);
      const int p = ctx[size_t(i)] == 0 ? 2 : ctx[size_t(i)] == 1 ? 50 : ctx[size_t(i)] == 2 ? 97 : ((i / 500) & 1) ? 90 : 10;
      bin[size_t(i)] = kind[size_t(i)] == 2 ? 0 : u8(int((r >> 20) % 100) < p);
    }
    std::vector<u8> buf;
    cabac::Ctx ce[4], cd[4];
    const int init[4] = {197, 154, 122, 139};
    for (int k = 0; k < 4; ++k) ce[k].init(init[k], qp), cd[k].init(init[k], qp);
    {
      cabac::Encoder e(buf);
      for (int i = 0; i < n; ++i) {
        if (kind[size_t(i)] == 0) e.decision(ce[ctx[size_t(i)]], bin[size_t(i)]);
        else if (kind[size_t(i)] == 1) e.bypass(bin[size_t(i)]);
        else e.terminate(0);
      }
      e.terminate(1);
      e.align_zero();
    }
    cabac::Decoder d(buf.data(), buf.size(), 0);
    bool ok = true;
    for (int i = 0; i < n && ok; ++i) {
      u32 b;
      if (kind[size_t(i)] == 0) b = d.decision(cd[ctx[size_t(i)]]);
      else if (kind[size_t(i)] == 1) b = d.bypass();
      else b = d.terminate();
      ok = b == bin[size_t(i)];
    }
    ok = ok && d.terminate() == 1 && d.aligned_bytepos() == buf.size();
    return py::make_tuple(ok, buf.size());
  });
  // Host parse cost of one AU (µs, mean over iters) and of its emulation-prevention scan alone.
  m.def("parse_cost_us", [](const AccessUnit& au, int iters, std::shared_ptr<AccessUnit> prime) {
    py::gil_scoped_release r;
    StreamParser p;
    MbUpdate u;
    if (prime) p.absorb_parameter_sets(*prime);
    p.parse(au, u);
    i64 t0 = mono_us();
    for (int k = 0; k < iters; ++k) {
      u.clear_payload();
      p.parse(au, u);
    }
    const double parse_us = double(mono_us() - t0) / iters;
    std::vector<u32> epb;
    t0 = mono_us();
    for (int k = 0; k < iters; ++k)
      for (size_t i = 0; i < au.nals.size(); ++i) find_epb(au.nal(i), au.nal_size(i), epb);
    const double scan_us = double(mono_us() - t0) / iters;
    return std::make_pair(parse_us, scan_us);
  }, py::arg("au"), py::arg("iters") = 100, py::arg("prime") = nullptr);
  m.def("rocdecode_available", [] { return gpu::rocdecode_available(); });
  m.def("cabac_bins_decoded", [] { return cabac::bins_decoded().load(); },
        "CABAC bins decoded by this process so far (H.264 and H.265 slices, counted as each ends)");
  m.def("tsc_now", [] { return u64(__builtin_ia32_rdtsc()); }, "the x86 time-stamp counter");
  m.def("hostprof_start", &hostprof::start, py::arg("interval_us") = 1000,
        "start sampling host CPU time (SIGPROF, every thread of the process)");
  m.def("hostprof_stop", &hostprof::stop, py::arg("path"), "stop sampling; write 'count object offset symbol' lines");
  // VCN backend (vcn.h): which librocdecode is loaded, why none is, load a specific build
  m.def("vcn_library", [] { return vcn::library(); });
  m.def("vcn_load_error", [] { return vcn::load_error(); });
  m.def("vcn_load", [](const std::string& path) { return vcn::load(path); }, py::arg("path"));
  m.def("pinned_pool_stats", [] {
    hostmem::PoolStats st = hostmem::pool_stats();
    py::dict d;
    d["enabled"] = hostmem::pool_enabled();
    d["chunks"] = st.chunks;
    d["bytes_reserved"] = st.bytes_reserved;
    d["blocks_live"] = st.blocks_live;
    d["blocks_reused"] = st.blocks_reused;
    d["fallbacks"] = st.fallbacks;
    return d;
  });
  m.def("hvcc_record", [](const std::string& vps, const std::string& sps, const std::string& pps) {
    auto v = [](const std::string& x) { return std::vector<u8>(x.begin(), x.end()); };
    std::vector<u8> r = hevc::hvcc_record(v(vps), v(sps), v(pps));
    return to_bytes(r.data(), r.size());
  });
  m.def("rbsp_to_ebsp", [](const std::string& r) {
    std::vector<u8> out;
    rbsp_to_ebsp(reinterpret_cast<const u8*>(r.data()), r.size(), out);
    return to_bytes(out.data(), out.size());
  });
  m.def("ebsp_to_rbsp", [](const std::string& e) {
    std::vector<u8> out(e.size());
    size_t n = ebsp_to_rbsp(reinterpret_cast<const u8*>(e.data()), e.size(), out.data());
    return to_bytes(out.data(), n);
  });
  m.def("find_epb", [](const std::string& e) {
    std::vector<u32> out;
    find_epb(reinterpret_cast<const u8*>(e.data()), e.size(), out);
    return out;
  });
  m.def("split_annexb", [](const std::string& b) {
    auto v = h264::split_annexb(reinterpret_cast<const u8*>(b.data()), b.size());
    py::list l;
    for (auto& [o, n] : v) l.append(py::bytes(b.data() + o, n));
    return l;
  });
  m.def("bitwriter_roundtrip", [](const std::vector<u32>& ue_vals, const std::vector<i32>& se_vals) {
    BitWriter bw;
    for (u32 v : ue_vals) bw.ue(v);
    for (i32 v : se_vals) bw.se(v);
    bw.trailing();
    BitReader br(bw.buf().data(), bw.buf().size());
    std::vector<u32> u;
    std::vector<i32> s;
    for (size_t i = 0; i < ue_vals.size(); ++i) u.push_back(br.ue());
    for (size_t i = 0; i < se_vals.size(); ++i) s.push_back(br.se());
    bool at_stop = br.bitpos() == br.stop_bit_pos();
    return py::make_tuple(u, s, at_stop);
  });

  m.def(
      "plan_host_domains",
      [](const std::vector<int>& devices, const std::vector<std::string>& explicit_cpus, int reserve) {
        py::list out;
        for (const HostDomain& d : plan_host_domains(devices, explicit_cpus, reserve)) out.append(domain_dict(d));
        return out;
      },
      py::arg("devices"), py::arg("explicit_cpus") = std::vector<std::string>{}, py::arg("reserve") = 1,
      "Per-worker host domains (hostplan.h): CPUs, NUMA node, parse / io thread counts");
  m.def("affinity_cpus", &affinity_cpus);
  m.def("parse_cpulist", &parse_cpulist);
  m.def("format_cpulist", &format_cpulist);
  m.def("cpu_budget", &cpu_budget);
  py::class_<Worker>(m, "Worker")
      .def(py::init([](int device, int letterbox_size, int chw_dtype, std::vector<float> mean,
                       std::vector<float> stdv, int max_cameras, int pack_threads,
                       int letterbox_format, int lanes, int stages, int queue, bool lane_threads,
                       const std::string& decoder, int kf_window_us, py::object host_domain,
                       bool ref_copies, bool backpressure) {
             WorkerOptions o;
             o.device = device;
             if (!host_domain.is_none()) {
               o.domain = domain_from(host_domain.cast<py::dict>());
               VEP_CHECK(o.domain.device == device, "host_domain belongs to another device");
             }
             if (decoder == "native") o.decoder = kDecoderNative;
             else if (decoder == "vcn") o.decoder = kDecoderVcn;
             else if (decoder == "auto") o.decoder = kDecoderAuto;
             else throw Error("decoder must be native, vcn or auto (got '" + decoder + "')");
             o.lanes = lanes;
             o.stages = stages;
             o.queue = queue;
             o.lane_threads = lane_threads;
             o.kf_window_us = kf_window_us;
             o.ref_copies = ref_copies;
             o.backpressure = backpressure;
             o.pack_threads = pack_threads;
             o.letterbox_format = letterbox_format;
             o.letterbox_size = letterbox_size;
             o.chw_dtype = chw_dtype;
             for (int k = 0; k < 3; ++k) {
               o.mean[k] = mean.size() == 3 ? mean[size_t(k)] : 0.f;
               o.std[k] = stdv.size() == 3 ? stdv[size_t(k)] : 1.f;
             }
             o.max_cameras = max_cameras;
             return std::make_unique<Worker>(o);
           }),
           py::arg("device") = 0, py::arg("letterbox_size") = 0, py::arg("chw_dtype") = 0,
           py::arg("mean") = std::vector<float>{}, py::arg("std") = std::vector<float>{},
           py::arg("max_cameras") = 256, py::arg("pack_threads") = 4,
           py::arg("letterbox_format") = 0, py::arg("lanes") = 0, py::arg("stages") = 0,
           py::arg("queue") = 0, py::arg("lane_threads") = false, py::arg("decoder") = "native",
           py::arg("kf_window_us") = -1, py::arg("host_domain") = py::none(), py::arg("ref_copies") = false,
           py::arg("backpressure") = false)
      .def_property_readonly("ref_copy_bytes", &Worker::ref_copy_bytes)
      .def_property_readonly("kf_window_us", &Worker::kf_window_us)
      .def_property_readonly("host_domain", [](Worker& w) { return domain_dict(w.host_domain()); })
      .def_property_readonly("ingest_parse_threads", &Worker::ingest_parse_threads)
      .def_property_readonly("device", [](Worker& w) { return w.device().id(); })
      .def_property_readonly("decoder", [](Worker& w) { return std::string(w.vcn() ? "vcn" : "native"); })
      .def_property_readonly("lanes", &Worker::lanes)
      .def_property_readonly("stages", &Worker::stages)
      .def_property_readonly("inflight", &Worker::inflight)
      .def_property_readonly("launch_seq", &Worker::launch_seq)
      .def("wait_published", &Worker::wait_published, py::arg("seq"),
           py::call_guard<py::gil_scoped_release>())
      .def("add_camera", &Worker::add_camera, py::arg("name"), py::arg("ring_slots") = 2, py::arg("history") = 0)
      .def("history_ring_slots", &Worker::history_ring_slots, py::arg("history"))
      .def("remove_camera", &Worker::remove_camera, py::call_guard<py::gil_scoped_release>())
      .def("find", [](Worker& w, const std::string& n) { auto c = w.find(n); return c ? c->index() : -1; })
      .def("num_cameras", &Worker::num_cameras)
      .def("start", &Worker::start)
      .def("stop", &Worker::stop, py::call_guard<py::gil_scoped_release>())
      .def("flush", &Worker::flush, py::call_guard<py::gil_scoped_release>())
      .def("complete_all", &Worker::complete_all, py::call_guard<py::gil_scoped_release>())
      .def("set_last_query", [](Worker& w, int i, i64 ms) { cam_of(w, i).last_query_ms.store(ms); })
      .def("last_query", [](Worker& w, int i) { return cam_of(w, i).last_query_ms.load(); })
      .def("set_keyframe_only", [](Worker& w, int i, bool v) { cam_of(w, i).keyframe_only.store(v); })
      .def("keyframe_only", [](Worker& w, int i) { return cam_of(w, i).keyframe_only.load(); })
      .def("set_proxy", [](Worker& w, int i, bool v) { cam_of(w, i).proxy_rtmp.store(v); })
      .def("proxy", [](Worker& w, int i) { return cam_of(w, i).proxy_rtmp.load(); })
      .def("set_idle_cutoff_ms", [](Worker& w, int i, i64 v) { cam_of(w, i).idle_cutoff_ms.store(v); })
      .def("submit_au",
           [](Worker& w, int i, std::shared_ptr<AccessUnit> au) {
             Camera& c = cam_of(w, i);
             py::gil_scoped_release r;
             return c.on_access_unit(au);
           })
      .def("read_surface",
           [](Worker& w, int i) -> py::object {
             HostSurface s;
             i64 pts = 0;
             bool ok;
             {
               py::gil_scoped_release r;
               ok = w.read_surface(i, s, &pts);
             }
             if (!ok) return py::none();
             return py::make_tuple(pts, surface_planes(s));
           },
           py::arg("cam"),
           "(pts, (y, uv)) of the DPB surface holding the camera's newest published picture at full "
           "sample depth (uint16 above 8 bits), coded size; None when none. Call with the camera idle.")
      .def("decode_now",
           [](Worker& w, int i, std::shared_ptr<AccessUnit> au) {
             Camera& c = cam_of(w, i);
             py::gil_scoped_release r;
             DecodeJob job;
             if (!c.make_job(au, job)) return false;
             std::vector<DecodeJob> v;
             v.push_back(std::move(job));
             w.run_batch(v);
             return true;
           })
      .def("decode_many",
           [](Worker& w, const std::vector<std::pair<int, std::vector<std::shared_ptr<AccessUnit>>>>& work,
              bool sync) {
             // one batch: per camera all given AUs (merged into one job, GOP catch-up style)
             std::vector<std::shared_ptr<Camera>> keep;
             for (auto& [idx, aus] : work) keep.push_back(cam_ref(w, idx));
             py::gil_scoped_release r;
             std::vector<DecodeJob> jobs;
             for (size_t k = 0; k < work.size(); ++k) {
               DecodeJob merged;
               bool have = false;
               for (auto& au : work[k].second) {
                 DecodeJob j;
                 if (!keep[k]->make_job(au, j)) continue;
                 if (!have) merged = std::move(j);
                 else merge_job(merged, std::move(j));
                 have = true;
               }
               if (have) jobs.push_back(std::move(merged));
             }
             const size_t n = jobs.size();
             if (sync) w.run_batch(jobs);
             else w.launch_async(jobs);  // published later (launch_seq / wait_published)
             return n;
           },
           py::arg("work"), py::arg("sync") = true)
      .def("avc_profile", [](Worker& w) {
        static const char* kNames[gpu::kAvcProfSlots] = {
            "intra_wait", "intra_load", "intra_luma", "intra_chroma", "intra_store", "intra_mbs",
            "dbk_wait", "dbk_load", "dbk_filter", "dbk_store", "dbk_mbs", "intra_residual",
            "hbd_intra", "hbd_dbk", "hbd_barrier", "hbd_pictures", "hbd_dbk_load", "hbd_dbk_edges",
            "hbd_dbk_store", "hbd_dbk_mbs"};
        const std::vector<u64> v = w.avc_profile();
        py::dict d;
        for (int i = 0; i < gpu::kAvcProfSlots; ++i) d[kNames[i]] = v[size_t(i)];
        return d;
      })
      .def("stats",
           [](Worker& w, int i) {
             Camera& c = cam_of(w, i);
             py::dict d;
             d["packets"] = c.packets.load();
             d["decoded"] = c.decoded.load();
             d["skipped"] = c.skipped.load();
             d["shed"] = c.shed.load();
             d["errors"] = c.errors.load();
             d["bytes_in"] = c.bytes_in.load();
             d["last_packet_ms"] = c.last_packet_ms.load();
             d["decoder"] = c.general_decoder() ? "general" : "fast";
             d["backend"] = c.backend();
             auto ring = c.ring();
             d["published"] = ring ? ring->published() : 0;
             d["width"] = ring ? ring->width() : 0;
             d["height"] = ring ? ring->height() : 0;
             d["ring_slots"] = ring ? ring->slots() : c.ring_slots_cfg;
             d["history"] = c.history();
             d["history_skipped"] = c.history_skipped.load();
             d["motion_evaluations"] = c.motion_evaluations.load();
             d["motion_frames"] = c.motion_frames.load();
             d["tamper_evaluations"] = c.tamper_evaluations.load();
             d["tamper_frames_tampered"] = c.tamper_frames.load();
             d["masked_frames"] = c.masked_frames.load();
             d["mask_dropped"] = c.mask_dropped.load();
             py::list hist;
             for (auto& h : c.lat_hist) hist.append(h.load());
             d["latency_hist"] = hist;
             d["latency_sum_ms"] = c.lat_sum_ms.load();
             py::list bounds;
             for (double b : Camera::kLatBucketsMs) bounds.append(b);
             d["latency_bounds_ms"] = bounds;
             return d;
           })
      .def("log", [](Worker& w, int i, bool err, const std::string& line) { cam_of(w, i).logs.add(err, line); })
      .def("logs", [](Worker& w, int i, bool err, int last) { return cam_of(w, i).logs.dump(err, size_t(last)); },
           py::arg("idx"), py::arg("err") = false, py::arg("last") = 100)
      .def("read_latest",
           [](Worker& w, int i, i64 after) -> py::object {
             std::shared_ptr<FrameRing> ring = cam_of(w, i).ring();
             if (!ring) return py::none();
             size_t n = ring->slot_bytes();
             py::array_t<uint8_t> out({ring->height(), ring->width(), 3});
             FrameMeta m;
             bool ok;
             u8* dst = out.mutable_data();
             {
               py::gil_scoped_release r;
               ok = w.read_latest(*ring, after, &m, dst, n);
             }
             if (!ok) return py::none();
             return py::make_tuple(meta_dict(m), out);
           },
           py::arg("idx"), py::arg("after") = 0)
      .def("read_latest_jpeg",
           // (meta, bytes) of the newest frame with seq > after as a JPEG stream, None if there
           // is none; encoded on the GPU from the ring slot (CPU backend: on the host).
           // width / height (0 = not given): fitted into that box and downscaled first; meta then
           // carries the scaled size.
           [](Worker& w, int i, i64 after, int quality, int width, int height) -> py::object {
             std::shared_ptr<Camera> keep = cam_ref(w, i);
             FrameMeta m;
             std::string out;
             bool ok;
             {
               py::gil_scoped_release r;
               ok = w.read_latest_jpeg(i, after, quality, &m, out, width, height);
             }
             if (!ok) return py::none();
             return py::make_tuple(meta_dict(m), py::bytes(out));
           },
           py::arg("idx"), py::arg("after") = 0, py::arg("quality") = 85, py::arg("width") = 0,
           py::arg("height") = 0)
      .def("read_latest_scaled",
           // (meta, ndarray) of the newest frame with seq > after, fitted into width x height
           // (0 = that side not given) and downscaled where it lies; None if there is none.
           [](Worker& w, int i, i64 after, int width, int height) -> py::object {
             std::shared_ptr<Camera> keep = cam_ref(w, i);
             FrameMeta m;
             std::vector<u8> px;
             bool ok;
             {
               py::gil_scoped_release r;
               ok = w.read_latest_scaled(i, after, width, height, &m, px);
             }
             if (!ok) return py::none();
             py::array_t<uint8_t> a({py::ssize_t(m.height), py::ssize_t(m.width), py::ssize_t(3)});
             std::memcpy(a.mutable_data(), px.data(), px.size());
             return py::make_tuple(meta_dict(m), a);
           },
           py::arg("idx"), py::arg("after") = 0, py::arg("width") = 0, py::arg("height") = 0)
      .def("read_wall_jpeg",
           // (seqs, bytes): one JPEG of the newest frames of `cams` (camera indices; -1 = an empty
           // tile), tile t fitted into cell t of a cols-wide grid of tile_width x tile_height
           // cells (cols 0: ceil(sqrt(n))). foreign[t], if not None, is (seq, ndarray): an already
           // scaled tile of a camera that lives on another worker. seqs[t] is 0 for a tile drawn
           // as background.
           // labels (a list of one str per tile, "" for none): drawn at the top-left corner of every
           // tile that shows a frame (docs/OVERLAY.md); more than 128 labels are a ValueError.
           [](Worker& w, const std::vector<int>& cams, int cols, int tw, int th, int quality, py::object foreign,
              py::object labels) {
             std::vector<std::string> names;
             if (!labels.is_none()) {
               names = labels.cast<std::vector<std::string>>();
               size_t labelled = 0;
               for (const std::string& l : names) {
                 if (l.size() > size_t(overlay::kMaxRawText)) throw py::value_error("overlay: a text has at most 256 bytes");
                 labelled += !l.empty();
               }
               if (names.size() != cams.size()) throw py::value_error("wall: one label per tile expected");
               if (labelled * 2 > size_t(overlay::kMaxPrims))
                 throw py::value_error("overlay: the wall's labels expand to more than 256 primitives");
             }
             std::vector<Worker::ForeignTile> ft;
             std::vector<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>> keep;
             if (!foreign.is_none()) {
               py::list fl = foreign.cast<py::list>();
               VEP_CHECK(fl.size() == cams.size(), "wall: one foreign tile entry per tile expected");
               ft.resize(cams.size());
               for (size_t t = 0; t < cams.size(); ++t) {
                 if (fl[t].is_none()) continue;
                 py::tuple e = fl[t].cast<py::tuple>();
                 VEP_CHECK(e.size() == 2, "wall: a foreign tile is (seq, ndarray)");
                 keep.push_back(e[1].cast<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>>());
                 const auto& a = keep.back();
                 VEP_CHECK(a.ndim() == 3 && a.shape(2) == 3 && a.shape(0) >= 1 && a.shape(1) >= 1 &&
                               a.shape(0) <= 65535 && a.shape(1) <= 65535,
                           "wall: a foreign tile is an (H, W, 3) uint8 picture");
                 ft[t].data = a.data();
                 ft[t].w = int(a.shape(1));
                 ft[t].h = int(a.shape(0));
                 ft[t].seq = e[0].cast<i64>();
               }
             }
             std::vector<i64> seqs;
             std::string out;
             {
               py::gil_scoped_release r;
               if (labels.is_none()) w.read_wall_jpeg(cams, cols, tw, th, quality, ft, seqs, out);
               else w.read_wall_jpeg_labelled(cams, cols, tw, th, quality, ft, names, seqs, out);
             }
             return py::make_tuple(seqs, py::bytes(out));
           },
           py::arg("cams"), py::arg("cols") = 0, py::arg("tile_width") = 320, py::arg("tile_height") = 180,
           py::arg("quality") = 85, py::arg("foreign") = py::none(), py::arg("labels") = py::none())
      .def("read_overlay_jpeg",
           // read_latest_jpeg with the overlay items drawn on the picture (docs/OVERLAY.md): {name},
           // {seq} and {time} come from `name` and the meta of the frame actually encoded.
           [](Worker& w, int i, const std::vector<ItemTuple>& items, const std::string& name, i64 after, int quality,
              int width, int height) -> py::object {
             std::shared_ptr<Camera> keep = cam_ref(w, i);
             const std::vector<overlay::Item> its = items_of(items);
             if (after < 0) throw py::value_error("overlay: after must be >= 0");
             if (quality < 1 || quality > 100) throw py::value_error("jpeg: quality must be 1..100");
             if (width < 0 || width > 65535 || height < 0 || height > 65535)
               throw py::value_error("scale: width and height must be 1..65535 (0: not given)");
             FrameMeta m;
             std::string out;
             bool ok;
             std::string refused;
             {
               py::gil_scoped_release r;
               try {
                 ok = w.read_overlay_jpeg(i, after, quality, its, name, &m, out, width, height);
               } catch (const Error& e) {
                 // (only the expansion can refuse a checked list: too many primitives)
                 if (std::string(e.what()).find("overlay:") == std::string::npos) throw;
                 refused = e.what();
                 ok = false;
               }
             }
             if (!refused.empty()) throw py::value_error(refused);
             if (!ok) return py::none();
             return py::make_tuple(meta_dict(m), py::bytes(out));
           },
           py::arg("idx"), py::arg("items"), py::arg("name") = "", py::arg("after") = 0, py::arg("quality") = 85,
           py::arg("width") = 0, py::arg("height") = 0)
      .def("overlay_counts", [](Worker& w) { return w.overlay_counts(); })
      .def_property("wall_max_tiles", &Worker::wall_max_tiles, &Worker::set_wall_max_tiles)
      .def("read_motion",
           // dict of the newest frame with seq > after against the camera's background model
           // (docs/MOTION.md), None if there is no such frame. A frame is evaluated once, on the
           // GPU from its ring slot (CPU backend: on the host); later calls get the stored answer.
           [](Worker& w, int i, i64 after) -> py::object {
             std::shared_ptr<Camera> keep = cam_ref(w, i);
             MotionResult r;
             bool ok;
             {
               py::gil_scoped_release rel;
               ok = w.read_motion(i, after, r);
             }
             if (!ok) return py::none();
             return motion_dict(r);
           },
           py::arg("idx"), py::arg("after") = 0)
      .def("read_motion_many",
           // [dict | None] of the newest frames of `cams`, every evaluation in one launch. None: an
           // unknown index, no ring, no frame, or a frame that stayed inconsistent.
           [](Worker& w, const std::vector<int>& cams) {
             std::vector<MotionResult> rs;
             std::vector<char> ok;
             {
               py::gil_scoped_release rel;
               w.read_motion_many(cams, rs, ok);
             }
             py::list out;
             for (size_t k = 0; k < rs.size(); ++k) out.append(ok[k] ? py::object(motion_dict(rs[k])) : py::object(py::none()));
             return out;
           },
           py::arg("cams"))
      .def("set_motion_params",
           [](Worker& w, int cell, int threshold, int learn_shift, int cell_percent, int min_cells) {
             motion::Params p;
             p.cell = cell;
             p.threshold = threshold;
             p.learn_shift = learn_shift;
             p.cell_percent = cell_percent;
             p.min_cells = min_cells;
             py::gil_scoped_release rel;
             w.set_motion_params(p);
           },
           py::arg("cell") = 16, py::arg("threshold") = 24, py::arg("learn_shift") = 4, py::arg("cell_percent") = 25,
           py::arg("min_cells") = 1)
      .def_property_readonly("motion_params",
                             [](Worker& w) {
                               const motion::Params p = w.motion_params();
                               py::dict d;
                               d["cell"] = p.cell;
                               d["threshold"] = p.threshold;
                               d["learn_shift"] = p.learn_shift;
                               d["cell_percent"] = p.cell_percent;
                               d["min_cells"] = p.min_cells;
                               return d;
                             })
      .def("motion_reset",
           [](Worker& w, int i) {
             std::shared_ptr<Camera> keep = cam_ref(w, i);
             py::gil_scoped_release rel;
             w.motion_reset(i);
           },
           py::arg("idx"))
      .def("read_tamper",
           // dict of the newest frame with seq > after: luma histogram, per-cell sums and energies
           // and the flags derived from them (docs/TAMPER.md), None if there is no such frame. A
           // frame is evaluated once, on the GPU from its ring slot (CPU backend: on the host);
           // later calls get the stored answer.
           [](Worker& w, int i, i64 after) -> py::object {
             std::shared_ptr<Camera> keep = cam_ref(w, i);
             TamperResult r;
             bool ok;
             {
               py::gil_scoped_release rel;
               ok = w.read_tamper(i, after, r);
             }
             if (!ok) return py::none();
             return tamper_dict(r);
           },
           py::arg("idx"), py::arg("after") = 0)
      .def("read_tamper_many",
           // [dict | None] of the newest frames of `cams`, every evaluation in one launch. None: an
           // unknown index, no ring, no frame, or a frame that stayed inconsistent.
           [](Worker& w, const std::vector<int>& cams) {
             std::vector<TamperResult> rs;
             std::vector<char> ok;
             {
               py::gil_scoped_release rel;
               w.read_tamper_many(cams, rs, ok);
             }
             py::list out;
             for (size_t k = 0; k < rs.size(); ++k) out.append(ok[k] ? py::object(tamper_dict(rs[k])) : py::object(py::none()));
             return out;
           },
           py::arg("cams"))
      .def("set_tamper_params",
           [](Worker& w, int cell, int dark_level, int bright_level, int spread_min, int focus_percent, int shift_level,
              int shift_percent) {
             const tamper::Params p =
                 tamper_params_of(cell, dark_level, bright_level, spread_min, focus_percent, shift_level, shift_percent);
             py::gil_scoped_release rel;
             w.set_tamper_params(p);
           },
           py::arg("cell") = 32, py::arg("dark_level") = 32, py::arg("bright_level") = 224, py::arg("spread_min") = 24,
           py::arg("focus_percent") = 50, py::arg("shift_level") = 24, py::arg("shift_percent") = 50)
      .def_property_readonly("tamper_params", [](Worker& w) { return tamper_params_dict(w.tamper_params()); })
      .def("tamper_set_reference",
           // the camera's newest frame becomes its reference; False when it has no frame
           [](Worker& w, int i) {
             std::shared_ptr<Camera> keep = cam_ref(w, i);
             py::gil_scoped_release rel;
             return w.tamper_set_reference(i);
           },
           py::arg("idx"))
      .def("tamper_reset",
           [](Worker& w, int i) {
             std::shared_ptr<Camera> keep = cam_ref(w, i);
             py::gil_scoped_release rel;
             w.tamper_reset(i);
           },
           py::arg("idx"))
      .def("set_privacy_masks",
           [](Worker& w, int i, const std::vector<MaskTuple>& masks) {
             std::shared_ptr<Camera> keep = cam_ref(w, i);
             const std::vector<mask::Mask> ms = masks_of(masks);
             py::gil_scoped_release rel;
             w.set_privacy_masks(i, ms);
           },
           py::arg("idx"), py::arg("masks"))
      .def("privacy_masks",
           [](Worker& w, int i) {
             std::shared_ptr<Camera> keep = cam_ref(w, i);
             return mask_tuples(w.privacy_masks(i));
           },
           py::arg("idx"))
      .def("read_crops",
           // (meta, ndarray (n, height, width, 3)) of the boxes of the newest frame with seq > after
           // (seq 0) or of frame `seq`, cut and resized where the frame lies; None if there is no
           // such frame. ValueError on an invalid list, size, fit or pad colour.
           [](Worker& w, int i, const std::vector<BoxTuple>& boxes, int width, int height, i64 after, i64 seq, int fit,
              const PadTuple& pad) -> py::object {
             std::shared_ptr<Camera> keep = cam_ref(w, i);
             const std::vector<crop::Box> bs = boxes_of(boxes);
             const crop::Pad p = crop_output_of(width, height, fit, pad);
             if (after < 0 || seq < 0) throw py::value_error("crop: after and seq must be >= 0");
             FrameMeta m;
             std::vector<u8> px;
             bool ok;
             {
               py::gil_scoped_release r;
               ok = w.read_crops(i, after, seq, bs, width, height, fit, p, &m, px);
             }
             if (!ok) return py::none();
             return py::make_tuple(meta_dict(m), crops_array(px, bs.size(), width, height));
           },
           py::arg("idx"), py::arg("boxes"), py::arg("width"), py::arg("height"), py::arg("after") = 0,
           py::arg("seq") = 0, py::arg("fit") = 0, py::arg("pad") = PadTuple(crop::kPad, crop::kPad, crop::kPad))
      .def("read_crops_many",
           // [(meta, ndarray) | None] for requests (idx, after, seq, boxes), a camera may repeat: the
           // crops of every request in one launch a round. None: an unknown index, no ring, no
           // such frame, or a frame that stayed inconsistent.
           [](Worker& w, const std::vector<std::tuple<int, i64, i64, std::vector<BoxTuple>>>& requests, int width,
              int height, int fit, const PadTuple& pad) {
             const crop::Pad p = crop_output_of(width, height, fit, pad);
             std::vector<Worker::CropRequest> reqs(requests.size());
             for (size_t k = 0; k < requests.size(); ++k) {
               reqs[k].cam = std::get<0>(requests[k]);
               reqs[k].after = std::get<1>(requests[k]);
               reqs[k].seq = std::get<2>(requests[k]);
               if (reqs[k].after < 0 || reqs[k].seq < 0) throw py::value_error("crop: after and seq must be >= 0");
               reqs[k].boxes = boxes_of(std::get<3>(requests[k]));
             }
             {
               py::gil_scoped_release r;
               w.read_crops_many(reqs, width, height, fit, p);
             }
             py::list out;
             for (Worker::CropRequest& r : reqs)
               out.append(r.ok ? py::object(py::make_tuple(meta_dict(r.meta), crops_array(r.data, r.boxes.size(), width, height)))
                               : py::object(py::none()));
             return out;
           },
           py::arg("requests"), py::arg("width"), py::arg("height"), py::arg("fit") = 0,
           py::arg("pad") = PadTuple(crop::kPad, crop::kPad, crop::kPad))
      .def("read_crop_jpeg",
           // (meta, bytes): one box as a JPEG, the encoder chained onto the crop on the device.
           [](Worker& w, int i, const BoxTuple& box, int width, int height, i64 after, i64 seq, int quality, int fit,
              const PadTuple& pad) -> py::object {
             std::shared_ptr<Camera> keep = cam_ref(w, i);
             const std::vector<crop::Box> bs = boxes_of({box});
             const crop::Pad p = crop_output_of(width, height, fit, pad);
             if (after < 0 || seq < 0) throw py::value_error("crop: after and seq must be >= 0");
             if (quality < 1 || quality > 100) throw py::value_error("jpeg: quality must be 1..100");
             FrameMeta m;
             std::string out;
             bool ok;
             {
               py::gil_scoped_release r;
               ok = w.read_crop_jpeg(i, after, seq, bs[0], width, height, fit, p, quality, &m, out);
             }
             if (!ok) return py::none();
             return py::make_tuple(meta_dict(m), py::bytes(out));
           },
           py::arg("idx"), py::arg("box"), py::arg("width"), py::arg("height"), py::arg("after") = 0,
           py::arg("seq") = 0, py::arg("quality") = 85, py::arg("fit") = 0,
           py::arg("pad") = PadTuple(crop::kPad, crop::kPad, crop::kPad))
      .def("read_history",
           // [(meta, ndarray)] of the newest `count` (0 = the camera's history depth) frames with
           // seq > after: ascending, contiguous in seq, ending at the newest frame.
           [](Worker& w, int i, i64 after, int count) {
             std::shared_ptr<Camera> keep = cam_ref(w, i);
             std::vector<Worker::HistoryFrame> fs;
             {
               py::gil_scoped_release r;
               fs = w.read_history(i, after, count);
             }
             py::list out;
             for (Worker::HistoryFrame& f : fs) {
               u8* p = f.data.release();
               py::capsule own(p, [](void* q) { delete[] static_cast<u8*>(q); });
               py::array_t<uint8_t> a({py::ssize_t(f.meta.height), py::ssize_t(f.meta.width), py::ssize_t(3)}, p, own);
               out.append(py::make_tuple(meta_dict(f.meta), a));
             }
             return out;
           },
           py::arg("idx"), py::arg("after") = 0, py::arg("count") = 0)
      .def("history_seqs",
           // the seqs read_history would return (nothing is copied)
           [](Worker& w, int i, i64 after, int count) {
             std::vector<i64> seqs;
             std::shared_ptr<FrameRing> ring = cam_of(w, i).ring();
             if (!ring) return seqs;
             const int depth = std::max(1, ring->history());
             std::vector<std::pair<FrameMeta, int>> v;
             ring->range(after, count > 0 ? std::min(count, depth) : depth, v);
             for (const auto& e : v) seqs.push_back(e.first.seq);
             return seqs;
           },
           py::arg("idx"), py::arg("after") = 0, py::arg("count") = 0)
      .def("video_frames",
           // [(seq, bytes)]: the same frames as serialized VideoFrame protos (encode_video_frame).
           [](Worker& w, int i, i64 after, int count, const std::string& device_id) {
             std::shared_ptr<Camera> keep = cam_ref(w, i);
             std::vector<Worker::HistoryFrame> fs;
             {
               py::gil_scoped_release r;
               fs = w.read_history(i, after, count);
             }
             py::list out;
             for (const Worker::HistoryFrame& f : fs) {
               const auto [pre, suf] = encode_video_frame(f.meta, f.bytes, device_id);
               PyObject* b = PyBytes_FromStringAndSize(nullptr, Py_ssize_t(pre.size() + f.bytes + suf.size()));
               if (!b) throw py::error_already_set();
               char* buf = PyBytes_AS_STRING(b);
               std::memcpy(buf, pre.data(), pre.size());
               std::memcpy(buf + pre.size(), f.data.get(), f.bytes);
               std::memcpy(buf + pre.size() + f.bytes, suf.data(), suf.size());
               out.append(py::make_tuple(f.meta.seq, py::reinterpret_steal<py::object>(b)));
             }
             return out;
           },
           py::arg("idx"), py::arg("after") = 0, py::arg("count") = 0, py::arg("device_id") = "")
      .def("video_frame_bound",
           // Upper bound of the serialized VideoFrame of this camera's current ring (0: no ring).
           [](Worker& w, int i, const std::string& device_id) -> size_t {
             std::shared_ptr<FrameRing> ring = cam_of(w, i).ring();
             if (!ring) return 0;
             FrameMeta probe{};
             probe.width = ring->width();
             probe.height = ring->height();
             return encode_video_frame(probe, ring->slot_bytes(), device_id).first.size() +
                    ring->slot_bytes() + video_frame_suffix_max(device_id);
           },
           py::arg("idx"), py::arg("device_id") = "")
      .def("video_frame_into",
           // The serialized VideoFrame written into caller memory at `addr` (e.g. a shared-memory
           // segment the front-end process maps): (seq, length, meta), None if no newer frame, or
           // the needed size (int) if `cap` is too small. pinned: the range is register_host()ed,
           // so the pixels arrive by one DMA with no staging copy.
           [](Worker& w, int i, i64 after, const std::string& device_id, uintptr_t addr, size_t cap,
              bool pinned) -> py::object {
             std::shared_ptr<Camera> cp = cam_ref(w, i);
             std::shared_ptr<FrameRing> ring = cp->ring();
             if (!ring) return py::none();
             const size_t n = ring->slot_bytes();
             FrameMeta probe;
             int slot;
             if (!ring->latest(after, &probe, &slot)) return py::none();
             const std::string pre = encode_video_frame(probe, n, device_id).first;
             const size_t need = pre.size() + n + video_frame_suffix_max(device_id);
             if (cap < need) return py::int_(need);
             char* buf = reinterpret_cast<char*>(addr);
             std::memcpy(buf, pre.data(), pre.size());
             FrameMeta m;
             bool ok;
             {
               py::gil_scoped_release r;
               ok = w.read_latest(*ring, after, &m, reinterpret_cast<u8*>(buf) + pre.size(), n, pinned);
             }
             if (!ok) return py::none();
             auto [pre2, suf] = encode_video_frame(m, n, device_id);
             VEP_CHECK(pre2 == pre && suf.size() <= video_frame_suffix_max(device_id),
                       "VideoFrame header changed while serving");
             std::memcpy(buf + pre.size() + n, suf.data(), suf.size());
             return py::make_tuple(m.seq, pre.size() + n + suf.size(), meta_dict(m));
           },
           py::arg("idx"), py::arg("after"), py::arg("device_id"), py::arg("addr"), py::arg("cap"),
           py::arg("pinned") = false)
      .def("register_host",
           [](Worker& w, uintptr_t addr, size_t n) { return w.register_host(reinterpret_cast<void*>(addr), n); })
      .def("unregister_host", [](Worker& w, uintptr_t addr) { w.unregister_host(reinterpret_cast<void*>(addr)); })
      .def("video_frame",
           // Serialized VideoFrame proto, built in place in its final bytes object: header, the
           // slot's pixels (D2H through a pinned pool buffer, GIL released), trailer; the object
           // is then shrunk to the exact length (no second copy of the frame).
           [](Worker& w, int i, i64 after, const std::string& device_id) -> py::object {
             Camera& c = cam_of(w, i);
             std::shared_ptr<FrameRing> ring = c.ring();
             if (!ring) return py::none();
             const size_t n = ring->slot_bytes();
             FrameMeta probe;
             int slot;
             if (!ring->latest(after, &probe, &slot)) return py::none();
             // the prefix holds width, height and the data length: fixed for this ring
             const std::string pre = encode_video_frame(probe, n, device_id).first;
             const size_t suf_max = video_frame_suffix_max(device_id);
             PyObject* b = PyBytes_FromStringAndSize(nullptr, Py_ssize_t(pre.size() + n + suf_max));
             if (!b) throw py::error_already_set();
             char* buf = PyBytes_AS_STRING(b);
             std::memcpy(buf, pre.data(), pre.size());
             FrameMeta m;
             bool ok;
             {
               py::gil_scoped_release r;
               try {
                 ok = w.read_latest(*ring, after, &m, reinterpret_cast<u8*>(buf) + pre.size(), n);
               } catch (...) {
                 py::gil_scoped_acquire a;
                 Py_DECREF(b);
                 throw;
               }
             }
             if (!ok) {
               Py_DECREF(b);
               return py::none();
             }
             auto [pre2, suf] = encode_video_frame(m, n, device_id);
             VEP_CHECK(pre2 == pre && suf.size() <= suf_max, "VideoFrame header changed while serving");
             std::memcpy(buf + pre.size() + n, suf.data(), suf.size());
             if (_PyBytes_Resize(&b, Py_ssize_t(pre.size() + n + suf.size())) != 0) throw py::error_already_set();
             py::object res = py::reinterpret_steal<py::object>(b);
             return py::make_tuple(m.seq, res, meta_dict(m));
           },
           py::arg("idx"), py::arg("after") = 0, py::arg("device_id") = "")
      .def("set_consumer_buffers",
           [](Worker& w, uintptr_t hwc, uintptr_t chw, int rows) {
             w.set_consumer_buffers(reinterpret_cast<u8*>(hwc), reinterpret_cast<void*>(chw), rows);
           })
      .def("snapshot_consumer",
           // Consistent copy of consumer rows [0, rows) into dst (device pointer on a GPU worker),
           // enqueued on `stream` (a hipStream_t as int, e.g. torch.cuda.current_stream().cuda_stream;
           // 0 = wait on the host): after every letterbox write already enqueued, before any later.
           [](Worker& w, uintptr_t dst, size_t cap, int rows, uintptr_t stream) {
             py::gil_scoped_release nogil;
             return w.snapshot_consumer(reinterpret_cast<void*>(dst), cap, rows, reinterpret_cast<hipStream_t>(stream));
           },
           py::arg("dst"), py::arg("cap"), py::arg("rows"), py::arg("stream") = 0)
      .def_property_readonly("snapshots", &Worker::snapshots)
      .def("wait_frame",
           // Block (GIL released) until the camera publishes a frame with seq > after.
           [](Worker& w, int i, i64 after, int timeout_ms) {
             std::shared_ptr<Camera> cp = cam_ref(w, i);
             Camera& c = *cp;
             py::gil_scoped_release r;
             const i64 deadline = mono_us() + i64(timeout_ms) * 1000;
             std::shared_ptr<FrameRing> ring;
             while (!(ring = c.ring())) {  // ring appears with the first decoded frame
               if (mono_us() >= deadline) return false;
               std::this_thread::sleep_for(std::chrono::milliseconds(2));
             }
             int left = int(std::max<i64>(0, (deadline - mono_us()) / 1000));
             return ring->wait_newer(after, left);
           },
           py::arg("idx"), py::arg("after"), py::arg("timeout_ms"))
      .def("published", [](Worker& w, int i) {
        auto ring = cam_of(w, i).ring();
        return ring ? ring->published() : i64(0);
      })
      .def("consumer_hwc_ptr", [](Worker& w) { return reinterpret_cast<uintptr_t>(w.consumer_hwc()); })
      .def("consumer_chw_ptr", [](Worker& w) { return reinterpret_cast<uintptr_t>(w.consumer_chw()); })
      .def("ring_slot_ptr", [](Worker& w, int i, int s) {
        auto ring = cam_of(w, i).ring();
        if (!ring) return uintptr_t(0);
        return reinterpret_cast<uintptr_t>(ring->slot_ptr(s));
      })
      .def("latest_slot", [](Worker& w, int i) -> py::object {
        auto ring = cam_of(w, i).ring();
        FrameMeta m;
        int slot;
        if (!ring || !ring->latest(0, &m, &slot)) return py::none();
        return py::make_tuple(slot, meta_dict(m));
      })
      .def("timings",
           [](Worker& w) {
             py::dict d;
             d["prepare_ms"] = w.timers.prepare / 1000.0;
             d["index_ms"] = w.timers.index / 1000.0;
             d["copy_ms"] = w.timers.copy / 1000.0;
             d["enqueue_ms"] = w.timers.enqueue / 1000.0;
             d["wait_ms"] = w.timers.wait / 1000.0;
             return d;
           })
      .def_property_readonly("batches", &Worker::batches)
      .def_property_readonly("frames", &Worker::frames)
      .def_property_readonly("dropped", &Worker::dropped)
      .def_property_readonly("shed", &Worker::shed)
      .def_property_readonly("merged", &Worker::merged)
      .def("hold_lanes", &Worker::hold_lanes, py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("pictures", &Worker::pictures)
      .def_property_readonly("gpu_ms_total", &Worker::gpu_ms_total)
      .def_property_readonly("bytes_inplace", &Worker::bytes_inplace)
      .def_property_readonly("records_gathered", &Worker::records_gathered)
      .def_property_readonly("direct_reads", &Worker::direct_reads)
      .def_property_readonly("bytes_staged", &Worker::bytes_staged)
      .def("compute_stream_ptr", [](Worker& w) { return reinterpret_cast<uintptr_t>(w.compute_stream()); });

  py::class_<ReplayBench>(m, "ReplayBench")
      .def(py::init([](Worker& w, int ncams, const SynthConfig& cfg, int cached, int threads,
                       int ring_slots, const std::string& prefix, int window, bool records) {
             py::gil_scoped_release r;
             return std::make_unique<ReplayBench>(w, ncams, cfg, cached, threads, ring_slots, prefix,
                                                  window, records);
           }),
           py::arg("worker"), py::arg("ncams"), py::arg("cfg"), py::arg("cached_frames") = 30,
           py::arg("threads") = 8, py::arg("ring_slots") = 2, py::arg("prefix") = "cam",
           py::arg("window") = 2, py::arg("records") = false, py::keep_alive<1, 2>())
      .def("step", &ReplayBench::step, py::call_guard<py::gil_scoped_release>())
      .def("parse_only_ms", &ReplayBench::parse_only_ms, py::call_guard<py::gil_scoped_release>())
      .def("drain", &ReplayBench::drain, py::call_guard<py::gil_scoped_release>())
      .def("quiesce", &ReplayBench::quiesce, py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("parse_failures", &ReplayBench::parse_failures)
      .def_property_readonly("frames", &ReplayBench::frames)
      .def_property_readonly("payload_bytes", &ReplayBench::bitstream_bytes)
      .def_property_readonly("stream_bytes", &ReplayBench::stream_bytes)
      .def_property_readonly("stream_frames", &ReplayBench::stream_frames)
      .def_property_readonly("parse_ms", &ReplayBench::parse_ms)
      .def_property_readonly("parse_wait_ms", &ReplayBench::parse_wait_ms)
      .def_property_readonly("batch_ms", &ReplayBench::batch_ms)
      .def_property_readonly("cameras", &ReplayBench::cameras);

  // CPU reference of the colour conversion (coded NV12 planes -> cropped BGR24).
  m.def("nv12_to_bgr_cpu", [](py::array_t<uint8_t, py::array::c_style> y, py::array_t<uint8_t, py::array::c_style> uv,
                              int crop_left, int crop_top, int width, int height) {
    VEP_CHECK(y.ndim() == 2 && uv.ndim() == 2 && uv.shape(0) * 2 == y.shape(0) && uv.shape(1) == y.shape(1),
              "nv12_to_bgr_cpu: Y (H, W) and UV (H / 2, W) planes expected");
    VEP_CHECK(crop_left + width <= y.shape(1) && crop_top + height <= y.shape(0), "crop window outside the planes");
    HostSurface s;
    s.coded_w = int(y.shape(1));
    s.coded_h = int(y.shape(0));
    s.y.assign(y.data(), y.data() + y.size());
    s.uv.assign(uv.data(), uv.data() + uv.size());
    py::array_t<uint8_t> o({height, width, 3});
    cpu_nv12_to_bgr(s, crop_left, crop_top, width, height, o.mutable_data());
    return o;
  });

  // Baseline JPEG (vep/jpeg.h) of a packed BGR24 picture on the host: the CPU backend's encoder
  // and the byte-exact reference of jpeg_encode.
  m.def("jpeg_encode_cpu",
        [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> bgr, int quality) {
          VEP_CHECK(bgr.ndim() == 3 && bgr.shape(2) == 3 && bgr.shape(0) >= 1 && bgr.shape(1) >= 1,
                    "jpeg_encode_cpu: (H, W, 3) uint8 picture expected");
          const u8* p = bgr.data();
          const int w = int(bgr.shape(1)), h = int(bgr.shape(0));
          VEP_CHECK(bgr.shape(1) <= 65535 && bgr.shape(0) <= 65535, "jpeg: picture size out of range");
          std::string out;
          {
            py::gil_scoped_release r;
            out = jpeg::encode_cpu(p, w, h, quality);
          }
          return py::bytes(out);
        },
        py::arg("bgr"), py::arg("quality") = 85);

  // Area-average downscale and wall composition (vep/scale.h) on the host: the CPU backend's
  // path and the byte-exact reference of resize_area / compose_wall.
  m.def("fit_geometry",
        [](int sw, int sh, int bw, int bh) {
          VEP_CHECK(sw >= 1 && sh >= 1 && sw <= 65535 && sh <= 65535, "fit_geometry: source size must be 1..65535");
          VEP_CHECK(bw >= 0 && bh >= 0 && bw <= 65535 && bh <= 65535, "fit_geometry: box sides must be 0..65535");
          const scale::Size f = scale::fit(sw, sh, bw, bh);
          return py::make_tuple(f.w, f.h);
        },
        py::arg("src_w"), py::arg("src_h"), py::arg("box_w") = 0, py::arg("box_h") = 0);
  m.def("wall_geometry",
        // (cols, rows, canvas_w, canvas_h) of n tiles
        [](int n, int cols, int tw, int th) {
          VEP_CHECK(n >= 1 && cols >= 0 && tw >= 1 && th >= 1, "wall_geometry: n, tile sides >= 1 and cols >= 0 expected");
          const scale::Wall g = scale::wall(n, cols, tw, th);
          return py::make_tuple(g.cols, g.rows, g.w, g.h);
        },
        py::arg("n"), py::arg("cols") = 0, py::arg("tile_width") = 320, py::arg("tile_height") = 180);
  m.def("resize_area_cpu",
        [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> bgr, int w, int h) {
          VEP_CHECK(bgr.ndim() == 3 && bgr.shape(2) == 3 && bgr.shape(0) >= 1 && bgr.shape(1) >= 1 &&
                        bgr.shape(0) <= 65535 && bgr.shape(1) <= 65535,
                    "resize_area_cpu: (H, W, 3) uint8 picture of at most 65535 x 65535 expected");
          const int sw = int(bgr.shape(1)), sh = int(bgr.shape(0));
          VEP_CHECK(w >= 1 && h >= 1 && w <= sw && h <= sh, "resize_area_cpu: output must be 1..source size");
          py::array_t<uint8_t> o({h, w, 3});
          const u8* p = bgr.data();
          u8* q = o.mutable_data();
          {
            py::gil_scoped_release r;
            scale::area_cpu(p, sw, sh, size_t(sw) * 3, q, size_t(w) * 3, w, h);
          }
          return o;
        },
        py::arg("bgr"), py::arg("width"), py::arg("height"));
  m.def("compose_wall_cpu",
        [](py::list frames, int cols, int tw, int th) {
          const int n = int(frames.size());
          VEP_CHECK(n >= 1, "compose_wall_cpu: at least one tile expected");
          VEP_CHECK(tw >= 1 && th >= 1 && tw <= 65535 && th <= 65535 && cols >= 0 && cols <= 65535,
                    "compose_wall_cpu: tile sides must be 1..65535, cols 0..65535");
          std::vector<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>> keep;
          keep.reserve(size_t(n));
          std::vector<scale::Tile> tiles((size_t(n)));
          for (int t = 0; t < n; ++t) {
            if (frames[size_t(t)].is_none()) continue;
            keep.push_back(frames[size_t(t)].cast<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>>());
            const auto& a = keep.back();
            VEP_CHECK(a.ndim() == 3 && a.shape(2) == 3 && a.shape(0) >= 1 && a.shape(1) >= 1 && a.shape(0) <= 65535 &&
                          a.shape(1) <= 65535,
                      "compose_wall_cpu: every tile is None or an (H, W, 3) uint8 picture");
            tiles[size_t(t)].src = a.data();
            tiles[size_t(t)].sw = int(a.shape(1));
            tiles[size_t(t)].sh = int(a.shape(0));
            tiles[size_t(t)].pitch = size_t(a.shape(1)) * 3;
          }
          const scale::Wall g = scale::wall(n, cols, tw, th);
          VEP_CHECK(i64(g.cols) * tw <= 65535 && i64(g.rows) * th <= 65535, "wall: canvas sides must be <= 65535");
          py::array_t<uint8_t> o({g.h, g.w, 3});
          u8* q = o.mutable_data();
          {
            py::gil_scoped_release r;
            scale::compose_cpu(tiles.data(), n, g.cols, tw, th, q, size_t(g.w) * 3);
          }
          return o;
        },
        py::arg("frames"), py::arg("cols") = 0, py::arg("tile_width") = 320, py::arg("tile_height") = 180);

  // ---- op API on caller-owned device buffers (torch tensors pass data_ptr / stream) ----
  // Tiles (src pointer or 0, width, height) -> a caller-owned canvas of wall_geometry(n, cols,
  // tile_width, tile_height), one launch of the gfx950 scale kernel on `stream` of the current
  // device (descriptors: one process-wide pool per device). cols < 0: no wall, the single tile is
  // resampled to tile_width x tile_height exactly (resize_area).
  m.def("compose_wall",
        [](const std::vector<std::tuple<uintptr_t, int, int>>& tiles, int cols, int tw, int th, uintptr_t canvas,
           uintptr_t stream) {
          const int n = int(tiles.size());
          VEP_CHECK(n >= 1 && n <= 65535, "compose_wall: 1..65535 tiles expected");
          VEP_CHECK(tw >= 1 && th >= 1 && tw <= 65535 && th <= 65535 && cols <= 65535,
                    "compose_wall: tile sides must be 1..65535");
          VEP_CHECK(cols >= 0 || n == 1, "resize_area: one picture expected");
          py::gil_scoped_release r;
          gpu::ScalePool& pool = pool_of_current_device<gpu::ScalePool>();
          const scale::Wall g = cols < 0 ? scale::Wall{1, 1, tw, th} : scale::wall(n, cols, tw, th);
          VEP_CHECK(i64(g.cols) * tw <= 65535 && i64(g.rows) * th <= 65535, "wall: canvas sides must be <= 65535");
          hipStream_t s = reinterpret_cast<hipStream_t>(stream);
          const int cells = g.cols * g.rows;  // (the cells past the last tile are background too)
          gpu::ScalePool::Lease set = pool.acquire();
          set->reserve(0, cells, 0);
          for (int t = 0; t < cells; ++t) {
            gpu::ScaleDesc d{};
            d.dst = reinterpret_cast<u8*>(canvas);
            d.dst_pitch = u32(g.w) * 3;
            d.src = t < n ? reinterpret_cast<const u8*>(std::get<0>(tiles[size_t(t)])) : nullptr;
            if (cols >= 0) {
              d.cx = (t % g.cols) * tw;
              d.cy = (t / g.cols) * th;
              d.cw = tw;
              d.ch = th;
            }
            if (d.src) {
              d.sw = std::get<1>(tiles[size_t(t)]);
              d.sh = std::get<2>(tiles[size_t(t)]);
              VEP_CHECK(d.sw >= 1 && d.sh >= 1 && d.sw <= 65535 && d.sh <= 65535, "scale: source size out of range");
              d.src_pitch = u32(d.sw) * 3;
              if (cols >= 0) {
                const scale::Placement p = scale::place(t, g.cols, tw, th, d.sw, d.sh);
                d.dx = p.x;
                d.dy = p.y;
                d.ow = p.w;
                d.oh = p.h;
              } else {
                d.ow = tw;
                d.oh = th;
              }
            }
            gpu::check_scale(d, g.w, g.h);
            set->h_descs.p[t] = d;
          }
          set->run(cells, s);
          VEP_HIP(hipEventSynchronize(set->ev));  // the descriptors are reused by the next call
        },
        py::arg("tiles"), py::arg("cols"), py::arg("tile_width"), py::arg("tile_height"), py::arg("canvas"),
        py::arg("stream"));
  // Motion detection (vep/motion.h) on the host: the CPU backend's path and the byte-exact
  // reference of motion_update.
  m.def("motion_grid",
        // (cols, rows) of the cell grid
        [](int w, int h, int cell) {
          VEP_CHECK(w >= 1 && h >= 1 && w <= 65535 && h <= 65535, "motion_grid: picture size must be 1..65535");
          VEP_CHECK(cell >= motion::kMinCell && cell <= motion::kMaxCell, "motion: cell must be 4..256");
          return py::make_tuple(motion::cells(u32(w), u32(cell)), motion::cells(u32(h), u32(cell)));
        },
        py::arg("width"), py::arg("height"), py::arg("cell") = 16);
  m.def("motion_pitch", [](int w) { return motion::pitch_for(u32(w)); }, py::arg("width"));
  m.def("motion_update_cpu",
        // (counts uint32 (rows, cols), background uint16 (H, W)); background None: prime
        [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> bgr, py::object background, int cell,
           int threshold, int learn_shift) {
          VEP_CHECK(bgr.ndim() == 3 && bgr.shape(2) == 3 && bgr.shape(0) >= 1 && bgr.shape(1) >= 1 &&
                        bgr.shape(0) <= 65535 && bgr.shape(1) <= 65535,
                    "motion_update_cpu: (H, W, 3) uint8 picture of at most 65535 x 65535 expected");
          motion::check_update_params(cell, threshold, learn_shift);
          const int w = int(bgr.shape(1)), h = int(bgr.shape(0));
          py::array_t<uint16_t, py::array::c_style | py::array::forcecast> bg;
          const uint16_t* in = nullptr;
          if (!background.is_none()) {
            VEP_CHECK(py::isinstance<py::array>(background) && py::array(background).dtype().is(py::dtype::of<uint16_t>()),
                      "motion_update_cpu: the background must be a uint16 array");
            bg = background.cast<py::array_t<uint16_t, py::array::c_style | py::array::forcecast>>();
            VEP_CHECK(bg.ndim() == 2 && bg.shape(0) == h && bg.shape(1) == w,
                      "motion_update_cpu: the background must be (H, W) like the picture");
            in = bg.data();
          }
          const int cols = int(motion::cells(u32(w), u32(cell))), rows = int(motion::cells(u32(h), u32(cell)));
          py::array_t<uint32_t> counts({rows, cols});
          py::array_t<uint16_t> out({h, w});
          const u8* p = bgr.data();
          uint32_t* cp = counts.mutable_data();
          uint16_t* op = out.mutable_data();
          {
            py::gil_scoped_release r;
            motion::update_cpu(p, w, h, size_t(w) * 3, in, op, size_t(w), cell, threshold, learn_shift, cp);
          }
          return py::make_tuple(counts, out);
        },
        py::arg("bgr"), py::arg("background") = py::none(), py::arg("cell") = 16, py::arg("threshold") = 24,
        py::arg("learn_shift") = 4);
  m.def("motion_summarize",
        // {changed, active, box, motion} of a counts grid
        [](py::array_t<uint32_t, py::array::c_style | py::array::forcecast> counts, int w, int h, int cell,
           int cell_percent, int min_cells) {
          VEP_CHECK(w >= 1 && h >= 1 && w <= 65535 && h <= 65535, "motion_summarize: picture size must be 1..65535");
          VEP_CHECK(cell >= motion::kMinCell && cell <= motion::kMaxCell, "motion: cell must be 4..256");
          VEP_CHECK(counts.ndim() == 2 && counts.shape(0) == py::ssize_t(motion::cells(u32(h), u32(cell))) &&
                        counts.shape(1) == py::ssize_t(motion::cells(u32(w), u32(cell))),
                    "motion_summarize: counts must be the (rows, cols) grid of the picture");
          return summary_dict(motion::summarize(counts.data(), w, h, cell, cell_percent, min_cells));
        },
        py::arg("counts"), py::arg("width"), py::arg("height"), py::arg("cell") = 16, py::arg("cell_percent") = 25,
        py::arg("min_cells") = 1);
  // Pictures (src, w, h, bg_in or 0, bg_out, bg_pitch in samples, counts) on caller-owned device
  // buffers: one launch of the gfx950 motion kernel on `stream` of the current device
  // (descriptors: one process-wide pool per device). src is h x w x 3 packed, the planes h rows of
  // bg_pitch u16, counts the (rows, cols) uint32 grid.
  m.def("motion_update",
        [](const std::vector<std::tuple<uintptr_t, int, int, uintptr_t, uintptr_t, int, uintptr_t>>& pics, int cell,
           int threshold, int learn_shift, uintptr_t stream) {
          const int n = int(pics.size());
          VEP_CHECK(n >= 1 && n <= 65535, "motion_update: 1..65535 pictures expected");
          motion::check_update_params(cell, threshold, learn_shift);
          py::gil_scoped_release r;
          hipStream_t s = reinterpret_cast<hipStream_t>(stream);
          gpu::MotionPool::Lease set = pool_of_current_device<gpu::MotionPool>().acquire();
          set->reserve(n, 0);
          for (int k = 0; k < n; ++k) {
            const auto& [src, w, h, bg_in, bg_out, bg_pitch, counts] = pics[size_t(k)];
            VEP_CHECK(w >= 1 && h >= 1 && w <= 65535 && h <= 65535, "motion: picture size must be 1..65535");
            VEP_CHECK(bg_pitch >= w && bg_pitch <= 65536, "motion: background pitch out of range");
            set->h_descs.p[k] = gpu::make_motion_desc(
                reinterpret_cast<const u8*>(src), size_t(w) * size_t(h) * 3, w, h, reinterpret_cast<const u16*>(bg_in),
                reinterpret_cast<u16*>(bg_out), u32(bg_pitch), size_t(bg_pitch) * size_t(h),
                reinterpret_cast<u32*>(counts), size_t(motion::cells(u32(w), u32(cell))) * motion::cells(u32(h), u32(cell)),
                cell, threshold, learn_shift);
          }
          set->run(n, 0, s);
          VEP_HIP(hipEventSynchronize(set->ev));  // the descriptors are reused by the next call
        },
        py::arg("pictures"), py::arg("cell"), py::arg("threshold"), py::arg("learn_shift"), py::arg("stream"));
  // Tamper detection (vep/tamper.h) on the host: the CPU backend's path and the byte-exact
  // reference of tamper_stats.
  m.def("tamper_grid",
        // (cols, rows) of the cell grid
        [](int w, int h, int cell) {
          VEP_CHECK(w >= 1 && h >= 1 && w <= 65535 && h <= 65535, "tamper_grid: picture size must be 1..65535");
          tamper::check_cell(cell);
          return py::make_tuple(tamper::cells(u32(w), u32(cell)), tamper::cells(u32(h), u32(cell)));
        },
        py::arg("width"), py::arg("height"), py::arg("cell") = 32);
  m.def("tamper_stats_cpu",
        // (hist uint32 (256,), sum_y uint32 (rows, cols), energy uint32 (rows, cols))
        [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> bgr, int cell) {
          VEP_CHECK(bgr.ndim() == 3 && bgr.shape(2) == 3 && bgr.shape(0) >= 1 && bgr.shape(1) >= 1 &&
                        bgr.shape(0) <= 65535 && bgr.shape(1) <= 65535,
                    "tamper_stats_cpu: (H, W, 3) uint8 picture of at most 65535 x 65535 expected");
          tamper::check_cell(cell);
          const int w = int(bgr.shape(1)), h = int(bgr.shape(0));
          const int cols = int(tamper::cells(u32(w), u32(cell))), rows = int(tamper::cells(u32(h), u32(cell)));
          py::array_t<uint32_t> hist = py::array_t<uint32_t>(py::ssize_t(tamper::kBins));
          py::array_t<uint32_t> sum_y({rows, cols}), energy({rows, cols});
          const u8* p = bgr.data();
          uint32_t* hp = hist.mutable_data();
          uint32_t* sp = sum_y.mutable_data();
          uint32_t* ep = energy.mutable_data();
          {
            py::gil_scoped_release r;
            tamper::stats_cpu(p, w, h, size_t(w) * 3, cell, hp, sp, ep);
          }
          return py::make_tuple(hist, sum_y, energy);
        },
        py::arg("bgr"), py::arg("cell") = 32);
  m.def("tamper_summarize",
        // the flags of one evaluation. params: a dict with any of tamper::Params' fields;
        // reference: None or (width, height, cell, sum_y, energy) of the frame declared normal.
        [](py::array_t<uint32_t, py::array::c_style | py::array::forcecast> hist,
           py::array_t<uint32_t, py::array::c_style | py::array::forcecast> sum_y,
           py::array_t<uint32_t, py::array::c_style | py::array::forcecast> energy, int w, int h, py::dict params,
           py::object reference) {
          VEP_CHECK(w >= 1 && h >= 1 && w <= 65535 && h <= 65535, "tamper_summarize: picture size must be 1..65535");
          const tamper::Params def;
          auto get = [&](const char* key, int dflt) { return params.contains(key) ? params[key].cast<int>() : dflt; };
          for (auto item : params) {
            const std::string k = py::str(item.first);
            VEP_CHECK(k == "cell" || k == "dark_level" || k == "bright_level" || k == "spread_min" ||
                          k == "focus_percent" || k == "shift_level" || k == "shift_percent",
                      "tamper_summarize: unknown parameter");
          }
          const tamper::Params p = tamper_params_of(
              get("cell", def.cell), get("dark_level", def.dark_level), get("bright_level", def.bright_level),
              get("spread_min", def.spread_min), get("focus_percent", def.focus_percent),
              get("shift_level", def.shift_level), get("shift_percent", def.shift_percent));
          const py::ssize_t cols = py::ssize_t(tamper::cells(u32(w), u32(p.cell))),
                            rows = py::ssize_t(tamper::cells(u32(h), u32(p.cell)));
          VEP_CHECK(hist.ndim() == 1 && hist.shape(0) == tamper::kBins, "tamper_summarize: hist must have 256 bins");
          VEP_CHECK(sum_y.ndim() == 2 && sum_y.shape(0) == rows && sum_y.shape(1) == cols && energy.ndim() == 2 &&
                        energy.shape(0) == rows && energy.shape(1) == cols,
                    "tamper_summarize: sum_y and energy must be the (rows, cols) grid of the picture");
          tamper::Reference ref;
          bool have_ref = false;
          if (!reference.is_none()) {
            py::tuple t = reference.cast<py::tuple>();
            VEP_CHECK(t.size() == 5, "tamper_summarize: reference must be (width, height, cell, sum_y, energy)");
            ref.w = t[0].cast<int>();
            ref.h = t[1].cast<int>();
            ref.cell = t[2].cast<int>();
            auto rs = t[3].cast<py::array_t<uint32_t, py::array::c_style | py::array::forcecast>>();
            auto re = t[4].cast<py::array_t<uint32_t, py::array::c_style | py::array::forcecast>>();
            VEP_CHECK(rs.size() == re.size(), "tamper_summarize: the reference's planes differ in size");
            ref.sum_y.assign(rs.data(), rs.data() + rs.size());
            for (py::ssize_t i = 0; i < re.size(); ++i) ref.energy_total += re.data()[i];
            have_ref = true;
          }
          return tamper_summary_dict(
              tamper::summarize(hist.data(), sum_y.data(), energy.data(), w, h, p, have_ref ? &ref : nullptr));
        },
        py::arg("hist"), py::arg("sum_y"), py::arg("energy"), py::arg("width"), py::arg("height"),
        py::arg("params") = py::dict(), py::arg("reference") = py::none());
  // Privacy masks (vep/mask.h) on the host: the CPU backend's path and the byte-exact reference
  // of privacy_mask.
  m.def("mask_pixels",
        // (x0, y0, x1, y1) in pixels of a mask of a w x h picture, rounded outward
        [](int w, int h, const MaskTuple& mk) {
          if (w < 1 || h < 1 || w > mask::kMaxSide || h > mask::kMaxSide)
            throw py::value_error("mask_pixels: picture size must be 1..65535");
          const std::vector<mask::Mask> ms = masks_of({mk});
          const mask::Rect r = mask::to_pixels(w, h, ms[0]);
          return py::make_tuple(r.x0, r.y0, r.x1, r.y1);
        },
        py::arg("width"), py::arg("height"), py::arg("mask"));
  m.def("mask_levels",
        [](int w, int h, const std::vector<MaskTuple>& mks) {
          if (w < 1 || h < 1 || w > mask::kMaxSide || h > mask::kMaxSide)
            throw py::value_error("mask_levels: picture size must be 1..65535");
          const std::vector<mask::Mask> ms = masks_of(mks);
          std::vector<int> lv(ms.size());
          mask::levels(w, h, ms.data(), int(ms.size()), lv.data());
          return lv;
        },
        py::arg("width"), py::arg("height"), py::arg("masks"));
  m.def("mask_apply_cpu",
        // the list applied in order, in place, to a writable C-contiguous (H, W, 3) uint8 array
        [](py::array_t<uint8_t, py::array::c_style> bgr, const std::vector<MaskTuple>& mks) {
          if (bgr.ndim() != 3 || bgr.shape(2) != 3 || bgr.shape(0) < 1 || bgr.shape(1) < 1 ||
              bgr.shape(0) > mask::kMaxSide || bgr.shape(1) > mask::kMaxSide || !bgr.writeable())
            throw py::value_error("mask_apply_cpu: writable (H, W, 3) uint8 picture of at most 65535 x 65535 expected");
          const std::vector<mask::Mask> ms = masks_of(mks);
          const int h = int(bgr.shape(0)), w = int(bgr.shape(1));
          u8* p = bgr.mutable_data();
          py::gil_scoped_release r;
          mask::apply_cpu(p, size_t(w) * 3, w, h, ms.data(), int(ms.size()));
        },
        py::arg("bgr").noconvert(), py::arg("masks"));
  // Pictures (dst, w, h, masks) on caller-owned device buffers, masked in place: one launch of the
  // gfx950 mask kernel per level, over all pictures, on `stream` of the current device
  // (descriptors: one process-wide pool per device). dst is h x w x 3 packed.
  m.def("mask_apply",
        [](const std::vector<std::tuple<uintptr_t, int, int, std::vector<MaskTuple>>>& pics, uintptr_t stream) {
          std::vector<std::vector<mask::Mask>> lists;
          size_t nd = 0;
          for (const auto& pc : pics) {
            lists.push_back(masks_of(std::get<3>(pc)));
            nd += lists.back().size();
          }
          if (nd == 0) return;
          VEP_CHECK(nd <= 65535, "mask_apply: at most 65535 masks per call");
          py::gil_scoped_release r;
          hipStream_t s = reinterpret_cast<hipStream_t>(stream);
          gpu::MaskPool::Lease set = pool_of_current_device<gpu::MaskPool>().acquire();
          set->reserve(int(nd));
          int k = 0;
          for (size_t i = 0; i < pics.size(); ++i) {
            const uintptr_t dst = std::get<0>(pics[i]);
            const int w = std::get<1>(pics[i]), h = std::get<2>(pics[i]);
            const std::vector<mask::Mask>& ms = lists[i];
            if (ms.empty()) continue;
            VEP_CHECK(w >= 1 && h >= 1 && w <= mask::kMaxSide && h <= mask::kMaxSide,
                      "mask: picture size must be 1..65535");
            gpu::fill_mask_descs(set->h_descs.p + k, reinterpret_cast<u8*>(dst), size_t(w) * size_t(h) * 3, w, h, ms.data(),
                                 int(ms.size()));
            k += int(ms.size());
          }
          set->run(k, s);
          VEP_HIP(hipEventSynchronize(set->ev));  // the descriptors are reused by the next call
        },
        py::arg("pictures"), py::arg("stream"));
  // Crops (vep/crop.h) on the host: the arithmetic itself, and the CPU backend's path, the
  // byte-exact reference of crop_resize.
  m.def("crop_taps",
        // (D, [(j, i, w), ...]): the taps of every output index of an axis of s source samples and
        // o outputs, over the denominator D
        [](int s, int o) {
          if (s < 1 || s > crop::kMaxSide || o < 1 || o > crop::kMaxOut)
            throw py::value_error("crop_taps: source extent must be 1..65535, output extent 1..4096");
          py::list taps;
          for (int j = 0; j < o; ++j) {
            const crop::Taps t = crop::taps(u32(j), u32(s), u32(o));
            for (u32 i = t.lo; i <= t.hi; ++i) taps.append(py::make_tuple(j, i, crop::weight_of(t, i)));
          }
          return py::make_tuple(crop::den(u32(s), u32(o)), taps);
        },
        py::arg("s"), py::arg("o"));
  m.def("crop_fit",
        // (x, y, w, h): where a letterboxed rect of sw x sh lies in a width x height output
        [](int sw, int sh, int width, int height) {
          if (sw < 1 || sh < 1 || sw > crop::kMaxSide || sh > crop::kMaxSide)
            throw py::value_error("crop_fit: rect size must be 1..65535");
          crop_output_of(width, height, crop::kLetterbox, PadTuple(0, 0, 0));
          const crop::Placement p = crop::fitted(sw, sh, width, height, crop::kLetterbox);
          return py::make_tuple(p.x, p.y, p.w, p.h);
        },
        py::arg("sw"), py::arg("sh"), py::arg("width"), py::arg("height"));
  m.def("crop_pixels",
        // (x0, y0, x1, y1) in pixels of a box of a w x h picture, rounded outward
        [](int w, int h, const BoxTuple& box) {
          if (w < 1 || h < 1 || w > crop::kMaxSide || h > crop::kMaxSide)
            throw py::value_error("crop_pixels: picture size must be 1..65535");
          const std::vector<crop::Box> bs = boxes_of({box});
          const mask::Rect r = crop::to_pixels(w, h, bs[0]);
          return py::make_tuple(r.x0, r.y0, r.x1, r.y1);
        },
        py::arg("width"), py::arg("height"), py::arg("box"));
  m.def("crop_resize_cpu",
        // (n, height, width, 3): the boxes of a C-contiguous (H, W, 3) uint8 picture
        [](py::array_t<uint8_t, py::array::c_style> bgr, const std::vector<BoxTuple>& boxes, int width, int height,
           int fit, const PadTuple& pad) {
          if (bgr.ndim() != 3 || bgr.shape(2) != 3 || bgr.shape(0) < 1 || bgr.shape(1) < 1 ||
              bgr.shape(0) > crop::kMaxSide || bgr.shape(1) > crop::kMaxSide)
            throw py::value_error("crop_resize_cpu: (H, W, 3) uint8 picture of at most 65535 x 65535 expected");
          const std::vector<crop::Box> bs = boxes_of(boxes);
          const crop::Pad p = crop_output_of(width, height, fit, pad);
          const int h = int(bgr.shape(0)), w = int(bgr.shape(1));
          py::array_t<uint8_t> o({py::ssize_t(bs.size()), py::ssize_t(height), py::ssize_t(width), py::ssize_t(3)});
          const u8* src = bgr.data();
          u8* q = o.mutable_data();
          {
            py::gil_scoped_release r;
            crop::apply_cpu(src, size_t(w) * 3, w, h, bs.data(), int(bs.size()), q, width, height, fit, p);
          }
          return o;
        },
        py::arg("bgr").noconvert(), py::arg("boxes"), py::arg("width"), py::arg("height"), py::arg("fit") = 0,
        py::arg("pad") = PadTuple(crop::kPad, crop::kPad, crop::kPad));
  // Pictures (src, w, h, boxes) on caller-owned device buffers into the caller-owned output `out`
  // of out_bytes (every crop width x height x 3 packed, one after the other in list order): ONE
  // launch of the gfx950 crop kernel for all boxes of all pictures, on `stream` of the current
  // device (descriptors: one process-wide pool per device). src is h x w x 3 packed.
  m.def("crop_resize",
        [](const std::vector<std::tuple<uintptr_t, int, int, std::vector<BoxTuple>>>& pics, int width, int height,
           int fit, const PadTuple& pad, uintptr_t out, size_t out_bytes, uintptr_t stream) {
          const crop::Pad p = crop_output_of(width, height, fit, pad);
          std::vector<std::vector<crop::Box>> lists;
          size_t nd = 0;
          for (const auto& pc : pics) {
            const int w = std::get<1>(pc), h = std::get<2>(pc);
            if (w < 1 || h < 1 || w > crop::kMaxSide || h > crop::kMaxSide)
              throw py::value_error("crop: picture size must be 1..65535");
            lists.push_back(boxes_of(std::get<3>(pc)));
            nd += lists.back().size();
          }
          if (nd == 0) return;
          const size_t one = size_t(width) * size_t(height) * 3;
          if (nd > 65535) throw py::value_error("crop_resize: at most 65535 boxes per call");
          if (nd * one > out_bytes) throw py::value_error("crop_resize: output smaller than the crops");
          py::gil_scoped_release r;
          hipStream_t s = reinterpret_cast<hipStream_t>(stream);
          gpu::CropPool::Lease set = pool_of_current_device<gpu::CropPool>().acquire();
          set->reserve(int(nd), 0, 0);
          const u32 pw = u32(p.b) | u32(p.g) << 8 | u32(p.r) << 16;
          size_t k = 0;
          for (size_t i = 0; i < pics.size(); ++i) {
            const u8* src = reinterpret_cast<const u8*>(std::get<0>(pics[i]));
            const int w = std::get<1>(pics[i]), h = std::get<2>(pics[i]);
            for (const crop::Box& b : lists[i]) {
              set->h_descs.p[k] = gpu::make_crop_desc(src, size_t(w) * size_t(h) * 3, w, h, crop::to_pixels(w, h, b),
                                                      reinterpret_cast<u8*>(out) + k * one, one, width, height, fit, pw);
              ++k;
            }
          }
          set->run(int(nd), 0, s);
          VEP_HIP(hipEventSynchronize(set->ev));  // the descriptors are reused by the next call
        },
        py::arg("pictures"), py::arg("width"), py::arg("height"), py::arg("fit"), py::arg("pad"), py::arg("out"),
        py::arg("out_bytes"), py::arg("stream"));
  // On-screen display (vep/overlay.h) on the host: the arithmetic itself, and the CPU backend's
  // path, the byte-exact reference of overlay_draw.
  m.def("overlay_font", [] {
    // (95, 8) uint8: the row bytes of the glyphs of 0x20..0x7E, bit 0 the leftmost column
    py::array_t<uint8_t> a({py::ssize_t(overlay::kGlyphs), py::ssize_t(overlay::kGlyphH)});
    for (int i = 0; i < overlay::kFontBytes; ++i) a.mutable_data()[i] = overlay::font_byte(u32(i));
    return a;
  });
  m.def("overlay_blend",
        // blend(d, c, a) elementwise over three uint8 arrays of one shape
        [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> d,
           py::array_t<uint8_t, py::array::c_style | py::array::forcecast> c,
           py::array_t<uint8_t, py::array::c_style | py::array::forcecast> a) {
          if (d.size() != c.size() || d.size() != a.size()) throw py::value_error("overlay_blend: three arrays of one size expected");
          py::array_t<uint8_t> o(std::vector<py::ssize_t>(d.shape(), d.shape() + d.ndim()));
          const uint8_t *pd = d.data(), *pc = c.data(), *pa = a.data();
          uint8_t* po = o.mutable_data();
          for (py::ssize_t i = 0; i < d.size(); ++i) po[i] = uint8_t(overlay::blend(pd[i], pc[i], pa[i]));
          return o;
        },
        py::arg("d"), py::arg("c"), py::arg("a"));
  m.def("overlay_time", [](i64 timestamp) { return overlay::time_text(timestamp); }, py::arg("timestamp"));
  m.def("overlay_check", [](const std::vector<ItemTuple>& items) { items_of(items); }, py::arg("items"));
  m.def("overlay_expand",
        // the primitives of the list on a width x height picture, in order: (0, x0, y0, x1, y1,
        // (b, g, r), a) for a FILL, (1, ox, oy, k, (b, g, r), a, text) for a TEXT
        [](int w, int h, const std::vector<ItemTuple>& items, const std::string& name, py::object meta) {
          const overlay::Expanded e = overlay_expand_of(items_of(items), w, h, name, overlay_meta_of(meta));
          py::list out;
          for (const overlay::Prim& p : e.prims) {
            py::tuple col = py::make_tuple(int(p.bgra & 255u), int((p.bgra >> 8) & 255u), int((p.bgra >> 16) & 255u));
            const int a = int(p.bgra >> 24);
            if (p.k == 0)
              out.append(py::make_tuple(0, int(p.x0), int(p.y0), int(p.x1), int(p.y1), col, a));
            else
              out.append(py::make_tuple(1, int(p.x0), int(p.y0), int(p.k), col, a, py::bytes(e.text.substr(p.off, p.len))));
          }
          return out;
        },
        py::arg("width"), py::arg("height"), py::arg("items"), py::arg("name") = "", py::arg("meta") = py::none());
  m.def("overlay_draw_cpu",
        // src (H, W, 3) uint8 rows of any pitch (strides[0]) drawn into dst of the same shape; the
        // same array for both: in place
        [](py::array_t<uint8_t> src, py::array_t<uint8_t> dst, const std::vector<ItemTuple>& items, const std::string& name,
           py::object meta) {
          auto bad = [](const py::array_t<uint8_t>& a) {
            return a.ndim() != 3 || a.shape(2) != 3 || a.shape(0) < 1 || a.shape(1) < 1 || a.shape(0) > overlay::kMaxSide ||
                   a.shape(1) > overlay::kMaxSide || a.strides(2) != 1 || a.strides(1) != 3 || a.strides(0) < a.shape(1) * 3;
          };
          if (bad(src) || bad(dst) || src.shape(0) != dst.shape(0) || src.shape(1) != dst.shape(1) || !dst.writeable())
            throw py::value_error("overlay_draw_cpu: two (H, W, 3) uint8 pictures of one size, rows packed, expected");
          const int h = int(src.shape(0)), w = int(src.shape(1));
          const overlay::Expanded e = overlay_expand_of(items_of(items), w, h, name, overlay_meta_of(meta));
          const u8* s = src.data();
          u8* d = dst.mutable_data();
          if (s == d && src.strides(0) != dst.strides(0)) throw py::value_error("overlay_draw_cpu: in place needs equal pitches");
          const size_t sp = size_t(src.strides(0)), dp = size_t(dst.strides(0));
          py::gil_scoped_release r;
          overlay::apply_cpu(s, sp, d, dp, w, h, e.prims.data(), int(e.prims.size()),
                             reinterpret_cast<const u8*>(e.text.data()), e.text.size());
        },
        py::arg("src").noconvert(), py::arg("dst").noconvert(), py::arg("items"), py::arg("name") = "",
        py::arg("meta") = py::none());
  // Pictures (src, src_pitch, dst, dst_pitch, w, h, items) on caller-owned device buffers: ONE launch
  // of the gfx950 overlay kernel for all of them, on `stream` of the current device (scratch: one
  // process-wide pool per device). dst == src: in place. Rows are packed BGR24 of any pitch.
  m.def("overlay_draw",
        [](const std::vector<std::tuple<uintptr_t, size_t, uintptr_t, size_t, int, int, std::vector<ItemTuple>>>& pics,
           const std::string& name, py::object meta, uintptr_t stream) {
          const overlay::Meta om = overlay_meta_of(meta);
          if (pics.size() > 65535) throw py::value_error("overlay_draw: at most 65535 pictures per call");
          std::vector<overlay::Expanded> ex;
          size_t nprims = 0, ntext = 0;
          for (const auto& pc : pics) {
            const int w = std::get<4>(pc), h = std::get<5>(pc);
            if (w < 1 || h < 1 || w > overlay::kMaxSide || h > overlay::kMaxSide)
              throw py::value_error("overlay: picture size must be 1..65535");
            const size_t sp = std::get<1>(pc), dp = std::get<3>(pc);
            if (sp < size_t(w) * 3 || dp < size_t(w) * 3 || sp > 0xFFFFFFFFu || dp > 0xFFFFFFFFu)
              throw py::value_error("overlay: pitch shorter than a row");
            ex.push_back(overlay_expand_of(items_of(std::get<6>(pc)), w, h, name, om));
            nprims += ex.back().prims.size();
            ntext += ex.back().text.size();
          }
          if (pics.empty()) return;
          py::gil_scoped_release r;
          hipStream_t s = reinterpret_cast<hipStream_t>(stream);
          gpu::OverlayPool::Lease set = pool_of_current_device<gpu::OverlayPool>().acquire();
          set->reserve(int(pics.size()), nprims, ntext, 0);
          size_t prim_at = 0, text_at = 0;
          for (size_t i = 0; i < pics.size(); ++i) {
            const auto& [src, sp, dst, dp, w, h, items] = pics[i];
            (void)items;
            const size_t row = size_t(w) * 3;
            set->put(int(i), reinterpret_cast<const u8*>(src), size_t(h - 1) * sp + row, u32(sp), reinterpret_cast<u8*>(dst),
                     size_t(h - 1) * dp + row, u32(dp), w, h, ex[i], prim_at, text_at);
          }
          set->run(int(pics.size()), prim_at, text_at, s);
          VEP_HIP(hipEventSynchronize(set->ev));  // the descriptors are reused by the next call
        },
        py::arg("pictures"), py::arg("name"), py::arg("meta"), py::arg("stream"));
  // Pictures (src, w, h, hist, sum_y, energy) on caller-owned device buffers: one launch of the
  // gfx950 tamper kernel on `stream` of the current device (descriptors: one process-wide pool
  // per device). src is h x w x 3 packed, hist 256 u32 (zeroed here, on the stream), the planes
  // the (rows, cols) u32 grids.
  m.def("tamper_stats",
        [](const std::vector<std::tuple<uintptr_t, int, int, uintptr_t, uintptr_t, uintptr_t>>& pics, int cell,
           uintptr_t stream) {
          const int n = int(pics.size());
          VEP_CHECK(n >= 1 && n <= 65535, "tamper_stats: 1..65535 pictures expected");
          tamper::check_cell(cell);
          py::gil_scoped_release r;
          hipStream_t s = reinterpret_cast<hipStream_t>(stream);
          gpu::TamperPool::Lease set = pool_of_current_device<gpu::TamperPool>().acquire();
          set->reserve(n, 0);
          for (int k = 0; k < n; ++k) {
            const auto& [src, w, h, hist, sum_y, energy] = pics[size_t(k)];
            VEP_CHECK(w >= 1 && h >= 1 && w <= 65535 && h <= 65535, "tamper: picture size must be 1..65535");
            set->h_descs.p[k] = gpu::make_tamper_desc(
                reinterpret_cast<const u8*>(src), size_t(w) * size_t(h) * 3, w, h, reinterpret_cast<u32*>(hist),
                reinterpret_cast<u32*>(sum_y), reinterpret_cast<u32*>(energy),
                size_t(tamper::cells(u32(w), u32(cell))) * tamper::cells(u32(h), u32(cell)), cell);
          }
          for (int k = 0; k < n; ++k)
            VEP_HIP(hipMemsetAsync(set->h_descs.p[k].hist, 0, size_t(tamper::kBins) * sizeof(u32), s));
          set->run(n, 0, 0, s);
          VEP_HIP(hipEventSynchronize(set->ev));  // the descriptors are reused by the next call
        },
        py::arg("pictures"), py::arg("cell"), py::arg("stream"));
  // JPEG stream of a device BGR24 picture, encoded by the gfx950 kernels on `stream` of the
  // current device (scratch: one process-wide pool per device).
  m.def("jpeg_encode",
        [](uintptr_t bgr, int w, int h, int quality, uintptr_t stream) {
          std::string out;
          {
            py::gil_scoped_release r;
            const u8* p = reinterpret_cast<const u8*>(bgr);
            if (!pool_of_current_device<gpu::JpegPool>().encode(p, w, h, quality, reinterpret_cast<hipStream_t>(stream), out)) {
              // the kernels reported an overflow of their scratch: encode on the host
              std::unique_ptr<u8[]> host(new u8[size_t(w) * size_t(h) * 3]);
              VEP_HIP(hipMemcpyAsync(host.get(), p, size_t(w) * size_t(h) * 3, hipMemcpyDeviceToHost,
                                     reinterpret_cast<hipStream_t>(stream)));
              VEP_HIP(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
              out = jpeg::encode_cpu(host.get(), w, h, quality);
            }
          }
          return py::bytes(out);
        },
        py::arg("bgr"), py::arg("w"), py::arg("h"), py::arg("quality"), py::arg("stream"));
  m.def("nv12_to_bgr",
        [](uintptr_t y, uintptr_t uv, uintptr_t mask, uintptr_t prefix, uintptr_t offsets,
           uintptr_t payload, int wmbs, int hmbs, int out_w, int out_h, int crop_left,
           int crop_top, uintptr_t out, uintptr_t stream) {
          gpu::DecodeDesc d{};
          d.y = reinterpret_cast<u8*>(y);
          d.uv = reinterpret_cast<u8*>(uv);
          d.mask = reinterpret_cast<const u32*>(mask);
          d.prefix = reinterpret_cast<const u32*>(prefix);
          d.offsets = reinterpret_cast<const u32*>(offsets);
          d.payload = reinterpret_cast<const u8*>(payload);
          d.bgr = reinterpret_cast<u8*>(out);
          d.wmbs = wmbs;
          d.hmbs = hmbs;
          d.out_w = out_w;
          d.out_h = out_h;
          d.crop_left = crop_left;
          d.crop_top = crop_top;
          d.tiles_x = (wmbs + gpu::kTileMbW - 1) / gpu::kTileMbW;
          d.tile_begin = 0;
          gpu::launch_decode_convert_one(d, reinterpret_cast<hipStream_t>(stream));
        });
  // Reconstructed surface (u8 or u16 samples, 4:2:0 or 4:2:2) -> BGR24 (gpu::SurfaceBgrDesc).
  m.def("surface_to_bgr",
        [](uintptr_t y, uintptr_t uv, int pitch, int coded_w, int coded_h, int bit_depth, int chroma_format,
           int crop_left, int crop_top, int out_w, int out_h, uintptr_t out, uintptr_t stream) {
          gpu::SurfaceBgrDesc d{};
          d.y = reinterpret_cast<const u8*>(y);
          d.uv = reinterpret_cast<const u8*>(uv);
          d.bgr = reinterpret_cast<u8*>(out);
          d.pitch = pitch;
          d.coded_w = coded_w;
          d.coded_h = coded_h;
          d.bit_depth = bit_depth;
          d.chroma_format = chroma_format;
          d.crop_left = crop_left;
          d.crop_top = crop_top;
          d.out_w = out_w;
          d.out_h = out_h;
          gpu::check_surface_bgr(d);
          gpu::launch_surface_to_bgr_one(d, reinterpret_cast<hipStream_t>(stream));
        },
        py::arg("y"), py::arg("uv"), py::arg("pitch"), py::arg("coded_w"), py::arg("coded_h"), py::arg("bit_depth"),
        py::arg("chroma_format"), py::arg("crop_left"), py::arg("crop_top"), py::arg("out_w"), py::arg("out_h"),
        py::arg("out"), py::arg("stream"));
  // Several pictures in ONE launch (the worker's per-round launch: descriptor table in device
  // memory, block -> picture by the tile prefix). pics: (y, uv, pitch, coded_w, coded_h, bit_depth,
  // chroma_format, crop_left, crop_top, out_w, out_h, out) each. Waits for the launch.
  m.def("surface_to_bgr_many",
        [](const std::vector<std::tuple<uintptr_t, uintptr_t, int, int, int, int, int, int, int, int, int, uintptr_t>>& pics,
           uintptr_t stream) {
          if (pics.empty()) return 0;
          std::vector<gpu::SurfaceBgrDesc> descs;
          int tiles = 0;
          for (const auto& p : pics) {
            gpu::SurfaceBgrDesc d{};
            d.y = reinterpret_cast<const u8*>(std::get<0>(p));
            d.uv = reinterpret_cast<const u8*>(std::get<1>(p));
            d.pitch = std::get<2>(p);
            d.coded_w = std::get<3>(p);
            d.coded_h = std::get<4>(p);
            d.bit_depth = std::get<5>(p);
            d.chroma_format = std::get<6>(p);
            d.crop_left = std::get<7>(p);
            d.crop_top = std::get<8>(p);
            d.out_w = std::get<9>(p);
            d.out_h = std::get<10>(p);
            d.bgr = reinterpret_cast<u8*>(std::get<11>(p));
            gpu::check_surface_bgr(d);
            d.tile_begin = tiles;
            tiles += gpu::tiles_for(d.coded_w / 16, d.coded_h / 16);
            descs.push_back(d);
          }
          const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
          void* dd = nullptr;
          const size_t bytes = descs.size() * sizeof(gpu::SurfaceBgrDesc);
          VEP_HIP(hipMalloc(&dd, bytes));
          try {
            VEP_HIP(hipMemcpyAsync(dd, descs.data(), bytes, hipMemcpyHostToDevice, s));
            gpu::launch_surface_to_bgr(static_cast<const gpu::SurfaceBgrDesc*>(dd), int(descs.size()), tiles, s);
            VEP_HIP(hipStreamSynchronize(s));
          } catch (...) {
            (void)hipFree(dd);
            throw;
          }
          (void)hipFree(dd);
          return tiles;
        },
        py::arg("pics"), py::arg("stream"));
  m.def("letterbox",
        [](uintptr_t y, uintptr_t uv, int pitch, int src_w, int src_h, int crop_left, int crop_top,
           int size, uintptr_t out_hwc, uintptr_t out_chw, int chw_dtype, std::vector<float> mean,
           std::vector<float> stdv, int pad, uintptr_t stream, int format) {
          gpu::LetterboxDesc d{};
          d.y = reinterpret_cast<const u8*>(y);
          d.uv = reinterpret_cast<const u8*>(uv);
          d.pitch = pitch;
          d.src_w = src_w;
          d.src_h = src_h;
          d.crop_left = crop_left;
          d.crop_top = crop_top;
          d.out_hwc = reinterpret_cast<u8*>(out_hwc);
          d.out_chw = reinterpret_cast<void*>(out_chw);
          gpu::LetterboxParams p{};
          p.format = format;
          p.size = size;
          p.chw_dtype = chw_dtype;
          for (int k = 0; k < 3; ++k) {
            p.mean[k] = mean.size() == 3 ? mean[size_t(k)] : 0.f;
            p.inv_std[k] = 1.f / (stdv.size() == 3 ? stdv[size_t(k)] : 1.f);
          }
          p.pad_value = u8(pad);
          gpu::check_letterbox(d, p);
          gpu::fill_letterbox_geometry(d, size, format == gpu::kLbNV12);
          gpu::launch_letterbox_one(d, p, reinterpret_cast<hipStream_t>(stream));
        },
        py::arg("y"), py::arg("uv"), py::arg("pitch"), py::arg("src_w"), py::arg("src_h"),
        py::arg("crop_left"), py::arg("crop_top"), py::arg("size"), py::arg("out_hwc"),
        py::arg("out_chw"), py::arg("chw_dtype"), py::arg("mean"), py::arg("std"), py::arg("pad"),
        py::arg("stream"), py::arg("format") = 0);
  m.def("nv12_to_chw",
        [](uintptr_t in, uintptr_t out, int n, int size, int chw_dtype, std::vector<float> mean,
           std::vector<float> stdv, uintptr_t stream) {
          float m3[3], is3[3];
          for (int k = 0; k < 3; ++k) {
            m3[k] = mean.size() == 3 ? mean[size_t(k)] : 0.f;
            is3[k] = 1.f / (stdv.size() == 3 ? stdv[size_t(k)] : 1.f);
          }
          gpu::launch_nv12_to_chw(reinterpret_cast<const u8*>(in), reinterpret_cast<void*>(out), n,
                                  size, chw_dtype, m3, is3, reinterpret_cast<hipStream_t>(stream));
        });
  m.def("letterbox_geometry", [](int src_w, int src_h, int size, bool even) {
    gpu::LetterboxDesc d{};
    d.src_w = src_w;
    d.src_h = src_h;
    gpu::fill_letterbox_geometry(d, size, even);
    return py::make_tuple(d.nw, d.nh, d.pad_x, d.pad_y);
  }, py::arg("src_w"), py::arg("src_h"), py::arg("size"), py::arg("even") = false);

  bind_net(m);
  bind_mux(m);
  bind_hevc(m);
  bind_bus(m);
  bind_rpc(m);
  bind_dbk(m);
  bind_hevc_lf(m);
}
