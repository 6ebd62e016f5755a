// Bindings of the Worker's serving reads (vep/serve.cpp) and what goes with them: latest, scaled, JPEG,
// wall, overlay, motion, tamper, privacy masks, crops, history and the serialized VideoFrames.
#include "bind_common.h"

void bind_worker_serving(py::class_<Worker>& cls) {
  cls
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
                 VEP_CHECK(is_bgr_picture(a), "wall: a foreign tile is an (H, W, 3) uint8 picture");
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
           py::arg("idx"), py::arg("after") = 0, py::arg("device_id") = "");
}
