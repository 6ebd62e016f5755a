// Bindings of the free functions on host arrays (the `*_cpu` references and the geometry helpers) and of
// the ops on caller-owned device buffers (torch tensors pass data_ptr / stream), grouped by op.
#include "bind_common.h"
#include "vep/gpu.h"
#include "vep/jpeg.h"
#include "vep/scale.h"

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

// The frame of every such op: with the GIL released, `fill` reserves, fills and runs a scratch set of the
// current device's pool on `stream`, and the call returns once the set's launch is over.
template <class Pool, class Fill>
static void on_pooled_set(uintptr_t stream, Fill&& fill) {
  py::gil_scoped_release r;
  typename Pool::Lease set = pool_of_current_device<Pool>().acquire();
  fill(set, reinterpret_cast<hipStream_t>(stream));
  VEP_HIP(hipEventSynchronize(set->ev));  // the descriptors are reused by the next call
}

// The checked descriptor of one picture of surface_to_bgr / surface_to_bgr_many, in their argument order.
static gpu::SurfaceBgrDesc surface_bgr_desc(uintptr_t y, uintptr_t uv, int pitch, int coded_w, int coded_h, int bit_depth,
                                            int chroma_format, int crop_left, int crop_top, int out_w, int out_h,
                                            uintptr_t out) {
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
  return d;
}

void bind_ops(py::module_& m) {
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

  // Area-average downscale and wall composition (vep/scale.h) on the host: the CPU backend's
  // path and the byte-exact reference of resize_area / compose_wall.
  m.def("fit_geometry",
        [](int sw, int sh, int bw, int bh) {
          VEP_CHECK(picture_size_ok(sw, sh), "fit_geometry: source size must be 1..65535");
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
          VEP_CHECK(is_bgr_picture(bgr), "resize_area_cpu: (H, W, 3) uint8 picture of at most 65535 x 65535 expected");
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
          VEP_CHECK(picture_size_ok(tw, th) && cols >= 0 && cols <= 65535,
                    "compose_wall_cpu: tile sides must be 1..65535, cols 0..65535");
          std::vector<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>> keep;
          keep.reserve(size_t(n));
          std::vector<scale::Tile> tiles((size_t(n)));
          for (int t = 0; t < n; ++t) {
            if (frames[size_t(t)].is_none()) continue;
            keep.push_back(frames[size_t(t)].cast<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>>());
            const auto& a = keep.back();
            VEP_CHECK(is_bgr_picture(a), "compose_wall_cpu: every tile is None or an (H, W, 3) uint8 picture");
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

  // Tiles (src pointer or 0, width, height) -> a caller-owned canvas of wall_geometry(n, cols,
  // tile_width, tile_height), one launch of the gfx950 scale kernel on `stream` of the current
  // device (descriptors: one process-wide pool per device). cols < 0: no wall, the single tile is
  // resampled to tile_width x tile_height exactly (resize_area).
  m.def("compose_wall",
        [](const std::vector<std::tuple<uintptr_t, int, int>>& tiles, int cols, int tw, int th, uintptr_t canvas,
           uintptr_t stream) {
          const int n = int(tiles.size());
          VEP_CHECK(n >= 1 && n <= 65535, "compose_wall: 1..65535 tiles expected");
          VEP_CHECK(picture_size_ok(tw, th) && cols <= 65535, "compose_wall: tile sides must be 1..65535");
          VEP_CHECK(cols >= 0 || n == 1, "resize_area: one picture expected");
          on_pooled_set<gpu::ScalePool>(stream, [&](gpu::ScalePool::Lease& set, hipStream_t s) {
            const scale::Wall g = cols < 0 ? scale::Wall{1, 1, tw, th} : scale::wall(n, cols, tw, th);
            VEP_CHECK(i64(g.cols) * tw <= 65535 && i64(g.rows) * th <= 65535, "wall: canvas sides must be <= 65535");
            const int cells = g.cols * g.rows;  // (the cells past the last tile are background too)
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
                VEP_CHECK(picture_size_ok(d.sw, d.sh), "scale: source size out of range");
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
          });
        },
        py::arg("tiles"), py::arg("cols"), py::arg("tile_width"), py::arg("tile_height"), py::arg("canvas"),
        py::arg("stream"));
  // Motion detection (vep/motion.h) on the host: the CPU backend's path and the byte-exact
  // reference of motion_update.
  m.def("motion_grid",
        // (cols, rows) of the cell grid
        [](int w, int h, int cell) {
          VEP_CHECK(picture_size_ok(w, h), "motion_grid: picture size must be 1..65535");
          VEP_CHECK(cell >= motion::kMinCell && cell <= motion::kMaxCell, "motion: cell must be 4..256");
          return py::make_tuple(motion::cells(u32(w), u32(cell)), motion::cells(u32(h), u32(cell)));
        },
        py::arg("width"), py::arg("height"), py::arg("cell") = 16);
  m.def("motion_pitch", [](int w) { return motion::pitch_for(u32(w)); }, py::arg("width"));
  m.def("motion_update_cpu",
        // (counts uint32 (rows, cols), background uint16 (H, W)); background None: prime
        [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> bgr, py::object background, int cell,
           int threshold, int learn_shift) {
          VEP_CHECK(is_bgr_picture(bgr), "motion_update_cpu: (H, W, 3) uint8 picture of at most 65535 x 65535 expected");
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
          VEP_CHECK(picture_size_ok(w, h), "motion_summarize: picture size must be 1..65535");
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
          on_pooled_set<gpu::MotionPool>(stream, [&](gpu::MotionPool::Lease& set, hipStream_t s) {
            set->reserve(n, 0);
            for (int k = 0; k < n; ++k) {
              const auto& [src, w, h, bg_in, bg_out, bg_pitch, counts] = pics[size_t(k)];
              VEP_CHECK(picture_size_ok(w, h), "motion: picture size must be 1..65535");
              VEP_CHECK(bg_pitch >= w && bg_pitch <= 65536, "motion: background pitch out of range");
              set->h_descs.p[k] = gpu::make_motion_desc(
                  reinterpret_cast<const u8*>(src), size_t(w) * size_t(h) * 3, w, h, reinterpret_cast<const u16*>(bg_in),
                  reinterpret_cast<u16*>(bg_out), u32(bg_pitch), size_t(bg_pitch) * size_t(h), reinterpret_cast<u32*>(counts),
                  size_t(motion::cells(u32(w), u32(cell))) * motion::cells(u32(h), u32(cell)), cell, threshold, learn_shift);
            }
            set->run(n, 0, s);
          });
        },
        py::arg("pictures"), py::arg("cell"), py::arg("threshold"), py::arg("learn_shift"), py::arg("stream"));
  // Tamper detection (vep/tamper.h) on the host: the CPU backend's path and the byte-exact
  // reference of tamper_stats.
  m.def("tamper_grid",
        // (cols, rows) of the cell grid
        [](int w, int h, int cell) {
          VEP_CHECK(picture_size_ok(w, h), "tamper_grid: picture size must be 1..65535");
          tamper::check_cell(cell);
          return py::make_tuple(tamper::cells(u32(w), u32(cell)), tamper::cells(u32(h), u32(cell)));
        },
        py::arg("width"), py::arg("height"), py::arg("cell") = 32);
  m.def("tamper_stats_cpu",
        // (hist uint32 (256,), sum_y uint32 (rows, cols), energy uint32 (rows, cols))
        [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> bgr, int cell) {
          VEP_CHECK(is_bgr_picture(bgr), "tamper_stats_cpu: (H, W, 3) uint8 picture of at most 65535 x 65535 expected");
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
          VEP_CHECK(picture_size_ok(w, h), "tamper_summarize: picture size must be 1..65535");
          const tamper::Params def;
          auto get = [&](const char* key, int dflt) { return params.contains(key) ? params[key].cast<int>() : dflt; };
          const py::dict known = tamper_params_dict(def);
          for (auto item : params) VEP_CHECK(known.contains(item.first), "tamper_summarize: unknown parameter");
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
          on_pooled_set<gpu::TamperPool>(stream, [&](gpu::TamperPool::Lease& set, hipStream_t s) {
            set->reserve(n, 0);
            for (int k = 0; k < n; ++k) {
              const auto& [src, w, h, hist, sum_y, energy] = pics[size_t(k)];
              VEP_CHECK(picture_size_ok(w, h), "tamper: picture size must be 1..65535");
              set->h_descs.p[k] = gpu::make_tamper_desc(
                  reinterpret_cast<const u8*>(src), size_t(w) * size_t(h) * 3, w, h, reinterpret_cast<u32*>(hist),
                  reinterpret_cast<u32*>(sum_y), reinterpret_cast<u32*>(energy),
                  size_t(tamper::cells(u32(w), u32(cell))) * tamper::cells(u32(h), u32(cell)), cell);
            }
            for (int k = 0; k < n; ++k)
              VEP_HIP(hipMemsetAsync(set->h_descs.p[k].hist, 0, size_t(tamper::kBins) * sizeof(u32), s));
            set->run(n, 0, 0, s);
          });
        },
        py::arg("pictures"), py::arg("cell"), py::arg("stream"));
  // Privacy masks (vep/mask.h) on the host: the CPU backend's path and the byte-exact reference
  // of privacy_mask.
  m.def("mask_pixels",
        // (x0, y0, x1, y1) in pixels of a mask of a w x h picture, rounded outward
        [](int w, int h, const MaskTuple& mk) {
          if (!picture_size_ok(w, h)) throw py::value_error("mask_pixels: picture size must be 1..65535");
          const std::vector<mask::Mask> ms = masks_of({mk});
          const mask::Rect r = mask::to_pixels(w, h, ms[0]);
          return py::make_tuple(r.x0, r.y0, r.x1, r.y1);
        },
        py::arg("width"), py::arg("height"), py::arg("mask"));
  m.def("mask_levels",
        [](int w, int h, const std::vector<MaskTuple>& mks) {
          if (!picture_size_ok(w, h)) throw py::value_error("mask_levels: picture size must be 1..65535");
          const std::vector<mask::Mask> ms = masks_of(mks);
          std::vector<int> lv(ms.size());
          mask::levels(w, h, ms.data(), int(ms.size()), lv.data());
          return lv;
        },
        py::arg("width"), py::arg("height"), py::arg("masks"));
  m.def("mask_apply_cpu",
        // the list applied in order, in place, to a writable C-contiguous (H, W, 3) uint8 array
        [](py::array_t<uint8_t, py::array::c_style> bgr, const std::vector<MaskTuple>& mks) {
          if (!is_bgr_picture(bgr) || !bgr.writeable())
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
          on_pooled_set<gpu::MaskPool>(stream, [&](gpu::MaskPool::Lease& set, hipStream_t s) {
            set->reserve(int(nd));
            int k = 0;
            for (size_t i = 0; i < pics.size(); ++i) {
              const uintptr_t dst = std::get<0>(pics[i]);
              const int w = std::get<1>(pics[i]), h = std::get<2>(pics[i]);
              const std::vector<mask::Mask>& ms = lists[i];
              if (ms.empty()) continue;
              VEP_CHECK(picture_size_ok(w, h), "mask: picture size must be 1..65535");
              gpu::fill_mask_descs(set->h_descs.p + k, reinterpret_cast<u8*>(dst), size_t(w) * size_t(h) * 3, w, h,
                                   ms.data(), int(ms.size()));
              k += int(ms.size());
            }
            set->run(k, s);
          });
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
          if (!picture_size_ok(sw, sh)) throw py::value_error("crop_fit: rect size must be 1..65535");
          crop_output_of(width, height, crop::kLetterbox, PadTuple(0, 0, 0));
          const crop::Placement p = crop::fitted(sw, sh, width, height, crop::kLetterbox);
          return py::make_tuple(p.x, p.y, p.w, p.h);
        },
        py::arg("sw"), py::arg("sh"), py::arg("width"), py::arg("height"));
  m.def("crop_pixels",
        // (x0, y0, x1, y1) in pixels of a box of a w x h picture, rounded outward
        [](int w, int h, const BoxTuple& box) {
          if (!picture_size_ok(w, h)) throw py::value_error("crop_pixels: picture size must be 1..65535");
          const std::vector<crop::Box> bs = boxes_of({box});
          const mask::Rect r = crop::to_pixels(w, h, bs[0]);
          return py::make_tuple(r.x0, r.y0, r.x1, r.y1);
        },
        py::arg("width"), py::arg("height"), py::arg("box"));
  m.def("crop_resize_cpu",
        // (n, height, width, 3): the boxes of a C-contiguous (H, W, 3) uint8 picture
        [](py::array_t<uint8_t, py::array::c_style> bgr, const std::vector<BoxTuple>& boxes, int width, int height,
           int fit, const PadTuple& pad) {
          if (!is_bgr_picture(bgr))
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
            if (!picture_size_ok(w, h)) throw py::value_error("crop: picture size must be 1..65535");
            lists.push_back(boxes_of(std::get<3>(pc)));
            nd += lists.back().size();
          }
          if (nd == 0) return;
          const size_t one = size_t(width) * size_t(height) * 3;
          if (nd > 65535) throw py::value_error("crop_resize: at most 65535 boxes per call");
          if (nd * one > out_bytes) throw py::value_error("crop_resize: output smaller than the crops");
          on_pooled_set<gpu::CropPool>(stream, [&](gpu::CropPool::Lease& set, hipStream_t s) {
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
          });
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
            return !is_bgr_picture(a) || a.strides(2) != 1 || a.strides(1) != 3 || a.strides(0) < a.shape(1) * 3;
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
            if (!picture_size_ok(w, h)) throw py::value_error("overlay: picture size must be 1..65535");
            const size_t sp = std::get<1>(pc), dp = std::get<3>(pc);
            if (sp < size_t(w) * 3 || dp < size_t(w) * 3 || sp > 0xFFFFFFFFu || dp > 0xFFFFFFFFu)
              throw py::value_error("overlay: pitch shorter than a row");
            ex.push_back(overlay_expand_of(items_of(std::get<6>(pc)), w, h, name, om));
            nprims += ex.back().prims.size();
            ntext += ex.back().text.size();
          }
          if (pics.empty()) return;
          on_pooled_set<gpu::OverlayPool>(stream, [&](gpu::OverlayPool::Lease& set, hipStream_t s) {
            set->reserve(int(pics.size()), nprims, ntext, 0);
            size_t prim_at = 0, text_at = 0;
            for (size_t i = 0; i < pics.size(); ++i) {
              const auto& [src, sp, dst, dp, w, h, items] = pics[i];
              (void)items;
              const size_t row = size_t(w) * 3;
              set->put(int(i), reinterpret_cast<const u8*>(src), size_t(h - 1) * sp + row, u32(sp),
                       reinterpret_cast<u8*>(dst), size_t(h - 1) * dp + row, u32(dp), w, h, ex[i], prim_at, text_at);
            }
            set->run(int(pics.size()), prim_at, text_at, s);
          });
        },
        py::arg("pictures"), py::arg("name"), py::arg("meta"), py::arg("stream"));
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
          gpu::launch_surface_to_bgr_one(surface_bgr_desc(y, uv, pitch, coded_w, coded_h, bit_depth, chroma_format, crop_left,
                                                          crop_top, out_w, out_h, out), reinterpret_cast<hipStream_t>(stream));
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
            gpu::SurfaceBgrDesc d = std::apply(surface_bgr_desc, p);
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
          fill_mean_std(mean, stdv, p.mean, p.inv_std, true);
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
          fill_mean_std(mean, stdv, m3, is3, true);
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
}
