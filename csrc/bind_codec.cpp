// Bindings of the synthetic encoders and the CPU decoders (tests, tools and the bench's sources).
#include "bind_common.h"
#include "vep/avc.h"
#include "vep/codec.h"
#include "vep/hevc_dec.h"
#include "vep/hevc_kern.h"
#include "vep/synth.h"

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

void bind_codec(py::module_& m) {
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
      .def("picture", [](const avc::AvcHighEncoder& e) { return surface_planes(e.reconstruction()); })
      .def("source", [](const avc::AvcHighEncoder& e) { return surface_planes(e.source()); })
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
      .def("picture", [](const hevc::HevcEncoder& e) { return surface_planes(e.reconstruction()); })
      .def("source", [](const hevc::HevcEncoder& e) { return surface_planes(e.source()); })
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
           [](hevc::Decoder& d, const AccessUnit& au) {
             std::vector<hevc::FramePtr> fs;
             {
               py::gil_scoped_release nogil;
               fs = d.decode(au, 0);
             }
             py::list l;
             for (const auto& f : fs) l.append(py::make_tuple(f->pts, f->poc, std::string(1, f->type), surface_planes(f->s)));
             return l;
           })
      .def("flush",
           [](hevc::Decoder& d) {
             py::list l;
             for (const auto& f : d.flush()) l.append(py::make_tuple(f->pts, f->poc, std::string(1, f->type), surface_planes(f->s)));
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
        const int cw = s.coded_w;
        // the coded picture (the decoder's surfaces are coded_w x coded_h, slots are 16-aligned)
        const int pw = coded_w_, ph = coded_h_;
        auto planes_of = [&](const auto& sy, const auto& suv) -> py::tuple {
          using T = std::decay_t<decltype(sy[0])>;
          py::array_t<T> y({ph, pw}), uv({ph / 2, pw});
          for (int r = 0; r < ph; ++r) std::memcpy(y.mutable_data() + size_t(r) * pw, &sy[size_t(r) * cw], size_t(pw) * sizeof(T));
          for (int r = 0; r < ph / 2; ++r)
            std::memcpy(uv.mutable_data() + size_t(r) * pw, &suv[size_t(r) * cw], size_t(pw) * sizeof(T));
          return py::make_tuple(y, uv);
        };
        const py::tuple planes = s.wide() ? planes_of(s.y16, s.uv16) : planes_of(s.y, s.uv);  // Main10: uint16 planes
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
}
