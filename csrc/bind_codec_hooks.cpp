// Test hooks into the parsers and the codec arithmetic: `_vep.recon` and the round trips, fuzzers and
// statistics the spec-oracle and parser tests call.
#include "bind_common.h"
#include "vep/avc.h"
#include "vep/avc_cavlc.h"
#include "vep/avc_recon.h"
#include "vep/cabac.h"
#include "vep/codec.h"
#include "vep/h264.h"
#include "vep/hevc_ctu.h"
#include "vep/hevc_dec.h"
#include "vep/hevc_kern.h"
#include "vep/synth.h"

// xorshift64 of the hooks that draw their own inputs, seeded from (seed, a salt per hook).
struct XorShift {
  u64 x;
  XorShift(u64 seed, u64 salt) : x(seed * 0x9E3779B97F4A7C15ull + salt) {}
  u64 operator()() { return x ^= x << 13, x ^= x >> 7, x ^= x << 17; }
};

// The RBSP of an escaped NAL unit.
static std::vector<u8> rbsp_of(const std::string& nal) {
  std::vector<u8> r(nal.size());
  r.resize(ebsp_to_rbsp(reinterpret_cast<const u8*>(nal.data()), nal.size(), r.data()));
  return r;
}

void bind_codec_hooks(py::module_& m) {
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
    const std::vector<u8> r = rbsp_of(nal);
    h264::Sps s = h264::parse_sps(r.data(), r.size());
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
    const std::vector<u8> r = rbsp_of(nal);
    hevc::Sps s = hevc::parse_sps(r.data(), r.size());
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
  m.def("parse_hevc_pps", [](const std::string& nal) {
    const std::vector<u8> r = rbsp_of(nal);
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
  m.def("hevc_scaling_factors", [](int size_id, int matrix_id, py::object sps_nal, py::object pps_nal) {
    VEP_CHECK(size_id >= 0 && size_id < 4 && matrix_id >= 0 && matrix_id < 6, "bad sizeId / matrixId");
    hevc::ScalingList sl;
    if (!sps_nal.is_none()) {
      const std::vector<u8> r = rbsp_of(sps_nal.cast<std::string>());
      sl = hevc::parse_sps(r.data(), r.size()).sl;
    }
    if (!pps_nal.is_none()) {
      const std::vector<u8> r = rbsp_of(pps_nal.cast<std::string>());
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
  m.def("hevc_slice_entry_points", [](const std::string& nal, const std::string& sps_nal,
                                               const std::string& pps_nal) {
    const std::vector<u8> rs = rbsp_of(sps_nal), rp = rbsp_of(pps_nal), r = rbsp_of(nal);
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
  // Sparse coefficient records against the dense blocks they encode: random blocks (any density,
  // int16 extremes, 4x4 and 8x8 transforms, any coded pattern) through store_mb -> expand_coefs
  // (H.264, avc_recon.h) and through hk_sparse_store -> hk_sparse_expand for every H.265 TB size
  // (hevc_kern.h). Returns (H.264 mismatches, H.265 mismatches).
  m.def("sparse_coef_fuzz", [](u64 seed, int trials) {
    XorShift rnd(seed, 1);
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
  // Record-size statistics of H.264 access units parsed in records mode (the bytes the GPU pulls
  // over PCIe per picture): macroblocks, coefficient-pool entries (sparse groups: mask words +
  // values), non-zero coefficients, motion-vector entries.
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
    XorShift next(seed, 7);
    auto rnd = [&]() { return int(next() & 255); };
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
    XorShift rnd(seed, 1);
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
    const std::vector<u8> r = rbsp_of(e);
    return to_bytes(r.data(), r.size());
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
}
