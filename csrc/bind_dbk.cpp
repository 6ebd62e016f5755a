// Test-only entry point: the H.264 loop filter alone, on caller-supplied macroblock records.
//
// avc_deblock_records / avc_deblock_records_many build the MbRec array from per-field numpy
// arrays (the 56-byte layout stays a C++ matter), validate everything the kernels index with,
// and run either avc::cpu_deblock (device -1) or, on a GPU, exactly the runtime's sequence:
// launch_avc_bs, then launch_avc_deblock (8-bit 4:2:0) and / or launch_avc_hbd (High 10, 4:2:2),
// one launch for the whole batch. A wavefront timeout or a bound violation reported in the
// picture's error word is an exception, never a silently wrong picture; the planes live between
// guard bands that must come back intact.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <string>
#include <vector>

#include "bind_ext.h"
#include "vep/avc.h"
#include "vep/avc_recon.h"
#include "vep/codec.h"
#include "vep/gpu.h"

namespace py = pybind11;
using namespace vep;

namespace {

struct DbkCase {
  int wmbs = 0, hmbs = 0, bd = 8, cf = 1, field = 0;
  std::vector<avc::MbRec> recs;
  std::vector<i16> mvs;
  std::vector<u8> y, uv;  // plane bytes (u16 samples above 8 bits)
  bool deblock = false;   // any MB with the filter enabled
  size_t bps() const { return bd > 8 ? 2 : 1; }
  size_t y_samples() const { return size_t(wmbs) * 16 * size_t(hmbs) * 16; }
  size_t uv_samples() const { return size_t(wmbs) * 16 * size_t(hmbs) * (cf == 2 ? 16 : 8); }
};

using IntArr = py::array_t<long long, py::array::c_style | py::array::forcecast>;

IntArr field(const py::dict& recs, const char* name, size_t n, size_t per) {
  VEP_CHECK(recs.contains(name), std::string("deblock records: missing field ") + name);
  IntArr a = IntArr::ensure(recs[name]);
  VEP_CHECK(a && size_t(a.size()) == n * per, std::string("deblock records: field ") + name + " has the wrong size");
  return a;
}

void load_plane(const py::array& a, int bd, size_t samples, const char* what, std::vector<u8>& out) {
  const bool wide = bd > 8;
  VEP_CHECK(a.dtype().is(wide ? py::dtype::of<u16>() : py::dtype::of<u8>()),
            std::string("deblock records: ") + what + " plane must be " + (wide ? "uint16" : "uint8"));
  VEP_CHECK(size_t(a.size()) == samples, std::string("deblock records: ") + what + " plane size does not match wmbs x hmbs");
  py::array c = py::array::ensure(a, py::array::c_style);
  VEP_CHECK(bool(c), "deblock records: plane not contiguous");
  out.resize(samples * (wide ? 2 : 1));
  std::memcpy(out.data(), c.data(), out.size());
  if (wide) {
    const u16* s = reinterpret_cast<const u16*>(out.data());
    for (size_t i = 0; i < samples; ++i) VEP_CHECK(s[i] < (1u << bd), "deblock records: sample above the bit depth");
  }
}

DbkCase make_case(const py::array& y, const py::array& uv, const py::dict& recs, const py::array& mvs, int wmbs, int hmbs,
                  int bd, int cf, int field_) {
  DbkCase c;
  VEP_CHECK(wmbs >= 1 && wmbs <= gpu::kAvcMaxCols && hmbs >= 1 && hmbs <= gpu::kAvcMaxRows,
            "deblock records: wmbs / hmbs out of range");
  VEP_CHECK(bd >= 8 && bd <= 10, "deblock records: bit_depth must be 8..10");
  VEP_CHECK(cf == 1 || cf == 2, "deblock records: chroma_format must be 1 or 2");
  VEP_CHECK(field_ >= 0 && field_ <= 2, "deblock records: field must be 0, 1 or 2");
  c.wmbs = wmbs;
  c.hmbs = hmbs;
  c.bd = bd;
  c.cf = cf;
  c.field = field_;
  load_plane(y, bd, c.y_samples(), "luma", c.y);
  load_plane(uv, bd, c.uv_samples(), "chroma", c.uv);
  {
    py::array_t<i16, py::array::c_style | py::array::forcecast> m = py::array_t<i16, py::array::c_style | py::array::forcecast>::ensure(mvs);
    VEP_CHECK(bool(m), "deblock records: mvs must be an int16 array");
    c.mvs.assign(m.data(), m.data() + m.size());
  }
  const size_t n = size_t(wmbs) * size_t(hmbs);
  const IntArr kind = field(recs, "kind", n, 1), qp = field(recs, "qp", n, 1), qpc = field(recs, "qpc", n, 1),
               qpc2 = field(recs, "qpc2", n, 1), dbk = field(recs, "dbk", n, 1), flags = field(recs, "flags", n, 1),
               nz = field(recs, "nz", n, 1), aoff = field(recs, "alpha_off", n, 1), boff = field(recs, "beta_off", n, 1),
               slice = field(recs, "slice", n, 1), ref = field(recs, "ref", n, 4), ref1 = field(recs, "ref1", n, 4),
               mv = field(recs, "mv", n, 1);
  const int bias = 6 * (bd - 8);
  const long long kFlags = avc::kMbT8x8 | avc::kMbL1 | avc::kMbMv8x8 | avc::kMbMv16;
  c.recs.assign(n, avc::MbRec{});
  for (size_t i = 0; i < n; ++i) {
    avc::MbRec& r = c.recs[i];
    const std::string at = " (MB " + std::to_string(i) + ")";
    VEP_CHECK(kind.data()[i] >= 0 && kind.data()[i] <= 5, "deblock records: kind above 5" + at);
    VEP_CHECK(qp.data()[i] >= 0 && qp.data()[i] <= 51 + bias, "deblock records: qp out of range" + at);
    VEP_CHECK(qpc.data()[i] >= 0 && qpc.data()[i] <= 51 + bias && qpc2.data()[i] >= 0 && qpc2.data()[i] <= 51 + bias,
              "deblock records: qpc out of range" + at);
    VEP_CHECK(dbk.data()[i] >= 0 && dbk.data()[i] <= 3, "deblock records: dbk out of range" + at);
    VEP_CHECK((flags.data()[i] & ~kFlags) == 0, "deblock records: unknown flag" + at);
    VEP_CHECK(nz.data()[i] >= 0 && nz.data()[i] <= 0xFFFF, "deblock records: nz out of range" + at);
    VEP_CHECK(aoff.data()[i] >= -12 && aoff.data()[i] <= 12 && boff.data()[i] >= -12 && boff.data()[i] <= 12,
              "deblock records: filter offset out of range" + at);
    VEP_CHECK(slice.data()[i] >= 0 && slice.data()[i] <= 0xFFFF, "deblock records: slice out of range" + at);
    r.kind = u8(kind.data()[i]);
    r.qp = u8(qp.data()[i]);
    r.qpc = u8(qpc.data()[i]);
    r.qpc2 = u8(qpc2.data()[i]);
    r.dbk = u8(dbk.data()[i]);
    r.flags = u8(flags.data()[i]);
    r.nz = u16(nz.data()[i]);
    r.alpha_off = avc::i8(aoff.data()[i]);
    r.beta_off = avc::i8(boff.data()[i]);
    r.slice = u16(slice.data()[i]);
    for (int k = 0; k < 4; ++k) {
      const long long a = ref.data()[i * 4 + size_t(k)], b = ref1.data()[i * 4 + size_t(k)];
      VEP_CHECK(a >= 0 && a <= 255 && b >= 0 && b <= 255, "deblock records: reference slot out of range" + at);
      r.ref[k] = u8(a);
      r.ref1[k] = u8(b);
    }
    r.res = avc::kNoRes;
    if (!avc::is_intra(r.kind)) {
      const long long off = mv.data()[i];
      const long long need = avc::mv_per_list(r.flags) * ((r.flags & avc::kMbL1) ? 2 : 1);
      VEP_CHECK(off >= 0 && off + need <= (long long)c.mvs.size(), "deblock records: motion vectors outside the pool" + at);
      r.mv = u32(off);
      // (a partition with no reference at all would send the bS rule to its two-vector branch,
      // which reads list-1 vectors the MB may not have)
      for (int k = 0; k < 4; ++k)
        VEP_CHECK(r.ref[k] != 0xFF || ((r.flags & avc::kMbL1) && r.ref1[k] != 0xFF),
                  "deblock records: inter partition without a reference" + at);
    }
    if (!(r.dbk & 1)) c.deblock = true;
  }
  return c;
}

py::array plane_out(const std::vector<u8>& bytes, int bd, size_t rows, size_t pitch) {
  if (bd > 8) {
    py::array_t<u16> a({rows, pitch});
    std::memcpy(a.mutable_data(), bytes.data(), bytes.size());
    return std::move(a);
  }
  py::array_t<u8> a({rows, pitch});
  std::memcpy(a.mutable_data(), bytes.data(), bytes.size());
  return std::move(a);
}

py::tuple case_out(const DbkCase& c) {
  const size_t pitch = size_t(c.wmbs) * 16;
  return py::make_tuple(plane_out(c.y, c.bd, size_t(c.hmbs) * 16, pitch),
                        plane_out(c.uv, c.bd, size_t(c.hmbs) * (c.cf == 2 ? 16 : 8), pitch));
}

void run_cpu(DbkCase& c) {
  avc::Picture pic;
  pic.wmbs = c.wmbs;
  pic.hmbs = c.hmbs;
  pic.mbs.append(c.recs.data(), c.recs.size());
  pic.mvs.append(c.mvs.data(), c.mvs.size());
  pic.structure = c.field;
  pic.bd = c.bd;
  pic.cf = c.cf;
  pic.qp_bias = pic.qpc_bias = 6 * (c.bd - 8);
  pic.deblock = c.deblock;
  HostSurface T;
  T.alloc(c.wmbs * 16, c.hmbs * 16, c.bd, c.cf);
  if (T.wide()) {
    std::memcpy(T.y16.data(), c.y.data(), c.y.size());
    std::memcpy(T.uv16.data(), c.uv.data(), c.uv.size());
  } else {
    std::memcpy(T.y.data(), c.y.data(), c.y.size());
    std::memcpy(T.uv.data(), c.uv.data(), c.uv.size());
  }
  avc::cpu_deblock(pic, T);
  if (T.wide()) {
    std::memcpy(c.y.data(), T.y16.data(), c.y.size());
    std::memcpy(c.uv.data(), T.uv16.data(), c.uv.size());
  } else {
    std::memcpy(c.y.data(), T.y.data(), c.y.size());
    std::memcpy(c.uv.data(), T.uv.data(), c.uv.size());
  }
}

constexpr size_t kGuard = 1024;  // bytes of kGuardByte on either side of every plane
constexpr u8 kGuardByte = 0xA5;

// One device allocation for the batch: descriptors, then per picture the records, the mv pool,
// the AvcDbkInfo scratch, the exchange words and the two planes (each between guard bands), then
// one error word per picture. Offsets are multiples of 256.
void run_gpu(std::vector<DbkCase>& cs, int device, int variant) {
  int ndev = 0;
  VEP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device < ndev, "deblock records: no such GPU");
  VEP_HIP(hipSetDevice(device));
  const size_t n = cs.size();
  struct Off {
    size_t recs, mvs, dbk, xg, y, uv;
  };
  std::vector<Off> off(n);
  size_t top = 0;
  auto take = [&](size_t bytes) {
    const size_t at = top;
    top += (std::max<size_t>(bytes, 1) + 255) & ~size_t(255);
    return at;
  };
  const size_t off_desc = take(n * sizeof(gpu::AvcDesc));
  for (size_t k = 0; k < n; ++k) {
    const DbkCase& c = cs[k];
    off[k].recs = take(c.recs.size() * sizeof(avc::MbRec));
    off[k].mvs = take(c.mvs.size() * sizeof(i16));
    off[k].dbk = take(c.recs.size() * sizeof(gpu::AvcDbkInfo));
    off[k].xg = take(gpu::avc_xg_bytes(c.wmbs, c.hmbs));
    take(kGuard);
    off[k].y = take(c.y.size());
    take(kGuard);
    off[k].uv = take(c.uv.size());
    take(kGuard);
  }
  const size_t off_err = take(n * sizeof(u32));
  std::vector<u8> host(top, kGuardByte);
  std::memset(host.data() + off_err, 0, n * sizeof(u32));
  u8* dev = nullptr;
  VEP_HIP(hipMalloc(reinterpret_cast<void**>(&dev), top));
  int mbs = 0, max_h = 0, variants = 0;
  bool narrow = false;
  auto* descs = reinterpret_cast<gpu::AvcDesc*>(host.data() + off_desc);
  for (size_t k = 0; k < n; ++k) {
    const DbkCase& c = cs[k];
    std::memcpy(host.data() + off[k].recs, c.recs.data(), c.recs.size() * sizeof(avc::MbRec));
    if (!c.mvs.empty()) std::memcpy(host.data() + off[k].mvs, c.mvs.data(), c.mvs.size() * sizeof(i16));
    std::memcpy(host.data() + off[k].y, c.y.data(), c.y.size());
    std::memcpy(host.data() + off[k].uv, c.uv.data(), c.uv.size());
    gpu::AvcDesc g{};
    g.mbs = dev + off[k].recs;
    g.mvs = reinterpret_cast<const i16*>(dev + off[k].mvs);
    g.y = dev + off[k].y;
    g.uv = dev + off[k].uv;
    g.slot_y = c.y.size();
    g.slot_uv = c.uv.size();
    g.wmbs = c.wmbs;
    g.hmbs = c.hmbs;
    g.target = 0;
    g.mb_begin = mbs;
    g.field = c.field;
    g.err = reinterpret_cast<u32*>(dev + off_err) + k;
    g.dbk = dev + off[k].dbk;
    g.xg = reinterpret_cast<u64*>(dev + off[k].xg);
    g.bd = c.bd;
    g.qp_bias = g.qpc_bias = 6 * (c.bd - 8);
    g.cf = c.cf;
    g.deblock = c.deblock ? 1 : 0;
    descs[k] = g;
    mbs += int(c.recs.size());
    max_h = std::max(max_h, c.hmbs);
    if (c.bd > 8 || c.cf == 2) variants |= c.cf != 2 ? 1 : (c.bd > 8 ? 4 : 2);
    else narrow = true;
  }
  try {
    const hipStream_t s = nullptr;
    VEP_HIP(hipMemcpyAsync(dev, host.data(), top, hipMemcpyHostToDevice, s));
    const auto* dd = reinterpret_cast<const gpu::AvcDesc*>(dev + off_desc);
    gpu::launch_avc_bs(dd, int(n), mbs, s);
    if (narrow) gpu::launch_avc_deblock(dd, int(n), max_h, s, variant);
    if (variants) gpu::launch_avc_hbd(dd, int(n), false, true, variants, s);
    VEP_HIP(hipStreamSynchronize(s));
    VEP_HIP(hipMemcpy(host.data(), dev, top, hipMemcpyDeviceToHost));
  } catch (...) {
    (void)hipFree(dev);
    throw;
  }
  (void)hipFree(dev);
  const u32* err = reinterpret_cast<const u32*>(host.data() + off_err);
  for (size_t k = 0; k < n; ++k) {
    VEP_CHECK(err[k] == 0, "deblock records: picture " + std::to_string(k) + " error word " + std::to_string(err[k]));
    DbkCase& c = cs[k];
    auto guard_ok = [&](size_t at) {
      for (size_t i = 0; i < kGuard; ++i)
        if (host[at + i] != kGuardByte) return false;
      return true;
    };
    VEP_CHECK(guard_ok(off[k].y - kGuard) && guard_ok(off[k].y + ((c.y.size() + 255) & ~size_t(255))) &&
                  guard_ok(off[k].uv + ((c.uv.size() + 255) & ~size_t(255))),
              "deblock records: picture " + std::to_string(k) + " guard band written");
    // (the padding between a plane's end and the next 256-byte boundary is guard as well)
    for (size_t i = c.y.size(); i < ((c.y.size() + 255) & ~size_t(255)); ++i)
      VEP_CHECK(host[off[k].y + i] == kGuardByte, "deblock records: byte after the luma plane written");
    for (size_t i = c.uv.size(); i < ((c.uv.size() + 255) & ~size_t(255)); ++i)
      VEP_CHECK(host[off[k].uv + i] == kGuardByte, "deblock records: byte after the chroma plane written");
    std::memcpy(c.y.data(), host.data() + off[k].y, c.y.size());
    std::memcpy(c.uv.data(), host.data() + off[k].uv, c.uv.size());
  }
}

void check_variant(int device, int variant) {
  VEP_CHECK(device >= -1, "deblock records: device must be -1 (CPU) or a GPU index");
  VEP_CHECK(variant == 0 || variant == 1 || variant == 3 || variant == 4 || variant == 5,
            "deblock records: variant must be one of 0, 1, 3, 4, 5");
}

}  // namespace

void bind_dbk(py::module_& m) {
  m.def(
      "avc_deblock_records",
      [](const py::array& y, const py::array& uv, const py::dict& recs, const py::array& mvs, int wmbs, int hmbs,
         int bit_depth, int chroma_format, int field, int device, int variant) {
        check_variant(device, variant);
        std::vector<DbkCase> cs;
        cs.push_back(make_case(y, uv, recs, mvs, wmbs, hmbs, bit_depth, chroma_format, field));
        if (device < 0) run_cpu(cs[0]);
        else {
          py::gil_scoped_release rel;
          run_gpu(cs, device, variant);
        }
        return case_out(cs[0]);
      },
      py::arg("y"), py::arg("uv"), py::arg("recs"), py::arg("mvs"), py::arg("wmbs"), py::arg("hmbs"), py::kw_only(),
      py::arg("bit_depth") = 8, py::arg("chroma_format") = 1, py::arg("field") = 0, py::arg("device") = -1,
      py::arg("variant") = 5);
  // Several pictures (dicts with the keyword names above), mixed sizes and formats, in ONE launch
  // sequence: one descriptor array, mb_begin as the exclusive prefix of MBs, the grid sized by
  // the tallest picture.
  m.def(
      "avc_deblock_records_many",
      [](const std::vector<py::dict>& pics, int device, int variant) {
        check_variant(device, variant);
        std::vector<DbkCase> cs;
        for (const py::dict& p : pics) {
          auto geti = [&](const char* k, int dflt) { return p.contains(k) ? p[k].cast<int>() : dflt; };
          for (const char* k : {"y", "uv", "recs", "mvs", "wmbs", "hmbs"})
            VEP_CHECK(p.contains(k), std::string("deblock records: picture lacks ") + k);
          cs.push_back(make_case(p["y"].cast<py::array>(), p["uv"].cast<py::array>(), p["recs"].cast<py::dict>(),
                                 p["mvs"].cast<py::array>(), p["wmbs"].cast<int>(), p["hmbs"].cast<int>(),
                                 geti("bit_depth", 8), geti("chroma_format", 1), geti("field", 0)));
        }
        if (!cs.empty()) {
          if (device < 0) {
            for (DbkCase& c : cs) run_cpu(c);
          } else {
            py::gil_scoped_release rel;
            run_gpu(cs, device, variant);
          }
        }
        py::list out;
        for (const DbkCase& c : cs) out.append(case_out(c));
        return out;
      },
      py::arg("pics"), py::arg("device") = -1, py::arg("variant") = 5);
}
