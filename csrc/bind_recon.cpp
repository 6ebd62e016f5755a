// Test-only entry point: H.264 reconstruction (motion compensation, intra prediction, residual;
// no loop filter) of caller-supplied macroblock records.
//
// avc_recon_records / avc_recon_records_many build the MbRec array, the sparse coefficient pool
// (the store / expand format of avc_recon.h), the mv pool and the weight pool from per-field
// numpy arrays (the 56-byte layout and the sparse format stay a C++ matter), validate everything
// a kernel indexes with, and run either avc::cpu_reconstruct (device -1) or, on a GPU, exactly
// the runtime's sequence: launch_avc_inter, then launch_avc_intra (8-bit 4:2:0 pictures) and /
// or launch_avc_hbd(intra, no loop filter) (High 10, 4:2:2), one launch sequence for the whole
// batch with mb_begin as the exclusive prefix. A non-zero error word (bit 1 a wavefront timeout,
// 0x4000 / 0x8000 a pool bound) is an exception, never a silently wrong picture; every DPB
// surface lives between guard bands that must come back intact, and the reference surfaces must
// come back unchanged.
//
// Records the parser can never produce are refused here, not run: the kernels index with them
// unchecked. avc::validate (avc.cpp validate_mb) refuses a partially coded 8x8 residual block, an
// inter partition without a reference, a list-1 reference without kMbL1, a mode above its range;
// this file adds what validate leaves to the caller of cpu_reconstruct: reference slots other
// than the target, weights in the WpEntry ranges, coefficients outside the coded blocks.
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

struct ReconCase {
  int wmbs = 0, hmbs = 0, bd = 8, cf = 1, field = 0, slots = 1, target = 0;
  bool constrained = false;
  std::vector<avc::MbRec> recs;
  std::vector<i16> mvs, coefs;
  std::vector<avc::WpEntry> wps;
  std::vector<u8> y, uv;  // every slot's plane bytes, slot after slot (u16 samples above 8 bits)
  int intra_mbs = 0, intra_res = 0;
  size_t bps() const { return bd > 8 ? 2 : 1; }
  size_t chroma_rows() const { return size_t(hmbs) * (cf == 2 ? 16 : 8); }
  size_t y_bytes() const { return size_t(wmbs) * 16 * size_t(hmbs) * 16 * bps(); }  // one slot
  size_t uv_bytes() const { return size_t(wmbs) * 16 * chroma_rows() * bps(); }
};

using IntArr = py::array_t<long long, py::array::c_style | py::array::forcecast>;

IntArr field(const py::dict& d, const char* name, size_t n, size_t per, const char* what = "recon records") {
  VEP_CHECK(d.contains(name), std::string(what) + ": missing field " + name);
  IntArr a = IntArr::ensure(d[name]);
  VEP_CHECK(a && size_t(a.size()) == n * per, std::string(what) + ": field " + name + " has the wrong size");
  return a;
}

IntArr field_or_zero(const py::dict& d, const char* name, size_t n) {
  if (d.contains(name)) return field(d, name, n, 1);
  IntArr a(static_cast<py::ssize_t>(n));
  std::memset(a.mutable_data(), 0, n * sizeof(long long));
  return a;
}

void load_planes(const py::array& a, int bd, size_t bytes, const char* what, std::vector<u8>& out) {
  const bool wide = bd > 8;
  VEP_CHECK(a.dtype().is(wide ? py::dtype::of<u16>() : py::dtype::of<u8>()),
            std::string("recon records: ") + what + " planes must be " + (wide ? "uint16" : "uint8"));
  VEP_CHECK(size_t(a.nbytes()) == bytes, std::string("recon records: ") + what + " planes do not match slots x hmbs x wmbs");
  py::array c = py::array::ensure(a, py::array::c_style);
  VEP_CHECK(bool(c), "recon records: planes not contiguous");
  out.resize(bytes);
  std::memcpy(out.data(), c.data(), bytes);
  if (wide) {
    const u16* s = reinterpret_cast<const u16*>(out.data());
    for (size_t i = 0; i < bytes / 2; ++i) VEP_CHECK(s[i] < (1u << bd), "recon records: sample above the bit depth");
  }
}

ReconCase make_case(const py::dict& p) {
  auto geti = [&](const char* k, int dflt) { return p.contains(k) ? p[k].cast<int>() : dflt; };
  for (const char* k : {"y", "uv", "recs", "mvs", "wps", "coefs", "wmbs", "hmbs", "slots", "target"})
    VEP_CHECK(p.contains(k), std::string("recon records: picture lacks ") + k);
  ReconCase c;
  c.wmbs = p["wmbs"].cast<int>();
  c.hmbs = p["hmbs"].cast<int>();
  c.slots = p["slots"].cast<int>();
  c.target = p["target"].cast<int>();
  c.bd = geti("bit_depth", 8);
  c.cf = geti("chroma_format", 1);
  c.field = geti("field", 0);
  c.constrained = geti("constrained_intra", 0) != 0;
  VEP_CHECK(c.wmbs >= 1 && c.wmbs <= gpu::kAvcMaxCols && c.hmbs >= 1 && c.hmbs <= gpu::kAvcMaxRows,
            "recon records: wmbs / hmbs out of range");
  VEP_CHECK(c.bd >= 8 && c.bd <= 10, "recon records: bit_depth must be 8..10");
  VEP_CHECK(c.cf == 1 || c.cf == 2, "recon records: chroma_format must be 1 or 2");
  VEP_CHECK(c.field >= 0 && c.field <= 2, "recon records: field must be 0, 1 or 2");
  // (Decoder::parse refuses High 10 / 4:2:2 field pictures as UnsupportedStream before a record is
  // written, so no kernel meets one; in 4:2:2 table 8-9's chroma offset would not apply, §8.4.1.4)
  VEP_CHECK(c.field == 0 || (c.bd == 8 && c.cf == 1), "recon records: field pictures are 8-bit 4:2:0 only");
  VEP_CHECK(c.slots >= 1 && c.slots <= avc::kMaxDpbSlots && c.target >= 0 && c.target < c.slots,
            "recon records: slots / target out of range");
  load_planes(p["y"].cast<py::array>(), c.bd, c.y_bytes() * size_t(c.slots), "luma", c.y);
  load_planes(p["uv"].cast<py::array>(), c.bd, c.uv_bytes() * size_t(c.slots), "chroma", c.uv);
  {
    auto m = py::array_t<i16, py::array::c_style | py::array::forcecast>::ensure(p["mvs"]);
    VEP_CHECK(bool(m), "recon records: mvs must be an int16 array");
    c.mvs.assign(m.data(), m.data() + m.size());
  }
  {  // the weight pool: per entry and component w0, w1, o, lwd
    const py::dict w = p["wps"].cast<py::dict>();
    VEP_CHECK(w.contains("lwd"), "recon weights: missing field lwd");
    const size_t nw = size_t(IntArr::ensure(w["lwd"]).size()) / 3;
    const IntArr w0 = field(w, "w0", nw, 3, "recon weights"), w1 = field(w, "w1", nw, 3, "recon weights"),
                 o = field(w, "o", nw, 3, "recon weights"), lwd = field(w, "lwd", nw, 3, "recon weights");
    const long long omax = 128ll << (c.bd - 8);
    c.wps.assign(nw, avc::WpEntry{});
    for (size_t i = 0; i < nw; ++i)
      for (size_t k = 0; k < 3; ++k) {
        const size_t j = i * 3 + k;
        // explicit weights are se(v) in -128..127, implicit ones 64 - w, w with w in -64..128;
        // offsets -128..127 at 8 bits, scaled by the host above
        VEP_CHECK(w0.data()[j] >= -128 && w0.data()[j] <= 128 && w1.data()[j] >= -128 && w1.data()[j] <= 128,
                  "recon weights: weight outside -128..128 (entry " + std::to_string(i) + ")");
        VEP_CHECK(o.data()[j] >= -omax && o.data()[j] < omax, "recon weights: offset out of range (entry " + std::to_string(i) + ")");
        VEP_CHECK(lwd.data()[j] >= 0 && lwd.data()[j] <= 7, "recon weights: logWD out of range (entry " + std::to_string(i) + ")");
        c.wps[i].w0[k] = i16(w0.data()[j]);
        c.wps[i].w1[k] = i16(w1.data()[j]);
        c.wps[i].o[k] = i16(o.data()[j]);
        c.wps[i].lwd[k] = u8(lwd.data()[j]);
      }
  }
  const py::dict recs = p["recs"].cast<py::dict>();
  const size_t n = size_t(c.wmbs) * size_t(c.hmbs);
  const IntArr kind = field(recs, "kind", n, 1), flags = field(recs, "flags", n, 1), slice = field(recs, "slice", n, 1),
               ref = field(recs, "ref", n, 4), ref1 = field(recs, "ref1", n, 4), mv = field(recs, "mv", n, 1),
               i16m = field(recs, "i16_mode", n, 1), cm = field(recs, "chroma_mode", n, 1), i4 = field(recs, "i4", n, 16),
               lc = field(recs, "luma_coded", n, 1), cc = field(recs, "chroma_coded", n, 1), wp = field(recs, "wp", n, 1),
               qp = field_or_zero(recs, "qp", n), qpc = field_or_zero(recs, "qpc", n), qpc2 = field_or_zero(recs, "qpc2", n),
               nz = field_or_zero(recs, "nz", n);
  const IntArr coefs = field(p, "coefs", n, size_t(avc::kDenseCoefs), "recon records");
  const int bias = 6 * (c.bd - 8);
  const long long kFlags = avc::kMbT8x8 | avc::kMbL1 | avc::kMbWp | avc::kMbMv8x8 | avc::kMbMv16;
  const int nbc = c.cf == 2 ? 8 : 4;               // chroma 4x4 blocks per component
  const size_t npcm = c.cf == 2 ? 512 : 384;       // I_PCM samples per MB
  c.recs.assign(n, avc::MbRec{});
  for (size_t i = 0; i < n; ++i) {
    avc::MbRec& r = c.recs[i];
    const std::string at = " (MB " + std::to_string(i) + ")";
    const long long* dc = coefs.data() + i * size_t(avc::kDenseCoefs);
    VEP_CHECK(kind.data()[i] >= 0 && kind.data()[i] <= 5, "recon records: kind above 5" + at);
    VEP_CHECK((flags.data()[i] & ~kFlags) == 0, "recon records: unknown flag" + at);
    VEP_CHECK(!((flags.data()[i] & avc::kMbMv8x8) && (flags.data()[i] & avc::kMbMv16)), "recon records: two mv granularities" + at);
    VEP_CHECK(slice.data()[i] >= 0 && slice.data()[i] <= 0xFFFF, "recon records: slice out of range" + at);
    VEP_CHECK(qp.data()[i] >= 0 && qp.data()[i] <= 51 + bias && qpc.data()[i] >= 0 && qpc.data()[i] <= 51 + bias &&
                  qpc2.data()[i] >= 0 && qpc2.data()[i] <= 51 + bias,
              "recon records: qp out of range" + at);
    VEP_CHECK(i16m.data()[i] >= 0 && i16m.data()[i] <= 3 && cm.data()[i] >= 0 && cm.data()[i] <= 3,
              "recon records: intra mode out of range" + at);
    VEP_CHECK(lc.data()[i] >= 0 && lc.data()[i] <= 0xFFFF && cc.data()[i] >= 0 && cc.data()[i] < (1ll << (2 * nbc)),
              "recon records: coded mask out of range" + at);
    VEP_CHECK(nz.data()[i] >= 0 && nz.data()[i] <= 0xFFFF, "recon records: nz out of range" + at);
    r.kind = u8(kind.data()[i]);
    r.flags = u8(flags.data()[i]);
    r.slice = u16(slice.data()[i]);
    r.qp = u8(qp.data()[i]);
    r.qpc = u8(qpc.data()[i]);
    r.qpc2 = u8(qpc2.data()[i]);
    r.nz = u16(nz.data()[i]);
    r.dbk = 1;  // the loop filter is off: this entry point stops before it
    r.i16_mode = u8(i16m.data()[i]);
    r.chroma_mode = u8(cm.data()[i]);
    r.res = avc::kNoRes;
    for (int k = 0; k < 16; ++k) {
      const long long m4 = i4.data()[i * 16 + size_t(k)];
      VEP_CHECK(m4 >= 0 && m4 <= 8, "recon records: Intra_4x4 / 8x8 mode out of range" + at);
      r.i4[k >> 1] = u8(r.i4[k >> 1] | (u8(m4) << ((k & 1) * 4)));
    }
    for (int k = 0; k < 4; ++k) {
      const long long a = ref.data()[i * 4 + size_t(k)], b = ref1.data()[i * 4 + size_t(k)];
      VEP_CHECK((a == 0xFF || (a >= 0 && a < c.slots && a != c.target)) && (b == 0xFF || (b >= 0 && b < c.slots && b != c.target)),
                "recon records: reference slot outside the DPB, or the target" + at);
      r.ref[k] = u8(a);
      r.ref1[k] = u8(b);
    }
    r.coef = u32(c.coefs.size());
    if (r.kind == avc::kIPcm) {
      // raw samples: 256 luma (raster), then Cb and Cr (8 wide), as bytes or u16
      VEP_CHECK(r.flags == 0 && lc.data()[i] == 0 && cc.data()[i] == 0, "recon records: I_PCM with flags or coded masks" + at);
      const size_t o = c.coefs.size();
      c.coefs.resize(o + (c.bd > 8 ? npcm : npcm / 2));
      for (size_t k = 0; k < npcm; ++k) {
        VEP_CHECK(dc[k] >= 0 && dc[k] < (1ll << c.bd), "recon records: I_PCM sample above the bit depth" + at);
        if (c.bd > 8) reinterpret_cast<u16*>(c.coefs.data() + o)[k] = u16(dc[k]);
        else reinterpret_cast<u8*>(c.coefs.data() + o)[k] = u8(dc[k]);
      }
      continue;
    }
    r.luma_coded = u16(lc.data()[i]);
    r.chroma_coded = u16(cc.data()[i]);
    const bool inter = r.kind == avc::kSkip || r.kind == avc::kInter;
    VEP_CHECK(r.kind != avc::kI8x8 || (r.flags & avc::kMbT8x8), "recon records: Intra_8x8 without the 8x8 transform" + at);
    VEP_CHECK(!((r.flags & avc::kMbT8x8) && (r.kind == avc::kI4x4 || r.kind == avc::kI16x16)),
              "recon records: Intra_4x4 / 16x16 with the 8x8 transform" + at);
    VEP_CHECK(inter || !(r.flags & (avc::kMbL1 | avc::kMbWp | avc::kMbMv8x8 | avc::kMbMv16)), "recon records: inter flag on an intra MB" + at);
    // the sparse groups: the mask words of the coded groups, then their non-zero values
    {
      const long long* grp[32];
      int ng = 0;
      bool used[avc::kDenseCoefs / 16] = {};
      if (r.flags & avc::kMbT8x8) {
        for (int q = 0; q < 4; ++q) {
          const u32 g = (u32(r.luma_coded) >> ((q & 1) * 2 + (q >> 1) * 8)) & 0x33u;
          VEP_CHECK(g == 0 || g == 0x33u, "recon records: 8x8 residual block partially coded" + at);
          if (g)
            for (int w = 0; w < 4; ++w) {
              grp[ng++] = dc + 64 * q + 16 * w;
              used[4 * q + w] = true;
            }
        }
      } else {
        for (u32 w = r.luma_coded; w; w &= w - 1) {
          grp[ng++] = dc + 16 * __builtin_ctz(w);
          used[__builtin_ctz(w)] = true;
        }
      }
      for (u32 w = r.chroma_coded; w; w &= w - 1) {
        grp[ng++] = dc + 256 + 16 * __builtin_ctz(w);
        used[16 + __builtin_ctz(w)] = true;
      }
      for (int g = 0; g < avc::kDenseCoefs / 16; ++g)
        for (int k = 0; k < 16 && !used[g]; ++k)
          VEP_CHECK(dc[16 * g + k] == 0, "recon records: coefficient in a block that is not coded" + at);
      const size_t o = c.coefs.size();
      c.coefs.resize(o + size_t(ng));
      for (int g = 0; g < ng; ++g) {
        u32 mask = 0;
        for (int k = 0; k < 16; ++k) {
          VEP_CHECK(grp[g][k] >= -32768 && grp[g][k] <= 32767, "recon records: coefficient outside int16" + at);
          if (grp[g][k]) {
            mask |= 1u << k;
            c.coefs.push_back(i16(grp[g][k]));
          }
        }
        c.coefs[o + size_t(g)] = i16(u16(mask));
      }
    }
    if (inter) {
      const long long off = mv.data()[i];
      const long long need = avc::mv_per_list(r.flags) * ((r.flags & avc::kMbL1) ? 2 : 1);
      VEP_CHECK(off >= 0 && off + need <= (long long)c.mvs.size(), "recon records: motion vectors outside the pool" + at);
      r.mv = u32(off);
      for (int k = 0; k < 4; ++k) {
        VEP_CHECK(r.ref[k] != 0xFF || r.ref1[k] != 0xFF, "recon records: inter partition without a reference" + at);
        VEP_CHECK(r.ref1[k] == 0xFF || (r.flags & avc::kMbL1), "recon records: list-1 reference without list-1 motion" + at);
      }
      if (r.flags & avc::kMbWp) {
        VEP_CHECK(wp.data()[i] >= 0 && size_t(wp.data()[i]) + 4 <= c.wps.size(), "recon records: weights outside the pool" + at);
        r.wp = u32(wp.data()[i]);
      }
    } else {
      ++c.intra_mbs;
      if (r.luma_coded | r.chroma_coded) r.res = u32(c.intra_res++);
    }
  }
  return c;
}

py::array plane_out(const u8* bytes, int bd, size_t rows, size_t pitch) {
  if (bd > 8) {
    py::array_t<u16> a({rows, pitch});
    std::memcpy(a.mutable_data(), bytes, rows * pitch * 2);
    return std::move(a);
  }
  py::array_t<u8> a({rows, pitch});
  std::memcpy(a.mutable_data(), bytes, rows * pitch);
  return std::move(a);
}

py::tuple case_out(const ReconCase& c) {
  const size_t pitch = size_t(c.wmbs) * 16;
  return py::make_tuple(plane_out(c.y.data() + size_t(c.target) * c.y_bytes(), c.bd, size_t(c.hmbs) * 16, pitch),
                        plane_out(c.uv.data() + size_t(c.target) * c.uv_bytes(), c.bd, c.chroma_rows(), pitch));
}

avc::Picture picture_of(const ReconCase& c) {
  avc::Picture pic;
  pic.wmbs = c.wmbs;
  pic.hmbs = c.hmbs;
  pic.mbs.append(c.recs.data(), c.recs.size());
  pic.mvs.append(c.mvs.data(), c.mvs.size());
  pic.coefs.append(c.coefs.data(), c.coefs.size());
  pic.wps.append(c.wps.data(), c.wps.size());
  pic.target = c.target;
  pic.dpb_slots = c.slots;
  pic.structure = c.field;
  pic.bd = c.bd;
  pic.cf = c.cf;
  pic.qp_bias = pic.qpc_bias = 6 * (c.bd - 8);
  pic.constrained_intra = c.constrained;
  pic.intra_mbs = c.intra_mbs;
  pic.intra_res = c.intra_res;
  pic.inter_mbs = int(c.recs.size()) - c.intra_mbs;
  pic.deblock = false;
  return pic;
}

void run_cpu(ReconCase& c) {
  const avc::Picture pic = picture_of(c);
  std::vector<HostSurface> S(size_t(c.slots));
  for (int k = 0; k < c.slots; ++k) {
    HostSurface& T = S[size_t(k)];
    T.alloc(c.wmbs * 16, c.hmbs * 16, c.bd, c.cf);
    std::memcpy(T.wide() ? static_cast<void*>(T.y16.data()) : T.y.data(), c.y.data() + size_t(k) * c.y_bytes(), c.y_bytes());
    std::memcpy(T.wide() ? static_cast<void*>(T.uv16.data()) : T.uv.data(), c.uv.data() + size_t(k) * c.uv_bytes(), c.uv_bytes());
  }
  avc::cpu_reconstruct(pic, S);
  for (int k = 0; k < c.slots; ++k) {
    const HostSurface& T = S[size_t(k)];
    const void* ys = T.wide() ? static_cast<const void*>(T.y16.data()) : T.y.data();
    const void* us = T.wide() ? static_cast<const void*>(T.uv16.data()) : T.uv.data();
    if (k != c.target)
      VEP_CHECK(!std::memcmp(ys, c.y.data() + size_t(k) * c.y_bytes(), c.y_bytes()) &&
                    !std::memcmp(us, c.uv.data() + size_t(k) * c.uv_bytes(), c.uv_bytes()),
                "recon records: reference surface " + std::to_string(k) + " changed");
    std::memcpy(c.y.data() + size_t(k) * c.y_bytes(), ys, c.y_bytes());
    std::memcpy(c.uv.data() + size_t(k) * c.uv_bytes(), us, c.uv_bytes());
  }
}

constexpr size_t kGuard = 1024;  // bytes of kGuardByte before, between and after the slots of a plane
constexpr u8 kGuardByte = 0xA5;

size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

// One device allocation for the batch: descriptors, then per picture the records, the three
// pools, the residual scratch, the exchange words and the two planes' slots (a guard band before
// the first slot and after every slot: the slot stride is the plane rounded up to 256 bytes plus
// the band), then one error word per picture.
void run_gpu(std::vector<ReconCase>& cs, int device) {
  int ndev = 0;
  VEP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device < ndev, "recon records: no such GPU");
  VEP_HIP(hipSetDevice(device));
  const size_t n = cs.size();
  struct Off {
    size_t recs, coefs, mvs, wps, res, xg, y, uv, sy, suv;  // sy / suv: slot strides
  };
  std::vector<Off> off(n);
  size_t top = 0;
  auto take = [&](size_t bytes) {
    const size_t at = top;
    top += up256(std::max<size_t>(bytes, 1));
    return at;
  };
  const size_t off_desc = take(n * sizeof(gpu::AvcDesc));
  for (size_t k = 0; k < n; ++k) {
    const ReconCase& c = cs[k];
    Off& o = off[k];
    o.recs = take(c.recs.size() * sizeof(avc::MbRec));
    o.coefs = take(c.coefs.size() * sizeof(i16));
    o.mvs = take(c.mvs.size() * sizeof(i16));
    o.wps = take(c.wps.size() * sizeof(avc::WpEntry));
    o.res = take(size_t(c.intra_res) * gpu::kAvcResSamples * sizeof(i16));
    o.xg = take(gpu::avc_xg_bytes(c.wmbs, c.hmbs));
    o.sy = up256(c.y_bytes()) + kGuard;
    o.suv = up256(c.uv_bytes()) + kGuard;
    take(kGuard);
    o.y = take(o.sy * size_t(c.slots));
    take(kGuard);
    o.uv = take(o.suv * size_t(c.slots));
  }
  const size_t off_err = take(n * sizeof(u32));
  std::vector<u8> host(top, kGuardByte);
  std::memset(host.data() + off_err, 0, n * sizeof(u32));
  u8* dev = nullptr;
  VEP_HIP(hipMalloc(reinterpret_cast<void**>(&dev), top));
  int mbs = 0, max_h = 0, variants = 0;
  bool narrow = false, intra = false;
  auto* descs = reinterpret_cast<gpu::AvcDesc*>(host.data() + off_desc);
  for (size_t k = 0; k < n; ++k) {
    const ReconCase& c = cs[k];
    const Off& o = off[k];
    auto put = [&](size_t at, const void* src, size_t bytes) {
      if (bytes) std::memcpy(host.data() + at, src, bytes);
    };
    put(o.recs, c.recs.data(), c.recs.size() * sizeof(avc::MbRec));
    put(o.coefs, c.coefs.data(), c.coefs.size() * sizeof(i16));
    put(o.mvs, c.mvs.data(), c.mvs.size() * sizeof(i16));
    put(o.wps, c.wps.data(), c.wps.size() * sizeof(avc::WpEntry));
    for (int s = 0; s < c.slots; ++s) {
      put(o.y + size_t(s) * o.sy, c.y.data() + size_t(s) * c.y_bytes(), c.y_bytes());
      put(o.uv + size_t(s) * o.suv, c.uv.data() + size_t(s) * c.uv_bytes(), c.uv_bytes());
    }
    gpu::AvcDesc g{};
    g.mbs = dev + o.recs;
    g.coefs = reinterpret_cast<const i16*>(dev + o.coefs);
    g.mvs = reinterpret_cast<const i16*>(dev + o.mvs);
    g.wps = dev + o.wps;
    g.y = dev + o.y;
    g.uv = dev + o.uv;
    g.slot_y = o.sy;
    g.slot_uv = o.suv;
    g.wmbs = c.wmbs;
    g.hmbs = c.hmbs;
    g.target = c.target;
    g.constrained = c.constrained ? 1 : 0;
    g.mb_begin = mbs;
    g.field = c.field;
    g.err = reinterpret_cast<u32*>(dev + off_err) + k;
    g.res = reinterpret_cast<i16*>(dev + o.res);
    g.xg = reinterpret_cast<u64*>(dev + o.xg);
    g.bd = c.bd;
    g.qp_bias = g.qpc_bias = 6 * (c.bd - 8);
    g.cf = c.cf;
    g.ncoef = u32(c.coefs.size());
    g.nres = u32(c.intra_res);
    g.intra_mbs = c.intra_mbs;
    g.deblock = 0;
    descs[k] = g;
    mbs += int(c.recs.size());
    max_h = std::max(max_h, c.hmbs);
    intra |= c.intra_mbs > 0;
    if (c.bd > 8 || c.cf == 2) variants |= c.cf != 2 ? 1 : (c.bd > 8 ? 4 : 2);
    else narrow = true;
  }
  try {
    const hipStream_t s = nullptr;
    VEP_HIP(hipMemcpyAsync(dev, host.data(), top, hipMemcpyHostToDevice, s));
    const auto* dd = reinterpret_cast<const gpu::AvcDesc*>(dev + off_desc);
    gpu::launch_avc_inter(dd, int(n), mbs, s);
    if (intra && narrow) gpu::launch_avc_intra(dd, int(n), max_h, s);
    if (variants) gpu::launch_avc_hbd(dd, int(n), intra, false, variants, s);
    VEP_HIP(hipStreamSynchronize(s));
    VEP_HIP(hipMemcpy(host.data(), dev, top, hipMemcpyDeviceToHost));
  } catch (...) {
    (void)hipFree(dev);
    throw;
  }
  (void)hipFree(dev);
  const u32* err = reinterpret_cast<const u32*>(host.data() + off_err);
  for (size_t k = 0; k < n; ++k) {
    const std::string pk = "recon records: picture " + std::to_string(k);
    VEP_CHECK(err[k] == 0, pk + " error word " + std::to_string(err[k]));
    ReconCase& c = cs[k];
    const Off& o = off[k];
    auto guard_ok = [&](size_t at, size_t len) {
      for (size_t i = 0; i < len; ++i)
        if (host[at + i] != kGuardByte) return false;
      return true;
    };
    VEP_CHECK(guard_ok(o.y - kGuard, kGuard) && guard_ok(o.uv - kGuard, kGuard), pk + " guard band before a plane written");
    for (int s = 0; s < c.slots; ++s) {
      const size_t ay = o.y + size_t(s) * o.sy, auv = o.uv + size_t(s) * o.suv;
      // (the padding between a plane's end and its band is guard as well)
      VEP_CHECK(guard_ok(ay + c.y_bytes(), o.sy - c.y_bytes()), pk + " guard band after luma slot " + std::to_string(s) + " written");
      VEP_CHECK(guard_ok(auv + c.uv_bytes(), o.suv - c.uv_bytes()), pk + " guard band after chroma slot " + std::to_string(s) + " written");
      if (s != c.target)
        VEP_CHECK(!std::memcmp(host.data() + ay, c.y.data() + size_t(s) * c.y_bytes(), c.y_bytes()) &&
                      !std::memcmp(host.data() + auv, c.uv.data() + size_t(s) * c.uv_bytes(), c.uv_bytes()),
                  pk + " reference surface " + std::to_string(s) + " changed");
    }
    std::memcpy(c.y.data() + size_t(c.target) * c.y_bytes(), host.data() + o.y + size_t(c.target) * o.sy, c.y_bytes());
    std::memcpy(c.uv.data() + size_t(c.target) * c.uv_bytes(), host.data() + o.uv + size_t(c.target) * o.suv, c.uv_bytes());
  }
}

py::list run_many(const std::vector<py::dict>& pics, int device) {
  VEP_CHECK(device >= -1, "recon records: device must be -1 (CPU) or a GPU index");
  std::vector<ReconCase> cs;
  for (const py::dict& p : pics) {
    cs.push_back(make_case(p));
    avc::validate(picture_of(cs.back()));
  }
  if (!cs.empty()) {
    if (device < 0) {
      for (ReconCase& c : cs) run_cpu(c);
    } else {
      py::gil_scoped_release rel;
      run_gpu(cs, device);
    }
  }
  py::list out;
  for (const ReconCase& c : cs) out.append(case_out(c));
  return out;
}

}  // namespace

void bind_recon(py::module_& m) {
  // One picture: the keyword arguments are the keys of a picture dict of avc_recon_records_many.
  //   y / uv     (slots, 16 hmbs, 16 wmbs) / (slots, 8 or 16 hmbs, 16 wmbs) uint8 or uint16: the DPB
  //   recs       dict of per-MB arrays: kind, flags, slice, ref (4), ref1 (4), mv, i16_mode,
  //              chroma_mode, i4 (16: Intra_4x4 mode per raster block, Intra_8x8 in the first 4),
  //              luma_coded, chroma_coded, wp; optional qp, qpc, qpc2, nz
  //   mvs        int16 pool; wps: dict w0, w1, o, lwd (entries x 3 components)
  //   coefs      (MBs, 512) dense coefficients (avc_recon.h "Dense layout") or I_PCM samples
  m.def(
      "avc_recon_records",
      [](const py::kwargs& kw) {
        py::dict p(kw);
        const int device = p.contains("device") ? p["device"].cast<int>() : -1;
        const py::list out = run_many({p}, device);
        return py::object(out[0]);
      });
  // Several pictures, mixed sizes and formats, in ONE launch sequence: one descriptor array,
  // mb_begin as the exclusive prefix of MBs, the wavefront grid sized by the tallest picture.
  m.def("avc_recon_records_many", &run_many, py::arg("pics"), py::arg("device") = -1);
}
