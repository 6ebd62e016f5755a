// Test-only entry points: the H.265 loop filters alone, on caller-supplied inputs.
//
// hevc_loopfilter_records runs deblocking and SAO on the loop-filter fields of a GpuPicture built
// from numpy arrays: hevc::cpu_execute on a picture without prediction / transform records
// (device -1), or, on a GPU, one HevcDesc per picture built as the runtime builds it and the
// runtime's launch sequence, once for the whole list. hevc_loopfilter_picture fills a PicCtx
// (the state the CTU parser leaves behind) and runs the host rules: deblock_strengths and
// finish_gpu_picture ("strengths"), the CPU decoder's deblock_picture + sao_picture ("cpu"), or
// finish_gpu_picture followed by the records layer ("records").
//
// Everything the kernels index with is validated first (ValueError, picture and block named).
// On a GPU the planes and the SAO scratch live between guard bands that must come back intact,
// like every input map; a non-zero error word raises.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "bind_ext.h"
#include "vep/codec.h"
#include "vep/gpu.h"
#include "vep/hevc_ctu.h"

namespace py = pybind11;
using namespace vep;
using hevc::i8;

namespace {

constexpr int kMaxSide = 8192;  // 512 macroblocks, the surfaces' limit

struct LfCase {
  hevc::GpuPicture g;
  int stride = 0;
  std::vector<u8> y, uv;  // plane bytes (u16 samples above 8 bits), `height` rows of `stride`
  size_t bps() const { return g.wide() ? 2 : 1; }
};

[[noreturn]] void bad(size_t pic, const std::string& msg) {
  throw py::value_error("hevc loop filter: picture " + std::to_string(pic) + ": " + msg);
}

using IntArr = py::array_t<long long, py::array::c_style | py::array::forcecast>;

py::object need(const py::dict& d, const char* k, size_t pic) {
  if (!d.contains(k)) bad(pic, std::string("missing field ") + k);
  return d[k];
}

long long geti(const py::dict& d, const char* k, size_t pic) {
  try {
    return need(d, k, pic).cast<long long>();
  } catch (const py::cast_error&) {
    bad(pic, std::string("field ") + k + " is not an integer");
  }
}

IntArr arr(const py::dict& d, const char* k, size_t n, size_t pic) {
  IntArr a = IntArr::ensure(need(d, k, pic));
  if (!a || size_t(a.size()) != n)
    bad(pic, std::string("field ") + k + " must hold " + std::to_string(n) + " integers");
  return a;
}

// values of `a` into `out`, each within [lo, hi]
template <class T>
void take(const IntArr& a, const char* k, long long lo, long long hi, const char* unit, size_t pic, std::vector<T>& out) {
  out.resize(size_t(a.size()));
  for (size_t i = 0; i < out.size(); ++i) {
    const long long v = a.data()[i];
    if (v < lo || v > hi)
      bad(pic, std::string(k) + " = " + std::to_string(v) + " out of range at " + unit + " " + std::to_string(i));
    out[i] = T(v);
  }
}

void geometry(const py::dict& d, size_t pic, int& w, int& h, int& log2ctb, int& bd_y, int& bd_c) {
  const long long W = geti(d, "width", pic), H = geti(d, "height", pic), L = geti(d, "log2ctb", pic);
  const long long by = geti(d, "bd_y", pic), bc = geti(d, "bd_c", pic);
  if (W < 8 || H < 8 || W > kMaxSide || H > kMaxSide || (W & 7) || (H & 7))
    bad(pic, "width / height must be multiples of 8 within 8.." + std::to_string(kMaxSide));
  if (L < 4 || L > 6) bad(pic, "log2ctb must be 4..6");
  if (by < 8 || by > 10 || by != bc) bad(pic, "bd_y must be 8..10 and equal bd_c");
  w = int(W);
  h = int(H);
  log2ctb = int(L);
  bd_y = int(by);
  bd_c = int(bc);
}

void load_plane(const py::dict& d, const char* k, bool wide, int bd, size_t rows, size_t pitch, size_t pic,
                std::vector<u8>& out) {
  py::array a = py::array::ensure(need(d, k, pic), py::array::c_style);
  if (!a || !a.dtype().is(wide ? py::dtype::of<u16>() : py::dtype::of<u8>()))
    bad(pic, std::string(k) + " plane must be a " + (wide ? "uint16" : "uint8") + " array");
  if (a.ndim() != 2 || size_t(a.shape(0)) != rows || size_t(a.shape(1)) != pitch)
    bad(pic, std::string(k) + " plane must be " + std::to_string(rows) + " x " + std::to_string(pitch));
  out.resize(rows * pitch * (wide ? 2 : 1));
  std::memcpy(out.data(), a.data(), out.size());
  if (wide) {
    const u16* s = reinterpret_cast<const u16*>(out.data());
    for (size_t i = 0; i < rows * pitch; ++i)
      if (s[i] >= (1u << bd)) bad(pic, std::string(k) + " sample above the bit depth at index " + std::to_string(i));
  }
}

void load_planes(const py::dict& d, size_t pic, LfCase& c) {
  c.stride = (c.g.width + 15) / 16 * 16;
  load_plane(d, "y", c.g.wide(), c.g.bd_y, size_t(c.g.height), size_t(c.stride), pic, c.y);
  load_plane(d, "uv", c.g.wide(), c.g.bd_c, size_t(c.g.height) / 2, size_t(c.stride), pic, c.uv);
}

std::vector<hevc::GpuSao> load_sao(const py::object& o, size_t nctb, int bd, size_t pic) {
  py::list l;
  try {
    l = o.cast<py::list>();
  } catch (const py::cast_error&) {
    bad(pic, "the SAO parameters must be a list");
  }
  if (l.size() != nctb) bad(pic, "the SAO parameters must hold one entry per CTB");
  const int lim = (1 << (std::min(bd, 10) - 5)) - 1;
  std::vector<hevc::GpuSao> out(nctb);
  for (size_t k = 0; k < nctb; ++k) {
    const py::dict s = l[k].cast<py::dict>();
    const IntArr type = arr(s, "type", 3, pic), band = arr(s, "band", 3, pic), eo = arr(s, "eo", 3, pic),
                 off = arr(s, "off", 12, pic);
    const std::string at = " at CTB " + std::to_string(k);
    for (int c = 0; c < 3; ++c) {
      if (type.data()[c] < 0 || type.data()[c] > 2) bad(pic, "SAO type above 2" + at);
      if (eo.data()[c] < 0 || eo.data()[c] > 3) bad(pic, "SAO eo above 3" + at);
      if (band.data()[c] < 0 || band.data()[c] > 31) bad(pic, "SAO band above 31" + at);
      out[k].type[c] = u8(type.data()[c]);
      out[k].eo[c] = u8(eo.data()[c]);
      out[k].band[c] = u8(band.data()[c]);
      for (int i = 0; i < 4; ++i) {
        const long long v = off.data()[c * 4 + i];
        if (v < -lim || v > lim) bad(pic, "SAO offset outside +-" + std::to_string(lim) + at);
        out[k].off[c][i] = i8(v);
      }
    }
  }
  return out;
}

// What the kernels index with, on a finished GpuPicture (either layer ends here).
void validate(const hevc::GpuPicture& g, size_t pic) {
  const size_t n4 = size_t(g.w4()) * size_t(g.h4()), nctb = size_t(g.wctb) * size_t(g.hctb);
  if (g.qp.size() != n4 || g.pcm_map.size() != n4) bad(pic, "qp / pcm_map must hold one entry per 4x4 block");
  if (g.deblock && (g.bs_v.size() != n4 || g.bs_h.size() != n4)) bad(pic, "bs_v / bs_h must hold one entry per 4x4 block");
  if (g.ctb_slice.size() != nctb || g.ctb_tile.size() != nctb || g.sao_params.size() != nctb)
    bad(pic, "ctb_slice / ctb_tile / sao_params must hold one entry per CTB");
  if (g.slices.empty()) bad(pic, "no slice");
  for (size_t k = 0; k < nctb; ++k) {
    if (g.ctb_slice[k] >= g.slices.size()) bad(pic, "ctb_slice names no slice at CTB " + std::to_string(k));
    if (g.ctb_tile[k] >= nctb) bad(pic, "ctb_tile above the CTB count at CTB " + std::to_string(k));
  }
  const int qlo = -6 * (g.bd_y - 8);
  for (size_t k = 0; k < n4; ++k)
    if (g.qp[k] < qlo || g.qp[k] > 51) bad(pic, "qp out of range at block " + std::to_string(k));
  if (!g.deblock) return;
  for (int dir = 0; dir < 2; ++dir) {
    const std::vector<u8>& bs = dir == 0 ? g.bs_v : g.bs_h;
    for (size_t k = 0; k < n4; ++k) {
      if (!bs[k]) continue;
      const std::string at = std::string(dir == 0 ? "bs_v" : "bs_h") + " at block " + std::to_string(k);
      if (bs[k] > 2) bad(pic, at + " above 2");
      // the kernel reads 4 samples before the edge, one thread per segment of the 8x8 grid
      const int pos = 4 * int(dir == 0 ? k % size_t(g.w4()) : k / size_t(g.w4()));
      if (pos == 0 || (pos & 7)) bad(pic, at + " is off the 8x8 grid or on the picture border");
    }
  }
}

LfCase records_case(const py::dict& d, size_t pic) {
  LfCase c;
  hevc::GpuPicture& g = c.g;
  geometry(d, pic, g.width, g.height, g.log2ctb, g.bd_y, g.bd_c);
  g.wctb = (g.width + (1 << g.log2ctb) - 1) >> g.log2ctb;
  g.hctb = (g.height + (1 << g.log2ctb) - 1) >> g.log2ctb;
  g.target = 0;
  const long long cb = geti(d, "cb_qp_offset", pic), cr = geti(d, "cr_qp_offset", pic);
  if (cb < -12 || cb > 12 || cr < -12 || cr > 12) bad(pic, "cb / cr qp offset outside +-12");
  g.cb_qp_offset = int(cb);
  g.cr_qp_offset = int(cr);
  g.deblock = geti(d, "deblock", pic) != 0;
  g.sao = geti(d, "sao", pic) != 0;
  g.pcm_nofilter = geti(d, "pcm_nofilter", pic) != 0;
  g.tiles_block_sao = geti(d, "tiles_block_sao", pic) != 0;
  const size_t n4 = size_t(g.w4()) * size_t(g.h4()), nctb = size_t(g.wctb) * size_t(g.hctb);
  take(arr(d, "bs_v", n4, pic), "bs_v", 0, 255, "block", pic, g.bs_v);
  take(arr(d, "bs_h", n4, pic), "bs_h", 0, 255, "block", pic, g.bs_h);
  take(arr(d, "qp", n4, pic), "qp", -128, 127, "block", pic, g.qp);
  take(arr(d, "pcm_map", n4, pic), "pcm_map", 0, 1, "block", pic, g.pcm_map);
  take(arr(d, "ctb_slice", nctb, pic), "ctb_slice", 0, 0xFFFF, "CTB", pic, g.ctb_slice);
  take(arr(d, "ctb_tile", nctb, pic), "ctb_tile", 0, 0xFFFF, "CTB", pic, g.ctb_tile);
  py::list sl;
  try {
    sl = need(d, "slices", pic).cast<py::list>();
  } catch (const py::cast_error&) {
    bad(pic, "slices must be a list");
  }
  for (size_t k = 0; k < sl.size(); ++k) {
    const py::dict s = sl[k].cast<py::dict>();
    const long long bo = geti(s, "beta_offset", pic), to = geti(s, "tc_offset", pic);
    if (bo < -12 || bo > 12 || to < -12 || to > 12 || (bo & 1) || (to & 1))
      bad(pic, "beta / tc offset must be even and within +-12 in slice " + std::to_string(k));
    hevc::GpuSlice gs{};
    gs.beta_offset = i8(bo);
    gs.tc_offset = i8(to);
    gs.across = u8(geti(s, "across", pic) != 0);
    gs.sao_luma = u8(geti(s, "sao_luma", pic) != 0);
    gs.sao_chroma = u8(geti(s, "sao_chroma", pic) != 0);
    g.slices.push_back(gs);
  }
  g.sao_params = load_sao(need(d, "sao_params", pic), nctb, g.bd_y, pic);
  validate(g, pic);
  load_planes(d, pic, c);
  return c;
}

py::array plane_out(const std::vector<u8>& bytes, bool wide, size_t rows, size_t pitch) {
  if (wide) {
    py::array_t<u16> a({rows, pitch});
    std::memcpy(a.mutable_data(), bytes.data(), bytes.size());
    return std::move(a);
  }
  py::array_t<u8> a({rows, pitch});
  std::memcpy(a.mutable_data(), bytes.data(), bytes.size());
  return std::move(a);
}

py::tuple case_out(const LfCase& c) {
  return py::make_tuple(plane_out(c.y, c.g.wide(), size_t(c.g.height), size_t(c.stride)),
                        plane_out(c.uv, c.g.wide(), size_t(c.g.height) / 2, size_t(c.stride)));
}

void surface_in(const LfCase& c, HostSurface& s) {
  s.alloc(c.stride, c.g.height, c.g.bd_y);
  if (s.wide()) {
    std::memcpy(s.y16.data(), c.y.data(), c.y.size());
    std::memcpy(s.uv16.data(), c.uv.data(), c.uv.size());
  } else {
    std::memcpy(s.y.data(), c.y.data(), c.y.size());
    std::memcpy(s.uv.data(), c.uv.data(), c.uv.size());
  }
}

void surface_out(const HostSurface& s, LfCase& c) {
  if (s.wide()) {
    std::memcpy(c.y.data(), s.y16.data(), c.y.size());
    std::memcpy(c.uv.data(), s.uv16.data(), c.uv.size());
  } else {
    std::memcpy(c.y.data(), s.y.data(), c.y.size());
    std::memcpy(c.uv.data(), s.uv.data(), c.uv.size());
  }
}

void run_cpu(LfCase& c) {
  std::vector<HostSurface> slots(1);
  surface_in(c, slots[0]);
  hevc::cpu_execute(c.g, slots);
  surface_out(slots[0], c);
}

constexpr size_t kGuard = 1024;  // bytes of kGuardByte around every plane and scratch plane
constexpr u8 kGuardByte = 0xA5;

// One device allocation for the batch: descriptors, then per picture its maps and, for luma and
// for chroma, guard | plane | guard | SAO scratch | guard (the scratch is the slot after the
// target, as in the camera surfaces: slot size = plane + guard), then an error word per picture.
void run_gpu(std::vector<LfCase>& cs, int device) {
  int ndev = 0;
  VEP_CHECK(hipGetDeviceCount(&ndev) == hipSuccess && device < ndev, "hevc loop filter: no such GPU");
  VEP_HIP(hipSetDevice(device));
  const size_t n = cs.size();
  struct Off {
    size_t bsv, bsh, qp, map, cslice, ctile, slices, sao, y, uv, slot_y, slot_uv;
  };
  std::vector<Off> off(n);
  size_t top = 0;
  auto take_bytes = [&](size_t bytes) {
    const size_t at = top;
    top += (std::max<size_t>(bytes, 1) + 255) & ~size_t(255);
    return at;
  };
  auto vec_bytes = [](const auto& v) { return v.size() * sizeof(v[0]); };
  const size_t off_desc = take_bytes(n * sizeof(gpu::HevcDesc));
  for (size_t k = 0; k < n; ++k) {
    const LfCase& c = cs[k];
    const hevc::GpuPicture& g = c.g;
    off[k].bsv = take_bytes(vec_bytes(g.bs_v));
    off[k].bsh = take_bytes(vec_bytes(g.bs_h));
    off[k].qp = take_bytes(vec_bytes(g.qp));
    off[k].map = take_bytes(vec_bytes(g.pcm_map));
    off[k].cslice = take_bytes(vec_bytes(g.ctb_slice));
    off[k].ctile = take_bytes(vec_bytes(g.ctb_tile));
    off[k].slices = take_bytes(vec_bytes(g.slices));
    off[k].sao = take_bytes(vec_bytes(g.sao_params));
    take_bytes(kGuard);
    off[k].y = take_bytes(c.y.size());
    take_bytes(kGuard);
    off[k].slot_y = top - off[k].y;
    take_bytes(c.y.size());
    take_bytes(kGuard);
    off[k].uv = take_bytes(c.uv.size());
    take_bytes(kGuard);
    off[k].slot_uv = top - off[k].uv;
    take_bytes(c.uv.size());
    take_bytes(kGuard);
  }
  const size_t off_err = take_bytes(n * sizeof(u32));
  std::vector<u8> host(top, kGuardByte);
  std::memset(host.data() + off_err, 0, n * sizeof(u32));
  u8* dev = nullptr;
  VEP_HIP(hipMalloc(reinterpret_cast<void**>(&dev), top));
  auto put = [&](size_t at, const auto& v) {
    if (!v.empty()) std::memcpy(host.data() + at, v.data(), v.size() * sizeof(v[0]));
  };
  int blks = 0;
  bool dbk = false, sao = false;
  auto* descs = reinterpret_cast<gpu::HevcDesc*>(host.data() + off_desc);
  for (size_t k = 0; k < n; ++k) {
    const LfCase& c = cs[k];
    const hevc::GpuPicture& p = c.g;
    put(off[k].bsv, p.bs_v);
    put(off[k].bsh, p.bs_h);
    put(off[k].qp, p.qp);
    put(off[k].map, p.pcm_map);
    put(off[k].cslice, p.ctb_slice);
    put(off[k].ctile, p.ctb_tile);
    put(off[k].slices, p.slices);
    put(off[k].sao, p.sao_params);
    put(off[k].y, c.y);
    put(off[k].uv, c.uv);
    gpu::HevcDesc g{};
    g.y = dev + off[k].y;
    g.uv = dev + off[k].uv;
    g.slot_y = off[k].slot_y;
    g.slot_uv = off[k].slot_uv;
    g.stride = c.stride;
    g.width = p.width;
    g.height = p.height;
    g.log2ctb = p.log2ctb;
    g.wctb = p.wctb;
    g.hctb = p.hctb;
    g.target = p.target;
    g.cb_qp_offset = p.cb_qp_offset;
    g.cr_qp_offset = p.cr_qp_offset;
    g.flags = (p.deblock ? 1 : 0) | (p.sao ? 2 : 0) | (p.pcm_nofilter ? 4 : 0) | (p.tiles_block_sao ? 8 : 0) |
              (p.wide() ? gpu::kHevcWide : 0);
    g.bd_y = p.bd_y;
    g.bd_c = p.bd_c;
    g.bs_v = dev + off[k].bsv;
    g.bs_h = dev + off[k].bsh;
    g.qp = reinterpret_cast<const signed char*>(dev + off[k].qp);
    g.pcm_map = dev + off[k].map;
    g.ctb_slice = reinterpret_cast<const u16*>(dev + off[k].cslice);
    g.slices = dev + off[k].slices;
    g.sao = dev + off[k].sao;
    g.ctb_tile = reinterpret_cast<const u16*>(dev + off[k].ctile);
    g.sao_y = g.y + 1 * g.slot_y;  // the extra surface after the (one) picture slot
    g.sao_uv = g.uv + 1 * g.slot_uv;
    g.err = reinterpret_cast<u32*>(dev + off_err) + k;
    g.npu = 0;
    g.pu_begin = 0;
    g.blk_begin = blks;
    descs[k] = g;
    blks += p.w4() * p.h4();
    dbk |= p.deblock;
    sao |= p.sao;
  }
  const std::vector<u8> sent = host;
  try {
    const hipStream_t s = nullptr;
    VEP_HIP(hipMemcpyAsync(dev, host.data(), top, hipMemcpyHostToDevice, s));
    const auto* dd = reinterpret_cast<const gpu::HevcDesc*>(dev + off_desc);
    if (dbk) {
      gpu::launch_hevc_deblock(dd, int(n), blks, 0, s);
      gpu::launch_hevc_deblock(dd, int(n), blks, 1, s);
    }
    if (sao) gpu::launch_hevc_sao(dd, int(n), blks, s);
    VEP_HIP(hipGetLastError());
    VEP_HIP(hipStreamSynchronize(s));
    VEP_HIP(hipMemcpy(host.data(), dev, top, hipMemcpyDeviceToHost));
  } catch (...) {
    (void)hipFree(dev);
    throw;
  }
  (void)hipFree(dev);
  const u32* err = reinterpret_cast<const u32*>(host.data() + off_err);
  // everything but the planes and the scratch of SAO pictures comes back as it was sent: the
  // guard bands, the padding up to each 256-byte boundary, the maps and the descriptors
  std::vector<u8> may_change(top, 0);
  for (size_t k = 0; k < n; ++k) {
    const LfCase& c = cs[k];
    std::fill_n(may_change.begin() + long(off[k].y), c.y.size(), u8(1));
    std::fill_n(may_change.begin() + long(off[k].uv), c.uv.size(), u8(1));
    if (c.g.sao) {
      std::fill_n(may_change.begin() + long(off[k].y + off[k].slot_y), c.y.size(), u8(1));
      std::fill_n(may_change.begin() + long(off[k].uv + off[k].slot_uv), c.uv.size(), u8(1));
    }
  }
  for (size_t k = 0; k < n; ++k)
    VEP_CHECK(err[k] == 0, "hevc loop filter: picture " + std::to_string(k) + " error word " + std::to_string(err[k]));
  for (size_t i = 0; i < top; ++i)
    VEP_CHECK(may_change[i] || host[i] == sent[i],
              "hevc loop filter: byte " + std::to_string(i) + " outside the planes written (guard band or input map)");
  for (size_t k = 0; k < n; ++k) {
    std::memcpy(cs[k].y.data(), host.data() + off[k].y, cs[k].y.size());
    std::memcpy(cs[k].uv.data(), host.data() + off[k].uv, cs[k].uv.size());
  }
}

// ---------------------------------------------------------------------------- host rules
// The parser's state of one picture. The PicCtx points into the object: it does not move.
struct PicState {
  hevc::Sps sps;
  hevc::Pps pps;
  HostSurface surf;
  hevc::PicCtx pc;
  hevc::GpuPicture g;
  std::map<long long, hevc::FramePtr> frames;
  PicState() = default;
  PicState(const PicState&) = delete;
  PicState& operator=(const PicState&) = delete;
};

void picture_state(const py::dict& d, PicState& st, LfCase& c) {
  const size_t pic = 0;
  int w, h, log2ctb, bd_y, bd_c;
  geometry(d, pic, w, h, log2ctb, bd_y, bd_c);
  hevc::Sps& sps = st.sps;
  hevc::Pps& pps = st.pps;
  sps.width = w;
  sps.height = h;
  sps.log2_ctb = log2ctb;
  sps.log2_min_cb = 3;
  sps.bit_depth_luma = bd_y;
  sps.bit_depth_chroma = bd_c;
  sps.pcm_loop_filter_disabled = geti(d, "pcm_loop_filter_disabled", pic) != 0;
  pps.transquant_bypass = geti(d, "transquant_bypass", pic) != 0;
  const long long cb = geti(d, "cb_qp_offset", pic), cr = geti(d, "cr_qp_offset", pic);
  if (cb < -12 || cb > 12 || cr < -12 || cr > 12) bad(pic, "cb / cr qp offset outside +-12");
  pps.cb_qp_offset = int(cb);
  pps.cr_qp_offset = int(cr);
  pps.loop_filter_across_tiles = geti(d, "across_tiles", pic) != 0;
  const int wctb = sps.width_ctbs(), hctb = sps.height_ctbs();
  const long long tcols = geti(d, "tile_cols", pic), trows = geti(d, "tile_rows", pic);
  if (tcols < 1 || tcols > wctb || trows < 1 || trows > hctb) bad(pic, "tile_cols / tile_rows outside the CTB grid");
  pps.tile_cols = int(tcols);
  pps.tile_rows = int(trows);
  pps.tiles = tcols > 1 || trows > 1;
  pps.uniform_spacing = geti(d, "uniform_spacing", pic) != 0;
  if (pps.tiles && !pps.uniform_spacing) {
    auto sizes = [&](const char* k, int count, int total, std::vector<int>& out) {
      const IntArr a = arr(d, k, size_t(count - 1), pic);
      long long sum = 0;
      for (int i = 0; i < count - 1; ++i) {
        if (a.data()[i] < 1) bad(pic, std::string(k) + " holds an empty tile");
        sum += a.data()[i];
        out.push_back(int(a.data()[i]));
      }
      if (sum >= total) bad(pic, std::string(k) + " does not fit the picture");
    };
    sizes("col_width", pps.tile_cols, wctb, pps.col_width);
    sizes("row_height", pps.tile_rows, hctb, pps.row_height);
  }
  c.g.width = w;
  c.g.height = h;
  c.g.bd_y = bd_y;
  c.g.bd_c = bd_c;
  load_planes(d, pic, c);
  surface_in(c, st.surf);
  hevc::PicCtx& pc = st.pc;
  pc.init(sps, pps, &st.surf);
  const size_t n4 = size_t(pc.w4) * size_t(pc.h4), nctb = size_t(wctb) * size_t(hctb);
  take(arr(d, "intra", n4, pic), "intra", 0, 1, "block", pic, pc.intra);
  take(arr(d, "cbf", n4, pic), "cbf", 0, 1, "block", pic, pc.cbf);
  take(arr(d, "edge", n4, pic), "edge", 0, 15, "block", pic, pc.edge);
  take(arr(d, "pcm", n4, pic), "pcm", 0, 1, "block", pic, pc.pcm);
  take(arr(d, "qp", n4, pic), "qp", -6 * (bd_y - 8), 51, "block", pic, pc.qp);
  {
    std::vector<u8> bypass;
    take(arr(d, "bypass", n4, pic), "bypass", 0, 1, "block", pic, bypass);
    for (size_t k = 0; k < n4; ++k)
      if (bypass[k]) {
        if (!pps.transquant_bypass) bad(pic, "bypass block without transquant_bypass at block " + std::to_string(k));
        pc.any_bypass = true;
      }
    if (pps.transquant_bypass) pc.bypass = bypass;
  }
  // slices: one SliceInfo per segment; reference lists as picture ids, one frame per id
  py::list sl;
  try {
    sl = need(d, "slices", pic).cast<py::list>();
  } catch (const py::cast_error&) {
    bad(pic, "slices must be a list");
  }
  if (sl.empty() || sl.size() > 0xFFFE) bad(pic, "no slice");
  int ords = 0;
  for (size_t k = 0; k < sl.size(); ++k) {
    const py::dict s = sl[k].cast<py::dict>();
    hevc::SliceInfo si;
    const long long ord = geti(s, "ord", pic);
    if (ord != ords && ord != ords - 1) bad(pic, "slice ordinals must count up from 0 in slice " + std::to_string(k));
    if (ord == ords) ++ords;
    else si.sh.dependent = true;
    si.ord = int(ord);
    const long long bo = geti(s, "beta_offset_div2", pic), to = geti(s, "tc_offset_div2", pic);
    if (bo < -6 || bo > 6 || to < -6 || to > 6) bad(pic, "beta / tc offset_div2 outside +-6 in slice " + std::to_string(k));
    si.sh.beta_offset = int(bo) * 2;
    si.sh.tc_offset = int(to) * 2;
    si.sh.deblocking_disabled = geti(s, "deblocking_disabled", pic) != 0;
    si.sh.loop_filter_across_slices = geti(s, "across_slices", pic) != 0;
    si.sh.sao_luma = geti(s, "sao_luma", pic) != 0;
    si.sh.sao_chroma = geti(s, "sao_chroma", pic) != 0;
    const py::sequence lists = need(s, "ref_lists", pic).cast<py::sequence>();
    if (lists.size() != 2) bad(pic, "ref_lists must hold two lists in slice " + std::to_string(k));
    for (int l = 0; l < 2; ++l) {
      const std::vector<long long> ids = lists[size_t(l)].cast<std::vector<long long>>();
      if (ids.size() > 16) bad(pic, "more than 16 reference pictures in slice " + std::to_string(k));
      for (long long id : ids) {
        hevc::FramePtr& f = st.frames[id];
        if (!f) {
          f = std::make_shared<hevc::HevcFrame>();
          f->poc = int(id);
        }
        si.list[l].push_back(f);
        si.list_poc[l].push_back(int(id));
        si.list_lt[l].push_back(0);
      }
    }
    pc.slices.push_back(std::move(si));
  }
  take(arr(d, "ctb_slice", nctb, pic), "ctb_slice", 0, (long long)sl.size() - 1, "CTB", pic, pc.slice);
  take(arr(d, "ctb_sord", nctb, pic), "ctb_sord", 0, ords - 1, "CTB", pic, pc.sord);
  for (size_t k = 0; k < nctb; ++k)
    if (pc.slices[pc.slice[k]].ord != int(pc.sord[k])) bad(pic, "ctb_sord differs from the segment's ordinal at CTB " + std::to_string(k));
  // motion: unused lists stay at the parser's defaults (ref -1, mv 0)
  const IntArr pred = arr(d, "mf_pred", n4, pic), ref = arr(d, "mf_ref", n4 * 2, pic), mv = arr(d, "mf_mv", n4 * 4, pic);
  for (size_t k = 0; k < n4; ++k) {
    const std::string at = " at block " + std::to_string(k);
    hevc::MvField m;
    const long long p = pred.data()[k];
    if (p < 0 || p > 3) bad(pic, "mf_pred above 3" + at);
    if (!p != bool(pc.intra[k])) bad(pic, "a block is intra exactly when it has no motion" + at);
    m.pred = u8(p);
    const size_t ctb = size_t(((int(k) / pc.w4 * 4) >> log2ctb) * wctb + ((int(k) % pc.w4 * 4) >> log2ctb));
    const hevc::SliceInfo& si = pc.slices[pc.slice[ctb]];
    for (int l = 0; l < 2; ++l) {
      if (!((p >> l) & 1)) continue;
      const long long r = ref.data()[k * 2 + size_t(l)];
      if (r < 0 || r >= (long long)si.list[l].size()) bad(pic, "mf_ref outside the slice's reference list" + at);
      m.ref[l] = i8(r);
      for (int i = 0; i < 2; ++i) {
        const long long v = mv.data()[k * 4 + size_t(l) * 2 + size_t(i)];
        if (v < -32768 || v > 32767) bad(pic, "mf_mv outside 16 bits" + at);
        m.mv[l][i] = i16(v);
      }
    }
    pc.mf[k] = m;
  }
  {
    const std::vector<hevc::GpuSao> sao = load_sao(need(d, "sao", pic), nctb, bd_y, pic);
    for (size_t k = 0; k < nctb; ++k)
      for (int cc = 0; cc < 3; ++cc) {
        pc.sao[k].type[cc] = sao[k].type[cc];
        pc.sao[k].band[cc] = sao[k].band[cc];
        pc.sao[k].eo[cc] = sao[k].eo[cc];
        for (int i = 0; i < 4; ++i) pc.sao[k].off[cc][i] = sao[k].off[cc][i];
      }
  }
  pc.multi = pc.multi || ords > 1;
}

py::dict records_out(const hevc::GpuPicture& g) {
  py::dict o;
  auto ints = [](const auto& v) {
    py::list l;
    for (auto x : v) l.append(int(x));
    return l;
  };
  o["bs_v"] = ints(g.bs_v);
  o["bs_h"] = ints(g.bs_h);
  o["qp"] = ints(g.qp);
  o["pcm_map"] = ints(g.pcm_map);
  o["ctb_slice"] = ints(g.ctb_slice);
  o["ctb_tile"] = ints(g.ctb_tile);
  py::list sl;
  for (const hevc::GpuSlice& s : g.slices) {
    py::dict e;
    e["beta_offset"] = int(s.beta_offset);
    e["tc_offset"] = int(s.tc_offset);
    e["across"] = int(s.across);
    e["sao_luma"] = int(s.sao_luma);
    e["sao_chroma"] = int(s.sao_chroma);
    sl.append(e);
  }
  o["slices"] = sl;
  py::list sao;
  for (const hevc::GpuSao& s : g.sao_params) {
    py::dict e;
    py::list type, band, eo, off;
    for (int c = 0; c < 3; ++c) {
      type.append(int(s.type[c]));
      band.append(int(s.band[c]));
      eo.append(int(s.eo[c]));
      py::list oc;
      for (int i = 0; i < 4; ++i) oc.append(int(s.off[c][i]));
      off.append(oc);
    }
    e["type"] = type;
    e["band"] = band;
    e["eo"] = eo;
    e["off"] = off;
    sao.append(e);
  }
  o["sao_params"] = sao;
  o["deblock"] = g.deblock;
  o["sao"] = g.sao;
  o["pcm_nofilter"] = g.pcm_nofilter;
  o["tiles_block_sao"] = g.tiles_block_sao;
  return o;
}

}  // namespace

void bind_hevc_lf(py::module_& m) {
  m.def(
      "hevc_loopfilter_records",
      [](const std::vector<py::dict>& pictures, int device) {
        if (device < -1) throw py::value_error("hevc loop filter: device must be -1 (CPU) or a GPU index");
        std::vector<LfCase> cs;
        for (size_t k = 0; k < pictures.size(); ++k) cs.push_back(records_case(pictures[k], k));
        if (!cs.empty()) {
          if (device < 0) {
            for (LfCase& c : cs) run_cpu(c);
          } else {
            py::gil_scoped_release rel;
            run_gpu(cs, device);
          }
        }
        py::list out;
        for (const LfCase& c : cs) out.append(case_out(c));
        return out;
      },
      py::arg("pictures"), py::arg("device") = -1);
  m.def(
      "hevc_loopfilter_picture",
      [](const py::dict& pic, int device, const std::string& path) -> py::object {
        if (device < -1) throw py::value_error("hevc loop filter: device must be -1 (CPU) or a GPU index");
        if (path != "strengths" && path != "cpu" && path != "records")
          throw py::value_error("hevc loop filter: path must be strengths, cpu or records");
        PicState st;
        LfCase c;
        picture_state(pic, st, c);
        hevc::PicCtx& pc = st.pc;
        if (path == "cpu") {
          bool deblock = false, sao = false;
          for (const hevc::SliceInfo& s : pc.slices) {
            deblock |= !s.sh.deblocking_disabled;
            sao |= s.sh.sao_luma || s.sh.sao_chroma;
          }
          if (deblock) hevc::deblock_picture(pc);
          if (sao) hevc::sao_picture(pc);
          surface_out(st.surf, c);
          return case_out(c);
        }
        pc.init_gpu(&c.g);
        hevc::finish_gpu_picture(pc);
        if (path == "strengths") {
          py::dict o = records_out(c.g);
          std::vector<u8> bsv, bsh;
          hevc::deblock_strengths(pc, bsv, bsh);
          py::list v, h;
          for (u8 x : bsv) v.append(int(x));
          for (u8 x : bsh) h.append(int(x));
          o["bs_v"] = v;
          o["bs_h"] = h;
          return std::move(o);
        }
        validate(c.g, 0);
        std::vector<LfCase> cs;
        cs.push_back(std::move(c));
        if (device < 0) run_cpu(cs[0]);
        else {
          py::gil_scoped_release rel;
          run_gpu(cs, device);
        }
        return case_out(cs[0]);
      },
      py::arg("pic"), py::arg("device") = -1, py::arg("path") = "strengths");
}
