// pybind11 bindings of the vep native data plane (module `video_edge_ai_proxy_amd._vep`).
// Every call that can block (decode, D2H, network) releases the GIL.
#include <malloc.h>

#include "bind_common.h"
#include "vep/cabac.h"
#include "vep/gpu.h"
#include "vep/hostprof.h"

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

  // registration order: a class before anything whose signature or default mentions it
  bind_codec(m);        // SynthConfig, AccessUnit, encoders, CPU decoders
  bind_codec_hooks(m);  // _vep.recon, parser and codec test hooks
  bind_worker(m);       // Worker (with bind_worker_serving), ReplayBench
  bind_ops(m);          // ops on host arrays and caller-owned device buffers
  bind_net(m);
  bind_mux(m);
  bind_hevc(m);
  bind_bus(m);
  bind_rpc(m);
  bind_dbk(m);
  bind_hevc_lf(m);
}
