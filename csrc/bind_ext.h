// Entry points of the binding files; bindings.cpp calls them in registration order.
#pragma once
#include <pybind11/pybind11.h>

namespace vep { class Worker; }

void bind_codec(pybind11::module_& m);        // synthetic encoders, CPU decoders
void bind_codec_hooks(pybind11::module_& m);  // _vep.recon, parser and codec test hooks
void bind_worker(pybind11::module_& m);       // Worker, ReplayBench
void bind_worker_serving(pybind11::class_<vep::Worker>& cls);  // Worker's serving reads (vep/serve.cpp)
void bind_ops(pybind11::module_& m);  // ops on host arrays and caller-owned device buffers
void bind_net(pybind11::module_& m);
void bind_mux(pybind11::module_& m);
void bind_hevc(pybind11::module_& m);
void bind_bus(pybind11::module_& m);
void bind_rpc(pybind11::module_& m);
void bind_dbk(pybind11::module_& m);  // loop filter on given records (tests)
void bind_hevc_lf(pybind11::module_& m);  // H.265 loop filters on given records / parser state (tests)
