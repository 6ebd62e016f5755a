// Bindings of the Worker (lifecycle, cameras, ingest, submit and decode, consumer buffers, stats; its
// serving reads continue in bind_serve.cpp) and of ReplayBench.
#include "bind_common.h"
#include "vep/bench_driver.h"
#include "vep/synth.h"

void bind_worker(py::module_& m) {
  py::class_<Worker> cls(m, "Worker");
  cls
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
             fill_mean_std(mean, stdv, o.mean, o.std, false);
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
           py::arg("idx"), py::arg("err") = false, py::arg("last") = 100);
  bind_worker_serving(cls);  // the serving reads continue the class here (bind_serve.cpp)
  cls
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
}
