#!/usr/bin/env python3
"""Cost of motion detection on the GPU against the only way to get the same answer without it:
pulling every camera's full frame to the host and differencing it there.

--cams static synthetic cameras (--width x --height) live in the ring slots of one worker of one
hub, their background models primed. Every round first decodes one fresh frame per camera
(outside the timed part), so every call evaluates every camera. Then

* in-process, alternating, p50 of --requests after --warmup: ``Hub.motion_many`` over all cameras
  (one kernel launch, only the counts come down) against --cams x ``Hub.latest_frame`` (the full
  frames D2H) plus the numpy oracle's update and summary on the host (tests/motion_oracle.py),
  with the bytes that crossed PCIe either way;
* request -> last byte over loopback HTTP (uvicorn, one keep-alive client) of
  ``/api/v1/process/{name}/motion`` (one evaluation), ``/api/v1/motion`` (the other cameras'
  evaluations in one launch) and ``frame.jpg?width=320`` as the yardstick.

    python tools/bench_motion.py                    # 32 x 1080p on GPU 0
    python tools/bench_motion.py --profile 50       # only 50 motion_many calls: the run to put under
                                                    # rocprofv3 --kernel-trace --stats -- python ...
    python tools/bench_motion.py --cpu --cams 4 --width 320 --height 240   (CPU rehearsal)
"""
from __future__ import annotations

import argparse
import http.client
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def summary(ms: list[float]) -> dict:
    return {"p50_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


class _NoSession:
    def stop(self):
        pass


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=32)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--requests", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--profile", type=int, default=0, help="only this many Hub.motion_many calls (profiler run)")
    ap.add_argument("--no-http", action="store_true")
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline")
    ap.add_argument("--cpu", action="store_true", help="CPU backend (rehearsal; says nothing about the GPU)")
    a = ap.parse_args()

    import motion_oracle as mo

    from video_edge_ai_proxy_amd._native import native
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle
    from video_edge_ai_proxy_amd.server.app import build_app

    if not a.cpu and native.device_count() == 0:
        raise SystemExit("no GPU (use --cpu for a rehearsal)")
    cfg = Config()
    cfg.data_dir = tempfile.mkdtemp(prefix="vep-bench-")
    cfg.gpu.devices = [-1 if a.cpu else a.device]
    cfg.serving.frontends = 0
    app = build_app(cfg, host="127.0.0.1", rest_port=0, grpc_port=0)
    hub = app.hub
    m = cfg.motion
    cols, rows = native.motion_grid(a.width, a.height, m.cell)
    out = {"cams": a.cams, "width": a.width, "height": a.height, "backend": "cpu" if a.cpu else "gpu",
           "cell": m.cell, "grid": [cols, rows], "requests": a.requests}
    try:
        wk = hub.workers[0]
        names, encs, cams = [], [], []
        for k in range(a.cams):
            sc = native.SynthConfig()
            sc.width, sc.height, sc.gop, sc.fps, sc.seed, sc.motion = a.width, a.height, 10, 30, 11 + k, 0.1
            enc = native.SynthH264(sc)
            name = f"bench_cam_{k:02d}"
            cam = wk.add_camera(name, 2)
            assert wk.decode_now(cam, enc.next())
            hub.cameras[name] = CameraHandle(name, 0, cam, "", session=_NoSession())
            names.append(name)
            encs.append(enc)
            cams.append(cam)

        def fresh():
            for cam, enc in zip(cams, encs):
                assert wk.decode_now(cam, enc.next())

        assert not any(r["primed"] for r in hub.motion_many(names).values())  # the models are primed now
        if a.profile:
            for _ in range(a.profile):
                fresh()
                assert all(r["primed"] for r in hub.motion_many(names).values())
            print(json.dumps({"profiled_calls": a.profile}))
            return
        # the host's own models, primed from the same frames
        host_bg = {}
        if not a.no_host:
            for n in names:
                host_bg[n] = mo.update(hub.latest_frame(n, 0)[1], None, m.cell, m.threshold, m.learn_shift)[1]
        gpu_ms, host_ms, agree = [], [], True
        for k in range(a.warmup + a.requests):
            fresh()
            t0 = time.perf_counter()
            got = hub.motion_many(names)
            t1 = time.perf_counter()
            want = {}
            if not a.no_host:
                for n in names:
                    meta, frame = hub.latest_frame(n, 0)
                    counts, host_bg[n] = mo.update(frame, host_bg[n], m.cell, m.threshold, m.learn_shift)
                    want[n] = mo.summarize(counts, a.width, a.height, m.cell, m.cell_percent, m.min_cells)
            t2 = time.perf_counter()
            for n in want:  # (untimed) the two answers are the same answer
                agree = agree and got[n]["changed"] == want[n]["changed"] and got[n]["motion"] == want[n]["motion"]
            if k >= a.warmup:
                gpu_ms.append((t1 - t0) * 1e3)
                host_ms.append((t2 - t1) * 1e3)
        out["motion_many"] = dict(summary(gpu_ms), pcie_bytes=a.cams * (64 + cols * rows * 4))
        if not a.no_host:
            out["latest_frame_plus_numpy_x_cams"] = dict(summary(host_ms), pcie_bytes=a.cams * a.width * a.height * 3)
            out["time_ratio"] = round(statistics.median(host_ms) / statistics.median(gpu_ms), 2)
            out["bytes_ratio"] = round(a.width * a.height * 3 / (64 + cols * rows * 4), 1)
            out["answers_agree"] = agree
        if not a.no_http:
            con = http.client.HTTPConnection("127.0.0.1", app.rest_port, timeout=30)
            for _ in range(100):  # the REST server starts listening on its own thread
                try:
                    con.connect()
                    break
                except ConnectionRefusedError:
                    time.sleep(0.05)
            paths = {"process/{name}/motion": f"/api/v1/process/{names[0]}/motion",
                     "motion": "/api/v1/motion?names=" + ",".join(names),
                     "frame.jpg?width=320": f"/api/v1/process/{names[0]}/frame.jpg?width=320"}
            times = {s: [] for s in paths}
            sizes = {s: 0 for s in paths}
            for k in range(a.warmup + a.requests):
                fresh()  # the first route evaluates one camera, the second the others in one launch
                for s, path in paths.items():
                    t0 = time.perf_counter()
                    con.request("GET", path)
                    r = con.getresponse()
                    body = r.read()
                    dt = (time.perf_counter() - t0) * 1e3
                    assert r.status == 200, (s, r.status, body[:200])
                    if k >= a.warmup:
                        times[s].append(dt)
                        sizes[s] = len(body)
            out["routes"] = {s: dict(summary(times[s]), response_bytes=sizes[s]) for s in paths}
            con.close()
    finally:
        for n in list(hub.cameras):
            if n.startswith("bench_cam_"):
                hub.cameras.pop(n)
        app.stop()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
