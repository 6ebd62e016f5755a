#!/usr/bin/env python3
"""Latency of the REST frame routes, request -> last byte: ``/frame`` (raw PPM) against
``/frame.jpg`` (JPEG encoded on the GPU), on one live camera of one hub.

An in-process loopback RTSP farm feeds one camera (--width x --height at --fps); the hub serves
REST on a loopback port (uvicorn, as ``vep serve`` does); one keep-alive HTTP client then sends
--requests requests to every route in --routes, alternating between the routes, after --warmup
unmeasured ones. Reported per route: p50 / min / max milliseconds, response bytes and the bytes
the request copies from the device.

The encode paths are also timed in-process (no HTTP): ``Hub.latest_jpeg`` (on a GPU: kernels +
the compressed bytes' copy) against copying the raw frame and encoding it with the CPU encoder.

    python tools/bench_frame_jpg.py                       # 1080p, GPU 0
    python tools/bench_frame_jpg.py --routes frame        # a tree without frame.jpg
    python tools/bench_frame_jpg.py --cpu --width 320 --height 240   (CPU backend rehearsal)
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


def summary(ms: list[float]) -> dict:
    return {"p50_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--fps", type=int, default=30)
    ap.add_argument("--requests", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--routes", default="frame,frame.jpg")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--cpu", action="store_true", help="CPU backend (rehearsal; says nothing about the GPU)")
    a = ap.parse_args()

    from video_edge_ai_proxy_amd._native import native
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.server.app import build_app

    if not a.cpu and native.device_count() == 0:
        raise SystemExit("no GPU (use --cpu for a rehearsal)")
    farm = native.RtspServer("127.0.0.1", 0)
    sc = native.SynthConfig()
    sc.width, sc.height, sc.gop, sc.fps, sc.seed = a.width, a.height, 10, a.fps, 11
    farm.add_stream("/cam", sc, realtime=True, cached_frames=20)
    farm.start()
    cfg = Config()
    cfg.data_dir = tempfile.mkdtemp(prefix="vep-bench-")
    cfg.gpu.devices = [-1 if a.cpu else a.device]
    cfg.serving.frontends = 0
    app = build_app(cfg, host="127.0.0.1", rest_port=0, grpc_port=0)
    out = {"width": a.width, "height": a.height, "backend": "cpu" if a.cpu else "gpu", "requests": a.requests,
           "quality": a.quality, "routes": {}}
    try:
        con = http.client.HTTPConnection("127.0.0.1", app.rest_port, timeout=30)
        for _ in range(100):  # the REST server starts listening on its own thread
            try:
                con.connect()
                break
            except ConnectionRefusedError:
                time.sleep(0.05)
        con.request("POST", "/api/v1/process", body=json.dumps(
            {"name": "bench_cam", "rtsp_endpoint": f"rtsp://127.0.0.1:{farm.port}/cam"}),
            headers={"Content-Type": "application/json"})
        r = con.getresponse()
        r.read()
        assert r.status == 200, r.status
        routes = [s for s in a.routes.split(",") if s]
        paths = {s: f"/api/v1/process/bench_cam/{s}" + (f"?quality={a.quality}" if s.endswith(".jpg") else "")
                 for s in routes}
        deadline = time.time() + 30
        while True:  # the first request wakes the lazy decoder
            con.request("GET", paths[routes[0]])
            r = con.getresponse()
            r.read()
            if r.status == 200:
                break
            assert time.time() < deadline, "no frame within 30 s"
            time.sleep(0.05)
        times = {s: [] for s in routes}
        sizes = {s: 0 for s in routes}
        bodies = {}
        for k in range(a.warmup + a.requests):
            for s in routes:
                t0 = time.perf_counter()
                con.request("GET", paths[s])
                r = con.getresponse()
                body = r.read()
                dt = (time.perf_counter() - t0) * 1e3
                assert r.status == 200, (s, r.status)
                if k >= a.warmup:
                    times[s].append(dt)
                    sizes[s] = len(body)
                    bodies[s] = body
        raw = a.width * a.height * 3
        for s in routes:
            d = summary(times[s])
            d["response_bytes"] = sizes[s]
            # /frame copies the whole ring slot; /frame.jpg the joined entropy stream (the response
            # minus the header up to SOS and the EOI, which the host writes) and 3 status words
            if a.cpu:
                d["d2h_bytes"] = 0
            elif s.endswith(".jpg"):
                d["d2h_bytes"] = sizes[s] - (bodies[s].index(b"\xff\xda") + 14) - 2 + 12
            else:
                d["d2h_bytes"] = raw
            out["routes"][s] = d
        if hasattr(app.hub, "latest_jpeg"):  # (a tree without the encoder has only /frame)
            gpu_ms, host_ms = [], []
            for k in range(a.warmup + a.requests):
                t0 = time.perf_counter()
                app.hub.latest_jpeg("bench_cam", 0, a.quality)
                t1 = time.perf_counter()
                _, frame = app.hub.latest_frame("bench_cam", 0)
                native.jpeg_encode_cpu(frame, a.quality)
                t2 = time.perf_counter()
                if k >= a.warmup:
                    gpu_ms.append((t1 - t0) * 1e3)
                    host_ms.append((t2 - t1) * 1e3)
            out["encode_gpu"] = summary(gpu_ms)
            out["copy_raw_and_encode_cpu"] = summary(host_ms)
        con.close()
    finally:
        app.stop()
        farm.stop()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
