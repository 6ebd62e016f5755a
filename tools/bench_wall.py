#!/usr/bin/env python3
"""Cost of the camera wall against the only way to see the same cameras without it: one
``frame.jpg`` per camera at native size.

--cams synthetic cameras (--width x --height, the synthetic camera's noisy picture) are decoded
into the ring slots of one worker of one hub; nothing is published while the measurement runs. Then

* in-process, alternating, p50 of --requests after --warmup: ``Hub.wall_jpeg`` (a --cols wide wall
  of --tile cells) against --cams x ``Hub.latest_jpeg`` at native size, with both byte counts and
  the ratio measured;
* request -> last byte over loopback HTTP (uvicorn, one keep-alive client, alternating) of
  ``wall.jpg``, ``frame.jpg?width=<tile width>`` and ``frame.jpg``.

    python tools/bench_wall.py                      # 32 x 1080p on GPU 0, 8 x 4 wall of 320x180
    python tools/bench_wall.py --profile 50         # only 50 walls: the run to put under
                                                    # rocprofv3 --kernel-trace --stats -- python ...
    python tools/bench_wall.py --cpu --cams 4 --width 320 --height 240 --cols 2   (CPU rehearsal)
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


class _NoSession:
    def stop(self):
        pass


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=32)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--cols", type=int, default=8)
    ap.add_argument("--tile", default="320x180")
    ap.add_argument("--requests", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--profile", type=int, default=0, help="only this many Hub.wall_jpeg calls (profiler run)")
    ap.add_argument("--no-http", action="store_true")
    ap.add_argument("--cpu", action="store_true", help="CPU backend (rehearsal; says nothing about the GPU)")
    a = ap.parse_args()

    from video_edge_ai_proxy_amd._native import native
    from video_edge_ai_proxy_amd.config import Config, parse_tile
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle
    from video_edge_ai_proxy_amd.server.app import build_app

    if not a.cpu and native.device_count() == 0:
        raise SystemExit("no GPU (use --cpu for a rehearsal)")
    tw, th = parse_tile(a.tile)
    cfg = Config()
    cfg.data_dir = tempfile.mkdtemp(prefix="vep-bench-")
    cfg.gpu.devices = [-1 if a.cpu else a.device]
    cfg.serving.frontends = 0
    cfg.serving.wall_max_tiles = max(64, a.cams)
    app = build_app(cfg, host="127.0.0.1", rest_port=0, grpc_port=0)
    hub = app.hub
    out = {"cams": a.cams, "width": a.width, "height": a.height, "backend": "cpu" if a.cpu else "gpu",
           "wall": [a.cols * tw, -(-a.cams // a.cols) * th], "tile": [tw, th], "quality": a.quality,
           "requests": a.requests}
    try:
        wk = hub.workers[0]
        wk.wall_max_tiles = int(cfg.serving.wall_max_tiles)
        names = []
        for k in range(a.cams):
            sc = native.SynthConfig()
            sc.width, sc.height, sc.gop, sc.fps, sc.seed = a.width, a.height, 10, 30, 11 + k
            enc = native.SynthH264(sc)
            name = f"bench_cam_{k:02d}"
            cam = wk.add_camera(name, 2)
            for _ in range(2):
                assert wk.decode_now(cam, enc.next())
            hub.cameras[name] = CameraHandle(name, 0, cam, "", session=_NoSession())
            names.append(name)
        wall = dict(names=names, cols=a.cols, tile_width=tw, tile_height=th, quality=a.quality)
        if a.profile:
            for _ in range(a.profile):
                hub.wall_jpeg(**wall)
            print(json.dumps({"profiled_walls": a.profile}))
            return
        wall_ms, each_ms, wall_bytes, each_bytes = [], [], 0, 0
        for k in range(a.warmup + a.requests):
            t0 = time.perf_counter()
            _, jpg = hub.wall_jpeg(**wall)
            t1 = time.perf_counter()
            total = 0
            for n in names:
                total += len(hub.latest_jpeg(n, 0, a.quality)[1])
            t2 = time.perf_counter()
            if k >= a.warmup:
                wall_ms.append((t1 - t0) * 1e3)
                each_ms.append((t2 - t1) * 1e3)
                wall_bytes, each_bytes = len(jpg), total
        out["wall_jpeg"] = dict(summary(wall_ms), bytes=wall_bytes)
        out["latest_jpeg_x_cams"] = dict(summary(each_ms), bytes=each_bytes)
        out["time_ratio"] = round(statistics.median(each_ms) / statistics.median(wall_ms), 2)
        out["bytes_ratio"] = round(each_bytes / wall_bytes, 2)
        if not a.no_http:
            con = http.client.HTTPConnection("127.0.0.1", app.rest_port, timeout=30)
            for _ in range(100):  # the REST server starts listening on its own thread
                try:
                    con.connect()
                    break
                except ConnectionRefusedError:
                    time.sleep(0.05)
            one = f"/api/v1/process/{names[0]}/frame.jpg?quality={a.quality}"
            paths = {"wall.jpg": f"/api/v1/wall.jpg?cols={a.cols}&tile={tw}x{th}&quality={a.quality}",
                     f"frame.jpg?width={tw}": one + f"&width={tw}", "frame.jpg": one}
            times = {s: [] for s in paths}
            sizes = {s: 0 for s in paths}
            for k in range(a.warmup + a.requests):
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
