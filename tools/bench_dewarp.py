#!/usr/bin/env python3
"""Cost of views on the GPU (docs/DEWARP.md, "Measured").

Two measurements, both on an MI355X:

1. The dewarp launch alone, through ``ops.remap_batch`` (one kernel launch for every view of the
   call, as ``Hub.views_many`` does for a worker's cameras), in three cases:

   * ``panorama``  32 fisheye pictures of 2880x2880, each to a 1920x480 panorama;
   * ``ptz``       the same pictures, each to a 640x640 virtual camera;
   * ``undistort`` one 1920x1080 picture through a Brown lens at native size.

   Timed with device events around windows of back-to-back calls after --warmup, each window at
   least --window-ms long and --iters calls (the descriptor and mesh upload and the call's host
   wait are inside, so this is an upper bound of the kernel); the
   kernel's own time comes from ``rocprofv3 --kernel-trace --stats -- python tools/bench_dewarp.py
   --profile 20 --case NAME``, each case a run of its own. Every case is checked once against the
   CPU twin. The module built with ``-DVEP_DEWARP_GLOBAL_ONLY`` gives the global-only column.

       python tools/bench_dewarp.py
       python tools/bench_dewarp.py --profile 20 --case ptz

2. The whole call (``--hub``): a Hub with --cams fisheye cameras of --size on one GPU, one view each
   through ``Hub.views_many`` (one launch; the meshes go up, only the views come down), beside
   pulling every full frame to the host (``Hub.latest_frame``) and remapping there on one thread
   (the CPU twin). Host clock around calls that end in a device synchronise.

       python tools/bench_dewarp.py --hub
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.environ.get("VEP_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FISHEYE = {"model": "equidistant", "fov_deg": 185}
BROWN = {"model": "brown", "fx": 6000, "fy": 10600, "k1": -0.28, "k2": 0.09, "k3": -0.01}
CASES = {  # name: (pictures, source side(s), lens, view)
    "panorama": (32, (2880, 2880), FISHEYE, {"type": "panorama", "mount": "ceiling", "pan0": -180, "pan1": 180, "tilt0": 0,
                                             "tilt1": -60, "width": 1920, "height": 480}),
    "ptz": (32, (2880, 2880), FISHEYE, {"type": "ptz", "mount": "ceiling", "pan": 30, "tilt": -35, "fov": 70, "width": 640,
                                        "height": 640}),
    "undistort": (1, (1920, 1080), BROWN, {"type": "ptz", "fov": 79.6, "width": 1920, "height": 1080}),
}


def spread(ms: list) -> dict:
    return {"p50": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def hub_run(a) -> None:
    import numpy as np

    from video_edge_ai_proxy_amd import views
    from video_edge_ai_proxy_amd._native import native
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub

    class NoSession:
        def stop(self):
            pass

    w, h = (int(v) for v in a.size.lower().split("x"))
    view = CASES[a.case][3]
    cfg = Config()
    cfg.data_dir = a.data_dir
    cfg.gpu.letterbox_size = 0
    hub = Hub(cfg, devices=[a.device])
    try:
        wk = hub.workers[0]
        asked = {}
        for k in range(a.cams):
            name = f"cam{k:02d}"
            cam = wk.add_camera(name, 2)
            hub.cameras[name] = CameraHandle(name, 0, cam, "", session=NoSession())
            c = native.SynthConfig()
            c.width, c.height, c.gop, c.seed, c.motion = w, h, 10, k + 1, 0.2
            if not wk.decode_now(cam, native.SynthH264(c).next()):
                raise SystemExit("the synthetic camera's first picture did not decode")
            hub.set_views(name, FISHEYE, {"v": view})
            asked[name] = "v"
        mesh = views.build_mesh(FISHEYE, view, w, h)
        got = hub.views_many(asked)
        name = f"cam{a.cams - 1:02d}"
        if not np.array_equal(got[name][1], native.remap_cpu(hub.latest_frame(name)[1], mesh, view["width"], view["height"])):
            raise SystemExit("Hub.views_many differs from the CPU twin on the pulled frame")
        for _ in range(a.warmup):
            hub.views_many(asked)
        ms = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(a.hub_iters):
                hub.views_many(asked)
            ms.append((time.perf_counter() - t0) * 1e3 / a.hub_iters)
        out = {"cams": a.cams, "source": a.size, "case": a.case, "views_many_ms": spread(ms),
               "views_many_pcie_bytes_down": a.cams * view["width"] * view["height"] * 3, "views_many_pcie_bytes_up": a.cams * mesh.nbytes}
        pull, host = [], []
        for _ in range(max(1, a.repeats // 2)):
            t0 = time.perf_counter()
            frames = {n: hub.latest_frame(n)[1] for n in asked}
            t1 = time.perf_counter()
            for f in frames.values():
                native.remap_cpu(f, mesh, view["width"], view["height"])
            t2 = time.perf_counter()
            pull.append((t1 - t0) * 1e3)
            host.append((t2 - t1) * 1e3)
        out["baseline_pull_ms"] = round(statistics.median(pull), 3)
        out["baseline_host_remap_ms"] = round(statistics.median(host), 3)
        out["baseline_pcie_bytes"] = a.cams * w * h * 3
        print(json.dumps(out))
    finally:
        hub.shutdown()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="calls a timed window, at least")
    ap.add_argument("--window-ms", type=float, default=1000.0, help="a timed window lasts at least this long")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per case (the spread is reported)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--profile", type=int, default=0, help="only this many calls of --case (profiler run)")
    ap.add_argument("--case", default="panorama", choices=list(CASES))
    ap.add_argument("--hub", action="store_true", help="Hub.views_many beside pulling the frames and remapping on the host")
    ap.add_argument("--cams", type=int, default=32)
    ap.add_argument("--size", default="1920x1920", help="--hub: the cameras' frames")
    ap.add_argument("--hub-iters", type=int, default=10)
    ap.add_argument("--data-dir", default="/tmp/vep_bench_dewarp")
    a = ap.parse_args()

    import torch

    from video_edge_ai_proxy_amd import ops, views
    from video_edge_ai_proxy_amd._native import native

    if native.device_count() == 0:
        raise SystemExit("no GPU: this measures the MI355X (a CPU run would say nothing about it)")
    if a.hub:
        hub_run(a)
        return
    out = {"module": os.path.dirname(native.__file__)}
    with torch.cuda.device(a.device):
        g = torch.Generator(device="cpu").manual_seed(1)
        for case in ([a.case] if a.profile else CASES):
            n, (w, h), lens, view = CASES[case]
            one = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g)
            src = [one.roll(k, 1).cuda() for k in range(n)]
            mesh = views.build_mesh(lens, view, w, h)
            meshes, whs = [mesh] * n, [(view["width"], view["height"])] * n
            dst = torch.empty((n * view["width"] * view["height"] * 3,), dtype=torch.uint8, device="cuda")
            if a.profile:
                for _ in range(a.profile):
                    ops.remap_batch(src, meshes, whs, out=dst)
                torch.cuda.synchronize()
                print(json.dumps({"profiled_calls": a.profile, "case": case}))
                return
            got = ops.remap_batch(src, meshes, whs, out=dst)[-1].cpu()
            if not bool((got == ops.remap_reference(src[-1], mesh, view["width"], view["height"])).all()):
                raise SystemExit(f"{case}: the kernel's view differs from the CPU twin's")
            def window(calls: int) -> float:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    ops.remap_batch(src, meshes, whs, out=dst)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / calls

            window(a.warmup)
            iters = max(a.iters, int(a.window_ms / window(a.iters)) + 1)
            ms = [window(iters) for _ in range(a.repeats)]
            out[case] = {"views": n, "calls_a_window": iters, "call_ms": spread(ms), "bytes_written": n * view["width"] * view["height"] * 3,
                         "mesh_bytes_up": n * mesh.nbytes, "mesh_error_px": round(views.mesh_error(lens, view, w, h), 4)}
            del src, dst
    print(json.dumps(out))


if __name__ == "__main__":
    main()
