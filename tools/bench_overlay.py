#!/usr/bin/env python3
"""Cost of the on-screen display on the GPU (docs/OVERLAY.md, "Measured").

Two measurements, both on an MI355X:

1. The overlay launch alone, through ``ops.overlay_draw_batch`` (one kernel launch for every
   picture of a request), in three cases:

   * ``inplace``  32 pictures of 1920x1080, 8 labelled boxes and a stamp each, drawn in place;
   * ``copy``     the same, out of place (copy and draw into a second tensor);
   * ``wall``     one 8 x 4 wall canvas of 320x180 tiles (2560x720) with 32 labels, in place.

   Timed with device events around --iters back-to-back calls after --warmup (the uploads of the
   descriptors, primitives and text and the call's host wait are inside, so this is an upper bound
   of the kernel); the kernel's own time comes from a run of ``--profile N --case NAME`` under
   ``rocprofv3 --kernel-trace --stats -- python tools/bench_overlay.py --profile 50 --case inplace``,
   each case a run of its own, no counters. Every case is checked once against the CPU twin.

       python tools/bench_overlay.py
       python tools/bench_overlay.py --profile 50 --case copy

2. The whole call (``--hub``): a Hub with one camera of 1920x1080 on one GPU, 8 labelled boxes
   stored; ``Hub.latest_jpeg(overlay=True, stamp=True)`` at native size and at ``width=640`` beside
   the same calls without an overlay, and beside the baseline the other documents use: pull the
   frame to the host (``Hub.latest_frame``), draw with the CPU twin on one thread, encode on the
   host. Host clock around calls that end in a device synchronise.

       python tools/bench_overlay.py --hub
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("inplace", "copy", "wall")
STAMP = {"type": "text", "x": 100, "y": 100, "text": "{name} {time}", "bg": [0, 0, 0], "bg_alpha": 128}
META = {"seq": 123456, "timestamp": 90 * 1790000000123}


def boxes_of(n: int, seed: int) -> list:
    """n labelled outlines of 1000 .. 4000 units a side, placed by a seeded generator."""
    import numpy as np

    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        bw, bh = int(rng.integers(1000, 4001)), int(rng.integers(1000, 4001))
        x0, y0 = int(rng.integers(0, 10001 - bw)), int(rng.integers(0, 10001 - bh))
        out.append({"x0": x0, "y0": y0, "x1": x0 + bw, "y1": y0 + bh, "alpha": 200,
                    "color": [int(c) for c in rng.integers(0, 256, 3)], "label": f"object {i} {50 + 5 * i}%"})
    return out


def wall_items(cols: int, rows: int) -> list:
    """What the labelled wall draws, spelled as items of the canvas: a name on black at the corner
    of every tile (the wall itself expands per tile; the primitives are the same rectangles)."""
    return [{"type": "text", "x": 10000 * (t % cols) // cols, "y": 10000 * (t // cols) // rows, "text": f"camera-{t:02d}",
             "scale": 1, "bg": [0, 0, 0], "bg_alpha": 160} for t in range(cols * rows)]


def hub_run(a) -> None:
    import numpy as np

    from video_edge_ai_proxy_amd import overlay
    from video_edge_ai_proxy_amd._native import native
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub

    class NoSession:
        def stop(self):
            pass

    cfg = Config()
    cfg.data_dir = a.data_dir
    cfg.gpu.letterbox_size = 0
    hub = Hub(cfg, devices=[a.device])
    try:
        wk = hub.workers[0]
        cam = wk.add_camera("cam", 2)
        hub.cameras["cam"] = CameraHandle("cam", 0, cam, "", session=NoSession())
        c = native.SynthConfig()
        c.width, c.height, c.gop, c.seed, c.motion = 1920, 1080, 10, 1, 0.2
        if not wk.decode_now(cam, native.SynthH264(c).next()):
            raise SystemExit("the synthetic camera's first picture did not decode")
        items = boxes_of(8, 1)
        hub.set_overlay("cam", items)
        meta, frame = hub.latest_frame("cam")
        want = np.zeros_like(frame)
        native.overlay_draw_cpu(frame, want, overlay.to_native(items + [STAMP]), "cam", meta)
        if hub.latest_jpeg("cam", quality=85, overlay=True, stamp=True)[1] != native.jpeg_encode_cpu(want, 85):
            raise SystemExit("Hub.latest_jpeg(overlay=True, stamp=True) differs from the CPU twin's JPEG")

        def timed(fn):
            for _ in range(a.warmup):
                fn()
            ms = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                for _ in range(a.hub_iters):
                    fn()
                ms.append((time.perf_counter() - t0) * 1e3 / a.hub_iters)
            return {"p50": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}

        out = {"picture": "1920x1080", "items": len(items) + 1}
        out["native_overlay_ms"] = timed(lambda: hub.latest_jpeg("cam", quality=85, overlay=True, stamp=True))
        out["native_plain_ms"] = timed(lambda: hub.latest_jpeg("cam", quality=85))
        out["w640_overlay_ms"] = timed(lambda: hub.latest_jpeg("cam", quality=85, overlay=True, stamp=True, width=640))
        out["w640_plain_ms"] = timed(lambda: hub.latest_jpeg("cam", quality=85, width=640))
        nat = overlay.to_native(items + [STAMP])
        pull, draw, enc = [], [], []
        for _ in range(max(1, a.repeats)):
            t0 = time.perf_counter()
            m, f = hub.latest_frame("cam")
            t1 = time.perf_counter()
            native.overlay_draw_cpu(f, want, nat, "cam", m)
            t2 = time.perf_counter()
            native.jpeg_encode_cpu(want, 85)
            t3 = time.perf_counter()
            pull.append((t1 - t0) * 1e3)
            draw.append((t2 - t1) * 1e3)
            enc.append((t3 - t2) * 1e3)
        out["baseline_pull_ms"] = round(statistics.median(pull), 3)
        out["baseline_host_draw_ms"] = round(statistics.median(draw), 3)
        out["baseline_host_encode_ms"] = round(statistics.median(enc), 3)
        out["baseline_pcie_bytes"] = 1920 * 1080 * 3
        print(json.dumps(out))
    finally:
        hub.shutdown()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=32)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per case (the spread is reported)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--profile", type=int, default=0, help="only this many calls of --case (profiler run)")
    ap.add_argument("--case", default="inplace", choices=CASES)
    ap.add_argument("--hub", action="store_true", help="Hub.latest_jpeg with an overlay beside the plain call and the host baseline")
    ap.add_argument("--hub-iters", type=int, default=20)
    ap.add_argument("--data-dir", default="/tmp/vep_bench_overlay")
    a = ap.parse_args()

    import torch

    from video_edge_ai_proxy_amd import ops
    from video_edge_ai_proxy_amd._native import native

    if native.device_count() == 0:
        raise SystemExit("no GPU: this measures the MI355X (a CPU run would say nothing about it)")
    if a.hub:
        hub_run(a)
        return
    out = {"cams": a.cams, "iters": a.iters}
    with torch.cuda.device(a.device):
        g = torch.Generator(device="cpu").manual_seed(1)
        for case in ([a.case] if a.profile else CASES):
            if case == "wall":
                n, w, h = 1, 2560, 720
                lists = [wall_items(8, 4)]
            else:
                n, w, h = a.cams, 1920, 1080
                lists = [boxes_of(8, k) + [STAMP] for k in range(n)]
            src = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).cuda() for _ in range(n)]
            outs = [torch.empty_like(s) for s in src] if case == "copy" else None
            call = lambda: ops.overlay_draw_batch(src, lists, outs, name="camera", meta=META)  # noqa: E731
            if a.profile:
                for _ in range(a.profile):
                    call()
                torch.cuda.synchronize()
                print(json.dumps({"profiled_calls": a.profile, "case": case}))
                return
            before = src[-1].clone()
            got = call()[-1]
            if not bool((got.cpu() == ops.overlay_draw_reference(before, lists[-1], "camera", META)).all()):
                raise SystemExit(f"{case}: the kernel's picture differs from the CPU twin's")
            for _ in range(a.warmup):
                call()
            ms = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    call()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / a.iters)
            prims = sum(len(native.overlay_expand(w, h, _native(l), "camera", META)) for l in lists)
            out[case] = {"pictures": n, "size": f"{w}x{h}", "primitives": prims, "call_ms_p50": round(statistics.median(ms), 4),
                         "call_ms_min": round(min(ms), 4), "call_ms_max": round(max(ms), 4), "picture_bytes": n * w * h * 3}
            del src, outs
    print(json.dumps(out))


def _native(items):
    from video_edge_ai_proxy_amd import overlay

    return overlay.to_native(items)


if __name__ == "__main__":
    main()
