#!/usr/bin/env python3
"""Cost of the privacy masks on the GPU (docs/PRIVACY.md, "Measured").

Two measurements, both on an MI355X:

1. The mask launches alone: --cams device pictures (--width x --height) with one mask each, through
   ``ops.privacy_mask_batch`` (one kernel launch for all of them, as the publish path does for a
   batch), for a rect of 25 % of the picture and for the full frame, ``pixelate`` at --block and
   ``fill``. Timed with device events around --iters back-to-back calls after --warmup (the
   descriptor upload and the call's host wait are inside, so this is an upper bound of the kernel);
   the kernel's own time comes from running ``--profile N`` under
   ``rocprofv3 --kernel-trace --stats -- python tools/bench_mask.py --profile 50 --case pixelate_full``.
   Every case is checked once against the CPU twin.

       python tools/bench_mask.py
       python tools/bench_mask.py --profile 50 --case pixelate_quarter

2. The headline benchmark with a full-frame ``pixelate`` mask on every camera: ``--headline`` runs
   bench.py's own main() in this process, with ``Worker.add_camera`` wrapped so that every camera
   gets the mask before its first frame. Arguments after ``--`` go to bench.py.

       python tools/bench_mask.py --headline -- --gpus 1 --steps 20 --warmup 5
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUARTER = {"x0": 2500, "y0": 2500, "x1": 7500, "y1": 7500}  # half of each side
FULL = {"x0": 0, "y0": 0, "x1": 10000, "y1": 10000}


def cases(block: int) -> dict:
    return {"pixelate_quarter": dict(QUARTER, mode="pixelate", block=block),
            "pixelate_full": dict(FULL, mode="pixelate", block=block),
            "fill_quarter": dict(QUARTER, mode="fill", b=16, g=16, r=16),
            "fill_full": dict(FULL, mode="fill", b=16, g=16, r=16)}


def headline(rest: list[str]) -> None:
    from video_edge_ai_proxy_amd import native, privacy

    mask = privacy.to_native([dict(FULL, mode="pixelate", block=16)])
    plain = native.Worker.add_camera

    def add_camera(self, *args, **kw):
        cam = plain(self, *args, **kw)
        self.set_privacy_masks(cam, mask)
        return cam

    native.Worker.add_camera = add_camera
    import bench

    sys.argv = ["bench.py", *rest]
    bench.main()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=32)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--block", type=int, default=16)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per case (the spread is reported)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--profile", type=int, default=0, help="only this many calls of --case (profiler run)")
    ap.add_argument("--case", default="pixelate_quarter")
    ap.add_argument("--headline", action="store_true", help="bench.py with a full-frame pixelate mask on every camera")
    ap.add_argument("rest", nargs="*")
    a = ap.parse_args()
    if a.headline:
        headline(a.rest)
        return

    import torch

    from video_edge_ai_proxy_amd import ops
    from video_edge_ai_proxy_amd._native import native

    if native.device_count() == 0:
        raise SystemExit("no GPU: this measures the MI355X (a CPU run would say nothing about it)")
    out = {"cams": a.cams, "width": a.width, "height": a.height, "block": a.block, "iters": a.iters}
    with torch.cuda.device(a.device):
        g = torch.Generator(device="cpu").manual_seed(1)
        src = [torch.randint(0, 256, (a.height, a.width, 3), dtype=torch.uint8, generator=g).cuda() for _ in range(a.cams)]
        work = [s.clone() for s in src]
        todo = cases(a.block)
        if a.profile:
            m = todo[a.case]
            for _ in range(a.profile):
                ops.privacy_mask_batch(work, [[m]] * a.cams)
            torch.cuda.synchronize()
            print(json.dumps({"profiled_calls": a.profile, "case": a.case}))
            return
        for name, m in todo.items():
            lists = [[m]] * a.cams
            for w, s in zip(work, src):
                w.copy_(s)
            ops.privacy_mask_batch(work, lists)
            want = ops.privacy_mask_reference(src[-1], [m])
            if not bool((work[-1].cpu() == want).all()):
                raise SystemExit(f"{name}: the kernel's picture differs from the CPU twin's")
            for _ in range(a.warmup):
                ops.privacy_mask_batch(work, lists)
            ms = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    ops.privacy_mask_batch(work, lists)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / a.iters)
            x0, y0, x1, y1 = native.mask_pixels(a.width, a.height, (m["x0"], m["y0"], m["x1"], m["y1"], 0, 16, 0, 0, 0))
            rect_bytes = (x1 - x0) * (y1 - y0) * 3 * a.cams
            out[name] = {"call_ms_p50": round(statistics.median(ms), 4), "call_ms_min": round(min(ms), 4),
                         "call_ms_max": round(max(ms), 4),
                         "bytes_read_plus_written": rect_bytes * (2 if m["mode"] == "pixelate" else 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
