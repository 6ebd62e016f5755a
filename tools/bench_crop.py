#!/usr/bin/env python3
"""Cost of crops on the GPU (docs/CROPS.md, "Measured").

Two measurements, both on an MI355X:

1. The crop launch alone, through ``ops.crop_resize_batch`` (one kernel launch for every box of
   every picture, as ``Hub.crops_many`` does for a worker's cameras), in three cases:

   * ``reduce``   32 pictures of 1920x1080 with 8 boxes each, 600x400 pixels and larger, to 224x224;
   * ``enlarge``  the same pictures with 8 boxes of 40x40 pixels each, to 224x224;
   * ``uhd64``    one picture of 3840x2160 with 64 boxes of mixed sizes, to 224x224.

   Timed with device events around --iters back-to-back calls after --warmup (the descriptor upload
   and the call's host wait are inside, so this is an upper bound of the kernel); the kernel's own
   time comes from a run of ``--profile N --case NAME`` under
   ``rocprofv3 --kernel-trace --stats -- python tools/bench_crop.py --profile 50 --case reduce``,
   each case a run of its own. Every case is checked once against the CPU twin.

       python tools/bench_crop.py
       python tools/bench_crop.py --profile 50 --case enlarge

2. The whole call (``--hub``): a Hub with --cams cameras of 1920x1080 on one GPU, 8 boxes each to
   224x224 through ``Hub.crops_many`` (one launch; only the crops cross PCIe), beside the baseline
   the other documents use: pull every full frame to the host (``Hub.latest_frame``) and cut and
   resize there (the CPU twin). Host clock around calls that end in a device synchronise.

       python tools/bench_crop.py --hub
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

UNIT = 10000


def rect_box(w: int, h: int, x0: int, y0: int, x1: int, y1: int) -> dict:
    """The box whose pixel rect in a w x h picture is [x0, x1) x [y0, y1)."""
    return {"x0": -(-x0 * UNIT // w), "y0": -(-y0 * UNIT // h), "x1": x1 * UNIT // w, "y1": y1 * UNIT // h}


def boxes_of(case: str, w: int, h: int, n: int, seed: int) -> list:
    """n boxes of a w x h picture: `reduce` 600x400 .. 900x700 pixels, `enlarge` 40x40, `uhd64`
    40 .. 1200 pixels a side; placed by a seeded generator (no two pictures share their boxes)."""
    import numpy as np

    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        if case == "enlarge":
            bw = bh = 40
        elif case == "reduce":
            bw, bh = int(rng.integers(600, 901)), int(rng.integers(400, 701))
        else:
            bw, bh = int(rng.integers(40, 1201)), int(rng.integers(40, 1201))
        x0, y0 = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
        out.append(rect_box(w, h, x0, y0, x0 + bw, y0 + bh))
    return out


def shape_of(case: str, cams: int) -> tuple:
    """(pictures, width, height, boxes per picture)"""
    return (1, 3840, 2160, 64) if case == "uhd64" else (cams, 1920, 1080, 8)


CASES = ("reduce", "enlarge", "uhd64")


def hub_run(a) -> None:
    import numpy as np

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
        lists = {}
        for k in range(a.cams):
            name = f"cam{k:02d}"
            cam = wk.add_camera(name, 2)
            hub.cameras[name] = CameraHandle(name, 0, cam, "", session=NoSession())
            c = native.SynthConfig()
            c.width, c.height, c.gop, c.seed, c.motion = 1920, 1080, 10, k + 1, 0.2
            if not wk.decode_now(cam, native.SynthH264(c).next()):
                raise SystemExit("the synthetic camera's first picture did not decode")
            lists[name] = boxes_of(a.case if a.case != "uhd64" else "reduce", 1920, 1080, 8, k)
        out = {"cams": a.cams, "boxes_per_camera": 8, "width": 224, "height": 224, "case": a.case}
        got = hub.crops_many(lists, 224, 224)
        # the baseline computes the same bytes (checked on one camera)
        name = f"cam{a.cams - 1:02d}"
        frame = hub.latest_frame(name)[1]
        from video_edge_ai_proxy_amd import crops

        want = native.crop_resize_cpu(frame, crops.to_native(lists[name]), 224, 224)
        if not np.array_equal(got[name][1], want):
            raise SystemExit("Hub.crops_many differs from the CPU twin on the pulled frame")
        for _ in range(a.warmup):
            hub.crops_many(lists, 224, 224)
        ms = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(a.hub_iters):
                hub.crops_many(lists, 224, 224)
            ms.append((time.perf_counter() - t0) * 1e3 / a.hub_iters)
        out["crops_many_ms"] = {"p50": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}
        out["crops_many_pcie_bytes"] = a.cams * 8 * 224 * 224 * 3
        pull, host = [], []
        for _ in range(max(1, a.repeats // 2)):
            t0 = time.perf_counter()
            frames = {n: hub.latest_frame(n)[1] for n in lists}
            t1 = time.perf_counter()
            for n, f in frames.items():
                native.crop_resize_cpu(f, crops.to_native(lists[n]), 224, 224)
            t2 = time.perf_counter()
            pull.append((t1 - t0) * 1e3)
            host.append((t2 - t1) * 1e3)
        out["baseline_pull_ms"] = round(statistics.median(pull), 3)
        out["baseline_host_crop_ms"] = round(statistics.median(host), 3)
        out["baseline_pcie_bytes"] = a.cams * 1920 * 1080 * 3
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
    ap.add_argument("--case", default="reduce", choices=CASES)
    ap.add_argument("--hub", action="store_true", help="Hub.crops_many beside pulling the frames and cropping on the host")
    ap.add_argument("--hub-iters", type=int, default=20)
    ap.add_argument("--data-dir", default="/tmp/vep_bench_crop")
    a = ap.parse_args()

    import torch

    from video_edge_ai_proxy_amd import ops
    from video_edge_ai_proxy_amd._native import native

    if native.device_count() == 0:
        raise SystemExit("no GPU: this measures the MI355X (a CPU run would say nothing about it)")
    if a.hub:
        hub_run(a)
        return
    out = {"cams": a.cams, "iters": a.iters, "output": "224x224"}
    with torch.cuda.device(a.device):
        g = torch.Generator(device="cpu").manual_seed(1)
        for case in ([a.case] if a.profile else CASES):
            n, w, h, per = shape_of(case, a.cams)
            src = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).cuda() for _ in range(n)]
            lists = [boxes_of(case, w, h, per, k) for k in range(n)]
            dst = torch.empty((n * per, 224, 224, 3), dtype=torch.uint8, device="cuda")
            if a.profile:
                for _ in range(a.profile):
                    ops.crop_resize_batch(src, lists, 224, 224, out=dst)
                torch.cuda.synchronize()
                print(json.dumps({"profiled_calls": a.profile, "case": case}))
                return
            ops.crop_resize_batch(src, lists, 224, 224, out=dst)
            want = ops.crop_resize_reference(src[-1], lists[-1], 224, 224)
            if not bool((dst[-per:].cpu() == want).all()):
                raise SystemExit(f"{case}: the kernel's crops differ from the CPU twin's")
            for _ in range(a.warmup):
                ops.crop_resize_batch(src, lists, 224, 224, out=dst)
            ms = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    ops.crop_resize_batch(src, lists, 224, 224, out=dst)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / a.iters)
            read = 0
            for bs in lists:
                for b in bs:
                    x0, y0, x1, y1 = native.crop_pixels(w, h, (b["x0"], b["y0"], b["x1"], b["y1"]))
                    read += (x1 - x0) * (y1 - y0) * 3
            out[case] = {"crops": n * per, "call_ms_p50": round(statistics.median(ms), 4), "call_ms_min": round(min(ms), 4),
                         "call_ms_max": round(max(ms), 4), "bytes_read": read, "bytes_written": n * per * 224 * 224 * 3}
            del src, dst
    print(json.dumps(out))


if __name__ == "__main__":
    main()
