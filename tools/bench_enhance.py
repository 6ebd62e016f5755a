"""Numbers of docs/ENHANCE.md, on an MI355X.

    python tools/bench_enhance.py kernels [--flat] [--reps 20]   # under rocprofv3 --kernel-trace --stats: per-kernel time
    python tools/bench_enhance.py calls                         # call times: ops.clahe_batch, served JPEGs, 32 cameras

`kernels` runs ops.clahe_batch on 32 1080p pictures (random, or --flat: one colour) at the default
parameters `reps` times after a warm-up; the profiler's statistics give each kernel's time per call.
`calls` prints one JSON line of medians and ranges (milliseconds) over `reps` calls each.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))

from video_edge_ai_proxy_amd import ops  # noqa: E402
from video_edge_ai_proxy_amd._native import native  # noqa: E402

N, W, H = 32, 1920, 1080


def pictures(flat: bool):
    rng = np.random.default_rng(1)
    dev = torch.device("cuda", 0)
    if flat:
        return [torch.full((H, W, 3), 20 + k, dtype=torch.uint8, device=dev) for k in range(N)]
    return [torch.from_numpy(rng.integers(0, 256, (H, W, 3)).astype(np.uint8)).to(dev) for _ in range(N)]


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def kernels(a):
    pics = pictures(a.flat)
    outs = [torch.empty_like(p) for p in pics]
    for _ in range(a.reps + 2):
        ops.clahe_batch(pics, outs=outs)
    torch.cuda.synchronize()


def calls(a):
    from conftest import synth
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub

    class NoSession:
        def stop(self):
            pass

    res = {}
    for flat in (False, True):
        pics = pictures(flat)
        outs = [torch.empty_like(p) for p in pics]

        def batch():
            ops.clahe_batch(pics, outs=outs)
            torch.cuda.synchronize()

        res["clahe_batch_32x1080p_" + ("flat" if flat else "random")] = timed(batch, a.reps)
    cfg = Config()
    cfg.data_dir = tempfile.mkdtemp(prefix="bench_enhance_")
    hub = Hub(cfg, devices=[0])
    try:
        wk = hub.workers[0]
        names = [f"c{k}" for k in range(N)]
        for k, name in enumerate(names):
            cam = wk.add_camera(name, 2)
            hub.cameras[name] = CameraHandle(name, 0, cam, "", session=NoSession())
            assert wk.decode_now(cam, synth(native, W, H, gop=6, motion=0.2, seed=k + 1).next())
        res["frame_jpg_plain"] = timed(lambda: hub.latest_jpeg("c0", quality=85), a.reps)
        res["frame_jpg_enhanced"] = timed(lambda: hub.latest_jpeg("c0", quality=85, enhance=True), a.reps)
        res["frame_jpg_640_plain"] = timed(lambda: hub.latest_jpeg("c0", quality=85, width=640), a.reps)
        res["frame_jpg_640_enhanced"] = timed(lambda: hub.latest_jpeg("c0", quality=85, width=640, enhance=True), a.reps)
        res["latest_enhanced_32_cameras"] = timed(lambda: [hub.latest_enhanced(n) for n in names], max(3, a.reps // 4))
        frames = []
        res["pull_32_frames"] = timed(lambda: frames.__setitem__(slice(None), [hub.latest_frame(n)[1] for n in names]),
                                      max(3, a.reps // 4))
        res["cpu_twin_32_frames_one_thread"] = timed(lambda: [native.clahe_cpu(f, 128, 32, 256) for f in frames], 3)
    finally:
        hub.shutdown()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "calls"))
    ap.add_argument("--flat", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_enhance: needs a GPU")
    (kernels if a.mode == "kernels" else calls)(a)


if __name__ == "__main__":
    main()
