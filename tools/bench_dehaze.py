"""Times of the dehazing (docs/DEHAZE.md), one JSON line:

    python tools/bench_dehaze.py [--reps 20] [--pictures 32]

ops.dehaze_batch on 32 1080p pictures (a synthetic hazy scene) at the defaults and at patch 31:
the seven launches together, by device events, the median of `reps` runs after three warm-up runs,
beside the traffic floor of the same run: the bytes the kernels must read and write (the picture
three times in, once out, 20 bytes a cell twice) over the bandwidth of a device copy of the same
pictures, measured the same way. And the host alternative: pulling one frame and running the CPU
twin on one thread. `--serving` adds Hub.latest_jpeg(dehaze=True) beside the plain call on one 1080p
camera of a GPU hub (wall clock, median). The per-kernel split comes from a kernel trace of this
tool (`rocprofv3 --kernel-trace --stats -- python tools/bench_dehaze.py`): docs/DEHAZE.md."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def serving(native, reps):
    import tempfile

    from conftest import synth
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub

    class NoSession:
        def touch(self):
            pass

        def stop(self):
            pass

    cfg = Config()
    cfg.data_dir = tempfile.mkdtemp()
    hub = Hub(cfg, devices=[0])
    try:
        wk = hub.workers[0]
        cam = wk.add_camera("a", 2)
        hub.cameras["a"] = CameraHandle("a", 0, cam, "", session=NoSession())
        assert wk.decode_now(cam, synth(native, 1920, 1080, gop=6, motion=0.2, seed=3).next())

        def wall(fn):
            for _ in range(3):
                fn()
            ms = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                ms.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(ms)

        return {"latest_jpeg_plain_ms": wall(lambda: hub.latest_jpeg("a", quality=85)),
                "latest_jpeg_dehaze_ms": wall(lambda: hub.latest_jpeg("a", quality=85, dehaze=True)),
                "latest_jpeg_dehaze_640_ms": wall(lambda: hub.latest_jpeg("a", quality=85, dehaze=True, width=640))}
    finally:
        hub.shutdown()


def main():
    from dehaze_oracle import hazy_scene
    from video_edge_ai_proxy_amd import _vep as native, ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pictures", type=int, default=32)
    ap.add_argument("--serving", action="store_true")
    a = ap.parse_args()
    frame = hazy_scene(1920, 1080, block=40)[1]
    dev = torch.device("cuda", 0)
    pics = [torch.from_numpy(frame).to(dev) for _ in range(a.pictures)]
    outs = [torch.empty_like(p) for p in pics]
    res = {"pictures": a.pictures}
    copy_ms = timed(lambda: [o.copy_(p) for o, p in zip(outs, pics)], a.reps)
    nbytes = frame.nbytes * a.pictures
    res["copy_GBps"] = 2 * nbytes / copy_ms / 1e6
    cells = (1920 // 4) * (1080 // 4) * a.pictures
    floor_ms = (4 * nbytes + 2 * 20 * cells) / (res["copy_GBps"] * 1e6)
    for patch in (15, 31):
        ms = timed(lambda: ops.dehaze_batch(pics, patch=patch, outs=outs), a.reps)
        res[f"dehaze_batch_patch{patch}_ms"] = ms
        res[f"dehaze_batch_patch{patch}_over_floor"] = ms / floor_ms
    res["traffic_floor_ms"] = floor_ms
    t0 = time.perf_counter()
    host = pics[0].cpu().numpy()
    native.dehaze_cpu(host)
    res["host_pull_and_twin_one_frame_ms"] = (time.perf_counter() - t0) * 1e3
    if a.serving:
        res.update(serving(native, a.reps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
