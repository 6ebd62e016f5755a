"""Times of the orientation (docs/ORIENT.md), one JSON line:

    python tools/bench_orient.py [--reps 20] [--pictures 32] [--serving]

ops.orient_batch on 32 1080p pictures of noise: the one launch, by device events, the median of
`reps` runs after three warm-up runs, for rotate=90, rotate=180 and flip=h, and the same launch
through native.orient_device_batch (no per-picture checks in Python), beside the traffic floor of
the same run: the bytes the kernel must move (one picture in, one out) over the bandwidth of one
device-to-device copy of the same pictures, measured the same way. `--serving` adds
Hub.latest_jpeg(orient={"rotate": 90}) beside the plain call on one 1080p camera of a GPU hub (wall
clock, median). Where the time goes comes from a kernel trace of this tool in a run of its own
(`rocprofv3 --kernel-trace --stats -- python tools/bench_orient.py`)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

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
        cam = wk.add_camera("a", wk.history_ring_slots(2), 2)
        hub.cameras["a"] = CameraHandle("a", 0, cam, "", session=NoSession())
        enc = synth(native, 1920, 1080, gop=6, motion=0.2, seed=3)
        for _ in range(2):
            assert wk.decode_now(cam, enc.next())

        def wall(fn):
            for _ in range(3):
                fn()
            ms = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                ms.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(ms)

        assert hub.latest_jpeg("a", orient={"rotate": 90})[0]["orient"] == "90"
        return {"latest_jpeg_plain_ms": wall(lambda: hub.latest_jpeg("a", quality=85)),
                "latest_jpeg_rotate90_ms": wall(lambda: hub.latest_jpeg("a", quality=85, orient={"rotate": 90})),
                "latest_jpeg_rotate90_640_ms": wall(lambda: hub.latest_jpeg("a", quality=85, orient={"rotate": 90}, width=640))}
    finally:
        hub.shutdown()


def main():
    from video_edge_ai_proxy_amd import _vep as native, ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pictures", type=int, default=32)
    ap.add_argument("--serving", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, w, h = a.pictures, 1920, 1080
    src = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev)
    flat = torch.empty_like(src)
    res = {"pictures": n, "reps": a.reps}
    copy_ms = timed(lambda: flat.copy_(src), a.reps)
    nbytes = src[0].numel() * n
    res["copy_GBps"] = 2 * nbytes / copy_ms / 1e6
    floor_ms = 2 * nbytes / (res["copy_GBps"] * 1e6)  # one picture in, one out
    res["traffic_floor_ms"] = floor_ms
    pictures = list(src.unbind(0))
    stream = int(torch.cuda.current_stream(dev).cuda_stream)
    for name, rotate, flip in (("rotate90", 90, "none"), ("rotate180", 180, "none"), ("flip_h", 0, "h")):
        ow, oh = (h, w) if rotate in (90, 270) else (w, h)
        outs = list(flat.view(n, oh, ow, 3).unbind(0))
        ms = timed(lambda: ops.orient_batch(pictures, rotate, flip, outs), a.reps)
        res[f"orient_batch_{name}_ms"] = ms
        span = w * h * 3
        work = [((p.data_ptr(), span, w * 3), (o.data_ptr(), span, ow * 3), w, h, rotate, {"none": 0, "h": 1, "v": 2}[flip])
                for p, o in zip(pictures, outs)]
        ms = timed(lambda: native.orient_device_batch(work, stream), a.reps)
        res[f"launch_{name}_ms"] = ms
        res[f"launch_{name}_over_floor"] = ms / floor_ms
    t0 = time.perf_counter()
    native.orient_cpu(src[0].cpu().numpy(), 90, "none")
    res["host_pull_and_twin_one_frame_ms"] = (time.perf_counter() - t0) * 1e3
    if a.serving:
        res.update(serving(native, a.reps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
