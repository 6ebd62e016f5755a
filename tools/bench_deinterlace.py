"""Times of the deinterlacing (docs/DEINTERLACE.md), one JSON line:

    python tools/bench_deinterlace.py [--reps 20] [--pictures 32] [--serving]

ops.deinterlace_batch on 32 1080p pairs (the moving-bar scene of the tests): the one launch, by
device events, the median of `reps` runs after three warm-up runs, with and without the previous
frame, beside the traffic floor of the same run: the bytes the kernel must move (two pictures in,
one out; spatial only: one in, one out) over the bandwidth of one device-to-device copy of the
same pictures, measured the same way. And the host alternative: pulling the two frames and running
the CPU twin on one thread. `--serving` adds Hub.latest_jpeg(deinterlace=True) beside the plain call
on one 1080p camera of a GPU hub (wall clock, median). Where the time goes comes from a kernel
trace of this tool in a run of its own (`rocprofv3 --kernel-trace --stats -- python
tools/bench_deinterlace.py`)."""
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

        assert hub.latest_jpeg("a", deinterlace=True)[0]["deinterlace_frames"] == 2
        return {"latest_jpeg_plain_ms": wall(lambda: hub.latest_jpeg("a", quality=85)),
                "latest_jpeg_deinterlace_ms": wall(lambda: hub.latest_jpeg("a", quality=85, deinterlace=True)),
                "latest_jpeg_deinterlace_640_ms": wall(lambda: hub.latest_jpeg("a", quality=85, deinterlace=True, width=640))}
    finally:
        hub.shutdown()


def main():
    from deinterlace_oracle import bar_scene
    from video_edge_ai_proxy_amd import _vep as native, ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pictures", type=int, default=32)
    ap.add_argument("--serving", action="store_true")
    a = ap.parse_args()
    newer, older, _ = bar_scene(1920, 1080, speed=24)
    dev = torch.device("cuda", 0)
    n = a.pictures
    new = torch.from_numpy(newer).to(dev).repeat(n, 1, 1, 1)
    old = torch.from_numpy(older).to(dev).repeat(n, 1, 1, 1)
    out = torch.empty_like(new)
    res = {"pictures": n}
    copy_ms = timed(lambda: out.copy_(new), a.reps)
    nbytes = newer.nbytes * n
    res["copy_GBps"] = 2 * nbytes / copy_ms / 1e6
    outs = list(out.unbind(0))
    for name, pairs, moved in (("pairs", list(zip(new.unbind(0), old.unbind(0))), 3), ("spatial", list(new.unbind(0)), 2)):
        ms = timed(lambda: ops.deinterlace_batch(pairs, outs=outs), a.reps)
        floor_ms = moved * nbytes / (res["copy_GBps"] * 1e6)
        res[f"deinterlace_batch_{name}_ms"] = ms
        res[f"traffic_floor_{name}_ms"] = floor_ms
        res[f"deinterlace_batch_{name}_over_floor"] = ms / floor_ms
        # the same launch without the tensor face's per-picture checks (host time that the events see too)
        span, row = newer.nbytes, newer.shape[1] * 3
        work = [((p[0].data_ptr(), span, row), (p[1].data_ptr(), span, row) if moved == 3 else (0, 0, 0),
                 (o.data_ptr(), span, row), newer.shape[1], newer.shape[0], 0, 1)
                for p, o in zip(pairs if moved == 3 else [(q, None) for q in pairs], outs)]
        stream = int(torch.cuda.current_stream(dev).cuda_stream)
        ms = timed(lambda: native.deinterlace_device_batch(work, stream), a.reps)
        res[f"launch_{name}_ms"] = ms
        res[f"launch_{name}_over_floor"] = ms / floor_ms
    t0 = time.perf_counter()
    host = new[0].cpu().numpy(), old[0].cpu().numpy()
    native.deinterlace_cpu(host[0], host[1])
    res["host_pull_and_twin_one_frame_ms"] = (time.perf_counter() - t0) * 1e3
    if a.serving:
        res.update(serving(native, a.reps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
