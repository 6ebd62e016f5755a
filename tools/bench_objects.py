"""Numbers of docs/OBJECTS.md, on an MI355X.

    python tools/bench_objects.py kernels [--decimate 2] [--scene typical|checkerboard|serpentine] [--reps 20]
    python tools/bench_objects.py calls

`kernels` runs ops.label_objects_batch on 32 1080p frame pairs `reps` times after a warm-up; run it
under a kernel-trace profiler for the time of flow_luma_kernel and of the five objects kernels per
call. `calls` prints one JSON line: medians and ranges (milliseconds) of ops.label_objects_batch for
every scene at d = 2 and d = 1, of Hub.objects_many (evaluated and stored), of pulling the frames and
running the host twin on them, the bytes that cross PCIe, and every stage's memory traffic (bytes) for
the floors in docs/OBJECTS.md.
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
SCENES = ("typical", "checkerboard", "serpentine")


def pairs(scene, d):
    """N (newer, older) pairs on the device. typical: a random texture with five rectangles of it
    replaced; the worst cases: the plane's checkerboard or serpentine, a sample being d x d pixels."""
    rng = np.random.default_rng(1)
    ph, pw = H // d, W // d
    y, x = np.mgrid[0:ph, 0:pw]
    if scene == "checkerboard":
        m = (x + y) % 2 == 0
    elif scene == "serpentine":
        m = (y % 4 == 0) | (x == np.where((y // 4) % 2 == 0, pw - 1, 0))
    out = []
    for n in range(4):
        older = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        newer = older.copy()
        if scene == "typical":
            for _ in range(5):
                bx, by = int(rng.integers(0, W - 200)), int(rng.integers(0, H - 300))
                newer[by:by + 300, bx:bx + 120] = rng.integers(0, 256, (300, 120, 3))
        else:
            up = np.repeat(np.repeat(m, d, axis=0), d, axis=1)
            newer[:up.shape[0], :up.shape[1]][up] ^= 0x80
        out.append((torch.from_numpy(newer).cuda(), torch.from_numpy(older).cuda()))
    return [tuple(p.clone() for p in out[n % 4]) for n in range(N)]


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def traffic(d):
    """Bytes every stage moves at least, for all N cameras: what it must read and write once."""
    s = (W // d) * (H // d)
    return {"luma": N * (2 * W * H * 3 + 2 * s), "mask": N * (2 * s + s // 8 + 8 * s), "seam": N * 4 * s * (64 + 32) // 2048,
            "count": N * 4 * s, "slot": N * 4 * s, "box": N * 8 * s}


def kernels(a):
    ps = pairs(a.scene, a.decimate)
    for _ in range(a.reps + 2):
        ops.label_objects_batch(ps, a.decimate)
    torch.cuda.synchronize()


def calls(a):
    from conftest import synth
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub

    class NoSession:
        def stop(self):
            pass

    res = {}
    for d in (2, 1):
        res[f"traffic_bytes_d{d}"] = traffic(d)
        for scene in SCENES:
            ps = pairs(scene, d)

            def batch():
                ops.label_objects_batch(ps, d)
                torch.cuda.synchronize()

            res[f"label_objects_batch_32x1080p_d{d}_{scene}"] = timed(batch, a.reps)
            del ps
    cfg = Config()
    cfg.data_dir = tempfile.mkdtemp(prefix="bench_objects_")
    hub = Hub(cfg, devices=[0])
    try:
        wk = hub.workers[0]
        names = [f"c{k}" for k in range(N)]
        encs = []
        for k, name in enumerate(names):
            cam = wk.add_camera(name, 6, 4)
            hub.cameras[name] = CameraHandle(name, 0, cam, "", session=NoSession())
            encs.append((cam, synth(native, W, H, gop=6, motion=0.2, seed=k + 1)))
            for _ in range(2):
                assert wk.decode_now(cam, encs[-1][1].next())

        def fresh():  # a new frame per camera, then one evaluated call
            for cam, enc in encs:
                assert wk.decode_now(cam, enc.next())
            t0 = time.perf_counter()
            out = hub.objects_many(names)
            return (time.perf_counter() - t0) * 1e3, out

        fresh()
        runs = [fresh() for _ in range(max(3, a.reps // 4))]
        ms = [r[0] for r in runs]
        res["objects_many_32_cameras_evaluated"] = {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}
        res["objects_many_32_cameras_stored"] = timed(lambda: hub.objects_many(names), a.reps)
        res["pcie_bytes_counts_and_records"] = N * 4 + 24 * sum(r["count"] for r in runs[-1][1].values())
        res["pcie_bytes_frames"] = N * 2 * W * H * 3
        hist = []
        res["pull_2x32_frames"] = timed(
            lambda: hist.__setitem__(slice(None), [[f for _, f in hub.history(n, 0, 2)][::-1] for n in names]), max(3, a.reps // 4))
        res["cpu_twin_32_cameras_one_thread"] = timed(lambda: [native.objects_cpu(f[0], f[1]) for f in hist], 2)
    finally:
        hub.shutdown()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "calls"))
    ap.add_argument("--decimate", type=int, default=2)
    ap.add_argument("--scene", choices=SCENES, default="typical")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_objects: needs a GPU")
    (kernels if a.mode == "kernels" else calls)(a)


if __name__ == "__main__":
    main()
