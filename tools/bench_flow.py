"""Numbers of docs/FLOW.md, on an MI355X.

    python tools/bench_flow.py kernels [--decimate 2] [--range 7] [--reps 20]   # under rocprofv3 --kernel-trace --stats: kernel times
    python tools/bench_flow.py calls                                            # call times: ops.block_flow_batch, Hub.flow_many, the host

`kernels` runs ops.block_flow_batch on 32 1080p frame pairs `reps` times after a warm-up; the
profiler's statistics give the time of flow_luma_kernel and flow_match_kernel per call. `calls`
prints one JSON line of medians and ranges (milliseconds) over `reps` calls each, the bytes that
cross PCIe, and the match kernel's arithmetic (packed SADs per call) for the floor in docs/FLOW.md.
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


def pairs():
    """N (newer, older) pairs on the device: four textures, each against itself moved by (6, -4) pixels."""
    rng = np.random.default_rng(1)
    four = []
    for _ in range(4):
        t = torch.from_numpy(rng.integers(0, 256, (H + 8, W + 8, 3)).astype(np.uint8)).to(torch.device("cuda", 0))
        four.append((t[4:4 + H, 4:4 + W].contiguous(), t[8:8 + H, :W].contiguous()))
    return [tuple(p.clone() for p in four[n % 4]) for n in range(N)]


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def kernels(a):
    ps = pairs()
    for _ in range(a.reps + 2):
        ops.block_flow_batch(ps, a.decimate, a.range)
    torch.cuda.synchronize()


def calls(a):
    from conftest import synth
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub

    class NoSession:
        def stop(self):
            pass

    res = {}
    ps = pairs()
    for d, r in ((2, 7), (1, 15)):
        def batch():
            ops.block_flow_batch(ps, d, r)
            torch.cuda.synchronize()

        res[f"block_flow_batch_32x1080p_d{d}_r{r}"] = timed(batch, a.reps)
        blocks = (W // d // 8) * (H // d // 8)
        res[f"packed_sads_d{d}_r{r}"] = N * blocks * (2 * r + 1) ** 2 * 16  # 4-byte SADs (a qsad forms four)
    del ps
    cfg = Config()
    cfg.data_dir = tempfile.mkdtemp(prefix="bench_flow_")
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
            out = hub.flow_many(names)
            return (time.perf_counter() - t0) * 1e3, out

        fresh()
        ms = [fresh()[0] for _ in range(max(3, a.reps // 4))]
        res["flow_many_32_cameras_evaluated"] = {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}
        res["flow_many_32_cameras_stored"] = timed(lambda: hub.flow_many(names), a.reps)
        res["pcie_bytes_records"] = N * (W // 2 // 8) * (H // 2 // 8) * 8
        res["pcie_bytes_frames"] = N * 2 * W * H * 3
        hist = []
        res["pull_2x32_frames"] = timed(
            lambda: hist.__setitem__(slice(None), [[f for _, f in hub.history(n, 0, 2)][::-1] for n in names]), max(3, a.reps // 4))
        res["cpu_twin_32_cameras_one_thread"] = timed(lambda: [native.flow_cpu(f[0], f[1], 2, 7) for f in hist], 2)
    finally:
        hub.shutdown()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "calls"))
    ap.add_argument("--decimate", type=int, default=2)
    ap.add_argument("--range", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flow: needs a GPU")
    (kernels if a.mode == "kernels" else calls)(a)


if __name__ == "__main__":
    main()
