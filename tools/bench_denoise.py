"""Numbers of docs/DENOISE.md, on an MI355X.

    python tools/bench_denoise.py kernels [--frames 4] [--reps 20]   # under rocprofv3 --kernel-trace --stats: kernel time
    python tools/bench_denoise.py calls                              # call times: ops.denoise_batch, served JPEGs, 32 cameras

`kernels` runs ops.denoise_batch on 32 1080p pictures of `frames` noisy frames each at the default
parameters `reps` times after a warm-up; the profiler's statistics give the kernel's time per call.
`calls` prints one JSON line of medians and ranges (milliseconds) over `reps` calls each, and the
JPEG sizes of a noisy dark synthetic scene plain, denoised, enhanced and both.
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


def noisy_frames(k: int, seed: int, dark: bool = False):
    """k frames [k, H, W, 3] on the device: one base picture plus per-frame noise of +-6 levels
    (dark: a dim ramp with a lamp, as a camera at night at high gain)."""
    rng = np.random.default_rng(seed)
    if dark:
        base = (np.arange(W)[None, :] * 40 // (W - 1) + np.arange(H)[:, None] * 20 // (H - 1))[..., None] + np.zeros(3, int)
        base[H // 3:H // 3 + 40, W // 2:W // 2 + 60] = 250
    else:
        base = rng.integers(40, 216, (H, W, 3))
    f = np.clip(base[None] + rng.integers(-6, 7, (k, H, W, 3)), 0, 255).astype(np.uint8)
    return torch.from_numpy(f).to(torch.device("cuda", 0))


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def pictures(k: int):
    """N pictures of k frames each: four different ones, cloned."""
    four = [noisy_frames(k, 1 + n) for n in range(4)]
    return [four[n % 4].clone() for n in range(N)]


def kernels(a):
    pics = pictures(a.frames)
    outs = [torch.empty_like(p[0]) for p in pics]
    for _ in range(a.reps + 2):
        ops.denoise_batch(pics, outs=outs)
    torch.cuda.synchronize()


def calls(a):
    from conftest import synth
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub

    class NoSession:
        def stop(self):
            pass

    res = {}
    for k in (4, 8):
        pics = pictures(k)
        outs = [torch.empty_like(p[0]) for p in pics]

        def batch():
            ops.denoise_batch(pics, outs=outs)
            torch.cuda.synchronize()

        res[f"denoise_batch_32x1080p_k{k}"] = timed(batch, a.reps)
        del pics, outs
    # what denoising saves in bytes: a noisy dark scene, quality 85
    night = noisy_frames(4, 9, dark=True)
    clean = ops.denoise(night)
    res["jpeg_bytes_dark_scene"] = {
        "plain": len(ops.jpeg_encode(night[0], 85)), "denoised": len(ops.jpeg_encode(clean, 85)),
        "enhanced": len(ops.jpeg_encode(ops.clahe(night[0]), 85)), "denoised_enhanced": len(ops.jpeg_encode(ops.clahe(clean), 85))}
    del night, clean
    cfg = Config()
    cfg.data_dir = tempfile.mkdtemp(prefix="bench_denoise_")
    hub = Hub(cfg, devices=[0])
    try:
        wk = hub.workers[0]
        names = [f"c{k}" for k in range(N)]
        for k, name in enumerate(names):
            cam = wk.add_camera(name, 6, 4)
            hub.cameras[name] = CameraHandle(name, 0, cam, "", session=NoSession())
            enc = synth(native, W, H, gop=6, motion=0.2, seed=k + 1)
            for _ in range(4):
                assert wk.decode_now(cam, enc.next())
        res["frame_jpg_plain"] = timed(lambda: hub.latest_jpeg("c0", quality=85), a.reps)
        res["frame_jpg_denoised"] = timed(lambda: hub.latest_jpeg("c0", quality=85, denoise=True), a.reps)
        res["frame_jpg_denoised_enhanced"] = timed(lambda: hub.latest_jpeg("c0", quality=85, denoise=True, enhance=True), a.reps)
        res["latest_denoised_32_cameras"] = timed(lambda: [hub.latest_denoised(n) for n in names], max(3, a.reps // 4))
        hist = []
        res["pull_4x32_frames"] = timed(
            lambda: hist.__setitem__(slice(None), [np.stack([f for _, f in hub.history(n, 0, 4)][::-1]) for n in names]),
            max(3, a.reps // 4))
        res["cpu_twin_32_cameras_one_thread"] = timed(lambda: [native.denoise_cpu(f, 8, 256) for f in hist], 3)
    finally:
        hub.shutdown()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "calls"))
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_denoise: needs a GPU")
    (kernels if a.mode == "kernels" else calls)(a)


if __name__ == "__main__":
    main()
