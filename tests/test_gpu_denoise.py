"""The gfx950 denoise kernel (csrc/vep/gpu_denoise.hip) against the CPU twin, byte for byte, at the
shapes where the kernel can go wrong, every frame at its own address and pitch, batched; and the
served pictures of a GPU hub against the CPU backend's."""
import numpy as np
import pytest
import torch

from conftest import synth
from test_clahe import BOX
from test_crop import _NoSession, _slots
from test_denoise import ramped
from test_gpu_clahe import placed

pytestmark = pytest.mark.gpu

OFFSETS, EXTRAS = (0, 1, 5, 15), (0, 1, 16)
KS, LEVELS, STRENGTHS, GUARD = (1, 2, 3, 8), (1, 8, 64), (256, 128, 0), 16


def frame_set(kind, w, h, k, level, seed):
    """k frames, newest first: the ramped noise; identical frames; a hard vertical edge that moves
    3 pixels per frame (weights cut beside still ones); random frames."""
    rng = np.random.default_rng(seed)
    if kind == 0:
        return ramped(w, h, k, level, seed)
    if kind == 1:
        return np.stack([rng.integers(0, 256, (h, w, 3)).astype(np.uint8)] * k)
    if kind == 2:
        f = np.empty((k, h, w, 3), np.uint8)
        for i in range(k):
            f[i] = (30, 40, 50)
            f[i, :, min(w, w // 2 + 3 * i):] = (200, 180, 220)
        return f + rng.integers(0, 3, (k, h, w, 3)).astype(np.uint8)
    return rng.integers(0, 256, (k, h, w, 3)).astype(np.uint8)


def run_and_compare(native, jobs):
    """jobs: (frames (K, H, W, 3), level, strength, n). One batch; frame i of job n sits at its own
    offset and pitch, the destination at another, between zeroed guard bytes."""
    dev = torch.device("cuda", 0)
    from video_edge_ai_proxy_amd import ops

    srcs, outs, bufs = [], [], []
    for frames, _, _, n in jobs:
        k, h, w = frames.shape[:3]
        srcs.append([placed(f, OFFSETS[(n + i) % 4], EXTRAS[(n + 2 * i) % 3], dev) for i, f in enumerate(frames)])
        off, pitch = OFFSETS[(n + 3) % 4], w * 3 + EXTRAS[(n + 1) % 3]
        buf = torch.zeros(GUARD + 16 + off + h * pitch + GUARD, dtype=torch.uint8, device=dev)
        base = (-buf.data_ptr()) % 16 + GUARD + off
        outs.append(buf.as_strided((h, w, 3), (pitch, 3, 1), base))
        bufs.append((buf, base, (h - 1) * pitch + w * 3))
    res = ops.denoise_batch(srcs, [j[1] for j in jobs], [j[2] / 256 for j in jobs], outs)
    torch.cuda.synchronize()
    for (frames, level, strength, n), placed_frames, out, (buf, base, span) in zip(jobs, srcs, res, bufs):
        what = (n, frames.shape, level, strength)
        assert np.array_equal(out.cpu().numpy(), native.denoise_cpu(frames, level, strength)), ("picture",) + what
        for f, p in zip(frames, placed_frames):
            assert np.array_equal(p.cpu().numpy(), f), ("a source was written",) + what
        host = buf.cpu().numpy()
        assert not host[base - GUARD:base].any() and not host[base + span:base + span + GUARD].any(), ("guard bytes",) + what


@pytest.mark.parametrize("h", [33, 17, 16, 15, 2, 1])
@pytest.mark.parametrize("w", [1, 2, 63, 64, 65, 129])
def test_kernel_equals_the_twin(native, w, h):
    """Below, at and above one tile and its halo, and a second tile in each direction; the four frame
    sets of a case are one batch and walk through K, the levels and the strengths."""
    c = w * 7 + h
    jobs = []
    for kind in range(4):
        k, level = KS[(c + kind) % 4], LEVELS[(c // 4 + kind) % 3]
        jobs.append((frame_set(kind, w, h, k, level, seed=c * 4 + kind), level, STRENGTHS[(c // 2 + kind) % 3], c + kind))
    run_and_compare(native, jobs)


def test_batch_of_different_sizes_and_parameters(native):
    shapes = [(1, 1, 8), (200, 130, 4), (577, 50, 2), (33, 300, 3), (640, 360, 8), (129, 257, 1), (96, 96, 5)]
    run_and_compare(native, [(frame_set(n % 4, w, h, k, LEVELS[n % 3], seed=90 + n), LEVELS[n % 3], STRENGTHS[n % 2], n)
                             for n, (w, h, k) in enumerate(shapes)])


def test_hub_denoised_pictures_equal_the_cpu_backend(native, tmp_path):
    """The denoised copy stands where the slot stood: encoded as it is, scaled, enhanced and drawn on;
    and copied down. All against the CPU backend's bytes; the ring's frames stay as they were."""
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub

    got = {}
    for dev in (0, -1):
        cfg = Config()
        cfg.data_dir = str(tmp_path / f"data{dev}")
        hub = Hub(cfg, devices=[dev])
        try:
            wk = hub.workers[0]
            cam = wk.add_camera("a", _slots(native, 4), 4)
            hub.cameras["a"] = CameraHandle("a", 0, cam, "", session=_NoSession())
            enc = synth(native, 640, 480, gop=6, motion=0.2, seed=3)
            for _ in range(4):
                assert wk.decode_now(cam, enc.next())
            ring = [f for _, f in wk.read_history(cam, 0, 4)]
            m, plain = hub.latest_jpeg("a", quality=80, denoise=True)
            got[dev] = (np.stack(ring), plain, hub.latest_jpeg("a", quality=80, denoise={"frames": 3}, width=300)[1],
                        hub.latest_jpeg("a", quality=80, denoise={"level": 20}, enhance={"tile": 64}, overlay=BOX)[1],
                        hub.latest_denoised("a", strength=0.5)[1], hub.latest_denoised("a", width=200)[1],
                        hub.latest_jpeg("a", quality=80)[1])
            assert m["denoise_frames"] == 4 and hub.denoise_count() == 5
            assert np.array_equal(np.stack([f for _, f in wk.read_history(cam, 0, 4)]), got[dev][0])
        finally:
            hub.shutdown()
    for a, b in zip(got[0], got[-1]):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    assert got[0][6] == native.jpeg_encode_cpu(got[0][0][-1], 80) != got[0][1]
