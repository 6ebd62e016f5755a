"""The gfx950 CLAHE kernels (csrc/vep/gpu_clahe.hip) against the CPU twin, byte for byte: the
enhanced picture and the intermediate histograms and LUTs, at the shapes where the kernels can go
wrong, at any address and pitch, in and out of place, batched; and the served JPEG of a GPU hub
against the CPU backend's."""
import numpy as np
import pytest
import torch

from conftest import synth
from test_clahe import BOX
from test_crop import _NoSession

pytestmark = pytest.mark.gpu

OFFSETS, CLIPS, STRENGTHS = (0, 1, 5, 15), (2.0, 1.0, 256.0), (1.0, 0.5, 0.0)


def sides(tile):
    """1, 7, 9 (below a column of 8 pixels and just above), around one tile, the thin and the
    not-thin last tile, three tiles, and a second chunk of the histogram kernel."""
    return [1, 7, 9, tile - 1, tile, tile + 1, tile + tile // 2 - 1, tile + tile // 2, 2 * tile + 3, 513 + tile]


def picture(kind, w, h, tile, seed):
    rng = np.random.default_rng(seed)
    if kind == 0:
        return rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == 1:  # one colour: the histogram kernel's vote
        return np.full((h, w, 3), (12, 40, 25), np.uint8)
    if kind == 2:  # two colours split at a tile boundary
        p = np.full((h, w, 3), (5, 9, 7), np.uint8)
        p[:, min(w, tile):] = (180, 200, 190)
        return p
    ramp = np.arange(w)[None, :] * 50 // max(1, w - 1) + np.arange(h)[:, None] * 30 // max(1, h - 1)
    return (ramp[..., None] + rng.integers(0, 6, (h, w, 3))).astype(np.uint8)


def placed(p, off, pitch_extra, dev):
    """The picture in a device buffer at byte offset `off` with rows `3 w + pitch_extra` apart."""
    h, w = p.shape[:2]
    pitch = w * 3 + pitch_extra
    buf = torch.zeros(16 + off + h * pitch, dtype=torch.uint8, device=dev)
    base = (-buf.data_ptr()) % 16 + off  # (the offset counts from a 16-byte boundary)
    view = buf.as_strided((h, w, 3), (pitch, 3, 1), base)
    view.copy_(torch.from_numpy(p).to(dev))
    return view


def run_and_compare(native, jobs):
    """jobs: (picture, tile, clip, strength, src offset, dst offset, pitch extra, in place). One batch."""
    from video_edge_ai_proxy_amd import enhance, ops

    dev = torch.device("cuda", 0)
    srcs = [placed(p, so, pe, dev) for p, _, _, _, so, _, pe, _ in jobs]
    outs = [s if inplace else placed(np.zeros_like(p), do, (pe + 1) % 17, dev)
            for s, (p, _, _, _, _, do, pe, inplace) in zip(srcs, jobs)]
    res = ops.clahe_batch(srcs, [j[1] for j in jobs], [j[2] for j in jobs], [j[3] for j in jobs], outs, planes=True)
    torch.cuda.synchronize()
    for k, ((p, tile, clip, strength, *_, inplace), (out, hist, lut)) in enumerate(zip(jobs, res)):
        want, whist, wlut = native.clahe_cpu(p, *enhance.to_native(tile, clip, strength))
        what = (k, p.shape, tile, clip, strength, inplace)
        assert np.array_equal(hist.cpu().numpy(), whist.astype(np.int64)), ("hist",) + what
        assert np.array_equal(lut.cpu().numpy(), wlut), ("lut",) + what
        assert np.array_equal(out.cpu().numpy(), want), ("picture",) + what
        if not inplace:
            assert np.array_equal(srcs[k].cpu().numpy(), p), ("the source was written",) + what


@pytest.mark.parametrize("tile", [32, 40])
@pytest.mark.parametrize("k", range(10))
def test_kernels_equal_the_twin(native, tile, k):
    """Widths against heights in reverse order; the four pictures of a case are one batch and walk
    through the offsets, pitches, clips and strengths, every second one in place."""
    w, h = sides(tile)[k], sides(tile)[9 - k]
    jobs = [(picture(kind, w, h, tile, seed=k * 4 + kind), tile, CLIPS[(k + kind) % 3], STRENGTHS[(k // 3 + kind) % 3],
             OFFSETS[(k + kind) % 4], OFFSETS[(k + 2 * kind + 1) % 4], (0, 1, 16)[(k + kind) % 3], (k + kind) % 2 == 1)
            for kind in range(4)]
    run_and_compare(native, jobs)


def test_batch_of_different_sizes_and_parameters(native):
    shapes = [(200, 130, 32), (577, 50, 64), (33, 300, 40), (1, 1, 128), (640, 360, 128), (129, 257, 256), (96, 96, 48)]
    jobs = [(picture(k % 4, w, h, tile, seed=50 + k), tile, CLIPS[k % 3], STRENGTHS[k % 2], OFFSETS[k % 4], OFFSETS[(k + 1) % 4],
             (0, 1, 16)[k % 3], k % 3 == 0) for k, (w, h, tile) in enumerate(shapes)]
    run_and_compare(native, jobs)


def test_hub_enhanced_jpeg_equals_the_cpu_backend(native, tmp_path):
    """Scaled, the scaler's canvas is enhanced in place and encoded; at native size the slot is
    enhanced out of place and stays as it was. Both against the CPU backend's bytes."""
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub

    got = {}
    for dev in (0, -1):
        cfg = Config()
        cfg.data_dir = str(tmp_path / f"data{dev}")
        hub = Hub(cfg, devices=[dev])
        try:
            wk = hub.workers[0]
            cam = wk.add_camera("a", 2)
            hub.cameras["a"] = CameraHandle("a", 0, cam, "", session=_NoSession())
            assert wk.decode_now(cam, synth(native, 640, 480, gop=6, motion=0.2, seed=3).next())
            frame = wk.read_latest(cam, 0)[1]
            got[dev] = (frame, hub.latest_jpeg("a", quality=80, enhance=True, width=300)[1],
                        hub.latest_jpeg("a", quality=80, enhance={"tile": 64, "clip": 4.0}, overlay=BOX)[1],
                        hub.latest_enhanced("a", tile=40)[1], hub.latest_jpeg("a", quality=80)[1])
            assert np.array_equal(wk.read_latest(cam, 0)[1], frame) and hub.enhance_count() == 3
        finally:
            hub.shutdown()
    for a, b in zip(got[0], got[-1]):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    assert got[0][4] == native.jpeg_encode_cpu(got[0][0], 80) != got[0][1]
