"""The gfx950 dehaze kernels (csrc/vep/gpu_dehaze.hip) against the CPU twin, byte for byte: the
dehazed picture and every intermediate plane (table, air light and normalisation tables, cell means,
a and b, their box means), at the shapes where the kernels can go wrong, at any address and pitch,
in and out of place, batched; and the served JPEG of a GPU hub against the CPU backend's."""
import numpy as np
import pytest
import torch

from conftest import synth
from dehaze_oracle import hazy_scene
from test_clahe import BOX
from test_crop import _NoSession, _slots

pytestmark = pytest.mark.gpu

# w x h: the window larger than the picture, partial cells and tiles, one tile and a sliver
SHAPES = [(16, 16), (67, 19), (130, 34), (257, 65)]
GUARD = 16


def picture(kind, w, h, seed):
    if kind == 0:
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == 1:  # one colour: every pixel in one bin of the table
        return np.full((h, w, 3), (200, 0, 90), np.uint8)
    return hazy_scene(w, h, seed=seed)[1]


def placed(p, off, pitch_extra, dev):
    """The picture in a zeroed device buffer, GUARD + `off` bytes behind a 16-byte boundary, rows
    `3 w + pitch_extra` apart, GUARD bytes behind it -> (buffer, view, base)."""
    h, w = p.shape[:2]
    pitch = w * 3 + pitch_extra
    buf = torch.zeros(16 + GUARD + off + h * pitch + GUARD, dtype=torch.uint8, device=dev)
    base = (-buf.data_ptr()) % 16 + GUARD + off
    view = buf.as_strided((h, w, 3), (pitch, 3, 1), base)
    view.copy_(torch.from_numpy(p).to(dev))
    return buf, view, base


def run_and_compare(native, jobs):
    """jobs: (picture, (patch, omega, t0, radius, strength), src offset, dst offset, pitch extra, in place). One batch."""
    from video_edge_ai_proxy_amd import dehaze as dh, ops

    dev = torch.device("cuda", 0)
    srcs = [placed(p, so, pe, dev) for p, _, so, _, pe, _ in jobs]
    dsts = [s if inplace else placed(np.zeros_like(p), do, (pe + 1) % 17, dev) for s, (p, _, _, do, pe, inplace) in zip(srcs, jobs)]
    res = ops.dehaze_batch([s[1] for s in srcs], *zip(*(j[1] for j in jobs)), outs=[d[1] for d in dsts], planes=True)
    torch.cuda.synchronize()
    for k, ((p, params, *_, inplace), (out, words)) in enumerate(zip(jobs, res)):
        h, w = p.shape[:2]
        want, wwords = native.dehaze_cpu(p, *dh.to_native(*params))
        got, exp = dh.split_planes(words.cpu().numpy().view(np.uint32), w, h), dh.split_planes(wwords, w, h)
        for name in ("table", "air", "norm", "cell", "ab", "mean"):
            assert np.array_equal(got[name], exp[name]), (name, k, p.shape, params, inplace)
        assert np.array_equal(out.cpu().numpy(), want), ("picture", k, p.shape, params, inplace)
        # the guards and the bytes between the rows are still zero: nothing but the rows was written
        buf, view, base = dsts[k]
        pitch = view.stride(0)
        rest = buf.cpu().numpy().copy()
        for y in range(h):
            rest[base + y * pitch:base + y * pitch + w * 3] = 0
        assert not rest.any(), ("bytes outside the destination's rows were written", k, p.shape)
        if not inplace:
            assert np.array_equal(srcs[k][1].cpu().numpy(), p), ("the source was written", k, p.shape)


@pytest.mark.parametrize("patch", [3, 31])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_the_twin(native, shape, patch):
    """Per shape and patch one batch of six pictures: radius 1 and 16 against strength 0, 0.5 and 1,
    walking through the contents, offsets and pitches, every second one in place."""
    w, h = shape
    jobs = [(picture(k % 3, w, h, seed=k), (patch, (0.95, 1.0, 0.5)[k % 3], (0.1, 0.05, 1.0)[k % 3], (1, 16)[k % 2], (0, 0.5, 1)[k // 2]),
             (0, 1, 5, 15)[k % 4], (15, 0, 1, 5)[k % 4], (0, 1, 16)[k % 3], k % 2 == 1) for k in range(6)]
    run_and_compare(native, jobs)


def test_batch_of_different_sizes_and_parameters(native):
    shapes = [(200, 130, 15, 8), (577, 50, 7, 3), (33, 300, 31, 16)]
    jobs = [(picture(2 - k, w, h, seed=50 + k), (patch, 0.95, 0.1, radius, 1.0), (1, 5, 0)[k], (0, 15, 1)[k], (16, 0, 1)[k], k == 1)
            for k, (w, h, patch, radius) in enumerate(shapes)]
    run_and_compare(native, jobs)


def test_overlapping_destination_and_foreign_source_is_refused(native):
    from video_edge_ai_proxy_amd import ops

    a = torch.zeros((32, 32, 3), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(ValueError, match="overlaps"):
        ops.dehaze_batch([a, a], outs=[a, None])


def test_hub_dehazed_jpeg_equals_the_cpu_backend(native, tmp_path):
    """At native size the slot is dehazed out of place and stays as it was; scaled, the scaler's
    canvas is dehazed in place; behind the denoise its picture is. All against the CPU backend's
    chain of twins, the air light included."""
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
            for _ in range(3):
                assert wk.decode_now(cam, enc.next())
            frame = wk.read_latest(cam, 0)[1]
            full = hub.latest_jpeg("a", quality=80, dehaze=True)
            got[dev] = (frame, full[1], full[0]["dehaze_air"], hub.latest_jpeg("a", quality=80, dehaze={"patch": 31}, width=300)[1],
                        hub.latest_jpeg("a", quality=80, dehaze=True, denoise=True, enhance=True, overlay=BOX)[1],
                        hub.latest_dehazed("a", radius=3)[1], hub.latest_dehazed("a", width=200)[1],
                        hub.latest_jpeg("a", quality=80)[1])
            assert np.array_equal(wk.read_latest(cam, 0)[1], frame) and hub.dehaze_count() == 5
        finally:
            hub.shutdown()
    for a, b in zip(got[0], got[-1]):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    assert got[0][7] == native.jpeg_encode_cpu(got[0][0], 80) != got[0][1] == native.jpeg_encode_cpu(native.dehaze_cpu(got[0][0])[0], 80)
