"""The gfx950 orient kernel (csrc/vep/gpu_orient.hip) against the CPU twin and numpy, byte for byte,
at the shapes where the kernel can go wrong, every picture at its own address and pitch, batched; and
the served pictures of a GPU hub against the CPU backend's."""
import numpy as np
import pytest
import torch

from conftest import synth
from test_clahe import BOX
from test_crop import _NoSession, _slots
from test_gpu_clahe import placed
from test_orient import ORIENTS, picture, turned

pytestmark = pytest.mark.gpu

OFFSETS, EXTRAS, GUARD = (0, 1, 5, 15), (0, 1, 16), 16
ELEMENTS = [o for o in ORIENTS if o not in ((0, "none"), (180, "h"), (180, "v"), (270, "h"), (270, "v"))]  # the 7 besides the identity
SHAPES = [(1, 1), (1, 70), (70, 1), (64, 64), (65, 63), (67, 19), (130, 35), (257, 65)]


def run_and_compare(native, jobs):
    """jobs: (picture, rotate, flip, n). One batch; the source of job n sits at its own offset and
    pitch, the destination at another in a zeroed buffer whose every other byte (16 in front, 16
    behind, and between the rows) must stay zero."""
    from video_edge_ai_proxy_amd import ops

    dev = torch.device("cuda", 0)
    srcs, outs, bufs = [], [], []
    for a, rotate, _, n in jobs:
        srcs.append(placed(a, OFFSETS[n % 4], EXTRAS[n % 3], dev))
        h, w = a.shape[:2]
        ow, oh = (h, w) if rotate in (90, 270) else (w, h)
        off, pitch = OFFSETS[(n + 3) % 4], ow * 3 + EXTRAS[(n + 1) % 3]
        buf = torch.zeros(GUARD + 16 + off + oh * pitch + GUARD, dtype=torch.uint8, device=dev)
        base = (-buf.data_ptr()) % 16 + GUARD + off
        outs.append(buf.as_strided((oh, ow, 3), (pitch, 3, 1), base))
        bufs.append(buf)
    res = ops.orient_batch(srcs, [j[1] for j in jobs], [j[2] for j in jobs], outs)
    torch.cuda.synchronize()
    for (a, rotate, flip, n), src, out, buf in zip(jobs, srcs, res, bufs):
        what = (n, a.shape, rotate, flip)
        got = out.cpu().numpy()
        assert np.array_equal(got, turned(a, rotate, flip)), ("picture against numpy",) + what
        assert np.array_equal(got, native.orient_cpu(a, rotate, flip)), ("picture against the twin",) + what
        assert np.array_equal(src.cpu().numpy(), a), ("the source was written",) + what
        out.zero_()
        assert not buf.any().item(), ("guard bytes",) + what


@pytest.mark.parametrize("rotate,flip", ELEMENTS)
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_twin_and_numpy(native, size, rotate, flip):
    """A case is one batch of four pictures of the shape, which walk through the offsets and pitches."""
    c = size[0] + rotate // 90 + 4 * ["none", "h", "v"].index(flip)
    run_and_compare(native, [(picture(*size, seed=c + k), rotate, flip, c + k) for k in range(4)])


def test_batch_of_different_sizes_and_orientations(native):
    shapes = [(1, 5), (200, 130), (577, 50), (33, 300), (640, 360), (129, 257), (64, 128), (3, 3)]
    run_and_compare(native, [(picture(w, h, seed=70 + n), *ORIENTS[(5 * n + 1) % 12], n) for n, (w, h) in enumerate(shapes)])


def test_hub_oriented_pictures_equal_the_cpu_backend(native, tmp_path):
    """The oriented copy stands where the slot stood: encoded as it is, scaled, and behind the
    deinterlacing dehazed, enhanced and drawn on; and copied down. All against the CPU backend's
    bytes; the ring's frames stay."""
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub

    got = {}
    for dev in (0, -1):
        cfg = Config()
        cfg.data_dir = str(tmp_path / f"data{dev}")
        hub = Hub(cfg, devices=[dev])
        try:
            wk = hub.workers[0]
            cam = wk.add_camera("a", _slots(native, 3), 3)
            hub.cameras["a"] = CameraHandle("a", 0, cam, "", session=_NoSession())
            enc = synth(native, 640, 480, gop=6, motion=0.2, seed=3)
            for _ in range(3):
                assert wk.decode_now(cam, enc.next())
            ring = np.stack([f for _, f in wk.read_history(cam, 0, 3)])
            m, plain = hub.latest_jpeg("a", quality=80, orient={"rotate": 90})
            got[dev] = (ring, plain, hub.latest_jpeg("a", quality=80, orient={"rotate": 270, "flip": "h"}, width=300)[1],
                        hub.latest_jpeg("a", quality=80, orient={"rotate": 90, "flip": "v"}, deinterlace=True, dehaze=True,
                                        enhance={"tile": 64}, overlay=BOX)[1],
                        hub.latest_jpeg("a", quality=80, orient={"flip": "h"}, denoise=True)[1],
                        hub.latest_oriented("a", rotate=180)[1], hub.latest_oriented("a", width=200, rotate=90)[1],
                        hub.latest_jpeg("a", quality=80)[1])
            assert (m["orient"], m["width"], m["height"]) == ("90", 480, 640) and hub.orient_count() == 6
            assert np.array_equal(np.stack([f for _, f in wk.read_history(cam, 0, 3)]), ring)
        finally:
            hub.shutdown()
    for a, b in zip(got[0], got[-1]):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    assert got[0][1] == native.jpeg_encode_cpu(turned(got[0][0][-1], 90, "none"), 80)
    assert got[0][7] == native.jpeg_encode_cpu(got[0][0][-1], 80) != got[0][1]
