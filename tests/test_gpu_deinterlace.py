"""The gfx950 deinterlace kernel (csrc/vep/gpu_deinterlace.hip) against the CPU twin, byte for byte,
at the shapes where the kernel can go wrong, every frame at its own address and pitch, batched; and
the served pictures of a GPU hub against the CPU backend's."""
import numpy as np
import pytest
import torch

from conftest import synth
from test_clahe import BOX
from test_crop import _NoSession, _slots
from test_gpu_clahe import placed

pytestmark = pytest.mark.gpu

OFFSETS, EXTRAS, GUARD = (0, 1, 5, 15), (0, 1, 16), 16
SHAPES = [(4, 4), (64, 16), (67, 19), (130, 35), (257, 65)]


def pair(kind, w, h, seed):
    """A woven frame and the one before it: noise; a static pair; a texture shifted by two pixels."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == 0:
        return f, rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == 1:
        return f, f.copy()
    yy, xx = np.mgrid[0:h, 0:w + 2]
    tex = np.clip(128 + 90 * np.sin(xx / 3.0 + yy / 5.0)[..., None] + rng.integers(-8, 9, (h, w + 2, 3)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(tex[:, 2:]), np.ascontiguousarray(tex[:, :-2])


def run_and_compare(native, jobs):
    """jobs: (newer, older or None, order, temporal, n). One batch; every frame of job n sits at its
    own offset and pitch, the destination at another in a zeroed buffer whose every other byte (in
    front, behind and between the rows) must stay zero."""
    from video_edge_ai_proxy_amd import ops

    dev = torch.device("cuda", 0)
    srcs, outs, bufs = [], [], []
    for newer, older, _, _, n in jobs:
        h, w = newer.shape[:2]
        srcs.append((placed(newer, OFFSETS[n % 4], EXTRAS[n % 3], dev),
                     None if older is None else placed(older, OFFSETS[(n + 1) % 4], EXTRAS[(n + 2) % 3], dev)))
        off, pitch = OFFSETS[(n + 3) % 4], w * 3 + EXTRAS[(n + 1) % 3]
        buf = torch.zeros(GUARD + 16 + off + h * pitch + GUARD, dtype=torch.uint8, device=dev)
        base = (-buf.data_ptr()) % 16 + GUARD + off
        outs.append(buf.as_strided((h, w, 3), (pitch, 3, 1), base))
        bufs.append(buf)
    res = ops.deinterlace_batch(srcs, [j[2] for j in jobs], [j[3] for j in jobs], outs)
    torch.cuda.synchronize()
    for (newer, older, order, temporal, n), placed_pair, out, buf in zip(jobs, srcs, res, bufs):
        what = (n, newer.shape, older is not None, order, temporal)
        assert np.array_equal(out.cpu().numpy(), native.deinterlace_cpu(newer, older, order, int(temporal))), ("picture",) + what
        for f, p in zip((newer, older), placed_pair):
            assert f is None or np.array_equal(p.cpu().numpy(), f), ("a source was written",) + what
        out.zero_()
        assert not buf.any().item(), ("guard bytes",) + what


@pytest.mark.parametrize("mix", ["pairs", "single", "mixed"])
@pytest.mark.parametrize("order", ["tff", "bff"])
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_the_twin(native, size, order, mix):
    """The issue's shapes; a case is one batch of the three contents at walking offsets and pitches,
    with the previous frame present, absent or both within the batch."""
    c = size[0] + (order == "bff") + 2 * ["pairs", "single", "mixed"].index(mix)
    jobs = []
    for kind in range(3):
        for rep in range(2):
            n = c + 2 * kind + rep
            newer, older = pair(kind, *size, seed=n)
            if mix == "single" or (mix == "mixed" and rep):
                older = None
            jobs.append((newer, older, order, not (mix == "pairs" and kind == 0 and rep), n))
    run_and_compare(native, jobs)


def test_batch_of_different_sizes_and_orders(native):
    shapes = [(4, 5), (200, 130), (577, 50), (33, 300), (640, 360), (129, 257)]
    jobs = []
    for n, (w, h) in enumerate(shapes):
        newer, older = pair(n % 3, w, h, seed=70 + n)
        jobs.append((newer, None if n % 4 == 3 else older, ("tff", "bff")[n % 2], True, n))
    run_and_compare(native, jobs)


def test_hub_deinterlaced_pictures_equal_the_cpu_backend(native, tmp_path):
    """The deinterlaced copy stands where the slot stood: encoded as it is, scaled, dehazed, enhanced
    and drawn on; and copied down. All against the CPU backend's bytes; the ring's frames stay."""
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
            m, plain = hub.latest_jpeg("a", quality=80, deinterlace=True)
            got[dev] = (ring, plain, hub.latest_jpeg("a", quality=80, deinterlace={"order": "bff"}, width=300)[1],
                        hub.latest_jpeg("a", quality=80, deinterlace=True, dehaze=True, enhance={"tile": 64}, overlay=BOX)[1],
                        hub.latest_jpeg("a", quality=80, deinterlace={"temporal": False})[1],
                        hub.latest_deinterlaced("a")[1], hub.latest_deinterlaced("a", width=200, order="bff")[1],
                        hub.latest_jpeg("a", quality=80)[1])
            assert m["deinterlace_frames"] == 2 and hub.deinterlace_count() == 6
            assert np.array_equal(np.stack([f for _, f in wk.read_history(cam, 0, 3)]), ring)
        finally:
            hub.shutdown()
    for a, b in zip(got[0], got[-1]):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    assert got[0][7] == native.jpeg_encode_cpu(got[0][0][-1], 80) != got[0][1]
