"""gfx950 camera wall: one launch for all tiles, byte equality with the CPU composition, and the
Worker's ring paths (run on an MI355X)."""
import threading

import numpy as np
import pytest
import torch

import scale_oracle as so
from conftest import synth

pytestmark = pytest.mark.gpu


def dev(frames):
    return [None if f is None else torch.from_numpy(f).cuda() for f in frames]


def host(frames):
    return [None if f is None else torch.from_numpy(f) for f in frames]


def test_one_tile():
    from video_edge_ai_proxy_amd import ops

    fs = [so.picture("noise", 64, 48)]
    got = ops.compose_wall(dev(fs), None, 16, 9)
    assert tuple(got.shape) == (9, 16, 3)
    assert torch.equal(got.cpu(), ops.compose_wall_reference(host(fs), None, 16, 9))


def test_mixed_sizes_with_an_empty_tile():
    from video_edge_ai_proxy_amd import ops

    fs = [so.picture("noise", 64, 36), so.picture("gradient", 200, 120), None, so.picture("noise", 64, 48),
          so.picture("checkerboard", 64, 36, seed=2)]
    got = ops.compose_wall(dev(fs), None, 31, 18)  # odd dx, bars on either axis (tests/test_wall.py)
    assert torch.equal(got.cpu(), ops.compose_wall_reference(host(fs), None, 31, 18))
    got = ops.compose_wall(dev(fs), 2, 320, 180)  # cells larger than the sources: never enlarged
    assert torch.equal(got.cpu(), ops.compose_wall_reference(host(fs), 2, 320, 180))


def test_more_tiles_than_lanes():
    """33 tiles: more than the lanes of a wave, and more than one row of the grid."""
    from video_edge_ai_proxy_amd import ops

    fs = [so.picture(so.KINDS[t % 4], 48, 32, seed=t) for t in range(33)]
    got = ops.compose_wall(dev(fs), None, 16, 9)
    assert tuple(got.shape) == (6 * 9, 6 * 16, 3)
    assert torch.equal(got.cpu(), ops.compose_wall_reference(host(fs), None, 16, 9))


def test_descriptors_grow_past_the_floor_and_come_back():
    """One tile, then 65 tiles of 8 x 8 in 4 x 4 cells (81 cells: more than the 64 descriptors a set
    starts with), then the one again: all three exact."""
    from video_edge_ai_proxy_amd import ops

    fs = [so.picture(so.KINDS[t % 4], 8, 8, seed=t) for t in range(65)]
    d = dev(fs)
    for n in (1, 65, 1):
        got = ops.compose_wall(d[:n], None, 4, 4)
        assert torch.equal(got.cpu(), ops.compose_wall_reference(host(fs[:n]), None, 4, 4)), f"{n} tiles"


def test_reused_canvas_has_no_stale_pixels():
    from video_edge_ai_proxy_amd import ops

    canvas = torch.empty((2 * 18, 3 * 31, 3), dtype=torch.uint8, device="cuda")
    full = [so.picture("noise", 62, 36, seed=t) for t in range(5)]  # fill their cells: 31 x 18
    ops.compose_wall(dev(full), None, 31, 18, out=canvas)
    assert torch.equal(canvas.cpu(), ops.compose_wall_reference(host(full), None, 31, 18))
    bars = [so.picture("noise", 64, 48), None, so.picture("noise", 64, 36), None, so.picture("gradient", 20, 40)]
    ops.compose_wall(dev(bars), None, 31, 18, out=canvas)  # bars and empty cells over the old pictures
    assert torch.equal(canvas.cpu(), ops.compose_wall_reference(host(bars), None, 31, 18))


def test_argument_checks():
    from video_edge_ai_proxy_amd import ops

    x = torch.zeros((16, 16, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.compose_wall([x], None, 8, 8)  # host tensor
    with pytest.raises(ValueError):
        ops.compose_wall([x.cuda()[:, ::2]], None, 8, 8)  # not contiguous
    with pytest.raises(TypeError):
        ops.compose_wall([x.cuda().float()], None, 8, 8)
    with pytest.raises(ValueError):
        ops.compose_wall([x.cuda()], None, 0, 8)
    with pytest.raises(ValueError):
        ops.compose_wall([x.cuda()], None, 8, 65536)
    with pytest.raises(ValueError):
        ops.compose_wall([], None, 8, 8)
    with pytest.raises(ValueError):
        ops.compose_wall([x.cuda(), x.cuda()], 1, 8, 40000)  # canvas taller than 65535
    with pytest.raises(ValueError):
        ops.compose_wall([x.cuda()], None, 8, 8, out=torch.empty((8, 9, 3), dtype=torch.uint8, device="cuda"))


# --------------------------------------------------------------------------------- ring path

@pytest.fixture(scope="module")
def ring(native):
    """A worker on GPU 0 with two synthetic cameras (640x480, 320x240) and one without frames; the
    host copies of their newest frames are the shared reference."""
    wk = native.Worker(device=0)
    cams, frames = [], []
    for name, (w, h) in {"a": (640, 480), "b": (320, 240)}.items():
        enc = synth(native, w, h, gop=6, motion=0.1)
        cam = wk.add_camera(name, 2)
        for _ in range(3):
            assert wk.decode_now(cam, enc.next())
        cams.append(cam)
        frames.append(wk.read_latest(cam, 0))
    cams.append(wk.add_camera("empty", 2))
    return wk, cams, frames


def test_ring_scaled_jpeg(native, ring):
    wk, cams, frames = ring
    meta, frame = frames[0]
    jmeta, jpg = wk.read_latest_jpeg(cams[0], 0, 85, 320, 180)  # 4:3 into 16:9: 240 x 180
    assert jmeta["seq"] == meta["seq"] and (jmeta["width"], jmeta["height"]) == (240, 180)
    assert jpg == native.jpeg_encode_cpu(native.resize_area_cpu(frame, 240, 180), 85)
    assert wk.read_latest_jpeg(cams[0], 0, 85)[1] == native.jpeg_encode_cpu(frame, 85)  # unscaled: as before
    assert wk.read_latest_jpeg(cams[0], meta["seq"], 85, 320, 180) is None  # nothing newer
    smeta, small = wk.read_latest_scaled(cams[1], 0, 0, 90)
    assert (smeta["width"], smeta["height"]) == (120, 90)
    assert np.array_equal(small, native.resize_area_cpu(frames[1][1], 120, 90))


def test_ring_wall(native, ring):
    wk, cams, frames = ring
    seqs, jpg = wk.read_wall_jpeg(cams, 0, 320, 180, 85)
    assert list(seqs) == [frames[0][0]["seq"], frames[1][0]["seq"], 0]
    want = native.jpeg_encode_cpu(native.compose_wall_cpu([frames[0][1], frames[1][1], None], 0, 320, 180), 85)
    assert jpg == want
    # a tile scaled elsewhere takes a camera's place: same picture
    small = native.resize_area_cpu(frames[0][1], 240, 180)
    seqs, jpg = wk.read_wall_jpeg([-1, cams[1], cams[2]], 0, 320, 180, 85, [(5, small), None, None])
    assert list(seqs) == [5, frames[1][0]["seq"], 0] and jpg == want


def test_concurrent_walls(native, ring):
    wk, cams, frames = ring
    layouts = [(cams, 0, 320, 180), ([cams[1], cams[0]], 1, 160, 120)]
    want = [native.jpeg_encode_cpu(native.compose_wall_cpu([frames[0][1], frames[1][1], None], 0, 320, 180), 85),
            native.jpeg_encode_cpu(native.compose_wall_cpu([frames[1][1], frames[0][1]], 1, 160, 120), 85)]
    bad = []

    def run(k):
        for i in range(20):
            if wk.read_wall_jpeg(*layouts[k], 85)[1] != want[k]:
                bad.append((k, i))

    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not bad
