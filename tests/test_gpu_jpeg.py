"""gfx950 JPEG encoder: byte equality with the CPU encoder (run on an MI355X)."""
import threading

import numpy as np
import pytest
import torch

from conftest import synth

pytestmark = pytest.mark.gpu

SMALL = [(16, 16), (17, 9), (1, 1), (48, 32), (200, 120)]  # (w, h)
QUALITIES = [1, 50, 85, 100]


def picture(kind: str, w: int, h: int) -> torch.Tensor:
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "noise":
        img = np.random.default_rng(w * 7919 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif kind == "gradient":
        img = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(w + h - 2, 1)],
                       -1).astype(np.uint8)
    elif kind == "checkerboard":
        img = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    else:
        img = np.full((h, w, 3), 77, np.uint8)
    return torch.from_numpy(np.ascontiguousarray(img))


@pytest.mark.parametrize("kind", ["noise", "gradient", "checkerboard", "constant"])
@pytest.mark.parametrize("w,h", SMALL)
def test_small_pictures_byte_equal(kind, w, h):
    from video_edge_ai_proxy_amd import ops

    x = picture(kind, w, h)
    xd = x.cuda()
    for q in QUALITIES:
        want = ops.jpeg_encode_reference(x, q)
        got = ops.jpeg_encode(xd, q)
        assert got == want, f"{kind} {w}x{h} q{q}: {len(got)} vs {len(want)} bytes"


@pytest.mark.parametrize("kind,q", [("noise", 100), ("gradient", 85)])
def test_1080p_byte_equal(kind, q):
    from video_edge_ai_proxy_amd import ops

    x = picture(kind, 1920, 1080)
    assert ops.jpeg_encode(x.cuda(), q) == ops.jpeg_encode_reference(x, q)


def test_argument_checks():
    from video_edge_ai_proxy_amd import ops

    x = torch.zeros((16, 16, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.jpeg_encode(x, 85)  # host tensor
    with pytest.raises(ValueError):
        ops.jpeg_encode(x.cuda(), 0)
    with pytest.raises(ValueError):
        ops.jpeg_encode(x.cuda(), 101)
    with pytest.raises(TypeError):
        ops.jpeg_encode(x.cuda().float(), 85)
    with pytest.raises(ValueError):
        ops.jpeg_encode(x.cuda()[:, ::2], 85)  # not contiguous


def test_ring_path(native):
    enc = synth(native, 640, 480, gop=6, motion=0.1)
    wk = native.Worker(device=0)
    cam = wk.add_camera("c", 2)
    for _ in range(3):
        assert wk.decode_now(cam, enc.next())
    meta, frame = wk.read_latest(cam, 0)
    jmeta, jpg = wk.read_latest_jpeg(cam, 0, 85)
    assert jmeta["seq"] == meta["seq"]
    assert jpg == native.jpeg_encode_cpu(frame, 85)
    assert wk.read_latest_jpeg(cam, meta["seq"], 85) is None  # nothing newer


def test_concurrent_encodes():
    from video_edge_ai_proxy_amd import ops

    pics = [picture("noise", 200, 120), picture("gradient", 320, 176)]
    want = [ops.jpeg_encode_reference(p, 85) for p in pics]
    dev = [p.cuda() for p in pics]
    torch.cuda.synchronize()
    bad = []

    def run(k):
        for i in range(20):
            if ops.jpeg_encode(dev[k], 85) != want[k]:
                bad.append((k, i))

    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not bad


def test_more_callers_than_scratch_sets():
    """8 threads, twice the pool's sets, 4 encodes each of a 17 x 9 picture: callers wait for a free
    set, and every stream is the CPU's."""
    from video_edge_ai_proxy_amd import ops

    kinds = ["noise", "gradient", "checkerboard", "constant"]
    pics = [picture(kinds[k % 4], 17, 9) for k in range(8)]
    want = [ops.jpeg_encode_reference(p, 50 + 5 * k) for k, p in enumerate(pics)]
    dev = [p.cuda() for p in pics]
    torch.cuda.synchronize()
    got, errors = {}, []

    def run(k):
        try:
            for i in range(4):
                got[k, i] = ops.jpeg_encode(dev[k], 50 + 5 * k)
        except Exception as e:
            errors.append(e)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors and len(got) == 32
    for (k, i), g in got.items():
        assert g == want[k], f"thread {k} call {i}"


def test_scratch_grows_and_comes_back():
    """16 x 16, then 64 x 48 (a larger scratch), then 16 x 16 again: all three exact."""
    from video_edge_ai_proxy_amd import ops

    for w, h in ((16, 16), (64, 48), (16, 16)):
        x = picture("noise", w, h)
        assert ops.jpeg_encode(x.cuda(), 85) == ops.jpeg_encode_reference(x, 85), f"{w}x{h}"
