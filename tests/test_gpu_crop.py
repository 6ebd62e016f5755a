"""gfx950 crops: byte equality of the kernel with the CPU implementation, sources and outputs at
every byte offset modulo 16 inside guarded buffers, batches, and the ring reads of a GPU camera
against the CPU backend's (run on an MI355X). The CPU implementation is held to the independent
oracle in tests/test_crop.py."""
import threading

import numpy as np
import pytest
import torch

import crop_oracle as co
from conftest import synth
from history_util import avc_stream
from video_edge_ai_proxy_amd import crops, privacy

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
GUARD = 96


def nb(boxes):
    return crops.to_native(boxes)


def device_view(p, lead):
    """The picture as a view into a larger device buffer, `lead` bytes past a 16-byte boundary."""
    h, w = p.shape[:2]
    buf = torch.zeros((GUARD + lead + h * w * 3 + GUARD,), dtype=torch.uint8, device="cuda")
    view = buf[GUARD + lead:GUARD + lead + h * w * 3].view(h, w, 3)
    view.copy_(torch.from_numpy(p))
    assert view.data_ptr() % 16 == lead
    return view


def run_guarded(src, boxes, W, H, fit, pad, lead):
    """ops.crop_resize into a view `lead` bytes past a 16-byte boundary of a buffer of sentinels.
    Returns the crops; asserts that not one guard byte before or after them was written."""
    from video_edge_ai_proxy_amd import ops

    n = len(boxes) * H * W * 3
    buf = torch.full((GUARD + lead + n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[GUARD + lead:GUARD + lead + n].view(len(boxes), H, W, 3)
    assert out.data_ptr() % 16 == lead
    assert ops.crop_resize(src, boxes, W, H, fit, pad, out=out) is out
    host = buf.cpu().numpy()
    assert (host[:GUARD + lead] == SENTINEL).all() and (host[GUARD + lead + n:] == SENTINEL).all(), "guard bytes written"
    return host[GUARD + lead:GUARD + lead + n].reshape(len(boxes), H, W, 3)


def check(native, p, views, boxes, W, H, fit, pad, k):
    """kernel == CPU twin, byte for byte, the source at offset k and the output at offset 7k + 3
    modulo 16 (every pair of offsets comes up over 16 x 16 calls)."""
    got = run_guarded(views[k % 16], boxes, W, H, fit, pad, (7 * (k // 16) + k + 3) % 16)
    want = native.crop_resize_cpu(p, nb(boxes), W, H, crops.fit_index(fit), tuple(pad))
    assert np.array_equal(got, want), f"{p.shape} -> {W}x{H} {fit}: {int((got != want).sum())} bytes differ"


@pytest.mark.parametrize("size", co.SMALL)
def test_byte_equal(native, size):
    w, h = size
    p = co.picture("noise", w, h, seed=w + h)
    views = [device_view(p, lead) for lead in range(16)]
    k = 0
    for boxes, W, H, fit, pad in co.cases(w, h):
        check(native, p, views, boxes, W, H, fit, pad, k)
        k += 1
    assert k >= 32 or w * h < 10
    check(native, p, views, co.boxes_of(w, h)[1:2], 4096, 1, "stretch", co.PAD, k)


def test_every_pair_of_offsets(native):
    """Source at every offset modulo 16 x output at every offset modulo 16, reduce and enlarge."""
    p = co.picture("noise", 64, 48, seed=6)
    views = [device_view(p, lead) for lead in range(16)]
    boxes = [co.WHOLE, co.rect_box(64, 48, 3, 1, 40, 30), co.rect_box(64, 48, 5, 7, 13, 12)]
    for W, H, fit in [(23, 17, "stretch"), (70, 50, "letterbox")]:
        want = native.crop_resize_cpu(p, nb(boxes), W, H, crops.fit_index(fit), co.PAD)
        for a in range(16):
            for b in range(16):
                got = run_guarded(views[a], boxes, W, H, fit, co.PAD, b)
                assert np.array_equal(got, want), (W, H, a, b)


def test_byte_equal_1080p(native):
    p = co.picture("noise", 1920, 1080, seed=5)
    views = {5: device_view(p, 5)}
    boxes = [co.WHOLE, co.rect_box(1920, 1080, 1, 3, 482, 271), co.rect_box(1920, 1080, 1437, 700, 1477, 740),
             co.rect_box(1920, 1080, 1919, 1079, 1920, 1080)]
    check(native, p, views, boxes, 224, 224, "stretch", co.PAD, 5)
    check(native, p, views, boxes, 224, 224, "letterbox", (1, 2, 250), 5)
    check(native, p, views, boxes[:2], 1921, 1079, "stretch", co.PAD, 5)  # x enlarges, y reduces, many tiles


def test_byte_equal_wide_path(native):
    """9000 x 3 -> 10 x 1024: Dx * Dy above kNarrowArea (64-bit accumulators), a footprint wider
    than the LDS buffer (staged in segments), x reducing while y enlarges."""
    p = co.picture("noise", 9000, 3, seed=4)
    views = {2: device_view(p, 2)}
    check(native, p, views, [co.WHOLE, co.rect_box(9000, 3, 1, 0, 9000, 3)], 10, 1024, "stretch", co.PAD, 2)
    w = co.picture("white", 9000, 3)
    assert (run_guarded(device_view(w, 9), [co.WHOLE], 10, 1024, "stretch", co.PAD, 1) == 255).all()


def test_closed_forms_on_the_gpu(native):
    p = co.picture("noise", 64, 48, seed=2)
    v = device_view(p, 11)
    assert np.array_equal(run_guarded(v, [co.WHOLE], 64, 48, "stretch", co.PAD, 3)[0], p)  # identity
    two = np.array([[[0, 0, 0], [255, 255, 255]]], np.uint8)
    assert run_guarded(device_view(two, 1), [co.WHOLE], 4, 1, "stretch", co.PAD, 5)[0, 0, :, 1].tolist() == [0, 64, 191, 255]
    one = np.array([[[7, 99, 250]]], np.uint8)
    assert (run_guarded(device_view(one, 15), [co.WHOLE], 4096, 1, "stretch", co.PAD, 15) == one[0, 0]).all()
    u = np.full((9, 17, 3), (3, 201, 255), np.uint8)
    assert (run_guarded(device_view(u, 4), [co.WHOLE], 224, 224, "stretch", co.PAD, 9) == u[0, 0]).all()


def _many_boxes(w, h, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        out.append(co.rect_box(w, h, x0, y0, int(rng.integers(x0 + 1, w + 1)), int(rng.integers(y0 + 1, h + 1))))
    return out


def test_batch_mixed_sizes(native):
    """Five pictures of three sizes with 0, 1 and 64 boxes in one launch; the boxes of the small
    pictures enlarge while those of the large ones reduce."""
    from video_edge_ai_proxy_amd import ops

    sizes = [(200, 120), (17, 9), (64, 48), (200, 120), (17, 9)]
    lists = [_many_boxes(200, 120, 64, 1), [], [co.WHOLE], [co.rect_box(200, 120, 3, 5, 190, 111)], _many_boxes(17, 9, 64, 2)]
    a = [co.picture("noise", w, h, seed=k) for k, (w, h) in enumerate(sizes)]
    dev = [torch.from_numpy(x).cuda() for x in a]
    for W, H, fit in [(40, 30, "stretch"), (33, 65, "letterbox")]:
        got = ops.crop_resize_batch(dev, lists, W, H, fit, (4, 5, 6)).cpu().numpy()
        assert got.shape == (130, H, W, 3)
        at = 0
        for k in range(5):
            want = native.crop_resize_cpu(a[k], nb(lists[k]), W, H, crops.fit_index(fit), (4, 5, 6))
            assert np.array_equal(got[at:at + len(lists[k])], want), f"picture {k}"
            at += len(lists[k])
    assert ops.crop_resize_batch(dev, [[]] * 5, 8, 8).shape == (0, 8, 8, 3)


def test_batch_of_33(native):
    from video_edge_ai_proxy_amd import ops

    sizes = [(48, 32), (33, 17), (64, 9)]
    a = [co.picture("noise", *sizes[k % 3], seed=k) for k in range(33)]
    lists = [_many_boxes(*sizes[k % 3], 1 + k % 3, 10 + k) for k in range(33)]
    got = ops.crop_resize_batch([torch.from_numpy(x).cuda() for x in a], lists, 36, 20).cpu().numpy()
    at = 0
    for k in range(33):
        want = native.crop_resize_cpu(a[k], nb(lists[k]), 36, 20)
        assert np.array_equal(got[at:at + len(lists[k])], want), f"picture {k}"
        at += len(lists[k])
    assert at == got.shape[0] == 66


def test_more_callers_than_scratch_sets(native):
    """8 threads, twice the pool's sets, 4 calls each: callers wait for a free set, and every result
    is the CPU's."""
    from video_edge_ai_proxy_amd import ops

    a = [co.picture("noise", 37, 21, seed=k) for k in range(8)]
    boxes = _many_boxes(37, 21, 5, 3)
    want = [native.crop_resize_cpu(x, nb(boxes), 50, 12) for x in a]
    dev = [torch.from_numpy(x).cuda() for x in a]
    torch.cuda.synchronize()
    got, errors = {}, []

    def run(k):
        try:
            for i in range(4):
                got[k, i] = ops.crop_resize(dev[k], boxes, 50, 12)
        except Exception as e:
            errors.append(e)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors and len(got) == 32
    for (k, i), g in got.items():
        assert np.array_equal(g.cpu().numpy(), want[k]), f"thread {k} call {i}"


def test_argument_checks():
    from video_edge_ai_proxy_amd import ops

    x = torch.zeros((16, 16, 3), dtype=torch.uint8)
    good = [{"x0": 0, "y0": 0, "x1": 5000, "y1": 5000}]
    with pytest.raises(ValueError):
        ops.crop_resize(x, good, 4, 4)  # host tensor
    with pytest.raises(TypeError):
        ops.crop_resize(x.cuda().float(), good, 4, 4)  # wrong dtype
    with pytest.raises(ValueError):
        ops.crop_resize(x.cuda()[:, :, :2], good, 4, 4)  # wrong shape
    with pytest.raises(ValueError):
        ops.crop_resize(x.cuda()[0], good, 4, 4)
    with pytest.raises(ValueError):
        ops.crop_resize(x.cuda()[:, ::2], good, 4, 4)  # not contiguous
    for bad in ([dict(good[0], x1=0)], good * 65, None, good[0]):
        with pytest.raises(ValueError):
            ops.crop_resize(x.cuda(), bad, 4, 4)
    for kw in (dict(width=0), dict(height=4097), dict(fit="zoom"), dict(pad=(1, 2)), dict(pad=(1, 2, 256))):
        args = dict(width=4, height=4)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.crop_resize(x.cuda(), good, **args)
    for out in (torch.zeros((1, 4, 4, 3), dtype=torch.uint8), torch.zeros((2, 4, 4, 3), dtype=torch.uint8).cuda(),
                torch.zeros((1, 4, 4, 3), dtype=torch.int8).cuda(), torch.zeros((1, 4, 8, 3), dtype=torch.uint8).cuda()[:, :, ::2]):
        with pytest.raises(ValueError):
            ops.crop_resize(x.cuda(), good, 4, 4, out=out)
    with pytest.raises(ValueError):
        ops.crop_resize_batch([x.cuda(), x.cuda()], [good], 4, 4)
    with pytest.raises(ValueError):
        ops.crop_resize_batch([x.cuda(), x], [good, good], 4, 4)
    assert ops.crop_resize(x.cuda(), [], 4, 4).shape == (0, 4, 4, 3)


# ----------------------------------------------------------------------------------- the ring

BOXES = [co.WHOLE, {"x0": 1000, "y0": 500, "x1": 6100, "y1": 7300}, {"x0": 4000, "y0": 4000, "x1": 4400, "y1": 4500},
         {"x0": 9990, "y0": 9990, "x1": 10000, "y1": 10000}]
MASKS = [{"x0": 1000, "y0": 500, "x1": 6100, "y1": 7300, "mode": "pixelate", "block": 16},
         {"x0": 5000, "y0": 6000, "x1": 10000, "y1": 10000, "mode": "fill", "b": 9, "g": 99, "r": 199}]


def _feeds(native):
    def fast(wk, cam):  # I_PCM / P_Skip: one picture per job
        enc = synth(native, 320, 240, gop=3, motion=0.2)
        for _ in range(4):
            assert wk.decode_now(cam, enc.next())

    h264 = avc_stream(native, 12)[0]

    def general(wk, cam):  # one job of many pictures: its earlier outputs are history conversions
        wk.decode_many([(cam, h264[:9])])
        for au in h264[9:]:
            wk.decode_now(cam, au)

    return {"fast": (fast, 3), "h264": (general, 5)}


def _answers(native, device, feed, history, masks):
    """What a camera of a worker on `device` answers after `feed`: its history, and for the newest
    frame (seq 0) and every frame of the history the crops and one crop as a JPEG."""
    wk = native.Worker(device=device)
    cam = wk.add_camera("c", wk.history_ring_slots(history), history)
    if masks:
        wk.set_privacy_masks(cam, privacy.to_native(masks))
    feed(wk, cam)
    frames = wk.read_history(cam, 0, history)
    out = {}
    for seq in [0] + [m["seq"] for m, _ in frames]:
        out[seq] = (wk.read_crops(cam, nb(BOXES), 96, 64, seq=seq),
                    wk.read_crops(cam, nb(BOXES), 400, 300, seq=seq, fit=1, pad=(9, 8, 7)),
                    wk.read_crop_jpeg(cam, nb(BOXES)[1], 224, 224, seq=seq, quality=80))
    assert frames[0][0]["seq"] > 1  # (seq 0 would mean the newest frame)
    gone = wk.read_crops(cam, nb(BOXES), 8, 8, seq=frames[0][0]["seq"] - 1)
    return frames, out, gone


@pytest.mark.parametrize("path", ["fast", "h264"])
@pytest.mark.parametrize("masked", [False, True])
def test_ring_crops_equal_the_cpu_backend(native, path, masked):
    feed, history = _feeds(native)[path]
    masks = MASKS if masked else None
    fg, gpu, gone_g = _answers(native, 0, feed, history, masks)
    fc, cpu, gone_c = _answers(native, -1, feed, history, masks)
    assert len(fg) == len(fc) == history and list(gpu) == list(cpu) and gone_g is None and gone_c is None
    by_seq = {m["seq"]: f for m, f in fg}
    newest = max(by_seq)
    for seq in gpu:
        for g, c in zip(gpu[seq][:2], cpu[seq][:2]):
            assert g[0]["seq"] == c[0]["seq"] == (seq or newest)
            assert np.array_equal(g[1], c[1]), f"{path} seq {seq}: GPU and CPU backends differ"
        frame = by_seq[seq or newest]
        assert np.array_equal(gpu[seq][0][1], native.crop_resize_cpu(frame, nb(BOXES), 96, 64))
        assert gpu[seq][2][0]["seq"] == (seq or newest) and gpu[seq][2][1] == cpu[seq][2][1]
        assert gpu[seq][2][1] == native.jpeg_encode_cpu(native.crop_resize_cpu(frame, nb(BOXES)[1:2], 224, 224)[0], 80)
    if masked:  # the crops show the masks: they are the crops of the masked frame, not of the raw one
        raw, _, _ = _answers(native, 0, feed, history, None)
        assert not np.array_equal(raw[-1][1], fg[-1][1])
        assert not np.array_equal(native.crop_resize_cpu(raw[-1][1], nb(BOXES), 96, 64)[:2], gpu[0][0][1][:2])


def test_mask_change_leaves_no_crop_readable(native):
    wk = native.Worker(device=0)
    cam = wk.add_camera("c", wk.history_ring_slots(3), 3)
    enc = synth(native, 320, 240, gop=6, motion=0.2)
    assert wk.decode_now(cam, enc.next()) and wk.decode_now(cam, enc.next())
    assert wk.read_crops(cam, nb(BOXES), 32, 32)[0]["seq"] == 2 and wk.read_crops(cam, nb(BOXES), 32, 32, seq=1) is not None
    wk.set_privacy_masks(cam, privacy.to_native(MASKS))
    assert wk.read_crops(cam, nb(BOXES), 32, 32) is None and wk.read_crops(cam, nb(BOXES), 32, 32, seq=1) is None
    assert wk.read_crop_jpeg(cam, nb(BOXES)[0], 32, 32) is None
    assert wk.decode_now(cam, enc.next())
    m, got = wk.read_crops(cam, nb(BOXES), 32, 32)
    assert m["seq"] == 3 and np.array_equal(got, native.crop_resize_cpu(wk.read_latest(cam, 0)[1], nb(BOXES), 32, 32))


class _NoSession:
    def stop(self):
        pass


def test_hub_crops_many_on_the_gpu(native, tmp_path):
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    hub = Hub(cfg, devices=[0])
    try:
        frames = {}
        for k, (name, w, h) in enumerate([("a", 320, 240), ("b", 160, 96), ("c", 640, 480)]):
            wk = hub.workers[0]
            cam = wk.add_camera(name, 2)
            hub.cameras[name] = CameraHandle(name, 0, cam, "", session=_NoSession())
            enc = synth(native, w, h, gop=6, motion=0.2, seed=k + 1)
            assert wk.decode_now(cam, enc.next())
            frames[name] = wk.read_latest(cam, 0)[1]
        lists = {"c": BOXES[:2], "b": BOXES, "a": BOXES[2:]}
        many = hub.crops_many(lists, 112, 112, fit="letterbox")
        for n, bs in lists.items():
            assert many[n][0] == 1 and np.array_equal(many[n][1], co.crop_resize(frames[n], bs, 112, 112, "letterbox"))
        seq, got = hub.crops("c", BOXES, 224, 224)
        assert seq == 1 and np.array_equal(got, co.crop_resize(frames["c"], BOXES, 224, 224))
        seq, jpg = hub.crop_jpeg("c", BOXES[1], 320, 240, quality=75)
        assert jpg == native.jpeg_encode_cpu(co.crop_resize(frames["c"], BOXES[1:2], 320, 240)[0], 75)
    finally:
        hub.shutdown()
