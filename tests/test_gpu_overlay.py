"""gfx950 on-screen display: byte equality of the kernel with the CPU implementation, pictures at
every byte offset modulo 16 and several pitches inside guarded buffers, batches, and the overlay
reads of a GPU camera against the CPU backend's (run on an MI355X). The CPU implementation is held
to the independent oracle in tests/test_overlay.py."""
import threading

import numpy as np
import pytest
import torch

import overlay_oracle as oo
from conftest import synth
from history_util import avc_stream
from video_edge_ai_proxy_amd import overlay, privacy

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
GUARD = 96
META = {"seq": 4711, "timestamp": 90 * 1790000000123}
LISTS = oo.lists()


def nat(items):
    return overlay.to_native(items)


def want_of(native, p, items):
    out = np.zeros_like(p)
    native.overlay_draw_cpu(p, out, nat(items), "cam-7", META)
    return out


class Guarded:
    """A w x h picture as a strided view (rows of `pitch` bytes, `lead` bytes past a 16-byte
    boundary) between guard bands of a device buffer filled with sentinels."""

    def __init__(self, w, h, pitch, lead, fill=None):
        self.w, self.h, self.pitch = w, h, pitch
        self.at = GUARD + lead
        self.span = (h - 1) * pitch + w * 3
        self.buf = torch.full((self.at + self.span + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.view = torch.as_strided(self.buf, (h, w, 3), (pitch, 3, 1), self.at)
        assert self.view.data_ptr() % 16 == lead % 16
        if fill is not None:
            self.view.copy_(torch.from_numpy(fill).cuda())
        self.before = self.buf.cpu().numpy().copy()

    def picture(self):
        host = self.buf.cpu().numpy()
        return np.lib.stride_tricks.as_strided(host[self.at:], (self.h, self.w, 3), (self.pitch, 3, 1)).copy()

    def outside_unchanged(self):
        """Guards and pitch padding: every byte that is not a pixel of the picture."""
        host = self.buf.cpu().numpy()
        mask = np.ones(host.shape, bool)
        for y in range(self.h):
            mask[self.at + y * self.pitch:self.at + y * self.pitch + self.w * 3] = False
        return np.array_equal(host[mask], self.before[mask])

    def unchanged(self):
        return np.array_equal(self.buf.cpu().numpy(), self.before)


def draw_checked(native, p, items, src_lead, dst_lead, src_extra, dst_extra, want=None):
    """ops.overlay_draw out of place and in place on guarded views == the CPU twin; guards, pitch
    padding and (out of place) the source unchanged."""
    from video_edge_ai_proxy_amd import ops

    h, w = p.shape[:2]
    want = want_of(native, p, items) if want is None else want
    src = Guarded(w, h, 3 * w + src_extra, src_lead, p)
    dst = Guarded(w, h, 3 * w + dst_extra, dst_lead)
    assert ops.overlay_draw(src.view, items, out=dst.view, name="cam-7", meta=META) is dst.view
    got = dst.picture()
    assert np.array_equal(got, want), f"{w}x{h} out of place: {int((got != want).sum())} bytes differ"
    assert dst.outside_unchanged() and src.unchanged()
    assert ops.overlay_draw(src.view, items, name="cam-7", meta=META) is src.view
    got = src.picture()
    assert np.array_equal(got, want), f"{w}x{h} in place: {int((got != want).sum())} bytes differ"
    assert src.outside_unchanged()


@pytest.mark.parametrize("size", oo.SMALL, ids=lambda s: "%dx%d" % s)
def test_byte_equal(native, size):
    w, h = size
    p = oo.picture(w, h)
    for k, (name, items) in enumerate(LISTS.items()):
        draw_checked(native, p, items, (5 * k + 1) % 16, (11 * k + 7) % 16, (0, 1, 13)[k % 3], (13, 0, 1)[k % 3])


def test_every_pair_of_offsets(native):
    """Source x destination at every byte offset modulo 16, on 65 x 17 (one tile and one pixel more
    on each axis), out of place; the pitches rotate through 3w, 3w + 1 and 3w + 13."""
    from video_edge_ai_proxy_amd import ops

    p = oo.picture(65, 17)
    items = LISTS["outlines"] + LISTS["text_k1"] + LISTS["three"]
    want = want_of(native, p, items)
    srcs = [Guarded(65, 17, 195 + (0, 1, 13)[a % 3], a, p) for a in range(16)]
    for a in range(16):
        for b in range(16):
            dst = Guarded(65, 17, 195 + (13, 0, 1)[(a + b) % 3], b)
            ops.overlay_draw(srcs[a].view, items, out=dst.view, name="cam-7", meta=META)
            assert np.array_equal(dst.picture(), want), (a, b)
            assert dst.outside_unchanged(), (a, b)
        assert srcs[a].unchanged(), a
    for a in range(16):  # in place at every offset
        ops.overlay_draw(srcs[a].view, items, name="cam-7", meta=META)
        assert np.array_equal(srcs[a].picture(), want) and srcs[a].outside_unchanged(), a


def test_byte_equal_1080p(native):
    p = oo.picture(1920, 1080)
    items = LISTS["outlines"] + LISTS["text_k8"] + LISTS["text_edges"] + LISTS["three"] + [overlay.STAMP]
    draw_checked(native, p, items, 5, 9, 0, 13)
    draw_checked(native, p, oo.dense(), 0, 0, 0, 0)


def test_a_crop_of_a_batch_tensor_and_a_321_wide_picture(native):
    """Picture k of a packed [n, H, W, 3] tensor and a 321-pixel-wide picture: rows at odd addresses."""
    from video_edge_ai_proxy_amd import ops

    a = np.stack([oo.picture(321, 45, seed=k) for k in range(3)])
    dev = torch.from_numpy(a).cuda()
    ops.overlay_draw(dev[1], LISTS["outlines"], name="cam-7", meta=META)
    got = dev.cpu().numpy()
    assert np.array_equal(got[1], want_of(native, a[1], LISTS["outlines"]))
    assert np.array_equal(got[0], a[0]) and np.array_equal(got[2], a[2])


def test_batch_mixed_sizes(native):
    """Five pictures of three sizes with 0, 1 and 256 primitives in one launch, in place and out of
    place mixed."""
    from video_edge_ai_proxy_amd import ops

    sizes = [(200, 120), (17, 9), (64, 48), (200, 120), (17, 9)]
    lists = [oo.dense(), [], LISTS["full"], LISTS["text_k1"], LISTS["three"]]
    assert [len(oo.expand(l, w, h, "cam-7", META)) for l, (w, h) in zip(lists, sizes)][:3] == [256, 0, 1]
    a = [oo.picture(w, h, seed=k) for k, (w, h) in enumerate(sizes)]
    dev = [torch.from_numpy(x).cuda() for x in a]
    outs = [None, torch.zeros_like(dev[1]), None, torch.zeros_like(dev[3]), None]
    res = ops.overlay_draw_batch(dev, lists, outs, name="cam-7", meta=META)
    for k in range(5):
        assert res[k] is (dev[k] if outs[k] is None else outs[k])
        assert np.array_equal(res[k].cpu().numpy(), want_of(native, a[k], lists[k])), f"picture {k}"
        if outs[k] is not None:
            assert np.array_equal(dev[k].cpu().numpy(), a[k])
    assert ops.overlay_draw_batch([], []) == []


def test_batch_of_33(native):
    from video_edge_ai_proxy_amd import ops

    sizes = [(48, 32), (33, 17), (64, 9)]
    names = list(LISTS)
    a = [oo.picture(*sizes[k % 3], seed=k) for k in range(33)]
    lists = [LISTS[names[k % len(names)]] for k in range(33)]
    dev = [torch.from_numpy(x).cuda() for x in a]
    ops.overlay_draw_batch(dev, lists, name="cam-7", meta=META)
    for k in range(33):
        assert np.array_equal(dev[k].cpu().numpy(), want_of(native, a[k], lists[k])), f"picture {k}"


def test_more_callers_than_scratch_sets(native):
    """8 threads, twice the pool's sets, 4 calls each: callers wait for a free set, and every result
    is the CPU's."""
    from video_edge_ai_proxy_amd import ops

    a = [oo.picture(37, 21, seed=k) for k in range(8)]
    items = LISTS["outlines"] + LISTS["text_k1"]
    want = [want_of(native, x, items) for x in a]
    dev = [torch.from_numpy(x).cuda() for x in a]
    torch.cuda.synchronize()
    got, errors = {}, []

    def run(k):
        try:
            for i in range(4):
                got[k, i] = ops.overlay_draw(dev[k], items, out=torch.empty_like(dev[k]), name="cam-7", meta=META)
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


def test_reference_and_argument_checks(native):
    from video_edge_ai_proxy_amd import ops

    p = oo.picture(64, 48)
    x = torch.from_numpy(p)
    good = LISTS["outlines"]
    assert np.array_equal(ops.overlay_draw_reference(x, good, "cam-7", META).numpy(), want_of(native, p, good))
    assert np.array_equal(ops.overlay_draw_reference(x.cuda(), good, "cam-7", META).numpy(), want_of(native, p, good))
    with pytest.raises(ValueError):
        ops.overlay_draw(x, good)  # host tensor
    with pytest.raises(TypeError):
        ops.overlay_draw(x.cuda().float(), good)  # wrong dtype
    with pytest.raises(TypeError):
        ops.overlay_draw(p, good)  # not a tensor
    with pytest.raises(ValueError):
        ops.overlay_draw(x.cuda()[:, :, :2], good)  # wrong shape
    with pytest.raises(ValueError):
        ops.overlay_draw(x.cuda()[0], good)
    with pytest.raises(ValueError):
        ops.overlay_draw(x.cuda()[:, ::2], good)  # pixels not packed
    for bad in ([dict(good[0], x1=0)], [good[0]] * 65, None, good[0], oo.dense() + [good[0]]):
        with pytest.raises(ValueError):
            ops.overlay_draw(x.cuda(), bad)
    d = x.cuda()
    for out in (torch.zeros_like(x), torch.zeros((48, 63, 3), dtype=torch.uint8).cuda(), d[:], d.view(-1)[3:3 + 47 * 192].view(47, 64, 3)):
        with pytest.raises(ValueError):
            ops.overlay_draw(d, good, out=out)
    with pytest.raises(TypeError):
        ops.overlay_draw(d, good, out=torch.zeros((48, 64, 3), dtype=torch.int8).cuda())
    with pytest.raises(ValueError):
        ops.overlay_draw_batch([d, d.clone()], [good])
    with pytest.raises(ValueError):
        ops.overlay_draw_batch([d, d], [good, good])  # one destination twice
    with pytest.raises(TypeError):
        ops.overlay_draw(d, good, meta=7)
    assert np.array_equal(ops.overlay_draw(d, []).cpu().numpy(), p)


# ----------------------------------------------------------------------------------- the ring

ITEMS = [{"x0": 1000, "y0": 2000, "x1": 6000, "y1": 9000, "label": "person 87%", "alpha": 160},
         {"x0": 5000, "y0": 500, "x1": 9900, "y1": 6000, "color": [0, 0, 255], "thickness": 2, "label": "{name} {seq}"},
         overlay.STAMP]
MASKS = [{"x0": 1000, "y0": 500, "x1": 6100, "y1": 7300, "mode": "pixelate", "block": 16},
         {"x0": 5000, "y0": 6000, "x1": 10000, "y1": 10000, "mode": "fill", "b": 9, "g": 99, "r": 199}]


def _feeds(native):
    def fast(wk, cam):  # I_PCM / P_Skip: one picture per job
        enc = synth(native, 320, 240, gop=3, motion=0.2)
        for _ in range(4):
            assert wk.decode_now(cam, enc.next())

    h264 = avc_stream(native, 12)[0]

    def general(wk, cam):
        wk.decode_many([(cam, h264[:9])])
        for au in h264[9:]:
            wk.decode_now(cam, au)

    return {"fast": fast, "h264": general}


def _answers(native, device, feed, masks):
    wk = native.Worker(device=device)
    cam = wk.add_camera("c", 2)
    other = wk.add_camera("o", 2)
    if masks:
        wk.set_privacy_masks(cam, privacy.to_native(masks))
    feed(wk, cam)
    assert wk.decode_now(other, synth(native, 160, 96, gop=3, motion=0.2, seed=5).next())
    before = wk.read_latest(cam, 0)
    out = {"native": wk.read_overlay_jpeg(cam, nat(ITEMS), "gate", quality=80),
           "scaled": wk.read_overlay_jpeg(cam, nat(ITEMS), "gate", quality=80, width=161),
           "wall": wk.read_wall_jpeg([cam, other, -1], 2, 160, 120, 85, None, ["north gate", "o", "none"])}
    after = wk.read_latest(cam, 0)
    assert after[0]["seq"] == before[0]["seq"] and np.array_equal(after[1], before[1]), "the slot's bytes changed"
    return before, out


@pytest.mark.parametrize("path", ["fast", "h264"])
@pytest.mark.parametrize("masked", [False, True])
def test_ring_overlays_equal_the_cpu_backend(native, path, masked):
    feed = _feeds(native)[path]
    masks = MASKS if masked else None
    (mg, fg), gpu = _answers(native, 0, feed, masks)
    (mc, fc), cpu = _answers(native, -1, feed, masks)
    assert mg["seq"] == mc["seq"] and mg["timestamp"] == mc["timestamp"] and np.array_equal(fg, fc)
    for key in ("native", "scaled"):
        for f in ("seq", "timestamp", "width", "height"):  # (the other fields are wall-clock times)
            assert gpu[key][0][f] == cpu[key][0][f], (key, f)
        assert gpu[key][0]["seq"] == mg["seq"]
        assert gpu[key][1] == cpu[key][1], f"{path} {key}: GPU and CPU backends differ"
    want = np.zeros_like(fg)
    native.overlay_draw_cpu(fg, want, nat(ITEMS), "gate", mg)
    assert gpu["native"][1] == native.jpeg_encode_cpu(want, 80) and not np.array_equal(want, fg)
    assert gpu["wall"][0] == cpu["wall"][0] and gpu["wall"][1] == cpu["wall"][1]
    if masked:  # drawn over the masked picture, not over the raw one
        (_, raw), _ = _answers(native, 0, feed, None)
        assert not np.array_equal(raw, fg)


class _NoSession:
    def stop(self):
        pass


def test_hub_overlay_on_the_gpu(native, tmp_path):
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    hub = Hub(cfg, devices=[0])
    try:
        wk = hub.workers[0]
        frames, metas = {}, {}
        for k, (name, w, h) in enumerate([("a", 320, 240), ("b", 640, 480)]):
            cam = wk.add_camera(name, 2)
            hub.cameras[name] = CameraHandle(name, 0, cam, "", session=_NoSession())
            assert wk.decode_now(cam, synth(native, w, h, gop=6, motion=0.2, seed=k + 1).next())
            metas[name], frames[name] = wk.read_latest(cam, 0)
        hub.set_overlay("b", ITEMS[:2])
        m, jpg = hub.latest_jpeg("b", quality=75, overlay=True, stamp=True)
        want = np.zeros_like(frames["b"])
        native.overlay_draw_cpu(frames["b"], want, nat(ITEMS), "b", metas["b"])
        assert jpg == native.jpeg_encode_cpu(want, 75)
        assert hub.latest_jpeg("b", quality=75)[1] == native.jpeg_encode_cpu(frames["b"], 75)
        assert np.array_equal(wk.read_latest(hub.cameras["b"].cam, 0)[1], frames["b"])
        assert hub.overlay_counts()[0] == 1
    finally:
        hub.shutdown()
