"""Crops on the CPU: the header's arithmetic (native.crop_taps / crop_fit) and the twin
(csrc/vep/crop.cpp) against the independent numpy oracle (crop_oracle.py), closed forms, the
scale oracle and torch's bilinear interpolation, then the Worker's CPU backend, the Hub, REST,
the config, /metrics and the CLI."""
import time

import numpy as np
import pytest
import torch

import crop_oracle as co
import jpeg_oracle as jo
import mask_oracle as mo
import scale_oracle as so
from conftest import synth
from video_edge_ai_proxy_amd import crops, ops, privacy


def nb(boxes):
    return crops.to_native(boxes)


def twin(native, p, boxes, W, H, fit="stretch", pad=co.PAD):
    return native.crop_resize_cpu(p, nb(boxes), W, H, crops.fit_index(fit), tuple(pad))


def check(native, p, boxes, W, H, fit="stretch", pad=co.PAD):
    got, want = twin(native, p, boxes, W, H, fit, pad), co.crop_resize(p, boxes, W, H, fit, pad)
    assert got.shape == want.shape == (len(boxes), H, W, 3)
    assert np.array_equal(got, want), (p.shape, W, H, fit, int((got != want).sum()))
    return got


# ----------------------------------------------------------------------------- the arithmetic

def test_taps_equal_the_oracle(native):
    pairs = [(s, o) for s in range(1, 41) for o in range(1, 41)]
    pairs += [(1, 4096), (65535, 1), (65535, 4096), (4095, 4096), (4096, 4095)]
    for s, o in pairs:
        D, taps = native.crop_taps(s, o)
        wantD, want = co.taps(s, o)
        assert D == wantD == (s if o <= s else 2 * o)
        assert [tuple(t) for t in taps] == want, (s, o)
        sums = np.zeros(o, np.int64)
        t = np.array(taps, np.int64)
        np.add.at(sums, t[:, 0], t[:, 2])
        assert (sums == D).all() and t[:, 1].min() >= 0 and t[:, 1].max() <= s - 1 and t[:, 2].min() >= 0, (s, o)


def test_taps_products_stay_in_32_bits():
    assert 8191 * 65535 < 2 ** 31  # (2j + 1) * s at j = 4095, s = 65535
    assert 255 * 65535 < 2 ** 32 and 255 * 2 * 4096 < 2 ** 32  # a row's weighted sum


def test_fit_equals_the_oracle(native):
    sides = [1, 2, 3, 7, 16, 100, 1080, 1920, 4096]
    for sw in sides + [65535]:
        for sh in sides + [65535]:
            for W in sides:
                for H in sides:
                    got = tuple(native.crop_fit(sw, sh, W, H))
                    assert got == co.fitted(sw, sh, W, H, "letterbox"), (sw, sh, W, H)
                    x, y, fw, fh = got
                    assert fw >= 1 and fh >= 1 and x >= 0 and y >= 0 and x + fw <= W and y + fh <= H
                    assert fw == W or fh == H
    assert tuple(native.crop_fit(100, 50, 64, 64)) == (0, 16, 64, 32)
    assert tuple(native.crop_fit(50, 100, 64, 64)) == (16, 0, 32, 64)


def test_pixels_round_outward(native):
    assert native.crop_pixels(1920, 1080, (1, 1, 9999, 9999)) == (0, 0, 1920, 1080)
    assert native.crop_pixels(1920, 1080, (5000, 5000, 5001, 5001)) == (960, 540, 961, 541)
    for w, h in co.SMALL:
        for b in co.boxes_of(w, h):
            assert native.crop_pixels(w, h, nb([b])[0]) == co.to_pixels(w, h, b) == mo.to_pixels(w, h, b)


# ----------------------------------------------------------------------------- twin == oracle

@pytest.mark.parametrize("size", co.SMALL)
def test_twin_equals_oracle(native, size):
    w, h = size
    p = co.picture("noise", w, h, seed=w + h)
    for boxes, W, H, fit, pad in co.cases(w, h):
        check(native, p, boxes, W, H, fit, pad)
    check(native, co.picture("gradient", w, h), co.boxes_of(w, h)[:8], 16, 16)
    check(native, p, co.boxes_of(w, h)[1:2], 4096, 1)


def test_twin_equals_oracle_1080p(native):
    p = co.picture("noise", 1920, 1080, seed=5)
    boxes = [co.WHOLE, co.rect_box(1920, 1080, 1, 3, 482, 271), co.rect_box(1920, 1080, 1437, 700, 1477, 740),
             co.rect_box(1920, 1080, 1919, 1079, 1920, 1080)]
    check(native, p, boxes, 224, 224)
    check(native, p, boxes[1:], 224, 224, "letterbox", (1, 2, 250))


def test_wide_path(native):
    """Dx * Dy = 9000 * 2048 is above scale's kNarrowArea with x reducing and y enlarging: the
    64-bit accumulator, on an 81 KB picture."""
    assert 9000 * 2048 > 16843009
    p = co.picture("noise", 9000, 3, seed=4)
    check(native, p, [co.WHOLE, co.rect_box(9000, 3, 1, 0, 9000, 3)], 10, 1024)
    got = twin(native, co.picture("white", 9000, 3), [co.WHOLE], 10, 1024)
    assert (got == 255).all()


# ----------------------------------------------------------------------------- closed forms

def test_identity_returns_the_bytes(native):
    for w, h in co.SMALL:
        p = co.picture("noise", w, h, seed=1)
        assert np.array_equal(twin(native, p, [co.WHOLE], w, h)[0], p)
    p = co.picture("noise", 64, 48, seed=2)
    b = co.rect_box(64, 48, 5, 3, 42, 40)
    assert np.array_equal(twin(native, p, [b], 37, 37)[0], p[3:40, 5:42])


def test_uniform_stays_uniform(native):
    p = np.full((9, 17, 3), (3, 201, 255), np.uint8)
    for W, H in [(1, 1), (5, 30), (224, 224), (16, 9), (18, 8), (4096, 1)]:
        got = twin(native, p, [co.WHOLE, co.rect_box(17, 9, 2, 1, 9, 8)], W, H)
        assert (got == np.array((3, 201, 255), np.uint8)).all(), (W, H)


def test_two_pixels_enlarged_to_four(native):
    p = np.array([[[0, 0, 0], [255, 255, 255]]], np.uint8)
    got = twin(native, p, [co.WHOLE], 4, 1)[0, 0]
    assert got[:, 0].tolist() == got[:, 2].tolist() == [0, 64, 191, 255]


def test_integer_ratio_is_the_block_mean(native):
    p = co.picture("noise", 12, 8, seed=9)
    got = twin(native, p, [co.WHOLE], 4, 2)[0]
    s = p.astype(np.int64).reshape(2, 4, 4, 3, 3).sum(axis=(1, 3))
    assert np.array_equal(got, ((s + 6) // 12).astype(np.uint8))


def test_one_pixel_enlarged_is_constant(native):
    p = np.array([[[7, 99, 250]]], np.uint8)
    got = twin(native, p, [co.WHOLE], 4096, 1)
    assert got.shape == (1, 1, 4096, 3) and (got == p[0, 0]).all()


def test_reduce_only_equals_the_scale_oracle(native):
    for sw, sh, ow, oh in so.SMALL_SHAPES + [(1920, 1080, 320, 180)]:
        p = so.picture("noise", sw, sh, seed=3)
        got = ops.crop_resize_reference(torch.from_numpy(p), [co.WHOLE], ow, oh)[0]
        assert torch.equal(got, ops.resize_area_reference(torch.from_numpy(p), ow, oh)), (sw, sh, ow, oh)
        if sw * sh < 100000:
            assert np.array_equal(got.numpy(), so.resize_area(p, ow, oh))


def test_enlarge_only_against_torch_bilinear(native):
    """The twin and F.interpolate(bilinear, align_corners=False) in float64 are the same rational
    number before the rounding, so the result is within 0.5 (+ float64 error) of the UNROUNDED
    float. Not compared with the rounded float: exact .5 ties round differently."""
    worst, samples = 0.0, 0
    for (sw, sh), (ow, oh) in co.ENLARGE:
        assert ow > sw and oh > sh
        p = co.picture("noise", sw, sh, seed=7)
        got = twin(native, p, [co.WHOLE], ow, oh)[0].astype(np.float64)
        x = torch.from_numpy(p).permute(2, 0, 1)[None].to(torch.float64)
        ref = torch.nn.functional.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False)[0]
        d = np.abs(got - ref.permute(1, 2, 0).numpy())
        worst, samples = max(worst, float(d.max())), samples + d.size
        assert d.max() <= 0.5 + 1e-6, ((sw, sh), (ow, oh), float(d.max()))
    print(f"enlarge vs float64 bilinear: {samples} samples, largest distance {worst!r}")


def test_letterbox(native):
    p = co.picture("noise", 200, 120, seed=8)
    for box, W, H in [(co.WHOLE, 64, 64), (co.WHOLE, 64, 20), (co.rect_box(200, 120, 5, 5, 15, 115), 224, 224),
                      (co.rect_box(200, 120, 0, 50, 200, 51), 16, 16), (co.rect_box(200, 120, 99, 0, 100, 120), 17, 3)]:
        for pad in co.PADS:
            got = check(native, p, [box], W, H, "letterbox", pad)[0]
            x0, y0, x1, y1 = co.to_pixels(200, 120, box)
            fx, fy, fw, fh = co.fitted(x1 - x0, y1 - y0, W, H, "letterbox")
            assert (fx, fy, fw, fh) == tuple(native.crop_fit(x1 - x0, y1 - y0, W, H))
            outside = np.ones((H, W), bool)
            outside[fy:fy + fh, fx:fx + fw] = False
            assert (got[outside] == np.array(pad, np.uint8)).all()
            assert np.array_equal(got[fy:fy + fh, fx:fx + fw], co.resample(p[y0:y1, x0:x1], fw, fh))


# ----------------------------------------------------------------------------- argument checks

GOOD = {"x0": 0, "y0": 0, "x1": 5000, "y1": 5000}
BAD_BOXES = [dict(GOOD, x0=-1), dict(GOOD, x1=10001), dict(GOOD, x0=5000), dict(GOOD, y0=6000), dict(GOOD, y1=0),
             dict(GOOD, x0=1.5), dict(GOOD, x0=True), {"x0": 0, "y0": 0, "x1": 1}, dict(GOOD, z=1), "box", None, (0, 0, 1)]


def test_argument_checks(native):
    p = torch.from_numpy(co.picture("noise", 16, 8))
    for bad in BAD_BOXES:
        with pytest.raises(ValueError):
            crops.to_native([bad])
        with pytest.raises(ValueError):
            ops.crop_resize_reference(p, [bad], 4, 4)
    for bad in (None, GOOD, "boxes", 5, [GOOD] * 65):
        with pytest.raises(ValueError):
            ops.crop_resize_reference(p, bad, 4, 4)
    for kw in (dict(width=0), dict(width=4097), dict(height=0), dict(height=4097), dict(width=4.0), dict(width=True),
               dict(fit="fill"), dict(fit=1), dict(pad=(0, 0)), dict(pad=(0, 0, 256)), dict(pad=(0, -1, 0)),
               dict(pad="114"), dict(pad=(1.0, 2, 3))):
        args = dict(width=4, height=4, fit="stretch", pad=(114, 114, 114))
        args.update(kw)
        with pytest.raises(ValueError):
            ops.crop_resize_reference(p, [GOOD], **args)
    with pytest.raises(TypeError):
        ops.crop_resize_reference(p.to(torch.int32), [GOOD], 4, 4)
    with pytest.raises(TypeError):
        ops.crop_resize_reference(p.numpy(), [GOOD], 4, 4)
    for shape in ((8, 16), (8, 16, 4), (0, 16, 3)):
        with pytest.raises(ValueError):
            ops.crop_resize_reference(torch.zeros(shape, dtype=torch.uint8), [GOOD], 4, 4)
    with pytest.raises(ValueError):
        ops.crop_resize_reference(p[:, ::2], [GOOD], 4, 4)  # not contiguous
    with pytest.raises(ValueError):
        ops.crop_resize(p, [GOOD], 4, 4)  # a host tensor
    # the native layer on its own
    a = p.numpy()
    one = (0, 0, 5000, 5000)
    for boxes, W, H, fit, pad in [([(0, 0, 0, 5)], 4, 4, 0, co.PAD), ([(0, 0, 5, 10001)], 4, 4, 0, co.PAD),
                                  ([(-1, 0, 5, 5)], 4, 4, 0, co.PAD), ([one] * 65, 4, 4, 0, co.PAD),
                                  ([one], 0, 4, 0, co.PAD), ([one], 4, 4097, 0, co.PAD), ([one], 4, 4, 2, co.PAD),
                                  ([one], 4, 4, -1, co.PAD), ([one], 4, 4, 0, (0, 0, 256))]:
        with pytest.raises(ValueError):
            native.crop_resize_cpu(a, boxes, W, H, fit, pad)
    for s, o in [(0, 1), (65536, 1), (1, 0), (1, 4097)]:
        with pytest.raises(ValueError):
            native.crop_taps(s, o)
    for args in [(0, 1, 1, 1), (1, 65536, 1, 1), (1, 1, 0, 1), (1, 1, 1, 4097)]:
        with pytest.raises(ValueError):
            native.crop_fit(*args)
    with pytest.raises(ValueError):
        native.crop_resize_cpu(np.zeros((4, 4), np.uint8), [one], 4, 4)
    assert native.crop_resize_cpu(a, [], 4, 4).shape == (0, 4, 4, 3)


# ----------------------------------------------------------------- the Worker's CPU backend

BOXES = [co.WHOLE, {"x0": 1000, "y0": 500, "x1": 6100, "y1": 7300}, {"x0": 4000, "y0": 4000, "x1": 4400, "y1": 4500},
         {"x0": 9990, "y0": 9990, "x1": 10000, "y1": 10000}]
MASKS = [{"x0": 1000, "y0": 500, "x1": 6100, "y1": 7300, "mode": "pixelate", "block": 16},
         {"x0": 5000, "y0": 6000, "x1": 10000, "y1": 10000, "mode": "fill", "b": 9, "g": 99, "r": 199}]


def _slots(native, history):
    return native.Worker(device=-1).history_ring_slots(history) if history else 2


def _camera(native, history=0, w=320, h=240, masks=None, **kw):
    wk = native.Worker(device=-1)
    cam = wk.add_camera("c", _slots(native, history), history)
    if masks:
        wk.set_privacy_masks(cam, privacy.to_native(masks))
    enc = synth(native, w, h, gop=6, motion=0.2, **kw)
    return wk, cam, lambda: wk.decode_now(cam, enc.next())


def test_worker_crops_equal_the_twin_of_the_frame(native):
    wk, cam, step = _camera(native)
    assert wk.read_crops(cam, nb(BOXES), 64, 48) is None  # no frame yet
    assert step()
    meta, frame = wk.read_latest(cam, 0)
    for W, H, fit, pad in [(64, 48, 0, co.PAD), (224, 224, 1, (1, 2, 3)), (400, 300, 0, co.PAD), (1, 1, 0, co.PAD)]:
        m, got = wk.read_crops(cam, nb(BOXES), W, H, fit=fit, pad=pad)
        assert m["seq"] == meta["seq"] == 1 and got.shape == (len(BOXES), H, W, 3)
        assert np.array_equal(got, native.crop_resize_cpu(frame, nb(BOXES), W, H, fit, pad))
    assert np.array_equal(wk.read_crops(cam, nb(BOXES), 64, 48)[1], co.crop_resize(frame, BOXES, 64, 48))
    m, none = wk.read_crops(cam, [], 8, 8)
    assert m["seq"] == 1 and none.shape == (0, 8, 8, 3)
    # after: only a newer frame answers
    assert wk.read_crops(cam, nb(BOXES), 8, 8, after=1) is None
    assert step()
    m, got = wk.read_crops(cam, nb(BOXES), 8, 8, after=1)
    assert m["seq"] == 2 and np.array_equal(got, native.crop_resize_cpu(wk.read_latest(cam, 0)[1], nb(BOXES), 8, 8))
    with pytest.raises(IndexError):
        wk.read_crops(99, nb(BOXES), 8, 8)
    for kw in (dict(width=0), dict(height=4097), dict(fit=2), dict(pad=(0, 0, 300)), dict(after=-1), dict(seq=-1)):
        args = dict(width=8, height=8)
        args.update(kw)
        with pytest.raises(ValueError):
            wk.read_crops(cam, nb(BOXES), **args)
    with pytest.raises(ValueError):
        wk.read_crops(cam, [(0, 0, 0, 1)], 8, 8)


def test_worker_crops_of_frame_seq(native):
    wk, cam, step = _camera(native, history=5)
    frames = {}
    for _ in range(3):
        assert step()
        m, f = wk.read_latest(cam, 0)
        frames[m["seq"]] = f
    for seq in (1, 2, 3):  # every frame of the history, not only the newest
        m, got = wk.read_crops(cam, nb(BOXES), 32, 32, seq=seq)
        assert m["seq"] == seq and np.array_equal(got, native.crop_resize_cpu(frames[seq], nb(BOXES), 32, 32))
        assert wk.read_crop_jpeg(cam, nb(BOXES)[1], 32, 32, seq=seq, quality=80)[0]["seq"] == seq
    assert wk.read_crops(cam, nb(BOXES), 32, 32, seq=4) is None  # not there yet
    assert wk.read_crops(cam, nb(BOXES), 32, 32, seq=2, after=2) is None  # seq > after holds for both
    assert wk.read_crops(cam, nb(BOXES), 32, 32, seq=3, after=2)[0]["seq"] == 3
    for _ in range(5):
        assert step()
    assert [m["seq"] for m, _ in wk.read_history(cam, 0, 5)] == [4, 5, 6, 7, 8]
    assert wk.read_crops(cam, nb(BOXES), 32, 32, seq=3) is None  # left the ring: no answer
    assert wk.read_crop_jpeg(cam, nb(BOXES)[1], 32, 32, seq=3) is None
    assert wk.read_crops(cam, nb(BOXES), 32, 32, seq=4)[0]["seq"] == 4
    # without a history only the newest frame can be named
    wk2, cam2, step2 = _camera(native)
    assert step2() and step2()
    assert wk2.read_crops(cam2, nb(BOXES), 8, 8, seq=2)[0]["seq"] == 2
    assert wk2.read_crops(cam2, nb(BOXES), 8, 8, seq=1) is None


def test_worker_crops_are_masked(native):
    """Crops read the ring slot, so a masked region is masked in every crop: equal to the twin on
    the masked frame, and different from the crop of the unmasked picture."""
    wk, cam, step = _camera(native, history=3, masks=MASKS)
    plain, pcam, pstep = _camera(native, history=3)
    assert step() and pstep()
    raw = plain.read_latest(pcam, 0)[1]
    want = mo.apply(raw, MASKS)
    assert np.array_equal(wk.read_latest(cam, 0)[1], want) and not np.array_equal(want, raw)
    for seq in (0, 1):
        got = wk.read_crops(cam, nb(BOXES), 96, 96, seq=seq)[1]
        assert np.array_equal(got, native.crop_resize_cpu(want, nb(BOXES), 96, 96))
        assert not np.array_equal(got[:2], native.crop_resize_cpu(raw, nb(BOXES), 96, 96)[:2])
    assert wk.read_crop_jpeg(cam, nb(BOXES)[1], 96, 96, quality=80)[1] == native.jpeg_encode_cpu(
        native.crop_resize_cpu(want, nb(BOXES)[1:2], 96, 96)[0], 80)
    # a mask change leaves nothing readable until the next frame, by seq either
    new = [{"x0": 0, "y0": 0, "x1": 10000, "y1": 10000, "mode": "pixelate", "block": 32}]
    wk.set_privacy_masks(cam, privacy.to_native(new))
    assert wk.read_crops(cam, nb(BOXES), 96, 96) is None and wk.read_crops(cam, nb(BOXES), 96, 96, seq=1) is None
    assert wk.read_crop_jpeg(cam, nb(BOXES)[0], 96, 96) is None
    assert step() and pstep()
    m, got = wk.read_crops(cam, nb(BOXES), 96, 96)
    assert m["seq"] == 2 and wk.read_crops(cam, nb(BOXES), 96, 96, seq=1) is None
    assert np.array_equal(got, native.crop_resize_cpu(mo.apply(plain.read_latest(pcam, 0)[1], new), nb(BOXES), 96, 96))


def test_worker_crops_many(native):
    wk = native.Worker(device=-1)
    a, b = wk.add_camera("a", 2), wk.add_camera("b", 2)
    ea, eb = synth(native, 320, 240, gop=6, motion=0.2), synth(native, 160, 96, gop=6, motion=0.2, seed=3)
    assert wk.decode_now(a, ea.next()) and wk.decode_now(b, eb.next()) and wk.decode_now(b, eb.next())
    fa, fb = wk.read_latest(a, 0)[1], wk.read_latest(b, 0)[1]
    # a repeated camera, an unknown one, an empty list, a cursor that nothing passes
    reqs = [(a, 0, 0, nb(BOXES)), (b, 0, 0, nb(BOXES[:1])), (a, 0, 0, nb(BOXES[2:])), (77, 0, 0, nb(BOXES)),
            (b, 0, 0, []), (b, 2, 0, nb(BOXES)), (-1, 0, 0, nb(BOXES))]
    rs = wk.read_crops_many(reqs, 48, 40, 1, (5, 6, 7))
    assert [r is None for r in rs] == [False, False, False, True, False, True, True]
    assert rs[0][0]["seq"] == 1 and rs[1][0]["seq"] == 2
    assert np.array_equal(rs[0][1], native.crop_resize_cpu(fa, nb(BOXES), 48, 40, 1, (5, 6, 7)))
    assert np.array_equal(rs[1][1], native.crop_resize_cpu(fb, nb(BOXES[:1]), 48, 40, 1, (5, 6, 7)))
    assert np.array_equal(rs[2][1], native.crop_resize_cpu(fa, nb(BOXES[2:]), 48, 40, 1, (5, 6, 7)))
    assert rs[4][1].shape == (0, 40, 48, 3)
    assert wk.read_crops_many([], 8, 8) == []
    with pytest.raises(ValueError):
        wk.read_crops_many([(a, 0, 0, [(5, 5, 5, 6)])], 8, 8)
    with pytest.raises(ValueError):
        wk.read_crops_many(reqs, 8, 0)


def test_worker_crop_jpeg(native):
    wk, cam, step = _camera(native)
    assert step()
    frame = wk.read_latest(cam, 0)[1]
    for box, W, H, fit, q in [(BOXES[1], 224, 224, 0, 85), (BOXES[2], 96, 64, 1, 60), (BOXES[0], 33, 17, 0, 100)]:
        m, jpg = wk.read_crop_jpeg(cam, nb([box])[0], W, H, quality=q, fit=fit)
        want = native.crop_resize_cpu(frame, nb([box]), W, H, fit)[0]
        assert m["seq"] == 1 and jpg == native.jpeg_encode_cpu(want, q)
        st = jo.read_stream(jpg)  # an independent decoder: the stream holds the twin's crop
        assert (st.w, st.h) == (W, H)
        jo.check_exact("crop.jpg", st.coefs, want, q)
    for kw in (dict(quality=0), dict(quality=101), dict(width=0)):
        args = dict(width=8, height=8)
        args.update(kw)
        with pytest.raises(ValueError):
            wk.read_crop_jpeg(cam, nb(BOXES)[0], **args)


# ------------------------------------------------------------------------ Hub, REST, CLI

class _NoSession:
    def stop(self):
        pass


def test_hub_crops(native, tmp_path):
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, CameraNotFound, Hub

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    hub = Hub(cfg, devices=[-1, -1])
    try:
        frames = {}
        for k, (name, w, h) in enumerate([("a", 320, 240), ("b", 160, 96), ("c", 320, 176)]):
            wk = hub.workers[k % 2]
            cam = wk.add_camera(name, _slots(native, 3), 3)
            hub.cameras[name] = CameraHandle(name, k % 2, cam, "", session=_NoSession())
            enc = synth(native, w, h, gop=6, motion=0.2, seed=k + 1)
            for _ in range(2):
                assert wk.decode_now(cam, enc.next())
            frames[name] = [f for _, f in wk.read_history(cam, 0, 3)]
        assert hub.workers[0].last_query(hub.cameras["a"].cam) == 0
        seq, got = hub.crops("a", BOXES, 64, 48)
        assert seq == 2 and np.array_equal(got, co.crop_resize(frames["a"][1], BOXES, 64, 48))
        assert hub.workers[0].last_query(hub.cameras["a"].cam) > 0  # a query: the lazy decoder stays awake
        seq, got = hub.crops("a", BOXES, 64, 48, seq=1, fit="letterbox", pad=(1, 2, 3))
        assert seq == 1 and np.array_equal(got, co.crop_resize(frames["a"][0], BOXES, 64, 48, "letterbox", (1, 2, 3)))
        assert hub.crops("a", BOXES, 64, 48, after=2) is None and hub.crops("a", BOXES, 64, 48, seq=9) is None
        many = hub.crops_many({"c": BOXES[:2], "b": BOXES, "a": []}, 32, 24)
        assert list(many) == ["c", "b", "a"] and all(v[0] == 2 for v in many.values())
        assert np.array_equal(many["c"][1], co.crop_resize(frames["c"][1], BOXES[:2], 32, 24))
        assert np.array_equal(many["b"][1], co.crop_resize(frames["b"][1], BOXES, 32, 24))
        assert many["a"][1].shape == (0, 24, 32, 3)
        assert hub.crops_many({"a": BOXES}, 8, 8, after=2) == {"a": None}
        seq, jpg = hub.crop_jpeg("b", BOXES[1], 224, 224, quality=70)
        assert seq == 2 and jpg == native.jpeg_encode_cpu(co.crop_resize(frames["b"][1], BOXES[1:2], 224, 224)[0], 70)
        assert hub.crop_jpeg("b", BOXES[1], 8, 8, seq=1)[0] == 1
        assert hub.crop_counts() == (8, 4 + 4 + 4 + 4 + 6 + 4 + 1 + 1)
        with pytest.raises(CameraNotFound):
            hub.crops("nope", BOXES, 8, 8)
        with pytest.raises(CameraNotFound):
            hub.crops_many({"a": BOXES, "nope": BOXES}, 8, 8)
        for bad in BAD_BOXES:
            with pytest.raises(ValueError):
                hub.crops("a", [bad], 8, 8)
        for kw in (dict(width=0), dict(height=4097), dict(fit="zoom"), dict(pad=(1, 2)), dict(after=-1), dict(seq=1.5)):
            args = dict(width=8, height=8)
            args.update(kw)
            with pytest.raises(ValueError):
                hub.crops("a", BOXES, **args)
        with pytest.raises(ValueError):
            hub.crop_jpeg("a", BOXES[0], 8, 8, quality=0)
        # the limits
        cfg.serving.crop_max_boxes = 3
        with pytest.raises(ValueError):
            hub.crops("a", BOXES, 8, 8)
        assert hub.crops("a", BOXES[:3], 8, 8)[1].shape == (3, 8, 8, 3)
        cfg.serving.crop_max_boxes, cfg.serving.crop_max_bytes = 64, 3 * 8 * 8 * 3
        assert hub.crops("a", BOXES[:3], 8, 8) is not None
        with pytest.raises(ValueError):
            hub.crops("a", BOXES, 8, 8)
        with pytest.raises(ValueError):
            hub.crops_many({"a": BOXES[:2], "b": BOXES[:2]}, 8, 8)
        with pytest.raises(ValueError):
            hub.crop_jpeg("a", BOXES[0], 25, 8)
    finally:
        hub.shutdown()


def test_process_hub_refuses_crops():
    from video_edge_ai_proxy_amd.engine.isolated import ProcessHub

    for call in (lambda: ProcessHub.crops(object(), "a", BOXES, 8, 8),
                 lambda: ProcessHub.crops_many(object(), {"a": BOXES}, 8, 8),
                 lambda: ProcessHub.crop_jpeg(object(), "a", BOXES[0], 8, 8)):
        with pytest.raises(NotImplementedError, match="gpu.isolation: process"):
            call()


def test_config_crops(tmp_path):
    from video_edge_ai_proxy_amd.config import load_config

    cfg = load_config(data_dir=str(tmp_path))
    assert cfg.serving.crop_max_boxes == 64 and cfg.serving.crop_max_bytes == 64 << 20
    (tmp_path / "conf.yaml").write_text("serving:\n  crop_max_boxes: 20\n  crop_max_bytes: 1000000\n")
    cfg = load_config(data_dir=str(tmp_path))
    assert cfg.serving.crop_max_boxes == 20 and cfg.serving.crop_max_bytes == 1000000
    for bad in ("crop_max_boxes: 0", "crop_max_boxes: 65", "crop_max_bytes: 0", 'crop_max_bytes: "many"'):
        (tmp_path / "conf.yaml").write_text(f"serving:\n  {bad}\n")
        with pytest.raises(ValueError):
            load_config(data_dir=str(tmp_path))


@pytest.fixture
def farm(native):
    srv = native.RtspServer("127.0.0.1", 0)
    cfg = native.SynthConfig()
    cfg.width, cfg.height, cfg.gop, cfg.fps, cfg.seed, cfg.motion = 320, 240, 10, 30, 11, 0.2
    srv.add_stream("/cam", cfg, realtime=True, cached_frames=20)
    srv.start()
    yield srv
    srv.stop()


def _app(tmp_path, **over):
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.server.app import build_app

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    cfg.gpu.devices = [-1]
    for k, v in over.items():
        obj = cfg
        *path, leaf = k.split(".")
        for part in path:
            obj = getattr(obj, part)
        setattr(obj, leaf, v)
    return build_app(cfg, host="127.0.0.1", rest_port=0, grpc_port=0)


def _rest(app):
    from fastapi.testclient import TestClient

    from video_edge_ai_proxy_amd.server.rest import create_app

    return TestClient(create_app(app.pm, app.settings, app.metrics))


def _first_frame(hub, name, deadline_s=15):
    deadline = time.time() + deadline_s
    while time.time() < deadline:
        hub.touch(name)
        r = hub.latest_frame(name)
        if r is not None:
            return r
        time.sleep(0.02)
    raise AssertionError(f"no frame of {name} within {deadline_s} s")


def _metric(text, name):
    line = [ln for ln in text.splitlines() if ln.startswith(name + " ")]
    assert len(line) == 1, (name, line)
    return float(line[0].rsplit(" ", 1)[1])


def test_rest_crops(native, farm, tmp_path):
    app = _app(tmp_path, **{"buffer.in_memory": 64, "serving.crop_max_boxes": 6,
                            "serving.crop_max_bytes": 6 * 224 * 224 * 3})
    try:
        rest = _rest(app)
        url = f"rtsp://127.0.0.1:{farm.port}/cam"
        body = {"boxes": BOXES, "width": 64, "height": 48}
        assert rest.post("/api/v1/process/nope/crops", json=body).status_code == 404
        assert rest.get("/api/v1/process/nope/crop.jpg?box=0,0,5000,5000&width=8&height=8").status_code == 404
        assert rest.post("/api/v1/process", json={"name": "door", "rtsp_endpoint": url}).status_code == 200
        meta, _ = _first_frame(app.hub, "door")
        # seq = N pins the frame, so the bytes can be compared with the twin of that very frame
        seq = int(meta["seq"])
        hist = {int(m["seq"]): f for m, f in app.hub.history("door", 0, 0)}
        r = rest.post("/api/v1/process/door/crops", json=dict(body, seq=seq))
        assert r.status_code == 200 and r.headers["content-type"] == "application/octet-stream"
        assert r.headers["X-Vep-Seq"] == str(seq) and r.headers["X-Vep-Crops"] == f"{len(BOXES)},64,48"
        got = np.frombuffer(r.content, np.uint8).reshape(len(BOXES), 48, 64, 3)
        assert np.array_equal(got, co.crop_resize(hist[seq], BOXES, 64, 48))
        r = rest.post("/api/v1/process/door/crops", json=dict(body, seq=seq, fit="letterbox", pad=[9, 8, 7], width=50))
        assert r.status_code == 200 and r.headers["X-Vep-Crops"] == f"{len(BOXES)},50,48"
        assert r.content == co.crop_resize(hist[seq], BOXES, 50, 48, "letterbox", (9, 8, 7)).tobytes()
        newest = rest.post("/api/v1/process/door/crops", json=body)
        assert newest.status_code == 200 and int(newest.headers["X-Vep-Seq"]) >= seq
        # no such frame: 404
        assert rest.post("/api/v1/process/door/crops", json=dict(body, after=10 ** 9)).status_code == 404
        assert rest.post("/api/v1/process/door/crops", json=dict(body, seq=10 ** 9)).status_code == 404
        # a bad body: 422, and it changes nothing
        before = app.hub.crop_counts()
        for bad in ([], "nope", {"boxes": BOXES, "width": 64}, dict(body, width=0), dict(body, height=4097),
                    dict(body, fit="zoom"), dict(body, pad=[1, 2]), dict(body, after=-1), dict(body, seq="7"),
                    dict(body, boxes=[dict(GOOD, x1=10001)]), dict(body, boxes=GOOD), dict(body, zoom=2),
                    dict(body, boxes=[GOOD] * 7),                      # above serving.crop_max_boxes
                    dict(body, boxes=[GOOD] * 6, width=225, height=224)):  # above serving.crop_max_bytes
            assert rest.post("/api/v1/process/door/crops", json=bad).status_code == 422, bad
        assert rest.post("/api/v1/process/door/crops", content=b"{not json").status_code == 422
        assert rest.post("/api/v1/process/door/crops", json=dict(body, boxes=[GOOD] * 6, width=224, height=224)).status_code == 200
        assert app.hub.crop_counts() == (before[0] + 1, before[1] + 6)
        # crop.jpg: one box, a JPEG of the twin's crop of that frame
        q = f"/api/v1/process/door/crop.jpg?box=1000,500,6100,7300&width=224&height=224&quality=80&seq={seq}"
        r = rest.get(q)
        assert r.status_code == 200 and r.headers["content-type"] == "image/jpeg" and r.headers["X-Vep-Seq"] == str(seq)
        want = co.crop_resize(hist[seq], BOXES[1:2], 224, 224)[0]
        assert r.content == native.jpeg_encode_cpu(want, 80)
        st = jo.read_stream(r.content)
        assert (st.w, st.h) == (224, 224)
        jo.check_exact("crop.jpg", st.coefs, want, 80)
        assert rest.get(q + "&fit=letterbox").content == native.jpeg_encode_cpu(
            co.crop_resize(hist[seq], BOXES[1:2], 224, 224, "letterbox")[0], 80)
        assert rest.get(q.replace(f"seq={seq}", "seq=1000000000")).status_code == 404
        for bad in ("box=0,0,5000", "box=a,b,c,d", "box=0,0,0,5000", "box=0,0,5000,5000&fit=zoom",
                    "box=0,0,5000,5000&quality=0"):
            assert rest.get(f"/api/v1/process/door/crop.jpg?{bad}&width=8&height=8").status_code == 422, bad
        assert rest.get("/api/v1/process/door/crop.jpg?box=0,0,5000,5000&width=0&height=8").status_code == 422
        assert rest.get("/api/v1/process/door/crop.jpg?width=8&height=8").status_code == 422  # no box
        text = rest.get("/metrics").text
        requests, boxes = app.hub.crop_counts()
        assert _metric(text, "vep_crop_requests_total") == requests >= 8
        assert _metric(text, "vep_crop_boxes_total") == boxes >= 3 * len(BOXES) + 6 + 3
        # the CLI is a client of crop.jpg
        from video_edge_ai_proxy_amd import cli

        a = cli.build_parser().parse_args(["crop", "--device", "door", "--rest", "hub:9000", "--box", "1000,500,6100,7300",
                                           "--size", "224x224", "--seq", str(seq), "--quality", "80", "--out", "x.jpg"])
        assert a.fn is cli.cmd_crop and cli.crop_url(a) == "http://hub:9000" + q.replace(
            "&quality=80", "").replace(f"&seq={seq}", f"&fit=stretch&seq={seq}&quality=80")
        assert rest.get(cli.crop_url(a)[len("http://hub:9000"):]).content == r.content
        # with gpu.isolation: process the hub refuses, and REST answers 501

        def refuse(*a, **k):
            raise NotImplementedError("crops are not served with gpu.isolation: process")

        app.hub.crops = app.hub.crop_jpeg = refuse
        try:
            assert rest.post("/api/v1/process/door/crops", json=body).status_code == 501
            assert rest.get(q).status_code == 501
        finally:
            del app.hub.crops, app.hub.crop_jpeg
    finally:
        app.stop()


def test_cli_crop(native, tmp_path, monkeypatch):
    """`vep crop` fetches crop.jpg and writes it; malformed --box / --size end it before any request."""
    import io
    import urllib.request

    from video_edge_ai_proxy_amd import cli

    seen = {}

    class Reply(io.BytesIO):
        headers = {"X-Vep-Seq": "12"}

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

    def urlopen(url, timeout=None):
        seen["url"] = url
        return Reply(b"\xff\xd8jpeg\xff\xd9")

    monkeypatch.setattr(urllib.request, "urlopen", urlopen)
    out = tmp_path / "zoom.jpg"
    cli.main(["crop", "--device", "front door", "--box", "0,0,5000,5000", "--size", "320x240", "--fit", "letterbox",
              "--out", str(out)])
    assert out.read_bytes() == b"\xff\xd8jpeg\xff\xd9"
    assert seen["url"] == ("http://127.0.0.1:8080/api/v1/process/front%20door/crop.jpg?"
                           "box=0,0,5000,5000&width=320&height=240&fit=letterbox")
    for bad in (["--box", "0,0,5000", "--size", "8x8"], ["--box", "0,0,1,1", "--size", "8"],
                ["--box", "a,0,1,1", "--size", "8x8"]):
        with pytest.raises(SystemExit):
            cli.main(["crop", "--device", "d", "--out", str(out)] + bad)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["crop", "--device", "d", "--box", "0,0,1,1", "--size", "8x8"])  # --out is required
