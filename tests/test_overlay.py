"""On-screen display (docs/OVERLAY.md) without a GPU: the arithmetic of csrc/vep/overlay.h against
the numpy oracle (tests/overlay_oracle.py), the CPU twin, and everything above the kernel through
the CPU-backend Worker, the Hub, REST and the CLI."""
import json
import time

import numpy as np
import pytest

import jpeg_oracle as jo
import mask_oracle as mo
import overlay_oracle as oo
from conftest import synth
from video_edge_ai_proxy_amd import overlay, privacy

META = {"seq": 4711, "timestamp": 90 * 1790000000123}  # 2026-09-21 14:13:20.123


def nat(items):
    return overlay.to_native(items)


@pytest.fixture(scope="module")
def font(native):
    return native.overlay_font()


def twin(native, img, items, name="", meta=None, pitch=None):
    """The CPU twin out of place; with `pitch` into a wider destination whose padding must survive."""
    H, W = img.shape[:2]
    if pitch is None:
        dst = np.zeros_like(img)
        native.overlay_draw_cpu(img, dst, nat(items), name, meta)
        return dst
    buf = np.full((H, pitch), 0xA5, np.uint8)
    dst = np.lib.stride_tricks.as_strided(buf, (H, W, 3), (pitch, 3, 1))
    native.overlay_draw_cpu(img, dst, nat(items), name, meta)
    assert (buf[:, W * 3:] == 0xA5).all()
    return np.ascontiguousarray(dst)


# ------------------------------------------------------------------------ blend, font

def test_blend_equals_the_formula_everywhere(native):
    d, c = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for a in range(256):  # all 256^3 triples, a plane at a time
        got = native.overlay_blend(d, c, np.full_like(d, a))
        want = (d.astype(np.int64) * (255 - a) + c.astype(np.int64) * a + 127) // 255
        assert np.array_equal(got, want), a
        if a == 0:
            assert np.array_equal(got, d)
        if a == 255:
            assert np.array_equal(got, c)
    assert np.array_equal(oo.blend(d, c, 77), native.overlay_blend(d, c, np.full_like(d, 77)))


def test_font_properties(font):
    assert font.shape == (95, 8) and font.dtype == np.uint8
    assert not font[0].any()                                  # space
    assert all(font[g].any() for g in range(1, 95))
    assert len({bytes(font[g]) for g in range(95)}) == 95     # all distinct
    assert not (font & 0xE0).any()                            # column 5 (and above) empty
    assert np.count_nonzero(font[ord("-") - 32]) == 1          # one row
    assert not font[ord(".") - 32][:4].any()                   # lower half
    bar = font[ord("|") - 32]
    assert len(set(bar[bar != 0])) == 1 and bin(int(bar.max())).count("1") == 1  # one column


# ------------------------------------------------------------------------ expansion

def same_expansion(native, items, W, H, name="", meta=None):
    got = native.overlay_expand(W, H, nat(items), name, meta)
    want = oo.expand(items, W, H, name, meta)
    assert got == want, (W, H, got, want)
    return got


def test_expand_outlines(native):
    # the rect is 10 x 10 pixels of a 100 x 100 picture: 2t below, at and above the short side
    box = {"x0": 2000, "y0": 3000, "x1": 3000, "y1": 4000}
    assert len(same_expansion(native, [dict(box, thickness=4)], 100, 100)) == 4
    assert len(same_expansion(native, [dict(box, thickness=5)], 100, 100)) == 1
    assert len(same_expansion(native, [dict(box, thickness=6)], 100, 100)) == 1
    assert len(same_expansion(native, [dict(box, thickness=1, fill=True)], 100, 100)) == 1
    # the four fills are disjoint and cover exactly the outline
    ps = same_expansion(native, [dict(box, thickness=3)], 100, 100)
    cov = sum(oo.coverage(p, 100, 100, None).astype(int) for p in ps)
    want = np.zeros((100, 100), int)
    want[30:40, 20:30] = 1
    want[33:37, 23:27] = 0
    assert np.array_equal(cov, want)
    # a one-pixel rect, and a rect rounded outward
    assert same_expansion(native, [{"x0": 5000, "y0": 5000, "x1": 5001, "y1": 5001}], 64, 16) == [
        (0, 32, 8, 33, 9, (0, 255, 0), 255)]
    assert same_expansion(native, [{"x0": 1, "y0": 1, "x1": 9999, "y1": 9999, "fill": True}], 7, 5) == [
        (0, 0, 0, 7, 5, (0, 255, 0), 255)]


def test_expand_labels(native):
    # room above, no room above, running off the right edge
    above = same_expansion(native, [{"x0": 1000, "y0": 5000, "x1": 5000, "y1": 9000, "label": "ab"}], 200, 120)
    assert above[4] == (0, 20, 51, 33, 60, (0, 255, 0), 255) and above[5] == (1, 21, 52, 1, (0, 0, 0), 255, b"ab")
    inside = same_expansion(native, [{"x0": 1000, "y0": 500, "x1": 5000, "y1": 9000, "label": "ab"}], 200, 120)
    assert inside[4][1:5] == (20, 6, 33, 15)
    off = same_expansion(native, [{"x0": 9000, "y0": 5000, "x1": 10000, "y1": 9000, "label": "long label",
                                   "color": [0, 0, 128]}], 200, 120)
    assert off[4][1:5] == (180, 51, 200, 60) and off[5][4] == (255, 255, 255)  # clipped strip, white ink
    # the ink threshold: 2r + 5g + b < 1024 is white
    for col, ink in (([4, 204, 0], 0), ([3, 204, 0], 255), ([255, 0, 255], 255), ([255, 255, 255], 0)):
        p = same_expansion(native, [{"x0": 0, "y0": 5000, "x1": 5000, "y1": 9000, "label": "x", "color": col}], 64, 64)
        assert p[-1][4] == (ink, ink, ink), col
    # at 1080 rows the label is drawn at k = 4
    p = same_expansion(native, [{"x0": 1000, "y0": 5000, "x1": 5000, "y1": 9000, "label": "abc"}], 1920, 1080)
    assert p[4][1:5] == (192, 540 - 36, 192 + 6 * 4 * 3 + 4, 540) and p[5][1:4] == (196, 540 - 32, 4)


def test_expand_text(native):
    for x, y in ((0, 0), (10000, 0), (0, 10000), (10000, 10000), (9999, 9999), (5000, 5000)):
        for bg in (None, [1, 2, 3]):
            it = {"type": "text", "x": x, "y": y, "text": "Hi", "scale": 2, "alpha": 200}
            if bg:
                it.update(bg=bg, bg_alpha=77)
            ps = same_expansion(native, [it], 65, 17)
            assert len(ps) == (2 if bg else 1)
    ps = same_expansion(native, [{"type": "text", "x": 0, "y": 0, "text": "Hi", "scale": 2, "bg": [1, 2, 3]}], 65, 17)
    assert ps[0] == (0, 0, 0, 24, 16, (1, 2, 3), 255) and ps[1] == (1, 0, 0, 2, (255, 255, 255), 255, b"Hi")
    assert same_expansion(native, [{"type": "text", "x": 0, "y": 0, "text": "", "bg": [1, 2, 3]}], 65, 17) == []


@pytest.mark.parametrize("H,k", [(1, 1), (269, 1), (270, 1), (539, 1), (540, 2), (1080, 4), (2160, 8), (4320, 8)])
def test_auto_scale(native, H, k):
    assert oo.auto_k(H) == k
    ps = same_expansion(native, [{"type": "text", "x": 0, "y": 0, "text": "k"},
                                 {"x0": 0, "y0": 0, "x1": 10000, "y1": 10000}], 400, H)
    assert ps[0][3] == k
    if H > 2 * k:
        assert ps[1][1:5] == (0, 0, 400, k)  # the auto thickness is the same k


def test_expand_placeholders_and_cut(native):
    it = {"type": "text", "x": 0, "y": 0, "text": "{name} #{seq} {time} {nope}", "scale": 1}
    ps = same_expansion(native, [it], 640, 360, "front door", META)
    assert ps[0][6] == b"front door #4711 2026-09-21 14:13:20.123 {nope}"
    assert native.overlay_time(META["timestamp"]) == oo.time_text(META["timestamp"]) == "2026-09-21 14:13:20.123"
    for ts in (0, 89, 90, 90 * 86400000 - 1, 90 * 951782400000, 90 * 4102444799999):  # 2000-02-29, 2099-12-31
        assert native.overlay_time(ts) == oo.time_text(ts), ts
    assert native.overlay_time(-5) == "1970-01-01 00:00:00.000"
    # a 65-byte text is cut at 64; the cut comes after the replacement; a byte 0x80 becomes '?'
    ps = same_expansion(native, [dict(it, text="x" * 65)], 640, 360)
    assert ps[0][6] == b"x" * 64
    ps = same_expansion(native, [dict(it, text="y" * 60 + "{seq}")], 640, 360, "", META)
    assert ps[0][6] == b"y" * 60 + b"4711"
    ps = same_expansion(native, [dict(it, text="a\x80b\x1f\x7f~")], 640, 360)
    assert ps[0][6] == b"a?b??~"
    ps = same_expansion(native, [{"x0": 0, "y0": 5000, "x1": 5000, "y1": 9000, "label": "café {name}"}], 640, 360, "c\n")
    assert ps[-1][6] == b"caf? c?"


def test_expand_limits(native):
    sixty_four = [{"x0": 100 * i, "y0": 0, "x1": 100 * i + 50, "y1": 10000, "fill": True} for i in range(64)]
    assert len(same_expansion(native, sixty_four, 640, 360)) == 64
    with pytest.raises(ValueError):
        nat(sixty_four + sixty_four[:1])
    with pytest.raises(ValueError):
        native.overlay_check(nat(sixty_four) + nat(sixty_four[:1]))
    dense = oo.dense()
    assert len(same_expansion(native, dense, 1920, 1080, "cam", META)) == 256
    assert len(same_expansion(native, dense, 200, 120, "cam", META)) == 256
    more = dense + [{"x0": 0, "y0": 0, "x1": 1, "y1": 1}]
    with pytest.raises(ValueError):
        oo.expand(more, 200, 120)
    with pytest.raises(ValueError, match="256"):
        native.overlay_expand(200, 120, nat(more), "", None)
    with pytest.raises(ValueError, match="256"):
        native.overlay_draw_cpu(oo.picture(200, 120), np.zeros((120, 200, 3), np.uint8), nat(more), "", None)
    for W, H in ((0, 5), (5, 0), (65536, 5)):
        with pytest.raises(ValueError):
            native.overlay_expand(W, H, [], "", None)


BOX = {"type": "box", "x0": 1000, "y0": 1000, "x1": 5000, "y1": 5000}
TXT = {"type": "text", "x": 100, "y": 100, "text": "t"}
BAD_ITEMS = [dict(BOX, x0=-1), dict(BOX, x0=5000), dict(BOX, x1=10001), dict(BOX, y0=5000), dict(BOX, y1=10001),
             dict(BOX, y0=-1), dict(BOX, color=[0, 0, 256]), dict(BOX, color=[0, 0]), dict(BOX, color="green"),
             dict(BOX, alpha=256), dict(BOX, alpha=-1), dict(BOX, thickness=33), dict(BOX, thickness=-1),
             dict(BOX, fill=2), dict(BOX, label=5), dict(BOX, label="x" * 257), dict(BOX, x0=1.5), dict(BOX, x0=True),
             dict(BOX, scale=2), dict(BOX, zoom=1), {k: v for k, v in BOX.items() if k != "y1"}, dict(BOX, type="line"),
             dict(TXT, x=-1), dict(TXT, x=10001), dict(TXT, y=10001), dict(TXT, scale=9), dict(TXT, scale=-1),
             dict(TXT, color=[-1, 0, 0]), dict(TXT, alpha=300), dict(TXT, bg=[0, 0, 300]), dict(TXT, bg=[0]),
             dict(TXT, bg_alpha=256), dict(TXT, text=None), dict(TXT, text="x" * 257), dict(TXT, thickness=1),
             {k: v for k, v in TXT.items() if k != "text"}, "box", None, 7]


def test_every_invalid_field_is_refused(native):
    for bad in BAD_ITEMS:
        with pytest.raises(ValueError):
            overlay.normalize(bad)
    for bad in (None, "items", {"x0": 1}, 5):
        with pytest.raises(ValueError):
            overlay.normalize_list(bad)
    # the native layer checks the tuples itself: position -> out-of-range value
    good_box, good_text = nat([BOX])[0], nat([dict(TXT, bg=[1, 2, 3])])[0]
    native.overlay_check([good_box, good_text])
    bad_box = {0: 2, 1: -1, 2: -1, 3: 10001, 4: 10001, 5: 256, 6: -1, 7: 256, 8: 256, 9: 33, 10: 2, 17: b"x" * 257}
    bad_text = {0: -1, 1: 10001, 2: -1, 5: 256, 8: -1, 11: 9, 12: 2, 13: 256, 14: -1, 15: 256, 16: 256, 17: b"x" * 257}
    for good, bads in ((good_box, bad_box), (good_text, bad_text)):
        for pos, v in bads.items():
            t = list(good)
            t[pos] = v
            with pytest.raises(ValueError):
                native.overlay_check([tuple(t)])
            with pytest.raises(ValueError):
                native.overlay_expand(64, 64, [tuple(t)], "", None)
    for t in ((good_box[:1] + (5000,) + good_box[2:]), (good_box[:2] + (5000,) + good_box[3:])):  # x0 = x1, y0 = y1
        with pytest.raises(ValueError):
            native.overlay_check([t])


# ------------------------------------------------------------------------ twin == oracle

LISTS = oo.lists()


@pytest.mark.parametrize("size", oo.SMALL, ids=lambda s: "%dx%d" % s)
def test_twin_equals_oracle(native, font, size):
    W, H = size
    img = oo.picture(W, H)
    results = {}
    for name, items in LISTS.items():
        want = oo.apply(img, items, font, "cam-7", META)
        assert np.array_equal(twin(native, img, items, "cam-7", META), want), name
        for extra in (1, 13):
            assert np.array_equal(twin(native, img, items, "cam-7", META, pitch=3 * W + extra), want), (name, extra)
        inplace = img.copy()
        native.overlay_draw_cpu(inplace, inplace, nat(items), "cam-7", META)
        assert np.array_equal(inplace, want), name
        results[name] = want
    assert np.array_equal(results["empty"], img)
    if W * H > 1:
        assert not np.array_equal(results["three"], results["three_reversed"])  # the order shows


def test_twin_equals_oracle_1080p(native, font):
    img = oo.picture(1920, 1080)
    items = LISTS["outlines"] + LISTS["text_k8"] + LISTS["text_edges"] + LISTS["three"] + LISTS["text_k1"] + [overlay.STAMP]
    want = oo.apply(img, items, font, "gate", META)
    assert np.array_equal(twin(native, img, items, "gate", META), want)
    assert np.array_equal(twin(native, img, oo.dense(), "gate", META), oo.apply(img, oo.dense(), font, "gate", META))


def test_text_runs_cross_tiles(native, font):
    """The runs of text_k1 and text_k8 really span several 64 x 16 tiles of the 200 x 120 picture."""
    for name in ("text_k1", "text_k8"):
        p = oo.expand(LISTS[name], 200, 120)[-1]
        ys, xs = np.nonzero(oo.coverage(p, 200, 120, font))
        assert len({(x // 64, y // 16) for x, y in zip(xs, ys)}) >= 3, name


def test_closed_forms(native):
    img = oo.picture(200, 120)
    got = twin(native, img, [{"x0": 1000, "y0": 2500, "x1": 6000, "y1": 7500, "color": [9, 8, 7], "fill": True}])
    want = img.copy()
    want[30:90, 20:120] = (9, 8, 7)
    assert np.array_equal(got, want)
    for it in LISTS["outlines"] + LISTS["text_k8"]:
        zero = dict(it, alpha=0)
        if "bg" in zero:
            zero["bg_alpha"] = 0
        if "label" in zero:
            del zero["label"]  # (a label's ink is opaque whatever the box's alpha)
        assert np.array_equal(twin(native, img, [zero]), img)
    flat = np.full((120, 200, 3), 90, np.uint8)
    got = twin(native, flat, [{"x0": 1000, "y0": 1000, "x1": 9000, "y1": 9000, "color": [200, 200, 200], "alpha": 100,
                               "thickness": 5}])
    inside = got[12:108, 20:180].reshape(-1, 3)
    assert len({tuple(p) for p in inside}) == 2  # every outline pixel blended once, the rest untouched
    assert np.array_equal(np.delete(got.reshape(-1), np.s_[0:0]), got.reshape(-1)) and (got[:12] == 90).all()


def test_draw_cpu_argument_checks(native):
    img = oo.picture(17, 9)
    with pytest.raises(ValueError):
        native.overlay_draw_cpu(img, np.zeros((9, 16, 3), np.uint8), [], "", None)
    with pytest.raises(ValueError):
        native.overlay_draw_cpu(img[:, :, :2], img[:, :, :2], [], "", None)
    with pytest.raises(ValueError):
        native.overlay_draw_cpu(img[:, ::2], np.zeros((9, 9, 3), np.uint8), [], "", None)
    with pytest.raises((ValueError, TypeError)):
        native.overlay_draw_cpu(img.astype(np.float32), img, [], "", None)


# ------------------------------------------------------------------------ Worker (CPU backend)

ITEMS = [{"x0": 1000, "y0": 2000, "x1": 6000, "y1": 9000, "label": "person 87%", "alpha": 160},
         {"x0": 5000, "y0": 500, "x1": 9900, "y1": 6000, "color": [0, 0, 255], "thickness": 2, "label": "{name} {seq}"},
         {"type": "text", "x": 200, "y": 9000, "text": "{time}", "scale": 2, "bg": [0, 0, 0], "bg_alpha": 128}]
MASKS = [{"x0": 1000, "y0": 500, "x1": 6100, "y1": 7300, "mode": "pixelate", "block": 16}]


def _camera(native, w=320, h=240, masks=None, history=0, **kw):
    wk = native.Worker(device=-1)
    slots = wk.history_ring_slots(history) if history else 2
    cam = wk.add_camera("c", slots, history)
    if masks:
        wk.set_privacy_masks(cam, privacy.to_native(masks))
    enc = synth(native, w, h, gop=6, motion=0.2, **kw)
    return wk, cam, lambda: wk.decode_now(cam, enc.next())


def _plain(d):
    """A detector's answer with its arrays as lists, so two answers compare with ==."""
    return {k: np.asarray(v).tolist() if isinstance(v, np.ndarray) else v for k, v in d.items()}


def test_worker_overlay_jpeg(native, font):
    wk, cam, step = _camera(native)
    assert wk.read_overlay_jpeg(cam, nat(ITEMS), "c") is None  # no frame yet
    assert step()
    meta, frame = wk.read_latest(cam, 0)
    motion, tamper = wk.read_motion(cam, 0), wk.read_tamper(cam, 0)
    plain = wk.read_latest_jpeg(cam, 0, 80)[1]
    m, jpg = wk.read_overlay_jpeg(cam, nat(ITEMS), "yard", quality=80)
    want = twin(native, frame, ITEMS, "yard", meta)
    assert np.array_equal(want, oo.apply(frame, ITEMS, font, "yard", meta)) and not np.array_equal(want, frame)
    assert m["seq"] == meta["seq"] and (m["width"], m["height"]) == (320, 240)
    assert jpg == native.jpeg_encode_cpu(want, 80)
    st = jo.read_stream(jpg)  # an independent decoder: the stream holds the twin's picture
    assert (st.w, st.h) == (320, 240)
    jo.check_exact("overlay.jpg", st.coefs, want, 80)
    # scaled: the items are drawn on the scaled picture, at its own auto scale
    m, jpg = wk.read_overlay_jpeg(cam, nat(ITEMS), "yard", quality=80, width=161)
    small = native.resize_area_cpu(frame, m["width"], m["height"])
    assert m["width"] == 161 and jpg == native.jpeg_encode_cpu(twin(native, small, ITEMS, "yard", meta), 80)
    # an empty list is the plain picture
    assert wk.read_overlay_jpeg(cam, [], "yard", quality=80)[1] == plain
    # the ring slot is never written: the frame, the plain JPEG and the detectors' answers stay
    again = wk.read_latest(cam, 0)
    assert again[0] == meta and np.array_equal(again[1], frame)
    assert wk.read_latest_jpeg(cam, 0, 80)[1] == plain
    assert _plain(wk.read_motion(cam, 0)) == _plain(motion) and _plain(wk.read_tamper(cam, 0)) == _plain(tamper)
    assert wk.overlay_counts() == (3, 2 * len(oo.expand(ITEMS, 320, 240, "yard", meta)))
    # after: only a newer frame answers; refusals
    assert wk.read_overlay_jpeg(cam, nat(ITEMS), "yard", after=1) is None
    with pytest.raises(IndexError):
        wk.read_overlay_jpeg(99, nat(ITEMS), "yard")
    for kw in (dict(quality=0), dict(quality=101), dict(width=-1), dict(height=65536)):
        with pytest.raises(ValueError):
            wk.read_overlay_jpeg(cam, nat(ITEMS), "yard", **kw)
    with pytest.raises(ValueError, match="256"):
        wk.read_overlay_jpeg(cam, nat(oo.dense() + [BOX]), "yard")
    bad = list(nat([BOX])[0])
    bad[8] = 256
    with pytest.raises(ValueError):
        wk.read_overlay_jpeg(cam, [tuple(bad)], "yard")


def test_worker_stamp_is_of_the_picked_frame(native):
    wk, cam, step = _camera(native, history=4)
    assert step() and step()
    hist = {int(m["seq"]): (m, f) for m, f in wk.read_history(cam, 0, 4)}
    assert hist[1][0]["timestamp"] != hist[2][0]["timestamp"]
    stamp = [overlay.STAMP, {"type": "text", "x": 100, "y": 5000, "text": "#{seq}"}]
    m, jpg = wk.read_overlay_jpeg(cam, nat(stamp), "gate", quality=90)
    assert m["seq"] == 2
    assert jpg == native.jpeg_encode_cpu(twin(native, hist[2][1], stamp, "gate", hist[2][0]), 90)
    assert jpg != native.jpeg_encode_cpu(twin(native, hist[2][1], stamp, "gate", hist[1][0]), 90)
    assert step()  # a later frame: the next request carries ITS seq and time
    m3, f3 = wk.read_latest(cam, 0)
    assert wk.read_overlay_jpeg(cam, nat(stamp), "gate", quality=90)[1] == native.jpeg_encode_cpu(
        twin(native, f3, stamp, "gate", m3), 90)


def test_worker_overlay_is_drawn_over_the_masked_frame(native):
    wk, cam, step = _camera(native, masks=MASKS)
    plain, pcam, pstep = _camera(native)
    assert step() and pstep()
    raw = plain.read_latest(pcam, 0)[1]
    masked = mo.apply(raw, MASKS)
    meta, frame = wk.read_latest(cam, 0)
    assert np.array_equal(frame, masked) and not np.array_equal(masked, raw)
    jpg = wk.read_overlay_jpeg(cam, nat(ITEMS), "m", quality=85)[1]
    assert jpg == native.jpeg_encode_cpu(twin(native, masked, ITEMS, "m", meta), 85)
    assert jpg != native.jpeg_encode_cpu(twin(native, raw, ITEMS, "m", meta), 85)


def wall_twin(native, frames, names, cols, tw, th, shown=None):
    """The labelled wall's canvas: the unlabelled one with tile t's label drawn as a text item at
    the origin of its own cell, on the cell alone."""
    canvas = native.compose_wall_cpu(frames, cols, tw, th).copy()
    gc = canvas.shape[1] // tw
    for t, n in enumerate(names):
        if not n or (shown is not None and not shown[t]):
            continue
        y, x = (t // gc) * th, (t % gc) * tw
        cell = np.ascontiguousarray(canvas[y:y + th, x:x + tw])
        canvas[y:y + th, x:x + tw] = twin(native, cell, [{"type": "text", "x": 0, "y": 0, "text": n, "bg": [0, 0, 0],
                                                          "bg_alpha": 160}])
    return canvas


def test_worker_wall_labels(native):
    wk = native.Worker(device=-1)
    cams, frames = [], []
    for k, (w, h) in enumerate([(320, 240), (160, 96), (320, 176)]):
        cam = wk.add_camera("c%d" % k, 2)
        assert wk.decode_now(cam, synth(native, w, h, gop=6, motion=0.2, seed=k + 1).next())
        cams.append(cam)
        frames.append(wk.read_latest(cam, 0)[1])
    names = ["north gate", "a-very-long-camera-name-that-is-clipped-to-its-tile", "yard"]
    for tw, th, cols in ((160, 120, 2), (97, 55, 0), (640, 540, 3)):
        plain = wk.read_wall_jpeg(cams, cols, tw, th, 85)
        seqs, jpg = wk.read_wall_jpeg(cams, cols, tw, th, 85, None, names)
        assert seqs == plain[0] == [1, 1, 1]
        assert plain[1] == native.jpeg_encode_cpu(native.compose_wall_cpu(frames, cols, tw, th), 85)
        assert jpg == native.jpeg_encode_cpu(wall_twin(native, frames, names, cols, tw, th), 85) and jpg != plain[1]
    # a tile without a frame, and one without a name, get no label
    empty = wk.add_camera("late", 2)
    seqs, jpg = wk.read_wall_jpeg(cams + [empty, -1], 3, 160, 120, 85, None, names[:2] + ["", "late", "gone"])
    assert seqs == [1, 1, 1, 0, 0]
    assert jpg == native.jpeg_encode_cpu(wall_twin(native, frames + [None, None], names[:2] + ["", "", ""], 3, 160, 120), 85)
    assert wk.read_wall_jpeg(cams, 2, 160, 120, 85, None, ["", "", ""])[1] == wk.read_wall_jpeg(cams, 2, 160, 120, 85)[1]
    with pytest.raises(ValueError):
        wk.read_wall_jpeg(cams, 2, 160, 120, 85, None, names[:2])
    wk.wall_max_tiles = 200
    with pytest.raises(ValueError, match="256"):
        wk.read_wall_jpeg([cams[0]] * 129, 0, 16, 16, 85, None, ["n"] * 129)
    assert wk.read_wall_jpeg([cams[0]] * 128, 0, 16, 16, 85, None, ["n"] * 128)[0] == [1] * 128


# ------------------------------------------------------------------------ Hub, REST, CLI

class _NoSession:
    def stop(self):
        pass


def test_hub_overlay(native, tmp_path):
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, CameraNotFound, Hub

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    hub = Hub(cfg, devices=[-1, -1])
    try:
        frames, metas = {}, {}
        for k, (name, w, h) in enumerate([("a", 320, 240), ("b", 160, 96), ("c", 320, 176)]):
            wk = hub.workers[k % 2]
            cam = wk.add_camera(name, 2)
            hub.cameras[name] = CameraHandle(name, k % 2, cam, "", session=_NoSession())
            assert wk.decode_now(cam, synth(native, w, h, gop=6, motion=0.2, seed=k + 1).next())
            metas[name], frames[name] = wk.read_latest(cam, 0)
        plain = hub.latest_jpeg("a", quality=80)
        assert plain[1] == native.jpeg_encode_cpu(frames["a"], 80)
        # an explicit list, the stamp, both, scaled
        m, jpg = hub.latest_jpeg("a", quality=80, overlay=ITEMS)
        assert jpg == native.jpeg_encode_cpu(twin(native, frames["a"], ITEMS, "a", metas["a"]), 80)
        m, jpg = hub.latest_jpeg("a", quality=80, stamp=True)
        assert jpg == native.jpeg_encode_cpu(twin(native, frames["a"], [overlay.STAMP], "a", metas["a"]), 80)
        m, jpg = hub.latest_jpeg("a", quality=80, overlay=ITEMS, stamp=True, width=160)
        small = native.resize_area_cpu(frames["a"], 160, 120)
        assert (m["width"], m["height"]) == (160, 120)
        assert jpg == native.jpeg_encode_cpu(twin(native, small, ITEMS + [overlay.STAMP], "a", metas["a"]), 80)
        # the stored list: nothing stored draws nothing
        assert hub.overlay("a") == [] and hub.latest_jpeg("a", quality=80, overlay=True)[1] == plain[1]
        hub.set_overlay("a", ITEMS)
        stored = hub.overlay("a")
        assert [overlay.normalize(i) for i in stored] == [overlay.normalize(i) for i in ITEMS]
        assert hub.latest_jpeg("a", quality=80, overlay=True)[1] == native.jpeg_encode_cpu(
            twin(native, frames["a"], ITEMS, "a", metas["a"]), 80)
        assert hub.latest_jpeg("a", quality=80)[1] == plain[1] and hub.overlay("b") == []
        # read_latest returns the same bytes before and after
        again = hub.workers[0].read_latest(hub.cameras["a"].cam, 0)
        assert again[0] == metas["a"] and np.array_equal(again[1], frames["a"])
        # a bad list changes nothing
        for bad in BAD_ITEMS[:6] + [dict(BOX, label="x" * 257)]:
            with pytest.raises(ValueError):
                hub.set_overlay("a", [bad])
        with pytest.raises(ValueError):
            hub.set_overlay("a", [BOX] * 65)
        for ttl in (-1, 1.5, True, "1"):
            with pytest.raises(ValueError):
                hub.set_overlay("a", [BOX], ttl_ms=ttl)
        assert hub.overlay("a") == stored
        # ttl_ms on an injected monotonic clock
        now = [100.0]
        hub.overlay_clock = lambda: now[0]
        hub.set_overlay("b", [BOX], ttl_ms=1500)
        hub.add_overlay_item("b", TXT)
        assert len(hub.overlay("b")) == 2
        now[0] = 101.4
        assert len(hub.overlay("b")) == 2
        now[0] = 101.5
        assert [i["type"] for i in hub.overlay("b")] == ["text"]  # the box expired, the text has no ttl
        assert hub.latest_jpeg("b", quality=80, overlay=True)[1] == native.jpeg_encode_cpu(
            twin(native, frames["b"], [TXT], "b", metas["b"]), 80)
        for i in range(70):  # a full list makes room by dropping its oldest item
            hub.add_overlay_item("b", dict(TXT, text=str(i)), ttl_ms=1000)
        assert [i["text"] for i in hub.overlay("b")] == [str(i) for i in range(6, 70)]
        now[0] = 103.0
        assert hub.overlay("b") == []
        hub.clear_overlay("a")
        assert hub.overlay("a") == []
        # a list that cannot be drawn is refused when it is asked for
        hub.set_overlay("c", oo.dense() + [BOX])
        with pytest.raises(ValueError, match="256"):
            hub.latest_jpeg("c", overlay=True)
        with pytest.raises(ValueError):
            hub.latest_jpeg("c", overlay=[BOX] * 64, stamp=True)  # 65 items
        with pytest.raises(ValueError):
            hub.latest_jpeg("c", stamp=1)
        for call in (lambda: hub.set_overlay("nope", []), lambda: hub.overlay("nope"), lambda: hub.clear_overlay("nope"),
                     lambda: hub.latest_jpeg("nope", stamp=True)):
            with pytest.raises(CameraNotFound):
                call()
        # the wall: labels are the cameras' names, across workers (b lives on the other one)
        order = ["a", "b", "c"]
        seqs, jpg = hub.wall_jpeg(order, cols=2, tile_width=160, tile_height=120, quality=85, labels=True)
        tiles = [frames["a"], native.resize_area_cpu(frames["b"], 160, 96), frames["c"]]
        assert seqs == {"a": 1, "b": 1, "c": 1}
        assert jpg == native.jpeg_encode_cpu(wall_twin(native, tiles, order, 2, 160, 120), 85)
        assert hub.wall_jpeg(order, cols=2, tile_width=160, tile_height=120, quality=85)[1] == native.jpeg_encode_cpu(
            native.compose_wall_cpu(tiles, 2, 160, 120), 85)
        cfg.serving.wall_max_tiles = 200
        for w in hub.workers:
            w.wall_max_tiles = 200
        with pytest.raises(overlay.Refused):
            hub.wall_jpeg(["a"] * 129, tile_width=16, tile_height=16, labels=True)
        assert len(hub.wall_jpeg(["a"] * 129, tile_width=16, tile_height=16)[1]) > 100
        requests, prims = hub.overlay_counts()
        assert requests == 7 and prims >= 3 * 13
        # a removed camera takes its list with it
        hub.set_overlay("a", ITEMS)
        hub.stop_camera("a")
        assert "a" not in hub._overlays
    finally:
        hub.shutdown()


def test_process_hub_refuses_overlays():
    from video_edge_ai_proxy_amd.engine.isolated import ProcessHub

    for call in (lambda: ProcessHub.set_overlay(object(), "a", []), lambda: ProcessHub.overlay(object(), "a"),
                 lambda: ProcessHub.clear_overlay(object(), "a"), lambda: ProcessHub.add_overlay_item(object(), "a", BOX),
                 lambda: ProcessHub.latest_jpeg(object(), "a", overlay=True),
                 lambda: ProcessHub.latest_jpeg(object(), "a", stamp=True),
                 lambda: ProcessHub.wall_jpeg(object(), ["a"], labels=True)):
        with pytest.raises(NotImplementedError, match="gpu.isolation: process"):
            call()


def test_config_overlay(tmp_path):
    from video_edge_ai_proxy_amd.config import load_config

    cfg = load_config(data_dir=str(tmp_path))
    assert cfg.overlay.from_annotations is False and cfg.overlay.annotation_ttl_ms == 1000
    (tmp_path / "conf.yaml").write_text("overlay:\n  from_annotations: true\n  annotation_ttl_ms: 250\n")
    cfg = load_config(data_dir=str(tmp_path))
    assert cfg.overlay.from_annotations is True and cfg.overlay.annotation_ttl_ms == 250
    (tmp_path / "conf.yaml").write_text("overlay:\n  annotation_ttl_ms: 0\n")
    with pytest.raises(ValueError):
        load_config(data_dir=str(tmp_path))


def test_pixel_box_is_converted_outward():
    for W, H, box in ((1920, 1080, (10, 10, 110, 210)), (333, 77, (1, 2, 332, 76)), (640, 360, (0, 0, 640, 360)),
                      (7, 5, (6, 4, 7, 5))):
        x0, y0, x1, y1 = overlay.from_pixel_box(*box, W, H)
        px0, px1 = oo.axis_pixels(W, x0, x1)
        py0, py1 = oo.axis_pixels(H, y0, y1)
        assert px0 <= box[0] and py0 <= box[1] and px1 >= box[2] and py1 >= box[3]  # never loses a pixel
        assert box[0] - px0 <= 1 and box[1] - py0 <= 1 and px1 - box[2] <= 1 and py1 - box[3] <= 1
    assert overlay.from_pixel_box(-5, -5, 5000, 5000, 640, 360) == (0, 0, 10000, 10000)


class _Ctx:
    def abort(self, code, msg):
        raise AssertionError(msg)


class _Queue:
    def __init__(self):
        self.sent = []

    def publish(self, b):
        self.sent.append(b)
        return True


class _Settings:
    class _S:
        edge_key = "k"

    def get(self):
        return self._S()


def test_annotations_become_boxes(native, tmp_path):
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub
    from video_edge_ai_proxy_amd.proto import pb
    from video_edge_ai_proxy_amd.server.grpc_server import ImageService
    from video_edge_ai_proxy_amd.utils import now_ms

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    hub = Hub(cfg, devices=[-1])
    try:
        cam = hub.workers[0].add_camera("door", 2)
        hub.cameras["door"] = CameraHandle("door", 0, cam, "", session=_NoSession())

        class PM:
            pass

        pm = PM()
        pm.hub = hub
        q = _Queue()
        svc = ImageService(pm, _Settings(), None, q)
        req = pb.AnnotateRequest(device_name="door", type="detection", start_timestamp=now_ms(), object_type="person",
                                 confidence=0.87, width=1920, height=1080,
                                 object_bouding_box=pb.BoudingBox(top=100, left=200, width=300, height=400))
        svc.Annotate(req, _Ctx())
        assert len(q.sent) == 1 and hub.overlay("door") == []  # off by default
        cfg.overlay.from_annotations, cfg.overlay.annotation_ttl_ms = True, 700
        now = [5.0]
        hub.overlay_clock = lambda: now[0]
        svc.Annotate(req, _Ctx())
        x0, y0, x1, y1 = overlay.from_pixel_box(200, 100, 500, 500, 1920, 1080)
        assert hub.overlay("door") == [{"type": "box", "x0": x0, "y0": y0, "x1": x1, "y1": y1, "color": [0, 255, 0],
                                        "alpha": 255, "thickness": 0, "fill": False, "label": "person 87%"}]
        assert q.sent == [req.SerializeToString()] * 2  # the queue gets the request as before
        # no box, or no picture size: the queue alone
        for other in (pb.AnnotateRequest(device_name="door", type="t", start_timestamp=now_ms(), width=1920, height=1080),
                      pb.AnnotateRequest(device_name="door", type="t", start_timestamp=now_ms(),
                                         object_bouding_box=pb.BoudingBox(top=1, left=1, width=5, height=5)),
                      pb.AnnotateRequest(device_name="elsewhere", type="t", start_timestamp=now_ms(), width=64, height=64,
                                         object_bouding_box=pb.BoudingBox(top=1, left=1, width=5, height=5))):
            svc.Annotate(other, _Ctx())
        assert len(q.sent) == 5 and len(hub.overlay("door")) == 1
        now[0] = 5.7
        assert hub.overlay("door") == []
    finally:
        hub.shutdown()


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


def test_rest_overlay(native, farm, tmp_path):
    app = _app(tmp_path, **{"buffer.in_memory": 64})
    try:
        rest = _rest(app)
        url = f"rtsp://127.0.0.1:{farm.port}/cam"
        base = "/api/v1/process/door"
        body = {"items": ITEMS}
        assert rest.get("/api/v1/process/nope/overlay").status_code == 404
        assert rest.put("/api/v1/process/nope/overlay", json=body).status_code == 404
        assert rest.delete("/api/v1/process/nope/overlay").status_code == 404
        assert rest.get("/api/v1/process/nope/frame.jpg?overlay=1").status_code == 404
        assert rest.post("/api/v1/process", json={"name": "door", "rtsp_endpoint": url}).status_code == 200
        _first_frame(app.hub, "door")
        assert rest.get(base + "/overlay").json() == {"items": []}
        r = rest.put(base + "/overlay", json=body)
        assert r.status_code == 204 and r.content == b""
        stored = rest.get(base + "/overlay").json()["items"]
        assert [overlay.normalize(i) for i in stored] == [overlay.normalize(i) for i in ITEMS]
        # a bad body: 422, and it changes nothing
        for bad in ([], "nope", {"ttl_ms": 5}, {"items": "x"}, {"items": [dict(BOX, alpha=256)]}, {"items": [BOX] * 65},
                    {"items": [BOX], "ttl_ms": -1}, {"items": [BOX], "ttl_ms": "1"}, {"items": [BOX], "zoom": 1},
                    {"items": [dict(TXT, scale=9)]}):
            assert rest.put(base + "/overlay", json=bad).status_code == 422, bad
        assert rest.put(base + "/overlay", content=b"{not json").status_code == 422
        assert rest.get(base + "/overlay").json()["items"] == stored
        # frame.jpg: the frame named by X-Vep-Seq, with the stored list and the stamp drawn on
        hist = lambda: {int(m["seq"]): (m, f) for m, f in app.hub.history("door", 0, 0)}  # noqa: E731
        for query, items in (("overlay=1", ITEMS), ("stamp=1", [overlay.STAMP]), ("overlay=1&stamp=1", ITEMS + [overlay.STAMP])):
            for attempt in range(5):
                r = rest.get(f"{base}/frame.jpg?quality=80&{query}")
                assert r.status_code == 200 and r.headers["content-type"] == "image/jpeg"
                h = hist()
                if int(r.headers["X-Vep-Seq"]) in h:
                    break
            m, f = h[int(r.headers["X-Vep-Seq"])]
            assert r.content == native.jpeg_encode_cpu(twin(native, f, items, "door", m), 80), query
        r = rest.get(f"{base}/frame.jpg?quality=80&overlay=1&stamp=1&width=160")
        m, f = hist()[int(r.headers["X-Vep-Seq"])]
        assert r.content == native.jpeg_encode_cpu(
            twin(native, native.resize_area_cpu(f, 160, 120), ITEMS + [overlay.STAMP], "door", m), 80)
        # without the new parameters: today's bytes
        r = rest.get(f"{base}/frame.jpg?quality=80")
        assert r.content == native.jpeg_encode_cpu(hist()[int(r.headers["X-Vep-Seq"])][1], 80)
        r = rest.get(f"{base}/frame.jpg?quality=80&overlay=0&stamp=0")
        assert r.content == native.jpeg_encode_cpu(hist()[int(r.headers["X-Vep-Seq"])][1], 80)
        assert rest.get(f"{base}/frame.jpg?overlay=2").status_code == 400
        # a stored list that cannot be drawn: 422
        assert rest.put(base + "/overlay", json={"items": oo.dense() + [BOX]}).status_code == 204
        assert rest.get(f"{base}/frame.jpg?overlay=1").status_code == 422
        assert rest.put(base + "/overlay", json={"items": ITEMS, "ttl_ms": 60000}).status_code == 204
        # stream.mjpg takes the same two parameters
        r = rest.get(f"{base}/stream.mjpg?frames=2&fps=1000&quality=80&overlay=1&stamp=1&width=160")
        assert r.status_code == 200
        parts = [p for p in r.content.split(b"--vepframe") if b"X-Vep-Seq" in p] or [
            p for p in r.content.split(b"\r\n--") if b"X-Vep-Seq" in p]
        assert len(parts) == 2
        h = hist()
        for p in parts:
            head, _, rest_of = p.partition(b"\r\n\r\n")
            seq = int(head.split(b"X-Vep-Seq: ")[1].split(b"\r\n")[0])
            n = int(head.split(b"Content-Length: ")[1].split(b"\r\n")[0])
            if seq in h:
                m, f = h[seq]
                assert rest_of[:n] == native.jpeg_encode_cpu(
                    twin(native, native.resize_area_cpu(f, 160, 120), ITEMS + [overlay.STAMP], "door", m), 80)
        # the wall
        r = rest.get("/api/v1/wall.jpg?tile=160x120&quality=85&labels=1")
        assert r.status_code == 200 and r.headers["X-Vep-Wall"].startswith("door:")
        seq = int(r.headers["X-Vep-Wall"].split(":")[1])
        f = hist()[seq][1]
        assert r.content == native.jpeg_encode_cpu(wall_twin(native, [native.resize_area_cpu(f, 160, 120)], ["door"], 0, 160, 120), 85)
        r = rest.get("/api/v1/wall.jpg?tile=160x120&quality=85")
        seq = int(r.headers["X-Vep-Wall"].split(":")[1])
        assert r.content == native.jpeg_encode_cpu(
            native.compose_wall_cpu([native.resize_area_cpu(hist()[seq][1], 160, 120)], 0, 160, 120), 85)
        assert rest.get("/api/v1/wall.jpg?labels=2").status_code == 400
        assert rest.get("/api/v1/wall.mjpg?frames=1&fps=1000&labels=1&tile=160x120").status_code == 200
        app.hub.cfg.serving.wall_max_tiles = 200
        for w in app.hub.workers:
            w.wall_max_tiles = 200
        names = ",".join(["door"] * 129)
        assert rest.get(f"/api/v1/wall.jpg?names={names}&tile=16x16&labels=1").status_code == 422
        assert rest.get(f"/api/v1/wall.jpg?names={names}&tile=16x16").status_code == 200
        # metrics
        text = rest.get("/metrics").text
        requests, prims = app.hub.overlay_counts()
        assert _metric(text, "vep_overlay_requests_total") == requests >= 8
        assert _metric(text, "vep_overlay_primitives_total") == prims >= 40
        # DELETE
        assert rest.delete(base + "/overlay").status_code == 204
        assert rest.get(base + "/overlay").json() == {"items": []}
        # the CLI is a client of frame.jpg and of .../overlay
        from video_edge_ai_proxy_amd import cli

        a = cli.build_parser().parse_args(["frame", "--device", "door", "--rest", "hub:9000", "--overlay", "--stamp",
                                           "--width", "160", "--out", "x.jpg"])
        assert a.fn is cli.cmd_frame and cli.frame_jpg_url(a) == "http://hub:9000" + base + "/frame.jpg?overlay=1&stamp=1&width=160"
        assert rest.get(cli.frame_jpg_url(a)[len("http://hub:9000"):]).status_code == 200
        # with gpu.isolation: process the hub refuses, and REST answers 501

        def refuse(*a, **k):
            raise NotImplementedError("overlays are not served with gpu.isolation: process")

        saved = app.hub.latest_jpeg, app.hub.wall_jpeg
        app.hub.set_overlay = app.hub.overlay = app.hub.clear_overlay = refuse
        app.hub.latest_jpeg = lambda *a, **k: refuse() if (k.get("overlay") is not None or k.get("stamp")) else saved[0](*a, **k)
        app.hub.wall_jpeg = lambda *a, **k: refuse() if k.get("labels") else saved[1](*a, **k)
        try:
            assert rest.get(base + "/overlay").status_code == 501
            assert rest.put(base + "/overlay", json=body).status_code == 501
            assert rest.delete(base + "/overlay").status_code == 501
            assert rest.get(base + "/frame.jpg?overlay=1").status_code == 501
            assert rest.get(base + "/frame.jpg?stamp=1").status_code == 501
            assert rest.get(base + "/stream.mjpg?frames=1&stamp=1").status_code == 501
            assert rest.get("/api/v1/wall.jpg?labels=1").status_code == 501
            assert rest.get(base + "/frame.jpg").status_code == 200
        finally:
            del app.hub.set_overlay, app.hub.overlay, app.hub.clear_overlay, app.hub.latest_jpeg, app.hub.wall_jpeg
    finally:
        app.stop()


def test_cli_overlay(native, tmp_path, monkeypatch, capsys):
    """`vep overlay` talks to .../overlay; `vep frame --overlay` fetches frame.jpg and writes it."""
    import io
    import urllib.request

    from video_edge_ai_proxy_amd import cli

    seen = []

    class Reply(io.BytesIO):
        headers = {"X-Vep-Seq": "12"}

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

    def urlopen(req, timeout=None):
        if isinstance(req, str):
            seen.append(("GET", req, None))
            if req.endswith("/overlay"):
                return Reply(json.dumps({"items": [BOX]}).encode())
            return Reply(b"\xff\xd8jpeg\xff\xd9")
        seen.append((req.get_method(), req.full_url, req.data))
        return Reply(b"")

    monkeypatch.setattr(urllib.request, "urlopen", urlopen)
    out = tmp_path / "osd.jpg"
    cli.main(["frame", "--device", "front door", "--overlay", "--out", str(out)])
    assert out.read_bytes() == b"\xff\xd8jpeg\xff\xd9"
    assert seen[-1][1] == "http://127.0.0.1:8080/api/v1/process/front%20door/frame.jpg?overlay=1"
    with pytest.raises(SystemExit):
        cli.main(["frame", "--device", "d", "--stamp", "--out", str(tmp_path / "x.ppm")])
    cli.main(["overlay", "--device", "d", "--set", json.dumps([BOX]), "--ttl-ms", "500"])
    assert seen[-2][0] == "PUT" and json.loads(seen[-2][2]) == {"items": [BOX], "ttl_ms": 500}
    assert seen[-1][:2] == ("GET", "http://127.0.0.1:8080/api/v1/process/d/overlay")
    assert "1 item(s)" in capsys.readouterr().out
    cli.main(["overlay", "--device", "d", "--clear"])
    assert seen[-2][0] == "DELETE"
    with pytest.raises(SystemExit):
        cli.main(["overlay", "--device", "d", "--set", "[]", "--clear"])
    with pytest.raises(SystemExit):
        cli.main(["overlay", "--device", "d", "--set", "{not json"])
