"""Privacy masks on the CPU: the twin (csrc/vep/mask.cpp) against the independent numpy oracle
(mask_oracle.py) and closed forms, then the Worker's CPU backend, the Hub, REST, persistence."""
import json
import time

import numpy as np
import pytest

import mask_oracle as mo
import motion_oracle as motion_o
import tamper_oracle as tamper_o
from conftest import synth
from video_edge_ai_proxy_amd import privacy


def twin(native, p, masks):
    out = np.array(p, copy=True)
    native.mask_apply_cpu(out, privacy.to_native(masks))
    return out


def check(native, p, masks):
    """twin == oracle, exactly; pixels outside every rect are the input's."""
    got, want = twin(native, p, masks), mo.apply(p, masks)
    assert np.array_equal(got, want), (p.shape, masks, int((got != want).sum()))
    h, w = p.shape[:2]
    outside = np.ones((h, w), bool)
    for m in masks:
        x0, y0, x1, y1 = mo.to_pixels(w, h, m)
        outside[y0:y1, x0:x1] = False
    assert np.array_equal(got[outside], p[outside])
    return got


SMALL = [(7, 5), (17, 9), (1, 9), (9, 1), (64, 48), (200, 120)]


@pytest.mark.parametrize("size", SMALL)
def test_twin_equals_oracle(native, size):
    w, h = size
    for kind in ("noise", "gradient"):
        p = mo.picture(kind, w, h, seed=w + h)
        for m in mo.cases(w, h):
            check(native, p, [m])


def test_twin_equals_oracle_block_128(native):
    p = mo.picture("noise", 300, 260, seed=3)
    for m in mo.cases(300, 260, blocks=(128,)):
        check(native, p, [m])


def test_twin_equals_oracle_wide_strip(native):
    p = mo.picture("noise", 9000, 3, seed=4)
    for m in mo.cases(9000, 3, blocks=(4, 128)):
        check(native, p, [m])


def test_twin_equals_oracle_1080p(native):
    p = mo.picture("noise", 1920, 1080, seed=5)
    check(native, p, [{"x0": 0, "y0": 0, "x1": 10000, "y1": 10000, "mode": "pixelate", "block": 16},
                      mo.rect_mask(1920, 1080, 1, 3, 482, 271, mode="pixelate", block=48),
                      mo.rect_mask(1920, 1080, 1437, 700, 1920, 1080, mode="fill", b=1, g=2, r=3)])


# ------------------------------------------------------------------------------- to_pixels

def px(native, w, h, **m):
    return native.mask_pixels(w, h, privacy.to_native([dict(m)])[0])


def test_to_pixels_rounds_outward(native):
    assert px(native, 1920, 1080, x0=1, y0=1, x1=9999, y1=9999) == (0, 0, 1920, 1080)
    assert px(native, 1920, 1080, x0=0, y0=0, x1=10000, y1=10000) == (0, 0, 1920, 1080)
    assert px(native, 1920, 1080, x0=2500, y0=5000, x1=7500, y1=10000) == (480, 540, 1440, 1080)
    # 1/10000 of 1920 is 0.192 pixel: the rect still has one pixel, the one it lies in
    assert px(native, 1920, 1080, x0=5000, y0=5000, x1=5001, y1=5001) == (960, 540, 961, 541)
    assert px(native, 1920, 1080, x0=9999, y0=9999, x1=10000, y1=10000) == (1919, 1079, 1920, 1080)
    assert px(native, 1, 1, x0=0, y0=0, x1=1, y1=1) == (0, 0, 1, 1)
    assert px(native, 1, 1, x0=9999, y0=9999, x1=10000, y1=10000) == (0, 0, 1, 1)
    assert px(native, 3, 3, x0=3333, y0=3334, x1=6667, y1=6666) == (0, 1, 3, 2)
    rng = np.random.default_rng(7)
    for _ in range(2000):
        w, h = int(rng.integers(1, 65536)), int(rng.integers(1, 65536))
        x0, y0 = int(rng.integers(0, 10000)), int(rng.integers(0, 10000))
        x1, y1 = int(rng.integers(x0 + 1, 10001)), int(rng.integers(y0 + 1, 10001))
        got = px(native, w, h, x0=x0, y0=y0, x1=x1, y1=y1)
        assert got == mo.to_pixels(w, h, {"x0": x0, "y0": y0, "x1": x1, "y1": y1})
        gx0, gy0, gx1, gy1 = got
        assert 0 <= gx0 < gx1 <= w and 0 <= gy0 < gy1 <= h  # never empty, never outside
        # outward: the pixel rect covers the exact rect
        assert gx0 * 10000 <= x0 * w and gx1 * 10000 >= x1 * w and gy0 * 10000 <= y0 * h and gy1 * 10000 >= y1 * h


# ----------------------------------------------------------------------------- closed forms

def test_closed_forms(native):
    w, h = 61, 45
    p = mo.picture("noise", w, h, seed=9)
    pix = mo.rect_mask(w, h, 3, 2, 58, 41, mode="pixelate", block=8)
    fill = mo.rect_mask(w, h, 5, 7, 33, 30, mode="fill", b=10, g=200, r=77)
    once = check(native, p, [pix])
    assert np.array_equal(twin(native, once, [pix]), once)  # pixelate is idempotent
    assert not np.array_equal(once, p)
    f1 = check(native, p, [fill])
    assert np.array_equal(twin(native, f1, [fill]), f1)  # fill is idempotent
    assert (f1[7:30, 5:33] == (10, 200, 77)).all()
    u = mo.picture("uniform", w, h, seed=2)
    assert np.array_equal(twin(native, u, [pix]), u)  # a uniform picture is unchanged
    # a 0 / 255 checker of period 1: every block of even area is half 0, half 255: 127.5 rounds up
    c = mo.picture("checker", 64, 48)
    out = twin(native, c, [mo.rect_mask(64, 48, 8, 4, 56, 44, mode="pixelate", block=8)])
    assert (out[4:44, 8:56] == 128).all() and np.array_equal(out[:4], c[:4]) and np.array_equal(out[:, :8], c[:, :8])
    # a 3 x 3 block of the checker anchored on a 0 pixel holds five 0 and four 255: (1020 + 4) // 9 = 113
    out = twin(native, c, [mo.rect_mask(64, 48, 10, 10, 13, 13, mode="pixelate", block=4)])
    assert (out[10:13, 10:13] == 113).all()


def test_list_order(native):
    w, h = 80, 60
    p = mo.picture("noise", w, h, seed=11)
    fill = mo.rect_mask(w, h, 10, 10, 50, 40, mode="fill", b=255, g=0, r=0)
    pix = mo.rect_mask(w, h, 30, 20, 70, 55, mode="pixelate", block=16)
    a, b = check(native, p, [fill, pix]), check(native, p, [pix, fill])
    assert not np.array_equal(a, b)
    assert (b[10:40, 10:50] == (255, 0, 0)).all() and not (a[10:40, 10:50] == (255, 0, 0)).all()


def lv(native, w, h, masks):
    return native.mask_levels(w, h, privacy.to_native(masks))


def test_levels(native):
    w, h = 100, 100
    r = lambda *a, **k: mo.rect_mask(w, h, *a, **k)  # noqa: E731
    disjoint = [r(0, 0, 10, 10), r(10, 0, 20, 10), r(0, 10, 10, 20), r(50, 50, 100, 100)]
    assert lv(native, w, h, disjoint) == [0, 0, 0, 0]  # rects that touch do not intersect
    chain = [r(0, 0, 30, 30), r(20, 20, 50, 50), r(40, 40, 70, 70), r(60, 60, 90, 90)]
    assert lv(native, w, h, chain) == [0, 1, 2, 3]
    nested = [r(0, 0, 100, 100), r(10, 10, 90, 90), r(20, 20, 30, 30), r(95, 95, 100, 100)]
    assert lv(native, w, h, nested) == [0, 1, 2, 1]
    mixed = [r(0, 0, 10, 10), r(50, 50, 60, 60), r(5, 5, 55, 55), r(70, 70, 80, 80), r(0, 0, 100, 100)]
    assert lv(native, w, h, mixed) == [0, 0, 1, 0, 2]
    assert lv(native, w, h, []) == []
    for ms in (disjoint, chain, nested, mixed):
        assert lv(native, w, h, ms) == mo.levels(w, h, ms)
    # sub-pixel neighbours: disjoint in 1/10000, but outward rounding makes them share a pixel
    a = {"x0": 0, "y0": 0, "x1": 5000, "y1": 10000}
    b = {"x0": 5000, "y0": 0, "x1": 10000, "y1": 10000}
    assert lv(native, 100, 100, [a, b]) == [0, 0] and lv(native, 101, 100, [a, b]) == [0, 1]


GOOD = {"x0": 0, "y0": 0, "x1": 5000, "y1": 5000, "mode": "pixelate", "block": 16}


RANGE_ERRORS = [
    [GOOD] * 9,
    [dict(GOOD, x0=5000)], [dict(GOOD, x0=6000)], [dict(GOOD, y0=5000)],
    [dict(GOOD, x1=10001)], [dict(GOOD, y1=10001)], [dict(GOOD, x0=-1)],
    [dict(GOOD, block=3)], [dict(GOOD, block=129)], [dict(GOOD, mode="fill", b=256)],
]


@pytest.mark.parametrize("bad", RANGE_ERRORS + [
    [dict(GOOD, mode="blur")], [dict(GOOD, mode=2)], [dict(GOOD, x0=1.5)], [dict(GOOD, colour=1)], ["x"], GOOD,
])
def test_validation(native, bad):
    import torch

    from video_edge_ai_proxy_amd import ops

    with pytest.raises(ValueError):
        privacy.to_native(bad)
    with pytest.raises(ValueError):
        ops.privacy_mask_reference(torch.zeros((8, 8, 3), dtype=torch.uint8), bad)


@pytest.mark.parametrize("bad", RANGE_ERRORS)
def test_native_validation(native, bad):
    """What is wrong with a list's numbers is refused by the native layer too, not only in Python."""
    raw = [(m["x0"], m["y0"], m["x1"], m["y1"], privacy.MODES.index(m["mode"]), m["block"], m.get("b", 0),
            m.get("g", 0), m.get("r", 0)) for m in bad]
    wk = native.Worker(device=-1)
    cam = wk.add_camera("c", 2)
    with pytest.raises(ValueError):
        wk.set_privacy_masks(cam, raw)
    with pytest.raises(ValueError):
        native.mask_levels(8, 8, raw)
    with pytest.raises(ValueError):
        native.mask_apply_cpu(np.zeros((8, 8, 3), np.uint8), raw)
    assert wk.privacy_masks(cam) == []


def test_native_refuses_unknown_mode(native):
    wk = native.Worker(device=-1)
    cam = wk.add_camera("c", 2)
    with pytest.raises(ValueError):
        wk.set_privacy_masks(cam, [(0, 0, 5000, 5000, 2, 16, 0, 0, 0)])
    with pytest.raises(ValueError):
        native.mask_pixels(8, 8, (0, 0, 5000, 5000, -1, 16, 0, 0, 0))
    ok = [(0, 0, 5000, 5000, 1, 16, 0, 0, 0)]
    wk.set_privacy_masks(cam, ok)
    assert wk.privacy_masks(cam) == ok
    wk.set_privacy_masks(cam, [])
    assert wk.privacy_masks(cam) == []


def test_reference_op(native):
    import torch

    from video_edge_ai_proxy_amd import ops

    p = mo.picture("noise", 50, 30, seed=1)
    t = torch.from_numpy(p.copy())
    out = ops.privacy_mask_reference(t, [GOOD])
    assert np.array_equal(out.numpy(), mo.apply(p, [GOOD])) and np.array_equal(t.numpy(), p)  # the input is left alone
    for bad in (t.float(), t[:, :, :2], t[:, ::2], t[0]):
        with pytest.raises(ValueError):
            ops.privacy_mask_reference(bad, [GOOD])
    with pytest.raises(ValueError):
        ops.privacy_mask(t, [GOOD])  # a host tensor


# ------------------------------------------------------------------------ CPU-backend Worker

MASKS = [{"x0": 1000, "y0": 500, "x1": 6100, "y1": 7300, "mode": "pixelate", "block": 16},
         {"x0": 5000, "y0": 6000, "x1": 10000, "y1": 10000, "mode": "fill", "b": 9, "g": 99, "r": 199},
         {"x0": 0, "y0": 0, "x1": 1500, "y1": 1500, "mode": "pixelate", "block": 5}]


def _pair(native, w=320, h=240, history=0, slots=2, **kw):
    """One worker, two cameras fed the same stream: `plain` unmasked, `masked` with MASKS set
    before its first access unit."""
    wk = native.Worker(device=-1)
    plain, masked = wk.add_camera("plain", slots, history), wk.add_camera("masked", slots, history)
    wk.set_privacy_masks(masked, privacy.to_native(MASKS))
    encs = [synth(native, w, h, gop=6, motion=0.2, **kw) for _ in range(2)]

    def step():
        for cam, enc in zip((plain, masked), encs):
            assert wk.decode_now(cam, enc.next())

    return wk, plain, masked, step


def test_worker_publishes_only_masked_frames(native):
    wk, plain, masked, step = _pair(native, history=3, slots=wk_slots(native, 3))
    step()
    m0, f0 = wk.read_latest(plain, 0)
    want0 = mo.apply(f0, MASKS)
    assert not np.array_equal(want0, f0)
    mm, got = wk.read_latest(masked, 0)
    assert np.array_equal(got, want0) and mm["seq"] == m0["seq"] == 1
    # every serving path reads the slot: JPEG, scaled, the wall, history
    assert wk.read_latest_jpeg(masked, 0, 80)[1] == native.jpeg_encode_cpu(want0, 80)
    assert wk.read_latest_jpeg(masked, 0, 80, 160, 120)[1] == native.jpeg_encode_cpu(native.resize_area_cpu(want0, 160, 120), 80)
    assert np.array_equal(wk.read_latest_scaled(masked, 0, 160, 0)[1], native.resize_area_cpu(want0, 160, 120))
    assert wk.read_wall_jpeg([masked, plain], 0, 160, 120, 85)[1] == native.jpeg_encode_cpu(
        native.compose_wall_cpu([want0, f0], 0, 160, 120), 85)
    # the detectors see the masked picture
    tp, mp = wk.tamper_params, wk.motion_params
    rt = wk.read_tamper(masked, 0)
    for key, plane in zip(("hist", "sum_y", "energy"), tamper_o.stats(want0, tp["cell"])):
        assert np.array_equal(rt[key], plane), key
    r0 = wk.read_motion(masked, 0)
    counts0, bg = motion_o.update(want0, None, mp["cell"], mp["threshold"], mp["learn_shift"])
    assert np.array_equal(r0["counts"], counts0)
    step()
    step()
    frames = [f for _, f in wk.read_history(plain, 0, 3)]
    hist = wk.read_history(masked, 0, 3)
    assert len(frames) == len(hist) == 3
    for f, (meta, g) in zip(frames, hist):
        assert np.array_equal(g, mo.apply(f, MASKS))
    counts2, _ = motion_o.update(hist[-1][1], bg, mp["cell"], mp["threshold"], mp["learn_shift"])
    assert np.array_equal(wk.read_motion(masked, 0)["counts"], counts2)
    st = wk.stats(masked)
    assert st["masked_frames"] == 3 and st["mask_dropped"] == 0 and wk.stats(plain)["masked_frames"] == 0
    assert privacy.from_native(wk.privacy_masks(masked)) == privacy.normalize_list(MASKS)


def wk_slots(native, history):
    return native.Worker(device=-1).history_ring_slots(history)


def test_worker_mask_change_fails_closed(native):
    wk, plain, masked, step = _pair(native, history=2, slots=wk_slots(native, 2))
    step()
    step()
    assert wk.read_latest(plain, 0)[0]["seq"] == 2 and len(wk.read_history(plain, 0, 2)) == 2
    assert wk.read_tamper(plain, 0) is not None and wk.tamper_set_reference(plain)
    # a change on a camera with frames: nothing published so far stays readable
    new = [{"x0": 0, "y0": 0, "x1": 10000, "y1": 10000, "mode": "pixelate", "block": 32}]
    wk.set_privacy_masks(plain, privacy.to_native(new))
    assert wk.read_latest(plain, 0) is None and wk.read_history(plain, 0, 2) == []
    assert wk.read_latest_jpeg(plain, 0, 80) is None and wk.read_latest_scaled(plain, 0, 160, 0) is None
    assert wk.read_motion(plain, 0) is None and wk.read_tamper(plain, 0) is None
    assert wk.stats(plain)["published"] == 2  # the counter does not go back
    step()
    m, f = wk.read_latest(plain, 0)
    _, fm = wk.read_latest(masked, 0)
    assert m["seq"] == 3 and wk.stats(plain)["published"] == 3
    # `masked` published oracle(MASKS)(frame); recover nothing from it: decode the frame on a third camera
    ref = native.Worker(device=-1)
    rc = ref.add_camera("ref", 2)
    enc = synth(native, 320, 240, gop=6, motion=0.2)
    for _ in range(3):
        assert ref.decode_now(rc, enc.next())
    raw = ref.read_latest(rc, 0)[1]
    assert np.array_equal(f, mo.apply(raw, new)) and np.array_equal(fm, mo.apply(raw, MASKS))
    assert [x[0]["seq"] for x in wk.read_history(plain, 0, 2)] == [3]  # the older frames are gone for good
    assert wk.read_tamper(plain, 0)["has_reference"] is False  # the detectors started over
    assert wk.read_motion(plain, 0)["primed"] is False
    # clearing behaves the same way, and the next frame is the unmasked camera's
    wk.set_privacy_masks(masked, [])
    assert wk.read_latest(masked, 0) is None and wk.read_history(masked, 0, 2) == []
    assert wk.stats(masked)["published"] == 3
    step()
    for _ in range(1):
        assert ref.decode_now(rc, enc.next())
    raw = ref.read_latest(rc, 0)[1]
    assert np.array_equal(wk.read_latest(masked, 0)[1], raw)
    assert np.array_equal(wk.read_latest(plain, 0)[1], mo.apply(raw, new))
    assert wk.stats(masked)["masked_frames"] == 3 and wk.stats(plain)["masked_frames"] == 2


def test_masks_survive_a_resolution_change(native):
    wk = native.Worker(device=-1)
    cam, ref = wk.add_camera("c", 2), wk.add_camera("ref", 2)
    wk.set_privacy_masks(cam, privacy.to_native(MASKS))
    for size in ((320, 240), (176, 144), (320, 240)):
        encs = [synth(native, *size, gop=6, motion=0.2, seed=5) for _ in range(2)]
        for _ in range(2):
            assert wk.decode_now(cam, encs[0].next()) and wk.decode_now(ref, encs[1].next())
        raw = wk.read_latest(ref, 0)[1]
        assert raw.shape[:2] == size[::-1]
        # the same units (1/10000 of the picture) give new pixels
        assert np.array_equal(wk.read_latest(cam, 0)[1], mo.apply(raw, MASKS))


@pytest.mark.parametrize("codec", ["h264", "h265"])
def test_earlier_outputs_of_a_multi_picture_job_are_masked(native, codec):
    """A job of several pictures (general decoders, history > 0) converts its earlier outputs into
    ring slots of their own: each of them is masked too."""
    from history_util import avc_stream, hevc_stream

    aus = avc_stream(native, 12)[0] if codec == "h264" else hevc_stream(native, 12, 64, 64)[0]
    wk = native.Worker(device=-1)
    slots = wk.history_ring_slots(5)
    cam, ref = wk.add_camera("c", slots, 5), wk.add_camera("ref", slots, 5)
    wk.set_privacy_masks(cam, privacy.to_native(MASKS))
    wk.decode_many([(cam, aus[:9]), (ref, aus[:9])])
    for au in aus[9:]:
        wk.decode_many([(cam, [au]), (ref, [au])])
    got, raw = wk.read_history(cam, 0, 5), wk.read_history(ref, 0, 5)
    assert len(got) == len(raw) == 5
    for (mg, fg), (mr, fr) in zip(got, raw):
        assert mg["pts"] == mr["pts"] and mg["seq"] == mr["seq"]
        assert np.array_equal(fg, mo.apply(fr, MASKS)) and not np.array_equal(fg, fr)
    assert wk.stats(cam)["masked_frames"] == wk.stats(cam)["published"] > 5


# ------------------------------------------------------------------- Hub, REST, persistence

class _NoSession:
    def stop(self):
        pass


def test_hub_masks(native, tmp_path):
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, CameraNotFound, Hub

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    hub = Hub(cfg, devices=[-1])
    try:
        wk = hub.workers[0]
        cam = wk.add_camera("a", 2)
        hub.cameras["a"] = CameraHandle("a", 0, cam, "", session=_NoSession())
        enc = synth(native, 160, 96, gop=6, motion=0.2)
        assert hub.privacy_masks("a") == []
        hub.set_privacy_masks("a", MASKS)
        assert hub.privacy_masks("a") == privacy.normalize_list(MASKS)
        assert wk.decode_now(cam, enc.next())
        hub.set_privacy_masks("a", None)
        assert hub.privacy_masks("a") == [] and hub.latest_frame("a") is None
        with pytest.raises(ValueError):
            hub.set_privacy_masks("a", [dict(GOOD, block=2)])
        with pytest.raises(CameraNotFound):
            hub.set_privacy_masks("nope", MASKS)
        with pytest.raises(CameraNotFound):
            hub.privacy_masks("nope")
        with pytest.raises(ValueError):  # before anything is created
            hub.start_camera("b", "rtsp://127.0.0.1:1/x", masks=[dict(GOOD, mode="blur")])
        assert not hub.has("b")
    finally:
        hub.shutdown()


def test_process_hub_forwards_masks():
    from video_edge_ai_proxy_amd.engine.child import EXPORTED
    from video_edge_ai_proxy_amd.engine.isolated import ProcessHub
    import threading

    assert {"set_privacy_masks", "privacy_masks"} <= EXPORTED

    class Fake:
        cameras = {"a": 1}
        _specs = {"a": {"args": ("a",), "masks": []}}
        _lock = threading.RLock()
        calls = []

        def handle(self, name):
            return self.cameras[name]

        def _call(self, name, method, *args):
            self.calls.append((name, method, args))
            return []

    f = Fake()
    ProcessHub.set_privacy_masks(f, "a", MASKS)
    norm = privacy.normalize_list(MASKS)
    assert f.calls[-1] == ("a", "set_privacy_masks", (norm,))
    assert f._specs["a"]["masks"] == norm  # a fresh child process starts the camera under this list
    assert ProcessHub.privacy_masks(f, "a") == [] and f.calls[-1] == ("a", "privacy_masks", ())
    with pytest.raises(ValueError):
        ProcessHub.set_privacy_masks(f, "a", [dict(GOOD, block=1)])
    with pytest.raises(KeyError):
        ProcessHub.set_privacy_masks(f, "nope", MASKS)


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


def _covered(frame, masks):
    """Every block of every pixelate mask is one colour and every fill rect its colour: the frame
    went through the masks (their own output is a fixed point of them)."""
    return np.array_equal(mo.apply(frame, masks), frame)


def test_rest_privacy_and_persistence(native, farm, tmp_path):
    app = _app(tmp_path)
    try:
        rest = _rest(app)
        url = f"rtsp://127.0.0.1:{farm.port}/cam"
        for call in (rest.get, rest.delete):
            assert call("/api/v1/process/nope/privacy").status_code == 404
        assert rest.put("/api/v1/process/nope/privacy", json=[]).status_code == 404
        assert rest.post("/api/v1/process", json={"name": "door", "rtsp_endpoint": url}).status_code == 200
        assert rest.get("/api/v1/process/door/privacy").json() == {"masks": [], "unmasked_outputs": []}
        one = [{"x0": 0, "y0": 0, "x1": 10000, "y1": 10000, "mode": "pixelate", "block": 64}]
        assert rest.put("/api/v1/process/door/privacy", json=one).status_code == 204
        got = rest.get("/api/v1/process/door/privacy").json()
        assert got["masks"] == privacy.normalize_list(one) and got["unmasked_outputs"] == []
        for bad in ([dict(one[0], block=3)], [dict(one[0], mode="blur")], one * 9, {"x0": 0}, "nope", [[1, 2]]):
            assert rest.put("/api/v1/process/door/privacy", json=bad).status_code == 422, bad
        assert rest.put("/api/v1/process/door/privacy", content=b"{not json").status_code == 422
        assert rest.get("/api/v1/process/door/privacy").json()["masks"] == privacy.normalize_list(one)  # unchanged
        _, frame = _first_frame(app.hub, "door")
        assert _covered(frame, one) and len(np.unique(frame.reshape(-1, 3), axis=0)) <= 20  # 5 x 4 blocks
        text = rest.get("/metrics").text
        line = [ln for ln in text.splitlines() if ln.startswith("vep_privacy_masked_frames_total{") and "door" in ln]
        assert len(line) == 1 and float(line[0].rsplit(" ", 1)[1]) >= 1
        assert "vep_privacy_dropped_frames_total{" in text
        # stored under a prefix of its own; the process record keeps its reference shape
        from video_edge_ai_proxy_amd.services.process_manager import PREFIX_PRIVACY_MASKS

        assert json.loads(app.pm.storage.get(PREFIX_PRIVACY_MASKS, "door")) == privacy.normalize_list(one)
        assert "masks" not in json.loads(app.pm.storage.get("/rtspprocess/", "door"))
        assert rest.delete("/api/v1/process/door/privacy").status_code == 204
        assert rest.get("/api/v1/process/door/privacy").json()["masks"] == []
        assert app.pm.storage.list(PREFIX_PRIVACY_MASKS) == {}
        assert rest.put("/api/v1/process/door/privacy", json=one).status_code == 204
    finally:
        app.stop()
    # a restart: restore() starts the camera under the stored list, in force for its first frame
    app = _app(tmp_path)
    try:
        assert app.hub.has("door") or app.pm.restore() == ["door"]
        assert app.hub.privacy_masks("door") == privacy.normalize_list(one)
        _, frame = _first_frame(app.hub, "door")
        assert _covered(frame, one)
        assert app.hub.state("door")["masked_frames"] == app.hub.state("door")["published"] >= 1
        app.pm.stop("door")
        assert app.pm.storage.list(PREFIX_PRIVACY_MASKS) == {}  # stop() deletes the list
    finally:
        app.stop()


def test_unmasked_outputs(native, farm, tmp_path):
    app = _app(tmp_path, **{"buffer.on_disk": True, "gpu.letterbox_size": 64})
    try:
        rest = _rest(app)
        url = f"rtsp://127.0.0.1:{farm.port}/cam"
        body = {"name": "gate", "rtsp_endpoint": url, "rtmp_endpoint": "rtmp://127.0.0.1:1/live/gate"}
        assert rest.post("/api/v1/process", json=body).status_code == 200
        assert rest.get("/api/v1/process/gate/privacy").json()["unmasked_outputs"] == ["rtmp", "archive", "consumer_batch"]
        app.hub.set_proxy("gate", False)
        assert rest.get("/api/v1/process/gate/privacy").json()["unmasked_outputs"] == ["archive", "consumer_batch"]
    finally:
        app.stop()


def test_cli_privacy_parser():
    from video_edge_ai_proxy_amd import cli

    a = cli.build_parser().parse_args(["privacy", "--device", "door"])
    assert (a.cmd, a.device, a.rest, a.set, a.clear, a.fn) == ("privacy", "door", "127.0.0.1:8080", None, False,
                                                               cli.cmd_privacy)
    a = cli.build_parser().parse_args(["privacy", "--device", "d", "--rest", "hub:9000", "--set", "[]"])
    assert (a.rest, a.set) == ("hub:9000", "[]")
    assert cli.build_parser().parse_args(["privacy", "--device", "d", "--clear"]).clear is True
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["privacy"])  # --device is required
    text = cli.format_privacy({"masks": privacy.normalize_list(MASKS[:2]), "unmasked_outputs": ["rtmp", "archive"]})
    assert text == ("mask 0: x 1000..6100 y 500..7300 (1/10000) pixelate block 16\n"
                    "mask 1: x 5000..10000 y 6000..10000 (1/10000) fill bgr (9,99,199)\n"
                    "unmasked outputs: rtmp, archive")
    assert cli.format_privacy({"masks": [], "unmasked_outputs": []}) == "no masks\nunmasked outputs: none"
