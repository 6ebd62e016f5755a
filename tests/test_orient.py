"""Orientation (csrc/vep/orient.h, docs/ORIENT.md) without a GPU: the CPU twin against numpy alone,
the closed forms, check_job's refusals, and the serving reads through Hub and REST on the CPU backend."""
import numpy as np
import pytest

from test_crop import _NoSession, _app, _first_frame, _metric, _rest, _slots, farm  # noqa: F401

ORIENTS = [(r, f) for r in (0, 90, 180, 270) for f in ("none", "h", "v")]
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 3), (67, 19)]


def turned(a, rotate, flip):
    """The reference: numpy alone."""
    a = np.rot90(a, -rotate // 90)
    return np.ascontiguousarray({"none": a, "h": np.fliplr(a), "v": np.flipud(a)}[flip])


def picture(w, h, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


@pytest.mark.parametrize("rotate,flip", ORIENTS)
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_twin_equals_numpy(native, size, rotate, flip):
    a = picture(*size)
    assert np.array_equal(native.orient_cpu(a, rotate, flip), turned(a, rotate, flip))


def test_closed_forms_and_refusals(native):
    a = picture(67, 19, 2)
    b = a
    for _ in range(4):
        b = native.orient_cpu(b, 90, "none")
    assert np.array_equal(b, a)  # four quarter turns
    assert np.array_equal(native.orient_cpu(a, 180, "none"), native.orient_cpu(native.orient_cpu(a, 0, "h"), 0, "v"))
    for bad in ((a, 45, "none"), (a, 90, "d"), (a, 90, 3), (np.zeros((4, 4, 2), np.uint8), 0, "none")):
        with pytest.raises(ValueError):
            native.orient_cpu(*bad)
    # check_job, met through the batch call, which checks every job before anything is launched:
    # a destination that overlaps the source, one too short for oh rows of ow pixels, a side of 0
    src, dst = np.zeros(5 * 3 * 3, np.uint8), np.zeros(5 * 3 * 3, np.uint8)
    s, d = src.ctypes.data, dst.ctypes.data
    for job, what in ((((s, 45, 15), (s + 44, 45, 9), 5, 3, 90, 0), "overlaps"), (((s, 45, 15), (d, 44, 9), 5, 3, 90, 0), "outside"),
                      (((s, 45, 15), (d, 45, 15), 5, 3, 90, 0), "outside"), (((s, 45, 15), (d, 45, 9), 0, 3, 90, 0), "1..65535")):
        with pytest.raises(ValueError, match=what):
            native.orient_device_batch([job], 0)


def test_hub_oriented_reads(native, tmp_path):
    from conftest import synth
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub
    from video_edge_ai_proxy_amd.engine.isolated import ProcessHub

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    hub = Hub(cfg, devices=[-1])
    try:
        wk = hub.workers[0]
        cam = wk.add_camera("a", _slots(native, 3), 3)
        hub.cameras["a"] = CameraHandle("a", 0, cam, "", session=_NoSession())
        hub.set_privacy_masks("a", [{"x0": 0, "y0": 0, "x1": 2500, "y1": 2500, "mode": "fill", "b": 1, "g": 2, "r": 3}])
        enc = synth(native, 320, 240, gop=6, motion=0.2, seed=2)
        for _ in range(2):
            assert wk.decode_now(cam, enc.next())
        newest = wk.read_latest(cam, 0)[1]
        assert (newest[:60, :80] == (1, 2, 3)).all() and not (newest[:60, 240:] == (1, 2, 3)).all()
        plain = hub.latest_jpeg("a", quality=80)
        assert "orient" not in plain[0] and plain[1] == native.jpeg_encode_cpu(newest, 80)
        m, jpg = hub.latest_jpeg("a", quality=80, orient={"rotate": 90})
        assert (m["orient"], m["width"], m["height"]) == ("90", 240, 320) and jpg == native.jpeg_encode_cpu(turned(newest, 90, "none"), 80)
        m, jpg = hub.latest_jpeg("a", quality=80, orient={"rotate": 270, "flip": "h"}, width=120)  # the box is the upright picture's
        want = native.resize_area_cpu(turned(newest, 270, "h"), 120, 160)
        assert (m["orient"], m["width"], m["height"]) == ("270,h", 120, 160) and jpg == native.jpeg_encode_cpu(want, 80)
        # the privacy mask is in the slot and turns with the picture: top-left -> top-right
        seq, up = hub.latest_oriented("a", rotate=90)
        assert seq == 2 and np.array_equal(up, turned(newest, 90, "none"))
        assert (up[:80, 180:] == (1, 2, 3)).all() and not (up[:80, :60] == (1, 2, 3)).all()
        small = hub.latest_scaled("a", width=150)[1]
        assert np.array_equal(hub.latest_oriented("a", width=150, flip="v")[1], native.resize_area_cpu(turned(newest, 0, "v"), *small.shape[1::-1]))
        assert np.array_equal(hub.latest_oriented("a")[1], newest)  # the identity: the frame, not counted
        assert hub.latest_jpeg("a", quality=80, orient={"rotate": 0, "flip": "none"}) == plain
        # behind the deinterlacing, ahead of the rest: upright labels on the upright picture
        chain = hub.latest_jpeg("a", quality=80, orient={"rotate": 90}, deinterlace=True, dehaze=True, enhance=True, stamp=True)
        assert (chain[0]["width"], chain[0]["height"], chain[0]["deinterlace_frames"]) == (240, 320, 2)
        assert hub.orient_count() == 5
        for bad in ({"rotate": 45}, {"flip": "d"}, {"rotate": "90"}, {"turn": 90}, 90):
            with pytest.raises(ValueError):
                hub.latest_jpeg("a", orient=bad)
        with pytest.raises(NotImplementedError, match="gpu.isolation: process"):
            ProcessHub.latest_jpeg(object(), "a", orient={"rotate": 90})
    finally:
        hub.shutdown()


def test_rest_oriented_frames(native, farm, tmp_path):
    url = f"rtsp://127.0.0.1:{farm.port}/cam"
    app = _app(tmp_path, **{"buffer.in_memory": 64, "orient.cameras": {"hall": {"rotate": 90, "flip": "h"}}})
    try:
        rest = _rest(app)
        for name in ("yard", "hall"):
            assert rest.post("/api/v1/process", json={"name": name, "rtsp_endpoint": url}).status_code == 200
            _first_frame(app.hub, name)

        def frame(name, query):
            r = rest.get(f"/api/v1/process/{name}/frame.jpg?quality=80{query}")
            assert r.status_code == 200, r.text
            hist = {int(m["seq"]): f for m, f in app.hub.history(name, 0, 0)}
            return r, hist[int(r.headers["X-Vep-Seq"])]

        r, f = frame("yard", "")  # no parameter, no config entry: the bytes of ever
        assert "X-Vep-Orient" not in r.headers and r.content == native.jpeg_encode_cpu(f, 80)
        r, f = frame("yard", "&rotate=90")
        assert r.headers["X-Vep-Orient"] == "90" and r.content == native.jpeg_encode_cpu(turned(f, 90, "none"), 80)
        r, f = frame("yard", "&flip=v&width=160&overlay=1&stamp=1&enhance=clahe")
        assert r.headers["X-Vep-Orient"] == "0,v"
        r, f = frame("hall", "")  # the camera's mounting applies by default
        assert r.headers["X-Vep-Orient"] == "90,h" and r.content == native.jpeg_encode_cpu(turned(f, 90, "h"), 80)
        r, f = frame("hall", "&rotate=0&flip=none")  # and an explicit identity returns the sensor picture
        assert "X-Vep-Orient" not in r.headers and r.content == native.jpeg_encode_cpu(f, 80)
        r = rest.get("/api/v1/process/hall/stream.mjpg?frames=1&width=160")
        assert r.status_code == 200 and b"X-Vep-Orient: 90,h\r\n" in r.content
        for q in ("rotate=45", "rotate=-90", "flip=d", "rotate=90&flip=hv"):
            assert rest.get(f"/api/v1/process/yard/frame.jpg?{q}").status_code == 422, q
            assert rest.get(f"/api/v1/process/yard/stream.mjpg?frames=1&{q}").status_code == 422, q
        assert _metric(rest.get("/metrics").text, "vep_orient_requests_total") == app.hub.orient_count() == 4
    finally:
        app.stop()
    from video_edge_ai_proxy_amd import cli
    from video_edge_ai_proxy_amd.config import Config, validate

    a = cli.build_parser().parse_args(["frame", "--device", "yard", "--rest", "h:1", "--rotate", "270", "--flip", "h", "--out", "x.jpg"])
    assert cli.frame_jpg_url(a) == "http://h:1/api/v1/process/yard/frame.jpg?rotate=270&flip=h"
    cfg = Config()
    cfg.orient.cameras = {"hall": {"rotate": 30}}
    with pytest.raises(ValueError, match="orient"):
        validate(cfg)
