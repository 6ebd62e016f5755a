"""Contrast enhancement (CLAHE on luma; csrc/vep/clahe.h, docs/ENHANCE.md) without a GPU: the CPU
twin against the numpy oracle, the closed forms, the float64 bilinear bound, and one read each
through Worker, Hub and REST on the CPU backend."""
import numpy as np
import pytest

import clahe_oracle as oracle
from test_crop import _NoSession, _app, _camera, _first_frame, _metric, _rest, farm  # noqa: F401

BOX = [{"type": "box", "x0": 1000, "y0": 1000, "x1": 6000, "y1": 7000, "color": [0, 255, 0]}]


def dark(w, h, seed=1):
    """A dark scene: a dim ramp with noise, and one bright lamp."""
    rng = np.random.default_rng(seed)
    ramp = (np.arange(w)[None, :] * 40 // max(1, w - 1) + np.arange(h)[:, None] * 20 // max(1, h - 1))[..., None]
    p = ramp + rng.integers(0, 12, (h, w, 3))
    p[h // 3:h // 3 + 5, w // 2:w // 2 + 9] = 250
    return p.astype(np.uint8)


# (w, h, tile, clip16, strength): both last tiles thin; neither thin; a single tile; w below tile / 2
# beside a not-thin last row; h below tile / 2 beside a thin last column; the defaults, both thin
CASES = [(100, 70, 32, 32, 256), (112, 80, 32, 16, 128), (31, 20, 32, 64, 256), (10, 100, 40, 32, 256),
         (200, 9, 64, 4096, 200), (300, 150, 128, 32, 256)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_twin_equals_oracle(native, case):
    w, h, tile, clip16, strength = case
    for p in (dark(w, h), np.random.default_rng(7).integers(0, 256, (h, w, 3)).astype(np.uint8)):
        out, hist, lut = native.clahe_cpu(p, tile, clip16, strength)
        assert hist.sum() == w * h and np.array_equal(lut, oracle.luts(oracle.luma(p), tile, clip16, strength))
        assert np.array_equal(out, oracle.clahe(p, tile, clip16, strength))


def test_closed_forms(native):
    p = dark(150, 90)
    assert np.array_equal(native.clahe_cpu(p, 32, 32, 0)[0], p)  # strength 0: the identity
    # clip16 4096 never clips: the LUT is the rounded cumulative distribution, monotone, ending at 255
    one = dark(40, 30)
    cdf = np.cumsum(np.bincount(oracle.luma(one).ravel(), minlength=256))
    lut = native.clahe_cpu(one, 64, 4096, 256)[2][0, 0]
    assert np.array_equal(lut, (cdf * 255 + 600) // 1200) and lut[255] == 255 and np.all(np.diff(lut.astype(int)) >= 0)
    assert np.array_equal(lut, native.clahe_lut_cpu(np.bincount(oracle.luma(one).ravel(), minlength=256), 1200, 4096, 256))
    with pytest.raises(ValueError, match="sum to n"):
        native.clahe_lut_cpu(np.bincount(oracle.luma(one).ravel(), minlength=256), 1199, 32, 256)
    # one colour: every channel moves by at most 2 + ceil(255 L / n), L = max(1, clip16 n / 4096), over
    # the smallest group (clahe.h derives it): here the 72 x 72 corner group of a 200 x 200 picture
    for clip16 in (16, 32, 1024):
        n = 72 * 72
        bound = 2 + -(-255 * max(1, clip16 * n // 4096) // n)
        for colour in ((0, 0, 0), (9, 30, 17), (200, 120, 90), (255, 255, 255)):
            flat = np.full((200, 200, 3), colour, np.uint8)
            moved = np.abs(native.clahe_cpu(flat, 128, clip16, 256)[0].astype(int) - flat)
            assert moved.max() <= bound, (clip16, colour, moved.max(), bound)


def test_blend_against_float64_bilinear(native):
    """The twin's blended luma against float64 bilinear interpolation of the twin's own LUTs at the
    pixel's true position. On a grey picture luma(Y, Y, Y) = Y, so an output channel IS Y'. The
    integer weights are the true fractions floored to 1/256, so with Dx, Dy the LUT differences along
    the two axes at that pixel the distance is below 1/2 + (Dx + Dy) / 256 (docs/ENHANCE.md, section
    2): within one level wherever Dx + Dy <= 128."""
    for p, tile in ((dark(200, 130), 32), (dark(131, 97, seed=3), 40)):
        p = np.repeat(p[:, :, :1], 3, axis=2)
        out, _, lut = native.clahe_cpu(p, tile, 32, 256)
        assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])

        def place(side):  # tile index and true weight: the position in units of tile centres
            n = -(-side // tile)
            t = np.clip((np.arange(side) + 0.5) / tile - 0.5, 0, n - 1)
            i0 = np.floor(t).astype(int)
            return i0, np.minimum(i0 + 1, n - 1), t - i0

        (i0, i1, fx), (j0, j1, fy) = place(p.shape[1]), place(p.shape[0])
        y, t = p[..., 0].astype(int), lut.astype(float)
        a, b = t[j0[:, None], i0[None], y], t[j0[:, None], i1[None], y]
        c, d = t[j1[:, None], i0[None], y], t[j1[:, None], i1[None], y]
        fx, fy = fx[None, :], fy[:, None]
        want = (1 - fx) * (1 - fy) * a + fx * (1 - fy) * b + (1 - fx) * fy * c + fx * fy * d
        dx, dy = np.maximum(abs(b - a), abs(d - c)), np.maximum(abs(c - a), abs(d - b))
        err = np.abs(out[..., 0] - want)
        print("largest distance", err.max(), "largest Dx + Dy", (dx + dy).max())
        # (1e-9: the float64 reference's own rounding)
        assert np.all(err <= 0.5 + (dx + dy) / 256.0 + 1e-9) and err.max() <= 1.0


def test_worker_enhanced_reads(native):
    wk, cam, step = _camera(native)
    eq = (32, 48, 200)
    assert wk.read_latest_enhanced(cam, 0, 0, 0, *eq) is None and step()
    frame = wk.read_latest(cam, 0)[1]
    plain = wk.read_latest_jpeg(cam, 0, 80)[1]
    assert plain == native.jpeg_encode_cpu(frame, 80) == wk.read_latest_jpeg(cam, 0, 80, 0, 0, None)[1]
    want = oracle.clahe(frame, *eq)
    assert wk.read_latest_jpeg(cam, 0, 80, 0, 0, eq)[1] == native.jpeg_encode_cpu(want, 80) != plain
    m, got = wk.read_latest_enhanced(cam, 0, 0, 0, *eq)
    assert m["seq"] == 1 and np.array_equal(got, want)
    small = wk.read_latest_scaled(cam, 0, 150, 0)[1]  # enhanced AFTER the scale
    m, got = wk.read_latest_enhanced(cam, 0, 150, 0, *eq)
    assert (m["width"], m["height"]) == small.shape[1::-1] and np.array_equal(got, oracle.clahe(small, *eq))
    assert wk.read_latest_jpeg(cam, 0, 80, 150, 0, eq)[1] == native.jpeg_encode_cpu(got, 80)
    assert wk.enhance_count() == 4
    for bad in ((33, 32, 256), (24, 32, 256), (264, 32, 256), (32, 15, 256), (32, 4097, 256), (32, 32, 257)):
        with pytest.raises(ValueError):
            wk.read_latest_jpeg(cam, 0, 80, 0, 0, bad)
        with pytest.raises(ValueError):
            wk.read_latest_enhanced(cam, 0, 0, 0, *bad)


def test_hub_enhanced_reads(native, tmp_path):
    import torch

    from conftest import synth
    from video_edge_ai_proxy_amd import ops
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub
    from video_edge_ai_proxy_amd.engine.isolated import ProcessHub

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    cfg.enhance.tile, cfg.enhance.clip = 64, 3.0
    hub = Hub(cfg, devices=[-1])
    try:
        wk = hub.workers[0]
        cam = wk.add_camera("a", 2)
        hub.cameras["a"] = CameraHandle("a", 0, cam, "", session=_NoSession())
        assert wk.decode_now(cam, synth(native, 320, 240, gop=6, motion=0.2, seed=2).next())
        frame = wk.read_latest(cam, 0)[1]
        want = oracle.clahe(frame, 64, 48, 256)  # the hub's defaults
        assert hub.latest_jpeg("a", quality=80)[1] == native.jpeg_encode_cpu(frame, 80)
        assert hub.latest_jpeg("a", quality=80, enhance=True)[1] == native.jpeg_encode_cpu(want, 80)
        seq, got = hub.latest_enhanced("a", strength=0.5)
        assert seq == 1 and np.array_equal(got, oracle.clahe(frame, 64, 48, 128))
        assert np.array_equal(ops.clahe(torch.from_numpy(frame), 64, 3.0, 0.5).numpy(), got)  # a host tensor: the twin
        # scaled, enhanced, THEN drawn on: the box keeps its colour
        small = hub.latest_scaled("a", width=160)[1]
        drawn = ops.overlay_draw_reference(torch.from_numpy(oracle.clahe(small, 32, 48, 256)), BOX).numpy()
        assert hub.latest_jpeg("a", quality=80, width=160, overlay=BOX, enhance={"tile": 32})[1] == native.jpeg_encode_cpu(drawn, 80)
        drawn = ops.overlay_draw_reference(torch.from_numpy(want), BOX).numpy()
        assert hub.latest_jpeg("a", quality=80, overlay=BOX, enhance=True)[1] == native.jpeg_encode_cpu(drawn, 80)
        assert hub.enhance_count() == 4
        for bad in ({"tile": 36}, {"clip": 0.5}, {"strength": 1.5}, {"gamma": 2}, "clahe", {"tile": True}):
            with pytest.raises(ValueError):
                hub.latest_jpeg("a", enhance=bad)
        with pytest.raises(NotImplementedError, match="gpu.isolation: process"):
            ProcessHub.latest_jpeg(object(), "a", enhance=True)
    finally:
        hub.shutdown()


def test_rest_enhanced_frames(native, farm, tmp_path):
    app = _app(tmp_path, **{"buffer.in_memory": 64})
    try:
        rest = _rest(app)
        url = f"rtsp://127.0.0.1:{farm.port}/cam"
        assert rest.post("/api/v1/process", json={"name": "yard", "rtsp_endpoint": url}).status_code == 200
        _first_frame(app.hub, "yard")

        def served(query):
            r = rest.get(f"/api/v1/process/yard/frame.jpg?quality=80{query}")
            assert r.status_code == 200 and r.headers["content-type"] == "image/jpeg", (query, r.text)
            seq = int(r.headers["X-Vep-Seq"])
            return r.content, {int(m["seq"]): f for m, f in app.hub.history("yard", 0, 0)}[seq]

        jpg, frame = served("")  # without the parameters: byte for byte what it was
        assert jpg == native.jpeg_encode_cpu(frame, 80)
        jpg, frame = served("&enhance=clahe")
        assert jpg == native.jpeg_encode_cpu(oracle.clahe(frame), 80)
        jpg, frame = served("&enhance=clahe&clip=4&tile=64&strength=0.5")
        assert jpg == native.jpeg_encode_cpu(oracle.clahe(frame, 64, 64, 128), 80)
        r = rest.get("/api/v1/process/yard/stream.mjpg?frames=1&width=160&enhance=clahe")
        assert r.status_code == 200 and b"image/jpeg" in r.content
        for q in ("enhance=gamma", "clip=2", "enhance=clahe&clip=0.5", "enhance=clahe&tile=36", "enhance=clahe&strength=2"):
            assert rest.get(f"/api/v1/process/yard/frame.jpg?{q}").status_code == 422, q
            assert rest.get(f"/api/v1/process/yard/stream.mjpg?frames=1&{q}").status_code == 422, q
        assert _metric(rest.get("/metrics").text, "vep_enhance_requests_total") == app.hub.enhance_count() >= 3
        from video_edge_ai_proxy_amd import cli

        a = cli.build_parser().parse_args(["frame", "--device", "yard", "--rest", "h:1", "--enhance", "--clip", "3.5", "--out", "x.jpg"])
        assert cli.frame_jpg_url(a) == "http://h:1/api/v1/process/yard/frame.jpg?enhance=clahe&clip=3.5"
    finally:
        app.stop()
