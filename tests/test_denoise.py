"""Temporal denoise (csrc/vep/denoise.h, docs/DENOISE.md) without a GPU: the CPU twin against the
numpy oracle on an input that exercises every weight class, the closed forms, and the serving
reads through Worker, Hub and REST on the CPU backend."""
import numpy as np
import pytest

import clahe_oracle
import denoise_oracle as oracle
from test_clahe import BOX
from test_crop import _NoSession, _app, _camera, _first_frame, _metric, _rest, _slots, farm  # noqa: F401

DN = (4, 8, 256)  # frames, level, strength as the native layer takes them


def ramped(w, h, k, level, seed=1):
    """k frames, newest first: a base picture plus per-frame uniform noise whose amplitude ramps
    from 0 at the left edge to 8 * level at the right."""
    rng = np.random.default_rng(seed)
    base = rng.integers(96, 160, (h, w, 3))
    amp = (8 * level * np.arange(w) / max(1, w - 1))[None, None, :, None]
    return np.clip(base[None] + np.rint(rng.uniform(-1, 1, (k, h, w, 3)) * amp), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("level", [1, 8, 24])
@pytest.mark.parametrize("size", [(65, 33), (129, 17), (64, 16), (9, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_twin_equals_oracle(native, size, level):
    frames = ramped(*size, 4, level)
    want, weights = oracle.denoise(frames, level, 256)
    # the input is conditioned on the oracle alone: cut, partial and full weights, a fifth each at least
    w = weights[1:]
    shares = [float(np.mean(c)) for c in (w == 0, (w > 0) & (w < 16), w == 16)]
    assert min(shares) >= 0.2, shares
    assert np.array_equal(native.denoise_cpu(frames, level, 256), want)
    assert np.array_equal(native.denoise_cpu(frames, level, 100), oracle.denoise(frames, level, 100)[0])
    assert np.array_equal(native.denoise_cpu(frames[:2], level), oracle.denoise(frames[:2], level)[0])


def test_closed_forms(native):
    frames = ramped(70, 40, 5, 8, seed=3)
    new = frames[0]
    assert np.array_equal(native.denoise_cpu(frames[:1], 8, 256), new)  # K = 1
    assert np.array_equal(native.denoise_cpu(frames, 8, 0), new)  # S = 0
    for s in (256, 77):  # K identical frames
        assert np.array_equal(native.denoise_cpu(np.stack([new] * 8), 1, s), new)
    # an earlier frame whose luma differs by more than 2 T everywhere contributes nothing
    far = np.stack([new, np.clip(new.astype(int) + 17, 0, 255).astype(np.uint8), new[::-1, ::-1]])
    assert np.abs(oracle.luma(far[0]) - oracle.luma(far[1])).min() > 16
    assert np.array_equal(native.denoise_cpu(far, 8), native.denoise_cpu(far[[0, 2]], 8))
    # two one-colour frames with |Y_a - Y_b| <= T: the rounded mean of the two colours
    a, b = np.full((9, 11, 3), (10, 100, 201), np.uint8), np.full((9, 11, 3), (13, 107, 196), np.uint8)
    assert abs(int(oracle.luma(a)[0, 0]) - int(oracle.luma(b)[0, 0])) <= 8
    assert np.array_equal(native.denoise_cpu(np.stack([a, b]), 8)[0, 0], [12, 104, 199])
    # every output channel lies between the minimum and maximum of that channel over the frames
    out = native.denoise_cpu(frames, 24, 200)
    assert np.all(out >= frames.min(0)) and np.all(out <= frames.max(0))
    for bad in ((0, 256), (65, 256), (8, 257), (8, -1)):
        with pytest.raises(ValueError):
            native.denoise_cpu(frames, *bad)


def newest_first(wk, cam, n):
    return np.stack([f for _, f in wk.read_history(cam, 0, n)][::-1])


def test_worker_denoised_reads(native):
    from video_edge_ai_proxy_amd import privacy

    wk, cam, step = _camera(native, history=4)
    assert wk.read_latest_denoised(cam, 0, 0, 0, *DN) is None
    for _ in range(3):
        assert step()
    frames = newest_first(wk, cam, 4)
    want = oracle.denoise(frames, 8, 256)[0]
    assert len(frames) == 3 and not np.array_equal(want, frames[0])
    m, got = wk.read_latest_denoised(cam, 0, 0, 0, *DN)  # fewer frames than asked for: fewer are used
    assert (m["seq"], m["denoise_frames"]) == (3, 3) and np.array_equal(got, want)
    m, got = wk.read_latest_denoised(cam, 0, 0, 0, 2, 20, 128)
    assert m["denoise_frames"] == 2 and np.array_equal(got, oracle.denoise(frames[:2], 20, 128)[0])
    assert wk.read_latest_denoised(cam, 3, 0, 0, *DN) is None  # after: only a newer frame answers
    m, jpg = wk.read_latest_jpeg(cam, 0, 80, 0, 0, None, DN)
    assert m["denoise_frames"] == 3 and jpg == native.jpeg_encode_cpu(want, 80)
    # without the parameter: the bytes and the meta of before
    m, jpg = wk.read_latest_jpeg(cam, 0, 80)
    assert jpg == native.jpeg_encode_cpu(frames[0], 80) and "denoise_frames" not in m
    # denoised BEFORE the scale
    small = wk.read_latest_scaled(cam, 0, 150, 0)[1]
    m, got = wk.read_latest_scaled(cam, 0, 150, 0, DN)
    assert np.array_equal(got, native.resize_area_cpu(want, *small.shape[1::-1])) and m["width"] == small.shape[1]
    assert wk.denoise_count() == 4
    for bad in ((1, 8, 256), (9, 8, 256), (4, 0, 256), (4, 65, 256), (4, 8, 257)):
        with pytest.raises(ValueError):
            wk.read_latest_jpeg(cam, 0, 80, 0, 0, None, bad)
        with pytest.raises(ValueError):
            wk.read_latest_denoised(cam, 0, 0, 0, *bad)
    # A privacy-mask change leaves no earlier frame readable (docs/PRIVACY.md: fail closed): nothing
    # until the next frame, which is then served alone and masked, never blended with unmasked ones.
    wk.set_privacy_masks(cam, privacy.to_native([{"x0": 5000, "y0": 6000, "x1": 10000, "y1": 10000, "mode": "fill",
                                                  "b": 9, "g": 99, "r": 199}]))
    assert wk.read_latest_denoised(cam, 0, 0, 0, *DN) is None
    assert step()
    m, got = wk.read_latest_denoised(cam, 0, 0, 0, *DN)
    assert m["denoise_frames"] == 1 and np.array_equal(got, wk.read_latest(cam, 0)[1]) and list(got[-1, -1]) == [9, 99, 199]
    assert step() and wk.read_latest_jpeg(cam, 0, 80, 0, 0, None, DN)[0]["denoise_frames"] == 2
    # a ring without history refuses: it must not serve the plain frame as if it were denoised
    wk, cam, step = _camera(native)
    assert step()
    with pytest.raises(ValueError, match="buffer.in_memory"):
        wk.read_latest_jpeg(cam, 0, 80, 0, 0, None, DN)
    with pytest.raises(ValueError, match="buffer.in_memory"):
        wk.read_latest_denoised(cam, 0, 0, 0, *DN)


def test_hub_denoised_reads(native, tmp_path):
    import torch

    from conftest import synth
    from video_edge_ai_proxy_amd import ops
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub
    from video_edge_ai_proxy_amd.engine.isolated import ProcessHub

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    cfg.denoise.frames, cfg.denoise.level = 3, 6
    hub = Hub(cfg, devices=[-1])
    try:
        wk = hub.workers[0]
        cam = wk.add_camera("a", _slots(native, 4), 4)
        hub.cameras["a"] = CameraHandle("a", 0, cam, "", session=_NoSession())
        enc = synth(native, 320, 240, gop=6, motion=0.2, seed=2)
        for _ in range(4):
            assert wk.decode_now(cam, enc.next())
        frames = newest_first(wk, cam, 4)
        want = oracle.denoise(frames[:3], 6, 256)[0]  # the hub's defaults
        assert hub.latest_jpeg("a", quality=80)[1] == native.jpeg_encode_cpu(frames[0], 80)
        m, jpg = hub.latest_jpeg("a", quality=80, denoise=True)
        assert m["denoise_frames"] == 3 and jpg == native.jpeg_encode_cpu(want, 80)
        seq, got = hub.latest_denoised("a", frames=4, strength=0.5)
        assert seq == 4 and np.array_equal(got, oracle.denoise(frames, 6, 128)[0])
        assert np.array_equal(ops.denoise(torch.from_numpy(frames), 6, 0.5).numpy(), got)  # host tensors: the twin
        # denoised, scaled, enhanced, THEN drawn on
        small = native.resize_area_cpu(want, *hub.latest_scaled("a", width=160)[1].shape[1::-1])
        drawn = ops.overlay_draw_reference(torch.from_numpy(clahe_oracle.clahe(small, 32, 32, 256)), BOX).numpy()
        assert hub.latest_jpeg("a", quality=80, width=160, overlay=BOX, enhance={"tile": 32}, denoise=True)[1] == \
            native.jpeg_encode_cpu(drawn, 80)
        assert hub.latest_jpeg("a", quality=80, enhance=True, denoise={"level": 6})[1] == \
            native.jpeg_encode_cpu(clahe_oracle.clahe(want), 80)
        assert hub.denoise_count() == 4 and hub.enhance_count() == 2
        for bad in ({"frames": 1}, {"frames": 9}, {"level": 0}, {"level": 2.5}, {"strength": 1.5}, {"clip": 2}, "1", {"frames": True}):
            with pytest.raises(ValueError):
                hub.latest_jpeg("a", denoise=bad)
        with pytest.raises(NotImplementedError, match="gpu.isolation: process"):
            ProcessHub.latest_jpeg(object(), "a", denoise=True)
    finally:
        hub.shutdown()


def test_rest_denoised_frames(native, farm, tmp_path):
    url = f"rtsp://127.0.0.1:{farm.port}/cam"
    app = _app(tmp_path, **{"buffer.in_memory": 64})
    try:
        rest = _rest(app)
        assert rest.post("/api/v1/process", json={"name": "yard", "rtsp_endpoint": url}).status_code == 200
        _first_frame(app.hub, "yard")
        app.hub.wait_frame("yard", 3, 5000)

        def served(query):
            r = rest.get(f"/api/v1/process/yard/frame.jpg?quality=80{query}")
            assert r.status_code == 200 and r.headers["content-type"] == "image/jpeg", (query, r.text)
            seq, used = int(r.headers["X-Vep-Seq"]), int(r.headers.get("X-Vep-Denoise-Frames", 0))
            hist = {int(m["seq"]): f for m, f in app.hub.history("yard", 0, 0)}
            return r.content, np.stack([hist[seq - k] for k in range(max(1, used))]), used

        jpg, frames, used = served("")  # without the parameters: byte for byte what it was
        assert used == 0 and jpg == native.jpeg_encode_cpu(frames[0], 80)
        jpg, frames, used = served("&denoise=1")
        assert used == 4 and jpg == native.jpeg_encode_cpu(oracle.denoise(frames, 8, 256)[0], 80)
        jpg, frames, used = served("&denoise=1&nr_frames=2&nr_level=12&nr_strength=0.5")
        assert used == 2 and jpg == native.jpeg_encode_cpu(oracle.denoise(frames, 12, 128)[0], 80)
        jpg, frames, used = served("&denoise=1&enhance=clahe")
        assert jpg == native.jpeg_encode_cpu(clahe_oracle.clahe(oracle.denoise(frames, 8, 256)[0]), 80)
        assert served("&denoise=1&width=160&enhance=clahe&overlay=1&stamp=1")[2] == 4
        r = rest.get("/api/v1/process/yard/stream.mjpg?frames=1&width=160&denoise=1")
        assert r.status_code == 200 and b"image/jpeg" in r.content and b"X-Vep-Denoise-Frames: " in r.content
        for q in ("nr_frames=3", "nr_level=8", "nr_strength=1", "denoise=0&nr_level=8", "denoise=2", "denoise=1&nr_frames=1",
                  "denoise=1&nr_frames=9", "denoise=1&nr_level=0", "denoise=1&nr_level=65", "denoise=1&nr_strength=2",
                  "enhance=gamma", "clip=2"):
            assert rest.get(f"/api/v1/process/yard/frame.jpg?{q}").status_code == 422, q
            assert rest.get(f"/api/v1/process/yard/stream.mjpg?frames=1&{q}").status_code == 422, q
        assert _metric(rest.get("/metrics").text, "vep_denoise_requests_total") == app.hub.denoise_count() >= 5
        from video_edge_ai_proxy_amd import cli

        a = cli.build_parser().parse_args(["frame", "--device", "yard", "--rest", "h:1", "--denoise", "--nr-level", "12", "--out", "x.jpg"])
        assert cli.frame_jpg_url(a) == "http://h:1/api/v1/process/yard/frame.jpg?denoise=1&nr_level=12"
    finally:
        app.stop()
    app = _app(tmp_path / "plain")  # buffer.in_memory 1: no history to denoise from
    try:
        rest = _rest(app)
        assert rest.post("/api/v1/process", json={"name": "yard", "rtsp_endpoint": url}).status_code == 200
        _first_frame(app.hub, "yard")
        for path in ("frame.jpg?denoise=1", "stream.mjpg?frames=1&denoise=1"):
            r = rest.get(f"/api/v1/process/yard/{path}")
            assert r.status_code == 422 and "buffer.in_memory" in r.text, (path, r.text)
        assert rest.get("/api/v1/process/yard/frame.jpg").status_code == 200
    finally:
        app.stop()
