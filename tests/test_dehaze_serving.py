"""Dehazed frames through Worker, Hub and REST on the CPU backend (docs/DEHAZE.md): the place in the
chain (denoise, scale, dehaze, CLAHE, overlay) by composing the twins, the bytes without the
parameter, the refusals, the header and the metric."""
import numpy as np
import pytest
import torch

import clahe_oracle
import denoise_oracle
from test_clahe import BOX
from test_crop import _NoSession, _app, _first_frame, _metric, _rest, _slots, farm  # noqa: F401

DH = (15, 243, 102, 8, 256)  # patch, omega, t0, radius, strength as the native layer takes them


def test_hub_dehazed_reads_and_the_chain_order(native, tmp_path):
    from conftest import synth
    from video_edge_ai_proxy_amd import ops
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub
    from video_edge_ai_proxy_amd.engine.isolated import ProcessHub

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    cfg.dehaze.patch = 7
    hub = Hub(cfg, devices=[-1])
    try:
        wk = hub.workers[0]
        cam = wk.add_camera("a", _slots(native, 4), 4)
        hub.cameras["a"] = CameraHandle("a", 0, cam, "", session=_NoSession())
        enc = synth(native, 320, 240, gop=6, motion=0.2, seed=2)
        for _ in range(3):
            assert wk.decode_now(cam, enc.next())
        frames = np.stack([f for _, f in wk.read_history(cam, 0, 4)][::-1])
        plain = hub.latest_jpeg("a", quality=80)
        assert plain[1] == native.jpeg_encode_cpu(frames[0], 80) and "dehaze_air" not in plain[0]  # the bytes of before
        want, words = native.dehaze_cpu(frames[0], 7, *DH[1:])  # the hub's defaults
        m, jpg = hub.latest_jpeg("a", quality=80, dehaze=True)
        assert jpg == native.jpeg_encode_cpu(want, 80) != plain[1] and m["dehaze_air"] == tuple(words[1024:1027])
        seq, got = hub.latest_dehazed("a", patch=15, strength=0.5)
        assert seq == 3 and np.array_equal(got, native.dehaze_cpu(frames[0], 15, 243, 102, 8, 128)[0])
        assert np.array_equal(ops.dehaze(torch.from_numpy(frames[0]), strength=0.5).numpy(), got)  # host tensors: the twin
        # denoised, scaled, dehazed, enhanced, THEN drawn on
        small = native.resize_area_cpu(denoise_oracle.denoise(frames, 8, 256)[0], *hub.latest_scaled("a", width=160)[1].shape[1::-1])
        clear = native.dehaze_cpu(small, 7, *DH[1:])[0]
        drawn = ops.overlay_draw_reference(torch.from_numpy(clahe_oracle.clahe(clear, 32, 32, 256)), BOX).numpy()
        assert hub.latest_jpeg("a", quality=80, width=160, overlay=BOX, enhance={"tile": 32}, denoise=True, dehaze=True)[1] == \
            native.jpeg_encode_cpu(drawn, 80)
        assert hub.latest_jpeg("a", quality=80, width=160, dehaze=True)[1] == \
            native.jpeg_encode_cpu(native.dehaze_cpu(native.resize_area_cpu(frames[0], *small.shape[1::-1]), 7, *DH[1:])[0], 80)
        assert hub.dehaze_count() == 4 and np.array_equal(wk.read_latest(cam, 0)[1], frames[0])  # the slot is not written
        for bad in ({"patch": 4}, {"patch": 33}, {"omega": 1.5}, {"t0": 0.01}, {"radius": 17}, {"strength": 2}, {"tile": 32}, "1"):
            with pytest.raises(ValueError):
                hub.latest_jpeg("a", dehaze=bad)
        with pytest.raises(ValueError, match="at least 16"):
            hub.latest_jpeg("a", width=12, dehaze=True)
        with pytest.raises(NotImplementedError, match="gpu.isolation: process"):
            ProcessHub.latest_jpeg(object(), "a", dehaze=True)
    finally:
        hub.shutdown()


def test_rest_dehazed_frames(native, farm, tmp_path):
    url = f"rtsp://127.0.0.1:{farm.port}/cam"
    app = _app(tmp_path, **{"buffer.in_memory": 64})
    try:
        rest = _rest(app)
        assert rest.post("/api/v1/process", json={"name": "yard", "rtsp_endpoint": url}).status_code == 200
        _first_frame(app.hub, "yard")

        def served(query):
            r = rest.get(f"/api/v1/process/yard/frame.jpg?quality=80{query}")
            assert r.status_code == 200 and r.headers["content-type"] == "image/jpeg", (query, r.text)
            hist = {int(m["seq"]): f for m, f in app.hub.history("yard", 0, 0)}
            return r.content, hist[int(r.headers["X-Vep-Seq"])], r.headers.get("X-Vep-Dehaze-Air")

        jpg, frame, air = served("")  # without the parameters: byte for byte what it was
        assert air is None and jpg == native.jpeg_encode_cpu(frame, 80)
        jpg, frame, air = served("&dehaze=1")
        want, words = native.dehaze_cpu(frame, *DH)
        assert jpg == native.jpeg_encode_cpu(want, 80) and air == ",".join(str(v) for v in words[1024:1027])
        jpg, frame, air = served("&dehaze=1&dh_patch=7&dh_omega=0.5&dh_t0=0.2&dh_radius=3&dh_strength=0.5&enhance=clahe")
        assert jpg == native.jpeg_encode_cpu(clahe_oracle.clahe(native.dehaze_cpu(frame, 7, 128, 205, 3, 128)[0]), 80)
        r = rest.get("/api/v1/process/yard/stream.mjpg?frames=1&width=160&dehaze=1")
        assert r.status_code == 200 and b"image/jpeg" in r.content and b"X-Vep-Dehaze-Air: " in r.content
        for q in ("dh_patch=15", "dh_omega=0.9", "dh_t0=0.1", "dh_radius=8", "dh_strength=1", "dehaze=0&dh_patch=15", "dehaze=2",
                  "dehaze=1&dh_patch=4", "dehaze=1&dh_patch=33", "dehaze=1&dh_omega=1.1", "dehaze=1&dh_t0=0.04",
                  "dehaze=1&dh_radius=0", "dehaze=1&dh_strength=2"):
            assert rest.get(f"/api/v1/process/yard/frame.jpg?{q}").status_code == 422, q
            assert rest.get(f"/api/v1/process/yard/stream.mjpg?frames=1&{q}").status_code == 422, q
        assert rest.get("/api/v1/process/yard/frame.jpg?nr_level=8").status_code == 422  # (as before)
        assert _metric(rest.get("/metrics").text, "vep_dehaze_requests_total") == app.hub.dehaze_count() >= 3
        # gpu.isolation: process: a hub without the dehaze face answers 501
        hub, app.pm.hub = app.pm.hub, type("Isolated", (), {"touch": lambda self, name: None})()
        try:
            assert rest.get("/api/v1/process/yard/frame.jpg?dehaze=1").status_code == 501
            assert rest.get("/api/v1/process/yard/stream.mjpg?frames=1&dehaze=1").status_code == 501
        finally:
            app.pm.hub = hub
        from video_edge_ai_proxy_amd import cli

        a = cli.build_parser().parse_args(["frame", "--device", "yard", "--rest", "h:1", "--dehaze", "--dh-patch", "7", "--out", "x.jpg"])
        assert cli.frame_jpg_url(a) == "http://h:1/api/v1/process/yard/frame.jpg?dehaze=1&dh_patch=7"
    finally:
        app.stop()
