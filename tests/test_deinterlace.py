"""Deinterlacing (csrc/vep/deinterlace.h, docs/DEINTERLACE.md) without a GPU: the CPU twin against
the numpy oracle on noise, the closed forms, the quality order on a moving bar, and the serving
reads through Worker, Hub and REST on the CPU backend."""
import numpy as np
import pytest

import deinterlace_oracle as oracle
from test_crop import _NoSession, _app, _first_frame, _metric, _rest, _slots, farm  # noqa: F401

SHAPES = [(4, 4), (64, 16), (67, 19), (130, 35), (257, 65)]


def noise(w, h, seed, near=False):
    """A woven pair of random frames; ``near``: the older one within +-12 of the newer, so both
    sides of the clamp and its inside are met."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (h, w, 3))
    g = np.clip(f + rng.integers(-12, 13, (h, w, 3)), 0, 255) if near else rng.integers(0, 256, (h, w, 3))
    return f.astype(np.uint8), g.astype(np.uint8)


@pytest.mark.parametrize("order", ["tff", "bff"])
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_twin_equals_oracle(native, size, order):
    for seed, near in ((1, False), (2, True)):
        f, g = noise(*size, seed, near)
        assert np.array_equal(native.deinterlace_cpu(f, g, order, 1), oracle.deinterlace(f, g, order))
        assert np.array_equal(native.deinterlace_cpu(f, None, order, 1), oracle.deinterlace(f, None, order))
        assert np.array_equal(native.deinterlace_cpu(f, g, order, 0), oracle.deinterlace(f, None, order))


@pytest.mark.parametrize("order", ["tff", "bff"])
def test_closed_forms_and_quality_order(native, order):
    f, g = noise(70, 41, 3)
    p = {"tff": 0, "bff": 1}[order]
    assert np.array_equal(native.deinterlace_cpu(f, f.copy(), order, 1), f)  # a static pair keeps its woven frame
    for older in (g, None):
        assert np.array_equal(native.deinterlace_cpu(f, older, order, 1)[p::2], f[p::2])  # kept rows
    # where F and G agree on rows up, y and dn of a column, the pixel is F's
    g2 = g.copy()
    g2[:, 20:30] = f[:, 20:30]
    assert np.array_equal(native.deinterlace_cpu(f, g2, order, 1)[:, 20:30], f[:, 20:30])
    # moving bar: woven < spatial < motion-adaptive, as measured against the progressive truth
    newer, older, truth = oracle.bar_scene(order=order)
    woven, spatial, full = (oracle.psnr(x, truth) for x in (newer, native.deinterlace_cpu(newer, None, order, 1),
                                                            native.deinterlace_cpu(newer, older, order, 1)))
    assert woven < spatial < full, (woven, spatial, full)
    for bad in ((f[:3], None, order, 1), (np.ascontiguousarray(f[:, :3]), None, order, 1), (f, g[:-1], order, 1), (f, None, "mid", 1), (f, None, order, 2)):
        with pytest.raises(ValueError):
            native.deinterlace_cpu(*bad)


def test_hub_deinterlaced_reads(native, tmp_path):
    import torch

    from conftest import synth
    from video_edge_ai_proxy_amd import ops
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub
    from video_edge_ai_proxy_amd.engine.isolated import ProcessHub

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    cfg.deinterlace.order = "bff"
    hub = Hub(cfg, devices=[-1])
    try:
        wk = hub.workers[0]
        for name, history in (("a", 3), ("b", 0)):  # b: buffer.in_memory 1, no earlier frame to read
            cam = wk.add_camera(name, _slots(native, history), history)
            hub.cameras[name] = CameraHandle(name, 0, cam, "", session=_NoSession())
            enc = synth(native, 320, 240, gop=6, motion=0.2, seed=2)
            assert wk.decode_now(cam, enc.next())
            f0 = wk.read_latest(cam, 0)[1]
            m, jpg = hub.latest_jpeg(name, quality=80, deinterlace=True)  # the first frame: spatial only
            assert m["deinterlace_frames"] == 1 and jpg == native.jpeg_encode_cpu(oracle.deinterlace(f0, None, "bff"), 80)
            assert wk.decode_now(cam, enc.next())
        cam = hub.cameras["a"].cam
        older, newer = (f for _, f in wk.read_history(cam, 0, 2))
        assert not np.array_equal(older, newer)
        want = oracle.deinterlace(newer, older, "bff")
        assert hub.latest_jpeg("a", quality=80)[1] == native.jpeg_encode_cpu(newer, 80)
        m, jpg = hub.latest_jpeg("a", quality=80, deinterlace=True)
        assert (m["seq"], m["deinterlace_frames"]) == (2, 2) and jpg == native.jpeg_encode_cpu(want, 80)
        assert hub.latest_jpeg("a", after=1, quality=80, deinterlace=True)[1] == jpg  # a polling client keeps the earlier frame
        assert hub.latest_jpeg("a", after=2, deinterlace=True) is None
        assert hub.latest_jpeg("b", deinterlace=True)[0]["deinterlace_frames"] == 1
        m, jpg = hub.latest_jpeg("a", quality=80, deinterlace={"order": "tff", "temporal": False})
        assert m["deinterlace_frames"] == 1 and jpg == native.jpeg_encode_cpu(oracle.deinterlace(newer, None, "tff"), 80)
        seq, got = hub.latest_deinterlaced("a", order="tff")
        assert seq == 2 and np.array_equal(got, oracle.deinterlace(newer, older, "tff"))
        assert np.array_equal(ops.deinterlace(torch.from_numpy(newer), torch.from_numpy(older)).numpy(), got)  # host: the twin
        # deinterlaced BEFORE the scale
        small = hub.latest_scaled("a", width=150)[1]
        assert np.array_equal(hub.latest_deinterlaced("a", width=150)[1], native.resize_area_cpu(want, *small.shape[1::-1]))
        assert hub.deinterlace_count() == 8  # (every served read above; the one that found no frame is none)
        for bad in ({"order": "mid"}, {"temporal": 2}, {"frames": 2}, "1"):
            with pytest.raises(ValueError):
                hub.latest_jpeg("a", deinterlace=bad)
        with pytest.raises(ValueError, match="denoise"):
            hub.latest_jpeg("a", deinterlace=True, denoise=True)
        with pytest.raises(ValueError, match="denoise"):
            wk.read_latest_jpeg(cam, 0, 80, 0, 0, None, (4, 8, 256), None, (0, 1))
        with pytest.raises(NotImplementedError, match="gpu.isolation: process"):
            ProcessHub.latest_jpeg(object(), "a", deinterlace=True)
    finally:
        hub.shutdown()


def test_rest_deinterlaced_frames(native, farm, tmp_path):
    url = f"rtsp://127.0.0.1:{farm.port}/cam"
    for memory, frames in ((64, 2), (1, 1)):  # buffer.in_memory 1: the spatial part alone, still served
        app = _app(tmp_path / str(memory), **{"buffer.in_memory": memory})
        try:
            rest = _rest(app)
            assert rest.post("/api/v1/process", json={"name": "yard", "rtsp_endpoint": url}).status_code == 200
            _first_frame(app.hub, "yard")
            app.hub.wait_frame("yard", 2, 5000)
            r = rest.get("/api/v1/process/yard/frame.jpg?quality=80&deinterlace=1&di_order=bff")
            assert r.status_code == 200 and int(r.headers["X-Vep-Deinterlace-Frames"]) == frames, r.text
            if memory > 1:
                hist = {int(m["seq"]): f for m, f in app.hub.history("yard", 0, 0)}
                seq = int(r.headers["X-Vep-Seq"])
                assert r.content == native.jpeg_encode_cpu(oracle.deinterlace(hist[seq], hist[seq - 1], "bff"), 80)
                r = rest.get("/api/v1/process/yard/frame.jpg?quality=80")  # without the parameters: today's bytes
                hist = {int(m["seq"]): f for m, f in app.hub.history("yard", 0, 0)}
                assert "X-Vep-Deinterlace-Frames" not in r.headers
                assert r.content == native.jpeg_encode_cpu(hist[int(r.headers["X-Vep-Seq"])], 80)
            r = rest.get("/api/v1/process/yard/frame.jpg?deinterlace=1&di_temporal=0&width=160&dehaze=1&enhance=clahe&overlay=1&stamp=1")
            assert r.status_code == 200 and r.headers["X-Vep-Deinterlace-Frames"] == "1"
            r = rest.get("/api/v1/process/yard/stream.mjpg?frames=1&width=160&deinterlace=1")
            assert r.status_code == 200 and b"X-Vep-Deinterlace-Frames: " in r.content
            for q in ("di_order=tff", "di_temporal=1", "deinterlace=0&di_order=bff", "deinterlace=2", "deinterlace=1&di_order=mid",
                      "deinterlace=1&di_temporal=2", "deinterlace=1&denoise=1"):
                assert rest.get(f"/api/v1/process/yard/frame.jpg?{q}").status_code == 422, q
                assert rest.get(f"/api/v1/process/yard/stream.mjpg?frames=1&{q}").status_code == 422, q
            assert _metric(rest.get("/metrics").text, "vep_deinterlace_requests_total") == app.hub.deinterlace_count() >= 3
        finally:
            app.stop()
    from video_edge_ai_proxy_amd import cli

    a = cli.build_parser().parse_args(["frame", "--device", "yard", "--rest", "h:1", "--deinterlace", "--di-order", "bff",
                                       "--di-no-temporal", "--out", "x.jpg"])
    assert cli.frame_jpg_url(a) == "http://h:1/api/v1/process/yard/frame.jpg?deinterlace=1&di_order=bff&di_temporal=0"
