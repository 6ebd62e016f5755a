"""The camera wall and scaled frames on the host: composition against the independent oracle
(tests/scale_oracle.py), the CPU-backend Worker and Hub paths against the composition, and the
REST routes. The GPU paths are held to the same CPU functions in tests/test_gpu_wall.py."""
import io
import time

import numpy as np
import pytest

import scale_oracle as so
from conftest import synth


def decode(jpg: bytes):
    from PIL import Image

    img = Image.open(io.BytesIO(jpg))
    img.load()
    return img


# ------------------------------------------------------------------------------ composition

def test_compose_one_tile(native):
    f = so.picture("noise", 64, 48)
    got = native.compose_wall_cpu([f], 0, 16, 9)
    assert got.shape == (9, 16, 3)
    assert np.array_equal(got, so.compose_wall([f], None, 16, 9))
    assert (got[:, :2] == so.BACKGROUND).all() and (got[:, 14:] == so.BACKGROUND).all()  # 4:3 in 16:9: 12 wide


def test_compose_three_tiles_two_columns(native):
    fs = [so.picture(k, 48, 32, seed=i) for i, k in enumerate(["noise", "gradient", "checkerboard"])]
    got = native.compose_wall_cpu(fs, 2, 24, 16)
    assert got.shape == (32, 48, 3)
    assert np.array_equal(got, so.compose_wall(fs, 2, 24, 16))
    assert (got[16:, 24:] == so.BACKGROUND).all()  # the empty cell


def test_compose_mixed_sizes(native):
    # three source sizes, one empty tile, one 4:3 source in a 16:9 cell (bars left and right)
    fs = [so.picture("noise", 64, 36), so.picture("gradient", 200, 120), None, so.picture("noise", 64, 48),
          so.picture("checkerboard", 64, 36, seed=2)]
    tw, th = 31, 18  # 64x48 fits as 24x18: dx = 3, an odd offset; 64x36 as 31x17: one bar row
    got = native.compose_wall_cpu(fs, 0, tw, th)
    cols, rows, cw, ch = so.wall_geometry(5, None, tw, th)
    assert (cols, rows) == (3, 2) and got.shape == (ch, cw, 3)
    assert np.array_equal(got, so.compose_wall(fs, None, tw, th))
    x, y, w, h = so.place(3, cols, tw, th, 64, 48)
    assert (w, h) == (24, 18) and (x, y) == (3, th)  # an odd dx
    cell = got[th:2 * th, 0:tw]  # tile 3 is cell (0, 1)
    assert (cell[:, :3] == so.BACKGROUND).all() and (cell[:, 27:] == so.BACKGROUND).all()
    assert np.array_equal(cell[:, 3:27], so.resize_area(fs[3], 24, 18))
    assert (got[0:th, 2 * tw:3 * tw] == so.BACKGROUND).all()  # the None tile
    assert (got[th:, 2 * tw:] == so.BACKGROUND).all()  # the cell past the last tile


def test_compose_argument_checks(native):
    f = so.picture("noise", 16, 8)
    for args in [([], 0, 8, 8), ([f], 0, 0, 8), ([f], 0, 8, 0), ([f], -1, 8, 8), ([f, f], 1, 8, 40000)]:
        with pytest.raises(Exception):
            native.compose_wall_cpu(*args)


def test_reference_ops(native):
    import torch

    from video_edge_ai_proxy_amd import ops

    f = so.picture("noise", 48, 32)
    t = torch.from_numpy(f)
    assert np.array_equal(ops.resize_area_reference(t, 8, 8).numpy(), so.resize_area(f, 8, 8))
    got = ops.compose_wall_reference([t, None, t], 2, 16, 9)
    assert np.array_equal(got.numpy(), so.compose_wall([f, None, f], 2, 16, 9))
    with pytest.raises(ValueError):
        ops.resize_area_reference(t, 49, 8)  # larger than the source
    with pytest.raises(ValueError):
        ops.resize_area_reference(t, 0, 8)
    with pytest.raises(TypeError):
        ops.resize_area_reference(t.float(), 8, 8)
    with pytest.raises(ValueError):
        ops.resize_area_reference(t[:, ::2], 8, 8)  # not contiguous
    with pytest.raises(ValueError):
        ops.compose_wall_reference([], 2, 16, 9)
    with pytest.raises(ValueError):
        ops.compose_wall_reference([t], 2, 0, 9)


# ------------------------------------------------------------------------ CPU-backend Worker

def _feed(native, wk, name, w, h, frames=2, seed_gop=6):
    enc = synth(native, w, h, gop=seed_gop)
    cam = wk.add_camera(name, 2)
    for _ in range(frames):
        assert wk.decode_now(cam, enc.next())
    return cam


def test_worker_scaled_jpeg_cpu_backend(native):
    wk = native.Worker(device=-1)
    cam = _feed(native, wk, "c", 320, 240)
    meta, frame = wk.read_latest(cam, 0)
    jmeta, jpg = wk.read_latest_jpeg(cam, 0, 70, 160, 0)
    assert jmeta["seq"] == meta["seq"] and (jmeta["width"], jmeta["height"]) == (160, 120)
    assert jpg == native.jpeg_encode_cpu(native.resize_area_cpu(frame, 160, 120), 70)
    assert decode(jpg).size == (160, 120)
    # the three-argument call is what it was; a box that holds the frame changes nothing either
    assert wk.read_latest_jpeg(cam, 0, 70)[1] == native.jpeg_encode_cpu(frame, 70)
    assert wk.read_latest_jpeg(cam, 0, 70, 4000, 4000)[1] == native.jpeg_encode_cpu(frame, 70)
    assert wk.read_latest_jpeg(cam, meta["seq"], 70, 160, 0) is None  # nothing newer
    smeta, small = wk.read_latest_scaled(cam, 0, 0, 60)
    assert (smeta["width"], smeta["height"]) == (80, 60) and smeta["seq"] == meta["seq"]
    assert np.array_equal(small, native.resize_area_cpu(frame, 80, 60))
    for w, h in [(-1, 0), (0, 65536), (70000, 10)]:
        with pytest.raises(Exception):
            wk.read_latest_jpeg(cam, 0, 70, w, h)
    with pytest.raises(Exception):
        wk.read_latest_scaled(cam, 0, 0, 0)


def test_worker_wall_cpu_backend(native):
    wk = native.Worker(device=-1)
    a = _feed(native, wk, "a", 320, 240)
    b = _feed(native, wk, "b", 160, 96, frames=3)
    empty = wk.add_camera("e", 2)
    fa, fb = wk.read_latest(a, 0), wk.read_latest(b, 0)
    seqs, jpg = wk.read_wall_jpeg([a, b, empty], 0, 64, 36, 70)
    assert list(seqs) == [fa[0]["seq"], fb[0]["seq"], 0]
    assert jpg == native.jpeg_encode_cpu(native.compose_wall_cpu([fa[1], fb[1], None], 0, 64, 36), 70)
    assert decode(jpg).size == (128, 72)
    # a foreign tile (a camera of another worker, scaled there) lands where the camera would
    small = native.resize_area_cpu(fa[1], 48, 36)
    seqs2, jpg2 = wk.read_wall_jpeg([-1, b, empty], 0, 64, 36, 70, [(7, small), None, None])
    assert list(seqs2) == [7, fb[0]["seq"], 0] and jpg2 == jpg
    assert wk.wall_max_tiles == 64
    wk.wall_max_tiles = 2
    with pytest.raises(Exception):
        wk.read_wall_jpeg([a, b, empty], 0, 64, 36, 70)
    wk.wall_max_tiles = 64
    for args in [([], 0, 64, 36, 70), ([a], 0, 0, 36, 70), ([a], 0, 64, 65536, 70), ([a], 0, 64, 36, 0),
                 ([a, b], 1, 64, 40000, 70), ([a], 0, 64, 36, 70, [(1, so.picture("noise", 65, 36))])]:
        with pytest.raises(Exception):
            wk.read_wall_jpeg(*args)


# ----------------------------------------------------------------------------------- Hub

class _NoSession:
    def stop(self):
        pass


def test_hub_wall_across_two_workers(native, tmp_path):
    """Two CPU workers: the wall is rendered by one, the other's cameras arrive as scaled tiles
    (the cross-GPU path), and the bytes are those of the single-canvas composition."""
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, CameraNotFound, Hub

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    cfg.serving.wall_tile = "64x36"
    hub = Hub(cfg, devices=[-1, -1])
    try:
        frames = {}
        for k, (name, w, h) in enumerate([("cam_a", 320, 240), ("cam_b", 160, 96), ("cam_c", 320, 176)]):
            wi = k % 2  # cameras on both workers: a and c on worker 0, b on worker 1
            cam = _feed(native, hub.workers[wi], name, w, h)
            hub.cameras[name] = CameraHandle(name, wi, cam, "", session=_NoSession())
            frames[name] = hub.workers[wi].read_latest(cam, 0)
        assert {h.worker_index for h in hub.cameras.values()} == {0, 1}
        seqs, jpg = hub.wall_jpeg(quality=70)
        order = ["cam_a", "cam_b", "cam_c"]
        assert seqs == {n: frames[n][0]["seq"] for n in order}
        want = native.jpeg_encode_cpu(native.compose_wall_cpu([frames[n][1] for n in order], 0, 64, 36), 70)
        assert jpg == want
        # another order, columns and tile size; the majority worker changes with the list
        seqs, jpg = hub.wall_jpeg(["cam_b", "cam_a"], cols=1, tile_width=40, tile_height=30, quality=70)
        assert list(seqs) == ["cam_b", "cam_a"]
        assert jpg == native.jpeg_encode_cpu(
            native.compose_wall_cpu([frames["cam_b"][1], frames["cam_a"][1]], 1, 40, 30), 70)
        # scaled single frames
        meta, small = hub.latest_scaled("cam_a", 0, width=160)
        assert np.array_equal(small, native.resize_area_cpu(frames["cam_a"][1], 160, 120))
        meta, sj = hub.latest_jpeg("cam_a", 0, 70, width=160)
        assert sj == native.jpeg_encode_cpu(small, 70)
        assert hub.latest_jpeg("cam_a", 0, 70)[1] == native.jpeg_encode_cpu(frames["cam_a"][1], 70)
        with pytest.raises(CameraNotFound):
            hub.wall_jpeg(["cam_a", "nope"])
        for bad in [dict(tile_width=0), dict(tile_height=65536), dict(cols=0), dict(quality=0)]:
            with pytest.raises(ValueError):
                hub.wall_jpeg(**bad)
        with pytest.raises(ValueError):
            hub.latest_jpeg("cam_a", 0, 70, width=0)
        cfg.serving.wall_max_tiles = 2
        with pytest.raises(ValueError):
            hub.wall_jpeg()
    finally:
        hub.shutdown()


def test_process_hub_refuses_wall():
    from video_edge_ai_proxy_amd.engine.child import EXPORTED
    from video_edge_ai_proxy_amd.engine.isolated import ProcessHub

    assert "latest_scaled" in EXPORTED and "latest_jpeg" in EXPORTED
    with pytest.raises(NotImplementedError, match="gpu.isolation: process"):
        ProcessHub.wall_jpeg(object())


# ------------------------------------------------------------------------ REST, config

@pytest.fixture
def farm(native):
    srv = native.RtspServer("127.0.0.1", 0)
    for path, (w, h, seed) in {"/cam": (320, 240, 11), "/wide": (320, 176, 12)}.items():
        cfg = native.SynthConfig()
        cfg.width, cfg.height, cfg.gop, cfg.fps, cfg.seed = w, h, 10, 30, seed
        srv.add_stream(path, cfg, realtime=True, cached_frames=20)
    srv.start()
    yield srv
    srv.stop()


@pytest.fixture
def hubapp(tmp_path, native):
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.server.app import build_app

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    cfg.gpu.devices = [-1]
    app = build_app(cfg, host="127.0.0.1", rest_port=0, grpc_port=0)
    yield app
    app.stop()


def _rest(app):
    from fastapi.testclient import TestClient

    from video_edge_ai_proxy_amd.server.rest import create_app

    return TestClient(create_app(app.pm, app.settings, app.metrics))


def _start_camera(rest, farm, name="front_door", path="/cam"):
    url = f"rtsp://127.0.0.1:{farm.port}{path}"
    assert rest.post("/api/v1/process", json={"name": name, "rtsp_endpoint": url}).status_code == 200
    deadline = time.time() + 15
    while time.time() < deadline:  # the first request wakes the lazy decoder
        r = rest.get(f"/api/v1/process/{name}/frame.jpg")
        if r.status_code == 200:
            return r
        assert r.status_code == 404
        time.sleep(0.05)
    raise AssertionError("no frame within 15 s")


def test_rest_scaled_frame(native, farm, hubapp):
    rest = _rest(hubapp)
    full = _start_camera(rest, farm)
    assert decode(full.content).size == (320, 240)
    r = rest.get("/api/v1/process/front_door/frame.jpg?width=160")
    assert r.status_code == 200 and int(r.headers["x-vep-seq"]) >= 1
    assert decode(r.content).size == (160, 120)
    assert decode(rest.get("/api/v1/process/front_door/frame.jpg?height=60").content).size == (80, 60)
    assert decode(rest.get("/api/v1/process/front_door/frame.jpg?width=100&height=100").content).size == (100, 75)
    assert decode(rest.get("/api/v1/process/front_door/frame.jpg?width=4000").content).size == (320, 240)  # never up
    for bad in ("width=0", "height=0", "width=65536", "width=-4", "width=10&height=70000"):
        assert rest.get(f"/api/v1/process/front_door/frame.jpg?{bad}").status_code == 400
        assert rest.get(f"/api/v1/process/front_door/stream.mjpg?frames=1&{bad}").status_code == 400
    assert rest.get("/api/v1/process/nope/frame.jpg?width=160").status_code == 404
    s = rest.get("/api/v1/process/front_door/stream.mjpg?frames=2&fps=30&width=160")
    assert s.status_code == 200
    boundary = s.headers["content-type"].split("boundary=")[1].encode()
    parts = s.content.split(b"--" + boundary + b"\r\n")[1:]
    assert len(parts) == 2
    for p in parts:
        head, _, body = p.partition(b"\r\n\r\n")
        hdr = dict(line.split(": ") for line in head.decode().split("\r\n"))
        assert decode(body[:int(hdr["Content-Length"])]).size == (160, 120)


def test_rest_wall(native, farm, hubapp):
    rest = _rest(hubapp)
    assert rest.get("/api/v1/wall.jpg").status_code == 404  # no camera running
    assert rest.get("/api/v1/wall").status_code == 404
    _start_camera(rest, farm, "front_door", "/cam")
    _start_camera(rest, farm, "back_yard", "/wide")
    _start_camera(rest, farm, "side_gate", "/cam")
    r = rest.get("/api/v1/wall.jpg")
    assert r.status_code == 200 and r.headers["content-type"] == "image/jpeg"
    assert decode(r.content).size == (2 * 320, 2 * 180)  # three tiles: 2 x 2 cells of serving.wall_tile
    shown = [e.split(":") for e in r.headers["x-vep-wall"].split(",")]
    assert [n for n, _ in shown] == ["back_yard", "front_door", "side_gate"] and all(int(s) >= 1 for _, s in shown)
    geo = rest.get("/api/v1/wall").json()
    assert (geo["cols"], geo["rows"], geo["tile"]) == (2, 2, [320, 180])
    assert [t["name"] for t in geo["tiles"]] == [n for n, _ in shown]  # tile order matches the header
    assert [(t["x"], t["y"], t["w"], t["h"]) for t in geo["tiles"]] == [(0, 0, 320, 180), (320, 0, 320, 180),
                                                                      (0, 180, 320, 180)]
    assert all(t["seq"] >= 1 for t in geo["tiles"])
    # named cameras in their own order, one column, small tiles
    r = rest.get("/api/v1/wall.jpg?names=side_gate,front_door&cols=1&tile=64x36&quality=60")
    assert r.status_code == 200 and decode(r.content).size == (64, 72)
    assert [e.split(":")[0] for e in r.headers["x-vep-wall"].split(",")] == ["side_gate", "front_door"]
    geo = rest.get("/api/v1/wall?names=side_gate,front_door&cols=1&tile=64x36").json()
    assert (geo["cols"], geo["rows"], geo["tile"]) == (1, 2, [64, 36])
    assert rest.get("/api/v1/wall.jpg?names=front_door,nope").status_code == 404
    assert rest.get("/api/v1/wall?names=nope").status_code == 404
    assert rest.get("/api/v1/wall.mjpg?names=nope&frames=1").status_code == 404
    for bad in ("tile=0x10", "tile=64", "tile=64x70000", "cols=0", "quality=0", "quality=101", "names=,"):
        assert rest.get(f"/api/v1/wall.jpg?{bad}").status_code == 400, bad
    assert rest.get("/api/v1/wall.mjpg?frames=0").status_code == 400
    assert rest.get("/api/v1/wall.mjpg?frames=1&fps=0").status_code == 400
    hubapp.hub.cfg.serving.wall_max_tiles = 2
    assert rest.get("/api/v1/wall.jpg").status_code == 400
    hubapp.hub.cfg.serving.wall_max_tiles = 64
    s = rest.get("/api/v1/wall.mjpg?frames=2&fps=30&tile=64x36")
    assert s.status_code == 200
    ctype = s.headers["content-type"]
    assert ctype.startswith("multipart/x-mixed-replace")
    boundary = ctype.split("boundary=")[1].encode()
    parts = s.content.split(b"--" + boundary + b"\r\n")
    assert parts[0] == b"" and len(parts) == 3
    walls = []
    for p in parts[1:]:
        head, _, body = p.partition(b"\r\n\r\n")
        hdr = dict(line.split(": ") for line in head.decode().split("\r\n"))
        jpg = body[:int(hdr["Content-Length"])]
        assert body[len(jpg):] == b"\r\n" and decode(jpg).size == (128, 72)
        walls.append({n: int(q) for n, q in (e.split(":") for e in hdr["X-Vep-Wall"].split(","))})
    assert any(walls[1][n] > walls[0][n] for n in walls[0])  # a part is sent when a tile is newer


def test_rest_wall_not_served_by_isolated_hub(native, hubapp):
    rest = _rest(hubapp)

    def refuse(*a, **k):
        raise NotImplementedError("the camera wall is not served with gpu.isolation: process")

    hubapp.hub.wall_layout = refuse
    try:
        assert rest.get("/api/v1/wall.jpg").status_code == 501
        assert rest.get("/api/v1/wall").status_code == 501
    finally:
        del hubapp.hub.wall_layout


def test_cli_frame_scaled(native, farm, hubapp, tmp_path):
    from video_edge_ai_proxy_amd import cli

    _start_camera(_rest(hubapp), farm)
    out = tmp_path / "small.jpg"
    cli.main(["frame", "--device", "front_door", "--grpc-port", str(hubapp.grpc_port), "--out", str(out),
              "--width", "160"])
    assert decode(out.read_bytes()).size == (160, 120)
    out = tmp_path / "small.ppm"
    cli.main(["frame", "--device", "front_door", "--grpc-port", str(hubapp.grpc_port), "--out", str(out),
              "--height", "60"])
    assert out.read_bytes().startswith(b"P6 80 60 255\n")


def test_config_wall(tmp_path):
    from video_edge_ai_proxy_amd.config import load_config, parse_tile

    cfg = load_config(data_dir=str(tmp_path))
    assert cfg.serving.wall_tile == "320x180" and cfg.serving.wall_max_tiles == 64
    assert parse_tile("320x180") == (320, 180)
    (tmp_path / "conf.yaml").write_text('serving:\n  wall_tile: "160x90"\n  wall_max_tiles: 16\n')
    cfg = load_config(data_dir=str(tmp_path))
    assert parse_tile(cfg.serving.wall_tile) == (160, 90) and cfg.serving.wall_max_tiles == 16
    for bad in ('wall_tile: "0x10"', 'wall_tile: "10x0"', 'wall_tile: "wide"', 'wall_tile: "70000x10"',
                "wall_max_tiles: 0", "wall_max_tiles: 70000"):
        (tmp_path / "conf.yaml").write_text(f"serving:\n  {bad}\n")
        with pytest.raises(ValueError):
            load_config(data_dir=str(tmp_path))
