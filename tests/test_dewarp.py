"""Views on the CPU: the twin (csrc/vep/dewarp.cpp) against the numpy transcription of the
arithmetic (dewarp_cases.oracle) and closed forms, the meshes of views.py against the float64
closed form of their rays, then the Worker's CPU backend, the Hub, REST and the stored views."""
import math

import numpy as np
import pytest

import dewarp_cases as dc
from conftest import synth
from test_crop import MASKS, _NoSession, _app, _camera, _first_frame, _metric, _rest, farm  # noqa: F401
from video_edge_ai_proxy_amd import privacy, views


@pytest.mark.parametrize("kind", dc.MESHES)
@pytest.mark.parametrize("size", dc.SOURCES)
def test_twin_equals_oracle(native, size, kind):
    w, h = size
    p = dc.picture(w, h, seed=w)
    for ow, oh in dc.OUT_SIZES:
        mesh = dc.mesh_of(kind, w, h, ow, oh)
        got = native.remap_cpu(p, mesh, ow, oh, dc.PAD)
        assert got.shape == (oh, ow, 3) and np.array_equal(got, dc.oracle(p, mesh, ow, oh, dc.PAD)), (ow, oh)
        if kind == "outside":
            assert (got == np.array(dc.PAD, np.uint8)).all()
        if kind == "half_inside":  # column j reads j + w / 2: pad from the picture's middle on
            assert (got[:, (w + 1) // 2:] == np.array(dc.PAD, np.uint8)).all()


@pytest.mark.parametrize("size", dc.SOURCES)
def test_closed_forms(native, size):
    w, h = size
    p = dc.picture(w, h, seed=3)
    q = p.astype(np.int64)
    assert np.array_equal(native.remap_cpu(p, dc.mesh_of("identity", w, h, w, h), w, h), p)
    assert np.array_equal(native.remap_cpu(p, views.identity_mesh(w, h), w, h), p)
    left = np.concatenate([q[:, :1], q[:, :-1]], 1)  # half a pixel to the left, the edge clamped
    assert np.array_equal(native.remap_cpu(p, dc.mesh_of("half", w, h, w, h), w, h), ((q + left + 1) >> 1).astype(np.uint8))
    assert np.array_equal(native.remap_cpu(p, dc.mesh_of("rot90", w, h, h, w), h, w), p.transpose(1, 0, 2)[:, ::-1])


def test_argument_checks(native):
    p = dc.picture(17, 9)
    m = views.identity_mesh(17, 9)
    for args in [(p, m, 33, 9), (p, m, 17, 0), (p, m, 4097, 9), (p, m.astype(np.int64), 17, 9), (p, m[:, :, 0], 17, 9),
                 (p[:, :, 0], m, 17, 9), (p, m, 17, 9, (0, 0, 256)), (np.zeros((1, 8193, 3), np.uint8), m, 17, 9)]:
        with pytest.raises((ValueError, TypeError)):
            native.remap_cpu(*args)


# ----------------------------------------------------------------------------------- views.py

LENSES = [{"model": "equidistant", "fov_deg": 185}, {"model": "equisolid", "cx": 5100, "cy": 4900, "radius": 4800},
          {"model": "stereographic", "fov_deg": 170},
          {"model": "brown", "fx": 6000, "fy": 10600, "k1": -0.28, "k2": 0.09, "k3": -0.01, "p1": 0.001, "p2": -0.002}]
VIEWS = [{"type": "ptz", "pan": 25, "tilt": -15, "roll": 10, "fov": 70, "width": 65, "height": 33},
         {"type": "ptz", "mount": "ceiling", "pan": 200, "tilt": -40, "fov": 60, "width": 33, "height": 17},
         {"type": "panorama", "pan0": -60, "pan1": 60, "tilt0": 30, "tilt1": -30, "width": 130, "height": 16}]


def _radius(lens, theta, w):
    """r(theta) of the issue's lens models, written out again."""
    big, half = lens.get("radius", 5000) / 10000 * w, math.radians(lens.get("fov_deg", 180)) / 2
    return {"equidistant": lambda: big / half * theta, "equisolid": lambda: big / math.sin(half / 2) * math.sin(theta / 2),
            "stereographic": lambda: big / math.tan(half / 2) * math.tan(theta / 2)}[lens["model"]]()


@pytest.mark.parametrize("lens", LENSES, ids=lambda d: d["model"])
def test_mesh_nodes_are_their_rays(lens):
    W, H = 640, 480
    for view in VIEWS:
        mesh = views.build_mesh(lens, view, W, H)
        assert mesh.dtype == np.int32 and mesh.shape == views.mesh_shape(view["width"], view["height"])
        v = views.check_view(view)
        for n, m in [(0, 0), (mesh.shape[0] - 1, mesh.shape[1] - 1), (1, 2), (0, mesh.shape[1] - 1)]:
            d = views.rays(v, [views.CELL * m], [views.CELL * n])[0, 0]  # the ray of that node, then the lens by hand
            cx, cy = lens.get("cx", 5000) / 10000 * W - 0.5, lens.get("cy", 5000) / 10000 * H - 0.5
            if lens["model"] == "brown":
                if d[2] <= 0:
                    continue
                a, b = d[0] / d[2], d[1] / d[2]
                r2 = a * a + b * b
                rad = 1 + lens["k1"] * r2 + lens["k2"] * r2 ** 2 + lens["k3"] * r2 ** 3
                want = (cx + 0.6 * W * (a * rad + 2 * lens["p1"] * a * b + lens["p2"] * (r2 + 2 * a * a)),
                        cy + 1.06 * H * (b * rad + lens["p1"] * (r2 + 2 * b * b) + 2 * lens["p2"] * a * b))
            else:
                rho = math.hypot(d[0], d[1])
                r = _radius(lens, math.atan2(rho, d[2]), W)
                want = (cx + r * d[0] / rho, cy + r * d[1] / rho)
            want = np.clip(np.array(want) * 256, dc.LO, dc.HI - 1)  # (the clamp every mesh word is under)
            assert np.abs(mesh[n, m] - want).max() <= 1, (view, n, m, mesh[n, m], want)


@pytest.mark.parametrize("lens", LENSES, ids=lambda d: d["model"])
def test_rays_land_where_the_model_says(lens):
    W, H = 641, 481
    centre = np.array([lens.get("cx", 5000) / 10000 * W - 0.5, lens.get("cy", 5000) / 10000 * H - 0.5])
    # a zero-angle ptz looks along the lens axis: its centre pixel is the lens's centre
    zero = {"type": "ptz", "width": 33, "height": 17, "fov": 60}
    assert np.allclose(views.positions(lens, zero, W, H, [16], [8])[0, 0], centre, atol=1e-9)
    # panning by theta turns the centre ray by theta: it lands r(theta) right of the centre
    for theta in (10, 45, 80):
        got = views.positions(lens, dict(zero, pan=theta), W, H, [16], [8])[0, 0] - centre
        t = math.radians(theta)
        want = 0.6 * W * math.tan(t) * (1 + lens["k1"] * math.tan(t) ** 2 + lens["k2"] * math.tan(t) ** 4
                                        + lens["k3"] * math.tan(t) ** 6) + 0.6 * W * lens["p2"] * 3 * math.tan(t) ** 2 \
            if lens["model"] == "brown" else _radius(lens, t, W)
        assert abs(got[0] - want) < 1e-9 * max(1.0, abs(want)) * W, (theta, got, want)
        assert lens["model"] == "brown" or abs(got[1]) < 1e-9 * W  # (brown: p1 moves it off the row)


R3, S20, C20, S80, C80 = math.sqrt(3) / 2, math.sin(math.radians(20)), math.cos(math.radians(20)), \
    math.sin(math.radians(80)), math.cos(math.radians(80))
_PTZ = {"type": "ptz", "width": 33, "height": 17, "fov": 90}  # pixel (16, 8) is the centre, f = 16.5 pixels
_PANO = {"type": "panorama", "width": 3, "height": 1}        # three columns: the middle of each third
RAYS = [  # view, pixel, its ray in the lens's frame (x right, y down, z along the axis), worked out by hand
    (dict(_PTZ, mount="ceiling", tilt=-90), (16, 8), (0, 0, 1)),            # straight down: the lens axis
    (dict(_PTZ, mount="ceiling", tilt=-30), (16, 8), (0, -R3, 0.5)),        # pan 0: towards the image's top
    (dict(_PTZ, mount="ceiling", pan=90, tilt=-30), (16, 8), (R3, 0, 0.5)),  # pan 90: towards its right
    (dict(_PTZ, mount="ceiling", pan=90, tilt=-30, roll=180), (16, 8), (R3, 0, 0.5)),  # roll keeps the centre
    (dict(_PTZ, pan=90, tilt=30), (16, 8), (R3, -0.5, 0)),                  # wall: tilt first, then pan about the vertical
    (dict(_PTZ, roll=90), (32, 8), (0, 16, 16.5)),                          # roll 90: the view's right is the lens's down
    (dict(_PTZ, tilt=90), (16, 0), (0, -16.5, -8)),                         # looking up, the top row looks behind
    (dict(_PANO, pan0=-120, pan1=120, tilt0=60, tilt1=-20), (1, 0), (0, -S20, C20)),  # azimuth 0, elevation 20
    (dict(_PANO, pan0=-120, pan1=120, tilt0=60, tilt1=-20), (2, 0), (C20 * S80, -S20, C20 * C80)),  # azimuth 80
    (dict(_PANO, mount="ceiling", pan0=0, pan1=180, tilt0=0, tilt1=-60), (1, 0), (R3, 0, 0.5)),  # azimuth 90, 30 below
    (dict(_PANO, mount="ceiling", pan0=0, pan1=180, tilt0=0, tilt1=-60), (0, 0), (R3 / 2, -0.75, 0.5)),  # azimuth 30
]


@pytest.mark.parametrize("view,pixel,want", RAYS)
def test_rays_by_hand(view, pixel, want):
    d = views.rays(views.check_view(view), [pixel[0]], [pixel[1]])[0, 0]
    assert np.allclose(d / np.linalg.norm(d), np.array(want) / np.linalg.norm(want), atol=1e-12), d


def test_bad_lenses_and_views():
    good_lens, good_view = LENSES[0], VIEWS[0]
    for bad in (None, {}, {"model": "pinhole"}, dict(good_lens, fov_deg=0), dict(good_lens, radius="big"),
                dict(good_lens, zoom=1), {"model": "brown"}, dict(LENSES[3], k1=float("nan"))):
        with pytest.raises(ValueError):
            views.check_lens(bad)
    for bad in (None, {"type": "ptz"}, dict(good_view, width=0), dict(good_view, height=4097), dict(good_view, fov=180),
                dict(good_view, type="dome"), dict(good_view, mount="floor"), dict(good_view, pan="left"),
                dict(VIEWS[2], pan1=-60), dict(good_view, width=64.0)):
        with pytest.raises(ValueError):
            views.check_view(bad)
    with pytest.raises(ValueError):
        views.build_mesh(good_lens, good_view, 8193, 100)
    with pytest.raises(ValueError):
        views.to_native(views.identity_mesh(16, 16), 17, 16)


# ----------------------------------------------------------------- the Worker's CPU backend

LENS = {"model": "equidistant", "fov_deg": 180}
VIEW = {"type": "ptz", "pan": 20, "tilt": 10, "fov": 80, "width": 96, "height": 64}


def test_worker_views(native):
    wk, cam, step = _camera(native, history=3, masks=MASKS)
    mesh = views.build_mesh(LENS, VIEW, 320, 240)
    assert wk.read_view(cam, mesh, 320, 240, 96, 64) is None  # no frame yet
    assert step() and step()
    frames = {m["seq"]: f for m, f in wk.read_history(cam, 0, 3)}
    for seq in (0, 1, 2):  # by seq, under the masks: the twin on the (masked) frame of the ring
        m, got = wk.read_view(cam, mesh, 320, 240, 96, 64, seq=seq, pad=dc.PAD)
        assert m["seq"] == (seq or 2) and np.array_equal(got, dc.oracle(frames[seq or 2], mesh, 96, 64, dc.PAD))
    assert wk.read_view(cam, mesh, 320, 240, 96, 64, after=2) is None
    m, jpg = wk.read_view_jpeg(cam, mesh, 320, 240, 96, 64, quality=80)
    assert m["seq"] == 2 and jpg == native.jpeg_encode_cpu(native.remap_cpu(frames[2], mesh, 96, 64), 80)
    # a mesh built for another source size: the distinct answer, with the frame's size
    m, none = wk.read_view(cam, mesh, 640, 480, 96, 64)
    assert none is None and (m["width"], m["height"]) == (320, 240)
    assert wk.read_view_jpeg(cam, mesh, 640, 480, 96, 64)[1] is None
    rs = wk.read_views_many([(cam, 0, 1, mesh, 320, 240, 96, 64), (77, 0, 0, mesh, 320, 240, 96, 64),
                             (cam, 0, 0, views.identity_mesh(20, 10), 320, 240, 20, 10), (cam, 0, 0, mesh, 64, 48, 96, 64)])
    assert rs[0][0]["seq"] == 1 and rs[1] is None and rs[3][1] is None
    assert np.array_equal(rs[0][1], native.remap_cpu(frames[1], mesh, 96, 64)) and np.array_equal(rs[2][1], frames[2][:10, :20])
    for kw in (dict(width=97), dict(height=0), dict(pad=(0, 0, 300)), dict(after=-1), dict(seq=-1), dict(src_width=8193)):
        args = dict(src_width=320, src_height=240, width=96, height=64)
        args.update(kw)
        with pytest.raises(ValueError):
            wk.read_view(cam, mesh, **args)
    # a mask change leaves no view readable until the next frame
    wk.set_privacy_masks(cam, privacy.to_native(MASKS[:1]))
    assert wk.read_view(cam, mesh, 320, 240, 96, 64) is None and wk.read_view(cam, mesh, 320, 240, 96, 64, seq=2) is None
    assert wk.read_view_jpeg(cam, mesh, 320, 240, 96, 64) is None
    assert step() and wk.read_view(cam, mesh, 320, 240, 96, 64)[0]["seq"] == 3


def test_hub_views(native, tmp_path):
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, CameraNotFound, Hub
    from video_edge_ai_proxy_amd.engine.isolated import ProcessHub

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    hub = Hub(cfg, devices=[-1, -1])
    try:
        frames = {}
        for k, (name, w, h) in enumerate([("a", 320, 240), ("b", 160, 96)]):
            wk = hub.workers[k]
            cam = wk.add_camera(name, 2)
            hub.cameras[name] = CameraHandle(name, k, cam, "", session=_NoSession())
            assert wk.decode_now(cam, synth(native, w, h, gop=6, motion=0.2, seed=k + 1).next())
            frames[name] = wk.read_latest(cam, 0)[1]
        with pytest.raises(ValueError):
            hub.view("a", VIEW)  # no lens yet
        hub.set_views("a", LENS, {"door": VIEW})
        hub.set_views("b", LENSES[3])
        assert hub.views("a")["views"]["door"]["pan"] == 20 and hub.views("b")["views"] == {}
        seq, got = hub.view("a", "door")
        assert seq == 1 and np.array_equal(got, dc.oracle(frames["a"], views.build_mesh(LENS, VIEW, 320, 240), 96, 64))
        assert hub.workers[0].last_query(hub.cameras["a"].cam) > 0  # a query: the lazy decoder stays awake
        ptz = {"type": "ptz", "width": 160, "height": 96}  # zero angles on a brown lens: the undistorted picture
        many = hub.views_many({"b": ptz, "a": dict(VIEW, pan=-30)}, pad=dc.PAD)
        assert list(many) == ["b", "a"] and np.array_equal(
            many["b"][1], dc.oracle(frames["b"], views.build_mesh(LENSES[3], ptz, 160, 96), 160, 96, dc.PAD))
        assert hub.view("a", "door", after=1) is None and hub.view_counts() == 3
        seq, jpg = hub.view_jpeg("a", "door", quality=70)
        assert jpg == native.jpeg_encode_cpu(got, 70)
        for call in (lambda: hub.view("a", "window"), lambda: hub.view("a", dict(VIEW, fov=0)), lambda: hub.view("a", 5),
                     lambda: hub.set_views("a", {"model": "x"}), lambda: hub.set_views("a", LENS, {"v": {"type": "ptz"}}),
                     lambda: hub.view("a", "door", seq=-1), lambda: hub.view_jpeg("a", "door", quality=0)):
            with pytest.raises(ValueError):
                call()
        cfg.serving.view_max_bytes = 96 * 64 * 3  # bounds the request: one such view, not two
        assert hub.view("a", "door")[0] == 1
        with pytest.raises(ValueError):
            hub.views_many({"a": "door", "b": dict(VIEW)})
        with pytest.raises(ValueError):
            hub.view_jpeg("a", dict(VIEW, width=97))
        with pytest.raises(CameraNotFound):
            hub.view("nope", "door")
        hub.clear_views("a")
        assert hub.views("a") is None
        with pytest.raises(NotImplementedError, match="gpu.isolation: process"):
            ProcessHub.view(object(), "a", "door")
    finally:
        hub.shutdown()


def test_rest_views_and_restore(native, farm, tmp_path):
    app = _app(tmp_path, **{"buffer.in_memory": 64})
    try:
        rest = _rest(app)
        body = {"lens": LENS, "views": {"door": VIEW}}
        assert rest.put("/api/v1/process/nope/views", json=body).status_code == 404
        url = f"rtsp://127.0.0.1:{farm.port}/cam"
        assert rest.post("/api/v1/process", json={"name": "dome", "rtsp_endpoint": url}).status_code == 200
        assert rest.get("/api/v1/process/dome/view.jpg?view=door").status_code == 422  # no lens yet
        for bad in ([], {"views": {}}, {"lens": {"model": "x"}}, {"lens": LENS, "views": {"v": {"type": "ptz"}}},
                    {"lens": LENS, "zoom": 1}):
            assert rest.put("/api/v1/process/dome/views", json=bad).status_code == 422, bad
        assert rest.put("/api/v1/process/dome/views", json=body).status_code == 204
        assert rest.get("/api/v1/process/dome/views").json()["views"]["door"]["fov"] == 80
        meta, _ = _first_frame(app.hub, "dome")
        seq = int(meta["seq"])
        frame = {int(m["seq"]): f for m, f in app.hub.history("dome", 0, 0)}[seq]
        want = dc.oracle(frame, views.build_mesh(LENS, VIEW, 320, 240), 96, 64)
        r = rest.post("/api/v1/process/dome/view", json={"view": "door", "seq": seq})
        assert r.status_code == 200 and r.headers["X-Vep-Seq"] == str(seq) and r.headers["X-Vep-View"] == "96,64"
        assert r.content == want.tobytes()
        r = rest.get(f"/api/v1/process/dome/view.jpg?view=door&seq={seq}&quality=80")
        assert r.status_code == 200 and r.headers["content-type"] == "image/jpeg" and r.content == native.jpeg_encode_cpu(want, 80)
        ptz = rest.get(f"/api/v1/process/dome/view.jpg?pan=20&tilt=10&fov=80&width=96&height=64&seq={seq}&quality=80")
        assert ptz.status_code == 200 and ptz.content == r.content  # the same view, ad hoc
        for q in ("view=window", "pan=20", "width=0&height=8", "width=8&height=8&fov=180", "view=door&quality=0"):
            assert rest.get(f"/api/v1/process/dome/view.jpg?{q}").status_code == 422, q
        assert rest.get("/api/v1/process/dome/view.jpg?view=door&seq=1000000000").status_code == 404
        assert rest.post("/api/v1/process/dome/view", json={"view": "door", "zoom": 2}).status_code == 422
        assert _metric(rest.get("/metrics").text, "vep_view_requests_total") == app.hub.view_counts() >= 4
        from video_edge_ai_proxy_amd import cli

        a = cli.build_parser().parse_args(["view", "--device", "dome", "--rest", "h:1", "--view", "door", "--out", "x.jpg"])
        assert a.fn is cli.cmd_view and cli.view_url(a) == "http://h:1/api/v1/process/dome/view.jpg?view=door"
        # the stored views are in force after a restart, and deleted with the camera
        app.hub.stop_camera("dome")
        assert app.pm.restore() == ["dome"] and app.hub.views("dome")["views"]["door"]["width"] == 96
        assert rest.delete("/api/v1/process/dome/views").status_code == 204 and app.pm.stored_views("dome") is None
        assert rest.put("/api/v1/process/dome/views", json=body).status_code == 204
        app.pm.stop("dome")
        assert app.pm.stored_views("dome") is None
    finally:
        app.stop()
