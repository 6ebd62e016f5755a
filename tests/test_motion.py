"""Motion detection on the host: the CPU twin (csrc/vep/motion.cpp) against the independent
oracle (tests/motion_oracle.py), the CPU-backend Worker and Hub paths against the oracle applied to
the frames they served, the REST routes, the config section and the CLI parser. Everything is
exact. The GPU paths are held to the same CPU functions in tests/test_gpu_motion.py."""
import time

import numpy as np
import pytest

import motion_oracle as mo
from conftest import synth

# picture (w, h), cell: one partial cell, partial right / bottom cells, an exact grid, single
# rows and columns, one cell wider than the picture
SHAPES = [((7, 5), 8), ((17, 9), 8), ((33, 17), 16), ((64, 48), 16), ((200, 120), 32), ((1, 9), 4), ((9, 1), 4),
          ((300, 3), 256)]


def check_update(native, a, b, cell, threshold=24, shift=4):
    """Prime on a, evaluate b: both steps equal the oracle in counts and background."""
    c0, bg0 = native.motion_update_cpu(a, None, cell, threshold, shift)
    wc0, wbg0 = mo.update(a, None, cell, threshold, shift)
    assert c0.dtype == np.uint32 and bg0.dtype == np.uint16
    assert np.array_equal(c0, wc0) and np.array_equal(bg0, wbg0)
    c1, bg1 = native.motion_update_cpu(b, bg0, cell, threshold, shift)
    wc1, wbg1 = mo.update(b, wbg0, cell, threshold, shift)
    assert c1.shape == wc1.shape == tuple(reversed(native.motion_grid(a.shape[1], a.shape[0], cell)))
    assert np.array_equal(c1, wc1) and np.array_equal(bg1, wbg1)
    return c1


# --------------------------------------------------------------------------------- the update

@pytest.mark.parametrize("size,cell", SHAPES)
@pytest.mark.parametrize("kind", ["noise", "gradient"])
def test_update_equals_oracle(native, size, cell, kind):
    w, h = size
    c = check_update(native, mo.picture(kind, w, h, 1), mo.picture(kind, w, h, 2), cell)
    assert c.sum() > 0  # the pairs do differ


def test_update_equals_oracle_1080p(native):
    c = check_update(native, mo.picture("noise", 1920, 1080, 1), mo.picture("noise", 1920, 1080, 2), 16)
    assert c.shape == (68, 120)  # 67.5 cell rows


@pytest.mark.parametrize("t", [0, 24, 254])
def test_threshold_edge(native, t):
    w, h, cell = 33, 17, 16
    base = 100 if 100 + t + 1 <= 255 else 0  # (base + 254 + 1 fits a byte only from base 0)
    _, bg = native.motion_update_cpu(mo.grey(base, w, h), None, cell, t, 0)
    assert (bg == base << 8).all()
    c, _ = native.motion_update_cpu(mo.grey(base + t, w, h), bg, cell, t, 0)
    assert not c.any()  # |Y - ref| == threshold is not a change
    c, _ = native.motion_update_cpu(mo.grey(base + t + 1, w, h), bg, cell, t, 0)
    assert c.sum() == w * h and np.array_equal(c, mo.update(mo.grey(base + t + 1, w, h), bg, cell, t, 0)[0])


def test_threshold_255_never_changes(native):
    _, bg = native.motion_update_cpu(mo.grey(0, 20, 10), None, 8, 255, 0)
    c, bg = native.motion_update_cpu(mo.grey(255, 20, 10), bg, 8, 255, 0)
    assert not c.any() and (bg == 255 << 8).all()


@pytest.mark.parametrize("shift", [0, 1, 4, 8])
def test_model_over_time(native, shift):
    """Six frames: every intermediate background and grid. A shift that truncates towards zero
    instead of flooring differs from the oracle wherever the background falls."""
    w, h, cell = 33, 17, 16
    frames = [mo.picture("noise", w, h, 10 + k) for k in range(6)]
    bg = want = None
    for k, f in enumerate(frames):
        c, bg = native.motion_update_cpu(f, bg, cell, 24, shift)
        wc, want = mo.update(f, want, cell, 24, shift)
        assert np.array_equal(c, wc) and np.array_equal(bg, want), (shift, k)
        assert 0 <= int(bg.min()) and int(bg.max()) <= 65280
        if shift == 0:
            assert np.array_equal(bg, mo.luma(f) << 8)  # plain frame differencing
    falling = mo.luma(frames[1]) < mo.luma(frames[0])
    assert falling.any()  # (the case a truncating shift gets wrong is in the sequence)


def test_priming(native):
    f = mo.picture("gradient", 33, 17)
    c, bg = native.motion_update_cpu(f, None, 16, 0, 4)
    assert c.shape == (2, 3) and not c.any()
    assert np.array_equal(bg, mo.luma(f) << 8)


def test_update_argument_checks(native):
    f = mo.picture("noise", 16, 8)
    bg = native.motion_update_cpu(f, None)[1]
    for args in [(f, None, 3), (f, None, 257), (f, None, 16, -1), (f, None, 16, 256), (f, None, 16, 24, -1),
                 (f, None, 16, 24, 9), (f[:, :, :2], None), (f, bg[:4]), (f, bg.astype(np.int32))]:
        with pytest.raises(Exception):
            native.motion_update_cpu(*args)
    for args in [(0, 8, 8), (8, 0, 8), (8, 8, 3), (65536, 8, 8)]:
        with pytest.raises(Exception):
            native.motion_grid(*args)


# -------------------------------------------------------------------------------- the summary

def test_summary_blob(native):
    w, h, cell = 100, 60, 16  # 7 x 4 cells, the right column 4 wide, the bottom row 12 high
    base = mo.grey(50, w, h)
    pic = mo.blob(50, w, h, 20, 10, 30, 25, 60)  # x 20..49, y 10..34: cells 1..3 x 0..2
    _, bg = native.motion_update_cpu(base, None, cell, 24, 4)
    c, _ = native.motion_update_cpu(pic, bg, cell, 24, 4)
    assert np.array_equal(c, mo.update(pic, bg, cell, 24, 4)[0]) and c.sum() == 30 * 25
    # 25 %: a 16 x 16 cell needs 64 pixels. Cell (1, 0) holds 12 x 6 = 72, (3, 0) 2 x 6 = 12,
    # (1, 2) 12 x 3 = 36, (2, 1) all 256.
    s = native.motion_summarize(c, w, h, cell, 25, 1)
    assert s == mo.summarize(c, w, h, cell, 25, 1)
    assert s["changed"] == 750 and s["active"] == 4 and s["box"] == (16, 0, 32, 32) and s["motion"]
    s = native.motion_summarize(c, w, h, cell, 1, 1)  # any 3 pixels of 256: all nine cells
    assert s == mo.summarize(c, w, h, cell, 1, 1) and s["active"] == 9 and s["box"] == (16, 0, 48, 48)
    s = native.motion_summarize(c, w, h, cell, 100, 1)
    assert s["active"] == 1 and s["box"] == (32, 16, 16, 16)
    assert native.motion_summarize(c, w, h, cell, 25, 5)["motion"] is False  # min_cells gates motion
    assert native.motion_summarize(c, w, h, cell, 25, 4)["motion"] is True
    z = native.motion_summarize(np.zeros_like(c), w, h, cell, 25, 1)
    assert z == {"changed": 0, "active": 0, "box": None, "motion": False}


def test_summary_partial_cells_use_their_true_size(native):
    w, h, cell = 100, 60, 16
    base = mo.grey(50, w, h)
    pic = mo.blob(50, w, h, 98, 50, 2, 10, 60)  # 20 pixels in the corner cell of 4 x 12 = 48 pixels
    _, bg = native.motion_update_cpu(base, None, cell, 24, 4)
    c, _ = native.motion_update_cpu(pic, bg, cell, 24, 4)
    assert c[3, 6] == 20 and c.sum() == 20
    # 20 of 48 is 41 %: active at 41, not at 42; of a full cell's 256 it would be 7 %
    for pct, active in [(25, 1), (41, 1), (42, 0)]:
        s = native.motion_summarize(c, w, h, cell, pct, 1)
        assert s == mo.summarize(c, w, h, cell, pct, 1) and s["active"] == active, pct
    assert native.motion_summarize(c, w, h, cell, 25, 1)["box"] == (96, 48, 4, 12)  # clipped to the picture
    for args in [(c, w, h, cell, 0, 1), (c, w, h, cell, 101, 1), (c, w, h, cell, 25, 0), (c, w, h, 32, 25, 1),
                 (c[:2], w, h, cell, 25, 1)]:
        with pytest.raises(Exception):
            native.motion_summarize(*args)


def test_reference_op(native):
    import torch

    from video_edge_ai_proxy_amd import ops

    a, b = mo.picture("noise", 33, 17, 1), mo.picture("noise", 33, 17, 2)
    c0, bg0 = ops.motion_update_reference(torch.from_numpy(a), None, 16, 24, 4)
    assert c0.dtype == torch.int32 and bg0.dtype == torch.uint16 and not c0.any()
    c1, bg1 = ops.motion_update_reference(torch.from_numpy(b), bg0, 16, 24, 4)
    wc, wbg = mo.update(b, mo.update(a, None, 16, 24, 4)[1], 16, 24, 4)
    assert np.array_equal(c1.numpy(), wc) and np.array_equal(bg1.numpy(), wbg)
    t = torch.from_numpy(a)
    for bad in [dict(cell=3), dict(cell=257), dict(threshold=256), dict(learn_shift=9), dict(cell=16.0)]:
        with pytest.raises(ValueError):
            ops.motion_update_reference(t, None, **bad)
    with pytest.raises(TypeError):
        ops.motion_update_reference(t.float())
    with pytest.raises(ValueError):
        ops.motion_update_reference(t[:, ::2])  # not contiguous
    with pytest.raises(TypeError):
        ops.motion_update_reference(t, bg0.to(torch.int32))
    with pytest.raises(ValueError):
        ops.motion_update_reference(t, bg0[:4])


# ------------------------------------------------------------------------ CPU-backend Worker

def _feed(native, wk, name, w, h, frames=1, **kw):
    enc = synth(native, w, h, gop=6, motion=0.2, **kw)
    cam = wk.add_camera(name, 2)
    for _ in range(frames):
        assert wk.decode_now(cam, enc.next())
    return cam, enc


def _expect(frame, bg, prm, seq):
    """The dict Worker.read_motion owes for `frame` against the oracle's background `bg`."""
    h, w = frame.shape[:2]
    counts, new = mo.update(frame, bg, prm["cell"], prm["threshold"], prm["learn_shift"])
    cols, rows = mo.grid(w, h, prm["cell"])
    want = mo.summarize(counts, w, h, prm["cell"], prm["cell_percent"], prm["min_cells"])
    want.update(seq=seq, width=w, height=h, cell=prm["cell"], cols=cols, rows=rows, threshold=prm["threshold"],
                primed=bg is not None)
    return want, counts, new


def _same(got, want, counts):
    assert got is not None
    g = dict(got)
    assert np.array_equal(g.pop("counts"), counts)
    assert g == want, (g, want)


def test_worker_motion_cpu_backend(native):
    wk = native.Worker(device=-1)
    prm = wk.motion_params
    assert prm == {"cell": 16, "threshold": 24, "learn_shift": 4, "cell_percent": 25, "min_cells": 1}
    cam, enc = _feed(native, wk, "c", 320, 240)
    m0, f0 = wk.read_latest(cam, 0)
    r0 = wk.read_motion(cam, 0)
    want, counts, bg = _expect(f0, None, prm, m0["seq"])
    _same(r0, want, counts)
    assert r0["primed"] is False and r0["motion"] is False and r0["changed"] == 0
    assert wk.stats(cam)["motion_evaluations"] == 1
    # a second frame: the oracle applied to the two frames read_latest served
    assert wk.decode_now(cam, enc.next())
    m1, f1 = wk.read_latest(cam, 0)
    assert m1["seq"] > m0["seq"]
    r1 = wk.read_motion(cam, m0["seq"])
    want, counts, bg = _expect(f1, bg, prm, m1["seq"])
    _same(r1, want, counts)
    assert r1["primed"] is True and r1["changed"] > 0
    # the same seq again: the stored answer, no second evaluation
    again = wk.read_motion(cam, 0)
    _same(again, want, counts)
    st = wk.stats(cam)
    assert st["motion_evaluations"] == 2 and st["motion_frames"] == int(r1["motion"])
    assert wk.read_motion(cam, m1["seq"]) is None  # nothing newer
    # a reset primes again, from the same frame
    wk.motion_reset(cam)
    r = wk.read_motion(cam, 0)
    want0, counts0, _ = _expect(f1, None, prm, m1["seq"])
    _same(r, want0, counts0)
    assert wk.stats(cam)["motion_evaluations"] == 3
    with pytest.raises(Exception):
        wk.read_motion(99, 0)
    with pytest.raises(Exception):
        wk.motion_reset(99)


def test_worker_motion_params(native):
    wk = native.Worker(device=-1)
    cam, enc = _feed(native, wk, "c", 160, 96)
    assert wk.read_motion(cam, 0)["primed"] is False
    wk.set_motion_params(8, 10, 0, 50, 2)
    prm = wk.motion_params
    assert prm == {"cell": 8, "threshold": 10, "learn_shift": 0, "cell_percent": 50, "min_cells": 2}
    m0, f0 = wk.read_latest(cam, 0)
    r = wk.read_motion(cam, 0)  # new parameters reset every model: the same frame primes again
    want, counts, bg = _expect(f0, None, prm, m0["seq"])
    _same(r, want, counts)
    assert wk.decode_now(cam, enc.next())
    m1, f1 = wk.read_latest(cam, 0)
    want, counts, bg = _expect(f1, bg, prm, m1["seq"])
    _same(wk.read_motion(cam, 0), want, counts)
    for bad in [(3, 24, 4, 25, 1), (257, 24, 4, 25, 1), (16, -1, 4, 25, 1), (16, 256, 4, 25, 1), (16, 24, -1, 25, 1),
                (16, 24, 9, 25, 1), (16, 24, 4, 0, 1), (16, 24, 4, 101, 1), (16, 24, 4, 25, 0)]:
        with pytest.raises(Exception):
            wk.set_motion_params(*bad)
    assert wk.motion_params == prm  # a refused call changes nothing


def test_worker_motion_many_cpu_backend(native):
    wk = native.Worker(device=-1)
    prm = wk.motion_params
    a, enc_a = _feed(native, wk, "a", 320, 240)
    b, enc_b = _feed(native, wk, "b", 160, 96, seed=5)
    empty = wk.add_camera("e", 2)
    fa, fb = wk.read_latest(a, 0), wk.read_latest(b, 0)
    rs = wk.read_motion_many([a, b, empty, 77, b])
    assert len(rs) == 5 and rs[2] is None and rs[3] is None
    wa, ca, bga = _expect(fa[1], None, prm, fa[0]["seq"])
    wb, cb, bgb = _expect(fb[1], None, prm, fb[0]["seq"])
    _same(rs[0], wa, ca)
    _same(rs[1], wb, cb)
    _same(rs[4], wb, cb)  # a camera named twice is evaluated once
    assert wk.stats(b)["motion_evaluations"] == 1
    assert wk.decode_now(a, enc_a.next())  # only a moves on: b answers from its store
    fa = wk.read_latest(a, 0)
    rs = wk.read_motion_many([b, a])
    wa, ca, _ = _expect(fa[1], bga, prm, fa[0]["seq"])
    _same(rs[1], wa, ca)
    _same(rs[0], wb, cb)
    assert wk.stats(a)["motion_evaluations"] == 2 and wk.stats(b)["motion_evaluations"] == 1
    assert wk.read_motion_many([]) == []
    wk.remove_camera(a)
    assert wk.read_motion_many([a, b])[0] is None


# ----------------------------------------------------------------------------------- Hub

class _NoSession:
    def stop(self):
        pass


KEYS = {"seq", "width", "height", "cell", "cols", "rows", "threshold", "primed", "changed", "active", "score", "box",
        "motion"}


def test_hub_motion_across_two_workers(native, tmp_path):
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, CameraNotFound, Hub

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    cfg.motion.cell, cfg.motion.threshold, cfg.motion.learn_shift = 8, 12, 2
    hub = Hub(cfg, devices=[-1, -1])
    try:
        prm = {"cell": 8, "threshold": 12, "learn_shift": 2, "cell_percent": 25, "min_cells": 1}
        assert all(w.motion_params == prm for w in hub.workers)  # the section reaches every worker
        encs, bgs = {}, {}
        for k, (name, w, h) in enumerate([("cam_a", 320, 240), ("cam_b", 160, 96), ("cam_c", 320, 176)]):
            wi = k % 2
            cam, encs[name] = _feed(native, hub.workers[wi], name, w, h, seed=k + 1)
            hub.cameras[name] = CameraHandle(name, wi, cam, "", session=_NoSession())
        assert hub.motion("cam_a")["primed"] is False
        first = hub.motion_many()
        assert list(first) == ["cam_a", "cam_b", "cam_c"] and all(set(r) == KEYS for r in first.values())
        assert not any(r["primed"] or r["motion"] for r in first.values())
        for name, h in hub.cameras.items():
            wk = hub.workers[h.worker_index]
            bgs[name] = mo.update(wk.read_latest(h.cam, 0)[1], None, 8, 12, 2)[1]
            assert wk.decode_now(h.cam, encs[name].next())
            assert wk.last_query(h.cam) > 0  # asking keeps the lazy decoder awake
        got = hub.motion_many(["cam_c", "cam_a", "cam_b"], grid=True)
        assert list(got) == ["cam_c", "cam_a", "cam_b"]
        for name, h in hub.cameras.items():
            meta, frame = hub.workers[h.worker_index].read_latest(h.cam, 0)
            want, counts, _ = _expect(frame, bgs[name], prm, meta["seq"])
            want["box"] = None if want["box"] is None else list(want["box"])
            want["score"] = want["changed"] / (want["width"] * want["height"])
            r = dict(got[name])
            assert r.pop("counts") == counts.tolist()
            assert r == want and r["primed"] is True and r["changed"] > 0
            assert hub.motion(name) == r and hub.motion(name, grid=True)["counts"] == counts.tolist()
            assert hub.motion(name, after=meta["seq"]) is None
            assert hub.workers[h.worker_index].stats(h.cam)["motion_evaluations"] == 2
        hub.motion_reset("cam_b")
        assert hub.motion("cam_b")["primed"] is False
        with pytest.raises(CameraNotFound):
            hub.motion("nope")
        with pytest.raises(CameraNotFound):
            hub.motion_many(["cam_a", "nope"])
        with pytest.raises(CameraNotFound):
            hub.motion_reset("nope")
    finally:
        hub.shutdown()


def test_process_hub_forwards_motion():
    from video_edge_ai_proxy_amd.engine.child import EXPORTED
    from video_edge_ai_proxy_amd.engine.isolated import ProcessHub

    assert {"motion", "motion_reset"} <= EXPORTED

    class Fake:
        cameras = {"b": 1, "a": 2}
        calls = []

        def handle(self, name):
            return self.cameras[name]

        def _call(self, name, method, *args):
            self.calls.append((name, method, args))
            return {"seq": 3}

    f = Fake()
    assert ProcessHub.motion(f, "a", 2, True) == {"seq": 3} and f.calls[-1] == ("a", "motion", (2, True))
    assert ProcessHub.motion_many(f) == {"a": {"seq": 3}, "b": {"seq": 3}}  # per name, sorted
    assert [c[0] for c in f.calls[1:]] == ["a", "b"]
    ProcessHub.motion_reset(f, "b")
    assert f.calls[-1] == ("b", "motion_reset", ())
    with pytest.raises(KeyError):
        ProcessHub.motion_many(f, ["a", "nope"])


# ------------------------------------------------------------------- REST, config, CLI, metrics

@pytest.fixture
def farm(native):
    srv = native.RtspServer("127.0.0.1", 0)
    for path, (w, h, seed) in {"/cam": (320, 240, 11), "/wide": (320, 176, 12)}.items():
        cfg = native.SynthConfig()
        cfg.width, cfg.height, cfg.gop, cfg.fps, cfg.seed, cfg.motion = w, h, 10, 30, seed, 0.2
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


def _start_camera(rest, farm, name, path):
    url = f"rtsp://127.0.0.1:{farm.port}{path}"
    assert rest.post("/api/v1/process", json={"name": name, "rtsp_endpoint": url}).status_code == 200


def _poll(rest, url, deadline_s=15):
    """The first 200 of url (the first request wakes the lazy decoder; 404 until a frame is there)."""
    deadline = time.time() + deadline_s
    while time.time() < deadline:
        r = rest.get(url)
        if r.status_code == 200:
            return r
        assert r.status_code == 404
        time.sleep(0.02)
    raise AssertionError(f"no 200 from {url} within {deadline_s} s")


def test_rest_motion(native, farm, hubapp):
    rest = _rest(hubapp)
    assert rest.get("/api/v1/motion").status_code == 404  # no camera running
    assert rest.get("/api/v1/process/nope/motion").status_code == 404
    assert rest.delete("/api/v1/process/nope/motion").status_code == 404
    _start_camera(rest, farm, "front_door", "/cam")
    _start_camera(rest, farm, "back_yard", "/wide")
    r = _poll(rest, "/api/v1/process/front_door/motion")
    first = r.json()
    assert set(first) == KEYS and int(r.headers["x-vep-seq"]) == first["seq"] >= 1
    assert first["primed"] is False and first["motion"] is False and (first["width"], first["height"]) == (320, 240)
    assert (first["cell"], first["cols"], first["rows"], first["threshold"]) == (16, 20, 15, 24)
    # the next frame is compared with the model; grid=1 adds the counts
    r = _poll(rest, f"/api/v1/process/front_door/motion?after={first['seq']}&grid=1")
    nxt = r.json()
    assert nxt["seq"] > first["seq"] and nxt["primed"] is True and set(nxt) == KEYS | {"counts"}
    assert len(nxt["counts"]) == 15 and all(len(row) == 20 for row in nxt["counts"])
    assert sum(map(sum, nxt["counts"])) == nxt["changed"]
    assert nxt["score"] == nxt["changed"] / (320 * 240)
    published = hubapp.hub.published("front_door")
    assert rest.get(f"/api/v1/process/front_door/motion?after={published + 1000}").status_code == 404
    # every camera, in request order; one without a frame has seq 0
    _poll(rest, "/api/v1/process/back_yard/motion")
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle

    idle = hubapp.hub.workers[0].add_camera("idle_cam", 2)
    hubapp.hub.cameras["idle_cam"] = CameraHandle("idle_cam", 0, idle, "", session=_NoSession())
    try:
        cams = rest.get("/api/v1/motion?names=idle_cam,front_door,back_yard").json()["cameras"]
        assert [c["name"] for c in cams] == ["idle_cam", "front_door", "back_yard"]
        assert cams[0] == {"name": "idle_cam", "seq": 0, "motion": False}
        assert all(set(c) == KEYS | {"name"} and c["seq"] >= 1 for c in cams[1:])
        cams = rest.get("/api/v1/motion?grid=1").json()["cameras"]
        assert [c["name"] for c in cams] == ["back_yard", "front_door", "idle_cam"]  # default: sorted
        assert "counts" in cams[0] and "counts" in cams[1]
    finally:
        hubapp.hub.cameras.pop("idle_cam")
        hubapp.hub.workers[0].remove_camera(idle)
    assert rest.get("/api/v1/motion?names=front_door,nope").status_code == 404
    for bad in ("/api/v1/motion?names=,", "/api/v1/motion?grid=2", "/api/v1/process/front_door/motion?grid=7",
                "/api/v1/process/front_door/motion?after=-1"):
        assert rest.get(bad).status_code == 400, bad
    # the reset: 204, and the next answer primes again
    assert rest.delete("/api/v1/process/front_door/motion").status_code == 204
    assert rest.get("/api/v1/process/front_door/motion").json()["primed"] is False
    # /metrics counts evaluations per camera
    text = rest.get("/metrics").text
    line = [ln for ln in text.splitlines() if ln.startswith("vep_motion_evaluations_total{") and "front_door" in ln]
    assert len(line) == 1 and float(line[0].rsplit(" ", 1)[1]) >= 3
    assert "vep_motion_frames_with_motion_total{" in text
    # existing routes answer as before
    assert rest.get("/api/v1/process/front_door/frame.jpg").status_code == 200
    assert rest.get("/api/v1/process/front_door").status_code == 200


def test_config_motion(tmp_path):
    from video_edge_ai_proxy_amd.config import load_config

    cfg = load_config(data_dir=str(tmp_path))
    m = cfg.motion
    assert (m.cell, m.threshold, m.learn_shift, m.cell_percent, m.min_cells) == (16, 24, 4, 25, 1)
    (tmp_path / "conf.yaml").write_text(
        "motion:\n  cell: 32\n  threshold: 10\n  learn_shift: 0\n  cell_percent: 50\n  min_cells: 3\n")
    m = load_config(data_dir=str(tmp_path)).motion
    assert (m.cell, m.threshold, m.learn_shift, m.cell_percent, m.min_cells) == (32, 10, 0, 50, 3)
    for bad in ("cell: 3", "cell: 257", "threshold: -1", "threshold: 256", "learn_shift: -1", "learn_shift: 9",
                "cell_percent: 0", "cell_percent: 101", "min_cells: 0", "cell: wide"):
        (tmp_path / "conf.yaml").write_text(f"motion:\n  {bad}\n")
        with pytest.raises(ValueError):
            load_config(data_dir=str(tmp_path))
    for edge in ("cell: 4", "cell: 256", "threshold: 0", "threshold: 255", "learn_shift: 8", "cell_percent: 100"):
        (tmp_path / "conf.yaml").write_text(f"motion:\n  {edge}\n")
        load_config(data_dir=str(tmp_path))


def test_cli_motion_parser():
    from video_edge_ai_proxy_amd import cli

    a = cli.build_parser().parse_args(["motion", "--device", "front_door"])
    assert (a.cmd, a.device, a.rest, a.watch, a.fn) == ("motion", "front_door", "127.0.0.1:8080", False, cli.cmd_motion)
    a = cli.build_parser().parse_args(["motion", "--device", "d", "--rest", "hub:9000", "--watch", "--interval", "0.5"])
    assert (a.rest, a.watch, a.interval) == ("hub:9000", True, 0.5)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["motion"])  # --device is required
    line = cli.format_motion({"seq": 7, "motion": True, "primed": True, "changed": 768, "score": 0.01, "active": 3,
                              "box": [16, 0, 32, 32]})
    assert line == "seq 7 MOTION changed 768 (1.00 %) active 3 box 16,0 32x32"
    assert "primed" in cli.format_motion({"seq": 1, "motion": False, "primed": False, "box": None})
