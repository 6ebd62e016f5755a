"""Motion vectors by block matching (csrc/vep/flow.h, docs/FLOW.md): the CPU twin against the numpy
oracle, exactly; the summary on hand-written grids; the serving reads on the CPU backend."""
import numpy as np
import pytest

import flow_oracle as oracle
from test_crop import _NoSession, _app, _camera, _first_frame, _rest, _slots, farm  # noqa: F401

SHIFTS = lambda R: ((0, 0), (3, -2), (-R, R), (R + 1, 0))  # noqa: E731  in samples of the plane
KINDS = 7  # the four shifts, identical, constant, stripes, random (pair() below)


def pair(kind, w, h, d, R, seed=0):
    """(newer, older): 0..3 a random texture shifted by SHIFTS(R)[kind] samples, 4 constant pictures,
    5 vertical stripes of period 4 samples shifted by 2 (vx = -2 and +2 tie), 6 independent noise."""
    rng = np.random.default_rng(seed * 8 + kind)
    if kind < 4:
        sx, sy = (s * d for s in SHIFTS(R)[kind])
        pad = (R + 3) * d
        t = rng.integers(0, 256, (h + 2 * pad, w + 2 * pad, 3)).astype(np.uint8)
        return t[pad:pad + h, pad:pad + w].copy(), t[pad + sy:pad + sy + h, pad + sx:pad + sx + w].copy()
    if kind == 4:
        return np.full((h, w, 3), 77, np.uint8), np.full((h, w, 3), 77, np.uint8)
    if kind == 5:
        x = np.arange(w + 2 * d) // d
        s = np.broadcast_to((np.where(x % 4 < 2, 40, 200).astype(np.uint8))[None, :, None], (h, w + 2 * d, 3))
        return s[:, :w].copy(), s[:, 2 * d:].copy()
    return rng.integers(0, 256, (h, w, 3)).astype(np.uint8), rng.integers(0, 256, (h, w, 3)).astype(np.uint8)


def check_pair(native, kind, w, h, d, R):
    newer, older = pair(kind, w, h, d, R, seed=w + h)
    planes, grid = native.flow_cpu(newer, older, d, R)
    want_planes, want = oracle.flow(newer, older, d, R)
    assert np.array_equal(planes, want_planes) and np.array_equal(grid, want), (kind, w, h, d, R)
    pw, ph = w // d, h // d
    assert grid.shape == (ph // 8, pw // 8, 4)
    for by, bx in np.ndindex(grid.shape[:2]):
        vx, vy, best, zero = grid[by, bx]
        if kind < 4:
            sx, sy = SHIFTS(R)[kind]
            inside = 0 <= bx * 8 - sx <= pw - 8 and 0 <= by * 8 - sy <= ph - 8
            if max(abs(sx), abs(sy)) <= R and inside:
                assert (vx, vy, best) == (sx, sy, 0), (kind, bx, by)
            elif inside:
                assert best > 0  # a shift beyond the range is not found
        elif kind == 4:
            assert (vx, vy, best, zero) == (0, 0, 0, 0)
        elif kind == 5 and R >= 2 and 2 <= bx * 8 <= pw - 10:
            assert (vx, vy, best) == (-2, 0, 0)


@pytest.mark.parametrize("R", [1, 7, 15])
@pytest.mark.parametrize("d", [1, 2, 4])
def test_twin_equals_oracle(native, d, R):
    for kind in range(KINDS):
        check_pair(native, kind, 43 * d + d - 1, 27 * d, d, R)  # w no multiple of d, w' = 43 no multiple of 8
    same = pair(6, 20 * d, 20 * d, d, R)[0]
    assert not native.flow_cpu(same, same, d, R)[1][..., :3].any()  # identical pictures: (0, 0), best 0


def test_edge_sizes_and_arguments(native):
    for d in (1, 2, 4):
        check_pair(native, 6, 8 * d, 8 * d, d, 7)  # exactly one block: only (0, 0) is valid
        a, b = pair(6, 8 * d - 1, 9 * d, d, 7)      # one sample short of a block: an empty grid
        assert native.flow_cpu(a, b, d, 7)[1].shape == (1, 0, 4)
    a, b = pair(6, 16, 16, 1, 1)
    for bad in ((3, 7), (0, 7), (2, 0), (2, 16)):
        with pytest.raises(ValueError):
            native.flow_cpu(a, b, *bad)
    with pytest.raises(ValueError):
        native.flow_cpu(a, b[:8], 1, 1)


def test_summary(native):
    def both(grid, d=2, min_gain=4, min_blocks=4, global_percent=60):
        got = native.flow_summarize(grid, d, min_gain, min_blocks, global_percent)
        want = oracle.summarize(grid.astype(np.int64), d, min_gain, min_blocks, global_percent)
        for k, v in want.items():
            assert got[k] == v, (k, got[k], v)
        return got

    g = np.zeros((3, 4, 4), np.int16)
    g[..., 3] = 1000
    # direction bins at the 5 / 12 boundaries: 12 b < 5 a is horizontal, equality is diagonal
    for n, (vx, vy) in enumerate([(12, 4), (12, 5), (5, 12), (4, 12), (-12, 5), (-12, 4), (5, -12), (4, -12), (-5, -12)]):
        g[n // 4, n % 4, :2] = (vx, vy)
    s = both(g)
    assert s["dirs"] == [1, 2, 1, 1, 1, 1, 1, 1]  # (12, 5) and (5, 12) are both SE
    assert s["moving"] == 9 and s["motion"] and s["box"] == (0, 0, 64, 48)
    assert s["mean"] == (pytest.approx(sum(g[..., 0].ravel().tolist()) * 2 / 9), pytest.approx(sum(g[..., 1].ravel().tolist()) * 2 / 9))
    # the gain threshold at equality, and min_blocks
    g = np.zeros((2, 2, 4), np.int16)
    g[0, 0] = (1, 0, 100, 100 + 64 * 4)
    g[0, 1] = (1, 0, 100, 100 + 64 * 4 - 1)
    s = both(g, min_blocks=1)
    assert s["moving"] == 1 and s["motion"] and s["box"] == (0, 0, 16, 16) and not both(g, min_blocks=2)["motion"]
    # the global mode: a tie goes to the shorter vector, then the smaller vy, then the smaller vx
    g = np.zeros((1, 4, 4), np.int16)
    g[0, :, 0] = (2, 2, -2, -2)
    assert both(g)["global"] == {"vx": -2, "vy": 0, "count": 2, "percent": 50}
    g[0, :, :2] = ((0, 3), (0, 3), (2, 1), (2, 1))
    assert both(g)["global"]["vy"] == 1
    # camera_moved at equality: 3 of 5 blocks at 60 percent, not at 61
    g = np.zeros((1, 5, 4), np.int16)
    g[0, :3, 0] = 3
    assert both(g)["camera_moved"] and not both(g, global_percent=61)["camera_moved"]
    g[0, :, 0] = 0
    assert not both(g)["camera_moved"] and not both(np.zeros((0, 3, 4), np.int16))["camera_moved"]


def test_flow_selftest():
    """csrc/tests/flow_selftest.cpp, un-instrumented (`make asan-flow` runs it under the sanitizers):
    the packed key orders candidates as docs/FLOW.md says for every range, and the multi-slot rounds
    of ring_read.h redo only the entry one of whose slots was reused, never committing a spoiled one."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["make", "-C", root, "flow-selftest"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "flow_selftest ok" in r.stdout, (r.stdout + r.stderr)[-4000:]


def newest_first(wk, cam, n):
    return [f for _, f in wk.read_history(cam, 0, n)][::-1]


@pytest.mark.parametrize("first_after", [0, 1, 2])  # who asks first about frame 3, and with which `after`
def test_worker_flow_reads(native, first_after):
    from video_edge_ai_proxy_amd import privacy

    wk, cam, step = _camera(native, history=4)
    wk.set_flow_params(decimate=1, range=3, gap=2)
    assert wk.read_flow(cam, 0) is None  # no frame yet
    for n in (1, 2):  # the ring is short: not primed, an empty grid, not an error
        assert step()
        r = wk.read_flow(cam, 0)
        assert (r["seq"], r["prev_seq"], r["primed"], r["motion"], r["grid"].shape) == (n, 0, False, False, (0, 0, 4))
    assert step()
    # `after` only decides whether the newest frame answers: the earlier frame is picked whatever it
    # is, so a client polling with the last seq it saw gets, and stores for everyone, the primed answer
    r = wk.read_flow(cam, first_after)
    f = newest_first(wk, cam, 4)
    assert (r["seq"], r["prev_seq"], r["primed"], r["block_px"]) == (3, 1, True, 8)
    assert np.array_equal(r["grid"], oracle.flow(f[0], f[2], 1, 3)[1])
    for after in (0, 1, 2):  # one evaluation however many ask, and one answer
        again = wk.read_flow(cam, after)
        assert again["primed"] and again["prev_seq"] == 1 and np.array_equal(again["grid"], r["grid"])
    assert wk.stats(cam)["flow_evaluations"] == 1
    assert wk.read_flow(cam, 3) is None
    many = wk.read_flow_many([cam, 99, cam])  # a repeated camera is evaluated once
    assert many[1] is None and np.array_equal(many[0]["grid"], r["grid"]) and np.array_equal(many[2]["grid"], r["grid"])
    assert wk.stats(cam)["flow_evaluations"] == 1
    # a privacy-mask change withdraws the earlier frames: never matched against
    wk.set_privacy_masks(cam, privacy.to_native([{"x0": 0, "y0": 0, "x1": 5000, "y1": 5000, "mode": "fill"}]))
    assert wk.read_flow(cam, 0) is None
    assert step() and wk.read_flow(cam, 0)["primed"] is False
    assert step() and step() and wk.read_flow(cam, 0)["primed"] is True
    for bad in ({"decimate": 3}, {"range": 16}, {"gap": 8}, {"min_gain": 256}, {"min_blocks": 0}, {"global_percent": 0}):
        with pytest.raises(ValueError):
            wk.set_flow_params(**bad)
    wk, cam, step = _camera(native)  # a ring without history refuses
    assert step()
    with pytest.raises(ValueError, match="buffer.in_memory"):
        wk.read_flow(cam, 0)
    with pytest.raises(ValueError, match="buffer.in_memory"):
        wk.read_flow_many([cam])


def hub_answers(native, tmp_path, dev):
    """What a hub on `dev` answers about two synthetic cameras with in_memory 4 (the GPU test compares
    a GPU hub's answers with the CPU backend's)."""
    from conftest import synth
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub

    cfg = Config()
    cfg.data_dir = str(tmp_path / f"data{dev}")
    cfg.flow.min_gain = 1
    hub = Hub(cfg, devices=[dev])
    try:
        wk, frames = hub.workers[0], {}
        for name, (w, h) in {"a": (320, 240), "b": (176, 144)}.items():
            cam = wk.add_camera(name, _slots(native, 4), 4)
            hub.cameras[name] = CameraHandle(name, 0, cam, "", session=_NoSession())
            enc = synth(native, w, h, gop=6, motion=0.5, seed=w)
            for _ in range(3):
                assert wk.decode_now(cam, enc.next())
            frames[name] = newest_first(wk, cam, 2)
        return frames, hub.flow("a", grid=True), hub.flow_many(["b", "a", "b"], grid=True), hub.flow_many()
    finally:
        hub.shutdown()


def test_hub_flow(native, tmp_path):
    frames, one, many, every = hub_answers(native, tmp_path, -1)
    assert list(many) == ["b", "a"] and list(every) == ["a", "b"] and many["a"] == one
    for name, r in many.items():
        grid = oracle.flow(frames[name][0], frames[name][1], 2, 7)[1]
        want = oracle.summarize(grid, 2, 1, 4, 60)
        assert (r["seq"], r["prev_seq"], r["primed"], r["block_px"]) == (3, 2, True, 16)
        assert r["blocks"] == [grid.shape[1], grid.shape[0]] and r["vx"] == grid[..., 0].ravel().tolist()
        assert r["best"] == grid[..., 2].ravel().tolist() and r["zero"] == grid[..., 3].ravel().tolist()
        assert (r["moving"], r["dirs"], r["motion"], r["camera_moved"]) == \
            (want["moving"], want["dirs"], want["motion"], want["camera_moved"])
        assert r["global"] == {k: want["global"][k] for k in ("vx", "vy", "percent")}
        assert r["box"] == (None if want["box"] is None else list(want["box"])) and "vx" not in every[name]


def test_rest_flow(native, farm, tmp_path):
    url = f"rtsp://127.0.0.1:{farm.port}/cam"
    app = _app(tmp_path, **{"buffer.in_memory": 8})
    try:
        rest = _rest(app)
        assert rest.get("/api/v1/process/yard/flow").status_code == 404
        assert rest.post("/api/v1/process", json={"name": "yard", "rtsp_endpoint": url}).status_code == 200
        _first_frame(app.hub, "yard")
        app.hub.wait_frame("yard", 2, 5000)
        r = rest.get("/api/v1/process/yard/flow?grid=1")
        assert r.status_code == 200 and r.json()["primed"] and len(r.json()["vx"]) == r.json()["blocks"][0] * r.json()["blocks"][1]
        assert int(r.headers["X-Vep-Seq"]) == r.json()["seq"] == r.json()["prev_seq"] + 1
        cams = rest.get("/api/v1/flow?names=yard,yard&wake=0").json()["cameras"]
        assert [c["name"] for c in cams] == ["yard"] and "vx" not in cams[0] and cams[0]["seq"] >= r.json()["seq"]
        assert rest.get("/api/v1/process/yard/flow?grid=2").status_code == 400
        assert rest.get("/api/v1/flow?names=nope").status_code == 404
        assert "vep_flow_evaluations_total{" in rest.get("/metrics").text
    finally:
        app.stop()
    app = _app(tmp_path / "plain")  # buffer.in_memory 1: no earlier frame to match against
    try:
        rest = _rest(app)
        assert rest.post("/api/v1/process", json={"name": "yard", "rtsp_endpoint": url}).status_code == 200
        _first_frame(app.hub, "yard")
        for path in ("/api/v1/process/yard/flow", "/api/v1/flow"):
            r = rest.get(path)
            assert r.status_code == 422 and "buffer.in_memory" in r.text, (path, r.text)
    finally:
        app.stop()
