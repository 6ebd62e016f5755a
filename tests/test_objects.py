"""Moving-object boxes (csrc/vep/objects.h, docs/OBJECTS.md): the CPU twin against the numpy oracle,
exactly; the serving reads, the hub, the routes, the config ranges and the CLI on the CPU backend."""
import numpy as np
import pytest

import objects_oracle as oracle
from test_crop import _NoSession, _app, _camera, _first_frame, _rest, _slots, farm  # noqa: F401
from test_flow import newest_first

TW, TH = 64, 32  # the kernels' tile
KINDS = ("empty", "full", "checkerboard", "lattice", "blocks", "diagonals", "serpentine", "serpentine_t", "u", "comb", "noise")


def mask_of(kind, pw, ph, seed=0):
    """The masks a labelling goes wrong on (bool, ph x pw)."""
    y, x = np.mgrid[0:ph, 0:pw]
    if kind == "empty":
        return np.zeros((ph, pw), bool)
    if kind == "full":
        return np.ones((ph, pw), bool)
    if kind == "checkerboard":  # one component, every link diagonal
        return (x + y) % 2 == 0
    if kind == "lattice":  # isolated samples: the most components there can be
        return (x % 2 == 0) & (y % 2 == 0)
    if kind == "blocks":  # isolated 2 x 2 blocks: the most records at min_area 4
        return (x % 3 < 2) & (y % 3 < 2)
    if kind == "diagonals":  # through the tile corner (TW, TH), both ways
        return (x - y == TW - TH) | (x + y == TW + TH - 1)
    if kind == "serpentine":  # one snake across every vertical seam on every fourth row
        return (y % 4 == 0) | (x == np.where((y // 4) % 2 == 0, pw - 1, 0))
    if kind == "serpentine_t":  # and across every horizontal seam on every fourth column
        return (x % 4 == 0) | (y == np.where((x // 4) % 2 == 0, ph - 1, 0))
    if kind == "u":  # two arms that join only in the last row: the smallest index is far from there
        return ((x == min(1, pw - 1)) | (x == pw - 2) | (y == ph - 1)) & (x >= min(1, pw - 1)) & (x <= max(pw - 2, 1))
    if kind == "comb":  # teeth that hang from the top row
        return (y == 0) | (x % 2 == 0)
    return np.random.default_rng(seed).random((ph, pw)) < 0.5


def check_twin(native, m, d=1, threshold=0, open=0, grow=0, min_area=4, extra=(0, 0)):
    newer, older = oracle.pictures(m, d, extra)
    got = native.objects_cpu(newer, older, d, threshold, open, grow, min_area)
    want = oracle.objects(newer, older, d, threshold, open, grow, min_area)
    for g, w, what in zip(got, want, ("records", "labels", "mask")):
        assert g.shape == w.shape and np.array_equal(g.astype(np.int64) if what != "mask" else g, w), (what, m.shape, d, open, grow)
    assert len(got[0]) <= m.size // min_area
    return got


@pytest.mark.parametrize("kind", KINDS)
def test_twin_equals_oracle(native, kind):
    d = (1, 2, 4)[KINDS.index(kind) % 3]
    rec, lab, _ = check_twin(native, mask_of(kind, TW + 3, TH + 2), d, extra=(d - 1, d // 2))
    if kind == "checkerboard":
        assert len(rec) == 1 and rec[0].tolist() == [0, ((TW + 3) * (TH + 2) + 1) // 2, 0, 0, TW + 3, TH + 2]
    if kind == "lattice":
        assert len(rec) == 0 and len(np.unique(lab)) == 1 + 34 * 17
    if kind == "u":
        assert rec[:, 0].tolist() == [1]


@pytest.mark.parametrize("open,grow", [(0, 0), (1, 0), (0, 1), (1, 1), (0, 3), (1, 2), (1, 3)])
def test_cleanup_equals_oracle(native, open, grow):
    m = mask_of("noise", 45, 23, seed=open * 4 + grow)
    m[3:14, 5:20] = True  # (something an opening leaves)
    many = check_twin(native, m, 2, 24, open, grow, 4, extra=(1, 1))[0]
    some = check_twin(native, m, 2, 24, open, grow, 200)[0]
    assert len(some) <= len(many) and set(some[:, 0].tolist()) <= set(many[:, 0].tolist())


def test_edge_sizes_arguments_and_summary(native):
    rec = check_twin(native, mask_of("full", 2, 2))[0]  # the count at the capacity bound
    assert rec.tolist() == [[0, 4, 0, 0, 2, 2]]
    assert len(check_twin(native, mask_of("blocks", 32, 32))[0]) == 121 <= 32 * 32 // 4
    a, b = oracle.pictures(mask_of("full", 3, 5), 1)
    assert native.objects_cpu(a, b, 4, 0, 0, 0, 4)[1].shape == (1, 0)  # narrower than one sample
    for bad in ((3, 24, 1, 1, 64), (2, 256, 1, 1, 64), (2, 24, 2, 1, 64), (2, 24, 1, 4, 64), (2, 24, 1, 1, 3), (2, 24, 1, 1, 65536)):
        with pytest.raises(ValueError):
            native.objects_cpu(a, b, *bad)
    with pytest.raises(ValueError):
        native.objects_cpu(a, b[:2], 1, 0, 0, 0, 4)
    # the summary: the largest first, ties to the smaller label, pixels clipped to the picture
    recs = np.array([[3, 9, 0, 0, 3, 3], [40, 30, 10, 2, 16, 7], [77, 9, 20, 20, 23, 23], [90, 5, 30, 30, 32, 33]], np.int64)
    for max_objects in (1, 3, 4):
        got = native.objects_summarize(recs, 2, max_objects, 63, 65)
        want = oracle.summarize(recs, 2, max_objects, 63, 65)
        assert {k: ([dict(o, box=list(o["box"])) for o in v] if k == "objects" else (list(v) if k == "box" else v))
                for k, v in got.items()} == want
    assert [o["label"] for o in native.objects_summarize(recs, 2, 3, 63, 65)["objects"]] == [40, 3, 77]
    assert native.objects_summarize(recs, 2, 4, 63, 65)["objects"][3]["box"] == (60, 60, 3, 5)
    none = native.objects_summarize(recs[:0], 2, 4, 63, 65)
    assert (none["count"], none["box"], none["motion"], none["objects"]) == (0, None, False, [])
    with pytest.raises(ValueError):
        native.objects_summarize(recs[::-1].copy(), 2, 4, 63, 65)


def test_objects_selftest():
    """csrc/tests/objects_selftest.cpp, un-instrumented (`make asan-objects` runs it under the
    sanitizers): the twin on hand-made masks, the job check's refusals and the capacity bound."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["make", "-C", root, "objects-selftest"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "objects_selftest ok" in r.stdout, (r.stdout + r.stderr)[-4000:]


def expected(f, prm):
    return oracle.objects(f[0], f[prm["gap"]], prm["decimate"], prm["threshold"], prm["open"], prm["grow"], prm["min_area"])[0]


@pytest.mark.parametrize("first_after", [0, 2])
def test_worker_objects_reads(native, first_after):
    from video_edge_ai_proxy_amd import privacy

    prm = {"decimate": 1, "threshold": 8, "gap": 2, "open": 0, "grow": 1, "min_area": 4, "max_objects": 2}
    wk, cam, step = _camera(native, history=4)
    wk.set_objects_params(**prm)
    assert wk.objects_params == prm and wk.read_objects(cam, 0) is None
    for n in (1, 2):  # the ring is short: not primed, no records, not an error
        assert step()
        r = wk.read_objects(cam, 0)
        assert (r["seq"], r["prev_seq"], r["primed"], r["motion"], r["records"].shape) == (n, 0, False, False, (0, 6))
    assert step()
    r = wk.read_objects(cam, first_after)  # `after` bounds the newest frame only
    want = expected(newest_first(wk, cam, 4), prm)
    assert (r["seq"], r["prev_seq"], r["primed"], r["count"]) == (3, 1, True, len(want)) and np.array_equal(r["records"], want)
    assert len(r["objects"]) == min(2, len(want)) and r["truncated"] == (len(want) > 2)
    for after in (0, 1, 2):  # one evaluation however many ask
        assert np.array_equal(wk.read_objects(cam, after)["records"], want)
    many = wk.read_objects_many([cam, 99, cam])
    assert many[1] is None and np.array_equal(many[0]["records"], want) and np.array_equal(many[2]["records"], want)
    assert wk.stats(cam)["objects_evaluations"] == 1 and wk.read_objects(cam, 3) is None
    wk.set_privacy_masks(cam, privacy.to_native([{"x0": 0, "y0": 0, "x1": 5000, "y1": 5000, "mode": "fill"}]))
    assert wk.read_objects(cam, 0) is None
    assert step() and wk.read_objects(cam, 0)["primed"] is False
    assert step() and step() and wk.read_objects(cam, 0)["primed"] is True
    for bad in ({"decimate": 3}, {"threshold": 256}, {"gap": 8}, {"open": 2}, {"grow": 4}, {"min_area": 3}, {"max_objects": 0}):
        with pytest.raises(ValueError):
            wk.set_objects_params(**bad)
    wk, cam, step = _camera(native)  # a ring without history refuses
    assert step()
    for read in (lambda: wk.read_objects(cam, 0), lambda: wk.read_objects_many([cam])):
        with pytest.raises(ValueError, match="buffer.in_memory"):
            read()


def hub_answers(native, tmp_path, dev):
    """What a hub on `dev` answers about two synthetic cameras with in_memory 4 (the GPU test compares
    a GPU hub's answers with the CPU backend's)."""
    from conftest import synth
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub

    cfg = Config()
    cfg.data_dir = str(tmp_path / f"data{dev}")
    cfg.objects.threshold, cfg.objects.min_area, cfg.objects.max_objects = 6, 4, 3
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
        return frames, hub.objects("a"), hub.objects_many(["b", "a", "b"]), hub.objects_many()
    finally:
        hub.shutdown()


def test_hub_objects(native, tmp_path):
    frames, one, many, every = hub_answers(native, tmp_path, -1)
    assert list(many) == ["b", "a"] and list(every) == ["a", "b"] and many["a"] == one and every == {"a": one, "b": many["b"]}
    for name, r in many.items():
        f = frames[name]
        want = oracle.summarize(oracle.objects(f[0], f[1], 2, 6, 1, 1, 4)[0], 2, 3, f[0].shape[1], f[0].shape[0])
        assert (r["seq"], r["prev_seq"], r["primed"], r["decimate"]) == (3, 2, True, 2)
        assert {k: r[k] for k in want} == want
    assert any(r["count"] for r in many.values())  # (the synthetic cameras do move)


def test_rest_config_and_cli(native, farm, tmp_path):
    from video_edge_ai_proxy_amd import cli, objects
    from video_edge_ai_proxy_amd.config import Config, validate

    url = f"rtsp://127.0.0.1:{farm.port}/cam"
    app = _app(tmp_path, **{"buffer.in_memory": 8})
    try:
        rest = _rest(app)
        assert rest.get("/api/v1/process/yard/objects").status_code == 404
        assert rest.post("/api/v1/process", json={"name": "yard", "rtsp_endpoint": url}).status_code == 200
        _first_frame(app.hub, "yard")
        app.hub.wait_frame("yard", 2, 5000)
        r = rest.get("/api/v1/process/yard/objects")
        assert r.status_code == 200 and r.json()["primed"] and r.json()["count"] >= len(r.json()["objects"])
        assert int(r.headers["X-Vep-Seq"]) == r.json()["seq"] == r.json()["prev_seq"] + 1
        assert rest.get(f"/api/v1/process/yard/objects?after={r.json()['seq'] + 1000}").status_code == 404
        cams = rest.get("/api/v1/objects?names=yard,yard&wake=0").json()["cameras"]
        assert [c["name"] for c in cams] == ["yard"] and cams[0]["seq"] >= r.json()["seq"]
        assert rest.get("/api/v1/process/yard/objects?wake=2").status_code == 400
        assert rest.get("/api/v1/objects?names=nope").status_code == 404
        text = rest.get("/metrics").text
        assert "vep_objects_evaluations_total{" in text and "vep_objects_frames_with_objects_total{" in text
    finally:
        app.stop()
    app = _app(tmp_path / "plain")  # buffer.in_memory 1: no earlier frame to compare with
    try:
        rest = _rest(app)
        assert rest.post("/api/v1/process", json={"name": "yard", "rtsp_endpoint": url}).status_code == 200
        _first_frame(app.hub, "yard")
        for path in ("/api/v1/process/yard/objects", "/api/v1/objects"):
            r = rest.get(path)
            assert r.status_code == 422 and "buffer.in_memory" in r.text, (path, r.text)
    finally:
        app.stop()
    assert objects.to_native() == objects.DEFAULTS == {k: getattr(Config().objects, k) for k in objects.DEFAULTS}
    for key, bad in (("decimate", 3), ("threshold", 256), ("gap", 0), ("open", 2), ("grow", 4), ("min_area", 3), ("max_objects", 1025),
                     ("grow", True), ("nope", 1)):
        with pytest.raises(ValueError, match="objects"):
            objects.to_native({key: bad})
    cfg = Config()
    cfg.objects.grow = 9
    with pytest.raises(ValueError, match="objects"):
        validate(cfg)
    a = cli.build_parser().parse_args(["objects", "--device", "yard", "--watch", "--as-crop-boxes"])
    assert a.fn is cli.cmd_objects and a.watch and a.as_crop_boxes and a.rest == "127.0.0.1:8080"
    answer = {"seq": 7, "primed": True, "motion": True, "count": 3, "area": 50, "truncated": True, "width": 300, "height": 200,
              "objects": [{"label": 1, "area": 40, "box": [30, 20, 31, 101]}]}
    assert cli.format_objects(answer) == "seq 7 OBJECTS count 3 area 50 boxes 30,20 31x101 +"
    assert objects.crop_boxes(answer) == ["1000,1000,2034,6050"]
