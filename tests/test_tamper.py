"""Tamper detection on the host: the CPU twin (csrc/vep/tamper.cpp) against the independent oracle
(tests/tamper_oracle.py), closed forms, the summary's threshold edges, the CPU-backend Worker and
Hub paths against the oracle applied to the frames they served, the REST routes, the config section
and the CLI parser. Everything is exact. The GPU paths are held to the same CPU functions in
tests/test_gpu_tamper.py."""
import time

import numpy as np
import pytest

import tamper_oracle as to
from conftest import synth

# picture (w, h), cell: one partial cell, partial right / bottom cells, an exact grid, cells that
# are no multiple of 8, single rows and columns, one cell wider than the picture
SHAPES = [((7, 5), 8), ((17, 9), 8), ((33, 17), 16), ((64, 48), 16), ((50, 30), 12), ((50, 30), 20), ((200, 120), 32),
          ((1, 9), 8), ((9, 1), 8), ((300, 3), 128)]


def check_stats(native, p, cell):
    got = native.tamper_stats_cpu(p, cell)
    want = to.stats(p, cell)
    h, w = p.shape[:2]
    assert all(g.dtype == np.uint32 for g in got)
    assert got[0].shape == (256,) and got[1].shape == got[2].shape == tuple(reversed(native.tamper_grid(w, h, cell)))
    for g, x, name in zip(got, want, ("hist", "sum_y", "energy")):
        assert np.array_equal(g, x), name
    return got


# ------------------------------------------------------------------------------ the statistics

@pytest.mark.parametrize("size,cell", SHAPES)
@pytest.mark.parametrize("kind", to.KINDS)
def test_stats_equal_oracle(native, size, cell, kind):
    w, h = size
    hist, sum_y, energy = check_stats(native, to.picture(kind, w, h, 1), cell)
    assert hist.sum() == w * h


def test_stats_equal_oracle_1080p(native):
    got = check_stats(native, to.picture("noise", 1920, 1080, 1), 32)
    assert got[1].shape == (34, 60)  # 33.75 cell rows


@pytest.mark.parametrize("size,cell", [((1100, 140), 127), ((100, 40), 9), ((530, 70), 66), ((2049, 33), 32)])
def test_stats_equal_oracle_odd_cells(native, size, cell):
    """The shapes tests/test_gpu_tamper.py adds for the kernel's column splits and wide chunks."""
    for kind in ("noise", "checker"):
        check_stats(native, to.picture(kind, *size, 2), cell)


@pytest.mark.parametrize("v", [0, 77, 255])
def test_uniform_grey(native, v):
    w, h, cell = 50, 30, 20
    hist, sum_y, energy = native.tamper_stats_cpu(to.grey(v, w, h), cell)
    assert hist[v] == w * h and hist.sum() == w * h
    assert not energy.any()
    pixels = np.array([[20 * 20, 20 * 20, 10 * 20], [20 * 10, 20 * 10, 10 * 10]])
    assert np.array_equal(sum_y, v * pixels)


def test_largest_cell_value(native):
    """The 128 x 128 checkerboard at cell 128: every one of the 2 * 128 * 127 pairs is 255^2."""
    hist, sum_y, energy = native.tamper_stats_cpu(to.picture("checker", 128, 128), 128)
    assert energy.shape == (1, 1) and int(energy[0, 0]) == 2114092800 == 2 * 128 * 127 * 255 * 255
    assert int(sum_y[0, 0]) == 64 * 128 * 255 and hist[0] == hist[255] == 64 * 128


def test_stripes_pair_directions(native):
    w, h, cell = 64, 48, 16
    _, _, ev = native.tamper_stats_cpu(to.picture("vstripes", w, h), cell)
    assert (ev == 15 * 16 * 65025).all()  # horizontal pairs only: 15 per row of a cell, 16 rows
    _, _, eh = native.tamper_stats_cpu(to.picture("hstripes", w, h), cell)
    assert (eh == 16 * 15 * 65025).all()  # vertical pairs only
    # partial cells tell the two directions apart: 40 x 20 at cell 16 has cells of 16 and 8 columns, 16 and 4 rows
    _, _, ev = native.tamper_stats_cpu(to.picture("vstripes", 40, 20), 16)
    assert np.array_equal(ev, 65025 * np.array([[15 * 16, 15 * 16, 7 * 16], [15 * 4, 15 * 4, 7 * 4]]))
    _, _, eh = native.tamper_stats_cpu(to.picture("hstripes", 40, 20), 16)
    assert np.array_equal(eh, 65025 * np.array([[16 * 15, 16 * 15, 8 * 15], [16 * 3, 16 * 3, 8 * 3]]))


def test_no_pair_crosses_a_cell(native):
    """Two cells side by side (and two above each other) whose only edge lies on the boundary."""
    plane = np.zeros((16, 32), dtype=np.uint8)
    plane[:, 16:] = 255
    _, sum_y, energy = native.tamper_stats_cpu(to.levels(plane), 16)
    assert not energy.any() and sum_y.tolist() == [[0, 16 * 16 * 255]]
    _, _, energy = native.tamper_stats_cpu(to.levels(plane.T), 16)
    assert energy.shape == (2, 1) and not energy.any()
    plane[:, 15] = 255  # one column earlier: 16 pairs inside the left cell
    _, _, energy = native.tamper_stats_cpu(to.levels(plane), 16)
    assert energy.tolist() == [[16 * 65025, 0]]


def test_stats_argument_checks(native):
    p = to.grey(1, 16, 16)
    for cell in (7, 129, 0, -8):
        with pytest.raises(Exception):
            native.tamper_stats_cpu(p, cell)
        with pytest.raises(Exception):
            native.tamper_grid(16, 16, cell)
    with pytest.raises(Exception):
        native.tamper_stats_cpu(p[:, :, :2], 8)
    with pytest.raises(Exception):
        native.tamper_grid(0, 16, 8)
    assert native.tamper_grid(65535, 1, 8) == (8192, 1)


# ----------------------------------------------------------------------------------- the summary

def summary(native, p, params=None, reference=None):
    """native.tamper_summarize of the CPU twin's statistics, checked against the oracle's summary."""
    params = dict(params or {})
    cell = params.get("cell", 32)
    h, w = p.shape[:2]
    hist, sum_y, energy = native.tamper_stats_cpu(p, cell)
    got = native.tamper_summarize(hist, sum_y, energy, w, h, params, reference)
    assert got == to.summarize(hist, sum_y, energy, w, h, params, reference), (got, params)
    return got


def reference_of(native, p, cell=32):
    h, w = p.shape[:2]
    _, sum_y, energy = native.tamper_stats_cpu(p, cell)
    return (w, h, cell, sum_y, energy)


def test_summary_dark_and_bright_edges(native):
    for level in (0, 32, 255):
        for v, want in ((level - 1, True), (level, True), (level + 1, False)):
            if 0 <= v <= 255:
                assert summary(native, to.grey(v, 40, 24), {"dark_level": level})["dark"] is want, (level, v)
        for v, want in ((level - 1, False), (level, True), (level + 1, True)):
            if 0 <= v <= 255:
                assert summary(native, to.grey(v, 40, 24), {"bright_level": level})["bright"] is want, (level, v)
    # the comparison is on sums, not on a rounded mean: one pixel above the level decides
    plane = np.full((24, 40), 32, dtype=np.uint8)
    assert summary(native, to.levels(plane))["dark"] is True
    plane[3, 5] = 33
    s = summary(native, to.levels(plane))
    assert s["dark"] is False and s["mean_sum"] == 32 * 960 + 1 and s["causes"] == ["flat"]


def test_summary_percentiles_and_flat(native):
    # 1000 pixels, two levels: p5 and p95 move with the share of the lower level
    def two(n_low, lo=50, hi=150):
        plane = np.full(1000, hi, dtype=np.uint8)
        plane[:n_low] = lo
        return to.levels(plane.reshape(25, 40))

    assert [summary(native, two(n))[k] for n in (49, 50, 51) for k in ("p5", "p95")] == [150, 150, 50, 150, 50, 150]
    assert [summary(native, two(n))["p95"] for n in (949, 950, 951)] == [150, 50, 50]
    # flat: p95 - p5 < spread_min, at the level, one below and one above
    for hi, want in ((50 + 23, True), (50 + 24, False), (50 + 25, False)):
        s = summary(native, two(500, 50, hi))
        assert (s["p5"], s["p95"], s["flat"]) == (50, hi, want)
    assert summary(native, two(500, 50, 50), {"spread_min": 0})["flat"] is False  # 0: never flat
    assert summary(native, two(500, 0, 255), {"spread_min": 255})["flat"] is False
    assert summary(native, two(500, 0, 254), {"spread_min": 255})["flat"] is True


def test_summary_defocused_edges(native):
    ref_p = to.picture("noise", 400, 8, 7)
    ref = reference_of(native, ref_p, 8)
    e_ref = int(ref[4].sum())
    assert e_ref > 0
    # the edge in energies, e * 100 < 50 * e_ref: one below half the reference's, at it and one above
    hist, sum_y, energy = native.tamper_stats_cpu(ref_p, 8)
    for num, want in ((e_ref // 2 - 1, True), (e_ref // 2, e_ref % 2 == 1), (e_ref // 2 + 1, False)):
        en = np.zeros_like(energy)
        en[0, 0] = num
        got = native.tamper_summarize(hist, sum_y, en, 400, 8, {"cell": 8}, ref)
        assert got == to.summarize(hist, sum_y, en, 400, 8, {"cell": 8}, ref)
        assert got["defocused"] is want and got["energy_total"] == num
    en = np.zeros_like(energy)
    assert native.tamper_summarize(hist, sum_y, en, 400, 8, {"cell": 8, "focus_percent": 0}, ref)["defocused"] is False
    assert native.tamper_summarize(hist, sum_y, en, 400, 8, {"cell": 8, "focus_percent": 100}, ref)["defocused"] is True
    assert native.tamper_summarize(hist, sum_y, energy, 400, 8, {"cell": 8, "focus_percent": 100}, ref)["defocused"] is False
    assert native.tamper_summarize(hist, sum_y, en, 400, 8, {"cell": 8}, None)["defocused"] is False  # no reference


def test_summary_moved_edges_and_partial_cells(native):
    # 40 x 24 at cell 16: cells of 16x16, 16x16, 8x16 over 16x8, 16x8, 8x8 pixels
    w, h, cell = 40, 24, 16
    base = to.grey(100, w, h)
    ref = reference_of(native, base, cell)
    prm = {"cell": cell, "shift_level": 24, "shift_percent": 50}

    def lifted(cells_up, delta):
        p = base.copy()
        for gx, gy in cells_up:
            p[gy * 16:(gy + 1) * 16, gx * 16:(gx + 1) * 16] = 100 + delta
        return p

    # a cell is shifted when |sum - ref| > shift_level * its TRUE pixel count: the 8 x 8 corner cell
    for delta, want in ((23, 0), (24, 0), (25, 1)):
        assert summary(native, lifted([(2, 1)], delta), prm, ref)["shifted"] == want
    # against the full cell size the corner cell would need 4 x the difference: 25 levels do it
    p = base.copy()
    p[16:24, 32:40] = 75  # downwards counts too
    assert summary(native, p, prm, ref)["shifted"] == 1
    # moved: shifted * 100 >= shift_percent * cells, 6 cells: 2, 3 and 4 shifted at 50 %
    for cells_up, want in (([(0, 0), (1, 0)], False), ([(0, 0), (1, 0), (2, 0)], True),
                           ([(0, 0), (1, 0), (2, 0), (0, 1)], True)):
        s = summary(native, lifted(cells_up, 60), prm, ref)
        assert (s["shifted"], s["cells"], s["moved"]) == (len(cells_up), 6, want)
    assert summary(native, lifted([(0, 0)], 60), dict(prm, shift_percent=16), ref)["moved"] is True  # 100 >= 96
    assert summary(native, lifted([(0, 0)], 60), dict(prm, shift_percent=17), ref)["moved"] is False  # 100 < 102
    s = summary(native, lifted([(0, 0), (1, 0), (2, 0)], 60), prm, ref)
    assert s["tampered"] is True and s["causes"] == ["moved"] and s["has_reference"] is True
    # pairs of partial cells: (cw - 1) * ch + cw * (ch - 1) over the six cells
    assert s["pairs_total"] == 2 * (15 * 16 + 16 * 15) + (7 * 16 + 8 * 15) + 2 * (15 * 8 + 16 * 7) + (7 * 8 + 8 * 7)


def test_summary_drops_a_foreign_reference(native):
    p = to.picture("noise", 64, 48, 1)
    other = to.picture("noise", 64, 48, 2) // 4
    ref = reference_of(native, other, 16)
    assert summary(native, p, {"cell": 16}, ref)["has_reference"] is True
    for bad in ((48, 64, 16), (64, 48, 32), (65, 48, 16)):
        s = summary(native, p, {"cell": 16}, bad + ref[3:])
        assert s["has_reference"] is False and not s["moved"] and not s["defocused"] and s["shifted"] == 0
    for bad in ({"cell": 7}, {"dark_level": 256}, {"bright_level": -1}, {"spread_min": 256}, {"focus_percent": 101},
                {"shift_level": 256}, {"shift_percent": 0}, {"shift_percent": 101}, {"nope": 1}):
        with pytest.raises(Exception):
            summary(native, p, bad)


def test_scenarios_against_a_reference(native):
    """A noise-plus-gradient scene declared normal: blurred, rolled, black, and itself."""
    w, h = 320, 240
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(5)
    scene = to.levels(np.clip(40 + x // 2 + rng.integers(0, 60, (h, w)), 0, 255))
    ref = reference_of(native, scene)
    s = summary(native, scene, None, ref)
    assert s["tampered"] is False and s["causes"] == [] and s["has_reference"] and s["shifted"] == 0
    assert summary(native, scene)["tampered"] is False  # nor without the reference
    blurred = summary(native, to.box_blur(scene, 5), None, ref)
    assert blurred["defocused"] is True and blurred["causes"] == ["defocused"]
    rolled = summary(native, np.ascontiguousarray(np.roll(scene, w // 2, axis=1)), None, ref)
    assert rolled["moved"] is True and rolled["causes"] == ["moved"]
    black = summary(native, to.grey(0, w, h), None, ref)
    assert black["dark"] and black["flat"] and black["tampered"] and black["causes"][:2] == ["dark", "flat"]
    assert black["sharpness"] == 0.0 and black["mean"] == 0.0


# ------------------------------------------------------------------------ CPU-backend Worker

def _feed(native, wk, name, w, h, frames=1, **kw):
    enc = synth(native, w, h, gop=6, motion=0.2, **kw)
    cam = wk.add_camera(name, 2)
    for _ in range(frames):
        assert wk.decode_now(cam, enc.next())
    return cam, enc


def _expect(frame, prm, seq, ref=None):
    """The dict Worker.read_tamper owes for `frame`, from the oracle; and the frame's reference."""
    h, w = frame.shape[:2]
    hist, sum_y, energy = to.stats(frame, prm["cell"])
    cols, rows = to.grid(w, h, prm["cell"])
    want = to.summarize(hist, sum_y, energy, w, h, prm, ref)
    want.update(seq=seq, width=w, height=h, cell=prm["cell"], cols=cols, rows=rows)
    return want, (hist, sum_y, energy), (w, h, prm["cell"], sum_y, energy)


def _same(got, want, planes):
    assert got is not None
    g = dict(got)
    for name, p in zip(("hist", "sum_y", "energy"), planes):
        assert np.array_equal(g.pop(name), p), name
    assert g == want, (g, want)


DEFAULTS = {"cell": 32, "dark_level": 32, "bright_level": 224, "spread_min": 24, "focus_percent": 50,
            "shift_level": 24, "shift_percent": 50}


def test_worker_tamper_cpu_backend(native):
    wk = native.Worker(device=-1)
    prm = wk.tamper_params
    assert prm == DEFAULTS
    cam, enc = _feed(native, wk, "c", 320, 240)
    m0, f0 = wk.read_latest(cam, 0)
    r0 = wk.read_tamper(cam, 0)
    want0, planes0, ref0 = _expect(f0, prm, m0["seq"])
    _same(r0, want0, planes0)
    assert r0["has_reference"] is False
    assert wk.stats(cam)["tamper_evaluations"] == 1
    # the same seq again: the stored answer, no second evaluation
    _same(wk.read_tamper(cam, 0), want0, planes0)
    assert wk.stats(cam)["tamper_evaluations"] == 1
    assert wk.read_tamper(cam, m0["seq"]) is None  # after = seq: nothing newer
    # this frame becomes the reference: no new evaluation, the stored answer now compares with it
    assert wk.tamper_set_reference(cam) is True
    want0r, _, _ = _expect(f0, prm, m0["seq"], ref0)
    _same(wk.read_tamper(cam, 0), want0r, planes0)
    assert want0r["has_reference"] and wk.stats(cam)["tamper_evaluations"] == 1
    # a second frame against the reference
    assert wk.decode_now(cam, enc.next())
    m1, f1 = wk.read_latest(cam, 0)
    assert m1["seq"] > m0["seq"]
    want1, planes1, ref1 = _expect(f1, prm, m1["seq"], ref0)
    _same(wk.read_tamper(cam, m0["seq"]), want1, planes1)
    st = wk.stats(cam)
    assert st["tamper_evaluations"] == 2
    assert st["tamper_frames_tampered"] == int(want0["tampered"]) + int(want1["tampered"])
    # the reset drops the reference and the stored answer: the same frame is evaluated again
    wk.tamper_reset(cam)
    want1n, _, _ = _expect(f1, prm, m1["seq"])
    _same(wk.read_tamper(cam, 0), want1n, planes1)
    assert wk.stats(cam)["tamper_evaluations"] == 3
    # a reference set without an earlier evaluation evaluates the newest frame itself
    wk.tamper_reset(cam)
    assert wk.tamper_set_reference(cam) is True and wk.stats(cam)["tamper_evaluations"] == 4
    _same(wk.read_tamper(cam, 0), _expect(f1, prm, m1["seq"], ref1)[0], planes1)
    empty = wk.add_camera("e", 2)
    assert wk.read_tamper(empty, 0) is None and wk.tamper_set_reference(empty) is False
    for call in (lambda: wk.read_tamper(99, 0), lambda: wk.tamper_reset(99), lambda: wk.tamper_set_reference(99)):
        with pytest.raises(Exception):
            call()


def test_worker_tamper_params(native):
    wk = native.Worker(device=-1)
    cam, enc = _feed(native, wk, "c", 160, 96)
    assert wk.read_tamper(cam, 0)["cell"] == 32 and wk.tamper_set_reference(cam)
    # the same cell: the stored answer goes, the reference stays
    wk.set_tamper_params(32, 10, 200, 30, 60, 12, 40)
    prm = wk.tamper_params
    assert prm == {"cell": 32, "dark_level": 10, "bright_level": 200, "spread_min": 30, "focus_percent": 60,
                   "shift_level": 12, "shift_percent": 40}
    m0, f0 = wk.read_latest(cam, 0)
    ref = _expect(f0, prm, m0["seq"])[2]
    want, planes, _ = _expect(f0, prm, m0["seq"], ref)
    _same(wk.read_tamper(cam, 0), want, planes)
    assert want["has_reference"] and wk.stats(cam)["tamper_evaluations"] == 2
    # another cell: the reference is dropped with the answer
    wk.set_tamper_params(cell=8)
    prm = wk.tamper_params
    assert prm == dict(DEFAULTS, cell=8)
    want, planes, _ = _expect(f0, prm, m0["seq"])
    _same(wk.read_tamper(cam, 0), want, planes)
    assert want["has_reference"] is False and (want["cols"], want["rows"]) == (20, 12)
    for bad in [(7,), (129,), (32, -1), (32, 256), (32, 32, -1), (32, 32, 256), (32, 32, 224, -1), (32, 32, 224, 256),
                (32, 32, 224, 24, -1), (32, 32, 224, 24, 101), (32, 32, 224, 24, 50, -1), (32, 32, 224, 24, 50, 256),
                (32, 32, 224, 24, 50, 24, 0), (32, 32, 224, 24, 50, 24, 101)]:
        with pytest.raises(Exception):
            wk.set_tamper_params(*bad)
    assert wk.tamper_params == prm  # a refused call changes nothing
    wk.set_tamper_params(128, 0, 255, 255, 0, 255, 100)  # every edge of the ranges
    wk.set_tamper_params(8, 255, 0, 0, 100, 0, 1)


def test_worker_tamper_many_cpu_backend(native):
    wk = native.Worker(device=-1)
    prm = wk.tamper_params
    a, enc_a = _feed(native, wk, "a", 320, 240)
    b, enc_b = _feed(native, wk, "b", 160, 96, seed=5)
    empty = wk.add_camera("e", 2)
    fa, fb = wk.read_latest(a, 0), wk.read_latest(b, 0)
    rs = wk.read_tamper_many([a, b, empty, 77, b])
    assert len(rs) == 5 and rs[2] is None and rs[3] is None
    wa, pa, _ = _expect(fa[1], prm, fa[0]["seq"])
    wb, pb, _ = _expect(fb[1], prm, fb[0]["seq"])
    _same(rs[0], wa, pa)
    _same(rs[1], wb, pb)
    _same(rs[4], wb, pb)  # a camera named twice is evaluated once
    assert wk.stats(b)["tamper_evaluations"] == 1
    assert wk.decode_now(a, enc_a.next())  # only a moves on: b answers from its store
    fa = wk.read_latest(a, 0)
    rs = wk.read_tamper_many([b, a])
    wa, pa, _ = _expect(fa[1], prm, fa[0]["seq"])
    _same(rs[1], wa, pa)
    _same(rs[0], wb, pb)
    assert wk.stats(a)["tamper_evaluations"] == 2 and wk.stats(b)["tamper_evaluations"] == 1
    assert wk.read_tamper_many([]) == []
    wk.remove_camera(a)
    assert wk.read_tamper_many([a, b])[0] is None


# ----------------------------------------------------------------------------------- Hub

class _NoSession:
    def stop(self):
        pass


KEYS = {"seq", "width", "height", "cell", "cols", "rows", "mean", "p5", "p95", "sharpness", "has_reference", "shifted",
        "dark", "bright", "flat", "defocused", "moved", "tampered", "causes"}


def _hub_view(want):
    return {k: want[k] for k in KEYS}


def test_hub_tamper_across_two_workers(native, tmp_path):
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, CameraNotFound, Hub

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    cfg.tamper.cell, cfg.tamper.spread_min, cfg.tamper.shift_percent = 16, 10, 30
    hub = Hub(cfg, devices=[-1, -1])
    try:
        prm = dict(DEFAULTS, cell=16, spread_min=10, shift_percent=30)
        assert all(w.tamper_params == prm for w in hub.workers)  # the section reaches every worker
        encs = {}
        for k, (name, w, h) in enumerate([("cam_a", 320, 240), ("cam_b", 160, 96), ("cam_c", 320, 176)]):
            wi = k % 2
            cam, encs[name] = _feed(native, hub.workers[wi], name, w, h, seed=k + 1)
            hub.cameras[name] = CameraHandle(name, wi, cam, "", session=_NoSession())
        # wake=False evaluates what the ring holds and leaves last_query alone
        quiet = hub.tamper_many(wake=False)
        assert list(quiet) == ["cam_a", "cam_b", "cam_c"] and all(set(r) == KEYS for r in quiet.values())
        assert hub.tamper("cam_a", wake=False) == quiet["cam_a"]
        for h in hub.cameras.values():
            assert hub.workers[h.worker_index].last_query(h.cam) == 0
        assert hub.tamper("cam_a") == quiet["cam_a"] and hub.workers[0].last_query(hub.cameras["cam_a"].cam) > 0
        hub.tamper_many(["cam_b"])
        assert hub.workers[1].last_query(hub.cameras["cam_b"].cam) > 0
        assert hub.workers[0].last_query(hub.cameras["cam_c"].cam) == 0
        assert hub.tamper_reference("cam_a") is True and hub.tamper_reference("cam_c") is True
        refs = {}
        for name, h in hub.cameras.items():
            wk = hub.workers[h.worker_index]
            meta, frame = wk.read_latest(h.cam, 0)
            refs[name] = _expect(frame, prm, meta["seq"])[2] if name != "cam_b" else None
            assert wk.decode_now(h.cam, encs[name].next())
        got = hub.tamper_many(["cam_c", "cam_a", "cam_b"], grid=True)
        assert list(got) == ["cam_c", "cam_a", "cam_b"]
        for name, h in hub.cameras.items():
            meta, frame = hub.workers[h.worker_index].read_latest(h.cam, 0)
            want, planes, _ = _expect(frame, prm, meta["seq"], refs[name])
            r = dict(got[name])
            for key, p in zip(("hist", "sum_y", "energy"), planes):
                assert r.pop(key) == p.tolist()
            assert r == _hub_view(want) and r["has_reference"] is (name != "cam_b")
            assert hub.tamper(name) == r and hub.tamper(name, grid=True)["sum_y"] == planes[1].tolist()
            assert hub.tamper(name, after=meta["seq"]) is None
            assert hub.workers[h.worker_index].stats(h.cam)["tamper_evaluations"] == 2
        hub.tamper_reset("cam_a")
        assert hub.tamper("cam_a")["has_reference"] is False
        with pytest.raises(CameraNotFound):
            hub.tamper("nope")
        with pytest.raises(CameraNotFound):
            hub.tamper_many(["cam_a", "nope"])
        with pytest.raises(CameraNotFound):
            hub.tamper_reference("nope")
        with pytest.raises(CameraNotFound):
            hub.tamper_reset("nope")
    finally:
        hub.shutdown()


def test_process_hub_forwards_tamper():
    from video_edge_ai_proxy_amd.engine.child import EXPORTED
    from video_edge_ai_proxy_amd.engine.isolated import ProcessHub

    assert {"tamper", "tamper_reference", "tamper_reset"} <= EXPORTED

    class Fake:
        cameras = {"b": 1, "a": 2}
        calls = []

        def handle(self, name):
            return self.cameras[name]

        def _call(self, name, method, *args):
            self.calls.append((name, method, args))
            return {"seq": 3}

    f = Fake()
    assert ProcessHub.tamper(f, "a", 2, True, False) == {"seq": 3} and f.calls[-1] == ("a", "tamper", (2, True, False))
    assert ProcessHub.tamper_many(f, wake=False) == {"a": {"seq": 3}, "b": {"seq": 3}}  # per name, sorted
    assert f.calls[1:] == [("a", "tamper", (0, False, False)), ("b", "tamper", (0, False, False))]
    assert ProcessHub.tamper_reference(f, "b") is True and f.calls[-1] == ("b", "tamper_reference", ())
    ProcessHub.tamper_reset(f, "b")
    assert f.calls[-1] == ("b", "tamper_reset", ())
    with pytest.raises(KeyError):
        ProcessHub.tamper_many(f, ["a", "nope"])


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


def test_rest_tamper(native, farm, hubapp):
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle

    rest = _rest(hubapp)
    assert rest.get("/api/v1/tamper").status_code == 404  # no camera running
    assert rest.get("/api/v1/process/nope/tamper").status_code == 404
    assert rest.put("/api/v1/process/nope/tamper/reference").status_code == 404
    assert rest.delete("/api/v1/process/nope/tamper").status_code == 404
    _start_camera(rest, farm, "front_door", "/cam")
    _start_camera(rest, farm, "back_yard", "/wide")
    r = _poll(rest, "/api/v1/process/front_door/tamper")
    first = r.json()
    assert set(first) == KEYS and int(r.headers["x-vep-seq"]) == first["seq"] >= 1
    assert (first["width"], first["height"], first["cell"], first["cols"], first["rows"]) == (320, 240, 32, 10, 8)
    assert first["has_reference"] is False and first["tampered"] is bool(first["causes"])
    # grid=1 adds the histogram and the planes, which carry the summary
    g = rest.get("/api/v1/process/front_door/tamper?grid=1&wake=0").json()
    assert set(g) == KEYS | {"hist", "sum_y", "energy"} and g["seq"] >= first["seq"]
    assert len(g["hist"]) == 256 and sum(g["hist"]) == 320 * 240
    assert len(g["sum_y"]) == len(g["energy"]) == 8 and all(len(row) == 10 for row in g["sum_y"] + g["energy"])
    assert g["mean"] == sum(map(sum, g["sum_y"])) / (320 * 240)
    published = hubapp.hub.published("front_door")
    assert rest.get(f"/api/v1/process/front_door/tamper?after={published + 1000}").status_code == 404
    # the reference: 204, and the next answers compare with it
    assert rest.put("/api/v1/process/front_door/tamper/reference").status_code == 204
    assert rest.get("/api/v1/process/front_door/tamper").json()["has_reference"] is True
    # every camera, in request order; one without a frame has seq 0 and cannot take a reference
    _poll(rest, "/api/v1/process/back_yard/tamper")
    idle = hubapp.hub.workers[0].add_camera("idle_cam", 2)
    hubapp.hub.cameras["idle_cam"] = CameraHandle("idle_cam", 0, idle, "", session=_NoSession())
    try:
        assert rest.put("/api/v1/process/idle_cam/tamper/reference").status_code == 404
        cams = rest.get("/api/v1/tamper?names=idle_cam,front_door,back_yard&wake=0").json()["cameras"]
        assert [c["name"] for c in cams] == ["idle_cam", "front_door", "back_yard"]
        assert cams[0] == {"name": "idle_cam", "seq": 0, "tampered": False, "causes": []}
        assert all(set(c) == KEYS | {"name"} and c["seq"] >= 1 for c in cams[1:])
        assert cams[1]["has_reference"] is True and cams[2]["has_reference"] is False
        cams = rest.get("/api/v1/tamper?grid=1").json()["cameras"]
        assert [c["name"] for c in cams] == ["back_yard", "front_door", "idle_cam"]  # default: sorted
        assert "hist" in cams[0] and "energy" in cams[1]
    finally:
        hubapp.hub.cameras.pop("idle_cam")
        hubapp.hub.workers[0].remove_camera(idle)
    assert rest.get("/api/v1/tamper?names=front_door,nope").status_code == 404
    for bad in ("/api/v1/tamper?names=,", "/api/v1/tamper?grid=2", "/api/v1/tamper?wake=2",
                "/api/v1/process/front_door/tamper?grid=7", "/api/v1/process/front_door/tamper?wake=-1",
                "/api/v1/process/front_door/tamper?after=-1"):
        assert rest.get(bad).status_code == 400, bad
    # the reset: 204, and the reference is gone
    assert rest.delete("/api/v1/process/front_door/tamper").status_code == 204
    assert rest.get("/api/v1/process/front_door/tamper").json()["has_reference"] is False
    # /metrics counts evaluations per camera
    text = rest.get("/metrics").text
    line = [ln for ln in text.splitlines() if ln.startswith("vep_tamper_evaluations_total{") and "front_door" in ln]
    assert len(line) == 1 and float(line[0].rsplit(" ", 1)[1]) >= 2
    assert "vep_tamper_frames_tampered_total{" in text
    # existing routes answer as before
    assert rest.get("/api/v1/process/front_door/motion").status_code == 200
    assert rest.get("/api/v1/process/front_door").status_code == 200


def test_config_tamper(tmp_path):
    from video_edge_ai_proxy_amd.config import load_config

    cfg = load_config(data_dir=str(tmp_path))
    t = cfg.tamper
    assert {k: getattr(t, k) for k in DEFAULTS} == DEFAULTS
    (tmp_path / "conf.yaml").write_text(
        "tamper:\n  cell: 64\n  dark_level: 10\n  bright_level: 240\n  spread_min: 12\n  focus_percent: 0\n"
        "  shift_level: 30\n  shift_percent: 75\n")
    t = load_config(data_dir=str(tmp_path)).tamper
    assert (t.cell, t.dark_level, t.bright_level, t.spread_min, t.focus_percent, t.shift_level, t.shift_percent) == (
        64, 10, 240, 12, 0, 30, 75)
    for bad in ("cell: 7", "cell: 129", "dark_level: -1", "dark_level: 256", "bright_level: -1", "bright_level: 256",
                "spread_min: -1", "spread_min: 256", "focus_percent: -1", "focus_percent: 101", "shift_level: -1",
                "shift_level: 256", "shift_percent: 0", "shift_percent: 101", "cell: wide", "cell: true"):
        (tmp_path / "conf.yaml").write_text(f"tamper:\n  {bad}\n")
        with pytest.raises(ValueError):
            load_config(data_dir=str(tmp_path))
    for edge in ("cell: 8", "cell: 128", "dark_level: 0", "bright_level: 255", "spread_min: 0", "focus_percent: 100",
                 "shift_level: 255", "shift_percent: 1", "shift_percent: 100"):
        (tmp_path / "conf.yaml").write_text(f"tamper:\n  {edge}\n")
        load_config(data_dir=str(tmp_path))


def test_cli_tamper_parser():
    from video_edge_ai_proxy_amd import cli

    a = cli.build_parser().parse_args(["tamper", "--device", "front_door"])
    assert (a.cmd, a.device, a.rest, a.watch, a.set_reference, a.fn) == (
        "tamper", "front_door", "127.0.0.1:8080", False, False, cli.cmd_tamper)
    a = cli.build_parser().parse_args(["tamper", "--device", "d", "--rest", "hub:9000", "--watch", "--set-reference",
                                       "--interval", "0.5"])
    assert (a.rest, a.watch, a.set_reference, a.interval) == ("hub:9000", True, True, 0.5)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["tamper"])  # --device is required
    line = cli.format_tamper({"seq": 7, "tampered": True, "causes": ["dark", "flat"], "mean": 3.25, "p5": 0, "p95": 9,
                              "sharpness": 1.5, "has_reference": True, "shifted": 4})
    assert line == "seq 7 TAMPERED dark,flat mean 3.2 p5 0 p95 9 sharpness 1.5 shifted 4"
    line = cli.format_tamper({"seq": 8, "tampered": False, "causes": [], "mean": 120.0, "p5": 40, "p95": 200,
                              "sharpness": 310.04, "has_reference": False})
    assert line == "seq 8 ok mean 120.0 p5 40 p95 200 sharpness 310.0 no reference"
