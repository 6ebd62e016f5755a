"""The H.265 loop filters at picture level against the spec oracle (tests/spec_oracle_hevc.py:
boundary_strengths, deblock_picture, sao_picture, written from H.265 8.7.2 / 8.7.3), on the
seeded pictures of tests/hevc_lf_cases.py. The CPU decoder, the records mirror, the kernels and
the closed-loop encoder share deblock_strengths / bs_of and finish_gpu_picture, so the stream tests
cannot see a wrong picture-level rule; here each of the three host paths is compared with the
oracle: the records mirror (hevc_loopfilter_records, device -1), the derivation of the records
from the parser's state (hevc_loopfilter_picture "strengths") and the CPU decoder's filters
("cpu"). The generator's coverage assertions (from the oracle's trace alone) and a few
hand-computed pictures that pin the oracle itself are here too. tests/test_gpu_hevc_loopfilter.py
runs the same cases through the kernels."""
from __future__ import annotations

import copy

import numpy as np
import pytest

import hevc_lf_cases as hc
import spec_oracle_hevc as so
from video_edge_ai_proxy_amd import native

PICS = hc.all_pictures()
TABLE = hc.bs_table()
BATCHES = hc.batch_cases()
_ids = [p["name"] for p in PICS]
_tids = [p["name"] for p in TABLE]


# ----------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("pic", PICS, ids=_ids)
def test_case_reaches_what_it_is_for(pic):
    tags = hc.coverage(hc.records_of(pic))
    missing = [t for t in pic["reach"] if t not in tags]
    assert not missing, f"{pic['name']} does not reach {missing}"


def test_cases_together_reach_every_branch():
    tags = set()
    for pic in PICS:
        tags |= hc.coverage(hc.records_of(pic))
    unreached = (hc.DEBLOCK_TAGS | hc.SAO_TAGS) - tags
    assert not unreached, sorted(map(str, unreached))


def test_chroma_sections_have_one_decision():
    """Each 4-line chroma section (8 luma lines) sees one bS 2 decision, QpY pair and exemption,
    as coding units of 8x8 and more guarantee: the oracle's section-wise reading of 8.7.2.5 and a
    reading per 4 luma lines then agree."""
    for pic in PICS:
        rec = hc.records_of(pic)
        w4 = rec["width"] // 4
        for d, m in ((0, rec["bs_v"]), (1, rec["bs_h"])):
            for b, v in enumerate(m):
                x4, y4 = b % w4, b // w4
                if (y4 if d == 0 else x4) % 2:
                    continue
                o = b + (w4 if d == 0 else 1)
                bp, op = (b - 1, o - 1) if d == 0 else (b - w4, o - w4)
                assert (v == 2) == (m[o] == 2), (pic["name"], d, b)
                if v == 2:
                    for k in ("qp", "pcm_map"):
                        assert rec[k][b] == rec[k][o] and rec[k][bp] == rec[k][op], (pic["name"], d, b, k)


@pytest.mark.parametrize("pic", TABLE, ids=_tids)
def test_bs_table_oracle_agrees_with_the_clause(pic):
    bs_v, bs_h = so.boundary_strengths(pic)
    w4 = pic["width"] // 4
    m, other = (bs_h, bs_v) if pic["horizontal"] else (bs_v, bs_h)
    for b, v in enumerate(m):
        at = 4 * (b // w4 if pic["horizontal"] else b % w4)
        assert v == (pic["want"] if at == pic["pos"] else 0), (pic["name"], b, v)
    assert not any(other)


# ----------------------------------------------------------------------------- the oracle itself
def _flat_rec(w=16, h=16, bd=8):
    n4, dt = (w // 4) * (h // 4), np.uint16 if bd > 8 else np.uint8
    st = hc.stride_of(w)
    return dict(name="hand", width=w, height=h, log2ctb=4, bd_y=bd, bd_c=bd, cb_qp_offset=0, cr_qp_offset=0,
                bs_v=[0] * n4, bs_h=[0] * n4, qp=[37] * n4, pcm_map=[0] * n4, pcm_nofilter=0, ctb_slice=[0], ctb_tile=[0],
                slices=[dict(beta_offset=0, tc_offset=0, across=1, sao_luma=1, sao_chroma=1)],
                sao_params=[dict(type=[0, 0, 0], band=[0, 0, 0], eo=[0, 0, 0], off=[[0] * 4 for _ in range(3)])],
                deblock=1, sao=0, tiles_block_sao=0, y=np.full((h, st), 100, dt), uv=np.full((h // 2, st), 128, dt))


def _hand_strong_edge():
    """p side 100, q side 104, bS 2, QpY 37 on both sides, no offsets, one 4-line segment at x = 8.
    Q = 37 + 2 * (bS - 1) = 39 -> tC' = 5; beta' (Q = 37) = 36. Both sides are flat: d = 0 < beta,
    2 * dpq = 0 < 9, |p3 - p0| + |q0 - q3| = 0 < 4, |p0 - q0| = 4 < (5 * 5 + 1) >> 1 = 13: strong.
      p0' = (100 + 200 + 200 + 208 + 104 + 4) >> 3 = 102   q0' = (100 + 200 + 208 + 208 + 104 + 4) >> 3 = 103
      p1' = (100 + 100 + 100 + 104 + 2) >> 2       = 101   q1' = (100 + 104 + 104 + 104 + 2) >> 2       = 103
      p2' = (200 + 300 + 100 + 100 + 104 + 4) >> 3 = 101   q2' = (100 + 104 + 104 + 312 + 208 + 4) >> 3 = 104
    all within +-2 tC of the input. x = 8 is off the chroma grid: chroma stays."""
    rec = _flat_rec()
    rec["y"][:, 8:16] = 104
    rec["bs_v"][2] = 2  # block (x4 = 2, y4 = 0)
    want_y = rec["y"].copy()
    want_y[0:4, 4:12] = [100, 101, 101, 102, 103, 103, 104, 104]
    return rec, want_y


def _hand_sao_corners(eo):
    """A flat picture (50) with local minima (40) in the four corners and at (5, 5); edge offsets
    (+5, 0, 0, 0). Every corner lacks one neighbour of every class (outside the picture:
    SaoOffsetVal[0] = 0 applies), so only (5, 5) moves, to 45; its neighbours see edgeIdx 3 (one
    neighbour lower, one equal), whose offset is 0."""
    rec = _flat_rec()
    rec.update(deblock=0, sao=1)
    rec["y"][:, :16] = 50
    for x, y in ((0, 0), (15, 0), (0, 15), (15, 15), (5, 5)):
        rec["y"][y, x] = 40
    rec["sao_params"][0].update(type=[2, 0, 0], eo=[eo, 0, 0], off=[[5, 0, 0, 0], [0] * 4, [0] * 4])
    want_y = rec["y"].copy()
    want_y[5, 5] = 45
    return rec, want_y


def _hand_sao_input_only():
    """Class 0 (left / right neighbours), SaoOffsetVal[1..4] = (+5, +7, 0, 0), a flat 50 with
      row 3: 50 40 50     -> edgeIdx = 2 - 1 - 1 = 0, remapped to 1: 40 + 5 = 45
      row 8: 50 40 40 50  -> each 40: 2 - 1 + 0 = 1, remapped to 2: 40 + 7 = 47
    and every 50 next to a 40 has edgeIdx 3 (offset 0). A filter that read its own output would
    give the second 40 of row 8 the neighbours 47 and 50: edgeIdx 0 -> 1, 45 instead of 47."""
    rec = _flat_rec()
    rec.update(deblock=0, sao=1)
    rec["y"][:, :16] = 50
    rec["y"][3, 4] = 40
    rec["y"][8, 4:6] = 40
    rec["sao_params"][0].update(type=[2, 0, 0], eo=[0, 0, 0], off=[[5, 7, 0, 0], [0] * 4, [0] * 4])
    want_y = rec["y"].copy()
    want_y[3, 4] = 45
    want_y[8, 4:6] = 47
    return rec, want_y


HAND = {"strong_edge": _hand_strong_edge, "sao_input_only": _hand_sao_input_only,
        **{f"sao_corners_eo{eo}": (lambda eo=eo: _hand_sao_corners(eo)) for eo in range(4)}}


@pytest.mark.parametrize("name", HAND)
def test_hand_computed_picture_pins_the_oracle(name):
    rec, want_y = HAND[name]()
    got = hc.oracle_filter(rec)
    assert np.array_equal(got[0], want_y) and np.array_equal(got[1], rec["uv"])


@pytest.mark.parametrize("name", HAND)
def test_hand_computed_picture_records_mirror(name):
    rec, want_y = HAND[name]()
    got = native.hevc_loopfilter_records([rec], -1)[0]
    assert np.array_equal(got[0], want_y) and np.array_equal(got[1], rec["uv"])


# ----------------------------------------------------------------------------- host paths
def _check_records(rec, got):
    msg = hc.explain(rec, got, hc.oracle_cached(rec))
    assert msg is None, msg


@pytest.mark.parametrize("pic", PICS + TABLE, ids=_ids + _tids)
def test_records_mirror_equals_oracle(pic):
    rec = hc.records_of(pic)
    _check_records(rec, native.hevc_loopfilter_records([rec], -1)[0])


@pytest.mark.parametrize("name,recs", BATCHES, ids=[b[0] for b in BATCHES])
def test_records_mirror_batches(name, recs):
    got = native.hevc_loopfilter_records(recs, -1)
    assert len(got) == len(recs)
    for rec, g in zip(recs, got):
        _check_records(rec, g)
    last = recs[-1]  # both filters off: returned as given
    assert np.array_equal(got[-1][0], last["y"]) and np.array_equal(got[-1][1], last["uv"])


@pytest.mark.parametrize("pic", PICS + TABLE, ids=_ids + _tids)
def test_host_strengths_and_derived_records(pic):
    got = native.hevc_loopfilter_picture(pic, -1, "strengths")
    want = hc.records_of(pic)
    w4 = pic["width"] // 4
    for k in ("bs_v", "bs_h"):
        diff = [(b % w4 * 4, b // w4 * 4, g, w) for b, (g, w) in enumerate(zip(got[k], want[k])) if g != w]
        assert not diff, f"{pic['name']}: {k} differs at (x, y, got, oracle) {diff[:5]}"
    for k in ("qp", "ctb_slice", "ctb_tile", "slices", "deblock", "sao", "tiles_block_sao"):
        assert got[k] == want[k], (pic["name"], k)
    assert got["sao_params"] == [dict(p) for p in want["sao_params"]], pic["name"]
    assert [int(got["pcm_nofilter"] and m) for m in got["pcm_map"]] == want["pcm_map"], pic["name"]


@pytest.mark.parametrize("pic", PICS + TABLE, ids=_ids + _tids)
def test_cpu_decoder_filters_equal_oracle(pic):
    _check_records(hc.records_of(pic), native.hevc_loopfilter_picture(pic, -1, "cpu"))


@pytest.mark.parametrize("pic", PICS[:3] + PICS[-3:], ids=_ids[:3] + _ids[-3:])
def test_records_path_from_the_parser_state(pic):
    _check_records(hc.records_of(pic), native.hevc_loopfilter_picture(pic, -1, "records"))


# ----------------------------------------------------------------------------- validation
def _pic(name):
    return next(p for p in PICS if p["name"] == name)


def _rec():
    return copy.deepcopy(hc.records_of(_pic("72x40_ctb32_bd8_s4")))  # 18 x 10 blocks, 3 x 2 CTBs


def _set(path, value):
    def f(r):
        o = r
        for k in path[:-1]:
            o = o[k]
        o[path[-1]] = value
    return f


BAD_RECORDS = {
    "width_not_multiple_of_8": _set(["width"], 68),
    "height_zero": _set(["height"], 0),
    "width_above_the_surfaces": _set(["width"], 8200),
    "log2ctb_3": _set(["log2ctb"], 3),
    "log2ctb_7": _set(["log2ctb"], 7),
    "bs_3": _set(["bs_v", 2], 3),
    "bs_off_the_grid": _set(["bs_v", 1], 1),
    "bs_h_off_the_grid": _set(["bs_h", 18], 2),
    "bs_at_the_left_border": _set(["bs_v", 0], 2),
    "bs_at_the_top_border": _set(["bs_h", 4], 1),
    "ctb_slice_names_no_slice": _set(["ctb_slice", 5], 1),
    "ctb_tile_above_the_ctb_count": _set(["ctb_tile", 0], 6),
    "sao_type_3": _set(["sao_params", 0, "type"], [3, 0, 0]),
    "sao_eo_4": _set(["sao_params", 1, "eo"], [0, 4, 4]),
    "sao_band_32": _set(["sao_params", 2, "band"], [0, 0, 32]),
    "sao_offset_8_at_8_bits": _set(["sao_params", 0, "off"], [[8, 0, 0, 0], [0] * 4, [0] * 4]),
    "sao_offset_minus_8_at_8_bits": _set(["sao_params", 0, "off"], [[0] * 4, [0] * 4, [0, 0, 0, -8]]),
    "qp_52": _set(["qp", 7], 52),
    "qp_negative_at_8_bits": _set(["qp", 7], -1),
    "beta_offset_14": _set(["slices", 0, "beta_offset"], 14),
    "bd_y_differs_from_bd_c": _set(["bd_c"], 10),
    "bd_11": lambda r: r.update(bd_y=11, bd_c=11),
    "qp_too_short": lambda r: r["qp"].pop(),
    "bs_v_too_long": lambda r: r["bs_v"].append(0),
    "ctb_slice_too_short": lambda r: r["ctb_slice"].pop(),
    "sao_params_too_short": lambda r: r["sao_params"].pop(),
    "no_slices": _set(["slices"], []),
    "luma_plane_of_the_wrong_shape": lambda r: r.update(y=r["y"][:, :72].copy()),
    "chroma_plane_of_the_wrong_height": lambda r: r.update(uv=r["uv"][:-1].copy()),
    "uint16_plane_at_8_bits": lambda r: r.update(y=r["y"].astype(np.uint16)),
    "missing_field": lambda r: r.pop("pcm_map"),
}


@pytest.mark.parametrize("name", BAD_RECORDS)
def test_records_validation(name):
    rec = _rec()
    native.hevc_loopfilter_records([rec], -1)  # the unchanged records pass
    BAD_RECORDS[name](rec)
    with pytest.raises(ValueError, match="picture 0"):
        native.hevc_loopfilter_records([rec], -1)


def test_records_validation_10_bit_and_batch_index():
    good = _rec()
    rec = copy.deepcopy(hc.records_of(_pic("24x16_ctb16_bd10_s7")))
    rec["sao_params"][0]["off"] = [[31, -31, 0, 0], [0] * 4, [0] * 4]
    rec["qp"][0] = -12
    native.hevc_loopfilter_records([good, rec], -1)
    for f in (_set(["sao_params", 0, "off"], [[32, 0, 0, 0], [0] * 4, [0] * 4]), _set(["qp", 0], -13),
              lambda r: r["y"].__setitem__((0, 0), 1024), lambda r: r.update(y=r["y"].astype(np.uint8))):
        bad = copy.deepcopy(rec)
        f(bad)
        with pytest.raises(ValueError, match="picture 1"):
            native.hevc_loopfilter_records([good, bad], -1)


BAD_PICTURES = {
    "height_not_multiple_of_8": _set(["height"], 36),
    "log2ctb_7": _set(["log2ctb"], 7),
    "ctb_slice_names_no_segment": _set(["ctb_slice", 0], 2),
    "ctb_sord_differs_from_the_segment": _set(["ctb_sord", 0], 1),
    "slice_ordinals_skip": _set(["slices", 1, "ord"], 2),
    "reference_index_outside_the_list": lambda p: (p["mf_pred"].__setitem__(0, 1), p["intra"].__setitem__(0, 0),
                                                   p["mf_ref"].__setitem__(0, 3)),
    "inter_block_without_motion": lambda p: (p["mf_pred"].__setitem__(0, 0), p["intra"].__setitem__(0, 0)),
    "bypass_without_transquant_bypass": lambda p: (p.update(transquant_bypass=0), p["bypass"].__setitem__(0, 1)),
    "edge_flags_above_15": _set(["edge", 3], 16),
    "qp_52": _set(["qp", 3], 52),
    "tile_columns_above_the_ctb_count": _set(["tile_cols"], 6),
    "explicit_tile_columns_too_wide": lambda p: p.update(tile_cols=2, uniform_spacing=0, col_width=[5]),
    "sao_offset_8": _set(["sao", 0, "off"], [[8, 0, 0, 0], [0] * 4, [0] * 4]),
    "mv_array_too_short": lambda p: p["mf_mv"].pop(),
    "unknown_path": None,
}


@pytest.mark.parametrize("name", BAD_PICTURES)
def test_picture_validation(name):
    pic = copy.deepcopy(hc.layout_cases()[0])
    for path in ("strengths", "cpu", "records"):
        native.hevc_loopfilter_picture(pic, -1, path)
    if name == "unknown_path":
        with pytest.raises(ValueError):
            native.hevc_loopfilter_picture(pic, -1, "gpu")
        return
    BAD_PICTURES[name](pic)
    for path in ("strengths", "cpu", "records"):
        with pytest.raises(ValueError):
            native.hevc_loopfilter_picture(pic, -1, path)
