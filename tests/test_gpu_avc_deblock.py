"""The H.264 loop-filter kernels alone, on hand-built macroblock records (tests/deblock_cases.py):
avc_bs_kernel + avc_deblock_kernel (8-bit 4:2:0, every variant of its edge code) and the
loop-filter pass of avc_hbd_kernel (High 10, 4:2:2), byte for byte against avc::cpu_deblock and,
for 4:2:0, against the spec oracle (tests/spec_oracle.py deblock_picture).

Shapes follow the kernels' structure (two MB rows per wave, eight per workgroup, an LDS ring of
eight columns, tagged hand-off between workgroups; 17 MBs on a diagonal for the High 10 / 4:2:2
kernel's strided loop), and the patterns are ones no stream of ours contains: one filtering MB in
a disabled picture, a checkerboard of disabled MBs, non-zero FilterOffsetA / B, pictures 1 MB wide
or tall. native.avc_deblock_records raises when a picture's error word is not zero (wavefront
timeout, bound violation) or a guard band around its planes is written, so every test here also
asserts both.
"""
from __future__ import annotations

import numpy as np
import pytest

import deblock_cases as dc
from video_edge_ai_proxy_amd import native

pytestmark = pytest.mark.gpu

VARIANTS = [5, 1, 0, 3]  # bit 0 packed vertical edges, bit 1 a sync per edge, bit 2 register edges (5: default)


def _cpu(case):
    """avc::cpu_deblock on the case, once."""
    if "_cpu" not in case:
        case["_cpu"] = dc.run_native(native, case, -1)
    return case["_cpu"]


def _check(case, got, what):
    gy, guv = got
    writer = None
    if case["cf"] == 1:  # the oracle first: it names the edge
        wy, wuv, _, writer = dc.oracle(case)
        msg = dc.explain(case, gy, guv, wy, wuv, writer)
        assert msg is None, f"{what} against the oracle: {msg}"
    cy, cuv = _cpu(case)
    msg = dc.explain(case, gy, guv, cy, cuv, writer)
    assert msg is None, f"{what} against cpu_deblock: {msg}"
    if case["pattern"] == "all_off":
        assert np.array_equal(gy, case["args"]["y"]) and np.array_equal(guv, case["args"]["uv"])


CASES8 = dc.cases_420(8)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("t", CASES8, ids=[dc.case_id(t) for t in CASES8])
def test_deblock_kernel(t, variant):
    case = dc.get_case(*t)
    dc.check_honest(case)
    _check(case, dc.run_native(native, case, 0, variant), f"avc_deblock_kernel variant {variant}")


@pytest.mark.parametrize("variant", VARIANTS)
def test_deblock_kernel_directed_edges(variant):
    """The bS table (one rule per row) as two-MB pictures: the bS of the MB edge decides p0."""
    for name, p, q, _, _ in dc.BS_TABLE:
        for vertical, field in ((True, 0), (False, 1), (False, 0), (True, 2)):
            case = dc.directed_case(p, q, vertical, field)
            _check(case, dc.run_native(native, case, 0, variant), f"{name}, variant {variant}")


@pytest.mark.parametrize("variant", VARIANTS)
def test_deblock_kernel_nine_pictures_one_launch(variant):
    """Heights 1, 2, 3, 8, 9, 16, 17, 9, 1 with mixed widths in ONE launch: the grid is sized by the
    tallest picture (three workgroups), and the ninth picture takes the second round of the
    picture -> workgroup map pic = (j / groups) * 8 + (b & 7). The binding keeps a guard band
    around every plane and raises if one is written."""
    cases = dc.many_cases(8)
    assert [c["hmbs"] for c in cases] == dc.MANY_HEIGHTS and len(cases) == 9
    outs = native.avc_deblock_records_many([c["args"] for c in cases], 0, variant)
    assert len(outs) == 9
    for k, (c, got) in enumerate(zip(cases, outs)):
        dc.check_honest(c)
        _check(c, got, f"picture {k} of the batch, variant {variant}")


# ------------------------------------------------------------------ avc_hbd_kernel, loop-filter pass
def _hbd_cases(bd, cf):
    out = [(pt, w, h, bd, cf, 0, None) for w, h in dc.HBD_SHAPES for pt in ("I", "B")]
    w, h = dc.BIG
    out += [("B", w, h, bd, cf, 0, "all_off"), ("B", w, h, bd, cf, 0, "checker"), ("B", w, h, bd, cf, 1, None),
            ("I", w, h, bd, cf, 2, None)]
    out += [("I" if i & 1 else "B", w, h, bd, cf, 0, ("only", a)) for i, a in enumerate(dc.only_addresses())]
    return out


HBD = _hbd_cases(10, 1) + _hbd_cases(8, 2) + _hbd_cases(10, 2)


@pytest.mark.parametrize("t", HBD, ids=[dc.case_id(t) for t in HBD])
def test_hbd_kernel(t):
    case = dc.get_case(*t)
    if case["cf"] == 1:
        dc.check_honest(case)
    else:  # no oracle for 4:2:2: at least the CPU reference filters both planes
        cy, cuv = _cpu(case)
        if case["pattern"] is None and case["wmbs"] * case["hmbs"] > 2:
            assert not np.array_equal(cuv[:, 0::2], case["args"]["uv"][:, 0::2])
            assert not np.array_equal(cuv[:, 1::2], case["args"]["uv"][:, 1::2])
    _check(case, dc.run_native(native, case, 0), "avc_hbd_kernel")


def test_hbd_kernel_directed_edges():
    for name, p, q, _, _ in dc.BS_TABLE:
        for vertical, field in ((True, 0), (False, 1)):
            case = dc.directed_case(p, q, vertical, field, bd=10)
            _check(case, dc.run_native(native, case, 0), name)


def test_mixed_format_batch_of_three():
    """High 10 4:2:0, 8-bit 4:2:2 and High 10 4:2:2 pictures in one descriptor array (three kernel
    instantiations, each skipping the other two pictures), with an 8-bit 4:2:0 picture between
    them for avc_deblock_kernel in the same round."""
    cases = [dc.get_case("B", 17, 3, 10, 1), dc.get_case("I", 9, 2, 8, 2), dc.get_case("B", 3, 3, 8, 1),
             dc.get_case("B", 33, 17, 10, 2)]
    outs = native.avc_deblock_records_many([c["args"] for c in cases], 0, 5)
    for k, (c, got) in enumerate(zip(cases, outs)):
        _check(c, got, f"picture {k} of the mixed batch")


def test_nine_high10_pictures_one_launch():
    cases = dc.many_cases(10)
    outs = native.avc_deblock_records_many([c["args"] for c in cases], 0, 5)
    for k, (c, got) in enumerate(zip(cases, outs)):
        dc.check_honest(c)
        _check(c, got, f"picture {k} of the High 10 batch")
