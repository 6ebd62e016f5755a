"""The H.264 reconstruction kernels alone, on hand-built macroblock records (tests/recon_cases.py):
avc_inter_kernel, avc_intra_kernel (8-bit 4:2:0) and the intra pass of avc_hbd_kernel (High 10,
4:2:2), byte for byte against avc::cpu_reconstruct and against the spec oracle
(tests/recon_oracle.py), single pictures and batches in one launch sequence.

Shapes follow the kernels' structure: widths around the 64-MB chunks of a row and the 240-MB LDS
lines of the intra wavefront, heights around its eight-row workgroups, nine pictures for the second
round of the picture -> workgroup map. native.avc_recon_records raises when a picture's error word
is not zero (wavefront timeout, pool bound), a guard band around a DPB surface is written or a
reference surface changes, so every test here asserts those too.

The oracle runs once per case (cached in recon_cases); its slowest cases on the CPU are the 241x9
structure picture (0.74 s measured) and the dense 33x17 pictures (0.5 - 0.9 s).
"""
from __future__ import annotations

import pytest

import recon_cases as rc
from video_edge_ai_proxy_amd import native

pytestmark = pytest.mark.gpu

ALL = [(n, bd, cf) for bd, cf in rc.FORMATS for n in rc.case_names(bd, cf)]
IDS = [f"{n}-{bd}bit-{'420' if cf == 1 else '422'}" for n, bd, cf in ALL]


def _cpu(case):
    if "_cpu" not in case:
        case["_cpu"] = rc.run_native(native, case, -1)
    return case["_cpu"]


def _check(case, got, what):
    msg = rc.explain(case, got, rc.oracle(case)[:3])  # the oracle first: it names the rule
    assert msg is None, f"{what} against the oracle: {msg}"
    msg = rc.explain(case, got, _cpu(case))
    assert msg is None, f"{what} against cpu_reconstruct: {msg}"


@pytest.mark.parametrize("name,bd,cf", ALL, ids=IDS)
def test_recon_kernels(name, bd, cf):
    case = rc.get_case(name, bd, cf)
    rc.check_honest(case)
    _check(case, rc.run_native(native, case, 0), "the kernels")


@pytest.mark.parametrize("bd,cf", rc.FORMATS)
def test_nine_pictures_one_launch(bd, cf):
    """Heights 1, 2, 3, 8, 9, 16, 17, 9, 1 with mixed widths in ONE launch sequence: the intra grid
    is sized by the tallest picture, the ninth picture takes the second round of pic = (j / groups)
    * 8 + (b & 7), and mb_begin is the exclusive prefix the inter kernel searches."""
    cases = [rc.get_case(n, bd, cf) for n in rc.many_names()]
    assert [c["pic"]["hmbs"] for c in cases] == rc.MANY_HEIGHTS
    outs = native.avc_recon_records_many([c["args"] for c in cases], 0)
    assert len(outs) == 9
    for k, (c, got) in enumerate(zip(cases, outs)):
        _check(c, rc.split(got), f"picture {k} of the batch")


def test_mixed_format_batch():
    """8-bit 4:2:0, High 10 4:2:0, 8-bit 4:2:2 and High 10 4:2:2 pictures in one descriptor array:
    the inter kernel takes all four, avc_intra_kernel and each avc_hbd_kernel instantiation skip the
    pictures of the others."""
    cases = [rc.get_case("shape_17x3", 10, 1), rc.get_case("avail_constrained", 8, 1), rc.get_case("shape_9x2", 8, 2),
             rc.get_case("inter_parts33", 8, 1), rc.get_case("shape_33x17", 10, 2), rc.get_case("inter_wpmix", 10, 2)]
    outs = native.avc_recon_records_many([c["args"] for c in cases], 0)
    for k, (c, got) in enumerate(zip(cases, outs)):
        _check(c, rc.split(got), f"picture {k} of the mixed batch")
