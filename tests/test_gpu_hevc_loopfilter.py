"""hevc_deblock_kernel, hevc_sao_copy_kernel and hevc_sao_kernel alone, on the seeded pictures of
tests/hevc_lf_cases.py, exactly equal to the spec oracle (tests/spec_oracle_hevc.py, written from
H.265 8.7.2 / 8.7.3): per picture, for two batches of mixed sizes and bit depths in one launch
(pick_blk / blk_begin, u8 and u16 descriptors side by side, a picture with the filters off beside
one that needs them), and from the parser's state through finish_gpu_picture for the slice / tile
layouts and the bS table. native.hevc_loopfilter_records raises when a guard band around a plane
or the SAO scratch, or an input map, comes back changed. The oracle's results are computed once
per case (hevc_lf_cases.oracle_cached)."""
from __future__ import annotations

import numpy as np
import pytest

import hevc_lf_cases as hc
from video_edge_ai_proxy_amd import native

pytestmark = pytest.mark.gpu

PICS = hc.all_pictures()
LAYOUTS = hc.layout_cases()
TABLE = hc.bs_table()
BATCHES = hc.batch_cases()


def _check(rec, got):
    msg = hc.explain(rec, got, hc.oracle_cached(rec))
    assert msg is None, msg


@pytest.mark.parametrize("pic", PICS, ids=[p["name"] for p in PICS])
def test_kernels_equal_oracle(pic):
    rec = hc.records_of(pic)
    _check(rec, native.hevc_loopfilter_records([rec], 0)[0])


@pytest.mark.parametrize("name,recs", BATCHES, ids=[b[0] for b in BATCHES])
def test_kernels_equal_oracle_in_one_launch(name, recs):
    got = native.hevc_loopfilter_records(recs, 0)
    assert len(got) == len(recs)
    for rec, g in zip(recs, got):
        _check(rec, g)
    last = recs[-1]  # both filters off, in a round that launches them: returned as given
    assert np.array_equal(got[-1][0], last["y"]) and np.array_equal(got[-1][1], last["uv"])


@pytest.mark.parametrize("pic", LAYOUTS + TABLE, ids=[p["name"] for p in LAYOUTS + TABLE])
def test_parser_state_through_the_kernels(pic):
    _check(hc.records_of(pic), native.hevc_loopfilter_picture(pic, 0, "records"))
