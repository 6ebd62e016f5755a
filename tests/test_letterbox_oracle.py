"""The float64 letterbox oracle (letterbox_oracle.py) checked without a GPU: its geometry against
the launcher's, the CPU backend's mirrors of the letterbox kernels against it (which validates the
oracle and the mirrors at once: they share no code), and the torch references of ``ops`` against it
where both are defined."""
import numpy as np
import pytest
import torch

import letterbox_checks as lc
import letterbox_oracle as lo
from conftest import synth

ALL_CASES = {**lc.CASES, **lc.NV12_EXTRA}


def test_geometry_equals_the_launcher(native):
    sizes = {(w, h, S) for (w, h, _, _, S) in ALL_CASES.values()}
    sizes |= {(w, h, 64) for (w, h) in lc.WORKER_CAMS} | {(1920, 1080, 640), (640, 480, 640), (352, 288, 640)}
    for S in (32, 64):
        sizes |= {(w, h, S) for w in range(1, 81) for h in range(1, 81)}
    for (w, h, S) in sorted(sizes):
        for even in (False, True):
            g = lo.geometry(w, h, S, even)
            assert tuple(native.letterbox_geometry(w, h, S, even)) == (g.nw, g.nh, g.pad_x, g.pad_y), (w, h, S, even)
            assert g.rx == float(np.float32(w) / np.float32(g.nw)) and g.ry == float(np.float32(h) / np.float32(g.nh))
            assert 0 <= g.pad_x and g.pad_x + g.nw <= S and 0 <= g.pad_y and g.pad_y + g.nh <= S


def test_exact_geometries_are_the_ones_meant():
    exact = {k for k, (w, h, _, _, S) in lc.CASES.items() if lo.is_exact(lo.geometry(w, h, S))}
    assert exact == {"identity", "down2", "down2-portrait", "down2-portrait40", "up2", "up2-portrait"}
    g = lo.geometry(40, 64, 32)
    assert (g.pad_x, g.nw) == (6, 20) and lo.geometry(48, 64, 32).pad_x == 4
    assert lo.geometry(250, 40, 64).nh == 10
    for k, (w, h, _, _, S) in lc.CASES.items():  # the even (NV12) geometry keeps the ratios exact
        assert lo.is_exact(lo.geometry(w, h, S, True)) == (k in exact), k


@pytest.mark.parametrize("case", sorted(ALL_CASES))
def test_undecidable_share_is_under_the_cap(case):
    """From the oracle alone, for both output formats of every case (the GPU tests assert it
    again before they compare)."""
    w, h, cl, ct, S = ALL_CASES[case]
    y, uv = lc.planes(7, w, h, cl, ct)
    inside = np.repeat(lo.inside_mask(w, h, S)[..., None], 3, axis=2)
    lc.u8_band(lo.bgr_canvas(y, uv, w, h, cl, ct, S, 114), lc.case_delta(w, h, S), inside)
    m = lo.inside_mask(w, h, S, True)
    luma, chroma = lo.nv12_canvas(y, uv, w, h, cl, ct, S, 114)
    lc.u8_band(luma, lc.case_delta(w, h, S, True), m)
    lc.u8_band(chroma, lc.case_delta(w, h, S, True), np.repeat(m[::2, ::2][..., None], 2, axis=2))


@pytest.mark.parametrize("fmt,chw_dtype", [(0, torch.float32), (0, torch.float16), (0, torch.bfloat16), (0, None),
                                           (1, None), (1, torch.float16)],
                         ids=["bgr-fp32", "bgr-fp16", "bgr-bf16", "bgr-hwc-only", "nv12", "nv12-no-chw"])
def test_cpu_backend_rows_match_the_oracle(native, fmt, chw_dtype):
    """cpu_letterbox / cpu_letterbox_nv12 through a CPU worker: three geometries in one batch.
    The half-precision CHW rows used to stay unwritten on this backend."""
    lc.run_worker_batch(native, synth, -1, fmt, chw_dtype)


def test_identity_is_the_plain_conversion(native):
    """Ratio 1 and no pad: the canvas is the BT.601 picture itself, so the oracle's integer
    conversion must equal the project's CPU converter byte for byte (full-range input, clipping
    in both directions)."""
    y, uv = lc.planes(11, 64, 64, 0, 0)
    canvas = lo.bgr_canvas(y, uv, 64, 64, 0, 0, 64, 0)
    assert np.array_equal(canvas, native.nv12_to_bgr_cpu(y, uv, 0, 0, 64, 64).astype(np.float64))
    c = lo.bgr_canvas(*lc.planes(12, 41, 27, 3, 2), 41, 27, 3, 2, 32, 0)
    assert c.min() == 0.0 and c.max() == 255.0, "the inputs do not reach the clipping"


@pytest.mark.parametrize("case", ["identity", "down2", "up2", "cif", "down2-portrait"])
def test_oracle_agrees_with_the_torch_reference_at_even_sizes(native, case):
    """ops.letterbox_reference (fp32 F.interpolate) and the oracle are two definitions of the same
    resize; where both are valid they agree within the tolerance the reference has always been
    used with (max 1 level, under 1 % of the bytes, CHW atol 2 / 255 / 0.224)."""
    from video_edge_ai_proxy_amd import ops

    w, h, cl, ct, S = lc.CASES[case]
    y, uv = lc.planes(21, w, h, cl, ct)
    canvas = lo.bgr_canvas(y, uv, w, h, cl, ct, S, 114)
    bgr = torch.from_numpy(native.nv12_to_bgr_cpu(y, uv, cl, ct, w, h))
    rh, rc = ops.letterbox_reference(bgr, S, chw_dtype=torch.float32, mean=lc.MEAN, std=lc.STD)
    d = np.abs(rh.numpy().astype(np.float64) - np.floor(canvas + 0.5))
    assert d.max() <= 1 and (d > 0).mean() < 0.01
    assert np.abs(rc.numpy() - lo.chw(canvas, lc.MEAN, lc.STD)).max() <= 2.0 / 255 / 0.224
    assert np.abs(rc.numpy() - lo.chw(canvas, lc.MEAN, lc.STD)).max() <= 1e-4, "fp32 interpolate is far closer than that"


@pytest.mark.parametrize("case", ["identity", "down2", "up2", "cif", "odd45", "odd41"])
def test_nv12_reference_agrees_with_the_oracle(case):
    """ops.letterbox_nv12_reference against the oracle: at even sizes as before, and at the odd
    sizes where it used to take the chroma ratio from the stored plane sizes."""
    from video_edge_ai_proxy_amd import ops

    w, h, cl, ct, S = ALL_CASES[case]
    y, uv = lc.planes(22, w, h, cl, ct)
    want = np.floor(lo.nv12_bytes(*lo.nv12_canvas(y, uv, w, h, cl, ct, S, 114)) + 0.5)
    got = ops.letterbox_nv12_reference(torch.from_numpy(y), torch.from_numpy(uv), S, w, h).numpy().astype(np.float64)
    d = np.abs(got - want)
    assert d.max() <= 1 and (d > 0).mean() < 0.01


def test_nv12_chroma_ratio_matters_at_odd_sizes():
    """The defect the oracle pins: sampling the chroma plane of 41 x 27 with the stored-size ratio
    (21 / 12, 14 / 8) instead of the luma ratio moves many chroma bytes; the rules would see it."""
    w, h, S = 41, 27, 32
    y, uv = lc.planes(23, w, h, 0, 0)
    g = lo.geometry(w, h, S, True)
    assert g.rx == 1.28125 and abs(g.ry - 1.35) < 1e-6
    _, chroma = lo.nv12_canvas(y, uv, w, h, 0, 0, S, 114)
    pairs = uv.reshape(uv.shape[0], -1, 2)[:(h + 1) // 2, :(w + 1) // 2].astype(np.float64)
    wrong = lo._bilinear(pairs, g.nh // 2, g.nw // 2, ((h + 1) // 2) / (g.nh // 2), ((w + 1) // 2) / (g.nw // 2))
    py, px = g.pad_y // 2, g.pad_x // 2
    right = chroma[py:py + g.nh // 2, px:px + g.nw // 2]
    assert (np.floor(wrong + 0.5) != np.floor(right + 0.5)).mean() > 0.5
