"""The model-input kernels on gfx950 (letterbox_kernel, letterbox_nv12_kernel, nv12_to_chw_kernel,
single launches and the worker's batched launch) against the float64 oracle of letterbox_oracle.py,
under the derived rules of letterbox_checks.py: byte-exact in the exact geometries, and elsewhere
exact but for the bytes the oracle itself declares undecidable (at most 5 % of the picture).

Shapes are the smallest at which each path can go wrong: portrait and landscape, up- and
downscaling, ratio 1, odd sizes and odd crops, a pad edge inside a 4-pixel quad, an extreme aspect,
and a canvas whose quads do not fill whole 256-thread blocks. Inputs are full range with forced
peaks, so the BT.601 clipping runs in both directions.
"""
import functools

import numpy as np
import pytest
import torch

import letterbox_checks as lc
import letterbox_oracle as lo
from conftest import high_encoder, synth
from history_util import narrow_planes

pytestmark = pytest.mark.gpu

ALL_CASES = {**lc.CASES, **lc.NV12_EXTRA}
PADS = [0, 114, 255]
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case_planes(case):
    w, h, cl, ct, _ = ALL_CASES[case]
    return _frozen(*lc.planes(sum(map(ord, case)), w, h, cl, ct))


@functools.lru_cache(maxsize=None)
def bgr_oracle(case, pad):
    w, h, cl, ct, S = ALL_CASES[case]
    return _frozen(lo.bgr_canvas(*case_planes(case), w, h, cl, ct, S, pad))[0]


@functools.lru_cache(maxsize=None)
def nv12_oracle(case, pad):
    w, h, cl, ct, S = ALL_CASES[case]
    return _frozen(*lo.nv12_canvas(*case_planes(case), w, h, cl, ct, S, pad))


def device_planes(case):
    y, uv = case_planes(case)
    return torch.from_numpy(y.copy()).cuda(), torch.from_numpy(uv.copy()).cuda()


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("case", sorted(lc.CASES))
def test_letterbox_bgr_matches_the_oracle(case, pad):
    """HWC and CHW in every output combination: HWC + fp32 CHW, CHW alone in fp16 and bf16
    (hwc=False), HWC alone (chw_dtype=None)."""
    from video_edge_ai_proxy_amd import ops

    w, h, cl, ct, S = lc.CASES[case]
    y, uv = device_planes(case)
    canvas = bgr_oracle(case, pad)
    ref = lo.chw(canvas, lc.MEAN, lc.STD)
    d = lc.case_delta(w, h, S)
    inside = np.repeat(lo.inside_mask(w, h, S)[..., None], 3, axis=2)
    kw = dict(size=S, width=w, height=h, crop_left=cl, crop_top=ct, mean=lc.MEAN, std=lc.STD, pad_value=pad)
    hwc, c32 = ops.letterbox(y, uv, chw_dtype=torch.float32, **kw)
    n16, c16 = ops.letterbox(y, uv, chw_dtype=torch.float16, hwc=False, **kw)
    nb16, cb16 = ops.letterbox(y, uv, chw_dtype=torch.bfloat16, hwc=False, **kw)
    only, none = ops.letterbox(y, uv, chw_dtype=None, **kw)
    torch.cuda.synchronize()
    assert n16 is None and nb16 is None and none is None
    assert c32.dtype == torch.float32 and c16.dtype == torch.float16 and cb16.dtype == torch.bfloat16
    got = hwc.cpu().numpy()
    lc.check_u8(f"bgr {case} pad {pad}", got, canvas, d, inside)
    assert (got[~inside] == pad).all(), "pad pixels must be the pad value"
    assert torch.equal(only, hwc), "HWC must not depend on whether CHW is written"
    lc.check_chw(f"bgr {case} pad {pad}", c32, ref, d, lc.STD)
    lc.check_chw(f"bgr {case} pad {pad}", c16, ref, d, lc.STD)
    lc.check_chw(f"bgr {case} pad {pad}", cb16, ref, d, lc.STD)
    if case == "identity":
        assert torch.equal(hwc, ops.nv12_to_bgr(y, uv)), "ratio 1 must be the plain conversion"


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("case", sorted(ALL_CASES))
def test_letterbox_nv12_matches_the_oracle(case, pad):
    from video_edge_ai_proxy_amd import ops

    w, h, cl, ct, S = ALL_CASES[case]
    y, uv = device_planes(case)
    luma, chroma = nv12_oracle(case, pad)
    got = ops.letterbox_nv12(y, uv, S, w, h, crop_left=cl, crop_top=ct, pad_value=pad)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == (S * S * 3 // 2,)
    m = lo.inside_mask(w, h, S, True)
    inside = np.concatenate([m.reshape(-1), np.repeat(m[::2, ::2].reshape(-1), 2)])
    lc.check_u8(f"nv12 {case} pad {pad}", got, lo.nv12_bytes(luma, chroma), lc.case_delta(w, h, S, True), inside)
    assert (got[:S * S][~m.reshape(-1)] == round(16 + pad * 219 / 255)).all()
    assert (got[S * S:][~inside[S * S:]] == 128).all()


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("S", [8, 40, 64])
def test_nv12_to_chw_matches_the_oracle(S, n, dtype):
    """No resampling: delta = 0, only the normalisation's rounding headroom remains."""
    from video_edge_ai_proxy_amd import ops

    rng = np.random.default_rng(1000 + S + n)
    batch = rng.integers(0, 256, (n, S * S * 3 // 2)).astype(np.uint8)
    batch[:, :4] = 255
    batch[:, S * S:S * S + 4] = 255
    batch[:, -4:] = 0
    got = ops.nv12_to_chw(torch.from_numpy(batch).cuda(), S, DTYPES[dtype], lc.MEAN, lc.STD)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (n, 3, S, S) and got.dtype == DTYPES[dtype]
    for i in range(n):
        ref = lo.chw(lo.nv12_picture_bgr(batch[i], S).astype(np.float64), lc.MEAN, lc.STD)
        lc.check_chw(f"nv12_to_chw S{S} picture {i}", got[i], ref, 0.0, lc.STD)


def test_letterbox_ops_reject_bad_arguments(native):
    """Every call raises before anything is launched."""
    from video_edge_ai_proxy_amd import ops

    y = torch.zeros((32, 48), dtype=torch.uint8, device="cuda")
    uv = torch.zeros((16, 48), dtype=torch.uint8, device="cuda")
    both = [lambda **kw: ops.letterbox(y, uv, **kw), lambda **kw: ops.letterbox_nv12(y, uv, **kw)]
    for op in both:
        with pytest.raises(ValueError):
            op(size=36)  # a multiple of 4, not of 8
        with pytest.raises(ValueError):
            op(size=0)
        with pytest.raises(ValueError):
            op(size=-8)
        with pytest.raises(ValueError):
            op(size=32, width=48, height=32, crop_left=1)  # leaves the planes at the right
        with pytest.raises(ValueError):
            op(size=32, width=49, height=32)
        with pytest.raises(ValueError):
            op(size=32, width=48, height=32, crop_top=1)  # leaves the planes at the bottom
        with pytest.raises(ValueError):
            op(size=32, width=48, height=33)
        with pytest.raises(ValueError):
            op(size=32, crop_left=-1, width=8, height=8)
        with pytest.raises(ValueError):
            op(size=32, width=0, height=32)
        with pytest.raises(ValueError):
            op(size=32, width=48, height=-2)
    with pytest.raises(ValueError):
        ops.letterbox(y, uv, 32, chw_dtype=torch.float32, std=(0.229, 0.0, 0.225))
    with pytest.raises(ValueError):
        ops.nv12_to_chw(torch.zeros((96,), dtype=torch.uint8, device="cuda"), 8, torch.float32, std=(1.0, 1.0, 0.0))
    with pytest.raises(ValueError):
        ops.letterbox(y, uv, 32, hwc=False)  # nothing to compute
    with pytest.raises(TypeError):
        ops.letterbox(y.to(torch.int16), uv, 32)
    with pytest.raises(TypeError):
        ops.letterbox_nv12(y, uv.to(torch.float16), 32)
    with pytest.raises(TypeError):
        ops.letterbox(y, uv, 32, chw_dtype=torch.float64)
    out = torch.zeros((32 * 32 * 3,), dtype=torch.uint8, device="cuda")
    args = lambda **kw: {**dict(y=y.data_ptr(), uv=uv.data_ptr(), pitch=48, src_w=48, src_h=32, crop_left=0, crop_top=0,
                                size=32, out_hwc=out.data_ptr(), out_chw=0, chw_dtype=0, mean=[0.0] * 3,
                                std=[1.0] * 3, pad=114, stream=0), **kw}
    for bad in (dict(crop_left=1), dict(chw_dtype=7), dict(chw_dtype=-1), dict(size=36), dict(src_w=0),
                dict(crop_top=-1), dict(y=0), dict(out_hwc=0), dict(format=2)):
        with pytest.raises(native.NativeError):  # the binding checks what it launches, too
            native.letterbox(**args(**bad))
    torch.cuda.synchronize()
    assert not out.any(), "a rejected call wrote its output"


@pytest.mark.parametrize("fmt,chw_dtype", [(0, torch.float32), (0, torch.float16), (1, None)],
                         ids=["bgr-fp32", "bgr-fp16", "nv12"])
def test_worker_batch_rows_match_the_oracle(native, fmt, chw_dtype):
    """320x240, 144x176 and 200x120 (coded 208x128) in one batched launch; all three sizes are
    accepted by the synthetic encoder as they are."""
    lc.run_worker_batch(native, synth, 0, fmt, chw_dtype)


def test_worker_letterboxes_the_narrowed_high10_surface(native):
    """A High 10 camera: the letterbox must read the 8-bit copy of the 10-bit surface, each sample
    min(255, (s + 2) >> 2). The oracle's input is the worker's own full-depth surface
    (read_surface) narrowed in numpy."""
    S, w, h = 64, 176, 144
    wk = native.Worker(device=0, letterbox_size=S, max_cameras=2, chw_dtype=lc.CHW_CODES[torch.float32],
                       mean=list(lc.MEAN), std=list(lc.STD))
    hwc, chw = lc.worker_buffers(S, 0, torch.float32, 2, "cuda")
    wk.set_consumer_buffers(hwc.data_ptr(), chw.data_ptr(), 2)
    cam = wk.add_camera("high10", 4)
    enc = high_encoder(native, w, h, bit_depth=10, seed=5, bframes=0)
    for _ in range(3):
        wk.decode_now(cam, enc.next())
    torch.cuda.synchronize()
    assert wk.stats(cam)["published"] == 3 and wk.stats(cam)["errors"] == 0
    pts, (y, uv) = wk.read_surface(cam)
    assert pts == enc.last_pts and y.dtype == np.uint16 and uv.dtype == np.uint16
    y8, uv8 = narrow_planes(y, uv, 10, 1)
    assert (y8 != (y >> 2)).any(), "rounding and truncating narrowing agree on this picture: no teeth"
    rows = hwc.cpu().numpy()
    lc.check_row("worker high10", rows[0], chw.cpu().view(torch.float32).view(2, 3, S, S)[0], y8, uv8, w, h, S, 0,
                 torch.float32)
    assert (rows[1] == 0xA5).all()
