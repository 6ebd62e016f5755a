"""Comparison rules and shared inputs of the letterbox tests (test_letterbox_oracle.py on the CPU,
test_gpu_letterbox.py on the GPU). A helper module like history_util.py.

None of the bounds is tuned to a result. With v the float64 oracle value and
``delta = letterbox_oracle.delta(src_w, src_h)`` the fp32 error bound of one resampled value
(0 in the exact geometries of ``is_exact`` and for nv12_to_chw, which does not resample):

* u8 outputs: a byte must equal floor(v + 0.5), unless v + 0.5 lies within delta of an integer;
  such a byte is *undecidable* and may take either neighbour. The undecidable bytes are counted
  from the oracle alone, before anything is compared, and may be at most 5 % of the picture's
  bytes (pad bytes are not counted in the denominator), so a wrong oracle or a loose delta
  cannot excuse a kernel.
* fp32 CHW: |got - ref| <= delta / (255 * std) + 2^-20 * max(1, |ref|): the resampling bound
  scaled by the normalisation, plus 16 fp32 roundings of headroom for its ~5 operations
  (1/255 and 1/std are themselves rounded).
* fp16 / bf16 CHW: RNE(ref - s) <= got <= RNE(ref + s) with s the fp32 slack above and RNE the
  round-to-nearest-even conversion torch does on the CPU; and at least 95 % of the elements equal
  RNE(ref) exactly, which a truncating conversion (half of all elements one step low) cannot meet.
"""
import numpy as np
import torch

import letterbox_oracle as lo

UNDECIDABLE_CAP = 0.05
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# id -> (src_w, src_h, crop_left, crop_top, S)
CASES = {
    "identity": (64, 64, 0, 0, 64),          # ratio 1
    "down2": (64, 48, 0, 0, 32),             # exact, pad_y > 0
    "down2-portrait": (48, 64, 0, 0, 32),    # exact, pad_x = 4: a whole quad of pad
    "down2-portrait40": (40, 64, 0, 0, 32),  # exact, pad_x = 6: the pad edge inside a 4-pixel quad
    "up2": (32, 24, 0, 0, 64),               # exact upscale: left clamp of s, right clamp of i1
    "up2-portrait": (24, 32, 0, 0, 64),      # exact upscale with pad_x > 0
    "odd-crop": (41, 27, 3, 2, 32),          # odd size, odd crop, general ratio
    "cif": (176, 144, 0, 0, 64),             # general ratio 2.75
    "wide-crop": (250, 40, 16, 1, 64),       # extreme aspect (nh = 10), crop
    "ragged-block": (200, 120, 5, 3, 40),    # 400 quads: a partial last 256-thread block
}
# odd sizes at which the plane-size chroma ratio differs from the luma ratio
NV12_EXTRA = {"odd45": (45, 35, 0, 0, 64), "odd41": (41, 27, 0, 0, 32)}


def coded(n):
    return (n + 15) // 16 * 16


def planes(seed, src_w, src_h, crop_left, crop_top):
    """Full-range coded NV12 planes (the window rounded up to macroblocks) with the peaks that
    make the BT.601 clipping run in both directions."""
    rng = np.random.default_rng(seed)
    W, H = coded(crop_left + src_w), coded(crop_top + src_h)
    y = rng.integers(0, 256, (H, W)).astype(np.uint8)
    uv = rng.integers(0, 256, (H // 2, W)).astype(np.uint8)
    y[0, :4] = 255
    uv[0, :4] = 255
    uv[-1, -4:] = 0
    return y, uv


def case_delta(src_w, src_h, S, even=False):
    return 0.0 if lo.is_exact(lo.geometry(src_w, src_h, S, even)) else lo.delta(src_w, src_h)


def u8_band(v, d, inside):
    """(lo, hi, share): the byte values the rule allows per element and the share of undecidable
    bytes among the picture's (inside) bytes; from the oracle alone. The cap is asserted here."""
    v = np.asarray(v, dtype=np.float64)
    low = np.floor(v + 0.5 - d)
    high = np.floor(v + 0.5 + d)
    und = low != high
    if d == 0.0:
        assert not und.any()
    assert not und[~inside].any(), "a pad byte cannot be undecidable"
    share = float(und[inside].mean()) if inside.any() else 0.0
    assert share <= UNDECIDABLE_CAP, f"oracle leaves {share:.2%} of the picture undecidable (delta {d:.3g})"
    return low, high, share


def check_u8(name, got, v, d, inside):
    """got: uint8 array, v: float64 oracle of the same shape, inside: bool mask of the same shape.
    Returns (undecidable share, max |got - v|)."""
    got = np.asarray(got)
    assert got.dtype == np.uint8 and got.shape == np.shape(v), (got.dtype, got.shape, np.shape(v))
    low, high, share = u8_band(v, d, inside)
    g = got.astype(np.float64)
    err = float(np.abs(g - v).max())
    bad = (g < low) | (g > high)
    other = int((g != np.floor(v + 0.5)).sum())  # undecidable bytes that took the other neighbour
    print(f"{name}: delta {d:.3g} undecidable {share:.3%} max|got-v| {err:.4f} "
          f"bytes != floor(v+0.5) {other} of {g.size}")
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} bytes outside the rule; first at {i}: "
                             f"got {got[i]}, oracle {v[i]:.6f}")
    return share, err


def chw_slack(ref, d, std):
    s = np.asarray(std, dtype=np.float64).reshape(3, 1, 1)
    return d / (255.0 * s) + 2.0 ** -20 * np.maximum(1.0, np.abs(ref))


def check_chw(name, got, ref, d, std):
    """got: torch tensor [3, S, S] (fp32 / fp16 / bf16, any device); ref: float64 oracle."""
    got = got.detach().cpu()
    assert tuple(got.shape) == ref.shape, (tuple(got.shape), ref.shape)
    slack = chw_slack(ref, d, std)
    g = got.to(torch.float64).numpy()
    assert np.isfinite(g).all(), f"{name}: non-finite values"
    if got.dtype == torch.float32:
        err = np.abs(g - ref)
        print(f"{name}: fp32 max err {err.max():.3g}, smallest slack {slack.min():.3g}")
        assert (err <= slack).all(), f"{name}: {int((err > slack).sum())} elements off, worst {err.max():.3g}"
        return float(err.max())
    rne = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(got.dtype).to(torch.float64).numpy()
    low, high, mid = rne(ref - slack), rne(ref + slack), rne(ref)
    out = (g < low) | (g > high)
    same = float((g == mid).mean())
    print(f"{name}: {got.dtype} equal to RNE(ref) {same:.3%}, outside the bracket {int(out.sum())}")
    assert not out.any(), f"{name}: {int(out.sum())} elements outside [RNE(ref - s), RNE(ref + s)]"
    assert same >= 0.95, f"{name}: only {same:.2%} of the elements are the correctly rounded value"
    return float(np.abs(g - ref).max())


# ------------------------------------------------------------------------------- worker batch

WORKER_CAMS = [(320, 240), (144, 176), (200, 120)]  # landscape, portrait, coded height 128 cropped to 120
WORKER_PAD = 114                                    # the worker's pad value
CHW_CODES = {None: 0, torch.float16: 1, torch.bfloat16: 2, torch.float32: 3}


def check_row(name, hwc_row, chw_row, y, uv, w, h, S, fmt, chw_dtype):
    """One consumer-batch row against the oracle of the planes (y, uv), window (0, 0, w, h).
    hwc_row: uint8 numpy row; chw_row: torch [3, S, S] or None. Returns (share, max err)."""
    d = case_delta(w, h, S, even=bool(fmt))
    if fmt:
        luma, chroma = lo.nv12_canvas(y, uv, w, h, 0, 0, S, WORKER_PAD)
        m = lo.inside_mask(w, h, S, True)
        inside = np.concatenate([m.reshape(-1), np.repeat(m[::2, ::2].reshape(-1), 2)])
        return check_u8(name, hwc_row, lo.nv12_bytes(luma, chroma), d, inside)
    canvas = lo.bgr_canvas(y, uv, w, h, 0, 0, S, WORKER_PAD)
    inside = np.repeat(lo.inside_mask(w, h, S)[..., None], 3, axis=2)
    r = check_u8(name, hwc_row.reshape(S, S, 3), canvas, d, inside)
    if chw_dtype is not None:
        check_chw(name + " chw", chw_row, lo.chw(canvas, MEAN, STD), d, STD)
    return r


def worker_buffers(S, fmt, chw_dtype, rows, device):
    """Caller-owned consumer buffers prefilled with 0xA5: (hwc [rows, bytes] uint8, chw bytes or None)."""
    nb = S * S * 3 // 2 if fmt else S * S * 3
    hwc = torch.full((rows, nb), 0xA5, dtype=torch.uint8, device=device)
    chw = None
    if chw_dtype is not None:
        es = 4 if chw_dtype == torch.float32 else 2
        chw = torch.full((rows, 3 * S * S * es), 0xA5, dtype=torch.uint8, device=device)
    return hwc, chw


def run_worker_batch(native, synth, device, fmt, chw_dtype, S=64):
    """Three cameras of different geometry decoded in ONE decode_many call (one batched letterbox
    launch: blockIdx.y -> descriptor) into caller-owned buffers of four rows; rows 0..2 follow the
    rules against the oracle of each camera's reference-decoder surface, row 3 keeps its 0xA5.
    The synthetic encoder crops at the right / bottom edge only, so every window starts at (0, 0);
    that is checked against the reference decoder's own BGR picture."""
    tdev = "cpu" if device < 0 else "cuda"
    wk = native.Worker(device=device, letterbox_size=S, max_cameras=4, letterbox_format=fmt,
                       chw_dtype=CHW_CODES[chw_dtype], mean=list(MEAN), std=list(STD))
    hwc, chw = worker_buffers(S, fmt, chw_dtype, 4, tdev)
    wk.set_consumer_buffers(hwc.data_ptr(), chw.data_ptr() if chw is not None else 0, 4)
    work, surfaces = [], []
    for k, (w, h) in enumerate(WORKER_CAMS):
        enc = synth(native, w, h, gop=4, seed=k + 1)
        ref = native.CpuDecoder()
        au = enc.next()
        bgr = ref.decode(au)
        y, uv = ref.surface()
        assert np.array_equal(native.nv12_to_bgr_cpu(y, uv, 0, 0, w, h), bgr), "the window does not start at (0, 0)"
        surfaces.append((y, uv))
        work.append((wk.add_camera(f"cam{k}", 2), [au]))
    assert [c for c, _ in work] == [0, 1, 2]
    assert wk.decode_many(work) == 3
    if device >= 0:
        torch.cuda.synchronize()
    rows = hwc.cpu().numpy()
    planes_chw = None
    if chw is not None:
        planes_chw = chw.cpu().view(chw_dtype).view(4, 3, S, S)
    out = []
    for k, (w, h) in enumerate(WORKER_CAMS):
        y, uv = surfaces[k]
        out.append(check_row(f"worker fmt{fmt} cam{k} {w}x{h}", rows[k], None if planes_chw is None else planes_chw[k],
                             y, uv, w, h, S, fmt, None if fmt else chw_dtype))
    assert (rows[3] == 0xA5).all(), "the unused row was written"
    if chw is not None:
        raw = chw.cpu().numpy()
        assert (raw[3] == 0xA5).all(), "the unused CHW row was written"
        if fmt:
            assert (raw == 0xA5).all(), "the NV12 consumer format has no CHW rows"
    return out
