"""Shared helpers of the frame-history tests (test_history.py, test_gpu_history.py, test_resp.py):
streams, the reference decoders' outputs and the numpy narrowing oracle."""
import time

import numpy as np

from conftest import high_encoder


def now_ms():
    return int(time.time() * 1000)


def narrow_planes(y, uv, bit_depth=8, chroma_format=1):
    """numpy oracle of narrow_surface (codec.cpp): 4:2:2 chroma = rounded mean of each row pair
    taken BEFORE narrowing, then 8-bit sample = min(255, (v + rnd) >> (bd - 8))."""
    sh = bit_depth - 8
    rnd = (1 << sh) >> 1
    n8 = lambda p: np.minimum(255, (p.astype(np.int64) + rnd) >> sh).astype(np.uint8)
    c = uv.astype(np.int64)
    if chroma_format == 2:
        c = (c[0::2] + c[1::2] + 1) >> 1
    return np.ascontiguousarray(n8(y)), np.ascontiguousarray(n8(c))


def oracle_bgr(native, y, uv, bit_depth, chroma_format, crop_left, crop_top, width, height):
    y8, uv8 = narrow_planes(y, uv, bit_depth, chroma_format)
    return native.nv12_to_bgr_cpu(y8, uv8, crop_left, crop_top, width, height)


def avc_stream(native, n, w=176, h=144, **kw):
    """n access units of a High-profile stream and the reference decoder's outputs over them:
    (aus, outs) with outs = [(pts, frame_type, is_keyframe, BGR24)] in output order, and
    outs_upto[k] = how many of them the reference had produced after access unit k."""
    kw.setdefault("bframes", 2)
    kw.setdefault("gop", 12)
    enc = high_encoder(native, w, h, **kw)
    bd, cf = int(kw.get("bit_depth", 8)), int(kw.get("chroma_format", 1))
    ref = native.CpuDecoder()
    aus, outs, upto, kind = [], [], [], {}
    for _ in range(n):
        au = enc.next()
        aus.append(au)
        kind[enc.last_pts] = (enc.last_type, bool(au.keyframe))
        ref.decode(au)
        for pts, (y, uv) in ref.frames():
            outs.append((pts, kind[pts][0], kind[pts][1], oracle_bgr(native, y, uv, bd, cf, 0, 0, w, h)))
        upto.append(len(outs))
    return aus, outs, upto


def hevc_stream(native, n, w=64, h=64, **kw):
    c = native.HevcEncConfig()
    c.width, c.height, c.gop, c.qp = w, h, 12, 30
    c.bframes = 2
    for k, x in kw.items():
        setattr(c, k, x)
    enc, ref = native.HevcEncoder(c), native.HevcDecoder()
    aus, outs, upto, key = [], [], [], {}
    for _ in range(n):
        au = enc.next()
        aus.append(au)
        key[enc.last_pts] = bool(au.keyframe)
        for pts, _poc, t, (y, uv) in ref.decode(au):
            bd = 10 if y.dtype == np.uint16 else 8
            outs.append((pts, t, key[pts], oracle_bgr(native, y, uv, bd, 1, 0, 0, w, h)))
        upto.append(len(outs))
    return aus, outs, upto


def check_window(frames, want):
    """`frames` = read_history() result; `want` = the reference outputs it must equal, in order."""
    assert [m["pts"] for m, _ in frames] == [o[0] for o in want]
    seqs = [m["seq"] for m, _ in frames]
    assert seqs == list(range(seqs[0], seqs[0] + len(seqs))) if seqs else not want, seqs
    for (m, got), (pts, t, key, bgr) in zip(frames, want):
        assert m["frame_type"] == t and m["is_keyframe"] == key, (m, t, key)
        assert got.shape == bgr.shape and np.array_equal(got, bgr), f"pts {pts}: history frame differs from the reference"
