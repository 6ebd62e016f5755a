"""Main / High profile H.264 on the CPU reference decoder.

* A real third-party High-profile clip: imageio's `realshort.mp4` (320x240, CABAC, 8x8
  transform + Intra_8x8, Intra_4x4, P pictures, two IDRs), present in this image under
  /opt/conda. Nothing in the image can decode it for a pixel reference (no FFmpeg / PyAV /
  OpenCV), so parity is *unpinned*: the test checks that every access unit decodes through the
  CABAC engine without a desync (any CABAC table or binarization error desynchronises the
  arithmetic decoder within a few macroblocks and ends in a range / overrun error or a wrong
  end_of_slice position), that the syntax it exercises is what the clip is known to contain,
  and that the pictures are temporally coherent (a desync or a wrong predictor produces
  garbage that breaks frame-to-frame similarity).
* Closed-loop High-profile streams from the synthetic encoder (CABAC / CAVLC, B pyramids,
  8x8, weighted prediction) where the encoder's reconstruction is the reference.
"""
import os

import numpy as np
import pytest

# imageio's sample clip realshort.mp4 (its resources/images collection), stored with the tests
CLIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "realshort.mp4")


def clip_aus(native):
    from video_edge_ai_proxy_amd.utils import mp4

    buf = open(CLIP, "rb").read()
    tr = mp4.parse(buf)
    out = []
    for i, (nals, key, dts, pts) in enumerate(mp4.samples(buf, tr)):
        au = native.AccessUnit.from_nals((tr.param_sets if i == 0 else []) + nals, keyframe=key,
                                         pts=pts, dts=dts)
        out.append(au)
    return tr, out


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


@pytest.mark.skipif(not os.path.exists(CLIP), reason="imageio sample clip not in this image")
def test_third_party_high_profile_cabac_clip(native):
    tr, aus = clip_aus(native)
    assert tr.codec == "avc1" and (tr.width, tr.height) == (320, 240) and len(aus) == 36
    dec = native.CpuDecoder()
    frames = [dec.decode(au) for au in aus]
    assert all(f is not None and f.shape == (240, 320, 3) for f in frames)
    st = dec.mb_stats
    # CABAC High profile syntax the clip is known to use
    assert st["types"] == "I" + "P" * 29 + "I" + "P" * 5
    assert st["i8x8"] > 0 and st["i4x4"] > 0 and st["t8x8"] > 1000 and st["skip"] > 0 and st["inter"] > 1000
    # natural content, temporally coherent (a CABAC desync or drift destroys both)
    for f in frames:
        assert f.std() > 20
    sims = [psnr(frames[i], frames[i + 1]) for i in range(len(frames) - 1)]
    assert min(sims) > 14 and np.median(sims) > 20, sims
    # the clip's two GOPs show the same scene (the IDR at 30 re-anchors it)
    assert psnr(frames[29], frames[30]) > 15


@pytest.mark.skipif(not os.path.exists(CLIP), reason="imageio sample clip not in this image")
def test_third_party_clip_corruption_never_crashes(native):
    """Bit flips in the CABAC slice data of the real clip: every access unit either decodes or
    raises; the stream recovers at its next IDR."""
    import random

    _, aus = clip_aus(native)
    clean = native.CpuDecoder()
    want = [clean.decode(a) for a in aus]
    rnd = random.Random(11)
    for trial in range(6):
        dec = native.CpuDecoder()
        bad_at = rnd.randrange(1, 29)
        broken = False
        for i, au in enumerate(aus):
            if i == bad_at:
                nals = [bytearray(n) for n in au.nals()]
                k = [j for j, x in enumerate(nals) if (x[0] & 0x1F) in (1, 5)][0]
                for _ in range(rnd.randint(1, 4)):
                    pos = rnd.randrange(4, len(nals[k]))
                    nals[k][pos] ^= 1 << rnd.randrange(8)
                au = native.AccessUnit.from_nals([bytes(x) for x in nals], keyframe=au.keyframe)
            try:
                got = dec.decode(au)
            except (native.NativeError, native.UnsupportedStream):
                broken = True
                continue
            if i >= 30:
                assert got is not None and np.array_equal(got, want[i]), f"trial {trial}: frame {i}"
        assert isinstance(broken, bool)


# ---------------------------------------------------------------------------------------------
# Closed-loop Main / High encoder (avc::AvcHighEncoder) <-> CPU decoder. The encoder writes
# every macroblock through the decoder's own macroblock layer (write mode) and reconstructs it
# with the decoder's reconstruction, so these round trips pin that both directions of the
# symmetric layer agree and that the slice / DPB / reference-list / output-order layers of the
# encoder and the decoder match. (The spec conformance of the B-slice CABAC syntax itself is
# pinned by no third-party stream available here: parity unpinned beyond this closed loop and
# the spec-derived table tests.)
from conftest import high_encoder, roundtrip  # noqa: E402

HIGH_CONFIGS = {
    "high-cabac-ibbp-pyramid": dict(bframes=2),
    "high-cabac-ibbbp-temporal": dict(bframes=3, direct_spatial=False),
    "high-cavlc-ibp": dict(bframes=1, cabac=False),
    "main-cabac-ibbp": dict(bframes=2, t8x8=False),
    "high-weighted-explicit": dict(bframes=2, weighted_p=True, weighted_b=1),
    "high-weighted-implicit-temporal": dict(bframes=3, weighted_b=2, direct_spatial=False),
    "cov-cabac": dict(bframes=2, coverage=True),
    "cov-cavlc-temporal": dict(bframes=2, coverage=True, cabac=False, direct_spatial=False),
    "cov-scaling-slices-wp": dict(bframes=3, coverage=True, scaling=True, slices=3, weighted_b=1,
                                  weighted_p=True, chroma_qp_offset=-2, second_chroma_qp_offset=3),
    "cov-implicit-dbk2": dict(bframes=2, coverage=True, direct_spatial=False, weighted_b=2,
                              slices=2, deblock_idc=2),
    "cov-refs4-nopyramid": dict(bframes=2, pyramid=False, refs=4, coverage=True, gop=7),
}


@pytest.mark.parametrize("name", sorted(HIGH_CONFIGS))
def test_high_encoder_roundtrip_bit_exact(native, name):
    kw = HIGH_CONFIGS[name]
    enc = high_encoder(native, 176, 144, gop=kw.pop("gop", 12), seed=7, **kw)
    rec, got, dec, _ = roundtrip(native, enc, 20)
    assert len(rec) == 20 and set(got) == set(rec)
    for pts in sorted(rec):
        ey, euv = rec[pts]
        gy, guv = got[pts]
        assert np.array_equal(ey, gy) and np.array_equal(euv, guv), f"{name}: pts {pts} differs"
    st = dec.mb_stats
    bf = HIGH_CONFIGS[name].get("bframes", 2)
    assert "B" in st["types"] if bf else "B" not in st["types"]
    if bf:
        assert st["bipred"] > 0 and st["list1_only"] > 0
    if HIGH_CONFIGS[name].get("t8x8", True):
        assert st["t8x8"] > 0 and st["i8x8"] > 0
    if HIGH_CONFIGS[name].get("weighted_b") or HIGH_CONFIGS[name].get("weighted_p"):
        assert st["weighted"] > 0
    if HIGH_CONFIGS[name].get("coverage"):
        assert st["i4x4"] > 0 and st["i16x16"] > 0 and st["pcm"] > 0 and st["skip"] > 0


def test_high_encoder_output_order_and_quality(native):
    """Realistic (non-coverage) High CABAC IBBP: frames leave the decoder in display order, one
    per access unit overall, and the reconstruction is close to the source scene."""
    enc = high_encoder(native, 320, 240, bframes=3, gop=16, seed=2, qp=26)
    dec = native.CpuDecoder()
    order, src = [], {}
    for _ in range(24):
        au = enc.next()
        src[enc.last_pts] = enc.source()[0].copy()
        dec.decode(au)
        order += [pts for pts, _ in dec.frames()]
        rec = enc.picture()[0]
        err = rec[:240, :320].astype(float) - src[enc.last_pts][:240, :320]
        assert 10 * np.log10(255.0 ** 2 / max(1e-9, (err ** 2).mean())) > 33
    order += [pts for pts, _ in dec.flush_frames()]
    assert order == sorted(order) and len(order) == 24


def test_high_profile_synth_camera(native):
    """SynthConfig.profile routes the synthetic camera to the High encoder (what the camera farm
    and bench --profile high stream)."""
    c = native.SynthConfig()
    c.width, c.height, c.gop, c.compressed, c.profile, c.bframes = 176, 144, 8, True, "high", 2
    s = native.SynthH264(c)
    nal_types = []
    dec = native.CpuDecoder()
    outs = 0
    for _ in range(10):
        au = s.next()
        nal_types += [n[0] & 0x1F for n in au.nals()]
        outs += dec.decode(au) is not None
    assert nal_types[:2] == [7, 8] and 5 in nal_types
    sps = native.parse_sps(s.sps_nal)
    assert sps["profile_idc"] == 100
    assert "B" in dec.mb_stats["types"] and outs >= 7  # (reorder depth 2 still holds some)
    c.profile = "bogus"
    with pytest.raises(native.NativeError):
        native.SynthH264(c)


def test_high_stream_corruption_never_crashes(native):
    """Bit flips in CABAC B / P slices: the decoder raises or decodes, never crashes, and
    recovers bit-exact at the next IDR."""
    import random

    rnd = random.Random(5)
    enc = high_encoder(native, 176, 144, bframes=2, gop=8, seed=9, coverage=True)
    aus = [enc.next() for _ in range(24)]
    clean = native.CpuDecoder()
    want = {}
    for a in aus:
        clean.decode(a)
        for pts, (y, uv) in clean.frames():
            want[pts] = y
    for trial in range(12):
        dec = native.CpuDecoder()
        bad = rnd.randrange(1, 14)
        for i, a in enumerate(aus):
            if i == bad:
                nals = [bytearray(n) for n in a.nals()]
                sl = [k for k, x in enumerate(nals) if (x[0] & 0x1F) in (1, 5)][0]
                for _ in range(rnd.randint(1, 5)):
                    pos = rnd.randrange(3, len(nals[sl]))
                    nals[sl][pos] ^= 1 << rnd.randrange(8)
                a = native.AccessUnit.from_nals([bytes(x) for x in nals], pts=a.pts, dts=a.dts, keyframe=a.keyframe)
            try:
                dec.decode(a)
            except (native.NativeError, native.UnsupportedStream):
                continue
            if i >= 16:  # pictures from the IDR at display 16 on equal the clean stream's
                for pts, (y, uv) in dec.frames():
                    if pts < 18 * 3000:  # (pts = (display + reorder depth 2) * 3000)
                        continue
                    assert np.array_equal(y, want[pts]), f"trial {trial} pts {pts}"


def test_lost_slice_is_concealed(native):
    """A picture that loses one of its slices still decodes: the MBs no slice covered are
    concealed from the first reference (P_Skip-like records, every record in range), the other
    slices' MBs decode normally, and the next IDR is bit-exact again."""
    enc = high_encoder(native, 176, 144, bframes=0, gop=6, seed=11, slices=3)
    dec = native.CpuDecoder()
    recon, got = {}, {}
    lost_pts = None
    for i in range(12):
        au = enc.next()
        y, uv = enc.picture()
        recon[enc.last_pts] = (y.copy(), uv.copy())
        if i == 3:  # a P picture: drop its second slice NAL
            nals = au.nals()
            slices = [k for k, n in enumerate(nals) if (n[0] & 0x1F) in (1, 5)]
            assert len(slices) == 3
            del nals[slices[1]]
            au = native.AccessUnit.from_nals(nals, au.pts, au.dts, au.keyframe)
            lost_pts = enc.last_pts
        dec.decode(au)
        got.update(dict(dec.frames()))
    got.update(dict(dec.flush_frames()))
    assert lost_pts in got and len(got) == 12
    ey, gy = recon[lost_pts][0], got[lost_pts][0]
    assert not np.array_equal(gy, ey)  # the lost rows are concealed, not decoded
    assert np.array_equal(gy[:16], ey[:16])  # the first slice's rows are untouched by the loss
    last = max(got)  # the GOP after the loss starts with an IDR: bit-exact again
    assert np.array_equal(got[last][0], recon[last][0])
