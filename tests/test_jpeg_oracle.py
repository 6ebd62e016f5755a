"""The CPU JPEG encoder against oracles that share nothing with it (jpeg_oracle.py): a strict
pure-Python stream reader validated against libjpeg, the documented arithmetic restated (exact
rule), and the float64 mathematics with its error bound (float rule, colour rule)."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_oracle as jo


def pillow_jpeg(bgr, q):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, "JPEG", quality=q, subsampling=2)
    return buf.getvalue()


def pillow_luma(data):
    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    im.load()
    assert im.mode == "L"
    return np.asarray(im)


# ------------------------------------------------------------------------- the oracle's own parts

def test_zigzag_walk():
    zz = jo.ZZ
    assert zz[:10] == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and zz[-3:] == [55, 62, 63]
    assert zz[35] == 56 and zz[36] == 57  # the turn at the bottom-left corner


def test_float_transform_is_orthonormal():
    assert np.allclose(jo.C @ jo.C.T, np.eye(8), atol=1e-15)
    p = np.random.default_rng(1).integers(-128, 128, (5, 8, 8)).astype(np.float64)
    d = jo.float_dct(p)
    assert np.allclose((d ** 2).sum(), (p ** 2).sum())
    assert np.allclose(d[:, 0, 0], p.sum(axis=(1, 2)) / 8.0)


def _blocks(kind, n, rng):
    if kind == "noise":
        return rng.integers(0, 256, (n, 8, 8)).astype(np.int64) - 128
    yy, xx = np.mgrid[0:8, 0:8]
    a, b = rng.uniform(-12, 12, (2, n, 1, 1))
    c = rng.uniform(0, 256, (n, 1, 1))
    return np.clip(np.floor(a * xx + b * yy + c), 0, 255).astype(np.int64) - 128


@pytest.mark.parametrize("kind,q,within_cap", [("noise", 1, True), ("noise", 25, True), ("noise", 50, True),
                                               ("noise", 85, False), ("noise", 100, False), ("ramps", 50, True),
                                               ("ramps", 85, True), ("ramps", 95, None)])
def test_integer_transform_stays_inside_its_bound(kind, q, within_cap):
    """The documented integer transform (c) against the float64 transform (d) on 2000 random
    blocks: the error never leaves ``bound``, and the share of coefficients the bound leaves
    undecidable (luma quantisers) is on the side of the 5 % cap that decides which inputs take the
    float rule."""
    p = _blocks(kind, 2000, np.random.default_rng(q * 2 + (kind == "ramps")))
    real = jo.format_dct(p) / 65536.0
    f = jo.float_dct(p.astype(np.float64))
    b = jo.bound(p)
    err = np.abs(real - f)
    Q = jo.ijg_tables(q)[0].reshape(8, 8).astype(np.float64)
    a = np.abs(f / Q)
    share = float((np.floor(a + 0.5 - b / Q) != np.floor(a + 0.5 + b / Q)).mean())
    print(f"{kind} q{q}: largest error {err.max():.4f}, largest bound {b.max():.4f}, smallest slack "
          f"{(b - err).min():.4f}, undecidable {share:.2%}")
    assert (err <= b).all()
    if within_cap is not None:  # (ramps at 95 are measured only: no case applies the float rule there)
        assert (share <= jo.UNDECIDABLE_CAP) == within_cap


# --------------------------------------------------------------------- the reader against libjpeg

@pytest.mark.parametrize("q", [50, 90])
@pytest.mark.parametrize("kind", ["noise", "gradient"])
@pytest.mark.parametrize("encoder", ["pillow", "ours"])
def test_reader_reconstructs_libjpegs_luma(native, encoder, kind, q):
    """The luma plane rebuilt from the reader's coefficients with a float64 IDCT differs from
    libjpeg's integer IDCT by at most one level. Pillow's streams come from an independent encoder
    and have no restart intervals; ours have them."""
    w, h = 200, 120
    img = jo.noise(w, h) if kind == "noise" else jo.gradient(w, h)
    data = pillow_jpeg(img, q) if encoder == "pillow" else native.jpeg_encode_cpu(img, q)
    st = jo.read_stream(data)
    assert (st.w, st.h) == (w, h) and st.sampling == [(2, 2), (1, 1), (1, 1)]
    assert st.dri == (0 if encoder == "pillow" else 3)
    ours, ref = jo.luma_plane(st).astype(np.int64), pillow_luma(data).astype(np.int64)
    assert ours.shape == ref.shape == (h, w)
    diff = np.abs(ours - ref)
    print(f"{encoder} {kind} q{q}: luma equal to libjpeg's {float((diff == 0).mean()):.3%}, largest difference {diff.max()}")
    assert diff.max() <= 1


def test_reader_rejects_what_a_strict_decoder_would(native):
    data = bytearray(native.jpeg_encode_cpu(jo.noise(200, 120), 50))
    jo.read_stream(bytes(data))
    first = data.index(b"\xff\xd0")
    bad = bytearray(data)
    bad[first + 1] = 0xD1  # RSTm out of order
    with pytest.raises(AssertionError, match="cycle"):
        jo.read_stream(bytes(bad))
    with pytest.raises(AssertionError):
        jo.read_stream(bytes(data[:first] + data[first + 2:]))  # an interval of 6 MCUs
    with pytest.raises(AssertionError, match="EOI"):
        jo.read_stream(bytes(data) + b"\0")
    with pytest.raises(AssertionError):
        jo.read_stream(bytes(data[:first - 1] + data[first:]))  # an interval that lost its last byte


# ----------------------------------------------------------------------------------- colour

def test_colour_formulas_over_all_colours():
    """The documented 16.16 formulas against the float64 JFIF definition over all 2^24 colours."""
    g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    und = np.zeros(3)
    for r in range(256):
        rr = np.full_like(g, r)
        f = jo.float_colour(b, g, rr)
        s = jo.format_colour(b, g, rr)
        for k in range(3):
            und[k] += jo.check_colour(f"r {r} {'Y Cb Cr'.split()[k]}", s[k], f[k])
    und /= 256
    print(f"undecidable over 2^24 colours: Y {und[0]:.2%} Cb {und[1]:.2%} Cr {und[2]:.2%}")
    assert [round(100 * u, 2) for u in und] == [1.10, 1.06, 1.22]


def test_constant_blocks_code_as_their_dc(native):
    """Quality 100, one grey per MCU, all 256 of them: DC = 8 * (s - 128) and no AC, which is what
    lets the "colours" and "cells" cases read samples back from a stream."""
    greys = np.arange(256, dtype=np.uint8)
    img = np.ascontiguousarray(np.broadcast_to(np.repeat(greys, 16)[None, :, None], (16, 4096, 3)))
    st = jo.read_stream(native.jpeg_encode_cpu(img, 100))
    assert all((t == 1).all() for t in st.qt.values())
    s = jo.constant_samples("greys", st.coefs, [0, 1, 2, 3, 4, 5])
    assert (s[:, :4] == greys[:, None]).all() and (s[:, 4:] == 128).all()


# ------------------------------------------------------------------------------ per picture

@pytest.mark.parametrize("case", list(jo.CASES))
def test_coefficients_follow_the_rules(native, case):
    """Exact rule at every listed quality, float rule where the table says so; "colours" and
    "cells" also through the samples read back from the DCs."""
    res = jo.check_case(case, native.jpeg_encode_cpu)
    assert len(res) == len(jo.CASES[case][4])
    assert all(share <= jo.UNDECIDABLE_CAP for _, share, _ in res)


@pytest.mark.parametrize("q", [1, 25, 50, 85, 100])
def test_structure_from_the_reader(native, q):
    w, h = 200, 120
    st = jo.read_stream(native.jpeg_encode_cpu(jo.gradient(w, h), q))
    jo.check_structure("gradient", st, w, h, q)  # size, 2x2 1x1 1x1, DRI 3, DQT = the IJG rule
    assert st.rst == [k % 8 for k in range(34)] and st.interval_mcus == [3] * 34 + [2]
