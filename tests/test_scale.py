"""Area-average downscale on the host (csrc/vep/scale.cpp) against the independent oracle
(tests/scale_oracle.py): byte equality, no tolerance. The GPU kernel is then held to this CPU
implementation (tests/test_gpu_scale.py)."""
import numpy as np
import pytest

import scale_oracle as so


@pytest.mark.parametrize("kind", so.KINDS)
@pytest.mark.parametrize("sw,sh,ow,oh", so.SMALL_SHAPES)
def test_small_shapes_equal_oracle(native, kind, sw, sh, ow, oh):
    src = so.picture(kind, sw, sh)
    got = native.resize_area_cpu(src, ow, oh)
    assert got.shape == (oh, ow, 3) and got.dtype == np.uint8
    assert np.array_equal(got, so.resize_area(src, ow, oh))
    if (ow, oh) == (sw, sh):
        assert np.array_equal(got, src)  # the identity


def test_integer_ratio_is_rounded_block_mean(native):
    src = so.picture("noise", 48, 32)
    got = native.resize_area_cpu(src, 8, 8)  # 6 x 4 blocks
    blocks = src.reshape(8, 4, 8, 6, 3).astype(np.int64).sum(axis=(1, 3))
    assert np.array_equal(got, ((blocks + 12) // 24).astype(np.uint8))


def test_1080p_to_wall_tile(native):
    src = so.picture("noise", 1920, 1080)
    assert np.array_equal(native.resize_area_cpu(src, 320, 180), so.resize_area(src, 320, 180))


@pytest.mark.parametrize("sw,sh,ow,oh", so.BOUNDARY_SHAPES)
def test_accumulator_boundary(native, sw, sh, ow, oh):
    """255 * sw * sh on either side of 2^32: the sums of an all-255 picture are the largest there are."""
    white = so.picture("white", sw, sh)
    got = native.resize_area_cpu(white, ow, oh)
    assert got.min() == 255 and got.max() == 255
    noise = so.picture("noise", sw, sh)
    assert np.array_equal(native.resize_area_cpu(noise, ow, oh), so.resize_area(noise, ow, oh))


@pytest.mark.parametrize("sw,sh,ow,oh", [(640, 480, 320, 240), (64, 48, 1, 1)])
def test_oracle_against_pillow_box(sw, sh, ow, oh):
    """The oracle itself against Pillow's BOX filter, at integer ratios only (elsewhere BOX is
    another filter). Pillow rounds between its two passes, hence one level."""
    from PIL import Image

    src = so.picture("noise", sw, sh)
    pil = np.asarray(Image.fromarray(src).resize((ow, oh), Image.BOX))
    diff = np.abs(pil.astype(np.int64) - so.resize_area(src, ow, oh).astype(np.int64)).max()
    print(f"{sw}x{sh} -> {ow}x{oh}: largest difference to Pillow BOX {diff}")
    assert diff <= 1


def test_argument_checks(native):
    src = so.picture("noise", 16, 8)
    for w, h in [(17, 8), (16, 9), (0, 4), (4, 0), (-1, 4)]:
        with pytest.raises(Exception):
            native.resize_area_cpu(src, w, h)
    with pytest.raises(Exception):
        native.resize_area_cpu(src[:, :, :2], 4, 4)


def test_fit_geometry_exhaustive(native):
    for sw in range(1, 25):
        for sh in range(1, 25):
            for bw in range(1, 25):
                for bh in range(1, 25):
                    got = tuple(native.fit_geometry(sw, sh, bw, bh))
                    assert got == so.fit(sw, sh, bw, bh), (sw, sh, bw, bh)
                    assert got[0] <= min(sw, bw) and got[1] <= min(sh, bh) and min(got) >= 1


@pytest.mark.parametrize("box,want", [((320, 180), (320, 180)), ((320, 65535), (320, 180)), ((65535, 180), (320, 180)),
                                      ((320, 0), (320, 180)), ((0, 180), (320, 180)), ((4000, 4000), (1920, 1080))])
def test_fit_geometry_1080p(native, box, want):
    assert tuple(native.fit_geometry(1920, 1080, *box)) == want
    assert so.fit(1920, 1080, *box) == want


def test_wall_geometry(native):
    for n in range(1, 70):
        assert tuple(native.wall_geometry(n, 0, 320, 180)) == so.wall_geometry(n, None, 320, 180)
        for cols in (1, 2, 5, 8):
            assert tuple(native.wall_geometry(n, cols, 16, 9)) == so.wall_geometry(n, cols, 16, 9)
    assert tuple(native.wall_geometry(32, 8, 320, 180)) == (8, 4, 2560, 720)
