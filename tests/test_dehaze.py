"""The CPU twin of the dehazing (csrc/vep/dehaze.cpp) against the independent integer oracle, plane
by plane and exactly; against the float64 pipeline within the bound docs/DEHAZE.md derives from the
fixed-point widths; its closed forms; and that it dehazes the synthetic scene."""
import numpy as np
import pytest
import torch

from dehaze_oracle import dehaze_float, dehaze_int, hazy_scene

SHAPES = [(16, 16), (67, 19), (130, 34), (257, 65)]


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize("radius", [1, 16])
@pytest.mark.parametrize("patch", [3, 31])
@pytest.mark.parametrize("shape", SHAPES)
def test_twin_equals_the_integer_oracle(native, shape, patch, radius):
    from video_edge_ai_proxy_amd import dehaze as dh

    w, h = shape
    noise = np.random.default_rng(w + patch + radius).integers(0, 256, (h, w, 3)).astype(np.uint8)
    for strength, img in ((0.0, noise), (0.5, hazy_scene(w, h)[1]), (1.0, noise)):
        p = dh.to_native(patch, 0.95, 0.1, radius, strength)
        out, words = native.dehaze_cpu(img, *p)
        got, want = dh.split_planes(words, w, h), dehaze_int(img, *p)
        assert np.array_equal(got["table"], want["table"]) and np.array_equal(got["air"], want["air"])
        assert np.array_equal(got["norm"].view(np.uint8).reshape(3, 256), want["norm"])
        assert np.array_equal(got["cell"], want["cell"])
        for name in ("ab", "mean"):
            assert np.array_equal(got[name].view(np.int32), want[name]), name
        assert np.array_equal(out, want["out"])
        if strength == 0.0:
            assert np.array_equal(out, img)  # the identity, byte for byte


@pytest.mark.parametrize("kind", ["scene", "noise"])
def test_twin_within_the_derived_bound_of_float64(native, kind):
    """docs/DEHAZE.md: t deviates by at most DT = 16 / 1024 (quantisation of N 1.9, of A 512 / A_min
    < 3, six roundings of 1/2 on the way, doubled for the guided filter's weights), and a pixel by
    1 + |I - A| (1 / (t - DT) - 1 / t) + (1 / t - 1) / 2. Measured on the scene: t 2.2 / 1024, the
    picture 1.32 levels at most and 0.27 in the mean; on noise 0.34 and 0.05."""
    img = hazy_scene()[1] if kind == "scene" else np.random.default_rng(5).integers(0, 256, (96, 160, 3)).astype(np.uint8)
    out = native.dehaze_cpu(img, 15, 243, 102, 8, 256)[0]
    want, t, air = dehaze_float(img, 15, 243 / 256, 102 / 1024, 8, 1.0)
    dt = 16 / 1024
    bound = 1 + np.abs(img - air) * (1 / (t - dt) - 1 / t)[..., None] + (1 / t - 1)[..., None] / 2
    dev = np.abs(out - want)
    # t itself, in units of 1/1024: at most DT, and in the mean at most the two systematic terms
    # (N's quantisation 0.95, A's rounding 512 / A_min) plus six roundings of mean 1/4
    t_dev = np.abs(dehaze_int(img, 15, 243, 102, 8, 256)["t"] - 1024 * t)
    t_mean_bound = 0.95 + 512 / air.min() + 1.5
    print(kind, "largest", dev.max(), "mean", dev.mean(), "largest bound", bound.max(), "t largest", t_dev.max(), "t mean",
          t_dev.mean(), "t mean bound", t_mean_bound)
    assert (dev <= bound).all() and t_dev.max() <= 16 and t_dev.mean() <= t_mean_bound


def test_closed_forms(native):
    one = np.full((40, 50, 3), (0, 130, 255), np.uint8)
    assert np.array_equal(native.dehaze_cpu(one)[0], one)  # one colour, which is I = A everywhere
    img = hazy_scene(80, 48)[1]
    for t0 in (0.05, 0.5, 1.0):
        out, words = native.dehaze_cpu(img, 15, 256, int(round(t0 * 1024)), 8, 256)
        air = words[1024:1027].astype(np.int64)
        assert (np.abs(out - air) <= np.abs(img - air) * 1024 / int(round(t0 * 1024)) + 1).all()  # t0 bounds the gain
    assert np.array_equal(native.dehaze_cpu(img, 15, 256, 1024, 8, 256)[0], img)  # t = 1: nothing is taken off
    for bad in ((4, 243, 102, 8, 256), (33, 243, 102, 8, 256), (15, 257, 102, 8, 256), (15, 243, 50, 8, 256),
                (15, 243, 102, 17, 256), (15, 243, 102, 8, 257)):
        with pytest.raises(ValueError):
            native.dehaze_cpu(img, *bad)
    with pytest.raises(ValueError):
        native.dehaze_cpu(img[:15])


def test_it_dehazes(native):
    """The synthetic scene of docs/DEHAZE.md: the float64 pipeline must gain what the float prototype
    of the design gained on such a scene, 3.8 dB (it gains 5.9), and the integer twin is held to
    within 0.5 dB of the float64 pipeline's own gain."""
    from video_edge_ai_proxy_amd import dehaze as dh, ops

    clear, hazy, _ = hazy_scene()
    out, words = ops.dehaze(torch.from_numpy(hazy), planes=True)
    before, twin, ideal = psnr(hazy, clear), psnr(out.numpy(), clear), psnr(dehaze_float(hazy, 15, 0.95, 0.1, 8, 1.0)[0], clear)
    print("PSNR hazy", before, "twin", twin, "float64", ideal)
    assert ideal - before >= 3.8 and abs((twin - before) - (ideal - before)) <= 0.5
    # the estimated A lies between the scene's brightest haze A (1 - t_lo) and the true A
    air = dh.split_planes(words.numpy(), 160, 96)["air"][:3]
    true = np.array((230, 225, 220))
    assert (air >= true * (1 - 0.35)).all() and (air <= true).all()
