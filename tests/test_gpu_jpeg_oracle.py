"""gfx950 JPEG encoder against oracles that share nothing with it (jpeg_oracle.py), and at the
sizes where the scan and gather kernels change path (run on an MI355X).

test_gpu_jpeg.py holds the kernels to the CPU encoder byte for byte; both take every line of
arithmetic from jpeg.h. Here the streams the kernels return are read by the strict pure-Python
reader and their coefficients held against the documented arithmetic restated (exact rule) and the
float64 mathematics with its bound (float rule, colour rule)."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_oracle as jo
from conftest import high_encoder, synth

pytestmark = pytest.mark.gpu

SCAN_THREADS = 1024  # jpeg_scan_kernel: per = ceil(intervals / 1024) intervals per thread


def gpu_encode(img, q):
    from video_edge_ai_proxy_amd import ops

    return ops.jpeg_encode(torch.from_numpy(np.ascontiguousarray(img)).cuda(), q)


# ---------------------------------------------------------------------------- coefficient level

@pytest.mark.parametrize("case", list(jo.CASES))
def test_coefficients_follow_the_rules(case):
    """Every case of jpeg_oracle.CASES: exact rule at all its qualities, float rule at the bracketed
    ones; "colours" and "cells" through the samples read back from the DCs at quality 100."""
    res = jo.check_case(case, gpu_encode)
    assert len(res) == len(jo.CASES[case][4])
    assert all(share <= jo.UNDECIDABLE_CAP for _, share, _ in res)


# -------------------------------------------------------------------------------- stream level

# (w, h) -> (MCUs, intervals, per): what the shape sits on
BOUNDARY = {
    (1024, 768): (3072, 1024, 1),    # the last per = 1 size: every scan thread owns one interval
    (112, 7024): (3073, 1025, 2),    # first per = 2: threads from 513 up own nothing, last interval of 1 MCU
    (1200, 656): (3075, 1025, 2),    # the same with a full last interval
    (256, 6144): (6144, 2048, 2),    # last per = 2
    (80, 19664): (6145, 2049, 3),    # first per = 3: threads from 683 up own nothing
    (65535, 1): (4096, 1366, 2),     # mcus_x = 4096, 15 of 16 rows replicated, last column 1 pixel wide
    (1, 65535): (4096, 1366, 2),     # mcus_x = 1, last row 1 pixel high
}


def check_stream(x, q, what):
    from video_edge_ai_proxy_amd import ops

    h, w = x.shape[:2]
    want = ops.jpeg_encode_reference(x, q)
    got = ops.jpeg_encode(x.cuda(), q)
    assert got == want, f"{what} {w}x{h} q{q}: {len(got)} vs {len(want)} bytes"
    assert Image.open(io.BytesIO(got)).size == (w, h)
    return got


@pytest.mark.parametrize("content", ["noise", "constant"])
@pytest.mark.parametrize("w,h", list(BOUNDARY))
def test_scan_boundaries_and_extreme_aspects(w, h, content):
    """Noise at quality 50: segment lengths vary and fall on both sides of the gather kernel's
    64-byte strides. The constant picture makes every segment equal and tiny."""
    mcus = -(-w // 16) * -(-h // 16)
    n = -(-mcus // jo.RESTART_INTERVAL)
    per = -(-n // SCAN_THREADS)
    assert (mcus, n, per) == BOUNDARY[(w, h)], ("with another restart interval or MCU size the shapes no longer sit on "
                                                "the scan kernel's boundaries: choose them again")
    assert w * h < 3.3e6
    if content == "noise":
        x = torch.from_numpy(jo.noise(w, h))
    else:
        x = torch.full((h, w, 3), 77, dtype=torch.uint8)
    check_stream(x, 50, content)


def test_scratch_shrinks_and_grows_again():
    """One thread, one pool: the small pictures run in scratch that still holds the large picture's
    lengths, offsets and segments behind their own intervals."""
    for w, h in [(1200, 656), (1, 1), (17, 9), (1200, 656)]:
        check_stream(torch.from_numpy(jo.noise(w, h)), 50, "scratch reuse")


# -------------------------------------------------------------------------------- ring path

def _ring_frame(native, wk, cam, enc, n, w, h, q):
    for _ in range(n):
        wk.decode_now(cam, enc.next())
    assert wk.stats(cam)["published"] == n and wk.stats(cam)["errors"] == 0
    meta, frame = wk.read_latest(cam, 0)
    jmeta, jpg = wk.read_latest_jpeg(cam, 0, q)
    assert jmeta["seq"] == meta["seq"]
    assert frame.shape == (h, w, 3)
    assert jpg == native.jpeg_encode_cpu(frame, q)
    st = jo.read_stream(jpg)
    jo.check_structure(f"ring {w}x{h}", st, w, h, q)
    jo.check_exact(f"ring {w}x{h}", st.coefs, frame, q)


def test_ring_path_at_cropped_sizes(native):
    """A 200 x 120 camera (coded height 128: the ring slot is the cropped picture, not the coded
    one) and an H.264 High 10 camera at 176 x 144 (the slot holds the narrowed 8-bit picture)."""
    wk = native.Worker(device=0, letterbox_size=0, max_cameras=2)
    _ring_frame(native, wk, wk.add_camera("cropped", 2), synth(native, 200, 120, gop=4, seed=3), 2, 200, 120, 85)
    _ring_frame(native, wk, wk.add_camera("high10", 4), high_encoder(native, 176, 144, bit_depth=10, seed=5, bframes=0),
                3, 176, 144, 50)
