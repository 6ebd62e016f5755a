"""Frame history on gfx950: the surface_to_bgr kernel (any supported sample format -> BGR24, the
narrowing in registers) against a numpy + nv12_to_bgr_cpu oracle, its batched launch, and GPU
workers whose multi-picture jobs publish every output: each history frame is converted between
reconstruction rounds, while its DPB surface is intact, and equals the CPU decoder's bit for bit."""
import numpy as np
import pytest
import torch

from history_util import avc_stream, check_window, hevc_stream, now_ms, oracle_bgr

pytestmark = pytest.mark.gpu


def planes(seed, cw, ch, bd, cf):
    """Random coded planes over the whole sample range (peaks included, so the saturating
    narrowing and the BT.601 clipping both happen)."""
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bd == 8 else np.uint16
    top = (1 << bd) - 1
    y = rng.integers(0, top + 1, (ch, cw)).astype(dt)
    uv = rng.integers(0, top + 1, (ch if cf == 2 else ch // 2, cw)).astype(dt)
    y[0, :4] = top
    uv[0, :4] = top
    uv[-1, -4:] = 0
    return y, uv


SHAPES = {
    "48x32-crop": (48, 32, 3, 2, 41, 27),    # ragged left / right edges, odd crop, unaligned rows
    "176x144": (176, 144, 0, 0, 176, 144),   # two tile columns, five tile rows, aligned stores
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("cf", [1, 2])
@pytest.mark.parametrize("bd", [8, 10])
def test_surface_to_bgr_matches_the_oracle(native, bd, cf, shape):
    from video_edge_ai_proxy_amd import ops

    cw, ch, cl, ct, w, h = SHAPES[shape]
    y, uv = planes(bd * 10 + cf, cw, ch, bd, cf)
    want = oracle_bgr(native, y, uv, bd, cf, cl, ct, w, h)
    got = ops.surface_to_bgr(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda(), bit_depth=bd,
                             chroma_format=cf, width=w, height=h, crop_left=cl, crop_top=ct)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == (h, w, 3)
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"


def test_surface_to_bgr_rejects_bad_geometry(native):
    from video_edge_ai_proxy_amd import ops

    y = torch.zeros((32, 48), dtype=torch.uint8, device="cuda")
    uv = torch.zeros((16, 48), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        ops.surface_to_bgr(y, uv, width=48, height=32, crop_left=1)  # window leaves the picture
    with pytest.raises(TypeError):
        ops.surface_to_bgr(y, uv, bit_depth=10)
    with pytest.raises(ValueError):
        ops.surface_to_bgr(y, uv, chroma_format=2)  # 4:2:2 needs a full-height chroma plane
    with pytest.raises(native.NativeError):  # the binding checks what it launches, too
        native.surface_to_bgr(y.data_ptr(), uv.data_ptr(), 48, 48, 32, 8, 1, 8, 0, 48, 32, y.data_ptr(), 0)


def test_batched_launch_three_formats(native):
    """Three pictures of different sizes and formats in ONE launch (descriptor found by the tile
    prefix search); the bytes after each output keep their guard pattern."""
    from video_edge_ai_proxy_amd import ops

    cases = [(48, 32, 8, 1, 3, 2, 41, 27), (176, 144, 10, 2, 0, 0, 176, 144), (272, 48, 10, 1, 16, 1, 250, 40)]
    guard, pics, bufs, wants = 256, [], [], []
    for k, (cw, ch, bd, cf, cl, ct, w, h) in enumerate(cases):
        y, uv = planes(100 + k, cw, ch, bd, cf)
        wants.append(oracle_bgr(native, y, uv, bd, cf, cl, ct, w, h))
        buf = torch.full((h * w * 3 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        bufs.append(buf)
        pics.append(dict(y=torch.from_numpy(y).cuda(), uv=torch.from_numpy(uv).cuda(), bit_depth=bd, chroma_format=cf,
                         width=w, height=h, crop_left=cl, crop_top=ct, out=buf[:h * w * 3].view(h, w, 3)))
    outs = ops.surface_to_bgr_batch(pics)
    torch.cuda.synchronize()
    for out, buf, want in zip(outs, bufs, wants):
        assert np.array_equal(out.cpu().numpy(), want)
        assert bool((buf[-guard:] == 0xA5).all()), "bytes past the output were written"


STREAMS = {
    "h264-high": ("avc", 176, 144, 12, 5, dict()),
    "h264-high10": ("avc", 176, 144, 12, 5, dict(bit_depth=10, seed=5)),
    "h264-422": ("avc", 176, 144, 12, 5, dict(chroma_format=2)),
    "h265-64": ("hevc", 64, 64, 12, 5, dict()),
    "h264-1080p": ("avc", 1920, 1080, 8, 4, dict(qp=26)),
}


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_worker_catch_up_is_bit_exact(native, name):
    """n - 1 access units nobody watches, a query, one more: one job of n pictures. The history
    holds the H newest outputs of the CPU reference decoder, in order, each bit-exact."""
    kind, w, h, n, H, kw = STREAMS[name]
    aus, outs, upto = (avc_stream if kind == "avc" else hevc_stream)(native, n, w, h, **kw)
    assert upto[n - 1] > H, "the reference alone must have more outputs than the history holds"
    wk = native.Worker(device=0)
    wk.start()
    try:
        cam = wk.add_camera("catchup", 2, H)
        for au in aus[:n - 1]:
            assert wk.submit_au(cam, au) is False
        wk.set_last_query(cam, now_ms())
        assert wk.submit_au(cam, aus[n - 1])
        wk.flush()
        frames = wk.read_history(cam)
        st = wk.stats(cam)
    finally:
        wk.stop()
    assert len(frames) == H and st["published"] == H and st["errors"] == 0
    check_window(frames, outs[:upto[n - 1]][-H:])
    assert st["history_skipped"] == upto[n - 1] - H
    assert st["ring_slots"] >= wk.history_ring_slots(H)


def test_worker_decode_many_and_retention(native):
    """merge_job path on the GPU, then single-picture jobs: the window slides by one per frame."""
    aus, outs, upto = avc_stream(native, 16)
    wk = native.Worker(device=0)
    cam = wk.add_camera("many", 2, 5)
    wk.decode_many([(cam, aus[:11])])
    check_window(wk.read_history(cam), outs[:upto[10]][-5:])
    for i in range(11, 16):
        wk.decode_now(cam, aus[i])
        frames = wk.read_history(cam)
        assert len(frames) == 5
        check_window(frames, outs[:upto[i]][-5:])
    assert wk.stats(cam)["published"] == 5 + (upto[15] - upto[10])


def test_history_zero_is_the_old_camera(native):
    """add_camera(..., history=0) is the camera of before: same frames, same counters."""
    aus, outs, upto = avc_stream(native, 8)
    wk = native.Worker(device=0)
    a = wk.add_camera("explicit", 4, history=0)
    b = wk.add_camera("implicit", 4)
    keys = ("packets", "decoded", "skipped", "shed", "errors", "bytes_in", "decoder", "published", "width", "height",
            "ring_slots", "history", "history_skipped")
    for i, au in enumerate(aus):
        wk.decode_now(a, au)
        wk.decode_now(b, au)
        ra, rb = wk.read_latest(a, 0), wk.read_latest(b, 0)
        assert (ra is None) == (rb is None)
        if ra is not None:
            assert ra[0]["seq"] == rb[0]["seq"] and ra[0]["pts"] == rb[0]["pts"] and np.array_equal(ra[1], rb[1])
            assert np.array_equal(ra[1], outs[upto[i] - 1][3])
    sa, sb = wk.stats(a), wk.stats(b)
    assert {k: sa[k] for k in keys} == {k: sb[k] for k in keys}
    assert sa["history"] == 0 and sa["history_skipped"] == 0 and len(wk.read_history(a)) == 1
