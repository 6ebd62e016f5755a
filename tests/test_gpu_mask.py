"""gfx950 privacy masks: byte equality of the kernel with the CPU implementation, inside guarded
buffers, and the Worker's publish path (run on an MI355X). The CPU implementation is held to the
independent oracle in tests/test_mask.py."""
import threading

import numpy as np
import pytest
import torch

import mask_oracle as mo
from conftest import synth
from history_util import avc_stream, hevc_stream
from video_edge_ai_proxy_amd import privacy

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
GUARD = 96


def run_guarded(p, masks, lead=0):
    """ops.privacy_mask on a view into a larger device buffer, `lead` bytes further in (the picture
    then starts at any byte offset modulo 16). Returns the picture; asserts the guards are intact."""
    from video_edge_ai_proxy_amd import ops

    h, w = p.shape[:2]
    n = h * w * 3
    buf = torch.full((GUARD + lead + n + GUARD,), SENTINEL, dtype=torch.uint8).cuda()
    view = buf[GUARD + lead:GUARD + lead + n].view(h, w, 3)
    view.copy_(torch.from_numpy(p).cuda())
    out = ops.privacy_mask(view, masks)
    assert out is view
    host = buf.cpu().numpy()
    assert (host[:GUARD + lead] == SENTINEL).all() and (host[GUARD + lead + n:] == SENTINEL).all(), "guard bytes written"
    return host[GUARD + lead:GUARD + lead + n].reshape(h, w, 3)


def check(p, masks, lead=0, what=""):
    """kernel == CPU twin, byte for byte; bytes outside every rect unchanged."""
    from video_edge_ai_proxy_amd import ops

    got = run_guarded(p, masks, lead)
    want = ops.privacy_mask_reference(torch.from_numpy(p), masks).numpy()
    assert np.array_equal(got, want), f"{what} {p.shape} {masks}: {int((got != want).sum())} bytes differ"
    h, w = p.shape[:2]
    outside = np.ones((h, w), bool)
    for m in masks:
        x0, y0, x1, y1 = mo.to_pixels(w, h, m)
        outside[y0:y1, x0:x1] = False
    assert np.array_equal(got[outside], p[outside]), f"{what}: bytes outside the rects changed"


@pytest.mark.parametrize("size", [(7, 5), (17, 9), (1, 9), (9, 1), (64, 48), (200, 120)])
def test_byte_equal(size):
    w, h = size
    for kind in ("noise", "gradient"):
        p = mo.picture(kind, w, h, seed=w + h)
        for k, m in enumerate(mo.cases(w, h)):
            check(p, [m], lead=k % 16, what=kind)


def test_byte_equal_block_128():
    p = mo.picture("noise", 300, 260, seed=3)
    for k, m in enumerate(mo.cases(300, 260, blocks=(128,))):
        check(p, [m], lead=k % 16)


def test_byte_equal_wide_strip():
    """9000 x 3: 18 chunks of 512 pixels, strips shorter than a block."""
    p = mo.picture("noise", 9000, 3, seed=4)
    for k, m in enumerate(mo.cases(9000, 3, blocks=(4, 128))):
        check(p, [m], lead=k % 16)


def test_byte_equal_1080p():
    p = mo.picture("noise", 1920, 1080, seed=5)
    check(p, [{"x0": 0, "y0": 0, "x1": 10000, "y1": 10000, "mode": "pixelate", "block": 16},
              mo.rect_mask(1920, 1080, 1, 3, 482, 271, mode="pixelate", block=48),
              mo.rect_mask(1920, 1080, 1437, 700, 1920, 1080, mode="fill", b=1, g=2, r=3)], lead=5)


def test_closed_forms_on_the_gpu():
    c = mo.picture("checker", 64, 48)
    out = run_guarded(c, [mo.rect_mask(64, 48, 8, 4, 56, 44, mode="pixelate", block=8)], lead=3)
    assert (out[4:44, 8:56] == 128).all()
    u = mo.picture("uniform", 61, 45, seed=2)
    pix = mo.rect_mask(61, 45, 3, 2, 58, 41, mode="pixelate", block=8)
    assert np.array_equal(run_guarded(u, [pix], lead=1), u)
    p = mo.picture("noise", 61, 45, seed=9)
    once = run_guarded(p, [pix], lead=2)
    assert np.array_equal(run_guarded(once, [pix], lead=7), once) and not np.array_equal(once, p)


THREE_LEVELS = [{"x0": 0, "y0": 0, "x1": 6000, "y1": 6000, "mode": "pixelate", "block": 8},
                {"x0": 4000, "y0": 4000, "x1": 9000, "y1": 9000, "mode": "fill", "b": 200, "g": 100, "r": 50},
                {"x0": 5000, "y0": 1000, "x1": 10000, "y1": 5000, "mode": "pixelate", "block": 12},
                {"x0": 0, "y0": 9000, "x1": 1000, "y1": 10000, "mode": "fill", "b": 1, "g": 2, "r": 3}]


def test_batch_mixed_sizes(native):
    """Five pictures of three sizes in one call with different lists: one empty, one with three
    levels (a chain of overlapping masks: fill over pixelate over fill differs by order)."""
    from video_edge_ai_proxy_amd import ops

    sizes = [(200, 120), (64, 48), (200, 120), (17, 9), (64, 48)]
    lists = [THREE_LEVELS,
             [],
             [mo.rect_mask(200, 120, 3, 5, 190, 111, mode="pixelate", block=16)],
             [{"x0": 0, "y0": 0, "x1": 10000, "y1": 10000, "mode": "pixelate", "block": 4}],
             [mo.rect_mask(64, 48, 1, 1, 30, 30, mode="fill", b=7, g=8, r=9),
              mo.rect_mask(64, 48, 33, 2, 63, 47, mode="pixelate", block=5)]]
    assert native.mask_levels(200, 120, privacy.to_native(THREE_LEVELS)) == [0, 1, 2, 0]
    a = [mo.picture(mo.KINDS[k % 2], w, h, seed=k) for k, (w, h) in enumerate(sizes)]
    dev = [torch.from_numpy(x).cuda() for x in a]
    out = ops.privacy_mask_batch(dev, lists)
    assert all(o is d for o, d in zip(out, dev))
    for k in range(5):
        want = ops.privacy_mask_reference(torch.from_numpy(a[k]), lists[k]).numpy()
        assert np.array_equal(dev[k].cpu().numpy(), want), f"picture {k}"
        assert np.array_equal(want, mo.apply(a[k], lists[k]))
    assert np.array_equal(dev[1].cpu().numpy(), a[1])  # the empty list leaves its picture alone
    rev = ops.privacy_mask_reference(torch.from_numpy(a[0]), THREE_LEVELS[::-1]).numpy()
    assert not np.array_equal(rev, dev[0].cpu().numpy())  # the order matters, and the levels keep it


def test_batch_of_33():
    """More pictures than one wave of workgroups has lanes, sizes alternating."""
    from video_edge_ai_proxy_amd import ops

    sizes = [(48, 32), (33, 17), (64, 9)]
    a = [mo.picture(mo.KINDS[k % 2], *sizes[k % 3], seed=k) for k in range(33)]
    lists = [[mo.rect_mask(*sizes[k % 3], 1 + k % 4, k % 3, sizes[k % 3][0] - k % 5, sizes[k % 3][1] - k % 2,
                           mode="pixelate" if k % 3 else "fill", block=4 + k % 9, b=k, g=2 * k, r=3 * k)] +
             ([THREE_LEVELS[1]] if k % 4 == 0 else []) for k in range(33)]
    dev = [torch.from_numpy(x).cuda() for x in a]
    ops.privacy_mask_batch(dev, lists)
    for k in range(33):
        want = ops.privacy_mask_reference(torch.from_numpy(a[k]), lists[k]).numpy()
        assert np.array_equal(dev[k].cpu().numpy(), want), f"picture {k}"


def test_more_callers_than_scratch_sets():
    """8 threads, twice the pool's sets, 4 calls each with two overlapping masks: callers wait for
    a free set, and every result is the CPU's."""
    from video_edge_ai_proxy_amd import ops

    masks = THREE_LEVELS[:2]
    a = [mo.picture(mo.KINDS[k % 2], 37, 21, seed=k) for k in range(8)]
    want = [ops.privacy_mask_reference(torch.from_numpy(x), masks).numpy() for x in a]
    dev = [torch.from_numpy(x).cuda() for x in a]
    torch.cuda.synchronize()
    got, errors = {}, []

    def run(k):
        try:
            for i in range(4):
                got[k, i] = ops.privacy_mask(dev[k].clone(), masks)
        except Exception as e:
            errors.append(e)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors and len(got) == 32
    for (k, i), g in got.items():
        assert np.array_equal(g.cpu().numpy(), want[k]), f"thread {k} call {i}"
        assert not np.array_equal(want[k], a[k])


def test_descriptors_grow_past_the_floor_and_come_back():
    """One picture with one mask, then 9 pictures with 8 masks each (72 descriptors: more than the
    64 a set starts with), then the one again: all three exact."""
    from video_edge_ai_proxy_amd import ops

    eight = [{"x0": 1000 * j, "y0": 500 * j, "x1": 1000 * j + 3000, "y1": 500 * j + 6000,
              "mode": "fill" if j % 2 else "pixelate", "block": 4, "b": 10 * j, "g": 20 * j, "r": 30 * j}
             for j in range(8)]
    a = [mo.picture(mo.KINDS[k % 2], 24, 16, seed=k) for k in range(9)]
    for n, lists in ((1, [eight[:1]]), (9, [eight] * 9), (1, [eight[:1]])):
        dev = [torch.from_numpy(x).cuda() for x in a[:n]]
        ops.privacy_mask_batch(dev, lists)
        for k in range(n):
            want = ops.privacy_mask_reference(torch.from_numpy(a[k]), lists[k]).numpy()
            assert np.array_equal(dev[k].cpu().numpy(), want), f"{n} pictures, picture {k}"
            assert not np.array_equal(want, a[k])


def test_argument_checks():
    from video_edge_ai_proxy_amd import ops

    x = torch.zeros((16, 16, 3), dtype=torch.uint8)
    good = [{"x0": 0, "y0": 0, "x1": 5000, "y1": 5000}]
    with pytest.raises(ValueError):
        ops.privacy_mask(x, good)  # host tensor
    with pytest.raises(ValueError):
        ops.privacy_mask(x.cuda().float(), good)  # wrong dtype
    with pytest.raises(ValueError):
        ops.privacy_mask(x.cuda()[:, :, :2], good)  # wrong shape
    with pytest.raises(ValueError):
        ops.privacy_mask(x.cuda()[0], good)
    with pytest.raises(ValueError):
        ops.privacy_mask(x.cuda()[:, ::2], good)  # not contiguous
    with pytest.raises(ValueError):
        ops.privacy_mask(x.cuda(), [dict(good[0], block=3)])
    with pytest.raises(ValueError):
        ops.privacy_mask(x.cuda(), good * 9)
    with pytest.raises(ValueError):
        ops.privacy_mask_batch([x.cuda(), x.cuda()], [good])
    with pytest.raises(ValueError):
        ops.privacy_mask_batch([x.cuda(), x], [good, good])
    y = x.cuda()
    assert ops.privacy_mask(y, []) is y and ops.privacy_mask_batch([], []) == []


# ----------------------------------------------------------------------------- publish path

MASKS = [{"x0": 1000, "y0": 500, "x1": 6100, "y1": 7300, "mode": "pixelate", "block": 16},
         {"x0": 5000, "y0": 6000, "x1": 10000, "y1": 10000, "mode": "fill", "b": 9, "g": 99, "r": 199},
         {"x0": 0, "y0": 0, "x1": 1500, "y1": 1500, "mode": "pixelate", "block": 5}]


def _history(native, device, feed, history, masks):
    """The frames a camera of a worker on `device` holds after `feed(worker, camera)`."""
    wk = native.Worker(device=device)
    cam = wk.add_camera("c", wk.history_ring_slots(history), history)
    if masks:
        wk.set_privacy_masks(cam, privacy.to_native(masks))
    feed(wk, cam)
    frames = wk.read_history(cam, 0, history)
    st = wk.stats(cam)
    assert st["errors"] == 0 and st["mask_dropped"] == 0
    assert st["masked_frames"] == (st["published"] if masks else 0)
    return frames


def _feeds(native):
    def fast(wk, cam):  # I_PCM / P_Skip: one picture per job
        enc = synth(native, 320, 240, gop=3, motion=0.2)
        for _ in range(4):
            assert wk.decode_now(cam, enc.next())

    h264 = avc_stream(native, 12)[0]
    h265 = hevc_stream(native, 12, 64, 64)[0]

    def general(aus):
        def feed(wk, cam):  # one job of many pictures: its earlier outputs are history conversions
            wk.decode_many([(cam, aus[:9])])
            for au in aus[9:]:
                wk.decode_now(cam, au)
        return feed

    return {"fast": (fast, 3), "h264": (general(h264), 5), "h265": (general(h265), 5)}


@pytest.mark.parametrize("path", ["fast", "h264", "h265"])
def test_worker_ring_bytes_equal_the_cpu_backend(native, path):
    feed, history = _feeds(native)[path]
    gpu = _history(native, 0, feed, history, MASKS)
    cpu = _history(native, -1, feed, history, MASKS)
    raw = _history(native, 0, feed, history, None)
    assert len(gpu) == len(cpu) == len(raw) == history
    for (mg, fg), (mc, fc), (mr, fr) in zip(gpu, cpu, raw):
        assert mg["pts"] == mc["pts"] == mr["pts"] and mg["seq"] == mc["seq"]
        assert np.array_equal(fg, fc), f"{path} pts {mg['pts']}: GPU and CPU backends differ"
        assert np.array_equal(fg, mo.apply(fr, MASKS)), f"{path} pts {mg['pts']}: not the masked picture"
        assert not np.array_equal(fg, fr)


def test_mask_change_in_flight_drops_the_frame(native):
    wk = native.Worker(device=0)
    cam, ref = wk.add_camera("c", 2), wk.add_camera("ref", 2)
    encs = [synth(native, 320, 240, gop=6, motion=0.2) for _ in range(2)]
    assert wk.decode_now(cam, encs[0].next()) and wk.decode_now(ref, encs[1].next())
    assert wk.read_latest(cam, 0)[0]["seq"] == 1
    # a batch is launched under the old (empty) list, the list changes, the batch completes
    assert wk.decode_many([(cam, [encs[0].next()])], sync=False) == 1
    wk.set_privacy_masks(cam, privacy.to_native(MASKS))
    wk.complete_all()
    st = wk.stats(cam)
    assert st["mask_dropped"] == 1 and st["published"] == 1 and st["masked_frames"] == 0
    assert wk.read_latest(cam, 0) is None  # neither the frame in flight nor the older one
    assert wk.decode_now(ref, encs[1].next())
    # the next batch's frame is masked
    assert wk.decode_now(cam, encs[0].next()) and wk.decode_now(ref, encs[1].next())
    m, f = wk.read_latest(cam, 0)
    assert m["seq"] == 2 and np.array_equal(f, mo.apply(wk.read_latest(ref, 0)[1], MASKS))
    st = wk.stats(cam)
    assert st["mask_dropped"] == 1 and st["masked_frames"] == 1
    # every serving path of the GPU reads the masked slot
    assert wk.read_latest_jpeg(cam, 0, 80)[1] == native.jpeg_encode_cpu(f, 80)
    assert np.array_equal(wk.read_latest_scaled(cam, 0, 160, 0)[1], native.resize_area_cpu(f, 160, 120))
