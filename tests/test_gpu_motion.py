"""gfx950 motion detection: byte equality of the kernel with the CPU implementation, counts and
background, and the Worker's ring paths (run on an MI355X). The CPU implementation is held to the
independent oracle in tests/test_motion.py."""
import threading

import numpy as np
import pytest
import torch

import motion_oracle as mo
from conftest import synth

pytestmark = pytest.mark.gpu

# the shapes of tests/test_motion.py, 1080p (67.5 cell rows), and a row wider than one block's
# staging (9000 pixels: 18 chunks of 512)
SHAPES = [((7, 5), 8), ((17, 9), 8), ((33, 17), 16), ((64, 48), 16), ((200, 120), 32), ((1, 9), 4), ((9, 1), 4),
          ((300, 3), 256), ((1920, 1080), 16), ((9000, 3), 16)]
SENTINEL = 0xABCD


def same(got, want, what=""):
    """(counts, background) of the kernel and of the CPU twin, byte for byte."""
    gc, gb = got[0].cpu().numpy(), got[1].cpu().numpy()
    wc, wb = want[0].numpy(), want[1].numpy()
    assert gc.dtype == np.int32 and gb.dtype == np.uint16 and gc.shape == wc.shape and gb.shape == wb.shape, what
    assert np.array_equal(gc, wc), f"{what}: {(gc != wc).sum()} cells differ"
    assert np.array_equal(gb, wb), f"{what}: {(gb != wb).sum()} background samples differ"


@pytest.mark.parametrize("size,cell", SHAPES)
@pytest.mark.parametrize("kind", ["noise", "gradient"])
def test_update_byte_equal(size, cell, kind):
    """Unprimed, then primed at shifts 0, 4 and 8 from the same background."""
    from video_edge_ai_proxy_amd import ops

    w, h = size
    a, b = torch.from_numpy(mo.picture(kind, w, h, 1)), torch.from_numpy(mo.picture(kind, w, h, 2))
    got0 = ops.motion_update(a.cuda(), None, cell, 24, 4)
    want0 = ops.motion_update_reference(a, None, cell, 24, 4)
    assert got0[0].is_cuda and got0[1].is_cuda and not got0[0].any()
    same(got0, want0, "prime")
    for shift in (0, 4, 8):
        got = ops.motion_update(b.cuda(), got0[1], cell, 24, shift)
        want = ops.motion_update_reference(b, want0[1], cell, 24, shift)
        same(got, want, f"shift {shift}")
        assert int(want[0].sum()) > 0


@pytest.mark.parametrize("t", [0, 24, 254, 255])
def test_threshold_edge(t):
    from video_edge_ai_proxy_amd import ops

    w, h, cell = 33, 17, 16
    base = 100 if 100 + t + 1 <= 255 else 0
    g = lambda v: torch.from_numpy(mo.grey(v, w, h))
    _, bg = ops.motion_update(g(base).cuda(), None, cell, t, 0)
    at = ops.motion_update(g(base + t).cuda(), bg, cell, t, 0)
    same(at, ops.motion_update_reference(g(base + t), bg, cell, t, 0))
    assert not at[0].any()
    if t == 255:
        return  # (black then white changed nothing: 255 is never exceeded)
    above = ops.motion_update(g(base + t + 1).cuda(), bg, cell, t, 0)
    same(above, ops.motion_update_reference(g(base + t + 1), bg, cell, t, 0))
    assert int(above[0].sum()) == w * h


def padded(w, h, fill=SENTINEL):
    """A background plane whose rows are padded to the kernel's pitch, every sample `fill`."""
    from video_edge_ai_proxy_amd import native

    return torch.from_numpy(np.full((h, native.motion_pitch(w)), fill, dtype=np.uint16)).cuda()


@pytest.mark.parametrize("w,h,cell", [(33, 17, 16), (7, 5, 8), (1, 9, 4), (1921, 3, 16)])
def test_out_argument_and_padding(w, h, cell):
    """out= is used where it lies when its rows are padded; the padding samples keep a sentinel."""
    from video_edge_ai_proxy_amd import ops

    a, b = torch.from_numpy(mo.picture("noise", w, h, 1)), torch.from_numpy(mo.picture("noise", w, h, 2))
    p0, p1 = padded(w, h), padded(w, h)
    c0, bg0 = ops.motion_update(a.cuda(), None, cell, 24, 4, out=p0[:, :w])
    assert bg0.data_ptr() == p0.data_ptr()
    c1, bg1 = ops.motion_update(b.cuda(), bg0, cell, 24, 4, out=p1[:, :w])
    assert bg1.data_ptr() == p1.data_ptr()
    want0 = ops.motion_update_reference(a, None, cell, 24, 4)
    same((c0, bg0), want0)
    same((c1, bg1), ops.motion_update_reference(b, want0[1], cell, 24, 4))
    for p in (p0, p1):
        pad = p.cpu().numpy()[:, w:]
        assert pad.size == 0 or (pad == SENTINEL).all()
    # a plane that is not padded (w % 8 != 0) goes through a padded copy: same bytes
    if w % 8:
        tight = torch.from_numpy(np.zeros((h, w), dtype=np.uint16)).cuda()
        c2, bg2 = ops.motion_update(b.cuda(), bg0.contiguous(), cell, 24, 4, out=tight)
        assert bg2 is tight
        same((c2, bg2), ops.motion_update_reference(b, want0[1], cell, 24, 4))


def test_batch_mixed_sizes():
    """Five pictures of three sizes in one launch, one of them unprimed, one a single cell."""
    from video_edge_ai_proxy_amd import ops

    sizes = [(200, 120), (64, 48), (200, 120), (16, 16), (64, 48)]
    a = [torch.from_numpy(mo.picture("noise", w, h, k)) for k, (w, h) in enumerate(sizes)]
    b = [torch.from_numpy(mo.picture("gradient", w, h, k)) for k, (w, h) in enumerate(sizes)]
    primes = ops.motion_update_batch([x.cuda() for x in a], 16, 24, 4)
    pics = [(x.cuda(), None if k == 2 else primes[k][1]) for k, x in enumerate(b)]
    got = ops.motion_update_batch(pics, 16, 24, 4)
    assert len(got) == 5 and tuple(got[3][0].shape) == (1, 1)
    for k in range(5):
        want0 = ops.motion_update_reference(a[k], None, 16, 24, 4)
        same(primes[k], want0, f"prime {k}")
        same(got[k], ops.motion_update_reference(b[k], None if k == 2 else want0[1], 16, 24, 4), f"picture {k}")


def test_batch_of_33():
    """More pictures than one wave of blocks has lanes, sizes alternating."""
    from video_edge_ai_proxy_amd import ops

    sizes = [(48, 32), (33, 17), (64, 9)]
    a = [torch.from_numpy(mo.picture("noise", *sizes[k % 3], seed=k)) for k in range(33)]
    b = [torch.from_numpy(mo.picture("noise", *sizes[k % 3], seed=100 + k)) for k in range(33)]
    primes = ops.motion_update_batch([x.cuda() for x in a], 8, 24, 2)
    got = ops.motion_update_batch([(x.cuda(), primes[k][1]) for k, x in enumerate(b)], 8, 24, 2)
    for k in range(33):
        want0 = ops.motion_update_reference(a[k], None, 8, 24, 2)
        same(got[k], ops.motion_update_reference(b[k], want0[1], 8, 24, 2), f"picture {k}")


def test_more_callers_than_scratch_sets():
    """8 threads, twice the pool's sets, 4 calls each on 37 x 21 at the smallest cell: callers wait
    for a free set, and every result is the CPU's."""
    from video_edge_ai_proxy_amd import ops

    a = [torch.from_numpy(mo.picture("noise", 37, 21, k)) for k in range(8)]
    b = [torch.from_numpy(mo.picture("noise", 37, 21, 100 + k)) for k in range(8)]
    bg = [ops.motion_update_reference(x, None, 4, 24, 4)[1] for x in a]
    want = [ops.motion_update_reference(b[k], bg[k], 4, 24, 4) for k in range(8)]
    dev = [(b[k].cuda(), bg[k].cuda()) for k in range(8)]
    torch.cuda.synchronize()
    got, errors = {}, []

    def run(k):
        try:
            for i in range(4):
                got[k, i] = ops.motion_update(dev[k][0], dev[k][1], 4, 24, 4)
        except Exception as e:
            errors.append(e)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors and len(got) == 32
    for (k, i), g in got.items():
        same(g, want[k], f"thread {k} call {i}")
        assert int(want[k][0].sum()) > 0


def test_descriptors_grow_past_the_floor_and_come_back():
    """One picture, then 65 in one launch (more than the 64 descriptors a set starts with), then
    the one again: all three exact."""
    from video_edge_ai_proxy_amd import ops

    a = [torch.from_numpy(mo.picture("noise", 8, 8, k)) for k in range(65)]
    b = [torch.from_numpy(mo.picture("noise", 8, 8, 100 + k)) for k in range(65)]
    bg = [ops.motion_update_reference(x, None, 4, 24, 2)[1] for x in a]
    want = [ops.motion_update_reference(b[k], bg[k], 4, 24, 2) for k in range(65)]
    pics = [(b[k].cuda(), bg[k].cuda()) for k in range(65)]
    for n in (1, 65, 1):
        got = ops.motion_update_batch(pics[:n], 4, 24, 2)
        assert len(got) == n
        for k in range(n):
            same(got[k], want[k], f"batch of {n}, picture {k}")


OFFSET_W, OFFSET_H = 37, 9  # rows of 111 bytes: successive rows differ in alignment as well
OFFSET_GUARD = 0xA5
_offset_want = {}


def offset_case(cell):
    """Two pictures and the CPU twin's answers, unprimed and primed: computed once per cell."""
    from video_edge_ai_proxy_amd import ops

    if cell not in _offset_want:
        a = torch.from_numpy(mo.picture("noise", OFFSET_W, OFFSET_H, 1))
        b = torch.from_numpy(mo.picture("noise", OFFSET_W, OFFSET_H, 2))
        want0 = ops.motion_update_reference(a, None, cell, 24, 4)
        _offset_want[cell] = (a, b, want0, ops.motion_update_reference(b, want0[1], cell, 24, 4))
    return _offset_want[cell]


def view_at(pic, o):
    """(flat, view): the picture as a contiguous view that starts at byte address o modulo 16 of a
    flat device tensor, guard bytes all around it."""
    n = pic.numel()
    flat = torch.full((n + 48,), OFFSET_GUARD, dtype=torch.uint8, device="cuda")
    view = flat[16 + o:16 + o + n].view(pic.shape)
    view.copy_(pic)
    assert view.is_contiguous() and view.data_ptr() % 16 == o
    return flat, view


def guard_intact(flat, pic, o):
    got = flat.cpu().numpy()
    n = pic.numel()
    assert (got[:16 + o] == OFFSET_GUARD).all() and (got[16 + o + n:] == OFFSET_GUARD).all(), "guard bytes changed"
    assert np.array_equal(got[16 + o:16 + o + n], pic.numpy().reshape(-1)), "the source changed"


@pytest.mark.parametrize("cell", [4, 16])
@pytest.mark.parametrize("o", range(16))
def test_source_at_every_byte_offset(o, cell):
    """The source starts at every address modulo 16 (its staging never had anything but freshly
    allocated tensors): unprimed and primed, counts and background are the CPU's, and nothing
    around the source is written."""
    from video_edge_ai_proxy_amd import ops

    a, b, want0, want1 = offset_case(cell)
    fa, va = view_at(a, o)
    fb, vb = view_at(b, o)
    got0 = ops.motion_update(va, None, cell, 24, 4)
    same(got0, want0, f"offset {o} prime")
    same(ops.motion_update(vb, got0[1], cell, 24, 4), want1, f"offset {o} primed")
    assert int(want1[0].sum()) > 0
    guard_intact(fa, a, o)
    guard_intact(fb, b, o)


def test_argument_checks():
    from video_edge_ai_proxy_amd import ops

    x = torch.zeros((16, 16, 3), dtype=torch.uint8)
    bg = torch.from_numpy(np.zeros((16, 16), dtype=np.uint16))
    with pytest.raises(ValueError):
        ops.motion_update(x)  # host tensor
    with pytest.raises(ValueError):
        ops.motion_update(x.cuda()[:, ::2])  # not contiguous
    with pytest.raises(TypeError):
        ops.motion_update(x.cuda().float())
    with pytest.raises(ValueError):
        ops.motion_update(x.cuda()[:, :, :2])
    for bad in [dict(cell=3), dict(cell=257), dict(threshold=-1), dict(threshold=256), dict(learn_shift=-1),
                dict(learn_shift=9), dict(cell=True)]:
        with pytest.raises(ValueError):
            ops.motion_update(x.cuda(), None, **bad)
    with pytest.raises(ValueError):
        ops.motion_update(x.cuda(), bg)  # host background
    with pytest.raises(TypeError):
        ops.motion_update(x.cuda(), torch.zeros((16, 16), dtype=torch.int16).cuda())
    with pytest.raises(ValueError):
        ops.motion_update(x.cuda(), bg.cuda()[:8])
    with pytest.raises(ValueError):
        ops.motion_update(x.cuda(), None, out=bg)  # host out
    with pytest.raises(ValueError):
        ops.motion_update(x.cuda(), None, out=bg.cuda()[:, :8])
    both = bg.cuda()
    with pytest.raises(ValueError):
        ops.motion_update(x.cuda(), both, out=both)  # in place
    with pytest.raises(ValueError):
        ops.motion_update_batch([])


# --------------------------------------------------------------------------------- ring path

@pytest.fixture(scope="module")
def ring(native):
    """A worker on GPU 0 with two synthetic cameras (640x480, 320x240), their encoders, and one
    camera without frames."""
    wk = native.Worker(device=0)
    cams, encs = [], []
    for name, (w, h) in {"a": (640, 480), "b": (320, 240)}.items():
        enc = synth(native, w, h, gop=6, motion=0.2)
        cam = wk.add_camera(name, 2)
        assert wk.decode_now(cam, enc.next())
        cams.append(cam)
        encs.append(enc)
    cams.append(wk.add_camera("empty", 2))
    return wk, cams, encs


def expect(native, wk, cam, bg):
    """The answer read_motion owes for the camera's newest frame against the host background bg,
    from the CPU twin on the frame read_latest serves; and the background after it."""
    prm = wk.motion_params
    meta, frame = wk.read_latest(cam, 0)
    counts, new = native.motion_update_cpu(frame, bg, prm["cell"], prm["threshold"], prm["learn_shift"])
    h, w = frame.shape[:2]
    want = native.motion_summarize(counts, w, h, prm["cell"], prm["cell_percent"], prm["min_cells"])
    cols, rows = native.motion_grid(w, h, prm["cell"])
    want.update(seq=meta["seq"], width=w, height=h, cell=prm["cell"], cols=cols, rows=rows,
                threshold=prm["threshold"], primed=bg is not None)
    return want, counts, new


def check(got, want, counts):
    assert got is not None
    g = dict(got)
    assert np.array_equal(g.pop("counts"), counts)
    assert g == want, (g, want)


def test_ring_motion_over_three_frames(native, ring):
    wk, cams, encs = ring
    bgs = [None, None]
    for cam in cams[:2]:
        wk.motion_reset(cam)
    for step in range(3):
        wants = []
        for k in range(2):
            if step:
                assert wk.decode_now(cams[k], encs[k].next())
            want, counts, bgs[k] = expect(native, wk, cams[k], bgs[k])
            wants.append((want, counts))
        evals = [wk.stats(c)["motion_evaluations"] for c in cams[:2]]
        if step == 1:  # one launch for both, the empty camera and an unknown index answer None
            rs = wk.read_motion_many([cams[0], cams[1], cams[2], 99])
            assert rs[2] is None and rs[3] is None
        else:
            rs = [wk.read_motion(cams[0], 0), wk.read_motion(cams[1], 0)]
        for k in range(2):
            check(rs[k], *wants[k])
            assert rs[k]["primed"] is (step > 0)
            if step:
                assert rs[k]["changed"] > 0
            # the same seq again: the stored answer, from either call, and no second evaluation
            check(wk.read_motion(cams[k], 0), *wants[k])
            check(wk.read_motion_many([cams[k]])[0], *wants[k])
            assert wk.stats(cams[k])["motion_evaluations"] == evals[k] + 1
            assert wk.read_motion(cams[k], rs[k]["seq"]) is None
    assert wk.read_motion(cams[2], 0) is None


def test_concurrent_pollers(native, ring):
    """Two threads ask about the same two static cameras: one evaluation each, one answer."""
    wk, cams, encs = ring
    wants = []
    for cam in cams[:2]:
        wk.motion_reset(cam)
        wants.append(expect(native, wk, cam, None)[:2])
    before = [wk.stats(c)["motion_evaluations"] for c in cams[:2]]
    bad = []

    def run(t):
        for i in range(20):
            for k in ((0, 1) if t == 0 else (1, 0)):
                r = wk.read_motion(cams[k], 0) if (i + t) % 2 else wk.read_motion_many([cams[k], cams[1 - k]])[0]
                try:
                    check(r, *wants[k])
                except AssertionError as e:
                    bad.append((t, i, k, str(e)[:200]))

    ts = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not bad
    assert [wk.stats(c)["motion_evaluations"] for c in cams[:2]] == [b + 1 for b in before]
