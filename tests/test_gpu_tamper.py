"""gfx950 tamper detection: byte equality of the kernel with the CPU implementation, in the
histogram and both grid planes, and the Worker's ring paths (run on an MI355X). The CPU
implementation is held to the independent oracle in tests/test_tamper.py."""
import threading

import numpy as np
import pytest
import torch

import tamper_oracle as to
from conftest import synth

pytestmark = pytest.mark.gpu

# the shapes of tests/test_tamper.py, and a row wider than one block's staging (9000 pixels: 18
# chunks of 512)
SHAPES = [((7, 5), 8), ((17, 9), 8), ((33, 17), 16), ((64, 48), 16), ((50, 30), 12), ((50, 30), 20), ((200, 120), 32),
          ((1, 9), 8), ((9, 1), 8), ((300, 3), 128), ((1920, 1080), 32), ((9000, 3), 16)]
SENTINEL = 0x5A5A5A5A
GUARD = 64


def same(got, want, what=""):
    """(hist, sum_y, energy) of the kernel and of the CPU twin, byte for byte."""
    assert len(got) == len(want) == 3
    for g, w, name in zip(got, want, ("hist", "sum_y", "energy")):
        g, w = g.cpu().numpy(), w.numpy()
        assert g.dtype == np.int64 and w.dtype == np.int64 and g.shape == w.shape, f"{what} {name}"
        assert np.array_equal(g, w), f"{what} {name}: {(g != w).sum()} values differ"


@pytest.mark.parametrize("size,cell", SHAPES)
@pytest.mark.parametrize("kind", ["noise", "gradient", "uniform", "checker"])
def test_stats_byte_equal(size, cell, kind):
    from video_edge_ai_proxy_amd import ops

    w, h = size
    p = torch.from_numpy(to.picture(kind, w, h, 1))
    got = ops.tamper_stats(p.cuda(), cell)
    assert all(t.is_cuda for t in got)
    want = ops.tamper_stats_reference(p, cell)
    same(got, want, f"{kind} {w}x{h}/{cell}")
    assert int(want[0].sum()) == w * h


@pytest.mark.parametrize("seed", [0, 1])
def test_cell_128_checkerboards(seed):
    """300 x 260 at cell 128: full cells at the u32 bound's value, partial cells on both edges."""
    from video_edge_ai_proxy_amd import ops

    p = torch.from_numpy(to.picture("checker", 300, 260, seed))
    got = ops.tamper_stats(p.cuda(), 128)
    same(got, ops.tamper_stats_reference(p, 128))
    assert int(got[2][0, 0]) == 2114092800 and tuple(got[2].shape) == (3, 3)


@pytest.mark.parametrize("w,h,cell", [(1100, 140, 127), (100, 40, 9), (530, 70, 66), (2049, 33, 32)])
def test_odd_cells_and_wide_chunks(w, h, cell):
    """Cells that are no multiple of 8 (columns of 8 pixels split between two cells at every
    position), the widest chunk (1016 pixels at cell 127: two segments of threads), a cell row
    of several passes, and a last chunk one pixel wide."""
    from video_edge_ai_proxy_amd import ops

    for kind in ("noise", "checker"):
        p = torch.from_numpy(to.picture(kind, w, h, 2))
        same(ops.tamper_stats(p.cuda(), cell), ops.tamper_stats_reference(p, cell), f"{kind} {w}x{h}/{cell}")


OFFSET_W, OFFSET_H, OFFSET_CELL = 37, 9, 8  # rows of 111 bytes: successive rows differ in alignment as well
OFFSET_GUARD = 0xA5
_offset_want = []


def offset_case():
    """The picture and the CPU twin's answer: computed once."""
    from video_edge_ai_proxy_amd import ops

    if not _offset_want:
        p = torch.from_numpy(to.picture("noise", OFFSET_W, OFFSET_H, 1))
        _offset_want.append((p, ops.tamper_stats_reference(p, OFFSET_CELL)))
    return _offset_want[0]


@pytest.mark.parametrize("o", range(16))
def test_source_at_every_byte_offset(o):
    """The source is a contiguous view that starts at every address modulo 16 of a flat tensor (its
    staging never had anything but freshly allocated tensors): all three results are the CPU's,
    and the guard bytes around the source keep their value."""
    from video_edge_ai_proxy_amd import ops

    p, want = offset_case()
    n = p.numel()
    flat = torch.full((n + 48,), OFFSET_GUARD, dtype=torch.uint8, device="cuda")
    view = flat[16 + o:16 + o + n].view(p.shape)
    view.copy_(p)
    assert view.is_contiguous() and view.data_ptr() % 16 == o
    same(ops.tamper_stats(view, OFFSET_CELL), want, f"offset {o}")
    assert int(want[0].sum()) == OFFSET_W * OFFSET_H
    got = flat.cpu().numpy()
    assert (got[:16 + o] == OFFSET_GUARD).all() and (got[16 + o + n:] == OFFSET_GUARD).all(), "guard bytes changed"
    assert np.array_equal(got[16 + o:16 + o + n], p.numpy().reshape(-1)), "the source changed"


def test_batch_mixed_sizes():
    """Five pictures of three sizes in one launch, one of them a single cell."""
    from video_edge_ai_proxy_amd import ops

    sizes = [(200, 120), (64, 48), (200, 120), (16, 16), (64, 48)]
    kinds = ["noise", "gradient", "uniform", "noise", "checker"]
    a = [torch.from_numpy(to.picture(kinds[k], w, h, k)) for k, (w, h) in enumerate(sizes)]
    got = ops.tamper_stats_batch([x.cuda() for x in a], 16)
    assert len(got) == 5 and tuple(got[3][1].shape) == (1, 1)
    for k in range(5):
        same(got[k], ops.tamper_stats_reference(a[k], 16), f"picture {k}")


def test_batch_of_33():
    """More pictures than one wave of blocks has lanes, sizes alternating."""
    from video_edge_ai_proxy_amd import ops

    sizes = [(48, 32), (33, 17), (64, 9)]
    a = [torch.from_numpy(to.picture(to.KINDS[k % 6], *sizes[k % 3], seed=k)) for k in range(33)]
    got = ops.tamper_stats_batch([x.cuda() for x in a], 8)
    for k in range(33):
        same(got[k], ops.tamper_stats_reference(a[k], 8), f"picture {k}")


def test_more_callers_than_scratch_sets():
    """8 threads, twice the pool's sets, 4 calls each on 37 x 21 at the smallest cell: callers wait
    for a free set, and every result is the CPU's."""
    from video_edge_ai_proxy_amd import ops

    a = [torch.from_numpy(to.picture(to.KINDS[k % 6], 37, 21, k)) for k in range(8)]
    want = [ops.tamper_stats_reference(x, 8) for x in a]
    dev = [x.cuda() for x in a]
    torch.cuda.synchronize()
    got, errors = {}, []

    def run(k):
        try:
            for i in range(4):
                got[k, i] = ops.tamper_stats(dev[k], 8)
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


def test_descriptors_grow_past_the_floor_and_come_back():
    """One picture, then 65 in one launch (more than the 64 descriptors a set starts with), then
    the one again: all three exact."""
    from video_edge_ai_proxy_amd import ops

    a = [torch.from_numpy(to.picture(to.KINDS[k % 6], 8, 8, k)) for k in range(65)]
    want = [ops.tamper_stats_reference(x, 8) for x in a]
    dev = [x.cuda() for x in a]
    for n in (1, 65, 1):
        got = ops.tamper_stats_batch(dev[:n], 8)
        assert len(got) == n
        for k in range(n):
            same(got[k], want[k], f"batch of {n}, picture {k}")


@pytest.mark.parametrize("w,h,cell", [(33, 17, 16), (7, 5, 8), (1, 9, 8), (1921, 3, 16), (300, 260, 128)])
def test_result_buffers_kept_clean(w, h, cell):
    """The results lie inside guarded buffers pre-filled with a sentinel: every bin and every cell
    is written, and nothing outside them."""
    from video_edge_ai_proxy_amd import native, ops

    cols, rows = native.tamper_grid(w, h, cell)
    sizes = [256, rows * cols, rows * cols]
    flat = [torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32).cuda() for n in sizes]
    out = (flat[0][GUARD:GUARD + 256], flat[1][GUARD:GUARD + sizes[1]].view(rows, cols),
           flat[2][GUARD:GUARD + sizes[2]].view(rows, cols))
    p = torch.from_numpy(to.picture("noise", w, h, 3))
    got = ops.tamper_stats(p.cuda(), cell, out=out)
    want = ops.tamper_stats_reference(p, cell)
    same(got, want)
    for f, n, wv in zip(flat, sizes, want):
        f = f.cpu().numpy()
        assert (f[:GUARD] == SENTINEL).all() and (f[GUARD + n:] == SENTINEL).all()
        assert np.array_equal(f[GUARD:GUARD + n].astype(np.int64) & 0xFFFFFFFF, wv.numpy().ravel())
    # no value of this picture equals the sentinel, so equality above proves every element written
    assert not any((wv.numpy() == SENTINEL).any() for wv in want)


def test_argument_checks():
    from video_edge_ai_proxy_amd import ops

    x = torch.zeros((16, 16, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.tamper_stats(x)  # host tensor
    with pytest.raises(ValueError):
        ops.tamper_stats(x.cuda()[:, ::2])  # not contiguous
    with pytest.raises(TypeError):
        ops.tamper_stats(x.cuda().float())
    with pytest.raises(ValueError):
        ops.tamper_stats(x.cuda()[:, :, :2])
    for bad in [dict(cell=7), dict(cell=129), dict(cell=True), dict(cell=32.0)]:
        with pytest.raises(ValueError):
            ops.tamper_stats(x.cuda(), **bad)
    with pytest.raises(ValueError):
        ops.tamper_stats_batch([])
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32).cuda()
    with pytest.raises(TypeError):
        ops.tamper_stats(x.cuda(), 8, out=(i32(256).long(), i32(2, 2), i32(2, 2)))
    with pytest.raises(ValueError):
        ops.tamper_stats(x.cuda(), 8, out=(i32(256), i32(2, 3), i32(2, 2)))
    with pytest.raises(ValueError):
        ops.tamper_stats(x.cuda(), 8, out=(i32(256), i32(2, 2).cpu(), i32(2, 2)))
    with pytest.raises(ValueError):
        ops.tamper_stats_batch([x.cuda(), x.cuda()], 8, out=[(i32(256), i32(2, 2), i32(2, 2))])


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


def expect(native, wk, cam, ref=None):
    """The answer read_tamper owes for the camera's newest frame, from the CPU twin on the frame
    read_latest serves; and that frame's reference tuple."""
    prm = wk.tamper_params
    meta, frame = wk.read_latest(cam, 0)
    h, w = frame.shape[:2]
    hist, sum_y, energy = native.tamper_stats_cpu(frame, prm["cell"])
    want = native.tamper_summarize(hist, sum_y, energy, w, h, prm, ref)
    cols, rows = native.tamper_grid(w, h, prm["cell"])
    want.update(seq=meta["seq"], width=w, height=h, cell=prm["cell"], cols=cols, rows=rows)
    return want, (hist, sum_y, energy), (w, h, prm["cell"], sum_y, energy)


def check(got, want, planes):
    assert got is not None
    g = dict(got)
    for name, p in zip(("hist", "sum_y", "energy"), planes):
        a = g.pop(name)
        assert a.dtype == np.uint32 and np.array_equal(a, p), name
    assert g == want, (g, want)


def test_ring_tamper_over_three_frames(native, ring):
    wk, cams, encs = ring
    for cam in cams[:2]:
        wk.tamper_reset(cam)
    refs = [None, None]
    for step in range(3):
        wants = []
        for k in range(2):
            if step:
                assert wk.decode_now(cams[k], encs[k].next())
            wants.append(expect(native, wk, cams[k], refs[k]))
        evals = [wk.stats(c)["tamper_evaluations"] for c in cams[:2]]
        if step == 1:  # one launch for both, the empty camera and an unknown index answer None
            rs = wk.read_tamper_many([cams[0], cams[1], cams[2], 99])
            assert rs[2] is None and rs[3] is None
        else:
            rs = [wk.read_tamper(cams[0], 0), wk.read_tamper(cams[1], 0)]
        for k in range(2):
            check(rs[k], *wants[k][:2])
            assert rs[k]["has_reference"] is (step > 0)
            # the same seq again: the stored answer, from either call, and no second evaluation
            check(wk.read_tamper(cams[k], 0), *wants[k][:2])
            check(wk.read_tamper_many([cams[k]])[0], *wants[k][:2])
            assert wk.stats(cams[k])["tamper_evaluations"] == evals[k] + 1
            assert wk.read_tamper(cams[k], rs[k]["seq"]) is None
            if step == 0:  # this frame becomes the reference: the stored answer is summarised against it
                assert wk.tamper_set_reference(cams[k]) is True
                refs[k] = wants[k][2]
                again = expect(native, wk, cams[k], refs[k])
                assert again[0]["has_reference"] and not again[0]["moved"] and not again[0]["defocused"]
                check(wk.read_tamper(cams[k], 0), *again[:2])
                assert wk.stats(cams[k])["tamper_evaluations"] == evals[k] + 1
    # dropped: no reference any more, and the frame is evaluated again
    wk.tamper_reset(cams[0])
    want = expect(native, wk, cams[0], None)
    check(wk.read_tamper(cams[0], 0), *want[:2])
    assert want[0]["has_reference"] is False
    # a camera without frames
    assert wk.read_tamper(cams[2], 0) is None and wk.tamper_set_reference(cams[2]) is False


def test_concurrent_pollers(native, ring):
    """Two threads ask about the same two static cameras: one evaluation each, one answer."""
    wk, cams, encs = ring
    wants = []
    for cam in cams[:2]:
        wk.tamper_reset(cam)
        wants.append(expect(native, wk, cam, None)[:2])
    before = [wk.stats(c)["tamper_evaluations"] for c in cams[:2]]
    bad = []

    def run(t):
        for i in range(20):
            for k in ((0, 1) if t == 0 else (1, 0)):
                r = wk.read_tamper(cams[k], 0) if (i + t) % 2 else wk.read_tamper_many([cams[k], cams[1 - k]])[0]
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
    assert [wk.stats(c)["tamper_evaluations"] for c in cams[:2]] == [b + 1 for b in before]
