"""gfx950 area-average downscale: byte equality with the CPU implementation (run on an MI355X).
The CPU implementation is held to the independent oracle in tests/test_scale.py."""
import threading

import pytest
import torch

import scale_oracle as so

pytestmark = pytest.mark.gpu


def both(kind, sw, sh, ow, oh):
    from video_edge_ai_proxy_amd import ops

    x = torch.from_numpy(so.picture(kind, sw, sh))
    got = ops.resize_area(x.cuda(), ow, oh)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (oh, ow, 3)
    return x, got.cpu(), ops.resize_area_reference(x, ow, oh)


@pytest.mark.parametrize("kind", so.KINDS)
@pytest.mark.parametrize("sw,sh,ow,oh", so.SMALL_SHAPES)
def test_small_shapes_byte_equal(kind, sw, sh, ow, oh):
    x, got, want = both(kind, sw, sh, ow, oh)
    assert torch.equal(got, want), f"{kind} {sw}x{sh} -> {ow}x{oh}: {(got != want).sum().item()} bytes differ"
    if (ow, oh) == (sw, sh):
        assert torch.equal(got, x)


def test_1080p_to_wall_tile():
    _, got, want = both("noise", 1920, 1080, 320, 180)
    assert torch.equal(got, want)


@pytest.mark.parametrize("kind", ["white", "noise"])
@pytest.mark.parametrize("sw,sh,ow,oh", so.BOUNDARY_SHAPES)
def test_accumulator_boundary(kind, sw, sh, ow, oh):
    """255 * sw * sh on either side of 2^32: the kernel's 32-bit and 64-bit accumulators. A
    footprint of 514 x 512 source pixels per output pixel, staged in LDS one piece at a time."""
    _, got, want = both(kind, sw, sh, ow, oh)
    assert torch.equal(got, want)
    if kind == "white":
        assert int(got.min()) == 255


def test_wide_footprint_is_staged_in_segments():
    """One output column whose source row does not fit the kernel's LDS buffer at once."""
    _, got, want = both("noise", 9000, 3, 1, 2)
    assert torch.equal(got, want)
    _, got, want = both("noise", 9000, 2, 2, 1)
    assert torch.equal(got, want)


def test_out_argument():
    from video_edge_ai_proxy_amd import ops

    x = torch.from_numpy(so.picture("noise", 200, 120))
    out = torch.full((119, 199, 3), 9, dtype=torch.uint8, device="cuda")
    r = ops.resize_area(x.cuda(), 199, 119, out=out)
    assert r is out and torch.equal(out.cpu(), ops.resize_area_reference(x, 199, 119))
    for bad in (torch.empty((119, 199, 3), dtype=torch.uint8), torch.empty((119, 198, 3), dtype=torch.uint8).cuda(),
                torch.empty((119, 199, 3)).cuda(), torch.empty((119, 398, 3), dtype=torch.uint8).cuda()[:, ::2]):
        with pytest.raises(ValueError):
            ops.resize_area(x.cuda(), 199, 119, out=bad)


def test_more_callers_than_scratch_sets():
    """8 threads, twice the pool's sets, 4 calls each from 37 x 21 to 9 x 5: callers wait for a free
    set, and every result is the CPU's."""
    from video_edge_ai_proxy_amd import ops

    a = [torch.from_numpy(so.picture(so.KINDS[k % 4], 37, 21, seed=k)) for k in range(8)]
    want = [ops.resize_area_reference(x, 9, 5) for x in a]
    dev = [x.cuda() for x in a]
    torch.cuda.synchronize()
    got, errors = {}, []

    def run(k):
        try:
            for i in range(4):
                got[k, i] = ops.resize_area(dev[k], 9, 5)
        except Exception as e:
            errors.append(e)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors and len(got) == 32
    for (k, i), g in got.items():
        assert torch.equal(g.cpu(), want[k]), f"thread {k} call {i}"


def test_argument_checks():
    from video_edge_ai_proxy_amd import ops

    x = torch.zeros((16, 16, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.resize_area(x, 8, 8)  # host tensor
    with pytest.raises(ValueError):
        ops.resize_area(x.cuda()[:, ::2], 4, 4)  # not contiguous
    with pytest.raises(TypeError):
        ops.resize_area(x.cuda().float(), 8, 8)
    with pytest.raises(ValueError):
        ops.resize_area(x.cuda(), 17, 8)  # larger than the source
    with pytest.raises(ValueError):
        ops.resize_area(x.cuda(), 8, 17)
    with pytest.raises(ValueError):
        ops.resize_area(x.cuda(), 0, 8)
    with pytest.raises(ValueError):
        ops.resize_area(x.cuda(), 8, 0)
    with pytest.raises(ValueError):
        ops.resize_area(x.cuda()[:, :, :2], 8, 8)
