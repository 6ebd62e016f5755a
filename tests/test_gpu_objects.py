"""The gfx950 objects kernels (csrc/vep/gpu_objects.hip) against the CPU twin, byte for byte: luma
planes, packed mask, label plane, records (sorted by label) and count, at the plane sizes and masks
where a labelling kernel can go wrong, every source at its own address and pitch, batched; and
ops.label_objects and a GPU hub's answers against the CPU backend's."""
import numpy as np
import pytest
import torch

import objects_oracle as oracle
from test_gpu_clahe import placed
from test_objects import KINDS, TH, TW, hub_answers, mask_of

pytestmark = pytest.mark.gpu

OFFSETS, EXTRAS, GUARD = (0, 1, 5, 15), (0, 1, 16), 64


def guarded(nbytes, dev):
    return torch.full((GUARD + max(nbytes, 4) + GUARD,), 0xA5, dtype=torch.uint8, device=dev)


def run_and_compare(native, masks, d, threshold=0, open=0, grow=0, min_area=4):
    """One batch: picture n shows masks[n] at decimate d with trailing pixels the planes do not use,
    both sources at their own offset and pitch, every output in a caller-owned buffer between guard
    bytes of 0xA5. Returns the records of every picture."""
    dev = torch.device("cuda", 0)
    work, keep = [], []
    for n, m in enumerate(masks):
        ph, pw = m.shape
        newer, older = oracle.pictures(m, d, (n % d, (n // 2) % d))
        h, w = newer.shape[:2]
        src = [placed(f, OFFSETS[(n + i) % 4], EXTRAS[(n + 2 * i) % 3], dev) for i, f in enumerate((newer, older))]
        pitch = native.flow_plane_pitch(pw)
        half, words, cap = (pitch * ph + 255) & ~255, (pw + 63) // 64 * ph, pw * ph // min_area
        bufs = {"planes": guarded(2 * half, dev), "mask": guarded(words * 8, dev), "labels": guarded(pw * ph * 4, dev),
                "area": guarded(pw * ph * 4, dev), "records": guarded(cap * 24, dev), "count": guarded(4, dev)}
        at = {k: b.data_ptr() + GUARD for k, b in bufs.items()}
        assert at["planes"] % 16 == 0 and at["mask"] % 8 == 0
        span = [(s.data_ptr(), (h - 1) * s.stride(0) + w * 3, s.stride(0)) for s in src]
        work.append((span[0], span[1], at["planes"], at["planes"] + half, half, at["mask"], words, at["labels"], at["area"],
                     pw * ph, at["records"], cap, at["count"], w, h))
        keep.append((newer, older, src, bufs, pitch, half, words, cap))
    native.objects_device_batch(work, d, threshold, open, grow, min_area, int(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    out = []
    for n, (m, (newer, older, src, bufs, pitch, half, words, cap)) in enumerate(zip(masks, keep)):
        ph, pw = m.shape
        what = (n, pw, ph, d, open, grow, min_area)
        want_rec, want_lab, want_mask = native.objects_cpu(newer, older, d, threshold, open, grow, min_area)
        want_planes = native.flow_cpu(newer, older, d, 1)[0]
        b = {k: v.cpu().numpy() for k, v in bufs.items()}
        for k in range(2):
            rows = b["planes"][GUARD + k * half:GUARD + k * half + pitch * ph].reshape(ph, pitch)
            assert np.array_equal(rows[:, :pw], want_planes[k]), ("plane", k) + what
            assert (rows[:, pw:] == 0xA5).all() and (b["planes"][GUARD + k * half + pitch * ph:GUARD + (k + 1) * half] == 0xA5).all(), \
                ("a plane row's padding was written", k) + what
        got_mask = b["mask"][GUARD:GUARD + words * 8].copy().view(np.uint64).reshape(want_mask.shape)
        assert np.array_equal(got_mask, want_mask), ("mask",) + what
        got_lab = b["labels"][GUARD:GUARD + pw * ph * 4].copy().view(np.uint32).reshape(want_lab.shape)
        assert np.array_equal(got_lab, want_lab), ("labels",) + what
        count = int(b["count"][GUARD:GUARD + 4].copy().view(np.uint32)[0])
        assert count == len(want_rec) <= cap, ("count",) + what
        rec = b["records"][GUARD:GUARD + count * 24].copy().view(np.uint32).reshape(count, 6).astype(np.int64)
        assert np.array_equal(rec[np.argsort(rec[:, 0])], want_rec), ("records",) + what
        assert (b["records"][GUARD + count * 24:] == 0xA5).all(), ("bytes behind the records",) + what
        used = {"planes": 2 * half, "mask": words * 8, "labels": pw * ph * 4, "area": pw * ph * 4, "records": cap * 24, "count": 4}
        for k, v in b.items():
            assert (v[:GUARD] == 0xA5).all() and (v[GUARD + used[k]:] == 0xA5).all(), ("guard bytes", k) + what
        for f, s in zip((newer, older), src):
            assert np.array_equal(s.cpu().numpy(), f), ("a source was written",) + what
        out.append(want_rec)
    return out


@pytest.mark.parametrize("ph", [1, TH - 1, TH, TH + 1, 2 * TH + 1])
@pytest.mark.parametrize("pw", [1, TW - 1, TW, TW + 1, 2 * TW + 1])
def test_kernels_equal_the_twin(native, pw, ph):
    """Below, at and above one ballot word and one tile of 64 x 32, and a second tile each way (TW is
    one ballot word, so the issue's 63, 64, 65 are TW - 1, TW, TW + 1). Every mask kind in one batch;
    a case walks through d."""
    run_and_compare(native, [mask_of(k, pw, ph, seed=pw + ph) for k in KINDS], (1, 2, 4)[(pw + ph) % 3])


@pytest.mark.parametrize("open,grow", [(0, 0), (1, 0), (0, 1), (1, 1), (0, 3), (1, 2), (1, 3)])
def test_cleanup_and_a_batch_of_sizes(native, open, grow):
    """Seeded 50 % noise (and a solid block that survives an opening) through every cleanup, pictures of
    different sizes in one batch; min_area 4 against one that drops some but not all components."""
    shapes = [(7, 3), (64, 32), (100, 50), (5, 70), (200, 9), (130, 66), (33, 33)]
    masks = [mask_of("noise", pw, ph, seed=n + 10 * grow) for n, (pw, ph) in enumerate(shapes)]
    for m in masks:
        m[m.shape[0] // 3:m.shape[0] // 3 + 9, 2:30] = True
    d = (1, 2, 4)[(open + grow) % 3]
    many = run_and_compare(native, masks, d, 24, open, grow, 4)
    some = run_and_compare(native, masks, d, 24, open, grow, 40)
    assert 0 < sum(map(len, some)) and (open or grow or sum(map(len, some)) < sum(map(len, many)))


def test_capacity_bound(native):
    """A record buffer of floor(w' h' / min_area) slots never overflows: a full 2 x 2 plane fills its
    single slot, isolated 2 x 2 blocks are the most records a plane can hold (run_and_compare asserts
    count <= capacity and the bytes behind the records untouched), and the lattice of single samples,
    the most components there can be, yields none."""
    rec = run_and_compare(native, [mask_of("full", 2, 2), mask_of("blocks", 2 * TW + 1, 2 * TH + 1), mask_of("lattice", 2 * TW + 1, TH)], 1)
    assert [len(r) for r in rec] == [1, 43 * 22, 0]


def test_ops_and_hub_equal_the_cpu_backend(native, tmp_path):
    from video_edge_ai_proxy_amd import ops

    newer, older = oracle.pictures(mask_of("noise", 150, 100, seed=3), 2, (1, 0))
    rec, lab = ops.label_objects(torch.from_numpy(newer).cuda(), torch.from_numpy(older).cuda(), open=0, planes=True)
    host_rec, host_lab = ops.label_objects(torch.from_numpy(newer), torch.from_numpy(older), open=0, planes=True)
    assert torch.equal(rec.cpu(), host_rec) and torch.equal(lab.cpu(), host_lab) and lab.shape == (100, 150) and len(rec)
    gpu, cpu = hub_answers(native, tmp_path, 0), hub_answers(native, tmp_path, -1)
    assert all(np.array_equal(a, b) for n in "ab" for a, b in zip(gpu[0][n], cpu[0][n]))  # the same frames
    assert gpu[1:] == cpu[1:] and gpu[1]["primed"]
