"""The gfx950 flow kernels (csrc/vep/gpu_flow.hip) against the CPU twin, byte for byte: luma planes
and records, at the shapes where the kernels can go wrong, every source at its own address and
pitch, batched; and a GPU hub's answers against the CPU backend's."""
import numpy as np
import pytest
import torch

from test_flow import KINDS, hub_answers, pair
from test_gpu_clahe import placed

pytestmark = pytest.mark.gpu

OFFSETS, EXTRAS, GUARD = (0, 1, 5, 15), (0, 1, 16), 64
DS, RS = (1, 2, 4), (1, 7, 15)


def run_and_compare(native, jobs, d, R):
    """jobs: (plane width, plane height, kind, n). One batch: both sources of job n at their own offset
    and pitch, planes and records in caller-owned buffers between guard bytes of 0xA5."""
    dev = torch.device("cuda", 0)
    work, keep = [], []
    for pw, ph, kind, n in jobs:
        w, h = pw * d + (n % d), ph * d + ((n // 2) % d)  # trailing pixels that the planes do not use
        newer, older = pair(kind, w, h, d, R, seed=n)
        src = [placed(f, OFFSETS[(n + i) % 4], EXTRAS[(n + 2 * i) % 3], dev) for i, f in enumerate((newer, older))]
        pitch = native.flow_plane_pitch(pw)
        half, nrec = (pitch * ph + 255) & ~255, (ph // 8) * (pw // 8)
        planes = torch.full((GUARD + max(2 * half, 256) + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        records = torch.full((GUARD + max(nrec, 1) * 8 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        assert (planes.data_ptr() + GUARD) % 16 == 0 and (records.data_ptr() + GUARD) % 8 == 0
        span = [(s.data_ptr(), (h - 1) * s.stride(0) + w * 3, s.stride(0)) for s in src]
        work.append((span[0], span[1], planes.data_ptr() + GUARD, planes.data_ptr() + GUARD + half, half,
                     records.data_ptr() + GUARD, max(nrec, 1), w, h))
        keep.append((newer, older, src, planes, records, pitch, half, nrec))
    native.flow_device_batch(work, d, R, int(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    for (pw, ph, kind, n), (newer, older, src, planes, records, pitch, half, nrec) in zip(jobs, keep):
        what = (pw, ph, kind, n, d, R)
        want_planes, want = native.flow_cpu(newer, older, d, R)
        p, r = planes.cpu().numpy(), records.cpu().numpy()
        for k in range(2):
            rows = p[GUARD + k * half:GUARD + k * half + pitch * ph].reshape(ph, pitch)
            assert np.array_equal(rows[:, :pw], want_planes[k]), ("plane", k) + what
            assert (rows[:, pw:] == 0xA5).all() and (p[GUARD + k * half + pitch * ph:GUARD + (k + 1) * half] == 0xA5).all(), \
                ("a plane row's padding was written", k) + what
        rec = r[GUARD:GUARD + nrec * 8].reshape(nrec, 8)
        got = np.concatenate([rec[:, :2].view(np.int8).astype(np.int16), rec[:, 2:6].copy().view(np.int16)], axis=1)
        assert np.array_equal(got.reshape(want.shape), want) and not rec[:, 6:].any(), ("records",) + what
        for buf, used in ((p, max(2 * half, 256)), (r, nrec * 8)):
            assert (buf[:GUARD] == 0xA5).all() and (buf[GUARD + max(used, 0):][-GUARD:] == 0xA5).all(), ("guard bytes",) + what
        assert (r[GUARD + nrec * 8:] == 0xA5).all(), ("bytes behind the records",) + what
        for f, s in zip((newer, older), src):
            assert np.array_equal(s.cpu().numpy(), f), ("a source was written",) + what


@pytest.mark.parametrize("ph", [8, 31, 32, 33, 40])
@pytest.mark.parametrize("pw", [8, 15, 63, 64, 65, 72, 136])
def test_kernels_equal_the_twin(native, pw, ph):
    """One block; below, at and above one tile of 8 x 4 blocks; a second tile each way. A case walks
    through d and R, and its pictures through the input kinds."""
    c = pw * 3 + ph
    d, R = DS[c % 3], RS[(c // 3) % 3]
    run_and_compare(native, [(pw, ph, (c + i) % KINDS, c + i) for i in range(3)], d, R)


@pytest.mark.parametrize("R", [1, 4, 7, 8, 11, 15])  # every split of the candidates over a wave: N = 1, 1, 1, 2, 3, 4
def test_every_range_split_and_a_batch_of_sizes(native, R):
    shapes = [(7, 7), (64, 32), (100, 50), (8, 70), (200, 9), (136, 40), (33, 33)]
    run_and_compare(native, [(pw, ph, n % KINDS, 50 + n) for n, (pw, ph) in enumerate(shapes)], DS[R % 3], R)


def test_ops_and_hub_equal_the_cpu_backend(native, tmp_path):
    from video_edge_ai_proxy_amd import ops

    newer, older = pair(1, 300, 200, 2, 7)
    grid, planes = ops.block_flow(torch.from_numpy(newer).cuda(), torch.from_numpy(older).cuda(), planes=True)
    host_grid, host_planes = ops.block_flow(torch.from_numpy(newer), torch.from_numpy(older), planes=True)
    assert torch.equal(grid.cpu(), host_grid) and torch.equal(planes.cpu(), host_planes) and grid.shape == (12, 18, 4)
    gpu, cpu = hub_answers(native, tmp_path, 0), hub_answers(native, tmp_path, -1)
    assert all(np.array_equal(a, b) for n in "ab" for a, b in zip(gpu[0][n], cpu[0][n]))  # the same frames
    assert gpu[1:] == cpu[1:] and gpu[1]["primed"] and len(gpu[1]["vx"]) == 20 * 15
