"""Several codecs and output kinds in ONE launch on gfx950, byte for byte against the CPU backend.

Every other GPU test launches batches of one kind; the offsets of the different kinds of region
(csrc/vep/stage_plan.h) meet only in a mixed batch: fast-path index tables, H.264 records and
rounds (8-bit frames with a frame history, High 10, PAFF field pairs and their weave), H.265
records, rounds and TU tables, history conversions, letterbox rows and two levels of privacy masks.

Three decode_many batches go through a GPU and a CPU worker with the same cameras: one access
unit per camera, then four (a catch-up job: unequal rounds and the history path), then one again.
The buffers' floors (4 MiB, 64 error words, 256 mask descriptors) are far above these pictures;
test_stage_buffers_regrow below goes over all three on stages that have already served a batch.
"""
import numpy as np
import pytest
import torch

import letterbox_checks as lc
import letterbox_oracle as lo
from conftest import high_encoder, synth
from history_util import narrow_planes
from test_avc_paff import PAFF
from video_edge_ai_proxy_amd import privacy

pytestmark = pytest.mark.gpu

S = 64
PIXELATE = [{"x0": 1000, "y0": 1500, "x1": 7000, "y1": 8000, "mode": "pixelate", "block": 8}]
TWO_FILLS = [{"x0": 0, "y0": 0, "x1": 6000, "y1": 6000, "mode": "fill", "b": 10, "g": 200, "r": 30},
             {"x0": 4000, "y0": 3000, "x1": 10000, "y1": 9000, "mode": "fill", "b": 250, "g": 5, "r": 90}]

# name, (w, h), history, bit depth, masks, encoder
CAMERAS = [
    ("fast", (176, 144), 0, 8, PIXELATE, lambda n: synth(n, 176, 144, gop=30, seed=2)),
    ("general", (320, 240), 3, 8, TWO_FILLS, lambda n: high_encoder(n, 320, 240, bframes=2, gop=12, seed=4)),
    ("high10", (176, 144), 0, 10, None, lambda n: high_encoder(n, 176, 144, gop=12, seed=5, bit_depth=10, bframes=2)),
    ("paff", (176, 144), 0, 8, None, lambda n: high_encoder(n, 176, 144, gop=6, seed=3, **PAFF)),
    ("hevc", (416, 240), 0, 8, None, lambda n: synth(n, 416, 240, gop=12, seed=6, codec="h265", compressed=True)),
]


WIDE_CAP = 0.08  # undecidable share accepted of the oracle at 416 x 240 (letterbox_checks: 0.05)


def check_rows(name, rows, chws, y8, uv8, w, h):
    """The GPU and the CPU row (rows / chws = [gpu, cpu]) under letterbox_checks.check_row, and
    equal to each other wherever the oracle decides the byte.

    At 416 x 240 the helper's own cap on the undecidable share (5 %) does not hold: its rounding
    bound grows with the source size (delta 0.0253 here against 0.0107 at 176 x 144), and a byte is
    undecidable when the oracle lies within delta of a rounding boundary, about 2 x delta of the
    bytes of a textured picture, so about 5 % at this size. The same per-byte band is applied
    there under WIDE_CAP, which leaves that estimate half as much again and is no value read off
    the rows under test."""
    d = lc.case_delta(w, h, S)
    canvas = lo.bgr_canvas(y8, uv8, w, h, 0, 0, S, lc.WORKER_PAD)
    low, high = np.floor(canvas + 0.5 - d), np.floor(canvas + 0.5 + d)
    for side, row, chw in zip(("gpu", "cpu"), rows, chws):
        if (w, h) != (416, 240):
            lc.check_row(f"{name} {side}", row, chw, y8, uv8, w, h, S, 0, torch.float32)
            continue
        inside = np.repeat(lo.inside_mask(w, h, S)[..., None], 3, axis=2)
        share = float((low != high)[inside].mean())
        assert not (low != high)[~inside].any() and share <= WIDE_CAP, f"{name}: oracle undecidable share {share:.2%}"
        got = row.reshape(S, S, 3).astype(np.float64)
        bad = (got < low) | (got > high)
        assert not bad.any(), f"{name} {side}: {int(bad.sum())} bytes outside the rule"
        lc.check_chw(f"{name} {side} chw", chw, lo.chw(canvas, lc.MEAN, lc.STD), d, lc.STD)
    g, c = (r.reshape(S, S, 3) for r in rows)
    differ = g != c
    assert not differ[low == high].any(), f"{name}: GPU and CPU rows differ at {int(differ[low == high].sum())} decided bytes"
    assert int(np.abs(g.astype(int) - c.astype(int)).max()) <= 1, f"{name}: GPU and CPU rows differ by more than one"


def make_worker(native, device):
    wk = native.Worker(device=device, letterbox_size=S, max_cameras=len(CAMERAS) + 1,
                       chw_dtype=lc.CHW_CODES[torch.float32], mean=list(lc.MEAN), std=list(lc.STD))
    bufs = lc.worker_buffers(S, 0, torch.float32, len(CAMERAS) + 1, "cpu" if device < 0 else "cuda")
    wk.set_consumer_buffers(bufs[0].data_ptr(), bufs[1].data_ptr(), len(CAMERAS) + 1)
    for k, (name, _, history, _, masks, _) in enumerate(CAMERAS):
        assert wk.add_camera(name, 4, history) == k
        if masks:
            wk.set_privacy_masks(k, privacy.to_native(masks))
    return wk, bufs


def test_mixed_batch_equals_the_cpu_backend(native):
    assert native.mask_levels(320, 240, privacy.to_native(TWO_FILLS)) == [0, 1], "the fills do not overlap"
    gpu, gbuf = make_worker(native, 0)
    cpu, cbuf = make_worker(native, -1)
    encs = [c[5](native) for c in CAMERAS]
    refs = [native.HevcDecoder() if name == "hevc" else native.CpuDecoder() for name, *_ in CAMERAS]
    planes = [{} for _ in CAMERAS]  # per camera: pts -> the reference decoder's (y, uv)
    for step, count in enumerate([1, 4, 1]):
        work = [(k, [enc.next() for _ in range(count)]) for k, enc in enumerate(encs)]
        for k, aus in work:
            for au in aus:
                out = refs[k].decode(au)
                if CAMERAS[k][0] == "hevc":
                    planes[k].update({pts: p for pts, _poc, _t, p in out})
                elif CAMERAS[k][0] == "fast":
                    planes[k] = {au.pts: refs[k].surface()}
                else:
                    planes[k].update(dict(refs[k].frames()))
        assert gpu.decode_many(work) == len(CAMERAS) and cpu.decode_many(work) == len(CAMERAS)
        torch.cuda.synchronize()
        grows, crows = gbuf[0].cpu().numpy(), cbuf[0].numpy()
        gchw = gbuf[1].cpu().view(torch.float32).view(-1, 3, S, S)
        cchw = cbuf[1].view(torch.float32).view(-1, 3, S, S)
        for k, (name, (w, h), history, bd, masks, _) in enumerate(CAMERAS):
            tag = f"batch {step} {name}"
            sg, sc = gpu.stats(k), cpu.stats(k)
            assert sg["errors"] == 0 and sc["errors"] == 0 and sg["published"] == sc["published"], (tag, sg, sc)
            a, b = gpu.read_latest(k, 0), cpu.read_latest(k, 0)
            assert (a is None) == (b is None), tag
            if a is None:  # (a first field, or a picture still in the reorder buffer: nothing published)
                assert sg["published"] == 0 and step == 0 and name != "fast", tag
                assert (grows[k] == 0xA5).all() and (crows[k] == 0xA5).all(), tag
                continue
            assert a[0]["pts"] == b[0]["pts"] and a[0]["seq"] == b[0]["seq"], tag
            assert np.array_equal(a[1], b[1]), f"{tag}: newest frame differs"
            ha, hb = gpu.read_history(k), cpu.read_history(k)
            assert [m["pts"] for m, _ in ha] == [m["pts"] for m, _ in hb], tag
            assert len(ha) == (min(3, sg["published"]) if history else 1), tag
            for (m, fa), (_, fb) in zip(ha, hb):
                assert np.array_equal(fa, fb), f"{tag}: history frame pts {m['pts']} differs"
            if name == "general":  # level 0 fill, and the level 1 fill over it where they overlap
                assert (a[1][10, 10] == [10, 200, 30]).all() and (a[1][h // 2, w // 2] == [250, 5, 90]).all(), tag
            # consumer rows: both backends under the oracle's rules on the reference decoder's planes
            y8, uv8 = narrow_planes(*planes[k][a[0]["pts"]], bd, 1)
            check_rows(tag, (grows[k], crows[k]), (gchw[k], cchw[k]), y8, uv8, w, h)
        assert (grows[len(CAMERAS)] == 0xA5).all(), "the unused row was written"


def test_stage_buffers_regrow(native):
    """Every stage of the lane first serves a one-camera batch (buffer pair at its 4 MiB floor, 64
    error words, 256 mask descriptors), then a batch above all three floors: 65 masked 64 x 48
    cameras with four masks each (65 error words, 260 descriptors) and two 1920 x 1080 keyframes
    (6 MiB of payload room). Each stage frees, reallocates and re-registers its buffers; every
    frame still equals the CPU backend's."""
    fills = [{"x0": 1000 * k, "y0": 500 * k, "x1": 1000 * k + 4000, "y1": 500 * k + 5000, "mode": "fill",
              "b": 40 * k, "g": 250 - 30 * k, "r": 7 * k} for k in range(4)]
    sizes = [(64, 48)] * 65 + [(1920, 1080)] * 2
    workers = [native.Worker(device=d, max_cameras=len(sizes)) for d in (0, -1)]
    for wk in workers:
        for k in range(len(sizes)):
            assert wk.add_camera(f"c{k}", 2) == k
            if k < 65:
                wk.set_privacy_masks(k, privacy.to_native(fills))
    encs = [synth(native, w, h, gop=1, seed=k + 1) for k, (w, h) in enumerate(sizes)]  # (keyframes only)
    everyone = range(len(sizes))
    for cams in ([0], [0], [0], everyone, everyone, everyone):  # (a lane has two or three stages)
        work = [(k, [encs[k].next()]) for k in cams]
        for wk in workers:
            assert wk.decode_many(work) == len(work)
        torch.cuda.synchronize()
        for k in cams:
            a, b = workers[0].read_latest(k, 0), workers[1].read_latest(k, 0)
            assert a is not None and b is not None and a[0]["pts"] == b[0]["pts"], k
            assert np.array_equal(a[1], b[1]), f"camera {k}: frame differs after the buffers grew"
            assert workers[0].stats(k)["errors"] == 0
    assert (workers[0].read_latest(3, 0)[1][30, 30] == [120, 160, 21]).all(), "the masks were not applied"
