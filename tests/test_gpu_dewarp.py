"""gfx950 views: byte equality of the dewarp kernel with the CPU implementation (held to the numpy
oracle in tests/test_dewarp.py), sources and outputs at offsets modulo 16 inside guarded buffers,
a mixed batch, and the ring reads of a GPU camera against the CPU backend's (run on an MI355X).
dewarp_cases.mesh_of says which mesh reaches the kernel's pad, staged and global tiles."""
import numpy as np
import pytest
import torch

import dewarp_cases as dc
from test_gpu_crop import GUARD, MASKS, SENTINEL, _NoSession, _feeds, device_view
from conftest import synth
from video_edge_ai_proxy_amd import ops, privacy, views

pytestmark = pytest.mark.gpu


def run_guarded(src, mesh, W, H, pad, lead):
    """ops.remap into a view `lead` bytes past a 16-byte boundary of a buffer of sentinels: the
    view, after asserting that not one guard byte before or after it was written."""
    n = H * W * 3
    buf = torch.full((GUARD + lead + n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[GUARD + lead:GUARD + lead + n].view(H, W, 3)
    assert out.data_ptr() % 16 == lead and ops.remap(src, mesh, W, H, pad, out=out) is out
    host = buf.cpu().numpy()
    assert (host[:GUARD + lead] == SENTINEL).all() and (host[GUARD + lead + n:] == SENTINEL).all(), "guard bytes written"
    return host[GUARD + lead:GUARD + lead + n].reshape(H, W, 3)


@pytest.mark.parametrize("kind", dc.MESHES)
@pytest.mark.parametrize("size", dc.SOURCES)
def test_byte_equal(native, size, kind):
    """kernel == CPU twin over the CPU test's cases, the source at offset k and the output at
    offset 7k + 3 modulo 16."""
    w, h = size
    p = dc.picture(w, h, seed=w)
    srcs = [device_view(p, lead) for lead in range(16)]
    for k, (ow, oh) in enumerate(dc.OUT_SIZES):
        mesh = dc.mesh_of(kind, w, h, ow, oh)
        got = run_guarded(srcs[k % 16], mesh, ow, oh, dc.PAD, (7 * k + 3) % 16)
        want = native.remap_cpu(p, mesh, ow, oh, dc.PAD)
        assert np.array_equal(got, want), f"{kind} {w}x{h} -> {ow}x{oh}: {int((got != want).sum())} bytes differ"


def test_every_output_offset_and_a_wide_picture(native):
    """Every output offset modulo 16 on a staged mesh and a global one; then 4000 x 40 -> 700 x 20:
    a tile's footprint of about 366 x 38 pixels is above the staging buffer (global), 11 tiles a row."""
    p = dc.picture(200, 120, seed=6)
    for kind in ("smooth", "minify6"):
        mesh = dc.mesh_of(kind, 200, 120, 65, 33)
        want = native.remap_cpu(p, mesh, 65, 33, dc.PAD)
        for lead in range(16):
            assert np.array_equal(run_guarded(device_view(p, 15 - lead), mesh, 65, 33, dc.PAD, lead), want), (kind, lead)
    p = dc.picture(4000, 40, seed=7)
    mesh = dc.mesh_of("smooth", 4000, 40, 700, 20)
    assert np.array_equal(run_guarded(device_view(p, 5), mesh, 700, 20, dc.PAD, 9), native.remap_cpu(p, mesh, 700, 20, dc.PAD))


def test_batch_mixed_sizes(native):
    """Five pictures of three sizes with 0, 1 and 3 views each, of different sizes, in one launch."""
    sizes = [(200, 120), (17, 9), (64, 48), (200, 120), (17, 9)]
    plan = [["smooth", "minify6", "garbage"], [], ["identity"], ["half_inside"], ["rot90", "outside", "smooth"]]
    outs = [(130, 33), (65, 17), (17, 16)]
    a = [dc.picture(w, h, seed=k) for k, (w, h) in enumerate(sizes)]
    dev = [torch.from_numpy(x).cuda() for x in a]
    pics, meshes, whs, want = [], [], [], []
    for k, kinds in enumerate(plan):
        for i, kind in enumerate(kinds):
            ow, oh = outs[i]
            meshes.append(dc.mesh_of(kind, *sizes[k], ow, oh, seed=k))
            pics.append(dev[k])
            whs.append((ow, oh))
            want.append(native.remap_cpu(a[k], meshes[-1], ow, oh, dc.PAD))
    got = ops.remap_batch(pics, meshes, whs, dc.PAD)
    assert len(got) == 8
    for g, wnt in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), wnt)
    assert ops.remap_batch([], [], []) == []
    with pytest.raises(ValueError):
        ops.remap(torch.from_numpy(a[0]), meshes[0], 130, 33)  # a host tensor
    with pytest.raises(ValueError):
        ops.remap(dev[0], meshes[0], 145, 33)  # the mesh of another size


LENS = {"model": "equidistant", "fov_deg": 200}
VIEWS = [{"type": "ptz", "pan": 20, "tilt": 10, "fov": 80, "width": 96, "height": 64},
         {"type": "panorama", "pan0": -100, "pan1": 100, "tilt0": 40, "tilt1": -40, "width": 400, "height": 100}]


def _answers(native, device, feed, history, masks):
    wk = native.Worker(device=device)
    cam = wk.add_camera("c", wk.history_ring_slots(history), history)
    if masks:
        wk.set_privacy_masks(cam, privacy.to_native(masks))
    feed(wk, cam)
    frames = wk.read_history(cam, 0, history)
    w, h = frames[0][1].shape[1], frames[0][1].shape[0]
    meshes = [views.build_mesh(LENS, v, w, h) for v in VIEWS]
    out = {}
    for seq in [0] + [m["seq"] for m, _ in frames]:
        out[seq] = [wk.read_view(cam, m, w, h, v["width"], v["height"], seq=seq, pad=dc.PAD) for m, v in zip(meshes, VIEWS)]
        out[seq].append(wk.read_view_jpeg(cam, meshes[0], w, h, 96, 64, seq=seq, quality=80))
    assert wk.read_view(cam, meshes[0], w + 16, h, 96, 64)[1] is None  # a mesh for another size
    return frames, meshes, out


@pytest.mark.parametrize("path", ["fast", "h264"])
@pytest.mark.parametrize("masked", [False, True])
def test_ring_views_equal_the_cpu_backend(native, path, masked):
    feed, history = _feeds(native)[path]
    fg, meshes, gpu = _answers(native, 0, feed, history, MASKS if masked else None)
    fc, _, cpu = _answers(native, -1, feed, history, MASKS if masked else None)
    assert len(fg) == len(fc) == history and list(gpu) == list(cpu)
    by_seq = {m["seq"]: f for m, f in fg}
    for seq in gpu:
        frame = by_seq[seq or max(by_seq)]
        for k in range(2):
            assert gpu[seq][k][0]["seq"] == cpu[seq][k][0]["seq"] == (seq or max(by_seq))
            assert np.array_equal(gpu[seq][k][1], cpu[seq][k][1]), f"{path} seq {seq} view {k}: GPU and CPU backends differ"
            assert np.array_equal(gpu[seq][k][1], native.remap_cpu(frame, meshes[k], VIEWS[k]["width"], VIEWS[k]["height"], dc.PAD))
        assert gpu[seq][2][1] == cpu[seq][2][1] == native.jpeg_encode_cpu(native.remap_cpu(frame, meshes[0], 96, 64), 80)


def test_hub_views_many_on_the_gpu(native, tmp_path):
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.engine.hub import CameraHandle, Hub

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    hub = Hub(cfg, devices=[0])
    try:
        frames = {}
        for k, (name, w, h) in enumerate([("a", 320, 240), ("b", 160, 96), ("c", 640, 480)]):
            cam = hub.workers[0].add_camera(name, 2)
            hub.cameras[name] = CameraHandle(name, 0, cam, "", session=_NoSession())
            assert hub.workers[0].decode_now(cam, synth(native, w, h, gop=6, motion=0.2, seed=k + 1).next())
            frames[name] = hub.workers[0].read_latest(cam, 0)[1]
            hub.set_views(name, LENS, {"pano": VIEWS[1]})
        asked = {"c": "pano", "a": VIEWS[0], "b": "pano"}
        many = hub.views_many(asked, pad=dc.PAD)
        for n, v in asked.items():
            v = VIEWS[1] if v == "pano" else v
            mesh = views.build_mesh(LENS, v, frames[n].shape[1], frames[n].shape[0])
            assert many[n][0] == 1 and np.array_equal(many[n][1], native.remap_cpu(frames[n], mesh, v["width"], v["height"], dc.PAD))
        seq, jpg = hub.view_jpeg("c", "pano", quality=75)
        assert jpg == native.jpeg_encode_cpu(native.remap_cpu(frames["c"], views.build_mesh(LENS, VIEWS[1], 640, 480), 400, 100), 75)
    finally:
        hub.shutdown()
