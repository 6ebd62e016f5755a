"""Baseline JPEG encoder (CPU implementation) and its way up to REST, the CLI and the config.
Pillow (libjpeg) is the independent decoder and the fidelity yardstick."""
import io
import math
import time

import numpy as np
import pytest
from PIL import Image

from conftest import synth

# PSNR margin against Pillow's own encoder at the same quality and subsampling. It covers what
# differs by design: the integer FDCT (13-bit matrix, 3 fraction bits between the passes), the
# chroma mean's rounding and the restart intervals' DC resets do not change pixels, so the gaps are
# small. Measured gaps of the CPU encoder (dB, Pillow minus ours): gradient q50 0.03, q85 0.22;
# synthetic camera frame q50 and q85 below 0.1; noise / checkerboard / constant at q100 0.00. The
# largest, 0.22, rounded up to the next 0.25 dB:
MARGIN_DB = 0.25


def psnr(a, b) -> float:
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return math.inf if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


def decode(data: bytes):
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def decode_bgr(data: bytes):
    return np.asarray(decode(data).convert("RGB"))[:, :, ::-1]


def pillow_jpeg(bgr, q: int) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, "JPEG", quality=q, subsampling=2)
    return buf.getvalue()


def gradient(w=200, h=120):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(w + h - 2, 1)],
                    -1).astype(np.uint8)


def noise(w, h, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def checkerboard(w=64, h=48):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 3, -1)


def check_fidelity(native, img, q, what):
    ours = psnr(decode_bgr(native.jpeg_encode_cpu(img, q)), img)
    ref = psnr(decode_bgr(pillow_jpeg(img, q)), img)
    print(f"{what} q{q}: ours {ours:.3f} dB, Pillow {ref:.3f} dB, gap {ref - ours:.3f} dB")
    assert ours >= ref - MARGIN_DB, f"{what} q{q}: {ours:.2f} dB vs Pillow's {ref:.2f} dB"


def walk(data: bytes):
    """Markers of a JPEG stream in order: [(marker, payload)] up to SOS, then the entropy data's
    intervals and RSTm indices, then EOI."""
    assert data[:2] == b"\xff\xd8"
    segs, i = [(0xD8, b"")], 2
    while True:
        assert data[i] == 0xFF, f"marker expected at {i}"
        m = data[i + 1]
        n = (data[i + 2] << 8) | data[i + 3]
        segs.append((m, data[i + 4:i + 2 + n]))
        i += 2 + n
        if m == 0xDA:
            break
    rst, intervals, start = [], [], i
    while True:
        j = data.index(b"\xff", i)
        m = data[j + 1]
        if m == 0x00:  # stuffed byte
            i = j + 2
            continue
        intervals.append(data[start:j])
        if 0xD0 <= m <= 0xD7:
            rst.append(m - 0xD0)
            i = start = j + 2
            continue
        assert m == 0xD9 and j + 2 == len(data), "EOI expected at the end"
        segs.append((0xD9, b""))
        return segs, intervals, rst


# ---------------------------------------------------------------------------------- encoder

@pytest.mark.parametrize("w,h", [(16, 16), (17, 9), (1, 1), (200, 120), (1920, 1080)])
def test_decodes_with_pillow(native, w, h):
    img = gradient(w, h) if (w, h) != (17, 9) else noise(w, h)
    im = decode(native.jpeg_encode_cpu(img, 85))
    assert im.size == (w, h) and im.mode in ("YCbCr", "RGB") and im.format == "JPEG"
    if (w, h) != (17, 9):  # and it is the picture, not just a picture
        assert psnr(np.asarray(im.convert("RGB"))[:, :, ::-1], img) > 30


@pytest.mark.parametrize("q", [1, 25, 50, 85, 100])
def test_quant_tables_are_pillows(native, q):
    img = gradient()
    ours = decode(native.jpeg_encode_cpu(img, q)).quantization
    ref = decode(pillow_jpeg(img, q)).quantization
    assert {k: list(v) for k, v in ours.items()} == {k: list(v) for k, v in ref.items()}


@pytest.mark.parametrize("q", [50, 85])
def test_fidelity_gradient(native, q):
    check_fidelity(native, gradient(), q, "gradient 200x120")


@pytest.mark.parametrize("q", [50, 85])
def test_fidelity_camera_frame(native, q):
    enc = synth(native, 640, 480, gop=10)
    frame = native.CpuDecoder().decode(enc.next())
    check_fidelity(native, frame, q, "synthetic camera 640x480")


@pytest.mark.parametrize("what", ["checkerboard", "noise", "constant"])
def test_extremes_at_quality_100(native, what):
    img = {"checkerboard": checkerboard(), "noise": noise(64, 48), "constant": np.full((48, 64, 3), 77, np.uint8)}[what]
    data = native.jpeg_encode_cpu(img, 100)
    assert decode(data).size == (64, 48)
    check_fidelity(native, img, 100, what)
    if what == "constant":  # every block is its DC (difference) and an EOB
        assert len(data) < 800


def test_structure(native):
    w, h = 200, 120
    data = native.jpeg_encode_cpu(gradient(w, h), 85)
    segs, intervals, rst = walk(data)
    order = [m for m, _ in segs]
    want = [0xD8, 0xE0, 0xDB, 0xC0, 0xC4, 0xDD, 0xDA, 0xD9]  # SOI APP0 DQT SOF0 DHT DRI SOS EOI
    dedup = [m for k, m in enumerate(order) if k == 0 or order[k - 1] != m]
    assert dedup == want, [hex(m) for m in order]
    sof = dict(segs)[0xC0]
    assert sof[0] == 8 and (sof[1] << 8 | sof[2], sof[3] << 8 | sof[4]) == (h, w) and sof[5] == 3
    assert sof[6:15] == bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])  # 4:2:0
    dri = dict(segs)[0xDD]
    ri = dri[0] << 8 | dri[1]
    mcus = ((w + 15) // 16) * ((h + 15) // 16)
    assert 1 < ri < 16 and mcus % ri != 0  # the last interval is a partial one
    n = -(-mcus // ri)
    assert len(intervals) == n and n > 9
    assert rst == [k % 8 for k in range(n - 1)]
    assert all(len(s) > 0 for s in intervals)


def test_thousands_of_intervals_at_1080p(native):
    data = native.jpeg_encode_cpu(gradient(1920, 1080), 50)
    _, intervals, rst = walk(data)
    assert len(intervals) >= 2000 and rst[:9] == [0, 1, 2, 3, 4, 5, 6, 7, 0]


def test_deterministic(native):
    img = noise(200, 120, 3)
    assert native.jpeg_encode_cpu(img, 85) == native.jpeg_encode_cpu(img.copy(), 85)


def test_argument_checks(native):
    img = gradient(16, 16)
    for q in (0, 101, -1):
        with pytest.raises(Exception):
            native.jpeg_encode_cpu(img, q)
    with pytest.raises(Exception):
        native.jpeg_encode_cpu(img[:, :, :2], 85)
    with pytest.raises(Exception):
        native.jpeg_encode_cpu(np.zeros((0, 16, 3), np.uint8), 85)


def test_reference_op(native):
    import torch

    from video_edge_ai_proxy_amd import ops

    img = noise(48, 32, 5)
    assert ops.jpeg_encode_reference(torch.from_numpy(img), 85) == native.jpeg_encode_cpu(img, 85)
    with pytest.raises(ValueError):
        ops.jpeg_encode_reference(torch.from_numpy(img), 0)
    with pytest.raises(TypeError):
        ops.jpeg_encode_reference(torch.from_numpy(img).float(), 85)


def test_worker_ring_path_cpu_backend(native):
    enc = synth(native, 320, 240, gop=6)
    wk = native.Worker(device=-1)
    cam = wk.add_camera("c", 2)
    assert wk.read_latest_jpeg(cam, 0, 85) is None
    for _ in range(2):
        assert wk.decode_now(cam, enc.next())
    meta, frame = wk.read_latest(cam, 0)
    jmeta, jpg = wk.read_latest_jpeg(cam, 0, 70)
    assert jmeta["seq"] == meta["seq"] and jpg == native.jpeg_encode_cpu(frame, 70)
    assert wk.read_latest_jpeg(cam, meta["seq"], 70) is None
    with pytest.raises(Exception):
        wk.read_latest_jpeg(cam, 0, 0)


# ------------------------------------------------------------------------ REST, CLI, config

@pytest.fixture
def farm(native):
    srv = native.RtspServer("127.0.0.1", 0)
    cfg = native.SynthConfig()
    cfg.width, cfg.height, cfg.gop, cfg.fps, cfg.seed = 320, 240, 10, 30, 11
    srv.add_stream("/cam", cfg, realtime=True, cached_frames=20)
    srv.start()
    yield srv
    srv.stop()


@pytest.fixture
def hubapp(tmp_path, native):
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.server.app import build_app

    cfg = Config()
    cfg.data_dir = str(tmp_path / "data")
    cfg.gpu.devices = [-1]
    app = build_app(cfg, host="127.0.0.1", rest_port=0, grpc_port=0)
    yield app
    app.stop()


def _rest(app):
    from fastapi.testclient import TestClient

    from video_edge_ai_proxy_amd.server.rest import create_app

    return TestClient(create_app(app.pm, app.settings, app.metrics))


def _start_camera(rest, farm, name="front_door"):
    url = f"rtsp://127.0.0.1:{farm.port}/cam"
    assert rest.post("/api/v1/process", json={"name": name, "rtsp_endpoint": url}).status_code == 200
    deadline = time.time() + 15
    while time.time() < deadline:  # the first request wakes the lazy decoder
        r = rest.get(f"/api/v1/process/{name}/frame.jpg")
        if r.status_code == 200:
            return r
        assert r.status_code == 404
        time.sleep(0.05)
    raise AssertionError("no frame within 15 s")


def test_rest_frame_jpg(native, farm, hubapp):
    rest = _rest(hubapp)
    assert rest.get("/api/v1/process/front_door/frame.jpg").status_code == 404  # no such camera
    r = _start_camera(rest, farm)
    assert r.headers["content-type"] == "image/jpeg" and int(r.headers["x-vep-seq"]) >= 1
    assert decode(r.content).size == (320, 240)
    for bad in ("0", "101", "-3"):
        assert rest.get(f"/api/v1/process/front_door/frame.jpg?quality={bad}").status_code == 400
    assert rest.get("/api/v1/process/nope/frame.jpg").status_code == 404
    assert rest.get(f"/api/v1/process/front_door/frame.jpg?after={10 ** 9}").status_code == 404  # nothing newer
    # the same frame through /frame (PPM) and /frame.jpg: the camera is live, so take a pair
    # between which nothing was published
    for _ in range(50):
        seq = hubapp.hub.published("front_door")
        ppm = rest.get("/api/v1/process/front_door/frame")
        jpg = rest.get("/api/v1/process/front_door/frame.jpg?quality=85")
        if int(jpg.headers["x-vep-seq"]) == seq and hubapp.hub.published("front_door") == seq:
            break
    else:
        raise AssertionError("no quiet moment between two frames of a 30 fps camera")
    head, _, pixels = ppm.content.partition(b"\n")
    assert head == b"P6 320 240 255"
    frame = np.frombuffer(pixels, np.uint8).reshape(240, 320, 3)[:, :, ::-1]
    assert jpg.content == native.jpeg_encode_cpu(np.ascontiguousarray(frame), 85)
    ours, ref = psnr(decode_bgr(jpg.content), frame), psnr(decode_bgr(pillow_jpeg(frame, 85)), frame)
    print(f"frame.jpg: ours {ours:.3f} dB, Pillow {ref:.3f} dB")
    assert ours >= ref - MARGIN_DB
    # no quality named: serving.jpeg_quality
    hubapp.hub.cfg.serving.jpeg_quality = 20
    low = rest.get("/api/v1/process/front_door/frame.jpg")
    tables = lambda b: {k: list(v) for k, v in decode(b).quantization.items()}
    assert tables(low.content) == tables(pillow_jpeg(frame, 20))


def test_rest_stream_mjpg(native, farm, hubapp):
    rest = _rest(hubapp)
    assert rest.get("/api/v1/process/front_door/stream.mjpg?frames=1").status_code == 404
    _start_camera(rest, farm)
    assert rest.get("/api/v1/process/front_door/stream.mjpg?frames=1&quality=0").status_code == 400
    assert rest.get("/api/v1/process/front_door/stream.mjpg?frames=0").status_code == 400
    assert rest.get("/api/v1/process/front_door/stream.mjpg?frames=1&fps=0").status_code == 400
    r = rest.get("/api/v1/process/front_door/stream.mjpg?frames=3&fps=30&quality=60")
    assert r.status_code == 200
    ctype = r.headers["content-type"]
    assert ctype.startswith("multipart/x-mixed-replace") and "boundary=" in ctype
    boundary = ctype.split("boundary=")[1].encode()
    parts = r.content.split(b"--" + boundary + b"\r\n")
    assert parts[0] == b"" and len(parts) == 4
    seqs = []
    for p in parts[1:]:
        head, _, body = p.partition(b"\r\n\r\n")
        hdr = dict(line.split(": ") for line in head.decode().split("\r\n"))
        assert hdr["Content-Type"] == "image/jpeg"
        jpg = body[:int(hdr["Content-Length"])]
        assert body[len(jpg):] == b"\r\n" and decode(jpg).size == (320, 240)
        seqs.append(int(hdr["X-Vep-Seq"]))
    assert seqs[0] < seqs[1] < seqs[2]


def test_cli_frame_out_jpg(native, farm, hubapp, tmp_path, capsys):
    from video_edge_ai_proxy_amd import cli

    _start_camera(_rest(hubapp), farm)
    for name in ("f.jpg", "f.JPEG"):
        out = tmp_path / name
        cli.main(["frame", "--device", "front_door", "--grpc-port", str(hubapp.grpc_port), "--out", str(out)])
        assert decode(out.read_bytes()).size == (320, 240) and decode(out.read_bytes()).format == "JPEG"
    out = tmp_path / "f.ppm"  # other names: as before
    cli.main(["frame", "--device", "front_door", "--grpc-port", str(hubapp.grpc_port), "--out", str(out)])
    assert out.read_bytes().startswith(b"P6 320 240 255\n")


def test_config_jpeg_quality(tmp_path):
    from video_edge_ai_proxy_amd.config import load_config

    assert load_config(data_dir=str(tmp_path)).serving.jpeg_quality == 85
    (tmp_path / "conf.yaml").write_text("serving:\n  jpeg_quality: 70\n")
    assert load_config(data_dir=str(tmp_path)).serving.jpeg_quality == 70
    for bad in (0, 101):
        (tmp_path / "conf.yaml").write_text(f"serving:\n  jpeg_quality: {bad}\n")
        with pytest.raises(ValueError):
            load_config(data_dir=str(tmp_path))
