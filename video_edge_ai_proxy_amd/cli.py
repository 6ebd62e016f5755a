"""``python -m video_edge_ai_proxy_amd <command>`` — daemon, synthetic camera farm, clients.

  serve     hub daemon: REST :8080 + gRPC :50001 (server/main.go analog)
  camera    single-camera hub (python/rtsp_to_rtmp.py flags: --rtsp --rtmp --device_id
            --memory_buffer --disk_path)
  farm      synthetic RTSP camera farm (H.264 I_PCM/P_Skip streams) for tests and benchmarks
  list | frame | annotate | storage | proxy   gRPC clients (examples/*.py analogs)
  motion    REST client of the motion detector (--device NAME --rest host:port [--watch])
  tamper    REST client of the tamper detector (--device NAME --rest host:port [--watch] [--set-reference])
  privacy   REST client of a camera's privacy masks (--device NAME --rest host:port [--set JSON | --clear])
  crop      REST client of crop.jpg: one box of a frame as a JPEG (--device NAME --rest host:port
            --box x0,y0,x1,y1 --size WxH [--seq N] --out f.jpg)
"""
from __future__ import annotations

import argparse
import os
import sys
import time


def _addr(a):
    return f"{a.host}:{a.grpc_port}"


def cmd_serve(a):
    from .config import load_config
    from .server.app import run_forever
    from .utils import setup_logging

    setup_logging(a.log_level)
    cfg = load_config(a.config, data_dir=a.data_dir)
    if a.port is not None:
        cfg.port = a.port
    if a.grpc_port is not None:
        cfg.grpc_port = a.grpc_port
    if a.isolate:
        cfg.gpu.isolation = "process"
    devices = [int(x) for x in a.devices.split(",")] if a.devices else None
    run_forever(cfg, host=a.bind, devices=devices)


def cmd_camera(a):
    from .config import load_config
    from .models import StreamProcess
    from .server.app import build_app
    from .utils import setup_logging

    setup_logging(a.log_level)
    cfg = load_config(None, data_dir=a.data_dir)
    cfg.buffer.in_memory = a.memory_buffer
    if a.disk_path:
        cfg.buffer.on_disk = True
        cfg.buffer.on_disk_folder = a.disk_path
    app = build_app(cfg, host=a.bind, rest_port=a.port, grpc_port=a.grpc_port, restore=False)
    app.pm.start(StreamProcess(name=a.device_id, rtsp_endpoint=a.rtsp, rtmp_endpoint=a.rtmp or ""))
    print(f"camera {a.device_id}: gRPC :{app.grpc_port} REST :{app.rest_port}", flush=True)
    try:
        while True:
            time.sleep(3600)
    except KeyboardInterrupt:
        app.stop()


def cmd_farm(a):
    from . import native

    srv = native.RtspServer(a.bind, a.port)
    for i in range(a.cams):
        c = native.SynthConfig()
        c.width, c.height, c.fps, c.gop, c.motion = a.width, a.height, a.fps, a.gop, a.motion
        c.seed = 1 + i
        c.codec = a.codec
        c.idr_phase = (i * a.gop) // max(1, a.cams)
        srv.add_stream(f"/cam{i}", c, realtime=not a.unpaced, cached_frames=a.cached_frames)
    srv.start()
    for i in range(a.cams):
        print(f"rtsp://{a.bind}:{srv.port}/cam{i}", flush=True)
    try:
        while True:
            time.sleep(3600)
    except KeyboardInterrupt:
        srv.stop()


def cmd_list(a):
    from .proto import pb
    from .server.grpc_server import ImageClient

    cli = ImageClient(_addr(a))
    for s in cli.ListStreams(pb.ListStreamRequest()):
        print(s)


def write_frame(path: str, img) -> None:
    """Write a BGR24 picture: ``.jpg`` / ``.jpeg`` as a JPEG (the hub's encoder, on the host), any
    other name as a PPM."""
    h, w = img.shape[:2]
    if path.lower().endswith((".jpg", ".jpeg")):
        from ._native import native

        data = native.jpeg_encode_cpu(img, 85)
    else:
        data = f"P6 {w} {h} 255\n".encode() + img[:, :, ::-1].tobytes()
    with open(path, "wb") as f:
        f.write(data)


def frame_jpg_url(a) -> str:
    """The frame.jpg request of ``vep frame --overlay / --stamp``."""
    import urllib.parse

    q = {}
    if a.overlay:
        q["overlay"] = "1"
    if a.stamp:
        q["stamp"] = "1"
    for k in ("width", "height"):
        if getattr(a, k) is not None:
            q[k] = str(getattr(a, k))
    return (f"http://{a.rest}/api/v1/process/{urllib.parse.quote(a.device, safe='')}/frame.jpg?"
            + urllib.parse.urlencode(q))


def cmd_frame_osd(a):
    """``vep frame --overlay / --stamp``: the on-screen display is drawn by the hub (on its GPU) onto
    the JPEG it serves, so the frame comes from ``frame.jpg`` over REST and is written as it is."""
    import json
    import urllib.error
    import urllib.request

    if not a.out or not a.out.lower().endswith((".jpg", ".jpeg")):
        raise SystemExit("frame: --overlay / --stamp write a JPEG: --out FILE.jpg")
    try:
        with urllib.request.urlopen(frame_jpg_url(a), timeout=10) as r:
            jpg, seq = r.read(), r.headers.get("X-Vep-Seq")
    except urllib.error.HTTPError as e:
        detail = ""
        try:
            detail = ": " + json.loads(e.read()).get("message", "")
        except ValueError:
            pass
        raise SystemExit(f"frame: HTTP {e.code} for {a.device!r}{detail}")
    with open(a.out, "wb") as f:
        f.write(jpg)
    print(f"seq {seq}: {len(jpg)} bytes -> {a.out}", flush=True)


def cmd_overlay(a):
    """REST client of ``/api/v1/process/{name}/overlay``: ``--set`` replaces the camera's stored
    on-screen display list with a JSON list of items (``--ttl-ms``: for that long), ``--clear``
    removes it; the list in force is printed afterwards."""
    import json
    import urllib.error
    import urllib.parse
    import urllib.request

    if a.set is not None and a.clear:
        raise SystemExit("overlay: --set and --clear exclude each other")
    url = f"http://{a.rest}/api/v1/process/{urllib.parse.quote(a.device, safe='')}/overlay"
    try:
        if a.set is not None:
            try:
                items = json.loads(a.set)
            except ValueError as e:
                raise SystemExit(f"overlay: --set is not JSON: {e}")
            body = json.dumps({"items": items, "ttl_ms": a.ttl_ms}).encode()
            req = urllib.request.Request(url, data=body, method="PUT", headers={"Content-Type": "application/json"})
            urllib.request.urlopen(req, timeout=10).close()
        elif a.clear:
            urllib.request.urlopen(urllib.request.Request(url, method="DELETE"), timeout=10).close()
        with urllib.request.urlopen(url, timeout=10) as r:
            items = json.loads(r.read()).get("items", [])
        print(f"{len(items)} item(s)" + "".join("\n  " + json.dumps(i, sort_keys=True) for i in items), flush=True)
    except urllib.error.HTTPError as e:
        detail = ""
        try:
            detail = ": " + json.loads(e.read()).get("message", "")
        except ValueError:
            pass
        raise SystemExit(f"overlay: HTTP {e.code} for {a.device!r}{detail}")


def cmd_frame(a):
    if a.overlay or a.stamp:
        return cmd_frame_osd(a)
    import numpy as np

    from .server.grpc_server import ImageClient

    cli = ImageClient(_addr(a))
    for _ in range(a.count):
        vf = cli.latest_frame(a.device, a.keyframe)
        print("is keyframe:", vf.is_keyframe, "frame type:", vf.frame_type,
              "shape:", [d.size for d in vf.shape.dim], "pts:", vf.pts)
        if a.out and vf.width:
            img = np.frombuffer(vf.data, np.uint8).reshape(vf.height, vf.width, 3)
            if a.width or a.height:
                # fitted into the box, never enlarged; area-averaged on the host (the hub's
                # frame.jpg?width=&height= does the same on the GPU)
                from ._native import native

                for v in (a.width, a.height):
                    if v is not None and not 1 <= v <= 65535:
                        raise SystemExit("--width / --height must be 1..65535")
                ow, oh = native.fit_geometry(vf.width, vf.height, a.width or 0, a.height or 0)
                img = native.resize_area_cpu(np.ascontiguousarray(img), ow, oh)
            write_frame(a.out, img)


def cmd_annotate(a):
    from .proto import pb
    from .server.grpc_server import ImageClient

    cli = ImageClient(_addr(a))
    now = int(time.time() * 1000)
    req = pb.AnnotateRequest(device_name=a.device, type=a.type, start_timestamp=now,
                             end_timestamp=now + 1000, object_type="person", confidence=0.9,
                             object_bouding_box=pb.BoudingBox(top=10, left=10, width=100, height=200),
                             ml_model="synthetic", ml_model_version="1")
    print(cli.Annotate(req))


def _bool(s):
    return str(s).lower() in ("1", "true", "yes", "on", "y", "t")


def cmd_storage(a):
    from .proto import pb
    from .server.grpc_server import ImageClient

    print(ImageClient(_addr(a)).Storage(pb.StorageRequest(device_id=a.device, start=_bool(a.on))))


def cmd_proxy(a):
    from .proto import pb
    from .server.grpc_server import ImageClient

    print(ImageClient(_addr(a)).Proxy(pb.ProxyRequest(device_id=a.device, passthrough=_bool(a.on))))


def format_motion(m: dict) -> str:
    """One line per evaluated frame of ``vep motion``."""
    box = "-" if m.get("box") is None else "{},{} {}x{}".format(*m["box"])
    flag = "MOTION" if m.get("motion") else ("still" if m.get("primed", True) else "primed")
    return (f"seq {m['seq']} {flag} changed {m.get('changed', 0)} ({100.0 * m.get('score', 0.0):.2f} %) "
            f"active {m.get('active', 0)} box {box}")


def cmd_motion(a):
    """REST client of ``/api/v1/process/{name}/motion``: one line per new evaluated frame."""
    import json
    import urllib.error
    import urllib.parse
    import urllib.request

    base = f"http://{a.rest}/api/v1/process/{urllib.parse.quote(a.device, safe='')}/motion"
    seq, idle = 0, 0
    while True:
        try:
            with urllib.request.urlopen(f"{base}?after={seq}", timeout=10) as r:
                m = json.loads(r.read())
        except urllib.error.HTTPError as e:
            if e.code != 404 or b"not found" in e.read():
                raise SystemExit(f"motion: HTTP {e.code} for {a.device!r}")
            m = None  # no newer frame yet
        if m is not None:
            seq, idle = int(m["seq"]), 0
            print(format_motion(m), flush=True)
            if not a.watch:
                return
        else:
            idle += 1
            if not a.watch and idle * a.interval > 10.0:
                raise SystemExit(f"motion: no frame of {a.device!r} within 10 s")
        time.sleep(a.interval)


def format_tamper(m: dict) -> str:
    """One line per evaluated frame of ``vep tamper``."""
    flag = "TAMPERED " + ",".join(m.get("causes") or []) if m.get("tampered") else "ok"
    ref = f"shifted {m.get('shifted', 0)}" if m.get("has_reference") else "no reference"
    return (f"seq {m['seq']} {flag} mean {m.get('mean', 0.0):.1f} p5 {m.get('p5', 0)} p95 {m.get('p95', 0)} "
            f"sharpness {m.get('sharpness', 0.0):.1f} {ref}")


def cmd_tamper(a):
    """REST client of ``/api/v1/process/{name}/tamper``: one line per new evaluated frame;
    ``--set-reference`` first declares the camera's newest frame normal."""
    import json
    import urllib.error
    import urllib.parse
    import urllib.request

    base = f"http://{a.rest}/api/v1/process/{urllib.parse.quote(a.device, safe='')}/tamper"
    seq, idle, ref_set = 0, 0, not a.set_reference
    while True:
        try:
            if not ref_set:
                req = urllib.request.Request(f"{base}/reference", method="PUT")
                with urllib.request.urlopen(req, timeout=10):
                    ref_set = True
                    print("reference set", flush=True)
            with urllib.request.urlopen(f"{base}?after={seq}", timeout=10) as r:
                m = json.loads(r.read())
        except urllib.error.HTTPError as e:
            if e.code != 404 or b"not found" in e.read():
                raise SystemExit(f"tamper: HTTP {e.code} for {a.device!r}")
            m = None  # no (newer) frame yet
        if m is not None:
            seq, idle = int(m["seq"]), 0
            print(format_tamper(m), flush=True)
            if not a.watch:
                return
        else:
            idle += 1
            if not a.watch and idle * a.interval > 10.0:
                raise SystemExit(f"tamper: no frame of {a.device!r} within 10 s")
        time.sleep(a.interval)


def format_privacy(r: dict) -> str:
    """What ``vep privacy`` prints: one line per mask, then the outputs the masks do not cover."""
    lines = []
    for k, m in enumerate(r.get("masks") or []):
        how = f"pixelate block {m['block']}" if m["mode"] == "pixelate" else f"fill bgr ({m['b']},{m['g']},{m['r']})"
        lines.append(f"mask {k}: x {m['x0']}..{m['x1']} y {m['y0']}..{m['y1']} (1/10000) {how}")
    if not lines:
        lines.append("no masks")
    un = r.get("unmasked_outputs") or []
    lines.append("unmasked outputs: " + (", ".join(un) if un else "none"))
    return "\n".join(lines)


def cmd_privacy(a):
    """REST client of ``/api/v1/process/{name}/privacy``: ``--set`` replaces the camera's list with
    a JSON list of masks, ``--clear`` removes it; the list in force is printed afterwards."""
    import json
    import urllib.error
    import urllib.parse
    import urllib.request

    if a.set is not None and a.clear:
        raise SystemExit("privacy: --set and --clear exclude each other")
    url = f"http://{a.rest}/api/v1/process/{urllib.parse.quote(a.device, safe='')}/privacy"
    try:
        if a.set is not None:
            try:
                masks = json.loads(a.set)
            except ValueError as e:
                raise SystemExit(f"privacy: --set is not JSON: {e}")
            req = urllib.request.Request(url, data=json.dumps(masks).encode(), method="PUT",
                                         headers={"Content-Type": "application/json"})
            urllib.request.urlopen(req, timeout=10).close()
        elif a.clear:
            urllib.request.urlopen(urllib.request.Request(url, method="DELETE"), timeout=10).close()
        with urllib.request.urlopen(url, timeout=10) as r:
            print(format_privacy(json.loads(r.read())), flush=True)
    except urllib.error.HTTPError as e:
        detail = ""
        try:
            detail = ": " + json.loads(e.read()).get("message", "")
        except ValueError:
            pass
        raise SystemExit(f"privacy: HTTP {e.code} for {a.device!r}{detail}")


def crop_url(a) -> str:
    """The crop.jpg request of ``vep crop``'s arguments (SystemExit on a malformed --box / --size)."""
    import re
    import urllib.parse

    m = re.fullmatch(r"(\d+),(\d+),(\d+),(\d+)", a.box.replace(" ", ""))
    if not m:
        raise SystemExit("crop: --box is x0,y0,x1,y1 in 1/10000 of the picture")
    sz = re.fullmatch(r"(\d{1,5})[xX](\d{1,5})", a.size.strip())
    if not sz:
        raise SystemExit("crop: --size is WxH")
    q = {"box": ",".join(m.groups()), "width": sz.group(1), "height": sz.group(2), "fit": a.fit}
    if a.seq:
        q["seq"] = str(a.seq)
    if a.quality is not None:
        q["quality"] = str(a.quality)
    return (f"http://{a.rest}/api/v1/process/{urllib.parse.quote(a.device, safe='')}/crop.jpg?"
            + urllib.parse.urlencode(q, safe=","))


def cmd_crop(a):
    """REST client of ``/api/v1/process/{name}/crop.jpg``: one box of the camera's newest frame (or
    of frame ``--seq``), cut and resized on the hub's GPU, written to ``--out``."""
    import json
    import urllib.error
    import urllib.request

    try:
        with urllib.request.urlopen(crop_url(a), timeout=10) as r:
            jpg, seq = r.read(), r.headers.get("X-Vep-Seq")
    except urllib.error.HTTPError as e:
        detail = ""
        try:
            detail = ": " + json.loads(e.read()).get("message", "")
        except ValueError:
            pass
        raise SystemExit(f"crop: HTTP {e.code} for {a.device!r}{detail}")
    with open(a.out, "wb") as f:
        f.write(jpg)
    print(f"seq {seq}: {len(jpg)} bytes -> {a.out}", flush=True)


def cmd_bench(a, rest):
    """``vep bench ...`` = the repo's bench.py (headline benchmark) with the same flags."""
    import subprocess

    bench = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")
    if not os.path.exists(bench):
        raise SystemExit("bench.py not found next to the package")
    raise SystemExit(subprocess.call([sys.executable, bench, *rest]))


def build_parser():
    ap = argparse.ArgumentParser(prog="vep", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)

    s = sub.add_parser("serve")
    s.add_argument("--config", default=None)
    s.add_argument("--data-dir", default=os.environ.get("VEP_DATA_DIR", "/data/chrysalis"))
    s.add_argument("--bind", default="0.0.0.0")
    s.add_argument("--port", type=int, default=None)
    s.add_argument("--grpc-port", type=int, default=None)
    s.add_argument("--devices", default="", help="comma-separated GPU ids; -1 = CPU backend")
    s.add_argument("--log-level", default="info")
    s.add_argument("--isolate", action="store_true",
                   help="one supervised worker process per GPU (gpu.isolation: process): a native "
                        "fault restarts that GPU's process, the other cameras keep running")
    s.set_defaults(fn=cmd_serve)

    c = sub.add_parser("camera")
    c.add_argument("--rtsp", required=True)
    c.add_argument("--rtmp", default=None)
    c.add_argument("--device_id", required=True)
    c.add_argument("--memory_buffer", type=int, default=1)
    c.add_argument("--disk_path", default=None)
    c.add_argument("--data-dir", default="/tmp/vep-camera")
    c.add_argument("--bind", default="0.0.0.0")
    c.add_argument("--port", type=int, default=8080)
    c.add_argument("--grpc-port", type=int, default=50001)
    c.add_argument("--log-level", default="info")
    c.set_defaults(fn=cmd_camera)

    f = sub.add_parser("farm")
    f.add_argument("--cams", type=int, default=4)
    f.add_argument("--width", type=int, default=640)
    f.add_argument("--height", type=int, default=480)
    f.add_argument("--fps", type=int, default=30)
    f.add_argument("--gop", type=int, default=30)
    f.add_argument("--motion", type=float, default=0.05)
    f.add_argument("--codec", choices=["h264", "h265"], default="h264")
    f.add_argument("--bind", default="127.0.0.1")
    f.add_argument("--port", type=int, default=8554)
    f.add_argument("--unpaced", action="store_true")
    f.add_argument("--cached-frames", type=int, default=60)
    f.set_defaults(fn=cmd_farm)

    for name, fn in (("list", cmd_list), ("frame", cmd_frame), ("annotate", cmd_annotate),
                     ("storage", cmd_storage), ("proxy", cmd_proxy)):
        p = sub.add_parser(name)
        p.add_argument("--host", default="127.0.0.1")
        p.add_argument("--grpc-port", type=int, default=50001)
        if name != "list":
            p.add_argument("--device", required=True)
        if name == "frame":
            p.add_argument("--keyframe", action="store_true")
            p.add_argument("--count", type=int, default=1)
            p.add_argument("--out", default=None, help="write the last frame: .jpg / .jpeg as a JPEG, else PPM")
            p.add_argument("--width", type=int, default=None, help="scale the written frame down to fit this width")
            p.add_argument("--height", type=int, default=None, help="... and / or this height (aspect kept)")
            p.add_argument("--overlay", action="store_true",
                           help="draw the camera's stored overlay list (the JPEG then comes from the hub's REST API)")
            p.add_argument("--stamp", action="store_true", help="draw the camera's name and the frame's time, likewise")
            p.add_argument("--rest", default="127.0.0.1:8080", help="host:port of the hub's REST API (--overlay / --stamp)")
        if name == "annotate":
            p.add_argument("--type", required=True)
        if name in ("storage", "proxy"):
            p.add_argument("--on", required=True)
        p.set_defaults(fn=fn)

    m = sub.add_parser("motion", help="did anything change: the hub's motion detection of one camera (REST)")
    m.add_argument("--device", required=True)
    m.add_argument("--rest", default="127.0.0.1:8080", help="host:port of the hub's REST API")
    m.add_argument("--watch", action="store_true", help="keep printing, one line per new evaluated frame")
    m.add_argument("--interval", type=float, default=0.1, help="seconds between polls")
    m.set_defaults(fn=cmd_motion)

    t = sub.add_parser("tamper", help="does the camera still show what it should: the hub's tamper detection (REST)")
    t.add_argument("--device", required=True)
    t.add_argument("--rest", default="127.0.0.1:8080", help="host:port of the hub's REST API")
    t.add_argument("--watch", action="store_true", help="keep printing, one line per new evaluated frame")
    t.add_argument("--set-reference", action="store_true", help="first declare the camera's newest frame normal")
    t.add_argument("--interval", type=float, default=0.1, help="seconds between polls")
    t.set_defaults(fn=cmd_tamper)

    pv = sub.add_parser("privacy", help="show, set or clear a camera's privacy masks (REST)")
    pv.add_argument("--device", required=True)
    pv.add_argument("--rest", default="127.0.0.1:8080", help="host:port of the hub's REST API")
    pv.add_argument("--set", default=None, metavar="JSON",
                    help='a JSON list of masks, e.g. \'[{"x0":0,"y0":0,"x1":2500,"y1":10000,"mode":"pixelate","block":16}]\'')
    pv.add_argument("--clear", action="store_true", help="remove the camera's masks")
    pv.set_defaults(fn=cmd_privacy)

    ov = sub.add_parser("overlay", help="show, set or clear a camera's stored on-screen display list (REST)")
    ov.add_argument("--device", required=True)
    ov.add_argument("--rest", default="127.0.0.1:8080", help="host:port of the hub's REST API")
    ov.add_argument("--set", default=None, metavar="JSON",
                    help='a JSON list of items, e.g. \'[{"x0":1000,"y0":1000,"x1":5000,"y1":8000,"label":"person 87%%"}]\'')
    ov.add_argument("--ttl-ms", type=int, default=0, help="with --set: drop the items after this many milliseconds")
    ov.add_argument("--clear", action="store_true", help="remove the camera's list")
    ov.set_defaults(fn=cmd_overlay)

    cr = sub.add_parser("crop", help="one box of a camera's frame as a JPEG, cut and resized on the GPU (REST)")
    cr.add_argument("--device", required=True)
    cr.add_argument("--rest", default="127.0.0.1:8080", help="host:port of the hub's REST API")
    cr.add_argument("--box", required=True, help="x0,y0,x1,y1 in 1/10000 of the picture")
    cr.add_argument("--size", required=True, help="WxH of the JPEG (each 1..4096)")
    cr.add_argument("--seq", type=int, default=0, help="that very frame (needs buffer.in_memory); default: the newest")
    cr.add_argument("--fit", default="stretch", choices=["stretch", "letterbox"])
    cr.add_argument("--quality", type=int, default=None)
    cr.add_argument("--out", required=True, help="file to write")
    cr.set_defaults(fn=cmd_crop)

    b = sub.add_parser("bench", help="run bench.py (flags passed through, e.g. --codec h265)")
    b.set_defaults(fn=None)
    return ap


def main(argv=None):
    ap = build_parser()
    a, rest = ap.parse_known_args(argv)
    if a.cmd == "bench":
        cmd_bench(a, rest)
    if rest:
        ap.error(f"unrecognized arguments: {' '.join(rest)}")
    a.fn(a)


if __name__ == "__main__":
    main(sys.argv[1:])
