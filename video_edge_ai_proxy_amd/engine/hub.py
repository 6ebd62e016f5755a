"""Hub: the node-level data-plane owner (one native Worker per local GPU, camera placement,
ingest sessions, archiver, latest-frame access).

Reference parity: replaces the per-camera Docker container + Redis pair
(services/rtsp_process_manager.go:50-150 starts a container per camera; python/ workers publish
frames to Redis). Here every camera is a native IngestSession thread feeding a Camera on the GPU
Worker chosen by the placement policy (camera data parallelism inside one process; across
processes/nodes see ``video_edge_ai_proxy_amd.parallel``).
"""
from __future__ import annotations

import hashlib
import logging
import os
import threading
import time
from dataclasses import dataclass, field
from typing import Optional

from .. import crops, privacy
from .. import overlay as osd
from .._native import gpu_count, native
from ..config import Config, parse_tile
from ..utils import now_ms

log = logging.getLogger("vep.hub")

_CHW = {"none": 0, "fp16": 1, "bf16": 2, "fp32": 3}


def new_bus_tag() -> str:
    """A frame-bus tag unique to one hub instance on this node (pid + random suffix)."""
    import secrets

    return f"n{os.getpid()}{secrets.token_hex(3)}"


class CameraNotFound(KeyError):
    pass


class CameraExists(ValueError):
    pass


@dataclass
class CameraHandle:
    name: str
    worker_index: int
    cam: int
    rtsp: str
    rtmp: str = ""
    session: Optional[object] = None
    created_ms: int = field(default_factory=now_ms)


def place_camera(name: str, loads: list[int], policy: str = "least_loaded") -> int:
    """Camera -> worker index. ``hash`` is stable across restarts; ``least_loaded`` balances."""
    if not loads:
        raise RuntimeError("no workers")
    if policy == "hash":
        h = int(hashlib.md5(name.encode()).hexdigest(), 16)
        return h % len(loads)
    return min(range(len(loads)), key=lambda i: (loads[i], i))


class Hub:
    def __init__(self, cfg: Config, devices: Optional[list[int]] = None, bus_owner: int = 0,
                 host_domains: Optional[list[dict]] = None):
        self.cfg = cfg
        if devices is None:
            devices = list(cfg.gpu.devices) if cfg.gpu.devices else list(range(gpu_count()))
        if not devices:
            devices = [-1]  # CPU backend (no GPU visible)
        self.devices = devices
        g = cfg.gpu
        # per-GPU host data plane (hostplan.h): each worker's ingest sockets, parse strands and
        # GPU feeder threads run on its own CPU set (the GPU's NUMA-local CPUs, split among the
        # workers sharing them), sized from the process's CPU budget / workers
        if host_domains is None:
            host_domains = native.plan_host_domains(list(devices), [str(c) for c in (g.host_cpus or [])])
        self.host_domains = host_domains
        self._crop_lock = threading.Lock()
        self._crop_counts = [0, 0]  # requests, boxes (Hub.crop_counts, /metrics)
        # on-screen display: the stored list of every camera, [(item, deadline | None), ...] with
        # the deadline on overlay_clock (monotonic seconds); kept here, not persisted
        self._overlay_lock = threading.Lock()
        self._overlays: dict[str, list] = {}
        self.overlay_clock = time.monotonic
        self.workers = []
        for d, dom in zip(devices, host_domains):
            w = native.Worker(device=d, letterbox_size=int(g.letterbox_size),
                              chw_dtype=_CHW.get(g.letterbox_dtype, 0), mean=list(g.mean),
                              std=list(g.std), max_cameras=int(g.max_cameras_per_gpu),
                              letterbox_format=1 if g.letterbox_format == "nv12" else 0,
                              decoder=str(getattr(g, "decoder", "native")), host_domain=dom)
            w.wall_max_tiles = int(cfg.serving.wall_max_tiles)
            m = cfg.motion
            w.set_motion_params(int(m.cell), int(m.threshold), int(m.learn_shift), int(m.cell_percent),
                                int(m.min_cells))
            t = cfg.tamper
            w.set_tamper_params(int(t.cell), int(t.dark_level), int(t.bright_level), int(t.spread_min),
                                int(t.focus_percent), int(t.shift_level), int(t.shift_percent))
            w.start()
            self.workers.append(w)
        # Consumer batch: with letterbox_size > 0 every worker letterboxes each frame it publishes
        # into row <camera slot> of a torch-owned tensor on its own GPU; consumer_batch() assembles
        # the node-wide batch from them.
        self.consumer: list = []
        if int(g.letterbox_size) > 0:
            import torch

            S = int(g.letterbox_size)
            shape = (S * S * 3 // 2,) if g.letterbox_format == "nv12" else (S, S, 3)
            for w, d in zip(self.workers, devices):
                dev = torch.device("cuda", d) if d >= 0 else torch.device("cpu")
                t = torch.zeros((int(g.max_cameras_per_gpu), *shape), dtype=torch.uint8, device=dev)
                w.set_consumer_buffers(t.data_ptr(), 0, int(g.max_cameras_per_gpu))
                self.consumer.append(t)
        self._snaps: list = [None] * len(self.consumer)
        self._cons_lock = threading.Lock()  # one consumer batch at a time (shared snapshot tensors)
        # Frame bus (cfg.bus_tag set: serving processes read frames from shared memory): one owner
        # per worker, index bus_owner + k; the pump DMAs a camera's newest frame on demand.
        self.bus = []
        if cfg.bus_tag:
            for k, w in enumerate(self.workers):
                o = native.BusOwner(cfg.bus_tag, bus_owner + k, int(g.max_cameras_per_gpu))
                o.attach(w)
                self.bus.append(o)
        self.archiver = native.Archiver()
        self.cameras: dict[str, CameraHandle] = {}
        self._lock = threading.RLock()
        log.info("hub up: devices=%s", devices)

    # ------------------------------------------------------------------ lifecycle
    def _loads(self) -> list[int]:
        loads = [0] * len(self.workers)
        for h in self.cameras.values():
            loads[h.worker_index] += 1
        return loads

    def archive_dir(self) -> str:
        if not self.cfg.buffer.on_disk:
            return ""
        return self.cfg.buffer.on_disk_folder or os.path.join(self.cfg.data_dir, "archive")

    def start_camera(self, name: str, rtsp: str, rtmp: str = "", disk_path: Optional[str] = None,
                     timeout_ms: int = 5000, reconnect_delay_ms: int = 1000, masks=None) -> CameraHandle:
        """``masks``: the camera's privacy masks (:mod:`..privacy`), in force before the session
        starts, so the first frame is already masked."""
        native_masks = privacy.to_native(masks)  # (ValueError before anything is created)
        with self._lock:
            if name in self.cameras:
                raise CameraExists(f"camera {name!r} already running")
            wi = place_camera(name, self._loads(), self.cfg.gpu.placement)
            w = self.workers[wi]
            cam = w.add_camera(name, self.cfg.ring_slots, self.cfg.history_depth)
            w.set_idle_cutoff_ms(cam, int(self.cfg.gpu.idle_cutoff_ms))
            if native_masks:
                w.set_privacy_masks(cam, native_masks)
            h = CameraHandle(name, wi, cam, rtsp, rtmp)
            disk = self.archive_dir() if disk_path is None else disk_path
            h.session = native.IngestSession(w, cam, name, rtsp, rtmp or "", disk or "",
                                             self.archiver, timeout_ms, reconnect_delay_ms, 30000)
            h.session.start()
            self.cameras[name] = h
            if self.bus:
                self.bus[wi].add(cam, name)
            log.info("camera %s -> worker %d (device %s) slot %d", name, wi, self.devices[wi], cam)
            return h

    def stop_camera(self, name: str) -> None:
        with self._lock:
            h = self.cameras.pop(name, None)
        if h is None:
            raise CameraNotFound(name)
        with self._overlay_lock:
            self._overlays.pop(name, None)
        if self.bus:
            self.bus[h.worker_index].remove(h.cam)
        h.session.stop()
        self.workers[h.worker_index].remove_camera(h.cam)

    def has(self, name: str) -> bool:
        return name in self.cameras

    def handle(self, name: str) -> CameraHandle:
        h = self.cameras.get(name)
        if h is None:
            raise CameraNotFound(name)
        return h

    def worker_of(self, name: str):
        h = self.handle(name)
        return self.workers[h.worker_index], h.cam

    def consumer_batch(self, device=None, names: Optional[list[str]] = None):
        """Node-wide letterboxed batch of the newest frame of every running camera (or of
        ``names``, in that order): ``(tensor [N, S, S, 3] uint8 (or NV12 rows), names)`` on
        ``device`` (default: the first worker's device). Each GPU's rows are gathered from its own
        consumer tensor and the per-GPU slices are concatenated on the destination with peer
        copies over xGMI (one process, many GPUs; the multi-process form is
        ``parallel.ConsumerBatch``, one RCCL all-gather). Rows of cameras that have not published
        a frame yet are zero."""
        from ..parallel import gather_to_device

        if not self.consumer:
            raise RuntimeError("consumer batch disabled (gpu.letterbox_size is 0)")
        with self._lock:
            order = list(names) if names is not None else sorted(self.cameras)
            hs = [self.handle(n) for n in order]
        if device is None:
            device = self.consumer[0].device
        with self._cons_lock:
            return self._consumer_batch(hs, order, device, gather_to_device)

    def _consumer_batch(self, hs, order, device, gather_to_device):
        import torch

        parts, where = [], []
        for wi, t in enumerate(self.consumer):
            mine = [(k, h.cam) for k, h in enumerate(hs) if h.worker_index == wi]
            if not mine:
                continue
            # a consistent snapshot of the rows in use (the lanes keep letterboxing into the
            # live rows; reading them directly could catch a row mid-rewrite), on the current
            # stream: the row selection below is ordered after it without a host wait
            snap = self.snapshot(wi, max(c for _, c in mine) + 1)
            idx = torch.tensor([c for _, c in mine], dtype=torch.long, device=t.device)
            parts.append(snap.index_select(0, idx))
            where += [k for k, _ in mine]
        if not parts:
            return torch.zeros((0, *self.consumer[0].shape[1:]), dtype=torch.uint8, device=device), []
        cat = gather_to_device(parts, torch.device(device))
        inv = torch.empty(len(where), dtype=torch.long)
        inv[torch.tensor(where, dtype=torch.long)] = torch.arange(len(where))
        return cat.index_select(0, inv.to(cat.device)), order

    def snapshot(self, wi: int, rows: int):
        """Consistent copy of worker wi's consumer rows [0, rows) (Worker.snapshot_consumer) into
        a per-worker snapshot tensor, enqueued on the device's current stream."""
        import torch

        t = self.consumer[wi]
        if self._snaps[wi] is None:
            self._snaps[wi] = torch.empty_like(t)
        snap = self._snaps[wi]
        stream = torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else 0
        n = snap[:rows].numel()
        self.workers[wi].snapshot_consumer(snap.data_ptr(), n, rows, stream)
        return snap[:rows]

    def shutdown(self) -> None:
        for name in list(self.cameras):
            try:
                self.stop_camera(name)
            except CameraNotFound:
                pass
        for o in self.bus:
            o.stop()
        self.bus = []  # (unlinks the segments now, not at garbage collection)
        for w in self.workers:
            w.stop()
        self.archiver.flush()

    # ------------------------------------------------------------------ state
    def host_plane(self) -> list[dict]:
        """Each worker's host domain: device, NUMA node, CPU list, parse / io threads planned and
        the parse strands its live ingest services run (0 until its first camera)."""
        out = []
        loads = self._loads()
        for i, w in enumerate(self.workers):
            d = dict(w.host_domain)
            d.pop("cpus", None)  # (cpulist says it compactly)
            d["ingest_parse_threads"] = w.ingest_parse_threads
            d["cameras"] = loads[i]
            d["pid"] = os.getpid()
            out.append(d)
        return out

    def state(self, name: str) -> dict:
        h = self.handle(name)
        w = self.workers[h.worker_index]
        st = h.session.state()
        st.update(w.stats(h.cam))
        st["device"] = self.devices[h.worker_index]
        return st

    def logs(self, name: str, last: int = 100) -> tuple[str, str]:
        w, cam = self.worker_of(name)
        return w.logs(cam, False, last), w.logs(cam, True, last)

    # ------------------------------------------------------------------ control
    def touch(self, name: str, keyframe_only: Optional[bool] = None) -> None:
        """A client asked for a frame: refresh last_query (and keyframe-only mode)."""
        w, cam = self.worker_of(name)
        if keyframe_only is not None:
            w.set_keyframe_only(cam, bool(keyframe_only))
        w.set_last_query(cam, now_ms())

    def set_proxy(self, name: str, on: bool) -> None:
        w, cam = self.worker_of(name)
        w.set_proxy(cam, bool(on))
        w.set_last_query(cam, now_ms())

    def proxy(self, name: str) -> bool:
        w, cam = self.worker_of(name)
        return bool(w.proxy(cam))

    # ------------------------------------------------------------------ frames
    def latest_frame_bytes(self, name: str, after: int = 0, wait_ms: int = 0):
        """(seq, serialized VideoFrame, meta) of the newest frame with seq > after, or None."""
        w, cam = self.worker_of(name)
        pub = w.published(cam)
        if pub < after:
            # the caller's cursor belongs to an older ring of this camera (a restarted worker
            # process or a resolution change starts a new ring at 0): start over
            after = 0
        if wait_ms > 0 and pub <= after:
            w.wait_frame(cam, after, wait_ms)
        return w.video_frame(cam, after, name)

    def latest_frame(self, name: str, after: int = 0):
        w, cam = self.worker_of(name)
        return w.read_latest(cam, after)

    def _quality(self, quality: Optional[int]) -> int:
        q = int(self.cfg.serving.jpeg_quality if quality is None else quality)
        if not 1 <= q <= 100:
            raise ValueError("quality must be 1..100")
        return q

    @staticmethod
    def _box(width: Optional[int], height: Optional[int]) -> tuple[int, int]:
        """A requested size as the native layer takes it (0 = that side not given)."""
        out = []
        for v, what in ((width, "width"), (height, "height")):
            if v is None:
                out.append(0)
                continue
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 65535:
                raise ValueError(f"{what} must be an integer 1..65535")
            out.append(v)
        return out[0], out[1]

    def latest_jpeg(self, name: str, after: int = 0, quality: Optional[int] = None,
                    width: Optional[int] = None, height: Optional[int] = None, overlay=None, stamp: bool = False):
        """``(meta, bytes)`` of the newest frame with seq > after as a baseline JPEG, or None.
        Encoded on the camera's GPU straight from its ring slot (CPU backend: on the host);
        ``quality`` 1..100, default ``serving.jpeg_quality``. With ``width`` and / or ``height``
        the frame is first fitted into that box (aspect kept, never enlarged) and downscaled by
        area averaging, on the GPU as well; ``meta`` then carries the scaled size.

        ``overlay``: ``True`` draws the camera's stored list (:meth:`set_overlay`), a list its
        items (:mod:`..overlay`, docs/OVERLAY.md); ``stamp`` appends the camera's name and the
        frame's time. They are drawn on a copy (scaled: on the scaled picture) in one kernel launch
        on the camera's GPU; the ring slot is never written. With neither, the call and its bytes
        are what they are without them."""
        q = self._quality(quality)
        bw, bh = self._box(width, height)
        if not isinstance(stamp, bool):
            raise ValueError("stamp must be true or false")
        w, cam = self.worker_of(name)
        if (overlay is None or overlay is False) and not stamp:
            if not (bw or bh):
                return w.read_latest_jpeg(cam, after, q)
            return w.read_latest_jpeg(cam, after, q, bw, bh)
        if overlay is None or overlay is False:
            items = []  # (the stamp alone)
        elif overlay is True:
            items = self.overlay(name)
        else:
            items = osd.normalize_list(overlay)
        if stamp:
            items = items + [osd.STAMP]
        return w.read_overlay_jpeg(cam, osd.to_native(items), name, after, q, bw, bh)

    # ------------------------------------------------------------------ on-screen display
    def set_overlay(self, name: str, items, ttl_ms: int = 0) -> None:
        """Replaces the camera's stored overlay list (``latest_jpeg(overlay=True)`` draws it).
        ``ttl_ms`` > 0: the items are dropped that many milliseconds from now. A bad list is a
        ``ValueError`` and changes nothing."""
        norm = osd.normalize_list(items)
        native.overlay_check(osd.to_native(norm))
        deadline = self._overlay_deadline(ttl_ms)
        self.handle(name)
        with self._overlay_lock:
            self._overlays[name] = [(it, deadline) for it in norm]

    def add_overlay_item(self, name: str, item, ttl_ms: int = 0) -> None:
        """Appends one item to the camera's stored list; when the list is full its oldest item
        makes room."""
        it = osd.normalize(item)
        native.overlay_check(osd.to_native([it]))
        deadline = self._overlay_deadline(ttl_ms)
        self.handle(name)
        now = self.overlay_clock()
        with self._overlay_lock:
            live = [e for e in self._overlays.get(name, []) if e[1] is None or e[1] > now]
            live.append((it, deadline))
            self._overlays[name] = live[-osd.MAX_ITEMS:]

    def _overlay_deadline(self, ttl_ms):
        if isinstance(ttl_ms, bool) or not isinstance(ttl_ms, int) or ttl_ms < 0:
            raise ValueError("ttl_ms must be an integer >= 0")
        return None if ttl_ms == 0 else self.overlay_clock() + ttl_ms / 1000.0

    def overlay(self, name: str) -> list:
        """The camera's stored list; items past their ``ttl_ms`` are dropped on this read."""
        self.handle(name)
        now = self.overlay_clock()
        with self._overlay_lock:
            live = [e for e in self._overlays.get(name, []) if e[1] is None or e[1] > now]
            if live:
                self._overlays[name] = live
            else:
                self._overlays.pop(name, None)
            return [osd.public(it) for it, _ in live]

    def clear_overlay(self, name: str) -> None:
        self.handle(name)
        with self._overlay_lock:
            self._overlays.pop(name, None)

    def overlay_counts(self) -> tuple:
        """``(requests, primitives)`` drawn since the hub started (/metrics)."""
        r = p = 0
        for w in self.workers:
            a, b = w.overlay_counts()
            r, p = r + int(a), p + int(b)
        return r, p

    def latest_scaled(self, name: str, after: int = 0, width: Optional[int] = None,
                      height: Optional[int] = None):
        """``(meta, ndarray)`` of the newest frame with seq > after, fitted into ``width x height``
        and downscaled on the camera's GPU; only the small picture is copied to the host."""
        bw, bh = self._box(width, height)
        if not (bw or bh):
            raise ValueError("width or height required")
        w, cam = self.worker_of(name)
        return w.read_latest_scaled(cam, after, bw, bh)

    def wall_tile(self) -> tuple[int, int]:
        tw, th = parse_tile(self.cfg.serving.wall_tile)
        return tw, th

    def wall_layout(self, names=None, cols: Optional[int] = None, tile_width: Optional[int] = None,
                    tile_height: Optional[int] = None):
        """``(names, cols, rows, tile_width, tile_height)`` a wall of these arguments has."""
        with self._lock:
            order = sorted(self.cameras) if names is None else list(names)
            for n in order:
                self.handle(n)
        dw, dh = self.wall_tile()
        tw, th = self._box(dw if tile_width is None else tile_width, dh if tile_height is None else tile_height)
        if cols is not None and (isinstance(cols, bool) or not isinstance(cols, int) or not 1 <= cols <= 65535):
            raise ValueError("cols must be an integer 1..65535")
        if not order:
            raise ValueError("no camera to show")
        if len(order) > int(self.cfg.serving.wall_max_tiles):
            raise ValueError(f"a wall shows at most serving.wall_max_tiles = {self.cfg.serving.wall_max_tiles} cameras")
        gc, gr, cw, ch = native.wall_geometry(len(order), cols or 0, tw, th)
        if cw > 65535 or ch > 65535:
            raise ValueError(f"canvas {cw}x{ch} larger than 65535")
        return order, gc, gr, tw, th

    def wall_jpeg(self, names=None, cols: Optional[int] = None, tile_width: Optional[int] = None,
                  tile_height: Optional[int] = None, quality: Optional[int] = None, labels: bool = False):
        """``({name: seq}, bytes)``: one JPEG showing the newest frame of every listed camera
        (default: the running cameras, sorted), tile ``t`` fitted into cell ``(t % cols, t // cols)``
        of ``tile_width x tile_height`` (default ``serving.wall_tile``) and centred, ``cols``
        defaulting to ``ceil(sqrt(n))``. A camera without a frame shows as background, seq 0.

        Rendered by the worker that owns most of the listed cameras (ties: the lowest index): its
        cameras are scaled from their ring slots in one kernel launch; cameras of other workers are
        scaled on their own GPU and only the small tiles travel. A wall refreshes ``last_query``
        of every camera it shows, so it keeps their lazy decoders awake.

        ``labels``: every tile that shows a frame gets its camera's name at its top-left corner, in
        one more kernel launch on the composed canvas (docs/OVERLAY.md). A wall whose labels expand
        to more than 256 primitives (more than 128 tiles) is refused (``overlay.Refused``, a
        ``ValueError``)."""
        q = self._quality(quality)
        if not isinstance(labels, bool):
            raise ValueError("labels must be true or false")
        order, gc, gr, tw, th = self.wall_layout(names, cols, tile_width, tile_height)
        if labels and 2 * len(order) > osd.MAX_PRIMS:
            raise osd.Refused(f"the labels of {len(order)} tiles expand to more than {osd.MAX_PRIMS} primitives")
        hs = []
        for n in order:
            h = self.cameras.get(n)
            if h is None:
                raise CameraNotFound(n)
            hs.append(h)
        now = now_ms()
        for h in hs:
            self.workers[h.worker_index].set_last_query(h.cam, now)
        count = [0] * len(self.workers)
        for h in hs:
            count[h.worker_index] += 1
        home = max(range(len(count)), key=lambda i: (count[i], -i))
        cams, foreign, any_foreign = [], [], False
        for h in hs:
            if h.worker_index == home:
                cams.append(h.cam)
                foreign.append(None)
                continue
            cams.append(-1)
            r = self.workers[h.worker_index].read_latest_scaled(h.cam, 0, tw, th)
            foreign.append(None if r is None else (int(r[0]["seq"]), r[1]))
            any_foreign = any_foreign or r is not None
        if labels:
            seqs, jpg = self.workers[home].read_wall_jpeg(cams, gc, tw, th, q, foreign if any_foreign else None,
                                                          list(order))
        else:
            seqs, jpg = self.workers[home].read_wall_jpeg(cams, gc, tw, th, q, foreign if any_foreign else None)
        return {n: int(s) for n, s in zip(order, seqs)}, jpg

    # ------------------------------------------------------------------ motion
    @staticmethod
    def _motion_dict(r, grid: bool) -> Optional[dict]:
        """A worker's motion answer as the hub serves it."""
        if r is None:
            return None
        box = r["box"]
        out = {"seq": int(r["seq"]), "width": int(r["width"]), "height": int(r["height"]), "cell": int(r["cell"]),
               "cols": int(r["cols"]), "rows": int(r["rows"]), "threshold": int(r["threshold"]),
               "primed": bool(r["primed"]), "changed": int(r["changed"]), "active": int(r["active"]),
               "score": int(r["changed"]) / float(int(r["width"]) * int(r["height"])),
               "box": None if box is None else [int(v) for v in box], "motion": bool(r["motion"])}
        if grid:
            out["counts"] = [[int(v) for v in row] for row in r["counts"]]
        return out

    def motion(self, name: str, after: int = 0, grid: bool = False) -> Optional[dict]:
        """Did the camera's newest frame with seq > after differ from its background model?
        ``None`` when there is no such frame, else a dict of ``seq, width, height, cell, cols,
        rows, threshold, primed, changed, active, score, box, motion`` (docs/MOTION.md), with
        ``grid`` also ``counts``, the changed pixels of every cell. The frame is evaluated on the
        camera's GPU, in its ring slot, once however many clients ask. Refreshes ``last_query``,
        so asking keeps the camera's lazy decoder awake."""
        w, cam = self.worker_of(name)
        w.set_last_query(cam, now_ms())
        return self._motion_dict(w.read_motion(cam, int(after)), grid)

    def motion_many(self, names=None, grid: bool = False) -> dict:
        """``{name: dict | None}`` for the newest frame of every listed camera (default: the
        running cameras, sorted): one kernel launch per worker covers all of its cameras that
        need an evaluation. ``None``: the camera has no frame yet."""
        with self._lock:
            order = sorted(self.cameras) if names is None else list(names)
            hs = [self.handle(n) for n in order]
        now = now_ms()
        for h in hs:
            self.workers[h.worker_index].set_last_query(h.cam, now)
        out = {}
        for wi, w in enumerate(self.workers):
            mine = [h for h in hs if h.worker_index == wi]
            if not mine:
                continue
            for h, r in zip(mine, w.read_motion_many([h.cam for h in mine])):
                out[h.name] = self._motion_dict(r, grid)
        return {n: out[n] for n in order}

    def motion_reset(self, name: str) -> None:
        """Forget the camera's background model: its next evaluation primes again."""
        w, cam = self.worker_of(name)
        w.motion_reset(cam)

    # ------------------------------------------------------------------ tamper
    @staticmethod
    def _tamper_dict(r, grid: bool) -> Optional[dict]:
        """A worker's tamper answer as the hub serves it."""
        if r is None:
            return None
        out = {k: int(r[k]) for k in ("seq", "width", "height", "cell", "cols", "rows", "p5", "p95", "shifted")}
        out.update({k: float(r[k]) for k in ("mean", "sharpness")})
        out.update({k: bool(r[k]) for k in ("has_reference", "dark", "bright", "flat", "defocused", "moved",
                                            "tampered")})
        out["causes"] = [str(c) for c in r["causes"]]
        if grid:
            out["hist"] = [int(v) for v in r["hist"]]
            out["sum_y"] = [[int(v) for v in row] for row in r["sum_y"]]
            out["energy"] = [[int(v) for v in row] for row in r["energy"]]
        return out

    def tamper(self, name: str, after: int = 0, grid: bool = False, wake: bool = True) -> Optional[dict]:
        """Does the camera's newest frame with seq > after still show what it should? ``None``
        when there is no such frame, else a dict of ``seq, width, height, cell, cols, rows, mean,
        p5, p95, sharpness, has_reference, shifted, dark, bright, flat, defocused, moved, tampered,
        causes`` (docs/TAMPER.md), with ``grid`` also ``hist``, ``sum_y`` and ``energy``. The frame
        is evaluated on the camera's GPU, in its ring slot, once however many clients ask.
        ``wake`` refreshes ``last_query``, so asking keeps the camera's lazy decoder awake;
        ``wake=False`` evaluates whatever the ring holds and leaves ``last_query`` alone (an idle
        camera's frame is then as old as its last query)."""
        w, cam = self.worker_of(name)
        if wake:
            w.set_last_query(cam, now_ms())
        return self._tamper_dict(w.read_tamper(cam, int(after)), grid)

    def tamper_many(self, names=None, grid: bool = False, wake: bool = True) -> dict:
        """``{name: dict | None}`` for the newest frame of every listed camera (default: the
        running cameras, sorted): one kernel launch per worker covers all of its cameras that
        need an evaluation. ``None``: the camera has no frame yet. ``wake`` as in :meth:`tamper`."""
        with self._lock:
            order = sorted(self.cameras) if names is None else list(names)
            hs = [self.handle(n) for n in order]
        if wake:
            now = now_ms()
            for h in hs:
                self.workers[h.worker_index].set_last_query(h.cam, now)
        out = {}
        for wi, w in enumerate(self.workers):
            mine = [h for h in hs if h.worker_index == wi]
            if not mine:
                continue
            for h, r in zip(mine, w.read_tamper_many([h.cam for h in mine])):
                out[h.name] = self._tamper_dict(r, grid)
        return {n: out[n] for n in order}

    def tamper_reference(self, name: str) -> bool:
        """Declare the camera's newest frame normal: its grid becomes the reference that
        ``defocused`` and ``moved`` compare with (host memory, not kept across restarts). False
        when the camera has no frame."""
        w, cam = self.worker_of(name)
        return bool(w.tamper_set_reference(cam))

    def tamper_reset(self, name: str) -> None:
        """Drop the camera's reference and its stored answer."""
        w, cam = self.worker_of(name)
        w.tamper_reset(cam)

    # ------------------------------------------------------------------ privacy masks
    def set_privacy_masks(self, name: str, masks) -> None:
        """Replace the camera's privacy masks (:mod:`..privacy`; ``None`` or ``[]`` clears them;
        ``ValueError`` on a bad list). They are written into the ring slot on the GPU before a frame
        is published, so every consumer of the ring sees them. Fail closed: the frames published
        under the old list stop being readable at once, frames in flight are given up, and with a
        frame bus the camera's entry is taken off the bus before the change and put back after it
        (a new entry generation with empty slots), so the serving processes drop their copies."""
        native_masks = privacy.to_native(masks)
        with self._lock:
            h = self.handle(name)
            w = self.workers[h.worker_index]
            if self.bus:
                self.bus[h.worker_index].remove(h.cam)
            try:
                w.set_privacy_masks(h.cam, native_masks)
            finally:
                if self.bus:
                    self.bus[h.worker_index].add(h.cam, name)

    def privacy_masks(self, name: str) -> list:
        w, cam = self.worker_of(name)
        return privacy.from_native(w.privacy_masks(cam))

    # ------------------------------------------------------------------ crops
    def _crop_args(self, lists, width, height, after, seq, fit, pad):
        """A crop request as the native layer takes it; ``ValueError`` on a bad value or one above
        ``serving.crop_max_boxes`` / ``serving.crop_max_bytes``."""
        width, height = crops.size(width, height)
        after, seq = crops.seq_args(after, seq)
        fit, pad = crops.fit_index(fit), crops.pad_tuple(pad)
        max_boxes = int(self.cfg.serving.crop_max_boxes)
        native_lists = [crops.to_native(boxes, max_boxes) for boxes in lists]
        total = sum(len(b) for b in native_lists) * width * height * 3
        if total > int(self.cfg.serving.crop_max_bytes):
            raise ValueError(f"the request asks for {total} bytes of crops, above serving.crop_max_bytes = "
                             f"{self.cfg.serving.crop_max_bytes}")
        return native_lists, width, height, after, seq, fit, pad

    def _count_crops(self, boxes: int) -> None:
        with self._crop_lock:
            self._crop_counts[0] += 1
            self._crop_counts[1] += boxes

    def crop_counts(self) -> tuple[int, int]:
        """(crop requests served or refused for want of a frame, boxes they named) since the start."""
        with self._crop_lock:
            return self._crop_counts[0], self._crop_counts[1]

    def crops(self, name: str, boxes, width: int, height: int, after: int = 0, seq: int = 0,
              fit: str = "stretch", pad=None):
        """``(seq, ndarray [n, height, width, 3])``: the ``boxes`` (dicts ``{"x0", "y0", "x1",
        "y1"}`` in 1/10000 of the picture, :mod:`..crops`) of a frame of the camera, cut and resized
        on its GPU in one kernel launch, in its ring slot; only the crops are copied to the host.
        ``seq=0``: the newest frame with seq > ``after``; ``seq=N``: that very frame, while
        ``buffer.in_memory`` still holds it (a detector's boxes belong to the frame it saw).
        ``None`` when there is no such frame. A box is reduced by area averaging and enlarged
        bilinearly, exact in integers (docs/CROPS.md); ``fit="letterbox"`` keeps the aspect and pads
        with ``pad`` ``(b, g, r)``, default 114. Crops read the ring slot, so they show the camera's
        privacy masks. Refreshes ``last_query``, so asking keeps the camera's lazy decoder awake."""
        (native_boxes,), width, height, after, seq, fit, pad = self._crop_args([boxes], width, height, after, seq, fit,
                                                                               pad)
        w, cam = self.worker_of(name)
        w.set_last_query(cam, now_ms())
        self._count_crops(len(native_boxes))
        r = w.read_crops(cam, native_boxes, width, height, after, seq, fit, pad)
        return None if r is None else (int(r[0]["seq"]), r[1])

    def crops_many(self, boxes_by_name: dict, width: int, height: int, after: int = 0, fit: str = "stretch",
                   pad=None) -> dict:
        """``{name: (seq, ndarray) | None}`` for the newest frame with seq > ``after`` of several
        cameras, each with its own boxes: one kernel launch per worker covers all of its cameras."""
        if not isinstance(boxes_by_name, dict):
            raise ValueError("boxes_by_name must be a dict {name: boxes}")
        order = list(boxes_by_name)
        lists, width, height, after, _, fit, pad = self._crop_args([boxes_by_name[n] for n in order], width, height,
                                                                   after, 0, fit, pad)
        with self._lock:
            hs = [self.handle(n) for n in order]
        now = now_ms()
        for h in hs:
            self.workers[h.worker_index].set_last_query(h.cam, now)
        self._count_crops(sum(len(b) for b in lists))
        out = {}
        for wi, w in enumerate(self.workers):
            mine = [(h, b) for h, b in zip(hs, lists) if h.worker_index == wi]
            if not mine:
                continue
            rs = w.read_crops_many([(h.cam, after, 0, b) for h, b in mine], width, height, fit, pad)
            for (h, _), r in zip(mine, rs):
                out[h.name] = None if r is None else (int(r[0]["seq"]), r[1])
        return {n: out[n] for n in order}

    def crop_jpeg(self, name: str, box, width: int, height: int, after: int = 0, seq: int = 0,
                  quality: Optional[int] = None, fit: str = "stretch", pad=None):
        """``(seq, bytes)``: one box of a frame as a baseline JPEG of ``width x height``, the encoder
        chained onto the crop on the camera's GPU; only compressed bytes are copied. Arguments as
        :meth:`crops`; ``quality`` 1..100, default ``serving.jpeg_quality``. A digital zoom for any
        viewer."""
        q = self._quality(quality)
        (native_boxes,), width, height, after, seq, fit, pad = self._crop_args([[box]], width, height, after, seq, fit,
                                                                               pad)
        w, cam = self.worker_of(name)
        w.set_last_query(cam, now_ms())
        self._count_crops(1)
        r = w.read_crop_jpeg(cam, native_boxes[0], width, height, after, seq, q, fit, pad)
        return None if r is None else (int(r[0]["seq"]), r[1])

    def history(self, name: str, after: int = 0, count: int = 0) -> list:
        """``[(meta, ndarray)]`` of the camera's newest ``count`` (0 = ``buffer.in_memory``) frames
        with seq > after, ascending and contiguous in seq (the reference's Redis stream of the
        last N decoded frames). Needs ``buffer.in_memory`` > 1 to hold more than the newest."""
        w, cam = self.worker_of(name)
        return w.read_history(cam, after, count)

    def history_bytes(self, name: str, after: int = 0, count: int = 0) -> list:
        """``[(seq, serialized VideoFrame)]`` of the same frames."""
        w, cam = self.worker_of(name)
        return w.video_frames(cam, after, count, name)

    def history_seqs(self, name: str, after: int = 0, count: int = 0) -> list:
        """The seqs ``history`` would return (no frame is copied)."""
        w, cam = self.worker_of(name)
        return list(w.history_seqs(cam, after, count))

    def published(self, name: str) -> int:
        w, cam = self.worker_of(name)
        return int(w.published(cam))

    def wait_frame(self, name: str, after: int, timeout_ms: int) -> bool:
        w, cam = self.worker_of(name)
        return bool(w.wait_frame(cam, after, int(timeout_ms)))

    def wait_decoded(self, name: str, n: int = 1, timeout_s: float = 10.0) -> bool:
        w, cam = self.worker_of(name)
        deadline = time.time() + timeout_s
        while time.time() < deadline:
            if w.published(cam) >= n:
                return True
            w.wait_frame(cam, w.published(cam), 50)
        return False
