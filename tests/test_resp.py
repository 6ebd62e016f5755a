"""Redis-stream-compatible endpoint of the frame history (server/resp.py), CPU backend, spoken to
over raw sockets in RESP2 (no Redis client library is needed).

Reference semantics: `XADD <device> MAXLEN <buffer.in_memory> data <VideoFrame>`
(python/read_image.py:121) on the Redis the reference publishes on port 6379."""
import socket
import time

import numpy as np
import pytest


class Resp:
    """Minimal RESP2 client."""

    def __init__(self, port):
        self.s = socket.create_connection(("127.0.0.1", port), timeout=10)
        self.f = self.s.makefile("rb")

    def send_raw(self, b):
        self.s.sendall(b)

    def cmd(self, *args):
        out = b"*%d\r\n" % len(args)
        for a in args:
            a = a if isinstance(a, bytes) else str(a).encode()
            out += b"$%d\r\n%s\r\n" % (len(a), a)
        self.s.sendall(out)
        return self.read()

    def read(self):
        line = self.f.readline()
        if not line:
            raise EOFError
        t, rest = line[:1], line[1:-2]
        if t == b"+":
            return rest.decode()
        if t == b"-":
            return RuntimeError(rest.decode())
        if t == b":":
            return int(rest)
        if t == b"$":
            n = int(rest)
            if n < 0:
                return None
            data = self.f.read(n + 2)
            return data[:-2]
        if t == b"*":
            n = int(rest)
            return None if n < 0 else [self.read() for _ in range(n)]
        raise ValueError(line)

    def closed(self):
        """True when the server has closed the connection."""
        self.s.settimeout(5)
        try:
            return self.f.read(1) == b""
        except OSError:
            return True

    def close(self):
        self.s.close()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture(scope="module")
def farm(native):
    srv = native.RtspServer("127.0.0.1", 0)
    cfg = native.SynthConfig()
    cfg.width, cfg.height, cfg.gop, cfg.fps, cfg.seed = 160, 96, 10, 30, 11
    srv.add_stream("/cam", cfg, realtime=True, cached_frames=20)
    srv.start()
    yield srv
    srv.stop()


@pytest.fixture(scope="module")
def app(tmp_path_factory, native, farm):
    from video_edge_ai_proxy_amd.config import Config
    from video_edge_ai_proxy_amd.server.app import build_app

    cfg = Config()
    cfg.data_dir = str(tmp_path_factory.mktemp("resp") / "data")
    cfg.gpu.devices = [-1]
    cfg.buffer.in_memory = 5
    cfg.serving.frontends = 0
    cfg.serving.native = False
    cfg.serving.resp_port = _free_port()
    cfg.serving.resp_host = "127.0.0.1"
    assert cfg.history_depth == 5 and cfg.ring_slots == 5
    a = build_app(cfg, host="127.0.0.1", rest_port=0, grpc_port=0, start_rest=False, restore=False)
    url = f"rtsp://127.0.0.1:{farm.port}/cam"
    a.hub.start_camera("door", url)
    a.hub.start_camera("idle", url)
    a.hub.touch("door")  # the first query wakes the lazy decoder
    assert a.hub.wait_decoded("door", 6, 20.0)
    yield a
    a.stop()


def test_defaults_are_off():
    from video_edge_ai_proxy_amd.config import Config

    c = Config()
    assert c.serving.resp_port == 0 and c.history_depth == 0
    c.buffer.in_memory = 2
    assert c.history_depth == 2


def test_xlen_and_xrevrange(app):
    from video_edge_ai_proxy_amd.proto import pb

    c = Resp(app.resp_server.port)
    assert c.cmd("PING") == "PONG"
    assert c.cmd("AUTH", "secret") == "OK" and c.cmd("SELECT", 0) == "OK" and c.cmd("CLIENT", "SETNAME", "t") == "OK"
    n = c.cmd("XLEN", "door")
    assert 1 <= n <= 5
    assert app.hub.state("door")["history"] == 5
    got = c.cmd("XREVRANGE", "door", "+", "-", "COUNT", 3)
    assert len(got) == 3
    ids = [e[0] for e in got]
    seqs = [int(i.split(b"-")[0]) for i in ids]
    assert all(i.endswith(b"-0") for i in ids) and seqs == sorted(seqs, reverse=True)
    assert seqs == list(range(seqs[0], seqs[0] - 3, -1))
    hist = {m["seq"]: f for m, f in app.hub.history("door")}
    checked = 0
    for (eid, fields), seq in zip(got, seqs):
        assert fields[0] == b"data" and len(fields) == 2
        vf = pb.VideoFrame()
        vf.ParseFromString(fields[1])
        assert vf.width == 160 and vf.height == 96 and vf.device_id == "door" and len(vf.data) == 160 * 96 * 3
        if seq in hist:  # (the camera is live: the oldest may have left the window meanwhile)
            assert np.array_equal(np.frombuffer(vf.data, np.uint8).reshape(96, 160, 3), hist[seq])
            checked += 1
    assert checked >= 1
    # XRANGE: ascending, bounded ids, COUNT takes the oldest
    asc = c.cmd("XRANGE", "door", "-", "+")
    a = [int(e[0].split(b"-")[0]) for e in asc]
    assert a == sorted(a) and 1 <= len(a) <= 5 and a == list(range(a[0], a[0] + len(a)))
    one = c.cmd("XRANGE", "door", f"{a[-1]}-0", f"{a[-1]}", "COUNT", 1)
    assert len(one) <= 1 and (not one or one[0][0] == b"%d-0" % a[-1])
    assert c.cmd("XRANGE", "door", "+", "-") == []
    c.close()


def test_xread_block_returns_a_newer_frame(app):
    c = Resp(app.resp_server.port)
    before = app.hub.published("door")
    r = c.cmd("XREAD", "BLOCK", 2000, "STREAMS", "door", "$")
    assert r is not None and len(r) == 1 and r[0][0] == b"door"
    ids = [int(e[0].split(b"-")[0]) for e in r[0][1]]
    assert ids and min(ids) > before
    # a cursor: entries after a known id; COUNT bounds them
    r2 = c.cmd("XREAD", "COUNT", 1, "STREAMS", "door", f"{ids[0] - 1}-0")
    assert r2 is not None and len(r2[0][1]) == 1 and int(r2[0][1][0][0].split(b"-")[0]) >= ids[0]
    assert c.cmd("XREAD", "STREAMS", "door", f"{1 << 40}-0") is None  # nothing newer, no BLOCK
    c.close()


def test_stream_read_wakes_an_idle_camera(app):
    assert app.hub.published("idle") == 0  # nobody has asked for it
    c = Resp(app.resp_server.port)
    assert c.cmd("XRANGE", "idle", "-", "+") == []
    assert app.hub.wait_decoded("idle", 1, 20.0), "the stream read did not count as a query"
    assert c.cmd("XLEN", "idle") >= 1
    c.close()


def test_unknown_key_and_command(app):
    c = Resp(app.resp_server.port)
    assert c.cmd("XRANGE", "nosuch", "-", "+") == [] and c.cmd("XLEN", "nosuch") == 0
    assert c.cmd("XREAD", "STREAMS", "nosuch", "0") is None
    e = c.cmd("FLUSHALL")
    assert isinstance(e, RuntimeError) and str(e).startswith("ERR unknown command")
    e = c.cmd("XRANGE", "door", "bogus", "+")
    assert isinstance(e, RuntimeError) and str(e).startswith("ERR")
    assert c.cmd("PING") == "PONG"  # command errors keep the connection
    c.close()


def test_malformed_input_closes_the_connection(app):
    srv = app.resp_server
    c = Resp(srv.port)
    c.send_raw(b"*100\r\n")  # more than 64 elements
    assert c.closed()
    c = Resp(srv.port)
    c.send_raw(b"*2\r\n$4\r\nXLEN\r\n$100\r\nabc")  # truncated bulk string, then end of stream
    c.s.shutdown(socket.SHUT_WR)
    assert c.closed()
    c = Resp(srv.port)
    c.send_raw(b"*1\r\n$4\r\nPINGxx")  # bulk string without its terminator
    assert c.closed()
    c = Resp(srv.port)
    c.send_raw(b"*1\r\n$70000\r\n")  # a request above 64 KB
    assert c.closed()
    c = Resp(srv.port)
    c.send_raw(b"*1\r\n$-5\r\n")
    assert c.closed()
    time.sleep(0.05)
    assert srv.errors == 0, "a connection thread raised"
    c = Resp(srv.port)
    assert c.cmd("PING") == "PONG"
    c.close()


def test_parser_units():
    from video_edge_ai_proxy_amd.server import resp

    assert resp.parse_request(b"") == (None, 0)
    assert resp.parse_request(b"*1\r\n$4\r\nPI") == (None, 0)
    assert resp.parse_request(b"*2\r\n$4\r\nXLEN\r\n$1\r\na\r\nrest") == ([b"XLEN", b"a"], 21)
    assert resp.parse_request(b"PING\r\n") == ([b"PING"], 6)
    for bad in (b"*65\r\n", b"*x\r\n", b"*1\r\n:1\r\n", b"*1\r\n$3\r\nabcde"):
        with pytest.raises(resp.ProtocolError):
            resp.parse_request(bad)
    assert resp.parse_id(b"-", True) == 0 and resp.parse_id(b"+", False) > 1 << 60
    assert resp.parse_id(b"7", True) == 7 and resp.parse_id(b"7-0", False) == 7
    assert resp.parse_id(b"7-1", True) == 8 and resp.parse_id(b"(7", True) == 8 and resp.parse_id(b"(7", False) == 6
    with pytest.raises(resp.CommandError):
        resp.parse_id(b"x", True)


def test_process_isolation_has_no_history():
    from video_edge_ai_proxy_amd.engine.isolated import ProcessHub

    with pytest.raises(NotImplementedError, match="not available"):
        ProcessHub.history(None, "cam")
    with pytest.raises(NotImplementedError, match="not available"):
        ProcessHub.history_bytes(None, "cam")
