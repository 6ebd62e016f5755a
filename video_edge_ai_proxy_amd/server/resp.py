"""Redis-stream-compatible endpoint of the frame history (``serving.resp_port``).

Reference parity: the reference's worker XADDs every decoded frame into a Redis stream keyed by
the device name, capped at ``buffer.in_memory`` entries, one field ``data`` holding the serialized
``VideoFrame`` (python/read_image.py:87-121), and publishes that Redis on host port 6379
(docker-compose.yml:28-31). A consumer written against it (``XREVRANGE cam + - COUNT n``,
``XREAD BLOCK ms STREAMS cam $``) works against this endpoint unchanged: stream key = device
name, entry id = ``<seq>-0`` (the ring's publish counter), field ``data``.

A small RESP2 server (one thread per connection, a handful of consumers): PING, XLEN, XRANGE,
XREVRANGE, XREAD [COUNT n] [BLOCK ms] STREAMS key... id...; AUTH / SELECT / CLIENT answer +OK;
anything else ``-ERR unknown command``. Ids: ``-``, ``+``, ``$``, ``N``, ``N-M``, ``(N`` (exclusive).

Deviation from the reference (docs/PARITY.md A.18): a stream read counts as a query — it calls
``Hub.touch``, so the lazy decoder wakes; in the reference only the gRPC call does.

Hardening: a request is at most 64 KB and 64 array elements; malformed input closes the
connection; an unknown key is an empty stream.
"""
from __future__ import annotations

import logging
import socket
import threading
import time
from typing import Optional

log = logging.getLogger("vep.resp")

MAX_REQUEST = 64 << 10
MAX_ELEMENTS = 64
_INF = 1 << 62


class ProtocolError(Exception):
    pass


def parse_request(buf: bytes):
    """One request from the head of ``buf``: ``(args, consumed)``, or ``(None, 0)`` when more bytes
    are needed. Raises ProtocolError on malformed or oversized input."""
    if not buf:
        return None, 0
    if buf[:1] != b"*":  # inline command ("PING\r\n")
        end = buf.find(b"\n")
        if end < 0:
            if len(buf) > MAX_REQUEST:
                raise ProtocolError("inline request too long")
            return None, 0
        args = buf[:end].strip().split()
        if len(args) > MAX_ELEMENTS:
            raise ProtocolError("too many arguments")
        return args, end + 1
    end = buf.find(b"\r\n")
    if end < 0:
        if len(buf) > 32:
            raise ProtocolError("array header too long")
        return None, 0
    n = _int(buf[1:end])
    if n < 0 or n > MAX_ELEMENTS:
        raise ProtocolError("array length out of range")
    pos, args = end + 2, []
    for _ in range(n):
        if pos >= len(buf):
            return None, 0
        if buf[pos:pos + 1] != b"$":
            raise ProtocolError("bulk string expected")
        end = buf.find(b"\r\n", pos)
        if end < 0:
            if len(buf) - pos > 32:
                raise ProtocolError("bulk header too long")
            return None, 0
        ln = _int(buf[pos + 1:end])
        if ln < 0 or ln > MAX_REQUEST or end + 2 + ln + 2 > MAX_REQUEST:
            raise ProtocolError("bulk string out of range")
        if len(buf) < end + 2 + ln + 2:
            return None, 0
        if buf[end + 2 + ln:end + 4 + ln] != b"\r\n":
            raise ProtocolError("bulk string not terminated")
        args.append(buf[end + 2:end + 2 + ln])
        pos = end + 4 + ln
    return args, pos


def _int(b: bytes) -> int:
    try:
        if not b or len(b) > 20 or not (b.lstrip(b"-").isdigit()):
            raise ValueError
        return int(b)
    except ValueError:
        raise ProtocolError("integer expected") from None


def _bulk(b: bytes) -> bytes:
    return b"$%d\r\n%s\r\n" % (len(b), b)


def _array(items: list) -> bytes:
    return b"*%d\r\n%s" % (len(items), b"".join(items))


def _err(msg: str) -> bytes:
    return b"-ERR " + msg.encode("utf-8", "replace").replace(b"\r", b" ").replace(b"\n", b" ") + b"\r\n"


NIL_ARRAY = b"*-1\r\n"


class CommandError(Exception):
    pass


def parse_id(s: bytes, low: bool) -> int:
    """Stream id -> inclusive seq bound. ``low``: a range start (else an end). ``N-M`` with M > 0
    lies after entry ``N-0``, the only one with that N."""
    excl = s.startswith(b"(")
    if excl:
        s = s[1:]
    if s == b"-":
        return 0
    if s == b"+":
        return _INF
    ms, _, sub = s.partition(b"-")
    if not ms.isdigit() or (sub and not sub.isdigit()) or len(ms) > 18:
        raise CommandError("Invalid stream ID specified as stream command argument")
    n, m = int(ms), int(sub or 0)
    if low:
        return n + 1 if (excl or m > 0) else n
    return n - 1 if (excl and m == 0) else n


def _entry(seq: int, data: bytes) -> bytes:
    return _array([_bulk(b"%d-0" % seq), _array([_bulk(b"data"), _bulk(data)])])


class RespServer:
    def __init__(self, hub, host: str = "0.0.0.0", port: int = 0):
        self.hub = hub
        self._stop = threading.Event()
        self._sock = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
        self._sock.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        self._sock.bind((host, port))
        self._sock.listen(64)
        self._sock.settimeout(0.2)
        self.port = self._sock.getsockname()[1]
        self.errors = 0  # handler exceptions that were not protocol / command errors
        self._conns: set = set()
        self._lock = threading.Lock()
        self._thread = threading.Thread(target=self._accept, daemon=True, name="vep-resp")
        self._thread.start()
        log.info("RESP endpoint on %s:%d", host, self.port)

    # ------------------------------------------------------------------ lifecycle
    def stop(self) -> None:
        self._stop.set()
        try:
            self._sock.close()
        except OSError:
            pass
        with self._lock:
            conns = list(self._conns)
        for c in conns:
            try:
                c.shutdown(socket.SHUT_RDWR)
            except OSError:
                pass
        self._thread.join(timeout=2)

    def _accept(self) -> None:
        while not self._stop.is_set():
            try:
                conn, _ = self._sock.accept()
            except socket.timeout:
                continue
            except OSError:
                return
            with self._lock:
                self._conns.add(conn)
            threading.Thread(target=self._serve, args=(conn,), daemon=True, name="vep-resp-conn").start()

    def _serve(self, conn: socket.socket) -> None:
        buf = b""
        try:
            conn.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
            while not self._stop.is_set():
                try:
                    args, used = parse_request(buf)
                except ProtocolError:
                    return  # malformed input: close
                if args is None:
                    if len(buf) > MAX_REQUEST:
                        return
                    chunk = conn.recv(65536)
                    if not chunk:
                        return
                    buf += chunk
                    continue
                buf = buf[used:]
                if args:
                    conn.sendall(self.execute(args))
        except OSError:
            pass
        except Exception:  # noqa: BLE001
            self.errors += 1
            log.exception("RESP connection failed")
        finally:
            with self._lock:
                self._conns.discard(conn)
            try:
                conn.close()
            except OSError:
                pass

    # ------------------------------------------------------------------ commands
    def execute(self, args: list) -> bytes:
        cmd = args[0].upper()
        try:
            if cmd == b"PING":
                return _bulk(args[1]) if len(args) > 1 else b"+PONG\r\n"
            if cmd in (b"AUTH", b"SELECT", b"CLIENT"):
                return b"+OK\r\n"
            if cmd == b"XLEN":
                self._arity(args, 2, 2)
                name = self._name(args[1])
                return b":%d\r\n" % (len(self.hub.history_seqs(name)) if name is not None else 0)
            if cmd in (b"XRANGE", b"XREVRANGE"):
                return self._xrange(args, cmd == b"XREVRANGE")
            if cmd == b"XREAD":
                return self._xread(args)
        except CommandError as e:
            return _err(str(e))
        except NotImplementedError as e:
            return _err(str(e))
        return _err("unknown command '%s'" % args[0][:64].decode("utf-8", "replace"))

    @staticmethod
    def _arity(args: list, lo: int, hi: int) -> None:
        if not lo <= len(args) <= hi:
            raise CommandError("wrong number of arguments for '%s' command" % args[0].decode("utf-8", "replace").lower())

    def _name(self, key: bytes) -> Optional[str]:
        try:
            name = key.decode("utf-8")
        except UnicodeDecodeError:
            return None
        return name if self.hub.has(name) else None

    def _frames(self, key: bytes, lo: int, hi: int, touch: bool = True, newest: int = 0) -> list:
        """[(seq, VideoFrame bytes)] of stream ``key`` with lo <= seq <= hi, ascending (``newest``
        > 0: at most that many, the newest ones). An unknown key is an empty stream."""
        name = self._name(key)
        if name is None:
            return []
        try:
            if touch:
                self.hub.touch(name)  # a stream read is a query: the lazy decoder wakes
            frames = self.hub.history_bytes(name, max(lo - 1, 0), newest if hi >= _INF else 0)
        except (KeyError, RuntimeError) as e:  # camera stopped meanwhile / its worker restarting
            if isinstance(e, NotImplementedError):
                raise
            return []
        return [(s, b) for s, b in frames if s <= hi]

    @staticmethod
    def _count(args: list, at: int) -> int:
        if len(args) == at:
            return 0
        if len(args) != at + 2 or args[at].upper() != b"COUNT" or not args[at + 1].isdigit():
            raise CommandError("syntax error")
        return int(args[at + 1][:9])

    def _xrange(self, args: list, rev: bool) -> bytes:
        self._arity(args, 4, 6)
        lo = parse_id(args[3] if rev else args[2], True)
        hi = parse_id(args[2] if rev else args[3], False)
        count = self._count(args, 4)
        frames = self._frames(args[1], lo, hi, newest=count if rev else 0)
        if rev:
            frames.reverse()
        if count:
            frames = frames[:count]
        return _array([_entry(s, b) for s, b in frames])

    def _xread(self, args: list) -> bytes:
        count, block, i = 0, None, 1
        while i < len(args) and args[i].upper() != b"STREAMS":
            opt = args[i].upper()
            if opt in (b"COUNT", b"BLOCK") and i + 1 < len(args) and args[i + 1].isdigit():
                if opt == b"COUNT":
                    count = int(args[i + 1][:9])
                else:
                    block = int(args[i + 1][:12])
                i += 2
            else:
                raise CommandError("syntax error")
        rest = args[i + 1:]
        if i >= len(args) or not rest or len(rest) % 2:
            raise CommandError("Unbalanced XREAD list of streams: for each stream key an ID or '$' must be specified.")
        keys, ids = rest[:len(rest) // 2], rest[len(rest) // 2:]
        after = []
        for k, s in zip(keys, ids):
            name = self._name(k)
            if s == b"$":
                after.append(self.hub.published(name) if name is not None else 0)
            else:
                after.append(parse_id(s.lstrip(b"("), False))  # entries after N-M: seq > N (only N-0 exists)

        def collect():
            out = []
            for k, a in zip(keys, after):
                frames = self._frames(k, a + 1, _INF)
                if count:
                    frames = frames[:count]
                if frames:
                    out.append(_array([_bulk(k), _array([_entry(s, b) for s, b in frames])]))
            return out

        out = collect()
        if not out and block is not None:
            deadline = None if block == 0 else time.monotonic() + block / 1000.0
            while not out and not self._stop.is_set():
                left = 250 if deadline is None else int(min(250, (deadline - time.monotonic()) * 1000))
                if left <= 0:
                    break
                live = [(self._name(k), a) for k, a in zip(keys, after)]
                live = [(n, a) for n, a in live if n is not None]
                if len(live) == 1:
                    try:
                        self.hub.wait_frame(live[0][0], live[0][1], left)
                    except (KeyError, RuntimeError):
                        time.sleep(left / 1000.0)
                else:
                    time.sleep(min(left, 10) / 1000.0)
                out = collect()
        return _array(out) if out else NIL_ARRAY
