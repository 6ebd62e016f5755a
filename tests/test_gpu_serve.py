"""The serving reads' GPU branches that no other GPU test reaches (csrc/vep/serve.cpp, run on an
MI355X): ``read_latest`` into page-locked memory (one DMA straight into the destination, only a
serve buffer's completion event) and ``read_latest_many`` (the frame bus pump's batched read).

Where the driver page-locks no memory that a program already has (tests/page_lock.py), both reads
are checked into memory that was allocated page-locked; the bus then stages its frames, which
``test_bus_pump_serves_newest_frame`` checks, and ``test_bus_pump_reads_many``, whose subject is
the bus's page-locked shared-memory segment, skips itself.

One camera on a 2-slot ring at 16x16, the smallest picture the synthetic camera makes (the Python
API has no way to write a smaller frame into a ring). The reference is the CPU backend's answer
for the same access units, byte for byte."""
import os

import numpy as np
import pytest
import torch

from conftest import synth
from page_lock import host_register_works, skip_unless_host_register_works

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def workers(native):
    """A worker on GPU 0 and a CPU-backend worker, one camera each, fed the same three access
    units."""
    gw, cw = native.Worker(device=0), native.Worker(device=-1)
    enc = synth(native, 16, 16, gop=4, motion=0.3)
    g, c = gw.add_camera("cam", 2), cw.add_camera("cam", 2)
    for _ in range(3):
        au = enc.next()
        assert gw.decode_now(g, au) and cw.decode_now(c, au)
    return gw, g, cw, c


@pytest.fixture(scope="module")
def pair(workers):
    """The GPU worker, its camera, and the shared reference: the CPU worker's serialized newest
    frame."""
    gw, g, cw, c = workers
    seq, want, _ = cw.video_frame(c, 0, "cam")
    assert seq == 3 and len(want) > 16 * 16 * 3
    return gw, g, want


def test_read_latest_into_page_locked_memory(native, pair):
    gw, g, want = pair
    cap = gw.video_frame_bound(g, "cam")
    registered = host_register_works(gw)
    if registered:
        buf = np.zeros(cap, np.uint8)
        addr = buf.ctypes.data
        assert gw.register_host(addr, cap)
    else:  # memory that was allocated page-locked
        keep = torch.zeros(cap, dtype=torch.uint8).pin_memory()
        assert keep.is_pinned()
        buf, addr = keep.numpy(), keep.data_ptr()
    try:
        seq, n, meta = gw.video_frame_into(g, 0, "cam", addr, cap, True)
        assert gw.video_frame_into(g, seq, "cam", addr, cap, True) is None  # nothing newer
    finally:
        if registered:
            gw.unregister_host(addr)
    assert seq == 3 and (meta["width"], meta["height"]) == (16, 16)
    assert bytes(buf[:n]) == want
    # ... and the staged (chunked) read of the same frame
    seq2, n2, _ = gw.video_frame_into(g, 0, "cam", addr, cap, False)
    assert seq2 == 3 and bytes(buf[:n2]) == want


def test_read_latest_many_into_page_locked_memory(native, workers):
    """The batched read as the bus pump issues it (one DMA per request straight into page-locked
    memory, one wait, then the slots checked again), here into memory allocated page-locked: two
    requests for the newest frame, one that has it already, and one that goes the staged way."""
    gw, g, cw, c = workers
    meta, pixels = cw.read_latest(c, 0)
    ref = np.ascontiguousarray(pixels).reshape(-1)
    n = 16 * 16 * 3
    assert meta["seq"] == 3 and ref.size == n
    keep = torch.full((4, n + 64), 0xA5, dtype=torch.uint8).pin_memory()
    assert keep.is_pinned()
    rows = keep.numpy()
    addr = [keep[k].data_ptr() for k in range(4)]
    res = gw.read_latest_many_into([(g, 0, addr[0], n, True), (g, 2, addr[1], n + 64, True),
                                    (g, 3, addr[2], n, True), (g, 0, addr[3], n, False)])
    assert res[2] is None and (rows[2] == 0xA5).all()  # nothing newer than 3: nothing written
    for k in (0, 1, 3):
        seq, m = res[k]
        assert seq == 3 and (m["width"], m["height"], m["pts"]) == (16, 16, meta["pts"])
        assert np.array_equal(rows[k, :n], ref)
        assert (rows[k, n:] == 0xA5).all()  # nothing past the frame
    with pytest.raises(native.NativeError, match="too small"):
        gw.read_latest_many_into([(g, 0, addr[0], n - 1, True)])


def _bus_read(native, gw, g, tag):
    """A frame bus on the worker: what one waiting reader got, the camera's entry, the counters."""
    o = native.BusOwner(tag, 0, 4)
    o.attach(gw)
    try:
        o.add(g, "cam")
        r = native.BusReader(tag)
        got = r.frame("cam", 0, 3000, 0)  # a waiting reader: the pump reads the ring's newest frame
        return got, r.info("cam"), o.published, o.dma_bytes
    finally:
        o.stop()


def test_bus_pump_serves_newest_frame(native, pair):
    """Whichever way the pump reads (into a page-locked segment by DMA, or staged where the segment
    could not be page-locked): the reader gets the ring's newest frame, read once."""
    gw, g, want = pair
    got, info, published, dma_bytes = _bus_read(native, gw, g, f"g{os.getpid()}n")
    assert got == (3, want) and published == 1 and dma_bytes == 16 * 16 * 3
    assert info["pinned"] == host_register_works(gw)


def test_bus_pump_reads_many(native, pair):
    gw, g, want = pair
    skip_unless_host_register_works(gw)  # the bus's shared-memory segment must be page-locked
    tag = f"g{os.getpid()}s"
    o = native.BusOwner(tag, 0, 4)
    o.attach(gw)
    try:
        o.add(g, "cam")
        r = native.BusReader(tag)
        got = r.frame("cam", 0, 3000, 0)  # a waiting reader: the pump reads the ring's newest frame
        assert got is not None and r.info("cam")["pinned"]
        assert got == (3, want) and o.published == 1 and o.dma_bytes == 16 * 16 * 3
    finally:
        o.stop()
