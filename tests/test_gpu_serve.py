"""The serving reads' GPU branches that no other GPU test reaches (csrc/vep/serve.cpp, run on an
MI355X): ``read_latest`` into page-locked memory (one DMA straight into the destination, only a
serve buffer's completion event) and ``read_latest_many`` (the frame bus pump's batched read).

One camera on a 2-slot ring at 16x16, the smallest picture the synthetic camera makes (the Python
API has no way to write a smaller frame into a ring). The reference is the CPU backend's answer
for the same access units, byte for byte."""
import os

import numpy as np
import pytest

from conftest import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pair(native):
    """A worker on GPU 0 and a CPU-backend worker, one camera each, fed the same three access
    units; the CPU worker's serialized newest frame is the shared reference."""
    gw, cw = native.Worker(device=0), native.Worker(device=-1)
    enc = synth(native, 16, 16, gop=4, motion=0.3)
    g, c = gw.add_camera("cam", 2), cw.add_camera("cam", 2)
    for _ in range(3):
        au = enc.next()
        assert gw.decode_now(g, au) and cw.decode_now(c, au)
    seq, want, _ = cw.video_frame(c, 0, "cam")
    assert seq == 3 and len(want) > 16 * 16 * 3
    return gw, g, want


def test_read_latest_into_page_locked_memory(native, pair):
    gw, g, want = pair
    cap = gw.video_frame_bound(g, "cam")
    buf = np.zeros(cap, np.uint8)
    addr = buf.ctypes.data
    assert gw.register_host(addr, cap)
    try:
        seq, n, meta = gw.video_frame_into(g, 0, "cam", addr, cap, True)
        assert gw.video_frame_into(g, seq, "cam", addr, cap, True) is None  # nothing newer
    finally:
        gw.unregister_host(addr)
    assert seq == 3 and (meta["width"], meta["height"]) == (16, 16)
    assert bytes(buf[:n]) == want
    # ... and the staged (chunked) read of the same frame
    seq2, n2, _ = gw.video_frame_into(g, 0, "cam", addr, cap, False)
    assert seq2 == 3 and bytes(buf[:n2]) == want


def test_bus_pump_reads_many(native, pair):
    gw, g, want = pair
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
