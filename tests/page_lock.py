"""Whether the driver page-locks memory that a program already has (``Worker.register_host``, i.e.
``hipHostRegister``). Some virtual machines refuse every such request: there page-locked memory can
only be allocated, so no shared-memory segment that another process maps can be page-locked, and
the tests whose subject is such a segment skip themselves."""
import ctypes
import mmap

import pytest

REASON = "hipHostRegister is not supported here"


def host_register_works(worker) -> bool:
    """Tried with the worker's own binding on one page of a shared mapping: the same kind of memory
    (shmem pages mapped shared) as the /dev/shm segments of the frame bus and the hub's slots."""
    mm = mmap.mmap(-1, mmap.PAGESIZE)
    anchor = ctypes.c_char.from_buffer(mm)
    addr = ctypes.addressof(anchor)
    try:
        ok = bool(worker.register_host(addr, mmap.PAGESIZE))
        if ok:
            worker.unregister_host(addr)
        return ok
    finally:
        del anchor
        mm.close()


def skip_unless_host_register_works(worker) -> None:
    if not host_register_works(worker):
        pytest.skip(REASON)
