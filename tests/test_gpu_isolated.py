"""The process-isolated hub on the GPU (``gpu.isolation: process``): a front-end program that
never touches the GPU supervises a worker process on device 0 (vep_bench/isolated_check.py). Checks
frames served through page-locked shared memory against the ring, the RCCL-group consumer batch
against the fp32 letterbox reference, and a SIGKILLed GPU worker's restart + group re-formation.
Started once as a child program with its own time limit (this pytest process holds a GPU context,
so the front-end must be a separate process); the tests share its result. Where the driver
page-locks no memory that a program already has (tests/page_lock.py), the worker stages its frames
into the shared memory: ``test_isolated_hub_stages_or_page_locks`` checks the hub either way, and
``test_isolated_hub_on_gpu``, which asks for page-locked shared memory, skips itself."""
import json
import os
import subprocess
import sys

import pytest

from page_lock import host_register_works, skip_unless_host_register_works

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(native):
    """A small worker on device 0 of this process: it carries ``register_host``."""
    return native.Worker(device=0, letterbox_size=0)


@pytest.fixture(scope="module")
def hub_run():
    cmd = [sys.executable, "-m", "vep_bench.isolated_check", "--devices=0", "--cams", "2",
           "--width", "1920", "--height", "1080", "--letterbox", "640", "--samples", "30", "--kill"]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=110, cwd=ROOT)


def test_isolated_hub_stages_or_page_locks(probe, hub_run):
    """Everything the hub is checked for, with the shared memory page-locked exactly where the
    driver can page-lock it."""
    r = hub_run
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, r.stderr[-3000:]
    d = json.loads(lines[-1])
    assert r.returncode == 0 and d["ok"], (d, r.stderr[-2000:])
    assert d["shm_pinned"] == host_register_works(probe)
    assert d["frame_equal"] and d["batch_max_abs_err"] <= 1
    assert d["group"][0]["backend"] == "nccl" and d["restarted"]


def test_isolated_hub_on_gpu(probe, request):
    skip_unless_host_register_works(probe)  # asks for page-locked shared memory
    r = request.getfixturevalue("hub_run")
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, r.stderr[-3000:]
    d = json.loads(lines[-1])
    assert r.returncode == 0 and d["ok"], (d, r.stderr[-2000:])
    assert d["shm_pinned"] and d["frame_equal"] and d["batch_max_abs_err"] <= 1
    assert d["group"][0]["backend"] == "nccl" and d["restarted"]
