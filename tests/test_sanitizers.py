"""ThreadSanitizer / AddressSanitizer runs of the native stress driver (csrc/tests/native_stress.cpp)
and of the scratch pool's stand-alone selftest (csrc/tests/scratch_selftest.cpp); the stage plan's
selftest (csrc/tests/stage_plan_selftest.cpp) and the serving reads' selftest
(csrc/tests/serve_selftest.cpp) un-instrumented (`make asan-plan` / `make asan-serve` run them
under AddressSanitizer + UndefinedBehaviorSanitizer).

Host-code sanitizers only (`-Xarch_host -fsanitize=...`; GPU sanitizers are unavailable), CPU
backend. Building takes about a minute per sanitizer, so the test runs when VEP_SANITIZERS=1
(`make tsan asan` runs the same thing; the last logs are kept in profiles/).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(os.environ.get("VEP_SANITIZERS") != "1", reason="set VEP_SANITIZERS=1")
@pytest.mark.parametrize("target", ["tsan", "asan", "tsan-scratch", "asan-scratch"])
def test_native_stress_under_sanitizer(target):
    r = subprocess.run(["make", "-C", ROOT, target], capture_output=True, text=True, timeout=900)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert ("scratch_selftest ok" if target.endswith("-scratch") else "native_stress ok") in out
    assert "WARNING: ThreadSanitizer" not in out and "ERROR: AddressSanitizer" not in out


def test_scratch_selftest():
    """The scratch pool's locking (csrc/vep/scratch.h), un-instrumented: bounded sets and leases
    under 16 threads, a set never shared, returned on a throw, moved leases, the wait for a free
    set, and no growth in steady state."""
    r = subprocess.run(["make", "-C", ROOT, "scratch-selftest"], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "scratch_selftest ok" in out


def test_stage_plan_selftest():
    """The stage plan's invariants (csrc/vep/stage_plan.h) on real jobs of every kind, planned on
    the host: regions inside the buffer, aligned, disjoint and in their section; copy tasks and
    gather chunks tiling their regions; rounds and history outputs complete. Linked against the
    objects of the build."""
    r = subprocess.run(["make", "-C", ROOT, "plan-selftest"], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "stage_plan_selftest ok" in out


def test_serve_selftest():
    """The serving reads' consistent-read rule (csrc/vep/ring_read.h), un-instrumented (`make
    asan-serve` runs it under AddressSanitizer + UndefinedBehaviorSanitizer): a slot rewritten or
    invalidated during the read is read again from the newer frame and never served or committed,
    kReadAttempts times at the most; stored answers are not evaluated again. Linked against the
    objects of the build."""
    r = subprocess.run(["make", "-C", ROOT, "serve-selftest"], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "serve_selftest ok" in out


def test_sanitizer_target_links():
    """The sanitizer binaries' source set links (every csrc/vep/*.cpp + *.hip): a cheap check
    that runs in the default CPU suite, so a missing kernel file breaks here, not only under
    VEP_SANITIZERS=1."""
    r = subprocess.run(["make", "-C", ROOT, "link-check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert os.path.exists(os.path.join(ROOT, "build", "linkcheck", "native_stress"))
