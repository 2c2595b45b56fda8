"""Device-memory hygiene of graph build and maintenance on the wave64 lockstep interpreter: the two tests of
tests/test_gpu_zz_hygiene.py that count the interpreter's live allocations (every hipMalloc / hipHostMalloc is one tracked mapping)
re-run in a child process against tests/emu/libvsgpu_emu.so — the fixed sequence build -> insert -> bulk_delete -> consolidate ->
repair -> label audit and repair -> compact three times over, and the sweep that makes the k-th allocation of every call fail
(vs_emu_fail_allocation, a hook of the fake runtime only)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")

CASES = "test_maintenance_calls_return_their_device_memory or test_every_allocation_failure_is_reported_and_nothing_leaks"


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def test_hygiene_cases_pass_on_the_wave64_interpreter(emu_lib):
    env = dict(os.environ, VS_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zz_hygiene.py"), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
           "-k", CASES]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=3000)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "8 passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
