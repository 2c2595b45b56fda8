"""The latency-mode search kernel on the wave64 lockstep interpreter: the cases of tests/test_gpu_zzzzzz_lat_search.py re-run in a child
process against tests/emu/libvsgpu_emu.so (the unmodified kernel sources compiled for the host, see tests/test_emu.py), under guard
pages behind every device allocation.  Its waves meet at workgroup barriers only, so the interpreter's fibers cannot deadlock; the
parametrised case is repeated with the lanes scheduled highest-first and in shuffled order: what the waves hand each other through
LDS between two barriers may not depend on who ran first."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
PARAMETRISED = "test_stream_rows_and_counters"


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def _run(env, *select):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zzzzzz_lat_search.py"), "-m", "gpu", "-x", "-q", "-p",
           "no:cacheprovider", *select]
    r = subprocess.run(cmd, env=dict(os.environ, VS_EMU="1", **env), capture_output=True, text=True, cwd=ROOT, timeout=3000)
    return r, (r.stdout + r.stderr)[-3000:]


@pytest.mark.parametrize("order,select", [(None, ()), ("reverse", ("-k", PARAMETRISED)), ("shuffle", ("-k", PARAMETRISED))],
                         ids=["default", "reverse", "shuffle"])
def test_latency_kernel_cases_pass_on_the_wave64_interpreter(emu_lib, order, select):
    r, tail = _run({"VS_EMU_ORDER": order} if order else {}, *select)
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
