"""The wide-k qualified calls on the wave64 lockstep interpreter: the cases of tests/test_gpu_zz_qual_wide.py re-run in a child process
against tests/emu/libvsgpu_emu.so, under guard pages behind every device allocation.  The randomised cases are repeated with the lanes
scheduled highest-first and in shuffled order: an emitted place is a popcount of the lanes below, a histogram count a sum of LDS
atomics — nothing may depend on the order.  (The whole file, k = 4096 over 6 000 rows included, takes about 20 s: nothing is dropped.)"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
RANDOMISED = "test_exact_wide or test_ties or test_keys or test_flat_wide"


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def _run(env, *select):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zz_qual_wide.py"), "-m", "gpu", "-x", "-q", "-p",
           "no:cacheprovider", *select]
    r = subprocess.run(cmd, env=dict(os.environ, VS_EMU="1", **env), capture_output=True, text=True, cwd=ROOT, timeout=3000)
    return r, (r.stdout + r.stderr)[-3000:]


@pytest.mark.parametrize("order,select", [(None, ()), ("reverse", ("-k", RANDOMISED)), ("shuffle", ("-k", RANDOMISED))],
                         ids=["default", "reverse", "shuffle"])
def test_wide_k_cases_pass_on_the_wave64_interpreter(emu_lib, order, select):
    r, tail = _run({"VS_EMU_ORDER": order} if order else {}, *select)
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
