"""Qualified scans on the wave64 lockstep interpreter: the cases of tests/test_gpu_zz_qual.py re-run in a child process against
tests/emu/libvsgpu_emu.so (the unmodified kernel sources compiled for the host, see tests/test_emu.py), under guard pages behind every
device allocation.  The randomised cases are repeated with the lanes scheduled highest-first and in shuffled order: a bitmap word is one
ballot, a kept row's place a popcount of lanes below it, the counts integer atomics — nothing may depend on the order."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
# case A (4 + 2), case C (2), extremes (1), the unqualified launch (1), unfused / replay (2), ties (1), a large window (1), label keys
# (1), plain (2), the device entry point (1), chunks and mixed slots (1), from_tids (1), insert (1), compact (1), refusals (1)
N_CASES = 23
RANDOMISED = "test_case_a or test_case_c or test_from_tids or test_a_host_batch or test_a_tie_heavy"
N_RANDOMISED = 13


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def _run(env, *select):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zz_qual.py"), "-m", "gpu", "-x", "-q", "-p",
           "no:cacheprovider", *select]
    r = subprocess.run(cmd, env=dict(os.environ, VS_EMU="1", **env), capture_output=True, text=True, cwd=ROOT, timeout=3000)
    return r, (r.stdout + r.stderr)[-3000:]


def test_qualified_scan_cases_pass_on_the_wave64_interpreter(emu_lib):
    r, tail = _run({})
    assert r.returncode == 0, tail
    assert f"{N_CASES} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail


@pytest.mark.parametrize("order", ["reverse", "shuffle"])
def test_randomised_cases_under_other_lane_orders(emu_lib, order):
    r, tail = _run({"VS_EMU_ORDER": order}, "-k", RANDOMISED)
    assert r.returncode == 0, tail
    assert f"{N_RANDOMISED} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
