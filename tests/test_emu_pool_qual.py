"""Qualified scan pools on the wave64 lockstep interpreter: the cases of tests/test_gpu_zz_pool_qual.py re-run in a child process
against tests/emu/libvsgpu_emu.so (the unmodified kernel sources compiled for the host, see tests/test_emu.py), under guard pages behind
every device allocation.  The randomised cases are repeated with the lanes scheduled highest-first and in shuffled order: the window
kernel's LDS bitmap is set with integer atomics by whichever lane resolves a row first — nothing may depend on the order."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
# pages (3 x 2 x 4), CUT resumes (1), every scan ends (2), extremes (1), mixed use (1), no window (1), label keys (1), a mask (1), ties
# (1), plain (4), the budget (1), refusals (1)
N_CASES = 39
RANDOMISED = "test_mixed or test_a_tie_heavy or test_a_visibility or (test_pages and chunk_7 and fast_prefetch)"
N_RANDOMISED = 6


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def _run(env, *select):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zz_pool_qual.py"), "-m", "gpu", "-x", "-q", "-p",
           "no:cacheprovider", *select]
    r = subprocess.run(cmd, env=dict(os.environ, VS_EMU="1", **env), capture_output=True, text=True, cwd=ROOT, timeout=3000)
    return r, (r.stdout + r.stderr)[-3000:]


def test_qualified_pool_cases_pass_on_the_wave64_interpreter(emu_lib):
    r, tail = _run({})
    assert r.returncode == 0, tail
    assert f"{N_CASES} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail


@pytest.mark.parametrize("order", ["reverse", "shuffle"])
def test_randomised_cases_under_other_lane_orders(emu_lib, order):
    r, tail = _run({"VS_EMU_ORDER": order}, "-k", RANDOMISED)
    assert r.returncode == 0, tail
    assert f"{N_RANDOMISED} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
