"""vs_pages_dev_* on the wave64 lockstep interpreter: the cases of tests/test_gpu_zx_pages_dev_matrix.py re-run in a child process
against tests/emu/libvsgpu_emu.so (the unmodified kernel sources compiled for the host, see tests/test_emu.py), so that
k_pages_decode and k_pages_labels are held to the host reader and the source arrays where no GPU is at hand — under guard pages behind
every device allocation, which is where a missing bounds check on a malformed page would show: as a segfault of the child, not as a
wrong answer.  The well-formed relations and the list ends run again with the lanes scheduled highest-first and in shuffled order:
the list end is a ballot, and the first error is taken by a compare-and-swap, so neither may depend on the order."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
# fourteen well-formed relations (14), the end of a neighbor list in nine slots (9), 26 malformed items in three places (78), wrong
# geometry (3) and the call sequence (1)
N_CASES = 105
N_DIFFERENTIAL = 14 + 9


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def _run(env, *select):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zx_pages_dev_matrix.py"), "-m", "gpu", "-x", "-q", "-p",
           "no:cacheprovider", *select]
    r = subprocess.run(cmd, env=dict(os.environ, VS_EMU="1", **env), capture_output=True, text=True, cwd=ROOT, timeout=3000)
    return r, (r.stdout + r.stderr)[-3000:]


def test_pages_dev_cases_pass_on_the_wave64_interpreter(emu_lib):
    r, tail = _run({})
    assert r.returncode == 0, tail
    assert f"{N_CASES} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail


@pytest.mark.parametrize("order", ["reverse", "shuffle"])
def test_differential_cases_under_other_lane_orders(emu_lib, order):
    r, tail = _run({"VS_EMU_ORDER": order}, "-k", "test_differential or test_neighbor_list_ends_at_first_invalid_pointer")
    assert r.returncode == 0, tail
    assert f"{N_DIFFERENTIAL} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
