"""k_search_plain on the wave64 lockstep interpreter: the whole of tests/test_gpu_zy_plain_search.py re-run in a child process against
tests/emu/libvsgpu_emu.so (the unmodified kernel sources compiled for the host, see tests/test_emu.py), so that the kernel, its
planner and the hand-over are checked against the oracle where no GPU is at hand.  Nothing is left out or shrunk.  The parity matrix
runs again with the lanes scheduled highest-first and in shuffled order: the dedup table's claims and the one-step push exchange
values through LDS and must not depend on which lane runs first."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
N_MATRIX = 16
N_CASES = N_MATRIX + 2 + 3 + 1 + 1 + 1 + 1 + 1 + 1 + 1  # + truncated, hand-over, spill, grid reuse, tiny, no start, deleted start, huge rows, growth


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def _run(env, *select):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zy_plain_search.py"), "-m", "gpu", "-x", "-q", "-p",
           "no:cacheprovider", *select]
    r = subprocess.run(cmd, env=dict(os.environ, VS_EMU="1", **env), capture_output=True, text=True, cwd=ROOT, timeout=3000)
    return r, (r.stdout + r.stderr)[-3000:]


def test_plain_search_cases_pass_on_the_wave64_interpreter(emu_lib):
    r, tail = _run({})
    assert r.returncode == 0, tail
    assert f"{N_CASES} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail


@pytest.mark.parametrize("order", ["reverse", "shuffle"])
def test_parity_matrix_under_other_lane_orders(emu_lib, order):
    r, tail = _run({"VS_EMU_ORDER": order}, "-k", "test_rows_bits_and_counters_match_oracle_and_general_kernel")
    assert r.returncode == 0, tail
    assert f"{N_MATRIX} passed" in r.stdout and "failed" not in r.stdout, tail
