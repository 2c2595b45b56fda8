"""vs_heap_res_*, k_heap_vis and vs_index_snapshot_eval / _put_dev / _patch on the wave64 lockstep interpreter: the cases of
tests/test_gpu_zx_heap_vis.py re-run in a child process against tests/emu/libvsgpu_emu.so (the unmodified kernel sources compiled for
the host, see tests/test_emu.py), so that the rule, the chain walk, the per-wave reductions and the resident fork are held to the
known answers and the Python restatement where no GPU is at hand — under guard pages behind every device allocation, which is where
a missing bounds check on a malformed page would show.  The randomised run is repeated with the lanes scheduled highest-first and in
shuffled order: the undecided list is filled through an atomic counter and sorted before it is handed out, so no output may depend
on the order."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
# known answers and line pointer classes (2), the randomised run (8) and the list's capacity (1), chains (2) and cycles (2), the
# resident fork (2), malformed pages (5), on an index (3)
N_CASES = 25
N_RANDOMISED = 8


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def _run(env, *select):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zx_heap_vis.py"), "-m", "gpu", "-x", "-q", "-p",
           "no:cacheprovider", *select]
    r = subprocess.run(cmd, env=dict(os.environ, VS_EMU="1", **env), capture_output=True, text=True, cwd=ROOT, timeout=3000)
    return r, (r.stdout + r.stderr)[-3000:]


def test_heap_vis_cases_pass_on_the_wave64_interpreter(emu_lib):
    r, tail = _run({})
    assert r.returncode == 0, tail
    assert f"{N_CASES} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail


@pytest.mark.parametrize("order", ["reverse", "shuffle"])
def test_randomised_run_under_other_lane_orders(emu_lib, order):
    r, tail = _run({"VS_EMU_ORDER": order}, "-k", "test_randomised_differential")
    assert r.returncode == 0, tail
    assert f"{N_RANDOMISED} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
