"""The SBQ build and insert batch step on the wave64 lockstep interpreter: the cases of tests/test_gpu_zy_build_twin.py re-run in a
child process against tests/emu/libvsgpu_emu.so (the unmodified kernel sources compiled for the host, see tests/test_emu.py), so
that both build-mode search kernels, k_build_prune_new, k_build_prune_merge, k_insert_merge_mates, the request sort with k_seg_heads
and k_build_backedges are held to the sequential restatement (tests/build_twin.py) where no GPU is at hand.  Nothing is left out or
shrunk.  The hub and the append case run again with the lanes scheduled highest-first and in shuffled order."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
# builds (5 geometries x 2 batch sizes), inserts (3 geometries x mates off / on), hub, append, labeled, both kernels (6), wide rows (2)
N_CASES = 10 + 6 + 1 + 1 + 1 + 6 + 2
ORDER_CASES = "test_a_hub_keeps_only_its_closest_requests or test_back_edges_are_appended_while_a_row_has_room"


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def _run(env, *select):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zy_build_twin.py"), "-m", "gpu", "-x", "-q", "-p",
           "no:cacheprovider", *select]
    r = subprocess.run(cmd, env=dict(os.environ, VS_EMU="1", **env), capture_output=True, text=True, cwd=ROOT, timeout=3000)
    return r, (r.stdout + r.stderr)[-3000:]


def test_build_twin_cases_pass_on_the_wave64_interpreter(emu_lib):
    r, tail = _run({})
    assert r.returncode == 0, tail
    assert f"{N_CASES} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail


@pytest.mark.parametrize("order", ["reverse", "shuffle"])
def test_hub_and_append_under_other_lane_orders(emu_lib, order):
    r, tail = _run({"VS_EMU_ORDER": order}, "-k", ORDER_CASES)
    assert r.returncode == 0, tail
    assert "2 passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
