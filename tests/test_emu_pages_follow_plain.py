"""vs_pages_follow_open_plain on the wave64 lockstep interpreter: the cases of tests/test_gpu_zx_pages_follow_plain.py re-run in a
child process against tests/emu/libvsgpu_emu.so (the unmodified kernel sources compiled for the host, see tests/test_emu.py), so
that k_pages_follow_plain's check pass, its scatter, the copy of the appended vectors and the table arithmetic are held to the numpy
restatement where no GPU is at hand.  The append step of every shape runs again with the lanes scheduled highest-first and in
shuffled order: the kernel assigns no slot atomically, so its output may not depend on the order."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
# the seven shapes in their six steps (42), vectors from the pages on the six full-width shapes, an index uploaded from its pages
# alone and the truncated one (8), a changed vector at two widths (2), the unchanged relation of the three cosine shapes (3), the
# refusals, the library's own pair
N_CASES = 58
N_SHAPES = 7


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def _run(env, *select):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zx_pages_follow_plain.py"), "-m", "gpu", "-x", "-q", "-p",
           "no:cacheprovider", *select]
    r = subprocess.run(cmd, env=dict(os.environ, VS_EMU="1", **env), capture_output=True, text=True, cwd=ROOT, timeout=3000)
    return r, (r.stdout + r.stderr)[-3000:]


def test_plain_follower_cases_pass_on_the_wave64_interpreter(emu_lib):
    r, tail = _run({})
    assert r.returncode == 0, tail
    assert f"{N_CASES} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail


@pytest.mark.parametrize("order", ["reverse", "shuffle"])
def test_append_under_other_lane_orders(emu_lib, order):
    r, tail = _run({"VS_EMU_ORDER": order}, "-k", "test_steps and append")
    assert r.returncode == 0, tail
    assert f"{N_SHAPES} passed" in r.stdout and "failed" not in r.stdout, tail
