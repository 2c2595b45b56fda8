"""The plain-storage build and insert on the wave64 lockstep interpreter: the cases of tests/test_gpu_zy_plain_build.py re-run in a
child process against tests/emu/libvsgpu_emu.so (the unmodified kernel sources compiled for the host, see tests/test_emu.py), so
that k_search<BUILD, PLAIN>, the plain forms of the prune and back-edge kernels, the plain mates kernel and the stand-alone prune are
checked against the numpy restatement and the oracle where no GPU is at hand.  Nothing is left out or shrunk.  The prune cases run
again with the lanes scheduled highest-first and in shuffled order."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
N_PRUNE = 32  # 4 dimension shapes x 4 list lengths x 2 distances
N_CASES = N_PRUNE + 4 + 4 + 1 + 1 + 2 + 1 + 1 + 1  # + mates, small builds, parity, quality, inserts, snapshots, empty index, refusals


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def _run(env, *select):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zy_plain_build.py"), "-m", "gpu", "-x", "-q", "-p",
           "no:cacheprovider", *select]
    r = subprocess.run(cmd, env=dict(os.environ, VS_EMU="1", **env), capture_output=True, text=True, cwd=ROOT, timeout=3000)
    return r, (r.stdout + r.stderr)[-3000:]


def test_plain_build_cases_pass_on_the_wave64_interpreter(emu_lib):
    r, tail = _run({})
    assert r.returncode == 0, tail
    assert f"{N_CASES} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail


@pytest.mark.parametrize("order", ["reverse", "shuffle"])
def test_prune_under_other_lane_orders(emu_lib, order):
    r, tail = _run({"VS_EMU_ORDER": order}, "-k", "test_prune_plain_is_exact")
    assert r.returncode == 0, tail
    assert f"{N_PRUNE} passed" in r.stdout and "failed" not in r.stdout, tail
