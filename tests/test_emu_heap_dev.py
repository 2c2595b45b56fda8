"""vs_heap_dev_* on the wave64 lockstep interpreter: the cases of tests/test_gpu_zx_heap_dev.py re-run in a child process against
tests/emu/libvsgpu_emu.so (the unmodified kernel sources compiled for the host, see tests/test_emu.py), so that k_heap_dev_heap's
tuple deforming, k_heap_dev_toast's chunk checks and copies, the finish pass, vs_index_alloc_vecs and vs_pages_follow_apply_dev are
held to the host reader and the source vectors where no GPU is at hand — under guard pages behind every device allocation, which
is where a missing bounds check on a malformed page would show.  The external shapes run again with the lanes scheduled
highest-first and in shuffled order: the table of references is filled through an atomic counter and sorted before use, so the
output may not depend on the order."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
# eleven shapes in three feeds (33), the chunk header forms (1), line pointers and gaps (4), the shuffled TOAST relation (1), 16 KB
# pages (2), compressed vectors (1), malformed heap (6) and TOAST (4) input, into an index (2), the followers (2)
N_CASES = 56
N_EXTERNAL = 6 * 3


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def _run(env, *select):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zx_heap_dev.py"), "-m", "gpu", "-x", "-q", "-p",
           "no:cacheprovider", *select]
    r = subprocess.run(cmd, env=dict(os.environ, VS_EMU="1", **env), capture_output=True, text=True, cwd=ROOT, timeout=3000)
    return r, (r.stdout + r.stderr)[-3000:]


def test_heap_dev_cases_pass_on_the_wave64_interpreter(emu_lib):
    r, tail = _run({})
    assert r.returncode == 0, tail
    assert f"{N_CASES} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail


@pytest.mark.parametrize("order", ["reverse", "shuffle"])
def test_external_shapes_under_other_lane_orders(emu_lib, order):
    r, tail = _run({"VS_EMU_ORDER": order}, "-k", "test_round_trip and ext")
    assert r.returncode == 0, tail
    assert f"{N_EXTERNAL} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
