"""The scan pools' plain-storage path on the wave64 lockstep interpreter: the whole of tests/test_gpu_zy_plain_pool.py re-run in a child
process against tests/emu/libvsgpu_emu.so (the unmodified kernel sources compiled for the host, see tests/test_emu.py), so that
k_search_plain_rs, its saved state, the pool's planning and the general kernel's pool path for plain storage are checked against the
oracle where no GPU is at hand.  Nothing is left out or shrunk.  The chunk-after-chunk matrix runs again with the lanes scheduled
highest-first and in shuffled order: the dedup table's claims and the one-step push exchange values through LDS and must not depend
on which lane runs first."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
N_MATRIX = 8  # four (dim, distance, R, L) cases on the plain kernel and on the general one
N_CASES = N_MATRIX + 2 + 1 + 1 + 3 + 1 + 1 + 2  # + truncated, exhaustive, spill boundary, capacities, region reuse, edges, prefetch on / off


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def _run(env, *select):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zy_plain_pool.py"), "-m", "gpu", "-x", "-q", "-p",
           "no:cacheprovider", *select]
    r = subprocess.run(cmd, env=dict(os.environ, VS_EMU="1", **env), capture_output=True, text=True, cwd=ROOT, timeout=3000)
    return r, (r.stdout + r.stderr)[-3000:]


def test_plain_pool_cases_pass_on_the_wave64_interpreter(emu_lib):
    r, tail = _run({})
    assert r.returncode == 0, tail
    assert f"{N_CASES} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail


@pytest.mark.parametrize("order", ["reverse", "shuffle"])
def test_chunk_matrix_under_other_lane_orders(emu_lib, order):
    r, tail = _run({"VS_EMU_ORDER": order}, "-k", "test_pooled_plain_scans_hand_out_the_oracles_rows_and_stats")
    assert r.returncode == 0, tail
    assert f"{N_MATRIX} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
