"""The resumable rescore window on the wave64 lockstep interpreter: the whole of tests/test_gpu_zt_cursor_window.py re-run in a child
process against tests/emu/libvsgpu_emu.so (the unmodified kernel sources compiled for the host, see tests/test_emu.py), so that
k_resort_cursor, k_resort_cursor_batch and the host code that carries their heaps from call to call are held to the oracle on tied,
negative and special distances where no GPU is at hand.  Nothing is left out or shrunk, the widest pool included.  The pools' chunk
matrix on the ties and ip corpora runs again with the lanes scheduled highest-first and in shuffled order: k_resort_cursor_batch passes
its heap, the keys it fetched ahead and the positions of the rows it produced through LDS and must not depend on which lane runs first.
(The special corpora, whose scans run to their end, are not repeated under the other orders: with them the three runs took 74 s on 8
cores, without them 47 s.  The interpreter's floating point is the host's: what the device makes of a NaN, a signed
zero or a denormal is the GPU tier's to say.)"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
N_MATRIX = 4 * 3 * 2  # ties, ip and the two special corpora x rescore 1, 4, 30 x the pools' two search kernels
# direct cursor 4 corpora x 5 windows, on special 2 x 2, restart 2, prefetch 1, the matrix, drains 2 x 2, widest 2, broker 4 x 2, batch 2
N_CASES = 20 + 4 + 2 + 1 + N_MATRIX + 4 + 2 + 8 + 2


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def _run(env, *select):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zt_cursor_window.py"), "-m", "gpu", "-x", "-q", "-p",
           "no:cacheprovider", *select]
    r = subprocess.run(cmd, env=dict(os.environ, VS_EMU="1", **env), capture_output=True, text=True, cwd=ROOT, timeout=3000)
    return r, (r.stdout + r.stderr)[-3000:]


def test_cursor_window_cases_pass_on_the_wave64_interpreter(emu_lib):
    r, tail = _run({})
    assert r.returncode == 0, tail
    assert f"{N_CASES} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail


@pytest.mark.parametrize("order", ["reverse", "shuffle"])
def test_pool_matrix_under_other_lane_orders(emu_lib, order):
    r, tail = _run({"VS_EMU_ORDER": order}, "-k", "test_pool_chunks_on_ties_negative_and_special_distances and not special_l2 and not special_ip")
    assert r.returncode == 0, tail
    assert f"{N_MATRIX // 2} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
