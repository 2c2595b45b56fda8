"""The lifecycle chains on the wave64 lockstep interpreter: chain A (cosine), B, C and two seeds of D of tests/test_gpu_zw_lifecycle.py
re-run in a child process against tests/emu/libvsgpu_emu.so (the unmodified kernel sources compiled for the host, see
tests/test_emu.py), so that an insert, a consolidation or a repair that forgets to invalidate what the index derived from its
arrays is noticed where no GPU is at hand.  The chains start from 300 rows there (N0 of the module)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")

CASES = ("(test_chain_a_unlabeled_grow_vacuum_grow_vacuum_reserve and cosine) or test_chain_b_labeled_new_label_vacuum_of_a_label_and_its_return or "
         "test_chain_c_live_scans_pool_and_broker_are_rescanned_not_recreated or test_chain_d_drawn_operations[1] or "
         "test_chain_d_drawn_operations[6]")


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def test_lifecycle_chains_pass_on_the_wave64_interpreter(emu_lib):
    env = dict(os.environ, VS_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zw_lifecycle.py"), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
           "-k", CASES]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=3000)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "5 passed" in r.stdout and "failed" not in r.stdout, tail
