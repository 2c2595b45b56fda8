"""The plain-storage lifecycle chains on the wave64 lockstep interpreter: chain A (cosine, 24 of 40 dimensions indexed), B, C (L2) and
two seeds of D of tests/test_gpu_zw_plain_lifecycle.py re-run in a child process against tests/emu/libvsgpu_emu.so (the unmodified
kernel sources compiled for the host, see tests/test_emu.py), so that an insert, a consolidation, a compaction, a shrink or a
followed page list that forgets to refresh what a plain index derives from its arrays — the slice divisors, the launch plan, a
pool's capacities, the qualifiers — is noticed where no GPU is at hand.  The chains start from 200 rows there (N0 of the module).
The interpreter build lacks nothing these chains need: none is left out for that reason."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")

CASES = ("(test_chain_a_reserve_grow_vacuum_compact_shrink_grow and cosine) or test_chain_b_uploaded_inner_product_delete_compact_shrink or "
         "(test_chain_c_a_followed_relation and l2) or test_chain_d_drawn_operations[1] or test_chain_d_drawn_operations[3]")


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def test_plain_lifecycle_chains_pass_on_the_wave64_interpreter(emu_lib):
    env = dict(os.environ, VS_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zw_plain_lifecycle.py"), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
           "-k", CASES]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=3000)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "5 passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
