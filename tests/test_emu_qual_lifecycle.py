"""The qualified and grouped lifecycle chains on the wave64 lockstep interpreter: chain Q-A (cosine), Q-B, Q-P and two seeds of Q-D of
tests/test_gpu_zz_qual_lifecycle.py re-run in a child process against tests/emu/libvsgpu_emu.so (the unmodified kernel sources
compiled for the host, see tests/test_emu.py), so that a reserve, a shrink or a compaction that forgets the mask in force, the
qualifier bitmaps or the group column is noticed where no GPU is at hand.  The SBQ chains start from 300 rows there, the plain one
from 200 (N0 of the modules they reuse).  The fresh-index cases of tombstones and a mask under a group rule
(tests/test_gpu_zz_grouped.py) run here too, on their own."""
import os
import subprocess
import sys

import pytest

from test_emu_qual import EMU_DIR, ROOT, emu_lib  # noqa: F401  (the fixture that builds the interpreter library)

CASES = ("(test_chain_qa and cosine) or test_chain_qb or test_chain_qp or test_chain_qd_drawn_operations[1] or "
         "test_chain_qd_drawn_operations[3]")
N_CASES = 5


def test_qualified_lifecycle_chains_pass_on_the_wave64_interpreter(emu_lib):  # noqa: F811
    env = dict(os.environ, VS_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zz_qual_lifecycle.py"), "-m", "gpu", "-x", "-q", "-p",
           "no:cacheprovider", "-k", CASES]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=3000)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert f"{N_CASES} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail


def test_tombstones_and_a_mask_under_a_group_rule_pass_on_the_wave64_interpreter(emu_lib):  # noqa: F811
    env = dict(os.environ, VS_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zz_grouped.py"), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
           "-k", "test_tombstones_and_a_mask_do_not_count_against_a_group"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=3000)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "4 passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
