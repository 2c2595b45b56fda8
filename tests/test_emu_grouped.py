"""Grouped scans on the wave64 lockstep interpreter (see tests/test_emu_qual.py): the cases of tests/test_gpu_zz_grouped.py in a child
process, the randomised ones also with the lanes highest-first and shuffled — the ballots and popcounts of the kept-group count may show no order."""
import os
import subprocess
import sys

import pytest

from test_emu_qual import EMU_DIR, ROOT, emu_lib  # noqa: F401  (the fixture that builds the interpreter library)

# states 1, rule 3 x 16, identities 2, composition 1, ties 1, fallback + replay 4, tombstones and a mask 4, plain 1, device entry 1, chunks 1,
# labels 1, insert 1, compact 1
N_CASES = 67
RANDOMISED = "test_rule and forty or test_a_tie_heavy or test_the_fallback or test_a_qualifier"
N_RANDOMISED = 16 + 1 + 4 + 1


def _run(env, *select):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zz_grouped.py"), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", *select]
    r = subprocess.run(cmd, env=dict(os.environ, VS_EMU="1", **env), capture_output=True, text=True, cwd=ROOT, timeout=3000)
    return r, (r.stdout + r.stderr)[-3000:]


@pytest.mark.parametrize("order,select,n", [(None, (), N_CASES), ("reverse", ("-k", RANDOMISED), N_RANDOMISED), ("shuffle", ("-k", RANDOMISED), N_RANDOMISED)])
def test_grouped_scan_cases_pass_on_the_wave64_interpreter(emu_lib, order, select, n):  # noqa: F811
    r, tail = _run({"VS_EMU_ORDER": order} if order else {}, *select)
    assert r.returncode == 0, tail
    assert f"{n} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
