"""The exact and the flat qualified top-k under a group rule on the wave64 lockstep interpreter (see tests/test_emu_qual_exact.py): the
cases of tests/test_gpu_zz_qual_exact_grouped.py in a child process, the randomised ones also with the lanes highest-first and shuffled
— a list place and the replaced entry of a group are popcounts and ballots over the lanes, nothing may depend on their order."""
import os
import subprocess
import sys

import pytest

from test_emu_qual import EMU_DIR, ROOT, emu_lib  # noqa: F401  (the fixture that builds the interpreter library)

RANDOMISED = "test_rule or test_forced or test_flat_grouped"


def _run(env, *select):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zz_qual_exact_grouped.py"), "-m", "gpu", "-x", "-q", "-p",
           "no:cacheprovider", *select]
    r = subprocess.run(cmd, env=dict(os.environ, VS_EMU="1", **env), capture_output=True, text=True, cwd=ROOT, timeout=3000)
    return r, (r.stdout + r.stderr)[-3000:]


@pytest.mark.parametrize("order,select", [(None, ()), ("reverse", ("-k", RANDOMISED)), ("shuffle", ("-k", RANDOMISED))],
                         ids=["default", "reverse", "shuffle"])
def test_grouped_exact_and_flat_cases_pass_on_the_wave64_interpreter(emu_lib, order, select):  # noqa: F811
    r, tail = _run({"VS_EMU_ORDER": order} if order else {}, *select)
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
