"""The visibility base, its overlays and the searches that name a slot per scan on the wave64 lockstep interpreter: the cases of
tests/test_gpu_zx_vis_overlay.py re-run in a child process against tests/emu/libvsgpu_emu.so (the unmodified kernel sources compiled
for the host, see tests/test_emu.py), under guard pages behind every device allocation.  The randomised cases are repeated with the
lanes scheduled highest-first and in shuffled order: the depends list is filled through an atomic counter and sorted before anything
reads it, so no class, list position, overlay or row may depend on the order."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
# classes and list (3), materialized masks (3), the mixed launch (2), other regimes (4), host chunks (1), label keys (1), a plain index
# (2), device slots (1), rescore 0 (1), refresh (1), refusals (1), a malformed page (1), inserted rows (1), compaction (1), the legacy
# path (1), the broker (1)
N_CASES = 25
RANDOMISED = "test_classes_list or test_materialized or test_mixed_launch_equals or test_refresh"
N_RANDOMISED = 9


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def _run(env, *select):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zx_vis_overlay.py"), "-m", "gpu", "-x", "-q", "-p",
           "no:cacheprovider", *select]
    r = subprocess.run(cmd, env=dict(os.environ, VS_EMU="1", **env), capture_output=True, text=True, cwd=ROOT, timeout=3000)
    return r, (r.stdout + r.stderr)[-3000:]


def test_vis_overlay_cases_pass_on_the_wave64_interpreter(emu_lib):
    r, tail = _run({})
    assert r.returncode == 0, tail
    assert f"{N_CASES} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail


@pytest.mark.parametrize("order", ["reverse", "shuffle"])
def test_randomised_cases_under_other_lane_orders(emu_lib, order):
    r, tail = _run({"VS_EMU_ORDER": order}, "-k", RANDOMISED)
    assert r.returncode == 0, tail
    assert f"{N_RANDOMISED} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
