"""vs_index_label_reach / vs_index_repair_labels / vs_nearest_masked on the wave64 lockstep interpreter: the exactness cases of
tests/test_gpu_zw_label_repair.py (1-6) re-run in a child process against tests/emu/libvsgpu_emu.so (the unmodified kernel sources
compiled for the host, see tests/test_emu.py), so that the reach sweep, the source kernel and the row edit are checked against the
numpy restatement where no GPU is at hand.  The 24-word index of case 5 has 300 rows there, the 2-word one 5 003."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")

CASES = ("test_audit_equals_the_restatement_and_the_oracles_filtered_streams or test_repair_equals_the_restatement_cell_for_cell or "
         "test_repair_after_delete_and_consolidate_equals_the_restatement or test_filtered_cursors_return_every_carrier_after_the_repair or "
         "test_seventy_labels_two_groups_and_a_label_without_a_start_node or test_nearest_masked_equals_numpy_at_the_kernels_edges or "
         "test_a_second_repair_writes_nothing_and_a_clean_index_is_untouched or test_refusals_leave_every_byte_as_it_was")


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def test_label_repair_cases_pass_on_the_wave64_interpreter(emu_lib):
    env = dict(os.environ, VS_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zw_label_repair.py"), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
           "-k", CASES]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=3000)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "18 passed" in r.stdout and "failed" not in r.stdout, tail
