"""vs_index_consolidate_deletes on the wave64 lockstep interpreter: cases 1-6 and 9 of tests/test_gpu_zw_consolidate.py re-run in a
child process against tests/emu/libvsgpu_emu.so (the unmodified kernel sources compiled for the host, see tests/test_emu.py), so
that k_consolidate_rows and the flag pass are checked against the numpy restatement where no GPU is at hand.  The 24-word index of
case 3 has 300 rows there."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")

CASES = ("test_rows_and_stats_equal_the_restatement or test_cap_keeps_the_closest_candidates or test_24_word_codes_both_forms_of_the_prune or "
         "test_a_deleted_default_start_node_stays_in_the_graph or test_a_node_whose_neighbors_are_all_deleted or "
         "test_a_whole_neighborhood_is_deleted or test_nothing_deleted_nothing_changes_and_a_second_call_rewrites_nothing or "
         "test_labeled_index_prunes_with_the_label_rule_and_keeps_label_start_nodes or "
         "test_after_the_full_call_no_kept_row_names_a_tombstone_and_scans_equal_the_oracle or test_refusals_leave_every_byte_as_it_was")


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def test_consolidation_cases_pass_on_the_wave64_interpreter(emu_lib):
    env = dict(os.environ, VS_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zw_consolidate.py"), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
           "-k", CASES]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=3000)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "13 passed" in r.stdout and "failed" not in r.stdout, tail
