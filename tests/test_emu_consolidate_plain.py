"""vs_index_consolidate_deletes_plain on the wave64 lockstep interpreter: cases 1-5, 7 and 8 of tests/test_gpu_zw_consolidate_plain.py
re-run in a child process against tests/emu/libvsgpu_emu.so (the unmodified kernel sources compiled for the host, see
tests/test_emu.py), so that the plain form of k_consolidate_rows and the path up to DiskAnnIndex.consolidate_deletes(plain=True) are
checked against the numpy restatement where no GPU is at hand.  Nothing is shrunk: the shapes are those of the GPU run."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")

CASES = ("test_rows_and_counters_equal_the_restatement or test_geometry_edges or test_ties_and_zero_distances or "
         "test_a_deleted_default_start_node_stays_in_the_graph or test_a_node_whose_neighbors_are_all_deleted or "
         "test_a_whole_neighborhood_is_deleted or test_nothing_deleted_nothing_changes_and_a_second_call_rewrites_nothing or "
         "test_after_the_full_call_compaction_cuts_nothing_and_scans_equal_the_oracle or test_an_uploaded_plain_index_is_accepted or "
         "test_refusals_leave_every_byte_as_it_was")
N_CASES = 4 + 12 + 2 + 4 + 2 + 2 + 1  # cases 1, 2, 3, 4, 5, 7, 8


@pytest.fixture(scope="module")
def emu_lib():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EMU_DIR, "libvsgpu_emu.so")


def test_plain_consolidation_cases_pass_on_the_wave64_interpreter(emu_lib):
    env = dict(os.environ, VS_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zw_consolidate_plain.py"), "-m", "gpu", "-x", "-q", "-p",
           "no:cacheprovider", "-k", CASES]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=3000)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert f"{N_CASES} passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
