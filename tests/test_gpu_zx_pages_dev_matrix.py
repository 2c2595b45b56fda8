"""vs_pages_dev_* held to the host reader, good pages and bad (the cases live in tests/pages_dev_checks.py): the wave-strided loops of
k_pages_decode and k_pages_labels past their first trip (W, R and label counts on both sides of 64 and 128), the end of a neighbor
list at every lane around a wave boundary, every refusal reason the two kernels can give — each by one change to one item, at node
40, at the last item of the last node page and at the item that ends eight bytes from the end of the staged buffer — custom node
layouts, relations of no and of one node, feeds in 1, 3 and n_blocks calls, wrong geometry and call-sequence errors.  Expectations
are the source arrays and the host reader (vs_pages.cpp) over the same bytes, compared exactly.  The malformed pages are in-range
fabricated bytes that must end in an error code: the file runs on the lockstep interpreter first (tests/test_emu_pages_dev.py), where
every device allocation ends at a guard page.  (Sorted late in the GPU tier like tests/test_gpu_zx_pages_dev.py.)"""
import pytest

import pages_dev_checks as PC

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]


@pytest.mark.parametrize("case", list(PC.GOOD))
def test_differential(gpu_ctx, oracle, case):
    """device arrays == source arrays == host reader's arrays; node_of; the quantizer; 8 scans return the oracle's rows where the shape
    has vectors.  one_trip: n 300, W 4, R 32, three never-initialised blocks, means behind the nodes | w64, w65: W on both sides of a
    wave | w_long: W 250, 0..3 labels, the means chain | r64 .. r130: R on both sides of one and two waves, half the rows full, degrees
    around every wave boundary | many_labels: 0, 1, 63, 64, 65, 130 labels in rotation, 200 distinct values of both signs (no mask
    path: the CSR is checked) | empty_sets: a labeled relation of empty sets | layout: (40, 32, 16, 0, 8), refused under the default
    layout | tiny: n 1 | no_nodes: n 0 builds an empty index, as the host reader does | chunks: 1, 3 and n_blocks calls of add."""
    PC.GOOD[case](gpu_ctx, oracle)


@pytest.mark.parametrize("slot", PC.LIST_END_SLOTS)
def test_neighbor_list_ends_at_first_invalid_pointer(gpu_ctx, oracle, slot):
    """R = 130, node 7 full: InvalidBlockNumber in `slot` ends the list, the pointer at the meta page behind it is ignored, not
    reported; row 7 is the source row up to `slot` and sentinel from there, every other row untouched, the host reader agrees."""
    PC.case_list_end(slot)(gpu_ctx, oracle)


@pytest.mark.parametrize("where", list(PC.MAL_NODES))
@pytest.mark.parametrize("name", list(PC.MALFORMED))
def test_malformed(gpu_ctx, oracle, name, where):
    """one change to one item: VsError naming the block, the item and the reason of PC.MALFORMED; the host reader's verdict on the same
    bytes; the handle closes; a good build on the same context follows"""
    PC.case_malformed(name, where)(gpu_ctx, oracle)


@pytest.mark.parametrize("case", list(PC.SEQUENCE))
def test_wrong_geometry_and_call_sequence(gpu_ctx, oracle, case):
    """words / num_neighbors the pages contradict, has_labels over classic nodes, add after build, add past n_blocks_total, add out
    of order, a second build: refused with the reason, nothing of a refused index left allocated (counted on the interpreter)"""
    PC.SEQUENCE[case](gpu_ctx, oracle)
