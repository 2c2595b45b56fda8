"""The register classes of the three hot 16-bit-table units of k_search_fast, read from the built objects (scripts/codeobj_notes.py).

The resident scans of a launch — and with them every decision of the launch planning that compares them — follow from the VGPR count
of the code object: up to 64 is eight waves per SIMD, up to 72 seven, up to 80 six.  The plain unit is HELD at 72 (a launch bound of
seven waves and a register marked as used, vs_search_fast.hip FAST_WAVES); nothing else would notice a compiler that allocates
differently under that bound, so the built object is checked here.  No GPU needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import codeobj_notes  # noqa: E402

CSRC = os.path.join(ROOT, "pgvectorscale_amd", "csrc")
PLAIN6 = "k_search_fast<3, 0, false, 6, false, false, 3, 7>"
KEYS6 = "k_search_fast<3, 0, false, 6, false, true, 3, 7>"
LEAN = "k_search_fast<3, 0, false, 7, false, false, 3, 7>"


def _unit(obj, name):
    path = os.path.join(CSRC, obj)
    if not os.path.exists(path):
        pytest.fail(f"{obj} is not built (make -C pgvectorscale_amd/csrc)")
    found = [k for k in codeobj_notes.kernels(path) if name in k["demangled"]]
    assert len(found) == 1, (obj, name, [k["demangled"] for k in found])
    return found[0]


def _no_scratch(k):
    return k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0


def test_plain_unit_is_held_at_seven_waves():
    k = _unit("vs_search_fast_plain6.o", PLAIN6)
    assert k["vgpr_count"] == 72 and _no_scratch(k), k  # 28 scans per CU: not 64 (eight waves), not 76 (six)


def test_keyed_unit_keeps_six_waves():
    k = _unit("vs_search_fast_keys6.o", KEYS6)
    assert 72 < k["vgpr_count"] <= 80 and _no_scratch(k), k


def test_lean_unit_keeps_seven_waves():
    k = _unit("vs_search_fast.o", LEAN)
    assert 64 < k["vgpr_count"] <= 72 and _no_scratch(k), k
