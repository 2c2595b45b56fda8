"""The C ABI of the visibility base, its overlays and the searches that name slots: every entry point is exported with the prototype
pgvectorscale_amd/_lib.py declares, the public constants are what the header says, and the argument checks that need no device —
NULL handles, slots and snapshot ids out of range — refuse before anything else is looked at."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
ENTRY_POINTS = ("vs_index_vis_base_eval", "vs_index_vis_base_drop", "vs_index_vis_base_info", "vs_index_vis_slot_eval",
                "vs_index_vis_slot_patch", "vs_index_vis_slot_drop", "vs_index_vis_materialize", "vs_index_vis_share",
                "vs_search_batch_vis", "vs_search_batch_dev_vis", "vs_search_batch_dev_vis_finish", "vs_broker_search_vis",
                "vs_broker_call_exclusive")


@pytest.fixture(scope="module")
def lib():
    from pgvectorscale_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):  # (a library that is absent is built, and one that cannot be built fails the tests)
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def header():
    with open(os.path.join(ROOT, "include", "vsgpu.h")) as f:
        return f.read()


def test_every_entry_point_is_declared_exported_and_prototyped(lib):
    h = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in ENTRY_POINTS:
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", h)
        assert decl, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes is not None, name
        n_params = len([p for p in decl.group(1).split(",") if p.strip()])
        assert len(fn.argtypes) == n_params, (name, len(fn.argtypes), n_params)


def test_constants_and_the_stats_struct():
    from pgvectorscale_amd import _lib
    h = header()
    assert int(re.search(r"#define VS_MAX_VIS_SLOTS (\d+)", h).group(1)) >= 1024
    body = re.search(r"typedef struct vs_vis_base_stats \{(.*?)\} vs_vis_base_stats;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    words = 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        assert decl.startswith("uint64_t"), decl
        for field in decl[len("uint64_t"):].split(","):
            m = re.match(r"\s*\w+(?:\[(\w+)\])?\s*$", field)
            assert m, field
            words += {None: 1, "3": 3, "VS_VIS_R_N": len(_lib.VIS_REASONS)}[m.group(1)]
    assert C.sizeof(_lib.VisBaseStats) == 8 * words
    assert [f[0] for f in _lib.VisBaseStats._fields_][:2] == ["n_class", "r"] and _lib.VisBaseStats._fields_[-1][0] == "chain_hops"


def test_null_handles_and_ranges_are_refused(lib):
    x = C.c_uint32(0)
    assert lib.vs_index_vis_base_eval(None, None, 100, None, None, 0, None) == INVALID
    assert b"index is NULL" in lib.vs_last_error()
    assert lib.vs_index_vis_base_drop(None) == INVALID
    assert lib.vs_index_vis_base_info(None, None, None, None, 0) == INVALID
    assert lib.vs_index_vis_slot_eval(None, None, 1, None, None, None, None, 0, None) == INVALID
    assert lib.vs_index_vis_slot_patch(None, 1, None, None, 0) == INVALID
    assert lib.vs_index_vis_slot_drop(None, 1) == INVALID
    assert lib.vs_index_vis_materialize(None, 1, 1) == INVALID
    assert lib.vs_index_vis_share(None, None) == INVALID
    assert lib.vs_search_batch_vis(None, None, None, None, None, 0, 10, 5, 10, None, None, None, None) == INVALID
    assert lib.vs_search_batch_dev_vis(None, None, None, None, None, 0, 10, 5, 10, None, None, None) == INVALID
    assert lib.vs_search_batch_dev_vis_finish(None, None) == INVALID
    assert lib.vs_broker_search_vis(None, None, None, 0, 0, 10, 5, 10, 1, C.byref(x), None, None) == INVALID
    assert lib.vs_broker_call_exclusive(None, None, None) == INVALID
