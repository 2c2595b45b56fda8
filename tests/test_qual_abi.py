"""The C ABI of the qualifiers and the qualified batches: every entry point is exported with the prototype pgvectorscale_amd/_lib.py
declares, the public constants and records are what the header says, and the argument checks that need no device — NULL handles, NULL
slots, slots out of range — refuse before anything else is looked at."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
ENTRY_POINTS = ("vs_index_qual_put", "vs_index_qual_put_dev", "vs_index_qual_from_tids", "vs_index_qual_from_tids_dev", "vs_index_qual_info",
                "vs_index_qual_get", "vs_index_qual_drop", "vs_search_batch_qual", "vs_search_batch_dev_qual", "vs_search_batch_dev_qual_finish")


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


def _u64_fields(h, name):
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            assert decl.startswith("uint64_t"), decl
            fields += [f.strip() for f in decl[len("uint64_t"):].split(",")]
    return fields


def test_constants_and_records_equal_the_header():
    from pgvectorscale_amd import _lib
    h = header()
    assert int(re.search(r"#define VS_MAX_QUAL_SLOTS (\d+)", h).group(1)) == _lib.MAX_QUAL_SLOTS == 64
    assert int(re.search(r"#define VS_QUAL_MAX_POPS (\d+)", h).group(1)) == _lib.QUAL_MAX_POPS == 65536
    states = re.search(r"enum \{ VS_QUAL_COMPLETE = (\d+), VS_QUAL_ENDED = (\d+), VS_QUAL_CUT = (\d+) \};", h)
    assert tuple(int(v) for v in states.groups()) == (_lib.QUAL_COMPLETE, _lib.QUAL_ENDED, _lib.QUAL_CUT) == (0, 1, 2)
    for rec, struct in (("vs_qual_info", _lib.QualInfo), ("vs_qual_batch_stats", _lib.QualBatchStats)):
        fields = _u64_fields(h, rec)
        assert [f[0] for f in struct._fields_] == fields, rec
        assert C.sizeof(struct) == 8 * len(fields), rec


def test_null_handles_slots_and_pop_limits_are_refused(lib):
    """what needs no index is checked first, so each refusal names its own cause even on a NULL handle"""
    from pgvectorscale_amd import _lib
    w = (C.c_uint64 * 4)()
    info = _lib.QualInfo()
    for slot, cause in ((0, b"slot 0 outside"), (65, b"slot 65 outside"), (1, b"index is NULL")):
        for call in (lambda: lib.vs_index_qual_put(None, slot, w), lambda: lib.vs_index_qual_put_dev(None, slot, w),
                     lambda: lib.vs_index_qual_from_tids(None, slot, w, 4, C.byref(info)),
                     lambda: lib.vs_index_qual_from_tids_dev(None, slot, w, 4, C.byref(info)),
                     lambda: lib.vs_index_qual_info(None, slot, C.byref(info)), lambda: lib.vs_index_qual_get(None, slot, w),
                     lambda: lib.vs_index_qual_drop(None, slot)):
            assert call() == INVALID
            assert cause in lib.vs_last_error(), (slot, lib.vs_last_error())
    assert lib.vs_index_qual_info(None, 1, None) == INVALID and b"info is NULL" in lib.vs_last_error()
    assert lib.vs_index_qual_get(None, 1, None) == INVALID and b"bits is NULL" in lib.vs_last_error()
    slots = (C.c_uint32 * 2)()
    out = (C.c_uint32 * 64)()
    host = lambda sl, k, max_pops: lib.vs_search_batch_qual(None, None, None, None, 0, 10, 5, k, sl, max_pops, out, None, None, out, out, out, None, None)  # noqa: E731
    dev = lambda sl, k, max_pops: lib.vs_search_batch_dev_qual(None, None, None, None, 0, 10, 5, k, sl, max_pops, out, None, None, out, out, out)  # noqa: E731
    for call in (host, dev):
        assert call(None, 10, 64) == INVALID and b"qual_slots is NULL" in lib.vs_last_error()
        assert call(slots, 10, 9) == INVALID and b"max_pops 9 outside" in lib.vs_last_error()
        assert call(slots, 10, 65537) == INVALID and b"max_pops 65537 outside" in lib.vs_last_error()
        assert call(slots, 0, 64) == INVALID and b"k must be" in lib.vs_last_error()
        assert call(slots, 10, 10) == INVALID and b"index is NULL" in lib.vs_last_error()
        assert call(slots, 10, 65536) == INVALID and b"index is NULL" in lib.vs_last_error()
    assert lib.vs_search_batch_dev_qual_finish(None, None, None) == INVALID and b"index is NULL" in lib.vs_last_error()
