"""The C ABI of the qualified scan-pool fetch: the entry point is exported with the prototype pgvectorscale_amd/_lib.py declares, the
new state and the record are what the header says, and the argument checks that need no device — NULL arrays, k and max_pops out of
range — refuse on a NULL pool, each naming its own cause."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


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


def test_the_entry_point_is_declared_exported_and_prototyped(lib):
    h = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    decl = re.search(r"\bint vs_scanpool_fetch_qual\(([^;]*)\);", h)
    assert decl
    params = [p.strip() for p in decl.group(1).split(",") if p.strip()]
    fn = lib.vs_scanpool_fetch_qual
    assert fn.restype is C.c_int and fn.argtypes is not None and len(fn.argtypes) == len(params) == 13
    # scalars where the header has scalars, pointers where it has pointers
    for p, t in zip(params, fn.argtypes):
        assert ("*" in p) == (t is not C.c_uint32), (p, t)
    assert params[-1].startswith("vs_pool_qual_stats*")


def test_the_new_state_and_the_record_equal_the_header():
    from pgvectorscale_amd import _lib
    h = header()
    assert int(re.search(r"#define VS_QUAL_BUDGET (\d+)", h).group(1)) == 3 == _lib.QUAL_BUDGET
    # the three states of the one-shot batch stand as they were
    assert "enum { VS_QUAL_COMPLETE = 0, VS_QUAL_ENDED = 1, VS_QUAL_CUT = 2 };" in h
    assert len({_lib.QUAL_COMPLETE, _lib.QUAL_ENDED, _lib.QUAL_CUT, _lib.QUAL_BUDGET}) == 4
    body = re.search(r"typedef struct vs_pool_qual_stats \{(.*?)\} vs_pool_qual_stats;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            assert decl.startswith("uint64_t"), decl
            fields += [f.strip() for f in decl[len("uint64_t"):].split(",")]
    assert fields == ["search_rounds", "window_launches", "first_pops", "pops", "complete", "ended", "cut", "budget"]
    assert [f[0] for f in _lib.PoolQualStats._fields_] == fields and all(f[1] is C.c_uint64 for f in _lib.PoolQualStats._fields_)
    assert C.sizeof(_lib.PoolQualStats) == 8 * len(fields)


def test_null_arrays_and_ranges_are_refused_on_a_null_pool(lib):
    """what needs no pool is checked first, so each refusal names its own cause even on a NULL handle"""
    from pgvectorscale_amd import _lib
    u = (C.c_uint32 * 8)()
    rows = (C.c_int32 * 8)()
    qst = _lib.PoolQualStats()

    def call(slots=u, k=10, qslots=u, max_pops=64, o_rows=rows, o_pops=u, o_state=u):
        return lib.vs_scanpool_fetch_qual(None, slots, 2, k, qslots, max_pops, None, None, None, o_rows, o_pops, o_state, C.byref(qst))

    for kw, cause in ((dict(slots=None), b"slots is NULL"), (dict(qslots=None), b"qual_slots is NULL"), (dict(o_rows=None), b"out_rows is NULL"),
                      (dict(o_pops=None), b"out_pops is NULL"), (dict(o_state=None), b"out_state is NULL"), (dict(k=0), b"k must be"),
                      (dict(max_pops=9), b"max_pops 9 outside"), (dict(max_pops=65537), b"max_pops 65537 outside"),
                      (dict(k=10, max_pops=10), b"pool is NULL"), (dict(max_pops=65536), b"pool is NULL")):
        assert call(**kw) == INVALID, kw
        assert cause in lib.vs_last_error(), (kw, lib.vs_last_error())
    assert all(getattr(qst, f[0]) == 0 for f in qst._fields_)
