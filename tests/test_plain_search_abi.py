"""vs_index_last_search_info and the VS_PLAIN_FAST / VS_PF_* options as the C ABI and the documents show them (no GPU: the symbol
table of the built library, the struct as ctypes lays it out, the argument checks that run before any device call)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS = ("VS_PLAIN_FAST", "VS_PF_HEAP_LDS", "VS_PF_HEAP_CAP", "VS_PF_DEDUP_SLOTS", "VS_PF_VISITED", "VS_PF_SCANS_PER_CU")


@pytest.fixture(scope="module")
def lib():
    from pgvectorscale_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return C.CDLL(_lib.LIB_PATH)


def test_symbol_is_exported_and_bound(lib):
    from pgvectorscale_amd import _lib
    assert hasattr(lib, "vs_index_last_search_info")
    assert "vs_index_last_search_info" in _lib.SYMBOLS
    assert (_lib.VS_SEARCH_GENERAL, _lib.VS_SEARCH_FAST_SBQ, _lib.VS_SEARCH_FAST_PLAIN) == (0, 1, 2)


def test_struct_is_32_bytes_and_matches_the_header():
    from pgvectorscale_amd import _lib
    assert C.sizeof(_lib.SearchInfo) == 32
    h = open(os.path.join(ROOT, "include", "vsgpu.h")).read()
    body = re.search(r"typedef struct vs_search_info \{(.*?)\} vs_search_info;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"uint32_t\s+([^;]+);", body) for n in decl.split(",")]
    assert names == ["kernel", "resident", "lds_bytes", "heap_lds", "dedup_slots", "visited_cap", "reserved[2]"]
    assert [f[0] for f in _lib.SearchInfo._fields_] == [n.split("[")[0] for n in names]
    assert re.search(r"VS_SEARCH_GENERAL = 0, VS_SEARCH_FAST_SBQ = 1, VS_SEARCH_FAST_PLAIN = 2", h)


def test_null_arguments_are_invalid(lib):
    from pgvectorscale_amd import _lib
    f = lib.vs_index_last_search_info
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    info = _lib.SearchInfo()
    VS_ERR_INVALID = -1
    h = open(os.path.join(ROOT, "include", "vsgpu.h")).read()
    assert int(re.search(r"VS_ERR_INVALID = (-?\d+)", h).group(1)) == VS_ERR_INVALID
    assert f(None, C.byref(info)) == VS_ERR_INVALID
    assert f(None, None) == VS_ERR_INVALID


def test_options_are_documented():
    h = open(os.path.join(ROOT, "include", "vsgpu.h")).read()
    d = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^## 10\..*?(?=^## \d)", d, re.S | re.M)
    assert m, "DESIGN.md section 10"
    for name in OPTIONS:
        assert name in h, name
        assert name in m.group(0), name
