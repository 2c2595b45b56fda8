"""vs_scanpool_info and the VS_POOL_PLAIN_FAST option as the C ABI and the documents show them (no GPU: the symbol table of the built
library, the Python binding, the argument checks that run before anything of a pool is read)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from pgvectorscale_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return C.CDLL(_lib.LIB_PATH)


def test_symbol_is_exported_and_bound(lib):
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.index import ScanPool
    assert hasattr(lib, "vs_scanpool_info")
    assert "vs_scanpool_info" in _lib.SYMBOLS
    res, args = _lib.SYMBOLS["vs_scanpool_info"]
    assert res is C.c_int and args[1] is C.POINTER(_lib.SearchInfo)
    assert callable(ScanPool.info)
    h = open(os.path.join(ROOT, "include", "vsgpu.h")).read()
    assert re.search(r"int vs_scanpool_info\(const vs_scan_pool\* pool, vs_search_info\* out\);", h)


def test_null_arguments_are_invalid(lib):
    from pgvectorscale_amd import _lib
    f = lib.vs_scanpool_info
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    info = _lib.SearchInfo()
    VS_ERR_INVALID = -1
    h = open(os.path.join(ROOT, "include", "vsgpu.h")).read()
    assert int(re.search(r"VS_ERR_INVALID = (-?\d+)", h).group(1)) == VS_ERR_INVALID
    assert f(None, C.byref(info)) == VS_ERR_INVALID
    assert f(None, None) == VS_ERR_INVALID
    not_read = C.create_string_buffer(64)  # stands in for a pool: the output pointer is checked before the pool is looked at
    assert f(C.addressof(not_read), None) == VS_ERR_INVALID


def test_option_is_documented():
    h = open(os.path.join(ROOT, "include", "vsgpu.h")).read()
    d = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^## 10\..*?(?=^## \d)", d, re.S | re.M)
    assert m, "DESIGN.md section 10"
    assert "VS_POOL_PLAIN_FAST" in h
    assert "VS_POOL_PLAIN_FAST" in m.group(0)
