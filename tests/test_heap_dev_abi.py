"""vs_heap_dev_*, vs_index_alloc_vecs and vs_pages_follow_apply_dev as the C ABI and the documents show them (no GPU: the symbol
table of the built library, the ctypes prototypes, the argument checks that run before any device call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vs_heap_dev_open", "vs_heap_dev_add", "vs_heap_dev_toast_add", "vs_heap_dev_finish", "vs_heap_dev_close", "vs_index_alloc_vecs",
       "vs_pages_follow_apply_dev")
VS_ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from pgvectorscale_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return C.CDLL(_lib.LIB_PATH)


def test_symbols_are_exported_bound_and_declared(lib):
    from pgvectorscale_amd import _lib
    h = open(os.path.join(ROOT, "include", "vsgpu.h")).read()
    assert int(re.search(r"VS_ERR_INVALID = (-?\d+)", h).group(1)) == VS_ERR_INVALID
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\b(int|void) %s\(" % name, h), name
    # the prototypes of the device reader are those of the host reader with the context in front and n_compressed behind
    assert _lib.SYMBOLS["vs_heap_dev_open"][1][1:] == _lib.SYMBOLS["vs_heap_open"][1]
    assert _lib.SYMBOLS["vs_heap_dev_add"] == _lib.SYMBOLS["vs_heap_add"] == _lib.SYMBOLS["vs_heap_dev_toast_add"]
    assert _lib.SYMBOLS["vs_heap_dev_finish"][1][:3] == _lib.SYMBOLS["vs_heap_finish"][1] and len(_lib.SYMBOLS["vs_heap_dev_finish"][1]) == 4
    assert _lib.SYMBOLS["vs_pages_follow_apply_dev"] == _lib.SYMBOLS["vs_pages_follow_apply"]


def test_python_layer_has_the_wrappers():
    from pgvectorscale_amd import index, pages
    for name in ("add", "toast_add", "finish", "close"):
        assert callable(getattr(pages.HeapColumnDev, name))
    assert callable(pages.PagesFollower.apply_dev) and callable(index.DiskAnnIndex.alloc_vecs)


def test_open_refuses_bad_arguments_before_touching_a_device(lib):
    """the checks of vs_heap_open, made before the context is looked at: the context handed in here is a block of zeroed memory"""
    from pgvectorscale_amd import _lib
    f = lib.vs_heap_dev_open
    f.restype, f.argtypes = _lib.SYMBOLS["vs_heap_dev_open"]
    ctx = C.create_string_buffer(1 << 16)  # (never dereferenced by a refused call)
    attrs = (_lib.HeapAttr * 2)(_lib.HeapAttr(4, b"i"), _lib.HeapAttr(-1, b"i"))
    tids = np.array([(1 << 16) | 1], np.uint64)
    out = C.c_void_p()
    tp, rows = tids.ctypes.data_as(C.c_void_p), C.c_void_p(4096)  # (a device pointer is not looked at either)

    def call(ctx_=ctx, page=8192, attrs_=attrs, natts=2, attno=2, dim=8, tids_=tp, n=1, rows_=rows, stride=8, out_=C.byref(out)):
        return f(ctx_, page, attrs_, natts, attno, dim, tids_, n, rows_, stride, out_)

    assert call(ctx_=None) == VS_ERR_INVALID
    assert call(attrs_=None) == VS_ERR_INVALID
    assert call(out_=None) == VS_ERR_INVALID
    assert call(tids_=None) == VS_ERR_INVALID and call(rows_=None) == VS_ERR_INVALID
    assert call(stride=7) == VS_ERR_INVALID                     # out_stride < dim
    assert call(attno=1) == VS_ERR_INVALID                      # a non-varlena vector attribute
    assert call(attno=0) == VS_ERR_INVALID and call(attno=3) == VS_ERR_INVALID
    assert call(dim=0) == VS_ERR_INVALID and call(dim=16001, stride=16001) == VS_ERR_INVALID
    for page in (0, 256, 8191, 12288, 65536):                   # a bad page size
        assert call(page=page) == VS_ERR_INVALID
    lib.vs_last_error.restype = C.c_char_p
    assert b"page size" in lib.vs_last_error()
    assert out.value is None


def test_null_handles_are_invalid(lib):
    from pgvectorscale_amd import _lib
    for name in ("vs_heap_dev_add", "vs_heap_dev_toast_add"):
        f = getattr(lib, name)
        f.restype, f.argtypes = _lib.SYMBOLS[name]
        assert f(None, 0, None, 0) == VS_ERR_INVALID
    f = lib.vs_heap_dev_finish
    f.restype, f.argtypes = _lib.SYMBOLS["vs_heap_dev_finish"]
    assert f(None, None, None, None) == VS_ERR_INVALID
    f = lib.vs_index_alloc_vecs
    f.restype, f.argtypes = _lib.SYMBOLS["vs_index_alloc_vecs"]
    assert f(None) == VS_ERR_INVALID
    f = lib.vs_pages_follow_apply_dev
    f.restype, f.argtypes = _lib.SYMBOLS["vs_pages_follow_apply_dev"]
    assert f(None, None, 0, None) == VS_ERR_INVALID
    lib.vs_heap_dev_close.restype, lib.vs_heap_dev_close.argtypes = None, [C.c_void_p]
    lib.vs_heap_dev_close(None)


def test_documents_describe_the_reader():
    for doc, words in (("README.md", ("vs_heap_dev",)), ("DESIGN.md", ("vs_heap_dev", "vs_index_alloc_vecs", "vs_pages_follow_apply_dev", "n_compressed")),
                       ("INTEGRATION.md", ("vs_heap_dev_open", "vs_index_alloc_vecs", "vs_pages_follow_apply_dev", "n_compressed"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
