"""vs_heap_res_*, vs_heap_res_visibility and vs_index_snapshot_eval / _put_dev / _patch as the C ABI and the documents show them (no
GPU: the symbol table of the built library, the ctypes prototypes, the argument checks that run before any device call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vs_heap_res_open", "vs_heap_res_put", "vs_heap_res_blocks", "vs_heap_res_close", "vs_heap_res_visibility", "vs_index_snapshot_eval",
       "vs_index_snapshot_put_dev", "vs_index_snapshot_patch")
VS_ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from pgvectorscale_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        f = getattr(L, name)
        f.restype, f.argtypes = _lib.SYMBOLS[name]
    L.vs_last_error.restype = C.c_char_p
    return L


def test_symbols_are_exported_bound_and_declared(lib):
    from pgvectorscale_amd import _lib
    h = open(os.path.join(ROOT, "include", "vsgpu.h")).read()
    assert int(re.search(r"VS_ERR_INVALID = (-?\d+)", h).group(1)) == VS_ERR_INVALID
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\b(int|void|uint32_t) %s\(" % name, h), name
    # put takes what vs_heap_dev_add takes; the evaluation on an index is the one on a fork less the two device arrays
    assert _lib.SYMBOLS["vs_heap_res_put"] == _lib.SYMBOLS["vs_heap_dev_add"]
    a, b = _lib.SYMBOLS["vs_heap_res_visibility"][1], _lib.SYMBOLS["vs_index_snapshot_eval"][1]
    assert a[3:5] == b[3:5] and a[6:] == b[5:] and len(a) == 10 and len(b) == 9
    assert _lib.SYMBOLS["vs_index_snapshot_put_dev"] == _lib.SYMBOLS["vs_index_snapshot_put"]


def test_structures_match_the_header():
    """field order and the reasons' order as include/vsgpu.h declares them; the sizes a C compiler gives them on x86-64"""
    from pgvectorscale_amd import _lib
    h = open(os.path.join(ROOT, "include", "vsgpu.h")).read()
    reasons = re.search(r"enum \{ (VS_VIS_R_MULTIXACT.*?), VS_VIS_R_N \};", h).group(1).split(", ")
    assert tuple(r[len("VS_VIS_R_"):].lower() for r in reasons) == _lib.VIS_REASONS
    snap = re.search(r"typedef struct vs_mvcc_snapshot \{(.*?)\} vs_mvcc_snapshot;", h, re.S).group(1)
    order = [m for m in re.findall(r"\b(xmin|xmax|xip|xcnt|subxip|subxcnt|suboverflowed|taken_during_recovery|own_xids|n_own|curcid)\b[,;]", snap)]
    assert order == [k for k, _ in _lib.MvccSnapshot._fields_]
    assert C.sizeof(_lib.MvccSnapshot) == 64 and C.sizeof(_lib.XactStatus) == 16 and C.sizeof(_lib.VisStats) == 8 * (7 + len(_lib.VIS_REASONS))
    st = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct vs_vis_stats \{(.*?)\} vs_vis_stats;", h, re.S).group(1))
    names = re.findall(r"\b(n_visible|n_invisible|n_undecided|n_deleted|n_not_found|n_dead_line_pointer|chain_hops|undecided_by_reason)\b", st)
    assert names == [k for k, _ in _lib.VisStats._fields_]


def test_python_layer_has_the_wrappers():
    from pgvectorscale_amd import index, pages
    for name in ("put", "blocks", "visibility", "close"):
        assert callable(getattr(pages.HeapResident, name))
    for name in ("snapshot_eval", "snapshot_put_dev", "snapshot_patch"):
        assert callable(getattr(index.DiskAnnIndex, name))


def test_vis_args_builds_the_c_form():
    from pgvectorscale_amd import _lib
    s, x, keep = _lib.vis_args(dict(xmin=10, xmax=20, xip=[15, 12], own_xids=[17], curcid=3, suboverflowed=True), (8, 16, np.zeros(4, np.uint8)))
    assert (s.xmin, s.xmax, s.xcnt, s.subxcnt, s.n_own, s.curcid, s.suboverflowed, s.taken_during_recovery) == (10, 20, 2, 0, 1, 3, 1, 0)
    assert s.subxip is None and np.ctypeslib.as_array(C.cast(s.xip, C.POINTER(C.c_uint32)), (2,)).tolist() == [15, 12]
    assert (x.first_xid, x.n_xids) == (8, 16)
    with pytest.raises(ValueError):
        _lib.vis_args(dict(xmin=10, xmax=20), (8, 17, np.zeros(4, np.uint8)))


def test_open_and_put_refuse_bad_arguments_before_touching_a_device(lib):
    """the checks of vs_heap_dev_open / _add, made before the context is looked at: the context handed in here is zeroed memory"""
    ctx = C.create_string_buffer(1 << 16)
    out = C.c_void_p()
    assert lib.vs_heap_res_open(None, 8192, 4, C.byref(out)) == VS_ERR_INVALID
    assert lib.vs_heap_res_open(ctx, 8192, 4, None) == VS_ERR_INVALID
    for page in (0, 256, 8191, 12288, 65536):
        assert lib.vs_heap_res_open(ctx, page, 4, C.byref(out)) == VS_ERR_INVALID
    assert b"page size" in lib.vs_last_error()
    assert lib.vs_heap_res_open(ctx, 8192, 4, C.byref(out)) == VS_ERR_INVALID  # (zeroed staging buffers hold no page)
    assert out.value is None
    assert lib.vs_heap_res_put(None, 0, None, 0) == VS_ERR_INVALID
    assert lib.vs_heap_res_blocks(None) == 0
    lib.vs_heap_res_close(None)


def test_evaluations_refuse_bad_arguments_before_touching_a_device(lib):
    from pgvectorscale_amd import _lib
    res = C.create_string_buffer(1 << 12)  # (a handle is not looked at by a refused call)
    dev = C.c_void_p(4096)
    xip = np.array([5], np.uint32)
    bits = np.zeros(4, np.uint8)
    und = np.zeros(4, np.uint32)

    def call(h=res, tids=dev, n=4, snap="ok", xact="ok", vis=dev, und_=und.ctypes.data_as(C.c_void_p), cap=4, **kw):
        s = _lib.MvccSnapshot(3, 9, xip.ctypes.data_as(C.c_void_p), 1, None, 0, 0, 0, None, 0, 0)
        x = _lib.XactStatus(0, 16, bits.ctypes.data_as(C.c_void_p))
        for k, v in kw.items():
            setattr(s if hasattr(s, k) else x, k, v)
        return lib.vs_heap_res_visibility(h, tids, n, C.byref(s) if snap else None, C.byref(x) if xact else None, vis, None, und_, cap, None)

    assert call(h=None) == VS_ERR_INVALID
    assert call(tids=None) == VS_ERR_INVALID and call(vis=None) == VS_ERR_INVALID
    assert call(snap=None) == VS_ERR_INVALID and call(xact=None) == VS_ERR_INVALID
    assert call(n=0x80000000) == VS_ERR_INVALID
    assert call(xip=None) == VS_ERR_INVALID and call(subxcnt=2) == VS_ERR_INVALID and call(n_own=1) == VS_ERR_INVALID
    assert call(first_xid=6) == VS_ERR_INVALID and b"multiple of 4" in lib.vs_last_error()
    assert call(bits=None) == VS_ERR_INVALID
    assert call(und_=None) == VS_ERR_INVALID and b"undecided_nodes" in lib.vs_last_error()
    # on an index: the snapshot id first, as vs_index_snapshot_put checks it
    ix = C.create_string_buffer(1 << 16)
    for sid in (0, 16):
        assert lib.vs_index_snapshot_eval(ix, res, sid, None, None, None, None, 0, None) == VS_ERR_INVALID
        assert lib.vs_index_snapshot_put_dev(ix, sid, dev) == VS_ERR_INVALID
        assert lib.vs_index_snapshot_patch(ix, sid, None, None, 0) == VS_ERR_INVALID
        assert b"snapshot id" in lib.vs_last_error()
    for f, args in ((lib.vs_index_snapshot_eval, (res, 1, None, None, None, None, 0, None)), (lib.vs_index_snapshot_put_dev, (1, dev)),
                    (lib.vs_index_snapshot_patch, (1, None, None, 0))):
        assert f(None, *args) == VS_ERR_INVALID
    assert lib.vs_index_snapshot_eval(ix, None, 1, None, None, None, None, 0, None) == VS_ERR_INVALID


def test_documents_describe_the_evaluation():
    for doc, words in (("README.md", ("vs_heap_res", "vs_index_snapshot_eval")),
                       ("DESIGN.md", ("6k", "7o", "vs_heap_res_put", "k_heap_vis", "vs_index_snapshot_eval", "vs_index_snapshot_patch", "undecided")),
                       ("INTEGRATION.md", ("vs_heap_res_open", "vs_heap_res_put", "vs_index_snapshot_eval", "vs_index_snapshot_patch",
                                           "vs_index_snapshot_put_dev"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
