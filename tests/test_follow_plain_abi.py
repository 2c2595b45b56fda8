"""vs_pages_follow_open_plain at the C ABI, without a device: the symbol is exported and bound with the arguments the header declares,
vs_pages_follow_info keeps its size, and NULL arguments are refused with a message before anything touches a device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def _declared_args(name):
    src = open(os.path.join(ROOT, "include", "vsgpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, f"{name} is not declared in include/vsgpu.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_symbol_is_exported_and_bound_with_the_declared_arguments():
    from pgvectorscale_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libvsgpu.so missing: run __graft_entry__.build()"
    L = C.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "vs_pages_follow_open_plain")
    args = _declared_args("vs_pages_follow_open_plain")
    assert len(args) == 6 and args == _declared_args("vs_pages_follow_open")  # (the plain twin takes what the SBQ call takes)
    res, bound = _lib.SYMBOLS["vs_pages_follow_open_plain"]
    assert res is C.c_int and len(bound) == len(args)
    assert bound == _lib.SYMBOLS["vs_pages_follow_open"][1]


def test_follow_info_keeps_its_size(tmp_path):
    """the struct is not changed: 10 uint32 and one uint64, 48 bytes, in the header as in the Python mirror"""
    import subprocess
    from pgvectorscale_amd import _lib
    assert C.sizeof(_lib.PagesFollowInfo) == 48
    assert [k for k, _ in _lib.PagesFollowInfo._fields_] == ["n_blocks_before", "n_blocks_now", "pages_listed", "node_pages_listed", "n_before",
                                                              "n_appended", "rows_relinked", "tids_cleared", "tids_changed", "codes_changed",
                                                              "label_vals_appended"]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vsgpu.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(vs_pages_follow_info), offsetof(vs_pages_follow_info, codes_changed), '
                   'offsetof(vs_pages_follow_info, label_vals_appended)); return 0; }\n')
    exe = tmp_path / "size"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.stdout.split() == ["48", "36", "40"], r.stdout + r.stderr


def test_null_arguments_are_refused_with_a_message():
    import pgvectorscale_amd as P
    L = P.load()
    out = C.c_void_p(0xDEAD)
    cnt = (C.c_uint32 * 2)(0, 0)
    assert L.vs_pages_follow_open_plain(None, 8192, None, cnt, 2, C.byref(out)) == INVALID
    msg = L.vs_last_error().decode()
    assert "vs_pages_follow_open_plain" in msg and "bad args" in msg
    assert L.vs_pages_follow_open_plain(None, 8192, None, cnt, 2, None) == INVALID
    assert "vs_pages_follow_open_plain" in L.vs_last_error().decode()
    with pytest.raises(P.VsError) as e:
        P._lib.check(L.vs_pages_follow_open_plain(None, 8192, None, None, 0, C.byref(out)))
    assert e.value.code == INVALID and "vs_pages_follow_open_plain" in str(e.value)
