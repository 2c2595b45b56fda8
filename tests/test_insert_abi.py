"""CPU tier of vs_index_insert: the ABI (header, ctypes table, struct size) and, on the wave64 lockstep interpreter build of the
same kernel sources (tests/emu), the batch-mates kernel at 65 rows and the findability of 63 / 65 inserted rows."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "vsgpu.h")).read()
NEW = ["vs_index_reserve", "vs_index_capacity", "vs_index_insert", "vs_index_insert_dev", "vs_index_insert_kernel_ms", "vs_batch_mates", "vs_batch_mates_filtered",
       "vs_index_repair"]


def _c_args(name):
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", HEADER, re.S)
    assert m, f"{name} is not declared in include/vsgpu.h"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [a.strip() for a in args.split(",") if a.strip() and a.strip() != "void"]


@pytest.mark.parametrize("name", NEW)
def test_symbol_is_declared_and_bound_with_the_same_arity_and_kinds(name):
    from pgvectorscale_amd import _lib
    assert name in _lib.SYMBOLS
    res, args = _lib.SYMBOLS[name]
    cargs = _c_args(name)
    assert len(cargs) == len(args), (cargs, args)
    for ca, pa in zip(cargs, args):
        if "*" in ca:
            assert pa is C.c_void_p or hasattr(pa, "contents") or pa is C.c_char_p, (ca, pa)
        elif ca.startswith("double"):
            assert pa is C.c_double
        elif ca.startswith("uint32_t"):
            assert pa is C.c_uint32
        elif ca.startswith("int"):
            assert pa is C.c_int
    assert res is (C.c_uint32 if name == "vs_index_capacity" else C.c_int)


def test_insert_stats_has_the_same_layout_in_c_and_ctypes():
    from pgvectorscale_amd import _lib
    m = re.search(r"typedef struct vs_insert_stats \{(.*?)\} vs_insert_stats;", HEADER, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            assert decl.startswith("uint32_t ")
            fields += [f.strip() for f in decl[len("uint32_t "):].split(",")]
    assert fields == [k for k, _ in _lib.InsertStats._fields_]
    assert C.sizeof(_lib.InsertStats) == 4 * len(fields) == 32


def test_python_surface():
    import pgvectorscale_amd as P
    for name in ("reserve", "capacity", "insert", "batch_mates", "repair"):
        assert hasattr(P.DiskAnnIndex, name)


def test_insert_kernels_on_the_wave64_interpreter():
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    emu = os.path.join(ROOT, "tests", "emu")
    r = subprocess.run(["make", "-C", emu, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    sel = "(test_batch_mates_match_the_numpy_twin and 65) or (test_every_inserted_row_is_found_and_anchored and (63 or 65))"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zv_insert.py"), "-m", "gpu", "-q", "-p",
                        "no:cacheprovider", "-k", sel], env=dict(os.environ, VS_EMU="1"), capture_output=True, text=True, cwd=ROOT,
                       timeout=1200)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and "3 passed" in r.stdout, tail
