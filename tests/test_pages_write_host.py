"""The host half of the page writer (vs_pages_out_*): vs_meta_page_encode is held, byte for byte, to the oracle's restatement of
rkyv::to_bytes::<MetaPage> (oracle/pages_py.py::rkyv_meta_page, B-tree included) and round-trips through vs_meta_page_decode; the
device half (k_pages_encode, tests/test_gpu_zzzz_pages_write.py) runs here on the wave64 lockstep interpreter."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from oracle import pages_py as PG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")

PERMUTED = ("max_alpha", "start_nodes", "quantizer_metadata", "extension_version_when_built", "magic_number", "version",
            "num_dimensions", "num_dimensions_to_index", "num_neighbors", "search_list_size", "distance_type",
            "bq_num_bits_per_dimension", "storage_type", "has_labels")

CASES = {
    "no_start_nodes": dict(num_dimensions=768),
    "default_start_only": dict(num_dimensions=1536, num_dimensions_to_index=512, bq_num_bits_per_dimension=1, distance_type=0,
                               num_neighbors=64, search_list_size=77, max_alpha=1.35, default_start=(3, 9), quantizer=(1, 1)),
    "inline_version_7_bytes": dict(num_dimensions=96, extension_version="0.8.0-a", default_start=(7, 1), labeled_starts={5: (9, 2)},
                                   has_labels=True),
    "long_version": dict(num_dimensions=128, extension_version="0.8.0-rc1+build.77", default_start=(7, 1),
                         labeled_starts={5: (9, 2), -3: (11, 4)}, has_labels=True, quantizer=(1, 1)),
    "600_labeled_starts": dict(num_dimensions=64, default_start=(2, 2), has_labels=True, extension_version="0.8.0-long-version",
                               labeled_starts={l: (9 + l, 1 + l % 50) for l in range(600)}),
    "all_smallints": dict(num_dimensions=64, default_start=(2, 2), has_labels=True, quantizer=(1, 1),
                          labeled_starts={l: (40000 + l, 1 + (l % 7)) for l in range(-32768, 32768)}),
    "permuted_layout": dict(num_dimensions=100, default_start=(4, 4), labeled_starts={l: (405 + l, 5) for l in range(-400, 400)},
                            has_labels=True, max_alpha=1.0625, layout=PG.meta_layout(PERMUTED), quantizer=(1, 1)),
    "starts_without_a_default": dict(num_dimensions=64, labeled_starts={1: (5, 5)}),  # Option<StartNodes> = None: nothing is written
}


def _fields(kw):
    """the keyword arguments of PG.rkyv_meta_page as the fields of vs_meta_page"""
    ds = kw.get("default_start")
    q = kw.get("quantizer", (PG.INVALID_BLOCK, PG.INVALID_OFFSET))
    return dict(magic_number=PG.TSV_MAGIC_NUMBER, version=PG.TSV_VERSION, extension_version_when_built=kw.get("extension_version", "0.8.0"),
                distance_type=kw.get("distance_type", 1), num_dimensions=kw["num_dimensions"],
                num_dimensions_to_index=kw.get("num_dimensions_to_index", kw["num_dimensions"]),
                bq_num_bits_per_dimension=kw.get("bq_num_bits_per_dimension", 2), storage_type=kw.get("storage_type", 2),
                num_neighbors=kw.get("num_neighbors", 50), search_list_size=kw.get("search_list_size", 100),
                max_alpha=kw.get("max_alpha", 1.2), has_start_nodes=int(ds is not None),
                default_start_block=PG.INVALID_BLOCK if ds is None else ds[0], default_start_offset=0 if ds is None else ds[1],
                quantizer_block=q[0], quantizer_offset=q[1], has_labels=int(bool(kw.get("has_labels"))))


@pytest.mark.parametrize("name", list(CASES))
def test_meta_page_encode_is_the_oracles_archive_byte_for_byte(name):
    from pgvectorscale_amd.pages import decode_meta_page, encode_meta_page
    kw = CASES[name]
    want = PG.rkyv_meta_page(**kw)
    lay = kw.get("layout")
    if name == "600_labeled_starts":  # precondition: this input makes the B-tree's root an inner node (two leaves under it)
        sn = len(want) - PG.DEFAULT_META_LAYOUT["root_size"] + PG.DEFAULT_META_LAYOUT["start_nodes"]
        rootnode = sn + 16 + struct.unpack_from("<i", want, sn + 16)[0]
        assert struct.unpack_from("<H", want, rootnode)[0] & 0x8000
    got = encode_meta_page(_fields(kw), kw.get("labeled_starts"), layout=lay)
    assert len(got) == len(want)
    assert got == want
    # ... and back through the decoder: every field and every start node
    f, starts = decode_meta_page(got, layout=lay)
    src = _fields(kw)
    for k, v in src.items():
        if k in ("default_start_block", "default_start_offset") and not src["has_start_nodes"]:
            continue
        assert f[k] == v, k
    expect = (kw.get("labeled_starts") or {}) if src["has_start_nodes"] else {}
    assert starts == expect and f["n_labeled_start_nodes"] == len(expect)
    assert PG.parse_meta_page(got, layout=lay or PG.DEFAULT_META_LAYOUT)["labeled_starts"] == expect


def test_meta_page_encode_reports_the_needed_length_and_respects_cap():
    import ctypes as C

    from pgvectorscale_amd import VsError, _lib
    from pgvectorscale_amd._lib import MetaPage, check
    L = _lib.load()
    kw = CASES["600_labeled_starts"]
    want = PG.rkyv_meta_page(**kw)
    m = MetaPage()
    for k, v in _fields(kw).items():
        setattr(m, k, v.encode() if isinstance(v, str) else v)
    ls = sorted(kw["labeled_starts"].items())
    lab = np.array([k for k, _ in ls], np.int16)
    blk = np.array([v[0] for _, v in ls], np.uint32)
    off = np.array([v[1] for _, v in ls], np.uint32)
    args = (C.byref(m), lab.ctypes.data_as(C.c_void_p), blk.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), len(ls), None)
    n = C.c_size_t(0)
    check(L.vs_meta_page_encode(*args, None, 0, C.byref(n)))  # query
    assert n.value == len(want)
    cap = 1000
    buf = np.full(len(want) + 64, 0xAB, np.uint8)
    n = C.c_size_t(0)
    with pytest.raises(VsError):
        check(L.vs_meta_page_encode(*args, buf.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
    assert n.value == len(want)
    assert (buf[cap:] == 0xAB).all(), "bytes written past cap"
    check(L.vs_meta_page_encode(*args, buf.ctypes.data_as(C.c_void_p), len(want), C.byref(n)))  # exactly enough
    assert buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAB).all()
    # unsorted keys are refused
    lab[3], lab[4] = lab[4], lab[3]
    with pytest.raises(VsError):
        check(L.vs_meta_page_encode(*args, None, 0, C.byref(n)))


def test_page_writer_passes_on_the_wave64_interpreter():
    """k_pages_encode and the whole vs_pages_out_* path, from the unmodified kernel source, on the lockstep interpreter: every case
    of tests/test_gpu_zzzz_pages_write.py in a child process with VS_EMU=1 (built the way tests/test_emu.py builds it)"""
    if os.environ.get("VS_EMU"):
        pytest.skip("already inside the emulated run")
    r = subprocess.run(["make", "-C", EMU_DIR, "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, VS_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_zzzz_pages_write.py"), "-m", "gpu", "-x", "-q",
           "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=3000)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, tail
