"""The 16-bit dedup tables at bucket counts that are no power of two (the fitted tables of the big indexes: the cut of a hashed id
into bucket and entry is a division by a constant of the launch, csrc/vs_q16.h).  The dedup set is exact whatever its geometry, so every
table size, crossed with the switches that change what surrounds the table, must give the oracle's stream bit for bit — ids, Hamming
distances, work counters, search rows, distance bits — on the two indexes of test_gpu_regimes.py, on the compile-time geometry of the
headline width, and through a scan pool whose planned table is no power of two."""
import os
import re

import numpy as np
import pytest

import pgvectorscale_amd as P
from pgvectorscale_amd import _lib
from helpers import cached_index
from test_gpu_regimes import INDEXES

pytestmark = pytest.mark.gpu

BASE = {"VS_F_LDS_MAX_INS": "0", "VS_F_VIRGIN": "3", "VS_F_SLOTMAP_FORCE": "1"}
GCAPS = (1280, 2304, 3328, 5120, 6144)  # 160, 288, 416, 640, 768 buckets
CROSS = {
    "full_buckets": {"VS_F_GLOAD_PCT": "90"},  # overflow inserts and lookups
    "one_wg_per_scan": {"VS_F_PERSIST": "0"},
    "ring": {"VS_F_VR": "0"},
    "heap_top_1023": {"VS_F_HL": "1023"},
    "heap_spill": {"VS_F_HL": "63"},
    "seven_waves": {"VS_F_MINW": "7"},
}
COUNTERS = ("visited_nodes", "candidate_nodes", "quantized_distance_comparisons", "node_reads", "next_calls")


def _hardware_unverified(name):
    """as test_gpu_regimes.py: a variant newer than its first hardware session is exact on the interpreter and an opt-in on hardware"""
    if "seven_waves" in name and not os.environ.get("VS_EMU") and not os.environ.get("VS_TEST_UNVERIFIED"):
        pytest.skip(f"{name}: not run on hardware yet")


class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def fitted_indexes(gpu_ctx):
    """index, handle and the oracle's answers (computed once, shared by every case, never changed)"""
    cache = {}
    for name, (kw, qkind, L, rescore) in INDEXES.items():
        ti = cached_index(**kw)
        q = ti.queries(96, seed=77, kind=qkind)
        qlabels = None
        if ti.label_off is not None:
            rng = np.random.default_rng(5)
            qlabels = [sorted(set(int(v) for v in rng.integers(1, 7, int(rng.integers(1, 3))))) for _ in range(len(q))]
        m = rescore + 15
        stream = ti.oracle.stream_batch(q, L=L, m=m, qlabels=qlabels)
        rows = ti.oracle.search_batch(q, L=L, rescore=rescore, k=10, qlabels=qlabels)
        cache[name] = dict(ti=ti, ix=ti.upload(gpu_ctx), q=q, qlabels=qlabels, L=L, rescore=rescore, m=m, stream=stream, rows=rows)
    yield cache
    for c in cache.values():
        c["ix"].close()


def _expected_heap_top(env, diag):
    """the heap top the launch must have: the switch, else the table-less regime's 511 — or 255 where the rule (choose_heap_top) finds that
    it buys at least a tenth more resident scans.  The rule is restated here from the two occupancy figures the device reported for this
    very launch (VS_WS_DEBUG prints them as they are queried); without such a line the rule was not consulted."""
    if "VS_F_HL" in env:
        return int(env["VS_F_HL"])
    m = re.findall(r"resident scans: heap top 511 (\d+), 255 (\d+)", diag)
    if not m:
        return 511
    res511, res255 = (int(v) for v in m[-1])
    return 255 if 10 * res255 >= 11 * res511 else 511


@pytest.mark.parametrize("cross", list(CROSS))
@pytest.mark.parametrize("gcap", GCAPS)
@pytest.mark.parametrize("iname", list(INDEXES))
def test_fitted_tables_are_exact(fitted_indexes, capfd, iname, gcap, cross):
    _hardware_unverified(cross)
    c = fitted_indexes[iname]
    ix, q, ql, L, rescore, m = c["ix"], c["q"], c["qlabels"], c["L"], c["rescore"], c["m"]
    oi, oh, ost = c["stream"]
    osi, osd, _ = c["rows"]
    env = dict(BASE, VS_F_GCAP=str(gcap), VS_WS_DEBUG="1", **CROSS[cross])
    with _Env(env):
        for _ in range(2):  # the second call runs with the statistics the first one left behind
            capfd.readouterr()
            gi, gh, gst = ix.stream_batch(q, search_list_size=L, m=m, qlabels=ql)
            diag = capfd.readouterr().err
            info = ix.last_search_info()
            assert info["dedup_slots"] == gcap and gcap & (gcap - 1), info  # the launch really had that many slots
            assert info["heap_lds"] == _expected_heap_top(env, diag), (info, diag[-600:])
            assert (gi == oi).all() and (gh == oh).all()
            for key in COUNTERS:
                assert gst[key] == ost[key], (key, gst[key], ost[key])
            if gcap == 1280 and iname == "l2_R50":  # far too small for these scans: they take the second attempt
                assert gst["fallback_scans"] > 0
            si, _, sd, _ = ix.search_batch(q, search_list_size=L, rescore=rescore, k=10, qlabels=ql)
            assert (si == osi).all()
            assert (sd.view(np.uint32) == osd.view(np.uint32)).all()


def test_fitted_tables_compile_time_geometry(gpu_ctx, capfd):
    """W = 24 (768 x 2 bit), num_neighbors <= 64: the plain unit at six waves per SIMD with its compile-time row geometry"""
    ti = cached_index(n=500, dim_full=768, bits=2, R=20, distance=1, seed=23, kind="gauss", L_build=40)
    ix = ti.upload(gpu_ctx)
    try:
        q = ti.queries(32, seed=6, kind="gauss")
        oi, oh, ost = ti.oracle.stream_batch(q, L=3, m=60)
        osi, osd, _ = ti.oracle.search_batch(q, L=3, rescore=40, k=10)
        for gcap in (1280, 2304):
            env = dict(BASE, VS_F_GCAP=str(gcap), VS_F_VR="0", VS_F_MINW="6", VS_WS_DEBUG="1")
            with _Env(env):
                for _ in range(2):
                    capfd.readouterr()
                    gi, gh, gst = ix.stream_batch(q, search_list_size=3, m=60)
                    diag = capfd.readouterr().err
                    info = ix.last_search_info()
                    assert info["kernel"] == _lib.VS_SEARCH_FAST_SBQ and info["dedup_slots"] == gcap, info
                    hl = _expected_heap_top(env, diag)
                    assert info["heap_lds"] == hl, (info, diag[-600:])
                    # The report names the kernel family, not the instantiation; what it does show is the LDS layout only the
                    # six-wave 16-bit units have (no key slot dropped, the query code's 192-byte copy, three survivor arrays), and an
                    # unkeyed, unmasked W = 24 launch with that layout is dispatched to the plain unit and nowhere else.
                    ocap = max(-(-(gcap // 16) // 128) * 128, 256)
                    lds = (hl + 1) * 4 + 3 * 256 + info["visited_cap"] * 8 + 128 + 192 + (gcap + ocap) // 32 * 4 + 32
                    assert info["lds_bytes"] == -(-lds // 16) * 16, info
                    assert (gi == oi).all() and (gh == oh).all()
                    for key in COUNTERS:
                        assert gst[key] == ost[key], (key, gst[key], ost[key])
                    si, _, sd, _ = ix.search_batch(q, search_list_size=3, rescore=40, k=10)
                    assert (si == osi).all()
                    assert (sd.view(np.uint32) == osd.view(np.uint32)).all()
    finally:
        ix.close()


STAT_KEYS = ("visited_nodes", "candidate_nodes", "quantized_distance_comparisons", "full_distance_comparisons", "node_reads",
             "node_heap_reads", "next_calls")


def test_scan_pool_with_a_fitted_table(fitted_indexes, monkeypatch):
    """8 pooled scans, 200 rows each in fetches of 20, continued by the resumable instantiation on a table of 87 x 256 slots"""
    monkeypatch.setenv("VS_POOL_FAST", "1")
    c = fitted_indexes["l2_R50"]
    ti, ix, q = c["ti"], c["ix"], c["q"]
    G, k, L, rescore = 8, 20, 20, 30
    pool = P.ScanPool(ix, G, search_list_size=L, rescore=rescore, kmax=k, rows_cap=256)
    try:
        info = pool.info()
        slots = info["dedup_slots"]
        assert info["kernel"] == _lib.VS_SEARCH_FAST_SBQ, info
        assert slots == 22272 and slots & (slots - 1), info  # ((2 L + rows_cap + 32) x 50 pushes x 4 / 3 + 256, in steps of 256)
        oscans = []
        for i in range(G):
            pool.rescan(i, q[i])
            oscans.append(ti.oracle.scan(q[i], L=L, rescore=rescore))
        for rnd in range(10):
            rows, ids, tids, dist = pool.fetch(list(range(G)), k)
            for i in range(G):
                assert rows[i] == k, (rnd, i, rows[i])
                for j in range(k):
                    o = oscans[i].gettuple()
                    assert o is not None and ids[i][j] == o[0] and tids[i][j] == o[1], (rnd, i, j)
                    assert np.float32(dist[i][j]).view(np.uint32) == np.float32(o[2]).view(np.uint32), (rnd, i, j)
                g, o = pool.stats(i), oscans[i].stats()
                for key in STAT_KEYS:
                    assert g[key] == o[key], (rnd, i, key, g[key], o[key])
    finally:
        pool.close()
