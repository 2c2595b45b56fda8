"""The consume side of fast_scan (vs_search_fast.hip): the rows a scan hands out between two expansions, at the stream lengths and
list sizes where the loop's exits sit.  Every case compares node ids in order, heap TIDs, distance bits and every counter of COUNTERS
with the oracle's: M = 29, M = 64 (rescore 55), M = 139 (rescore 130), a search list of 40 (runs of consumed rows between
expansions), streams that end before M, tombstoned and hidden rows between emitted ones, label keys, the W = 24 instantiations that
live in translation units of their own, a scan continued over several launches (row_stats), and a stream-only batch, whose Hamming
keys are its output.  Written with the rotated consume loop of docs/experiments/consume_loop.patch (measured neutral, not applied);
it holds any rewrite of that loop to the same rows.  Also runs on the lockstep interpreter (VS_EMU=1)."""
import numpy as np
import pytest

from helpers import cached_index
from lifecycle_checks import check_pool_slot, regime
from oracle import oracle_py as O
from test_gpu_zzz_rerank_window import COUNTERS, INVALID, Corpus, tie_vectors

pytestmark = pytest.mark.gpu

# (search_list_size, rescore, k): M = rescore + k - 1
POINTS = [(3, 20, 10), (3, 55, 10), (3, 130, 10), (40, 20, 10)]
POINT_IDS = ["M29", "M64", "M139", "L40"]
STREAM_KEYS = ("visited_nodes", "candidate_nodes", "quantized_distance_comparisons", "node_reads", "next_calls")


def compare(ix, oidx, tids, q, L, rescore, k, qlabels=None, where=""):
    oi, od, ost = oidx.search_batch(q, L=L, rescore=rescore, k=k, qlabels=qlabels)
    gi, gt, gd, gst = ix.search_batch(q, search_list_size=L, rescore=rescore, k=k, qlabels=qlabels)
    assert (gi == oi).all(), (where, np.argwhere(gi != oi)[:5])
    live = gi != INVALID
    assert (gt[live] == tids[gi[live]]).all() and (gt[~live] == 0).all(), where
    assert (gd.view(np.uint32)[live] == od.view(np.uint32)[live]).all(), where
    assert np.isnan(gd[~live]).all(), where
    for key in COUNTERS:
        assert gst[key] == ost[key], (where, key, gst[key], ost[key])
    return oi


def queries(c, nq, seed):
    near = c.vecs[:min(3, nq)]
    return np.vstack([near, np.random.default_rng(seed).random((nq - len(near), c.dim), dtype=np.float32)])


@pytest.fixture(scope="module")
def ties():
    return Corpus(tie_vectors(3000, 300, 64, seed=3))


@pytest.fixture(scope="module")
def keyed():
    return Corpus(tie_vectors(3000, 300, 64, seed=4), n_labels=5)


@pytest.mark.parametrize("nq", [1, 5, 70])
@pytest.mark.parametrize("point", POINTS, ids=POINT_IDS)
def test_rows_and_counters(gpu_ctx, ties, point, nq):
    L, rescore, k = point
    ix = ties.upload(gpu_ctx)
    try:
        for name, env in (("default", {}), ("tableless", {"VS_F_LDS_MAX_INS": "0"})):
            with regime(env):
                compare(ix, ties.oracle, ties.tids, queries(ties, nq, 100 + nq), L, rescore, k, where=name)
    finally:
        ix.close()


@pytest.mark.parametrize("nq", [5, 70])
@pytest.mark.parametrize("point", POINTS, ids=POINT_IDS)
def test_dead_and_hidden_rows_between_emitted_ones(gpu_ctx, ties, point, nq):
    """a third of the rows tombstoned, a quarter of the rest hidden by the visibility mask: the skips of consume() run between
    emitted rows, with st_pops / st_invis (node_heap_reads, next_calls) as the oracle counts them"""
    L, rescore, k = point
    rng = np.random.default_rng(17)
    tids = ties.tids.copy()
    tids[rng.random(ties.n) < 0.33] &= ~np.uint64(0xFFFF)
    mask = (rng.random(ties.n) >= 0.25).astype(np.uint8)
    oidx = O.OracleIndex(codes=ties.codes, nbrs=ties.nbrs, heap_tids=tids, vecs=ties.vecs, mean=ties.mean, m2=ties.m2, count=ties.count,
                         bits=ties.bits, dim_index=ties.dim, num_neighbors=ties.R, distance_type=ties.distance, default_start=ties.start)
    oidx.set_visibility(mask)
    ix = ties.upload(gpu_ctx)
    try:
        ix.mark_deleted(np.flatnonzero((tids & np.uint64(0xFFFF)) == 0).astype(np.uint32))
        ix.set_visibility(mask)
        for name, env in (("default", {}), ("tableless", {"VS_F_LDS_MAX_INS": "0"})):
            with regime(env):
                compare(ix, oidx, tids, queries(ties, nq, 200 + nq), L, rescore, k, where=name)
    finally:
        ix.close()


@pytest.mark.parametrize("point", POINTS, ids=POINT_IDS)
def test_stream_ends_before_m(gpu_ctx, point):
    """9 rows: next() returns None long before M rows; the padding follows the rows that were emitted"""
    L, rescore, k = point
    small = Corpus(np.random.default_rng(2).random((9, 32), dtype=np.float32), R=8, L_build=10)
    ix = small.upload(gpu_ctx)
    try:
        for nq in (1, 5, 70):
            oi = compare(ix, small.oracle, small.tids, np.random.default_rng(nq).random((nq, 32), dtype=np.float32), L, rescore, k, where=nq)
            assert ((oi != INVALID).sum(axis=1) == 9).all()
    finally:
        ix.close()


@pytest.mark.parametrize("nq", [1, 5, 70])
@pytest.mark.parametrize("point", POINTS, ids=POINT_IDS)
def test_label_keys(gpu_ctx, keyed, point, nq):
    L, rescore, k = point
    rng = np.random.default_rng(nq)
    qlabels = [sorted(set(int(v) for v in rng.integers(1, 6, int(rng.integers(1, 3))))) for _ in range(nq)]
    ix = keyed.upload(gpu_ctx)
    try:
        for name, env in (("default", {}), ("tableless", {"VS_F_LDS_MAX_INS": "0"})):
            with regime(env):
                compare(ix, keyed.oracle, keyed.tids, queries(keyed, nq, 300 + nq), L, rescore, k, qlabels=qlabels, where=name)
    finally:
        ix.close()


# the instantiations of the headline geometry (24-word code rows, 16-bit tables, six waves per SIMD) that are compiled as translation
# units of their own: without label keys and a visibility mask, and with
@pytest.mark.parametrize("point", POINTS, ids=POINT_IDS)
@pytest.mark.parametrize("unit", ["plain6", "keys6"])
def test_w24_six_wave_units(gpu_ctx, unit, point):
    L, rescore, k = point
    ti = cached_index(n=500, dim_full=768, bits=2, R=20, distance=1, seed=23, kind="gauss", L_build=40, n_labels=4 if unit == "keys6" else 0,
                      deleted_frac=0.2)
    nq = 70
    q = ti.queries(nq, seed=6, kind="gauss")
    rng = np.random.default_rng(3)
    qlabels = [sorted(set(int(v) for v in rng.integers(1, 5, int(rng.integers(1, 3))))) for _ in range(nq)] if unit == "keys6" else None
    ix = ti.upload(gpu_ctx)
    try:
        with regime({"VS_F_LDS_MAX_INS": "0", "VS_F_VR": "0", "VS_F_MINW": "6", "VS_F_HL": "63"}):
            compare(ix, ti.oracle, ti.tids, q, L, rescore, k, qlabels=qlabels, where=unit)
            oi, oh, ost = ti.oracle.stream_batch(q, L=L, m=rescore + k - 1, qlabels=qlabels)
            gi, gh, gst = ix.stream_batch(q, search_list_size=L, m=rescore + k - 1, qlabels=qlabels)
            assert (gi == oi).all() and (gh == oh).all(), unit
    finally:
        ix.close()


@pytest.mark.parametrize("point", POINTS, ids=POINT_IDS)
def test_stream_only_batch_returns_hamming_keys(gpu_ctx, ties, point):
    """vs_stream_batch: the Hamming keys are the caller's output — after a rerank batch on the same handle, which has no use for them"""
    L, rescore, k = point
    m = rescore + k - 1
    ix = ties.upload(gpu_ctx)
    try:
        for nq in (1, 5, 70):
            q = queries(ties, nq, 400 + nq)
            compare(ix, ties.oracle, ties.tids, q, L, rescore, k, where=("before", nq))
            oi, oh, ost = ties.oracle.stream_batch(q, L=L, m=m)
            gi, gh, gst = ix.stream_batch(q, search_list_size=L, m=m)
            assert (gi == oi).all() and (gh == oh).all(), nq
            for key in STREAM_KEYS:
                assert gst[key] == ost[key], (nq, key, gst[key], ost[key])
    finally:
        ix.close()


@pytest.mark.parametrize("L,rescore", [(3, 20), (40, 20)])
def test_scan_pool_continuation(gpu_ctx, ties, L, rescore):
    """a pooled scan continued over five launches of 16 rows: the rows, and after every launch the counters as they stood when its
    last row was emitted (row_stats), are those of the oracle's one scan"""
    import pgvectorscale_amd as P
    q = queries(ties, 4, 500)
    ix = ties.upload(gpu_ctx)
    pool = P.ScanPool(ix, 4, search_list_size=L, rescore=rescore, kmax=16, rows_cap=1024)
    try:
        for slot in range(4):
            pool.rescan(slot, q[slot])
        for slot in (2, 0):
            check_pool_slot(pool, slot, ties.oracle.scan(q[slot], L=L, rescore=rescore), 16, 5, where=slot)
    finally:
        pool.close()
        ix.close()
