"""The exact brute force (vs_bruteforce_topk: k_rerank over contiguous chunks of rows, k_bf_fold into a top-k list that lives in
global memory between chunks) where it serves as recall ground truth: several chunks (row_base != 0, the list reloaded, a chunk that
is no multiple of the wave, a short last chunk, equal distances on both sides of a chunk boundary), the ends of k, and the special
values under the (f32::total_cmp, node id) order.  Ids are compared with `==` and f32 distances by their bit patterns,
NaNs included: total_cmp puts a NaN with the sign set before every number and one with the sign clear after every number."""
import os

import numpy as np
import pytest

from helpers import make_vectors
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu
EMU = bool(os.environ.get("VS_EMU"))
INV = 0xFFFFFFFF
DISTANCES = {"l2": O.L2, "cosine": O.COSINE, "ip": O.IP}


def _live_tids(n):
    return ((np.arange(n, dtype=np.uint64) + 7) << np.uint64(16)) | np.uint64(1)


def _delete(tids, rows):
    tids[rows] &= ~np.uint64(0xFFFF)  # InvalidOffsetNumber: a deleted tuple


def _upload(gpu_ctx, vecs, tids, distance, plain=False):
    """no graph (every neighbor slot empty), as tests/test_gpu_scan.py::_flat_index, with the vector column"""
    import pgvectorscale_amd as P
    from pgvectorscale_amd import _lib
    n, dim = vecs.shape
    nbrs = np.full((n, 4), INV, np.uint32)
    if plain:
        return P.DiskAnnIndex.upload(gpu_ctx, codes=None, nbrs=nbrs, heap_tids=tids, vecs=vecs, mean=None, m2=None, count=0, bits=None,
                                     dim_index=dim, num_neighbors=4, distance_type=distance, default_start=0,
                                     storage_type=_lib.VS_STORAGE_PLAIN)
    return P.DiskAnnIndex.upload(gpu_ctx, codes=np.zeros((n, (dim + 63) // 64), np.uint64), nbrs=nbrs, heap_tids=tids, vecs=vecs,
                                 mean=np.zeros(dim, np.float32), m2=None, count=1, bits=1, dim_index=dim, num_neighbors=4,
                                 distance_type=distance, default_start=0)


def _oracle_of(vecs, tids, distance, plain=False):
    n, dim = vecs.shape
    return O.OracleIndex(codes=np.zeros((n, (dim + 63) // 64), np.uint64), nbrs=np.full((n, 4), INV, np.uint32), heap_tids=tids, vecs=vecs,
                         mean=np.zeros(dim, np.float32), m2=np.zeros(dim, np.float32), count=1, bits=1, dim_index=dim, num_neighbors=4,
                         distance_type=distance, default_start=0, storage_plain=plain)


def _bruteforce(gpu_ctx, ix, q, k):
    dq = gpu_ctx.alloc(q.nbytes)
    try:
        gpu_ctx.upload(dq, q)
        return ix.bruteforce_topk(dq, len(q), k)
    finally:
        gpu_ctx.free(dq)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# several chunks
# ---------------------------------------------------------------------------------------------------------------------------------
# The chunk length depends on the number of queries alone — max(4096, 256Mi / nq) rows, a 1 GiB distance buffer — so a large batch of
# few DISTINCT queries folds a small corpus in several chunks while the reference stays 64 queries.
#   nq, rows per chunk, n, chunks
CHUNKED = {
    "wave_aligned": (65536, 4096, 3 * 4096 + 37, 4),    # chunks of 64 full waves, the last chunk 37 rows
    "partial_wave": (40000, 6710, 2 * 6710 + 5, 3),     # 54 rows in the last wave of every full chunk, the last chunk 5 rows
}
A, B, CQ, DQ = 3, 17, 40, 63  # the queries whose exact copies are planted in the corpus


def _chunked_case(shape, dim, seed):
    nq, chunk, n, _ = CHUNKED[shape]
    rng = np.random.default_rng(seed)
    q = make_vectors(64, dim, seed + 1, "gauss")
    # rows drawn from 2 500 distinct vectors, five copies of each on average: equal distances in different chunks are the rule, and
    # only the id decides between them
    pool = make_vectors(2500, dim, seed + 2, "gauss") * rng.uniform(0.2, 3.0, (2500, 1)).astype(np.float32)
    vecs = np.ascontiguousarray(pool[rng.integers(0, 2500, n)])
    tids = _live_tids(n)
    _delete(tids, rng.random(n) < 0.1)
    plants = {A: [0, 1],                                  # the first rows
              B: [chunk - 1, chunk],                      # the last row of the first chunk and the first row of the second
              CQ: [2 * chunk - 1, 2 * chunk, n - 1],      # the next boundary and the last row of the corpus
              DQ: [chunk - 2, chunk + 1, n - 2]}          # ... of which chunk - 2 is deleted
    for qi, rows in plants.items():
        vecs[rows] = q[qi]
        tids[rows] = _live_tids(n)[rows]
    _delete(tids, [chunk - 2])
    plants[DQ] = plants[DQ][1:]
    return q, vecs, tids, plants, chunk


@pytest.mark.skipif(EMU, reason="65 536 queries x 12 000 rows: hours on the interpreter")
@pytest.mark.parametrize("distance", list(DISTANCES))
@pytest.mark.parametrize("dim,k", [(8, 10), (40, 64)])  # 8: the tail loop only; 40: one 32-float step plus a tail
@pytest.mark.parametrize("shape,plain", [("wave_aligned", False), ("partial_wave", False), ("partial_wave", True)])
def test_bruteforce_folds_several_chunks(gpu_ctx, oracle, shape, plain, dim, k, distance):
    nq, _, n, chunks = CHUNKED[shape]
    dt = DISTANCES[distance]
    q, vecs, tids, plants, chunk = _chunked_case(shape, dim, seed=dim + len(shape))
    assert len(vecs) == n
    oi, od = _oracle_of(vecs, tids, dt, plain).bruteforce(q, k=k)
    assert not np.isnan(od).any() and (oi != INV).all()
    if distance == "l2":  # an exact copy is at distance 0: the planted rows lead their query's list in id order, the deleted one absent
        for qi, rows in plants.items():
            assert oi[qi, :len(rows)].tolist() == rows and (od[qi, :len(rows)] == 0).all()
    assert not (oi == chunk - 2).any()
    # most lists hold rows of the first AND of later chunks, and equal distances stand on both sides of a boundary
    assert ((oi >= chunk).any(axis=1) & (oi < chunk).any(axis=1)).mean() > 0.9
    tie = _bits(od)[:, 1:] == _bits(od)[:, :-1]
    assert (tie & (oi[:, :-1] // chunk != oi[:, 1:] // chunk)).any(axis=1).sum() >= 32
    ix = _upload(gpu_ctx, vecs, tids, dt, plain)
    try:
        gpu_ctx.profile_read()
        gpu_ctx.profile_enable(True)
        gi, gd = _bruteforce(gpu_ctx, ix, np.ascontiguousarray(np.tile(q, (nq // 64, 1))), k)
        launches = gpu_ctx.profile_read()["rerank"][1]
    finally:
        gpu_ctx.profile_enable(False)
        ix.close()
    # one "rerank" span per chunk (the only k_rerank launches of a brute force): the fold really ran over several chunks
    assert launches == chunks
    gi, gd = gi.reshape(nq // 64, 64, k), _bits(gd).reshape(nq // 64, 64, k)
    assert (gi == oi[None]).all()          # every copy of a query has its original's rows ...
    assert (gd == _bits(od)[None]).all()   # ... and distance bits


# ---------------------------------------------------------------------------------------------------------------------------------
# the ends of k and the special values
# ---------------------------------------------------------------------------------------------------------------------------------
def _total_key(d):
    """f32::total_cmp as a sortable integer (Rust core: bits ^ (((bits >> 31) as u32) >> 1), compared as i32)"""
    b = _bits(d).astype(np.int64)
    return np.where(b & 0x80000000, -1 - (b & 0x7FFFFFFF), b)


def _stated_topk(dist, tids, k):
    """rows of the live tuples by (total_cmp key, node id), the rest (INVALID, NaN): the contract of the brute force, restated"""
    nq, n = dist.shape
    live = np.flatnonzero(tids & np.uint64(0xFFFF))
    ids = np.full((nq, k), INV, np.uint32)
    bits = np.full((nq, k), 0x7FC00000, np.uint32)
    for qi in range(nq):
        order = live[np.lexsort((live, _total_key(dist[qi, live])))][:k]
        ids[qi, :len(order)] = order
        bits[qi, :len(order)] = _bits(dist[qi])[order]
    return ids, bits


def test_total_key_is_total_cmp():
    v = np.array([-np.nan, -np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf, np.nan], np.float32)
    assert (_bits(v[[0, -1]]) == [0xFFC00000, 0x7FC00000]).all()
    assert (np.diff(_total_key(v)) > 0).all()


DIM = 36  # one 32-float step plus a tail of 4


def _special_corpus():
    n = 300
    rng = np.random.default_rng(12)
    vecs = make_vectors(n, DIM, 3, "gauss") * rng.uniform(0.2, 3.0, (n, 1)).astype(np.float32)
    vecs[5, 2] = np.inf                      # L2 to the inf query: inf - inf = NaN; IP: +-inf
    vecs[6, 2] = -np.inf
    vecs[7, 5] = np.nan
    vecs[8, [2, 33]] = [np.inf, -np.inf]     # ... in the 32-float step and in the tail
    vecs[9] = 0                              # IP / cosine with anything: a sum of +-0.0 products
    vecs[10] = -0.0
    vecs[11] = 0
    vecs[11, 4] = 1                          # orthogonal to the one-hot queries below: IP exactly +-0.0
    vecs[12] = 1e-30                         # against the query of -1e-30: every product underflows to -0.0, the IP distance is +0.0
    vecs[200:220] = vecs[40:60]              # duplicated rows: equal keys, the id decides
    vecs[220:224] = 0                        # ... and more zero rows
    vecs[224:228] = -vecs[44]                # the same distances as row 44 with the sign flipped under IP
    q = make_vectors(12, DIM, 4, "gauss")
    q[3] = 0
    q[4, 2] = np.inf
    q[5] = -0.0
    q[6] = vecs[41]                          # distance 0 to rows 41 and 201
    q[7] = 0
    q[7, 9] = 1                              # one-hot
    q[8] = 0
    q[8, 9] = -1
    q[9, 33] = -np.inf
    q[10] = -1e-30
    tids = _live_tids(n)
    _delete(tids, rng.random(n) < 0.1)
    special = [5, 6, 7, 8, 9, 10, 11, 12, 41, 201, 220, 225]
    tids[special] = _live_tids(n)[special]
    _delete(tids, [221, 44])
    return vecs, q, tids


def _oracle_rows(distance, vecs, q):
    """the oracle's distance of every row to every query, prepared as a scan prepares them"""
    if distance == O.COSINE:
        vecs = np.stack([O.preprocess_cosine(v)[0] for v in vecs])
        q = np.stack([O.preprocess_cosine(v)[0] for v in q])
    return np.array([[O.distance_by_type(distance, v, x) for v in vecs] for x in q], np.float32)


SCENARIOS = {
    "k1": (1, None), "k10": (10, None), "k64": (64, None),
    "k_above_live_rows": (64, 23),  # 23 live rows: the tail of every list is (INVALID, NaN)
    "nothing_live": (10, 0),
}
CASES = [(False, d, s) for d in DISTANCES for s in SCENARIOS] + [(True, d, s) for d in DISTANCES for s in ("k10", "k_above_live_rows")]


def _check_special(gpu_ctx, vecs, q, tids, od_rows, dt, plain, k):
    n = len(vecs)
    live = tids & np.uint64(0xFFFF) != 0
    # the oracle, and its order restated over its own per-row distances: asserted, not merely copied
    oi, od = _oracle_of(vecs, tids, dt, plain).bruteforce(q, k=k)
    si, sb = _stated_topk(od_rows, tids, k)
    assert (oi == si).all() and (_bits(od) == sb).all()
    assert ((oi != INV).sum(axis=1) == min(k, int(live.sum()))).all()
    ix = _upload(gpu_ctx, vecs, tids, dt, plain)
    try:
        gd_rows = np.stack(ix.rerank(q, [np.arange(n, dtype=np.uint32)] * len(q)))
        gi, gd = _bruteforce(gpu_ctx, ix, q, k)
    finally:
        ix.close()
    assert (gi == oi).all(), (gi, oi)
    assert (_bits(gd) == _bits(od)).all()  # NaN payloads and signs, the sign of zero and the (INVALID, NaN) tail included
    # (what the fold ranks: k_rerank's distance of every row, bit for bit the oracle's)
    assert (_bits(gd_rows) == _bits(od_rows)).all()


@pytest.mark.parametrize("plain,distance,scenario", CASES, ids=["-".join(("plain" if c[0] else "sbq",) + c[1:]) for c in CASES])
def test_bruteforce_special_values_and_ends_of_k(gpu_ctx, oracle, plain, distance, scenario):
    k, keep = SCENARIOS[scenario]
    dt = DISTANCES[distance]
    vecs, q, tids = _special_corpus()
    od_rows = _oracle_rows(dt, vecs, q)
    live = tids & np.uint64(0xFFFF) != 0
    # the corpus does hold what it is meant to hold
    assert live.sum() > 64
    if distance == "l2":
        assert np.isnan(od_rows[4, 5]) and np.isposinf(od_rows[4, 6]) and np.isnan(od_rows[0, 7])
    if distance == "ip":
        assert np.isinf(od_rows[0, 5]) and od_rows[0, 5] == -od_rows[0, 6]
        zeros = od_rows[:, live][od_rows[:, live] == 0]
        assert np.signbit(zeros).any() and not np.signbit(zeros).all()  # both -0.0 and +0.0 distances occur
    if distance == "cosine":  # fmaxf(1 - d, 0) swallows the NaN of a row or query that inf normalises to NaN
        assert not np.isnan(od_rows).any() and (od_rows >= 0).all() and (od_rows[:, live] == 0).any()
    else:  # NaN distances of both signs: the ones that rank before every number and the ones that rank after
        nans = od_rows[:, live][np.isnan(od_rows[:, live])]
        assert np.signbit(nans).any() and not np.signbit(nans).all()
    if keep is not None:  # only the first `keep` live rows stay (the special rows 5..12 among them)
        _delete(tids, np.flatnonzero(live)[keep:])
    _check_special(gpu_ctx, vecs, q, tids, od_rows, dt, plain, k)
