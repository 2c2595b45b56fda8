"""k_search_plain (vs_search.hip): the first attempt of every batch over a `plain` storage index — one wave per scan on a persistent
grid, the scan's state on chip.  Rows (ids AND f32 distance bits), tids and the reference counters must equal the oracle's and the
general kernel's (VS_PLAIN_FAST=0); vs_index_last_search_info tells which kernel ran.  At these index sizes the planned capacities
clamp to n, so nothing may be handed over unless a VS_PF_* capacity is set too small on purpose."""
import contextlib
import functools

import numpy as np
import pytest

from helpers import make_vectors
from oracle import oracle_py as O
from test_gpu_zy_plain import PlainIndex

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
INV = 0xFFFFFFFF
GENERAL, FAST_SBQ, FAST_PLAIN = 0, 1, 2
COUNTERS = ("visited_nodes", "candidate_nodes", "full_distance_comparisons", "node_reads", "next_calls")
PLAIN_LDS_BUDGET = 40 * 1024  # DESIGN.md "Plain storage: the search kernel": a scan's LDS state beyond this stays on the general kernel


@contextlib.contextmanager
def options(**kv):
    from pgvectorscale_amd.index import set_option
    for k, v in kv.items():
        set_option(k, v)
    try:
        yield
    finally:
        for k in kv:
            set_option(k, None)


def _oracle_of(pi):
    w = (pi.dim_index + 63) // 64
    return O.OracleIndex(codes=np.zeros((pi.n, w), np.uint64), nbrs=pi.nbrs, heap_tids=pi.tids, vecs=pi.vecs,
                         mean=np.zeros(pi.dim_index, np.float32), m2=np.zeros(pi.dim_index, np.float32), count=0, bits=1,
                         dim_index=pi.dim_index, num_neighbors=pi.R, distance_type=pi.distance, default_start=pi.start, storage_plain=True)


@functools.lru_cache(maxsize=None)
def corpus(dim, distance, R, n=1200, dim_index=None):
    """un-normalised gauss rows over any connected graph; rows 200..219 are exact copies of rows 40..59 (equal keys: the BinaryHeap
    tie order decides) and row 3 is zero"""
    pi = PlainIndex(n=n, dim=dim, R=R, distance=distance, seed=dim + R, kind="gauss", deleted_frac=0.1, dim_index=dim_index)
    if n >= 220:
        pi.vecs[200:220] = pi.vecs[40:60]
    pi.vecs[3] = 0
    pi.oracle = _oracle_of(pi)
    return pi


def queries(nq, dim, seed=9):
    q = make_vectors(nq, dim, seed, "gauss")
    q[min(5, nq - 1)] = 0  # one all-zero query
    return q


def same(a, b):
    return (a[0] == b[0]).all() and (a[2].view(np.uint32) == b[2].view(np.uint32)).all() and (a[1] == b[1]).all()


def check_against_oracle(pi, got, ref, counters=COUNTERS):
    gi, gt, gd, gst = got
    oi, od, ost = ref
    assert (gi == oi).all()
    assert (gd.view(np.uint32) == od.view(np.uint32)).all()
    live = gi != INV
    assert (gt[live] == pi.tids[gi[live]]).all()
    for key in counters:
        assert gst[key] == ost[key], key
    assert gst["quantized_distance_comparisons"] == 0


# dim: 8 = tail only, 36 = one step + tail, 100 = 3 steps + tail 4, 128 = 4 steps, 768 = 24 steps (two load groups of 12)
MATRIX = [
    (8, O.L2, 24, 1, 25), (8, O.COSINE, 50, 30, 300), (8, O.IP, 24, 100, 25),
    (36, O.IP, 50, 30, 25), (36, O.L2, 24, 100, 300), (36, O.COSINE, 24, 1, 300),
    (100, O.COSINE, 24, 30, 25), (100, O.L2, 50, 1, 25), (100, O.IP, 50, 100, 300),
    (128, O.L2, 50, 100, 25), (128, O.IP, 24, 30, 300), (128, O.COSINE, 50, 1, 25),
    (768, O.COSINE, 50, 30, 25), (768, O.L2, 24, 30, 25), (768, O.IP, 24, 1, 25), (768, O.L2, 50, 100, 25),
]


@pytest.mark.parametrize("dim,distance,R,L,k", MATRIX)
def test_rows_bits_and_counters_match_oracle_and_general_kernel(gpu_ctx, oracle, dim, distance, R, L, k):
    pi = corpus(dim, distance, R)
    ix = pi.upload(gpu_ctx)
    q = queries(40, dim)
    got = ix.search_batch(q, search_list_size=L, rescore=50, k=k)  # rescore is ignored: no resort for plain storage
    info = ix.last_search_info()
    assert info["kernel"] == FAST_PLAIN and info["resident"] >= 1 and info["lds_bytes"] > 0
    check_against_oracle(pi, got, pi.oracle.search_batch(q, L=L, rescore=50, k=k))
    assert got[3]["fallback_scans"] == 0  # the capacities clamp to n = 1200: no scan can outgrow them
    si, sd, sst = ix.stream_batch(q, search_list_size=L, m=k)
    assert (si == got[0]).all() and (sd[si != INV] == got[2].view(np.uint32)[si != INV]).all()
    assert sst["fallback_scans"] == 0
    with options(VS_PLAIN_FAST="0"):
        old = ix.search_batch(q, search_list_size=L, rescore=50, k=k)
        assert ix.last_search_info()["kernel"] == GENERAL
    assert same(got, old)
    for key in COUNTERS:
        assert got[3][key] == old[3][key], key
    ix.close()


@pytest.mark.parametrize("distance", [O.COSINE, O.L2])
def test_truncated_index_under_a_visibility_mask(gpu_ctx, oracle, distance):
    pi = corpus(96, distance, 24, n=1000, dim_index=64)
    ix = pi.upload(gpu_ctx)
    vis = (np.random.default_rng(7).random(pi.n) >= 0.2).astype(np.uint8)
    ix.set_visibility(vis)
    pi.oracle.set_visibility(vis)
    try:
        q = queries(32, 96, seed=3)
        got = ix.search_batch(q, search_list_size=30, rescore=15, k=12)
        assert ix.last_search_info()["kernel"] == FAST_PLAIN
        check_against_oracle(pi, got, pi.oracle.search_batch(q, L=30, rescore=15, k=12),
                             counters=("visited_nodes", "candidate_nodes", "full_distance_comparisons", "node_reads"))
        assert got[3]["fallback_scans"] == 0
        with options(VS_PLAIN_FAST="0"):
            old = ix.search_batch(q, search_list_size=30, rescore=15, k=12)
        assert same(got, old)
        for key in COUNTERS + ("node_heap_reads",):
            assert got[3][key] == old[3][key], key
    finally:
        pi.oracle.set_visibility(None)
    ix.close()


@pytest.mark.parametrize("knob", [dict(VS_PF_HEAP_CAP="40", VS_PF_HEAP_LDS="16"), dict(VS_PF_DEDUP_SLOTS="64"), dict(VS_PF_VISITED="20")])
def test_scans_that_outgrow_a_capacity_are_handed_over_whole(gpu_ctx, oracle, knob):
    pi = corpus(36, O.L2, 24)
    ix = pi.upload(gpu_ctx)
    q = queries(40, 36)
    with options(**knob):
        got = ix.search_batch(q, search_list_size=30, rescore=0, k=25)
        assert ix.last_search_info()["kernel"] == FAST_PLAIN
    check_against_oracle(pi, got, pi.oracle.search_batch(q, L=30, rescore=0, k=25))
    assert got[3]["fallback_scans"] > 0 and got[3]["fallback_visited_nodes"] > 0
    assert got[3]["fallback_scans"] <= 40 and got[3]["queries"] == 40
    ix.close()


def test_a_small_lds_heap_spills_without_a_hand_over(gpu_ctx, oracle):
    pi = corpus(36, O.L2, 24)
    ix = pi.upload(gpu_ctx)
    q = queries(40, 36)
    with options(VS_PF_HEAP_LDS="7"):
        got = ix.search_batch(q, search_list_size=30, rescore=0, k=300)
        assert ix.last_search_info()["heap_lds"] == 7
    check_against_oracle(pi, got, pi.oracle.search_batch(q, L=30, rescore=0, k=300))
    assert got[3]["fallback_scans"] == 0
    ix.close()


def test_workgroups_reuse_their_regions_scan_after_scan(gpu_ctx, oracle):
    pi = corpus(36, O.L2, 24)
    ix = pi.upload(gpu_ctx)
    ix.search_batch(queries(4, 36), search_list_size=10, rescore=0, k=5)
    resident = ix.last_search_info()["resident"]  # what the device holds at once, whatever the batch
    assert resident >= 1
    for nq, seed in ((3 * resident + 7, 21), (resident + 3, 22)):  # the second batch reuses the regions; nothing is cleared
        q = queries(nq, 36, seed=seed)
        got = ix.search_batch(q, search_list_size=10, rescore=0, k=5)
        info = ix.last_search_info()
        assert info["kernel"] == FAST_PLAIN and info["resident"] == resident
        assert got[3]["fallback_scans"] == 0
        with options(VS_PLAIN_FAST="0"):
            assert same(got, ix.search_batch(q, search_list_size=10, rescore=0, k=5))
        oi, od, _ = pi.oracle.search_batch(q[:64], L=10, rescore=0, k=5)
        assert (got[0][:64] == oi).all() and (got[2][:64].view(np.uint32) == od.view(np.uint32)).all()
    ix.close()


def test_tiny_index(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    pi = corpus(12, O.L2, 4, n=5)
    ix = pi.upload(gpu_ctx)
    with pytest.raises(P.VsError) as e:  # before the first batch of the handle: VS_ERR_STATE
        ix.last_search_info()
    assert e.value.code == -5
    q = queries(9, 12)
    got = ix.search_batch(q, search_list_size=3, rescore=0, k=8)
    assert ix.last_search_info()["kernel"] == FAST_PLAIN
    check_against_oracle(pi, got, pi.oracle.search_batch(q, L=3, rescore=0, k=8))
    assert got[3]["fallback_scans"] == 0
    ix.close()


def test_index_without_a_start_node_returns_nothing(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    pi = corpus(36, O.L2, 24)
    ix = P.DiskAnnIndex.upload(gpu_ctx, codes=None, nbrs=pi.nbrs, heap_tids=pi.tids, vecs=pi.vecs, mean=None, m2=None, count=0, bits=None,
                               dim_index=36, num_neighbors=24, distance_type=O.L2, default_start=INV, storage_type=P._lib.VS_STORAGE_PLAIN)
    gi, gt, gd, st = ix.search_batch(queries(10, 36), search_list_size=20, rescore=0, k=6)
    assert ix.last_search_info()["kernel"] == FAST_PLAIN
    assert (gi == INV).all()
    for key in ("visited_nodes", "candidate_nodes", "full_distance_comparisons", "node_reads", "fallback_scans"):
        assert st[key] == 0, key
    ix.close()


def test_start_node_with_a_deleted_tid(gpu_ctx, oracle):
    base = corpus(36, O.L2, 24)
    pi = PlainIndex.__new__(PlainIndex)
    pi.__dict__.update(base.__dict__)
    pi.tids = base.tids.copy()
    pi.tids[pi.start] &= ~np.uint64(0xFFFF)
    pi.oracle = _oracle_of(pi)
    ix = pi.upload(gpu_ctx)
    q = queries(16, 36)
    got = ix.search_batch(q, search_list_size=10, rescore=0, k=20)
    assert ix.last_search_info()["kernel"] == FAST_PLAIN
    check_against_oracle(pi, got, pi.oracle.search_batch(q, L=10, rescore=0, k=20))
    assert (got[0] != pi.start).all()
    ix.close()


def test_huge_rows_stay_on_the_general_kernel_exactly_when_lds_is_short(gpu_ctx, oracle):
    pi = corpus(12000, O.L2, 8, n=80)
    ix = pi.upload(gpu_ctx)
    q = queries(6, 12000)
    got = ix.search_batch(q, search_list_size=10, rescore=0, k=10)
    info = ix.last_search_info()
    check_against_oracle(pi, got, pi.oracle.search_batch(q, L=10, rescore=0, k=10))
    # the query slice alone is 4 * 12000 B: more than the budget, whatever the other capacities are
    assert 4 * 12000 > PLAIN_LDS_BUDGET and info["kernel"] == GENERAL
    small = corpus(2048, O.L2, 8, n=80)  # 8 KB of query: well inside
    ix2 = small.upload(gpu_ctx)
    q2 = queries(6, 2048)
    got2 = ix2.search_batch(q2, search_list_size=10, rescore=0, k=10)
    info2 = ix2.last_search_info()
    assert info2["kernel"] == FAST_PLAIN and info2["lds_bytes"] <= PLAIN_LDS_BUDGET
    check_against_oracle(small, got2, small.oracle.search_batch(q2, L=10, rescore=0, k=10))
    ix.close()
    ix2.close()


def test_search_after_the_index_grew(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    n0, m, dim, R = 600, 100, 48, 24
    X = make_vectors(n0 + m, dim, 48, "gauss")
    tids = ((np.arange(n0 + m, dtype=np.uint64) + 11) << np.uint64(16)) | np.uint64(1)
    ix = P.DiskAnnIndex.alloc(gpu_ctx, n=n0, dim_full=dim, num_neighbors=R, distance_type=O.L2, storage_type=P._lib.VS_STORAGE_PLAIN)
    vp, stride = ix.array(P._lib.ARR_VECS)
    Xp = np.zeros((n0, stride), np.float32)
    Xp[:, :dim] = X[:n0]
    gpu_ctx.upload(vp, Xp)
    ix.refresh_norms()
    gpu_ctx.upload(ix.array(P._lib.ARR_TIDS)[0], np.ascontiguousarray(tids[:n0]))
    ix.build_graph(search_list_size=40, max_alpha=1.2)
    q = queries(40, dim)

    def check(n):
        got = ix.search_batch(q, search_list_size=30, rescore=0, k=25)
        info = ix.last_search_info()
        assert info["kernel"] == FAST_PLAIN and got[3]["fallback_scans"] == 0
        with options(VS_PLAIN_FAST="0"):
            assert same(got, ix.search_batch(q, search_list_size=30, rescore=0, k=25))
        host = ix.download(codes=False)
        pi = PlainIndex.__new__(PlainIndex)
        pi.__dict__.update(n=n, dim=dim, dim_index=dim, R=R, distance=O.L2, nbrs=host["nbrs"], tids=tids[:n], vecs=X[:n], start=ix.desc.default_start)
        check_against_oracle(pi, got, _oracle_of(pi).search_batch(q, L=30, rescore=0, k=25))
        return info

    a = check(n0)
    ix.insert(X[n0:], tids[n0:], search_list_size=32, max_alpha=1.2)  # the arrays may move; n changes
    assert ix.desc.n == n0 + m
    b = check(n0 + m)
    assert b["visited_cap"] >= a["visited_cap"]
    ix.close()
