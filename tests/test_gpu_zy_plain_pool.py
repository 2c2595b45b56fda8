"""Scan pools over `plain` storage (vs_scanpool.cpp): the continuations of the pooled scans run the resumable form of k_search_plain
(k_search_plain_rs, vs_search.hip) — one wave per pool slot, the scan's state on chip during a launch and saved per slot between
launches, the slot's heap spill / dedup regions never cleared.  Every slot must hand out the oracle's rows (ids, tids, f32 distance
bits) with the oracle's GreedySearchStats after every chunk, whatever mix of slots and chunk sizes the fetches name, across rescans,
at the LDS / spill boundary of the heap and when a capacity is outgrown (that slot fails alone).  ScanPool.info() tells which kernel a
pool runs; with VS_POOL_PLAIN_FAST=0 it is the general kernel, held to the oracle in the same way."""
import numpy as np
import pytest

import pgvectorscale_amd as P
from helpers import make_vectors
from oracle import oracle_py as O
from test_gpu_zy_plain import PlainIndex
from test_gpu_zy_plain_search import _oracle_of, corpus, options, queries

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
INV = 0xFFFFFFFF
GENERAL, FAST_SBQ, FAST_PLAIN = 0, 1, 2
VS_ERR_CAPACITY = -4
COUNTERS = ("visited_nodes", "candidate_nodes", "full_distance_comparisons", "node_reads", "next_calls")


def check_chunk(got_rows, ids, tids, dist, oscan, k, where):
    """the next k amgettuple calls of the oracle's scan against one slot's chunk"""
    n = 0
    for j in range(k):
        o = oscan.gettuple()
        if o is None:
            break
        assert j < got_rows, (where, "the pool ended the scan early", j)
        assert ids[j] == o[0] and tids[j] == o[1], (where, j, int(ids[j]), o[0])
        assert np.float32(dist[j]).view(np.uint32) == np.float32(o[2]).view(np.uint32), (where, j)
        n += 1
    assert got_rows == n, (where, got_rows, n)
    return n


def check_stats(pool, slot, oscan, where, keys=COUNTERS):
    g, o = pool.stats(slot), oscan.stats()
    for key in keys:
        assert g[key] == o[key], (where, key, g[key], o[key])
    assert g["quantized_distance_comparisons"] == 0


# dim: 8 = tail only, 36 = one step + tail, 100 = 3 steps + tail 4, 768 = 24 steps (two load groups of 12)
@pytest.mark.parametrize("fast", ["1", "0"], ids=["plain_kernel", "general_kernel"])
@pytest.mark.parametrize("dim,distance,R,L", [(8, O.IP, 24, 10), (36, O.L2, 24, 20), (100, O.COSINE, 50, 30), (768, O.L2, 24, 10)])
def test_pooled_plain_scans_hand_out_the_oracles_rows_and_stats(gpu_ctx, oracle, dim, distance, R, L, fast):
    pi = corpus(dim, distance, R)
    ix = pi.upload(gpu_ctx)
    G, k = 12, 16
    q = queries(G + 2, dim)  # q[5] is all zero
    qs = [q[i] for i in range(G)]
    qs[7] = None  # the SQL-NULL query
    with options(VS_POOL_PLAIN_FAST=fast):
        pool = P.ScanPool(ix, G, search_list_size=L, rescore=50, kmax=k, rows_cap=1024)  # rescore is ignored: no resort for plain storage
    try:
        info = pool.info()
        if fast == "1":
            assert info["kernel"] == FAST_PLAIN and info["resident"] == G and 0 < info["lds_bytes"] <= 96 * 1024
            assert info["heap_lds"] > 0 and info["dedup_slots"] >= 64 and info["visited_cap"] > 0
        else:
            assert info["kernel"] == GENERAL and info["resident"] == 0
            assert (info["heap_lds"], info["dedup_slots"], info["visited_cap"]) == (0, 0, 0)
        oscans = []
        for i in range(G):
            pool.rescan(i, qs[i])
            oscans.append(pi.oracle.scan(qs[i], L=L, rescore=50))
        handed = [0] * G
        ended = [False] * G
        rng = np.random.default_rng(9)
        for rnd in range(40):
            # who asks in this round: everybody, a random few, or one slot alone; chunk sizes vary
            if rnd % 3 == 0:
                who = [i for i in range(G) if not ended[i]]
            elif rnd % 3 == 1:
                who = [i for i in range(G) if not ended[i] and rng.random() < 0.4]
            else:
                who = [i for i in range(G) if not ended[i]][:1]
            if not who:
                break
            kk = int(rng.choice([1, 5, k]))
            rows, ids, tids, dist = pool.fetch(who, kk)
            for a, i in enumerate(who):
                assert rows[a] >= 0, (rnd, i, rows[a])
                n = check_chunk(int(rows[a]), ids[a], tids[a], dist[a], oscans[i], kk, (rnd, i))
                handed[i] += n
                ended[i] = n < kk
                check_stats(pool, i, oscans[i], (rnd, i))
            if rnd == 7:  # one slot is rescanned with another query while the others go on
                pool.rescan(1, q[G])
                oscans[1] = pi.oracle.scan(q[G], L=L, rescore=50)
                handed[1], ended[1] = 0, False
        assert sum(handed) > 40 * 4
        w = pool.work()
        assert w["rounds"] <= w["launches"] <= 2 * w["rounds"]
        assert pool.info() == info  # decided at creation
    finally:
        pool.close()
        ix.close()


@pytest.mark.parametrize("distance", [O.COSINE, O.L2])
def test_truncated_index_with_a_rescore_window_under_a_visibility_mask(gpu_ctx, oracle, distance):
    pi = corpus(96, distance, 24, n=1000, dim_index=64)
    ix = pi.upload(gpu_ctx)
    vis = (np.random.default_rng(7).random(pi.n) >= 0.2).astype(np.uint8)
    ix.set_visibility(vis)
    pi.oracle.set_visibility(vis)
    G, k = 6, 8
    q = queries(G, 96, seed=3)
    pool = P.ScanPool(ix, G, search_list_size=30, rescore=15, kmax=k, rows_cap=512)
    try:
        assert pool.info()["kernel"] == FAST_PLAIN
        oscans = []
        for i in range(G):
            pool.rescan(i, q[i])
            oscans.append(pi.oracle.scan(q[i], L=30, rescore=15))
        for rnd in range(10):
            who = list(range(G)) if rnd % 2 == 0 else [rnd % G, (rnd + 3) % G]
            kk = k if rnd % 3 else 3
            rows, ids, tids, dist = pool.fetch(who, kk)
            for a, i in enumerate(who):
                assert rows[a] >= 0
                check_chunk(int(rows[a]), ids[a], tids[a], dist[a], oscans[i], kk, (rnd, i))  # next_with_resort order
                assert pool.stats(i)["node_heap_reads"] == oscans[i].stats()["node_heap_reads"], (rnd, i)
    finally:
        pi.oracle.set_visibility(None)
        pool.close()
        ix.close()


def _reachable(pi):
    """the nodes a scan can ever visit: the oracle's builder leaves part of these un-normalised corpora unreachable from the start node"""
    seen, todo = {pi.start}, [pi.start]
    while todo:
        for v in pi.nbrs[todo.pop()][:pi.R]:
            if v == INV:
                break
            if int(v) not in seen:
                seen.add(int(v))
                todo.append(int(v))
    return seen


def test_a_pooled_plain_scan_equals_the_single_cursor_and_ends_like_it(gpu_ctx, oracle):
    """every live row the graph reaches exactly once through a pool slot, as through vs_gettuple; calls past the end keep asking next() in
    vain; a scan that outgrows the pool's row budget fails alone (VS_ERR_CAPACITY) while its neighbour is served"""
    pi = corpus(36, O.L2, 24, n=700)
    ix = pi.upload(gpu_ctx)
    q = queries(3, 36, seed=3)
    pool = P.ScanPool(ix, 4, search_list_size=3, rescore=0, kmax=64, rows_cap=1024)
    scan = ix.beginscan()
    try:
        assert pool.info()["kernel"] == FAST_PLAIN
        pool.rescan(2, q[0])
        scan.rescan(q[0], search_list_size=3, rescore=0)
        os_ = pi.oracle.scan(q[0], L=3, rescore=0)
        total, seen = 0, []
        while True:
            rows, ids, tids, dist = pool.fetch([2], 64)
            n = int(rows[0])
            for j in range(n):
                r = scan.gettuple()
                assert r is not None and r[1] == ids[0][j] and r[0] == tids[0][j]
                assert np.float32(r[2]).view(np.uint32) == dist[0][j].view(np.uint32)
                seen.append(int(ids[0][j]))
            total += check_chunk(n, ids[0], tids[0], dist[0], os_, 64, ("exhaustive", total))
            if n < 64:
                break
        live = sorted(v for v in _reachable(pi) if int(pi.tids[v]) & 0xFFFF)
        assert len(live) > 500 and total == len(live) and sorted(seen) == live  # every live row in reach, exactly once
        for _ in range(2):  # past the end
            rows, _, _, _ = pool.fetch([2], 8)
            assert rows[0] == 0 and os_.gettuple() is None
        check_stats(pool, 2, os_, "past the end")
    finally:
        scan.endscan()
        pool.close()
    # a row budget smaller than the scan: the slot fails alone
    pool = P.ScanPool(ix, 2, search_list_size=3, rescore=0, kmax=32, rows_cap=96)
    try:
        assert pool.info()["kernel"] == FAST_PLAIN
        pool.rescan(0, q[0])
        pool.rescan(1, q[1])
        for _ in range(3):  # 96 stream rows: still inside
            r0, _, _, _ = pool.fetch([0], 32)
            assert r0[0] == 32
        rows, ids, tids, dist = pool.fetch([0, 1], 32)  # slot 0 would need 128 stream rows
        assert rows[0] == VS_ERR_CAPACITY and rows[1] == 32
        check_chunk(32, ids[1], tids[1], dist[1], pi.oracle.scan(q[1], L=3, rescore=0), 32, "neighbour of the failed slot")
    finally:
        pool.close()
        ix.close()


def test_state_survives_launches_at_the_lds_spill_boundary(gpu_ctx, oracle):
    pi = corpus(36, O.L2, 24)
    ix = pi.upload(gpu_ctx)
    G = 4
    q = queries(G, 36, seed=14)
    with options(VS_PF_HEAP_LDS="7"):
        pool = P.ScanPool(ix, G, search_list_size=30, rescore=0, kmax=16, rows_cap=512)
    try:
        info = pool.info()
        assert info["kernel"] == FAST_PLAIN and info["heap_lds"] == 7
        oscans = [pi.oracle.scan(q[i], L=30, rescore=0) for i in range(G)]
        for i in range(G):
            pool.rescan(i, q[i])
        for rnd in range(300):  # chunks of 1: heap entries cross between LDS and the slot's spill region launch after launch
            rows, ids, tids, dist = pool.fetch(list(range(G)), 1)
            for i in range(G):
                assert rows[i] == 1, (rnd, i, rows[i])
                check_chunk(1, ids[i], tids[i], dist[i], oscans[i], 1, (rnd, i))
            if rnd % 25 == 0 or rnd == 299:
                for i in range(G):
                    check_stats(pool, i, oscans[i], (rnd, i))
    finally:
        pool.close()
        ix.close()


# (visited: at this search list size some of the eight scans outgrow the list early, some late and some never; a heap of 40 entries or a
# table of 48 ids is outgrown by every scan within its first visits, whatever the search list size)
@pytest.mark.parametrize("knob,L", [(dict(VS_PF_VISITED="20"), 12), (dict(VS_PF_HEAP_CAP="40", VS_PF_HEAP_LDS="16"), 3), (dict(VS_PF_DEDUP_SLOTS="64"), 3)],
                         ids=["visited", "heap", "dedup"])
def test_a_scan_that_outgrows_a_capacity_fails_alone(gpu_ctx, oracle, knob, L):
    pi = corpus(36, O.L2, 24)
    ix = pi.upload(gpu_ctx)
    G, k = 8, 4
    q = queries(G + 1, 36, seed=15)
    with options(**knob):
        pool = P.ScanPool(ix, G, search_list_size=L, rescore=0, kmax=k, rows_cap=512)
    try:
        assert pool.info()["kernel"] == FAST_PLAIN
        oscans = [pi.oracle.scan(q[i], L=L, rescore=0) for i in range(G)]
        for i in range(G):
            pool.rescan(i, q[i])
        failed = [False] * G
        for rnd in range(40):
            rows, ids, tids, dist = pool.fetch(list(range(G)), k)
            for i in range(G):
                if rows[i] < 0:
                    assert rows[i] == VS_ERR_CAPACITY
                    failed[i] = True
                    continue
                assert not failed[i], "a failed scan stays failed until its slot is rescanned"
                check_chunk(int(rows[i]), ids[i], tids[i], dist[i], oscans[i], k, (rnd, i))
                check_stats(pool, i, oscans[i], (rnd, i))
        assert any(failed)
        # the pool stays usable: a failed slot takes a new scan, which is served from its first row (until it outgrows the capacity too)
        f = failed.index(True)
        pool.rescan(f, q[G])
        os_ = pi.oracle.scan(q[G], L=L, rescore=0)
        rows, ids, tids, dist = pool.fetch([f], 1)
        if rows[0] != VS_ERR_CAPACITY:
            check_chunk(int(rows[0]), ids[0], tids[0], dist[0], os_, 1, "rescanned")
        others = [i for i in range(G) if not failed[i]]
        if others:
            rows, ids, tids, dist = pool.fetch(others, k)
            for a, i in enumerate(others):
                if rows[a] >= 0:
                    check_chunk(int(rows[a]), ids[a], tids[a], dist[a], oscans[i], k, ("after", i))
    finally:
        pool.close()
        ix.close()


def test_a_slots_regions_are_reused_without_clearing(gpu_ctx, oracle):
    pi = corpus(36, O.L2, 24)
    ix = pi.upload(gpu_ctx)
    q = queries(3, 36, seed=16)
    with options(VS_PF_HEAP_LDS="15"):  # most of the heap in the slot's spill region; the dedup ids are in the slot's table region
        pool = P.ScanPool(ix, 2, search_list_size=20, rescore=0, kmax=20, rows_cap=512)
    try:
        info = pool.info()
        assert info["kernel"] == FAST_PLAIN and info["dedup_slots"] > 1024

        def stream(query):
            os_ = pi.oracle.scan(query, L=20, rescore=0)
            for c in range(15):  # 300 rows
                rows, ids, tids, dist = pool.fetch([0], 20)
                assert rows[0] == 20
                check_chunk(20, ids[0], tids[0], dist[0], os_, 20, c)
            check_stats(pool, 0, os_, "end")

        pool.rescan(0, q[0])
        stream(q[0])
        pool.rescan(0, q[1])  # the regions hold what query A's scan left there
        stream(q[1])
        pool.endscan(0)
        pool.rescan(0, q[2])
        stream(q[2])
    finally:
        pool.close()
        ix.close()


def test_edges_no_start_node_three_rows_deleted_start(gpu_ctx, oracle):
    # an index without a start node hands out nothing
    pi = corpus(36, O.L2, 24)
    ix = P.DiskAnnIndex.upload(gpu_ctx, codes=None, nbrs=pi.nbrs, heap_tids=pi.tids, vecs=pi.vecs, mean=None, m2=None, count=0, bits=None,
                               dim_index=36, num_neighbors=24, distance_type=O.L2, default_start=INV, storage_type=P._lib.VS_STORAGE_PLAIN)
    pool = P.ScanPool(ix, 2, search_list_size=20, rescore=0, kmax=6, rows_cap=64)
    try:
        assert pool.info()["kernel"] == FAST_PLAIN
        pool.rescan(1, queries(1, 36)[0])
        for _ in range(2):
            rows, ids, _, _ = pool.fetch([1], 6)
            assert rows[0] == 0
        st = pool.stats(1)
        for key in ("visited_nodes", "candidate_nodes", "full_distance_comparisons", "node_reads"):
            assert st[key] == 0, key
    finally:
        pool.close()
        ix.close()
    # n = 3
    tiny = PlainIndex(n=3, dim=12, R=4, distance=O.L2, seed=5, kind="uniform")
    tiny.oracle = _oracle_of(tiny)
    ix = tiny.upload(gpu_ctx)
    q = make_vectors(2, 12, 6, "uniform")
    pool = P.ScanPool(ix, 2, search_list_size=3, rescore=0, kmax=8, rows_cap=64)
    try:
        assert pool.info()["kernel"] == FAST_PLAIN
        for i in range(2):
            pool.rescan(i, q[i])
        oscans = [tiny.oracle.scan(q[i], L=3, rescore=0) for i in range(2)]
        for kk in (2, 8, 8):
            rows, ids, tids, dist = pool.fetch([0, 1], kk)
            for i in range(2):
                check_chunk(int(rows[i]), ids[i], tids[i], dist[i], oscans[i], kk, ("tiny", kk, i))
                check_stats(pool, i, oscans[i], ("tiny", kk, i))
    finally:
        pool.close()
        ix.close()
    # a start node with a deleted tid
    dead = PlainIndex.__new__(PlainIndex)
    dead.__dict__.update(pi.__dict__)
    dead.tids = pi.tids.copy()
    dead.tids[dead.start] &= ~np.uint64(0xFFFF)
    dead.oracle = _oracle_of(dead)
    ix = dead.upload(gpu_ctx)
    q = queries(3, 36)
    pool = P.ScanPool(ix, 3, search_list_size=10, rescore=0, kmax=10, rows_cap=64)
    try:
        assert pool.info()["kernel"] == FAST_PLAIN
        for i in range(3):
            pool.rescan(i, q[i])
        oscans = [dead.oracle.scan(q[i], L=10, rescore=0) for i in range(3)]
        for _ in range(2):
            rows, ids, tids, dist = pool.fetch([0, 1, 2], 10)
            for i in range(3):
                assert rows[i] == 10 and (ids[i] != dead.start).all()
                check_chunk(10, ids[i], tids[i], dist[i], oscans[i], 10, ("dead start", i))
                check_stats(pool, i, oscans[i], ("dead start", i))
    finally:
        pool.close()
        ix.close()


@pytest.mark.parametrize("prefetch", ["1", "0"])
def test_streaming_with_and_without_prefetched_rounds(gpu_ctx, oracle, prefetch):
    pi = corpus(36, O.L2, 24)
    ix = pi.upload(gpu_ctx)
    G, k = 8, 16
    q = queries(G, 36, seed=17)
    with options(VS_POOL_PREFETCH=prefetch):
        pool = P.ScanPool(ix, G, search_list_size=20, rescore=0, kmax=k, rows_cap=1024)
        try:
            assert pool.info()["kernel"] == FAST_PLAIN
            for i in range(G):
                pool.rescan(i, q[i])
            oscans = [pi.oracle.scan(q[i], L=20, rescore=0) for i in range(G)]
            for rnd in range(20):
                rows, ids, tids, dist = pool.fetch(list(range(G)), k)
                for i in range(G):
                    assert rows[i] == k
                    check_chunk(k, ids[i], tids[i], dist[i], oscans[i], k, (rnd, i))
                    check_stats(pool, i, oscans[i], (rnd, i))
            w = pool.work()
            assert w["rounds"] <= w["launches"] <= 2 * w["rounds"]
        finally:
            pool.close()
            ix.close()
