"""Shared expectations of the qualified scan-pool tests (tests/test_gpu_zz_pool_qual.py): one fetch restated on the oracle's scan —
amgettuple until k rows pass the qualifier, a call returns None, max_pops calls have returned a row, or the row budget is reached —
with the oracle's GreedySearchStats as they stand afterwards.  Nothing here looks at the library under test."""
import collections
import functools

import numpy as np

import qual_checks as QC

INV = 0xFFFFFFFF
COMPLETE, ENDED, CUT, BUDGET = 0, 1, 2, 3
CAPACITY = -4  # VS_ERR_CAPACITY
G = 12         # pool slots
STAT_KEYS = ("visited_nodes", "candidate_nodes", "quantized_distance_comparisons", "full_distance_comparisons", "node_reads",
             "node_heap_reads", "next_calls")  # the seven of tests/test_gpu_zt_scanpool.py

Page = collections.namedtuple("Page", "ids tids dist pops state stats")


def page(oscan, passes, k, max_pops, calls_left=None):
    """The next fetch of one scan.  passes: a bool per node (None: every node passes).  calls_left: the calls that may still return a
    row before the next one would stand on more stream rows than the pool's budget (None: no budget)."""
    ids, tids, dist, pops = [], [], [], 0
    while True:
        if len(ids) == k:
            state = COMPLETE
            break
        if pops == max_pops:
            state = CUT
            break
        if calls_left is not None and pops == calls_left:
            state = BUDGET
            break
        o = oscan.gettuple()
        if o is None:
            state = ENDED
            break
        pops += 1
        if passes is None or passes[o[0]]:
            ids.append(o[0])
            tids.append(o[1])
            dist.append(o[2])
    st = oscan.stats()
    return Page(np.array(ids, np.uint32), np.array(tids, np.uint64), np.array(dist, np.float32), pops, state, {key: st[key] for key in STAT_KEYS})


def assert_page(got, a, exp, where=""):
    """row `a` of what ScanPool.fetch_qual returned (rows, ids, tids, dist, pops, state, ..) against a Page; a plain fetch's
    (rows, ids, tids, dist) is checked as far as it goes"""
    rows, ids, tids, dist = got[:4]
    n = exp.ids.size
    assert rows[a] == n, (where, "rows", int(rows[a]), n)
    if len(got) > 4:
        assert got[4][a] == exp.pops, (where, "pops", int(got[4][a]), exp.pops)
        assert got[5][a] == exp.state, (where, "state", int(got[5][a]), exp.state)
    assert (ids[a, :n] == exp.ids).all(), (where, "ids", ids[a, :n], exp.ids)
    assert (tids[a, :n] == exp.tids).all(), (where, "tids")
    same = dist[a, :n].view(np.uint32) == exp.dist.view(np.uint32)
    assert (same | (np.isnan(dist[a, :n]) & np.isnan(exp.dist))).all(), (where, "distance bits")
    # entries past the rows are not written: the caller's prefill stands
    assert (ids[a, n:] == INV).all() and (tids[a, n:] == 0).all() and (dist[a, n:] == 0).all(), (where, "past the rows")


def assert_stats(got, exp, where=""):
    for key in STAT_KEYS:
        assert got[key] == exp.stats[key], (where, key, got[key], exp.stats[key])


def a_queries():
    return QC.index_a().queries(G + 2, seed=31)


@functools.lru_cache(maxsize=None)
def a_pages(pages=4, k=QC.A_K, max_pops=512):
    """case A of the issue: per pool slot the oracle's `pages` successive fetches under the 0.10 qualifier — computed once, shared by
    every run of the pages test"""
    ti, bits, q = QC.index_a(), QC.qual_a(), a_queries()
    out = []
    for i in range(G):
        oscan = ti.oracle.scan(q[i], L=QC.A_L, rescore=QC.A_RESCORE)
        out.append(tuple(page(oscan, bits, k, max_pops) for _ in range(pages)))
        oscan.close()
    return tuple(out)
