"""Shared expectations of the qualified-scan tests (tests/test_gpu_zz_qual.py): the oracle's rows post-filtered on the host, which is
the reference's own way to an `ORDER BY ... LIMIT k` under a WHERE clause, and the rounds a batch must have run given the oracle's pop
counts.  Nothing here looks at the library under test."""
import functools

import numpy as np

from helpers import TestIndex
from oracle import oracle_py as O

INV = 0xFFFFFFFF
COMPLETE, ENDED, CUT = 0, 1, 2
NQ = 48
# case A of the issue: n is no multiple of 64 (the last word of a bitmap is partial), a qualifier of density 0.10
A_KW = dict(n=2037, dim_full=64, R=16, distance=O.L2, seed=3, L_build=30)
A_L, A_RESCORE, A_K = 20, 10, 10
# case C: a tiny index whose every scan ends, a qualifier of 6 nodes
C_KW = dict(n=300, dim_full=64, R=16, distance=O.L2, seed=3, L_build=30)
C_L, C_RESCORE, C_K, C_MAX_POPS = 30, 50, 10, 512


@functools.lru_cache(maxsize=None)
def index_a(deleted_frac=0.0):
    return TestIndex(deleted_frac=deleted_frac, **A_KW)


@functools.lru_cache(maxsize=None)
def index_c():
    return TestIndex(**C_KW)


def qual_a(n=2037):
    return np.random.default_rng(11).random(n) < 0.10


def qual_c():
    b = np.zeros(300, bool)
    b[np.random.default_rng(12).choice(300, 6, replace=False)] = True
    return b


def words_of(bits, garbage_tail=False):
    """a bool array per node -> uint64 words, node i at bit i & 63 of word i >> 6; garbage_tail: ones at every position >= n"""
    pad = -bits.size % 64
    tail = np.ones(pad, bool) if garbage_tail else np.zeros(pad, bool)
    return np.packbits(np.concatenate([bits.astype(bool), tail]), bitorder="little").view(np.uint64).copy()


@functools.lru_cache(maxsize=64)
def _oracle_rows(oracle_index, qkey, L, rescore, max_pops, lkey):
    q = np.frombuffer(qkey[0], np.float32).reshape(qkey[1])
    return oracle_index.search_batch(q, L=L, rescore=rescore, k=max_pops, qlabels=None if lkey is None else [list(l) for l in lkey])


def expect(oracle_index, tids, q, quals, slots, L, rescore, k, max_pops, qlabels=None):
    """The contract restated: per scan the oracle's first max_pops rows (under whatever mask is in force on the oracle), kept where
    the scan's qualifier (quals[slot], a bool array per node; slot 0: all) has the node's bit, cut at k.
    -> ids, tids, dist [nq, k], rows, pops, state [nq], and all_pops [nq] (rows the oracle's scan has within max_pops)."""
    q = np.ascontiguousarray(q, np.float32)
    if oracle_index.visible is None:  # (the cache must not outlive a mask)
        lkey = None if qlabels is None else tuple(tuple(l) for l in qlabels)
        oi, od, _ = _oracle_rows(oracle_index, (q.tobytes(), q.shape), L, rescore, max_pops, lkey)
    else:
        oi, od, _ = oracle_index.search_batch(q, L=L, rescore=rescore, k=max_pops, qlabels=qlabels)
    nq = q.shape[0]
    ids = np.full((nq, k), INV, np.uint32)
    tid = np.zeros((nq, k), np.uint64)
    dist = np.full((nq, k), np.nan, np.float32)
    rows, pops, state, allp = (np.zeros(nq, np.uint32) for _ in range(4))
    for s in range(nq):
        live = oi[s] != INV
        total = int(live.sum())
        assert (~live[total:]).all()  # rows, then nothing but the end
        allp[s] = total
        ok = np.ones(total, bool) if slots[s] == 0 else quals[int(slots[s])][oi[s, :total]]
        hit = np.flatnonzero(ok)[:k]
        ids[s, :hit.size] = oi[s, hit]
        tid[s, :hit.size] = tids[oi[s, hit]]
        dist[s, :hit.size] = od[s, hit]
        rows[s] = hit.size
        if hit.size == k:
            state[s], pops[s] = COMPLETE, hit[-1] + 1
        elif total < max_pops:
            state[s], pops[s] = ENDED, total
        else:
            state[s], pops[s] = CUT, max_pops
    return ids, tid, dist, rows, pops, state, allp


def assert_equal(got, exp, what=""):
    gi, gt, gd, grows, gpops, gstate = got[:6]
    ei, et, ed, erows, epops, estate = exp[:6]
    assert (grows == erows).all(), (what, "rows", np.flatnonzero(grows != erows)[:8], grows[:8], erows[:8])
    assert (gstate == estate).all(), (what, "state", np.flatnonzero(gstate != estate)[:8])
    assert (gpops == epops).all(), (what, "pops", np.flatnonzero(gpops != epops)[:8], gpops[:8], epops[:8])
    assert (gi == ei).all(), (what, "ids", np.argwhere(gi != ei)[:8])
    assert (gt == et).all(), (what, "tids")
    assert (gd.view(np.uint32) == ed.view(np.uint32)).all(), (what, "distance bits")
    # past the rows: VS_INVALID_NODE / 0 / NaN
    for s in range(gi.shape[0]):
        assert (gi[s, grows[s]:] == INV).all() and (gt[s, grows[s]:] == 0).all() and np.isnan(gd[s, grows[s]:]).all()


def rounds_implied(exp, first_pops, max_pops):
    """(rounds, scans_rerun, pops_launched) of a batch whose first round runs P1 pops and every later one twice as many, up to
    max_pops: a scan is done after a round at P pops iff it is complete within P, or its scan ends within P, or P == max_pops"""
    rows, pops, state, allp = exp[3], exp[4], exp[5], exp[6]
    left = np.ones(rows.size, bool)
    P, rounds, rerun, launched = int(first_pops), 0, 0, 0
    while True:
        m = int(left.sum())
        rounds += 1
        launched += m * P
        if rounds > 1:
            rerun += m
        done = ((state == COMPLETE) & (pops <= P)) | (allp < P) | (P == max_pops)
        left &= ~done
        if not left.any() or P == max_pops:
            return rounds, rerun, launched
        P = min(2 * P, max_pops)
