"""Qualified scan pools (vs_scanpool_fetch_qual): a pooled scan continued to its next k rows that pass the qualifier the fetch names
for it.  Every test holds a pool to the oracle's scan (ti.oracle.scan): gettuple() until k rows pass, None, or max_pops rows
(tests/pool_qual_checks.py); node ids, heap tids, distance BITS, rows, pops, states and — after every fetch — the seven
GreedySearchStats counters must be equal.  Also runs on the lockstep interpreter (tests/test_emu_pool_qual.py)."""
import contextlib

import numpy as np
import pytest

import pool_qual_checks as PQ
import qual_checks as QC
from helpers import Corpus, TestIndex, make_vectors, tie_vectors
from oracle import oracle_py as O
from pool_qual_checks import BUDGET, CAPACITY, COMPLETE, CUT, ENDED, G
from qual_checks import A_K, A_L, A_RESCORE

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
INVALID, STATE = -1, -5


@contextlib.contextmanager
def options(**kv):
    import pgvectorscale_amd as P
    for name, v in kv.items():
        P.set_option(name, None if v is None else str(v))
    try:
        yield
    finally:
        for name in kv:
            P.set_option(name, None)


class Rig:
    """an uploaded index with its qualifiers, a pool of G scans over it and the oracle's scans of the same queries"""

    def __init__(self, gpu_ctx, ti, q, L, rescore, quals=None, labels=None, kmax=A_K, rows_cap=2048, vis=None, live=True):
        import pgvectorscale_amd as P
        self.ti, self.q, self.L, self.rescore, self.live = ti, q, L, rescore, live
        self.quals = dict(quals or {})
        self.labels = labels or [None] * G
        self.ix = ti.upload(gpu_ctx)
        self.pool = None
        try:
            if vis is not None:
                ti.oracle.set_visibility(vis)
                self.ix.set_visibility(vis)
            for sl, b in self.quals.items():
                self.ix.qual_put(sl, b)
            self.pool = P.ScanPool(self.ix, G, search_list_size=L, rescore=rescore, kmax=kmax, rows_cap=rows_cap)
            self.oscans = [None] * G
            for i in range(G):
                self.rescan(i, q[i])
        except BaseException:
            self.close()
            raise

    def rescan(self, i, query):
        self.pool.rescan(i, query, labels=self.labels[i])
        if self.live:
            self.oscans[i] = self.ti.oracle.scan(query, labels=self.labels[i], L=self.L, rescore=self.rescore)

    def check(self, got, a, i, exp, where):
        PQ.assert_page(got, a, exp, where)
        PQ.assert_stats(self.pool.stats(i), exp, where)

    def fetch_qual(self, who, k, qslots, max_pops, where="", calls_left=None):
        """one fetch_qual held to the oracle's scans; -> (what the pool returned, the expected pages)"""
        got = self.pool.fetch_qual(who, k, qslots, max_pops)
        exps = []
        for a, i in enumerate(who):
            passes = self.quals[int(qslots[a])] if qslots[a] else None
            exps.append(PQ.page(self.oscans[i], passes, k, max_pops, None if calls_left is None else calls_left[a]))
            self.check(got, a, i, exps[-1], (where, i))
        return got, exps

    def fetch(self, who, k, where=""):
        got = self.pool.fetch(who, k)
        for a, i in enumerate(who):
            self.check(got, a, i, PQ.page(self.oscans[i], None, k, k), (where, i))
        return got

    def close(self):
        self.ti.oracle.set_visibility(None)
        if self.pool is not None:
            self.pool.close()
        self.ix.close()


@contextlib.contextmanager
def rig(*a, **kw):
    r = Rig(*a, **kw)
    try:
        yield r
    finally:
        r.close()


ALL = list(range(G))
ONES = np.ones(G, np.uint32)


# ---- pages: four successive fetches of 10 qualifying rows per slot ---------------------------------------------------------------------
@pytest.mark.parametrize("fast,prefetch", [("1", "1"), ("1", "0"), ("0", "1"), ("0", "0")],
                         ids=["fast_prefetch", "fast", "general_prefetch", "general"])
@pytest.mark.parametrize("chunk", [None, 7], ids=["chunk_default", "chunk_7"])
@pytest.mark.parametrize("first", [None, 10, 512], ids=["p1_rule", "p1_10", "p1_512"])
def test_pages_of_ten_qualifying_rows(gpu_ctx, oracle, first, chunk, fast, prefetch):
    exp = PQ.a_pages()
    # preconditions on the oracle's side: pages that complete, at pop counts that differ from slot to slot and from page to page
    pops = np.array([[pg.pops for pg in slot] for slot in exp])
    assert all(pg.state == COMPLETE for slot in exp for pg in slot) and pops.min() >= A_K and pops.max() > 100 and len(set(pops.ravel())) > 20
    with options(VS_QUAL_FIRST_POPS=first, VS_POOL_QUAL_CHUNK=chunk, VS_POOL_FAST=fast, VS_POOL_PREFETCH=prefetch):
        with rig(gpu_ctx, QC.index_a(), PQ.a_queries(), A_L, A_RESCORE, quals={1: QC.qual_a()}, live=False) as r:
            total = 0
            for pg in range(4):
                got = r.pool.fetch_qual(ALL, A_K, ONES, 512)
                for i in ALL:
                    r.check(got, i, i, exp[i][pg], (pg, i))
                qst = got[6]
                total += qst["pops"]
                assert qst["pops"] == sum(exp[i][pg].pops for i in ALL) and qst["complete"] == G
                assert qst["ended"] == qst["cut"] == qst["budget"] == 0
                if first is not None:
                    assert qst["first_pops"] == first
                if first == 512 and chunk is None:
                    assert qst["window_launches"] == 1  # the rows of 512 pops are there: one launch serves the page
                if chunk == 7:
                    assert qst["window_launches"] >= -(-int(pops[:, pg].max()) // 7)  # launches end mid-page
            assert total == int(pops.sum())


def test_a_cut_scan_resumes_where_it_stopped(gpu_ctx, oracle):
    """max_pops = k = 10 again and again until a fetch is COMPLETE or the scan has ENDED: every fetch before that is CUT after exactly
    10 pops, nothing is lost or repeated on the way (each fetch is held to the oracle's scan), and the rows so gathered begin with the
    rows of ONE fetch_qual(max_pops=512) on a second pool"""
    ti, q, quals = QC.index_a(), PQ.a_queries(), {1: QC.qual_a()}
    with rig(gpu_ctx, ti, q, A_L, A_RESCORE, quals=quals) as r, rig(gpu_ctx, ti, q, A_L, A_RESCORE, quals=quals) as whole:
        one, _ = whole.fetch_qual(ALL, A_K, ONES, 512)
        assert (one[5] == COMPLETE).all() and (one[4] > A_K).all()
        rows = [[] for _ in ALL]
        left, steps = list(ALL), 0
        while left:
            got, _ = r.fetch_qual(left, A_K, np.ones(len(left), np.uint32), A_K, steps)
            nxt = []
            for a, i in enumerate(left):
                rows[i] += [(int(got[1][a, j]), int(got[2][a, j]), int(got[3][a, j].view(np.uint32))) for j in range(int(got[0][a]))]
                if got[5][a] == CUT:  # every intermediate state: cut after exactly max_pops = k pops
                    assert got[4][a] == A_K
                    nxt.append(i)
                else:
                    assert got[5][a] in (COMPLETE, ENDED)
            left, steps = nxt, steps + 1
        assert steps > 5
        for i in ALL:
            assert rows[i][:A_K] == [(int(one[1][i, j]), int(one[2][i, j]), int(one[3][i, j].view(np.uint32))) for j in range(A_K)], i


@pytest.mark.parametrize("first", [None, 16], ids=["p1_rule", "p1_16"])
def test_every_scan_ends_and_stays_ended(gpu_ctx, oracle, first):
    ti = QC.index_c()
    with options(VS_QUAL_FIRST_POPS=first):
        with rig(gpu_ctx, ti, ti.queries(G, seed=32), QC.C_L, QC.C_RESCORE, quals={1: QC.qual_c()}) as r:
            got, exps = r.fetch_qual(ALL, QC.C_K, ONES, QC.C_MAX_POPS, "first")
            assert (got[5] == ENDED).all() and (got[0] == 6).all() and (got[4] == 300).all()  # fewer than k rows: all six of them
            assert got[6]["ended"] == G
            got, _ = r.fetch_qual(ALL, QC.C_K, ONES, QC.C_MAX_POPS, "again")  # (stats: the oracle's after the extra None call)
            assert (got[5] == ENDED).all() and (got[0] == 0).all() and (got[4] == 0).all()
            r.fetch(ALL, 3, "plain, past the end")


# ---- extremes ---------------------------------------------------------------------------------------------------------------------------
def test_empty_full_slot_0_garbage_beyond_n_and_the_smallest_and_largest_k(gpu_ctx, oracle):
    ti, q = QC.index_a(), PQ.a_queries()
    bits = QC.qual_a()
    quals = {1: np.zeros(ti.n, bool), 2: np.ones(ti.n, bool), 3: bits}
    kmax = 16
    with rig(gpu_ctx, ti, q, A_L, A_RESCORE, quals=quals, kmax=kmax) as r, rig(gpu_ctx, ti, q, A_L, A_RESCORE, kmax=kmax) as twin:
        r.ix.qual_put(3, QC.words_of(bits, garbage_tail=True))  # (bits at positions >= n are the library's to clear)
        # an empty qualifier: no row passes, the scan is cut at max_pops
        got, _ = r.fetch_qual(ALL[:4], A_K, np.full(4, 1, np.uint32), 64, "empty")
        assert (got[0] == 0).all() and (got[4] == 64).all() and (got[5] == CUT).all() and got[6]["first_pops"] == 64
        # a full one and slot 0: vs_scanpool_fetch bit for bit, pops = rows
        for sl, who in ((2, ALL[4:8]), (0, ALL[8:12])):
            for k in (A_K, 1, kmax):
                got, _ = r.fetch_qual(who, k, np.full(4, sl, np.uint32), 128, ("full", sl, k))
                plain = twin.pool.fetch(who, k)
                assert (got[0] == plain[0]).all() and (got[0] == k).all() and (got[4] == k).all() and (got[5] == COMPLETE).all()
                assert (got[1] == plain[1]).all() and (got[2] == plain[2]).all() and (got[3].view(np.uint32) == plain[3].view(np.uint32)).all()
                assert got[6]["first_pops"] == k
        # k = 1 and k = kmax under the sparse qualifier, garbage past n and all
        for k in (1, kmax, 1):
            r.fetch_qual(ALL[:4], k, np.full(4, 3, np.uint32), 512, ("garbage tail", k))


# ---- mixed use ------------------------------------------------------------------------------------------------------------------------
def test_mixed_qualifiers_alternating_calls_subsets_and_a_rescan(gpu_ctx, oracle):
    ti, q = QC.index_a(), PQ.a_queries()
    quals = {1: QC.qual_a(), 5: np.random.default_rng(17).random(ti.n) < 0.5}
    rng = np.random.default_rng(33)
    with rig(gpu_ctx, ti, q, A_L, A_RESCORE, quals=quals) as r:
        seen = set()
        for rnd in range(14):
            who = ALL if rnd % 4 == 0 else [i for i in ALL if rng.random() < 0.5] or [3]
            if 2 not in who:  # slot 2 takes part in every round: fetch and fetch_qual alternate on it
                who = who + [2]
            if rnd % 2 == 1:
                r.fetch([2], int(rng.choice([1, 4, A_K])), ("plain", rnd))
                who = [i for i in who if i != 2] or [5]
            qslots = np.array([(0, 1, 5)[(i + rnd) % 3] for i in who], np.uint32)  # different qualifiers and none, in one fetch
            k = int(rng.choice([1, 3, A_K]))
            got, _ = r.fetch_qual(who, k, qslots, int(rng.choice([k, 40, 512])), ("qual", rnd))
            seen |= set(int(s) for s in got[5])
            if rnd == 6:  # one slot is rescanned with another query while the others go on
                r.rescan(1, q[G])
        assert seen >= {COMPLETE, CUT}


# ---- regimes --------------------------------------------------------------------------------------------------------------------------
def run_pages(r, qslot, pages=3, k=A_K, max_pops=512):
    states = set()
    for pg in range(pages):
        who = ALL if pg != 1 else ALL[::2]
        got, _ = r.fetch_qual(who, k, np.full(len(who), qslot, np.uint32), max_pops, pg)
        states |= set(int(s) for s in got[5])
    return states


def test_without_a_rescore_window(gpu_ctx, oracle):
    with options(VS_POOL_QUAL_CHUNK=33):
        with rig(gpu_ctx, QC.index_a(), PQ.a_queries(), A_L, 0, quals={1: QC.qual_a()}) as r:
            assert run_pages(r, 1) == {COMPLETE}
            r.fetch(ALL, 4, "plain")
            assert run_pages(r, 1, max_pops=30) >= {CUT}


def test_label_keys_keyed_and_unkeyed_scans_in_one_fetch(gpu_ctx, oracle):
    ti = TestIndex(n=1200, dim_full=64, R=16, distance=O.L2, seed=4, L_build=30, n_labels=6)
    rng = np.random.default_rng(15)
    keys = [None if i % 3 == 0 else sorted(set(int(v) for v in rng.integers(1, 7, int(rng.integers(1, 3))))) for i in range(G)]
    with rig(gpu_ctx, ti, ti.queries(G, seed=34), A_L, A_RESCORE, quals={1: rng.random(ti.n) < 0.2}, labels=keys) as r:
        assert COMPLETE in run_pages(r, 1)


def test_a_visibility_mask_over_deleted_rows(gpu_ctx, oracle):
    ti = QC.index_a(deleted_frac=0.05)
    vis = (np.random.default_rng(21).random(ti.n) >= 0.10).astype(np.uint8)
    with rig(gpu_ctx, ti, PQ.a_queries(), A_L, A_RESCORE, quals={1: QC.qual_a()}, vis=vis) as r:
        got, _ = r.fetch_qual(ALL, A_K, ONES, 512, "masked")
        ids = got[1][got[1] != PQ.INV]
        assert ids.size and vis[ids].all() and ((ti.tids[ids] & np.uint64(0xFFFF)) != 0).all()
        assert run_pages(r, 1, pages=2) == {COMPLETE}


def test_a_tie_heavy_corpus(gpu_ctx, oracle):
    co = Corpus(tie_vectors(900, 40, 64, 5), distance=O.L2, R=16, L_build=30)
    bits = np.random.default_rng(13).random(900) < 0.3
    with options(VS_POOL_QUAL_CHUNK=5):
        with rig(gpu_ctx, co, tie_vectors(G, 40, 64, 6), 20, 16, quals={1: bits}) as r:
            got, exps = r.fetch_qual(ALL, A_K, ONES, 96, "ties")
            d = np.concatenate([e.dist for e in exps if e.dist.size > 1])
            assert (d[1:].view(np.uint32) == d[:-1].view(np.uint32)).mean() > 0.2  # equal distances abound
            run_pages(r, 1, pages=2, max_pops=96)


@pytest.mark.parametrize("plain_fast", ["1", "0"], ids=["resumable_plain_kernel", "general_kernel"])
@pytest.mark.parametrize("dim_index", [None, 64], ids=["dim_index_eq_dim_full", "dim_index_lt_dim_full"])
def test_a_plain_index(gpu_ctx, oracle, dim_index, plain_fast):
    from test_gpu_zy_plain import PlainIndex
    pi = PlainIndex(n=1000, dim=96, R=24, distance=O.L2, seed=120, kind="gauss", dim_index=dim_index)
    bits = np.random.default_rng(16).random(pi.n) < 0.15
    with options(VS_POOL_PLAIN_FAST=plain_fast):
        with rig(gpu_ctx, pi, make_vectors(G, 96, 3, "gauss"), 30, 20, quals={1: bits}) as r:
            import pgvectorscale_amd as P
            assert (r.pool.info()["kernel"] == P._lib.VS_SEARCH_FAST_PLAIN) == (plain_fast == "1")
            assert COMPLETE in run_pages(r, 1)
            r.fetch(ALL, 5, "plain fetch")
            run_pages(r, 1, pages=1, max_pops=20)


# ---- the row budget -------------------------------------------------------------------------------------------------------------------
def test_the_row_budget_ends_a_fetch_with_the_rows_kept_so_far(gpu_ctx, oracle):
    ti, q = QC.index_a(), PQ.a_queries()
    bits = np.random.default_rng(35).random(ti.n) < 0.01
    rows_cap = 256
    budget = rows_cap - A_RESCORE + 1  # the calls that stand on no more than rows_cap stream rows
    for i in ALL:  # the oracle's own streams are clearly longer than the budget
        s = ti.oracle.scan(q[i], L=A_L, rescore=A_RESCORE)
        assert all(s.gettuple() is not None for _ in range(2 * rows_cap)), i
        s.close()
    with rig(gpu_ctx, ti, q, A_L, A_RESCORE, quals={1: bits}, rows_cap=rows_cap) as r:
        first = ALL[:6]
        r.fetch(first[:3], 7, "plain rows first")  # (three of them have made calls already: their budget is what is left)
        left = [budget - 7] * 3 + [budget] * 3
        got, exps = r.fetch_qual(first, A_K, ONES[:6], 512, "to the budget", calls_left=left)
        assert (got[5] == BUDGET).all() and (got[4] == left).all() and (got[0] < A_K).all() and got[6]["budget"] == 6
        assert sum(e.ids.size for e in exps) > 0  # rows were kept on the way
        # a slot at its budget can make no pop at all: VS_ERR_CAPACITY for it alone, the other slots of the fetch are served
        got = r.pool.fetch_qual(ALL, A_K, ONES, 100)
        assert (got[0][:6] == CAPACITY).all()
        for a in range(6, G):
            r.check(got, a, a, PQ.page(r.oscans[a], bits, A_K, 100), ("served", a))
        assert (got[5][6:] == CUT).all() and (got[4][6:] == 100).all()
        plain = r.pool.fetch(first, 1)
        assert (plain[0] == CAPACITY).all()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_move_no_cursor(gpu_ctx, oracle):
    import ctypes as C

    import pgvectorscale_amd as P
    ti, q = QC.index_a(), PQ.a_queries()
    quals = {1: QC.qual_a()}
    with rig(gpu_ctx, ti, q, A_L, A_RESCORE, quals=quals) as r, rig(gpu_ctx, ti, q, A_L, A_RESCORE, quals=quals) as twin:
        r.fetch_qual(ALL, 3, ONES, 64, "before")
        twin.fetch_qual(ALL, 3, ONES, 64, "before, twin")
        lib, h = r.pool._L, r.pool.h
        sl = (C.c_uint32 * 2)(0, 1)
        qs = (C.c_uint32 * 2)(1, 1)
        out = (C.c_uint32 * 64)()
        rows = (C.c_int32 * 2)()

        def raw(slots=sl, n=2, k=A_K, qslots=qs, max_pops=64, o_rows=rows, o_pops=out, o_state=out):
            return lib.vs_scanpool_fetch_qual(h, slots, n, k, qslots, max_pops, None, None, None, o_rows, o_pops, o_state, None)

        def refused(code, cause, **kw):
            assert raw(**kw) == code, (kw, lib.vs_last_error())
            assert cause in lib.vs_last_error(), (cause, lib.vs_last_error())
            # ... and a fetch returns exactly the rows of an untouched twin pool
            a, b = r.pool.fetch(ALL, 2), twin.pool.fetch(ALL, 2)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all() and (a[3].view(np.uint32) == b[3].view(np.uint32)).all()

        refused(INVALID, b"slots is NULL", slots=None)
        refused(INVALID, b"qual_slots is NULL", qslots=None)
        refused(INVALID, b"out_rows is NULL", o_rows=None)
        refused(INVALID, b"out_pops is NULL", o_pops=None)
        refused(INVALID, b"out_state is NULL", o_state=None)
        refused(INVALID, b"k must be", k=0)
        refused(INVALID, b"k 11 outside", k=A_K + 1, max_pops=64)
        refused(INVALID, b"max_pops 9 outside", max_pops=A_K - 1)
        refused(INVALID, b"max_pops 65537 outside", max_pops=65537)
        refused(INVALID, b"qualifier slot 65 outside", qslots=(C.c_uint32 * 2)(1, 65))
        refused(STATE, b"qualifier slot 2, which is empty", qslots=(C.c_uint32 * 2)(1, 2))
        refused(INVALID, b"slot 1 listed twice", slots=(C.c_uint32 * 2)(1, 1))
        r.pool.endscan(11)
        twin.pool.endscan(11)
        assert raw(slots=(C.c_uint32 * 2)(0, 11)) == INVALID and b"slot 11 is not an open scan" in lib.vs_last_error()
        assert raw(slots=(C.c_uint32 * 2)(0, G)) == INVALID and b"is not an open scan" in lib.vs_last_error()
        a, b = r.pool.fetch(ALL[:11], 2), twin.pool.fetch(ALL[:11], 2)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[3].view(np.uint32) == b[3].view(np.uint32)).all()
        # a pool on a view handle: slot 0 is served, a qualifier is the owner's
        view = r.ix.view(gpu_ctx)
        vpool = P.ScanPool(view, 2, search_list_size=A_L, rescore=A_RESCORE, kmax=A_K)
        try:
            vpool.rescan(0, q[0])
            vpool.rescan(1, q[1])
            with pytest.raises(P.VsError, match="view") as e:
                vpool.fetch_qual([0, 1], A_K, [0, 1], 64)
            assert e.value.code == STATE
            got = vpool.fetch_qual([0, 1], A_K, [0, 0], 64)
            for i in (0, 1):
                PQ.assert_page(got, i, PQ.page(ti.oracle.scan(q[i], L=A_L, rescore=A_RESCORE), None, A_K, 64), ("view", i))
        finally:
            vpool.close()
            view.close()
