"""Grouped scans (vs_index_groups_*, vs_search_batch_grouped / _dev_grouped): the first k rows of a scan with at most per_group rows per
group.  Expected everywhere: the header's rule ("grouped scans") restated in plain Python over the oracle's first max_pops rows; ids, tids,
distance BITS, rows, pops and states must all be equal.  Also runs on the lockstep interpreter (tests/test_emu_grouped.py)."""
import itertools

import numpy as np
import pytest

import qual_checks as QC
from helpers import Corpus, TestIndex, make_vectors, tie_vectors
from oracle import oracle_py as O
from qual_checks import A_L, COMPLETE, CUT, ENDED, INV, NQ
from test_gpu_zz_qual import options, uploaded

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
INVALID, STATE, NONE = -1, -5, 0xFFFFFFFF


def expect(oracle_index, tids, q, groups, per_group, k, max_pops, L, rescore, quals=None, slots=None, qlabels=None):
    """the rule restated over the oracle's first max_pops rows -> what QC.expect returns"""
    nq = q.shape[0]
    slots = np.zeros(nq, np.uint32) if slots is None else slots
    oi, ot, od, allp = (QC.expect(oracle_index, tids, q, {}, np.zeros(nq, np.uint32), L, rescore, max_pops, max_pops, qlabels=qlabels)[i] for i in (0, 1, 2, 6))
    ids, tid, dist = np.full((nq, k), INV, np.uint32), np.zeros((nq, k), np.uint64), np.full((nq, k), np.nan, np.float32)
    rows, pops, state = (np.zeros(nq, np.uint32) for _ in range(3))
    for s in range(nq):
        hit, held = [], {}
        for i in range(int(allp[s])):
            node = int(oi[s, i])
            g = int(groups[node])
            if (slots[s] and not quals[int(slots[s])][node]) or (g != NONE and held.get(g, 0) >= per_group):
                continue
            held[g] = held.get(g, 0) + 1
            hit.append(i)
            if len(hit) == k:
                break
        ids[s, :len(hit)], tid[s, :len(hit)], dist[s, :len(hit)], rows[s] = oi[s, hit], ot[s, hit], od[s, hit], len(hit)
        state[s], pops[s] = (COMPLETE, hit[-1] + 1) if len(hit) == k else (ENDED, allp[s]) if allp[s] < max_pops else (CUT, max_pops)
    return ids, tid, dist, rows, pops, state, allp


def layout(name, n=2037):
    rng = np.random.default_rng(31)
    if name == "forty":  # groups repeat in every window
        return rng.integers(0, 40, n).astype(np.uint32)
    if name == "distinct":  # the rule never bites
        return rng.permutation(n).astype(np.uint32)
    g = rng.integers(0, 40, n).astype(np.uint32)  # "none": a tenth ungrouped, the values 0 and 0xFFFFFFFE present
    g[g == 39] = 0xFFFFFFFE
    g[rng.random(n) < 0.10] = NONE
    return g


def run(ix, q, k, per_group, max_pops, L, rescore, **kw):
    return ix.search_batch_grouped(q, k=k, per_group=per_group, max_pops=max_pops, search_list_size=L, rescore=rescore, **kw)


def check(got, exp, max_pops, what=""):
    QC.assert_equal(got, exp, what)
    qst = got[7]
    assert (qst["complete"], qst["ended"], qst["cut"]) == tuple(int((exp[5] == s).sum()) for s in (COMPLETE, ENDED, CUT)), qst
    assert (qst["rounds"], qst["scans_rerun"], qst["pops_launched"]) == QC.rounds_implied(exp, qst["first_pops"], max_pops), qst


@pytest.fixture(scope="module")
def ix_a(gpu_ctx, oracle):
    with uploaded(gpu_ctx, QC.index_a()) as ix:
        yield ix


SIZES = [(pg, k, mp, rs) for pg, k, big, rs in itertools.product((1, 3), (10, 70), (False, True), (10, 50)) for mp in [512 if big else k]]
# 3 050 stream rows x 8 bytes of distances and groups pass the fused kernel's 24 KB; 40 groups hold no 70 rows of an index of 2 037: every scan ENDS
ABOVE_THE_LINE = (1, 70, 3000, 50)


def test_the_expectations_cover_every_state(oracle):
    ti, seen = QC.index_a(), set()
    for name, (pg, k, mp, rs) in itertools.product(("forty", "distinct", "none"), SIZES):
        seen |= set(int(s) for s in expect(ti.oracle, ti.tids, ti.queries(NQ), layout(name), pg, k, mp, A_L, rs)[5])
    pg, k, mp, rs = ABOVE_THE_LINE
    seen |= set(int(s) for s in expect(ti.oracle, ti.tids, ti.queries(8), layout("forty"), pg, k, mp, A_L, rs)[5])
    assert seen == {COMPLETE, ENDED, CUT}


@pytest.mark.parametrize("per_group,k,max_pops,rescore", SIZES)
@pytest.mark.parametrize("name", ["forty", "distinct", "none"])
def test_rule(ix_a, name, per_group, k, max_pops, rescore):
    ti, g, q = QC.index_a(), layout(name), QC.index_a().queries(NQ)
    ix_a.groups_put(g)
    assert (ix_a.groups_get() == g).all()
    exp = expect(ti.oracle, ti.tids, q, g, per_group, k, max_pops, A_L, rescore)
    assert not (name == "forty" and per_group == 1 and k == 70 and (exp[5] == COMPLETE).any())  # 40 groups hold no 70 rows
    check(run(ix_a, q, k, per_group, max_pops, A_L, rescore), exp, max_pops)


@pytest.mark.parametrize("k", [10, 70])
def test_per_group_k_is_the_qualified_scan_and_the_plain_first_k(ix_a, k):
    ti = QC.index_a()
    q, bits, slots = ti.queries(NQ), QC.qual_a(), np.ones(NQ, np.uint32)
    ix_a.groups_put(layout("forty"))
    ix_a.qual_put(1, bits)
    got = run(ix_a, q, k, k, 256, A_L, 10, qual_slots=slots)
    check(got, QC.expect(ti.oracle, ti.tids, q, {1: bits}, slots, A_L, 10, k, 256), 256)
    qual = ix_a.search_batch_qual(q, slots, k=k, max_pops=256, search_list_size=A_L, rescore=10)
    QC.assert_equal(got, qual)
    assert got[7] == qual[7]
    plain = ix_a.search_batch(q, search_list_size=A_L, rescore=10, k=k)
    got = run(ix_a, q, k, k, k, A_L, 10)
    assert all((x.view(np.uint32) == y.view(np.uint32)).all() for x, y in zip(got[:3], plain[:3])) and (got[3] == k).all() and (got[4] == k).all() and (got[5] == COMPLETE).all()


def test_a_qualifier_of_density_a_tenth_with_forty_groups(ix_a):
    ti, g = QC.index_a(), layout("forty")
    q, bits, slots = ti.queries(NQ), QC.qual_a(), np.ones(NQ, np.uint32)
    ix_a.groups_put(g)
    ix_a.qual_put(1, bits)
    exp = expect(ti.oracle, ti.tids, q, g, 1, 10, 512, A_L, 10, quals={1: bits}, slots=slots)
    assert (exp[4] > 100).any()  # (rows that fail the qualifier do not count against their group: the scans go far)
    check(run(ix_a, q, 10, 1, 512, A_L, 10, qual_slots=slots), exp, 512)


def test_a_tie_heavy_corpus_runs_the_rule_inside_the_replay(gpu_ctx, oracle):
    co = Corpus(tie_vectors(900, 40, 64, 5), distance=O.L2, R=16, L_build=30)
    q, g = tie_vectors(NQ, 40, 64, 6), layout("forty", 900)
    exp = expect(co.oracle, co.tids, q, g, 2, 10, 96, 20, 16)
    assert (exp[2][:, 1:].view(np.uint32) == exp[2][:, :-1].view(np.uint32))[exp[0][:, 1:] != INV].mean() > 0.2  # equal distances abound
    with uploaded(gpu_ctx, co) as ix:
        ix.groups_put(g)
        check(run(ix, q, 10, 2, 96, 20, 16), exp, 96)


@pytest.mark.parametrize("how", ["unfused", "forced_replay", "rescore_0", "above_the_line"])
def test_the_fallback_kernel_and_the_forced_replay(ix_a, how):
    ti, g = QC.index_a(), layout("forty" if how == "above_the_line" else "none")
    q = ti.queries(NQ if how != "above_the_line" else 8)
    pg, k, mp, rs = ABOVE_THE_LINE if how == "above_the_line" else (3, 70, 512, 0 if how == "rescore_0" else 10)
    ix_a.groups_put(g)
    exp = expect(ti.oracle, ti.tids, q, g, pg, k, mp, A_L, rs)
    opts = {"unfused": dict(VS_RERANK_FUSED="0"), "forced_replay": dict(VS_RERANK_FUSED="2"), "above_the_line": dict(VS_GROUP_FIRST_POPS=mp)}.get(how, {})
    with options(**opts):
        got = run(ix_a, q, k, pg, mp, A_L, rs)
    check(got, exp, mp)
    assert how != "above_the_line" or got[7]["first_pops"] == mp  # (else round 1 would have fitted the fused kernel)


@pytest.mark.parametrize("how", ["fused", "unfused", "forced_replay", "rescore_0"])
def test_tombstones_and_a_mask_do_not_count_against_a_group(gpu_ctx, oracle, how):
    """5 % of the rows deleted and 10 % hidden by a mask: such a row is no row of the scan, so it takes no place in its group.  With
    rescore 0 the reference never fetches the heap, so the mask hides nothing there; a tombstone is no row of the scan even so."""
    ti, g, q = QC.index_a(deleted_frac=0.05), layout("forty"), QC.index_a(deleted_frac=0.05).queries(NQ)
    vis = (np.random.default_rng(41).random(ti.n) > 0.10).astype(np.uint8)
    pg, k, mp, rs = 1, 10, 128, 0 if how == "rescore_0" else 10
    opts = {"unfused": dict(VS_RERANK_FUSED="0"), "forced_replay": dict(VS_RERANK_FUSED="2")}.get(how, {})
    with uploaded(gpu_ctx, ti) as ix:
        # precondition, on the reference alone: with the filter off — no mask, the same graph without a tombstone — the rows differ,
        # and rows the filter takes out were among them
        unfiltered = QC.index_a()
        assert (unfiltered.oracle.nbrs == ti.oracle.nbrs).all() and (unfiltered.tids != ti.tids).any()
        off = expect(unfiltered.oracle, ti.tids, q, g, pg, k, mp, A_L, rs)
        unmasked = expect(ti.oracle, ti.tids, q, g, pg, k, mp, A_L, rs)
        ti.oracle.set_visibility(vis)
        exp = expect(ti.oracle, ti.tids, q, g, pg, k, mp, A_L, rs)
        dead, hidden = (ti.tids & np.uint64(0xFFFF)) == 0, vis == 0
        took, kept = off[0][off[0] != INV], exp[0][exp[0] != INV]
        assert (off[0] != exp[0]).any() and dead[took].any() and hidden[took].any() and not dead[kept].any()
        if rs:
            assert (unmasked[0] != exp[0]).any() and not hidden[kept].any()
        else:
            assert (unmasked[0] == exp[0]).all() and (unmasked[4] == exp[4]).all() and hidden[kept].any()
        ix.set_visibility(vis)
        ix.groups_put(g)
        with options(**opts):
            check(run(ix, q, k, pg, mp, A_L, rs), exp, mp)


def test_a_plain_index(gpu_ctx, oracle):
    from test_gpu_zy_plain import PlainIndex
    pi = PlainIndex(n=1000, dim=96, R=24, distance=O.L2, seed=120, kind="gauss", dim_index=None)
    q, g = make_vectors(NQ, 96, 3, "gauss"), layout("forty", 1000)
    exp = expect(pi.oracle, pi.tids, q, g, 1, 10, 128, 30, 20)
    with uploaded(gpu_ctx, pi) as ix:
        ix.groups_put(g)
        check(run(ix, q, 10, 1, 128, 30, 20), exp, 128)


def test_the_device_entry_point_at_another_first_pops_and_a_batch_in_flight(gpu_ctx, ix_a):
    ti, g, k, q = QC.index_a(), layout("forty"), 10, QC.index_a().queries(NQ)
    exp = expect(ti.oracle, ti.tids, q, g, 1, k, 512, A_L, 10)  # (test_rule[forty-1-10-512-10] holds the default P1, 10, to the same rows)
    bufs = [gpu_ctx.alloc(s) for s in (q.nbytes, g.nbytes, NQ * k * 4, NQ * k * 8, NQ * k * 4, NQ * 4, NQ * 4, NQ * 4)]
    dq, dg, d_ids, d_tids, d_dist, d_rows, d_pops, d_state = bufs
    try:
        gpu_ctx.upload(dg, g)
        ix_a.groups_put_dev(dg)
        gpu_ctx.upload(dq, q)
        with options(VS_GROUP_FIRST_POPS=12):
            launch = lambda: ix_a.search_batch_dev_grouped(dq, NQ, A_L, 10, k, 1, None, 512, d_ids, d_rows, d_pops, d_state, d_out_tids=d_tids, d_out_dist=d_dist)
            launch()
            for f in (launch, lambda: run(ix_a, q, k, 1, 512, A_L, 10), lambda: ix_a.groups_put(g), lambda: ix_a.groups_patch(0, g[:4]), ix_a.groups_get, ix_a.groups_drop):
                with pytest.raises(Exception, match="in flight") as e:  # (each refused: the batch in flight goes on)
                    f()
                assert e.value.code == STATE
            st, qst = ix_a.search_batch_dev_grouped_finish()
        got = [gpu_ctx.download(b, np.empty(sh, t)) for b, sh, t in ((d_ids, (NQ, k), np.uint32), (d_tids, (NQ, k), np.uint64), (d_dist, (NQ, k), np.float32),
                                                                     (d_rows, NQ, np.uint32), (d_pops, NQ, np.uint32), (d_state, NQ, np.uint32))]
        check(got + [st, qst], exp, 512)
        assert qst["first_pops"] == 12 and qst["rounds"] > 1 and st["queries"] == NQ + qst["scans_rerun"]
    finally:
        for b in bufs:
            gpu_ctx.free(b)


def test_a_host_batch_cut_into_chunks_with_mixed_slots(ix_a):
    ti, g, q = QC.index_a(), layout("forty"), QC.index_a().queries(NQ)
    quals = {1: QC.qual_a(), 5: np.random.default_rng(17).random(ti.n) < 0.5}
    slots = np.array([(0, 1, 5)[i % 3] for i in range(NQ)], np.uint32)
    ix_a.groups_put(g)
    for sl, b in quals.items():
        ix_a.qual_put(sl, b)
    exp = expect(ti.oracle, ti.tids, q, g, 3, 10, 256, A_L, 10, quals=quals, slots=slots)
    with options(VS_HOST_CHUNK_MIN=20, VS_GROUP_FIRST_POPS=25):
        got = run(ix_a, q, 10, 3, 256, A_L, 10, qual_slots=slots)
    QC.assert_equal(got, exp)
    assert got[7]["rounds"] >= 3


def test_a_labeled_index_with_scan_keys(gpu_ctx, oracle):
    ti = TestIndex(n=1200, dim_full=64, R=16, distance=O.L2, seed=4, L_build=30, n_labels=6)
    rng = np.random.default_rng(15)
    q, g = ti.queries(NQ), layout("forty", 1200)
    keys = [sorted(set(int(v) for v in rng.integers(1, 7, int(rng.integers(1, 3))))) for _ in range(NQ)]
    exp = expect(ti.oracle, ti.tids, q, g, 1, 10, 128, A_L, 10, qlabels=keys)
    with uploaded(gpu_ctx, ti) as ix:
        ix.groups_put(g)
        with options(VS_GROUP_FIRST_POPS=12):  # (later rounds carry the label keys of the scans that are left)
            got = run(ix, q, 10, 1, 128, A_L, 10, qlabels=keys)
        check(got, exp, 128)
        assert got[7]["rounds"] > 1


def test_inserted_rows_are_unlimited_until_they_are_patched(gpu_ctx, oracle):
    ti = QC.index_c()
    with uploaded(gpu_ctx, ti) as ix:
        ix.groups_put(np.zeros(ti.n, np.uint32))
        cap0 = ix.capacity
        new = make_vectors(500, ti.dim_full, 77)
        ix.insert(new, ((np.arange(500, dtype=np.uint64) + 5000) << np.uint64(16)) | np.uint64(1), search_list_size=30)
        assert ix.capacity > cap0  # (the arrays have moved)
        now = ix.groups_get()
        assert now.size == ti.n + 500 and (now[:ti.n] == 0).all() and (now[ti.n:] == NONE).all()
        q = new[:NQ] + np.float32(0.001)
        got = run(ix, q, 5, 1, 64, 30, 10)
        assert ((got[0] < ti.n) & (got[0] != INV)).sum(1).max() <= 1 and ((got[0] >= ti.n) & (got[0] != INV)).sum(1).max() >= 2
        ix.groups_patch(ti.n, np.zeros(500, np.uint32))
        got = run(ix, q, 5, 1, 64, 30, 10)
        assert (got[3] == 1).all() and (got[5] == CUT).all()  # one group now: one row per scan


def test_compact_drops_the_column_and_the_refusals_leave_the_index_untouched(gpu_ctx, oracle):
    ti = QC.index_a(deleted_frac=0.05)
    q, g = ti.queries(8), layout("forty")

    def refused(code, match, f, *a, **kw):
        with pytest.raises(Exception, match=match) as e:
            f(*a, **kw)
        assert e.value.code == code

    with uploaded(gpu_ctx, ti) as ix:
        refused(STATE, "no group column", run, ix, q, 10, 1, 64, A_L, 10)
        refused(STATE, "no group column", ix.groups_get)
        ix.groups_put(g)
        before = run(ix, q, 10, 1, 64, A_L, 10)
        for pg in (0, 11):
            refused(INVALID, "per_group", run, ix, q, 10, pg, 64, A_L, 10)
        for mp in (9, 65537):
            refused(INVALID, "max_pops", run, ix, q, 10, 1, mp, A_L, 10)
        refused(INVALID, "slot 65", run, ix, q, 10, 1, 64, A_L, 10, qual_slots=np.full(8, 65, np.uint32))
        refused(STATE, "slot 2, which is empty", run, ix, q, 10, 1, 64, A_L, 10, qual_slots=np.full(8, 2, np.uint32))
        refused(INVALID, "VS_GROUP_MAX_K", run, ix, q, 8193, 1, 8193, A_L, 10)
        refused(INVALID, "reach past", ix.groups_patch, ti.n - 1, np.zeros(2, np.uint32))
        view = ix.view(gpu_ctx)
        try:
            refused(STATE, "view", run, view, q, 10, 1, 64, A_L, 10)
            refused(STATE, "view", view.groups_put, g)
        finally:
            view.close()
        assert (ix.groups_get() == g).all()
        QC.assert_equal(run(ix, q, 10, 1, 64, A_L, 10), before)
        ix.compact()
        refused(STATE, "no group column", run, ix, q, 10, 1, 64, A_L, 10)
        refused(STATE, "no group column", ix.groups_drop)
