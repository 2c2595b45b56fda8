"""Qualified scans (vs_index_qual_*, vs_search_batch_qual / _dev_qual): the first k rows of a scan whose node passes the qualifier the
scan names.  The expected value everywhere is the oracle's row sequence at k = max_pops, post-filtered on the host by the bitmap
(tests/qual_checks.py): node ids, heap tids, distance BITS, rows, pops and states must all be equal.  The oracle-side counts the issue
gives for its inputs are asserted as preconditions, so a drifting input cannot hollow a case out.  Also runs on the lockstep
interpreter (tests/test_emu_qual.py)."""
import contextlib

import numpy as np
import pytest

import qual_checks as QC
from helpers import Corpus, TestIndex, make_vectors, tie_vectors
from oracle import oracle_py as O
from qual_checks import A_K, A_L, A_RESCORE, COMPLETE, CUT, ENDED, INV, NQ

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
INVALID, STATE = -1, -5


@contextlib.contextmanager
def options(**kv):
    import pgvectorscale_amd as P
    for name, v in kv.items():
        P.set_option(name, v)
    try:
        yield
    finally:
        for name in kv:
            P.set_option(name, None)


@contextlib.contextmanager
def uploaded(gpu_ctx, ti):
    ix = ti.upload(gpu_ctx)
    try:
        yield ix
    finally:
        ti.oracle.set_visibility(None)
        ix.close()


def run(ix, q, slots, k, max_pops, L, rescore, **kw):
    return ix.search_batch_qual(q, slots, k=k, max_pops=max_pops, search_list_size=L, rescore=rescore, **kw)


def counts(exp):
    return tuple(int((exp[5] == s).sum()) for s in (COMPLETE, ENDED, CUT))


def check_stats(qst, exp, max_pops):
    assert (qst["complete"], qst["ended"], qst["cut"]) == counts(exp), qst
    assert (qst["rounds"], qst["scans_rerun"], qst["pops_launched"]) == QC.rounds_implied(exp, qst["first_pops"], max_pops), qst


# ---- case A: density 0.10, a partial last word, under three round rules ---------------------------------------------------------------
A_ORACLE = {256: ((48, 0, 0), (34, 163)), 128: ((44, 0, 4), None), 96: ((33, 0, 15), None), 64: ((7, 0, 41), None)}


@pytest.mark.parametrize("max_pops", [256, 128, 96, 64])
def test_case_a_under_three_round_rules(gpu_ctx, oracle, max_pops):
    ti = QC.index_a()
    q = ti.queries(NQ)
    bits = QC.qual_a()
    slots = np.ones(NQ, np.uint32)
    exp = QC.expect(ti.oracle, ti.tids, q, {1: bits}, slots, A_L, A_RESCORE, A_K, max_pops)
    # preconditions: what the oracle does with this input
    want_counts, pop_range = A_ORACLE[max_pops]
    assert counts(exp) == want_counts
    if pop_range:
        assert (int(exp[4].min()), int(exp[4].max())) == pop_range
    if max_pops in (128, 64):  # a scan whose 10th row is its max_pops-th pop exactly
        assert ((exp[5] == COMPLETE) & (exp[4] == max_pops)).any()
    if max_pops == 64:
        cut = exp[5] == CUT
        assert int(exp[3][cut].min()) == 1 and int(exp[3][cut].max()) == 9
    with uploaded(gpu_ctx, ti) as ix:
        ix.qual_put(1, bits)
        assert ix.qual_info(1) == {"n_nodes": ti.n, "n_set": int(bits.sum()), "tids_unmatched": 0}
        seen = []
        for first in (None, 10, max_pops):
            with options(VS_QUAL_FIRST_POPS=first):
                got = run(ix, q, slots, A_K, max_pops, A_L, A_RESCORE)
            QC.assert_equal(got, exp, f"first_pops {first}")
            qst = got[7]
            if first is not None:
                assert qst["first_pops"] == first
            assert A_K <= qst["first_pops"] <= max_pops
            check_stats(qst, exp, max_pops)
            seen.append(qst["rounds"])
        assert seen[2] == 1 and seen[1] >= 4  # one round when it starts at max_pops, many when it starts at k


@pytest.mark.parametrize("masked", [False, True], ids=["deleted_rows", "deleted_rows_and_a_mask"])
def test_case_a_with_deleted_rows_and_a_mask_in_force(gpu_ctx, oracle, masked):
    ti = QC.index_a(deleted_frac=0.05)
    q = ti.queries(NQ)
    bits = QC.qual_a()
    slots = np.ones(NQ, np.uint32)
    if not masked:
        exp = QC.expect(ti.oracle, ti.tids, q, {1: bits}, slots, A_L, A_RESCORE, A_K, 256)
        assert counts(exp) == (48, 0, 0) and (int(exp[4].min()), int(exp[4].max())) == (30, 155)
    with uploaded(gpu_ctx, ti) as ix:
        if masked:  # hidden rows stay out BEFORE the window (the oracle under set_visibility); the qualifier acts after the pop
            vis = (np.random.default_rng(21).random(ti.n) >= 0.10).astype(np.uint8)
            ti.oracle.set_visibility(vis)
            ix.set_visibility(vis)
            exp = QC.expect(ti.oracle, ti.tids, q, {1: bits}, slots, A_L, A_RESCORE, A_K, 256)
            assert not (exp[0][exp[0] != INV][:, None] == np.flatnonzero(vis == 0)[None, :]).any()
        ix.qual_put(1, bits)
        got = run(ix, q, slots, A_K, 256, A_L, A_RESCORE)
        QC.assert_equal(got, exp)
        check_stats(got[7], exp, 256)
        dead = (ti.tids & np.uint64(0xFFFF)) == 0
        assert not dead[got[0][got[0] != INV]].any()


# ---- case C: every scan ends ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescore", [QC.C_RESCORE, 0])
def test_case_c_every_scan_ends_with_six_rows(gpu_ctx, oracle, rescore):
    ti = QC.index_c()
    q = ti.queries(NQ)
    bits = QC.qual_c()
    slots = np.ones(NQ, np.uint32)
    exp = QC.expect(ti.oracle, ti.tids, q, {1: bits}, slots, QC.C_L, rescore, QC.C_K, QC.C_MAX_POPS)
    assert (exp[5] == ENDED).all() and (exp[4] == 300).all() and (exp[3] == 6).all()
    with uploaded(gpu_ctx, ti) as ix:
        ix.qual_put(1, bits)
        got = run(ix, q, slots, QC.C_K, QC.C_MAX_POPS, QC.C_L, rescore)
        QC.assert_equal(got, exp)
        check_stats(got[7], exp, QC.C_MAX_POPS)
        with options(VS_QUAL_FIRST_POPS=16):  # 16, 32, ..., 512: the end is found in the last round only
            again = run(ix, q, slots, QC.C_K, QC.C_MAX_POPS, QC.C_L, rescore)
        QC.assert_equal(again, exp)
        assert again[7]["rounds"] == 6


# ---- extremes ---------------------------------------------------------------------------------------------------------------------------
def test_empty_full_and_slot_0_and_garbage_beyond_n(gpu_ctx, oracle):
    ti = QC.index_a()
    q = ti.queries(NQ)
    with uploaded(gpu_ctx, ti) as ix:
        plain = ix.search_batch(q, search_list_size=A_L, rescore=A_RESCORE, k=A_K)
        ix.qual_put(1, np.zeros(ti.n, bool))
        ix.qual_put(2, np.ones(ti.n, bool))
        ix.qual_put(3, QC.words_of(QC.qual_a(), garbage_tail=True))
        ix.qual_put(4, np.full((ti.n + 63) // 64, 0xFFFFFFFFFFFFFFFF, np.uint64))
        # an empty qualifier: no rows, every scan cut (2037 rows are more than 64 pops)
        got = run(ix, q, np.full(NQ, 1, np.uint32), A_K, 64, A_L, A_RESCORE)
        assert (got[3] == 0).all() and (got[0] == INV).all() and np.isin(got[5], (CUT, ENDED)).all() and (got[4] == 64).all()
        assert got[7]["rounds"] == 1 and got[7]["first_pops"] == 64  # (nothing to wait for: straight to max_pops)
        # a full one and slot 0: vs_search_batch at k, bit for bit
        for sl in (2, 0, 4):
            got = run(ix, q, np.full(NQ, sl, np.uint32), A_K, 128, A_L, A_RESCORE)
            assert (got[0] == plain[0]).all() and (got[1] == plain[1]).all() and (got[2].view(np.uint32) == plain[2].view(np.uint32)).all(), sl
            assert (got[3] == A_K).all() and (got[4] == A_K).all() and (got[5] == COMPLETE).all()
            assert got[7]["rounds"] == 1 and got[7]["first_pops"] == A_K
            with options(VS_QUAL_FIRST_POPS=40):  # (a window of 40 pops that stops at its 10th kept row: the same rows)
                wide = run(ix, q, np.full(NQ, sl, np.uint32), A_K, 128, A_L, A_RESCORE)
            assert (wide[0] == plain[0]).all() and (wide[2].view(np.uint32) == plain[2].view(np.uint32)).all() and (wide[4] == A_K).all(), sl
        # bits at positions >= n are the library's to clear
        assert ix.qual_info(4)["n_set"] == ti.n and ix.qual_info(3)["n_set"] == int(QC.qual_a().sum())
        assert (ix.qual_download(3) == QC.qual_a()).all() and ix.qual_download(4).all()
        exp = QC.expect(ti.oracle, ti.tids, q, {3: QC.qual_a()}, np.full(NQ, 3, np.uint32), A_L, A_RESCORE, A_K, 256)
        QC.assert_equal(run(ix, q, np.full(NQ, 3, np.uint32), A_K, 256, A_L, A_RESCORE), exp)


def test_all_slots_0_at_max_pops_k_is_the_unqualified_launch(gpu_ctx, oracle):
    ti = QC.index_a()
    q = ti.queries(NQ)
    # (each on a fresh handle: a handle sizes its next launch from what its last batch needed)
    with uploaded(gpu_ctx, ti) as ix:
        plain = ix.search_batch(q, search_list_size=A_L, rescore=A_RESCORE, k=A_K)
        info = ix.last_search_info()
    with uploaded(gpu_ctx, ti) as ix:
        got = run(ix, q, np.zeros(NQ, np.uint32), A_K, A_K, A_L, A_RESCORE)
        assert ix.last_search_info() == info
        assert (got[0] == plain[0]).all() and (got[1] == plain[1]).all() and (got[2].view(np.uint32) == plain[2].view(np.uint32)).all()
        assert (got[3] == A_K).all() and (got[4] == A_K).all() and (got[5] == COMPLETE).all()
        assert got[6] == plain[3]  # the same work, counted the same
        assert got[7] == {"rounds": 1, "first_pops": A_K, "scans_rerun": 0, "pops_launched": NQ * A_K, "complete": NQ, "ended": 0, "cut": 0}


# ---- paths ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", ["0", "2"])
def test_case_a_on_the_unfused_pair_and_the_forced_replay(gpu_ctx, oracle, fused):
    ti = QC.index_a()
    q = ti.queries(NQ)
    bits = QC.qual_a()
    slots = np.ones(NQ, np.uint32)
    exp = QC.expect(ti.oracle, ti.tids, q, {1: bits}, slots, A_L, A_RESCORE, A_K, 128)
    with uploaded(gpu_ctx, ti) as ix:
        ix.qual_put(1, bits)
        with options(VS_RERANK_FUSED=fused, VS_QUAL_FIRST_POPS=40):
            QC.assert_equal(run(ix, q, slots, A_K, 128, A_L, A_RESCORE), exp)


def test_a_tie_heavy_corpus_runs_the_replay_under_a_qualifier(gpu_ctx, oracle):
    n = 900
    co = Corpus(tie_vectors(n, 40, 64, 5), distance=O.L2, R=16, L_build=30)
    q = tie_vectors(NQ, 40, 64, 6)
    bits = np.random.default_rng(13).random(n) < 0.3
    slots = np.ones(NQ, np.uint32)
    exp = QC.expect(co.oracle, co.tids, q, {1: bits}, slots, 20, 16, 10, 96)
    d = exp[2]
    assert (d[:, 1:].view(np.uint32) == d[:, :-1].view(np.uint32))[exp[0][:, 1:] != INV].mean() > 0.2  # equal distances abound
    with uploaded(gpu_ctx, co) as ix:
        ix.qual_put(1, bits)
        QC.assert_equal(run(ix, q, slots, 10, 96, 20, 16), exp)


def test_a_window_too_large_for_the_fused_kernel(gpu_ctx, oracle):
    """rescore 900 at up to 4 096 pops: a stream of 4 995 rows is beyond k_rerank_window (4 096), so k_rerank + k_resort run"""
    ti = QC.index_a()
    q = ti.queries(8)
    bits = np.random.default_rng(14).random(ti.n) < 0.004
    slots = np.ones(8, np.uint32)
    exp = QC.expect(ti.oracle, ti.tids, q, {1: bits}, slots, A_L, 900, 3, 4096)
    assert (exp[5] == ENDED).any() or (exp[4] > 1024).any()
    with uploaded(gpu_ctx, ti) as ix:
        ix.qual_put(1, bits)
        with options(VS_QUAL_FIRST_POPS=4096):
            QC.assert_equal(run(ix, q, slots, 3, 4096, A_L, 900), exp)


def test_a_labeled_index_with_scan_keys(gpu_ctx, oracle):
    ti = TestIndex(n=1200, dim_full=64, R=16, distance=O.L2, seed=4, L_build=30, n_labels=6)
    q = ti.queries(NQ)
    rng = np.random.default_rng(15)
    keys = [sorted(set(int(v) for v in rng.integers(1, 7, int(rng.integers(1, 3))))) for _ in range(NQ)]
    bits = rng.random(ti.n) < 0.2
    slots = np.ones(NQ, np.uint32)
    exp = QC.expect(ti.oracle, ti.tids, q, {1: bits}, slots, A_L, A_RESCORE, A_K, 128, qlabels=keys)
    assert (exp[5] == COMPLETE).sum() > 10
    with uploaded(gpu_ctx, ti) as ix:
        ix.qual_put(1, bits)
        with options(VS_QUAL_FIRST_POPS=12):  # (later rounds carry the label keys of the scans that are left)
            got = run(ix, q, slots, A_K, 128, A_L, A_RESCORE, qlabels=keys)
        QC.assert_equal(got, exp)
        check_stats(got[7], exp, 128)
        assert got[7]["rounds"] > 1


@pytest.mark.parametrize("dim_index", [None, 64], ids=["dim_index_eq_dim_full", "dim_index_lt_dim_full"])
def test_a_plain_index(gpu_ctx, oracle, dim_index):
    from test_gpu_zy_plain import PlainIndex
    pi = PlainIndex(n=1000, dim=96, R=24, distance=O.L2, seed=120, kind="gauss", dim_index=dim_index)
    q = make_vectors(NQ, 96, 3, "gauss")
    bits = np.random.default_rng(16).random(pi.n) < 0.15
    slots = np.ones(NQ, np.uint32)
    exp = QC.expect(pi.oracle, pi.tids, q, {1: bits}, slots, 30, 20, 10, 128)
    with uploaded(gpu_ctx, pi) as ix:
        ix.qual_put(1, bits)
        with options(VS_QUAL_FIRST_POPS=20):
            got = run(ix, q, slots, 10, 128, 30, 20)
        QC.assert_equal(got, exp)
        check_stats(got[7], exp, 128)


def test_the_device_resident_entry_point_with_device_slots(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    ti = QC.index_a()
    q = ti.queries(NQ)
    bits = QC.qual_a()
    slots = np.ones(NQ, np.uint32)
    exp = QC.expect(ti.oracle, ti.tids, q, {1: bits}, slots, A_L, A_RESCORE, A_K, 128)
    with uploaded(gpu_ctx, ti) as ix:
        words = QC.words_of(bits, garbage_tail=True)
        sizes = [q.nbytes, NQ * 4, NQ * A_K * 4, NQ * A_K * 8, NQ * A_K * 4, NQ * 4, NQ * 4, NQ * 4, words.nbytes]
        bufs = [gpu_ctx.alloc(s) for s in sizes]
        dq, ds, d_ids, d_tids, d_dist, d_rows, d_pops, d_state, d_bits = bufs
        try:
            gpu_ctx.upload(d_bits, words)
            ix.qual_put_dev(1, d_bits)
            assert ix.qual_info(1)["n_set"] == int(bits.sum()) and (ix.qual_download(1) == bits).all()
            gpu_ctx.upload(dq, q)
            gpu_ctx.upload(ds, slots)
            with options(VS_QUAL_FIRST_POPS=32):
                ix.search_batch_dev_qual(dq, NQ, A_L, A_RESCORE, A_K, ds, 128, d_ids, d_rows, d_pops, d_state, d_out_tids=d_tids, d_out_dist=d_dist)
                with pytest.raises(P.VsError, match="qualified") as e:  # its own finish runs the rounds that are left
                    ix.search_batch_dev_finish()
                assert e.value.code == STATE
                st, qst = ix.search_batch_dev_qual_finish()
            got = (gpu_ctx.download(d_ids, np.empty((NQ, A_K), np.uint32)), gpu_ctx.download(d_tids, np.empty((NQ, A_K), np.uint64)),
                   gpu_ctx.download(d_dist, np.empty((NQ, A_K), np.float32)), gpu_ctx.download(d_rows, np.empty(NQ, np.uint32)),
                   gpu_ctx.download(d_pops, np.empty(NQ, np.uint32)), gpu_ctx.download(d_state, np.empty(NQ, np.uint32)))
            QC.assert_equal(got, exp)
            check_stats(qst, exp, 128)
            assert st["queries"] == NQ + qst["scans_rerun"]  # (the device's work over all rounds, re-runs included)
            # a device slot that is empty is refused before anything is launched: no batch is in flight afterwards
            gpu_ctx.upload(ds, np.full(NQ, 9, np.uint32))
            with pytest.raises(P.VsError, match="slot 9") as e:
                ix.search_batch_dev_qual(dq, NQ, A_L, A_RESCORE, A_K, ds, 128, d_ids, d_rows, d_pops, d_state)
            assert e.value.code == STATE
            with pytest.raises(P.VsError, match="no qualified batch in flight"):
                ix.search_batch_dev_qual_finish()
        finally:
            for b in bufs:
                gpu_ctx.free(b)


def test_a_host_batch_cut_into_chunks_with_mixed_slots(gpu_ctx, oracle):
    """two qualifiers of different density and slot 0 in one batch, the batch cut into chunks of 20, 20 and 8 scans"""
    ti = QC.index_a()
    q = ti.queries(NQ)
    quals = {1: QC.qual_a(), 5: np.random.default_rng(17).random(ti.n) < 0.5}
    slots = np.array([(0, 1, 5)[i % 3] for i in range(NQ)], np.uint32)
    exp = QC.expect(ti.oracle, ti.tids, q, quals, slots, A_L, A_RESCORE, A_K, 128)
    assert (exp[4][slots == 0] == A_K).all() and exp[4][slots == 5].mean() < exp[4][slots == 1].mean()
    with uploaded(gpu_ctx, ti) as ix:
        for sl, b in quals.items():
            ix.qual_put(sl, b)
        one = run(ix, q, slots, A_K, 128, A_L, A_RESCORE)
        QC.assert_equal(one, exp, "one chunk")
        check_stats(one[7], exp, 128)
        with options(VS_HOST_CHUNK_MIN=20, VS_QUAL_FIRST_POPS=25):
            cut = run(ix, q, slots, A_K, 128, A_L, A_RESCORE)
        QC.assert_equal(cut, exp, "three chunks")
        assert cut[7]["rounds"] >= 3 and (cut[7]["complete"], cut[7]["ended"], cut[7]["cut"]) == counts(exp)


# ---- from_tids ------------------------------------------------------------------------------------------------------------------------
def test_from_tids_equals_a_numpy_restatement(gpu_ctx, oracle):
    ti = QC.index_a(deleted_frac=0.05)
    rng = np.random.default_rng(18)
    dead = np.flatnonzero((ti.tids & np.uint64(0xFFFF)) == 0)
    live = np.flatnonzero((ti.tids & np.uint64(0xFFFF)) != 0)
    assert dead.size > 50
    pick = rng.choice(live, 300, replace=False)
    stray = ((np.arange(40, dtype=np.uint64) + np.uint64(900000)) << np.uint64(16)) | np.uint64(3)  # tids no node carries
    # deleted nodes keep their block number: their old tid (offset 1) is in the list, and so is the tid they carry now (offset 0)
    gone = (ti.tids[dead[:30]] | np.uint64(1))
    lst = np.concatenate([ti.tids[pick], ti.tids[pick[:70]], stray, stray[:5], gone])
    rng.shuffle(lst)
    want = np.zeros(ti.n, bool)
    want[pick] = True
    carried = set(int(t) for t in ti.tids[live])
    unmatched = len(set(int(t) for t in lst) - carried)
    assert unmatched == 40 + 30
    with uploaded(gpu_ctx, ti) as ix:
        info = ix.qual_from_tids(1, lst)
        assert info == {"n_nodes": ti.n, "n_set": 300, "tids_unmatched": unmatched} and ix.qual_info(1) == info
        assert (ix.qual_download(1) == want).all()
        srt = np.sort(lst)  # (duplicates stay)
        d = gpu_ctx.alloc(srt.nbytes)
        try:
            gpu_ctx.upload(d, srt)
            assert ix.qual_from_tids_dev(2, d, srt.size) == info
        finally:
            gpu_ctx.free(d)
        assert (ix.qual_download(2) == want).all()
        assert ix.qual_from_tids(3, np.zeros(0, np.uint64)) == {"n_nodes": ti.n, "n_set": 0, "tids_unmatched": 0}
        assert not ix.qual_download(3).any()
        # ... and a search under it
        q = ti.queries(NQ)
        slots = np.ones(NQ, np.uint32)
        exp = QC.expect(ti.oracle, ti.tids, q, {1: want}, slots, A_L, A_RESCORE, 5, 128)
        QC.assert_equal(run(ix, q, slots, 5, 128, A_L, A_RESCORE), exp)


# ---- life cycle -----------------------------------------------------------------------------------------------------------------------
def test_inserted_rows_do_not_qualify_and_old_bits_survive_a_growth(gpu_ctx, oracle):
    ti = QC.index_c()
    bits = np.random.default_rng(19).random(ti.n) < 0.4
    with uploaded(gpu_ctx, ti) as ix:
        ix.qual_put(1, bits)
        ix.qual_put(7, ~bits)
        cap0 = ix.capacity
        new = make_vectors(500, ti.dim_full, 77)
        ix.insert(new, ((np.arange(500, dtype=np.uint64) + 5000) << np.uint64(16)) | np.uint64(1), search_list_size=30)
        assert ix.capacity > cap0 and ix.desc.n == ti.n + 500  # (the arrays have moved)
        for sl, b in ((1, bits), (7, ~bits)):
            now = ix.qual_download(sl)
            assert now.size == ti.n + 500 and (now[:ti.n] == b).all() and not now[ti.n:].any()
        # the rows of a qualified scan are old nodes carrying the bit; an unqualified one finds new rows among its first
        q = new[:NQ] + np.float32(0.001)
        got = run(ix, q, np.ones(NQ, np.uint32), 5, 256, 30, 10)
        ids = got[0][got[0] != INV]
        assert ids.size and (ids < ti.n).all() and bits[ids].all()
        free = ix.search_batch(q, search_list_size=30, rescore=10, k=5)
        assert (free[0] >= ti.n).any()
        assert ix.qual_info(1)["n_nodes"] == ti.n


def test_compact_drops_the_qualifiers(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    ti = QC.index_a(deleted_frac=0.05)
    with uploaded(gpu_ctx, ti) as ix:
        ix.qual_put(1, QC.qual_a())
        ix.compact()
        with pytest.raises(P.VsError, match="slot 1") as e:
            ix.qual_info(1)
        assert e.value.code == STATE
        with pytest.raises(P.VsError, match="slot 1, which is empty") as e:
            run(ix, ti.queries(4), np.ones(4, np.uint32), 5, 64, A_L, A_RESCORE)
        assert e.value.code == STATE
        ix.qual_put(1, np.ones(ix.desc.n, bool))  # (and a new one can be made for the new numbering)
        assert ix.qual_info(1)["n_set"] == ix.desc.n


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_index_untouched(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    ti = QC.index_a()
    q = ti.queries(8)
    bits = QC.qual_a()
    with uploaded(gpu_ctx, ti) as ix:
        ix.qual_put(1, bits)
        before = run(ix, q, np.ones(8, np.uint32), A_K, 128, A_L, A_RESCORE)
        for sl in (0, 65):
            with pytest.raises(P.VsError, match="slot") as e:
                ix.qual_put(sl, bits)
            assert e.value.code == INVALID
            with pytest.raises(P.VsError, match="slot") as e:
                ix.qual_from_tids(sl, ti.tids[:5])
            assert e.value.code == INVALID
        with pytest.raises(P.VsError, match="slot 2, which is empty") as e:
            run(ix, q, np.array([1, 1, 2, 1, 1, 1, 1, 1], np.uint32), A_K, 128, A_L, A_RESCORE)
        assert e.value.code == STATE
        with pytest.raises(P.VsError, match="slot 65") as e:
            run(ix, q, np.full(8, 65, np.uint32), A_K, 128, A_L, A_RESCORE)
        assert e.value.code == INVALID
        for bad in (A_K - 1, 65537):
            with pytest.raises(P.VsError, match="max_pops") as e:
                run(ix, q, np.ones(8, np.uint32), A_K, bad, A_L, A_RESCORE)
            assert e.value.code == INVALID
        with pytest.raises(P.VsError, match="holds no qualifier") as e:
            ix.qual_drop(2)
        assert e.value.code == STATE
        view = ix.view(gpu_ctx)
        try:
            with pytest.raises(P.VsError, match="view") as e:
                view.qual_put(2, bits)
            assert e.value.code == STATE
        finally:
            view.close()
        assert ix.qual_info(1)["n_set"] == int(bits.sum()) and (ix.qual_download(1) == bits).all()
        after = run(ix, q, np.ones(8, np.uint32), A_K, 128, A_L, A_RESCORE)
        QC.assert_equal(after, before)
        ix.qual_drop(1)
        with pytest.raises(P.VsError, match="which is empty"):
            run(ix, q, np.ones(8, np.uint32), A_K, 128, A_L, A_RESCORE)
