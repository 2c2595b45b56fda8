"""Scans of different snapshots in one launch: the class byte per node of vs_index_vis_base_eval, the per-snapshot overlays of
vs_index_vis_slot_eval, vs_index_vis_materialize and the searches that name a slot per scan (vs_search_batch_vis / _dev_vis).  The
corpus, the family of eight admissible snapshots and every expectation come from tests/vis_overlay_checks.py — a Python restatement of
the class rule of include/vsgpu.h over the reference walk of tests/heap_vis_checks.py — and from the oracle; every comparison is
exact.  Also runs on the lockstep interpreter (tests/test_emu_vis_overlay.py)."""
import contextlib
import os

import numpy as np
import pytest

import heap_vis_checks as V
import vis_overlay_checks as VO
from heap_vis_checks import INVALID, STATE, XMAX_COMMITTED
from helpers import make_vectors
from vis_overlay_checks import COUNTERS, K, L, RESCORE, SLOT_SNAP, SLOTS, WRAP_BASE

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
GENERAL, FAST_SBQ, FAST_PLAIN = 0, 1, 2
NQ = 48
SHAPES = [(600, 23, 0), (600, 23, WRAP_BASE), (1500, 31, WRAP_BASE)]
SHAPE_IDS = ["n600_low_xids", "n600_across_the_wrap", "n1500_across_the_wrap"]


@contextlib.contextmanager
def environ(**kv):
    saved = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def opened(gpu_ctx, oracle, w):
    """the world's index and resident heap fork on the device"""
    ti = w.index()
    ix = ti.upload(gpu_ctx)
    heap = VO.resident(gpu_ctx, w.rel)
    try:
        yield ti, ix, heap
    finally:
        ti.oracle.set_visibility(None)
        heap.close()
        ix.close()


def deal(nq):
    return np.array([SLOTS[i % len(SLOTS)] for i in range(nq)], np.uint32)


def run_host(ix, **kw):
    return lambda q, slots: ix.search_batch(q, search_list_size=L, rescore=RESCORE, k=K, vis_slots=slots, **kw)


# ---- 1. classes and list ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed,base", SHAPES, ids=SHAPE_IDS)
def test_classes_list_and_stats_equal_the_restatement(gpu_ctx, oracle, n, seed, base):
    w = VO.world(n, seed, base)
    VO.check_input_conditions(w)
    VO.check_soundness(w)
    with opened(gpu_ctx, oracle, w) as (ti, ix, heap):
        st = ix.vis_base_eval(heap, w.horizon, w.clog.xact())
        assert st == w.base_stats, (st, w.base_stats)
        hz, dep = ix.vis_base_info()
        assert hz == w.horizon and dep.dtype == np.uint32 and (dep == w.dep).all()
        cls, _ = VO.device_classes(ix, gpu_ctx, w, heap)
        assert (cls == w.cls).all(), np.flatnonzero(cls != w.cls)[:10]
        # evaluating again replaces the base in place
        assert ix.vis_base_eval(heap, w.horizon, w.clog.xact()) == w.base_stats


# ---- 2. materialized masks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed,base", SHAPES, ids=SHAPE_IDS)
def test_materialized_masks_equal_the_reference_for_every_snapshot(gpu_ctx, oracle, n, seed, base):
    w = VO.world(n, seed, base)
    with opened(gpu_ctx, oracle, w) as (ti, ix, heap):
        ix.vis_base_eval(heap, w.horizon, w.clog.xact())
        for j, s in enumerate(w.family):
            slot, sid = (1, 1023, 7)[j % 3], 1 + j % 15
            rmask, _, rund, _ = w.refs[j]
            want_st, want_und = w.ref_on_list(j)
            st, und, nu = ix.vis_slot_eval(heap, slot, s, w.clog.xact())
            assert st == want_st, (j, st, want_st)
            assert nu == len(want_und) and (und == want_und).all() and (want_und == rund).all()  # (every undecided node is of class 2)
            ix.vis_materialize(slot, sid)
            assert (VO.read_mask(ix, gpu_ctx, sid, n) == rmask).all(), j
            _, und3, nu3 = ix.vis_slot_eval(heap, slot, s, w.clog.xact(), cap=3)  # cap bounds what is handed back, not what is counted
            assert nu3 == len(rund) and (und3 == rund[:3]).all()
            # the shim settles the undecided few: every other one turns out invisible; the last entry of a node wins
            settled = (np.arange(len(rund)) % 2).astype(np.uint8)
            ix.vis_slot_patch(slot, np.append(rund, rund[:1]), np.append(settled, 9))
            want = rmask.copy()
            want[rund] = settled
            if len(rund):
                want[rund[0]] = 1
            ix.vis_materialize(slot, sid)
            assert (VO.read_mask(ix, gpu_ctx, sid, n) == want).all(), j
        assert len(w.refs[0][2]) > 5


# ---- 3. a mixed launch on the fast SBQ kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed,base", SHAPES[:1] + SHAPES[2:], ids=SHAPE_IDS[:1] + SHAPE_IDS[2:])
def test_mixed_launch_equals_the_oracle_and_the_legacy_path_scan_for_scan(gpu_ctx, oracle, n, seed, base):
    w = VO.world(n, seed, base)
    with opened(gpu_ctx, oracle, w) as (ti, ix, heap):
        ix.vis_base_eval(heap, w.horizon, w.clog.xact())
        VO.eval_overlays(ix, heap, w)
        q = ti.queries(NQ, seed=5, kind="gauss")
        VO.check_mixed_launch(ix, ti.oracle, q, deal(NQ), w.mask, run_host(ix), w.tids, min_affected=NQ // 4)
        info = ix.last_search_info()
        assert info["kernel"] == FAST_SBQ


# ---- 4. the same over the other kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["general_kernel", "one_wg_per_scan", "tableless_ring", "second_attempt_off"])
def test_mixed_launch_in_other_regimes(gpu_ctx, oracle, regime):
    env = {"general_kernel": {"VS_FAST": "0"}, "one_wg_per_scan": {"VS_F_PERSIST": "0"},
           "tableless_ring": {"VS_F_LDS_MAX_INS": "0", "VS_F_VR": "0"},
           "second_attempt_off": {"VS_F_LDS_MAX_INS": "0", "VS_F_GCAP": "1024", "VS_F_RETRY": "0"}}[regime]
    w = VO.world()
    with opened(gpu_ctx, oracle, w) as (ti, ix, heap):
        ix.vis_base_eval(heap, w.horizon, w.clog.xact())
        VO.eval_overlays(ix, heap, w)
        q = ti.queries(NQ, seed=5, kind="gauss")
        with environ(**env):
            VO.check_mixed_launch(ix, ti.oracle, q, deal(NQ), w.mask, run_host(ix), w.tids)
            assert ix.last_search_info()["kernel"] == (GENERAL if regime == "general_kernel" else FAST_SBQ)


def test_mixed_launch_in_host_chunks(gpu_ctx, oracle):
    """a host batch cut into uneven chunks: every chunk reads its own stretch of the slots"""
    w = VO.world()
    with opened(gpu_ctx, oracle, w) as (ti, ix, heap):
        ix.vis_base_eval(heap, w.horizon, w.clog.xact())
        VO.eval_overlays(ix, heap, w)
        q = ti.queries(NQ, seed=5, kind="gauss")
        with environ(VS_HOST_CHUNK_MIN="20"):
            VO.check_mixed_launch(ix, ti.oracle, q, deal(NQ), w.mask, run_host(ix), w.tids, legacy=False)


def test_mixed_launch_with_label_keys(gpu_ctx, oracle):
    from helpers import TestIndex
    from oracle import oracle_py as O
    w = VO.world()
    ti = TestIndex(n=w.n, n_labels=6, **VO.INDEX_KW)
    ti.tids = w.tids
    ti.oracle = O.OracleIndex(codes=ti.codes, nbrs=ti.nbrs, heap_tids=ti.tids, vecs=ti.vecs, mean=ti.mean, m2=ti.m2, count=ti.count,
                              bits=ti.bits, dim_index=ti.dim_index, num_neighbors=ti.R, distance_type=ti.distance, default_start=ti.start,
                              label_off=ti.label_off, label_val=ti.label_val, label_starts=ti.label_starts)
    ix = ti.upload(gpu_ctx)
    heap = VO.resident(gpu_ctx, w.rel)
    try:
        ix.vis_base_eval(heap, w.horizon, w.clog.xact())
        VO.eval_overlays(ix, heap, w)
        q = ti.queries(NQ, seed=5, kind="gauss")
        rng = np.random.default_rng(6)
        keys = [sorted(set(int(v) for v in rng.integers(1, 7, int(rng.integers(1, 3))))) for _ in range(NQ)]
        VO.check_mixed_launch(ix, ti.oracle, q, deal(NQ), w.mask, run_host(ix, qlabels=keys), w.tids, qlabels=keys)
    finally:
        ti.oracle.set_visibility(None)
        heap.close()
        ix.close()


PLAIN_COUNTERS = ("visited_nodes", "candidate_nodes", "full_distance_comparisons", "node_reads")  # what the plain kernels share with the oracle


@pytest.mark.parametrize("plain_fast", ["1", "0"], ids=["k_search_plain", "general_kernel"])
def test_mixed_launch_on_a_plain_index_whose_window_runs(gpu_ctx, oracle, plain_fast):
    from oracle import oracle_py as O
    from test_gpu_zy_plain import PlainIndex
    w = VO.world()
    pi = PlainIndex(n=w.n, dim=96, R=24, distance=O.L2, seed=120, kind="gauss", dim_index=64)  # dim_index < dim: the window runs
    pi.tids = w.tids
    words = (pi.dim_index + 63) // 64
    pi.oracle = O.OracleIndex(codes=np.zeros((pi.n, words), np.uint64), nbrs=pi.nbrs, heap_tids=pi.tids, vecs=pi.vecs,
                              mean=np.zeros(pi.dim_index, np.float32), m2=np.zeros(pi.dim_index, np.float32), count=0, bits=1,
                              dim_index=pi.dim_index, num_neighbors=pi.R, distance_type=pi.distance, default_start=pi.start, storage_plain=True)
    ix = pi.upload(gpu_ctx)
    heap = VO.resident(gpu_ctx, w.rel)
    try:
        ix.vis_base_eval(heap, w.horizon, w.clog.xact())
        VO.eval_overlays(ix, heap, w)
        q = make_vectors(NQ, 96, 3, "gauss")
        with environ(VS_PLAIN_FAST=plain_fast):
            VO.check_mixed_launch(ix, pi.oracle, q, deal(NQ), w.mask, run_host(ix), w.tids, counters=PLAIN_COUNTERS)
            assert ix.last_search_info()["kernel"] == (FAST_PLAIN if plain_fast == "1" else GENERAL)
    finally:
        pi.oracle.set_visibility(None)
        heap.close()
        ix.close()


def test_device_slots_and_finish(gpu_ctx, oracle):
    w = VO.world()
    with opened(gpu_ctx, oracle, w) as (ti, ix, heap):
        ix.vis_base_eval(heap, w.horizon, w.clog.xact())
        VO.eval_overlays(ix, heap, w)
        q = ti.queries(NQ, seed=5, kind="gauss")
        bufs = [gpu_ctx.alloc(q.nbytes), gpu_ctx.alloc(NQ * 4), gpu_ctx.alloc(NQ * K * 4), gpu_ctx.alloc(NQ * K * 8), gpu_ctx.alloc(NQ * K * 4)]
        dq, ds, d_ids, d_tids, d_dist = bufs

        def run(q, slots):
            gpu_ctx.upload(dq, q)
            gpu_ctx.upload(ds, np.ascontiguousarray(slots, np.uint32))
            ix.search_batch_dev(dq, NQ, L, RESCORE, K, d_ids, d_tids, d_dist, d_vis_slots=ds)
            st = ix.search_batch_dev_finish()
            return (gpu_ctx.download(d_ids, np.empty((NQ, K), np.uint32)), gpu_ctx.download(d_tids, np.empty((NQ, K), np.uint64)),
                    gpu_ctx.download(d_dist, np.empty((NQ, K), np.float32)), st)
        try:
            VO.check_mixed_launch(ix, ti.oracle, q, deal(NQ), w.mask, run, w.tids)
            # a device slot without an overlay is refused before anything is launched: no batch is in flight afterwards
            import pgvectorscale_amd as P
            gpu_ctx.upload(ds, np.full(NQ, 9, np.uint32))
            with pytest.raises(P.VsError, match="slot 9") as e:
                ix.search_batch_dev(dq, NQ, L, RESCORE, K, d_ids, d_tids, d_dist, d_vis_slots=ds)
            assert e.value.code == STATE
            with pytest.raises(P.VsError, match="no batch in flight"):
                ix.search_batch_dev_finish()
        finally:
            for b in bufs:
                gpu_ctx.free(b)


def test_rescore_0_ignores_the_slots(gpu_ctx, oracle):
    w = VO.world()
    with opened(gpu_ctx, oracle, w) as (ti, ix, heap):
        ix.vis_base_eval(heap, w.horizon, w.clog.xact())
        VO.eval_overlays(ix, heap, w)
        q = ti.queries(NQ, seed=5, kind="gauss")
        oi, od, ost = ti.oracle.search_batch(q, L=L, rescore=0, k=K)  # (no mask)
        gi, _, gd, gst = ix.search_batch(q, search_list_size=L, rescore=0, k=K, vis_slots=deal(NQ))
        assert (gi == oi).all() and (gd.view(np.uint32) == od.view(np.uint32)).all()
        hidden = w.refs[0][0] == 0
        assert hidden[gi[gi != VO.INV]].any()  # (rows the snapshots cannot see are among them: nothing was filtered)
        for c in ("visited_nodes", "quantized_distance_comparisons", "next_calls"):
            assert gst[c] == ost[c], c


# ---- 5. refresh -------------------------------------------------------------------------------------------------------------------------
def test_refresh_for_changed_blocks(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    w = VO.World(1500, 31, 0)  # (its own copy: the pages are patched; 1 500 rows lie on nine heap blocks)
    with opened(gpu_ctx, oracle, w) as (ti, ix, heap):
        x = w.clog.xact()
        ix.vis_base_eval(heap, w.horizon, x)
        VO.eval_overlays(ix, heap, w)
        # a later horizon, and "deletes" and "updates" on a handful of blocks since: by an old committed xid (class 1 -> 0), by a
        # transaction still running for some of the family (-> 2); one block is listed although nothing on it changed
        horizon2 = (w.horizon + 30) & V.M32
        blocks = sorted(set(int(t) >> 16 for t in w.tids if int(t) & 0xFFFF))
        assert len(blocks) >= 8
        changed = [blocks[0], blocks[3], blocks[5], blocks[-1]]
        old = int(w.snap["xip"][0])
        committed_old = next(xid for xid in range(w.horizon - 150, w.horizon) if w.clog.get(xid) == V.COMMITTED)
        touched = 0
        for i, t in enumerate(w.tids):
            t = int(t)
            if (t >> 16) in (changed[0], changed[1], changed[3]) and (t & 0xFFFF) and w.cls[i] == 1 and w.refs[0][3][i] == "visible":
                V.patch_header(w.rel, _root_tid(w, t), xmax=committed_old if touched % 2 else old, m=XMAX_COMMITTED if touched % 2 else 0)
                touched += 1
        assert touched > 10
        for b in changed:
            heap.put(bytes(w.rel.pages[b]), first_block=b)
        want_cls, want_dep, want_st = VO.ref_base(*w.pages(), w.tids, horizon2, w.clog, changed=set(changed), prev=w.cls)
        full_cls, _, _ = VO.ref_base(*w.pages(), w.tids, horizon2, w.clog)
        on_changed = np.isin(w.tids >> np.uint64(16), changed)
        assert (want_cls[on_changed] == full_cls[on_changed]).all() and (want_cls[~on_changed] == w.cls[~on_changed]).all()
        assert (want_cls != w.cls).sum() > 10 and 0 < want_st["n_walked"] < w.n
        st = ix.vis_base_eval(heap, horizon2, x, changed_blocks=changed)
        assert st == want_st, (st, want_st)
        hz, dep = ix.vis_base_info()
        assert hz == horizon2 and (dep == want_dep).all()
        # every overlay is gone
        q = ti.queries(NQ, seed=5, kind="gauss")
        with pytest.raises(P.VsError, match="no overlay") as e:
            ix.search_batch(q, search_list_size=L, rescore=RESCORE, k=K, vis_slots=deal(NQ))
        assert e.value.code == STATE
        cls, _ = VO.device_classes(ix, gpu_ctx, w, heap)
        assert (cls == want_cls).all(), np.flatnonzero(cls != want_cls)[:10]
        # a snapshot taken before the new horizon is no longer admissible; the others are evaluated again and the mixed launch holds
        with pytest.raises(P.VsError, match="precedes the base's horizon") as e:
            ix.vis_slot_eval(heap, 1, w.family[0], x)
        assert e.value.code == INVALID
        fam = [dict(s, xmin=s["xmin"] if V.follows_eq(s["xmin"], horizon2) else horizon2) for s in w.family]
        masks = {slot: V.ref_visibility(*w.pages(), w.tids, fam[j], w.clog)[0] for slot, j in SLOT_SNAP.items()}
        for slot, j in SLOT_SNAP.items():
            ix.vis_slot_eval(heap, slot, fam[j], x)
            ix.vis_materialize(slot, 2)
            assert (VO.read_mask(ix, gpu_ctx, 2, w.n) == masks[slot]).all(), slot
        VO.check_mixed_launch(ix, ti.oracle, q, deal(NQ), lambda slot: masks.get(slot), run_host(ix), w.tids, min_affected=NQ // 4)
        # an empty list of changed blocks walks nothing, keeps every class and still drops the overlays
        st = ix.vis_base_eval(heap, horizon2, x, changed_blocks=[])
        assert st["n_walked"] == 0 and st["n_class"] == want_st["n_class"] and (ix.vis_base_info()[1] == want_dep).all()
        # ... and so does a listed block beyond the resident fork (no row of the fork lies there), however far beyond
        st = ix.vis_base_eval(heap, horizon2, x, changed_blocks=[len(w.rel.pages), 0xFFFFFFF0])
        assert st["n_walked"] == 0 and st["n_class"] == want_st["n_class"] and (ix.vis_base_info()[1] == want_dep).all()
        st = ix.vis_base_eval(heap, horizon2, x, changed_blocks=[changed[0], 0xFFFFFFF0])
        assert st["n_walked"] == int((w.tids >> np.uint64(16) == changed[0]).sum()) and st["n_class"] == want_st["n_class"]


def _root_tid(w, tid):
    """the tid of the tuple behind an index tid (the corpus hangs a few rows behind a redirect)"""
    import struct
    blk, off = tid >> 16, tid & 0xFFFF
    lp = struct.unpack_from("<I", w.rel.pages[blk], 24 + 4 * (off - 1))[0]
    return V.tid_of(blk, lp & 0x7FFF) if (lp >> 15) & 3 == 2 else tid


# ---- 6. lifetime and refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    w = VO.world()
    with opened(gpu_ctx, oracle, w) as (ti, ix, heap):
        x = w.clog.xact()
        q = ti.queries(8, seed=6, kind="gauss")

        def refused(code, match, call):
            with pytest.raises(P.VsError, match=match) as e:
                call()
            assert e.value.code == code, (e.value.code, str(e.value))
        # no base
        refused(STATE, "no visibility base", lambda: ix.vis_slot_eval(heap, 1, w.family[0], x))
        refused(STATE, "no visibility base", lambda: ix.vis_slot_patch(1, [0], [0]))
        refused(STATE, "no visibility base", lambda: ix.vis_materialize(1, 1))
        refused(STATE, "no visibility base", lambda: ix.vis_base_eval(heap, w.horizon, x, changed_blocks=[0]))
        refused(STATE, "no visibility base", lambda: ix.vis_base_info())
        refused(STATE, "no overlay", lambda: ix.search_batch(q, search_list_size=L, rescore=RESCORE, k=K, vis_slots=np.full(8, 1)))
        ix.vis_base_eval(heap, w.horizon, x)
        ix.vis_slot_eval(heap, 1, w.family[0], x)

        def unchanged():
            hz, dep = ix.vis_base_info()
            assert hz == w.horizon and (dep == w.dep).all()
            ix.vis_materialize(1, 3)
            assert (VO.read_mask(ix, gpu_ctx, 3, w.n) == w.refs[0][0]).all()
        # slot 0 and slots beyond the table
        for slot in (0, 1024, 0xFFFFFFFF):
            refused(INVALID, "slot", lambda: ix.vis_slot_eval(heap, slot, w.family[0], x))
            refused(INVALID, "slot", lambda: ix.vis_slot_patch(slot, [int(w.dep[0])], [0]))
            refused(INVALID, "slot", lambda: ix.vis_slot_drop(slot))
            refused(INVALID, "slot", lambda: ix.vis_materialize(slot, 1))
        refused(INVALID, "slot 1024", lambda: ix.search_batch(q, search_list_size=L, rescore=RESCORE, k=K, vis_slots=np.full(8, 1024)))
        refused(STATE, "slot 2, which has no overlay", lambda: ix.search_batch(q, search_list_size=L, rescore=RESCORE, k=K, vis_slots=[1, 1, 2, 1, 1, 1, 1, 1]))
        for sid in (0, 16):
            refused(INVALID, "snapshot id", lambda: ix.vis_materialize(1, sid))
        refused(STATE, "no overlay", lambda: ix.vis_materialize(2, 1))
        refused(STATE, "no overlay", lambda: ix.vis_slot_patch(2, [int(w.dep[0])], [0]))
        # a snapshot that can see behind the horizon
        before = (w.horizon - 1) & V.M32
        refused(INVALID, f"xmin {before} precedes", lambda: ix.vis_slot_eval(heap, 1, dict(w.family[0], xmin=before), x))
        refused(INVALID, f"own xid {before} precedes", lambda: ix.vis_slot_eval(heap, 1, dict(w.family[0], own_xids=[w.horizon + 5, before]), x))
        refused(INVALID, "own xid 2 precedes", lambda: ix.vis_slot_eval(heap, 1, dict(w.family[0], own_xids=[2]), x))
        # a node that is not on the depends list
        off_list = int(np.flatnonzero(w.cls != 2)[0])
        refused(INVALID, f"node {off_list} is not on the depends list", lambda: ix.vis_slot_patch(1, [int(w.dep[0]), off_list], [0, 0]))
        refused(INVALID, "not on the depends list", lambda: ix.vis_slot_patch(1, [w.n], [0]))
        # the argument checks
        refused(INVALID, "multiple of 4", lambda: ix.vis_base_eval(heap, w.horizon, (x[0] + 1, x[1], x[2])))
        refused(INVALID, "multiple of 4", lambda: ix.vis_slot_eval(heap, 1, w.family[0], (x[0] + 1, x[1], x[2])))
        refused(INVALID, "ascending", lambda: ix.vis_base_eval(heap, w.horizon, x, changed_blocks=[3, 3]))
        refused(INVALID, "ascending", lambda: ix.vis_base_eval(heap, w.horizon, x, changed_blocks=[4, 1]))
        refused(INVALID, "no normal xid", lambda: ix.vis_base_eval(heap, 2, x))
        unchanged()
        # a view handle
        from pgvectorscale_amd import _lib
        import ctypes as C
        vh = C.c_void_p()
        _lib.check(ix._L.vs_index_view(ix.h, gpu_ctx.h, C.byref(vh)))
        try:
            assert ix._L.vs_index_vis_base_eval(vh, heap.h, w.horizon, None, None, 0, None) == STATE
            assert ix._L.vs_index_vis_slot_drop(vh, 1) == STATE and ix._L.vs_index_vis_materialize(vh, 1, 1) == STATE
            assert ix._L.vs_index_vis_base_drop(vh) == STATE
        finally:
            ix._L.vs_index_free(vh)
        # while a batch of the handle is in flight
        dq, d_ids = gpu_ctx.alloc(q.nbytes), gpu_ctx.alloc(len(q) * K * 4)
        gpu_ctx.upload(dq, q)
        ix.search_batch_dev(dq, len(q), L, RESCORE, K, d_ids)
        try:
            for call in (lambda: ix.vis_base_eval(heap, w.horizon, x), lambda: ix.vis_slot_eval(heap, 1, w.family[1], x),
                         lambda: ix.vis_slot_patch(1, [int(w.dep[0])], [0]), lambda: ix.vis_slot_drop(1), lambda: ix.vis_materialize(1, 1),
                         lambda: ix.vis_base_drop()):
                refused(STATE, "in flight", call)
        finally:
            ix.search_batch_dev_finish()
            gpu_ctx.free(dq)
            gpu_ctx.free(d_ids)
        unchanged()
        # dropping: an overlay, then the base
        ix.vis_slot_drop(1)
        ix.vis_slot_drop(1)  # (nothing to drop is no error)
        refused(STATE, "no overlay", lambda: ix.vis_materialize(1, 1))
        ix.vis_base_drop()
        refused(STATE, "no visibility base", lambda: ix.vis_base_info())


def test_a_malformed_page_drops_the_base(gpu_ctx, oracle):
    import struct
    import pgvectorscale_amd as P
    w = VO.World(600, 23, 0)  # (its own copy: a page is damaged)
    with opened(gpu_ctx, oracle, w) as (ti, ix, heap):
        x = w.clog.xact()
        ix.vis_base_eval(heap, w.horizon, x)
        ix.vis_slot_eval(heap, 1, w.family[0], x)
        blk = int(w.tids[np.flatnonzero(w.tids & np.uint64(0xFFFF))[0]]) >> 16
        struct.pack_into("<H", w.rel.pages[blk], 12, w.rel.page_size + 8)  # pd_lower beyond the page
        heap.put(bytes(w.rel.pages[blk]), first_block=blk)
        with pytest.raises(P.VsError, match=f"heap block {blk} item .*page header") as e:
            ix.vis_base_eval(heap, w.horizon, x, changed_blocks=[blk])
        assert e.value.code == INVALID
        with pytest.raises(P.VsError, match="no visibility base") as e:
            ix.vis_base_info()
        assert e.value.code == STATE
        with pytest.raises(P.VsError, match="no overlay") as e:
            ix.search_batch(ti.queries(4, seed=1, kind="gauss"), search_list_size=L, rescore=RESCORE, k=K, vis_slots=[1, 1, 1, 1])
        assert e.value.code == STATE


def test_rows_inserted_after_an_evaluation_are_hidden_until_the_next(gpu_ctx, oracle):
    w = VO.world()
    with opened(gpu_ctx, oracle, w) as (ti, ix, heap):
        n, x = w.n, w.clog.xact()
        ix.vis_base_eval(heap, w.horizon, x)
        ix.vis_slot_eval(heap, 1, w.family[0], x)
        q = ti.queries(16, seed=5, kind="gauss")
        before = ix.search_batch(q, search_list_size=L, rescore=RESCORE, k=K, vis_slots=np.ones(16, np.uint32))
        # the new rows are the queries themselves, on tids of a visible row's kind: each would be the first row of its scan
        vis_tid = w.tids[np.flatnonzero(w.cls == 1)[:4]]
        ix.insert(q[:4].copy(), vis_tid, search_list_size=L)
        ix._refresh()
        assert ix.desc.n == n + 4
        after = ix.search_batch(q, search_list_size=L, rescore=RESCORE, k=K, vis_slots=np.ones(16, np.uint32))
        assert not (after[0] >= n)[after[0] != VO.INV].any()  # hidden from slot scans ...
        free = ix.search_batch(q, search_list_size=L, rescore=RESCORE, k=K, vis_slots=np.zeros(16, np.uint32))
        assert (free[0][:4, 0] >= n).all()  # ... though slot 0 sees them
        ix.vis_materialize(1, 1)
        got = VO.read_mask(ix, gpu_ctx, 1, n + 4)
        assert (got[:n] == w.refs[0][0]).all() and not got[n:].any()
        # the next evaluation judges them like every other row
        st = ix.vis_base_eval(heap, w.horizon, x)
        assert st["n_class"][1] == w.base_stats["n_class"][1] + 4 and st["n_walked"] == n + 4
        ix.vis_slot_eval(heap, 1, w.family[0], x)
        again = ix.search_batch(q, search_list_size=L, rescore=RESCORE, k=K, vis_slots=np.ones(16, np.uint32))
        assert (again[0][:4, 0] >= n).all()
        assert before[0].shape == after[0].shape


def test_compact_drops_base_and_overlays(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    w = VO.world()
    with opened(gpu_ctx, oracle, w) as (ti, ix, heap):
        x = w.clog.xact()
        ix.vis_base_eval(heap, w.horizon, x)
        ix.vis_slot_eval(heap, 1, w.family[0], x)
        ix.compact()
        with pytest.raises(P.VsError, match="no visibility base") as e:
            ix.vis_base_info()
        assert e.value.code == STATE
        with pytest.raises(P.VsError, match="no overlay") as e:
            ix.search_batch(ti.queries(4, seed=1, kind="gauss"), search_list_size=L, rescore=RESCORE, k=K, vis_slots=[1, 1, 1, 1])
        assert e.value.code == STATE


# ---- 8. the legacy path is what it was --------------------------------------------------------------------------------------------------
def test_a_batch_without_slots_launches_what_it_launched(gpu_ctx, oracle):
    w = VO.world()
    with opened(gpu_ctx, oracle, w) as (ti, ix, heap):
        x = w.clog.xact()
        q = ti.queries(NQ, seed=5, kind="gauss")
        # (the launch of a batch is sized by what the handle's earlier batches needed: a twin handle that never sees a base runs the
        # same sequence of batches, and the two are compared batch for batch)
        twin = ti.upload(gpu_ctx)
        try:
            plain = ix.search_batch(q, search_list_size=L, rescore=RESCORE, k=K)
            twin.search_batch(q, search_list_size=L, rescore=RESCORE, k=K)
            assert ix.last_search_info() == twin.last_search_info()
            ix.vis_base_eval(heap, w.horizon, x)
            VO.eval_overlays(ix, heap, w)
            # a base and overlays on the index change nothing for a batch that names none ...
            again = ix.search_batch(q, search_list_size=L, rescore=RESCORE, k=K)
            twin.search_batch(q, search_list_size=L, rescore=RESCORE, k=K)
            assert ix.last_search_info() == twin.last_search_info()
            # ... nor for one whose slots are all 0
            zeros = ix.search_batch(q, search_list_size=L, rescore=RESCORE, k=K, vis_slots=np.zeros(NQ, np.uint32))
            twin.search_batch(q, search_list_size=L, rescore=RESCORE, k=K)
            assert ix.last_search_info() == twin.last_search_info()
        finally:
            twin.close()
        for got in (again, zeros):
            assert (got[0] == plain[0]).all() and (got[1] == plain[1]).all() and (got[2].view(np.uint32) == plain[2].view(np.uint32)).all()
            for c in COUNTERS:
                assert got[3][c] == plain[3][c], c
        oi, od, ost = ti.oracle.search_batch(q, L=L, rescore=RESCORE, k=K)
        assert (plain[0] == oi).all()
        # under a legacy mask the rows are the oracle's, slots or no slots on the index; a slot batch does not consult that mask
        rmask = w.refs[0][0]
        ix._L.vs_index_snapshot_put(ix.h, 2, rmask.ctypes.data)
        ti.oracle.set_visibility(rmask)
        oi, od, ost = ti.oracle.search_batch(q, L=L, rescore=RESCORE, k=K)
        li, _, ld, lst = VO.search_under(ix, 2, q)
        assert (li == oi).all() and (ld.view(np.uint32) == od.view(np.uint32)).all()
        for c in COUNTERS:
            assert lst[c] == ost[c], c
        from pgvectorscale_amd import _lib
        _lib.check(ix._L.vs_index_snapshot_use(ix.h, 2, None))
        try:
            zeros2 = ix.search_batch(q, search_list_size=L, rescore=RESCORE, k=K, vis_slots=np.zeros(NQ, np.uint32))
        finally:
            _lib.check(ix._L.vs_index_snapshot_use(ix.h, 0, None))
        assert (zeros2[0] == plain[0]).all()


# ---- 7. the broker: scans that name slots share their launch ----------------------------------------------------------------------------
def test_broker_scans_of_different_slots_share_a_launch(gpu_ctx, oracle):
    import threading
    import pgvectorscale_amd as P
    w = VO.world()
    ti = w.index()
    ix = ti.upload(gpu_ctx)
    heap = VO.resident(gpu_ctx, w.rel)
    n_clients = 32
    q = ti.queries(n_clients, seed=5, kind="gauss")
    slots = [tuple(SLOT_SNAP)[i % len(SLOT_SNAP)] for i in range(n_clients)]  # six slots between the clients
    want = {}
    try:
        for slot in set(slots):
            sel = [i for i in range(n_clients) if slots[i] == slot]
            ti.oracle.set_visibility(w.mask(slot))
            oi, od, _ = ti.oracle.search_batch(q[sel], L=L, rescore=RESCORE, k=K)
            for j, i in enumerate(sel):
                want[i] = (oi[j], od[j])
    finally:
        ti.oracle.set_visibility(None)
    br = P.Broker(ix, max_batch=n_clients, max_wait_us=5_000_000)  # (the launch goes when the 32nd scan has arrived, not when the time is up)
    try:
        # the base and the overlays reach the index through the dispatcher
        br.call(lambda: ix.vis_base_eval(heap, w.horizon, w.clog.xact()))
        br.call(lambda: VO.eval_overlays(ix, heap, w))
        got, errs = {}, []

        def client(i):
            try:
                got[i] = br.search(q[i], search_list_size=L, rescore=RESCORE, k=K, vis_slot=slots[i])
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        before = br.stats()
        th = [threading.Thread(target=client, args=(i,)) for i in range(n_clients)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        st = br.stats()
        assert st["scans"] - before["scans"] == n_clients
        assert st["batches"] - before["batches"] == 1 < len(set(slots))  # one setting of the GUCs: one launch for six snapshots
        for i in range(n_clients):
            gi, gt, gd = got[i]
            assert (gi == want[i][0]).all() and (gd.view(np.uint32) == want[i][1].view(np.uint32)).all(), i
            live = gi != VO.INV
            assert (gt[live] == w.tids[gi[live]]).all()
        # a slot without an overlay, and a slot beyond the table (a broker that does not hold a lone scan back for others)
        br.close()
        br = P.Broker(ix, max_wait_us=0)
        with pytest.raises(P.VsError, match="no overlay") as e:
            br.search(q[0], search_list_size=L, rescore=RESCORE, k=K, vis_slot=9)
        assert e.value.code == STATE
        with pytest.raises(P.VsError) as e:
            br.search(q[0], search_list_size=L, rescore=RESCORE, k=K, vis_slot=1024)
        assert e.value.code == INVALID
    finally:
        br.close()
        heap.close()
        ix.close()
