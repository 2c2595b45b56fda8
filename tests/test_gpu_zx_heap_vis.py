"""Heap visibility decided on the device from resident heap pages: vs_heap_res_*, k_heap_vis (vs_heap_res_visibility) and
vs_index_snapshot_eval / _put_dev / _patch.  Pages are manufactured with oracle/heap_py.py (tests/heap_vis_checks.py); expectations
are hand-written known answers and a scalar Python restatement of the rule of include/vsgpu.h, never the device's own output; every
comparison is exact.  Also runs on the lockstep interpreter (tests/test_emu_heap_vis.py), where the malformed pages of this file
meet guard pages behind every device allocation."""
import ctypes as C
import struct

import numpy as np
import pytest

import heap_vis_checks as V
from heap_vis_checks import (COMBOCID, EXCL_LOCK, FROZEN, HOT_UPDATED, INVALID, IS_MULTI, KEYSHR_LOCK, LOCK_ONLY, MOVED_IN, MOVED_OFF,
                             ONLY_TUPLE, STATE, XMAX_COMMITTED, XMAX_INVALID, XMIN_COMMITTED, XMIN_INVALID, tup)
from helpers import TestIndex, make_vectors
from oracle import heap_py as HP

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

VIS, INV = "visible", "invisible"
MI = XMAX_INVALID

# ---- 1. known answers -------------------------------------------------------------------------------------------------------------------
# The snapshot of the table: xmin 100, xmax 200, xip {150, 120} (unsorted), subxip {160}, the backend's own xids {170, 171}, curcid 5.
# pg_xact window [40, 300): committed 50 60 99 100 110 120 130 180 200 210, aborted 55 115, in progress 150 160 170 171, sub-committed
# 135; 30 and 400 lie outside.
SNAP = dict(xmin=100, xmax=200, xip=[150, 120], subxip=[160], own_xids=[171, 170], curcid=5)
SNAP_SUBOVER = dict(SNAP, suboverflowed=True)
SNAP_RECOVERY = dict(SNAP, taken_during_recovery=True)
SNAP_RECOVERY_SUBOVER = dict(SNAP, taken_during_recovery=True, suboverflowed=True)
# a snapshot that straddles the 2^32 wrap: xip {0xFFFFFF80, 0x10}; window [0xFFFFFE00, +0x400): everything committed
SNAP_WRAP = dict(xmin=0xFFFFFF00, xmax=0x00000040, xip=[0xFFFFFF80, 0x10], curcid=5)


def _clog():
    c = V.Clog(40, 260)
    for x in (50, 60, 99, 100, 110, 120, 130, 180, 200, 210):
        c.set(x, V.COMMITTED)
    for x in (55, 115):
        c.set(x, V.ABORTED)
    c.set(135, V.SUB_COMMITTED)
    return c


def _clog_wrap():
    return V.Clog(0xFFFFFE00, 0x400, default=V.COMMITTED)


# (what the row shows, snapshot, header, expected byte, expected verdict: VIS / INV / the undecided reason) — written out, not computed
KAT = [
    # xmin not hinted committed
    ("XMIN_INVALID hint", "n", dict(xmin=50, m=XMIN_INVALID | MI), 0, INV),
    ("MOVED_OFF", "n", dict(xmin=50, m=MOVED_OFF | MI), 1, "moved"),
    ("MOVED_IN", "n", dict(xmin=50, m=MOVED_IN | MI), 1, "moved"),
    ("own xmin, combo cid", "n", dict(xmin=170, cid=1, m=COMBOCID | MI), 1, "combocid"),
    ("own xmin, cid == curcid", "n", dict(xmin=170, cid=5, m=MI), 0, INV),
    ("own xmin, cid > curcid", "n", dict(xmin=171, cid=7, m=MI), 0, INV),
    ("own xmin, cid < curcid, no xmax", "n", dict(xmin=170, cid=4, m=MI), 1, VIS),
    ("own xmin, xmax LOCK_ONLY", "n", dict(xmin=170, xmax=171, cid=4, m=LOCK_ONLY), 1, VIS),
    ("own xmin, xmax EXCL_LOCK alone", "n", dict(xmin=170, xmax=60, cid=4, m=EXCL_LOCK), 1, VIS),
    ("own xmin, xmax multixact", "n", dict(xmin=170, xmax=9999, cid=4, m=IS_MULTI), 1, "multixact"),
    ("own xmin, xmax multixact with EXCL_LOCK", "n", dict(xmin=170, xmax=9999, cid=4, m=IS_MULTI | EXCL_LOCK), 1, "multixact"),
    ("own xmin, xmax multixact LOCK_ONLY", "n", dict(xmin=170, xmax=9999, cid=4, m=IS_MULTI | LOCK_ONLY), 1, VIS),
    ("own xmin, xmax not own", "n", dict(xmin=170, xmax=60, cid=4), 1, VIS),
    ("own xmin, own xmax, cid < curcid", "n", dict(xmin=170, xmax=171, cid=4), 0, INV),
    ("xmin in xip", "n", dict(xmin=120, m=MI), 0, INV),
    ("xmin in xip (in progress)", "n", dict(xmin=150, m=MI), 0, INV),
    ("xmin in subxip", "n", dict(xmin=160, m=MI), 0, INV),
    ("xmin == snapshot xmax", "n", dict(xmin=200, m=MI), 0, INV),
    ("xmin > snapshot xmax", "n", dict(xmin=210, m=MI), 0, INV),
    ("xmin aborted, before the snapshot", "n", dict(xmin=55, m=MI), 0, INV),
    ("xmin aborted, inside the snapshot's range", "n", dict(xmin=115, m=MI), 0, INV),
    ("xmin 0 (invalid)", "n", dict(xmin=0, m=MI), 0, INV),
    ("xmin 1 (bootstrap)", "n", dict(xmin=1, m=MI), 1, VIS),
    ("xmin 2 (frozen xid)", "n", dict(xmin=2, m=MI), 1, VIS),
    ("xmin committed, before the snapshot", "n", dict(xmin=50, m=MI), 1, VIS),
    ("xmin committed, == snapshot xmin - 1", "n", dict(xmin=99, m=MI), 1, VIS),
    ("xmin committed, == snapshot xmin", "n", dict(xmin=100, m=MI), 1, VIS),
    ("xmin committed, inside the range, not in xip", "n", dict(xmin=110, m=MI), 1, VIS),
    ("xmin sub-committed", "n", dict(xmin=135, m=MI), 1, "subcommitted"),
    ("xmin outside the pg_xact window", "n", dict(xmin=30, m=MI), 1, "clog_range"),
    # xmin hinted committed / frozen
    ("XMIN_COMMITTED but in xip", "n", dict(xmin=120, m=XMIN_COMMITTED | MI), 0, INV),
    ("XMIN_COMMITTED, old", "n", dict(xmin=50, m=XMIN_COMMITTED | MI), 1, VIS),
    ("XMIN_COMMITTED, outside the window: the hint decides", "n", dict(xmin=30, m=XMIN_COMMITTED | MI), 1, VIS),
    ("frozen, raw xmin in xip", "n", dict(xmin=120, m=FROZEN | MI), 1, VIS),
    ("frozen, raw xmin > snapshot xmax", "n", dict(xmin=210, m=FROZEN | MI), 1, VIS),
    # xmax
    ("xmax LOCK_ONLY", "n", dict(xmin=50, xmax=60, m=XMIN_COMMITTED | LOCK_ONLY), 1, VIS),
    ("xmax EXCL_LOCK alone", "n", dict(xmin=50, xmax=60, m=XMIN_COMMITTED | EXCL_LOCK), 1, VIS),
    ("xmax EXCL_LOCK | KEYSHR_LOCK is no lock-only form", "n", dict(xmin=50, xmax=60, m=XMIN_COMMITTED | EXCL_LOCK | KEYSHR_LOCK), 0, INV),
    ("xmax multixact", "n", dict(xmin=50, xmax=9999, m=XMIN_COMMITTED | IS_MULTI), 1, "multixact"),
    ("xmax multixact LOCK_ONLY", "n", dict(xmin=50, xmax=9999, m=XMIN_COMMITTED | IS_MULTI | LOCK_ONLY), 1, VIS),
    ("own xmax, cid == curcid", "n", dict(xmin=50, xmax=170, cid=5, m=XMIN_COMMITTED), 1, VIS),
    ("own xmax, cid < curcid", "n", dict(xmin=50, xmax=171, cid=4, m=XMIN_COMMITTED), 0, INV),
    ("own xmax, combo cid", "n", dict(xmin=50, xmax=170, cid=4, m=XMIN_COMMITTED | COMBOCID), 1, "combocid"),
    ("xmax in xip", "n", dict(xmin=50, xmax=120, m=XMIN_COMMITTED), 1, VIS),
    ("xmax in subxip", "n", dict(xmin=50, xmax=160, m=XMIN_COMMITTED), 1, VIS),
    ("xmax == snapshot xmax", "n", dict(xmin=50, xmax=200, m=XMIN_COMMITTED), 1, VIS),
    ("xmax > snapshot xmax", "n", dict(xmin=50, xmax=210, m=XMIN_COMMITTED), 1, VIS),
    ("xmax beyond the window but after the snapshot", "n", dict(xmin=50, xmax=400, m=XMIN_COMMITTED), 1, VIS),
    ("xmax aborted", "n", dict(xmin=50, xmax=115, m=XMIN_COMMITTED), 1, VIS),
    ("xmax 0 without XMAX_INVALID", "n", dict(xmin=50, xmax=0, m=XMIN_COMMITTED), 1, VIS),
    ("xmax committed, before the snapshot", "n", dict(xmin=50, xmax=60, m=XMIN_COMMITTED), 0, INV),
    ("xmax committed, == snapshot xmin - 1", "n", dict(xmin=50, xmax=99, m=XMIN_COMMITTED), 0, INV),
    ("xmax committed, == snapshot xmin", "n", dict(xmin=50, xmax=100, m=XMIN_COMMITTED), 0, INV),
    ("xmax committed, inside the range", "n", dict(xmin=50, xmax=110, m=XMIN_COMMITTED), 0, INV),
    ("xmax sub-committed", "n", dict(xmin=50, xmax=135, m=XMIN_COMMITTED), 1, "subcommitted"),
    ("xmax outside the pg_xact window", "n", dict(xmin=50, xmax=30, m=XMIN_COMMITTED), 1, "clog_range"),
    ("XMAX_COMMITTED but in xip", "n", dict(xmin=50, xmax=120, m=XMIN_COMMITTED | XMAX_COMMITTED), 1, VIS),
    ("XMAX_COMMITTED, after the snapshot", "n", dict(xmin=50, xmax=210, m=XMIN_COMMITTED | XMAX_COMMITTED), 1, VIS),
    ("XMAX_COMMITTED, old", "n", dict(xmin=50, xmax=60, m=XMIN_COMMITTED | XMAX_COMMITTED), 0, INV),
    ("XMAX_COMMITTED, outside the window: the hint decides", "n", dict(xmin=50, xmax=30, m=XMIN_COMMITTED | XMAX_COMMITTED), 0, INV),
    # suboverflowed and recovery snapshots
    ("suboverflowed: in xip", "so", dict(xmin=120, m=MI), 0, INV),
    ("suboverflowed: not in xip", "so", dict(xmin=130, m=MI), 1, "suboverflow"),
    ("suboverflowed: xmax not in xip", "so", dict(xmin=50, xmax=130, m=XMIN_COMMITTED), 1, "suboverflow"),
    ("suboverflowed: before the snapshot needs no subtrans", "so", dict(xmin=50, m=MI), 1, VIS),
    ("recovery: in subxip", "r", dict(xmin=160, m=MI), 0, INV),
    ("recovery: xip is not looked at", "r", dict(xmin=120, m=MI), 1, VIS),
    ("recovery: not in subxip", "r", dict(xmin=130, m=MI), 1, VIS),
    ("recovery, suboverflowed: in subxip", "rso", dict(xmin=160, m=MI), 0, INV),
    ("recovery, suboverflowed: not in subxip", "rso", dict(xmin=130, m=MI), 1, "suboverflow"),
    # across the wrap
    ("wrap: well before xmin", "w", dict(xmin=0xFFFFFE80, m=MI), 1, VIS),
    ("wrap: == xmin", "w", dict(xmin=0xFFFFFF00, m=MI), 1, VIS),
    ("wrap: in xip before the wrap", "w", dict(xmin=0xFFFFFF80, m=MI), 0, INV),
    ("wrap: between, before the wrap", "w", dict(xmin=0xFFFFFFF0, m=MI), 1, VIS),
    ("wrap: xid 3, the first after the wrap", "w", dict(xmin=3, m=MI), 1, VIS),
    ("wrap: in xip after the wrap", "w", dict(xmin=0x10, m=MI), 0, INV),
    ("wrap: between, after the wrap", "w", dict(xmin=0x20, m=MI), 1, VIS),
    ("wrap: == xmax", "w", dict(xmin=0x40, m=MI), 0, INV),
    ("wrap: after xmax", "w", dict(xmin=0x50, m=MI), 0, INV),
    ("wrap: xmax after the snapshot's xmax", "w", dict(xmin=0xFFFFFE80, xmax=0x50, m=XMIN_COMMITTED), 1, VIS),
    ("wrap: xmax before the snapshot's xmin", "w", dict(xmin=0xFFFFFE80, xmax=0xFFFFFEF0, m=XMIN_COMMITTED), 0, INV),
    ("wrap: frozen xid under a wrapped snapshot", "w", dict(xmin=2, m=MI), 1, VIS),
]
KAT_SNAPS = {"n": (SNAP, _clog), "so": (SNAP_SUBOVER, _clog), "r": (SNAP_RECOVERY, _clog), "rso": (SNAP_RECOVERY_SUBOVER, _clog),
             "w": (SNAP_WRAP, _clog_wrap)}


def test_known_answers(gpu_ctx):
    rel = HP.HeapRelation()
    tids = np.array([V.tid_of(*rel.add_item(tup(**hdr))) for _, _, hdr, _, _ in KAT], np.uint64)
    heap = V.resident(gpu_ctx, rel)
    try:
        seen = set()
        for key, (snap, mk) in KAT_SNAPS.items():
            rows = [i for i, r in enumerate(KAT) if r[1] == key]
            mask, st, und, nu = V.dev_visibility(gpu_ctx, heap, tids[rows], snap, mk())
            for j, i in enumerate(rows):
                what, _, _, byte, verdict = KAT[i]
                assert mask[j] == byte, what
                assert (j in und) == (verdict not in (VIS, INV)), what
                seen.add(verdict)
            want = {r: sum(1 for i in rows if KAT[i][4] == r) for r in V.REASONS}
            assert st["undecided_by_reason"] == want, (key, st)
            assert st["n_visible"] == sum(1 for i in rows if KAT[i][4] == VIS) and st["n_invisible"] == sum(1 for i in rows if KAT[i][4] == INV)
            assert st["n_undecided"] == nu == len(und) and st["chain_hops"] == 0
            assert st["n_deleted"] == st["n_not_found"] == st["n_dead_line_pointer"] == 0
            # (the restatement agrees with the table: what the randomised run is held to is the same rule)
            rmask, rst, rund, kinds = V.ref_visibility(rel.pages, rel.page_size, len(rel.pages), tids[rows], snap, mk())
            assert kinds == [KAT[i][4] for i in rows] and (rmask == mask).all() and rst == st and (rund == und).all()
        assert seen == {VIS, INV, *V.REASONS}
    finally:
        heap.close()


def test_line_pointer_classes(gpu_ctx):
    """offset 0 is a vacuumed index tuple; LP_UNUSED / LP_DEAD first pointers; an offset beyond the line pointers; a block beyond the fork"""
    rel = HP.HeapRelation()
    t = [V.tid_of(*rel.add_item(tup(50, m=MI))) for _ in range(6)]
    rel.set_line_pointer(0, 2, HP.LP_DEAD)
    rel.set_line_pointer(0, 3, HP.LP_UNUSED)
    tids = np.array([t[0], t[1], t[2], V.tid_of(0, 0), V.tid_of(3, 0), V.tid_of(0, 7), V.tid_of(0, 0xFFFF), V.tid_of(1, 1),
                     V.tid_of(0xFFFFFFFF, 1), t[5]], np.uint64)
    heap = V.resident(gpu_ctx, rel)
    try:
        mask, st, und, nu = V.dev_visibility(gpu_ctx, heap, tids, SNAP, _clog())
    finally:
        heap.close()
    assert mask.tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    assert (st["n_visible"], st["n_invisible"], st["n_undecided"]) == (2, 8, 0) and nu == 0 and und.size == 0
    assert (st["n_dead_line_pointer"], st["n_deleted"], st["n_not_found"]) == (2, 2, 4)


# ---- 2. the randomised differential run -------------------------------------------------------------------------------------------------
_corpora = {}


def corpus(base):
    """n = 2000 in shuffled index order with 5 % deleted tids, and the reference's answers under the four kinds of snapshot: made once"""
    if base not in _corpora:
        rel, tids, snap, clog = V.random_corpus(2000, seed=19, base=base)
        tids = V.index_order(tids, seed=3)
        snaps = {"plain": snap, "suboverflowed": dict(snap, suboverflowed=True), "recovery": dict(snap, taken_during_recovery=True),
                 "recovery_suboverflowed": dict(snap, taken_during_recovery=True, suboverflowed=True)}
        refs = {k: V.ref_visibility(rel.pages, rel.page_size, len(rel.pages), tids, s, clog) for k, s in snaps.items()}
        _corpora[base] = (rel, tids, snaps, clog, refs)
    return _corpora[base]


@pytest.mark.parametrize("kind", ["plain", "suboverflowed", "recovery", "recovery_suboverflowed"])
@pytest.mark.parametrize("base", [0, 0x100000000 - 1500], ids=["low_xids", "across_the_wrap"])
def test_randomised_differential(gpu_ctx, base, kind):
    rel, tids, snaps, clog, refs = corpus(base)
    n = len(tids)
    assert snaps[kind]["xip"] != sorted(snaps[kind]["xip"]) and len(rel.pages) > 10
    # the reference alone decides most of the corpus and shows every outcome: the device cannot pass by deciding nothing
    rmask, rst, rund, kinds = refs[kind]
    assert rst["n_visible"] + rst["n_invisible"] >= 0.8 * n and rst["n_visible"] >= 5 and rst["n_invisible"] - rst["n_deleted"] >= 5
    assert rst["n_deleted"] >= 50 and rst["n_dead_line_pointer"] >= 5
    total = {r: sum(refs[k][1]["undecided_by_reason"][r] for k in refs) for r in V.REASONS}
    assert all(v >= 5 for v in total.values()), total
    always = [r for r in V.REASONS if r != "suboverflow"]
    assert all(rst["undecided_by_reason"][r] >= 5 for r in always), rst
    assert (rst["undecided_by_reason"]["suboverflow"] >= 5) == ("suboverflowed" in kind)
    print(kind, {k: v for k, v in rst.items()})
    mask, st, und, _ = V.check_against_ref(gpu_ctx, rel, tids, snaps[kind], clog)
    assert (mask == rmask).all() and st == rst and (und == rund).all()
    if base:  # the snapshot straddles the wrap
        assert snaps[kind]["xmin"] > 0xF0000000 and snaps[kind]["xmax"] < 0x1000


def test_undecided_list_capacity(gpu_ctx):
    """cap bounds what is handed back (the smallest nodes), never what is counted; cap 0 wants no list"""
    rel, tids, snaps, clog, refs = corpus(0)
    rund = refs["plain"][2]
    heap = V.resident(gpu_ctx, rel)
    try:
        for cap in (0, 1, 7, len(rund), len(rund) + 5):
            mask, st, und, nu = V.dev_visibility(gpu_ctx, heap, tids, snaps["plain"], clog, cap=cap)
            assert nu == len(rund) == st["n_undecided"] and (und == rund[:cap]).all() and (mask == refs["plain"][0]).all()
        mask, st, und, nu = V.dev_visibility(gpu_ctx, heap, tids[:0], snaps["plain"], clog)  # no node at all
        assert st == V.empty_stats() and nu == 0 and und.size == 0
    finally:
        heap.close()


# ---- 3. HOT chains ----------------------------------------------------------------------------------------------------------------------
def _chain(rel, members, redirect=True):
    """members: header dicts in chain order; t_ctid of each is pointed at the next -> the tid an index would hold (the redirected
    root, or the first member) and the members' offsets"""
    blk = max(len(rel.pages) - 1, 0)
    root = None
    if redirect:
        blk, root = rel.add_item(tup(0, m=XMIN_INVALID))
    offs = []
    for hdr in members:
        b, o = rel.add_item(tup(**hdr))
        assert b == blk or not offs and root is None
        blk = b
        offs.append(o)
    for o, nxt in zip(offs, offs[1:]):
        V.patch_header(rel, V.tid_of(blk, o), ctid_off=nxt)
    if redirect:
        rel.set_line_pointer(blk, root, HP.LP_REDIRECT, lp_off=offs[0])
    return V.tid_of(blk, root if redirect else offs[0]), offs


def _versions(length, visible_at):
    """a row updated length - 1 times by committed transactions 50, 52, ..: member i was made by xid 50 + 2i and replaced by the
    next one; the member at `visible_at` is the last the snapshot sees (its replacement, if any, is still running: xid 150 is in xip)"""
    out = []
    for i in range(length):
        last = i == length - 1
        xmin = 50 + 2 * i if i <= visible_at else 150
        xmax = 0 if last else (150 if i >= visible_at else 52 + 2 * i)
        out.append(dict(xmin=xmin, xmax=xmax, m=(MI if last else 0), m2=(0 if last else HOT_UPDATED) | (ONLY_TUPLE if i else 0)))
    return out


def test_hot_chains_with_the_visible_member_at_each_position(gpu_ctx):
    rel = HP.HeapRelation()
    tids, expect = [], []
    for redirect in (True, False):
        for length in range(1, 6):
            for at in range(length):
                tid, _ = _chain(rel, _versions(length, at), redirect)
                tids.append(tid)
                expect.append((1, at))
    # nothing visible: every version replaced by a committed update, the last one deleted
    dead = _versions(5, 4)
    dead[4].update(xmax=60, m=0)
    tid, _ = _chain(rel, dead)
    tids.append(tid)
    expect.append((0, 4))
    assert len(rel.pages) == 1
    tids = np.array(tids, np.uint64)
    c = _clog()
    for x in (52, 54, 56, 58):
        c.set(x, V.COMMITTED)
    heap = V.resident(gpu_ctx, rel)
    try:
        mask, st, und, nu = V.dev_visibility(gpu_ctx, heap, tids, SNAP, c)
        assert mask.tolist() == [e[0] for e in expect] and nu == 0
        assert st["chain_hops"] == sum(e[1] for e in expect) and st["n_visible"] == len(tids) - 1 and st["n_invisible"] == 1
        V.check_against_ref(gpu_ctx, rel, tids, SNAP, c, heap=heap)
        for i in (0, 7, len(tids) - 1):  # one chain alone: its hops
            _, st1, _, _ = V.dev_visibility(gpu_ctx, heap, tids[i:i + 1], SNAP, c)
            assert st1["chain_hops"] == expect[i][1]
    finally:
        heap.close()


def test_broken_and_odd_chains(gpu_ctx):
    rel = HP.HeapRelation()
    old = dict(xmin=50, xmax=60, m2=HOT_UPDATED)                     # replaced by the committed xid 60
    new = dict(xmin=60, m=MI, m2=ONLY_TUPLE)                         # ... whose version everyone sees
    cases = []
    cases.append(("a whole chain", _chain(rel, [old, new])[0], 1, None))
    cases.append(("xmin != the previous xmax: broken", _chain(rel, [old, dict(new, xmin=99)])[0], 0, None))
    cases.append(("a frozen successor reads as xid 2: broken", _chain(rel, [old, dict(new, m=MI | FROZEN)])[0], 0, None))
    cases.append(("a frozen successor of xmax 2 matches", _chain(rel, [dict(old, xmax=2, m=XMAX_COMMITTED), dict(new, xmin=777, m=MI | FROZEN)])[0], 1, None))
    cases.append(("a heap-only tuple at the start", _chain(rel, [new], redirect=False)[0], 0, None))
    cases.append(("a heap-only tuple behind a redirect is a chain's member", _chain(rel, [new])[0], 1, None))
    tid, offs = _chain(rel, [old, new])
    rel.set_line_pointer(0, offs[1], HP.LP_REDIRECT, lp_off=offs[0])
    cases.append(("a redirect met after the start", tid, 0, None))
    tid, offs = _chain(rel, [old, new])
    rel.set_line_pointer(0, offs[1], HP.LP_DEAD)
    cases.append(("a dead line pointer inside a chain", tid, 0, None))
    tid, offs = _chain(rel, [old])
    V.patch_header(rel, V.tid_of(0, offs[0]), ctid_off=999)
    cases.append(("t_ctid beyond the line pointers", tid, 0, None))
    cases.append(("not HOT updated: the chain ends", _chain(rel, [dict(old, m2=0), new])[0], 0, None))
    cases.append(("xmin known aborted ends the chain", _chain(rel, [dict(xmin=55, xmax=60, m=XMIN_INVALID, m2=HOT_UPDATED), new])[0], 0, None))
    # a multixact updater in the middle: where the rule itself meets it, and where only the chain walk does (the member's xmin aborted)
    mid = dict(xmin=60, xmax=9999, m=IS_MULTI, m2=HOT_UPDATED | ONLY_TUPLE)
    cases.append(("multixact updater, member's xmin committed", _chain(rel, [old, mid, dict(new, xmin=9999)])[0], 1, "multixact"))
    cases.append(("multixact updater, member's xmin aborted",
                  _chain(rel, [dict(xmin=55, xmax=115, m2=HOT_UPDATED), dict(mid, xmin=115), dict(new, xmin=9999)])[0], 1, "multixact"))
    # a multixact that only locks hides no update xid: the walk goes on (to a version of xid 9999, which the snapshot cannot see)
    cases.append(("multixact locker only: followed", _chain(rel, [dict(xmin=55, xmax=115, m2=HOT_UPDATED),
                                                                  dict(mid, xmin=115, m=IS_MULTI | LOCK_ONLY), dict(new, xmin=9999)])[0], 0, None))
    assert len(rel.pages) == 1
    tids = np.array([c[1] for c in cases], np.uint64)
    heap = V.resident(gpu_ctx, rel)
    try:
        mask, st, und, nu = V.dev_visibility(gpu_ctx, heap, tids, SNAP, _clog())
        for i, (what, _, byte, reason) in enumerate(cases):
            assert mask[i] == byte and (i in und) == (reason is not None), what
        assert st["undecided_by_reason"]["multixact"] == 2 == nu
        V.check_against_ref(gpu_ctx, rel, tids, SNAP, _clog(), heap=heap)
    finally:
        heap.close()


@pytest.mark.parametrize("length", [1, 2])
def test_a_cycle_is_an_error(gpu_ctx, length):
    import pgvectorscale_amd as P
    rel = HP.HeapRelation()
    for _ in range(5):
        rel.add_item(tup(50, m=MI))
    # aborted versions (xid 115) pointing at each other: every one invisible, every one followed
    tid, offs = _chain(rel, [dict(xmin=115, xmax=115, m2=HOT_UPDATED | (ONLY_TUPLE if i else 0)) for i in range(length)], redirect=False)
    V.patch_header(rel, V.tid_of(0, offs[-1]), ctid_off=offs[0])
    heap = V.resident(gpu_ctx, rel)
    try:
        with pytest.raises(V.Malformed, match="cycle"):
            V.ref_visibility(rel.pages, rel.page_size, 1, [tid], SNAP, _clog())
        with pytest.raises(P.VsError, match=r"heap block 0 item \d+: .*cycle") as e:
            V.dev_visibility(gpu_ctx, heap, np.array([V.tid_of(0, 1), tid], np.uint64), SNAP, _clog())
        assert e.value.code == INVALID
        mask, st, _, _ = V.dev_visibility(gpu_ctx, heap, np.array([V.tid_of(0, 1)], np.uint64), SNAP, _clog())  # the fork is still good
        assert mask.tolist() == [1]
    finally:
        heap.close()


# ---- 4. the resident fork ---------------------------------------------------------------------------------------------------------------
def _rows(n, page_size=HP.BLCKSZ):
    rel = HP.HeapRelation(page_size)
    tids = np.array([V.tid_of(*rel.add_item(tup(50 if i % 3 else 120, m=MI))) for i in range(n)], np.uint64)
    return rel, tids


def test_blocks_in_any_order_overwrites_and_growth(gpu_ctx):
    from pgvectorscale_amd.pages import HeapResident
    rel, tids = _rows(1200)
    nb, ps = len(rel.pages), rel.page_size
    assert nb >= 6 and max(rel.max_offset(b) for b in range(nb)) == 185
    c = _clog()
    heap = HeapResident(gpu_ctx, 2)  # (capacity for two blocks: every put below the first grows the buffer)
    try:
        assert heap.blocks() == 0
        rmask, rst, _, _ = V.ref_visibility(rel.pages, ps, 0, tids, SNAP, c)
        mask, st, _, _ = V.dev_visibility(gpu_ctx, heap, tids, SNAP, c)  # nothing put yet: nothing found
        assert not mask.any() and st == rst and st["n_not_found"] == len(tids)
        # descending, one block at a time; a tid on a block never put is not found
        for b in range(nb - 1, 1, -1):
            heap.put(bytes(rel.pages[b]), first_block=b)
            assert heap.blocks() == nb
        holes = [bytearray(ps), bytearray(ps)] + rel.pages[2:]
        rmask, rst, _, _ = V.ref_visibility(holes, ps, nb, tids, SNAP, c)
        mask, st, _, _ = V.dev_visibility(gpu_ctx, heap, tids, SNAP, c)
        assert (mask == rmask).all() and st == rst and st["n_not_found"] == int(((tids >> np.uint64(16)) < 2).sum()) > 0
        # two overlapping ranges
        heap.put(b"".join(bytes(p) for p in rel.pages[0:4]), first_block=0)
        heap.put(b"".join(bytes(p) for p in rel.pages[2:nb]), first_block=2)
        assert heap.blocks() == nb
        V.check_against_ref(gpu_ctx, rel, tids, SNAP, c, heap=heap)
        # a "delete" by the committed xid 60 on block 1, the block put again: the bytes flip
        seen = V.ref_visibility(rel.pages, ps, nb, tids, SNAP, c)[0]
        victims = [int(t) for t, v in zip(tids, seen) if int(t) >> 16 == 1 and v][::7]
        assert len(victims) > 10
        for t in victims:
            V.patch_header(rel, t, xmax=60, m=XMAX_COMMITTED)
        before, _, _, _ = V.dev_visibility(gpu_ctx, heap, np.array(victims, np.uint64), SNAP, c)
        assert before.all()
        heap.put(bytes(rel.pages[1]), first_block=1)
        after, _, _, _ = V.dev_visibility(gpu_ctx, heap, np.array(victims, np.uint64), SNAP, c)
        assert not after.any()
        V.check_against_ref(gpu_ctx, rel, tids, SNAP, c, heap=heap)
        # far beyond the capacity: the blocks in between read as new pages
        far = nb + 40
        heap.put(bytes(rel.pages[0]), first_block=far)
        assert heap.blocks() == far + 1
        t2 = np.append(tids, [V.tid_of(far, 1), V.tid_of(far - 1, 1), V.tid_of(far + 1, 1)]).astype(np.uint64)
        mask, st, _, _ = V.dev_visibility(gpu_ctx, heap, t2, SNAP, c)
        assert mask[-3:].tolist() == [int(rmask_first(rel, SNAP, c)), 0, 0] and st["n_not_found"] == 2
    finally:
        heap.close()


def rmask_first(rel, snap, c):
    return V.ref_visibility(rel.pages, rel.page_size, len(rel.pages), [V.tid_of(0, 1)], snap, c)[0][0]


def test_16k_pages(gpu_ctx):
    rel, tids = _rows(800, page_size=16384)
    assert len(rel.pages) >= 2 and max(rel.max_offset(b) for b in range(len(rel.pages))) > 300
    _, rst, _, _ = V.check_against_ref(gpu_ctx, rel, tids, SNAP, _clog())
    assert rst["n_visible"] > 0 and rst["n_invisible"] > 0


# ---- 5. malformed pages -----------------------------------------------------------------------------------------------------------------
def _damage_item_low(rel):
    rel.set_line_pointer(1, 5, HP.LP_NORMAL, lp_off=40, lp_len=40)  # inside the line pointer array, below pd_upper
    return 5


def _damage_item_high(rel):
    rel.set_line_pointer(1, 6, HP.LP_NORMAL, lp_off=rel.page_size - 16, lp_len=40)  # runs past pd_special
    return 6


def _damage_len(rel):
    lp = struct.unpack_from("<I", rel.pages[1], 24 + 4 * 6)[0]
    rel.set_line_pointer(1, 7, HP.LP_NORMAL, lp_off=lp & 0x7FFF, lp_len=22)
    return 7


def _damage_page_size(rel):
    struct.pack_into("<H", rel.pages[1], 18, 4096 | 4)
    return 9


def _damage_header(rel):
    struct.pack_into("<H", rel.pages[1], 12, rel.page_size + 8)  # pd_lower beyond the page: the line pointers would run out of it
    return 9


@pytest.mark.parametrize("damage,why", [(_damage_item_low, "outside pd_upper"), (_damage_item_high, "outside pd_upper"),
                                        (_damage_len, "outside pd_upper"), (_damage_page_size, "pagesize"), (_damage_header, "page header")],
                         ids=["item_below_upper", "item_past_special", "lp_len_22", "page_size_word", "pd_lower"])
def test_malformed_pages_are_errors_that_name_the_place(gpu_ctx, damage, why):
    import pgvectorscale_amd as P
    rel, tids = _rows(400)
    off = damage(rel)
    with pytest.raises(V.Malformed) as r:
        V.ref_visibility(rel.pages, rel.page_size, len(rel.pages), [V.tid_of(1, off)], SNAP, _clog())
    assert (r.value.blk, r.value.off) == (1, off)
    heap = V.resident(gpu_ctx, rel)
    try:
        with pytest.raises(P.VsError, match=f"heap block 1 item {off}: .*{why}") as e:
            V.dev_visibility(gpu_ctx, heap, np.array([V.tid_of(0, 1), V.tid_of(1, off), V.tid_of(2, 1)], np.uint64), SNAP, _clog())
        assert e.value.code == INVALID
        on_good = tids[(tids >> np.uint64(16)) != 1]
        mask, _, _, _ = V.dev_visibility(gpu_ctx, heap, on_good, SNAP, _clog())  # the other blocks still answer
        assert (mask == V.ref_visibility(rel.pages, rel.page_size, len(rel.pages), on_good, SNAP, _clog())[0]).all()
    finally:
        heap.close()


# ---- 6. on an index ---------------------------------------------------------------------------------------------------------------------
COUNTERS = ("visited_nodes", "candidate_nodes", "quantized_distance_comparisons", "full_distance_comparisons", "node_reads", "node_heap_reads",
            "next_calls")


def _mask_of(ix, ctx, sid, n):
    """the library's own mask of a snapshot id, read back through vs_index_snapshot_use"""
    from pgvectorscale_amd import _lib
    prev, mine = C.c_void_p(), C.c_void_p()
    _lib.check(ix._L.vs_index_snapshot_use(ix.h, sid, C.byref(prev)))
    _lib.check(ix._L.vs_index_snapshot_use(ix.h, 0, C.byref(mine)))
    _lib.check(ix._L.vs_index_set_visibility_dev(ix.h, prev))
    return ctx.download(mine, np.empty(n, np.uint8))


def _search_under(ix, sid, q):
    from pgvectorscale_amd import _lib
    _lib.check(ix._L.vs_index_snapshot_use(ix.h, sid, None))
    try:
        return ix.search_batch(q, search_list_size=40, rescore=20, k=10)
    finally:
        _lib.check(ix._L.vs_index_snapshot_use(ix.h, 0, None))


def _same_search(a, b):
    (ai, at, ad, ast), (bi, bt, bd, bst) = a, b
    assert (ai == bi).all() and (at == bt).all() and (ad.view(np.uint32) == bd.view(np.uint32)).all()
    for c in COUNTERS:
        assert ast[c] == bst[c], c


@pytest.fixture
def vis_index(gpu_ctx, oracle):
    n = 600
    rel, tids, snap, clog = V.random_corpus(n, seed=23)
    tids = V.index_order(tids, seed=4)
    ti = TestIndex(n=n, dim_full=64, bits=2, R=16, distance=oracle.L2, seed=81, kind="gauss", L_build=30)
    ti.tids = tids
    ix = ti.upload(gpu_ctx)
    heap = V.resident(gpu_ctx, rel)
    ref = V.ref_visibility(rel.pages, rel.page_size, len(rel.pages), tids, snap, clog)
    yield ti, ix, heap, snap, clog, ref
    heap.close()
    ix.close()


def test_snapshot_eval_patch_and_put_dev_on_an_index(gpu_ctx, vis_index):
    from pgvectorscale_amd import _lib
    ti, ix, heap, snap, clog, (rmask, rst, rund, _) = vis_index
    n = ti.n
    q = ti.queries(32, seed=5, kind="gauss")
    st, und, nu = ix.snapshot_eval(heap, 1, snap, clog.xact())
    assert st == rst and nu == len(rund) and (und == rund).all() and len(rund) > 5 and rst["n_invisible"] > 100
    assert (_mask_of(ix, gpu_ctx, 1, n) == rmask).all()
    # a batch under the evaluated mask == the same batch under the reference's mask put from the host
    _lib.check(ix._L.vs_index_snapshot_put(ix.h, 2, rmask.ctypes.data_as(C.c_void_p)))
    under_eval = _search_under(ix, 1, q)
    _same_search(under_eval, _search_under(ix, 2, q))
    live = under_eval[0][under_eval[0] != 0xFFFFFFFF]
    assert rmask[live].all() and not (_search_under(ix, 0, q)[0] == under_eval[0]).all()  # (the mask matters to these queries)
    # the shim settles the undecided few: here every other one turns out invisible
    settled = (np.arange(len(rund)) % 2).astype(np.uint8)
    ix.snapshot_patch(1, rund, settled)
    want = rmask.copy()
    want[rund] = settled
    assert (_mask_of(ix, gpu_ctx, 1, n) == want).all()
    _lib.check(ix._L.vs_index_snapshot_put(ix.h, 2, want.ctypes.data_as(C.c_void_p)))
    _same_search(_search_under(ix, 1, q), _search_under(ix, 2, q))
    ix.snapshot_patch(1, [5, 9, 5], [0, 1, 7])  # the last entry of a node wins; any non-zero value is 1
    want[5], want[9] = 1, 1
    assert (_mask_of(ix, gpu_ctx, 1, n) == want).all()
    # evaluating again replaces the mask in place
    st2, _, _ = ix.snapshot_eval(heap, 1, snap, clog.xact(), cap=0)
    assert st2 == rst and (_mask_of(ix, gpu_ctx, 1, n) == rmask).all()
    # a mask that is already in device memory
    d = gpu_ctx.alloc(n)
    try:
        other = (np.arange(n) % 3 != 0).astype(np.uint8)
        gpu_ctx.upload(d, other)
        ix.snapshot_put_dev(3, d)
        gpu_ctx.upload(d, np.zeros(n, np.uint8))  # (a copy was taken)
        assert (_mask_of(ix, gpu_ctx, 3, n) == other).all()
        _lib.check(ix._L.vs_index_snapshot_put(ix.h, 2, other.ctypes.data_as(C.c_void_p)))
        _same_search(_search_under(ix, 3, q), _search_under(ix, 2, q))
    finally:
        gpu_ctx.free(d)


def test_rows_inserted_after_an_evaluation_are_invisible_to_it(gpu_ctx, vis_index):
    ti, ix, heap, snap, clog, (rmask, _, _, _) = vis_index
    n = ti.n
    ix.snapshot_eval(heap, 1, snap, clog.xact())
    new = make_vectors(4, 64, 78, "gauss")
    ix.insert(new, ((np.arange(4, dtype=np.uint64) + 9000) << np.uint64(16)) | np.uint64(1), search_list_size=40)
    ix._refresh()
    assert ix.desc.n == n + 4
    got = _mask_of(ix, gpu_ctx, 1, n + 4)
    assert (got[:n] == rmask).all() and not got[n:].any()
    # ... and an evaluation after the insert judges them like every other row: their blocks were never put
    st, _, _ = ix.snapshot_eval(heap, 1, snap, clog.xact())
    assert st["n_not_found"] == 4 and (_mask_of(ix, gpu_ctx, 1, n + 4)[:n] == rmask).all()


def test_refusals_change_nothing(gpu_ctx, vis_index):
    import pgvectorscale_amd as P
    ti, ix, heap, snap, clog, (rmask, _, _, _) = vis_index
    n = ti.n
    x = clog.xact()
    for sid in (0, 16):
        for call in (lambda: ix.snapshot_eval(heap, sid, snap, x), lambda: ix.snapshot_put_dev(sid, C.c_void_p(4096)),
                     lambda: ix.snapshot_patch(sid, [0], [0])):
            with pytest.raises(P.VsError, match="snapshot id") as e:
                call()
            assert e.value.code == INVALID
    with pytest.raises(P.VsError, match="no visibility mask") as e:
        ix.snapshot_patch(4, [0], [0])
    assert e.value.code == STATE
    with pytest.raises(P.VsError, match="multiple of 4") as e:
        ix.snapshot_eval(heap, 1, snap, (x[0] + 1, x[1], x[2]))
    assert e.value.code == INVALID
    with pytest.raises(P.VsError) as e:  # (no mask was made by the refused call)
        P._lib.check(ix._L.vs_index_snapshot_use(ix.h, 1, None))
    assert e.value.code == STATE
    ix.snapshot_eval(heap, 1, snap, x)
    with pytest.raises(P.VsError, match=f"node {n}") as e:
        ix.snapshot_patch(1, [3, n], [0, 0])
    assert e.value.code == INVALID and (_mask_of(ix, gpu_ctx, 1, n) == rmask).all()
    # while a batch of the handle is in flight
    q = ti.queries(8, seed=6, kind="gauss")
    dq, d_ids = gpu_ctx.alloc(q.nbytes), gpu_ctx.alloc(len(q) * 10 * 4)
    gpu_ctx.upload(dq, q)
    ix.search_batch_dev(dq, len(q), 40, 20, 10, d_ids)
    try:
        for call in (lambda: ix.snapshot_eval(heap, 1, snap, x), lambda: ix.snapshot_put_dev(1, dq), lambda: ix.snapshot_patch(1, [0], [0])):
            with pytest.raises(P.VsError, match="in flight") as e:
                call()
            assert e.value.code == STATE
    finally:
        ix.search_batch_dev_finish()
        gpu_ctx.free(dq)
        gpu_ctx.free(d_ids)
    assert (_mask_of(ix, gpu_ctx, 1, n) == rmask).all()
