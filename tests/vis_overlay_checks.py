"""Shared checks of the visibility base and its overlays (vs_index_vis_base_eval / _slot_eval / _materialize, vs_search_batch_vis):
the corpus and the family of admissible snapshots, a Python restatement of the class rule of include/vsgpu.h, and the references the
device is held to.  Pages, the rule and the reference masks come from tests/heap_vis_checks.py, which this file imports and does not
change; expectations never come from the device."""
import contextlib

import numpy as np

import heap_vis_checks as V
from heap_vis_checks import M32, random_corpus, index_order, ref_visibility, resident  # noqa: F401  (re-exported for the tests)
from helpers import TestIndex
from oracle import oracle_py as O

WRAP_BASE = 0x100000000 - 1500
COUNTERS = ("visited_nodes", "candidate_nodes", "quantized_distance_comparisons", "full_distance_comparisons", "node_reads", "node_heap_reads",
            "next_calls")
INV = 0xFFFFFFFF
L, RESCORE, K = 40, 20, 10
INDEX_KW = dict(dim_full=64, bits=2, R=16, distance=1, seed=81, kind="gauss", L_build=30)  # the vis_index fixture's shape (distance 1 = L2)
SLOTS = (0, 1, 2, 3, 500, 1023, 7)  # slot 0 and six overlays, dealt round-robin to the scans of a mixed launch
SLOT_SNAP = {1: 0, 2: 1, 3: 2, 500: 4, 1023: 6, 7: 7}  # slot -> the family member whose overlay it holds


# ---- the class rule, restated ---------------------------------------------------------------------------------------------------------
class _RecordingOwn(frozenset):
    """the own-xid set of a snapshot that writes down every xid it is asked about: own(x) of the rule"""

    def __new__(cls, xids, consulted):
        self = super().__new__(cls, xids)
        self.consulted = consulted
        return self

    def __contains__(self, x):
        self.consulted.append(x)
        return super().__contains__(x)


@contextlib.contextmanager
def _recording(consulted):
    """The reference walk with every xid handed to own / in_snapshot / did_commit written down: in_snapshot and did_commit are the
    reference's functions wrapped, own() is the membership test of the set the reference makes of the snapshot's own_xids."""
    real_in, real_dc, real_set = V.in_snapshot, V.did_commit, getattr(V, "set", None)

    def recording_set(xs=()):
        return xs if isinstance(xs, _RecordingOwn) else set(xs)

    def in_snapshot(s, x):
        consulted.append(x)
        return real_in(s, x)

    def did_commit(clog, x):
        consulted.append(x)
        return real_dc(clog, x)

    V.in_snapshot, V.did_commit, V.set = in_snapshot, did_commit, recording_set  # (satisfies_mvcc: own = set(s.get("own_xids", ())))
    try:
        yield
    finally:
        V.in_snapshot, V.did_commit = real_in, real_dc
        if real_set is None:
            del V.set
        else:
            V.set = real_set


def class_of(pages, page_size, n_blocks, tid, horizon, clog):
    """-> (class, kind, hops, recent) of one tid under S_H: xmin = xmax = horizon, nothing else"""
    consulted = []
    s_h = dict(xmin=horizon, xmax=horizon, own_xids=_RecordingOwn((), consulted))
    with _recording(consulted):
        kind, hops = V.hot_search(pages, page_size, n_blocks, int(tid), s_h, clog)
    recent = any(x >= 3 and V.follows_eq(x, horizon) for x in consulted)
    undecided = kind in V.REASONS
    cls = 2 if (recent or undecided) else 1 if kind == "visible" else 0
    return cls, kind, hops, recent


def empty_base_stats():
    d = {k: 0 for k in ("r", "n_walked", "n_deleted", "n_not_found", "n_dead_line_pointer", "n_recent", "n_undecided", "chain_hops")}
    d["n_class"] = [0, 0, 0]
    d["undecided_by_reason"] = {r: 0 for r in V.REASONS}
    return d


def ref_base(pages, page_size, n_blocks, tids, horizon, clog, changed=None, prev=None):
    """the whole base evaluation -> (classes uint8 [n], depends list uint32 ascending, stats as VisBaseStats.as_dict gives them).
    changed (a set of block numbers) with prev (the classes before): only nodes on those blocks are walked."""
    n = len(tids)
    cls = np.zeros(n, np.uint8)
    if prev is not None:
        cls[:len(prev)] = prev[:n]
    st = empty_base_stats()
    for i, tid in enumerate(tids):
        if changed is not None and (int(tid) >> 16) not in changed:
            continue
        c, kind, hops, recent = class_of(pages, page_size, n_blocks, tid, horizon, clog)
        cls[i] = c
        st["n_walked"] += 1
        st["chain_hops"] += hops
        if kind in V.REASONS:
            st["n_undecided"] += 1
            st["undecided_by_reason"][kind] += 1
        elif recent:
            st["n_recent"] += 1
        if kind in ("deleted", "not_found", "dead_lp"):
            st[{"deleted": "n_deleted", "not_found": "n_not_found", "dead_lp": "n_dead_line_pointer"}[kind]] += 1
    dep = np.flatnonzero(cls == 2).astype(np.uint32)
    st["n_class"] = [int((cls == c).sum()) for c in range(3)]
    st["r"] = len(dep)
    return cls, dep, st


# ---- the family of admissible snapshots -----------------------------------------------------------------------------------------------
def family(snap, base, seed):
    """eight snapshots a backend could hold while the horizon is snap's xmin: xmin raised by 0..400, xmax lowered or raised, subsets
    of xip / subxip and of the own xids, other curcids, the suboverflowed and the recovery kind"""
    rng = np.random.default_rng(seed)
    B = lambda x: (x + base) & M32  # noqa: E731

    def subset(xs, p):
        return [int(x) for x in xs if rng.random() < p]

    xmin, xmax = snap["xmin"], snap["xmax"]
    fam = [
        dict(snap),
        dict(snap, xmin=(xmin + 137) & M32),
        dict(snap, xmin=(xmin + 400) & M32, xmax=(xmax - 300) & M32, xip=subset(snap["xip"], 0.5), subxip=subset(snap["subxip"], 0.5)),
        dict(snap, xmax=(xmax + 150) & M32, xip=subset(snap["xip"], 0.7)),
        dict(snap, own_xids=[B(1501)], curcid=3),
        dict(snap, own_xids=[], curcid=0, xip=subset(snap["xip"], 0.3), subxip=[]),
        dict(snap, suboverflowed=True, xmin=(xmin + 20) & M32),
        dict(snap, taken_during_recovery=True, xmin=(xmin + 50) & M32, subxip=subset(snap["subxip"], 0.6), curcid=15),
    ]
    # (shifted across the wrap, the corpus's own xids 1500..1502 land on the special xids 0..2, which no backend holds and the library
    # refuses: a family member keeps its normal own xids only)
    for s in fam:
        s["own_xids"] = [x for x in s.get("own_xids", ()) if x >= 3]
    return fam


class World:
    """a corpus in index order, its horizon, the restated base and the reference mask of every family snapshot: made once per shape"""

    def __init__(self, n, seed, base):
        self.n, self.base = n, base
        self.rel, tids, self.snap, self.clog = random_corpus(n, seed=seed, base=base)
        self.tids = index_order(tids, seed=seed + 1)
        self.horizon = self.snap["xmin"]
        self.family = family(self.snap, base, seed + 2)
        self.pages = lambda: (self.rel.pages, self.rel.page_size, len(self.rel.pages))
        self.cls, self.dep, self.base_stats = ref_base(*self.pages(), self.tids, self.horizon, self.clog)
        self.refs = [ref_visibility(*self.pages(), self.tids, s, self.clog) for s in self.family]  # (mask, stats, undecided, kinds)
        self._ti = None

    def index(self):
        """the index over this corpus: the fixture's shape, the corpus's tids (5 % of them vacuumed) in the oracle's view as well"""
        if self._ti is None:
            ti = TestIndex(n=self.n, **INDEX_KW)  # (not the cached one: the tids below are this world's)
            ti.tids = self.tids
            ti.oracle = O.OracleIndex(codes=ti.codes, nbrs=ti.nbrs, heap_tids=ti.tids, vecs=ti.vecs, mean=ti.mean, m2=ti.m2, count=ti.count,
                                      bits=ti.bits, dim_index=ti.dim_index, num_neighbors=ti.R, distance_type=ti.distance,
                                      default_start=ti.start)
            self._ti = ti
        return self._ti

    def mask(self, slot):
        return None if slot == 0 else self.refs[SLOT_SNAP[slot]][0]

    def ref_on_list(self, j, dep=None):
        """the reference of family snapshot j restricted to the depends list -> (stats, undecided nodes ascending)"""
        dep = self.dep if dep is None else dep
        _, st, und, _ = ref_visibility(*self.pages(), self.tids[dep], self.family[j], self.clog)
        return st, dep[und]


_worlds = {}


def world(n=600, seed=23, base=0):
    key = (n, seed, base)
    if key not in _worlds:
        _worlds[key] = World(n, seed, base)
    return _worlds[key]


def check_input_conditions(w):
    """what the inputs must show for the device not to pass by accident: asserted on the reference alone"""
    n = w.n
    assert (w.cls != 2).sum() >= 0.4 * n, w.base_stats
    assert (w.cls == 2).sum() >= 0.1 * n, w.base_stats
    masks = [r[0] for r in w.refs]
    most = max(int((masks[a] != masks[b]).sum()) for a in range(len(masks)) for b in range(a))
    assert most >= 20, most
    assert w.base_stats["n_recent"] >= 5 and w.base_stats["n_undecided"] >= 5
    for s in w.family:  # admissible: xmin and every own xid at or after the horizon
        assert V.follows_eq(s["xmin"], w.horizon) and all(V.follows_eq(x, w.horizon) for x in s.get("own_xids", ()))
    if w.base:
        assert w.horizon > 0xF0000000 and w.snap["xmax"] < 0x1000  # the family straddles the wrap


def check_soundness(w):
    """a class-0 / class-1 node has exactly that verdict under every snapshot of the family"""
    settled = w.cls != 2
    for (mask, _, und, _), s in zip(w.refs, w.family):
        assert (mask[settled] == w.cls[settled]).all(), s
        assert not np.isin(und, np.flatnonzero(settled)).any()


# ---- the device side ------------------------------------------------------------------------------------------------------------------
def read_mask(ix, ctx, sid, n):
    """the library's own mask of a legacy snapshot id, read back through vs_index_snapshot_use"""
    import ctypes as C
    from pgvectorscale_amd import _lib
    prev, mine = C.c_void_p(), C.c_void_p()
    _lib.check(ix._L.vs_index_snapshot_use(ix.h, sid, C.byref(prev)))
    _lib.check(ix._L.vs_index_snapshot_use(ix.h, 0, C.byref(mine)))
    _lib.check(ix._L.vs_index_set_visibility_dev(ix.h, prev))
    return ctx.download(mine, np.empty(n, np.uint8))


def device_classes(ix, ctx, w, heap, slot=1, sid=15):
    """the class bytes as the device holds them, read through two materialized masks: an overlay of all ones shows class 0 as the
    only zeros, an overlay of all zeros shows class 1 as the only ones"""
    hz, dep = ix.vis_base_info()
    ix.vis_slot_eval(heap, slot, dict(xmin=hz, xmax=hz), w.clog.xact(), cap=0)  # (any admissible snapshot: every byte is patched below)
    out = []
    for v in (1, 0):
        ix.vis_slot_patch(slot, dep, np.full(len(dep), v, np.uint8))
        ix.vis_materialize(slot, sid)
        out.append(read_mask(ix, ctx, sid, ix.desc.n))
    ix.vis_slot_drop(slot)
    ones, zeros = out
    cls = np.where(zeros == 1, 1, np.where(ones == 0, 0, 2)).astype(np.uint8)
    return cls, dep


def eval_overlays(ix, heap, w, slots=SLOT_SNAP):
    for slot, j in slots.items():
        ix.vis_slot_eval(heap, slot, w.family[j], w.clog.xact())


def search_under(ix, sid, q, **kw):
    from pgvectorscale_amd import _lib
    _lib.check(ix._L.vs_index_snapshot_use(ix.h, sid, None))
    try:
        return ix.search_batch(q, search_list_size=L, rescore=RESCORE, k=K, **kw)
    finally:
        _lib.check(ix._L.vs_index_snapshot_use(ix.h, 0, None))


def check_mixed_launch(ix, oracle_ix, q, slots, mask_of, run, tids, qlabels=None, counters=COUNTERS, min_affected=None, legacy=True):
    """One launch of len(q) scans that name `slots` (run(q, slots) -> the rows and counters of that launch).  Every scan's rows and
    distance bits equal the oracle run alone under the mask of that scan's snapshot; the counters equal the sum over the scans;
    and, scan for scan, the launch equals the legacy path under the materialized mask of the scan's slot (legacy id 1)."""
    nq = len(q)
    slots = np.asarray(slots, np.uint32)
    sub = lambda sel: None if qlabels is None else [qlabels[i] for i in sel]  # noqa: E731
    oi, od = np.empty((nq, K), np.uint32), np.empty((nq, K), np.float32)
    want = {c: 0 for c in counters}
    affected = 0
    try:
        oracle_ix.set_visibility(None)
        free_i, _, _ = oracle_ix.search_batch(q, L=L, rescore=RESCORE, k=K, qlabels=qlabels)
        for slot in sorted(set(int(s) for s in slots)):
            sel = np.flatnonzero(slots == slot)
            oracle_ix.set_visibility(mask_of(slot))
            oi[sel], od[sel], ost = oracle_ix.search_batch(q[sel], L=L, rescore=RESCORE, k=K, qlabels=sub(sel))
            for c in counters:
                want[c] += ost[c]
        affected = int((oi != free_i).any(axis=1).sum())
    finally:
        oracle_ix.set_visibility(None)
    if min_affected is not None:  # (asserted on the oracle alone, before the device is asked)
        assert affected >= min_affected, (affected, nq)
    gi, gt, gd, gst = run(q, slots)
    assert (gi == oi).all(), np.flatnonzero((gi != oi).any(axis=1))
    assert (gd.view(np.uint32) == od.view(np.uint32)).all()
    live = gi != INV
    assert (gt[live] == tids[gi[live]]).all()
    for c in counters:
        assert gst[c] == want[c], (c, gst[c], want[c])
    if legacy:
        total = {c: 0 for c in COUNTERS}
        for slot in sorted(set(int(s) for s in slots)):
            sel = np.flatnonzero(slots == slot)
            if slot:
                ix.vis_materialize(slot, 1)
            li, lt, ld, lst = search_under(ix, 1 if slot else 0, q[sel], qlabels=sub(sel))
            assert (li == gi[sel]).all() and (lt == gt[sel]).all() and (ld.view(np.uint32) == gd[sel].view(np.uint32)).all(), slot
            for c in COUNTERS:
                total[c] += lst[c]
        for c in COUNTERS:
            assert gst[c] == total[c], (c, gst[c], total[c])
    return gi, gt, gd, gst
