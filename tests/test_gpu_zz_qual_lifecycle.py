"""The chains of tests/test_gpu_zw_lifecycle.py and tests/test_gpu_zw_plain_lifecycle.py run again with a qualifier, a group column,
a mask and stored snapshots on the index, and with check_qualified_everywhere (tests/qual_lifecycle_checks.py) next to the chain's own
check after EVERY step: the exact qualified top-k, the qualified flat scan, grouped graph scans, the two top-k calls under a group cap
and a qualified scan pool read the mask in force, the tombstones, the qualifier bitmaps and the group column of the index AS IT
STANDS, and vs_index_reserve, growing inserts, vs_index_shrink_to_fit and vs_index_compact move, regrow or drop those by hand.  The
chains keep the host's own account of the group column next to the accounts `Chain` / `PlainChain` keep: old rows keep their value,
rows added since read VS_GROUP_NONE until they are patched, a compaction drops the column and every qualifier.  What the reference
did with the states a chain went through is asserted at the chain's end (qual_lifecycle_checks.require).  Also runs on the lockstep
interpreter (tests/test_emu_qual_lifecycle.py)."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_zw_plain_lifecycle as PL
from lifecycle_checks import INV, OFFSET, make_tids
from qual_lifecycle_checks import NONE, SEEN, check_qualified_everywhere, group_layout, merge, new_seen, require
from test_gpu_zw_lifecycle import COSINE, GEOM_A, IP, L2, L_BUILD, N0, NLABELS, NQ, Chain, _label_rows, _pointers

gpu = pytest.mark.gpu
STATE = -5
SLOT = 5
DENSITY = 0.4
# every chain must have shown all of these but the states a chain's docstring excepts
ALL_SEEN = tuple(SEEN)
# The queries the qualified checker runs: the first four (on the labeled chain those with the keys chain B sets by hand) and the four
# next to the first inserted rows.  With all 24 chain Q-A took 1.22 s on the device next to 0.32 s of chain A of
# tests/test_gpu_zw_lifecycle.py in the same run, with these eight 0.66 s (14 checked states against that chain's 10, each of them
# through both checkers); what a check costs is the host's restatements, which grow with the scans.
CHECKED = np.r_[0:4, NQ - 4:NQ]
CHECKED_PLAIN = np.r_[0:4, PL.NQ - 4:PL.NQ]


def _bits(n, seed):
    return np.random.default_rng(seed).random(n) < DENSITY


def _refused_state(call, word=""):
    import pgvectorscale_amd as P
    with pytest.raises(P.VsError) as e:
        call()
    assert e.value.code == STATE and word in str(e.value), str(e.value)


class QualChain(Chain):
    """`Chain` plus the group column's account, stored snapshots, shrink_to_fit and compact.  Heap tids come from a counter (a
    compaction renumbers the nodes, so a tid cannot be a function of the node id as in `Chain`)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.groups = None           # the column as it must stand now
        self.first_n = self.n        # the nodes below this were there from the start (renumbered by a compaction)
        self.tid_next = self.n
        self.total = new_seen()

    # -- the accounts
    def groups_put(self, values):
        values = np.ascontiguousarray(values, np.uint32)
        assert values.shape == (self.n,)
        self.ix.groups_put(values)
        self.groups = values.copy()

    def groups_patch(self, first, values):
        values = np.ascontiguousarray(values, np.uint32)
        self.ix.groups_patch(first, values)
        self.groups[first:first + values.size] = values

    def snapshot_put(self, sid, mask):
        from pgvectorscale_amd import _lib
        mask = np.ascontiguousarray(mask, np.uint8)
        assert mask.shape == (self.n,)
        _lib.check(self.ix._L.vs_index_snapshot_put(self.ix.h, sid, mask.ctypes.data_as(C.c_void_p)))
        self.snaps[sid] = mask

    def insert(self, k, labels=None):
        """Chain.insert with the tids of a counter; the new rows are ungrouped"""
        assert self.n + k <= len(self.rows) and (labels is not None) == self.labeled
        grew = int(self.n + k > self.capacity)
        if grew:
            self.capacity = max(self.n + k, self.capacity + self.capacity // 2)
        tids = make_tids(self.tid_next, k)
        st = self.ix.insert(self.rows[self.n:self.n + k], tids, labels=labels, search_list_size=L_BUILD)
        assert (st["first_node"], st["inserted"], st["grew"]) == (self.n, k, grew), st
        self.tid_next += k
        self.tids = np.concatenate([self.tids, tids])
        if self.labeled:
            self.sets += [list(s) for s in labels]
            self._first_carriers(self.n)
        if self.own is not None:
            self.own = np.concatenate([self.own, np.ones(k, np.uint8)])
        self.snaps = {sid: np.concatenate([m, np.zeros(k, np.uint8)]) for sid, m in self.snaps.items()}
        if self.groups is not None:
            self.groups = np.concatenate([self.groups, np.full(k, NONE, np.uint32)])
        self.n += k
        assert self.ix.desc.n == self.n and self.ix.capacity == self.capacity
        return st

    def bulk_delete(self, nodes, seed=0):
        nodes = np.unique(np.asarray(nodes, np.int64))
        rng = np.random.default_rng(seed)
        absent = ((rng.integers(10 ** 6, 10 ** 9, 7).astype(np.uint64)) << np.uint64(16)) | np.uint64(5)
        named = self.tids[nodes] | np.uint64(3)  # (make_tids: every live offset is 3; a dead node's tid names nothing any more)
        dead = np.concatenate([named, absent, named[:3]])
        rng.shuffle(dead)
        hit = self.live & np.isin(np.arange(self.n), nodes)
        want = dict(tuples_removed=int(hit.sum()), num_index_tuples=int((self.live & ~hit).sum()), already_deleted=int((~self.live).sum()))
        assert self.ix.bulk_delete(dead) == want
        self.tids[hit] &= ~OFFSET
        return want

    def shrink(self):
        self.ix.shrink_to_fit()
        self.capacity = self.n
        assert self.ix.capacity == self.capacity and self.ix.desc.n == self.n

    def compact(self):
        """the host renumbers its accounts with the map the call returns, after holding the map to its own: every live node and the
        default start node stay, in order.  Both the group column and the qualifier are gone afterwards."""
        assert not self.labeled
        keep = self.live.copy()
        keep[int(self.ix.desc.default_start)] = True
        want = np.where(keep, np.cumsum(keep) - 1, INV).astype(np.uint32)
        st, new_of = self.ix.compact(return_map=True)
        assert (new_of == want).all() and (st["n_before"], st["n_after"]) == (keep.size, int(keep.sum())), st
        self.rows = np.concatenate([self.rows[:keep.size][keep], self.rows[keep.size:]])
        self.tids = self.tids[keep]
        if self.own is not None:
            self.own = self.own[keep]
        self.snaps = {sid: m[keep] for sid, m in self.snaps.items()}
        self.first_n = int(keep[:self.first_n].sum())
        self.n = int(keep.sum())
        if self.qual is not None:
            _refused_state(lambda: self.ix.qual_info(self.qual[0]))
        self.qual = self.groups = None
        assert self.ix.desc.n == self.n and self.ix.capacity == self.capacity  # (the capacity stays as room for the next insert)
        return st

    def put_both(self, seed):
        self.qual_put(SLOT, _bits(self.n, seed))
        self.groups_put(group_layout(self.n, seed + 1))

    def check(self, where):
        host, oidx = super().check(where)
        keys = None if self.keys is None else [self.keys[i] for i in CHECKED]
        seen = check_qualified_everywhere(self.ix, self.O, self.distance, self.q[CHECKED], host, oidx, visible=self.own, snapshots=self.snaps,
                                          qualifier=self.qual, groups=self.groups, keys=keys, where=where)
        seen["inserted_row"] = seen["slot0_max_id"] >= self.first_n
        merge(self.total, seen)
        return host, oidx


def _sparse_snapshot(n, seed):
    """a snapshot that sees about one row in thirty: under it a scan runs out of rows before it has kept 10 (VS_QUAL_ENDED)"""
    return (np.random.default_rng(seed).random(n) < 0.03).astype(np.uint8)


# ---- chain Q-A: an unlabeled index through growth, vacuum, a snapshot, growth, reserve, shrink, growth, compaction -------------------
@gpu
@pytest.mark.parametrize("geom", list(GEOM_A))
def test_chain_qa_grow_patch_vacuum_snapshot_grow_reserve_shrink_grow_compact(gpu_ctx, oracle, geom):
    ch = QualChain(gpu_ctx, oracle, seed=1, **GEOM_A[geom])
    try:
        n0 = ch.n
        rng = np.random.default_rng(2)
        ch.put_both(12)                                                        # 1
        ch.check("built")
        assert ch.insert(65)["grew"] == 1                                      # 2: the bitmap crosses a word, the new rows neither
        assert not ch.ix.qual_download(SLOT)[n0:].any() and (ch.groups[n0:] == NONE).all()  # qualify nor carry a group
        ch.check("insert 65")
        ch.groups_patch(n0, group_layout(65, 13))                              # 3
        ch.qual_put(SLOT, _bits(ch.n, 14))
        ch.check("patched and put again")
        ch.bulk_delete(np.flatnonzero(rng.random(ch.n) < 0.2), seed=3)         # 4
        ch.check("bulk delete 20 %")
        ch.set_visibility((rng.random(ch.n) > 0.2).astype(np.uint8))           # 5
        ch.check("a mask hiding 20 %")
        assert ch.consolidate()["rows_rewritten"] >= 1                         # 6
        ch.check("consolidate")
        ch.snapshot_put(1, (rng.random(ch.n) > 0.3).astype(np.uint8))          # 7
        ch.snapshot_put(2, _sparse_snapshot(ch.n, 15))
        ch.check("snapshots stored")
        assert ch.insert(300)["grew"] == 1                                     # 8: the snapshots do not see these rows
        assert not ch.snaps[1][-300:].any() and ch.own[-300:].all()
        ch.check("insert 300")
        before = _pointers(ch.ix)
        ch.reserve(3000)                                                       # 9: every array moves, the column, the bitmap and the
        assert all(a != b for a, b in zip(before, _pointers(ch.ix)))           #    mask in force with them
        ch.check("reserve")
        before = _pointers(ch.ix)
        ch.shrink()                                                            # 10
        assert all(a != b for a, b in zip(before, _pointers(ch.ix)))
        ch.check("shrink_to_fit")
        assert ch.insert(1)["grew"] == 1                                       # 11: grows again, after the shrink
        assert ch.groups[-1] == NONE
        ch.check("insert 1 after the shrink")
        n_before = ch.n
        ch.compact()                                                           # 12: the column and the qualifier are dropped
        assert ch.n < n_before and ch.groups is None and ch.qual is None
        ch.check("compact")
        ch.put_both(16)
        ch.check("both put over the new numbering")
        require(ch.total, ALL_SEEN, geom)
    finally:
        ch.close()


# ---- chain Q-B: a labeled index; the grouped scan runs with label keys under a mask throughout ------------------------------------------
@gpu
def test_chain_qb_labeled_keys_under_a_mask(gpu_ctx, oracle):
    """(no snapshot is stored and the index is never compacted; the key [99] names a label no row carries: its scan ENDS at once)"""
    ch = QualChain(gpu_ctx, oracle, dim=64, bits=2, distance=L2, labeled=True, seed=2)
    try:
        n0 = ch.n
        ch.keys[0], ch.keys[1], ch.keys[2], ch.keys[3] = [7], [7, 2], [99], [3]
        rng = np.random.default_rng(5)
        ch.set_visibility((rng.random(ch.n) > 0.2).astype(np.uint8))
        ch.put_both(22)
        ch.check("built")
        ch.insert(65, labels=_label_rows(rng, 65, extra=7))                    # 1: label 7 arrives with the insert
        assert ch.first[7] == n0 + 1 and ch.ix.desc.n_label_starts == NLABELS + 1
        ch.check("insert 65 with a new label")
        ch.groups_patch(n0, group_layout(65, 23))
        ch.qual_put(SLOT, _bits(ch.n, 24))
        carriers = np.array([i for i, s in enumerate(ch.sets) if 3 in s])
        ch.bulk_delete(carriers, seed=6)                                       # 2: every carrier of label 3
        ch.check("bulk delete of a label")
        ch.consolidate()                                                       # 3
        ch.check("consolidate")
        g4 = group_layout(ch.n, 25)                                            # 4: every row patched into four groups or none: under
        ch.groups_patch(0, np.where(g4 == NONE, NONE, g4 % 4))                 #    a cap of 1 no scan finds 10 rows within 64 pops
        ch.check("every row patched into four groups")
        require(ch.total, ALL_SEEN, "chain Q-B")
    finally:
        ch.close()


# ---- chain Q-P: plain storage --------------------------------------------------------------------------------------------------------
class QualPlainChain(PL.PlainChain):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.groups = None
        self.first_n = self.n
        self.total = new_seen()

    def groups_put(self, values):
        values = np.ascontiguousarray(values, np.uint32)
        assert values.shape == (self.n,)
        self.ix.groups_put(values)
        self.groups = values.copy()

    def groups_patch(self, first, values):
        values = np.ascontiguousarray(values, np.uint32)
        self.ix.groups_patch(first, values)
        self.groups[first:first + values.size] = values

    def _appended(self, vecs, tids):
        super()._appended(vecs, tids)
        if self.groups is not None:
            self.groups = np.concatenate([self.groups, np.full(len(tids), NONE, np.uint32)])

    def check(self, where, pages=False):
        host, oidx = super().check(where, pages=pages)
        seen = check_qualified_everywhere(self.ix, self.O, self.distance, self.q[CHECKED_PLAIN], host, oidx, visible=self.own,
                                          snapshots=self.snaps, qualifier=self.qual, groups=self.groups, where=where)
        seen["inserted_row"] = seen["slot0_max_id"] >= self.first_n
        merge(self.total, seen)
        return host, oidx


@gpu
def test_chain_qp_plain_grow_vacuum_shrink_grow(gpu_ctx, oracle):
    """cosine over the first 24 of 40 dimensions: the scans fetch the heap (next_with_resort), so the mask acts on them.  The flat
    calls refuse plain storage (the checker asserts VS_ERR_STATE), so no flat cap is seen."""
    ch = QualPlainChain.built(gpu_ctx, oracle, seed=1, dim=40, dim_index=24, distance=COSINE)
    try:
        n0 = ch.n
        rng = np.random.default_rng(2)
        ch.set_visibility((rng.random(ch.n) > 0.2).astype(np.uint8))           # 1
        ch.snapshot_put(1, _sparse_snapshot(ch.n, 35))
        ch.qual_put(PL.QUAL_SLOT, _bits(ch.n, 32))
        ch.groups_put(group_layout(ch.n, 33))
        ch.check("built: mask, snapshot, qualifier, groups")
        before = PL._pointers(ch.ix)
        assert ch.insert(130)["grew"] == 1                                     # 2: the arrays move
        assert all(a != b for a, b in zip(before, PL._pointers(ch.ix))) and (ch.groups[n0:] == NONE).all()
        ch.check("insert 130")
        ch.groups_patch(n0, group_layout(130, 34))
        ch.bulk_delete(np.flatnonzero(rng.random(ch.n) < 0.3), seed=3)         # 3
        ch.check("patched; bulk delete 30 %")
        assert ch.consolidate()["rows_rewritten"] >= 1                         # 4
        ch.check("consolidate")
        ch.reserve(ch.n + 200)
        ch.shrink()                                                            # 5
        ch.check("reserve, shrink_to_fit")
        assert ch.insert(65)["grew"] == 1                                      # 6: past the shrunk capacity
        ch.check("insert 65 after the shrink")
        g4 = group_layout(ch.n, 36)                                            # 7: every row patched into four groups or none: under
        ch.groups_patch(0, np.where(g4 == NONE, NONE, g4 % 4))                 #    a cap of 1 no scan finds 10 rows within 64 pops
        ch.check("every row patched into four groups")
        require(ch.total, [k for k in ALL_SEEN if k != "cap_bites_flat"], "chain Q-P")
    finally:
        ch.close()


# ---- chain Q-D: drawn chains --------------------------------------------------------------------------------------------------------------
KINDS = ("insert", "bulk_delete", "mark_deleted", "consolidate", "repair", "reserve", "set_visibility",  # (KINDS of chain D)
         "groups_patch", "qual_put", "shrink_to_fit", "compact")
GEOM_D = (dict(dim=50, bits=1, distance=COSINE), dict(dim=96, dim_index=64, bits=2, distance=L2), dict(dim=48, bits=2, distance=IP))
SEEDS = (1, 2, 3, 4)
N_OPS = 10
MAX_USED = 1300


def draw_chain(seed):
    """-> (geometry, [operation, ...]): ten operations, every argument drawn here, all legal in the state the ones before leave.
    Impossible draws are drawn again: an insert past the rows a chain has, a delete that leaves fewer than 150 live rows.  A
    compaction wants tombstones that no kept row names any more: a drawn one brings the bulk_delete and the consolidation (with its
    repair) it still lacks as steps of their own in front of it.  It is followed by a put of both the qualifier and the column (the step after it is checked with both again)."""
    rng = np.random.default_rng(100 + seed)
    geom = GEOM_D[int(rng.integers(len(GEOM_D)))]
    n = cap = used = N0
    live = np.ones(n, bool)
    unconsolidated = False
    ops = []
    while len(ops) < N_OPS:
        kind = KINDS[int(rng.integers(len(KINDS)))]
        if kind == "insert":
            k = int(rng.choice([1, 63, 65, 130]))
            if used + k > MAX_USED:
                continue
            grew = n + k > cap
            if grew:
                cap = max(n + k, cap + cap // 2)
            n, used = n + k, used + k
            live = np.concatenate([live, np.ones(k, bool)])
            ops.append(dict(kind=kind, k=k, grew=grew))
        elif kind in ("bulk_delete", "mark_deleted"):
            alive = np.flatnonzero(live)
            if kind == "bulk_delete":
                nodes = alive[rng.random(alive.size) < float(rng.choice([0.05, 0.2, 0.4]))]
            else:
                nodes = rng.choice(alive, min(alive.size, int(rng.integers(1, 20))), replace=False)
            if alive.size - nodes.size < 150 or nodes.size == 0:
                continue
            live[nodes] = False
            unconsolidated = True
            ops.append(dict(kind=kind, nodes=np.sort(nodes)))
        elif kind == "consolidate":
            repair = bool(rng.integers(2))
            unconsolidated &= not repair
            ops.append(dict(kind=kind, repair=repair, tombstones=int((~live).sum())))
        elif kind == "repair":
            ops.append(dict(kind=kind))
        elif kind == "reserve":
            c = int(rng.choice([n // 2, n + 1, n + 200, 2 * n]))
            ops.append(dict(kind=kind, capacity=c, moves=c > cap))
            cap = max(cap, c)
        elif kind == "shrink_to_fit":
            ops.append(dict(kind=kind, moves=cap != n))
            cap = n
        elif kind == "compact":
            # a compaction wants tombstones that no kept row names: what is missing of that is drawn in front of it
            if len(ops) + 1 + int(live.all()) + int(unconsolidated or live.all()) > N_OPS:
                continue
            if live.all():
                nodes = np.flatnonzero(rng.random(n) < 0.2)
                live[nodes] = False
                unconsolidated = True
                ops.append(dict(kind="bulk_delete", nodes=nodes))
            if unconsolidated:
                ops.append(dict(kind="consolidate", repair=True, tombstones=int((~live).sum())))
            ops.append(dict(kind=kind, seed=int(rng.integers(1 << 30))))  # (n afterwards depends on the start node: the chain knows)
            live = None  # the numbering is the chain's to know from here on: deletes are drawn as fractions of the live rows
            break
        elif kind == "groups_patch":
            first = int(rng.integers(0, n - 1))
            ops.append(dict(kind=kind, first=first, count=int(rng.integers(1, min(n - first, 200) + 1)), seed=int(rng.integers(1 << 30))))
        else:
            ops.append(dict(kind=kind, seed=int(rng.integers(1 << 30)), clear=bool(kind == "set_visibility" and rng.random() < 0.3)))
    # after a compaction the node ids are the chain's alone: the rest of the chain is drawn from operations that name no node
    while len(ops) < N_OPS:
        kind = ("insert", "reserve", "set_visibility", "groups_patch", "qual_put", "shrink_to_fit", "repair")[int(rng.integers(7))]
        if kind == "insert":
            k = int(rng.choice([1, 63, 65, 130]))
            if used + k > MAX_USED:
                continue
            used += k
            ops.append(dict(kind=kind, k=k, grew=None))
        elif kind == "reserve":
            ops.append(dict(kind=kind, capacity=int(rng.choice([700, 1500])), moves=None))
        elif kind == "shrink_to_fit":
            ops.append(dict(kind=kind, moves=None))
        elif kind == "repair":
            ops.append(dict(kind=kind))
        elif kind == "groups_patch":
            ops.append(dict(kind=kind, first=int(rng.integers(0, 100)), count=int(rng.integers(1, 50)), seed=int(rng.integers(1 << 30))))
        else:
            ops.append(dict(kind=kind, seed=int(rng.integers(1 << 30)), clear=False))
    return geom, ops


def test_the_drawn_chains_cover_every_operation():
    """(no device needed) what the four seeds draw between them"""
    count = dict.fromkeys(KINDS, 0)
    geoms = set()
    grew = after_shrink = 0
    for seed in SEEDS:
        geom, ops = draw_chain(seed)
        assert len(ops) == N_OPS
        geoms.add(tuple(sorted(geom.items())))
        shrunk = False
        for op in ops:
            count[op["kind"]] += 1
            grew += bool(op.get("grew"))
            after_shrink += shrunk and op["kind"] == "insert"  # an insert after a shrink_to_fit (it grows: capacity == n)
            shrunk |= op["kind"] == "shrink_to_fit"
    assert all(v >= 1 for v in count.values()), count
    assert len(geoms) >= 2 and grew >= 1 and after_shrink >= 1, (geoms, grew, after_shrink)


def _run_drawn(ch, op, seed):
    kind = op["kind"]
    rng = np.random.default_rng(op.get("seed", 0))
    if kind == "insert":
        grew = ch.insert(op["k"])["grew"]
        assert op["grew"] is None or grew == int(op["grew"])
    elif kind == "bulk_delete":
        ch.bulk_delete(op["nodes"], seed=seed)
    elif kind == "mark_deleted":
        ch.mark_deleted(op["nodes"])
    elif kind == "consolidate":
        assert ch.consolidate(repair=op["repair"])["tombstones"] == op["tombstones"]
    elif kind == "repair":
        ch.ix.repair()
    elif kind == "reserve":
        before = _pointers(ch.ix)
        ch.reserve(op["capacity"])
        assert op["moves"] is None or all(a != b for a, b in zip(before, _pointers(ch.ix))) == op["moves"]
    elif kind == "shrink_to_fit":
        ch.shrink()
    elif kind == "set_visibility":
        ch.set_visibility(None if op["clear"] else (rng.random(ch.n) > 0.3).astype(np.uint8))
    elif kind == "groups_patch":
        first = min(op["first"], ch.n - 1)
        count = min(op["count"], ch.n - first)
        ch.groups_patch(first, group_layout(count, op["seed"] % 1000))
    elif kind == "qual_put":
        ch.qual_put(SLOT, _bits(ch.n, op["seed"]))
    else:
        ch.compact()


@gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_chain_qd_drawn_operations(gpu_ctx, oracle, seed):
    """(a drawn chain need not delete, hide or insert: only that the cap bites is required of each)"""
    geom, ops = draw_chain(seed)
    ch = QualChain(gpu_ctx, oracle, seed=20 + seed, **geom)
    try:
        ch.put_both(40 + seed)
        ch.check((seed, "built"))
        for step, op in enumerate(ops):
            _run_drawn(ch, op, seed * 10 + step)
            ch.check((seed, step, op["kind"]))
            if op["kind"] == "compact":
                ch.put_both(op["seed"] % 1000)
        require(ch.total, ("cap_bites", "cap_bites_exact", "cap_bites_flat", "complete"), ("chain Q-D", seed))
    finally:
        ch.close()
