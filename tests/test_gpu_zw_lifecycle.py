"""Chains of vs_index_insert / vs_index_bulk_delete / vs_index_consolidate_deletes / vs_index_repair / vs_index_reserve on one
device-resident index, with check_index_everywhere (tests/lifecycle_checks.py) after EVERY step: each mutation invalidates or
regrows by hand what the index derived from its arrays (cosine divisors, label masks, the neighbors' masks, the visibility and
snapshot masks, what the launch planner remembered, the capacity), and a forgotten line only shows in an entry point the
single-step tests do not run.  `Chain` is the host's own account of what the index must hold — heap tids, label sets, first
carriers, masks, capacity — kept without asking the library.  Also runs on the lockstep interpreter (tests/test_emu_lifecycle.py)."""
import numpy as np
import pytest

from helpers import make_vectors
from lifecycle_checks import (CURSOR, EMU, INV, OFFSET, SEARCH, check_index_everywhere, check_pool_slot, check_search_batch, fresh_index,
                              label_csr, make_tids, oracle_of, pull_and_compare)

gpu = pytest.mark.gpu

N0 = 300 if EMU else 600   # starting rows (the interpreter runs the same chains on half of them)
R, L_BUILD, NQ, NLABELS = 16, 40, 24, 6
MAX_ROWS = 1400
COSINE, L2, IP = 0, 1, 2


class Chain:
    def __init__(self, gpu_ctx, O, *, dim, bits, distance, dim_index=None, labeled=False, seed=0, n0=None):
        self.ctx, self.O, self.distance, self.dim, self.labeled = gpu_ctx, O, distance, dim, labeled
        n0 = n0 or N0
        rng = np.random.default_rng(1000 + seed)
        self.rows = make_vectors(MAX_ROWS, dim, 500 + seed, "gauss")  # the rows of every insert to come, in node order
        if distance == COSINE:  # non-unit rows, and a zero row among the first rows and in every insert of 65 or more
            self.rows[::3] *= 2.5
            self.rows[7] = 0
            self.rows[n0 + 40::97] = 0
        self.n = n0
        self.capacity = n0
        self.tids = make_tids(0, n0)
        self.own = None      # the mask set_visibility put in force, grown by ones
        self.snaps = {}      # {id: mask} of the stored snapshots, grown by zeros
        self.qual = None     # (slot, bits as they were put): carried over a growth, rows added later read 0
        self.sets = self.first = None
        ix = fresh_index(gpu_ctx, self.rows[:n0], distance=distance, bits=bits, dim_index=dim_index, R=R, L=L_BUILD, tids=self.tids,
                         build=not labeled)
        if labeled:
            self.sets = [sorted(set(int(v) for v in rng.integers(1, NLABELS + 1, int(rng.integers(1, 4))))) for _ in range(n0)]
            ix.set_labels(*label_csr(self.sets))
            ix.build_graph(search_list_size=L_BUILD, max_alpha=1.2)
            self.first = {}
            self._first_carriers(0)
            assert ix.desc.n_label_starts == len(self.first) == NLABELS
        self.ix = ix
        self.q = np.concatenate([make_vectors(NQ - 4, dim, 900 + seed, "gauss"),
                                 self.rows[n0:n0 + 4] + np.float32(0.01) * make_vectors(4, dim, 901 + seed, "gauss")]).astype(np.float32)
        self.keys = None
        if labeled:
            self.keys = [sorted(set(int(v) for v in rng.integers(1, NLABELS + 1, int(rng.integers(1, 3))))) for _ in range(NQ)]

    def _first_carriers(self, begin):
        for i in range(begin, len(self.sets)):
            for l in self.sets[i]:
                self.first.setdefault(l, i)

    @property
    def live(self):
        return (self.tids & OFFSET) != 0

    def insert(self, k, labels=None):
        """-> stats; first_node, inserted and grew are held to the host's account"""
        assert self.n + k <= MAX_ROWS and (labels is not None) == self.labeled
        grew = int(self.n + k > self.capacity)
        if grew:
            self.capacity = max(self.n + k, self.capacity + self.capacity // 2)
        st = self.ix.insert(self.rows[self.n:self.n + k], make_tids(self.n, k), labels=labels, search_list_size=L_BUILD)
        assert (st["first_node"], st["inserted"], st["grew"]) == (self.n, k, grew), st
        self.tids = np.concatenate([self.tids, make_tids(self.n, k)])
        if self.labeled:
            self.sets += [list(s) for s in labels]
            self._first_carriers(self.n)
        if self.own is not None:
            self.own = np.concatenate([self.own, np.ones(k, np.uint8)])
        self.snaps = {sid: np.concatenate([m, np.zeros(k, np.uint8)]) for sid, m in self.snaps.items()}
        self.n += k
        assert self.ix.desc.n == self.n and self.ix.capacity == self.capacity
        return st

    def bulk_delete(self, nodes, seed=0):
        """ambulkdelete of the nodes' heap tids, handed over unsorted among tids no node has and duplicates"""
        nodes = np.unique(np.asarray(nodes, np.int64))
        rng = np.random.default_rng(seed)
        absent = ((rng.integers(10 ** 6, 10 ** 9, 7).astype(np.uint64)) << np.uint64(16)) | np.uint64(5)
        dead = np.concatenate([make_tids(0, self.n)[nodes], absent, make_tids(0, self.n)[nodes[:3]]])
        rng.shuffle(dead)
        hit = self.live & np.isin(np.arange(self.n), nodes)
        want = dict(tuples_removed=int(hit.sum()), num_index_tuples=int((self.live & ~hit).sum()), already_deleted=int((~self.live).sum()))
        assert self.ix.bulk_delete(dead) == want
        self.tids[hit] &= ~OFFSET
        return want

    def mark_deleted(self, nodes):
        nodes = np.unique(np.asarray(nodes, np.uint32))
        self.ix.mark_deleted(nodes)
        self.tids[nodes] &= ~OFFSET

    def consolidate(self, repair=True):
        st = self.ix.consolidate_deletes(repair=repair)
        assert st["tombstones"] == int((~self.live).sum()), st
        return st

    def reserve(self, capacity):
        self.ix.reserve(capacity)
        self.capacity = max(self.capacity, capacity)
        assert self.ix.capacity == self.capacity

    def set_visibility(self, mask):
        self.own = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.ix.set_visibility(self.own)

    def qual_put(self, slot, bits):
        bits = np.ascontiguousarray(bits, bool)
        assert bits.shape == (self.n,)
        self.ix.qual_put(slot, bits)
        self.qual = (slot, bits)

    def check(self, where):
        host, oidx = check_index_everywhere(self.ix, self.O, self.distance, self.q, self.keys, label_starts=self.first, label_sets=self.sets,
                                            visible=self.own, snapshots=self.snaps, qualifier=self.qual, where=where)
        assert (host["heap_tids"] == self.tids).all(), where
        assert host["vecs"].tobytes() == self.rows[:self.n].tobytes(), where
        return host, oidx

    def close(self):
        self.ix.close()


def _pointers(ix):
    from pgvectorscale_amd import _lib
    return [ix.array(a)[0].value for a in (_lib.ARR_CODES, _lib.ARR_NBRS, _lib.ARR_TIDS, _lib.ARR_VECS, _lib.ARR_VNORM)]


# ---- chain A: an unlabeled index through two growths, two vacuums, a reserve -----------------------------------------------------
GEOM_A = {"cosine_1bit_dim50": dict(dim=50, bits=1, distance=COSINE),            # vec_stride 52: a scalar tail of 18 in the rerank
          "l2_2bit_slice_64_of_96": dict(dim=96, dim_index=64, bits=2, distance=L2)}


def _pages_case(gpu_ctx, O, ch, host):
    """the grown, vacuumed index written out: the oracle writer's bytes; read back on the device: an index that searches like it"""
    from oracle import pages_py as PG
    from pgvectorscale_amd.pages import DevicePages
    ix = ch.ix
    mean, m2, cnt = ix.get_quantizer()
    meta = dict(num_dimensions=ix.desc.dim_full, num_dimensions_to_index=ix.desc.dim_index, bq_num_bits_per_dimension=ix.desc.bits,
                distance_type=ch.distance, num_neighbors=R, default_start=ix.desc.default_start, labeled_starts={},
                extension_version="0.8.0", search_list_size=100, max_alpha=1.2)
    w = PG.write_index(codes=host["codes"], nbrs=host["nbrs"], heap_tids=host["heap_tids"], mean=mean, m2=m2, count=cnt, means_first=True,
                       meta=meta)
    image = ix.write_pages(extension_version="0.8.0", search_list_size=100, max_alpha=1.2)
    assert image == w.rel.tobytes()
    pages = DevicePages(gpu_ctx, len(image) // PG.BLCKSZ)
    pages.add(image)
    back = pages.build_from_meta(vecs=host["vecs"])
    pages.close()
    try:
        got = back.download(vecs=True)
        assert all(got[k].tobytes() == host[k].tobytes() for k in ("codes", "nbrs", "heap_tids", "vecs"))
        check_search_batch(back, oracle_of(O, back, host, ch.distance), ch.q, None, "read back from the pages")
    finally:
        back.close()


@gpu
@pytest.mark.parametrize("geom", list(GEOM_A))
def test_chain_a_unlabeled_grow_vacuum_grow_vacuum_reserve(gpu_ctx, oracle, geom):
    ch = Chain(gpu_ctx, oracle, seed=1, **GEOM_A[geom])
    try:
        n0 = ch.n
        ch.qual_put(5, np.random.default_rng(12).random(n0) < 0.4)             # (carried through every growth and reserve below)
        ch.check("built")                                                      # 1
        assert ch.insert(65)["grew"] == 1                                      # 2: just over one wave, past the capacity of the upload
        ch.check("insert 65")
        rng = np.random.default_rng(2)
        ch.bulk_delete(np.flatnonzero(rng.random(ch.n) < 0.2), seed=3)         # 3
        ch.check("bulk delete 20 %")
        assert ch.consolidate()["rows_rewritten"] >= 1                         # 4
        ch.check("consolidate")
        assert ch.insert(300)["grew"] == 1                                     # 5: more than the first growth left room for
        ch.check("insert 300")
        start = int(ch.ix.desc.default_start)
        pick = np.concatenate([np.flatnonzero(rng.random(ch.n) < 0.1), np.arange(n0 + 60, n0 + 90), [start]])
        ch.bulk_delete(pick, seed=4)                                           # 6: inserted rows and the default start node among them
        assert not ch.live[start] and not ch.live[n0 + 70]
        ch.check("bulk delete with the start node")
        st = ch.consolidate(repair=False)                                      # 7
        assert st["rows_rewritten"] >= 1 and st["tombstones_kept"] == 1
        ch.check("consolidate without repair")
        ch.ix.repair()
        ch.check("repair")
        before = _pointers(ch.ix)
        ch.reserve(3000)                                                       # 8: every array moves
        assert all(a != b for a, b in zip(before, _pointers(ch.ix)))
        ch.check("reserve")
        assert ch.insert(1)["grew"] == 0                                       # 9: one row, one wave, into the reserved room
        host, _ = ch.check("insert 1")
        _pages_case(gpu_ctx, oracle, ch, host)
    finally:
        ch.close()


# ---- chain B: a labeled index; the neighbors' masks are part of every check --------------------------------------------------------
def _label_rows(rng, k, extra=None, every=3):
    sets = [sorted(set(int(v) for v in rng.integers(1, NLABELS + 1, int(rng.integers(1, 4))))) for _ in range(k)]
    if extra is not None:
        for i in range(1, k, every):
            sets[i] = sorted(set(sets[i] + [extra]))
    return sets


@gpu
def test_chain_b_labeled_new_label_vacuum_of_a_label_and_its_return(gpu_ctx, oracle):
    ch = Chain(gpu_ctx, oracle, dim=64, bits=2, distance=L2, labeled=True, seed=2)
    try:
        n0 = ch.n
        ch.keys[0], ch.keys[1], ch.keys[2], ch.keys[3] = [7], [7, 2], [99], [3]
        ch.check("built")
        rng = np.random.default_rng(5)
        ch.insert(65, labels=_label_rows(rng, 65, extra=7))                    # 1: label 7 arrives with the insert
        assert ch.first[7] == n0 + 1 and ch.ix.desc.n_label_starts == NLABELS + 1
        _, oidx = ch.check("insert 65 with a new label")
        assert (oidx.search_batch(ch.q[:1], qlabels=[[7]], **SEARCH)[0] >= n0)[0, 0]  # (the key [7] does find inserted rows)
        carriers = np.array([i for i, s in enumerate(ch.sets) if 3 in s])
        ch.bulk_delete(carriers, seed=6)                                       # 2: every carrier of label 3
        _, oidx = ch.check("bulk delete of a label")
        assert (oidx.search_batch(ch.q[3:4], qlabels=[[3]], **SEARCH)[0] == INV).all()
        assert (ch.ix.search_batch(ch.q[3:4], search_list_size=40, rescore=20, k=10, qlabels=[[3]])[0] == INV).all()
        assert ch.consolidate(repair=False)["rows_rewritten"] >= 1             # 3: the row rewrite alone, then the whole call (its
        ch.check("consolidate without repair")                                 #    repair pass; nothing names a tombstone any more)
        assert ch.consolidate()["rows_rewritten"] == 0
        ch.check("consolidate")
        ch.insert(40, labels=_label_rows(rng, 40, extra=3, every=2))           # 4: label 3 comes back
        _, oidx = ch.check("insert of the deleted label")
        assert (oidx.search_batch(ch.q[3:4], qlabels=[[3]], **SEARCH)[0] != INV).any()
        ch.ix.repair()                                                         # 5
        ch.check("repair")
    finally:
        ch.close()


# ---- chain C: scans, a pool and a broker that live across an insert and a consolidation ------------------------------------------
@gpu
def test_chain_c_live_scans_pool_and_broker_are_rescanned_not_recreated(gpu_ctx, oracle):
    """include/vsgpu.h: after an insert "open vs_scans, scan pools and brokers of the index must be ended or rescanned" — so a
    rescan on the old descriptor must hand out the grown index's rows"""
    import pgvectorscale_amd as P
    ch = Chain(gpu_ctx, oracle, dim=64, bits=2, distance=L2, seed=3)
    ix, q = ch.ix, ch.q
    n0 = ch.n
    L, rescore = CURSOR["L"], CURSOR["rescore"]
    scan = ix.beginscan()
    pool = P.ScanPool(ix, 2, search_list_size=L, rescore=rescore, kmax=16, rows_cap=1024)
    broker = P.Broker(ix, max_batch=8, max_wait_us=200, cursor_lanes=0)
    bscan = broker.beginscan()
    try:
        rng = np.random.default_rng(7)
        snap = (rng.random(n0) > 0.3).astype(np.uint8)
        broker.snapshot_put(1, snap)          # a snapshot taken before any of the inserts
        ch.snaps[1] = snap
        own = (rng.random(n0) > 0.2).astype(np.uint8)
        ch.set_visibility(own)                # the library's own mask: old zeros stay, new rows show

        def live_objects(where):
            host, oidx = ch.check(where)
            near = q[NQ - 4:]  # queries next to the first inserted rows
            oidx.set_visibility(ch.own)
            scan.rescan(near[0], search_list_size=L, rescore=rescore)
            pull_and_compare(scan, oidx.scan(near[0], L=L, rescore=rescore), where=(where, "scan"))
            for slot in (0, 1):
                pool.rescan(slot, near[slot + 1])
            for slot in (0, 1):
                check_pool_slot(pool, slot, oidx.scan(near[slot + 1], L=L, rescore=rescore), 16, 3, (where, "pool", slot))
            new_seen = dict.fromkeys([0] + list(ch.snaps), False)
            for sid, mask in [(0, None)] + sorted(ch.snaps.items()):
                oidx.set_visibility(mask)
                for i in range(NQ - 6, NQ):
                    ids, tids, dist = broker.search(q[i], None, SEARCH["L"], SEARCH["rescore"], SEARCH["k"], snapshot=sid)
                    oi, od, _ = oidx.search_batch(q[i:i + 1], **SEARCH)
                    assert (ids == oi[0]).all() and (dist.view(np.uint32) == od[0].view(np.uint32)).all(), (where, "broker", sid, i)
                    assert (tids[ids != INV] == ch.tids[ids[ids != INV]]).all()
                    new_seen[sid] |= bool((ids[ids != INV] >= n0).any())
                bscan.set_snapshot(sid)
                bscan.rescan(near[3], search_list_size=L, rescore=rescore)
                pull_and_compare(bscan, oidx.scan(near[3], L=L, rescore=rescore), rows=40, where=(where, "scan on the broker", sid))
            oidx.set_visibility(None)
            return host, new_seen

        live_objects("before any mutation")
        assert ch.insert(65)["grew"] == 1
        host, seen = live_objects("after an insert that moved the arrays")
        assert seen[0] and not seen[1]  # the inserted rows are there for everybody but the snapshot from before
        gi = ix.search_batch(q[NQ - 4:], search_list_size=40, rescore=20, k=10)[0]
        assert (gi >= n0).any() and ch.own[gi[gi != INV]].all()  # the own mask shows the new rows and keeps its zeros
        assert (ch.own[:n0] == own).all() and (ch.snaps[1][:n0] == snap).all() and not ch.snaps[1][n0:].any()
        ch.bulk_delete(np.flatnonzero(rng.random(ch.n) < 0.2), seed=8)
        assert ch.consolidate()["rows_rewritten"] >= 1
        live_objects("after a consolidation")
        # a snapshot stored into reserved room (capacity > n), then an insert that does not grow: the new row's byte of that mask is
        # whatever the allocation held unless the insert clears it.  (A block of ones is freed first so that "whatever" is not zero
        # by luck where the allocator hands the block back.)
        assert ix.capacity > ch.n + 1
        dirty = gpu_ctx.alloc(ix.capacity)
        gpu_ctx.upload(dirty, np.ones(ix.capacity, np.uint8))
        gpu_ctx.free(dirty)
        broker.snapshot_put(2, np.ones(ch.n, np.uint8))
        ch.snaps[2] = np.ones(ch.n, np.uint8)
        assert ch.insert(1)["grew"] == 0
        assert ch.snaps[2][:-1].all() and not ch.snaps[2][-1]
        live_objects("after an insert into reserved room")
    finally:
        bscan.endscan()
        broker.close()
        pool.close()
        scan.endscan()
        ch.close()


# ---- chain D: drawn chains ---------------------------------------------------------------------------------------------------------
KINDS = ("insert", "bulk_delete", "mark_deleted", "consolidate", "repair", "reserve", "set_visibility")
GEOM_D = (dict(dim=50, bits=1, distance=COSINE), dict(dim=64, bits=2, distance=L2, labeled=True),
          dict(dim=96, dim_index=64, bits=2, distance=L2), dict(dim=48, bits=2, distance=IP))
SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)
# A consolidation is expected to rewrite a row once this many nodes were deleted since the last one: with lists of up to 16 over a
# few hundred nodes the mean in-degree is several edges per node, so eight deleted nodes without a single in-edge between them
# (start nodes aside, of which an unlabeled index has one) do not happen; fewer are not asserted on.
REWRITE_FROM = 8


def draw_chain(seed):
    """-> (geometry, [operation, ...]): six operations, every argument drawn here, all legal in the state the ones before leave (an
    insert always is on an owner handle with a trained quantizer, no view and no caller-owned mask; deletes name live nodes; a
    consolidation needs no writer open, and none ever is)"""
    rng = np.random.default_rng(seed)
    geom = GEOM_D[int(rng.integers(len(GEOM_D)))]
    n = cap = N0
    live = np.ones(n, bool)
    fresh_dead = 0
    ops = []
    for _ in range(6):
        kind = KINDS[int(rng.integers(len(KINDS)))]
        if kind == "insert":
            k = int(rng.choice([1, 63, 64, 65, 130]))
            labels = None
            if geom.get("labeled"):
                labels = [sorted(set(int(v) for v in rng.integers(1, NLABELS + 3, int(rng.integers(1, 4))))) for _ in range(k)]
            grew = n + k > cap
            if grew:
                cap = max(n + k, cap + cap // 2)
            n += k
            live = np.concatenate([live, np.ones(k, bool)])
            ops.append(dict(kind=kind, k=k, labels=labels, grew=grew))
        elif kind in ("bulk_delete", "mark_deleted"):
            alive = np.flatnonzero(live)
            if kind == "bulk_delete":
                nodes = alive[rng.random(alive.size) < float(rng.choice([0.05, 0.2, 0.4]))]
            else:
                nodes = rng.choice(alive, min(alive.size, int(rng.integers(1, 20))), replace=False)
            live[nodes] = False
            fresh_dead += nodes.size
            ops.append(dict(kind=kind, nodes=np.sort(nodes)))
        elif kind == "consolidate":
            ops.append(dict(kind=kind, repair=bool(rng.integers(2)), tombstones=int((~live).sum()), nonempty=fresh_dead >= REWRITE_FROM))
            fresh_dead = 0
        elif kind == "repair":
            ops.append(dict(kind=kind))
        elif kind == "reserve":
            c = int(rng.choice([n // 2, n + 1, n + 200, 2 * n]))
            ops.append(dict(kind=kind, capacity=c, moves=c > cap))
            cap = max(cap, c)
        else:
            ops.append(dict(kind=kind, mask=(rng.random(n) > 0.3).astype(np.uint8) if rng.random() < 0.7 else None))
    return geom, ops


def test_the_drawn_chains_cover_every_operation():
    """(no device needed) what the eight seeds draw between them"""
    count = dict.fromkeys(KINDS, 0)
    grew = consolidated = labeled = moved = 0
    for seed in SEEDS:
        geom, ops = draw_chain(seed)
        labeled += bool(geom.get("labeled"))
        for op in ops:
            count[op["kind"]] += 1
            grew += op.get("grew", False)
            consolidated += op.get("nonempty", False)
            moved += op.get("moves", False)
    assert all(v >= 2 for v in count.values()), count
    assert grew >= 1 and consolidated >= 1 and labeled >= 1 and moved >= 1, (grew, consolidated, labeled, moved)


@gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_chain_d_drawn_operations(gpu_ctx, oracle, seed):
    geom, ops = draw_chain(seed)
    ch = Chain(gpu_ctx, oracle, seed=10 + seed, **geom)
    try:
        ch.check((seed, "built"))
        for step, op in enumerate(ops):
            kind = op["kind"]
            if kind == "insert":
                assert ch.insert(op["k"], labels=op["labels"])["grew"] == int(op["grew"])
            elif kind == "bulk_delete":
                ch.bulk_delete(op["nodes"], seed=seed * 10 + step)
            elif kind == "mark_deleted":
                ch.mark_deleted(op["nodes"])
            elif kind == "consolidate":
                st = ch.consolidate(repair=op["repair"])
                assert st["tombstones"] == op["tombstones"] and (st["rows_rewritten"] >= 1 or not op["nonempty"]), (st, op)
            elif kind == "repair":
                ch.ix.repair()
            elif kind == "reserve":
                before = _pointers(ch.ix)
                ch.reserve(op["capacity"])
                assert all(a != b for a, b in zip(before, _pointers(ch.ix))) == op["moves"]
            else:
                ch.set_visibility(op["mask"])
            ch.check((seed, step, kind))
    finally:
        ch.close()
