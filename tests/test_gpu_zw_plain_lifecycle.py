"""Chains of vs_index_insert / vs_index_bulk_delete / vs_index_consolidate_deletes_plain / vs_index_compact / vs_index_reserve /
vs_index_shrink_to_fit / vs_pages_follow_apply on one device-resident `plain` storage index, with check_plain_everywhere
(tests/plain_lifecycle_checks.py) after EVERY step.  Plain storage keeps derived state SBQ does not — the launch plan of k_search_plain
sized from n for every batch, the capacities a plain scan pool clamps to the n of its creation, the divisors of the index slices of a
truncated cosine index, the qualifiers an insert carries over and a compaction drops — and a forgotten line only shows in an entry
point the single-step tests do not run after a mutation.  `PlainChain` is the host's own account of what the index must hold — rows,
heap tids, capacity, own mask, snapshots, qualifier bits — kept without asking the library.  Also runs on the lockstep interpreter
(tests/test_emu_plain_lifecycle.py)."""
import ctypes as C

import numpy as np
import pytest

import pages_follow_plain_checks as FC
import plain_build_checks as PB
from helpers import make_vectors
from lifecycle_checks import CURSOR, EMU, INV, OFFSET, check_pool_slot, make_tids, pull_and_compare
from plain_lifecycle_checks import FAST_PLAIN, PLAIN_CURSOR_KEYS, POOL, check_plain_everywhere

gpu = pytest.mark.gpu

# Starting rows and queries: 400 rows and 24 queries made chain A take three times the SBQ chain A on the device (0.60 s against 0.20 s),
# 300 and 16 still 2.2 times; what a check costs there is the host's row-by-row cursor walks and the oracle's scans, which grow with both.
N0 = 200 if EMU else 240
R, L_BUILD, NQ = 16, 32, 12
MAX_ROWS = 1000
COSINE, L2, IP = 0, 1, 2
INVALID, CAPACITY, STATE = -1, -4, -5
QUAL_SLOT = 3


def _rows(dim, distance, seed, n0):
    """the rows of the index and of every insert to come, in the order they are used: gauss, un-normalised; on cosine a zero row
    among the first rows and one in every 60 of the later ones (so in every insert of 65 rows or more)"""
    rows = make_vectors(MAX_ROWS, dim, 500 + seed, "gauss")
    rows[::3] *= 2.5
    if distance == COSINE:
        rows[7] = 0
        rows[n0 + 40::60] = 0
    return rows


def _queries(dim, seed, near):
    """NQ queries, the last four next to `near` (rows of a later insert)"""
    return np.concatenate([make_vectors(NQ - 4, dim, 900 + seed, "gauss"), near[:4] + np.float32(0.01) * make_vectors(4, dim, 901 + seed, "gauss")]).astype(np.float32)


class PlainChain:
    def __init__(self, ix, O, distance, vecs, tids, q, capacity, rows=None, used=0):
        self.ix, self.ctx, self.O, self.distance = ix, ix.ctx, O, distance
        self.vecs = np.ascontiguousarray(vecs, np.float32).copy()   # the vector column as it must stand
        self.tids = np.ascontiguousarray(tids, np.uint64).copy()
        self.q, self.capacity = q, capacity                         # capacity None: not the host's to know (a follower's index)
        self.rows, self.used = rows, used                           # the rows of the inserts to come
        self.tid_next = 10 ** 4
        self.own = None      # the mask set_visibility put in force, grown by ones
        self.snaps = {}      # {id: mask} of the stored snapshots, grown by zeros
        self.qual = None     # (slot, bits as they were put): rows added later read 0

    @classmethod
    def built(cls, gpu_ctx, O, *, dim, distance, dim_index=None, seed=0, n0=None):
        """an index made on the device: vs_index_alloc, the rows, vs_build_graph"""
        import pgvectorscale_amd as P
        n0 = n0 or N0
        rows = _rows(dim, distance, seed, n0)
        tids = make_tids(0, n0)
        ix = P.DiskAnnIndex.alloc(gpu_ctx, n=n0, dim_full=dim, dim_index=dim_index, num_neighbors=R, distance_type=distance,
                                  storage_type=P._lib.VS_STORAGE_PLAIN)
        vp, stride = ix.array(P._lib.ARR_VECS)
        Xp = np.zeros((n0, stride), np.float32)
        Xp[:, :dim] = rows[:n0]
        gpu_ctx.upload(vp, Xp)
        gpu_ctx.upload(ix.array(P._lib.ARR_TIDS)[0], tids)
        ix.refresh_norms()
        ix.build_graph(search_list_size=L_BUILD, max_alpha=1.2)
        return cls(ix, O, distance, rows[:n0], tids, _queries(dim, seed, rows[n0:]), n0, rows=rows, used=n0)

    @classmethod
    def uploaded(cls, gpu_ctx, O, *, dim, distance, seed=0, n0=None):
        """an index that mirrors a relation: a graph made elsewhere (plain_build_checks.sbq_graph), vs_index_upload"""
        import pgvectorscale_amd as P
        n0 = n0 or N0
        rows = _rows(dim, distance, seed, n0)
        tids = make_tids(0, n0)
        nbrs, start = PB.sbq_graph(O, np.array(rows[:n0]), R, L_BUILD)
        ix = P.DiskAnnIndex.upload(gpu_ctx, codes=None, nbrs=nbrs, heap_tids=tids, vecs=rows[:n0], mean=None, m2=None, count=0, bits=1,
                                   dim_index=dim, num_neighbors=R, distance_type=distance, default_start=start,
                                   storage_type=P._lib.VS_STORAGE_PLAIN)
        return cls(ix, O, distance, rows[:n0], tids, _queries(dim, seed, rows[n0:]), n0, rows=rows, used=n0)

    @property
    def n(self):
        return self.tids.size

    @property
    def live(self):
        return (self.tids & OFFSET) != 0

    def _appended(self, vecs, tids):
        """the host's account of k rows behind n: visible in the own mask, in no stored snapshot, in no qualifier"""
        k = len(tids)
        self.vecs = np.concatenate([self.vecs, np.ascontiguousarray(vecs, np.float32)])
        self.tids = np.concatenate([self.tids, np.ascontiguousarray(tids, np.uint64)])
        if self.own is not None:
            self.own = np.concatenate([self.own, np.ones(k, np.uint8)])
        self.snaps = {sid: np.concatenate([m, np.zeros(k, np.uint8)]) for sid, m in self.snaps.items()}

    def _grown(self, k):
        grew = int(self.n + k > self.capacity)
        if grew:  # the insert's rule: by half, at least to fit
            self.capacity = max(self.n + k, self.capacity + self.capacity // 2)
        return grew

    def insert(self, k):
        """-> stats; first_node, inserted and grew are held to the host's account"""
        assert self.used + k <= MAX_ROWS
        first, grew = self.n, self._grown(k)
        new, tids = self.rows[self.used:self.used + k], make_tids(self.tid_next, k)
        st = self.ix.insert(new, tids, search_list_size=L_BUILD, max_alpha=1.2)
        assert (st["first_node"], st["inserted"], st["grew"]) == (first, k, grew), st
        self.used += k
        self.tid_next += k
        self._appended(new, tids)
        assert self.ix.desc.n == self.n and self.ix.capacity == self.capacity
        return st

    def bulk_delete(self, nodes, seed=0):
        """ambulkdelete of the nodes' heap tids, handed over unsorted among tids no node has and duplicates"""
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

    def consolidate(self):
        st = self.ix.consolidate_deletes(plain=True)
        assert st["tombstones"] == int((~self.live).sum()) and st["unreachable_live"] == 0, st
        return st

    def compact(self, check_edges=True):
        """the host renumbers its account with the map the call returns — after holding the map to its own: every live node and the
        default start node stay, in order"""
        import pgvectorscale_amd as P
        keep = self.live.copy()
        keep[int(self.ix.desc.default_start)] = True
        want = np.where(keep, np.cumsum(keep) - 1, INV).astype(np.uint32)
        st, new_of = self.ix.compact(check_edges=check_edges, return_map=True)
        assert (new_of == want).all() and (st["n_before"], st["n_after"]) == (keep.size, int(keep.sum())), st
        assert not check_edges or st["edges_cut"] == 0, st
        self.vecs, self.tids = self.vecs[keep], self.tids[keep]
        if self.own is not None:
            self.own = self.own[keep]
        self.snaps = {sid: m[keep] for sid, m in self.snaps.items()}
        if self.qual is not None:  # include/vsgpu.h, qualified scans, LIFETIME: "vs_index_compact renumbers the nodes and DROPS every qualifier"
            with pytest.raises(P.VsError) as e:
                self.ix.qual_info(self.qual[0])
            assert e.value.code == STATE
            self.qual = None
        assert self.ix.desc.n == self.n and self.ix.capacity == self.capacity  # (the capacity stays as room for the next insert)
        return st

    def reserve(self, capacity):
        self.ix.reserve(capacity)
        self.capacity = max(self.capacity, capacity)
        assert self.ix.capacity == self.capacity

    def shrink(self):
        self.ix.shrink_to_fit()
        self.capacity = self.n
        assert self.ix.capacity == self.capacity and self.ix.desc.n == self.n

    def set_visibility(self, mask):
        self.own = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.ix.set_visibility(self.own)

    def snapshot_put(self, sid, mask):
        from pgvectorscale_amd import _lib
        mask = np.ascontiguousarray(mask, np.uint8)
        assert mask.shape == (self.n,)
        _lib.check(self.ix._L.vs_index_snapshot_put(self.ix.h, sid, mask.ctypes.data_as(C.c_void_p)))
        self.snaps[sid] = mask

    def qual_put(self, slot, bits):
        bits = np.ascontiguousarray(bits, bool)
        assert bits.shape == (self.n,)
        self.ix.qual_put(slot, bits)
        self.qual = (slot, bits)

    def check(self, where, pages=False):
        host, oidx = check_plain_everywhere(self.ix, self.O, self.distance, self.q, visible=self.own, snapshots=self.snaps, qualifier=self.qual,
                                            pages=pages, where=where)
        assert (host["heap_tids"] == self.tids).all(), where
        assert host["vecs"].tobytes() == self.vecs.tobytes(), where
        assert self.capacity is None or self.ix.capacity == self.capacity, where
        return host, oidx

    def bytes(self):
        h = self.ix.download(codes=False, vecs=True)
        return b"".join(h[k].tobytes() for k in ("nbrs", "heap_tids", "vecs")), self.ix.desc.n, self.ix.desc.default_start, self.ix.capacity

    def refused(self, code, word, call):
        """a refusal leaves every byte as it was"""
        import pgvectorscale_amd as P
        before = self.bytes()
        with pytest.raises(P.VsError) as e:
            call()
        assert e.value.code == code and word in str(e.value), str(e.value)
        assert self.bytes() == before, "a refused call wrote"

    def close(self):
        self.ix.close()


def _pointers(ix):
    from pgvectorscale_amd import _lib
    return [ix.array(a)[0].value for a in (_lib.ARR_NBRS, _lib.ARR_TIDS, _lib.ARR_VECS)]


# ---- chain A: a device-made index through reserve, growth, vacuum, compaction, shrink and growth again --------------------------------
# cosine 24 of 40: divisors of the index slices next to those of the rows, a rescore window, a scalar tail of 8 in the rerank
GEOM_A = {"l2_dim48": dict(dim=48, distance=L2), "cosine_slice_24_of_40": dict(dim=40, dim_index=24, distance=COSINE)}


@gpu
@pytest.mark.parametrize("geom", list(GEOM_A))
def test_chain_a_reserve_grow_vacuum_compact_shrink_grow(gpu_ctx, oracle, geom):
    ch = PlainChain.built(gpu_ctx, oracle, seed=1, **GEOM_A[geom])
    try:
        rng = np.random.default_rng(2)
        ch.check("built")                                                      # 1
        ch.set_visibility((rng.random(ch.n) > 0.2).astype(np.uint8))           # 2
        ch.snapshot_put(1, (rng.random(ch.n) > 0.3).astype(np.uint8))
        ch.qual_put(QUAL_SLOT, rng.random(ch.n) < 0.4)
        ch.check("mask, snapshot, qualifier")
        ch.reserve(ch.n + 40)                                                  # 3: fits after the reserve
        assert ch.insert(40)["grew"] == 0
        ch.check("insert 40 into reserved room")
        before = _pointers(ch.ix)
        assert ch.insert(160)["grew"] == 1                                     # 4: the arrays move
        assert all(a != b for a, b in zip(before, _pointers(ch.ix)))
        ch.check("insert 160")
        ch.bulk_delete(np.flatnonzero(rng.random(ch.n) < 0.3), seed=3)         # 5
        # a compaction that is refused (kept rows still name the tombstones) changes nothing, the qualifier included
        ch.refused(STATE, "name a dropped node", lambda: ch.ix.compact(check_edges=True))
        ch.check("bulk delete 30 %")
        assert ch.consolidate()["rows_rewritten"] >= 1                         # 6
        ch.check("consolidate")
        n_before = ch.n
        st = ch.compact()                                                      # 7: cuts no edge, drops the qualifier
        assert st["edges_cut"] == 0 and ch.n < n_before and ch.qual is None
        ch.check("compact", pages=True)
        ch.qual_put(QUAL_SLOT, rng.random(ch.n) < 0.4)                         # 8
        ch.check("qualifier over the new numbering")
        assert ch.capacity - ch.n >= 100
        assert ch.insert(100)["grew"] == 0                                     # 9: into the freed room
        ch.check("insert into the freed room")
        before = _pointers(ch.ix)
        ch.shrink()                                                            # 10
        assert all(a != b for a, b in zip(before, _pointers(ch.ix)))
        ch.check("shrink_to_fit")
        assert ch.insert(65)["grew"] == 1                                      # 11: just over one wave, past the shrunk capacity
        ch.check("insert 65", pages=True)
    finally:
        ch.close()


# ---- chain B: an uploaded inner-product index — the only way the inner product meets a mutation -----------------------------------------
@gpu
def test_chain_b_uploaded_inner_product_delete_compact_shrink(gpu_ctx, oracle):
    """vs_build_graph refuses the inner product on plain storage, so such an index is always uploaded; what it is documented not to
    take is asserted as a refusal that leaves every byte as it was:
      - vs_index_insert (include/vsgpu.h: "VS_ERR_INVALID, the index left byte for byte as it was, for a plain index whose distance is
        the inner product (see vs_build_graph) ... or that came from vs_index_upload");
      - vs_index_consolidate_deletes_plain ("Refusals leave every byte as it was: VS_ERR_INVALID for ... an index the pair distance
        cannot score (the inner-product distance ...").
    So the tombstones leave through a compaction that cuts the edges naming them, which every entry point must survive too."""
    ch = PlainChain.uploaded(gpu_ctx, oracle, dim=48, distance=IP, seed=2)
    try:
        rng = np.random.default_rng(4)
        ch.qual_put(QUAL_SLOT, rng.random(ch.n) < 0.4)
        ch.check("uploaded")
        new = ch.rows[ch.used:ch.used + 40]
        ch.refused(INVALID, "vs_index_insert", lambda: ch.ix.insert(new, make_tids(ch.tid_next, 40), search_list_size=L_BUILD))
        ch.bulk_delete(np.flatnonzero(rng.random(ch.n) < 0.3), seed=5)
        ch.check("bulk delete 30 %")
        ch.refused(INVALID, "inner-product", lambda: ch.ix.consolidate_deletes(plain=True))
        ch.refused(STATE, "name a dropped node", lambda: ch.ix.compact(check_edges=True))
        ch.check("refused consolidation and compaction")
        n_before = ch.n
        st = ch.compact(check_edges=False)
        assert st["edges_cut"] > 0 and ch.n < n_before and ch.qual is None
        ch.check("compact")
        ch.shrink()
        ch.check("shrink_to_fit")
        ch.refused(INVALID, "vs_index_insert", lambda: ch.ix.insert(new, make_tids(ch.tid_next, 40), search_list_size=L_BUILD))
    finally:
        ch.close()


# ---- chain C: the follower ----------------------------------------------------------------------------------------------------------------
# cosine with every dimension indexed: apply(None) takes the appended rows' vectors from the pages (the normalised node vectors)
GEOM_C = {"l2_dim48": dict(dim=48, distance=L2, from_pages=False), "cosine_dim40_vectors_from_the_pages": dict(dim=40, distance=COSINE, from_pages=True)}


@gpu
@pytest.mark.parametrize("geom", list(GEOM_C))
def test_chain_c_a_followed_relation(gpu_ctx, oracle, geom):
    """a relation written by the oracle's plain writer, staged and followed through two rounds of changed blocks made with the same
    writer: one that only rewrites neighbor lists and clears tids, one that appends rows past the capacity"""
    from pgvectorscale_amd.pages import IndexPages
    g = GEOM_C[geom]
    n0 = N0 - 60
    m, relinked, cleared = 90, 40, 25
    fam = FC.Family(dim=g["dim"], R=R, distance=g["distance"], n_max=n0 + m, seed=71, zero_row=5 if g["distance"] == COSINE else None)
    # The starting graph: the oracle's builder over codes of the NORMALISED rows.  (Family.s0 quantizes the rows as they are, scaled
    # by 0.2 .. 3, and at this size its graph reaches 17 nodes from the start node: no scan would outgrow a capacity, which the
    # hand-over precondition of the checker refuses.)
    X = fam.vecs[:n0].copy()
    norm = np.linalg.norm(X, axis=1, keepdims=True)
    norm[norm == 0] = 1
    nbrs, start = PB.sbq_graph(oracle, (X / norm).astype(np.float32), R, L_BUILD)
    assert nbrs.shape == (n0, R) and PB.reach(nbrs, start).sum() > 0.9 * n0
    s0 = FC.State(np.ascontiguousarray(nbrs, np.uint32), fam.tids[:n0].copy(), X, fam.nodevecs[:n0].copy(), int(start))
    s1 = fam.mutate(s0, 0, relinked, cleared, seed=72)
    s2 = fam.mutate(s1, m, 0, 0, seed=73)
    r0, r1, r2 = (fam.relation(s)[0] for s in (s0, s1, s2))
    rd = IndexPages(plain=True)
    rd.add(r0)
    assert rd.finish().n_nodes == n0
    ix = rd.upload_plain(gpu_ctx, distance_type=fam.distance, default_start=s0.start, vecs=s0.vecs)
    fol = rd.follower(ix)
    rd.close()
    ch = PlainChain(ix, oracle, fam.distance, s0.vecs, s0.tids, _queries(g["dim"], 7, fam.vecs[n0:]), n0)
    try:
        rng = np.random.default_rng(6)
        ch.set_visibility((rng.random(ch.n) > 0.2).astype(np.uint8))
        ch.snapshot_put(1, (rng.random(ch.n) > 0.3).astype(np.uint8))
        ch.qual_put(QUAL_SLOT, rng.random(ch.n) < 0.4)
        ch.check("staged", pages=True)
        # round 1: lists and tids only
        assert len(r1) == len(r0)
        blocks = FC.dirty(r0, r1)
        info = fol.stage(blocks, FC.gather(r1, blocks), len(r1) // FC.B)
        assert info["n_appended"] == 0 and info["rows_relinked"] > 0 and info["tids_cleared"] == cleared and info["codes_changed"] == 0
        fol.apply(None)
        ch.tids = s1.tids.copy()
        host, _ = ch.check("followed: relinked rows, cleared tids", pages=True)
        assert (host["nbrs"] == s1.nbrs).all()
        # round 2: rows appended past the capacity
        blocks = FC.dirty(r1, r2)
        info = fol.stage(blocks, FC.gather(r2, blocks), len(r2) // FC.B)
        assert info["n_appended"] == m and info["codes_changed"] == 0
        assert (fol.new_tids() == s2.tids[n0:]).all()
        before = _pointers(ix)
        fol.apply(None if g["from_pages"] else s2.vecs[n0:])
        assert all(a != b for a, b in zip(before, _pointers(ix)))
        new = s2.nodevecs[n0:] if g["from_pages"] else s2.vecs[n0:]
        if g["from_pages"]:
            assert (new != s2.vecs[n0:]).any()  # (the pages hold the normalised rows: not what the heap holds)
        ch._grown(m)
        ch._appended(new, s2.tids[n0:])
        host, _ = ch.check("followed: appended rows", pages=not g["from_pages"])
        assert (host["nbrs"] == s2.nbrs).all()
        if not g["from_pages"]:
            assert ix.write_pages(plain=True) == r2
    finally:
        fol.close()
        ch.close()


# ---- chain D: drawn chains --------------------------------------------------------------------------------------------------------------------
KINDS = ("insert_small", "insert_growing", "bulk_delete", "consolidate", "compact", "reserve", "shrink_to_fit", "set_visibility", "qual_put")
GEOM_D = (dict(dim=48, distance=L2), dict(dim=40, dim_index=24, distance=COSINE), dict(dim=40, dim_index=24, distance=L2),
          dict(dim=36, distance=COSINE))
SEEDS = (1, 2, 3, 4, 5, 6)
N_OPS = 8


def draw_chain(seed):
    """-> (geometry, [operation, ...]): eight operations, every argument drawn here, all legal in the state the ones before leave.
    Impossible draws are drawn again: a compaction while rows may still name tombstones (deletes since the last consolidation: it
    runs with VS_COMPACT_KEEP_EDGES_CHECK and would be refused), an insert past MAX_ROWS rows used, a delete that names nothing or
    leaves fewer than 100 live rows.  Node 0, the default start node of a device build, is never deleted, so that a compaction keeps
    exactly the live rows and the sizes are known here."""
    rng = np.random.default_rng(seed)
    geom = GEOM_D[int(rng.integers(len(GEOM_D)))]
    n = cap = used = N0
    live = np.ones(n, bool)
    unconsolidated = False
    ops = []
    while len(ops) < N_OPS:
        kind = KINDS[int(rng.integers(len(KINDS)))]
        if kind in ("insert_small", "insert_growing"):
            k = int(rng.choice([1, 40, 64])) if kind == "insert_small" else max(cap - n, 0) + int(rng.choice([1, 65, 130]))
            if used + k > MAX_ROWS:
                continue
            grew = n + k > cap
            if grew:
                cap = max(n + k, cap + cap // 2)
            n, used = n + k, used + k
            live = np.concatenate([live, np.ones(k, bool)])
            ops.append(dict(kind=kind, k=k, grew=grew))
        elif kind == "bulk_delete":
            alive = np.flatnonzero(live)[1:]
            nodes = alive[rng.random(alive.size) < float(rng.choice([0.05, 0.2, 0.4]))]
            if alive.size - nodes.size < 100 or nodes.size == 0:
                continue
            live[nodes] = False
            unconsolidated = True
            ops.append(dict(kind=kind, nodes=np.sort(nodes)))
        elif kind == "consolidate":
            unconsolidated = False
            ops.append(dict(kind=kind, tombstones=int((~live).sum())))
        elif kind == "compact":
            if unconsolidated:
                continue
            n = int(live.sum())
            live = np.ones(n, bool)
            ops.append(dict(kind=kind, n_after=n))
        elif kind == "reserve":
            c = int(rng.choice([n // 2, n + 1, n + 200, 2 * n]))
            ops.append(dict(kind=kind, capacity=c, moves=c > cap))
            cap = max(cap, c)
        elif kind == "shrink_to_fit":
            ops.append(dict(kind=kind, moves=cap != n))
            cap = n
        else:
            ops.append(dict(kind=kind, seed=int(rng.integers(1 << 30)), clear=bool(kind == "set_visibility" and rng.random() < 0.3)))
    return geom, ops


def test_the_drawn_chains_cover_every_operation():
    """(no device needed) what the six seeds draw between them"""
    count = dict.fromkeys(KINDS, 0)
    geoms = set()
    grew = 0
    for seed in SEEDS:
        geom, ops = draw_chain(seed)
        assert len(ops) == N_OPS
        geoms.add(tuple(sorted(geom.items())))
        for op in ops:
            count[op["kind"]] += 1
            grew += op.get("grew", False)
    assert all(v >= 1 for v in count.values()), count
    assert len(geoms) >= 2 and grew >= 1, (geoms, grew)


def _run_drawn(ch, op, seed):
    kind = op["kind"]
    if kind in ("insert_small", "insert_growing"):
        assert ch.insert(op["k"])["grew"] == int(op["grew"])
    elif kind == "bulk_delete":
        assert int(ch.ix.desc.default_start) == 0
        ch.bulk_delete(op["nodes"], seed=seed)
    elif kind == "consolidate":
        assert ch.consolidate()["tombstones"] == op["tombstones"]
    elif kind == "compact":
        ch.compact()
        assert ch.n == op["n_after"]
    elif kind == "reserve":
        before = _pointers(ch.ix)
        ch.reserve(op["capacity"])
        assert all(a != b for a, b in zip(before, _pointers(ch.ix))) == op["moves"]
    elif kind == "shrink_to_fit":
        ch.shrink()
    elif kind == "set_visibility":
        ch.set_visibility(None if op["clear"] else (np.random.default_rng(op["seed"]).random(ch.n) > 0.3).astype(np.uint8))
    else:
        ch.qual_put(QUAL_SLOT, np.random.default_rng(op["seed"]).random(ch.n) < 0.4)


@gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_chain_d_drawn_operations(gpu_ctx, oracle, seed):
    geom, ops = draw_chain(seed)
    ch = PlainChain.built(gpu_ctx, oracle, seed=10 + seed, **geom)
    try:
        ch.check((seed, "built"))
        for step, op in enumerate(ops):
            _run_drawn(ch, op, seed * 10 + step)
            ch.check((seed, step, op["kind"]), pages=step == len(ops) - 1)
    finally:
        ch.close()


# ---- chain E: a cursor and a pool that live across an insert ------------------------------------------------------------------------------
@gpu
def test_chain_e_a_cursor_is_rescanned_and_a_plain_pool_recreated_after_a_growth(gpu_ctx, oracle):
    """include/vsgpu.h: after an insert "open vs_scans, scan pools ... of the index must be ended or rescanned" — so a rescan on the
    old descriptor must hand out the grown index's rows; and of a plain pool: "The plain form clamps its capacities to the n of the
    pool's creation: after vs_index_insert has grown a plain index, free the pool and create it again (one that is kept and
    rescanned may fail scans the grown index makes longer with VS_ERR_CAPACITY)" — so a pool that is kept may fail a scan with that
    code and with no other, and hands out no wrong row; one created again hands out the oracle's rows."""
    import pgvectorscale_amd as P
    ch = PlainChain.built(gpu_ctx, oracle, dim=48, distance=L2, seed=3)
    ix, q = ch.ix, ch.q
    L, rescore, k = CURSOR["L"], CURSOR["rescore"], POOL["k"]
    near = q[NQ - 4:]  # queries next to the first inserted rows
    scan = ix.beginscan()
    pool = P.ScanPool(ix, 2, search_list_size=L, rescore=rescore, kmax=k, rows_cap=POOL["rows_cap"])
    try:
        assert pool.info()["kernel"] == FAST_PLAIN
        n0 = ch.n
        _, oidx = ch.check("before the insert")
        scan.rescan(near[0], search_list_size=L, rescore=rescore)
        pull_and_compare(scan, oidx.scan(near[0], L=L, rescore=rescore), rows=20, where="cursor before", keys=PLAIN_CURSOR_KEYS)
        for slot in (0, 1):
            pool.rescan(slot, near[slot + 1])
            check_pool_slot(pool, slot, oidx.scan(near[slot + 1], L=L, rescore=rescore), k, 1, ("pool before", slot), keys=PLAIN_CURSOR_KEYS)
        assert ch.insert(300)["grew"] == 1  # the arrays move under the open cursor and pool
        _, oidx = ch.check("after the insert")
        # the cursor, rescanned on its old descriptor
        scan.rescan(near[0], search_list_size=L, rescore=rescore)
        peek = oidx.scan(near[0], L=L, rescore=rescore)
        assert any(peek.gettuple()[0] >= n0 for _ in range(20)), "the scan must come by inserted rows among its first"
        pull_and_compare(scan, oidx.scan(near[0], L=L, rescore=rescore), where="cursor rescanned", keys=PLAIN_CURSOR_KEYS)
        # the pool that was kept: rescanned, a slot hands out the oracle's rows or fails with VS_ERR_CAPACITY — never a wrong row
        for slot in (0, 1):
            pool.rescan(slot, near[slot + 1])
            oscan = oidx.scan(near[slot + 1], L=L, rescore=rescore)
            for _ in range(3):
                rows, ids, tids, dist = pool.fetch([slot], k)
                if rows[0] < 0:
                    assert rows[0] == CAPACITY, rows[0]
                    break
                for j in range(int(rows[0])):
                    o = oscan.gettuple()
                    assert o is not None and ids[0][j] == o[0] and tids[0][j] == o[1], ("pool kept", slot, j)
                    assert np.float32(dist[0][j]).view(np.uint32) == np.float32(o[2]).view(np.uint32)
        pool.close()
        # ... and created again
        pool = P.ScanPool(ix, 2, search_list_size=L, rescore=rescore, kmax=k, rows_cap=POOL["rows_cap"])
        assert pool.info()["kernel"] == FAST_PLAIN
        for slot in (0, 1):
            pool.rescan(slot, near[slot + 1])
        for slot in (0, 1):
            check_pool_slot(pool, slot, oidx.scan(near[slot + 1], L=L, rescore=rescore), k, 3, ("pool recreated", slot), keys=PLAIN_CURSOR_KEYS)
    finally:
        pool.close()
        scan.endscan()
        ch.close()
