"""vs_index_label_reach / vs_index_repair_labels / vs_nearest_masked: which rows a single-label scan cannot
reach, and the in-edges that mend it.  The reference is `_audit` / `_twin`, a numpy restatement of the definitions and of steps 1-5
written here; the oracle's exhaustive filtered stream is the second witness of the audit.  Also runs on the lockstep interpreter
(tests/test_emu_label_repair.py).

Conventions of the restatement (vsgpu.h states the same): a label that is carried but has no start node is not judged and has no
bit in mask / reach / need; `rounds` counts the rounds that found something lost; `rows_changed` counts distinct rows written; the source kernel takes
the lost nodes in tiles of 8, or of 4 when at most 4 are lost (`source_tiles`)."""
import functools
import os

import numpy as np
import pytest

from helpers import TestIndex

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF
STATE, INVALID = -5, -1
EMU = bool(os.environ.get("VS_EMU"))
U64 = np.uint64
COUNTERS = ("lost_pairs_before", "lost_pairs_after", "lost_nodes_before", "lost_nodes_after", "placed_free", "placed_over_dropped",
            "placed_victim", "blocked", "contended", "rows_changed", "source_tiles", "rounds", "labels_without_start", "unreachable_live")


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
class _Graph:
    """the arrays a call sees: node classes, the judged labels in groups of 64, their masks"""

    def __init__(self, nbrs, tids, default_start, label_starts, sets):
        n = len(tids)
        self.n, self.R = n, nbrs.shape[1]
        dead = (tids & U64(0xFFFF)) == 0
        kept = np.zeros(n, bool)
        kept[[default_start] + list(label_starts.values())] = True
        self.live, self.D = ~dead, dead & ~kept
        self.default_start = default_start
        carried = set(l for s in sets for l in s)
        self.labels = sorted(carried | set(label_starts))
        self.without_start = len(carried - set(label_starts))
        self.groups = []
        for g0 in range(0, len(self.labels), 64):
            grp = self.labels[g0:g0 + 64]
            bit = {l: t for t, l in enumerate(grp)}
            judged = [l for l in grp if l in carried and l in label_starts]
            mask = np.zeros(n, U64)       # the judged labels of the group a node carries
            full = np.zeros(n, U64)       # every label of the group it carries (the carrier counts)
            for i, s in enumerate(sets):
                for l in s:
                    if l in bit:
                        full[i] |= U64(1 << bit[l])
                        if l in judged:
                            mask[i] |= U64(1 << bit[l])
            seeds = {}
            for l in judged:
                seeds[label_starts[l]] = seeds.get(label_starts[l], 0) | (1 << bit[l])
            self.groups.append((grp, bit, mask, full, seeds))

    def reach(self, nbrs, g):
        _, _, mask, _, seeds = self.groups[g]
        u = np.repeat(np.arange(self.n), self.R)
        v = nbrs.ravel().astype(np.int64)
        ok = v != INV
        u, v = u[ok], v[ok]
        reach = np.zeros(self.n, U64)
        for s, b in seeds.items():
            reach[s] |= U64(b)
        while True:
            new = reach.copy()
            np.bitwise_or.at(new, v, reach[u] & mask[v])
            if (new == reach).all():
                return reach
            reach = new

    def need(self, reach, g):
        return np.where(self.live, self.groups[g][2] & ~reach, U64(0))


def _audit(G, nbrs):
    """-> (pairs, node_lost bool [n], {label: (live carriers, lost)}, {label: reached node set})"""
    per, node_lost, reached = {}, np.zeros(G.n, bool), {}
    for g, (grp, bit, mask, full, _) in enumerate(G.groups):
        reach = G.reach(nbrs, g)
        need = G.need(reach, g)
        node_lost |= need != 0
        for l in grp:
            b = U64(1 << bit[l])
            per[l] = (int(((full & b) != 0)[G.live].sum()), int(((need & b) != 0).sum()))
            reached[l] = set(np.flatnonzero((reach & b) != 0).tolist())
    return sum(v[1] for v in per.values()), node_lost, per, reached


def _unreachable_live(G, nbrs):
    seen = np.zeros(G.n, bool)
    seen[G.default_start] = True
    front = [G.default_start]
    while front:
        nxt = nbrs[front].ravel()
        nxt = np.unique(nxt[nxt != INV])
        nxt = nxt[~seen[nxt]]
        seen[nxt] = True
        front = nxt.tolist()
    return int((G.live & ~seen).sum())


def _nearest(codes, x, adm):
    ids = np.flatnonzero(adm)
    if ids.size == 0:
        return None
    ham = np.bitwise_count(codes[ids] ^ codes[x]).sum(axis=1).astype(np.uint64)
    key = (ham << U64(32)) | ids.astype(np.uint64)
    k = int(key.min())
    return k & 0xFFFFFFFF, k >> 32


def _twin(codes, nbrs, tids, default_start, label_starts, sets, max_rounds=16):
    nbrs = nbrs.copy()
    G = _Graph(nbrs, tids, default_start, label_starts, sets)
    st = dict.fromkeys(COUNTERS, 0)
    st["labels_without_start"] = G.without_start
    pairs, nl, _, _ = _audit(G, nbrs)
    st["lost_pairs_before"] = st["lost_pairs_after"] = pairs
    st["lost_nodes_before"] = st["lost_nodes_after"] = int(nl.sum())
    changed = set()
    R = G.R
    for _ in range(max_rounds if pairs else 0):
        any_lost = False
        for g, (_, _, mask, _, _) in enumerate(G.groups):
            reach = G.reach(nbrs, g)                                                   # step 1
            need = G.need(reach, g)
            lost = np.flatnonzero(need != 0)
            if lost.size == 0:
                continue
            any_lost = True
            st["source_tiles"] += (int(lost.size) + 3) // 4 if lost.size <= 4 else (int(lost.size) + 7) // 8
            q = np.repeat(np.arange(G.n), R)                                           # step 2
            y = nbrs.ravel().astype(np.int64)
            ok = (y != INV) & ~G.D[q]
            q, y = q[ok], y[ok]
            strong = np.bincount(y[(mask[y] & ~reach[q]) == 0], minlength=G.n)
            claim = {}
            for x in lost:                                                             # steps 3 and 4 (ascending x: the smallest wins)
                adm = ~G.D & ((reach & need[x]) != 0)
                adm[x] = False
                p, _ = _nearest(codes, x, adm)
                claim.setdefault(p, int(x))
            st["contended"] += int(lost.size) - len(claim)
            for p, x in claim.items():                                                 # step 5
                row = nbrs[p]
                free = np.flatnonzero(row == INV)
                ln = int(free[0]) if free.size else R
                if x in row[:ln]:
                    continue
                slot, kind = None, None
                if ln < R:
                    slot, kind = ln, "placed_free"
                else:
                    for t in range(R - 1, -1, -1):
                        if G.D[row[t]]:
                            slot, kind = t, "placed_over_dropped"
                            break
                    if slot is None:
                        for t in range(R - 1, -1, -1):
                            yy = int(row[t])
                            if strong[yy] >= 1 + int((mask[yy] & ~reach[p]) == 0):
                                slot, kind = t, "placed_victim"
                                break
                if slot is None:
                    st["blocked"] += 1
                    continue
                row[slot] = x
                st[kind] += 1
                changed.add(p)
        if not any_lost:
            break
        st["rounds"] += 1
    if st["rounds"]:
        pairs, nl, _, _ = _audit(G, nbrs)
        st["lost_pairs_after"], st["lost_nodes_after"] = pairs, int(nl.sum())
    st["rows_changed"] = len(changed)
    st["unreachable_live"] = _unreachable_live(G, nbrs)
    return nbrs, st, G


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ti(labels):
    from oracle import oracle_py as O
    kw = dict(n_labels=32, label_zipf=True) if labels == "zipf32" else dict(n_labels=8)
    return TestIndex(n=1400, dim_full=64, bits=2, R=24, distance=O.L2, seed=19, kind="gauss", L_build=50, **kw)


@functools.lru_cache(maxsize=None)
def _graph(labels, graph):
    """-> (ti, nbrs, default start, {label: start node})"""
    from oracle import oracle_py as O
    ti = _ti(labels)
    if graph == "plain":
        return ti, ti.nbrs, int(ti.start), dict(ti.label_starts)
    nbrs, start, ls = O.build_graph_labeled(ti.codes, ti.label_off, ti.label_val, num_neighbors=ti.R, search_list_size=50)
    return ti, nbrs, start, ls


def _sets(ti):
    return [set(int(v) for v in ti.label_val[ti.label_off[i]:ti.label_off[i + 1]]) for i in range(ti.n)]


def _upload(ctx, ti, nbrs, start, ls):
    import pgvectorscale_amd as P
    return P.DiskAnnIndex.upload(ctx, codes=ti.codes, nbrs=nbrs, heap_tids=ti.tids, vecs=ti.vecs, mean=ti.mean, m2=ti.m2, count=ti.count,
                                 bits=ti.bits, dim_index=ti.dim_index, num_neighbors=ti.R, distance_type=ti.distance, default_start=start,
                                 label_off=ti.label_off, label_val=ti.label_val, label_starts=ls)


def _oracle_index(O, ti, host, start, ls):
    return O.OracleIndex(codes=host["codes"], nbrs=host["nbrs"], heap_tids=host["heap_tids"], vecs=ti.vecs, mean=ti.mean, m2=ti.m2,
                         count=ti.count, bits=ti.bits, dim_index=ti.dim_index, num_neighbors=ti.R, distance_type=ti.distance,
                         default_start=start, label_off=ti.label_off, label_val=ti.label_val, label_starts=ls)


def _dead_nodes(ti, frac, seed, must=(), never=()):
    rng = np.random.default_rng(seed)
    pick = rng.random(ti.n) < frac
    pick[list(must)] = True
    pick[list(never)] = False
    return np.flatnonzero(pick)


def _check_audit(got, G, nbrs):
    pairs, node_lost, per, reached = _audit(G, nbrs)
    print("audit: lost pairs", pairs, "lost nodes", int(node_lost.sum()), "labels", len(per), "sweeps", got["sweeps"])
    assert got["per_label"] == per
    assert (got["lost_pairs"], got["lost_nodes"], got["labels"], got["labels_without_start"]) == \
        (pairs, int(node_lost.sum()), len(G.labels), G.without_start)
    assert (got["node_lost"] != 0).tolist() == node_lost.tolist()
    return pairs, node_lost, per, reached


def _check_repair(before, after, got, want_nbrs, wst, G):
    print("restatement:", wst)
    assert after["codes"].tobytes() == before["codes"].tobytes() and after["heap_tids"].tobytes() == before["heap_tids"].tobytes()
    bad = np.flatnonzero((after["nbrs"] != want_nbrs).any(1))
    assert bad.size == 0, (bad[:8], after["nbrs"][bad[:1]], want_nbrs[bad[:1]])
    assert {k: got[k] for k in COUNTERS} == wst
    # what the restatement met with the default 16 rounds on these inputs
    assert got["lost_pairs_after"] == 0 and got["lost_nodes_after"] == 0 and got["blocked"] == 0 and got["unreachable_live"] == 0
    named = after["nbrs"][~G.D]
    named = named[named != INV]
    assert not G.D[named].any()  # no kept row names a dropped tombstone
    assert after["nbrs"][G.D].tobytes() == before["nbrs"][G.D].tobytes()  # rows of D are never written


CASES = [("zipf32", "labeled"), ("zipf32", "plain"), ("uni8", "labeled"), ("uni8", "plain")]


# ---- case 1: the audit --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels,graph", CASES)
def test_audit_equals_the_restatement_and_the_oracles_filtered_streams(gpu_ctx, oracle, labels, graph):
    ti, nbrs, start, ls = _graph(labels, graph)
    ix = _upload(gpu_ctx, ti, nbrs, start, ls)
    before = ix.download()
    G = _Graph(nbrs, ti.tids, start, ls, _sets(ti))
    got = ix.label_reach(per_node=True)
    pairs, node_lost, per, reached = _check_audit(got, G, nbrs)
    assert pairs > 0, "the defect must show on this input"
    assert ix.download()["nbrs"].tobytes() == before["nbrs"].tobytes()
    # the exhaustive filtered stream of the oracle returns, per label, exactly the carriers the sweep calls reached
    oidx = _oracle_index(oracle, ti, before, start, ls)
    keys = [[l] for l in G.labels]
    ids, _, _ = oidx.stream_batch(ti.queries(len(keys), seed=5, kind="gauss"), L=2, m=ti.n, qlabels=keys)
    sets = _sets(ti)
    for l, row in zip(G.labels, ids):
        seen = set(row[row != INV].tolist())
        assert seen == set(i for i in reached[l] if l in sets[i]), l
        assert len(seen) == got["per_label"][l][0] - got["per_label"][l][1]
    ix.close()


# ---- case 2: the repair, cell for cell ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels,graph", CASES)
def test_repair_equals_the_restatement_cell_for_cell(gpu_ctx, oracle, labels, graph):
    ti, nbrs, start, ls = _graph(labels, graph)
    ix = _upload(gpu_ctx, ti, nbrs, start, ls)
    before = ix.download()
    want, wst, G = _twin(before["codes"], before["nbrs"], before["heap_tids"], start, ls, _sets(ti))
    got = ix.repair_labels()
    assert wst["lost_pairs_before"] > 0 and wst["rounds"] >= 1
    _check_repair(before, ix.download(), got, want, wst, G)
    ix.close()


@pytest.mark.parametrize("labels", ["zipf32", "uni8"])
def test_repair_after_delete_and_consolidate_equals_the_restatement(gpu_ctx, oracle, labels):
    ti, nbrs, start, ls = _graph(labels, "labeled")
    ix = _upload(gpu_ctx, ti, nbrs, start, ls)
    lstart = next(v for v in ls.values() if v != start)
    dead = _dead_nodes(ti, 0.3, 9, must=[lstart], never=[start])
    ix.bulk_delete(ti.tids[dead])
    assert ix.consolidate_deletes()["unreachable_live"] == 0
    before = ix.download()
    G0 = _Graph(before["nbrs"], before["heap_tids"], start, ls, _sets(ti))
    _check_audit(ix.label_reach(per_node=True), G0, before["nbrs"])
    want, wst, G = _twin(before["codes"], before["nbrs"], before["heap_tids"], start, ls, _sets(ti))
    assert wst["lost_pairs_before"] > 0 and G.D.sum() > 300 and not G.D[lstart]
    got = ix.repair_labels()
    after = ix.download()
    _check_repair(before, after, got, want, wst, G)
    ix.close()


# ---- case 3: what a user sees --------------------------------------------------------------------------------------------------------
def _pull(ix, q, label):
    scan = ix.beginscan()
    scan.rescan(q, labels=[label], search_list_size=2, rescore=4)
    rows = []
    while True:
        r = scan.gettuple()
        if r is None:
            break
        rows.append(r[1])
    scan.endscan()
    return rows


def test_filtered_cursors_return_every_carrier_after_the_repair(gpu_ctx, oracle):
    ti, nbrs, start, ls = _graph("zipf32", "labeled")
    ix = _upload(gpu_ctx, ti, nbrs, start, ls)
    sets = _sets(ti)
    carriers = {l: set(i for i in range(ti.n) if l in sets[i]) for l in ls}
    per = ix.label_reach()["per_label"]
    rare = max(per, key=lambda l: (per[l][1] / max(per[l][0], 1), l))  # the label that loses the largest share of its carriers
    q = ti.queries(1, seed=6, kind="gauss")[0]
    rows = _pull(ix, q, rare)
    print("label", rare, "carriers", per[rare][0], "lost", per[rare][1], "rows before", len(rows))
    assert per[rare][1] > 0 and set(rows) < carriers[rare] and len(rows) == per[rare][0] - per[rare][1]
    st = ix.repair_labels()
    assert st["lost_pairs_after"] == 0
    for l in sorted(ls):
        rows = _pull(ix, q, l)
        assert len(rows) == len(set(rows)) and set(rows) == carriers[l], l
    host = ix.download()
    oidx = _oracle_index(oracle, ti, host, start, ls)
    qs = ti.queries(32, seed=7, kind="gauss")
    order = sorted(ls)
    keys = [[order[i % len(order)]] if i % 2 == 0 else sorted({order[i % len(order)], order[(7 * i + 3) % len(order)]}) for i in range(32)]
    gi, _, gd, gst = ix.search_batch(qs, search_list_size=40, rescore=20, k=10, qlabels=keys)
    oi, od, ost = oidx.search_batch(qs, L=40, rescore=20, k=10, qlabels=keys)
    assert (gi == oi).all() and (gd.view(np.uint32) == od.view(np.uint32)).all() and gst["visited_nodes"] == ost["visited_nodes"]
    ix.close()


# ---- case 4: more than 64 distinct labels --------------------------------------------------------------------------------------------
def test_seventy_labels_two_groups_and_a_label_without_a_start_node(gpu_ctx, oracle):
    """the label-aware graph (R = 24, L = 50) as in case 1.  (The plain graph of this index, which knows nothing of its 70 labels, is
    beyond 16 rounds: the restatement leaves 18 of its 1035 lost pairs at R = 24 and 67 of 1060 at R = 16, with rows blocked.)"""
    ti = TestIndex(n=600, dim_full=64, bits=2, R=24, distance=oracle.L2, seed=23, kind="gauss", L_build=50, n_labels=70)
    sets = _sets(ti)
    assert len(set(l for s in sets for l in s)) == 70
    nbrs, start, ls = oracle.build_graph_labeled(ti.codes, ti.label_off, ti.label_val, num_neighbors=ti.R, search_list_size=50)
    built = dict(ls)
    orphan = 37
    del ls[orphan]          # carried by rows, absent from the start map: not judged, left alone
    ls[99] = 5              # a key of the start map nobody carries: a label of the second group without carriers
    ix = _upload(gpu_ctx, ti, nbrs, start, built)
    ix.set_start_nodes(start, ls)  # by hand
    before = ix.download()
    G = _Graph(before["nbrs"], before["heap_tids"], start, ls, sets)
    assert len(G.groups) == 2 and G.without_start == 1
    got = ix.label_reach(per_node=True)
    pairs, _, per, _ = _check_audit(got, G, before["nbrs"])
    assert pairs > 0 and per[orphan][1] == 0 and per[orphan][0] > 0 and per[99] == (0, 0)
    want, wst, G = _twin(before["codes"], before["nbrs"], before["heap_tids"], start, ls, sets)
    st = ix.repair_labels()
    _check_repair(before, ix.download(), st, want, wst, G)
    assert st["labels_without_start"] == 1
    ix.close()


# ---- case 5: the source kernel at its edges ------------------------------------------------------------------------------------------
def _codes_index(ctx, n, words, seed):
    """an index that is nothing but code rows (random bits, some rows duplicated so that the id tie-break decides)"""
    import pgvectorscale_amd as P
    rng = np.random.default_rng(seed)
    dim = {2: 64, 7: 200, 24: 768, 50: 1600}[words]
    codes = rng.integers(0, 1 << 63, (n, words), dtype=np.int64).astype(np.uint64)
    if dim * 2 % 64:
        codes[:, -1] &= U64((1 << (dim * 2 % 64)) - 1)
    dup = rng.integers(0, n, n // 4)
    codes[dup] = codes[(dup * 7 + 3) % n]
    nbrs = np.full((n, 4), INV, np.uint32)
    tids = ((np.arange(n, dtype=np.uint64) + 7) << U64(16)) | U64(1)
    ix = P.DiskAnnIndex.upload(ctx, codes=codes, nbrs=nbrs, heap_tids=tids, vecs=None, mean=np.zeros(dim, np.float32), m2=np.ones(dim, np.float32), count=2, bits=2,
                               dim_index=dim, num_neighbors=4, distance_type=P.VS_L2, default_start=0)
    return ix, codes


@pytest.mark.parametrize("words,n", [(2, 5003 if EMU else 150001), (7, 333), (24, 300 if EMU else 600), (50, 203)])
def test_nearest_masked_equals_numpy_at_the_kernels_edges(gpu_ctx, oracle, words, n):
    """2 words with more rows than one 64-row step per wave, 7 words (not a multiple of the 16-byte load), 24 words (the 768-d form),
    50 words (the looped form); n is no multiple of 64; 19 queries = two tiles of 8 and one of 3"""
    ix, codes = _codes_index(gpu_ctx, n, words, 31 + words)
    assert ix.desc.words == words and n % 64 != 0
    rng = np.random.default_rng(words)
    bits = rng.integers(0, 1 << 20, n, dtype=np.int64).astype(np.uint64)
    bits[rng.random(n) < 0.3] = 0
    skip = (rng.random(n) < 0.25).astype(np.uint8)
    nq = 19
    nodes = rng.choice(n, nq, replace=False).astype(np.uint32)
    want = rng.integers(1, 1 << 20, nq, dtype=np.int64).astype(np.uint64)
    # a query whose only admissible row is the last row, and one with none
    bits[n - 1] |= U64(1 << 40)
    skip[n - 1] = 0
    nodes[3] = 0 if nodes[3] == n - 1 else nodes[3]
    want[3] = U64(1 << 40)
    want[5] = U64(1 << 41)
    for cut, sk in ((slice(None), skip), (slice(None), None), (slice(0, 3), None)):
        ids, ham = ix.nearest_masked(nodes[cut], want[cut], bits, sk)
        for q, (xq, w) in enumerate(zip(nodes[cut], want[cut])):
            adm = (bits & w) != 0
            if sk is not None:
                adm &= sk == 0
            adm[xq] = False
            ref = _nearest(codes, int(xq), adm)
            assert (int(ids[q]), int(ham[q])) == (ref if ref is not None else (INV, INV)), (words, q)
        if cut == slice(None):
            assert ids[3] == n - 1 and ids[5] == INV and ham[5] == INV
    # ties: every row admissible, the nearest of a duplicated row is its lowest-numbered duplicate
    allb = np.ones(n, np.uint64)
    dupq = np.array([i for i in range(n) if (codes[i] == codes[(i * 7 + 3) % n]).all() and (i * 7 + 3) % n != i][:8], np.uint32)
    assert dupq.size > 0
    ids, ham = ix.nearest_masked(dupq, np.ones(dupq.size, np.uint64), allb)
    for q, xq in enumerate(dupq):
        same = np.flatnonzero((codes == codes[xq]).all(1))
        assert ham[q] == 0 and ids[q] == min(int(i) for i in same if i != xq)
    ix.close()


# ---- case 6: idempotence and refusals ------------------------------------------------------------------------------------------------
def test_a_second_repair_writes_nothing_and_a_clean_index_is_untouched(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    ti, nbrs, start, ls = _graph("uni8", "labeled")
    ix = _upload(gpu_ctx, ti, nbrs, start, ls)
    first = ix.repair_labels()
    once = ix.download()
    again = ix.repair_labels()
    assert first["rows_changed"] > 0 and first["lost_pairs_after"] == 0
    assert again["rows_changed"] == 0 and again["rounds"] == 0 and again["lost_pairs_before"] == 0 and again["unreachable_live"] == 0
    assert ix.download()["nbrs"].tobytes() == once["nbrs"].tobytes()
    audit = ix.label_reach()
    assert audit["lost_pairs"] == 0 and audit["lost_nodes"] == 0
    # the neighbors' label masks are rebuilt on demand and filtered scans still equal the oracle
    P.set_option("VS_F_NBRMASK", 1)
    try:
        qs = ti.queries(16, seed=8, kind="gauss")
        keys = [[sorted(ls)[i % len(ls)]] for i in range(16)]
        gi, _, gd, gst = ix.search_batch(qs, search_list_size=40, rescore=20, k=10, qlabels=keys)
        assert ix._L.vs_index_has_neighbor_masks(ix.h) == 1
        oi, od, ost = _oracle_index(oracle, ti, once, start, ls).search_batch(qs, L=40, rescore=20, k=10, qlabels=keys)
        assert (gi == oi).all() and (gd.view(np.uint32) == od.view(np.uint32)).all() and gst["visited_nodes"] == ost["visited_nodes"]
        ix.repair_labels()
        assert ix._L.vs_index_has_neighbor_masks(ix.h) == 1  # (nothing lost, nothing written: the cache stays)
    finally:
        P.set_option("VS_F_NBRMASK", None)
    ix.close()


def _refused(ix, code, call):
    import pgvectorscale_amd as P
    before = ix.download(codes=ix.desc.storage_type != P._lib.VS_STORAGE_PLAIN)
    with pytest.raises(P._lib.VsError) as e:
        call()
    assert e.value.code == code, str(e.value)
    after = ix.download(codes=ix.desc.storage_type != P._lib.VS_STORAGE_PLAIN)
    assert all(after[k].tobytes() == before[k].tobytes() for k in ("codes", "nbrs", "heap_tids") if before[k] is not None)
    return str(e.value)


def test_refusals_leave_every_byte_as_it_was(gpu_ctx, oracle):
    import ctypes as C
    import pgvectorscale_amd as P
    from pgvectorscale_amd.pages import PagesOut
    ti = TestIndex(n=400, dim_full=64, bits=2, R=16, distance=oracle.L2, seed=73, kind="gauss", L_build=30, n_labels=8)
    ix = ti.upload(gpu_ctx)
    assert ix.label_reach()["lost_pairs"] > 0
    _refused(ix, INVALID, lambda: ix.repair_labels(max_rounds=65))
    st = P._lib.LabelRepairStats()
    _refused(ix, INVALID, lambda: P._lib.check(ix._L.vs_index_repair_labels(ix.h, 0, 1, C.byref(st))))  # unknown flags
    out = PagesOut(ix)
    assert "writer" in _refused(ix, STATE, ix.repair_labels)
    out.close()
    ctx2 = P.Context(0)
    view = ix.view(ctx2)
    assert "view" in _refused(ix, STATE, ix.repair_labels)
    assert "view" in _refused(view, STATE, view.repair_labels)
    assert view.label_reach()["lost_pairs"] == ix.label_reach()["lost_pairs"]  # the audit works on a view
    view.close()
    ctx2.close()
    assert ix.repair_labels()["rows_changed"] > 0  # (the writer and the view are gone: the call goes through)
    ix.close()
    bare = TestIndex(n=400, dim_full=64, bits=2, R=16, distance=oracle.L2, seed=73, kind="gauss", L_build=30)
    nolabels = bare.upload(gpu_ctx)
    assert "label" in _refused(nolabels, INVALID, nolabels.repair_labels)
    assert "label" in _refused(nolabels, INVALID, nolabels.label_reach)
    nolabels.close()
    plain = P.DiskAnnIndex.upload(gpu_ctx, codes=None, nbrs=ti.nbrs, heap_tids=ti.tids, vecs=ti.vecs, mean=None, m2=None, count=0, bits=1,
                                  dim_index=64, num_neighbors=16, distance_type=P.VS_L2, default_start=ti.start,
                                  storage_type=P._lib.VS_STORAGE_PLAIN)
    assert "plain" in _refused(plain, INVALID, plain.repair_labels)
    plain.close()


# ---- case 7: quality -----------------------------------------------------------------------------------------------------------------
# the build's seed-to-seed spread of recall@10 (tests/test_gpu_zv_insert.py)
QUALITY_MARGIN = 0.0117


@pytest.mark.skipif(EMU, reason="a 20 000 x 128 device build: hardware only, as the consolidation test it mirrors")
def test_recall_with_and_without_a_label_key_is_no_worse_after_the_repair(gpu_ctx, oracle):
    """20 000 x 128, R = 32, label-aware device build (L = 64) with 32 Zipf labels, 256 queries, recall@10 at L = 100 / rescore 50
    against the exact f32 top-10: unfiltered over all rows, and under single-label keys over that label's carriers for the 8 rarest
    labels with at least 10 carriers.  The baseline is the same graph before the repair; all four values are printed."""
    import pgvectorscale_amd as P
    from pgvectorscale_amd.datagen import DatagenParams, fill_device, rows_numpy
    n, dim, R, nl = 20000, 128, 32, 32
    p = DatagenParams(seed=9, dim=dim, latent_dim=24, n_clusters=64)
    q = rows_numpy(p, 10 ** 9, 256)
    rng = np.random.default_rng(77)
    pz = 1.0 / np.arange(1, nl + 1)
    pz /= pz.sum()
    off, vals = np.zeros(n + 1, np.uint32), []
    for i in range(n):
        vals.extend(sorted(set(int(v) + 1 for v in rng.choice(nl, int(rng.integers(1, 4)), p=pz))))
        off[i + 1] = len(vals)
    vals = np.array(vals, np.int16)
    ix = P.DiskAnnIndex.alloc(gpu_ctx, n=n, dim_full=dim, num_neighbors=R, distance_type=P.VS_L2)
    fill_device(gpu_ctx, p, 0, n, ix.array(P._lib.ARR_VECS)[0])
    gpu_ctx.upload(ix.array(P._lib.ARR_TIDS)[0], ((np.arange(n, dtype=np.uint64) + 11) << U64(16)) | U64(3))
    ix.set_labels(off, vals)
    ix.sbq_train()
    ix.sbq_quantize_corpus()
    ix.build_graph(search_list_size=64, max_alpha=1.2)
    X = ix.download(codes=False, nbrs=False, tids=False, vecs=True)["vecs"]
    d = (q ** 2).sum(1)[:, None] - 2 * q @ X.T + (X ** 2).sum(1)[None, :]
    node_of = np.repeat(np.arange(n), np.diff(off))
    carriers = {l: np.unique(node_of[vals == l]) for l in range(1, nl + 1)}
    rare = sorted((l for l in carriers if carriers[l].size >= 10), key=lambda l: (carriers[l].size, l))[:8]
    gt_all = np.argsort(d, axis=1, kind="stable")[:, :10]
    gt = {l: carriers[l][np.argsort(d[:, carriers[l]], axis=1, kind="stable")[:, :10]] for l in rare}

    def recall(got, want):
        return float(np.mean([len(set(a) & set(b)) / 10 for a, b in zip(got.tolist(), want.tolist())]))

    def measure():
        r_all = recall(ix.search_batch(q, search_list_size=100, rescore=50, k=10)[0], gt_all)
        r_lab = float(np.mean([recall(ix.search_batch(q, search_list_size=100, rescore=50, k=10, qlabels=[[l]] * 256)[0], gt[l]) for l in rare]))
        return r_all, r_lab

    audit = ix.label_reach()
    base_all, base_lab = measure()
    st = ix.repair_labels()
    after_all, after_lab = measure()
    print("rare labels", rare, [int(carriers[l].size) for l in rare], "lost before", audit["lost_pairs"], audit["lost_nodes"], st)
    print("recall@10 unfiltered: before", base_all, "after", after_all, " single-label keys: before", base_lab, "after", after_lab)
    assert st["lost_pairs_before"] == audit["lost_pairs"] and st["unreachable_live"] == 0
    assert after_all >= base_all - QUALITY_MARGIN
    assert after_lab >= base_lab - QUALITY_MARGIN
    ix.close()
