"""vs_index_consolidate_deletes: the rows that name a deleted node take over that node's neighbors and are pruned again (DESIGN.md
section 6d).  The reference is `_twin`, a numpy restatement of rules 1-8 written here (its prune in tests/build_twin.py): np.bitwise_count for the Hamming distance,
np.float32 arithmetic for the alpha ladder, the general loop of wave_prune line by line (its inner loop over j as one numpy
expression).  Every case asserts its own preconditions on the restatement before it looks at the device.  Also runs on the lockstep
interpreter (tests/test_emu_consolidate.py)."""
import functools
import os

import numpy as np
import pytest

from build_twin import _ham, _pmask, _prune
from helpers import TestIndex, make_vectors

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF
STATE, INVALID = -5, -1
EMU = bool(os.environ.get("VS_EMU"))
COUNTERS = ("tombstones", "tombstones_kept", "rows_rewritten", "edges_dropped", "edges_added", "rows_pruned", "rows_capped", "rows_emptied")


# ---- the restatement (_ham, _prune and _pmask live in tests/build_twin.py, which the build and insert restatement shares) -----------
def _twin(codes, nbrs, tids, starts, R, max_alpha=1.2, cand_max=0, sets=None):
    n = len(tids)
    dead = (tids & np.uint64(0xFFFF)) == 0
    keep = ~dead
    keep[sorted(starts)] = True                                                      # rule 1
    D = ~keep
    cap = cand_max or min(4 * R, 256)
    out = nbrs.copy()
    st = dict.fromkeys(COUNTERS, 0)
    st["tombstones"], st["tombstones_kept"] = int(dead.sum()), int((dead & keep).sum())
    for p in range(n):
        if D[p]:
            continue                                                                 # rule 2
        row = nbrs[p][nbrs[p] != INV]
        gone = row[D[row]]
        if gone.size == 0:
            continue                                                                 # rule 3
        st["rows_rewritten"] += 1
        st["edges_dropped"] += int(gone.size)
        cand = set(int(v) for v in row if keep[v])                                   # rule 4
        for d in gone:
            cand |= set(int(w) for w in nbrs[d] if w != INV and keep[w])
        cand.discard(p)
        ids = np.array(sorted(cand), np.int64)
        dist = _ham(codes, ids, p) if ids.size else np.zeros(0, np.uint32)           # rule 5
        order = np.lexsort((ids, dist))                                              # rule 6
        ids, dist = ids[order], dist[order]
        if ids.size > cap:                                                           # rule 7
            st["rows_capped"] += 1
            ids, dist = ids[:cap], dist[:cap]
        if ids.size <= R:                                                            # rule 8
            new = ids
        else:
            st["rows_pruned"] += 1
            pm = None if sets is None else np.array([_pmask(sets, p, int(w)) for w in ids], np.uint64)
            new = ids[_prune(codes, ids, dist, R, max_alpha, pm)]
        st["rows_emptied"] += int(new.size == 0)
        st["edges_added"] += len(set(new.tolist()) - set(row.tolist()))
        out[p] = INV
        out[p, :new.size] = new
    return out, st, D


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _index(which):
    from oracle import oracle_py as O
    if which == "general":
        return TestIndex(n=1400, dim_full=64, bits=2, R=24, distance=O.L2, seed=18, kind="gauss", L_build=50)
    if which == "wide":  # 24-word codes: the register form of the prune
        return TestIndex(n=300 if EMU else 600, dim_full=768, bits=2, R=16, distance=O.L2, seed=21, kind="gauss", L_build=40)
    if which == "labeled":
        return TestIndex(n=1400, dim_full=64, bits=2, R=24, distance=O.L2, seed=19, kind="gauss", L_build=50, n_labels=8)
    raise KeyError(which)


def _dead_nodes(ti, frac, seed, must=(), never=()):
    rng = np.random.default_rng(seed)
    pick = rng.random(ti.n) < frac
    pick[list(must)] = True
    pick[list(never)] = False
    return np.flatnonzero(pick)


def _sets(ti):
    return [set(int(v) for v in ti.label_val[ti.label_off[i]:ti.label_off[i + 1]]) for i in range(ti.n)]


def _sorted_sets(ti):
    return [sorted(s) for s in _sets(ti)]


class _SetsView:
    """sets[p] iterates in sorted order (label_pmask numbers p's labels that way); `in` is a set test"""

    def __init__(self, ti):
        self.s, self.o = _sets(ti), _sorted_sets(ti)

    def __getitem__(self, i):
        return _Both(self.s[i], self.o[i])


class _Both:
    def __init__(self, s, o):
        self.s, self.o = s, o

    def __iter__(self):
        return iter(self.o)

    def __contains__(self, x):
        return x in self.s


def _run(gpu_ctx, ti, dead, *, cand_max=0, repair=False, sets=None):
    """upload, bulk_delete the tids of `dead`, consolidate -> (index, before, after, stats, twin rows, twin stats, D)"""
    ix = ti.upload(gpu_ctx)
    if len(dead):
        st = ix.bulk_delete(ti.tids[dead])
        assert st["tuples_removed"] == len(dead)
    before = ix.download()
    starts = {int(ti.start)} | set(int(v) for v in ti.label_starts.values())
    want, wst, D = _twin(before["codes"], before["nbrs"], before["heap_tids"], starts, ti.R, 1.2, cand_max, sets)
    got = ix.consolidate_deletes(max_alpha=1.2, cand_max=cand_max, repair=repair)
    after = ix.download()
    return ix, before, after, got, want, wst, D


def _same(before, after, got, want, wst):
    assert after["heap_tids"].tobytes() == before["heap_tids"].tobytes()
    assert after["codes"].tobytes() == before["codes"].tobytes()
    bad = np.flatnonzero((after["nbrs"] != want).any(1))
    assert bad.size == 0, (bad[:8], after["nbrs"][bad[:1]], want[bad[:1]])
    assert {k: got[k] for k in COUNTERS} == wst
    assert got["unreachable_live"] == INV  # (not judged without the repair pass)


# ---- case 1: the general path -------------------------------------------------------------------------------------------------------
# At 30 % deleted and R = 24 a row's de-duplicated union outgrows the default cap of 96 for most rows of this index (830 of the 970
# rewritten ones), so "no row capped" cannot hold at the default cap on this shape.  Both are checked: the default cap as it is, and
# cand_max = 1024 (more than the R + R * R = 600 candidates a row can have), where no row is capped and the whole union is pruned.
@pytest.mark.parametrize("cand_max", [0, 1024], ids=["default_cap_96", "uncapped"])
def test_rows_and_stats_equal_the_restatement(gpu_ctx, oracle, cand_max):
    ti = _index("general")
    ix, before, after, got, want, wst, D = _run(gpu_ctx, ti, _dead_nodes(ti, 0.3, 5, never=[ti.start]), cand_max=cand_max)
    print("restatement:", wst)
    assert wst["rows_pruned"] > 0 and wst["rows_rewritten"] > 500
    if cand_max:
        assert wst["rows_capped"] == 0
    _same(before, after, got, want, wst)
    assert (after["nbrs"][D] == before["nbrs"][D]).all()  # rows of D are never written
    ix.close()


# ---- case 2: the cap ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", ["R+1", "2R"])
def test_cap_keeps_the_closest_candidates(gpu_ctx, oracle, cap):
    ti = _index("general")
    cand_max = ti.R + 1 if cap == "R+1" else 2 * ti.R
    ix, before, after, got, want, wst, _ = _run(gpu_ctx, ti, _dead_nodes(ti, 0.3, 5, never=[ti.start]), cand_max=cand_max)
    assert wst["rows_capped"] > 0 and wst["rows_pruned"] >= wst["rows_capped"]
    _same(before, after, got, want, wst)
    ix.close()


# ---- case 3: 24-word codes, the register form of the prune and the general loop over LDS codes ----------------------------------------
@pytest.mark.parametrize("cand_max", [64, 128])
def test_24_word_codes_both_forms_of_the_prune(gpu_ctx, oracle, cand_max):
    ti = _index("wide")
    assert ti.codes.shape[1] == 24
    ix, before, after, got, want, wst, _ = _run(gpu_ctx, ti, _dead_nodes(ti, 0.3, 6, never=[ti.start]), cand_max=cand_max)
    assert wst["rows_pruned"] > 0
    _same(before, after, got, want, wst)
    ix.close()


# ---- case 4: corners ----------------------------------------------------------------------------------------------------------------
def test_a_deleted_default_start_node_stays_in_the_graph(gpu_ctx, oracle):
    ti = _index("general")
    s = int(ti.start)
    ix, before, after, got, want, wst, D = _run(gpu_ctx, ti, _dead_nodes(ti, 0.3, 7, must=[s]))
    assert not D[s] and wst["tombstones_kept"] == 1 and D[before["nbrs"][s][before["nbrs"][s] != INV]].any()
    _same(before, after, got, want, wst)
    assert (after["nbrs"][s] != before["nbrs"][s]).any() and not D[after["nbrs"][s][after["nbrs"][s] != INV]].any()
    # a kept row names the start node only where rule 4 puts it among the row's candidates: it was in the row, or in the row of
    # one of the row's deleted neighbors
    for p in np.flatnonzero(((after["nbrs"] == s).any(1)) & ~D):
        row = before["nbrs"][p]
        gone = [int(d) for d in row if d != INV and D[d]]
        assert s in row or any(s in before["nbrs"][d] for d in gone), p
    ix.close()


def test_a_node_whose_neighbors_are_all_deleted(gpu_ctx, oracle):
    ti = _index("general")
    p = next(i for i in range(700, ti.n) if i != ti.start and (ti.nbrs[i] != INV).sum() >= 8)
    dead = np.array(sorted(set(int(v) for v in ti.nbrs[p] if v != INV) - {int(ti.start), p}))
    ix, before, after, got, want, wst, D = _run(gpu_ctx, ti, dead)
    assert D[before["nbrs"][p][before["nbrs"][p] != INV]].all()
    _same(before, after, got, want, wst)
    new = after["nbrs"][p][after["nbrs"][p] != INV]
    assert new.size > 0 and not (set(new.tolist()) & set(dead.tolist()))
    ix.close()


def test_a_whole_neighborhood_is_deleted(gpu_ctx, oracle):
    """a node, its neighbors and theirs: the node's own neighbor p, left alive, finds nothing to take over"""
    ti = _index("general")
    nb = ti.nbrs
    hood = lambda xs: set(int(v) for x in xs for v in nb[x] if v != INV)
    p = next(i for i in range(900, ti.n) if i != ti.start and ti.start not in hood(hood([i]) | {i}))
    dead = np.array(sorted((hood([p]) | hood(hood([p]))) - {p}))
    ix, before, after, got, want, wst, D = _run(gpu_ctx, ti, dead)
    assert wst["rows_emptied"] >= 1 and dead.size < ti.n // 2
    _same(before, after, got, want, wst)
    assert (after["nbrs"][p] == INV).all()
    ix.close()
    # with the repair pass the emptied row's node is still reachable (it keeps its in-edges from the rest of the graph or gets one)
    ix = ti.upload(gpu_ctx)
    ix.bulk_delete(ti.tids[dead])
    assert ix.consolidate_deletes()["unreachable_live"] == 0
    ix.close()


def test_nothing_deleted_nothing_changes_and_a_second_call_rewrites_nothing(gpu_ctx, oracle):
    ti = _index("general")
    ix, before, after, got, want, wst, _ = _run(gpu_ctx, ti, np.zeros(0, np.int64))
    assert all(got[k] == 0 for k in COUNTERS) and all(after[k].tobytes() == before[k].tobytes() for k in ("codes", "nbrs", "heap_tids"))
    ix.bulk_delete(ti.tids[_dead_nodes(ti, 0.3, 8, never=[ti.start])])
    first = ix.consolidate_deletes(repair=False)
    once = ix.download()
    again = ix.consolidate_deletes(repair=False)
    assert first["rows_rewritten"] > 0 and again["tombstones"] == first["tombstones"]
    assert all(again[k] == 0 for k in COUNTERS if k not in ("tombstones", "tombstones_kept"))
    assert ix.download()["nbrs"].tobytes() == once["nbrs"].tobytes()
    ix.close()


# ---- case 5: labels -----------------------------------------------------------------------------------------------------------------
def test_labeled_index_prunes_with_the_label_rule_and_keeps_label_start_nodes(gpu_ctx, oracle):
    ti = _index("labeled")
    ls = next(v for v in ti.label_starts.values() if v != ti.start)
    ix, before, after, got, want, wst, D = _run(gpu_ctx, ti, _dead_nodes(ti, 0.3, 9, must=[ls], never=[ti.start]), sets=_SetsView(ti))
    assert ix.desc.n_label_starts == len(ti.label_starts) and not D[ls]
    kept = set(int(v) for v in ti.label_starts.values() if (before["heap_tids"][v] & np.uint64(0xFFFF)) == 0)
    assert ls in kept and wst["tombstones_kept"] == len(kept) and wst["rows_pruned"] > 0
    plain, _, _ = _twin(before["codes"], before["nbrs"], before["heap_tids"], {int(ti.start)} | set(ti.label_starts.values()), ti.R)
    assert (plain != want).any(), "the label rule must matter on this input"
    _same(before, after, got, want, wst)
    ix.close()


# ---- case 6: invariant and scans -----------------------------------------------------------------------------------------------------
def test_after_the_full_call_no_kept_row_names_a_tombstone_and_scans_equal_the_oracle(gpu_ctx, oracle):
    O = oracle
    ti = _index("general")
    dead = _dead_nodes(ti, 0.3, 5, never=[ti.start])
    ix, before, after, got, want, wst, D = _run(gpu_ctx, ti, dead, repair=True)
    assert {k: got[k] for k in COUNTERS} == wst and got["unreachable_live"] == 0
    named = after["nbrs"][~D]
    assert not D[named[named != INV]].any()
    assert (after["nbrs"][D] == before["nbrs"][D]).all()
    live = ti.n - dead.size
    host = ix.download(vecs=True)
    oidx = O.OracleIndex(codes=host["codes"], nbrs=host["nbrs"], heap_tids=host["heap_tids"], vecs=host["vecs"], mean=ti.mean, m2=ti.m2,
                         count=ti.count, bits=ti.bits, dim_index=ti.dim_index, num_neighbors=ti.R, distance_type=ti.distance,
                         default_start=ti.start)
    # the reference's exhaustiveness pin (AM/build.rs:1254-1269): search_list_size 2, a stream longer than the live count
    q = ti.queries(32, seed=44, kind="gauss")
    scan = ix.beginscan()
    scan.rescan(q[0], search_list_size=2, rescore=4)
    rows = []
    for _ in range(ti.n + 1):
        r = scan.gettuple()
        if r is None:
            break
        rows.append(r[1])
    scan.endscan()
    assert len(rows) == live and len(set(rows)) == live and not (set(rows) & set(dead.tolist()))
    gi, _, gd, gst = ix.search_batch(q, search_list_size=40, rescore=20, k=10)
    oi, od, ost = oidx.search_batch(q, L=40, rescore=20, k=10)
    assert (gi == oi).all() and (gd.view(np.uint32) == od.view(np.uint32)).all() and gst["visited_nodes"] == ost["visited_nodes"]
    assert not (set(gi.ravel().tolist()) & set(dead.tolist()))
    ix.close()


# ---- case 7: less work ---------------------------------------------------------------------------------------------------------------
def test_scans_compare_fewer_codes_after_the_pass(gpu_ctx, oracle):
    O = oracle
    ti = _index("general")
    ix, before, after, got, _, _, _ = _run(gpu_ctx, ti, _dead_nodes(ti, 0.3, 5, never=[ti.start]), repair=True)
    q = ti.queries(64, seed=45, kind="gauss")
    work = []
    for host in (before, after):
        oidx = O.OracleIndex(codes=host["codes"], nbrs=host["nbrs"], heap_tids=host["heap_tids"], vecs=ti.vecs, mean=ti.mean, m2=ti.m2,
                             count=ti.count, bits=ti.bits, dim_index=ti.dim_index, num_neighbors=ti.R, distance_type=ti.distance,
                             default_start=ti.start)
        work.append(oidx.search_batch(q, L=40, rescore=20, k=10)[2]["quantized_distance_comparisons"])
    print("quantized distance comparisons of 64 scans: before", work[0], "after", work[1])
    assert work[1] < work[0]
    ix.close()


# ---- case 8: quality -----------------------------------------------------------------------------------------------------------------
# the build's seed-to-seed spread of recall@10 (tests/test_gpu_zv_insert.py)
QUALITY_MARGIN = 0.9531 - 0.9414


@pytest.mark.skipif(EMU, reason="20 000 x 128 device builds: hardware only, as the insert test it mirrors")
def test_a_consolidated_graph_is_as_good_as_one_rebuilt_over_the_live_rows(gpu_ctx, oracle):
    """recall@10 (L = 100, rescore 50, 256 queries, exact f32 top-10 over the live rows) of the consolidated graph against that of
    vs_build_graph over the live 70 % alone; both are printed"""
    import pgvectorscale_amd as P
    from pgvectorscale_amd.datagen import DatagenParams, fill_device, rows_numpy
    n, dim, R = 20000, 128, 32
    p = DatagenParams(seed=9, dim=dim, latent_dim=24, n_clusters=64)
    q = rows_numpy(p, 10 ** 9, 256)
    tids = ((np.arange(n, dtype=np.uint64) + 11) << np.uint64(16)) | np.uint64(3)

    def mk(X=None, rows=n):
        ix = P.DiskAnnIndex.alloc(gpu_ctx, n=rows, dim_full=dim, num_neighbors=R, distance_type=P.VS_L2)
        if X is None:
            fill_device(gpu_ctx, p, 0, rows, ix.array(P._lib.ARR_VECS)[0])
        else:
            gpu_ctx.upload(ix.array(P._lib.ARR_VECS)[0], X)
        ix.sbq_train()
        ix.sbq_quantize_corpus()
        ix.build_graph(search_list_size=64, max_alpha=1.2)
        return ix

    def recall(ix, gt):
        gi = ix.search_batch(q, search_list_size=100, rescore=50, k=10)[0]
        return float(np.mean([len(set(a) & set(b)) / 10 for a, b in zip(gi.tolist(), gt.tolist())]))

    ix = mk()
    gpu_ctx.upload(ix.array(P._lib.ARR_TIDS)[0], tids)
    X = ix.download(codes=False, nbrs=False, tids=False, vecs=True)["vecs"]
    dead = np.flatnonzero(np.random.default_rng(12).random(n) < 0.3)
    dead = dead[dead != ix.desc.default_start]
    alive = np.setdiff1d(np.arange(n), dead)
    d = (q ** 2).sum(1)[:, None] - 2 * q @ X[alive].T + (X[alive] ** 2).sum(1)[None, :]
    gt_local = np.argsort(d, axis=1, kind="stable")[:, :10]
    ix.bulk_delete(tids[dead])
    st = ix.consolidate_deletes()
    assert st["unreachable_live"] == 0 and st["rows_rewritten"] > 0
    r_cons = recall(ix, alive[gt_local])
    ix.close()
    base = mk(np.ascontiguousarray(X[alive]), rows=alive.size)
    r_base = recall(base, gt_local)
    base.close()
    print("recall@10: consolidated", r_cons, "rebuilt over the live rows", r_base, st)
    assert r_cons >= r_base - QUALITY_MARGIN


# ---- case 9: refusals ----------------------------------------------------------------------------------------------------------------
def _refused(ix, code, **kw):
    import pgvectorscale_amd as P
    before = ix.download()
    with pytest.raises(P._lib.VsError) as e:
        ix.consolidate_deletes(**kw)
    assert e.value.code == code, str(e.value)
    after = ix.download()
    assert all(after[k].tobytes() == before[k].tobytes() for k in ("nbrs", "heap_tids") if before[k] is not None)
    return str(e.value)


def test_refusals_leave_every_byte_as_it_was(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    from pgvectorscale_amd.pages import PagesOut
    ti = TestIndex(n=400, dim_full=64, bits=2, R=16, distance=oracle.L2, seed=73, kind="gauss", L_build=30)
    ix = ti.upload(gpu_ctx)
    ix.bulk_delete(ti.tids[_dead_nodes(ti, 0.3, 10, never=[ti.start])])
    _refused(ix, INVALID, cand_max=16)    # cand_max = R
    _refused(ix, INVALID, cand_max=1025)
    _refused(ix, INVALID, max_alpha=0.5)
    out = PagesOut(ix)
    assert "writer" in _refused(ix, STATE)
    out.close()
    ctx2 = P.Context(0)
    view = ix.view(ctx2)
    assert "view" in _refused(ix, STATE)
    with pytest.raises(P._lib.VsError) as e:
        view.consolidate_deletes()
    assert e.value.code == STATE
    view.close()
    ctx2.close()
    assert ix.consolidate_deletes()["rows_rewritten"] > 0  # (the writer and the view are gone: the call goes through)
    ix.close()
    plain = P.DiskAnnIndex.upload(gpu_ctx, codes=None, nbrs=ti.nbrs, heap_tids=ti.tids, vecs=ti.vecs, mean=None, m2=None, count=0, bits=1,
                                  dim_index=64, num_neighbors=16, distance_type=P.VS_L2, default_start=ti.start,
                                  storage_type=P._lib.VS_STORAGE_PLAIN)
    assert "plain" in _refused(plain, INVALID)
    plain.close()


# ---- case 10: with the delta writer --------------------------------------------------------------------------------------------------
def test_delta_after_a_consolidation_names_exactly_the_pages_of_the_changed_nodes(gpu_ctx, oracle, tmp_path):
    from pgvectorscale_amd.pages import PagesOut
    ti = _index("general")
    ix = ti.upload(gpu_ctx)
    path = tmp_path / "rel"
    out = PagesOut(ix)
    out.write_file(str(path))
    base = out.baseline()
    old = path.read_bytes()
    out.close()
    before = ix.download()
    # Two deleted nodes.  The rows that change are theirs (the tid) and those of the kept nodes that name them, which lie anywhere in
    # the index: a vacuum of a tenth of the rows leaves no node page clean at this size.  Few enough of them that fewer rows change
    # than the relation has node pages, so that "exactly the pages of the changed nodes" also says which pages stay as they were.
    indeg = np.bincount(ti.nbrs[ti.nbrs != INV], minlength=ti.n)
    dead = np.array([i for i in range(100, ti.n) if i != ti.start and 4 <= indeg[i] <= 12][:2])
    assert dead.size == 2 and indeg[dead].sum() + 2 < 30
    ix.bulk_delete(ti.tids[dead])
    st = ix.consolidate_deletes()
    after = ix.download()
    changed = np.flatnonzero((after["heap_tids"] != before["heap_tids"]) | (after["nbrs"] != before["nbrs"]).any(1))
    assert st["rows_rewritten"] > 0 and set(dead.tolist()) < set(changed.tolist())
    out = PagesOut(ix)
    want_blocks = sorted(set(out.item_pointer_of(int(i))[0] for i in changed))
    blocks, nb_now, new_base = out.delta(base)
    fresh = out.read().tobytes()
    B = len(fresh) // out.n_blocks
    node_blocks = set(out.item_pointer_of(i)[0] for i in range(ti.n))
    meta_changed = [b for b in range(out.n_blocks) if b not in node_blocks and fresh[b * B:(b + 1) * B] != old[b * B:(b + 1) * B]]
    assert blocks.tolist() == sorted(want_blocks + meta_changed) and nb_now == out.n_blocks == len(old) // B
    assert len(want_blocks) < len(node_blocks), "some node page must have stayed clean"
    third = out.patch_file(str(path), base)
    assert path.read_bytes() == fresh
    for b in (base, new_base, third):
        b.close()
    out.close()
    ix.close()
