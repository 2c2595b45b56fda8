"""vs_index_compact / vs_index_shrink_to_fit: the tombstones leave the arrays, the kept nodes are renumbered in place (DESIGN.md
section 6e).  The reference is `_twin`, a numpy restatement of the rule written here: the keep mask from the heap offsets plus the
start nodes, cumsum, fancy indexing, and a per-row rename-and-close-up loop.  Searches are held to the oracle over the downloaded
arrays (lifecycle_checks).  Also runs on the lockstep interpreter (tests/test_emu_compact.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import lifecycle_checks as LC
from helpers import TestIndex

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF
STATE, INVALID = -5, -1
EMU = bool(os.environ.get("VS_EMU"))
COUNTERS = ("n_before", "n_after", "tombstones", "tombstones_kept", "rows_moved", "edges_cut", "rows_emptied", "chunks")
ARRAYS = ("codes", "nbrs", "heap_tids", "vecs")
STAGE_DEFAULT = 256 << 20  # the header's default
SEARCH = dict(search_list_size=40, rescore=20, k=10)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def _twin(host, starts, stage_bytes=0):
    """-> (arrays of K in order, new_of, the counters)"""
    tids, nb = host["heap_tids"], host["nbrs"]
    n = len(tids)
    dead = (tids & np.uint64(0xFFFF)) == 0
    keep = ~dead
    keep[sorted(starts)] = True                                                      # rule 1
    new_of = np.where(keep, np.cumsum(keep) - 1, INV).astype(np.uint32)              # rule 2
    old_of = np.flatnonzero(keep)
    out = {k: (None if host[k] is None else host[k][old_of].copy()) for k in ARRAYS}  # rule 3
    cut = emptied = 0
    for j, i in enumerate(old_of):                                                   # rule 4
        row = nb[i][nb[i] != INV]
        stay = new_of[row][new_of[row] != INV]
        cut += row.size - stay.size
        emptied += int(stay.size == 0 and row.size > 0)
        out["nbrs"][j] = INV
        out["nbrs"][j, :stay.size] = stay
    moved = int((new_of[old_of] != old_of).sum())
    vec_row = -(-host["vecs"].shape[1] // 4) * 16  # the widest column: vec_stride floats
    per = min((stage_bytes or STAGE_DEFAULT) // vec_row, moved)
    st = dict(n_before=n, n_after=int(old_of.size), tombstones=int(dead.sum()), tombstones_kept=int((dead & keep).sum()), rows_moved=moved,
              edges_cut=int(cut), rows_emptied=int(emptied), chunks=-(-moved // per) if moved else 0)
    return out, new_of, st


def _twin_labels(off, val, new_of):
    sets = [val[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1) if new_of[i] != INV]
    return LC.label_csr(sets), sets


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _index(which):
    from oracle import oracle_py as O
    if which == "general":
        return TestIndex(n=1400, dim_full=64, bits=2, R=24, distance=O.L2, seed=18, kind="gauss", L_build=50)
    if which == "wide":  # 24-word codes, 3 KB vector rows: one row per wave in the mover
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


def _starts(ti):
    return {int(ti.start)} | set(int(v) for v in ti.label_starts.values())


def _same_bytes(a, b):
    return all((a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes() for k in ARRAYS)


def _assert_twin(after, got, gmap, want, wmap, wst):
    assert {k: got[k] for k in COUNTERS} == wst, (got, wst)
    assert (gmap == wmap).all()
    for k in ARRAYS:
        if want[k] is None:
            continue
        assert after[k].shape == want[k].shape, k
        bad = np.flatnonzero((after[k] != want[k]).reshape(len(want[k]), -1).any(1))
        assert bad.size == 0 and after[k].tobytes() == want[k].tobytes(), (k, bad[:8])


def _compact_against_twin(ix, ti, stage_bytes=0, start=None, **kw):
    """compact and compare with the restatement over the arrays as they stood -> (before, after, stats, new_of); start: the default
    start node where the test moved it away from the builder's"""
    before = ix.download(vecs=True)
    n_starts, cap = ix.desc.n_label_starts, ix.capacity
    start = int(ti.start) if start is None else start
    want, wmap, wst = _twin(before, (_starts(ti) - {int(ti.start)}) | {start}, stage_bytes)
    got, gmap = ix.compact(stage_bytes=stage_bytes, return_map=True, **kw)
    print("compact:", got)
    after = ix.download(vecs=True)
    _assert_twin(after, got, gmap, want, wmap, wst)
    assert ix.desc.n == wst["n_after"] and ix.capacity == cap and ix.desc.n_label_starts == n_starts
    assert ix.desc.default_start == wmap[start]
    return before, after, got, gmap


def _oracle(O, ix, ti, host, **kw):
    return LC.oracle_of(O, ix, host, ti.distance, **kw)


def _searches_equal_the_oracle(O, ix, ti, q, **okw):
    host = ix.download(vecs=True)
    oidx = _oracle(O, ix, ti, host, **okw)
    LC.check_search_batch(ix, oidx, q, None, "after compact")
    return oidx


# ---- cases 1, 2, 10: 30 % deleted, consolidated with repair, compacted ---------------------------------------------------------------
@pytest.fixture(scope="module")
def compacted(gpu_ctx, oracle):
    ti = _index("general")
    ix = ti.upload(gpu_ctx)
    dead = _dead_nodes(ti, 0.3, 5, never=[ti.start])
    assert ix.bulk_delete(ti.tids[dead])["tuples_removed"] == dead.size
    assert ix.consolidate_deletes()["unreachable_live"] == 0
    q = ti.queries(32, seed=44, kind="gauss")
    mean, m2, cnt = ix.get_quantizer()
    qcodes = oracle.quantize(mean, m2, cnt, ti.bits, LC.prepared_slice(oracle, q, ti.distance, ti.dim_index))
    pre = dict(search=ix.search_batch(q, **SEARCH), topk=ix.scan_topk(qcodes, 17))
    before, after, got, new_of = _compact_against_twin(ix, ti)
    yield dict(ti=ti, ix=ix, dead=dead, q=q, qcodes=qcodes, pre=pre, before=before, after=after, got=got, new_of=new_of)
    ix.close()


def test_bytes_equal_the_twin(compacted):
    c = compacted
    assert c["got"]["edges_cut"] == 0 and c["got"]["rows_emptied"] == 0 and c["got"]["tombstones_kept"] == 0
    assert c["got"]["n_after"] == c["ti"].n - c["dead"].size and c["got"]["rows_moved"] > 0 and c["got"]["chunks"] == 1
    assert (c["new_of"][c["dead"]] == INV).all()


def test_renumbering_changes_no_answer(compacted, oracle):
    c = compacted
    ix, new_of = c["ix"], c["new_of"]
    bi, bt, bd, bst = c["pre"]["search"]
    ai, at, ad, ast = ix.search_batch(c["q"], **SEARCH)
    assert (at == bt).all() and (ad.view(np.uint32) == bd.view(np.uint32)).all()
    assert (bi != INV).all() and (ai == new_of[bi]).all()
    for key in ("visited_nodes", "quantized_distance_comparisons", "full_distance_comparisons", "node_heap_reads", "next_calls"):
        assert ast[key] == bst[key], key
    (bti, bth), (ati, ath) = c["pre"]["topk"], ix.scan_topk(c["qcodes"], 17)
    # the flat scan also ranks dropped rows before the compaction: the survivors keep their (Hamming, id) order, mapped
    for r in range(len(c["q"])):
        live = new_of[bti[r]] != INV
        m = int(live.sum())
        assert (new_of[bti[r]][live] == ati[r][:m]).all() and (bth[r][live] == ath[r][:m]).all()
    LC.check_index_everywhere(ix, oracle, c["ti"].distance, c["q"], where="compacted")


# ---- case 3: without a prior consolidation -------------------------------------------------------------------------------------------
def test_without_a_consolidation_edges_are_cut_and_the_check_refuses(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    ti = _index("general")
    ix = ti.upload(gpu_ctx)
    ix.bulk_delete(ti.tids[_dead_nodes(ti, 0.3, 5, never=[ti.start])])
    before = ix.download(vecs=True)
    with pytest.raises(P._lib.VsError) as e:
        ix.compact(check_edges=True)
    assert e.value.code == STATE and "consolidate" in str(e.value)
    assert _same_bytes(ix.download(vecs=True), before) and ix.desc.n == ti.n
    _, after, got, _ = _compact_against_twin(ix, ti)
    assert got["edges_cut"] > 0
    LC.well_formed(after["nbrs"], ti.R)
    _searches_equal_the_oracle(oracle, ix, ti, ti.queries(32, seed=44, kind="gauss"))
    ix.close()


# ---- case 4: chunks that overlap their own sources ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dead_set", ["shift_below_a_chunk", "shift_above_a_chunk"])
def test_chunk_overlap(gpu_ctx, oracle, dead_set):
    import pgvectorscale_amd as P
    ti = _index("wide")
    row, per = 768 * 4, 25 if EMU else 50  # vector rows a chunk holds (the interpreter's index has half the rows)
    if dead_set == "shift_below_a_chunk":  # 10 %, spread evenly, the first tombstone at row 3: rows shift by less than a chunk until late
        dead = np.array([i for i in range(3, ti.n, 10) if i != ti.start])
    else:                                  # rows 0 .. 199 but the start node: every row shifts by more than a chunk
        dead = np.array([i for i in range(200) if i != ti.start])
    ix = ti.upload(gpu_ctx)
    ix.bulk_delete(ti.tids[dead])
    ix.consolidate_deletes()
    with pytest.raises(P._lib.VsError) as e:
        ix.compact(stage_bytes=row - 16)
    assert e.value.code == INVALID and ix.desc.n == ti.n
    _, _, got, _ = _compact_against_twin(ix, ti, stage_bytes=per * row + 100)
    assert got["chunks"] >= 3 and got["edges_cut"] == 0
    _searches_equal_the_oracle(oracle, ix, ti, ti.queries(8, seed=44, kind="gauss"))
    ix.close()


# ---- case 5: edges ------------------------------------------------------------------------------------------------------------------
def test_nothing_deleted_nothing_moves(gpu_ctx, oracle):
    ti = _index("general")
    ix = ti.upload(gpu_ctx)
    before, after, got, new_of = _compact_against_twin(ix, ti)
    assert got["rows_moved"] == 0 and got["chunks"] == 0 and ix.desc.n == ti.n and _same_bytes(before, after)
    assert (new_of == np.arange(ti.n)).all()
    ix.close()


def test_every_row_deleted_but_the_start_node(gpu_ctx, oracle):
    ti = _index("general")
    ix = ti.upload(gpu_ctx)
    ix.bulk_delete(np.delete(ti.tids, ti.start))
    _, after, got, _ = _compact_against_twin(ix, ti)
    assert got["n_after"] == 1 and (after["nbrs"] == INV).all() and ix.desc.default_start == 0
    ix.bulk_delete(ti.tids[[ti.start]])
    gi, _, _, _ = ix.search_batch(ti.queries(4, seed=44, kind="gauss"), **SEARCH)
    assert (gi == INV).all()
    ix.close()


def test_a_deleted_default_start_node_stays(gpu_ctx, oracle):
    ti = _index("general")
    s = 700  # (the builder's start node is node 0, which a stable renumbering never moves: scans begin at a node that does move)
    assert ti.start != s and (ti.nbrs[s] != INV).sum() >= 8
    ix = ti.upload(gpu_ctx)
    ix.set_start_nodes(s)
    ix.bulk_delete(ti.tids[_dead_nodes(ti, 0.3, 7, must=[s])])
    ix.consolidate_deletes()
    _, after, got, new_of = _compact_against_twin(ix, ti, start=s)
    assert got["tombstones_kept"] == 1 and got["edges_cut"] == 0
    assert ix.desc.default_start == new_of[s] != INV and new_of[s] < s and (after["heap_tids"][new_of[s]] & np.uint64(0xFFFF)) == 0
    _searches_equal_the_oracle(oracle, ix, ti, ti.queries(32, seed=44, kind="gauss"))
    ix.close()


def test_labeled_index_keeps_deleted_label_start_nodes_and_the_label_sets_of_k(gpu_ctx, oracle):
    ti = _index("labeled")
    ls = next(v for v in ti.label_starts.values() if v != ti.start)
    ix = ti.upload(gpu_ctx)
    ix.bulk_delete(ti.tids[_dead_nodes(ti, 0.3, 9, must=[ls], never=[ti.start])])
    ix.consolidate_deletes()
    _, after, got, new_of = _compact_against_twin(ix, ti)
    kept = set(v for v in ti.label_starts.values() if (ti.tids[v] & np.uint64(0xFFFF)) != 0 and new_of[v] != INV
               and (after["heap_tids"][new_of[v]] & np.uint64(0xFFFF)) == 0)
    assert ls in kept and got["tombstones_kept"] == len(kept)
    (woff, wval), sets = _twin_labels(ti.label_off, ti.label_val, new_of)
    goff, gval = LC.download_labels(ix)
    assert goff.tobytes() == woff.tobytes() and gval.tobytes() == wval.tobytes()
    starts = {l: int(new_of[v]) for l, v in ti.label_starts.items()}
    q = ti.queries(32, seed=44, kind="gauss")
    rng = np.random.default_rng(3)
    keys = [sorted(set(int(v) for v in rng.integers(1, 9, 2))) for _ in range(len(q))]
    # The label start nodes have no download: the keyed searches, streams and cursors below begin at them, and the oracle they
    # are held to (ids, counters) is handed the twin's mapped nodes.
    LC.check_index_everywhere(ix, oracle, ti.distance, q, keys, label_starts=starts, label_sets=sets, where="labeled, compacted")
    ix.close()


# ---- case 6: visibility -------------------------------------------------------------------------------------------------------------
def test_visibility_masks_keep_the_rows_of_k(gpu_ctx, oracle):
    from pgvectorscale_amd import _lib
    ti = _index("general")
    ix = ti.upload(gpu_ctx)
    rng = np.random.default_rng(11)
    own = (rng.random(ti.n) > 0.25).astype(np.uint8)
    snap = (rng.random(ti.n) > 0.35).astype(np.uint8)
    ix.set_visibility(own)
    _lib.check(ix._L.vs_index_snapshot_put(ix.h, 3, snap.ctypes.data_as(C.c_void_p)))
    ix.bulk_delete(ti.tids[_dead_nodes(ti, 0.3, 5, never=[ti.start])])
    ix.consolidate_deletes()
    _, _, _, new_of = _compact_against_twin(ix, ti)
    k = new_of != INV
    q = ti.queries(32, seed=44, kind="gauss")
    LC.check_index_everywhere(ix, oracle, ti.distance, q, visible=own[k], snapshots={3: snap[k]}, where="masks, compacted")
    ix.close()


# ---- case 7: the freed room is used --------------------------------------------------------------------------------------------------
def test_an_insert_fills_the_freed_room_without_growing(gpu_ctx, oracle):
    ti = _index("general")
    ix = ti.upload(gpu_ctx)
    dead = _dead_nodes(ti, 0.3, 5, never=[ti.start])
    ix.bulk_delete(ti.tids[dead])
    ix.consolidate_deletes()
    ix.compact()
    cap = ix.capacity
    assert cap == ti.n and ix.desc.n == ti.n - dead.size
    X = np.random.default_rng(5).standard_normal((dead.size, ti.dim_full)).astype(np.float32)
    st = ix.insert(X, LC.make_tids(10 ** 6, dead.size), search_list_size=48)
    assert st["grew"] == 0 and st["inserted"] == dead.size and ix.capacity == cap and ix.desc.n == ti.n
    LC.check_index_everywhere(ix, oracle, ti.distance, ti.queries(32, seed=44, kind="gauss"), where="compacted, refilled")
    ix.close()


# ---- case 8: pages ------------------------------------------------------------------------------------------------------------------
def test_pages_of_the_compacted_index_and_a_delta_from_before(gpu_ctx, oracle, tmp_path):
    from oracle import pages_py as PG
    from pgvectorscale_amd.pages import PagesOut
    ti = _index("general")
    ix = ti.upload(gpu_ctx)
    ix.bulk_delete(ti.tids[_dead_nodes(ti, 0.3, 5, never=[ti.start])])
    ix.consolidate_deletes()
    kw = dict(extension_version="0.8.0", search_list_size=48, max_alpha=1.2)
    path = tmp_path / "rel"
    out = PagesOut(ix, **kw)
    out.write_file(str(path))
    base, blocks_before = out.baseline(), out.n_blocks
    out.close()
    ix.compact()
    host = ix.download()
    mean, m2, cnt = ix.get_quantizer()
    d = ix.desc
    want = PG.write_index(codes=host["codes"], nbrs=host["nbrs"], heap_tids=host["heap_tids"], mean=mean, m2=m2, count=cnt, means_first=True,
                          meta=dict(num_dimensions=ti.dim_full, num_dimensions_to_index=d.dim_index, bq_num_bits_per_dimension=d.bits,
                                    distance_type=d.distance_type, num_neighbors=ti.R, default_start=int(d.default_start), **kw)).rel.tobytes()
    out = PagesOut(ix, **kw)
    fresh = out.read().tobytes()
    assert fresh == want and out.n_blocks < blocks_before
    new_base = out.patch_file(str(path), base)
    assert path.read_bytes() == fresh
    for b in (base, new_base):
        b.close()
    out.close()
    ix.close()


# ---- case 9: refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_byte_as_it_was(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    from pgvectorscale_amd.pages import PagesOut
    ti = TestIndex(n=400, dim_full=64, bits=2, R=16, distance=oracle.L2, seed=73, kind="gauss", L_build=30)
    ix = ti.upload(gpu_ctx)
    ix.bulk_delete(ti.tids[_dead_nodes(ti, 0.3, 10, never=[ti.start])])
    before = ix.download(vecs=True)

    def refused(handle, word, call=lambda h: h.compact()):
        with pytest.raises(P._lib.VsError) as e:
            call(handle)
        assert e.value.code == STATE and word in str(e.value), str(e.value)
        assert _same_bytes(ix.download(vecs=True), before) and ix.desc.n == ti.n

    out = PagesOut(ix)
    refused(ix, "writer")
    out.close()
    ctx2 = P.Context(0)
    view = ix.view(ctx2)
    refused(ix, "view")
    refused(view, "view")
    refused(ix, "view", lambda h: h.shrink_to_fit())
    refused(view, "view", lambda h: h.shrink_to_fit())
    view.close()
    ctx2.close()
    q = ti.queries(8, seed=1, kind="gauss")
    dq, nq = gpu_ctx.alloc(q.nbytes), len(q)
    d_ids = gpu_ctx.alloc(nq * 10 * 4)
    gpu_ctx.upload(dq, q)
    ix.search_batch_dev(dq, nq, 40, 20, 10, d_ids)
    try:
        refused(ix, "in flight")
        refused(ix, "in flight", lambda h: h.shrink_to_fit())
    finally:
        ix.search_batch_dev_finish()
        gpu_ctx.free(dq)
        gpu_ctx.free(d_ids)
    assert ix.compact()["rows_moved"] > 0  # (the writer, the view and the batch are gone: the call goes through)
    ix.close()


# ---- plain storage --------------------------------------------------------------------------------------------------------------------
def test_plain_storage_moves_every_column_it_holds(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    ti = _index("general")
    ix = P.DiskAnnIndex.upload(gpu_ctx, codes=None, nbrs=ti.nbrs, heap_tids=ti.tids, vecs=ti.vecs, mean=None, m2=None, count=0, bits=1,
                               dim_index=ti.dim_full, num_neighbors=ti.R, distance_type=P.VS_L2, default_start=ti.start,
                               storage_type=P._lib.VS_STORAGE_PLAIN)
    ix.bulk_delete(ti.tids[_dead_nodes(ti, 0.3, 5, never=[ti.start])])
    before = ix.download(codes=False, vecs=True)
    want, wmap, wst = _twin(before, {int(ti.start)})
    got, gmap = ix.compact(return_map=True)
    after = ix.download(codes=False, vecs=True)
    _assert_twin(after, got, gmap, want, wmap, wst)
    assert got["edges_cut"] > 0 and ix.desc.default_start == wmap[ti.start] and ix.desc.n == wst["n_after"]
    LC.well_formed(after["nbrs"], ti.R)
    # no consolidation exists for plain storage, so edges were cut: the scans still run, and every row they return is a live row
    # of the compacted arrays under its heap tid
    ai, at, _, _ = ix.search_batch(ti.queries(16, seed=44, kind="gauss"), **SEARCH)
    found = ai != INV
    assert found.any() and (at[found] == after["heap_tids"][ai[found]]).all() and ((at[found] & np.uint64(0xFFFF)) != 0).all()
    ix.close()


# ---- case 10: shrink_to_fit ----------------------------------------------------------------------------------------------------------
# hipMalloc hands out device memory in granules of 2 MiB for allocations of this size: the free memory reported can lag what an
# array gave back by up to one granule
GRANULE = 2 << 20


def test_shrink_to_fit_gives_the_room_back_and_a_later_insert_grows_again(gpu_ctx, oracle):
    ti = _index("general")
    ix = ti.upload(gpu_ctx)
    dead = _dead_nodes(ti, 0.3, 5, never=[ti.start])
    ix.bulk_delete(ti.tids[dead])
    ix.consolidate_deletes()
    ix.compact()
    q = ti.queries(32, seed=44, kind="gauss")
    bi, bt, bd, _ = ix.search_batch(q, **SEARCH)
    gpu_ctx.sync()
    free0 = gpu_ctx.mem_info()[0]
    ix.shrink_to_fit()
    free1 = gpu_ctx.mem_info()[0]
    assert ix.capacity == ix.desc.n == ti.n - dead.size
    if not EMU:  # (the interpreter's "device" reports a constant)
        assert free1 - free0 >= dead.size * ti.dim_full * 4 - GRANULE, (free0, free1)
    ai, at, ad, _ = ix.search_batch(q, **SEARCH)
    assert (ai == bi).all() and (at == bt).all() and (ad.view(np.uint32) == bd.view(np.uint32)).all()
    ix.shrink_to_fit()  # (nothing left to give back)
    X = np.random.default_rng(6).standard_normal((40, ti.dim_full)).astype(np.float32)
    st = ix.insert(X, LC.make_tids(2 * 10 ** 6, 40), search_list_size=48)
    assert st["grew"] == 1 and ix.capacity >= ix.desc.n == ti.n - dead.size + 40
    LC.check_index_everywhere(ix, oracle, ti.distance, q, where="shrunk, grown again")
    ix.close()
