"""vs_index_consolidate_deletes_plain: the consolidation pass over a `plain` storage index ("plain storage").
The rows that name a deleted node take over that node's neighbors, ordered and pruned with the full-precision pair distance of the
plain build.  The reference is `twin` of tests/consolidate_plain_checks.py, the restatement of the SBQ test with
plain_build_checks.PairRule as its distance and prune: neighbor arrays are compared whole with ==, the eight counters as a dict.
Every case asserts its own preconditions on the restatement before it looks at the device.  Also runs on the lockstep interpreter
(tests/test_emu_consolidate_plain.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import plain_build_checks as PB
from consolidate_plain_checks import COUNTERS, WatchedRule, twin
from helpers import make_vectors
from lifecycle_checks import make_tids, well_formed
from oracle import oracle_py as O
from plain_lifecycle_checks import check_plain_everywhere
from oracle import pages_py as PG

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

INV = 0xFFFFFFFF
STATE, INVALID = -5, -1
EMU = bool(os.environ.get("VS_EMU"))
B = PG.BLCKSZ


# ---- corpora, rules, indexes ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _corpus(kind, n, dim, seed):
    X = make_vectors(n, dim, seed, "gauss")
    if kind == "scaled":  # un-normalised rows, so that the cosine divisors matter
        X *= np.random.default_rng(seed).uniform(0.2, 3.0, (n, 1)).astype(np.float32)
    elif kind == "dups":  # three groups of exact copies: of row 5 (rows 40..47), of row 9 (rows 60..62), of row 12 (rows 80, 81)
        X[40:48] = X[5]
        X[60:63] = X[9]
        X[80:82] = X[12]
    else:
        assert kind == "gauss"
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _rule(kind, n, dim, seed, distance, dim_index):
    """one WatchedRule per corpus and geometry: its memo of pair distances is shared by every case over that corpus"""
    O.build()
    return WatchedRule(O, _corpus(kind, n, dim, seed), distance, dim_index)


def _alloc(gpu_ctx, X, *, distance, R, dim_index=None, tids=None, L=32, build=True):
    """a plain index made on the device: vs_index_alloc, the rows, vs_build_graph"""
    import pgvectorscale_amd as P
    n, dim = X.shape
    ix = P.DiskAnnIndex.alloc(gpu_ctx, n=n, dim_full=dim, dim_index=dim_index, num_neighbors=R, distance_type=distance,
                              storage_type=P._lib.VS_STORAGE_PLAIN)
    vp, stride = ix.array(P._lib.ARR_VECS)
    Xp = np.zeros((n, stride), np.float32)
    Xp[:, :dim] = X
    gpu_ctx.upload(vp, Xp)
    gpu_ctx.upload(ix.array(P._lib.ARR_TIDS)[0], np.ascontiguousarray(make_tids(0, n) if tids is None else tids, np.uint64))
    ix.refresh_norms()
    if build:
        ix.build_graph(search_list_size=L, max_alpha=1.2)
    return ix


@functools.lru_cache(maxsize=None)
def _host_graph(kind, n, dim, seed, R):
    """a graph made elsewhere (the oracle's builder over 2-bit codes of the rows): what an uploaded plain index is given"""
    O.build()
    return PB.sbq_graph(O, np.array(_corpus(kind, n, dim, seed)), R, 32)


def _uploaded(gpu_ctx, kind, n, dim, seed, *, distance, R, dim_index=None, tids=None):
    import pgvectorscale_amd as P
    nbrs, start = _host_graph(kind, n, dim, seed, R)
    return P.DiskAnnIndex.upload(gpu_ctx, codes=None, nbrs=nbrs, heap_tids=make_tids(0, n) if tids is None else tids,
                                 vecs=np.array(_corpus(kind, n, dim, seed)), mean=None, m2=None, count=0, bits=1, dim_index=dim_index or dim,
                                 num_neighbors=R, distance_type=distance, default_start=start, storage_type=P._lib.VS_STORAGE_PLAIN)


def _dead(n, frac, seed, must=(), never=()):
    pick = np.random.default_rng(seed).random(n) < frac
    pick[list(must)] = True
    pick[list(never)] = False
    return np.flatnonzero(pick)


def _arrays(ix):
    return ix.download(codes=False, vecs=True)


def _run(ix, rule, dead, *, cand_max=0, repair=False):
    """bulk_delete the tids of `dead`, consolidate -> (before, after, stats, twin rows, twin stats, D, notes)"""
    if len(dead):
        tids = _arrays(ix)["heap_tids"]
        assert ix.bulk_delete(tids[dead])["tuples_removed"] == len(dead)
    before = _arrays(ix)
    want, wst, D, notes = twin(rule, before["nbrs"], before["heap_tids"], ix.desc.default_start, ix.desc.num_neighbors, 1.2, cand_max)
    print("restatement:", wst, "ties in", len(notes["ties"]), "rows, zero distances in", len(notes["zeros"]), "arms", sorted(notes["arms"]))
    got = ix.consolidate_deletes(max_alpha=1.2, cand_max=cand_max, repair=repair, plain=True)
    return before, _arrays(ix), got, want, wst, D, notes


def _same(before, after, got, want, wst):
    assert after["heap_tids"].tobytes() == before["heap_tids"].tobytes()
    assert after["vecs"].tobytes() == before["vecs"].tobytes()
    bad = np.flatnonzero((after["nbrs"] != want).any(1))
    assert bad.size == 0, (bad[:8], after["nbrs"][bad[:1]], want[bad[:1]])
    assert (after["nbrs"] == want).all()
    assert {k: got[k] for k in COUNTERS} == wst
    assert got["unreachable_live"] == INV  # (not judged without the repair pass)


# ---- case 1: rows and counters equal the restatement ---------------------------------------------------------------------------------
GENERAL = dict(n=600, dim=48, seed=18)


def _general(gpu_ctx, distance, R=12):
    """600 x 48 gauss, a device-built graph; for cosine the rows are scaled by 0.2 .. 3, so that their divisors matter"""
    kind = "scaled" if distance == O.COSINE else "gauss"
    X = _corpus(kind, **GENERAL)
    return _alloc(gpu_ctx, X, distance=distance, R=R), _rule(kind, GENERAL["n"], GENERAL["dim"], GENERAL["seed"], distance, 48)


@pytest.mark.parametrize("cand_max", [0, 1024], ids=["default_cap_48", "uncapped"])
@pytest.mark.parametrize("distance", [O.L2, O.COSINE], ids=["l2", "cosine"])
def test_rows_and_counters_equal_the_restatement(gpu_ctx, oracle, distance, cand_max):
    """600 x 48, R = 12, a device-built graph, 30 % deleted, the default start node never.  At the default cap of 48 the union of a
    row outgrows the cap for some rows; cand_max = 1024 is more than the R + R * R = 156 candidates a row can have."""
    ix, rule = _general(gpu_ctx, distance)
    dead = _dead(ix.desc.n, 0.3, 5, never=[ix.desc.default_start])
    before, after, got, want, wst, D, _ = _run(ix, rule, dead, cand_max=cand_max)
    assert wst["rows_pruned"] > 0 and wst["rows_rewritten"] > 200
    if cand_max:
        assert wst["rows_capped"] == 0
    else:
        assert wst["rows_capped"] > 0
    _same(before, after, got, want, wst)
    assert (after["nbrs"][D] == before["nbrs"][D]).all()  # rows of D are never written
    ix.close()


# ---- case 2: geometry edges ----------------------------------------------------------------------------------------------------------
# R = 70: the row loops (one ballot per 64 entries) run past one wave and the default cap is 256; gathered counts that are no
# multiple of 8 leave the last eight-lane pass of the key loop partly idle (asserted below on the input).
@pytest.mark.parametrize("R", [4, 24, 70])
@pytest.mark.parametrize("dim,dim_index,distance", [(8, 8, O.L2), (40, 40, O.L2), (64, 64, O.L2), (40, 24, O.COSINE)],
                         ids=["8", "40", "64", "40_24_cosine"])
def test_geometry_edges(gpu_ctx, oracle, dim, dim_index, distance, R):
    n = 200
    X = _corpus("scaled", n, dim, 31 + dim)
    ix = _alloc(gpu_ctx, X, distance=distance, R=R, dim_index=dim_index, L=max(32, 2 * R))
    rule = _rule("scaled", n, dim, 31 + dim, distance, dim_index)
    dead = _dead(n, 0.3 if R < 70 else 0.15, 6 + R, never=[ix.desc.default_start])
    before, after, got, want, wst, D, _ = _run(ix, rule, dead)
    lens = (before["nbrs"] != INV).sum(1)
    assert wst["rows_rewritten"] > 20 and wst["rows_pruned"] > 0 and (lens[D] % 8 != 0).any()
    if R == 70:
        assert lens.max() > 64
    _same(before, after, got, want, wst)
    ix.close()


# ---- case 3: ties and zero distances -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distance", [O.L2, O.COSINE], ids=["l2", "cosine"])
def test_ties_and_zero_distances(gpu_ctx, oracle, distance):
    """exact copies of rows, copies of p among p's own candidates included: equal keys are ordered by id, and both arms of the
    FLT_EPSILON rule of PlainPair::factor are taken (a copy of p scored against another copy of p; a copy of another row scored
    against that row)"""
    n, dim, R = 200, 40, 6
    ix = _uploaded(gpu_ctx, "dups", n, dim, 77, distance=distance, R=R)
    rule = _rule("dups", n, dim, 77, distance, dim)
    # The first row of each group is deleted.  Its copies name it (equal codes) and take over its list, which names them; a row
    # outside a group names at most the group's lowest id (the builder's prune drops the copies behind it), so deleting that one is
    # what puts several copies of one row among the candidates of an outside row.
    copies = [*range(40, 48), *range(60, 63), 80, 81]
    dead = _dead(n, 0.25, 3, must=[5, 9, 12], never=[ix.desc.default_start, *copies])
    before, after, got, want, wst, D, notes = _run(ix, rule, dead, cand_max=64)
    assert notes["ties"], "a rewritten row must have candidates at equal distance"
    assert notes["zeros"], "a rewritten row must have a candidate at a zero pair distance"
    assert notes["arms"] == {"one", "fmax"}, notes["arms"]
    assert wst["rows_pruned"] > 0
    _same(before, after, got, want, wst)
    ix.close()


# ---- case 4: structure ---------------------------------------------------------------------------------------------------------------
def test_a_deleted_default_start_node_stays_in_the_graph(gpu_ctx, oracle):
    ix, rule = _general(gpu_ctx, O.L2)
    s = int(ix.desc.default_start)
    before, after, got, want, wst, D, _ = _run(ix, rule, _dead(ix.desc.n, 0.3, 7, must=[s]))
    assert not D[s] and wst["tombstones_kept"] == 1 and D[before["nbrs"][s][before["nbrs"][s] != INV]].any()
    _same(before, after, got, want, wst)
    assert (after["nbrs"][s] != before["nbrs"][s]).any() and not D[after["nbrs"][s][after["nbrs"][s] != INV]].any()
    ix.close()


def test_a_node_whose_neighbors_are_all_deleted(gpu_ctx, oracle):
    ix, rule = _general(gpu_ctx, O.L2)
    nb = _arrays(ix)["nbrs"]
    s = int(ix.desc.default_start)
    p = next(i for i in range(300, ix.desc.n) if i != s and (nb[i] != INV).sum() >= 6 and s not in nb[i])
    dead = np.array(sorted(set(int(v) for v in nb[p] if v != INV) - {p}))
    before, after, got, want, wst, D, _ = _run(ix, rule, dead)
    assert D[before["nbrs"][p][before["nbrs"][p] != INV]].all()
    _same(before, after, got, want, wst)
    new = after["nbrs"][p][after["nbrs"][p] != INV]
    assert new.size > 0 and not (set(new.tolist()) & set(dead.tolist()))
    ix.close()


def test_a_whole_neighborhood_is_deleted(gpu_ctx, oracle):
    """a node's neighbors and theirs: the node, left alive, finds nothing to take over — a tombstone's tombstones are not followed"""
    ix, rule = _general(gpu_ctx, O.L2)
    nb = _arrays(ix)["nbrs"]
    s = int(ix.desc.default_start)
    hood = lambda xs: set(int(v) for x in xs for v in nb[x] if v != INV)
    p = next(i for i in range(400, ix.desc.n) if i != s and s not in hood(hood([i]) | {i}))
    dead = np.array(sorted((hood([p]) | hood(hood([p]))) - {p}))
    before, after, got, want, wst, D, _ = _run(ix, rule, dead)
    assert wst["rows_emptied"] >= 1 and dead.size < ix.desc.n // 2
    # (following a second level would find live rows: some tombstone of the second ring names a kept node other than p)
    assert any((~D[nb[d][nb[d] != INV]]).any() for d in hood(hood([p])) - {p})
    _same(before, after, got, want, wst)
    assert (after["nbrs"][p] == INV).all()
    # with the repair pass the emptied row's node is still reachable
    assert ix.consolidate_deletes(plain=True)["unreachable_live"] == 0
    ix.close()


def test_nothing_deleted_nothing_changes_and_a_second_call_rewrites_nothing(gpu_ctx, oracle):
    ix, rule = _general(gpu_ctx, O.COSINE)
    before, after, got, want, wst, _, _ = _run(ix, rule, np.zeros(0, np.int64))
    assert all(got[k] == 0 for k in COUNTERS) and all(after[k].tobytes() == before[k].tobytes() for k in ("nbrs", "heap_tids", "vecs"))
    ix.bulk_delete(before["heap_tids"][_dead(ix.desc.n, 0.3, 8, never=[ix.desc.default_start])])
    first = ix.consolidate_deletes(repair=False, plain=True)
    once = _arrays(ix)
    again = ix.consolidate_deletes(repair=False, plain=True)
    assert first["rows_rewritten"] > 0 and again["tombstones"] == first["tombstones"]
    assert all(again[k] == 0 for k in COUNTERS if k not in ("tombstones", "tombstones_kept"))
    assert _arrays(ix)["nbrs"].tobytes() == once["nbrs"].tobytes()
    ix.close()


# ---- case 5: the full call ------------------------------------------------------------------------------------------------------------
def _scans_equal_the_oracle(ix, q, *, distance, dim_index, L=40, rescore=50, k=10):
    """every plain entry point against the oracle over the arrays as they stand (check_plain_everywhere: both search kernels and the
    hand-over, stream, cursor, pools, brute force); then the default batch once more for what this file adds -> its ids"""
    assert ix.desc.dim_index == dim_index
    host, oidx = check_plain_everywhere(ix, O, distance, q, where="after the consolidation")
    gi, gt, gd, gst = ix.search_batch(q, search_list_size=L, rescore=rescore, k=k)
    oi, od, ost = oidx.search_batch(q, L=L, rescore=rescore, k=k)
    assert (gi == oi).all() and (gd.view(np.uint32) == od.view(np.uint32)).all() and gst["visited_nodes"] == ost["visited_nodes"]
    found = gi != INV
    assert found.any() and (gt[found] == host["heap_tids"][gi[found]]).all()
    assert ((gt[found] & np.uint64(0xFFFF)) != 0).all(), "a deleted row was returned"
    return gi


@pytest.mark.parametrize("distance", [O.L2, O.COSINE], ids=["l2", "cosine"])
def test_after_the_full_call_compaction_cuts_nothing_and_scans_equal_the_oracle(gpu_ctx, oracle, distance):
    ix, rule = _general(gpu_ctx, distance)
    n = ix.desc.n
    dead = _dead(n, 0.3, 5, never=[ix.desc.default_start])
    before, after, got, want, wst, D, _ = _run(ix, rule, dead, repair=True)
    assert {k: got[k] for k in COUNTERS} == wst and got["unreachable_live"] == 0
    named = after["nbrs"][~D]
    assert not D[named[named != INV]].any()
    assert (after["nbrs"][D] == before["nbrs"][D]).all()
    q = make_vectors(32, 48, 44, "gauss")
    gi = _scans_equal_the_oracle(ix, q, distance=distance, dim_index=48)
    assert not (set(gi.ravel().tolist()) & set(dead.tolist()))
    st = ix.compact(check_edges=True)
    assert st["edges_cut"] == 0 and ix.desc.n == n - dead.size
    _scans_equal_the_oracle(ix, q, distance=distance, dim_index=48)
    ix.close()


# ---- case 6: lifecycle on a device-made index -----------------------------------------------------------------------------------------
def _relation_of(ix):
    """the oracle's plain writer over the arrays of an L2 index as they are on the device now"""
    host = _arrays(ix)
    d = ix.desc
    meta = dict(storage_type=0, num_dimensions=d.dim_full, num_dimensions_to_index=d.dim_index, bq_num_bits_per_dimension=d.bits,
                distance_type=d.distance_type, num_neighbors=d.num_neighbors,
                default_start=None if d.default_start == INV else int(d.default_start), labeled_starts={}, extension_version="0.8.0",
                search_list_size=100, max_alpha=1.2)
    return PG.write_plain_index(vectors=host["vecs"][:, :d.dim_index], nbrs=host["nbrs"], heap_tids=host["heap_tids"],
                                num_neighbors=d.num_neighbors, meta=meta).rel.tobytes()


def test_lifecycle_on_a_device_made_index(gpu_ctx, oracle):
    """alloc -> build -> insert -> bulk_delete -> consolidate -> compact -> insert into the freed room -> write_pages"""
    n0, m1, m2, dim, R = 400, 60, 50, 48, 16
    X = make_vectors(n0 + m1 + m2, dim, 61, "gauss")
    tids = make_tids(0, n0 + m1 + m2)
    ix = _alloc(gpu_ctx, X[:n0], distance=O.L2, R=R, tids=tids[:n0])
    st = ix.insert(X[n0:n0 + m1], tids[n0:n0 + m1], search_list_size=32, max_alpha=1.2)
    assert st["inserted"] == m1 and st["orphans_left"] == 0
    n1 = n0 + m1
    dead = _dead(n1, 0.3, 9, never=[ix.desc.default_start])
    assert ix.bulk_delete(tids[dead])["tuples_removed"] == dead.size
    st = ix.consolidate_deletes(plain=True)
    assert st["rows_rewritten"] > 0 and st["unreachable_live"] == 0
    cap = ix.capacity
    st = ix.compact(check_edges=True)
    assert st["edges_cut"] == 0 and ix.desc.n == n1 - dead.size and dead.size >= m2
    st = ix.insert(X[n1:], tids[n1:], search_list_size=32, max_alpha=1.2)
    assert st["inserted"] == m2 and st["orphans_left"] == 0 and st["grew"] == 0 and ix.capacity == cap  # (the freed room took them)
    host = _arrays(ix)
    alive = np.setdiff1d(np.arange(n1), dead)
    assert (host["vecs"] == np.concatenate([X[alive], X[n1:]])).all() and (host["heap_tids"] == np.concatenate([tids[alive], tids[n1:]])).all()
    well_formed(host["nbrs"], R)
    want = _relation_of(ix)
    got = ix.write_pages(plain=True)
    assert got == want, "the written relation differs from the oracle's plain writer"
    _scans_equal_the_oracle(ix, make_vectors(32, dim, 45, "gauss"), distance=O.L2, dim_index=dim)
    ix.close()


# ---- case 7: an uploaded plain index ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dim_index,distance", [(48, 48, O.L2), (40, 24, O.COSINE)], ids=["l2", "cosine_truncated"])
def test_an_uploaded_plain_index_is_accepted(gpu_ctx, oracle, dim, dim_index, distance):
    """the index mirrors a relation (a graph made elsewhere): its rows equal the restatement, only neighbor lists change, and the
    plain page writer still takes it.  The cosine index keeps divisors of its 24-dimension slices next to those of the whole rows."""
    from pgvectorscale_amd.pages import PagesOut
    n, R = 300, 12
    ix = _uploaded(gpu_ctx, "scaled", n, dim, 52, distance=distance, R=R, dim_index=dim_index)
    rule = _rule("scaled", n, dim, 52, distance, dim_index)
    before, after, got, want, wst, D, _ = _run(ix, rule, _dead(n, 0.3, 4, never=[ix.desc.default_start]))
    assert wst["rows_pruned"] > 0 and wst["rows_rewritten"] > 100
    _same(before, after, got, want, wst)
    out = PagesOut(ix, plain=True)
    assert out.n_blocks > 1
    out.close()
    ix.close()


# ---- case 8: refusals ------------------------------------------------------------------------------------------------------------------
def _bytes(ix):
    h = ix.download(codes=ix.desc.storage_type != 0, nbrs=True, tids=True, vecs=True)
    return b"".join(h[k].tobytes() for k in ("codes", "nbrs", "heap_tids", "vecs") if h[k] is not None), ix.desc.n, ix.desc.default_start


def _refused(ix, code, call=None, word=None, on=None):
    import pgvectorscale_amd as P
    on = on or ix
    before = _bytes(ix)
    with pytest.raises(P._lib.VsError) as e:
        (call or (lambda h: h.consolidate_deletes(plain=True)))(on)
    assert e.value.code == code, str(e.value)
    assert word is None or word in str(e.value), str(e.value)
    assert _bytes(ix) == before
    return str(e.value)


def test_refusals_leave_every_byte_as_it_was(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    from helpers import TestIndex
    from pgvectorscale_amd.pages import PagesOut
    n, dim, R = 300, 48, 12
    ix = _uploaded(gpu_ctx, "scaled", n, dim, 52, distance=O.L2, R=R)
    ix.bulk_delete(make_tids(0, n)[_dead(n, 0.3, 10, never=[ix.desc.default_start])])
    # arguments
    cons = lambda **kw: (lambda h: h.consolidate_deletes(plain=True, **kw))
    _refused(ix, INVALID, cons(cand_max=R), "cand_max")
    _refused(ix, INVALID, cons(cand_max=1025), "cand_max")
    _refused(ix, INVALID, cons(max_alpha=0.5), "max_alpha")
    _refused(ix, INVALID, cons(max_alpha=5.5), "max_alpha")
    _refused(ix, INVALID, lambda h: P._lib.check(h._L.vs_index_consolidate_deletes_plain(h.h, 1.2, 0, 2, None)), "flags")
    # the SBQ call keeps refusing the plain index, and now names the call that takes it
    msg = _refused(ix, INVALID, lambda h: h.consolidate_deletes(), "plain")
    assert "vs_index_consolidate_deletes_plain" in msg
    # state: an open plain writer, a view (the owner and the view handle), a batch in flight
    out = PagesOut(ix, plain=True)
    _refused(ix, STATE, word="writer")
    out.close()
    ctx2 = P.Context(0)
    view = ix.view(ctx2)
    _refused(ix, STATE, word="view")
    _refused(ix, STATE, word="view", on=view)
    view.close()
    ctx2.close()
    q = make_vectors(8, dim, 1, "gauss")
    dq, d_ids = gpu_ctx.alloc(q.nbytes), gpu_ctx.alloc(len(q) * 10 * 4)
    gpu_ctx.upload(dq, q)
    ix.search_batch_dev(dq, len(q), 40, 20, 10, d_ids)
    try:
        _refused(ix, STATE, word="in flight")
    finally:
        ix.search_batch_dev_finish()
        gpu_ctx.free(dq)
        gpu_ctx.free(d_ids)
    # (the writer, the view and the batch are gone: the call goes through)
    assert ix.consolidate_deletes(plain=True)["rows_rewritten"] > 0
    ix.close()
    # an SBQ index: the message names the call that takes it
    ti = TestIndex(n=200, dim_full=32, bits=2, R=8, distance=O.L2, seed=9, kind="gauss", L_build=20)
    sbq = ti.upload(gpu_ctx)
    sbq.bulk_delete(ti.tids[_dead(ti.n, 0.3, 11, never=[ti.start])])
    msg = _refused(sbq, INVALID)
    assert "vs_index_consolidate_deletes " in msg.replace("vs_index_consolidate_deletes_plain", "")
    assert sbq.consolidate_deletes()["rows_rewritten"] > 0
    sbq.close()
    # what the pair distance cannot score: the inner product.  (An index without the vector column, or a cosine index with dim_index <
    # dim_full without divisors of its slices, does not come into being through vs_index_alloc, vs_index_upload or the page reader.)
    nbrs, start = _host_graph("scaled", n, dim, 52, R)
    tids = make_tids(0, n)
    tids[5] &= ~np.uint64(0xFFFF)
    ip = P.DiskAnnIndex.upload(gpu_ctx, codes=None, nbrs=nbrs, heap_tids=tids, vecs=np.array(_corpus("scaled", n, dim, 52)), mean=None,
                               m2=None, count=0, bits=1, dim_index=dim, num_neighbors=R, distance_type=P.VS_IP, default_start=start,
                               storage_type=P._lib.VS_STORAGE_PLAIN)
    _refused(ip, INVALID, word="inner-product")
    ip.close()
    # a layout beyond 160 KiB of LDS: 41 000 dimensions are 164 000 bytes of prepared vector alone
    wide = np.zeros((6, 4), np.uint32) + INV
    for i in range(6):
        wide[i, :3] = [(i + 1) % 6, (i + 2) % 6, (i + 3) % 6]
    tids = make_tids(0, 6)
    tids[2] &= ~np.uint64(0xFFFF)
    big = P.DiskAnnIndex.upload(gpu_ctx, codes=None, nbrs=wide, heap_tids=tids, vecs=make_vectors(6, 41000, 3, "gauss"), mean=None, m2=None,
                                count=0, bits=1, dim_index=41000, num_neighbors=4, distance_type=P.VS_L2, default_start=0,
                                storage_type=P._lib.VS_STORAGE_PLAIN)
    _refused(big, INVALID, word="LDS")
    big.close()


# ---- case 9: with the delta writer ---------------------------------------------------------------------------------------------------
def test_delta_after_a_consolidation_names_exactly_the_pages_of_the_changed_nodes(gpu_ctx, oracle, tmp_path):
    from pgvectorscale_amd.pages import PagesOut
    n, dim, R = 700, 48, 16  # 22 items per page, 32 node pages
    ix = _uploaded(gpu_ctx, "gauss", n, dim, 31, distance=O.L2, R=R)
    tids = make_tids(0, n)
    path = tmp_path / "rel"
    out = PagesOut(ix, plain=True)
    out.write_file(str(path))
    base = out.baseline()
    old = path.read_bytes()
    out.close()
    before = _arrays(ix)
    # two deleted nodes with few in-edges, so that fewer rows change than the relation has node pages
    nb = before["nbrs"]
    indeg = np.bincount(nb[nb != INV], minlength=n)
    dead = np.array([i for i in range(100, n) if i != ix.desc.default_start and 4 <= indeg[i] <= 12][:2])
    assert dead.size == 2 and indeg[dead].sum() + 2 < 30
    ix.bulk_delete(tids[dead])
    st = ix.consolidate_deletes(plain=True)
    after = _arrays(ix)
    changed = np.flatnonzero((after["heap_tids"] != before["heap_tids"]) | (after["nbrs"] != before["nbrs"]).any(1))
    assert st["rows_rewritten"] > 0 and set(dead.tolist()) < set(changed.tolist())
    out = PagesOut(ix, plain=True)
    want_blocks = sorted(set(out.item_pointer_of(int(i))[0] for i in changed))
    blocks, nb_now, new_base = out.delta(base)
    fresh = out.read().tobytes()
    node_blocks = set(out.item_pointer_of(i)[0] for i in range(n))
    meta_changed = [b for b in range(out.n_blocks) if b not in node_blocks and fresh[b * B:(b + 1) * B] != old[b * B:(b + 1) * B]]
    assert blocks.tolist() == sorted(want_blocks + meta_changed) and nb_now == out.n_blocks == len(old) // B
    assert len(want_blocks) < len(node_blocks), "some node page must have stayed clean"
    third = out.patch_file(str(path), base)
    assert path.read_bytes() == fresh == _relation_of(ix)
    for b in (base, new_base, third):
        b.close()
    out.close()
    ix.close()


# ---- case 10: quality ------------------------------------------------------------------------------------------------------------------
QUALITY = dict(n=1500, dim=48, nq=256, R=16, L=32, seed=9, share=0.3, dead_seed=12)


def quality_setup():
    """the quality shape of tests/test_gpu_zy_plain_build.py, its deleted rows, and the exact top-10 over the live rows"""
    c = QUALITY
    X = make_vectors(c["n"], c["dim"], c["seed"], "gauss")
    Q = make_vectors(c["nq"], c["dim"], c["seed"] + 100, "gauss")
    dead = _dead(c["n"], c["share"], c["dead_seed"], never=[0])  # (node 0 is the default start of a device build)
    alive = np.setdiff1d(np.arange(c["n"]), dead)
    return X, Q, dead, alive, PB.exact_top10(X[alive], Q)


@pytest.mark.skipif(EMU, reason="two 1 500-row device builds: hardware only, as the SBQ quality case")
def test_a_consolidated_graph_is_as_good_as_one_rebuilt_over_the_live_rows(gpu_ctx, oracle):
    """recall@10 of the oracle's plain search at L = 32 (256 queries, exact f32 top-10 over the live rows): the consolidated and
    compacted graph against vs_build_graph over the live 70 % alone, within SEQ_RECALL_SPREAD of plain_build_checks (the
    seed-to-seed spread recorded for this shape).  The same comparison with the restatement's rows (no repair pass) in place of the
    kernel's, on the graph the wave64 interpreter builds for this seed and the 30 % share (468 rows), gave 0.925781 against 0.923438
    for the interpreter's build over the live rows: inside the margin of 0.009375, so the share stays at 30 %.  Both recalls are
    printed."""
    c = QUALITY
    X, Q, dead, alive, truth = quality_setup()
    tids = make_tids(0, c["n"])
    ix = _alloc(gpu_ctx, X, distance=O.L2, R=c["R"], tids=tids, L=c["L"])
    assert ix.desc.default_start == 0
    ix.bulk_delete(tids[dead])
    st = ix.consolidate_deletes(plain=True)
    assert st["unreachable_live"] == 0 and st["rows_rewritten"] > 0
    assert ix.compact(check_edges=True)["edges_cut"] == 0
    host = _arrays(ix)
    assert (host["vecs"] == X[alive]).all()
    r_cons = PB.recall_at_10(oracle, X[alive], host["nbrs"], ix.desc.default_start, Q, truth, c["L"])
    ix.close()
    base = _alloc(gpu_ctx, np.ascontiguousarray(X[alive]), distance=O.L2, R=c["R"], L=c["L"])
    r_base = PB.recall_at_10(oracle, X[alive], base.download(codes=False)["nbrs"], base.desc.default_start, Q, truth, c["L"])
    base.close()
    print(f"recall@10: consolidated {r_cons:.4f}, rebuilt over the live rows {r_base:.4f}, margin {PB.SEQ_RECALL_SPREAD}", st)
    assert r_cons >= r_base - PB.SEQ_RECALL_SPREAD
