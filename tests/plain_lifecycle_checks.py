"""The plain twin of lifecycle_checks.check_index_everywhere: one checker for a device-resident `plain` storage index in whatever
state a chain of inserts, deletes, consolidations, compactions, reserves, shrinks or followed page lists left it
(tests/test_gpu_zw_plain_lifecycle.py).  check_plain_everywhere downloads the arrays once, builds the oracle over exactly those
arrays (storage_plain=True) and holds EVERY plain entry point to it: the batched search on k_search_plain and on the general kernel,
the hand-over between the two, the stream, the amgettuple cursor, a scan pool on either of its kernels (created here, i.e. after
the mutation, as include/vsgpu.h requires of a plain pool), the stored snapshots, qualified scans, the brute force and — where asked
for — the page writer.  Every expectation is the oracle's or a numpy restatement written here; nothing compares the library with
itself.

What a visibility mask means here is the reference's: a plain scan fetches the heap only inside next_with_resort, i.e. when
num_dimensions_to_index < num_dimensions (AM/scan.rs:392-401); with every dimension indexed no mask hides anything, on the oracle
and on the device alike.  So the precondition "the mask hides a row the unmasked batch returned" is asserted where a mask can act
(dim_index < dim_full); elsewhere the rows under the mask are still held to the oracle's, which ignores it."""
import ctypes as C

import numpy as np

from lifecycle_checks import (CURSOR, INV, OFFSET, _same_bits, check_pool_slot, check_qualifier, cosine_divisors, make_tids,  # noqa: F401
                              pull_and_compare, regime, well_formed)
from test_gpu_zx_vis_overlay import PLAIN_COUNTERS
from test_gpu_zy_plain_pool import COUNTERS as PLAIN_CURSOR_KEYS

GENERAL, FAST_SBQ, FAST_PLAIN = 0, 1, 2
SEARCH = dict(L=40, rescore=20, k=10)    # rescore only acts when dim_index < dim_full: then the window runs
SHORT_QUERIES = 2                        # ... of which this many also run with k = n + 3: no scan can return that many rows
STREAM = dict(L=40, m=35)
HAND_OVER = {"VS_PF_VISITED": "20"}      # a visited list of 20 nodes at L = 40: scans outgrow it and are handed over whole
POOL = dict(slots=2, k=16, rounds=3, rows_cap=1024)


def oracle_plain(O, host, *, distance, dim_index, R, start, visible=None):
    """the oracle over downloaded arrays: a plain index has no codes, so their place is held by zeros of the right width"""
    n = host["vecs"].shape[0]
    w = (dim_index + 63) // 64
    return O.OracleIndex(codes=np.zeros((n, w), np.uint64), nbrs=host["nbrs"], heap_tids=host["heap_tids"], vecs=host["vecs"],
                         mean=np.zeros(dim_index, np.float32), m2=np.zeros(dim_index, np.float32), count=0, bits=1, dim_index=dim_index,
                         num_neighbors=R, distance_type=distance, default_start=start, storage_plain=True, visible=visible)


def node_vectors(O, vecs, dim_index, distance):
    """PlainNode.vector: the first dim_index floats of the row, under cosine the oracle's preprocess_cosine of that slice"""
    out = np.ascontiguousarray(vecs[:, :dim_index], np.float32).copy()
    if distance == O.COSINE:
        for i in range(out.shape[0]):
            out[i] = O.preprocess_cosine(out[i])[0]
    return out


def relation_of(O, ix, host, distance):
    """the oracle's plain writer over the downloaded arrays -> the relation's bytes"""
    from oracle import pages_py as PG
    d = ix.desc
    meta = dict(storage_type=0, num_dimensions=d.dim_full, num_dimensions_to_index=d.dim_index, bq_num_bits_per_dimension=d.bits,
                distance_type=distance, num_neighbors=d.num_neighbors, default_start=None if d.default_start == INV else int(d.default_start),
                labeled_starts={}, extension_version="0.8.0", search_list_size=100, max_alpha=1.2)
    return PG.write_plain_index(vectors=node_vectors(O, host["vecs"], d.dim_index, distance), nbrs=host["nbrs"], heap_tids=host["heap_tids"],
                                num_neighbors=d.num_neighbors, meta=meta).rel.tobytes()


def _search_keys(ix):
    """PLAIN_COUNTERS, and next_calls where tests/test_gpu_zy_plain.py compares it: with every dimension indexed"""
    return PLAIN_COUNTERS + (("next_calls",) if ix.desc.dim_index == ix.desc.dim_full else ())


def check_search(ix, ref, q, k, want_kernel, where, env=None, handed_over=None):
    """ref = (the oracle index, its search_batch of these queries at this k).  ids exact, heap tids those of the rows, distance
    bits, the counters the plain kernels share with the oracle, which kernel ran; handed_over False: no scan may leave
    k_search_plain, True: at least one must -> ids"""
    oidx, (oi, od, ost) = ref
    with regime(env or {}):
        gi, gt, gd, gst = ix.search_batch(q, search_list_size=SEARCH["L"], rescore=SEARCH["rescore"], k=k)
        info = ix.last_search_info()
    assert info["kernel"] == want_kernel, (where, info)
    assert (gi == oi).all(), (where, np.flatnonzero((gi != oi).any(1))[:4])
    assert _same_bits(gd, od), where
    found = gi != INV
    assert (gt[found] == oidx.heap_tids[gi[found]]).all(), where
    for key in _search_keys(ix):
        assert gst[key] == ost[key], (where, key, gst[key], ost[key])
    assert gst["quantized_distance_comparisons"] == 0, where
    if handed_over is False:
        assert gst["fallback_scans"] == 0, (where, gst["fallback_scans"])
    if handed_over is True:
        assert gst["fallback_scans"] > 0 and gst["fallback_visited_nodes"] > 0, (where, "the knob handed no scan over: nothing was tested")
    return gi


def oracle_batch(oidx, q, k):
    """the reference of a batch, computed once for every kernel it is compared with (under the mask in force on the oracle NOW)"""
    return oidx, oidx.search_batch(q, L=SEARCH["L"], rescore=SEARCH["rescore"], k=k)


def check_searches(ix, oidx, q, where, short=True):
    """the batch on k_search_plain, on the general kernel, and with scans handed over from the one to the other; the first queries
    once more with k beyond what the index holds, so that short rows are compared too"""
    n = ix.desc.n
    fast, general = {"VS_PLAIN_FAST": "1"}, {"VS_PLAIN_FAST": "0"}
    ref = oracle_batch(oidx, q, SEARCH["k"])
    check_search(ix, ref, q, SEARCH["k"], FAST_PLAIN, (where, "k_search_plain"), fast, handed_over=False)
    check_search(ix, ref, q, SEARCH["k"], GENERAL, (where, "general kernel"), general)
    if not short:
        return
    check_search(ix, ref, q, SEARCH["k"], FAST_PLAIN, (where, "hand-over"), dict(fast, **HAND_OVER), handed_over=True)
    ref = oracle_batch(oidx, q[:SHORT_QUERIES], n + 3)
    for env, kernel in ((fast, FAST_PLAIN), (general, GENERAL)):
        gi = check_search(ix, ref, q[:SHORT_QUERIES], n + 3, kernel, (where, "short rows", kernel), env)
        assert (gi[:, -3:] == INV).all(), where


def check_stream(ix, oidx, q, where):
    """ids, and the graph distances: on plain storage the oracle's stream hands back the f32 distance it scored, bit for bit"""
    gi, gd, gst = ix.stream_batch(q, search_list_size=STREAM["L"], m=STREAM["m"])
    oi, od, ost = oidx.stream_batch(q, L=STREAM["L"], m=STREAM["m"])
    assert (gi == oi).all(), (where, np.flatnonzero((gi != oi).any(1))[:4])
    found = gi != INV
    assert (gd[found] == od[found]).all(), (where, "the graph distances are the f32 distance bits")
    for key in PLAIN_CURSOR_KEYS:
        assert gst[key] == ost[key], (where, key, gst[key], ost[key])


def check_cursor(ix, oidx, query, where, null_query=True):
    """70 rows one gettuple at a time with a list of 10, stats at the checkpoints; then a NULL query drained to its end"""
    scan = ix.beginscan()
    try:
        scan.rescan(query, search_list_size=CURSOR["L"], rescore=CURSOR["rescore"])
        pulled = pull_and_compare(scan, oidx.scan(query, L=CURSOR["L"], rescore=CURSOR["rescore"]), where=(where, "cursor"), keys=PLAIN_CURSOR_KEYS)
        if not null_query:
            return pulled
        scan.rescan(None, search_list_size=CURSOR["L"], rescore=CURSOR["rescore"])
        oscan = oidx.scan(None, L=CURSOR["L"], rescore=CURSOR["rescore"])
        n = ix.desc.n
        pulled = pull_and_compare(scan, oscan, rows=n + 1, checkpoints=(), where=(where, "NULL query"))
        assert pulled <= n and scan.gettuple() is None and oscan.gettuple() is None, (where, "NULL query", pulled)
        g, ref = scan.stats(), oscan.stats()
        for key in PLAIN_CURSOR_KEYS:
            assert g[key] == ref[key], (where, "NULL query", key, g[key], ref[key])
        return pulled
    finally:
        scan.endscan()


def check_pools(ix, oidx, queries, where):
    """a pool made NOW on each of its two kernels: every slot hands out the oracle's rows and stats, chunk after chunk"""
    import pgvectorscale_amd as P
    for fast, kernel in (("1", FAST_PLAIN), ("0", GENERAL)):
        with regime({"VS_POOL_PLAIN_FAST": fast}):
            pool = P.ScanPool(ix, POOL["slots"], search_list_size=CURSOR["L"], rescore=CURSOR["rescore"], kmax=POOL["k"], rows_cap=POOL["rows_cap"])
        try:
            assert pool.info()["kernel"] == kernel, (where, fast, pool.info())
            for slot in range(POOL["slots"]):
                pool.rescan(slot, queries[slot])
            for slot in range(POOL["slots"]):  # (check_pool_slot refuses a negative row count: VS_ERR_CAPACITY is one)
                check_pool_slot(pool, slot, oidx.scan(queries[slot], L=CURSOR["L"], rescore=CURSOR["rescore"]), POOL["k"], POOL["rounds"],
                                (where, "pool", kernel, slot), keys=PLAIN_CURSOR_KEYS)
        finally:
            pool.close()


def check_pages(ix, O, distance, q, host, oidx, where):
    """check 9: the written relation is the oracle writer's, byte for byte (under cosine with dim_index < dim_full this is what pins
    the slice divisors: the writer divides by them); staged again it is an index that searches like the oracle"""
    from pgvectorscale_amd.pages import IndexPages
    want = relation_of(O, ix, host, distance)
    got = ix.write_pages(plain=True)
    B = 8192
    assert got == want, (where, "written relation", [b for b in range(min(len(got), len(want)) // B) if got[b * B:(b + 1) * B] != want[b * B:(b + 1) * B]][:4])
    rd = IndexPages(plain=True)
    rd.add(got)
    info = rd.finish()
    assert info.n_nodes == ix.desc.n, where
    _, d, _ = rd.meta()
    back = rd.upload_plain(ix.ctx, distance_type=distance, default_start=int(d.default_start), vecs=host["vecs"])
    rd.close()
    held = oidx.visible
    try:
        oidx.set_visibility(None)
        check_search(back, oracle_batch(oidx, q, SEARCH["k"]), q, SEARCH["k"], FAST_PLAIN, (where, "staged again from the written pages"))
    finally:
        oidx.set_visibility(held)
        back.close()


def check_plain_everywhere(ix, O, distance, q, *, visible=None, snapshots=None, qualifier=None, pages=False, where=""):
    """ix: a live plain DiskAnnIndex; O: the oracle module; q: queries [nq][dim_full], the last four near rows of a later insert.
    visible: the mask the test put in force with set_visibility, as it must stand NOW (uint8 [n]); snapshots: {id: mask as it must
    stand now}; qualifier: (slot, the bits it was filled with — shorter than n when rows were added since); pages: also check 9 (L2
    and cosine only).  -> (downloaded arrays, the OracleIndex)"""
    from pgvectorscale_amd import _lib
    ix._refresh()
    d = ix.desc
    n, R = d.n, d.num_neighbors
    assert d.storage_type == _lib.VS_STORAGE_PLAIN and n > 0, where
    truncated = d.dim_index < d.dim_full
    host = ix.download(codes=False, vecs=True)
    oidx = oracle_plain(O, host, distance=distance, dim_index=d.dim_index, R=R, start=d.default_start)

    # -- arrays (vs_index_array does not expose the slice divisors: the scans below and check 9 hold them)
    well_formed(host["nbrs"], R)
    assert ix.capacity >= n, where
    vn_ptr = ix.array(_lib.ARR_VNORM)[0]
    assert vn_ptr.value or distance != O.COSINE, where
    if distance == O.COSINE:
        vnorm = ix.ctx.download(vn_ptr, np.empty(n, np.float32))
        assert vnorm.tobytes() == cosine_divisors(host["vecs"]).tobytes(), (where, "cosine divisors")

    # -- the mask in force: on the oracle too, from the batched search to the pool
    if visible is not None:
        visible = np.ascontiguousarray(visible, np.uint8)
        assert visible.shape == (n,), where
        if truncated:
            oi = oidx.search_batch(q, L=SEARCH["L"], rescore=SEARCH["rescore"], k=SEARCH["k"])[0]
            assert (visible[oi[oi != INV]] == 0).any(), (where, "the mask hides no row the unmasked batch returned")
    oidx.set_visibility(visible)
    check_searches(ix, oidx, q, where)
    check_stream(ix, oidx, q, (where, "stream"))
    check_cursor(ix, oidx, q[0], where)
    check_pools(ix, oidx, (q[1], q[len(q) - 1]), where)
    if qualifier is not None:
        check_qualifier(ix, oidx, q, qualifier, where)

    # -- the stored snapshots
    for sid, smask in sorted((snapshots or {}).items()):
        assert np.asarray(smask).shape == (n,), where
        prev = C.c_void_p()
        _lib.check(ix._L.vs_index_snapshot_use(ix.h, sid, C.byref(prev)))
        try:
            oidx.set_visibility(smask)
            check_searches(ix, oidx, q, (where, "snapshot", sid), short=False)
            check_cursor(ix, oidx, q[0], (where, "snapshot cursor", sid), null_query=False)
        finally:
            _lib.check(ix._L.vs_index_set_visibility_dev(ix.h, prev))
            oidx.set_visibility(visible)

    # -- the exact f32 brute force (deleted tuples are not part of the ground truth, on either side)
    dq = ix.ctx.alloc(q.nbytes)
    try:
        ix.ctx.upload(dq, q)
        bi, bd = ix.bruteforce_topk(dq, len(q), 10)
    finally:
        ix.ctx.free(dq)
    oi, od = oidx.bruteforce(q, k=10)
    assert (bi == oi).all() and _same_bits(bd, od), (where, "bruteforce")
    live_rows = int(((host["heap_tids"] & OFFSET) != 0).sum())
    assert ((bi != INV).sum(1) == min(10, live_rows)).all(), where

    if pages:
        assert distance != 2, "the inner product is outside the page layout"
        check_pages(ix, O, distance, q, host, oidx, where)
    return host, oidx
