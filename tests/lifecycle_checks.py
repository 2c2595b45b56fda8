"""One checker for a device-resident index in whatever state a chain of inserts, deletes, consolidations and repairs left it
(tests/test_gpu_zw_lifecycle.py).  check_index_everywhere downloads the arrays once, builds the oracle over exactly those arrays
and holds EVERY entry point to it: the batched search in the three kernel regimes (and with the neighbors' label masks on a
labeled index), the SBQ-ordered stream, the amgettuple cursor, the flat scans and the brute force, with the visibility mask or
snapshot in force.  Every expectation is the oracle's or a numpy restatement written here; nothing compares the library with
itself.  The index builders and graph checks the insert tests share live here too."""
import contextlib
import ctypes as C
import os

import numpy as np

INV = 0xFFFFFFFF
OFFSET = np.uint64(0xFFFF)
EMU = bool(os.environ.get("VS_EMU"))

STREAM_KEYS = ("visited_nodes", "candidate_nodes", "quantized_distance_comparisons", "node_reads", "next_calls")
CURSOR_KEYS = ("visited_nodes", "candidate_nodes", "quantized_distance_comparisons", "full_distance_comparisons", "node_reads",
               "node_heap_reads", "next_calls")
# the kernel regimes as tests/test_gpu_regimes.py forces them
REGIMES = {"default": {}, "tableless": {"VS_F_LDS_MAX_INS": "0"}, "general_kernel": {"VS_FAST": "0"}}
NBRMASK_REGIMES = {"nbrmask": {"VS_F_NBRMASK": "1"}, "nbrmask_tableless": {"VS_F_NBRMASK": "1", "VS_F_LDS_MAX_INS": "0"}}
SEARCH = dict(L=40, rescore=20, k=10)   # the parameters of the insert tests' parity check
STREAM = dict(L=40, m=35)
CURSOR = dict(L=10, rescore=12)         # a short list: 70 rows need the scan continued several times
CURSOR_ROWS, CURSOR_CHECKPOINTS = 70, (1, 17, 65)


# ---- builders and graph checks shared with tests/test_gpu_zv_insert.py -----------------------------------------------------------
def fresh_index(gpu_ctx, X, *, distance, bits=None, dim_index=None, R=24, L=48, tids=None, build=True):
    """an index over the rows of X manufactured on the device: norms, training, codes, graph"""
    import pgvectorscale_amd as P
    n, dim = X.shape
    ix = P.DiskAnnIndex.alloc(gpu_ctx, n=n, dim_full=dim, dim_index=dim_index, bits=bits, num_neighbors=R, distance_type=distance)
    vp, stride = ix.array(P._lib.ARR_VECS)
    Xp = np.zeros((max(n, 1), stride), np.float32)
    Xp[:n, :dim] = X
    if n:
        gpu_ctx.upload(vp, Xp[:n])
        ix.refresh_norms()
        ix.sbq_train()
        ix.sbq_quantize_corpus()
        if tids is not None:
            gpu_ctx.upload(ix.array(P._lib.ARR_TIDS)[0], np.ascontiguousarray(tids, np.uint64))
        if build:
            ix.build_graph(search_list_size=L, max_alpha=1.2)
    return ix


def make_tids(first, n):
    return ((np.arange(first, first + n, dtype=np.uint64) + 11) << np.uint64(16)) | np.uint64(3)


def well_formed(nb, R):
    n = nb.shape[0]
    assert nb.shape[1] == R
    live = nb != INV
    deg = live.sum(1)
    assert (live == (np.arange(R)[None, :] < deg[:, None])).all(), "lists must be prefix-packed"
    assert (nb[live] < n).all()
    assert not (nb == np.arange(n, dtype=np.uint32)[:, None]).any(), "self loop"
    s = np.sort(nb, axis=1)
    assert not ((s[:, 1:] == s[:, :-1]) & (s[:, 1:] != INV)).any(), "a list names a node twice"


def oracle_of(O, ix, host, distance, **kw):
    mean, m2, cnt = ix.get_quantizer()
    return O.OracleIndex(codes=host["codes"], nbrs=host["nbrs"], heap_tids=host["heap_tids"], vecs=host["vecs"], mean=mean, m2=m2,
                         count=cnt, bits=ix.desc.bits, dim_index=ix.desc.dim_index, num_neighbors=ix.desc.num_neighbors,
                         distance_type=distance, default_start=ix.desc.default_start, **kw)


# ---- numpy restatements ------------------------------------------------------------------------------------------------------------
def cosine_divisors(vecs):
    """k_row_norms: the sum of squares of a row in element order, in f32; 0 = the row is left as it is (a sum below epsilon, or within
    dim x epsilon of 1), else the square root"""
    v = np.ascontiguousarray(vecs, np.float32)
    norm = np.zeros(v.shape[0], np.float32)
    for c in range(v.shape[1]):
        p = v[:, c] * v[:, c]
        norm = norm + p
    eps = np.float32(1.1920929e-07)
    adj = np.float32(eps * np.float32(v.shape[1]))
    one = np.float32(1.0)
    keep = (norm < eps) | ((norm >= one - adj) & (norm <= one + adj))
    return np.where(keep, np.float32(0.0), np.sqrt(norm)).astype(np.float32)


def prepared_slice(O, X, distance, dim_index):
    """what the quantizer sees of a row: its first dim_index dimensions, cosine-normalised on their own (AM/pg_vector.rs:143-157)"""
    sl = np.ascontiguousarray(np.asarray(X, np.float32)[:, :dim_index]).copy()
    if distance == O.COSINE:
        for i in range(sl.shape[0]):
            sl[i] = O.preprocess_cosine(sl[i])[0]
    return sl


def label_csr(sets):
    off = np.zeros(len(sets) + 1, np.uint32)
    off[1:] = np.cumsum([len(s) for s in sets])
    return off, np.array([l for s in sets for l in s], np.int16)


def download_labels(ix):
    """the label CSR as the device holds it"""
    from pgvectorscale_amd import _lib
    n = ix.desc.n
    off = np.empty(n + 1, np.uint32)
    ix.ctx.download(ix.array(_lib.ARR_LABEL_OFF)[0], off)
    val = np.empty(int(off[n]), np.int16)
    if val.size:
        ix.ctx.download(ix.array(_lib.ARR_LABEL_VAL)[0], val)
    return off, val


@contextlib.contextmanager
def regime(env):
    saved = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _same_bits(g, o):
    g, o = np.asarray(g, np.float32), np.asarray(o, np.float32)
    return ((np.isnan(g) & np.isnan(o)) | (g.view(np.uint32) == o.view(np.uint32))).all()


# ---- the entry points ------------------------------------------------------------------------------------------------------------
def check_search_batch(ix, oidx, q, qlabels=None, where=""):
    """ids exact, heap tids those of the rows, distances bit-identical, the counters tests/test_gpu_visibility.py compares"""
    gi, gt, gd, gst = ix.search_batch(q, search_list_size=SEARCH["L"], rescore=SEARCH["rescore"], k=SEARCH["k"], qlabels=qlabels)
    oi, od, ost = oidx.search_batch(q, L=SEARCH["L"], rescore=SEARCH["rescore"], k=SEARCH["k"], qlabels=qlabels)
    assert (gi == oi).all(), (where, np.flatnonzero((gi != oi).any(1))[:4])
    assert _same_bits(gd, od), where
    found = gi != INV
    assert (gt[found] == oidx.heap_tids[gi[found]]).all(), where
    for key in ("visited_nodes", "quantized_distance_comparisons", "full_distance_comparisons", "node_heap_reads", "next_calls"):
        assert gst[key] == ost[key], (where, key, gst[key], ost[key])
    return gi


def check_stream_batch(ix, oidx, q, qlabels=None, where=""):
    gi, gh, gst = ix.stream_batch(q, search_list_size=STREAM["L"], m=STREAM["m"], qlabels=qlabels)
    oi, oh, ost = oidx.stream_batch(q, L=STREAM["L"], m=STREAM["m"], qlabels=qlabels)
    assert (gi == oi).all() and (gh == oh).all(), where
    for key in STREAM_KEYS:
        assert gst[key] == ost[key], (where, key, gst[key], ost[key])


def pull_and_compare(scan, oscan, rows=CURSOR_ROWS, checkpoints=CURSOR_CHECKPOINTS, where="", stats=True, keys=CURSOR_KEYS):
    """amgettuple one row at a time against the oracle's streaming scan: rows, heap tids, distance bits; GreedySearchStats (`keys`)
    at the checkpoints -> rows pulled"""
    pulled = 0
    while pulled < rows:
        r, o = scan.gettuple(), oscan.gettuple()
        assert (r is None) == (o is None), (where, pulled)
        if r is None:
            break
        assert r[1] == o[0] and r[0] == o[1], (where, pulled, r, o)
        assert _same_bits(r[2], o[2]), (where, pulled)
        pulled += 1
        if stats and pulled in checkpoints:
            g, ref = scan.stats(), oscan.stats()
            for key in keys:
                assert g[key] == ref[key], (where, pulled, key, g[key], ref[key])
    return pulled


def check_cursor(ix, oidx, query, labels=None, where=""):
    scan = ix.beginscan()
    try:
        scan.rescan(query, labels=labels, search_list_size=CURSOR["L"], rescore=CURSOR["rescore"])
        return pull_and_compare(scan, oidx.scan(query, labels=labels, L=CURSOR["L"], rescore=CURSOR["rescore"]), where=where)
    finally:
        scan.endscan()


def check_pool_slot(pool, slot, oscan, k, rounds, where="", keys=CURSOR_KEYS):
    """`rounds` chunks of k rows of one pool slot against the oracle's scan (as tests/test_gpu_zt_scanpool.py checks a chunk)"""
    for rnd in range(rounds):
        rows, ids, tids, dist = pool.fetch([slot], k)
        assert rows[0] >= 0, (where, rnd, rows[0])
        n = 0
        for j in range(k):
            o = oscan.gettuple()
            if o is None:
                break
            assert j < rows[0], (where, rnd, "the pool ended the scan early", j)
            assert ids[0][j] == o[0] and tids[0][j] == o[1], (where, rnd, j)
            assert _same_bits(dist[0][j], o[2]), (where, rnd, j)
            n += 1
        assert rows[0] == n, (where, rnd, rows[0], n)
        g, ref = pool.stats(slot), oscan.stats()
        for key in keys:
            assert g[key] == ref[key], (where, rnd, key, g[key], ref[key])
        if n < k:
            break


QUAL = dict(k=10, max_pops=64)


def check_qualifier(ix, oidx, q, qualifier, where="", L=SEARCH["L"], rescore=SEARCH["rescore"]):
    """qualifier = (slot, the bits the slot was filled with — fewer than n when rows were added since).  The slot holds those bits and
    zeros behind them (include/vsgpu.h, qualified scans, LIFETIME: "vs_index_reserve and growing inserts carry the qualifiers over,
    rows added later read 0 and do not qualify"); scans that name it, dealt among unqualified ones, are the oracle's rows
    post-filtered on the host (tests/qual_checks.py), under whatever mask is in force on the oracle"""
    import qual_checks as QC
    slot, bits = qualifier
    n = ix.desc.n
    bits = np.asarray(bits, bool)
    assert bits.size <= n, where
    want = np.concatenate([bits, np.zeros(n - bits.size, bool)])
    now = ix.qual_download(slot)
    assert now.shape == (n,) and (now[:bits.size] == bits).all(), (where, "qualifier bits")
    assert not now[bits.size:].any(), (where, "rows added later read 0")
    assert ix.qual_info(slot)["n_set"] == int(bits.sum()), where
    slots = np.where(np.arange(len(q)) % 2 == 0, slot, 0).astype(np.uint32)
    exp = QC.expect(oidx, oidx.heap_tids, q, {slot: want}, slots, L, rescore, QUAL["k"], QUAL["max_pops"])
    got = ix.search_batch_qual(q, slots, k=QUAL["k"], max_pops=QUAL["max_pops"], search_list_size=L, rescore=rescore)
    QC.assert_equal(got, exp, (where, "qualified scans"))
    picked = got[0][slots == slot]
    assert want[picked[picked != INV]].all(), where


def check_index_everywhere(ix, O, distance, q, keys=None, *, label_starts=None, label_sets=None, visible=None, snapshots=None, qualifier=None,
                           where=""):
    """ix: a live DiskAnnIndex; O: the oracle module; q: queries [nq][dim_full]; keys: one non-empty label key per query (a labeled
    index).  label_starts {label: start node} / label_sets (one sorted list per node): what the test knows the index must hold.
    visible: the mask the test put in force with set_visibility, as it must stand NOW (uint8 [n]); snapshots: {id: mask as it
    must stand now} of the stored snapshots the batched search and the cursor are also run under; qualifier: (slot, bits) as
    check_qualifier takes it.  -> (downloaded arrays, the OracleIndex)"""
    from pgvectorscale_amd import _lib
    ix._refresh()
    d = ix.desc
    n, R = d.n, d.num_neighbors
    labeled = bool(d.has_labels)
    host = ix.download(vecs=True)
    mean, m2, cnt = ix.get_quantizer()
    okw = {}
    if labeled:
        assert keys is not None and label_starts is not None and d.n_label_starts == len(label_starts), where
        loff, lval = download_labels(ix)
        if label_sets is not None:
            woff, wval = label_csr(label_sets)
            assert (loff == woff).all() and (lval == wval).all(), (where, "label sets on the device")
        okw = dict(label_off=loff, label_val=lval, label_starts=label_starts)
    oidx = oracle_of(O, ix, host, distance, **okw)

    # -- arrays
    well_formed(host["nbrs"], R)
    assert ix.capacity >= n, where
    vn_ptr = ix.array(_lib.ARR_VNORM)[0]
    assert vn_ptr.value or distance != O.COSINE, where
    if vn_ptr.value and n:
        vnorm = ix.ctx.download(vn_ptr, np.empty(n, np.float32))
        assert vnorm.tobytes() == cosine_divisors(host["vecs"]).tobytes(), (where, "cosine divisors")
    want_codes = O.quantize(mean, m2, cnt, d.bits, prepared_slice(O, host["vecs"], distance, d.dim_index))
    assert (host["codes"] == want_codes).all(), (where, "codes", np.flatnonzero((host["codes"] != want_codes).any(1))[:4])

    # -- the batched search in every regime, under the mask in force
    if visible is not None:
        assert np.asarray(visible).shape == (n,), where
    oidx.set_visibility(visible)
    for name, env in REGIMES.items():
        with regime(env):
            check_search_batch(ix, oidx, q, None, (where, name))
            if labeled:
                check_search_batch(ix, oidx, q, keys, (where, name, "keyed"))
    if labeled:
        for name, env in NBRMASK_REGIMES.items():
            with regime(env):
                check_search_batch(ix, oidx, q, keys, (where, name))
                assert ix._L.vs_index_has_neighbor_masks(ix.h) == 1, (where, name, "the scans did not run with the neighbors' masks")

    # -- the SBQ-ordered stream (no heap fetch: the mask does not matter to it)
    check_stream_batch(ix, oidx, q, None, (where, "stream"))
    if labeled:
        check_stream_batch(ix, oidx, q, keys, (where, "stream keyed"))

    # -- the cursor
    check_cursor(ix, oidx, q[0], None, (where, "cursor"))
    if labeled:
        check_cursor(ix, oidx, q[1], keys[1], (where, "cursor keyed"))

    # -- qualified scans, under the mask in force
    if qualifier is not None:
        check_qualifier(ix, oidx, q, qualifier, where)

    # -- the stored snapshots
    for sid, smask in sorted((snapshots or {}).items()):
        assert np.asarray(smask).shape == (n,), where
        prev = C.c_void_p()
        _lib.check(ix._L.vs_index_snapshot_use(ix.h, sid, C.byref(prev)))
        try:
            oidx.set_visibility(smask)
            check_search_batch(ix, oidx, q, None, (where, "snapshot", sid))
            check_cursor(ix, oidx, q[0], None, (where, "snapshot cursor", sid))
        finally:
            _lib.check(ix._L.vs_index_set_visibility_dev(ix.h, prev))
            oidx.set_visibility(visible)

    # -- the flat scans: exact SBQ top-k, order (Hamming, node id)
    qcodes = O.quantize(mean, m2, cnt, d.bits, prepared_slice(O, q, distance, d.dim_index))
    for k in (1, 17):
        gi, gh = ix.scan_topk(qcodes, k)
        oi, oh = O.hamming_scan_topk(host["codes"], qcodes, k)
        assert (gi == oi).all() and (gh == oh).all(), (where, "scan_topk", k)
        if labeled:
            skeys = [[]] + [list(x) for x in keys[1:]]  # (an empty key filters nothing)
            for live in (False, True):
                gi, gh = ix.scan_topk(qcodes, k, qlabels=skeys, live_only=live)
                oi, oh = O.hamming_scan_topk(host["codes"], qcodes, k, label_off=loff, label_val=lval,
                                             heap_tids=host["heap_tids"] if live else None, qlabels=skeys)
                assert (gi == oi).all() and (gh == oh).all(), (where, "scan_topk filtered", k, live)

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
    return host, oidx
