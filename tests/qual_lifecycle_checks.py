"""The qualified and grouped twin of lifecycle_checks.check_index_everywhere: one checker for the read paths that make promises about
the STATE of an index — the exact qualified top-k, the qualified flat scan, grouped graph scans, the exact and the flat top-k under a
group cap and qualified scan pools (include/vsgpu.h: "the mask in force on the index", "whose heap tid offset is not 0", LIFETIME of
the qualifiers and of the group column) — in whatever state a chain of inserts, deletes, consolidations, reserves, shrinks and
compactions left it (tests/test_gpu_zz_qual_lifecycle.py).  check_qualified_everywhere takes the arrays check_index_everywhere (or its
plain twin) downloaded and the oracle built over exactly those arrays, plus the host's own account of the mask, the snapshots, the
qualifier bits and the group column as they must stand now.  Every expectation is the oracle's, or a plain Python restatement the
single-step tests already hold the library to (`expect` / `check` of tests/test_gpu_zz_grouped.py, `capped` of
tests/test_gpu_zz_qual_exact_grouped.py, `page` of tests/pool_qual_checks.py); nothing compares the library with itself except the
identity the header states (EQUIVALENCE: a flat scan whose rescore reaches every qualifying row gives the exact call's rows).

What the reference does with the state — that the cap bites, that a deleted and a hidden row would have been in an answer, that
inserted rows are in one, that every end state of a scan occurs — is recorded in the dict the checker returns, from the reference
alone and before the device result is looked at; a chain ORs these together and asserts them at its end (`require`)."""
import ctypes as C

import numpy as np

import pool_qual_checks as PQ
import qual_checks as QC
import test_gpu_zz_grouped as GR
import test_gpu_zz_qual_exact as XQ
from lifecycle_checks import INV, OFFSET, SEARCH, oracle_of, prepared_slice
from plain_lifecycle_checks import oracle_plain
from test_gpu_zz_qual import options
from test_gpu_zz_qual_exact_grouped import capped

NONE = 0xFFFFFFFF
STATE = -5
NAN_BITS = 0x7FC00000
EXACT_KS = (1, 10)
FLAT = dict(k=10, rescores=(10, 33), all_rows=4096)
GROUPED = dict(k=10, max_pops=64, per_groups=(1, 3))
POOL = dict(slots=2, k=8, pages=2, max_pops=64, rows_cap=1024)
SEEN = ("cap_bites", "cap_bites_exact", "cap_bites_flat", "deleted_row_exact", "hidden_row_exact", "deleted_row_scan", "hidden_row_scan",
        "inserted_row", "complete", "ended", "cut")


def new_seen():
    return dict.fromkeys(SEEN, False) | {"slot0_max_id": -1}


def merge(total, seen):
    for key in SEEN:
        total[key] |= seen[key]
    total["slot0_max_id"] = max(total["slot0_max_id"], seen["slot0_max_id"])
    return total


def require(total, keys, where=""):
    """the preconditions a chain asserts at its end"""
    missing = [key for key in keys if not total[key]]
    assert not missing, (where, "the reference never showed", missing)


def group_layout(n, seed):
    """about 40 groups over the rows, a tenth ungrouped, the values 0 and 0xFFFFFFFE present.  The groups are of unequal size (group g
    about as 1 / (g + 1)): under a cap of 1 the few large groups fill early, so that within 64 pops some scans keep 10 rows and some
    do not — with groups of equal size every scan of these chains completes and VS_QUAL_CUT never occurs"""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, 41)
    g = rng.choice(40, n, p=p / p.sum()).astype(np.uint32)
    g[g == 39] = 0xFFFFFFFE
    g[rng.random(n) < 0.10] = NONE
    return g


def _is_plain(ix):
    from pgvectorscale_amd import _lib
    return ix.desc.storage_type == _lib.VS_STORAGE_PLAIN


def _oracle_over(O, ix, host, distance, tids):
    """the oracle over the downloaded arrays with another heap tid column"""
    h = dict(host, heap_tids=np.ascontiguousarray(tids, np.uint64))
    if _is_plain(ix):
        d = ix.desc
        return oracle_plain(O, h, distance=distance, dim_index=d.dim_index, R=d.num_neighbors, start=d.default_start)
    return oracle_of(O, ix, h, distance)


def _zeroed_outside(tids, inside):
    t = tids.copy()
    t[~inside] &= ~OFFSET
    return t


def _revived(tids):
    """every tombstone given an offset again: the expectation with the tombstone filter off"""
    return np.where((tids & OFFSET) == 0, tids | np.uint64(1), tids)


def _quals(qualifier, n):
    """-> (slot, {slot: bool [n] as the slot must read now}) — (0, {}) without a qualifier"""
    if qualifier is None:
        return 0, {}
    slot, bits = qualifier
    bits = np.asarray(bits, bool)
    assert bits.size <= n
    return slot, {slot: np.concatenate([bits, np.zeros(n - bits.size, bool)])}


def _slots(nq, slot, shift=0):
    """the slots alternate between the qualifier and 0 ("every node")"""
    return np.where((np.arange(nq) + shift) % 2 == 0, slot, 0).astype(np.uint32)


def exact_expect(O, ix, host, distance, q, slots, quals, k, visible, tids=None):
    """the construction of tests/test_gpu_zz_qual_exact.py::expect over the downloaded arrays: per distinct slot the oracle's brute
    force on an oracle index whose tid offsets are zeroed outside bits AND visible (a tombstone's is zero already)
    -> ids, tids, distance bits, rows"""
    tids = host["heap_tids"] if tids is None else tids
    nq, n = len(q), tids.size
    ids, rows = np.full((nq, k), INV, np.uint32), np.zeros(nq, np.uint32)
    bits = np.full((nq, k), NAN_BITS, np.uint32)
    shown = np.ones(n, bool) if visible is None else np.asarray(visible) != 0
    for s in np.unique(slots):
        inside = shown if s == 0 else quals[int(s)] & shown
        oi, od = _oracle_over(O, ix, host, distance, _zeroed_outside(tids, inside)).bruteforce(q[slots == s], k=k)
        ids[slots == s], bits[slots == s], rows[slots == s] = oi, XQ._bits(od), (oi != INV).sum(axis=1)
    return ids, np.where(ids != INV, host["heap_tids"][np.minimum(ids, n - 1)], 0).astype(np.uint64), bits, rows


def flat_expect(O, ix, host, distance, q, qcodes, slots, quals, k, rescore, visible):
    """per slot S = the oracle's (Hamming, node id) selection over the codes the DEVICE holds with the tid offsets zeroed outside C,
    per scan the oracle's brute force with the offsets zeroed outside S -> ids, tids, distance bits, rows"""
    tids = host["heap_tids"]
    nq, n = len(q), tids.size
    ids, rows = np.full((nq, k), INV, np.uint32), np.zeros(nq, np.uint32)
    bits = np.full((nq, k), NAN_BITS, np.uint32)
    shown = np.ones(n, bool) if visible is None else np.asarray(visible) != 0
    for s in np.unique(slots):
        inside = shown if s == 0 else quals[int(s)] & shown
        of_slot = np.flatnonzero(slots == s)
        cands = O.hamming_scan_topk(host["codes"], qcodes[of_slot], rescore, heap_tids=_zeroed_outside(tids, inside))[0]
        for qi, cand in zip(of_slot, cands):
            t = _zeroed_outside(tids, np.isin(np.arange(n), cand[cand != INV]))
            oi, od = _oracle_over(O, ix, host, distance, t).bruteforce(q[qi:qi + 1], k=k)
            ids[qi], bits[qi], rows[qi] = oi[0], XQ._bits(od)[0], (oi[0] != INV).sum()
    return ids, np.where(ids != INV, tids[np.minimum(ids, n - 1)], 0).astype(np.uint64), bits, rows


def _refused(code, word, call, where):
    import pgvectorscale_amd as P
    try:
        call()
    except P.VsError as e:
        assert e.code == code and word in str(e), (where, str(e))
        return
    raise AssertionError((where, "was not refused", word))


def _differs(a, b):
    return bool((a[0] != b[0]).any())


def _scan_oracle(O, ix, host, distance, oidx, tids, visible):
    """an oracle over the same graph with another tid column and mask (labels as oidx holds them)"""
    if _is_plain(ix):
        o = _oracle_over(O, ix, host, distance, tids)
    else:
        kw = {}
        if oidx.label_off is not None:
            kw = dict(label_off=oidx.label_off, label_val=oidx.label_val, label_starts=dict(zip(oidx.ls_labels.tolist(), oidx.ls_nodes.tolist())))
        o = oracle_of(O, ix, dict(host, heap_tids=np.ascontiguousarray(tids, np.uint64)), distance, **kw)
    o.set_visibility(visible)
    return o


def _check_grouped_scans(ix, O, distance, q, host, oidx, visible, slot, quals, groups, keys, seen, where, once=False):
    """the grouped graph scan under the mask in force on oidx (the caller set it); once: a single run (a stored snapshot)"""
    L, rescore, k, max_pops = SEARCH["L"], SEARCH["rescore"], GROUPED["k"], GROUPED["max_pops"]
    tids = host["heap_tids"]
    for pg in GROUPED["per_groups"][:1 if once else None]:
        slots = _slots(len(q), slot, shift=pg)
        exp = GR.expect(oidx, tids, q, groups, pg, k, max_pops, L, rescore, quals=quals, slots=slots)
        # -- what the reference does with this state
        free = QC.expect(oidx, tids, q, quals, slots, L, rescore, k, max_pops)
        seen["cap_bites"] |= _differs(exp, free)
        if pg == GROUPED["per_groups"][0] and not once:  # (the filters off: once per check is enough for a precondition)
            dead_on = GR.expect(_scan_oracle(O, ix, host, distance, oidx, _revived(tids), visible), tids, q, groups, pg, k, max_pops, L, rescore, quals=quals, slots=slots)
            seen["deleted_row_scan"] |= _differs(exp, dead_on)
        if visible is not None and pg == GROUPED["per_groups"][0] and not once:
            shown = GR.expect(_scan_oracle(O, ix, host, distance, oidx, tids, None), tids, q, groups, pg, k, max_pops, L, rescore, quals=quals, slots=slots)
            seen["hidden_row_scan"] |= _differs(exp, shown)
        zero = exp[0][slots == 0]
        seen["slot0_max_id"] = max(seen["slot0_max_id"], int(zero[zero != INV].astype(np.int64).max(initial=-1)))
        for name, state in (("complete", QC.COMPLETE), ("ended", QC.ENDED), ("cut", QC.CUT)):
            seen[name] |= bool((exp[5] == state).any())
        # -- the device
        GR.check(GR.run(ix, q, k, pg, max_pops, L, rescore, qual_slots=slots), exp, max_pops, (where, "grouped scan", pg))
        if once:
            return
        if pg == GROUPED["per_groups"][-1]:
            with options(VS_RERANK_FUSED="0"):
                GR.check(GR.run(ix, q, k, pg, max_pops, L, rescore, qual_slots=slots), exp, max_pops, (where, "grouped scan, unfused", pg))
    # rescore 0: the reference never fetches the heap, so the mask in force hides nothing (a tombstone is no row of the scan even so)
    pg, slots = GROUPED["per_groups"][0], _slots(len(q), slot)
    exp = GR.expect(oidx, tids, q, groups, pg, k, max_pops, L, 0, quals=quals, slots=slots)
    if visible is not None:
        bare = GR.expect(_scan_oracle(O, ix, host, distance, oidx, tids, None), tids, q, groups, pg, k, max_pops, L, 0, quals=quals, slots=slots)
        assert not _differs(exp, bare) and (exp[4] == bare[4]).all(), (where, "the reference looked at the mask with rescore 0")
    GR.check(GR.run(ix, q, k, pg, max_pops, L, 0, qual_slots=slots), exp, max_pops, (where, "grouped scan, rescore 0"))
    if keys is not None:
        exp = GR.expect(oidx, tids, q, groups, pg, k, max_pops, L, rescore, quals=quals, slots=slots, qlabels=keys)
        for name, state in (("complete", QC.COMPLETE), ("ended", QC.ENDED), ("cut", QC.CUT)):
            seen[name] |= bool((exp[5] == state).any())
        GR.check(GR.run(ix, q, k, pg, max_pops, L, rescore, qual_slots=slots, qlabels=keys), exp, max_pops, (where, "grouped scan, keyed"))


def _check_exact(ix, O, distance, q, host, visible, slot, quals, groups, seen, where, once=False):
    """the exact top-k and, with a group column, the exact top-k under the cap -> the exact call's rows at k = 10"""
    tids, n = host["heap_tids"], host["heap_tids"].size
    got10 = None
    for i, k in enumerate(EXACT_KS[1:] if once else EXACT_KS):
        slots = _slots(len(q), slot, shift=i)
        exp = exact_expect(O, ix, host, distance, q, slots, quals, k, visible)
        if not once:  # (the filters off)
            seen["deleted_row_exact"] |= _differs(exp, exact_expect(O, ix, host, distance, q, slots, quals, k, visible, tids=_revived(tids)))
        if visible is not None and not once:
            seen["hidden_row_exact"] |= _differs(exp, exact_expect(O, ix, host, distance, q, slots, quals, k, None))
        zero = exp[0][slots == 0]
        seen["slot0_max_id"] = max(seen["slot0_max_id"], int(zero[zero != INV].astype(np.int64).max(initial=-1)))
        got = ix.search_batch_qual_exact(q, slots, k=k)
        XQ.assert_equal(got, exp, (where, "exact", k))
        if k == FLAT["k"]:
            got10 = (slots, got)
    if groups is not None:
        slots = _slots(len(q), slot)
        full = exact_expect(O, ix, host, distance, q, slots, quals, n, visible)
        for pg in GROUPED["per_groups"][:1 if once else None]:
            exp = capped(full, groups, GROUPED["k"], pg)
            seen["cap_bites_exact"] |= bool((exp[0] != full[0][:, :GROUPED["k"]]).any())
            XQ.assert_equal(ix.search_batch_qual_exact_grouped(q, slots, k=GROUPED["k"], per_group=pg), exp, (where, "exact under the cap", pg))
    return got10


def _check_flat(ix, O, distance, q, host, visible, slot, quals, groups, exact10, seen, where):
    d = ix.desc
    k = FLAT["k"]
    if _is_plain(ix):
        slots = _slots(len(q), slot)
        _refused(STATE, "", lambda: ix.search_batch_qual_flat(q, slots, k=k, rescore=FLAT["rescores"][0]), (where, "flat on plain storage"))
        return
    mean, m2, cnt = ix.get_quantizer()
    qcodes = O.quantize(mean, m2, cnt, d.bits, prepared_slice(O, q, distance, d.dim_index))
    for i, rescore in enumerate(FLAT["rescores"]):
        slots = _slots(len(q), slot, shift=i + 1)
        exp = flat_expect(O, ix, host, distance, q, qcodes, slots, quals, k, rescore, visible)
        XQ.assert_equal(ix.search_batch_qual_flat(q, slots, k=k, rescore=rescore), exp, (where, "flat", rescore))
    slots, exact = exact10
    got = ix.search_batch_qual_flat(q, slots, k=k, rescore=FLAT["all_rows"])
    XQ.assert_equal(got, (exact[0], exact[1], XQ._bits(exact[2]), exact[3]), (where, "flat with every row rescored is the exact call"))
    if groups is not None:
        rescore = FLAT["rescores"][-1]
        slots = _slots(len(q), slot)
        full = flat_expect(O, ix, host, distance, q, qcodes, slots, quals, rescore, rescore, visible)
        for pg in GROUPED["per_groups"]:
            exp = capped(full, groups, k, pg)
            seen["cap_bites_flat"] |= bool((exp[0] != full[0][:, :k]).any())
            XQ.assert_equal(ix.search_batch_qual_flat_grouped(q, slots, k=k, per_group=pg, rescore=rescore), exp, (where, "flat under the cap", pg))


def _check_pool(ix, oidx, q, slot, quals, where):
    """a pool created NOW: 2 slots, two pages of 8 rows within 64 pops each, one slot under the qualifier and one under none"""
    import pgvectorscale_amd as P
    L, rescore = SEARCH["L"], SEARCH["rescore"]
    queries = (q[1], q[len(q) - 1])  # (the last one sits next to the first inserted rows)
    qslots = np.array([slot, 0], np.uint32)
    pool = P.ScanPool(ix, POOL["slots"], search_list_size=L, rescore=rescore, kmax=POOL["k"], rows_cap=POOL["rows_cap"])
    try:
        oscans = []
        for i in range(POOL["slots"]):
            pool.rescan(i, queries[i])
            oscans.append(oidx.scan(queries[i], L=L, rescore=rescore))
        for pg in range(POOL["pages"]):
            exps = [PQ.page(oscans[i], quals[int(qslots[i])] if qslots[i] else None, POOL["k"], POOL["max_pops"]) for i in range(POOL["slots"])]
            got = pool.fetch_qual(list(range(POOL["slots"])), POOL["k"], qslots, POOL["max_pops"])
            for i in range(POOL["slots"]):
                PQ.assert_page(got, i, exps[i], (where, "pool", pg, i))
                PQ.assert_stats(pool.stats(i), exps[i], (where, "pool", pg, i))
        for o in oscans:
            o.close()
    finally:
        pool.close()


def check_qualified_everywhere(ix, O, distance, q, host, oidx, *, visible, snapshots, qualifier, groups, keys=None, where=""):
    """ix: a live DiskAnnIndex of either storage; host, oidx: what check_index_everywhere / check_plain_everywhere just returned (the
    downloaded arrays, the OracleIndex over exactly those); visible: the mask set_visibility put in force as it must stand NOW (uint8
    [n]) or None; snapshots: {id: mask as it must stand now}; qualifier: (slot, the bits as they were put — shorter than n when rows
    were added since) or None; groups: the group column as it must stand now (uint32 [n]) or None: no column, every grouped call
    refuses; keys: one label key per query (a labeled index).  -> what the reference showed (new_seen / merge / require)"""
    from pgvectorscale_amd import _lib
    ix._refresh()
    n = ix.desc.n
    seen = new_seen()
    assert host["heap_tids"].shape == (n,) and oidx.n == n, where
    if visible is not None:
        visible = np.ascontiguousarray(visible, np.uint8)
        assert visible.shape == (n,), where
    slot, quals = _quals(qualifier, n)

    # -- the column and the bitmap as they stand
    if groups is None:
        s0 = np.zeros(len(q), np.uint32)
        _refused(STATE, "no group column", ix.groups_get, (where, "groups_get"))
        _refused(STATE, "no group column", lambda: GR.run(ix, q, 10, 1, 64, SEARCH["L"], SEARCH["rescore"]), (where, "grouped scan"))
        _refused(STATE, "no group column", lambda: ix.search_batch_qual_exact_grouped(q, s0, k=10, per_group=1), (where, "exact under the cap"))
        if not _is_plain(ix):
            _refused(STATE, "no group column", lambda: ix.search_batch_qual_flat_grouped(q, s0, k=10, per_group=1, rescore=33), (where, "flat under the cap"))
    else:
        groups = np.ascontiguousarray(groups, np.uint32)
        assert groups.shape == (n,), where
        now = ix.groups_get()
        assert now.shape == (n,) and (now == groups).all(), (where, "group column", np.flatnonzero(now != groups)[:8])
    if qualifier is not None:
        now = ix.qual_download(slot)
        assert now.shape == (n,) and (now == quals[slot]).all(), (where, "qualifier bits", np.flatnonzero(now != quals[slot])[:8])
        assert ix.qual_info(slot)["n_set"] == int(quals[slot].sum()), where

    # -- under the mask in force
    oidx.set_visibility(visible)
    try:
        exact10 = _check_exact(ix, O, distance, q, host, visible, slot, quals, groups, seen, where)
        _check_flat(ix, O, distance, q, host, visible, slot, quals, groups, exact10, seen, where)
        if groups is not None:
            _check_grouped_scans(ix, O, distance, q, host, oidx, visible, slot, quals, groups, keys, seen, where)
        _check_pool(ix, oidx, q, slot, quals, where)

        # -- each stored snapshot
        for sid, smask in sorted((snapshots or {}).items()):
            smask = np.ascontiguousarray(smask, np.uint8)
            assert smask.shape == (n,), where
            prev = C.c_void_p()
            _lib.check(ix._L.vs_index_snapshot_use(ix.h, sid, C.byref(prev)))
            try:
                oidx.set_visibility(smask)
                _check_exact(ix, O, distance, q, host, smask, slot, quals, groups, seen, (where, "snapshot", sid), once=True)
                if groups is not None:
                    _check_grouped_scans(ix, O, distance, q, host, oidx, smask, slot, quals, groups, None, seen, (where, "snapshot", sid), once=True)
            finally:
                _lib.check(ix._L.vs_index_set_visibility_dev(ix.h, prev))
                oidx.set_visibility(visible)
    finally:
        oidx.set_visibility(visible)
    return seen
