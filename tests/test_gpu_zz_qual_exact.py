"""The exact qualified top-k (vs_search_batch_qual_exact / _dev, vs_qual_exact.h): for every scan the k nearest rows among those whose
bit is set in the scan's qualifier, that are not deleted and that the mask in force does not hide.  The reference everywhere is the
oracle's own OracleIndex.bruteforce on an oracle index whose heap tids have the offset zeroed for every node outside that set — one
oracle index per distinct slot.  Ids and rows are compared with `==`, tids where the id is valid, distances by bit pattern, the
(INVALID, NaN) tail included.  The indexes are flat (no graph is walked).  Also runs on the lockstep interpreter
(tests/test_emu_qual_exact.py)."""
import numpy as np
import pytest

from helpers import make_vectors, tie_vectors
from oracle import oracle_py as O
from test_gpu_scan_bruteforce import DISTANCES, INV, _bits, _delete, _live_tids, _oracle_of, _special_corpus, _upload
from test_gpu_zz_qual import options

pytestmark = pytest.mark.gpu
N = 2037  # the last bitmap word is partial
INVALID, STATE = -1, -5


def expect(vecs, tids, dt, plain, q, slots, quals, k, hidden=None):
    """quals: {slot: bool [n]} -> ids, tids, distance bits, rows"""
    nq, n = len(q), len(vecs)
    ids, rows = np.full((nq, k), INV, np.uint32), np.zeros(nq, np.uint32)
    bits = np.full((nq, k), 0x7FC00000, np.uint32)
    for s in np.unique(slots):
        inside = np.ones(n, bool) if s == 0 else quals[int(s)].copy()
        if hidden is not None:
            inside &= ~hidden
        t = tids.copy()
        _delete(t, ~inside)
        oi, od = _oracle_of(vecs, t, dt, plain).bruteforce(q[slots == s], k=k)
        ids[slots == s], bits[slots == s], rows[slots == s] = oi, _bits(od), (oi != INV).sum(axis=1)
    return ids, np.where(ids != INV, tids[np.minimum(ids, n - 1)], 0).astype(np.uint64), bits, rows


def assert_equal(got, exp, what=""):
    assert (got[3] == exp[3]).all(), what
    assert (got[0] == exp[0]).all(), what
    assert (got[1] == exp[1]).all(), what
    assert (_bits(got[2]) == exp[2]).all(), what


LENGTHS = lambda k: [0, 1, k - 1, 31, 32, 33, 200]  # noqa: E731  |C| of slots 1 .. 7
CASES = [(dim, d, st, (1, 10, 64)[i % 3]) for i, (dim, d, st) in
         enumerate((dim, d, st) for dim in (8, 40, 96) for d in DISTANCES for st in ("sbq", "plain"))]


@pytest.mark.parametrize("dim,distance,storage,k", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_list_lengths_tiles_and_k_with_deleted_and_hidden_rows(gpu_ctx, oracle, dim, distance, storage, k):
    """dim 8: the tail only; 40: one step plus a tail; 96: steps only.  Seven qualifiers of their own list lengths plus slot 0 in one
    interleaved batch, 1 / TQ - 1 / TQ / TQ + 1 / 2 TQ + 1 scans per slot."""
    dt, plain = DISTANCES[distance], storage == "plain"
    rng = np.random.default_rng(dim + k)
    vecs = make_vectors(N, dim, dim, "gauss") * rng.uniform(0.2, 3.0, (N, 1)).astype(np.float32)
    vecs[:40:4] = 0                                                     # divisor 0: zero rows ...
    vecs[1:40:4] /= np.linalg.norm(vecs[1:40:4], axis=1, keepdims=True)  # ... and rows that are unit already
    tids = _live_tids(N)
    _delete(tids, rng.random(N) < 0.05)
    hidden = rng.random(N) < 0.05
    ix = _upload(gpu_ctx, vecs, tids.copy(), dt, plain)
    try:
        tq = ix.search_batch_qual_exact(vecs[:1], np.zeros(1, np.uint32), k=k)[4]["tile_queries"]
        per_slot = [tq + 1, 1, tq - 1, tq, tq + 1, 2 * tq + 1, 1, tq]
        slots = rng.permutation(np.repeat(np.arange(8, dtype=np.uint32), per_slot))
        q = make_vectors(len(slots), dim, dim + 1, "gauss")
        # disjoint bit sets of |C| + 2 live, visible rows; the two rows nearest to the slot's first scan are then deleted / hidden
        free = rng.permutation(np.flatnonzero((tids & np.uint64(0xFFFF) != 0) & ~hidden))
        quals, at = {}, 0
        for s, m in enumerate(LENGTHS(k), start=1):
            quals[s] = np.zeros(N, bool)
            quals[s][free[at:at + m + 2]] = True
            at += m + 2
            first = np.flatnonzero(slots == s)[:1]
            near = expect(vecs, tids, dt, plain, q[first], slots[first], quals, 2)[0][0]
            assert (near != INV).all() and quals[s][near].all()  # precondition: both would be in the oracle's list
            _delete(tids, near[:1])
            hidden[near[1]] = True
        exp = expect(vecs, tids, dt, plain, q, slots, quals, k, hidden)
        for s, m in enumerate(LENGTHS(k), start=1):
            assert (exp[3][slots == s] == min(k, m)).all() and quals[s].sum() == m + 2
        ix.close()
        ix = _upload(gpu_ctx, vecs, tids, dt, plain)
        ix.set_visibility((~hidden).astype(np.uint8))
        for s, b in quals.items():
            ix.qual_put(s, b)
        got = ix.search_batch_qual_exact(q, slots, k=k)
        assert_equal(got, exp)
        st = got[4]
        in_slot_0 = int(((tids & np.uint64(0xFFFF) != 0) & ~hidden).sum())
        assert (st["tile_queries"], st["lists"], st["rows_listed"]) == (tq, 8, sum(LENGTHS(k)) + in_slot_0)
        assert st["tiles"] == sum(-(-c // tq) for c in per_slot)
        # slot 0 without a mask: oracle.bruteforce on the untouched index
        ix.set_visibility(None)
        z = slots == 0
        oi, od = _oracle_of(vecs, tids, dt, plain).bruteforce(q[z], k=k)
        g0 = ix.search_batch_qual_exact(q[z], slots[z], k=k)
        assert (g0[0] == oi).all() and (_bits(g0[2]) == _bits(od)).all()
    finally:
        ix.close()


@pytest.mark.parametrize("corpus", ["gauss", "ties"])
def test_forced_slices_and_tiles_change_no_row_and_ties_break_by_node_id(gpu_ctx, oracle, corpus):
    k, dim, nq = 10, 40, 9
    vecs = make_vectors(N, dim, 5, "gauss") if corpus == "gauss" else tie_vectors(N, 40, dim, 5)
    q = make_vectors(nq, dim, 6, "gauss") if corpus == "gauss" else tie_vectors(nq, 40, dim, 7)
    tids = _live_tids(N)
    bits = np.zeros(N, bool)
    rows = np.sort(np.random.default_rng(8).choice(N, 200, replace=False))
    bits[rows] = True
    slots = np.ones(nq, np.uint32)
    exp = expect(vecs, tids, O.L2, False, q, slots, {1: bits}, k)
    if corpus == "ties":  # equal distances on both sides of the boundary of two slices (list place 128), and at places k - 1 / k
        place = np.searchsorted(rows, exp[0])
        tie = exp[2][:, 1:] == exp[2][:, :-1]
        assert (tie & ((place[:, 1:] < 128) != (place[:, :-1] < 128))).any()
        wider = expect(vecs, tids, O.L2, False, q, slots, {1: bits}, k + 1)
        assert (wider[2][:, k - 1] == wider[2][:, k]).any()
    ix = _upload(gpu_ctx, vecs, tids, O.L2)
    try:
        ix.qual_put(1, bits)
        tq = ix.search_batch_qual_exact(q[:1], slots[:1], k=k)[4]["tile_queries"]
        for S, T in [(1, tq), (2, tq), (7, tq), (2, 1), (2, 2), (2, 4), (2, 16)]:  # every instantiation of the tile
            with options(VS_QUAL_EXACT_SLICES=S, VS_QUAL_EXACT_TQ=T):
                got = ix.search_batch_qual_exact(q, slots, k=k)
            assert_equal(got, exp, f"{S} slices, tiles of {T}")
            assert (got[4]["slices"], got[4]["tile_queries"], got[4]["tiles"]) == (S, T, -(-nq // T))
            assert got[4]["row_reads"] == 200 * got[4]["tiles"]
    finally:
        ix.close()


@pytest.mark.parametrize("distance", ["l2", "ip"])
def test_nan_inf_and_negative_zero_order_by_total_cmp_key(gpu_ctx, oracle, distance):
    vecs, q, tids = _special_corpus()
    bits = np.random.default_rng(9).random(len(vecs)) < 0.3
    bits[[5, 6, 7, 8, 9, 10, 11, 12, 41, 201, 220, 225]] = True
    slots = np.ones(len(q), np.uint32)
    exp = expect(vecs, tids, DISTANCES[distance], False, q, slots, {1: bits}, 64)
    d = exp[2].view(np.float32)[exp[0] != INV]
    assert np.isnan(d).any() and np.isinf(d).any() and (np.signbit(d) & ((d == 0) | np.isnan(d))).any()
    ix = _upload(gpu_ctx, vecs, tids, DISTANCES[distance])
    try:
        ix.qual_put(1, bits)
        assert_equal(ix.search_batch_qual_exact(q, slots, k=64), exp)
    finally:
        ix.close()


def test_the_device_entry_point_and_the_refusals(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    k, nq = 10, 11
    vecs, q, tids = make_vectors(N, 40, 1, "gauss"), make_vectors(nq, 40, 2, "gauss"), _live_tids(N)
    bits = np.random.default_rng(3).random(N) < 0.1
    slots = (np.arange(nq) % 2).astype(np.uint32)
    exp = expect(vecs, tids, O.COSINE, False, q, slots, {1: bits}, k)
    ix = _upload(gpu_ctx, vecs, tids, O.COSINE)
    bufs = [gpu_ctx.alloc(s) for s in (q.nbytes, nq * 4, nq * k * 4, nq * k * 8, nq * k * 4, nq * 4, nq * k * 4)]
    dq, ds, d_ids, d_tids, d_dist, d_rows, d_busy = bufs
    outs = (d_ids, np.empty((nq, k), np.uint32)), (d_tids, np.empty((nq, k), np.uint64)), (d_dist, np.empty((nq, k), np.float32)), \
        (d_rows, np.empty(nq, np.uint32))
    try:
        ix.qual_put(1, bits)
        gpu_ctx.upload(dq, q)
        gpu_ctx.upload(ds, slots)
        ix.search_batch_qual_exact_dev(dq, nq, k, ds, d_ids, d_rows, d_out_tids=d_tids, d_out_dist=d_dist)
        assert_equal([gpu_ctx.download(d, a) for d, a in outs], exp)
        assert ix.search_batch_qual_exact(q[:0], slots[:0], k=k)[3].size == 0  # nq = 0
        for d, a in outs:  # a refusal writes nothing: a poison fill
            gpu_ctx.upload(d, np.full(a.nbytes, 0xA5, np.uint8))
        view = ix.view(gpu_ctx)
        busy = _upload(gpu_ctx, vecs, tids, O.COSINE)  # a batch of the handle in flight
        busy.search_batch_dev(dq, nq, 10, 10, k, d_busy)
        codes_only = P.DiskAnnIndex.upload(gpu_ctx, codes=np.zeros((N, 1), np.uint64), nbrs=np.full((N, 4), INV, np.uint32), heap_tids=tids,
                                           vecs=None, mean=np.zeros(40, np.float32), m2=None, count=1, bits=1, dim_index=40, num_neighbors=4,
                                           distance_type=O.COSINE, default_start=0)  # no vector column on the device
        # (code, handle, k, the slot every scan names, d_slots, d_rows)
        refused = [(INVALID, ix, 0, 1, ds, d_rows), (INVALID, ix, 65, 1, ds, d_rows), (INVALID, ix, k, 65, ds, d_rows),
                   (INVALID, ix, k, 1, None, d_rows), (INVALID, ix, k, 1, ds, None), (STATE, ix, k, 2, ds, d_rows), (STATE, view, k, 1, ds, d_rows),
                   (INVALID, None, k, 0, ds, d_rows), (STATE, busy, k, 0, ds, d_rows), (STATE, codes_only, k, 0, ds, d_rows)]
        try:
            for code, h, kk, slot, dsl, drw in refused:
                gpu_ctx.upload(ds, np.full(nq, slot, np.uint32))
                if h is None:  # (no handle to call a method of)
                    assert ix._L.vs_search_batch_qual_exact_dev(None, dq, nq, kk, dsl, d_ids, d_tids, d_dist, drw, None) == code
                    continue
                with pytest.raises(P.VsError) as e:
                    h.search_batch_qual_exact_dev(dq, nq, kk, dsl, d_ids, drw, d_out_tids=d_tids, d_out_dist=d_dist)
                assert e.value.code == code, (kk, slot)
                if dsl is not None and drw is not None and kk:  # (the host form allocates its own outputs: k = 0 has none)
                    with pytest.raises(P.VsError) as e:
                        h.search_batch_qual_exact(q, np.full(nq, slot, np.uint32), k=kk)
                    assert e.value.code == code, (kk, slot)
        finally:
            busy.search_batch_dev_finish()
            for h in (view, busy, codes_only):
                h.close()
        assert all((gpu_ctx.download(d, a).view(np.uint8) == 0xA5).all() for d, a in outs)
    finally:
        for b in bufs:
            gpu_ctx.free(b)
        ix.close()
