"""The qualified flat scan (vs_search_batch_qual_flat / _dev, vs_qual_flat.h): per scan the `rescore` rows of its qualifier's live,
visible rows that are smallest by (Hamming distance of the SBQ codes, node id), then the k of those that are smallest by (exact
distance, node id).  The reference is the oracle alone: per slot oracle_py.hamming_scan_topk over the oracle's own codes with the tid
offsets zeroed outside C gives S, per scan OracleIndex.bruteforce with the offsets zeroed outside S gives the rows.  Ids and rows are
compared with `==`, tids where the id is valid, distances by bit pattern, the (INVALID, NaN) tail included.  The indexes carry the
oracle's codes (the flat indexes of test_gpu_scan_bruteforce carry zero codes, under which every Hamming distance ties) and no graph.
Also runs on the lockstep interpreter (tests/test_emu_qual_flat.py)."""
import functools

import numpy as np
import pytest

from helpers import make_vectors
from oracle import oracle_py as O
from test_gpu_scan_bruteforce import DISTANCES, INV, _bits, _delete, _live_tids, _upload
from test_gpu_zz_qual import options

pytestmark = pytest.mark.gpu
N = 2037  # the last bitmap word is partial
INVALID, STATE = -1, -5


@functools.lru_cache(maxsize=None)
def corpus(dim, dt):
    """vectors and the oracle's quantizer and codes over them (2 bits per dimension at these widths)"""
    vecs = make_vectors(N, dim, dim, "gauss") * np.random.default_rng(dim).uniform(0.2, 3.0, (N, 1)).astype(np.float32)
    rows = vecs if dt != O.COSINE else np.stack([O.preprocess_cosine(v)[0] for v in vecs])
    bits = O.default_bits(dim)
    mean, m2, count = O.train(rows, bits)
    return vecs, dict(mean=mean, m2=m2, count=count, bits=bits), O.quantize(mean, m2, count, bits, rows)


def query_codes(dim, dt, q):
    _, sbq, _ = corpus(dim, dt)
    return O.quantize(sbq["mean"], sbq["m2"], sbq["count"], sbq["bits"], q if dt != O.COSINE else np.stack([O.preprocess_cosine(v)[0] for v in q]))


def index_args(dim, dt, tids):
    vecs, sbq, codes = corpus(dim, dt)
    return dict(codes=codes, nbrs=np.full((N, 4), INV, np.uint32), heap_tids=tids, vecs=vecs, dim_index=dim, num_neighbors=4, distance_type=dt,
                default_start=0, **sbq)


def upload(gpu_ctx, dim, dt, tids):
    import pgvectorscale_amd as P
    return P.DiskAnnIndex.upload(gpu_ctx, **index_args(dim, dt, tids))


def candidates(dim, dt, tids, qcodes, inside, rescore):
    """S of each query code: [nq][rescore] node ids, INV past |S|"""
    t = tids.copy()
    _delete(t, ~inside)
    return O.hamming_scan_topk(corpus(dim, dt)[2], qcodes, rescore, heap_tids=t)[0]


def expect(dim, dt, tids, q, slots, quals, k, rescore, hidden=None):
    """quals: {slot: bool [n]} -> ids, tids, distance bits, rows, sum of |S|"""
    nq, qcodes = len(q), query_codes(dim, dt, q)
    ids, rows = np.full((nq, k), INV, np.uint32), np.zeros(nq, np.uint32)
    bits = np.full((nq, k), 0x7FC00000, np.uint32)
    reranked = 0
    for s in np.unique(slots):
        inside = np.ones(N, bool) if s == 0 else quals[int(s)].copy()
        if hidden is not None:
            inside &= ~hidden
        of_slot = np.flatnonzero(slots == s)
        for qi, cand in zip(of_slot, candidates(dim, dt, tids, qcodes[of_slot], inside, rescore)):
            t = tids.copy()
            _delete(t, ~np.isin(np.arange(N), cand[cand != INV]))
            oi, od = O.OracleIndex(**index_args(dim, dt, t)).bruteforce(q[qi:qi + 1], k=k)
            ids[qi], bits[qi], rows[qi] = oi[0], _bits(od)[0], (oi[0] != INV).sum()
            reranked += int((cand != INV).sum())
    return ids, np.where(ids != INV, tids[np.minimum(ids, N - 1)], 0).astype(np.uint64), bits, rows, reranked


def assert_equal(got, exp, what=""):
    assert (got[3] == exp[3]).all(), what
    assert (got[0] == exp[0]).all(), what
    assert (got[1] == exp[1]).all(), what
    assert (_bits(got[2]) == exp[2]).all(), what


LENGTHS = lambda k, r: [0, 1, k - 1, r - 1, r, r + 1, 700]  # noqa: E731  |C| of slots 1 .. 7
CASES = [(dim, d, (1, 10, 64)[i % 3], (0, 33, 200)[i // 3]) for i, (dim, d) in enumerate((dim, d) for dim in (40, 96, 300) for d in DISTANCES)]


@pytest.mark.parametrize("dim,distance,k,rescore", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_list_lengths_code_widths_and_distances_with_deleted_and_hidden_rows(gpu_ctx, oracle, dim, distance, k, rescore):
    """dim 40: 2 code words, the last partial; 96: 3 words in a row of 4; 300: 10 words, a row crosses a 64-byte sector.  Seven
    qualifiers of their own list lengths plus slot 0 in one interleaved batch, 1 / TQ - 1 / TQ / TQ + 1 / 2 TQ + 1 scans per slot."""
    dt, rescore = DISTANCES[distance], max(rescore, k)
    rng = np.random.default_rng(dim + k)
    tids = _live_tids(N)
    _delete(tids, rng.random(N) < 0.05)
    hidden = rng.random(N) < 0.05
    ix = upload(gpu_ctx, dim, dt, tids.copy())
    try:
        tq = ix.search_batch_qual_flat(corpus(dim, dt)[0][:1], np.zeros(1, np.uint32), k=k, rescore=rescore)[4]["tile_queries"]
        per_slot = [tq + 1, 1, max(tq - 1, 1), tq, tq + 1, 2 * tq + 1, 1, tq]
        slots = rng.permutation(np.repeat(np.arange(8, dtype=np.uint32), per_slot))
        q = make_vectors(len(slots), dim, dim + 1, "gauss")
        qcodes = query_codes(dim, dt, q)
        # disjoint bit sets of |C| + 2 live, visible rows; the two rows nearest by code to the slot's first scan are then deleted / hidden
        free = rng.permutation(np.flatnonzero((tids & np.uint64(0xFFFF) != 0) & ~hidden))
        quals, at = {}, 0
        for s, m in enumerate(LENGTHS(k, rescore), start=1):
            quals[s] = np.zeros(N, bool)
            quals[s][free[at:at + m + 2]] = True
            at += m + 2
            near = candidates(dim, dt, tids, qcodes[np.flatnonzero(slots == s)[:1]], quals[s], 2)[0]
            assert (near != INV).all() and quals[s][near].all()  # precondition: both would lead the oracle's candidates
            _delete(tids, near[:1])
            hidden[near[1]] = True
        exp = expect(dim, dt, tids, q, slots, quals, k, rescore, hidden)
        for s, m in enumerate(LENGTHS(k, rescore), start=1):
            assert (exp[3][slots == s] == min(k, m)).all() and quals[s].sum() == m + 2
        ix.close()
        ix = upload(gpu_ctx, dim, dt, tids)
        ix.set_visibility((~hidden).astype(np.uint8))
        for s, b in quals.items():
            ix.qual_put(s, b)
        got = ix.search_batch_qual_flat(q, slots, k=k, rescore=rescore)
        assert_equal(got, exp)
        st = got[4]
        in_slot_0 = int(((tids & np.uint64(0xFFFF) != 0) & ~hidden).sum())
        assert (st["tile_queries"], st["lists"], st["rows_listed"]) == (tq, 8, sum(LENGTHS(k, rescore)) + in_slot_0)
        assert (st["tiles"], st["reranked"]) == (sum(-(-c // tq) for c in per_slot), exp[4])
    finally:
        ix.close()


def test_ties_at_the_threshold_under_forced_slices_tiles_and_chunks(gpu_ctx, oracle):
    """dim 40: 80 code bits over 700 rows, so many rows share the threshold value; which of them are taken is decided by node id
    alone, across the boundary of two slices (list place 256 under 3 slices), in every tile width and with a chunk per tile."""
    k, rescore, dim, nq, dt = 10, 50, 40, 9, O.L2
    tids = _live_tids(N)
    rows = np.sort(np.random.default_rng(8).choice(N, 700, replace=False))
    inside = np.isin(np.arange(N), rows)
    q = make_vectors(nq, dim, 6, "gauss")
    slots = np.ones(nq, np.uint32)
    # precondition, from the oracle's numbers: some scan has more rows at the threshold than its quota, on both sides of place 256
    straddles = 0
    for qc in query_codes(dim, dt, q):
        t = tids.copy()
        _delete(t, ~inside)
        ids, ham = O.hamming_scan_topk(corpus(dim, dt)[2], qc[None], 700, heap_tids=t)
        at_t = np.searchsorted(rows, ids[0][ham[0] == ham[0][rescore - 1]])
        quota = rescore - int((ham[0] < ham[0][rescore - 1]).sum())
        straddles += len(at_t) > quota and (at_t < 256).any() and (at_t >= 256).any()
    assert straddles
    exp = expect(dim, dt, tids, q, slots, {1: inside}, k, rescore)
    ix = upload(gpu_ctx, dim, dt, tids)
    try:
        ix.qual_put(1, inside)
        for S, T, mb in [(1, 8, 1024), (3, 8, 1024), (3, 1, 1024), (3, 4, 1024), (3, 4, 0), (1, 1, 0)]:
            with options(VS_QUAL_FLAT_SLICES=S, VS_QUAL_FLAT_TQ=T, VS_QUAL_FLAT_WS_MB=mb):
                got = ix.search_batch_qual_flat(q, slots, k=k, rescore=rescore)
            assert_equal(got, exp, f"{S} slices, tiles of {T}, {mb} MiB")
            st = got[4]
            assert (st["slices"], st["tile_queries"], st["tiles"], st["code_reads"]) == (S, T, -(-nq // T), 700 * -(-nq // T))
            assert st["chunks"] == (1 if mb else st["tiles"]) and (mb or st["chunks"] >= 2)
    finally:
        ix.close()


def test_rescore_of_at_least_the_qualifying_rows_gives_the_exact_call_s_rows(gpu_ctx, oracle):
    k, dim, dt = 10, 96, O.COSINE
    tids = _live_tids(N)
    _delete(tids, np.arange(N) % 17 == 3)
    bits = np.random.default_rng(4).random(N) < 0.1
    slots = (np.arange(11) % 2).astype(np.uint32)
    q = make_vectors(len(slots), dim, 9, "gauss")
    ix = upload(gpu_ctx, dim, dt, tids)
    try:
        ix.qual_put(1, bits)
        exact = ix.search_batch_qual_exact(q, slots, k=k)
        got = ix.search_batch_qual_flat(q, slots, k=k, rescore=4096)  # slot 0: |C| = 1 917
        assert_equal(got, (exact[0], exact[1], _bits(exact[2]), exact[3]))
        live = tids & np.uint64(0xFFFF) != 0
        assert got[4]["reranked"] == 6 * int(live.sum()) + 5 * int((bits & live).sum())  # S = C for the 6 scans of slot 0 and the 5 of slot 1
    finally:
        ix.close()


def _device_call(gpu_ctx, ix, q, slots, k, rescore, poison=False):
    """the _dev form over buffers of its own -> (ids, tids, dist, rows) or, refused, the error code and whether anything was written"""
    import pgvectorscale_amd as P
    nq, kk = len(q), max(k, 1)
    outs = [np.empty((nq, kk), np.uint32), np.empty((nq, kk), np.uint64), np.empty((nq, kk), np.float32), np.empty(nq, np.uint32)]
    bufs = [gpu_ctx.alloc(a.nbytes) for a in (q, slots, *outs)]
    try:
        gpu_ctx.upload(bufs[0], q)
        gpu_ctx.upload(bufs[1], slots)
        for b, a in zip(bufs[2:], outs):
            gpu_ctx.upload(b, np.full(a.nbytes, 0xA5, np.uint8))
        try:
            ix.search_batch_qual_flat_dev(bufs[0], nq, k, rescore, bufs[1], bufs[2], bufs[5], d_out_tids=bufs[3], d_out_dist=bufs[4])
        except P.VsError as e:
            return e.code, all((gpu_ctx.download(b, a).view(np.uint8) == 0xA5).all() for b, a in zip(bufs[2:], outs))
        return [gpu_ctx.download(b, a) for b, a in zip(bufs[2:], outs)]
    finally:
        for b in bufs:
            gpu_ctx.free(b)


def test_the_device_entry_point_gives_the_host_form_s_rows(gpu_ctx, oracle):
    k, rescore, dim, dt = 10, 33, 40, O.IP
    bits = np.random.default_rng(3).random(N) < 0.1
    slots = (np.arange(11) % 2).astype(np.uint32)
    q = make_vectors(len(slots), dim, 2, "gauss")
    ix = upload(gpu_ctx, dim, dt, _live_tids(N))
    try:
        ix.qual_put(1, bits)
        host = ix.search_batch_qual_flat(q, slots, k=k, rescore=rescore)
        assert_equal(_device_call(gpu_ctx, ix, q, slots, k, rescore), (host[0], host[1], _bits(host[2]), host[3]))
        assert_equal(host, expect(dim, dt, _live_tids(N), q, slots, {1: bits}, k, rescore))
        assert ix.search_batch_qual_flat(q[:0], slots[:0], k=k, rescore=rescore)[3].size == 0  # nq = 0
    finally:
        ix.close()


REFUSED = {"plain_storage": (STATE, 10, 50, 0), "k_0": (INVALID, 0, 50, 1), "k_65": (INVALID, 65, 70, 1), "rescore_below_k": (INVALID, 10, 9, 1),
           "rescore_4097": (INVALID, 10, 4097, 1), "slot_65": (INVALID, 10, 50, 65), "empty_slot": (STATE, 10, 50, 2)}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refusals_write_nothing(gpu_ctx, oracle, case):
    code, k, rescore, slot = REFUSED[case]
    dim, tids = 40, _live_tids(N)
    ix = _upload(gpu_ctx, corpus(dim, O.L2)[0], tids, O.L2, plain=True) if case == "plain_storage" else upload(gpu_ctx, dim, O.L2, tids)
    try:
        if case != "plain_storage":
            ix.qual_put(1, np.arange(N) % 3 == 0)
        q = make_vectors(5, dim, 2, "gauss")
        assert _device_call(gpu_ctx, ix, q, np.full(5, slot, np.uint32), k, rescore) == (code, True)
    finally:
        ix.close()
