"""The exact and the flat qualified top-k for k up to 4096 (vs_search_batch_qual_exact_wide / vs_search_batch_qual_flat_wide and their
_dev forms, vs_qual_wide.h).  The references are those of the narrow calls' tests: OracleIndex.bruteforce(k=...) with the tid offsets
zeroed outside C (test_gpu_zz_qual_exact.expect), and oracle_py.hamming_scan_topk for S, then the same brute force
(test_gpu_zz_qual_flat.expect).  Ids and rows are compared with `==`, tids where the id is valid, distances by bit pattern, the
(INVALID, NaN) tail included.  Also runs on the lockstep interpreter (tests/test_emu_qual_wide.py)."""
import numpy as np
import pytest

import test_gpu_zz_qual_flat as F
from helpers import make_vectors, tie_vectors
from oracle import oracle_py as O
from test_gpu_scan_bruteforce import DISTANCES, INV, _bits, _delete, _live_tids, _special_corpus, _upload
from test_gpu_zz_qual import options
from test_gpu_zz_qual_exact import assert_equal, expect

pytestmark = pytest.mark.gpu
N = 5989  # the last bitmap word is partial; more than 4096 rows stay live and visible
INVALID, STATE = -1, -5
CASES = [(dim, d, st, (1, 64, 65, 100, 1000, 4096)[(i + i // 6) % 6]) for i, (dim, d, st) in
         enumerate((dim, d, st) for dim in (8, 40, 96) for d in DISTANCES for st in ("sbq", "plain"))]


def as_exp(got):
    return got[0], got[1], _bits(got[2]), got[3]


def device_call(gpu_ctx, fn, q, slots, k, *after_k):
    """a _dev form over poisoned buffers of its own -> (ids, tids, dist, rows) or, refused, the error code and whether nothing was written"""
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
            fn(bufs[0], nq, k, *after_k, bufs[1], bufs[2], bufs[5], d_out_tids=bufs[3], d_out_dist=bufs[4])
        except P.VsError as e:
            return e.code, all((gpu_ctx.download(b, a).view(np.uint8) == 0xA5).all() for b, a in zip(bufs[2:], outs))
        return [gpu_ctx.download(b, a) for b, a in zip(bufs[2:], outs)]
    finally:
        for b in bufs:
            gpu_ctx.free(b)


@pytest.mark.parametrize("dim,distance,storage,k", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_exact_wide_list_lengths_and_k_with_deleted_and_hidden_rows(gpu_ctx, oracle, dim, distance, storage, k):
    """dim 8: the tail only; 40: one step plus a tail; 96: steps only.  Qualifiers with |C| = 0, 1, k - 1, k, k + 1 and 1 500 (dozens
    of slices), each with a deleted and a hidden row among its bits, plus slot 0 (|C| > 4096) in one interleaved batch."""
    dt, plain = DISTANCES[distance], storage == "plain"
    rng = np.random.default_rng(dim + k)
    vecs = make_vectors(N, dim, dim, "gauss") * rng.uniform(0.2, 3.0, (N, 1)).astype(np.float32)
    vecs[:40:4] = 0                                                     # divisor 0: zero rows ...
    vecs[1:40:4] /= np.linalg.norm(vecs[1:40:4], axis=1, keepdims=True)  # ... and rows that are unit already
    tids = _live_tids(N)
    _delete(tids, rng.random(N) < 0.05)
    hidden = rng.random(N) < 0.05
    live = tids & np.uint64(0xFFFF) != 0
    inside = np.flatnonzero(live & ~hidden)
    lengths = [0, 1, k - 1, k, k + 1, 1500]
    assert len(inside) > max(4096, k + 1)
    quals = {}
    for s, m in enumerate(lengths, start=1):
        quals[s] = np.zeros(N, bool)
        quals[s][rng.choice(inside, m, replace=False)] = True
        quals[s][[np.flatnonzero(~live)[s], np.flatnonzero(hidden & live)[s]]] = True
    ix = _upload(gpu_ctx, vecs, tids, dt, plain)
    try:
        ix.set_visibility((~hidden).astype(np.uint8))
        for s, b in quals.items():
            ix.qual_put(s, b)
        tq = ix.search_batch_qual_exact_wide(vecs[:1], np.zeros(1, np.uint32), k=k)[4]["tile_queries"]
        per_slot = [tq + 1, 1, 2, 1, tq, 2, tq + 1]
        slots = rng.permutation(np.repeat(np.arange(7, dtype=np.uint32), per_slot))
        q = make_vectors(len(slots), dim, dim + 1, "gauss")
        exp = expect(vecs, tids, dt, plain, q, slots, quals, k, hidden)
        for s, m in enumerate(lengths, start=1):
            assert (exp[3][slots == s] == min(k, m)).all()
        got = ix.search_batch_qual_exact_wide(q, slots, k=k)
        assert_equal(got, exp)
        st = got[4]
        assert (st["tile_queries"], st["lists"], st["rows_listed"]) == (tq, 7, sum(lengths) + len(inside))
        assert st["tiles"] == sum(-(-c // tq) for c in per_slot)
        assert_equal(device_call(gpu_ctx, ix.search_batch_qual_exact_wide_dev, q, slots, k), exp, "_dev")
    finally:
        ix.close()


def test_ties_at_the_threshold_break_by_node_id_under_forced_slices_tiles_and_chunks(gpu_ctx, oracle):
    k, dim, nq, n = 100, 40, 9, 2037
    vecs, q, tids = tie_vectors(n, 40, dim, 5), tie_vectors(nq, 40, dim, 7), _live_tids(n)
    bits = np.zeros(n, bool)
    bits[np.random.default_rng(8).choice(n, 700, replace=False)] = True
    slots = np.ones(nq, np.uint32)
    wider = expect(vecs, tids, O.L2, False, q, slots, {1: bits}, k + 2)[2]
    # at least three equal keys straddle the cut: how many of them are taken (k - rows below) decides, and which by node id
    assert ((wider[:, k - 1] == wider[:, k]) & ((wider[:, k - 2] == wider[:, k - 1]) | (wider[:, k] == wider[:, k + 1]))).any()
    exp = expect(vecs, tids, O.L2, False, q, slots, {1: bits}, k)
    ix = _upload(gpu_ctx, vecs, tids, O.L2)
    try:
        ix.qual_put(1, bits)
        for S, T, mb in [(1, 8, 1024), (3, 8, 1024), (11, 1, 1024), (2, 2, 1024), (2, 8, 0), (22, 4, 0)]:  # every instantiation of the tile
            with options(VS_QUAL_EXACT_SLICES=S, VS_QUAL_EXACT_TQ=T, VS_QUAL_WIDE_WS_MB=mb):
                got = ix.search_batch_qual_exact_wide(q, slots, k=k)
            assert_equal(got, exp, f"{S} slices, tiles of {T}, {mb} MiB")
            assert (got[4]["slices"], got[4]["tile_queries"], got[4]["tiles"]) == (S, T, -(-nq // T))
    finally:
        ix.close()


@pytest.mark.parametrize("distance", ["l2", "ip"])
def test_keys_that_share_their_leading_digit_are_told_apart_by_the_later_levels(gpu_ctx, oracle, distance):
    """one base vector plus a perturbation of 1e-4: every distance of C has the same top 16 bits (positive keys under L2, negative
    ones — the inverted image of total_cmp — under inner product), so the first selection level decides nothing"""
    k, dim, nq, n = 300, 40, 3, 2037
    base = np.full(dim, np.sqrt(1.50390625 / dim), np.float32)  # |base|^2 sits in the middle of a 16-bit prefix
    vecs = base + 1e-4 * make_vectors(n, dim, 1, "gauss")
    q = (2 if distance == "l2" else 1) * base + 1e-5 * make_vectors(nq, dim, 2, "gauss")
    tids = _live_tids(n)
    bits = np.random.default_rng(3).random(n) < 0.7
    slots = np.ones(nq, np.uint32)
    full = expect(vecs, tids, DISTANCES[distance], False, q, slots, {1: bits}, int(bits.sum()))[2]
    assert (full >> 16 == full[0, 0] >> 16).all() and (full[0, 0] >> 31 == (distance == "ip"))
    assert all(len(np.unique(row)) > 1000 for row in full)
    ix = _upload(gpu_ctx, vecs, tids, DISTANCES[distance])
    try:
        ix.qual_put(1, bits)
        assert_equal(ix.search_batch_qual_exact_wide(q, slots, k=k), expect(vecs, tids, DISTANCES[distance], False, q, slots, {1: bits}, k))
    finally:
        ix.close()


@pytest.mark.parametrize("distance", ["l2", "ip"])
def test_nan_inf_and_negative_zero_order_by_total_cmp_key_with_k_above_the_rows(gpu_ctx, oracle, distance):
    vecs, q, tids = _special_corpus()
    bits = np.random.default_rng(9).random(len(vecs)) < 0.3
    bits[[5, 6, 7, 8, 9, 10, 11, 12, 41, 201, 220, 225]] = True
    slots = (np.arange(len(q)) % 2).astype(np.uint32)
    exp = expect(vecs, tids, DISTANCES[distance], False, q, slots, {1: bits}, 500)
    d = exp[2].view(np.float32)[exp[0] != INV]
    assert np.isnan(d).any() and np.isinf(d).any() and (np.signbit(d) & ((d == 0) | np.isnan(d))).any() and (exp[3] < 500).all()
    ix = _upload(gpu_ctx, vecs, tids, DISTANCES[distance])
    try:
        ix.qual_put(1, bits)
        assert_equal(ix.search_batch_qual_exact_wide(q, slots, k=500), exp)
    finally:
        ix.close()


def test_wide_equals_narrow_up_to_64_and_flat_wide_with_a_full_rescore_equals_exact_wide(gpu_ctx, oracle):
    dim, dt = 96, O.COSINE
    tids = _live_tids(F.N)
    _delete(tids, np.arange(F.N) % 17 == 3)
    slots = (np.arange(11) % 2).astype(np.uint32)
    q = make_vectors(len(slots), dim, 9, "gauss")
    ix = F.upload(gpu_ctx, dim, dt, tids)
    try:
        ix.qual_put(1, np.random.default_rng(4).random(F.N) < 0.1)
        for k in (10, 64):
            assert_equal(ix.search_batch_qual_exact_wide(q, slots, k=k), as_exp(ix.search_batch_qual_exact(q, slots, k=k)), f"exact, k {k}")
            assert_equal(ix.search_batch_qual_flat_wide(q, slots, k=k, rescore=70), as_exp(ix.search_batch_qual_flat(q, slots, k=k, rescore=70)),
                         f"flat, k {k}")
        exact = ix.search_batch_qual_exact_wide(q, slots, k=300)
        assert (exact[3][slots == 0] == 300).all() and (exact[3][slots == 1] < 300).all()
        assert_equal(ix.search_batch_qual_flat_wide(q, slots, k=300, rescore=4096), as_exp(exact))  # slot 0: |C| = 1 917
    finally:
        ix.close()


FLAT = [(40, "l2", 65, 65), (96, "cosine", 300, 300), (40, "ip", 300, 4096), (40, "l2", 4096, 4096)]


@pytest.mark.parametrize("dim,distance,k,rescore", FLAT, ids=["-".join(map(str, c)) for c in FLAT])
def test_flat_wide_against_the_oracle_s_candidates_and_brute_force(gpu_ctx, oracle, dim, distance, k, rescore):
    dt = DISTANCES[distance]
    rng = np.random.default_rng(k + rescore)
    tids = _live_tids(F.N)
    _delete(tids, rng.random(F.N) < 0.05)
    hidden = rng.random(F.N) < 0.05
    quals = {1: rng.random(F.N) < 0.4, 2: rng.random(F.N) < 0.02}  # |C| above rescore where it is not 4096; below k
    slots = (np.arange(7) % 3).astype(np.uint32)
    q = make_vectors(len(slots), dim, dim + 1, "gauss")
    exp = F.expect(dim, dt, tids, q, slots, quals, k, rescore, hidden)
    in_1 = int((quals[1] & (tids & np.uint64(0xFFFF) != 0) & ~hidden).sum())
    assert (exp[3][slots == 2] < min(k, 65)).all() and (exp[3][slots == 1] == min(k, rescore, in_1)).all() and in_1 > 300
    ix = F.upload(gpu_ctx, dim, dt, tids)
    try:
        ix.set_visibility((~hidden).astype(np.uint8))
        for s, b in quals.items():
            ix.qual_put(s, b)
        got = ix.search_batch_qual_flat_wide(q, slots, k=k, rescore=rescore)
        F.assert_equal(got, exp)
        assert got[4]["reranked"] == exp[4]
        F.assert_equal(device_call(gpu_ctx, ix.search_batch_qual_flat_wide_dev, q, slots, k, rescore), exp, "_dev")
    finally:
        ix.close()


#          (call, code, k, rescore, slot)
REFUSED = {"exact_k_0": ("exact", INVALID, 0, None, 1), "exact_k_4097": ("exact", INVALID, 4097, None, 1), "exact_empty_slot": ("exact", STATE, 100, None, 2),
           "flat_k_0": ("flat", INVALID, 0, 50, 1), "flat_k_4097": ("flat", INVALID, 4097, 4097, 1), "flat_rescore_below_k": ("flat", INVALID, 100, 99, 1),
           "flat_rescore_4097": ("flat", INVALID, 100, 4097, 1), "flat_empty_slot": ("flat", STATE, 100, 200, 2),
           "flat_plain_storage": ("flat", STATE, 100, 200, 0)}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refusals_write_nothing(gpu_ctx, oracle, case):
    call, code, k, rescore, slot = REFUSED[case]
    dim, tids = 40, _live_tids(F.N)
    ix = _upload(gpu_ctx, F.corpus(dim, O.L2)[0], tids, O.L2, plain=True) if "plain" in case else F.upload(gpu_ctx, dim, O.L2, tids)
    try:
        ix.qual_put(1, np.arange(F.N) % 3 == 0)
        q, slots = make_vectors(5, dim, 2, "gauss"), np.full(5, slot, np.uint32)
        if call == "exact":
            assert device_call(gpu_ctx, ix.search_batch_qual_exact_wide_dev, q, slots, k) == (code, True)
        else:
            assert device_call(gpu_ctx, ix.search_batch_qual_flat_wide_dev, q, slots, k, rescore) == (code, True)
    finally:
        ix.close()
