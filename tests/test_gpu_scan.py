"""K5 flat SBQ scan (vs_scan_topk) and the exact brute force (vs_bruteforce_topk) against numpy / the oracle.
Hamming ranking is bit-exact with ties broken by node id; brute-force distances are bit-identical to the oracle's
AVX2-order distance (asserted at the 1e-5 bar of north_star).  Every instantiation of the scan kernel (query tile x chunk count) and
its refusals are here; the step loop at sizes taken from the device is in test_gpu_scan_steps.py, the brute force over several chunks
and at its special values in test_gpu_scan_bruteforce.py."""
import contextlib
import os
import re

import numpy as np
import pytest

from helpers import cached_index

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 0xFFFFFFFF


@contextlib.contextmanager
def options(**kv):
    from pgvectorscale_amd.index import set_option
    for k, v in kv.items():
        set_option(k, v)
    try:
        yield
    finally:
        for k in kv:
            set_option(k, None)


def _popcount(a):
    a = a.copy()
    a = a - ((a >> np.uint64(1)) & np.uint64(0x5555555555555555))
    a = (a & np.uint64(0x3333333333333333)) + ((a >> np.uint64(2)) & np.uint64(0x3333333333333333))
    a = (a + (a >> np.uint64(4))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    return ((a * np.uint64(0x0101010101010101)) >> np.uint64(56)).astype(np.uint32)


def _flat_index(gpu_ctx, codes):
    import pgvectorscale_amd as P
    n, words = codes.shape
    return P.DiskAnnIndex.upload(gpu_ctx, codes=codes, nbrs=np.full((n, 4), 0xFFFFFFFF, np.uint32),
                                 heap_tids=np.ones(n, np.uint64), vecs=None, mean=np.zeros(words * 64, np.float32),
                                 m2=None, count=1, bits=1, dim_index=words * 64, num_neighbors=4, distance_type=P.VS_L2,
                                 default_start=0)


@pytest.mark.parametrize("words,n,nq,k", [(24, 20011, 19, 10), (4, 5000, 8, 64), (12, 70001, 3, 1), (48, 3001, 9, 17),
                                          (3, 100, 2, 10), (24, 7, 1, 10)])
def test_scan_topk_exact(gpu_ctx, words, n, nq, k):
    rng = np.random.default_rng(words * 1000 + n)
    # few distinct values per word => many Hamming ties, so the (hamming, id) tie rule is exercised
    codes = rng.integers(0, 4, (n, words), dtype=np.uint64) * np.uint64(0x0101010101010101)
    qcodes = rng.integers(0, 4, (nq, words), dtype=np.uint64) * np.uint64(0x0101010101010101)
    ix = _flat_index(gpu_ctx, codes)
    ids, ham = ix.scan_topk(qcodes, k)
    for q in range(nq):
        d = _popcount(codes ^ qcodes[q]).sum(axis=1).astype(np.int64)
        order = np.lexsort((np.arange(n), d))[:k]
        want_ids = np.full(k, 0xFFFFFFFF, np.uint32)
        want_ham = np.full(k, 0xFFFFFFFF, np.uint32)
        want_ids[:len(order)] = order
        want_ham[:len(order)] = d[order]
        assert (ids[q] == want_ids).all(), (q, ids[q], want_ids)
        assert (ham[q] == want_ham).all()
    ix.close()


def _tied_codes(rng, rows, words):
    """few distinct values per word => ties at the k-th place are the rule"""
    return rng.integers(0, 4, (rows, words), dtype=np.uint64) * np.uint64(0x0101010101010101)


def _check_against_lexsort(codes, qcodes, k, ids, ham):
    n = len(codes)
    assert ids.shape == ham.shape == (len(qcodes), k)
    for q in range(len(qcodes)):
        d = _popcount(codes ^ qcodes[q]).sum(axis=1).astype(np.int64)
        order = np.lexsort((np.arange(n), d))[:k]
        want_ids = np.full(k, INV, np.uint32)
        want_ham = np.full(k, INV, np.uint32)
        want_ids[:len(order)] = order
        want_ham[:len(order)] = d[order]
        assert (ids[q] == want_ids).all(), (q, ids[q], want_ids)
        assert (ham[q] == want_ham).all(), (q, ham[q], want_ham)


# every chunk-count instantiation NCH of k_scan_topk at both ends of its range of code widths (1-8 words: 1, 9-16: 2, 17-24: 3,
# 25-32: 4, 33-48: 6, where 33-40 words need five chunks and run the <6> instantiation with a sixth chunk that loads nothing);
# odd widths have a stride padded to even
SCAN_WORDS = (1, 8, 9, 16, 17, 25, 32, 33, 39, 47, 48)
SCAN_TILES = (4, 8, 16)
# words x tile is complete; k walks 1, 10, 64 along it so that every k meets every tile (11 widths per tile, k of period 3)
SCAN_MATRIX = [(w, t, (1, 10, 64)[(wi + ti) % 3]) for wi, w in enumerate(SCAN_WORDS) for ti, t in enumerate(SCAN_TILES)]


@pytest.mark.parametrize("words,tile,k", SCAN_MATRIX)
def test_scan_topk_every_instantiation(gpu_ctx, words, tile, k):
    n, nq = 1511, 2 * tile + 3  # n is no multiple of the 64-row step; the third tile of queries is ragged (3 of Q)
    rng = np.random.default_rng(words * 100 + tile)
    codes, qcodes = _tied_codes(rng, n, words), _tied_codes(rng, nq, words)
    ix = _flat_index(gpu_ctx, codes)
    try:
        with options(VS_SCAN_Q=tile):
            ids, ham = ix.scan_topk(qcodes, k)
    finally:
        ix.close()
    _check_against_lexsort(codes, qcodes, k, ids, ham)


@pytest.mark.parametrize("tile", SCAN_TILES)
@pytest.mark.parametrize("n,k", [(7, 10), (1, 64), (1, 1)])
def test_scan_topk_fewer_rows_than_k(gpu_ctx, n, k, tile):
    rng = np.random.default_rng(n + k)
    codes, qcodes = _tied_codes(rng, n, 5), _tied_codes(rng, tile + 1, 5)
    ix = _flat_index(gpu_ctx, codes)
    try:
        with options(VS_SCAN_Q=tile):
            ids, ham = ix.scan_topk(qcodes, k)
    finally:
        ix.close()
    _check_against_lexsort(codes, qcodes, k, ids, ham)
    assert (ids[:, min(n, k):] == INV).all() and (ham[:, min(n, k):] == INV).all()


def _argument_error_code():
    """what VS_REQUIRE returns (vs_internal.h), by its value in the public header"""
    macro = open(os.path.join(ROOT, "pgvectorscale_amd", "csrc", "vs_internal.h")).read()
    name = re.search(r"#define VS_REQUIRE\(cond, \.\.\.\).*?return (\w+);", macro, re.S).group(1)
    return int(re.search(name + r" = (-?\d+)", open(os.path.join(ROOT, "include", "vsgpu.h")).read()).group(1))


def test_flat_scan_refusals(gpu_ctx):
    """arguments the flat scan refuses before it launches anything, and the empty batch"""
    import pgvectorscale_amd as P
    invalid = _argument_error_code()
    assert invalid == -1
    rng = np.random.default_rng(1)
    codes, qcodes = _tied_codes(rng, 200, 4), _tied_codes(rng, 3, 4)
    ix = _flat_index(gpu_ctx, codes)
    try:
        gpu_ctx.profile_read()
        gpu_ctx.profile_enable(True)
        for k in (0, 65):
            for kw in ({}, dict(live_only=True)):
                with pytest.raises(P.VsError, match=r"k must be in \[1, 64\]") as e:
                    ix.scan_topk(qcodes, k, **kw)
                assert e.value.code == invalid
        ids, ham = ix.scan_topk(qcodes[:0], 10)
        assert ids.shape == ham.shape == (0, 10) and ids.dtype == ham.dtype == np.uint32
        ids, ham = ix.scan_topk(qcodes[:0], 10, live_only=True)
        assert ids.shape == ham.shape == (0, 10)
        assert gpu_ctx.profile_read()["scan"][1] == 0  # nothing was launched
        ids, _ = ix.scan_topk(qcodes, 64)  # the index still scans
        assert gpu_ctx.profile_read()["scan"][1] == 1 and (ids[:, 0] != INV).all()
    finally:
        gpu_ctx.profile_enable(False)
        ix.close()
    # 49 words: stride 50, seven chunks of four lanes x 16 B — one more than the widest instantiation
    wide = _flat_index(gpu_ctx, _tied_codes(rng, 100, 49))
    try:
        gpu_ctx.profile_enable(True)
        with pytest.raises(P.VsError, match="not supported by the flat scan") as e:
            wide.scan_topk(_tied_codes(rng, 2, 49), 10)
        assert e.value.code == invalid
        assert gpu_ctx.profile_read()["scan"][1] == 0
    finally:
        gpu_ctx.profile_enable(False)
        wide.close()


def test_scan_topk_matches_oracle_hamming(gpu_ctx, oracle):
    ti = cached_index(n=3000, dim_full=96, R=24, seed=5)
    ix = ti.upload(gpu_ctx)
    Q = ti.queries(11, seed=3)
    qcodes = oracle.quantize(ti.mean, ti.m2, ti.count, ti.bits, Q)
    ids, ham = ix.scan_topk(qcodes, 10)
    want_ids, want_ham = oracle.hamming_scan_topk(ti.codes, qcodes, 10)
    assert (ids == want_ids).all()
    assert (ham == want_ham).all()
    ix.close()


@pytest.mark.parametrize("distance", ["l2", "cosine", "ip"])
def test_bruteforce_topk_matches_oracle(gpu_ctx, oracle, distance):
    O = oracle
    dt = {"l2": O.L2, "cosine": O.COSINE, "ip": O.IP}[distance]
    ti = cached_index(n=2500, dim_full=72, R=16, seed=9, distance=dt, kind="gauss")
    ix = ti.upload(gpu_ctx)
    Q = ti.queries(7, seed=4, kind="gauss")
    dq = gpu_ctx.alloc(Q.nbytes)
    gpu_ctx.upload(dq, Q)
    ids, dist = ix.bruteforce_topk(dq, len(Q), 10)
    gt_ids, gt_d = ti.oracle.bruteforce(Q, k=10)
    assert (ids == gt_ids).all()
    assert np.allclose(dist, gt_d, rtol=1e-5, atol=0)
    assert (dist.view(np.uint32) == np.asarray(gt_d, np.float32).view(np.uint32)).all()
    gpu_ctx.free(dq)
    ix.close()


def test_scan_topk_filtered_is_the_exact_filtered_ranking(gpu_ctx, oracle):
    """vs_scan_topk_filtered: exact SBQ top-k among the rows a label-filtered scan may return (label sets overlap, an empty key
    filters nothing, deleted tuples skipped with live_only) — against the oracle twin, with keys from common to absent labels,
    and as the upper bound of what the label-filtered graph walk finds (its stream is a subsequence of this ranking's rows)."""
    ti = cached_index(n=3000, dim_full=64, bits=2, R=32, distance=1, seed=11, kind="gauss", L_build=64, n_labels=6, deleted_frac=0.1)
    ix = ti.upload(gpu_ctx)
    q = ti.queries(24, seed=3, kind="gauss")
    qcodes = ix.quantize(q)
    rng = np.random.default_rng(4)
    keys = [sorted(set(int(v) for v in rng.integers(1, 7, int(rng.integers(0, 3))))) for _ in range(len(q))]
    keys[0], keys[1], keys[2] = [], [6], [99]  # no filter / one label / a label nobody carries
    for live in (False, True):
        for k in (1, 10, 64):
            oi, oh = oracle.hamming_scan_topk(ti.codes, qcodes, k, label_off=ti.label_off, label_val=ti.label_val,
                                              heap_tids=ti.tids if live else None, qlabels=keys)
            gi, gh = ix.scan_topk(qcodes, k, qlabels=keys, live_only=live)
            assert (gi == oi).all() and (gh == oh).all()
            # every tile width: the key of query q0 + qi in the second and later tiles (24 queries: 6, 3 and 2 tiles, the last of
            # 16 ragged)
            for tile in SCAN_TILES:
                with options(VS_SCAN_Q=tile):
                    gi, gh = ix.scan_topk(qcodes, k, qlabels=keys, live_only=live)
                assert (gi == oi).all() and (gh == oh).all(), (live, k, tile)
    assert (gi[2] == 0xFFFFFFFF).all()
    # no key at all = the plain flat scan
    a, _ = ix.scan_topk(qcodes, 10)
    b, _ = ix.scan_topk(qcodes, 10, qlabels=[[] for _ in keys])
    assert (a == b).all()
    # the graph walk's SBQ-ordered stream only ever returns rows of the filtered set, at Hamming distances no smaller than the
    # exact ranking's at the same position
    si, sh, _ = ix.stream_batch(q[3:], search_list_size=100, m=10, qlabels=keys[3:])
    gi, gh = ix.scan_topk(qcodes[3:], 10, qlabels=keys[3:], live_only=True)
    live = sh != 0xFFFFFFFF
    assert (sh[live] >= gh[live]).all()
    ix.close()
