"""The rerank order of a batch keyed by the region labels kept per corpus row (VS_RERANK_ORDER=3, and 1 where the rule orders):
label[i] = the seed row s * (n / S) whose code is nearest to row i's by Hamming distance (lowest seed among equals), key(q) = the
label of the first row of q's stream (S for a scan without a row: last), perm = the scan numbers stably sorted by key.  As with the
seed pass on the query codes (tests/test_gpu_zzz_rerank_order.py) only the order in which workgroups take the scans may change: node
ids in order, heap TIDs, distance bits and the counters must be the oracle's, and the reported permutation must be the numpy
reference's — also after everything that changes codes or row numbers on one index (quantising again, an insert, delete +
consolidate, compact), where stale labels would show as another permutation.  Also runs on the lockstep interpreter (VS_EMU=1)."""
import numpy as np
import pytest

from lifecycle_checks import EMU, fresh_index, make_tids, oracle_of
from oracle import oracle_py as O
from test_gpu_zzz_rerank_window import COUNTERS, INVALID, Corpus, tie_vectors

pytestmark = pytest.mark.gpu

LABEL_SEEDS = 2048  # the library's default seed count of the labels (VS_RERANK_SEEDS unset)
POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], np.uint16)


def region_labels(codes, seeds):
    """-> (labels [n], S): nearest seed row of every row's code, lowest seed among equals"""
    n = len(codes)
    S = min(seeds, n)
    sc = codes[np.arange(S) * (n // S)]
    lab = np.empty(n, np.int64)
    for r0 in range(0, n, 512):
        x = np.ascontiguousarray(codes[r0:r0 + 512, None, :] ^ sc[None, :, :])
        lab[r0:r0 + 512] = POP16[x.view(np.uint16)].sum(axis=2, dtype=np.int64).argmin(axis=1)
    return lab, S


def expected_order(codes, seeds, first_rows):
    lab, S = region_labels(codes, seeds)
    first_rows = np.asarray(first_rows, np.int64)
    has = first_rows != INVALID
    key = np.where(has, lab[np.where(has, first_rows, 0)], S)
    return np.argsort(key, kind="stable").astype(np.uint32)


def set_opts(**kw):
    import pgvectorscale_amd as P
    for name, v in kw.items():
        P.set_option(name, v)


def reset_opts():
    set_opts(VS_RERANK_ORDER=None, VS_RERANK_DEAL=None, VS_RERANK_SEEDS=None)


def check_batch(ix, oidx, codes, tids, q, L, rescore, k, order, deal, seeds, qlabels=None, where=""):
    """one batch under the given options against the oracle; -> the reported permutation"""
    tag = (where, order, deal, seeds)
    oi, od, ost = oidx.search_batch(q, L=L, rescore=rescore, k=k, qlabels=qlabels)
    set_opts(VS_RERANK_ORDER=order, VS_RERANK_DEAL=deal, VS_RERANK_SEEDS=seeds)
    gi, gt, gd, gst = ix.search_batch(q, search_list_size=L, rescore=rescore, k=k, qlabels=qlabels)
    perm = ix.rerank_order()
    assert (gi == oi).all(), (tag, np.argwhere(gi != oi)[:5])
    live = gi != INVALID
    assert (gt[live] == tids[gi[live]]).all() and (gt[~live] == 0).all(), tag
    assert (gd.view(np.uint32)[live] == od.view(np.uint32)[live]).all(), tag
    assert np.isnan(gd[~live]).all(), tag
    for key in COUNTERS:
        assert gst[key] == ost[key], (tag, key, gst[key], ost[key])
    if order == 3:
        first = oidx.stream_batch(q, L=L, m=1, qlabels=qlabels)[0][:, 0]
        want = expected_order(codes, seeds or LABEL_SEEDS, first)
        assert perm.size == len(q) and (np.sort(perm) == np.arange(len(q))).all(), (tag, perm)
        assert (perm == want).all(), (tag, perm, want)
    else:
        assert perm.size == 0, tag  # by rule: a batch this small is not ordered
    return perm


@pytest.fixture(scope="module")
def ties():
    return Corpus(tie_vectors(3000, 300, 64, seed=3))


# (the batch sizes of tests/test_gpu_zzz_rerank_order.py: fewer scans than XCDs, not a multiple of 8, one and several tiles)
@pytest.mark.parametrize("nq", [5, 27, 64, 200])
def test_forced_label_order(gpu_ctx, ties, nq):
    q = np.vstack([ties.vecs[:3], np.random.default_rng(nq).random((nq - 3, 64), dtype=np.float32)])
    ix = ties.upload(gpu_ctx)
    try:
        for order, deal, seeds in ((3, 1, 1024), (3, 0, 1024), (3, 1, 70), (3, 0, 70), (3, 1, None), (1, 1, None)):
            check_batch(ix, ties.oracle, ties.codes, ties.tids, q, 40, 20, 10, order, deal, seeds)
    finally:
        reset_opts()
        ix.close()


def test_scans_without_a_row_go_last(gpu_ctx):
    """label keys that no node carries: those scans have no start node, their streams are empty, their key is S"""
    c = Corpus(tie_vectors(600, 150, 64, seed=8), n_labels=3)
    nq = 21
    q = np.random.default_rng(9).random((nq, 64), dtype=np.float32)
    qlabels = [[50] if i % 4 == 1 else [1 + i % 3] for i in range(nq)]
    first = c.oracle.stream_batch(q, L=30, m=1, qlabels=qlabels)[0][:, 0]
    assert (first == INVALID).sum() == len([i for i in range(nq) if i % 4 == 1])
    ix = c.upload(gpu_ctx)
    try:
        for seeds in (1024, 70):
            perm = check_batch(ix, c.oracle, c.codes, c.tids, q, 30, 16, 10, 3, 1, seeds, qlabels=qlabels)
            assert (np.sort(perm[-(first == INVALID).sum():]) == np.flatnonzero(first == INVALID)).all()
    finally:
        reset_opts()
        ix.close()


def test_corpus_smaller_than_the_seed_count(gpu_ctx):
    """9 rows: every row is a seed and its own label; streams shorter than M"""
    small = Corpus(np.random.default_rng(2).random((9, 32), dtype=np.float32), R=8, L_build=10)
    q = np.random.default_rng(4).random((11, 32), dtype=np.float32)
    ix = small.upload(gpu_ctx)
    try:
        for seeds in (1024, 4):
            check_batch(ix, small.oracle, small.codes, small.tids, q, 20, 50, 5, 3, 1, seeds)
    finally:
        reset_opts()
        ix.close()


# (the interpreter runs 500 rows: 300 seeds keep what 1 024 are for on the device — fewer seeds than rows, and n / S unmoved by 50 more rows)
@pytest.mark.parametrize("seeds", [300 if EMU else 1024, 70])
def test_labels_follow_the_index(gpu_ctx, seeds):
    """one index through everything that moves codes or row numbers (70 seeds: 50 more rows also move the seed rows; 1 024: they do
    not, the new rows are labelled in place); the permutation after every step is the one of the arrays as they stand.  Two steps
    really change the codes of existing rows at an unchanged n and S — another quantiser, a write through the array's pointer — so
    that only the codes epoch can have told the library"""
    from pgvectorscale_amd import _lib
    n0 = 500 if EMU else 3000
    X = tie_vectors(n0 + 50, 300, 64, seed=3)
    tids = make_tids(0, n0)
    q = np.vstack([X[:3], np.random.default_rng(21).random((61, 64), dtype=np.float32)])
    ix = fresh_index(gpu_ctx, X[:n0], distance=O.L2, R=24, L=40, tids=tids)

    def step(where, stale=None):
        """the batches under test on the index as it stands; stale: the codes before the step — labels left over from them would show,
        because they order this batch differently"""
        ix._refresh()
        host = ix.download(vecs=True)
        oidx = oracle_of(O, ix, host, O.L2)
        for deal in (1, 0):
            check_batch(ix, oidx, host["codes"], host["heap_tids"], q, 40, 20, 10, 3, deal, seeds, where=where)
        if stale is not None:
            first = oidx.stream_batch(q, L=40, m=1)[0][:, 0]
            assert (stale != host["codes"]).any(), where
            assert (expected_order(stale, seeds, first) != expected_order(host["codes"], seeds, first)).any(), where
        return host["codes"]

    try:
        codes = step("built")
        ix.sbq_quantize_corpus()
        step("quantised again")
        mean, m2, cnt = ix.get_quantizer()
        ix.set_quantizer(mean + np.float32(0.12), m2, cnt)  # (other thresholds: most rows get another code)
        ix.sbq_quantize_corpus()
        step("quantised with another quantiser", stale=codes)
        st = ix.insert(X[n0:], make_tids(n0, 50), search_list_size=40)
        assert st["inserted"] == 50 and ix.desc.n == n0 + 50
        step("50 rows inserted")
        dead = np.random.default_rng(5).choice(n0 + 50, 120, replace=False).astype(np.uint32)
        ix.mark_deleted(dead)
        ix.consolidate_deletes()
        step("deleted and consolidated")
        ix.compact()
        assert n0 + 50 - 120 <= ix.desc.n < n0 + 50  # (rows have new numbers)
        codes = step("compacted")
        # the caller writes other codes through the array's pointer: only the hand-out tells the library
        ptr, stride = ix.array(_lib.ARR_CODES)
        rows = np.zeros((len(codes), stride), np.uint64)
        rows[:, :codes.shape[1]] = np.roll(codes, 7, axis=0)
        gpu_ctx.upload(ptr, rows)
        step("codes overwritten through vs_index_array", stale=codes)
    finally:
        reset_opts()
        ix.close()
