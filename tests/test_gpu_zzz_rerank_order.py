"""The rerank order of a batch (VS_RERANK_ORDER: k_scan_regions, the counting sort, the `perm` / per-XCD dealing of k_rerank_window and
k_rerank) against the oracle and against the option switched off.  Only the order in which workgroups take the scans may change: node
ids in order, heap TIDs, distance bits and the counters must be those of the oracle under every setting, and the order itself must be
a permutation of the scan numbers, sorted by (nearest seed row, scan number).  Also runs on the lockstep interpreter (VS_EMU=1)."""
import numpy as np
import pytest

from oracle import oracle_py as O
from test_gpu_zzz_rerank_window import COUNTERS, INVALID, Corpus, tie_vectors

pytestmark = pytest.mark.gpu

# (VS_RERANK_ORDER, VS_RERANK_DEAL, VS_RERANK_SEEDS): off, by rule (off at these sizes), forced with / without the per-XCD split,
# forced with a seed count that is not a multiple of the kernel's tile
SETTINGS = ((0, 1, None), (1, 1, None), (2, 1, None), (2, 0, None), (2, 1, 70))


def set_opts(P, **kw):
    for name, v in kw.items():
        P.set_option(name, v)


def expected_order(corpus, q, seeds):
    """the order the library must produce, from the oracle's codes: key = nearest seed row by Hamming distance (lowest seed among
    equals), stable by scan number"""
    rows = np.ascontiguousarray(q, np.float32).copy()
    if corpus.distance == O.COSINE:
        for i in range(len(rows)):
            rows[i] = O.preprocess_cosine(rows[i])[0]
    qc = O.quantize(corpus.mean, corpus.m2, corpus.count, corpus.bits, rows)
    S = min(seeds, corpus.n)
    sc = corpus.codes[np.arange(S) * (corpus.n // S)]
    ham = np.zeros((len(qc), S), np.int64)
    for w in range(qc.shape[1]):
        x = qc[:, None, w] ^ sc[None, :, w]
        ham += np.unpackbits(np.ascontiguousarray(x).view(np.uint8).reshape(len(qc), S, 8), axis=2).sum(axis=2, dtype=np.int64)
    return np.argsort(ham.argmin(axis=1), kind="stable").astype(np.uint32)


def check(ctx, corpus, q, L, rescore, k, fused=(1,), dev=False, expect_rows=None, prepare=None, extra=None):
    import pgvectorscale_amd as P
    oi, od, ost = corpus.oracle.search_batch(q, L=L, rescore=rescore, k=k)
    if expect_rows is not None:
        rows = (oi != INVALID).sum(axis=1)
        assert expect_rows(rows), rows
    nq = len(q)
    ix = corpus.upload(ctx)
    try:
        if prepare:
            prepare(ix)
        set_opts(P, **(extra or {}))
        for mode in fused:
            P.set_option("VS_RERANK_FUSED", mode)
            for order, deal, seeds in SETTINGS:
                set_opts(P, VS_RERANK_ORDER=order, VS_RERANK_DEAL=deal, VS_RERANK_SEEDS=seeds)
                tag = (mode, order, deal, seeds)
                if dev:
                    dq, dids, dtids, ddist = ctx.alloc(q.nbytes), ctx.alloc(nq * k * 4), ctx.alloc(nq * k * 8), ctx.alloc(nq * k * 4)
                    ctx.upload(dq, q)
                    ix.search_batch_dev(dq, nq, L, rescore, k, dids, dtids, ddist)
                    gst = ix.search_batch_dev_finish()
                    gi, gt, gd = np.empty((nq, k), np.uint32), np.empty((nq, k), np.uint64), np.empty((nq, k), np.float32)
                    ctx.download(dids, gi), ctx.download(dtids, gt), ctx.download(ddist, gd)
                    for p in (dq, dids, dtids, ddist):
                        ctx.free(p)
                else:
                    gi, gt, gd, gst = ix.search_batch(q, search_list_size=L, rescore=rescore, k=k)
                assert (gi == oi).all(), (tag, np.argwhere(gi != oi)[:5])
                live = gi != INVALID
                assert (gt[live] == corpus.tids[gi[live]]).all() and (gt[~live] == 0).all(), tag
                assert (gd.view(np.uint32)[live] == od.view(np.uint32)[live]).all(), tag
                assert np.isnan(gd[~live]).all(), tag
                for key in COUNTERS:
                    assert gst[key] == ost[key], (tag, key, gst[key], ost[key])
                perm = ix.rerank_order()
                if order == 2 and not extra:  # (one launch: the order of the whole batch)
                    assert perm.size == nq and (np.sort(perm) == np.arange(nq)).all(), (tag, perm)
                    assert (perm == expected_order(corpus, q, seeds or 1024)).all(), (tag, perm)
                elif order != 2:
                    assert perm.size == 0, tag  # off, and the rule says no for a batch this small
    finally:
        set_opts(P, VS_RERANK_FUSED=None, VS_RERANK_ORDER=None, VS_RERANK_DEAL=None, VS_RERANK_SEEDS=None, **{n: None for n in (extra or {})})
        ix.close()


@pytest.fixture(scope="module")
def ties():
    return Corpus(tie_vectors(3000, 300, 64, seed=3))


# 27: not a multiple of 8 (the last places of some XCDs' eighths do not exist); 5: fewer scans than XCDs; 64 / 200: whole and several
# tiles of k_scan_regions
@pytest.mark.parametrize("nq", [5, 27, 64, 200])
def test_l2_fused_pair_and_forced_replay(gpu_ctx, ties, nq):
    q = np.vstack([ties.vecs[:3], np.random.default_rng(nq).random((nq - 3, 64), dtype=np.float32)])
    check(gpu_ctx, ties, q, L=40, rescore=20, k=10, fused=(0, 1, 2))


@pytest.mark.parametrize("nq", [7, 43])
def test_cosine_with_scalar_tail(gpu_ctx, nq):
    X = tie_vectors(1500, 500, 72, seed=11) - np.float32(0.5)
    c = Corpus(X, distance=O.COSINE)
    q = np.random.default_rng(12).random((nq, 72), dtype=np.float32) - np.float32(0.5)
    check(gpu_ctx, c, q, L=50, rescore=25, k=10, fused=(0, 1))


def test_short_and_exhausted_scans(gpu_ctx):
    """cnt < M: corpora smaller than the stream (and than the seed count: every row is a seed)"""
    small = Corpus(np.random.default_rng(2).random((9, 32), dtype=np.float32), R=8, L_build=10)
    q = np.random.default_rng(4).random((11, 32), dtype=np.float32)
    check(gpu_ctx, small, q, L=20, rescore=50, k=5, fused=(0, 1, 2), expect_rows=lambda r: (r == 5).all())
    check(gpu_ctx, small, q, L=20, rescore=3, k=12, fused=(0, 1, 2), expect_rows=lambda r: (r == 9).all())


def test_device_batch(gpu_ctx, ties):
    q = np.random.default_rng(13).random((61, 64), dtype=np.float32)
    check(gpu_ctx, ties, q, L=30, rescore=16, k=10, fused=(0, 1), dev=True)


def test_host_batch_in_chunks(gpu_ctx, ties):
    """a host batch cut into chunks of 10 scans: every chunk is ordered on its own"""
    q = np.random.default_rng(14).random((30, 64), dtype=np.float32)
    check(gpu_ctx, ties, q, L=30, rescore=16, k=10, fused=(0, 1), extra={"VS_HOST_CHUNKS": 3, "VS_HOST_CHUNK_MIN": 8})


def test_after_requantize(gpu_ctx, ties):
    """the seed codes are read from the index as it stands: a batch, the corpus quantised again on the device, the batches under test"""
    q = np.random.default_rng(15).random((37, 64), dtype=np.float32)

    def prepare(ix):
        import pgvectorscale_amd as P
        P.set_option("VS_RERANK_ORDER", 2)
        ix.search_batch(q, search_list_size=30, rescore=16, k=10)
        P.set_option("VS_RERANK_ORDER", None)
        ix.sbq_quantize_corpus()

    check(gpu_ctx, ties, q, L=30, rescore=16, k=10, prepare=prepare)
