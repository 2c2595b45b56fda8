"""The fused rerank + rescore-window kernel of the batch path (k_rerank_window, VS_RERANK_FUSED) against the oracle, for all
three settings of the option: 0 = the k_rerank + k_resort pair, 1 = fused (wave-parallel selection, serial replay only for scans
whose pops tie), 2 = fused with the serial replay forced for every scan.  Every case compares node ids in order, heap TIDs,
distance bits and the counters the call returns.  Also runs on the lockstep interpreter (VS_EMU=1, tests/emu/README.md)."""
import numpy as np
import pytest

from helpers import Corpus, tie_vectors
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2)
COUNTERS = ("visited_nodes", "candidate_nodes", "quantized_distance_comparisons", "full_distance_comparisons", "node_reads",
            "node_heap_reads", "next_calls")
INVALID = 0xFFFFFFFF


def check(ctx, corpus, q, L, rescore, k, qlabels=None, expect_rows=None):
    import pgvectorscale_amd as P
    oi, od, ost = corpus.oracle.search_batch(q, L=L, rescore=rescore, k=k, qlabels=qlabels)
    if expect_rows is not None:  # the case is the one it claims to be
        rows = (oi != INVALID).sum(axis=1)
        assert expect_rows(rows), rows
    ix = corpus.upload(ctx)
    try:
        for mode in MODES:
            P.set_option("VS_RERANK_FUSED", mode)
            gi, gt, gd, gst = ix.search_batch(q, search_list_size=L, rescore=rescore, k=k, qlabels=qlabels)
            assert (gi == oi).all(), (mode, np.argwhere(gi != oi)[:5])
            live = gi != INVALID
            assert (gt[live] == corpus.tids[gi[live]]).all() and (gt[~live] == 0).all(), mode
            assert (gd.view(np.uint32)[live] == od.view(np.uint32)[live]).all(), mode
            assert np.isnan(gd[~live]).all(), mode
            for key in COUNTERS:
                assert gst[key] == ost[key], (mode, key, gst[key], ost[key])
    finally:
        P.set_option("VS_RERANK_FUSED", None)
        ix.close()
    return oi, od


@pytest.fixture(scope="module")
def ties():
    return Corpus(tie_vectors(3000, 300, 64, seed=3))


# rescore 4: with ~10 copies of every vector the first pops tie; 30 / 100: ties inside the first k pops and across the window's edge
@pytest.mark.parametrize("rescore", [1, 4, 30, 100])
def test_tie_corpus(gpu_ctx, ties, rescore):
    q = np.vstack([ties.vecs[:8], np.random.default_rng(8).random((24, 64), dtype=np.float32)])  # (corpus rows: distance 0, tied)
    oi, od = check(gpu_ctx, ties, q, L=60, rescore=rescore, k=12)
    bits = od.view(np.uint32)
    assert any(len(set(row.tolist())) < row.size for row in bits), "the corpus did not produce tied distances among the rows returned"


def test_k1_and_wide_k(gpu_ctx, ties):
    q = np.random.default_rng(9).random((16, 64), dtype=np.float32)
    check(gpu_ctx, ties, q, L=40, rescore=20, k=1)
    check(gpu_ctx, ties, q, L=40, rescore=20, k=70)  # (more rows than one pass of the wave writes)


def test_scans_that_end_early(gpu_ctx):
    small = Corpus(np.random.default_rng(2).random((9, 32), dtype=np.float32), R=8, L_build=10)
    q = np.random.default_rng(4).random((8, 32), dtype=np.float32)
    check(gpu_ctx, small, q, L=20, rescore=50, k=5, expect_rows=lambda r: (r == 5).all())    # n < rescore
    check(gpu_ctx, small, q, L=20, rescore=50, k=12, expect_rows=lambda r: (r == 9).all())   # n < k
    check(gpu_ctx, small, q, L=20, rescore=3, k=12, expect_rows=lambda r: (r == 9).all())    # n < k, window smaller than n
    lab = Corpus(np.random.default_rng(6).random((400, 32), dtype=np.float32), n_labels=3)
    ql = [[3], [77], [1, 2], [77]] * 2  # label 77 occurs nowhere: those scans return nothing
    check(gpu_ctx, lab, q, L=20, rescore=10, k=6, qlabels=ql, expect_rows=lambda r: (r[1] == 0) and (r[0] == 6))  # n = 0


def test_window_at_the_lds_bound(gpu_ctx, ties):
    """24 KB of LDS per workgroup: 4 dim + 8 rescore + 4 M + 4 (k + 1) bytes.  dim 64, k 10: rescore 1000 (the GUC's maximum) fits with
    room to spare, so the bound is reached through k: M = rescore + k - 1."""
    q = np.random.default_rng(10).random((4, 64), dtype=np.float32)
    rescore = 1000
    k_fit = (24 * 1024 - 4 * 64 - 8 * rescore - 4 * (rescore - 1) - 4) // 8          # 4 M + 4 (k + 1) = 8 k + 4 rescore
    assert 4 * 64 + 8 * rescore + 4 * (rescore + k_fit - 1) + 4 * (k_fit + 1) <= 24 * 1024
    assert 4 * 64 + 8 * rescore + 4 * (rescore + k_fit) + 4 * (k_fit + 2) > 24 * 1024
    check(gpu_ctx, ties, q, L=100, rescore=rescore, k=k_fit)      # the last window the fused kernel takes
    check(gpu_ctx, ties, q, L=100, rescore=rescore, k=k_fit + 1)  # one past it: the pair takes over under every setting


@pytest.mark.parametrize("distance,dim", [(O.COSINE, 72), (O.IP, 72), (O.L2, 50), (O.COSINE, 32)])
def test_cosine_ip_and_scalar_tail(gpu_ctx, distance, dim):
    """dims that are not a multiple of 32 take the scalar tail of the row distance"""
    X = tie_vectors(1500, 500, dim, seed=11) - np.float32(0.5)
    c = Corpus(X, distance=distance)
    q = np.random.default_rng(12).random((24, dim), dtype=np.float32) - np.float32(0.5)
    check(gpu_ctx, c, q, L=50, rescore=25, k=10)


def test_device_batch_counters_and_table_fit(gpu_ctx, ties):
    """vs_search_batch_dev + finish: rows, the counters finish returns (summed on the device) and a second batch whose launch is sized
    from the first one's inserts, under every setting"""
    import pgvectorscale_amd as P
    q = np.random.default_rng(13).random((64, 64), dtype=np.float32)
    oi, od, ost = ties.oracle.search_batch(q, L=30, rescore=16, k=10)
    ix = ties.upload(gpu_ctx)
    try:
        dq, dids, ddist = gpu_ctx.alloc(q.nbytes), gpu_ctx.alloc(64 * 10 * 4), gpu_ctx.alloc(64 * 10 * 4)
        gpu_ctx.upload(dq, q)
        for mode in MODES:
            P.set_option("VS_RERANK_FUSED", mode)
            for _ in range(2):
                ix.search_batch_dev(dq, 64, 30, 16, 10, dids, None, ddist)
                st = ix.search_batch_dev_finish()
                gi, gd = np.empty((64, 10), np.uint32), np.empty((64, 10), np.float32)
                gpu_ctx.download(dids, gi)
                gpu_ctx.download(ddist, gd)
                assert (gi == oi).all() and (gd.view(np.uint32) == od.view(np.uint32)).all(), mode
                for key in COUNTERS:
                    assert st[key] == ost[key], (mode, key, st[key], ost[key])
                assert st["queries"] == 64
    finally:
        P.set_option("VS_RERANK_FUSED", None)
        ix.close()
