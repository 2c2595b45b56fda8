"""K5 flat SBQ scan (vs_scan_topk) where every wave walks several 64-row steps on the device in use: the admission threshold a wave
carries from step to step ("a row whose hamming equals the threshold has a larger id, so `<` is exact"), the per-wave id order and
the merge's preference for the lower wave, at query tiles of 4, 8 and 16.  The corpus is sized from the device's CU count; ids and
Hamming values are compared exactly with oracle.hamming_scan_topk, and with the closed form where the corpus has one.  Not run on the
wave64 interpreter: it reports 4 CUs and takes several steps at a few thousand rows already (tests/test_gpu_scan.py), and these
sizes would take it minutes."""
import functools
import os
import re

import numpy as np
import pytest

from test_gpu_scan import INV, SCAN_TILES, _flat_index, _popcount, _tied_codes, options

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(bool(os.environ.get("VS_EMU")), reason="sized for hardware: minutes on the interpreter")]

WORDS = 4   # 256-bit codes: 13 MB at 393 000 rows
NQ = 19     # 5 tiles of 4, 3 of 8, 2 of 16, the last one ragged each time
PERIOD, PLATEAU = 4096, 16


def _rows_for(gpu_ctx):
    cus = int(re.search(r"(\d+) CUs\)$", gpu_ctx.device_name()).group(1))
    # The scan deals the rows to 8 waves per CU, at least one 64-row step each: up to 64 * 8 * CUs rows every wave takes ONE step, its
    # threshold never meets a second step and nothing of the step loop is checked.  Three steps' worth of rows per wave plus a remainder
    # puts at least three steps on every wave but the last, which is short (37 rows) — whatever the CU count of the part in use.
    return 3 * 64 * 8 * cus + 37


def _low_bits(p):
    """[len(p)][WORDS] codes with exactly the lowest p[i] bits set"""
    out = np.empty((len(p), WORDS), np.uint64)
    for w in range(WORDS):
        b = np.clip(p.astype(np.int64) - 64 * w, 0, 64).astype(np.uint64)
        out[:, w] = np.where(b == 64, np.uint64(0xFFFFFFFFFFFFFFFF), (np.uint64(1) << np.minimum(b, np.uint64(63))) - np.uint64(1))
    return out


@functools.lru_cache(maxsize=None)
def _corpus(kind, n):
    """-> (codes, qcodes, the Hamming distance of every row to every query where the corpus fixes it, else None)"""
    rng = np.random.default_rng(n)
    i = np.arange(n)
    if kind == "random_ties":
        return _tied_codes(rng, n, WORDS), _tied_codes(rng, NQ, WORDS), None
    # the structured corpora: every query is the same code x, row i = x ^ (a code of popcount ham[i])
    if kind == "best_last":          # non-increasing in id over the whole corpus, in plateaus of n / 256 rows
        ham = 255 - i * 255 // (n - 1)
    elif kind == "best_first":       # its mirror image
        ham = i * 255 // (n - 1)
    elif kind == "best_last_saw":    # falling by one every 16 rows, back up every 4096: EVERY step of every wave brings better rows
        ham = 255 - (i % PERIOD) // PLATEAU
    elif kind == "best_first_saw":   # rising: after a wave's first step only ties at the threshold and worse rows follow
        ham = (i % PERIOD) // PLATEAU
    elif kind == "identical":
        ham = np.zeros(n, np.int64) + 77
    else:
        raise ValueError(kind)
    x = rng.integers(0, 1 << 63, WORDS, dtype=np.uint64)
    codes = _low_bits(ham) ^ x
    assert (_popcount(codes[::997] ^ x).sum(axis=1) == ham[::997]).all()
    return codes, np.tile(x, (NQ, 1)), ham.astype(np.int64)


@pytest.mark.parametrize("kind", ["random_ties", "best_last", "best_first", "best_last_saw", "best_first_saw", "identical"])
def test_flat_scan_several_steps_per_wave(gpu_ctx, oracle, kind):
    n = _rows_for(gpu_ctx)
    codes, qcodes, ham = _corpus(kind, n)
    want_ids, want_ham = oracle.hamming_scan_topk(codes, qcodes, 64)
    if ham is not None:  # the expected rows in closed form: (hamming, id) ascending — stated here, not taken from the oracle
        order = np.lexsort((np.arange(n), ham))[:64]
        assert (want_ids == order).all() and (want_ham == ham[order]).all()
        if kind in ("best_first", "identical"):
            assert (order == np.arange(64)).all()
    ix = _flat_index(gpu_ctx, codes)
    try:
        for tile in SCAN_TILES:
            for k in (10, 64):
                with options(VS_SCAN_Q=tile):
                    ids, hm = ix.scan_topk(qcodes, k)
                assert (ids == want_ids[:, :k]).all(), (tile, k)
                assert (hm == want_ham[:, :k]).all(), (tile, k)
    finally:
        ix.close()


def test_flat_scan_filtered_several_steps_per_wave(gpu_ctx, oracle):
    """label keys and deleted tuples at the same size: a row the threshold lets through may still be refused by the predicate, and
    the threshold must not move for it"""
    import pgvectorscale_amd as P
    n = _rows_for(gpu_ctx)
    codes, qcodes, _ = _corpus("random_ties", n)
    rng = np.random.default_rng(5)
    a, b = rng.integers(1, 7, n), rng.integers(1, 7, n)  # one or two of six labels per row, sorted
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum(1 + (lo != hi))
    val = np.empty(int(off[-1]), np.int16)
    val[off[:-1]] = lo
    val[off[:-1][lo != hi] + 1] = hi[lo != hi]
    tids = ((np.arange(n, dtype=np.uint64) + 7) << np.uint64(16)) | np.uint64(1)
    tids[rng.random(n) < 0.1] &= ~np.uint64(0xFFFF)
    keys = [sorted(set(int(v) for v in rng.integers(1, 7, int(rng.integers(0, 3))))) for _ in range(NQ)]
    keys[0], keys[1], keys[2] = [], [6], [99]  # no filter / one label / a label nobody carries
    ix = P.DiskAnnIndex.upload(gpu_ctx, codes=codes, nbrs=np.full((n, 4), INV, np.uint32), heap_tids=tids, vecs=None,
                               mean=np.zeros(WORDS * 64, np.float32), m2=None, count=1, bits=1, dim_index=WORDS * 64, num_neighbors=4,
                               distance_type=P.VS_L2, default_start=0, label_off=off, label_val=val)
    try:
        for live in (False, True):
            oi, oh = oracle.hamming_scan_topk(codes, qcodes, 64, label_off=off, label_val=val, heap_tids=tids if live else None,
                                              qlabels=keys)
            assert (oi[2] == INV).all() and (oi[0] != INV).all()
            if live:
                assert (tids[oi[oi != INV]] & np.uint64(0xFFFF) != 0).all()
            for tile in SCAN_TILES:
                for k in (10, 64):
                    with options(VS_SCAN_Q=tile):
                        gi, gh = ix.scan_topk(qcodes, k, qlabels=keys, live_only=live)
                    assert (gi == oi[:, :k]).all() and (gh == oh[:, :k]).all(), (live, tile, k)
    finally:
        ix.close()
