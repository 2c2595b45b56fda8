"""vs_index_insert: rows that arrive after the index is resident (aminsert, AM/build.rs:464-558) — growable arrays, the three
insert kernels (k_batch_mates, k_insert_merge_mates, k_insert_anchor), vs_index_repair.  Expectations are numpy twins written
here, the oracle searching the downloaded arrays, and the definitions of include/vsgpu.h recomputed from those arrays."""
import ctypes as C
import zlib

import numpy as np
import pytest

from helpers import TestIndex, make_vectors
from lifecycle_checks import fresh_index as _fresh, make_tids as _tids, oracle_of as _oracle_of, well_formed as _well_formed  # noqa: F401

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def _parity(O, ix, distance, q, qlabels=None, **kw):
    host = ix.download(vecs=True)
    oidx = _oracle_of(O, ix, host, distance, **kw)
    gi, gt, gd, _ = ix.search_batch(q, search_list_size=40, rescore=20, k=10, qlabels=qlabels)
    oi, od, _ = oidx.search_batch(q, L=40, rescore=20, k=10, qlabels=qlabels)
    assert (gi == oi).all()
    assert (gd.view(np.uint32) == od.view(np.uint32)).all()
    return host, oidx


def _exhaustive(oidx, q, labels=None):
    s = oidx.scan(q, labels=labels, L=2, rescore=0)
    seen = 0
    while s.next_sbq() is not None:
        seen += 1
    return seen


def _anchored(nb, batches):
    """the anchoring rule of vs_index_insert recomputed from the neighbor lists: per batch (b0, bn) a new node is anchored when the
    row of a node with id < b0 names it, or the row of an anchored node of the batch does -> the unanchored nodes"""
    out = []
    for b0, bn in batches:
        named_by = {x: set() for x in range(b0, b0 + bn)}
        for src in range(nb.shape[0]):
            for v in nb[src]:
                if v != INV and b0 <= v < b0 + bn:
                    named_by[int(v)].add(src)
        anch = {x for x, srcs in named_by.items() if any(s < b0 for s in srcs)}
        grew = True
        while grew:
            grew = False
            for x, srcs in named_by.items():
                if x not in anch and srcs & anch:
                    anch.add(x)
                    grew = True
        out += [x for x in range(b0, b0 + bn) if x not in anch]
    return out


# ---- case 1: k_batch_mates against a numpy twin -----------------------------------------------------------------------------------
def _mates_twin(codes, c):
    n = codes.shape[0]
    ham = np.zeros((n, n), np.uint64)
    for w in range(codes.shape[1]):
        x = codes[:, None, w] ^ codes[None, :, w]
        ham += np.unpackbits(np.ascontiguousarray(x).view(np.uint8).reshape(n, n, 8), axis=2).sum(2, dtype=np.uint64)
    ids = np.full((n, c), INV, np.uint32)
    hm = np.full((n, c), INV, np.uint32)
    for i in range(n):
        keys = sorted((int(ham[i, j]), j) for j in range(n) if j != i)
        assert len(set(keys)) == len(keys)  # (Hamming, row) is a total order: the expected output is unambiguous
        for t, (h, j) in enumerate(keys[:c]):
            ids[i, t], hm[i, t] = j, h
    return ids, hm


@pytest.mark.parametrize("n,W,c", [(1, 3, 4), (3, 3, 16), (65, 3, 16), (130, 24, 16), (300, 5, 32)])
def test_batch_mates_match_the_numpy_twin(gpu_ctx, n, W, c):
    import pgvectorscale_amd as P
    rng = np.random.default_rng(n * 31 + W)
    codes = rng.integers(0, 1 << 63, (n, W), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, W), dtype=np.uint64)
    if n >= 3:  # planted ties: duplicated rows (distance 0) and rows one bit away from a duplicated row (equal non-zero distances)
        for k in range(0, n - 2, 7):
            codes[k + 1] = codes[k]
            codes[k + 2] = codes[k]
            codes[k + 2, 0] ^= np.uint64(1)
    ix = P.DiskAnnIndex.alloc(gpu_ctx, n=1, dim_full=64 * W, bits=1, num_neighbors=8, distance_type=P.VS_L2, with_vecs=False)
    assert ix.desc.words == W
    want_ids, want_ham = _mates_twin(codes, c)
    if n >= 3:
        assert (want_ham[:, 0] == 0).any() and (want_ham[:, :2].min(1) == want_ham[:, :2].max(1)).any()
    ids, ham = ix.batch_mates(codes, c)
    assert (ids == want_ids).all()
    assert (ham == want_ham).all()
    ix.close()


def test_filtered_batch_mates_only_pair_rows_whose_label_sets_overlap(gpu_ctx):
    """the form the filtered pass of a labeled insert runs: the numpy twin with every pair of disjoint label sets struck out"""
    import pgvectorscale_amd as P
    n, W, c = 150, 3, 16
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 1 << 62, (n, W), dtype=np.uint64)
    for k in range(0, n - 2, 7):
        codes[k + 1] = codes[k]
        codes[k + 2] = codes[k]
    labels = [sorted(set(int(v) for v in rng.integers(1, 9, int(rng.integers(0, 4))))) for _ in range(n)]  # (some rows carry none)
    labels[1], labels[2] = [1, 2], [3]  # duplicates of row 0's code that must not see each other
    ham = np.zeros((n, n), np.int64)
    for w in range(W):
        x = codes[:, None, w] ^ codes[None, :, w]
        ham += np.unpackbits(np.ascontiguousarray(x).view(np.uint8).reshape(n, n, 8), axis=2).sum(2, dtype=np.int64)
    want_ids = np.full((n, c), INV, np.uint32)
    want_ham = np.full((n, c), INV, np.uint32)
    struck = 0
    for i in range(n):
        keys = sorted((int(ham[i, j]), j) for j in range(n) if j != i and set(labels[i]) & set(labels[j]))
        struck += (n - 1) - len(keys)
        for t, (h, j) in enumerate(keys[:c]):
            want_ids[i, t], want_ham[i, t] = j, h
    assert struck > n and (want_ids[:, -1] == INV).any() and (want_ids[:, -1] != INV).any()
    ix = P.DiskAnnIndex.alloc(gpu_ctx, n=1, dim_full=64 * W, bits=1, num_neighbors=8, distance_type=P.VS_L2, with_vecs=False)
    ids, hm = ix.batch_mates(codes, c, labels=labels)
    assert (ids == want_ids).all() and (hm == want_ham).all()
    assert 2 not in ids[1] and 1 not in ids[2]
    plain_ids, _ = ix.batch_mates(codes, c)
    assert 2 in plain_ids[1]  # (without the filter they are each other's nearest rows)
    ix.close()


# ---- case 2: bit-level invariants ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distance,bits,dim_index", [(1, 2, None), (0, 1, None), (0, 2, 64)], ids=["l2_2bit", "cosine_1bit", "slice_64_of_96"])
def test_insert_leaves_old_rows_and_quantizer_alone_and_quantizes_with_the_old_quantizer(gpu_ctx, oracle, distance, bits, dim_index):
    O = oracle
    n0, n1, dim, R = 3000, 257, 96, 24
    X = make_vectors(n0 + n1, dim, 40 + distance, "gauss")
    if distance == 0:  # non-unit rows and one zero row among the old and the new rows: the cosine rescale path runs
        X[::3] *= 2.5
        X[7] = 0
        X[n0 + 5] = 0
    nbrs = []
    for rep in range(2):
        ix = _fresh(gpu_ctx, X[:n0], distance=distance, bits=bits, dim_index=dim_index, R=R, tids=_tids(0, n0))
        if rep == 0:
            before = ix.download(vecs=True)
            q_before = ix.get_quantizer()
        st = ix.insert(X[n0:], _tids(n0, n1), search_list_size=48)
        assert st["first_node"] == n0 and st["inserted"] == n1 and st["grew"] == 1 and st["orphans_left"] == 0
        assert ix.desc.n == n0 + n1 and ix.capacity >= n0 + n1
        host = ix.download(vecs=True)
        nbrs.append(host["nbrs"].copy())
        if rep == 0:
            for k in ("codes", "heap_tids", "vecs"):
                assert host[k][:n0].tobytes() == before[k].tobytes(), k
            q_after = ix.get_quantizer()
            assert q_after[2] == q_before[2] == n0
            assert q_after[0].tobytes() == q_before[0].tobytes() and q_after[1].tobytes() == q_before[1].tobytes()
            assert (host["heap_tids"][n0:] == _tids(n0, n1)).all()
            assert host["vecs"][n0:].tobytes() == X[n0:].tobytes()
            di = dim_index or dim
            sl = np.ascontiguousarray(X[n0:, :di]).copy()
            if distance == 0:
                for i in range(n1):
                    sl[i] = O.preprocess_cosine(sl[i])[0]
            want = O.quantize(q_before[0], q_before[1], q_before[2], ix.desc.bits, sl)
            assert (host["codes"][n0:] == want).all()
            _well_formed(host["nbrs"], R)
            assert ((host["nbrs"][n0:] != INV).sum(1) >= 1).all()
        ix.close()
    assert nbrs[0].tobytes() == nbrs[1].tobytes(), "the same sequence on two fresh indexes must give the same graph"


# ---- case 3: search parity after an insert, with and without growth ---------------------------------------------------------------
@pytest.mark.parametrize("distance", [1, 0], ids=["l2", "cosine"])
def test_search_on_the_grown_index_equals_the_oracle(gpu_ctx, oracle, distance):
    import pgvectorscale_amd as P
    n0, n1, dim = 1500, 300, 64
    X = make_vectors(n0 + 2 * n1, dim, 50 + distance, "gauss")
    if distance == 0:
        X[::4] *= 3.0
    q = make_vectors(24, dim, 77, "gauss")
    ix = _fresh(gpu_ctx, X[:n0], distance=distance, tids=_tids(0, n0))
    st = ix.insert(X[n0:n0 + n1], _tids(n0, n1), search_list_size=48)
    assert st["grew"] == 1
    _parity(oracle, ix, distance, q)
    assert ix.capacity == n0 + n0 // 2  # grown by half (more than the insert needed)
    ix.reserve(100)  # (never shrinks)
    assert ix.capacity == n0 + n0 // 2
    ix.reserve(4000)
    assert ix.capacity == 4000
    _parity(oracle, ix, distance, q)  # (the arrays moved: the same rows)
    ptrs = [ix.array(a)[0].value for a in (P._lib.ARR_CODES, P._lib.ARR_NBRS, P._lib.ARR_TIDS, P._lib.ARR_VECS, P._lib.ARR_VNORM)]
    st = ix.insert(X[n0 + n1:], _tids(n0 + n1, n1), search_list_size=48)
    assert st["grew"] == 0 and st["first_node"] == n0 + n1
    assert ptrs == [ix.array(a)[0].value for a in (P._lib.ARR_CODES, P._lib.ARR_NBRS, P._lib.ARR_TIDS, P._lib.ARR_VECS, P._lib.ARR_VNORM)]
    host, oidx = _parity(oracle, ix, distance, q)
    _well_formed(host["nbrs"], ix.desc.num_neighbors)
    ix.close()


# ---- case 4: findability ----------------------------------------------------------------------------------------------------------
def _batches_of(n0, n_new, batch_max):
    out, b0 = [], n0
    while b0 < n0 + n_new:
        bn = min(batch_max, b0, n0 + n_new - b0)
        out.append((b0, bn))
        b0 += bn
    return out


@pytest.mark.parametrize("n_new", [1, 63, 64, 65])
def test_every_inserted_row_is_found_and_anchored(gpu_ctx, oracle, n_new):
    n0, dim, R = 1200, 64, 16
    X = make_vectors(n0 + n_new, dim, 60, "gauss")
    ix = _fresh(gpu_ctx, X[:n0], distance=1, R=R, L=40, tids=_tids(0, n0))
    st = ix.insert(X[n0:], _tids(n0, n_new), search_list_size=40, batch_max=64)
    assert st["batches"] == (2 if n_new == 65 else 1) and st["orphans_left"] == 0
    host = ix.download(vecs=True)
    _well_formed(host["nbrs"], R)
    oidx = _oracle_of(oracle, ix, host, 1)
    assert _exhaustive(oidx, X[n0]) == n0 + n_new - st["orphans_left"]
    assert _anchored(host["nbrs"], _batches_of(n0, n_new, 64)) == []
    assert _anchored(host["nbrs"], [(n0, n_new)]) == []  # ... and against the graph as it was before the call
    ix.close()


@pytest.mark.parametrize("copy_exists", [False, True], ids=["new_point", "copy_of_an_old_row"])
def test_identical_rows_of_one_batch_stay_findable(gpu_ctx, oracle, copy_exists):
    """8 copies of one vector arrive in one batch: without the batch's mates they cannot see each other, and only one of them can
    keep the back-edges of the targets they all ask (the others are pruned as covered).  None may end up unfindable."""
    n0, dim, R = 1000, 64, 16
    X = make_vectors(n0, dim, 61, "gauss")
    v = X[17].copy() if copy_exists else make_vectors(1, dim, 62, "gauss")[0] * 6.0  # (far from everything)
    new = np.repeat(v[None, :], 8, 0)
    ix = _fresh(gpu_ctx, X, distance=1, R=R, L=40, tids=_tids(0, n0))
    gpu_ctx.profile_enable(True)
    ix.insert_kernel_ms(reset=True)
    try:
        st = ix.insert(new, _tids(n0, 8), search_list_size=40)
    finally:
        gpu_ctx.profile_enable(False)
    ms = ix.insert_kernel_ms(reset=True)
    assert all(v > 0 for v in ms.values()) and ix.insert_kernel_ms() == dict.fromkeys(ms, 0.0)  # the three kernels ran and were timed
    assert st["batches"] == 1 and st["orphans_left"] == 0
    host = ix.download(vecs=True)
    _well_formed(host["nbrs"], R)
    assert _anchored(host["nbrs"], [(n0, 8)]) == []
    assert st["mate_edges"] >= 1  # the copies did see each other
    oidx = _oracle_of(oracle, ix, host, 1)
    assert _exhaustive(oidx, v) == n0 + 8
    ix.close()


def test_two_new_rows_that_only_name_each_other_are_not_left_alone(gpu_ctx, oracle):
    """two duplicates far from everything: each is the other's nearest candidate; the pair must end up with an in-edge from the old
    graph (kept back-edges or a placement), never as an island"""
    n0, dim, R = 600, 64, 8
    X = make_vectors(n0, dim, 63, "gauss")
    v = make_vectors(1, dim, 64, "gauss")[0] * 8.0
    ix = _fresh(gpu_ctx, X, distance=1, R=R, L=30, tids=_tids(0, n0))
    st = ix.insert(np.stack([v, v]), _tids(n0, 2), search_list_size=30)
    host = ix.download(vecs=True)
    nb = host["nbrs"]
    old_in = sum(int(((nb[:n0] == x).any())) for x in (n0, n0 + 1))
    assert st["orphans_placed"] >= 1 or old_in >= 1
    assert st["orphans_left"] == 0 and _anchored(nb, [(n0, 2)]) == []
    assert _exhaustive(_oracle_of(oracle, ix, host, 1), v) == n0 + 2
    ix.close()


# ---- case 5: empty and tiny -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0", [0, 1])
def test_insert_into_an_empty_and_a_one_row_index(gpu_ctx, oracle, n0):
    import pgvectorscale_amd as P
    dim, R, n1 = 64, 12, 90
    X = make_vectors(n0 + n1, dim, 65, "gauss")
    ref = TestIndex(n=200, dim_full=dim, bits=2, R=R, distance=oracle.L2, seed=66, kind="gauss", L_build=30)
    ix = P.DiskAnnIndex.alloc(gpu_ctx, n=n0, dim_full=dim, bits=2, num_neighbors=R, distance_type=P.VS_L2)
    if n0:
        gpu_ctx.upload(ix.array(P._lib.ARR_VECS)[0], X[:n0])
        ix.refresh_norms()
    ix.set_quantizer(ref.mean, ref.m2, ref.count)  # a trained quantizer from elsewhere: the insert must not train
    if n0:
        ix.sbq_quantize_corpus()
        ix.build_graph(search_list_size=30)
    st = ix.insert(X[n0:], _tids(n0, n1), search_list_size=30)
    assert st["first_node"] == n0 and ix.desc.n == n0 + n1 and ix.desc.default_start == 0 and st["orphans_left"] == 0
    mean, m2, cnt = ix.get_quantizer()
    assert cnt == ref.count and mean.tobytes() == ref.mean.tobytes() and m2.tobytes() == ref.m2.tobytes()
    host, oidx = _parity(oracle, ix, 1, make_vectors(8, dim, 67, "gauss"))
    _well_formed(host["nbrs"], R)
    assert _exhaustive(oidx, X[0]) == n0 + n1
    ix.close()


# ---- case 6: labels ---------------------------------------------------------------------------------------------------------------
def test_insert_into_a_labeled_index(gpu_ctx, oracle):
    # R = 50 / L = 100: the reference's defaults, as in test_label_aware_build (lists of 24 drop a rare label's far carriers when they
    # fill up, in the sequential builder too: prune_neighbors stops at num_neighbors whatever labels the rest would bring)
    n0, n1, dim, R, NL = 1000, 200, 64, 50, 8
    X = make_vectors(n0 + n1 + 1, dim, 68, "gauss")
    rng = np.random.default_rng(69)
    sets = [sorted(set(int(v) for v in rng.integers(1, NL, int(rng.integers(1, 4))))) for _ in range(n0 + n1)]  # labels 1 .. 7
    for i in range(n0 + 3, n0 + n1, 3):
        sets[i] = sorted(set(sets[i] + [NL]))  # label 8: only inserted rows carry it
    off = np.zeros(n0 + 1, np.uint32)
    off[1:] = np.cumsum([len(s) for s in sets[:n0]])
    vals = np.array([l for s in sets[:n0] for l in s], np.int16)
    ix = _fresh(gpu_ctx, X[:n0], distance=1, R=R, L=100, tids=_tids(0, n0), build=False)
    ix.set_labels(off, vals)
    ix.build_graph(search_list_size=100)
    st = ix.insert(X[n0:n0 + n1], _tids(n0, n1), labels=sets[n0:], search_list_size=100)
    assert st["orphans_left"] == 0 and ix.desc.has_labels == 1
    first = {}
    for i, s in enumerate(sets):
        for l in s:
            first.setdefault(l, i)
    assert first[NL] == n0 + 3 and ix.desc.n_label_starts == NL
    aoff = np.zeros(n0 + n1 + 1, np.uint32)
    aoff[1:] = np.cumsum([len(s) for s in sets])
    avals = np.array([l for s in sets for l in s], np.int16)
    q = make_vectors(32, dim, 70, "gauss")
    keys = [[int(rng.integers(1, NL + 1))] for _ in range(len(q))]
    keys[0] = [NL]
    # (the oracle is given the start map the insert must have produced: a scan from any other start node returns other rows)
    host, oidx = _parity(oracle, ix, 1, q, qlabels=keys, label_off=aoff, label_val=avals, label_starts=first)
    _well_formed(host["nbrs"], R)
    carriers = sum(NL in s for s in sets)
    assert _exhaustive(oidx, q[0], labels=[NL]) == carriers
    # one more row pushes the distinct labels past 64: the label masks are dropped, the scans keep the sorted-merge test
    wide = list(range(100, 160))
    st = ix.insert(X[n0 + n1:], _tids(n0 + n1, 1), labels=[wide], search_list_size=100)
    sets.append(wide)
    for l in wide:
        first.setdefault(l, n0 + n1)
    aoff = np.append(aoff, aoff[-1] + len(wide)).astype(np.uint32)
    avals = np.append(avals, np.array(wide, np.int16))
    keys[1] = [130]
    _parity(oracle, ix, 1, q, qlabels=keys, label_off=aoff, label_val=avals, label_starts=first)
    ix.close()


# ---- case 7: quality ----------------------------------------------------------------------------------------------------------------
def _recall10(ix, q, X):
    gi = ix.search_batch(q, search_list_size=100, rescore=50, k=10)[0]
    d = (q ** 2).sum(1)[:, None] - 2 * q @ X.T + (X ** 2).sum(1)[None, :]
    gt = np.argsort(d, axis=1, kind="stable")[:, :10]
    return float(np.mean([len(set(a) & set(b)) / 10 for a, b in zip(gi, gt)]))


# recall@10 (L = 100, rescore 50, 256 queries) of vs_build_graph(L = 64) over all 20 000 x 128 rows at corpus seeds 9 .. 13, measured
# once on an MI355X: 0.9426, 0.9477, 0.9438, 0.9531, 0.9414.  The margin is their spread (max - min).  On the same run the graph
# grown by four inserts of 1 000 rows (seed 9) reached 0.9391, the whole-set build 0.9426, the oracle's sequential build over the
# grown index's codes 0.9402.
QUALITY_MARGIN = 0.9531 - 0.9414


def test_a_graph_grown_by_inserts_is_as_good_as_one_built_whole(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    from pgvectorscale_amd.datagen import DatagenParams, fill_device, rows_numpy
    n, n0, dim, R = 20000, 16000, 128, 32
    p = DatagenParams(seed=9, dim=dim, latent_dim=24, n_clusters=64)
    q = rows_numpy(p, 10 ** 9, 256)

    def mk(rows):
        ix = P.DiskAnnIndex.alloc(gpu_ctx, n=rows, dim_full=dim, num_neighbors=R, distance_type=P.VS_L2)
        fill_device(gpu_ctx, p, 0, rows, ix.array(P._lib.ARR_VECS)[0])
        ix.sbq_train()
        ix.sbq_quantize_corpus()
        ix.build_graph(search_list_size=64, max_alpha=1.2)
        return ix
    whole = mk(n)
    X = whole.download(codes=False, nbrs=False, tids=False, vecs=True)["vecs"]
    r_whole = _recall10(whole, q, X)
    whole.close()
    ix = mk(n0)
    for k in range(n0, n, 1000):
        st = ix.insert(X[k:k + 1000], _tids(k, 1000), search_list_size=64)
        assert st["orphans_left"] == 0
    r_insert = _recall10(ix, q, X)
    host = ix.download()
    _well_formed(host["nbrs"], R)
    onb, ostart = oracle.build_graph(host["codes"], num_neighbors=R, search_list_size=64)
    gp, stride = ix.array(P._lib.ARR_NBRS)
    full = np.full((n, stride), INV, np.uint32)
    full[:, :R] = onb[:, :R]
    gpu_ctx.upload(gp, full)
    ix.set_start_nodes(int(ostart))
    r_oracle = _recall10(ix, q, X)
    ix.close()
    print("recall@10: grown by inserts", r_insert, "whole-set device build", r_whole, "oracle's sequential build", r_oracle)
    assert r_insert >= r_whole - QUALITY_MARGIN
    assert r_insert >= r_oracle - QUALITY_MARGIN


# ---- vs_build_graph is what it was ---------------------------------------------------------------------------------------------------
# sha256 of the downloaded neighbor arrays of the builds tests/test_gpu_build.py makes, recorded on an MI355X from the library as it
# was BEFORE the batch machinery was lifted out of build_graph_impl (the build is deterministic for given codes and parameters)
BUILD_SHA256 = {
    "20000x128": "276574f065bf09958d823f859ede64c35cc811eb08929c6e239c445418cd63da",
    "700x8": "e9cae8c9b3cbb4c517668ccd147c6f8b6a001b078749afe1f59e88044098543f",
    "2126x6": "9fd5ce065a538dd0e800bf16b2629cc564512b157c38a788e7f39ea7513b61cf",
    "labeled1000": "1b80c856ed9e1aee2c7a458de2ccd92a5801da57007d064b5ff0454cff33d74c",
}


def test_build_graph_output_is_byte_identical_to_the_recorded_one(gpu_ctx):
    import hashlib
    import pgvectorscale_amd as P
    from pgvectorscale_amd.datagen import DatagenParams, fill_device
    got = {}
    ix = P.DiskAnnIndex.alloc(gpu_ctx, n=20000, dim_full=128, num_neighbors=32, distance_type=P.VS_L2)
    fill_device(gpu_ctx, DatagenParams(seed=9, dim=128, latent_dim=24, n_clusters=64), 0, 20000, ix.array(P._lib.ARR_VECS)[0])
    ix.sbq_train()
    ix.sbq_quantize_corpus()
    ix.build_graph(search_list_size=64, max_alpha=1.2)
    got["20000x128"] = ix.download()["nbrs"]
    ix.close()
    for n, dim, R, L, seed in ((700, 8, 8, 40, 20), (2126, 6, 10, 20, 31)):
        X = make_vectors(n, dim, seed, "uniform")
        ix = _fresh(gpu_ctx, X, distance=1, bits=1, R=R, L=L)
        got[f"{n}x{dim}"] = ix.download()["nbrs"]
        ix.close()
    n, dim, R, NL = 1000, 128, 50, 32
    X = make_vectors(n, dim, 1, "uniform")
    rng = np.random.default_rng(3)
    off, vals = np.zeros(n + 1, np.uint32), []
    for i in range(n):
        vals += sorted(set(int(v) for v in rng.integers(1, NL + 1, int(rng.integers(1, 4)))))
        off[i + 1] = len(vals)
    ix = _fresh(gpu_ctx, X, distance=1, R=R, build=False)
    ix.set_labels(off, np.array(vals, np.int16))
    ix.build_graph(search_list_size=100, max_alpha=1.2)
    got["labeled1000"] = ix.download()["nbrs"]
    ix.close()
    for k, nb in got.items():
        assert hashlib.sha256(nb.tobytes()).hexdigest() == BUILD_SHA256[k], k


# ---- case 8: vs_index_repair ------------------------------------------------------------------------------------------------------
def _reach(nbrs, start):
    seen = np.zeros(nbrs.shape[0], bool)
    seen[start] = True
    stack = [int(start)]
    while stack:
        v = stack.pop()
        for u in nbrs[v]:
            if u != INV and not seen[u]:
                seen[u] = True
                stack.append(int(u))
    return int(seen.sum())


def test_repair_on_its_own_reports_what_the_build_reported(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    n, n1, dim, R = 2126, 80, 6, 10  # many identical codes, short lists: most rows are hard to reach
    X = make_vectors(n + n1, dim, 31, "uniform")
    ix = P.DiskAnnIndex.alloc(gpu_ctx, n=n, dim_full=dim, bits=1, num_neighbors=R, distance_type=P.VS_L2)
    vp, stride = ix.array(P._lib.ARR_VECS)
    Xp = np.zeros((n + n1, stride), np.float32)
    Xp[:, :dim] = X
    gpu_ctx.upload(vp, Xp[:n])
    ix.refresh_norms()
    ix.sbq_train()
    ix.sbq_quantize_corpus()
    ix.build_graph(search_list_size=20, max_alpha=1.2)
    reported = ix.build_unreachable()
    assert ix.repair() == reported == n - _reach(ix.download()["nbrs"], ix.desc.default_start)
    ix.insert(X[n:], _tids(n, n1), search_list_size=20)
    un = ix.repair()
    assert ix.build_unreachable() == un
    assert _reach(ix.download()["nbrs"], ix.desc.default_start) == n + n1 - un
    ix.close()


# ---- case 9: the grown index written out as relation pages ------------------------------------------------------------------------
def test_pages_after_an_insert_are_the_oracle_writers(gpu_ctx, oracle):
    from oracle import pages_py as PG
    ti = TestIndex(n=500, dim_full=64, bits=2, R=16, distance=oracle.L2, seed=71, kind="gauss", L_build=40)
    ix = ti.upload(gpu_ctx)
    new = make_vectors(100, 64, 72, "gauss")
    ix.insert(new, _tids(500, 100), search_list_size=40)
    host = ix.download()
    meta = dict(num_dimensions=64, num_dimensions_to_index=64, bq_num_bits_per_dimension=2, distance_type=oracle.L2, num_neighbors=16,
                default_start=ix.desc.default_start, labeled_starts={}, extension_version="0.8.0", search_list_size=100, max_alpha=1.2)
    want = PG.write_index(codes=host["codes"], nbrs=host["nbrs"], heap_tids=host["heap_tids"], mean=ti.mean, m2=ti.m2, count=ti.count,
                          means_first=True, meta=meta).rel.tobytes()
    assert ix.write_pages(extension_version="0.8.0", search_list_size=100, max_alpha=1.2) == want
    ix.close()


# ---- case 10: refusals ------------------------------------------------------------------------------------------------------------
def _state(ix):
    return ix.desc.n, ix.capacity, zlib.crc32(ix.download()["nbrs"].tobytes())


def _refused(ix, code, *a, **kw):
    import pgvectorscale_amd as P
    before = _state(ix)
    with pytest.raises(P._lib.VsError) as e:
        ix.insert(*a, **kw)
    assert e.value.code == code, str(e.value)
    assert _state(ix) == before
    return str(e.value)


def test_refusals_leave_the_index_as_it_was(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    STATE, INVALID = -5, -1
    ti = TestIndex(n=400, dim_full=64, bits=2, R=16, distance=oracle.L2, seed=73, kind="gauss", L_build=30)
    new, tids = make_vectors(5, 64, 74, "gauss"), _tids(400, 5)
    ix = ti.upload(gpu_ctx)
    ctx2 = P.Context(0)
    view = ix.view(ctx2)
    _refused(ix, STATE, new, tids)  # a live view holds the array pointers
    with pytest.raises(P._lib.VsError) as e:
        ix.reserve(1000)
    assert e.value.code == STATE and ix.capacity == 400
    with pytest.raises(P._lib.VsError) as e:
        view.insert(new, tids)
    assert e.value.code == STATE
    view.close()
    ctx2.close()
    d_mask = gpu_ctx.alloc(400)
    gpu_ctx.upload(d_mask, np.ones(400, np.uint8))
    P._lib.check(ix._L.vs_index_set_visibility_dev(ix.h, d_mask))
    _refused(ix, STATE, new, tids)  # a caller-owned device mask cannot be grown by the library
    P._lib.check(ix._L.vs_index_set_visibility_dev(ix.h, None))
    gpu_ctx.free(d_mask)
    _refused(ix, INVALID, new, None)  # NULL tids
    _refused(ix, INVALID, new, tids, labels=[[1]] * 5)  # labels on an unlabeled index
    # n + n_new reaching VS_INVALID_NODE (checked before any pointer is read: only the count matters)
    before = _state(ix)
    r = ix._L.vs_index_insert(ix.h, new.ctypes.data_as(C.c_void_p), tids.ctypes.data_as(C.c_void_p), None, None, INV - 400, 40, 1.2, 0, None)
    assert r == INVALID and _state(ix) == before
    ix.close()
    # an untrained quantizer
    raw = P.DiskAnnIndex.alloc(gpu_ctx, n=0, dim_full=64, bits=2, num_neighbors=16, distance_type=P.VS_L2)
    _refused(raw, STATE, new, tids)
    raw.close()
    # plain storage
    plain = P.DiskAnnIndex.upload(gpu_ctx, codes=None, nbrs=ti.nbrs, heap_tids=ti.tids, vecs=ti.vecs, mean=None, m2=None, count=0, bits=1,
                                  dim_index=64, num_neighbors=16, distance_type=P.VS_L2, default_start=ti.start,
                                  storage_type=P._lib.VS_STORAGE_PLAIN)
    assert "plain" in _refused(plain, INVALID, new, tids)
    plain.close()
    # a labeled index: rows without label sets, a row with more than 64 labels
    tl = TestIndex(n=300, dim_full=64, bits=2, R=16, distance=oracle.L2, seed=75, kind="gauss", L_build=30, n_labels=6)
    lix = tl.upload(gpu_ctx)
    _refused(lix, INVALID, new, tids)
    _refused(lix, INVALID, new, tids, labels=[[1], [2], list(range(1, 66)), [3], [4]])
    lix.close()


def test_snapshots_hide_inserted_rows_and_the_own_mask_shows_them(gpu_ctx, oracle):
    ti = TestIndex(n=400, dim_full=64, bits=2, R=16, distance=oracle.L2, seed=76, kind="gauss", L_build=30)
    ix = ti.upload(gpu_ctx)
    import pgvectorscale_amd as P
    P._lib.check(ix._L.vs_index_snapshot_put(ix.h, 1, np.ones(400, np.uint8).ctypes.data_as(C.c_void_p)))
    ix.set_visibility(np.ones(400, np.uint8))
    q = make_vectors(1, 64, 77, "gauss")[0] * 5.0
    new = np.repeat(q[None, :], 4, 0) + 0.001 * make_vectors(4, 64, 78, "gauss")
    ix.insert(new, _tids(400, 4), search_list_size=40)
    gi, _, _, _ = ix.search_batch(q[None, :], search_list_size=40, rescore=20, k=4)
    assert set(gi[0].tolist()) == {400, 401, 402, 403}  # the library's own mask shows the new rows
    P._lib.check(ix._L.vs_index_snapshot_use(ix.h, 1, None))
    gi, _, _, _ = ix.search_batch(q[None, :], search_list_size=40, rescore=20, k=4)
    assert not (set(gi[0].tolist()) & {400, 401, 402, 403})  # a snapshot stored before the insert cannot see them
    P._lib.check(ix._L.vs_index_snapshot_use(ix.h, 0, None))
    ix.close()
