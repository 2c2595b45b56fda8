"""Building and inserting into `plain` storage indexes on the device: vs_build_graph / vs_index_insert score
with the full-precision pair distance of the reference's IndexFullDistanceMeasure.  The two kernels that can be pinned exactly
(vs_prune_plain, vs_batch_mates_plain) are held to the numpy restatement of the rule in plain_build_checks.py, the built graph to
the oracle's plain search bit for bit, its quality to the graph a plain index could be given before (the oracle's builder over SBQ
codes) and to a sequential f32 Vamana, inserts to reachability, visibility and the whole-set build, refusals to byte identity."""
import ctypes as C

import numpy as np
import pytest

import plain_build_checks as PB
from helpers import make_vectors
from lifecycle_checks import make_tids, well_formed
from oracle import oracle_py as O

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
INV = 0xFFFFFFFF


def _plain(gpu_ctx, X, *, distance, R, dim_index=None, tids=None):
    """a plain index over the rows of X with an empty graph, its divisors in place"""
    import pgvectorscale_amd as P
    n, dim = X.shape
    ix = P.DiskAnnIndex.alloc(gpu_ctx, n=n, dim_full=dim, dim_index=dim_index, num_neighbors=R, distance_type=distance,
                              storage_type=P._lib.VS_STORAGE_PLAIN)
    if n:
        vp, stride = ix.array(P._lib.ARR_VECS)
        Xp = np.zeros((n, stride), np.float32)
        Xp[:, :dim] = X
        gpu_ctx.upload(vp, Xp)
        ix.refresh_norms()
        if tids is not None:
            gpu_ctx.upload(ix.array(P._lib.ARR_TIDS)[0], np.ascontiguousarray(tids, np.uint64))
    return ix


def _edge_corpus(n, dim, seed):
    """un-normalised gauss rows; rows 20..29 repeat row 5 (both branches of the FLT_EPSILON rule), row 7 is zero"""
    X = make_vectors(n, dim, seed, "gauss")
    X *= np.random.default_rng(seed).uniform(0.2, 3.0, (n, 1)).astype(np.float32)
    X[20:30] = X[5]
    X[7] = 0
    return X


def _oracle_plain(X, nbrs, tids, *, distance, dim_index, R, start):
    w = (dim_index + 63) // 64
    return O.OracleIndex(codes=np.zeros((X.shape[0], w), np.uint64), nbrs=nbrs, heap_tids=tids, vecs=X, mean=np.zeros(dim_index, np.float32),
                         m2=np.zeros(dim_index, np.float32), count=0, bits=1, dim_index=dim_index, num_neighbors=R,
                         distance_type=distance, default_start=start, storage_plain=True)


# ---- 1. prune ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distance", [O.L2, O.COSINE])
@pytest.mark.parametrize("R", [4, 24, 50, 70])
@pytest.mark.parametrize("dim,dim_index", [(8, 8), (40, 40), (64, 64), (40, 24)])
def test_prune_plain_is_exact(gpu_ctx, oracle, dim, dim_index, R, distance):
    """rows, order and lengths of vs_prune_plain against the restatement: candidate counts around R, at one and two passes of eight
    candidates per lane group and beyond 64; one, two and three alpha passes; points and candidates among duplicated rows and the
    zero row; lists that name the point and repeat ids"""
    n = 200
    X = _edge_corpus(n, dim, 31 + dim)
    ix = _plain(gpu_ctx, X, distance=distance, R=R, dim_index=dim_index)
    rule = PB.PairRule(oracle, X, distance, dim_index)
    rng = np.random.default_rng(R * 100 + dim)
    specials = [5, 7, 21, 50]  # a duplicated row, the zero row, a copy, an ordinary row
    points, lists = [], []
    for t, Cn in enumerate(sorted({R - 1, R, R + 1, 64, 65, 130})):
        for p in (specials[t % 4], int(rng.integers(30, n))):
            others = [i for i in range(n) if i != p]
            cand = rng.choice(others, Cn, replace=False).tolist()
            if p != 5 and 5 not in cand:  # duplicates of one another among the candidates
                cand[:3] = [c for c in (5, 22, 27) if c != p][:3]
                cand = list(dict.fromkeys(cand))
                while len(cand) < Cn:
                    x = int(rng.integers(0, n))
                    if x != p and x not in cand:
                        cand.append(x)
            if t % 2:  # the list names the point and repeats ids
                cand = cand + [p] + cand[:5] + [p]
                rng.shuffle(cand)
            assert len(set(cand) - {p}) == Cn
            points.append(p)
            lists.append(cand)
    for max_alpha in (1.0, 1.2, 1.5):
        rows, lens = ix.prune_plain(points, lists, max_alpha=max_alpha)
        for i, (p, cand) in enumerate(zip(points, lists)):
            want = rule.prune(p, cand, R, max_alpha)
            print(f"alpha {max_alpha} point {p} C {len(set(cand) - {p})}: kept {int(lens[i])}, want {len(want)}")
            assert int(lens[i]) == len(want), (max_alpha, p)
            assert rows[i, :len(want)].tolist() == want, (max_alpha, p)
            assert (rows[i, len(want):] == INV).all()
    ix.close()


# ---- 2. mates ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distance", [O.L2, O.COSINE])
@pytest.mark.parametrize("dim", [40, 64])
def test_batch_mates_plain_is_exact(gpu_ctx, oracle, dim, distance):
    """ids and f32 distances of vs_batch_mates_plain: ranges of one row, two, around one tile of 64 and over two; c from 1 to 64,
    c >= n - 1 included; duplicated rows tie to the lower row"""
    X = _edge_corpus(200, dim, 57 + dim)
    ix = _plain(gpu_ctx, X, distance=distance, R=8)
    rule = PB.PairRule(oracle, X, distance)
    first = 3  # (rows 5, 7 and 20..29 are inside every range of more than a few rows)
    for n in (1, 2, 63, 64, 65, 130):
        for c in (1, 16, 64):
            ids, dist = ix.batch_mates_plain(first, n, c)
            wids, wdist = rule.mates(first, n, c)
            assert (ids == wids).all(), (n, c)
            assert (dist.view(np.uint32) == wdist.view(np.uint32)).all(), (n, c)
    ix.close()


# ---- 3. build, small shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,R,L", [(1, 8, 10), (2, 8, 10), (60, 8, 10), (300, 4, 1)])
def test_plain_build_small_shapes(gpu_ctx, oracle, n, R, L):
    import pgvectorscale_amd as P
    X = make_vectors(n, 64, 21, "gauss")
    ix = _plain(gpu_ctx, X, distance=P.VS_COSINE, R=R)
    ix.build_graph(search_list_size=L, max_alpha=1.2)
    assert ix.desc.default_start == 0
    nb = ix.download(codes=False)["nbrs"]
    well_formed(nb, R)
    seen = PB.reach(nb, 0)
    assert ix.build_unreachable() == n - int(seen.sum())
    if n == 2:
        assert nb[0, 0] == 1 and nb[1, 0] == 0
    ix.close()


# ---- 4. build, parity on the result ----------------------------------------------------------------------------------------------
def test_plain_built_graph_searches_like_the_oracle(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    n, dim, R, L = 1200, 40, 24, 30
    X = make_vectors(n, dim, 40, "gauss")
    X *= np.random.default_rng(40).uniform(0.2, 3.0, (n, 1)).astype(np.float32)  # un-normalised rows
    X[3] = 0
    tids = make_tids(0, n)
    tids[np.random.default_rng(41).random(n) < 0.1] &= ~np.uint64(0xFFFF)
    ix = _plain(gpu_ctx, X, distance=P.VS_COSINE, R=R, tids=tids)
    ix.build_graph(search_list_size=40, max_alpha=1.2)
    host = ix.download(codes=False)
    well_formed(host["nbrs"], R)
    assert (host["heap_tids"] == tids).all()
    oidx = _oracle_plain(X, host["nbrs"], tids, distance=O.COSINE, dim_index=dim, R=R, start=ix.desc.default_start)
    q = make_vectors(40, dim, 9, "gauss")
    k = 25
    gi, gt, gd, gst = ix.search_batch(q, search_list_size=L, rescore=50, k=k)
    oi, od, ost = oidx.search_batch(q, L=L, rescore=50, k=k)
    assert (gi == oi).all()
    assert (gd.view(np.uint32) == od.view(np.uint32)).all()
    live = gi != INV
    assert (gt[live] == tids[gi[live]]).all()
    for key in ("visited_nodes", "candidate_nodes", "full_distance_comparisons", "node_reads", "next_calls"):
        assert gst[key] == ost[key], key
    assert gst["quantized_distance_comparisons"] == 0
    si, sd, _ = ix.stream_batch(q, search_list_size=L, m=k)
    assert (si == oi).all() and (sd[si != INV] == od.view(np.uint32)[si != INV]).all()
    ix.close()


# ---- 5. quality ------------------------------------------------------------------------------------------------------------------
QUALITY = dict(n=1500, nq=256)


def _quality_setup(seed):
    X = make_vectors(QUALITY["n"], 48, seed, "gauss")
    Q = make_vectors(QUALITY["nq"], 48, seed + 100, "gauss")
    return X, Q, PB.exact_top10(X, Q)


def test_plain_build_quality(gpu_ctx, oracle):
    """recall@10 of the oracle's plain search at L = 32 over the device-built graph: (a) strictly above the oracle's SBQ-code graph
    of the same vectors, (b) >= the sequential f32 Vamana of plain_build_checks on the same seed minus that restatement's own spread
    over corpus seeds 9..13 (a constant measured without the device, SEQ_RECALL_SPREAD)"""
    import pgvectorscale_amd as P
    X, Q, truth = _quality_setup(9)
    ix = _plain(gpu_ctx, X, distance=P.VS_L2, R=16)
    ix.build_graph(search_list_size=32, max_alpha=1.2, batch_max=64)
    nb = ix.download(codes=False)["nbrs"]
    well_formed(nb, 16)
    assert ix.build_unreachable() == 0
    got = PB.recall_at_10(oracle, X, nb, ix.desc.default_start, Q, truth, 32)
    sb, sstart = PB.sbq_graph(oracle, X, 16, 32)
    sbq = PB.recall_at_10(oracle, X, sb, sstart, Q, truth, 32)
    seq = PB.recall_at_10(oracle, X, PB.sequential_vamana(X, 16, 32), 0, Q, truth, 32)
    print(f"recall@10: device plain build {got:.4f}, SBQ-code graph {sbq:.4f}, sequential f32 Vamana {seq:.4f}, "
          f"margin {PB.SEQ_RECALL_SPREAD}")
    assert got > sbq
    assert got >= seq - PB.SEQ_RECALL_SPREAD
    ix.close()


# ---- 6. insert -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reserved", [True, False])
def test_insert_into_a_built_plain_index(gpu_ctx, oracle, reserved):
    import pgvectorscale_amd as P
    n0 = 1200
    sizes = [100, 100, 100, 1, 0]
    n1 = n0 + sum(sizes)
    X = make_vectors(n1, 48, 9, "gauss")
    Q = make_vectors(QUALITY["nq"], 48, 109, "gauss")
    truth = PB.exact_top10(X, Q)
    tids = make_tids(0, n1)
    ix = _plain(gpu_ctx, X[:n0], distance=P.VS_L2, R=16, tids=tids[:n0])
    ix.build_graph(search_list_size=32, max_alpha=1.2, batch_max=64)
    if reserved:
        ix.reserve(n1)
    at = n0
    for m in sizes:
        cap = ix.capacity
        st = ix.insert(X[at:at + m], tids[at:at + m], search_list_size=32, max_alpha=1.2, batch_max=64)
        assert st["first_node"] == at and st["inserted"] == m and st["orphans_left"] == 0, st
        assert st["batches"] == (m + 63) // 64, st
        assert st["grew"] == int(at + m > cap) and not (reserved and st["grew"]), st
        assert st["mate_edges"] > 0 or m <= 1, st
        at += m
        assert ix.desc.n == at
    host = ix.download(codes=False, vecs=True)
    assert (host["vecs"] == X).all() and (host["heap_tids"] == tids).all()
    well_formed(host["nbrs"], 16)
    assert PB.reach(host["nbrs"], ix.desc.default_start)[n0:].all()  # every new node is reachable from the start
    probe = X[n1 - 5:n1]  # the new rows are found, with their tids
    gi, gt, _, _ = ix.search_batch(probe, search_list_size=32, rescore=0, k=1)
    assert gi[:, 0].tolist() == list(range(n1 - 5, n1)) and (gt[:, 0] == tids[n1 - 5:n1]).all()
    # the grown graph against the whole-set device build of the same rows
    grown = PB.recall_at_10(oracle, X, host["nbrs"], ix.desc.default_start, Q, truth, 32)
    whole = _plain(gpu_ctx, X, distance=P.VS_L2, R=16)
    whole.build_graph(search_list_size=32, max_alpha=1.2, batch_max=64)
    ref = PB.recall_at_10(oracle, X, whole.download(codes=False)["nbrs"], 0, Q, truth, 32)
    print(f"recall@10: grown by inserts {grown:.4f}, whole-set build {ref:.4f}, margin {PB.SEQ_RECALL_SPREAD}")
    assert grown >= ref - PB.SEQ_RECALL_SPREAD
    whole.close()
    ix.close()


def test_snapshots_hide_inserted_plain_rows_and_the_own_mask_shows_them(gpu_ctx, oracle):
    """dim_index < dim_full, so that scans resort on the heap vectors and the visibility masks apply (a plain scan over all its
    dimensions never fetches the heap, AM/scan.rs:392-399)"""
    import pgvectorscale_amd as P
    n0, m = 100, 20
    X = make_vectors(n0 + m, 40, 14, "gauss")
    tids = make_tids(0, n0 + m)
    ix = _plain(gpu_ctx, X[:n0], distance=P.VS_L2, R=8, dim_index=24, tids=tids[:n0])
    ix.build_graph(search_list_size=20)
    P._lib.check(ix._L.vs_index_snapshot_put(ix.h, 1, np.ones(n0, np.uint8).ctypes.data_as(C.c_void_p)))
    ix.set_visibility(np.ones(n0, np.uint8))
    st = ix.insert(X[n0:], tids[n0:], search_list_size=20)
    assert st["inserted"] == m and st["grew"] == 1 and st["orphans_left"] == 0, st
    gi, gt, _, _ = ix.search_batch(X[n0:], search_list_size=40, rescore=10, k=1)
    assert gi[:, 0].tolist() == list(range(n0, n0 + m)) and (gt[:, 0] == tids[n0:]).all()
    P._lib.check(ix._L.vs_index_snapshot_use(ix.h, 1, None))
    gi, _, _, _ = ix.search_batch(X[n0:], search_list_size=40, rescore=10, k=5)
    assert (gi != INV).any() and (gi[gi != INV] < n0).all()  # a snapshot stored before the insert cannot see the new rows
    P._lib.check(ix._L.vs_index_snapshot_use(ix.h, 0, None))
    ix.close()


def test_insert_into_an_empty_plain_index(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    X = make_vectors(51, 40, 12, "gauss")
    X *= np.random.default_rng(12).uniform(0.2, 3.0, (51, 1)).astype(np.float32)
    tids = make_tids(0, 51)
    for distance, dim_index in ((P.VS_COSINE, 24), (P.VS_L2, None)):
        ix = _plain(gpu_ctx, X[:0], distance=distance, R=8, dim_index=dim_index)
        assert ix.desc.default_start == INV
        st = ix.insert(X[:1], tids[:1], search_list_size=20)
        assert st["first_node"] == 0 and st["inserted"] == 1 and st["grew"] == 1 and st["orphans_left"] == 0, st
        assert ix.desc.default_start == 0 and ix.desc.n == 1
        st = ix.insert(X[1:], tids[1:], search_list_size=20)
        assert st["first_node"] == 1 and st["inserted"] == 50 and st["grew"] == 1 and st["orphans_left"] == 0, st
        host = ix.download(codes=False, vecs=True)
        assert (host["vecs"] == X).all() and (host["heap_tids"] == tids).all()
        well_formed(host["nbrs"], 8)
        assert PB.reach(host["nbrs"], 0).all()
        # scans of the grown index equal the oracle's over the downloaded arrays, bit for bit (the divisors of the new rows included)
        oidx = _oracle_plain(X, host["nbrs"], tids, distance=distance, dim_index=dim_index or 40, R=8, start=0)
        q = make_vectors(8, 40, 13, "gauss")
        gi, _, gd, _ = ix.search_batch(q, search_list_size=20, rescore=10, k=5)
        oi, od, _ = oidx.search_batch(q, L=20, rescore=10, k=5)
        assert (gi == oi).all() and (gd.view(np.uint32) == od.view(np.uint32)).all()
        ix.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def _bytes(ix):
    h = ix.download(codes=True, nbrs=True, tids=True, vecs=True)
    return b"".join(h[k].tobytes() for k in ("codes", "nbrs", "heap_tids", "vecs")), ix.desc.n, ix.desc.default_start, ix.capacity


def _refused(ix, call, match=None):
    import pgvectorscale_amd as P
    before = _bytes(ix)
    with pytest.raises(P.VsError, match=match) as e:
        call()
    assert e.value.code == -1  # VS_ERR_INVALID
    assert _bytes(ix) == before


def test_refusals_leave_every_byte_as_it_was(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    from lifecycle_checks import fresh_index
    n = 120
    X = make_vectors(n + 4, 40, 17, "gauss")
    tids = make_tids(n, 4)
    # out-of-range build parameters: nothing of a built graph is lost, plain and SBQ alike
    built = _plain(gpu_ctx, X[:n], distance=P.VS_L2, R=8)
    built.build_graph(search_list_size=20)
    sbq = fresh_index(gpu_ctx, X[:n], distance=P.VS_L2, bits=2, R=8, L=20)
    for ix in (built, sbq):
        assert (ix.download()["nbrs"] != INV).any()
        _refused(ix, lambda: ix.build_graph(search_list_size=0), "search_list_size")
        _refused(ix, lambda: ix.build_graph(search_list_size=1001), "search_list_size")
        _refused(ix, lambda: ix.build_graph(search_list_size=20, max_alpha=0.9), "max_alpha")
        _refused(ix, lambda: ix.build_graph(search_list_size=20, max_alpha=5.5), "max_alpha")
    sbq.close()
    # label sets, what stays out of scope
    _refused(built, lambda: built.insert(X[n:], tids, labels=[[1], [2], [1, 2], []], search_list_size=20), "label")
    _refused(built, lambda: built.set_labels(np.zeros(n + 1, np.uint32), np.zeros(0, np.int16)), "label")
    _refused(built, lambda: built.consolidate_deletes(), "plain")
    _refused(built, lambda: built.write_pages(), "plain")
    _refused(built, lambda: built.repair_labels(), "plain")
    st = built.insert(X[n:], tids, search_list_size=20)  # (and the index still takes rows)
    assert st["inserted"] == 4 and st["orphans_left"] == 0
    built.close()
    # the inner-product distance: a graph made elsewhere stays searchable, and untouched by build and insert
    nbrs, start = PB.sbq_graph(oracle, X[:n], 8, 20)
    ip = P.DiskAnnIndex.upload(gpu_ctx, codes=None, nbrs=nbrs, heap_tids=make_tids(0, n), vecs=X[:n], mean=None, m2=None, count=0, bits=None,
                               dim_index=40, num_neighbors=8, distance_type=P.VS_IP, default_start=start,
                               storage_type=P._lib.VS_STORAGE_PLAIN)
    _refused(ip, lambda: ip.build_graph(search_list_size=20), "inner-product")
    _refused(ip, lambda: ip.insert(X[n:], tids, search_list_size=20), "inner-product")
    with pytest.raises(P.VsError, match="inner-product"):
        ip.prune_plain([1], [[2, 3]])
    gi, _, _, _ = ip.search_batch(X[:3], search_list_size=20, rescore=0, k=3)
    assert (gi != INV).any()
    ip.close()
    # an uploaded plain index mirrors a relation the page writer cannot write back: it still takes no rows
    up = P.DiskAnnIndex.upload(gpu_ctx, codes=None, nbrs=nbrs, heap_tids=make_tids(0, n), vecs=X[:n], mean=None, m2=None, count=0, bits=None,
                               dim_index=40, num_neighbors=8, distance_type=P.VS_L2, default_start=start,
                               storage_type=P._lib.VS_STORAGE_PLAIN)
    _refused(up, lambda: up.insert(X[n:], tids, search_list_size=20), "uploaded")
    up.close()
    # alloc: a plain index is its vectors
    with pytest.raises(P.VsError, match="with_vecs") as e:
        P.DiskAnnIndex.alloc(gpu_ctx, n=10, dim_full=40, num_neighbors=8, with_vecs=False, storage_type=P._lib.VS_STORAGE_PLAIN)
    assert e.value.code == -1
