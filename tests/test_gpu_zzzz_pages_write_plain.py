"""vs_pages_out_open_plain: a device-resident `plain` storage index written out as the pages of a `diskann` index relation
(k_pages_encode_plain composes the PlainNode pages on the device).  Every expectation is the oracle's writer
(oracle/pages_py.py::write_plain_index(vectors=, nbrs=, heap_tids=, num_neighbors=, meta=)) byte for byte, or what the existing
readers make of the result.  Item bytes, items per page and blocks of the shapes used here, from the oracle:
700 x 48 R 16: 352 / 22 / 33; 301 x 100 R 10: 512 / 15 / 22; 41 x 768 R 50: 3504 / 2 / 22; 9 x 1536 R 50: 6576 / 1 / 10;
5 x 1930 R 50: 8152 / 1 / 6; 1 x 48 R 16: 352 / 1 / 2.  Also runs on the lockstep interpreter (tests/test_emu_pages_write_plain.py)."""
import ctypes as C

import numpy as np
import pytest

from helpers import make_vectors
from oracle import pages_py as PG

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

B = PG.BLCKSZ
INV = 0xFFFFFFFF
INVALID, STATE = -1, -5  # VS_ERR_INVALID, VS_ERR_STATE


def _first_difference(got, want):
    if len(got) != len(want):
        return f"{len(got)} bytes, expected {len(want)}"
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    at = int(np.flatnonzero(a != b)[0])
    return f"first difference in block {at // B} at byte {at % B}: {a[at]} != {b[at]} ({int((a != b).sum())} bytes differ)"


def _assert_same(got, want):
    assert got == want, _first_difference(got, want)


def _hand_made(n, R, seed):
    """neighbor lists of every length 0 .. min(R, n - 1) without duplicates (and without the node itself), padded with the
    sentinel; heap tids with about a tenth of the offsets 0"""
    rng = np.random.default_rng(seed)
    nbrs = np.full((n, R), INV, np.uint32)
    for i in range(n):
        k = min(i % (R + 1), n - 1)
        if k:
            others = np.delete(np.arange(n, dtype=np.uint32), i)
            nbrs[i, :k] = rng.permutation(others)[:k]
    off = rng.integers(1, 200, n).astype(np.uint64)
    off[rng.random(n) < 0.1] = 0
    if n > 10:
        off[3] = 0
    tids = (rng.integers(0, 1 << 20, n).astype(np.uint64) << np.uint64(16)) | off
    return nbrs, tids


class Plain:
    """the flat arrays of one plain index, what the oracle writes for them, and an upload of them"""

    def __init__(self, oracle, n, dim_full, R, distance, seed, dim_index=None, rows=None, default_start=0):
        self.O = oracle
        self.n, self.dim_full, self.dim_index, self.R, self.distance = n, dim_full, dim_index or dim_full, R, distance
        self.vecs = make_vectors(n, dim_full, seed, "gauss") if rows is None else np.ascontiguousarray(rows, np.float32)
        self.nbrs, self.tids = _hand_made(n, R, seed + 1)
        self.start = default_start

    def node_vectors(self):
        """PlainNode.vector of every node (oracle/vs_oracle.cpp, plain_distance): the index slice, for cosine preprocess_cosine of it
        -> (vectors, changed?)"""
        out = self.vecs[:, :self.dim_index].copy()
        changed = np.zeros(self.n, bool)
        if self.distance == self.O.COSINE:
            for i in range(self.n):
                out[i], changed[i] = self.O.preprocess_cosine(out[i])
        return out, changed

    def meta(self, **kw):
        m = dict(storage_type=0, num_dimensions=self.dim_full, num_dimensions_to_index=self.dim_index, bq_num_bits_per_dimension=1,
                 distance_type=self.distance, num_neighbors=self.R, default_start=None if self.start == INV else self.start,
                 labeled_starts={}, extension_version="0.8.0", search_list_size=100, max_alpha=1.2)
        m.update(kw)
        return m

    def relation(self):
        return PG.write_plain_index(vectors=self.node_vectors()[0], nbrs=self.nbrs, heap_tids=self.tids, num_neighbors=self.R,
                                    meta=self.meta())

    def upload(self, ctx):
        import pgvectorscale_amd as P
        return P.DiskAnnIndex.upload(ctx, codes=None, nbrs=self.nbrs, heap_tids=self.tids, vecs=self.vecs, mean=None, m2=None, count=0,
                                     bits=1, dim_index=self.dim_index, num_neighbors=self.R, distance_type=self.distance,
                                     default_start=self.start, storage_type=P._lib.VS_STORAGE_PLAIN)


def _relation_of(ix):
    """the oracle's writer over the arrays of a plain L2 index as they are on the device now -> (bytes, host arrays)"""
    host = ix.download(codes=False, vecs=True)
    d = ix.desc
    meta = dict(storage_type=0, num_dimensions=d.dim_full, num_dimensions_to_index=d.dim_index, bq_num_bits_per_dimension=d.bits,
                distance_type=d.distance_type, num_neighbors=d.num_neighbors,
                default_start=None if d.default_start == INV else int(d.default_start), labeled_starts={}, extension_version="0.8.0",
                search_list_size=100, max_alpha=1.2)
    w = PG.write_plain_index(vectors=host["vecs"][:, :d.dim_index], nbrs=host["nbrs"], heap_tids=host["heap_tids"],
                             num_neighbors=d.num_neighbors, meta=meta)
    return w.rel.tobytes(), host


def _small_ring_context():
    """a context with 2 x 24 KiB of staging: three pages per chunk"""
    import pgvectorscale_amd as P
    from pgvectorscale_amd._lib import check
    ctx = P.Context.__new__(P.Context)
    ctx._L, ctx.device, ctx.h = P.load(), 0, C.c_void_p()
    check(ctx._L.vs_ctx_create_staging(0, 3 * B, C.byref(ctx.h)))
    return ctx


@pytest.fixture(scope="module")
def l2(oracle):
    return Plain(oracle, 700, 48, 16, oracle.L2, seed=31)


@pytest.fixture(scope="module")
def cosine(oracle):
    """dim_full 48 / dim_index 45: items of 4 * 45 + 8 * 12 + 32 = 308 bytes, 4 mod 8; a zero row, a row whose index slice is
    exactly normalised and the same row scaled by 1.001 among the gaussian ones"""
    rows = make_vectors(230, 48, 37, "gauss")
    rows[7] = 0
    unit = np.zeros(48, np.float32)
    unit[[2, 11, 30, 44]] = 0.5  # the slice's norm is exactly 1; the three dimensions past it are not zero
    unit[45:] = (3.0, -2.0, 0.25)
    rows[19] = unit
    rows[20] = unit
    rows[20, :45] *= np.float32(1.001)
    return Plain(oracle, 230, 48, 12, oracle.COSINE, seed=41, dim_index=45, rows=rows, default_start=4)


def test_l2_index_is_written_as_the_oracle_writes_it(gpu_ctx, l2):
    from pgvectorscale_amd.pages import IndexPages, PagesOut
    p = l2
    w = p.relation()
    want = w.rel.tobytes()
    lens = (p.nbrs != INV).sum(1)
    assert set(lens.tolist()) == set(range(p.R + 1)) and 40 < ((p.tids & 0xFFFF) == 0).sum() < 110
    assert len(want) // B == 33 and max(o for _, o in w.node_ptrs) == 22 and len(w.rel.item(1, 1)) == 352
    ix = p.upload(gpu_ctx)
    _assert_same(ix.write_pages(plain=True), want)
    out = PagesOut(ix, plain=True)
    nb = out.n_blocks
    assert nb == len(w.rel.pages) == 33
    # the reader's view of the same relation: what vs_pages_out_open_plain reports
    rd = IndexPages(plain=True)
    rd.add(want)
    ri = rd.finish()
    for f in ("n_blocks", "n_nodes", "words", "num_neighbors", "has_labels", "n_deleted", "n_label_vals", "new_pages", "meta_magic", "meta_version"):
        assert getattr(out.info, f) == getattr(ri, f), f
    assert list(out.info.pages_by_type) == list(ri.pages_by_type) and ri.n_deleted > 0 and ri.new_pages == 0
    assert ri.words == 48 and ri.has_labels == 0 and ri.pages_by_type[PG.PT_NODE] == 32 and ri.pages_by_type[PG.PT_SBQ_NODE] == 0
    assert ri.n_deleted == int(((p.tids & 0xFFFF) == 0).sum())
    rd.close()
    _assert_same(out.read().tobytes(), want)
    cut = [0, nb // 3, 2 * nb // 3, nb]
    parts = {}
    for i in (2, 1, 0):  # three ranges, last one first
        parts[i] = out.read(cut[i], cut[i + 1] - cut[i]).tobytes()
    _assert_same(parts[0] + parts[1] + parts[2], want)
    for b in reversed(range(nb)):  # single blocks
        assert out.read(b, 1).tobytes() == want[b * B:(b + 1) * B], b
    _assert_same(out.read().tobytes(), want)  # and the same bytes again
    assert [out.item_pointer_of(i) for i in range(p.n)] == [tuple(q) for q in w.node_ptrs]
    # into device memory
    d = gpu_ctx.alloc(nb * B)
    out.read_dev(d)
    _assert_same(gpu_ctx.download(d, np.empty(nb * B, np.uint8)).tobytes(), want)
    out.read_dev(d, 3, 5)
    _assert_same(gpu_ctx.download(d, np.empty(5 * B, np.uint8)).tobytes(), want[3 * B:8 * B])
    gpu_ctx.free(d)
    # gathered: a shuffled list with repeats
    rng = np.random.default_rng(5)
    blocks = rng.permutation(np.concatenate([np.arange(nb), rng.integers(0, nb, 9)])).astype(np.uint32)
    got = out.read_blocks(blocks).tobytes()
    for i, b in enumerate(blocks.tolist()):
        assert got[i * B:(i + 1) * B] == want[b * B:(b + 1) * B], (i, b)
    # a block the relation does not have: refused, nothing written
    import pgvectorscale_amd as P
    buf = np.full((nb + 2) * B, 0xCD, np.uint8)
    for first, cnt in ((0, nb + 1), (nb, 1), (nb - 1, 2)):
        with pytest.raises(P.VsError, match="blocks"):
            out.read(first, cnt, out=buf)
    with pytest.raises(P.VsError, match="blocks"):
        out.read_blocks(np.array([1, nb, 2], np.uint32), out=buf)
    assert (buf == 0xCD).all()
    _assert_same(out.read(nb - 3, 3).tobytes(), want[-3 * B:])  # the handle is still good
    out.close()
    ix.close()


def test_last_node_page_with_one_item(gpu_ctx, oracle):
    p = Plain(oracle, 301, 100, 10, oracle.L2, seed=33, default_start=300)
    w = p.relation()
    want = w.rel.tobytes()
    assert len(want) // B == 22 and len(w.rel.item(1, 1)) == 512 and w.node_ptrs[300] == (21, 1) and w.node_ptrs[299] == (20, 15)
    ix = p.upload(gpu_ctx)
    _assert_same(ix.write_pages(plain=True), want)
    ix.close()


def test_cosine_index_slice_with_items_that_are_no_multiple_of_eight(gpu_ctx, cosine):
    from pgvectorscale_amd.pages import PagesOut
    p = cosine
    vectors, changed = p.node_vectors()
    # precondition: the oracle left rows alone (the zero row, the normalised one) and changed rows (the scaled one among them)
    assert not changed[7] and not changed[19] and changed[20] and changed.sum() > 200
    assert (vectors[19] == p.vecs[19, :45]).all() and (vectors[20] != p.vecs[20, :45]).any()
    w = p.relation()
    want = w.rel.tobytes()
    assert len(w.rel.item(1, 1)) == 308 and 308 % 8 == 4
    ix = p.upload(gpu_ctx)
    out = PagesOut(ix, plain=True)
    assert out.info.words == 45
    _assert_same(out.read().tobytes(), want)
    assert [out.item_pointer_of(i) for i in range(p.n)] == [tuple(q) for q in w.node_ptrs]
    out.close()
    ix.close()


@pytest.mark.parametrize("n,dim,item,K,blocks", [(41, 768, 3504, 2, 22), (9, 1536, 6576, 1, 10), (5, 1930, 8152, 1, 6)])
def test_large_shapes_through_a_small_staging_ring(oracle, n, dim, item, K, blocks):
    """R = 50; three pages of staging per chunk, so the double-buffered encode / copy pipeline runs over several chunks with a
    partial last one.  One or two items fill a page here: the vector copy is what all four waves of a workgroup share."""
    from pgvectorscale_amd.pages import PagesOut
    p = Plain(oracle, n, dim, 50, oracle.L2, seed=dim, default_start=n - 1)
    w = p.relation()
    want = w.rel.tobytes()
    assert len(want) // B == blocks and len(w.rel.item(1, 1)) == item and max(o for _, o in w.node_ptrs) == K
    ctx = _small_ring_context()
    try:
        ix = p.upload(ctx)
        out = PagesOut(ix, plain=True)
        assert out.n_blocks == blocks and out.info.pages_by_type[PG.PT_NODE] == blocks - 1 > 3
        _assert_same(out.read().tobytes(), want)
        _assert_same(out.read(1, blocks - 2).tobytes(), want[B:-B])
        _assert_same(out.read_blocks(np.arange(blocks - 1, -1, -1, dtype=np.uint32)).tobytes(),
                     b"".join(want[b * B:(b + 1) * B] for b in reversed(range(blocks))))
        out.close()
        ix.close()
    finally:
        ctx.close()


def test_large_shapes_one_dimension_too_many_is_refused(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    from pgvectorscale_amd.pages import PagesOut
    p = Plain(oracle, 3, 1931, 50, oracle.L2, seed=3)
    with pytest.raises(AssertionError):
        p.relation()  # (the oracle's Tape refuses the item too)
    ix = p.upload(gpu_ctx)
    with pytest.raises(P.VsError, match="fit") as e:
        PagesOut(ix, plain=True)
    assert e.value.code == INVALID
    host = ix.download(codes=False, vecs=True)  # the index is still usable
    assert (host["vecs"] == p.vecs).all() and (host["nbrs"] == p.nbrs).all()
    gi, _, _, _ = ix.search_batch(p.vecs[:2], search_list_size=8, rescore=8, k=1)
    assert gi.shape == (2, 1)
    ix.close()


def test_smallest_indexes(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    from pgvectorscale_amd.pages import PagesOut
    # one row
    p = Plain(oracle, 1, 48, 16, oracle.L2, seed=51)
    w = p.relation()
    want = w.rel.tobytes()
    assert len(want) // B == 2 and len(w.rel.item(1, 1)) == 352
    ix = p.upload(gpu_ctx)
    _assert_same(ix.write_pages(plain=True), want)
    ix.close()
    # no default start: start_nodes = None
    p = Plain(oracle, 30, 48, 16, oracle.L2, seed=52, default_start=INV)
    want = p.relation().rel.tobytes()
    m = PG.parse_meta_page(PG.read_chain(_as_relation(want), 0, 2, PG.PT_META))
    assert m["default_start"] is None and m["storage_type"] == 0 and m["quantizer_metadata"] == (INV, 0) and not m["has_labels"]
    ix = p.upload(gpu_ctx)
    _assert_same(ix.write_pages(plain=True), want)
    ix.close()
    # zero rows (vs_index_alloc makes such an index): the Meta page and one empty node page
    ix = P.DiskAnnIndex.alloc(gpu_ctx, n=0, dim_full=48, num_neighbors=16, distance_type=P.VS_L2, storage_type=P._lib.VS_STORAGE_PLAIN)
    assert ix.desc.n == 0 and ix.desc.default_start == INV
    want = PG.write_plain_index(vectors=np.zeros((0, 48), np.float32), nbrs=np.zeros((0, 16), np.uint32), heap_tids=np.zeros(0, np.uint64),
                                num_neighbors=16, meta=Plain(oracle, 1, 48, 16, oracle.L2, seed=1, default_start=INV).meta()).rel.tobytes()
    assert len(want) // B == 2
    out = PagesOut(ix, plain=True)
    assert out.n_blocks == 2 and out.info.n_nodes == 0 and out.info.pages_by_type[PG.PT_NODE] == 1
    _assert_same(out.read().tobytes(), want)
    out.close()
    ix.close()


def _as_relation(raw):
    rel = PG.Relation()
    rel.pages = [bytearray(raw[b * B:(b + 1) * B]) for b in range(len(raw) // B)]
    return rel


def test_round_trip_through_the_plain_reader(gpu_ctx, cosine):
    from pgvectorscale_amd.pages import IndexPages
    p = cosine
    src = p.upload(gpu_ctx)
    raw = src.write_pages(plain=True)
    rd = IndexPages(plain=True)
    rd.add(raw)
    info = rd.finish()
    assert info.n_nodes == p.n and info.words == 45
    arr = rd.arrays()
    dev = src.download(codes=False)
    assert (arr["nbrs"] == dev["nbrs"]).all() and (arr["heap_tids"] == dev["heap_tids"]).all()
    assert (arr["nbrs"] == p.nbrs).all() and (arr["heap_tids"] == p.tids).all()
    assert arr["vecs"].view(np.uint32).tobytes() == p.node_vectors()[0].view(np.uint32).tobytes()
    m, d, starts = rd.meta()
    assert (m["storage_type"], m["has_labels"], m["quantizer_block"], m["quantizer_offset"]) == (0, 0, INV, 0) and starts == {}
    assert (d.default_start, d.dim_full, d.dim_index, d.num_neighbors, d.distance_type) == (p.start, 48, 45, p.R, p.distance)
    ix = rd.upload_plain(gpu_ctx, distance_type=p.distance, default_start=int(d.default_start), vecs=p.vecs)
    rd.close()
    q = make_vectors(64, 48, 77, "gauss")
    gi, gt, gd, _ = ix.search_batch(q, search_list_size=32, rescore=32, k=10)
    si, st, sd, _ = src.search_batch(q, search_list_size=32, rescore=32, k=10)
    assert (si != INV).any()
    assert (gi == si).all() and (gt == st).all() and gd.view(np.uint32).tobytes() == sd.view(np.uint32).tobytes()
    ix.close()
    src.close()


def test_life_cycle_on_the_device(gpu_ctx, tmp_path):
    """alloc, build, write; vacuum two tuples and patch two blocks; insert 40 rows and patch what they touched"""
    import pgvectorscale_amd as P
    from pgvectorscale_amd.pages import PagesOut
    n, dim, R = 600, 48, 16
    X = make_vectors(n + 40, dim, 61, "gauss")
    tids = (np.arange(1, n + 41, dtype=np.uint64) << np.uint64(16)) | np.uint64(1)
    ix = P.DiskAnnIndex.alloc(gpu_ctx, n=n, dim_full=dim, num_neighbors=R, distance_type=P.VS_L2, storage_type=P._lib.VS_STORAGE_PLAIN)
    vp, stride = ix.array(P._lib.ARR_VECS)
    assert stride == dim
    gpu_ctx.upload(vp, X[:n])
    gpu_ctx.upload(ix.array(P._lib.ARR_TIDS)[0], tids[:n])
    ix.refresh_norms()
    ix.build_graph(search_list_size=32, max_alpha=1.2)
    path = tmp_path / "rel"
    out = PagesOut(ix, plain=True)
    base = out.baseline()
    out.write_file(str(path), chunk_blocks=5)
    ptr = [out.item_pointer_of(i) for i in (5, 300)]
    out.close()
    before, _ = _relation_of(ix)
    _assert_same(path.read_bytes(), before)
    # a. ambulkdelete of two tuples: exactly the two node blocks that hold them
    st = ix.bulk_delete(tids[[5, 300]])
    assert st["tuples_removed"] == 2
    after, host = _relation_of(ix)
    assert (host["heap_tids"][[5, 300]] & 0xFFFF == 0).all()
    out = PagesOut(ix, plain=True)
    blocks, nb_now, nb2 = out.delta(base)
    assert blocks.tolist() == sorted(b for b, _ in ptr) == [b for b in range(len(after) // B) if after[b * B:(b + 1) * B] != before[b * B:(b + 1) * B]]
    assert 0 < blocks.size < out.n_blocks and len(set(blocks.tolist())) == 2 and nb_now == out.n_blocks
    nb2.close()
    base2 = out.patch_file(str(path), base)
    out.close()
    base.close()
    _assert_same(path.read_bytes(), after)
    # b. aminsert of 40 rows: the blocks that differ between the two oracle relations, the appended ones among them
    before = after
    st = ix.insert(X[n:], tids[n:], search_list_size=32, max_alpha=1.2)
    assert st["inserted"] == 40 and st["orphans_left"] == 0
    after, host = _relation_of(ix)
    nb_b, nb_a = len(before) // B, len(after) // B
    want = [b for b in range(nb_a) if b >= nb_b or after[b * B:(b + 1) * B] != before[b * B:(b + 1) * B]]
    assert nb_a > nb_b and 0 < len(want) and min(want) < nb_b
    out = PagesOut(ix, plain=True)
    blocks, nb_now, nb3 = out.delta(base2)
    assert blocks.tolist() == want and nb_now == nb_a
    nb3.close()
    base3 = out.patch_file(str(path), base2)
    _assert_same(path.read_bytes(), after)
    # c. nothing is dirty against the fresh baseline
    again, nb_now, base4 = out.delta(base3)
    assert again.size == 0 and nb_now == nb_a
    for b in (base2, base3, base4):
        b.close()
    out.close()
    ix.close()


def test_what_the_plain_writer_refuses(gpu_ctx, oracle, l2):
    import pgvectorscale_amd as P
    from helpers import TestIndex
    from pgvectorscale_amd.pages import PagesOut
    # an SBQ index: vs_pages_out_open writes those
    ti = TestIndex(n=200, dim_full=32, bits=2, R=8, distance=oracle.L2, seed=9, kind="gauss", L_build=20)
    sbq = ti.upload(gpu_ctx)
    with pytest.raises(P.VsError, match="vs_pages_out_open") as e:
        PagesOut(sbq, plain=True)
    assert e.value.code == INVALID and "vs_pages_out_open_plain: " in str(e.value)
    assert len(sbq.write_pages()) % B == 0  # (and no writer was left open on it)
    sbq.close()
    # a plain index without the vector column
    d, h = P._lib.IndexDesc(), P._lib.IndexHost()
    d.n, d.dim_full, d.dim_index, d.bits, d.words = l2.n, 48, 48, 1, 1
    d.num_neighbors, d.distance_type, d.has_labels = l2.R, P.VS_L2, 0
    d.default_start, d.n_label_starts, d.storage_type = 0, 0, P._lib.VS_STORAGE_PLAIN
    h.nbrs, h.nbr_stride, h.heap_tids = l2.nbrs.ctypes.data, l2.R, l2.tids.ctypes.data
    raw = C.c_void_p()
    # (vs_index_upload does not let such an index come into being: the writer's own check is never reached from here)
    with pytest.raises(P.VsError, match="vecs") as e:
        P._lib.check(gpu_ctx._L.vs_index_upload(gpu_ctx.h, C.byref(d), C.byref(h), C.byref(raw)))
    assert e.value.code == INVALID and not raw.value
    # another page size
    ix = l2.upload(gpu_ctx)
    with pytest.raises(P.VsError, match="page_size") as e:
        PagesOut(ix, plain=True, page_size=4096)
    assert e.value.code == INVALID
    # without the flag a plain index keeps being refused
    with pytest.raises(P.VsError, match="SBQ"):
        PagesOut(ix)
    _assert_same(ix.write_pages(plain=True), l2.relation().rel.tobytes())
    ix.close()
    # an open plain writer holds an insert off, as an SBQ one does
    X = make_vectors(64, 16, 71, "gauss")
    tids = (np.arange(1, 65, dtype=np.uint64) << np.uint64(16)) | np.uint64(1)
    ix = P.DiskAnnIndex.alloc(gpu_ctx, n=60, dim_full=16, num_neighbors=8, distance_type=P.VS_L2, storage_type=P._lib.VS_STORAGE_PLAIN)
    gpu_ctx.upload(ix.array(P._lib.ARR_VECS)[0], X[:60])
    gpu_ctx.upload(ix.array(P._lib.ARR_TIDS)[0], tids[:60])
    ix.refresh_norms()
    ix.build_graph(search_list_size=20)
    out = PagesOut(ix, plain=True)
    with pytest.raises(P.VsError) as e:
        ix.insert(X[60:], tids[60:], search_list_size=20)
    assert e.value.code == STATE
    want, _ = _relation_of(ix)
    _assert_same(out.read().tobytes(), want)
    out.close()
    st = ix.insert(X[60:], tids[60:], search_list_size=20)
    assert st["inserted"] == 4
    ix.close()
