"""vs_pages_out_*: a device-resident index written out as the pages of a `diskann` index relation (k_pages_encode composes the
SbqNode pages on the device).  Every expectation is the oracle's writer (oracle/pages_py.py::write_index, means_first=True,
meta=...) byte for byte, or what the existing readers make of the result.  Also runs on the lockstep interpreter
(tests/test_pages_write_host.py).  Sorted last in the GPU tier."""
import numpy as np
import pytest

from helpers import TestIndex
from oracle import pages_py as PG

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]


def _meta(ti, label_starts=None, **kw):
    m = dict(num_dimensions=ti.dim_full, num_dimensions_to_index=ti.dim_index, bq_num_bits_per_dimension=ti.bits,
             distance_type=ti.distance, num_neighbors=ti.R, default_start=ti.start,
             labeled_starts=dict(ti.label_starts if label_starts is None else label_starts), extension_version="0.8.0",
             search_list_size=100, max_alpha=1.2)
    m.update(kw)
    return m


def _oracle_relation(ti, meta, **kw):
    return PG.write_index(codes=ti.codes, nbrs=ti.nbrs, heap_tids=ti.tids, mean=ti.mean, m2=ti.m2, count=ti.count,
                          label_off=ti.label_off, label_val=ti.label_val, means_first=True, meta=meta, **kw)


def _page_types(raw):
    return [raw[b * PG.BLCKSZ + PG.BLCKSZ - 8] for b in range(len(raw) // PG.BLCKSZ)]


def _first_difference(got, want):
    if len(got) != len(want):
        return f"{len(got)} bytes, expected {len(want)}"
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    at = int(np.flatnonzero(a != b)[0])
    return f"first difference in block {at // PG.BLCKSZ} at byte {at % PG.BLCKSZ}: {a[at]} != {b[at]} ({int((a != b).sum())} bytes differ)"


def _assert_same(got, want):
    assert got == want, _first_difference(got, want)


def _give_labels(ti, seed, n_labels=9, max_set=14):
    """label sets of 0 .. max_set labels, so that the item size — and with it the fill of the pages — varies from node to node"""
    rng = np.random.default_rng(seed)
    off = np.zeros(ti.n + 1, np.uint32)
    vals, starts = [], {}
    for i in range(ti.n):
        k = int(rng.integers(0, max_set + 1)) if i % 5 else 0
        ls = sorted(set(int(v) for v in rng.integers(-3, n_labels + 40, k)))
        vals.extend(ls)
        off[i + 1] = len(vals)
        for l in ls:
            starts.setdefault(l, i)
    ti.label_off, ti.label_val, ti.label_starts = off, np.array(vals, np.int16), starts
    return ti


@pytest.fixture(scope="module")
def classic(oracle):
    return TestIndex(n=1400, dim_full=96, dim_index=64, bits=2, R=24, distance=oracle.L2, seed=18, kind="gauss", deleted_frac=0.1,
                     L_build=50)


@pytest.fixture(scope="module")
def labeled(oracle):
    ti = TestIndex(n=1300, dim_full=80, dim_index=64, bits=2, R=20, distance=oracle.COSINE, seed=23, kind="gauss", deleted_frac=0.05,
                   L_build=50)
    return _give_labels(ti, seed=5)


def test_classic_index_is_written_as_the_oracle_writes_it(gpu_ctx, classic):
    from pgvectorscale_amd.pages import IndexPages, PagesOut
    ti = classic
    w = _oracle_relation(ti, _meta(ti))
    want = w.rel.tobytes()
    ix = ti.upload(gpu_ctx)
    _assert_same(ix.write_pages(), want)
    out = PagesOut(ix)
    nb = out.n_blocks
    assert nb == len(w.rel.pages) and nb > 20
    # the reader's view of the same relation: what vs_pages_out_open reports
    rd = IndexPages()
    rd.add(want)
    ri = rd.finish()
    for f in ("n_blocks", "n_nodes", "words", "num_neighbors", "has_labels", "n_deleted", "n_label_vals", "new_pages", "meta_magic", "meta_version"):
        assert getattr(out.info, f) == getattr(ri, f), f
    assert list(out.info.pages_by_type) == list(ri.pages_by_type) and ri.n_deleted > 0 and ri.new_pages == 0
    rd.close()
    _assert_same(out.read().tobytes(), want)
    cut = [0, nb // 3, 2 * nb // 3, nb]
    parts = {}
    for i in (2, 1, 0):  # three ranges, last one first
        parts[i] = out.read(cut[i], cut[i + 1] - cut[i]).tobytes()
    _assert_same(parts[0] + parts[1] + parts[2], want)
    for b in reversed(range(nb)):  # single blocks
        assert out.read(b, 1).tobytes() == want[b * PG.BLCKSZ:(b + 1) * PG.BLCKSZ], b
    _assert_same(out.read().tobytes(), want)  # and the same bytes again
    assert [out.item_pointer_of(i) for i in range(ti.n)] == [tuple(p) for p in w.node_ptrs]
    # into device memory
    d = gpu_ctx.alloc(nb * PG.BLCKSZ)
    out.read_dev(d)
    _assert_same(gpu_ctx.download(d, np.empty(nb * PG.BLCKSZ, np.uint8)).tobytes(), want)
    out.read_dev(d, 3, 5)
    _assert_same(gpu_ctx.download(d, np.empty(5 * PG.BLCKSZ, np.uint8)).tobytes(), want[3 * PG.BLCKSZ:8 * PG.BLCKSZ])
    gpu_ctx.free(d)
    out.close()
    ix.close()


@pytest.mark.parametrize("which", ["classic", "labeled"])
def test_many_chunks_through_a_small_staging_ring(classic, labeled, which):
    """a context with 2 x 24 KiB of staging: three pages per chunk, so the double-buffered encode / copy pipeline of
    vs_pages_out_read runs over dozens of chunks, partial last chunk included"""
    import ctypes as C

    import pgvectorscale_amd as P
    from pgvectorscale_amd._lib import check
    from pgvectorscale_amd.pages import PagesOut
    ti = classic if which == "classic" else labeled
    ctx = P.Context.__new__(P.Context)
    ctx._L, ctx.device, ctx.h = P.load(), 0, C.c_void_p()
    check(ctx._L.vs_ctx_create_staging(0, 3 * PG.BLCKSZ, C.byref(ctx.h)))
    try:
        want = _oracle_relation(ti, _meta(ti)).rel.tobytes()
        ix = ti.upload(ctx)
        out = PagesOut(ix)
        assert out.info.pages_by_type[PG.PT_SBQ_NODE] > 3 * 9
        _assert_same(out.read().tobytes(), want)
        _assert_same(out.read(1, out.n_blocks - 2).tobytes(), want[PG.BLCKSZ:-PG.BLCKSZ])
        _assert_same(out.read(9, 17).tobytes(), want[9 * PG.BLCKSZ:26 * PG.BLCKSZ])
        out.close()
        ix.close()
    finally:
        ctx.close()


def test_labeled_index_with_label_sets_of_every_size(gpu_ctx, labeled, tmp_path):
    from pgvectorscale_amd.pages import PagesOut
    ti = labeled
    sizes = np.diff(ti.label_off.astype(np.int64))
    assert sizes.min() == 0 and sizes.max() >= 8
    w = _oracle_relation(ti, _meta(ti))
    want = w.rel.tobytes()
    per_page = np.bincount([b for b, _ in w.node_ptrs])
    assert len(set(per_page[per_page > 0][:-1])) > 1, "the fill must vary from page to page"
    ix = ti.upload(gpu_ctx)
    out = PagesOut(ix)
    assert out.n_blocks == len(w.rel.pages) and out.info.has_labels == 1 and out.info.n_label_vals == len(ti.label_val)
    _assert_same(out.read().tobytes(), want)
    assert [out.item_pointer_of(i) for i in range(ti.n)] == [tuple(p) for p in w.node_ptrs]
    for b0 in (out.n_blocks - 4, 7, 0):
        assert out.read(b0, 4).tobytes() == want[b0 * PG.BLCKSZ:(b0 + 4) * PG.BLCKSZ], b0
    path = tmp_path / "rel"
    out.write_file(str(path), chunk_blocks=7)
    _assert_same(path.read_bytes(), want)
    out.close()
    ix.close()


def test_meta_page_that_outgrows_block_0_chains_behind_the_node_pages(gpu_ctx, labeled):
    ti = labeled
    rng = np.random.default_rng(3)
    starts = {int(l): int(rng.integers(0, ti.n)) for l in range(-450, 450)}  # 900 entries: two leaves and a root, > 8 KB
    ix = ti.upload(gpu_ctx)
    ix.set_start_nodes(ti.start, starts)
    want = _oracle_relation(ti, _meta(ti, label_starts=starts)).rel.tobytes()
    got = ix.write_pages()
    _assert_same(got, want)
    types = _page_types(got)
    assert types[0] == PG.PT_META and types[-1] == PG.PT_META and types[-2] == PG.PT_SBQ_NODE and types.count(PG.PT_META) >= 2
    ix.close()


def test_means_chain_over_several_pages(gpu_ctx, oracle):
    ti = TestIndex(n=260, dim_full=1536, dim_index=1536, bits=1, R=16, distance=oracle.L2, seed=4, kind="gauss", L_build=30)
    want = _oracle_relation(ti, _meta(ti)).rel.tobytes()
    assert _page_types(want)[1:3] == [PG.PT_SBQ_MEANS, PG.PT_SBQ_MEANS]
    ix = ti.upload(gpu_ctx)
    _assert_same(ix.write_pages(), want)
    ix.close()


@pytest.mark.parametrize("which", ["classic", "labeled"])
def test_another_field_order_of_the_archived_node(gpu_ctx, classic, labeled, which):
    ti = classic if which == "classic" else labeled
    layout = (32, 24, 16, 0, 8)  # heap pointer last, neighbors first
    want = _oracle_relation(ti, _meta(ti), layout=layout).rel.tobytes()
    ix = ti.upload(gpu_ctx)
    _assert_same(ix.write_pages(layout=layout), want)
    assert ix.write_pages() != want
    # and a MetaPage in another field order
    order = ("max_alpha", "start_nodes", "quantizer_metadata", "extension_version_when_built", "magic_number", "version",
             "num_dimensions", "num_dimensions_to_index", "num_neighbors", "search_list_size", "distance_type",
             "bq_num_bits_per_dimension", "storage_type", "has_labels")
    ml = PG.meta_layout(order)
    want = _oracle_relation(ti, _meta(ti, layout=ml, extension_version="0.8.1-dev+longer", search_list_size=64, max_alpha=1.5)).rel.tobytes()
    _assert_same(ix.write_pages(meta_layout=ml, extension_version="0.8.1-dev+longer", search_list_size=64, max_alpha=1.5), want)
    ix.close()


@pytest.mark.parametrize("on_device", [False, True])
def test_round_trip_through_the_readers(gpu_ctx, labeled, on_device):
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.pages import DevicePages, IndexPages
    ti = labeled
    src = ti.upload(gpu_ctx)
    raw = src.write_pages()
    if on_device:
        pages = DevicePages(gpu_ctx, len(raw) // PG.BLCKSZ)
        pages.add(raw)
        m, d, starts = pages.meta()
        ix = pages.build_from_meta(vecs=ti.vecs)
    else:
        pages = IndexPages(has_labels=True)
        pages.add(raw)
        m, d, starts = pages.meta()
        ix = pages.upload_from_meta(gpu_ctx, vecs=ti.vecs)
    pages.close()
    assert d.default_start == ti.start == ix.desc.default_start and starts == ti.label_starts
    assert ix.desc.n_label_starts == len(ti.label_starts)
    assert (m["search_list_size"], m["max_alpha"], m["extension_version_when_built"], m["storage_type"]) == (100, 1.2, "0.8.0", 2)
    dev = ix.download()
    assert (dev["codes"] == ti.codes).all() and (dev["nbrs"] == ti.nbrs).all() and (dev["heap_tids"] == ti.tids).all()
    lo = gpu_ctx.download(ix.array(_lib.ARR_LABEL_OFF)[0], np.empty(ti.n + 1, np.uint32))
    lv = gpu_ctx.download(ix.array(_lib.ARR_LABEL_VAL)[0], np.empty(len(ti.label_val), np.int16))
    assert (lo == ti.label_off).all() and (lv == ti.label_val).all()
    mean, m2, cnt = ix.get_quantizer()
    assert (mean == ti.mean).all() and (m2 == ti.m2).all() and cnt == ti.count
    q = ti.queries(32, seed=8, kind="gauss")
    rng = np.random.default_rng(4)
    keys = [sorted(set(int(x) for x in rng.integers(0, 12, int(rng.integers(1, 3))))) for _ in range(32)]
    oracle_ix = type(ti.oracle)(codes=ti.codes, nbrs=ti.nbrs, heap_tids=ti.tids, vecs=ti.vecs, mean=ti.mean, m2=ti.m2, count=ti.count,
                                bits=ti.bits, dim_index=ti.dim_index, num_neighbors=ti.R, distance_type=ti.distance,
                                default_start=ti.start, label_off=ti.label_off, label_val=ti.label_val, label_starts=ti.label_starts)
    for kk in (None, keys):
        gi, gt, gd, gst = ix.search_batch(q, search_list_size=40, rescore=20, k=10, qlabels=kk)
        si, st, sd, sst = src.search_batch(q, search_list_size=40, rescore=20, k=10, qlabels=kk)
        oi, od, ost = oracle_ix.search_batch(q, L=40, rescore=20, k=10, qlabels=kk)
        assert (gi == si).all() and (gt == st).all() and gd.view(np.uint32).tobytes() == sd.view(np.uint32).tobytes()
        assert (gi == oi).all() and gst["visited_nodes"] == sst["visited_nodes"] == ost["visited_nodes"]
    ix.close()
    src.close()


def test_device_built_index_goes_out_as_pages(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    from pgvectorscale_amd.datagen import DatagenParams, fill_device
    from pgvectorscale_amd.pages import IndexPages
    n, dim, R = 3000, 96, 24
    ix = P.DiskAnnIndex.alloc(gpu_ctx, n=n, dim_full=dim, num_neighbors=R, distance_type=P.VS_L2)
    vp, stride = ix.array(P._lib.ARR_VECS)
    assert stride == dim
    fill_device(gpu_ctx, DatagenParams(seed=21, dim=dim, latent_dim=16, n_clusters=32), 0, n, vp)
    ix.sbq_train()
    ix.sbq_quantize_corpus()
    ix.build_graph(search_list_size=48, max_alpha=1.2)
    ix.mark_deleted(np.arange(5, n, 97, dtype=np.uint32))
    host = ix.download()
    mean, m2, cnt = ix.get_quantizer()
    d = ix.desc
    raw = ix.write_pages(extension_version="0.8.0", search_list_size=48, max_alpha=1.2)
    want = PG.write_index(codes=host["codes"], nbrs=host["nbrs"], heap_tids=host["heap_tids"], mean=mean, m2=m2, count=cnt, means_first=True,
                          meta=dict(num_dimensions=dim, num_dimensions_to_index=d.dim_index, bq_num_bits_per_dimension=d.bits,
                                    distance_type=d.distance_type, num_neighbors=R, default_start=int(d.default_start),
                                    extension_version="0.8.0", search_list_size=48, max_alpha=1.2)).rel.tobytes()
    _assert_same(raw, want)
    rd = IndexPages()
    rd.add(raw)
    info = rd.finish()
    arr = rd.arrays()
    assert info.n_nodes == n and info.n_deleted == len(range(5, n, 97))
    assert (arr["codes"] == host["codes"]).all() and (arr["nbrs"] == host["nbrs"]).all() and (arr["heap_tids"] == host["heap_tids"]).all()
    m, dd, _ = rd.meta()
    assert dd.default_start == d.default_start and (dd.dim_full, dd.dim_index, dd.bits, dd.words, dd.num_neighbors) == (dim, d.dim_index, d.bits, d.words, R)
    c2, mean2, m22 = rd.sbq_means(m["quantizer_block"], m["quantizer_offset"])
    assert c2 == cnt and (mean2 == mean).all() and (m22 == m2).all()
    rd.close()
    ix.close()


def test_what_the_writer_refuses(gpu_ctx, classic):
    import pgvectorscale_amd as P
    from pgvectorscale_amd.pages import PagesOut
    ti = classic
    plain = P.DiskAnnIndex.upload(gpu_ctx, codes=None, nbrs=ti.nbrs, heap_tids=ti.tids, vecs=ti.vecs, mean=None, m2=None, count=0, bits=1,
                                  dim_index=ti.dim_full, num_neighbors=ti.R, distance_type=ti.distance, default_start=ti.start,
                                  storage_type=P._lib.VS_STORAGE_PLAIN)
    with pytest.raises(P.VsError, match="SBQ"):
        PagesOut(plain)
    with pytest.raises(P.VsError):
        plain.write_pages()
    plain.close()
    ix = ti.upload(gpu_ctx)
    with pytest.raises(P.VsError, match="page_size"):
        PagesOut(ix, page_size=4096)
    out = PagesOut(ix)
    want = _oracle_relation(ti, _meta(ti)).rel.tobytes()
    buf = np.full((out.n_blocks + 2) * PG.BLCKSZ, 0xCD, np.uint8)
    for first, cnt in ((0, out.n_blocks + 1), (out.n_blocks, 1), (out.n_blocks - 1, 2), (0xFFFFFFFF, 2)):
        with pytest.raises(P.VsError, match="blocks"):
            out.read(first, cnt, out=buf)
    assert (buf == 0xCD).all()
    with pytest.raises(P.VsError):
        out.item_pointer_of(ti.n)
    # the handle is still good
    _assert_same(out.read(out.n_blocks - 3, 3).tobytes(), want[-3 * PG.BLCKSZ:])
    assert out.read(out.n_blocks, 0).size == 0
    _assert_same(out.read(out=buf)[:out.n_blocks * PG.BLCKSZ].tobytes(), want)
    out.close()
    ix.close()
