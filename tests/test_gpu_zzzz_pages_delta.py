"""vs_pages_out_baseline / _delta / _read_blocks: only the blocks an insert or a vacuum changed are written back.  The reference for
every expectation is the oracle's writer (oracle/pages_py.py::write_index, means_first=True) fed the arrays downloaded from the
device BEFORE and AFTER the mutation: want_before, want_after, and the expected dirty set
{b : b >= blocks(before) or want_after[b] != want_before[b]}.  Every case asserts (i) the delta's list is that set, ascending,
(ii) read_blocks(list) is those blocks of want_after, (iii) want_before patched with them and cut to n_blocks_now is want_after,
(iv) a second delta against the new baseline is empty — and its own precondition.  Also runs on the lockstep interpreter
(tests/test_pages_delta_host.py)."""
import ctypes as C

import numpy as np
import pytest

from helpers import TestIndex, make_vectors
from oracle import pages_py as PG

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

B = PG.BLCKSZ
INV = 0xFFFFFFFF


def _give_labels(ti, seed, n_labels=9, max_set=14):
    """label sets of 0 .. max_set labels: the item size, and with it the fill of the pages, varies from node to node"""
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


def _relation(ctx, ix, starts):
    """the oracle's writer over the arrays as they are on the device now"""
    from pgvectorscale_amd import _lib
    host = ix.download()
    mean, m2, cnt = ix.get_quantizer()
    d = ix.desc
    lo = lv = None
    if d.has_labels:
        lo = ctx.download(ix.array(_lib.ARR_LABEL_OFF)[0], np.empty(d.n + 1, np.uint32))
        lv = ctx.download(ix.array(_lib.ARR_LABEL_VAL)[0], np.empty(max(int(lo[-1]), 1), np.int16))[:int(lo[-1])]
    meta = dict(num_dimensions=d.dim_full, num_dimensions_to_index=d.dim_index, bq_num_bits_per_dimension=d.bits,
                distance_type=d.distance_type, num_neighbors=d.num_neighbors, default_start=int(d.default_start),
                labeled_starts=dict(starts), extension_version="0.8.0", search_list_size=100, max_alpha=1.2)
    w = PG.write_index(codes=host["codes"], nbrs=host["nbrs"], heap_tids=host["heap_tids"], mean=mean, m2=m2, count=cnt, label_off=lo,
                       label_val=lv, means_first=True, meta=meta)
    return w.rel.tobytes(), host


def _blk(raw, b):
    return raw[b * B:(b + 1) * B]


def _page_types(raw):
    return [raw[b * B + B - 8] for b in range(len(raw) // B)]


def _expected(before, after):
    nb_b, nb_a = len(before) // B, len(after) // B
    return [b for b in range(nb_a) if b >= nb_b or _blk(after, b) != _blk(before, b)]


def _check(out, base, before, after):
    """(i) .. (iv) of the module docstring on writer `out`; -> (the dirty blocks, the new baseline)"""
    blocks, nb_now, new_base = out.delta(base)
    want = _expected(before, after)
    assert blocks.dtype == np.uint32 and blocks.tolist() == want                                  # (i)
    assert (np.diff(blocks.astype(np.int64)) > 0).all() and nb_now == len(after) // B == out.n_blocks
    got = out.read_blocks(blocks).tobytes()
    for i, b in enumerate(want):                                                                  # (ii)
        assert _blk(got, i) == _blk(after, b), b
    patched = bytearray(before[:nb_now * B]) + bytes(max(nb_now * B - len(before), 0))
    for i, b in enumerate(want):
        patched[b * B:(b + 1) * B] = _blk(got, i)
    assert bytes(patched) == after                                                                # (iii)
    again, nb2, third = out.delta(new_base)
    assert again.size == 0 and nb2 == nb_now and new_base.n_blocks == third.n_blocks == nb_now    # (iv)
    third.close()
    return want, new_base


class Staged:
    """a fresh upload of `ti` with its baseline taken and the writer closed again: ready to be mutated"""

    def __init__(self, ctx, ti, before, starts=None):
        from pgvectorscale_amd.pages import PagesOut
        self.ctx, self.ti = ctx, ti
        self.starts = dict(ti.label_starts if starts is None else starts)
        self.ix = ti.upload(ctx)
        if starts is not None:
            self.ix.set_start_nodes(ti.start, starts)
        out = PagesOut(self.ix)
        self.base = out.baseline()
        self.ptr = [out.item_pointer_of(i) for i in range(ti.n)]
        self.n_blocks = out.n_blocks
        self.means_block = next(b for b, t in enumerate(_page_types(before)) if t == PG.PT_SBQ_MEANS)
        assert self.base.n_blocks == out.n_blocks == len(before) // B
        out.close()
        self.before = before

    def check(self):
        from pgvectorscale_amd.pages import PagesOut
        after, host = _relation(self.ctx, self.ix, self.starts)
        out = PagesOut(self.ix)
        try:
            want, nb = _check(out, self.base, self.before, after)
            nb.close()
        finally:
            out.close()
        return want, after, host

    def close(self):
        self.base.close()
        self.ix.close()


@pytest.fixture(scope="module")
def classic(oracle):
    return TestIndex(n=1400, dim_full=96, dim_index=64, bits=2, R=24, distance=oracle.L2, seed=18, kind="gauss", deleted_frac=0.1, L_build=50)


@pytest.fixture(scope="module")
def labeled(oracle):
    ti = TestIndex(n=1300, dim_full=80, dim_index=64, bits=2, R=20, distance=oracle.COSINE, seed=23, kind="gauss", deleted_frac=0.05, L_build=50)
    return _give_labels(ti, seed=5)


def _before_of(ctx, ti, starts=None):
    ix = ti.upload(ctx)
    if starts is not None:
        ix.set_start_nodes(ti.start, starts)
    raw, _ = _relation(ctx, ix, ti.label_starts if starts is None else starts)
    got = ix.write_pages()
    ix.close()
    assert got == raw  # (the relation a fresh upload writes is the oracle's: what every baseline below records)
    return raw


@pytest.fixture(scope="module")
def classic_before(gpu_ctx, classic):
    return _before_of(gpu_ctx, classic)


@pytest.fixture(scope="module")
def labeled_before(gpu_ctx, labeled):
    return _before_of(gpu_ctx, labeled)


def _tids(first, n):
    return ((np.arange(first, first + n, dtype=np.uint64) + 5000) << np.uint64(16)) | np.uint64(3)


# ---- no change ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["classic", "labeled"])
def test_no_change_no_dirty_block(gpu_ctx, classic, labeled, classic_before, labeled_before, which):
    s = Staged(gpu_ctx, classic if which == "classic" else labeled, classic_before if which == "classic" else labeled_before)
    want, after, _ = s.check()
    assert want == [] and after == s.before
    s.close()


def test_reserve_between_baseline_and_delta_changes_nothing(gpu_ctx, classic, classic_before):
    """the arrays move; the baseline does not depend on where they live"""
    from pgvectorscale_amd import _lib
    s = Staged(gpu_ctx, classic, classic_before)
    was = s.ix.array(_lib.ARR_CODES)[0].value
    s.ix.reserve(3000)
    assert s.ix.capacity == 3000 and s.ix.array(_lib.ARR_CODES)[0].value != was
    want, after, _ = s.check()
    assert want == [] and after == s.before
    s.close()


# ---- single-field changes: exactly the block item_pointer_of(node) names --------------------------------------------------------------
def _live(ti, nodes):
    return [i for i in nodes if ti.tids[i] & np.uint64(0xFFFF)]


def _poke(ctx, ix, which, node, col, value, dtype):
    """one element of a device array through vs_index_array + vs_dev_upload"""
    ptr, stride = ix.array(which)
    ctx.upload(C.c_void_p(ptr.value + (node * stride + col) * np.dtype(dtype).itemsize), np.array([value], dtype))


@pytest.mark.parametrize("case", ["delete_first_page", "delete_last_page", "delete_middle", "code_bit", "neighbor_replaced", "list_shortened"])
def test_one_field_of_one_node_dirties_exactly_its_block(gpu_ctx, classic, classic_before, case):
    from pgvectorscale_amd import _lib
    ti = classic
    s = Staged(gpu_ctx, ti, classic_before)
    first_blk, last_blk = s.ptr[0][0], s.ptr[ti.n - 1][0]
    if case == "delete_first_page":
        node = _live(ti, range(0, 20))[3]
        assert s.ptr[node][0] == first_blk
    elif case == "delete_last_page":
        node = _live(ti, range(ti.n - 1, 0, -1))[0]
        assert s.ptr[node][0] == last_blk and s.ptr[ti.n - 1][1] < max(p[1] for p in s.ptr), "the last node page must be partly filled"
    else:
        node = _live(ti, range(ti.n // 2, ti.n))[0]
        assert first_blk < s.ptr[node][0] < last_blk
    if case.startswith("delete"):
        s.ix.mark_deleted(np.array([node], np.uint32))
    elif case == "code_bit":
        _poke(gpu_ctx, s.ix, _lib.ARR_CODES, node, 1, ti.codes[node, 1] ^ np.uint64(1 << 17), np.uint64)
    elif case == "neighbor_replaced":
        other = next(u for u in range(ti.n) if u != node and u not in ti.nbrs[node])
        _poke(gpu_ctx, s.ix, _lib.ARR_NBRS, node, 2, other, np.uint32)
    else:
        assert (ti.nbrs[node] != INV).sum() >= 4
        _poke(gpu_ctx, s.ix, _lib.ARR_NBRS, node, 2, INV, np.uint32)
    want, _, _ = s.check()
    assert want == [s.ptr[node][0]]
    s.close()


def test_three_nodes_on_three_pages_give_three_blocks(gpu_ctx, classic, classic_before):
    ti = classic
    s = Staged(gpu_ctx, ti, classic_before)
    nodes = [_live(ti, range(a, ti.n))[0] for a in (40, 700, 1390)]
    s.ix.mark_deleted(np.array(nodes, np.uint32))
    want, _, _ = s.check()
    assert want == sorted(s.ptr[i][0] for i in nodes) and len(set(want)) == 3
    s.close()


# ---- bulk_delete ----------------------------------------------------------------------------------------------------------------------
def test_bulk_delete_dirties_the_pages_of_its_hits(gpu_ctx, classic, classic_before):
    ti = classic
    s = Staged(gpu_ctx, ti, classic_before)
    rng = np.random.default_rng(31)
    nodes = rng.choice(_live(ti, range(ti.n // 3)), 60, replace=False)  # (a third of the index: fewer than half of the blocks)
    dead = np.concatenate([ti.tids[nodes], _tids(10 ** 6, 20)])
    rng.shuffle(dead)
    st = s.ix.bulk_delete(dead)
    assert st["tuples_removed"] == 60
    want, _, _ = s.check()
    assert want == sorted(set(s.ptr[i][0] for i in nodes)) and 1 < len(want) < s.n_blocks // 2
    s.close()


# ---- insert ---------------------------------------------------------------------------------------------------------------------------
def _insert_case(gpu_ctx, ti, before, new_sets, starts=None):
    n0, n1 = ti.n, 100
    s = Staged(gpu_ctx, ti, before, starts=starts)
    new = make_vectors(n1, ti.dim_full, 91, "gauss")
    st = s.ix.insert(new, _tids(n0, n1), labels=new_sets, search_list_size=50)
    assert st["inserted"] == n1 and s.ix.desc.n == n0 + n1
    for i, ls in enumerate(new_sets or []):  # (update_start_nodes: a label first carried by an inserted node gets it as its start node)
        for l in ls:
            s.starts.setdefault(int(l), n0 + i)
    want, after, host = s.check()
    nb_before, nb_after = s.n_blocks, len(after) // B
    assert want and nb_after > nb_before
    assert s.ptr[n0 - 1][0] in want, "the new items continue on the old last node page"
    assert set(range(nb_before, nb_after)) <= set(want)
    old_rows = host["nbrs"][:n0]
    named = np.flatnonzero(((old_rows >= n0) & (old_rows != INV)).any(1))
    assert named.size and set(s.ptr[u][0] for u in named) <= set(want), "old nodes whose lists now name a new node"
    return s, want, after


def test_insert_into_a_classic_index(gpu_ctx, classic, classic_before):
    s, want, after = _insert_case(gpu_ctx, classic, classic_before, None)
    assert 0 not in want  # (the MetaPage of a classic index does not change: same start node, same geometry)
    s.close()


def _new_label_sets(n1, fresh=None):
    rng = np.random.default_rng(77)
    sets = [sorted(set(int(v) for v in rng.integers(0, 9, int(rng.integers(1, 4))))) for _ in range(n1)]
    if fresh is not None:
        sets[7] = sorted(set(sets[7] + [fresh]))
    return sets


def test_insert_into_a_labeled_index_with_a_label_nobody_carried(gpu_ctx, labeled, labeled_before):
    assert 300 not in labeled.label_starts
    s, want, after = _insert_case(gpu_ctx, labeled, labeled_before, _new_label_sets(100, fresh=300))
    assert s.starts[300] == labeled.n + 7 and 0 in want, "the MetaPage's start-node B-tree gained an entry"
    s.close()


@pytest.mark.parametrize("n_starts", [600, 900])
def test_meta_chain_behind_the_node_pages_moves_with_an_insert(gpu_ctx, labeled, n_starts):
    """hundreds of labeled start nodes (vs_index_set_start_nodes).  600 of them make the B-tree's root an inner node but still fit
    block 0 at this geometry (the archive is about 6 KB); 900 are more than 8 KB, so the Meta chain continues after the last node
    page: the insert grows the node pages into the blocks the overflow pages held, and the blocks that change kind must be in
    the set by the byte rule"""
    ti = labeled
    rng = np.random.default_rng(3)
    starts = {int(l): int(rng.integers(0, ti.n)) for l in range(-n_starts // 2, n_starts // 2)}
    before = _before_of(gpu_ctx, ti, starts)
    tb = _page_types(before)
    overflows = n_starts == 900
    assert tb[0] == PG.PT_META and (tb[-1] == PG.PT_META and tb[-2] == PG.PT_SBQ_NODE) == overflows
    s, want, after = _insert_case(gpu_ctx, ti, before, _new_label_sets(100), starts=starts)
    ta = _page_types(after)
    changed_kind = [b for b in range(len(tb)) if ta[b] != tb[b]]
    assert set(changed_kind) <= set(want)
    if overflows:
        assert changed_kind and ta[-1] == PG.PT_META and tb.count(PG.PT_META) == ta.count(PG.PT_META) >= 2
    s.close()


# ---- the gathered reader --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(oracle):
    """77 node pages: room for 38 dirty blocks no two of which are adjacent"""
    return TestIndex(n=2600, dim_full=96, dim_index=64, bits=2, R=24, distance=oracle.L2, seed=19, kind="gauss", L_build=40)


def test_dirty_list_through_a_small_staging_ring(wide):
    """a context with 2 x 24 KiB of staging: three pages per chunk, so 38 non-adjacent dirty blocks run over 13 chunks of the
    double-buffered encode / copy pipeline, the partial last one included; the host and the device form"""
    import pgvectorscale_amd as P
    from pgvectorscale_amd._lib import check
    from pgvectorscale_amd.pages import PagesOut
    ti = wide
    ctx = P.Context.__new__(P.Context)
    ctx._L, ctx.device, ctx.h = P.load(), 0, C.c_void_p()
    check(ctx._L.vs_ctx_create_staging(0, 3 * B, C.byref(ctx.h)))
    try:
        before = _before_of(ctx, ti)
        s = Staged(ctx, ti, before)
        pages = sorted(set(p[0] for p in s.ptr))
        assert len(pages) >= 76
        nodes = [next(i for i in range(ti.n) if s.ptr[i][0] == pages[2 * k]) for k in range(38)]
        s.ix.mark_deleted(np.array(nodes, np.uint32))
        want, after, _ = s.check()
        assert want == [pages[2 * k] for k in range(38)] and (np.diff(want) >= 2).all() and len(want) >= 30
        assert -(-len(want) // 3) > 12 and len(want) % 3 != 0
        out = PagesOut(s.ix)
        d = ctx.alloc(len(want) * B)
        out.read_blocks_dev(d, want)
        got = ctx.download(d, np.empty(len(want) * B, np.uint8)).tobytes()
        ctx.free(d)
        assert got == b"".join(_blk(after, b) for b in want) == out.read_blocks(want).tobytes()
        out.close()
        s.close()
    finally:
        ctx.close()


def test_read_blocks_any_list_any_order(gpu_ctx, classic, classic_before):
    import pgvectorscale_amd as P
    from pgvectorscale_amd.pages import PagesOut
    s = Staged(gpu_ctx, classic, classic_before)
    out = PagesOut(s.ix)
    nb = out.n_blocks
    blocks = [nb - 1, 0, 7, s.means_block, 7, 7, 3, 0, nb - 2, s.means_block, 8, 9, 2]
    want = b"".join(_blk(s.before, b) for b in blocks)
    assert out.read_blocks(blocks).tobytes() == want
    d = gpu_ctx.alloc(len(blocks) * B)
    out.read_blocks_dev(d, blocks)
    assert gpu_ctx.download(d, np.empty(len(blocks) * B, np.uint8)).tobytes() == want
    gpu_ctx.free(d)
    assert out.read_blocks([]).size == 0
    # a list that names n_blocks fails and writes nothing
    buf = np.full(4 * B, 0xAB, np.uint8)
    with pytest.raises(P.VsError) as e:
        out.read_blocks([1, 5, nb, 2], out=buf)
    assert e.value.code == -1 and (buf == 0xAB).all()
    assert out.read_blocks([5], out=buf)[:B].tobytes() == _blk(s.before, 5)  # (the handle is still good)
    out.close()
    s.close()


# ---- patch_file -----------------------------------------------------------------------------------------------------------------------
def test_patch_file_brings_the_relation_file_up_to_date(gpu_ctx, classic, classic_before, tmp_path):
    from pgvectorscale_amd.pages import IndexPages, PagesOut
    ti = classic
    ix = ti.upload(gpu_ctx)
    path = tmp_path / "rel"
    out = PagesOut(ix)
    out.write_file(str(path), chunk_blocks=7)
    base = out.baseline()
    out.close()
    assert path.read_bytes() == classic_before
    ix.bulk_delete(ti.tids[_live(ti, range(100, 130))])
    ix.insert(make_vectors(100, ti.dim_full, 92, "gauss"), _tids(ti.n, 100), search_list_size=50)
    after, host = _relation(gpu_ctx, ix, {})
    out = PagesOut(ix)
    new_base = out.patch_file(str(path), base, chunk_blocks=5)
    assert path.read_bytes() == after and len(after) > len(classic_before)
    assert out.delta(new_base)[0].size == 0
    out.close()
    rd = IndexPages()
    rd.add(path.read_bytes())
    rd.finish()
    arr = rd.arrays()
    assert (arr["codes"] == host["codes"]).all() and (arr["nbrs"] == host["nbrs"]).all() and (arr["heap_tids"] == host["heap_tids"]).all()
    rd.close()
    # and back: a relation that got shorter is truncated
    ix2 = ti.upload(gpu_ctx)
    out = PagesOut(ix2)
    third = out.patch_file(str(path), new_base)
    assert path.read_bytes() == classic_before and third.n_blocks == len(classic_before) // B
    out.close()
    for b in (base, new_base, third):
        b.close()
    ix2.close()
    ix.close()
