"""vs_heap_dev_*: the heap's vector column decoded on the device from heap and TOAST pages (k_heap_dev_heap, k_heap_dev_toast,
k_heap_dev_finish), vs_index_alloc_vecs and vs_pages_follow_apply_dev.  Tables are manufactured with oracle/heap_py.py
(tests/heap_dev_checks.py); every expectation comes from the source vectors, the pure-Python reader (HP.read_vector_column) and the
host reader (HeapColumn) over the same pages, and every comparison is exact: bytes, no tolerance, no row left out.  The target rows
are pre-filled with a sentinel and stand between guard rows, so a write to a padding float or outside [0, n) shows.  The malformed
pages of this file are in-range fabricated bytes that must end in an error code.  Also runs on the lockstep interpreter
(tests/test_emu_heap_dev.py)."""
import struct

import numpy as np
import pytest

import heap_dev_checks as HC
from heap_dev_checks import ATTRS, INVALID, STATE, VEC_ATT
from oracle import heap_py as HP

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

# dim -> (table, rows, out_stride - dim): what each shape exercises is in the table of the docstring of test_round_trip
SHAPES = {2: ("one", 400, 3), 3: ("six", 400, 0), 30: ("six", 400, 3), 31: ("six", 400, 0), 128: ("six", 400, 3), 499: ("six", 400, 0),
          529: ("six", 400, 3), 530: ("six", 400, 0), 768: ("six", 400, 3), 1536: ("six", 400, 0), 4000: ("six", 120, 3)}
_shapes = {}


def shape(dim):
    """the table of a shape with its references, made once and never changed"""
    if dim not in _shapes:
        kind, n, pad = SHAPES[dim]
        if kind == "one":
            t, tids, expect = HC.make_one_column_table(n, dim, seed=dim)
            attrs, att = HC.ONE_COL, 1
        else:
            t, tids, expect = HC.make_table(n, dim, seed=dim)
            attrs, att = ATTRS, VEC_ATT
        tids, tids_idx, expect, dele = HC.index_order(tids, expect)
        ref = HP.read_vector_column(t, tids, att - 1, dim)
        for i in range(n):
            assert (ref[i] is None) == (expect[i] is None) and (ref[i] is None or ref[i].tobytes() == expect[i].tobytes())
        expect = [None if dele[i] else e for i, e in enumerate(expect)]
        host = HC.read_host(t, tids_idx, dim, attrs, att)
        _shapes[dim] = (t, tids_idx, expect, dele, attrs, att, dim + pad, host)
    return _shapes[dim]


# ---- 1. round trip per storage form -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feed", [None, 1, 3], ids=["at_once", "1_block", "3_blocks"])
@pytest.mark.parametrize("dim", list(SHAPES), ids=[("ext%d" if d >= 499 else "inl%d") % d for d in SHAPES])
def test_round_trip(gpu_ctx, dim, feed):
    """2: 185 items on a page, more wanted tuples than lanes | 3, 30: 1-byte header, unaligned body | 31, 128: 4-byte header in line |
    499: external, last chunk 4 bytes under a 1-byte header | 529: last chunk 124 bytes, 1-byte header | 530: last chunk 128 bytes, 4-byte
    header | 768: two chunks | 1536: four | 4000: nine, the last 36 bytes under a 1-byte header.  NULLs, rows older than the column,
    shuffled index order, 5 % deleted tids; out_stride = dim + 3 on half the shapes."""
    t, tids, expect, dele, attrs, att, stride, (hvecs, hinfo, hfound) = shape(dim)
    rows, info, found, ncomp = HC.read_dev(gpu_ctx, t, tids, dim, HC.ranges(len(t.heap.pages), feed), HC.ranges(len(t.toast.pages), feed),
                                           stride=stride, attrs=attrs, vec_att=att)
    HC.check_rows(rows, dim, expect, found)
    assert rows[:, :dim].tobytes() == hvecs.tobytes()
    assert (found == hfound).all() and info == hinfo and ncomp == 0
    assert info["n_deleted"] == int(dele.sum()) and info["n_inline"] + info["n_external"] == int(found.sum())
    assert (info["n_external"] > 0) == (dim >= 499) and (info["n_inline"] > 0) == (dim < 499)
    if dim >= 499:
        assert info["n_chunks"] == info["n_external"] * -(-(4 + 4 * dim) // HP.toast_max_chunk_size())
    if dim == 2:
        assert max(t.heap.max_offset(b) for b in range(len(t.heap.pages))) >= 185  # (185 rows with a vector fill a page; a NULL row is shorter)


def test_chunk_header_forms():
    """the last chunks of the external shapes are what the table above says (a fact about the fabricated pages, no device involved)"""
    want = {499: (4, 1), 529: (124, 1), 530: (128, 4), 4000: (36, 1)}
    for dim, (size, hdr) in want.items():
        t = shape(dim)[0]
        last = max(HC.chunk_fields(it)[1] for _, _, it in HC.toast_items(t.toast))
        for _, _, it in HC.toast_items(t.toast):
            _, seq, _, (s, l) = HC.chunk_fields(it)
            if seq == last:
                assert (l - 1, 1) == (size, hdr) if it[s] & 1 else (l - 4, 4) == (size, hdr)


# ---- 2. line pointers and gaps ----------------------------------------------------------------------------------------------------------
def test_redirects_dead_pointers_and_missing_blocks(gpu_ctx):
    dim = 16
    t, tids, expect = HC.make_table(60, dim, seed=7, null_frac=0.0)
    expect = list(expect)
    heap = t.heap
    live = [i for i in range(60) if expect[i] is not None]
    # a pruned HOT chain: the root line pointer of a row redirects to a later version of the row on the same page (same vector)
    last = len(heap.pages) - 1
    ra = next(i for i in live if (int(tids[i]) >> 16) == last)
    vals = [struct.pack("<q", 5), None, None, None, ("inline", HP.vector_datum_body(expect[ra])), struct.pack("<i", 5)]
    nb, no = heap.add_item(HP.form_tuple(ATTRS, vals))
    assert nb == last
    heap.set_line_pointer(last, int(tids[ra]) & 0xFFFF, HP.LP_REDIRECT, lp_off=no)
    # two rows vacuumed away under the index's feet
    dead = [i for i in live if i != ra][:2]
    for i, fl in zip(dead, (HP.LP_DEAD, HP.LP_UNUSED)):
        heap.set_line_pointer(int(tids[i]) >> 16, int(tids[i]) & 0xFFFF, fl)
        expect[i] = None
    tids = np.append(tids, np.uint64((9999 << 16) | 1))  # a TID beyond the relation
    expect.append(None)
    rows, info, found, ncomp = HC.read_dev(gpu_ctx, t, tids, dim)
    HC.check_rows(rows, dim, expect, found)
    hvecs, hinfo, hfound = HC.read_host(t, tids, dim)
    assert found[ra] and info == hinfo and (found == hfound).all() and rows.tobytes() == hvecs.tobytes() and ncomp == 0
    assert info["n_dead_line_pointer"] == len(dead) == 2 and info["n_not_found"] == 1


def test_heap_feed_with_a_gap(gpu_ctx):
    dim = 128
    t, tids, expect, dele, attrs, att, _, _ = shape(dim)
    nb, skip = len(t.heap.pages), 2
    assert nb > 4
    on_gap = ((tids >> np.uint64(16)) == skip) & ~dele
    assert on_gap.any()
    exp = [None if on_gap[i] else e for i, e in enumerate(expect)]
    rows, info, found, ncomp = HC.read_dev(gpu_ctx, t, tids, dim, heap_ranges=[(0, skip), (skip + 1, nb - skip - 1)])
    HC.check_rows(rows, dim, exp, found)
    assert info["n_not_found"] == int(on_gap.sum()) and info["heap_blocks"] == nb and info["n_toast_incomplete"] == 0 and ncomp == 0
    assert sum(info[k] for k in ("n_inline", "n_external", "n_deleted", "n_null", "n_dead_line_pointer", "n_not_found", "n_toast_incomplete")) == len(tids)


def test_toast_feed_with_a_gap(gpu_ctx):
    dim = 768
    t, tids, expect, dele, attrs, att, _, _ = shape(dim)
    nb, skip = len(t.toast.pages), 3
    vids = HC.external_value_ids(t, tids)
    lost = {HC.chunk_fields(it)[0] for blk, _, it in HC.toast_items(t.toast) if blk == skip}
    hit = np.array([v is not None and v in lost and expect[i] is not None for i, v in enumerate(vids)])
    assert hit.any() and not hit.all()
    exp = [None if hit[i] else e for i, e in enumerate(expect)]
    rows, info, found, ncomp = HC.read_dev(gpu_ctx, t, tids, dim, toast_ranges=[(0, skip), (skip + 1, nb - skip - 1)])
    HC.check_rows(rows, dim, exp, found)
    assert info["n_toast_incomplete"] == int(hit.sum()) and info["toast_blocks"] == nb and info["n_not_found"] == 0 and ncomp == 0
    assert not found[hit].any() and not rows[hit].any()


def test_descending_ranges_are_refused(gpu_ctx):
    from pgvectorscale_amd import VsError
    dim = 768
    t = shape(dim)[0]
    for kw in (dict(heap_ranges=[(2, 2), (3, 1)]), dict(toast_ranges=[(0, 4), (2, 1)])):
        with pytest.raises(VsError, match="below the end of the previous range") as e:
            HC.read_dev(gpu_ctx, t, shape(dim)[1], dim, **kw)
        assert e.value.code == INVALID


# ---- 3. TOAST order -------------------------------------------------------------------------------------------------------------------------
def test_toast_rows_in_shuffled_order(gpu_ctx):
    dim = 1536
    t, tids, expect, dele, attrs, att, stride, (hvecs, hinfo, hfound) = shape(dim)
    items = HC.toast_items(t.toast)
    t2 = HP.Table(ATTRS)
    t2.heap = t.heap
    for k in np.random.default_rng(5).permutation(len(items)):
        t2.toast.add_item(items[k][2])
    rows, info, found, ncomp = HC.read_dev(gpu_ctx, t2, tids, dim, toast_ranges=HC.ranges(len(t2.toast.pages), 5))
    HC.check_rows(rows, dim, expect, found)
    assert rows.tobytes() == hvecs.tobytes() and (found == hfound).all() and info["n_chunks"] == hinfo["n_chunks"] and ncomp == 0


# ---- 4. page size ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [768, 1536])
def test_16k_pages(gpu_ctx, dim):
    """TOAST_MAX_CHUNK_SIZE is 4 044 on 16 KB pages: 768 dimensions are one chunk, 1 536 two"""
    assert HP.toast_max_chunk_size(16384) == 4044
    t, tids, expect = HC.make_table(100, dim, seed=16 + dim, page_size=16384)
    tids, tids_idx, expect, dele = HC.index_order(tids, expect)
    expect = [None if dele[i] else e for i, e in enumerate(expect)]
    rows, info, found, ncomp = HC.read_dev(gpu_ctx, t, tids_idx, dim, HC.ranges(len(t.heap.pages), 2), HC.ranges(len(t.toast.pages), 3), stride=dim + 1)
    HC.check_rows(rows, dim, expect, found)
    hvecs, hinfo, hfound = HC.read_host(t, tids_idx, dim)
    assert info == hinfo and (found == hfound).all() and rows[:, :dim].tobytes() == hvecs.tobytes() and ncomp == 0
    assert info["n_chunks"] == info["n_external"] * (1 if dim == 768 else 2) > 0


# ---- 5. compressed vectors ----------------------------------------------------------------------------------------------------------------
def test_compressed_vectors_are_left_to_the_host_reader(gpu_ctx):
    dim = 600
    rng = np.random.default_rng(21)
    v = np.zeros(dim, np.float32)
    v[::7] = 1.5  # compressible
    body = HP.vector_datum_body(v)
    comp = HC.pglz_compress(body)
    t = HP.Table(ATTRS)
    vecs = rng.standard_normal((20, dim)).astype(np.float32)
    row = lambda i, vec: [struct.pack("<q", i), None, None, None, vec, struct.pack("<i", i)]
    tids = [t.insert(row(i, ("inline", HP.vector_datum_body(vecs[i])))) for i in range(10)]
    inline_c = ("raw", struct.pack("<II", ((len(comp) + 8) << 2) | 2, len(body)) + comp)  # 4-byte header (compressed), tcinfo, data
    tid_a = t.insert(row(100, inline_c))
    stored = struct.pack("<I", len(body)) + comp  # external + compressed: the TOAST relation holds tcinfo + data
    vid = t.next_value
    t.next_value += 1
    for seq, at in enumerate(range(0, len(stored), t.chunk)):
        t.toast.add_item(HP.form_tuple(HP.TOAST_ATTRS, [struct.pack("<I", vid), struct.pack("<i", seq), ("inline", stored[at:at + t.chunk])]))
    tid_b = t.insert(row(101, ("external", len(body) + 4, len(stored), vid, t.toast_relid)))
    tids += [t.insert(row(i, ("inline", HP.vector_datum_body(vecs[i])))) for i in range(10, 20)]
    order = list(range(10)) + [20, 21] + list(range(10, 20))  # rows 10 and 11 of the index are the compressed ones
    all_tids = np.array(tids[:10] + [tid_a, tid_b] + tids[10:], np.uint64)
    expect = [vecs[i] for i in range(10)] + [None, None] + [vecs[i] for i in range(10, 20)]
    assert len(order) == len(all_tids) == 22
    rows, info, found, ncomp = HC.read_dev(gpu_ctx, t, all_tids, dim)
    HC.check_rows(rows, dim, expect, found)
    assert ncomp == 2 and info["n_external"] == 20 and info["n_inline"] == 0 and info["n_chunks"] == 20 * 2
    assert sum(info[k] for k in ("n_inline", "n_external", "n_deleted", "n_null", "n_dead_line_pointer", "n_not_found", "n_toast_incomplete")) + ncomp == 22
    rest = all_tids[found == 0]
    hvecs, hinfo, hfound = HC.read_host(t, rest, dim)
    assert rest.size == 2 and hfound.all() and hvecs[0].tobytes() == v.tobytes() == hvecs[1].tobytes()


# ---- 6. malformed input ---------------------------------------------------------------------------------------------------------------------
def _heap_case():
    dim = 64
    t, tids, expect = HC.make_table(40, dim, seed=3, null_frac=0.0)
    i0 = next(i for i in range(40) if expect[i] is not None)
    good = bytearray(t.heap.tobytes())
    blk, off = int(tids[i0]) >> 16, int(tids[i0]) & 0xFFFF
    lp_at = blk * HP.BLCKSZ + HP.SIZE_OF_PAGE_HEADER + 4 * (off - 1)
    lp = struct.unpack_from("<I", good, lp_at)[0]
    tup = blk * HP.BLCKSZ + (lp & 0x7FFF)
    vs, vl = HP.parse_tuple(ATTRS, bytes(good[tup:tup + (lp >> 17)]))[VEC_ATT - 1]
    return dict(dim=dim, t=t, tids=tids, good=good, blk=blk, lp_at=lp_at, lp=lp, tup=tup, vs=vs, vl=vl)


HEAP_MUTATIONS = {
    "another_page_size": (lambda b, c: struct.pack_into("<H", b, c["blk"] * HP.BLCKSZ + 18, 4096 | 4), "pagesize"),
    "item_inside_the_header": (lambda b, c: struct.pack_into("<I", b, c["lp_at"], (c["lp"] & ~0x7FFF) | 8), "outside"),
    "t_hoff_not_aligned": (lambda b, c: b.__setitem__(c["tup"] + 22, 255), "t_hoff"),
    "t_hoff_into_the_data": (lambda b, c: b.__setitem__(c["tup"] + 22, 200), None),  # caught downstream
    "another_dim": (lambda b, c: struct.pack_into("<h", b, c["tup"] + c["vs"] + 4, c["dim"] + 1), "dimensions"),
    "varlena_past_the_tuple": (lambda b, c: struct.pack_into("<I", b, c["tup"] + c["vs"], (c["vl"] + 4000) << 2), "runs past"),
}


@pytest.mark.parametrize("name", list(HEAP_MUTATIONS))
def test_malformed_heap_pages_are_rejected(gpu_ctx, name):
    from pgvectorscale_amd import VsError
    c = _heap_case()
    mut, match = HEAP_MUTATIONS[name]
    b = bytearray(c["good"])
    mut(b, c)
    t2 = HP.Table(ATTRS)
    t2.heap.pages = [b[i:i + HP.BLCKSZ] for i in range(0, len(b), HP.BLCKSZ)]
    t2.toast = c["t"].toast
    with pytest.raises(VsError, match=match) as e:
        HC.read_dev(gpu_ctx, t2, c["tids"], c["dim"])  # (checks the guard rows on its way out)
    assert e.value.code == INVALID and f"heap block {c['blk']} " in str(e.value)
    # the host reader refuses the same page
    with pytest.raises(VsError, match=match):
        HC.read_host(t2, c["tids"], c["dim"])


def _toast_case():
    dim = 768
    t, tids, expect = HC.make_table(8, dim, seed=9, null_frac=0.0)
    items = HC.toast_items(t.toast)
    return dim, t, tids, items


def _patched_toast(t, blk, item_bytes, old_item):
    t2 = HP.Table(ATTRS)
    t2.heap = t.heap
    t2.toast.pages = [bytearray(p) for p in t.toast.pages]
    at = bytes(t2.toast.pages[blk]).index(old_item)
    t2.toast.pages[blk][at:at + len(item_bytes)] = item_bytes
    return t2


@pytest.mark.parametrize("name", ["negative_seq", "short_non_final_chunk", "chunk_past_extsize", "value_referenced_twice"])
def test_malformed_toast_input_is_rejected(gpu_ctx, name):
    from pgvectorscale_amd import VsError
    dim, t, tids, items = _toast_case()
    wanted = set(v for v in HC.external_value_ids(t, tids) if v is not None)
    first = next((blk, it) for blk, _, it in items if HC.chunk_fields(it)[0] in wanted and HC.chunk_fields(it)[1] == 0)
    last = next((blk, it) for blk, _, it in items if HC.chunk_fields(it)[0] in wanted and HC.chunk_fields(it)[1] == 1)
    if name == "negative_seq":
        blk, it = first
        b = bytearray(it)
        struct.pack_into("<i", b, HC.chunk_fields(it)[2], -1)
        t2, where, match = _patched_toast(t, blk, bytes(b), it), f"TOAST block {blk} ", "chunk does not fit"
    elif name == "short_non_final_chunk":
        blk, it = first
        b = bytearray(it)
        s, l = HC.chunk_fields(it)[3]
        assert not it[s] & 1 and l == 4 + t.chunk
        struct.pack_into("<I", b, s, (l - 8) << 2)
        t2, where, match = _patched_toast(t, blk, bytes(b), it), f"TOAST block {blk} ", "chunk does not fit"
    elif name == "chunk_past_extsize":
        blk, it = last
        b = bytearray(it)
        struct.pack_into("<i", b, HC.chunk_fields(it)[2], 2)
        t2, where, match = _patched_toast(t, blk, bytes(b), it), f"TOAST block {blk} ", "chunk does not fit"
    else:
        vid = next(iter(wanted))
        t2 = HP.Table(ATTRS)
        t2.heap.pages = [bytearray(p) for p in t.heap.pages]
        t2.toast = t.toast
        dup = t2.insert([struct.pack("<q", 99), None, None, None, ("external", 4 + 4 + 4 * dim, 4 + 4 * dim, vid, t.toast_relid), struct.pack("<i", 99)])
        tids = np.append(tids, np.uint64(dup))
        t2, where, match = t2, "heap block ", "referenced by two heap tuples"
    with pytest.raises(VsError, match=match) as e:
        HC.read_dev(gpu_ctx, t2, tids, dim)
    assert e.value.code == INVALID and where in str(e.value)
    with pytest.raises(VsError):  # the host reader refuses the same input
        HC.read_host(t2, tids, dim)


# ---- 7. into an index -----------------------------------------------------------------------------------------------------------------------
B = HP.BLCKSZ


def _sbq_family(oracle):
    import pages_follow_checks as FC
    fam = FC.Family(dim=96, bits=2, R=16, distance=oracle.COSINE, n_max=400, seed=31)
    t, fam.tids = HC.table_of(fam.vecs, seed=31)  # (the index points into this table)
    return fam, t


def _plain_family(oracle):
    import pages_follow_plain_checks as FCP
    fam = FCP.Family(dim=768, R=50, distance=oracle.L2, n_max=200, seed=32)
    t, fam.tids = HC.table_of(fam.vecs, seed=32)
    return fam, t


def _stage_sbq(ctx, raw, vecs):
    from pgvectorscale_amd.pages import DevicePages
    dp = DevicePages(ctx, len(raw) // B)
    dp.add(raw)
    ix = dp.build_from_meta(vecs=vecs)
    fol = dp.follower(ix)
    dp.close()
    return ix, fol


def _stage_plain(ctx, fam, s, raw, vecs):
    from pgvectorscale_amd.pages import IndexPages
    rd = IndexPages(plain=True)
    rd.add(raw)
    rd.finish()
    ix = rd.upload_plain(ctx, distance_type=fam.distance, default_start=s.start, vecs=vecs)
    fol = rd.follower(ix)
    rd.close()
    return ix, fol


def test_sbq_index_takes_its_column_from_heap_pages(gpu_ctx, oracle):
    """400 x 96, cosine: staged with vs_pages_dev_build without vectors, alloc_vecs, the device reader into array(VS_ARR_VECS),
    refresh_norms — the twin was staged with the host-decoded column"""
    import lifecycle_checks as LC
    import pgvectorscale_amd as P
    from pgvectorscale_amd import _lib
    fam, t = _sbq_family(oracle)
    s = fam.s0(400)
    raw, _ = fam.relation(s)
    hvecs, _, hfound = HC.read_host(t, s.tids, fam.dim)
    assert hfound.all() and hvecs.tobytes() == fam.vecs.tobytes()
    a, fa = _stage_sbq(gpu_ctx, raw, hvecs)
    b, fb = _stage_sbq(gpu_ctx, raw, None)
    fa.close(), fb.close()
    assert not b.array(_lib.ARR_VECS)[0].value
    b.alloc_vecs()
    ptr, stride = b.array(_lib.ARR_VECS)
    assert ptr.value and stride == a.array(_lib.ARR_VECS)[1]
    assert not gpu_ctx.download(ptr, np.empty((400, stride), np.uint32)).any()  # a zeroed column
    info, found, ncomp = HC.fill_column(gpu_ctx, t, s.tids, fam.dim, ptr, stride)
    assert found.all() and info["n_inline"] == 400 and ncomp == 0
    b.refresh_norms()
    assert HC.index_bytes(a) == HC.index_bytes(b)
    da, db = a.download(vecs=True), b.download(vecs=True)
    assert all(da[k].tobytes() == db[k].tobytes() for k in da) and db["vecs"].tobytes() == fam.vecs.tobytes()
    q = np.ascontiguousarray(fam.vecs[:32] * np.float32(1.01))
    ga = LC.check_search_batch(a, fam.oracle(s), q, None, "host-decoded column")
    gb = LC.check_search_batch(b, fam.oracle(s), q, None, "device-decoded column")
    ra, rb = (x.search_batch(q, search_list_size=40, rescore=20, k=10) for x in (a, b))
    assert (ga == gb).all() and (ra[0] == rb[0]).all() and ra[2].view(np.uint32).tobytes() == rb[2].view(np.uint32).tobytes()
    # on an index that has the column: OK, nothing changes
    held = HC.index_bytes(b)
    b.alloc_vecs()
    assert b.array(_lib.ARR_VECS)[0].value == ptr.value and HC.index_bytes(b) == held
    a.close(), b.close()
    # refused while a view is alive
    c, fc = _stage_sbq(gpu_ctx, raw, None)
    fc.close()
    ctx2 = P.Context(0)
    v = c.view(ctx2)
    with pytest.raises(P.VsError, match="view") as e:
        c.alloc_vecs()
    assert e.value.code == STATE and not c.array(_lib.ARR_VECS)[0].value
    with pytest.raises(P.VsError) as e:
        v.alloc_vecs()
    assert e.value.code == STATE
    v.close()
    c.alloc_vecs()
    assert c.array(_lib.ARR_VECS)[0].value
    c.close(), ctx2.close()


def _check_plain_scans(ix, fam, s, where=""):
    q = np.ascontiguousarray(fam.vecs[:16] * np.float32(1.01))
    gi, gt, gd, gst = ix.search_batch(q, search_list_size=20, rescore=10, k=8)
    oi, od, ost = fam.oracle(s).search_batch(q, L=20, rescore=10, k=8)
    assert (gi == oi).all(), where
    assert (gd.view(np.uint32) == od.view(np.uint32)).all(), where
    return gi, gd


def test_plain_index_takes_its_column_from_heap_pages(gpu_ctx, oracle):
    """200 x 768, L2, every vector external in two chunks: upload_plain without vectors leaves the node vectors in the column; it is
    overwritten with a sentinel, then filled from the heap and TOAST pages"""
    from pgvectorscale_amd import _lib
    fam, t = _plain_family(oracle)
    s = fam.s0(200)
    raw, _ = fam.relation(s)
    hvecs, _, hfound = HC.read_host(t, s.tids, fam.dim)
    assert hfound.all()
    a, fa = _stage_plain(gpu_ctx, fam, s, raw, hvecs)
    b, fb = _stage_plain(gpu_ctx, fam, s, raw, None)
    fa.close(), fb.close()
    ptr, stride = b.array(_lib.ARR_VECS)
    b.alloc_vecs()  # (a plain index always has the column)
    assert b.array(_lib.ARR_VECS)[0].value == ptr.value and stride == 768
    gpu_ctx.upload(ptr, np.full(200 * stride, HC.SENTINEL, np.uint32))
    info, found, ncomp = HC.fill_column(gpu_ctx, t, s.tids, fam.dim, ptr, stride)
    assert found.all() and info["n_external"] == 200 and info["n_chunks"] == 400 and ncomp == 0
    b.refresh_norms()
    assert HC.index_bytes(a) == HC.index_bytes(b)
    assert b.download(vecs=True)["vecs"].tobytes() == fam.vecs.tobytes()
    ga, gb = _check_plain_scans(a, fam, s, "host"), _check_plain_scans(b, fam, s, "device")
    assert (ga[0] == gb[0]).all() and ga[1].tobytes() == gb[1].tobytes()
    a.close(), b.close()


# ---- 8. follower ----------------------------------------------------------------------------------------------------------------------------
def _follow_twins(ctx, fam, t, s0, s1, before, after, stage):
    """two indexes staged from `before` follow to `after`: one takes apply with host rows, the other apply_dev with rows the device
    reader took from only the heap and TOAST blocks the new rows touch -> both closed, their arrays compared"""
    import pages_follow_checks as FC
    from pgvectorscale_amd.pages import dirty_blocks
    hvecs, _, _ = HC.read_host(t, fam.tids[:s1.n], fam.dim)  # (the heap's rows: a tid the step clears keeps its row in the index)
    blocks = dirty_blocks(before, after)
    pages = FC.gather(after, blocks.tolist())
    m = s1.n - s0.n
    (a, fa), (b, fb) = stage(hvecs[:s0.n]), stage(hvecs[:s0.n])
    try:
        ia = fa.stage(blocks, pages, len(after) // B)
        ib = fb.stage(blocks, pages, len(after) // B)
        assert ia == ib and ia["n_appended"] == m
        new = fb.new_tids()
        assert (new == s1.tids[s0.n:]).all()
        ha, _, hfound = HC.read_host(t, new, fam.dim)
        assert hfound.all() and ha.tobytes() == fam.vecs[s0.n:s1.n].tobytes()
        done_a = fa.apply(ha)
        heap_blocks, toast_blocks = HC.blocks_of(t, new)
        assert len(heap_blocks) < len(t.heap.pages) and (not t.toast.pages or 0 < len(toast_blocks) < len(t.toast.pages))
        stride = fam.dim + 1
        tgt = HC.Target(ctx, m, stride)
        info, found, ncomp = HC.fill_column(ctx, t, new, fam.dim, tgt.ptr, stride, heap_blocks, toast_blocks)
        assert found.all() and ncomp == 0 and info["n_not_found"] == info["n_toast_incomplete"] == 0
        done_b = fb.apply_dev(tgt.ptr, stride)
        rows = tgt.read()
        tgt.free()
        assert rows[:, :fam.dim].tobytes() == ha.tobytes() and (rows[:, fam.dim:] == HC.SENTINEL).all()
        assert done_a == done_b
        ba, bb = HC.index_bytes(a), HC.index_bytes(b)
        assert ba["n"] == s1.n and ba == bb
        assert a.download(vecs=True)["vecs"].tobytes() == b.download(vecs=True)["vecs"].tobytes() == fam.vecs[:s1.n].tobytes()
    finally:
        fa.close(), fb.close(), a.close(), b.close()


def test_sbq_follower_applies_rows_read_on_the_device(gpu_ctx, oracle):
    fam, t = _sbq_family(oracle)
    s0 = fam.s0(300)
    s1 = fam.mutate(s0, 40, 10, 3, seed=5)
    before, after = fam.relation(s0)[0], fam.relation(s1)[0]
    _follow_twins(gpu_ctx, fam, t, s0, s1, before, after, lambda vecs: _stage_sbq(gpu_ctx, before, vecs))


def test_plain_follower_applies_rows_read_on_the_device(gpu_ctx, oracle):
    fam, t = _plain_family(oracle)
    s0 = fam.s0(150)
    s1 = fam.mutate(s0, 20, 8, 2, seed=6)
    before, after = fam.relation(s0)[0], fam.relation(s1)[0]
    _follow_twins(gpu_ctx, fam, t, s0, s1, before, after, lambda vecs: _stage_plain(gpu_ctx, fam, s0, before, vecs))
    # apply_dev refuses a NULL pointer for appended rows exactly as apply does
    import pgvectorscale_amd as P
    from pgvectorscale_amd.pages import dirty_blocks
    import pages_follow_checks as FC
    trunc = type(fam)(dim=40, dim_index=24, R=6, distance=oracle.L2, n_max=90, seed=16)
    ts0 = trunc.s0(60)
    ts1 = trunc.mutate(ts0, 5, 2, 0, seed=2)
    tb, ta = trunc.relation(ts0)[0], trunc.relation(ts1)[0]
    ix, fol = _stage_plain(gpu_ctx, trunc, ts0, tb, ts0.vecs)
    blocks = dirty_blocks(tb, ta)
    fol.stage(blocks, FC.gather(ta, blocks.tolist()), len(ta) // B)
    with pytest.raises(P.VsError, match="new_vecs is NULL") as e:
        fol.apply_dev(None, 0)
    assert e.value.code == INVALID
    fol.close(), ix.close()
