"""Shared fabricators of the device heap reader's tests (tests/test_gpu_zx_heap_dev.py): tables
manufactured with oracle/heap_py.py, the host reader (HeapColumn) and the device reader (HeapColumnDev) run over the same pages, and
a target buffer with sentinel padding and guard rows on both sides.  Expectations never come from the device."""
import struct

import numpy as np

from oracle import heap_py as HP

# id bigint, label smallint, tags smallint[] (varlena), note text (varlena), embedding vector, extra int4
ATTRS = [(8, "d"), (2, "s"), (-1, "i"), (-1, "i"), (-1, "i"), (4, "i")]
VEC_ATT = 5  # 1-based attnum of `embedding`
ONE_COL = [(-1, "i")]  # a table of nothing but the vector: 185 two-dimensional rows on an 8 KB page
SENTINEL = np.uint32(0x7FC0BEEF)  # a NaN no vector holds
GUARD = 3  # rows in front of and behind the target rows
VS_ARR_VECS = 3
INVALID, STATE = -1, -5


def make_table(n, dim, seed, null_frac=0.05, page_size=HP.BLCKSZ):
    """the six-column table: NULLs in every nullable column, short and long varlenas in front of the vector, rows older than
    ADD COLUMN extra -> (table, tids uint64 [n], expect: per row the source vector or None)"""
    rng = np.random.default_rng(seed)
    t = HP.Table(ATTRS, page_size=page_size)
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    tids, expect = [], []
    for i in range(n):
        tags = None if rng.random() < 0.3 else ("inline", struct.pack("<iiiii", 1, 0, 21, 3, 1) + rng.bytes(int(rng.integers(0, 9)) * 2))
        note = None if rng.random() < 0.2 else ("inline", rng.bytes(int(rng.choice([0, 3, 60, 126, 127, 200, 900]))))
        vec = None if rng.random() < null_frac else ("inline", HP.vector_datum_body(vecs[i]))
        label = None if rng.random() < 0.1 else struct.pack("<h", int(rng.integers(-5, 100)))
        natts = len(ATTRS) if rng.random() < 0.8 else int(rng.integers(VEC_ATT - 1, len(ATTRS) + 1))  # some rows older than the vector
        vals = [struct.pack("<q", i), label, tags, note, vec, struct.pack("<i", i)]
        tids.append(t.insert(vals, natts=natts))
        expect.append(None if vec is None or natts < VEC_ATT else vecs[i])
    return t, np.array(tids, np.uint64), expect


def make_one_column_table(n, dim, seed, null_frac=0.05):
    rng = np.random.default_rng(seed)
    t = HP.Table(ONE_COL)
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    tids, expect = [], []
    for i in range(n):
        vec = None if rng.random() < null_frac else ("inline", HP.vector_datum_body(vecs[i]))
        tids.append(t.insert([vec]))
        expect.append(None if vec is None else vecs[i])
    return t, np.array(tids, np.uint64), expect


def index_order(tids, expect, seed=1, deleted=0.05):
    """index order is not heap order: shuffled, and a few index tuples deleted (vacuum: offset 0) -> (tids as the heap has them,
    tids as the index names them, expect, deleted mask)"""
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(tids))
    tids, expect = tids[order], [expect[i] for i in order]
    dele = rng.random(len(tids)) < deleted
    tids_idx = tids.copy()
    tids_idx[dele] &= ~np.uint64(0xFFFF)
    return tids, tids_idx, expect, dele


def pglz_compress(data):
    """a plain greedy pglz encoder (test infrastructure): control byte per 8 items; match = 2 bytes (+1 for lengths >= 18)"""
    out = bytearray()
    i, n = 0, len(data)
    while i < n:
        ctrl_at = len(out)
        out.append(0)
        for bit in range(8):
            if i >= n:
                break
            best_len, best_off = 0, 0
            for off in range(1, min(i, 4095) + 1):
                l = 0
                while l < 273 and i + l < n and data[i + l - off] == data[i + l]:
                    l += 1
                if l > best_len:
                    best_len, best_off = l, off
                    if l == 273:
                        break
            if best_len >= 3:
                out[ctrl_at] |= 1 << bit
                if best_len >= 18:
                    out += bytes([((best_off >> 4) & 0xF0) | 0x0F, best_off & 0xFF, best_len - 18])
                else:
                    out += bytes([((best_off >> 4) & 0xF0) | (best_len - 3), best_off & 0xFF])
                i += best_len
            else:
                out.append(data[i])
                i += 1
    return bytes(out)


def ranges(n_blocks, step=None):
    """[(first_block, n_blocks)] covering [0, n_blocks) in calls of `step` blocks (None: one call)"""
    step = step or max(n_blocks, 1)
    return [(b, min(step, n_blocks - b)) for b in range(0, n_blocks, step)] or [(0, 0)]


def read_host(t, tids, dim, attrs=ATTRS, vec_att=VEC_ATT):
    """the host reader over the whole table -> (vecs [n][dim], info, found)"""
    from pgvectorscale_amd.pages import HeapColumn
    hc = HeapColumn(attrs, vec_att, dim, tids, page_size=t.heap.page_size)
    hc.add(t.heap.tobytes())
    hc.toast_add(t.toast.tobytes())
    info, found = hc.finish()
    vecs = hc.vecs.copy()
    hc.close()
    return vecs, info, found


class Target:
    """n rows of out_stride floats in device memory, every word a sentinel, with GUARD rows in front and behind"""

    def __init__(self, ctx, n, stride):
        self.ctx, self.n, self.stride = ctx, n, stride
        self.rows = n + 2 * GUARD
        self.d = ctx.alloc(self.rows * stride * 4)
        ctx.upload(self.d, np.full(self.rows * stride, SENTINEL, np.uint32))
        self.ptr = self.d.value + GUARD * stride * 4

    def read(self):
        """-> the n target rows as uint32 [n][stride]; the guard rows must still hold the sentinel"""
        buf = self.ctx.download(self.d, np.empty((self.rows, self.stride), np.uint32))
        assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + self.n:] == SENTINEL).all(), "a row outside [0, n) was written"
        return buf[GUARD:GUARD + self.n]

    def free(self):
        self.ctx.free(self.d)


def read_dev(ctx, t, tids, dim, heap_ranges=None, toast_ranges=None, stride=None, attrs=ATTRS, vec_att=VEC_ATT):
    """the device reader over the listed block ranges (None: the whole relation in one call) -> (rows uint32 [n][stride], info,
    found, n_compressed).  The guard rows are checked whether the read succeeds or raises."""
    from pgvectorscale_amd.pages import HeapColumnDev
    ps = t.heap.page_size
    stride = stride or dim
    tgt = Target(ctx, len(tids), stride)
    hc = None
    try:
        try:
            hc = HeapColumnDev(ctx, attrs, vec_att, dim, tids, tgt.ptr, stride, page_size=ps)
            heap, toast = t.heap.tobytes(), t.toast.tobytes()
            for fb, nb in (ranges(len(t.heap.pages)) if heap_ranges is None else heap_ranges):
                hc.add(heap[fb * ps:(fb + nb) * ps], first_block=fb)
            for fb, nb in (ranges(len(t.toast.pages)) if toast_ranges is None else toast_ranges):
                hc.toast_add(toast[fb * ps:(fb + nb) * ps], first_block=fb)
            info, found, ncomp = hc.finish()
        finally:
            if hc is not None:
                hc.close()
            rows = tgt.read()
    finally:
        tgt.free()
    return rows, info, found, ncomp


def check_rows(rows, dim, expect, found):
    """found rows hold the source bytes, every other row is zero, the padding floats are untouched"""
    assert (rows[:, dim:] == SENTINEL).all(), "padding floats were written"
    for i, e in enumerate(expect):
        if e is None:
            assert not found[i] and not rows[i, :dim].any(), i
        else:
            assert found[i] and rows[i, :dim].tobytes() == np.asarray(e, np.float32).tobytes(), i


def toast_items(rel):
    """[(block, offset, item bytes)] of a relation's LP_NORMAL items"""
    out = []
    for blk in range(len(rel.pages)):
        for off in range(1, rel.max_offset(blk) + 1):
            lp = struct.unpack_from("<I", rel.pages[blk], HP.SIZE_OF_PAGE_HEADER + 4 * (off - 1))[0]
            if (lp >> 15) & 3 == HP.LP_NORMAL:
                out.append((blk, off, bytes(rel.pages[blk][lp & 0x7FFF:(lp & 0x7FFF) + (lp >> 17)])))
    return out


def chunk_fields(item):
    """(chunk_id, chunk_seq, offset of chunk_seq inside the item, (start, size) of chunk_data inside the item)"""
    spans = HP.parse_tuple(HP.TOAST_ATTRS, item)
    return (struct.unpack_from("<I", item, spans[0][0])[0], struct.unpack_from("<i", item, spans[1][0])[0], spans[1][0], spans[2])


def external_value_ids(t, tids, vec_att=VEC_ATT):
    """per tid: the TOAST value id its tuple's vector points at, or None"""
    out = []
    for tid in tids:
        blk, off = int(tid) >> 16, int(tid) & 0xFFFF
        if off == 0:  # a deleted index tuple
            out.append(None)
            continue
        lp = struct.unpack_from("<I", t.heap.pages[blk], HP.SIZE_OF_PAGE_HEADER + 4 * (off - 1))[0]
        tup = bytes(t.heap.pages[blk][lp & 0x7FFF:(lp & 0x7FFF) + (lp >> 17)])
        span = HP.parse_tuple(t.attrs, tup)[vec_att - 1]
        out.append(struct.unpack_from("<I", tup, span[0] + 10)[0] if span is not None and tup[span[0]] == 0x01 else None)
    return out


def table_of(vecs, seed):
    """the six-column table holding one row per given vector, in order, none NULL -> (table, tids uint64 [n])"""
    rng = np.random.default_rng(seed)
    t = HP.Table(ATTRS)
    tids = []
    for i, v in enumerate(vecs):
        tags = None if rng.random() < 0.3 else ("inline", struct.pack("<iiiii", 1, 0, 21, 3, 1) + rng.bytes(int(rng.integers(0, 9)) * 2))
        note = None if rng.random() < 0.2 else ("inline", rng.bytes(int(rng.choice([0, 3, 60, 126, 127, 200, 900]))))
        label = None if rng.random() < 0.1 else struct.pack("<h", int(rng.integers(-5, 100)))
        tids.append(t.insert([struct.pack("<q", i), label, tags, note, ("inline", HP.vector_datum_body(v)), struct.pack("<i", i)]))
    return t, np.array(tids, np.uint64)


def blocks_of(t, tids):
    """(heap blocks, TOAST blocks) the rows behind `tids` touch, ascending"""
    heap = sorted({int(x) >> 16 for x in tids if int(x) & 0xFFFF})
    vids = {v for v in external_value_ids(t, tids) if v is not None}
    toast = sorted({blk for blk, _, it in toast_items(t.toast) if chunk_fields(it)[0] in vids})
    return heap, toast


def fill_column(ctx, t, tids, dim, d_ptr, stride, heap_blocks=None, toast_blocks=None):
    """the device reader into rows at d_ptr, fed block by block over the listed blocks only (None: every block) -> (info, found, n_compressed)"""
    from pgvectorscale_amd.pages import HeapColumnDev
    ps = t.heap.page_size
    hc = HeapColumnDev(ctx, ATTRS, VEC_ATT, dim, tids, d_ptr, stride, page_size=ps)
    try:
        for b in (range(len(t.heap.pages)) if heap_blocks is None else heap_blocks):
            hc.add(bytes(t.heap.pages[b]), first_block=b)
        for b in (range(len(t.toast.pages)) if toast_blocks is None else toast_blocks):
            hc.toast_add(bytes(t.toast.pages[b]), first_block=b)
        return hc.finish()
    finally:
        hc.close()


def index_bytes(ix):
    """every per-node array of an index as the device holds it (rows at their device strides) -> {name: bytes}"""
    from pgvectorscale_amd import _lib
    ix._refresh()
    n, ctx = ix.desc.n, ix.ctx
    out = {"n": n}
    for name, which, dt in (("codes", _lib.ARR_CODES, np.uint64), ("nbrs", _lib.ARR_NBRS, np.uint32), ("tids", _lib.ARR_TIDS, np.uint64),
                            ("vecs", _lib.ARR_VECS, np.uint32), ("vnorm", _lib.ARR_VNORM, np.float32)):
        ptr, stride = ix.array(which)
        out[name] = ctx.download(ptr, np.empty((n, stride), dt)).tobytes() if ptr.value and n else b""
    return out
