"""Index relation pages -> an index resident in HBM (host-side mirror of the vs_pages_* calls of include/vsgpu.h).

`IndexPages` stands for the main fork of a `diskann` index relation (Meta chain on block 0, SbqMeans chain, SbqNode
pages; UT/page.rs:28-39).  Blocks are appended in block order, decoded by libvsgpu on the host cores into the flat
arrays of `vs_index_host`, and `upload()` streams them to the device through the pinned staging ring.  What is NOT
read from the pages is what the reference itself keeps elsewhere or only the Rust side can decode: the heap's vector
column (`vecs`, needed for rerank).  The MetaPage body (geometry, start nodes, the SbqMeans pointer) is decoded by
`meta()` / `upload_from_meta()` (vs_pages_meta), or passed by hand to `upload()`.

The way back is `PagesOut` (vs_pages_out_*): a device-resident index written out as the same relation, block range by block
range — or, against a `PagesBase`, only the blocks that changed since it was last written (`delta` / `read_blocks` /
`patch_file`) — and `encode_meta_page` next to `decode_meta_page`.

`PagesFollower` (vs_pages_follow_*) is the opposite direction page by page: when something else writes the relation (a standby's
WAL replay, the CPU extension's aminsert and vacuum), the blocks that changed are staged, checked on the device and scattered
into the resident arrays (SBQ and, with plain=True, `plain` storage indexes); `dirty_blocks` is the bytewise page compare that finds them where nothing better names them.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (HeapAttr, HeapInfo, IndexDesc, IndexHost, MetaLayout, MetaPage, NodeLayout, PagesFollowInfo, PagesInfo, PagesOutParams,
                   check)

BLCKSZ = 8192
PAGE_SBQ_MEANS, PAGE_META = 7, 8


def _meta_layout(layout):
    """None, or a {"root_size": .., field: offset} dict as oracle/pages_py.meta_layout() gives / offset_of! prints"""
    if layout is None:
        return None
    lay = MetaLayout()
    lay.root_size = layout["root_size"]
    for k, _ in MetaLayout._fields_[1:]:
        setattr(lay, k, layout[k[4:]])
    return lay


def decode_meta_page(data, layout=None):
    """rkyv::from_bytes::<MetaPage> over the payload of the chain at (0, 2) -> (fields, {label: (block, offset)})"""
    L = _lib.load()
    buf = np.frombuffer(bytes(data), np.uint8)
    lay = _meta_layout(layout)
    m = MetaPage()
    check(L.vs_meta_page_decode(buf.ctypes.data_as(C.c_void_p), buf.size, None if lay is None else C.byref(lay), C.byref(m), None,
                                None, None, 0))
    n = int(m.n_labeled_start_nodes)
    lab, blk, off = np.empty(n, np.int16), np.empty(n, np.uint32), np.empty(n, np.uint32)
    check(L.vs_meta_page_decode(buf.ctypes.data_as(C.c_void_p), buf.size, None if lay is None else C.byref(lay), C.byref(m),
                                lab.ctypes.data_as(C.c_void_p), blk.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), n))
    return m.as_dict(), {int(l): (int(b), int(o)) for l, b, o in zip(lab, blk, off)}


def encode_meta_page(fields, labeled_starts=None, layout=None):
    """rkyv::to_bytes::<MetaPage>: `fields` as decode_meta_page returns them (missing keys are zero; has_start_nodes selects
    Some(StartNodes)), labeled_starts {label: (block, offset)} -> the bytes of the chain payload at (0, 2)"""
    L = _lib.load()
    m = MetaPage()
    for k, v in fields.items():
        setattr(m, k, v.encode() if isinstance(v, str) else v)
    ls = sorted((labeled_starts or {}).items())
    lab = np.array([k for k, _ in ls], np.int16)
    blk = np.array([v[0] for _, v in ls], np.uint32)
    off = np.array([v[1] for _, v in ls], np.uint32)
    lay = _meta_layout(layout)
    args = (C.byref(m), lab.ctypes.data_as(C.c_void_p), blk.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), len(ls),
            None if lay is None else C.byref(lay))
    n = C.c_size_t()
    check(L.vs_meta_page_encode(*args, None, 0, C.byref(n)))
    buf = np.empty(int(n.value), np.uint8)
    check(L.vs_meta_page_encode(*args, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)))
    return buf.tobytes()


def _meta_of(fn, handle, layout):
    lay = _meta_layout(layout)
    m, d = MetaPage(), IndexDesc()
    check(fn(handle, None if lay is None else C.byref(lay), C.byref(m), C.byref(d), None, None, 0))
    n = int(d.n_label_starts)
    lab, nodes = np.empty(n, np.int16), np.empty(n, np.uint32)
    check(fn(handle, None if lay is None else C.byref(lay), C.byref(m), C.byref(d), lab.ctypes.data_as(C.c_void_p),
             nodes.ctypes.data_as(C.c_void_p), n))
    return m.as_dict(), d, {int(l): int(v) for l, v in zip(lab, nodes)}


class HeapColumn:
    """The heap's vector column, staged from the pages of the table and its TOAST relation (vs_heap_*): `vecs[node]` = the
    vector of the heap tuple node's heap TID names — what the reference fetches per rescore candidate."""

    def __init__(self, attrs, vector_attno, dim, heap_tids, page_size=BLCKSZ):
        """attrs: [(attlen, attalign)] of the table's columns in attnum order; vector_attno 1-based"""
        self._L = _lib.load()
        self.page_size = page_size
        self._attrs = (HeapAttr * len(attrs))(*[HeapAttr(int(l), a.encode()) for l, a in attrs])
        self._tids = np.ascontiguousarray(heap_tids, np.uint64)
        self.vecs = np.empty((self._tids.size, dim), np.float32)
        h = C.c_void_p()
        check(self._L.vs_heap_open(page_size, self._attrs, len(attrs), vector_attno, dim, self._tids.ctypes.data_as(C.c_void_p),
                                   self._tids.size, self.vecs.ctypes.data_as(C.c_void_p), dim, C.byref(h)))
        self.h = h
        self._nb = [0, 0]

    def _add(self, fn, which, pages, first_block):
        buf = np.frombuffer(pages, np.uint8)
        if buf.size % self.page_size:
            raise ValueError(f"{buf.size} bytes is not a whole number of {self.page_size}-byte pages")
        nb = buf.size // self.page_size
        fb = self._nb[which] if first_block is None else first_block
        check(fn(self.h, fb, buf.ctypes.data_as(C.c_void_p), nb))
        self._nb[which] += nb

    def add(self, pages, first_block=None):
        self._add(self._L.vs_heap_add, 0, pages, first_block)

    def toast_add(self, pages, first_block=None):
        self._add(self._L.vs_heap_toast_add, 1, pages, first_block)

    def finish(self):
        info = HeapInfo()
        found = np.zeros(self._tids.size, np.uint8)
        check(self._L.vs_heap_finish(self.h, C.byref(info), found.ctypes.data_as(C.c_void_p)))
        return info.as_dict(), found

    def close(self):
        if self.h:
            self._L.vs_heap_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HeapColumnDev:
    """The same column decoded on the device (vs_heap_dev_*): the pages go to HBM as they are and kernels scatter the floats into
    rows of device memory `d_out` ([n][out_stride] floats: Context.alloc, or DiskAnnIndex.array(VS_ARR_VECS) plus a row offset).
    Block ranges may have gaps (first_block ascending); compressed vectors are counted, not decoded: read those rows with
    HeapColumn over heap_tids[found == 0]."""

    def __init__(self, ctx, attrs, vector_attno, dim, heap_tids, d_out, out_stride, page_size=BLCKSZ):
        self._L = _lib.load()
        self.ctx = ctx
        self.page_size = page_size
        self._attrs = (HeapAttr * len(attrs))(*[HeapAttr(int(l), a.encode()) for l, a in attrs])
        self._tids = np.ascontiguousarray(heap_tids, np.uint64)
        self.h = None
        h = C.c_void_p()
        d_out = d_out if isinstance(d_out, C.c_void_p) else C.c_void_p(d_out)
        check(self._L.vs_heap_dev_open(ctx.h, page_size, self._attrs, len(attrs), vector_attno, dim, self._tids.ctypes.data_as(C.c_void_p),
                                       self._tids.size, d_out, out_stride, C.byref(h)))
        self.h = h
        self._nb = [0, 0]

    def _add(self, fn, which, pages, first_block):
        buf = np.frombuffer(pages, np.uint8)
        if buf.size % self.page_size:
            raise ValueError(f"{buf.size} bytes is not a whole number of {self.page_size}-byte pages")
        nb = buf.size // self.page_size
        fb = self._nb[which] if first_block is None else first_block
        check(fn(self.h, fb, buf.ctypes.data_as(C.c_void_p), nb))
        self._nb[which] = fb + nb

    def add(self, pages, first_block=None):
        """blocks of the heap's main fork from first_block on (None: behind the previous range)"""
        self._add(self._L.vs_heap_dev_add, 0, pages, first_block)

    def toast_add(self, pages, first_block=None):
        self._add(self._L.vs_heap_dev_toast_add, 1, pages, first_block)

    def finish(self):
        """-> (info dict as HeapColumn.finish gives it, found uint8 [n], n_compressed)"""
        info = HeapInfo()
        found = np.zeros(self._tids.size, np.uint8)
        nc = C.c_uint32(0)
        check(self._L.vs_heap_dev_finish(self.h, C.byref(info), found.ctypes.data_as(C.c_void_p), C.byref(nc)))
        return info.as_dict(), found, int(nc.value)

    def close(self):
        if self.h:
            self._L.vs_heap_dev_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HeapResident:
    """The heap's main fork resident in device memory (vs_heap_res_*), indexed by block number: put() the whole fork once and the
    changed blocks afterwards; visibility() then decides, on the device, what table_index_fetch_tuple would find behind every heap
    tid under an MVCC snapshot (include/vsgpu.h has the rule).  DiskAnnIndex.snapshot_eval runs it over an index's own tid column."""

    def __init__(self, ctx, capacity_blocks=0, page_size=BLCKSZ):
        self._L = _lib.load()
        self.ctx = ctx
        self.page_size = page_size
        self.h = None
        h = C.c_void_p()
        check(self._L.vs_heap_res_open(ctx.h, page_size, capacity_blocks, C.byref(h)))
        self.h = h

    def put(self, pages, first_block=0):
        """host pages of blocks first_block.. (any order across calls; a later put of a block overwrites it)"""
        buf = np.frombuffer(pages, np.uint8)
        if buf.size % self.page_size:
            raise ValueError(f"{buf.size} bytes is not a whole number of {self.page_size}-byte pages")
        check(self._L.vs_heap_res_put(self.h, first_block, buf.ctypes.data_as(C.c_void_p), buf.size // self.page_size))

    def blocks(self):
        """one past the highest block ever put"""
        return int(self._L.vs_heap_res_blocks(self.h))

    def visibility(self, d_heap_tids, n, snapshot, xact, d_visible, cap=None):
        """d_heap_tids: device uint64 [n]; d_visible: device uint8 [n], written.  snapshot / xact: see _lib.vis_args.  cap: how many
        undecided nodes to hand back (None: all of them) -> (stats dict, undecided nodes uint32 ascending, their full number)"""
        s, x, _keep = _lib.vis_args(snapshot, xact)
        cap = n if cap is None else cap
        und = np.empty(max(cap, 1), np.uint32)
        st, nu = _lib.VisStats(), C.c_uint32(0)
        as_ptr = lambda p: p if isinstance(p, C.c_void_p) or p is None else C.c_void_p(p)  # noqa: E731
        check(self._L.vs_heap_res_visibility(self.h, as_ptr(d_heap_tids), n, C.byref(s), C.byref(x), as_ptr(d_visible), C.byref(st),
                                             und.ctypes.data_as(C.c_void_p), cap, C.byref(nu)))
        return st.as_dict(), und[:min(cap, int(nu.value))].copy(), int(nu.value)

    def close(self):
        if self.h:
            self._L.vs_heap_res_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IndexPages:
    def __init__(self, has_labels=False, page_size=BLCKSZ, layout=None, threads=0, plain=False):
        """plain=True: a `plain` storage index (PlainNode items: full-precision vectors in the nodes, no SBQ codes, no labels)"""
        self._L = _lib.load()
        h = C.c_void_p()
        lay = None
        if layout is not None:
            lay = NodeLayout(*layout)
        self.plain = bool(plain)
        if plain:
            check(self._L.vs_pages_open_plain(page_size, None if lay is None else C.byref(lay), threads, C.byref(h)))
        else:
            check(self._L.vs_pages_open(page_size, int(has_labels), None if lay is None else C.byref(lay), threads, C.byref(h)))
        self.h = h
        self.page_size = page_size
        self.has_labels = bool(has_labels)
        self.n_blocks = 0
        self.info = None

    @staticmethod
    def default_layout(has_labels):
        lay = NodeLayout()
        check(_lib.load().vs_node_layout_default(int(has_labels), C.byref(lay)))
        return tuple(int(getattr(lay, k)) for k, _ in NodeLayout._fields_)

    def add(self, pages, first_block=None):
        """Append whole blocks (bytes-like, a multiple of page_size long)."""
        buf = np.frombuffer(pages, np.uint8)
        if buf.size % self.page_size:
            raise ValueError(f"{buf.size} bytes is not a whole number of {self.page_size}-byte pages")
        nb = buf.size // self.page_size
        fb = self.n_blocks if first_block is None else first_block
        check(self._L.vs_pages_add(self.h, fb, buf.ctypes.data_as(C.c_void_p), nb))
        self.n_blocks += nb

    def add_file(self, path, chunk_blocks=16384):
        """Append a relation segment file (base/<db>/<relfilenode>[.N]) chunk by chunk."""
        with open(path, "rb") as f:
            while True:
                b = f.read(chunk_blocks * self.page_size)
                if not b:
                    break
                self.add(b)

    def finish(self):
        info = PagesInfo()
        check(self._L.vs_pages_finish(self.h, C.byref(info)))
        self.info = info
        return info

    def node_of(self, block, offset):
        """IndexPointer -> node id (e.g. the MetaPage's start nodes)."""
        out = C.c_uint32()
        check(self._L.vs_pages_node_of(self.h, block, offset, C.byref(out)))
        return int(out.value)

    def item_pointer_of(self, node):
        b, o = C.c_uint32(), C.c_uint32()
        check(self._L.vs_pages_item_pointer_of(self.h, node, C.byref(b), C.byref(o)))
        return int(b.value), int(o.value)

    def block_table(self):
        """-> (blk_base, blk_cnt): dense id of every block's first node, SbqNode items on every block (copies)"""
        return _block_table(self._L.vs_pages_block_table, self.h)

    def follower(self, index, layout=None):
        """a PagesFollower of `index` (staged from these pages) that starts at this relation's block table"""
        return PagesFollower(index, self.block_table()[1], layout=layout, page_size=self.page_size, plain=self.plain)

    def read_chain(self, block, offset, page_type):
        n = C.c_size_t()
        check(self._L.vs_pages_read_chain(self.h, block, offset, page_type, None, 0, C.byref(n)))
        buf = np.empty(int(n.value), np.uint8)
        check(self._L.vs_pages_read_chain(self.h, block, offset, page_type, buf.ctypes.data_as(C.c_void_p), buf.size,
                                          C.byref(n)))
        return buf.tobytes()

    def sbq_means(self, block, offset):
        """SbqMeans::load at MetaPage.quantizer_metadata -> (count, mean, m2)"""
        dim, cnt = C.c_uint32(), C.c_uint64()
        check(self._L.vs_pages_sbq_means(self.h, block, offset, None, None, 0, C.byref(dim), C.byref(cnt)))
        mean = np.empty(dim.value, np.float32)
        m2 = np.empty(dim.value, np.float32)
        check(self._L.vs_pages_sbq_means(self.h, block, offset, mean.ctypes.data_as(C.c_void_p),
                                         m2.ctypes.data_as(C.c_void_p), dim.value, C.byref(dim), C.byref(cnt)))
        return int(cnt.value), mean, m2

    def meta(self, layout=None):
        """MetaPage::fetch (AM/meta_page.rs:380-403): -> (MetaPage fields, vs_index_desc with node-id start, {label: start node})"""
        if self.info is None:
            self.finish()
        return _meta_of(self._L.vs_pages_meta, self.h, layout)

    def upload_from_meta(self, ctx, vecs=None, meta_layout=None):
        """everything but the heap's vector column comes from the relation: geometry and start nodes from the MetaPage, the
        quantizer from the SbqMeans chain it points at, nodes from the SbqNode pages"""
        m, d, starts = self.meta(meta_layout)
        assert bool(m["has_labels"]) == self.has_labels
        has_q = m["quantizer_block"] != 0xFFFFFFFF
        return self.upload(ctx, dim_index=d.dim_index, bits=d.bits, distance_type=d.distance_type,
                           default_start=None if d.default_start == _lib.VS_INVALID_NODE else int(d.default_start),
                           quantizer_metadata=(m["quantizer_block"], m["quantizer_offset"]) if has_q else None,
                           vecs=vecs, label_starts=starts)

    def _host(self):
        if self.info is None:
            self.finish()
        h = IndexHost()
        check(self._L.vs_pages_host(self.h, C.byref(h)))
        return h

    def arrays(self):
        """Copies of the decoded flat arrays (tests / inspection)."""
        h = self._host()
        n, W, R = self.info.n_nodes, self.info.words, self.info.num_neighbors

        def view(ptr, dtype, count):
            if not ptr or count == 0:
                return np.zeros(0, dtype)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), (count,)).copy()

        out = {"nbrs": view(h.nbrs, np.uint32, n * R).reshape(n, R), "heap_tids": view(h.heap_tids, np.uint64, n)}
        if self.plain:
            out["vecs"] = view(h.vecs, np.float32, n * W).reshape(n, W)  # PlainNode.vector
        else:
            out["codes"] = view(h.codes, np.uint64, n * W).reshape(n, W)
        if self.has_labels:
            out["label_off"] = view(h.label_off, np.uint32, n + 1)
            out["label_val"] = view(h.label_val, np.int16, int(self.info.n_label_vals))
        return out

    def upload_plain(self, ctx, *, distance_type, default_start, vecs=None):
        """a `plain` storage index in HBM: the graph from the pages; `vecs` = the heap's vector column (HeapColumn) or, when
        None, the node vectors themselves (the cosine-normalised index slice: enough when num_dimensions_to_index = num_dimensions)"""
        from .index import DiskAnnIndex
        assert self.plain
        a = self.arrays()
        node = self.node_of(*default_start) if isinstance(default_start, tuple) else default_start
        v = a["vecs"] if vecs is None else np.ascontiguousarray(vecs, np.float32)
        return DiskAnnIndex._upload_plain(ctx, nbrs=a["nbrs"], heap_tids=a["heap_tids"], vecs=v, num_neighbors=self.info.num_neighbors,
                                          distance_type=distance_type, default_start=_lib.VS_INVALID_NODE if node is None else int(node),
                                          dim_index=a["vecs"].shape[1])

    def upload(self, ctx, *, dim_index, bits, distance_type, default_start, quantizer_metadata=None, mean=None, m2=None,
               count=0, vecs=None, label_starts=None):
        """vs_index_upload of the decoded arrays.  default_start / label_starts values are IndexPointers (block, offset)
        or node ids; quantizer_metadata is the IndexPointer of the SbqMeans chain (or pass mean / m2 / count)."""
        from .index import DiskAnnIndex
        h = self._host()
        info = self.info
        if quantizer_metadata is not None:
            count, mean, m2 = self.sbq_means(*quantizer_metadata)
        mean = np.ascontiguousarray(mean, np.float32)
        m2 = None if m2 is None else np.ascontiguousarray(m2, np.float32)
        vecs = None if vecs is None else np.ascontiguousarray(vecs, np.float32)

        def node(x):
            return self.node_of(*x) if isinstance(x, tuple) else int(x)

        d = IndexDesc()
        d.n, d.dim_index, d.bits, d.words = info.n_nodes, dim_index, bits, info.words
        d.dim_full = dim_index if vecs is None else vecs.shape[1]
        d.num_neighbors, d.distance_type, d.has_labels = info.num_neighbors, distance_type, int(self.has_labels)
        d.default_start = _lib.VS_INVALID_NODE if default_start is None else node(default_start)
        ls = sorted((int(k), node(v)) for k, v in (label_starts or {}).items())
        d.n_label_starts = len(ls)
        lsl = np.array([k for k, _ in ls], np.int16)
        lsn = np.array([v for _, v in ls], np.uint32)
        h.vecs = None if vecs is None else vecs.ctypes.data
        h.mean = mean.ctypes.data
        h.m2 = None if m2 is None else m2.ctypes.data
        h.count = count
        h.label_start_labels = lsl.ctypes.data if ls else None
        h.label_start_nodes = lsn.ctypes.data if ls else None
        out = C.c_void_p()
        check(ctx._L.vs_index_upload(ctx.h, C.byref(d), C.byref(h), C.byref(out)))
        return DiskAnnIndex(ctx, out)

    def close(self):
        if self.h:
            self._L.vs_pages_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DevicePages:
    """The same relation, decoded on the device (vs_pages_dev_*): blocks are copied to HBM as they are, a kernel decodes
    the SbqNode items (label sets included) into the index arrays.  memory_optimized indexes."""

    def __init__(self, ctx, n_blocks_total, page_size=BLCKSZ, layout=None):
        self.ctx = ctx
        self._L = ctx._L
        lay = None if layout is None else NodeLayout(*layout)
        h = C.c_void_p()
        check(self._L.vs_pages_dev_open(ctx.h, page_size, None if lay is None else C.byref(lay), n_blocks_total, C.byref(h)))
        self.h = h
        self.page_size = page_size
        self.n_blocks = 0
        self.info = None

    def add(self, pages, first_block=None):
        buf = np.frombuffer(pages, np.uint8)
        if buf.size % self.page_size:
            raise ValueError(f"{buf.size} bytes is not a whole number of {self.page_size}-byte pages")
        nb = buf.size // self.page_size
        fb = self.n_blocks if first_block is None else first_block
        check(self._L.vs_pages_dev_add(self.h, fb, buf.ctypes.data_as(C.c_void_p), nb))
        self.n_blocks += nb

    def node_of(self, block, offset):
        out = C.c_uint32()
        check(self._L.vs_pages_dev_node_of(self.h, block, offset, C.byref(out)))
        return int(out.value)

    def sbq_means(self, block, offset):
        dim, cnt = C.c_uint32(), C.c_uint64()
        check(self._L.vs_pages_dev_sbq_means(self.h, block, offset, None, None, 0, C.byref(dim), C.byref(cnt)))
        mean = np.empty(dim.value, np.float32)
        m2 = np.empty(dim.value, np.float32)
        check(self._L.vs_pages_dev_sbq_means(self.h, block, offset, mean.ctypes.data_as(C.c_void_p), m2.ctypes.data_as(C.c_void_p),
                                             dim.value, C.byref(dim), C.byref(cnt)))
        return int(cnt.value), mean, m2

    def meta(self, layout=None):
        """MetaPage::fetch on the metadata pages the host kept -> (fields, vs_index_desc, {label: start node})"""
        return _meta_of(self._L.vs_pages_dev_meta, self.h, layout)

    def build_from_meta(self, vecs=None, meta_layout=None):
        m, d, starts = self.meta(meta_layout)
        has_q = m["quantizer_block"] != 0xFFFFFFFF
        return self.build(words=d.words, num_neighbors=d.num_neighbors, dim_index=d.dim_index, bits=d.bits,
                          distance_type=d.distance_type,
                          default_start=None if d.default_start == _lib.VS_INVALID_NODE else int(d.default_start),
                          quantizer_metadata=(m["quantizer_block"], m["quantizer_offset"]) if has_q else None, vecs=vecs,
                          has_labels=bool(m["has_labels"]), label_starts=starts)

    def build(self, *, words, num_neighbors, dim_index, bits, distance_type, default_start, quantizer_metadata=None, mean=None,
              m2=None, count=0, vecs=None, has_labels=False, label_starts=None):
        """default_start / label_starts values: IndexPointer (block, offset) or node id; quantizer_metadata: IndexPointer of
        the SbqMeans chain."""
        from .index import DiskAnnIndex
        if quantizer_metadata is not None:
            count, mean, m2 = self.sbq_means(*quantizer_metadata)
        mean = np.ascontiguousarray(mean, np.float32)
        m2 = None if m2 is None else np.ascontiguousarray(m2, np.float32)
        vecs = None if vecs is None else np.ascontiguousarray(vecs, np.float32)
        d = IndexDesc()
        d.dim_index, d.bits, d.words, d.num_neighbors = dim_index, bits, words, num_neighbors
        d.dim_full = dim_index if vecs is None else vecs.shape[1]

        def node(x):
            return self.node_of(*x) if isinstance(x, tuple) else int(x)

        ls = sorted((int(k), node(v)) for k, v in (label_starts or {}).items())
        lsl = np.array([k for k, _ in ls], np.int16)
        lsn = np.array([v for _, v in ls], np.uint32)
        d.distance_type, d.has_labels, d.n_label_starts, d.storage_type = distance_type, int(bool(has_labels)), len(ls), 0
        d.default_start = _lib.VS_INVALID_NODE if default_start is None else node(default_start)
        h = IndexHost()
        h.label_start_labels = lsl.ctypes.data if ls else None
        h.label_start_nodes = lsn.ctypes.data if ls else None
        h.vecs = None if vecs is None else vecs.ctypes.data
        h.mean = mean.ctypes.data
        h.m2 = None if m2 is None else m2.ctypes.data
        h.count = count
        info = PagesInfo()
        out = C.c_void_p()
        check(self._L.vs_pages_dev_build(self.h, C.byref(d), C.byref(h), C.byref(info), C.byref(out)))
        self.info = info
        return DiskAnnIndex(self.ctx, out)

    def block_table(self):
        """-> (blk_base, blk_cnt) as IndexPages.block_table; the host-side table outlives build()"""
        return _block_table(self._L.vs_pages_dev_block_table, self.h)

    def follower(self, index, layout=None):
        """a PagesFollower of `index` (built from these pages) that starts at this relation's block table"""
        return PagesFollower(index, self.block_table()[1], layout=layout, page_size=self.page_size)

    def close(self):
        if self.h:
            self._L.vs_pages_dev_close(self.h)
            self.h = None


def _block_table(fn, handle):
    pb, pc, nb = C.c_void_p(), C.c_void_p(), C.c_uint32()
    check(fn(handle, C.byref(pb), C.byref(pc), C.byref(nb)))
    n = int(nb.value)
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    as_u32 = lambda p: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), (n,)).copy()
    return as_u32(pb), as_u32(pc)


def dirty_blocks(old_bytes, new_bytes, page_size=BLCKSZ):
    """the blocks of new_bytes that are not, byte for byte, what old_bytes holds at the same place (every block past its end
    included), ascending uint32: what a PagesFollower.stage takes when nothing better (WAL records, the writer's own list)
    names the changed pages"""
    old = np.frombuffer(old_bytes, np.uint8)
    new = np.frombuffer(new_bytes, np.uint8)
    if old.size % page_size or new.size % page_size:
        raise ValueError(f"not a whole number of {page_size}-byte pages")
    nb_old, nb_new = old.size // page_size, new.size // page_size
    both = min(nb_old, nb_new)
    diff = (old[:both * page_size].reshape(both, page_size) != new[:both * page_size].reshape(both, page_size)).any(1)
    return np.concatenate([np.flatnonzero(diff), np.arange(both, nb_new)]).astype(np.uint32)


class PagesFollower:
    """Brings a device-resident index up to date from the blocks of its relation that something else changed
    (vs_pages_follow_*): `stage` checks the listed pages on the device and reports what they would do, `new_tids` names the heap
    tuples of the appended nodes (HeapColumn reads their vectors), `apply` scatters.  The start nodes and the quantizer are not
    read from block 0: decode the MetaPage (decode_meta_page) and call set_start_nodes / set_quantizer after the apply.
    plain=True: a `plain` storage index (vs_pages_follow_open_plain; PlainNode items, blk_cnt as IndexPages(plain=True) reports
    it) — layout is then a plain-layout tuple as PagesOut(plain=True) takes it, and `apply(None)` takes the appended rows' vectors
    from the pages when the index indexes every dimension.  The storage type of `index` does not select the call: the keyword does."""

    def __init__(self, index, blk_cnt, layout=None, page_size=BLCKSZ, plain=False):
        self._L = index._L
        self.index = index
        self.page_size = page_size
        self.plain = bool(plain)
        if layout is not None and plain:
            layout = tuple(0xFFFFFFFF if v is None else v for v in layout)
        lay = None if layout is None else NodeLayout(*layout)
        cnt = np.ascontiguousarray(blk_cnt, np.uint32)
        h = C.c_void_p()
        opener = self._L.vs_pages_follow_open_plain if plain else self._L.vs_pages_follow_open
        check(opener(index.h, page_size, None if lay is None else C.byref(lay), cnt.ctypes.data_as(C.c_void_p), cnt.size, C.byref(h)))
        self.h = h
        self._n_appended = None  # rows the staged list appends (None: nothing is staged)

    def stage(self, blocks, pages, n_blocks_total):
        """blocks: strictly ascending block numbers; pages: their bytes as they are now, in list order -> info dict"""
        b = np.ascontiguousarray(blocks, np.uint32)
        buf = np.frombuffer(pages, np.uint8)
        if buf.size != b.size * self.page_size:
            raise ValueError(f"{buf.size} bytes for {b.size} blocks of {self.page_size} bytes")
        info = PagesFollowInfo()
        self._n_appended = None
        check(self._L.vs_pages_follow_stage(self.h, b.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), b.size, n_blocks_total,
                                            C.byref(info)))
        self._n_appended = int(info.n_appended)
        return info.as_dict()

    def new_tids(self):
        out = np.empty(self._n_appended or 0, np.uint64)
        check(self._L.vs_pages_follow_new_tids(self.h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def apply(self, new_vecs=None):
        """new_vecs [n_appended][dim_full] float32: required when the index holds the vector column and rows are appended — except on
        a plain follower whose index indexes every dimension: None then takes the appended nodes' vectors from the pages"""
        info = PagesFollowInfo()
        v = None if new_vecs is None else np.ascontiguousarray(new_vecs, np.float32).reshape(-1, np.shape(new_vecs)[-1])
        if v is not None and self._n_appended is not None and v.shape[0] != self._n_appended:
            raise ValueError(f"{v.shape[0]} vectors for {self._n_appended} appended rows")
        check(self._L.vs_pages_follow_apply(self.h, None if v is None else v.ctypes.data_as(C.c_void_p), 0 if v is None else v.shape[1],
                                            C.byref(info)))
        self._n_appended = None
        self.index._refresh()
        return info.as_dict()

    def apply_dev(self, d_new_vecs, vec_stride):
        """apply with the appended rows in device memory ([n_appended][vec_stride] floats, e.g. what HeapColumnDev read over
        new_tids()): vs_pages_follow_apply_dev"""
        info = PagesFollowInfo()
        d = d_new_vecs if isinstance(d_new_vecs, C.c_void_p) or d_new_vecs is None else C.c_void_p(d_new_vecs)
        check(self._L.vs_pages_follow_apply_dev(self.h, d, vec_stride, C.byref(info)))
        self._n_appended = None
        self.index._refresh()
        return info.as_dict()

    def discard(self):
        check(self._L.vs_pages_follow_discard(self.h))
        self._n_appended = None

    def close(self):
        if self.h:
            self._L.vs_pages_follow_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PagesBase:
    """What a relation looked like when a PagesOut last wrote it (vs_pages_base): a digest per node page in device memory and
    the host-encoded pages.  Outlives the writer and the index it was taken from."""

    def __init__(self, L, h):
        self._L = L
        self.h = h

    @property
    def n_blocks(self):
        return int(self._L.vs_pages_base_blocks(self.h))

    def close(self):
        if self.h:
            self._L.vs_pages_base_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PagesOut:
    """A device-resident index written out as the pages of a `diskann` index relation (vs_pages_out_*): the layout is fixed here,
    `read` hands out any block range any number of times.  layout: a vs_node_layout 5-tuple (root size, heap pointer, code,
    neighbors, labels / fourth field), meta_layout: a dict as oracle/pages_py.meta_layout() gives.  plain=True: a `plain` storage
    index (vs_pages_out_open_plain; PlainNode items, as IndexPages(plain=True) reads them) — layout is then a plain-layout tuple
    (root size, heap pointer, vector, neighbors, unused)."""

    def __init__(self, index, extension_version="0.8.0", search_list_size=100, max_alpha=1.2, layout=None, meta_layout=None,
                 page_size=BLCKSZ, plain=False):
        self._L = index._L
        self.index = index
        self.page_size = page_size
        self.plain = bool(plain)
        if layout is not None and plain:
            layout = tuple(0xFFFFFFFF if v is None else v for v in layout)
        self._lay = None if layout is None else NodeLayout(*layout)
        self._mlay = _meta_layout(meta_layout)
        p = PagesOutParams()
        p.page_size = page_size
        p.node_layout = None if self._lay is None else C.pointer(self._lay)
        p.meta_layout = None if self._mlay is None else C.pointer(self._mlay)
        p.extension_version = extension_version.encode()
        p.search_list_size, p.max_alpha = search_list_size, max_alpha
        h, info = C.c_void_p(), PagesInfo()
        opener = self._L.vs_pages_out_open_plain if plain else self._L.vs_pages_out_open
        check(opener(index.h, C.byref(p), C.byref(h), C.byref(info)))
        self.h = h
        self.info = info
        self.n_blocks = int(info.n_blocks)

    def read(self, first_block=0, n_blocks=None, out=None):
        """blocks first_block .. first_block + n_blocks - 1 as a uint8 array (into `out` when given)"""
        nb = self.n_blocks - first_block if n_blocks is None else n_blocks
        if out is None:
            out = np.empty(max(nb, 0) * self.page_size, np.uint8)
        assert out.flags["C_CONTIGUOUS"] and out.nbytes >= nb * self.page_size
        check(self._L.vs_pages_out_read(self.h, first_block, nb, out.ctypes.data_as(C.c_void_p)))
        return out

    def read_dev(self, dev_ptr, first_block=0, n_blocks=None):
        """the same into device memory (Context.alloc): the node pages never cross PCIe"""
        nb = self.n_blocks - first_block if n_blocks is None else n_blocks
        check(self._L.vs_pages_out_read_dev(self.h, first_block, nb, dev_ptr))

    def item_pointer_of(self, node):
        b, o = C.c_uint32(), C.c_uint32()
        check(self._L.vs_pages_out_item_pointer_of(self.h, node, C.byref(b), C.byref(o)))
        return int(b.value), int(o.value)

    def baseline(self):
        """the relation exactly as this writer would write it now, as a PagesBase"""
        h = C.c_void_p()
        check(self._L.vs_pages_out_baseline(self.h, C.byref(h)))
        return PagesBase(self._L, h)

    def delta(self, base):
        """-> (blocks, n_blocks_now, new_base): the blocks (ascending uint32) that are not, byte for byte, what `base` recorded,
        the relation's size now, and the baseline of the relation as it is now"""
        nd, nb, h = C.c_uint32(), C.c_uint32(), C.c_void_p()
        check(self._L.vs_pages_out_delta(self.h, base.h, C.byref(nd), C.byref(nb), C.byref(h)))
        new_base = PagesBase(self._L, h)
        blocks = np.empty(int(nd.value), np.uint32)
        check(self._L.vs_pages_out_delta_blocks(self.h, blocks.ctypes.data_as(C.c_void_p), blocks.size))
        return blocks, int(nb.value), new_base

    def read_blocks(self, blocks, out=None):
        """the gathered form of read: page i of the result is block blocks[i] (any order, repeats allowed)"""
        b = np.ascontiguousarray(blocks, np.uint32)
        if out is None:
            out = np.empty(b.size * self.page_size, np.uint8)
        assert out.flags["C_CONTIGUOUS"] and out.nbytes >= b.size * self.page_size
        check(self._L.vs_pages_out_read_blocks(self.h, b.ctypes.data_as(C.c_void_p), b.size, out.ctypes.data_as(C.c_void_p)))
        return out

    def read_blocks_dev(self, dev_ptr, blocks):
        """the same into device memory (Context.alloc)"""
        b = np.ascontiguousarray(blocks, np.uint32)
        check(self._L.vs_pages_out_read_blocks_dev(self.h, b.ctypes.data_as(C.c_void_p), b.size, dev_ptr))

    def patch_file(self, path, base, chunk_blocks=16384):
        """bring the relation file at `path` (as `base` recorded it) up to date in place: the dirty blocks are written where they
        belong, the file is extended or truncated to the relation's size now -> the new baseline"""
        blocks, nb, new_base = self.delta(base)
        ps = self.page_size
        buf = np.empty(min(chunk_blocks, max(blocks.size, 1)) * ps, np.uint8)
        with open(path, "r+b") as f:
            f.truncate(nb * ps)
            for i0 in range(0, blocks.size, chunk_blocks):
                part = blocks[i0:i0 + chunk_blocks]
                self.read_blocks(part, out=buf)
                j = 0
                while j < part.size:  # one write per run of adjacent blocks
                    e = j + 1
                    while e < part.size and part[e] == part[e - 1] + 1:
                        e += 1
                    f.seek(int(part[j]) * ps)
                    f.write(buf[j * ps:e * ps].data)
                    j = e
        return new_base

    def write_file(self, path, chunk_blocks=16384):
        """the relation's main fork as one file, streamed chunk by chunk"""
        buf = np.empty(min(chunk_blocks, max(self.n_blocks, 1)) * self.page_size, np.uint8)
        with open(path, "wb") as f:
            for b0 in range(0, self.n_blocks, chunk_blocks):
                nb = min(chunk_blocks, self.n_blocks - b0)
                f.write(self.read(b0, nb, out=buf)[:nb * self.page_size].data)

    def close(self):
        if self.h:
            self._L.vs_pages_out_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
