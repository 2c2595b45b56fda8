"""Shared cases of the device page decoder's matrix (tests/test_gpu_zx_pages_dev_matrix.py, re-run on the lockstep interpreter by
tests/test_emu_pages_dev.py): index relations manufactured with oracle/pages_py.py, decoded by vs_pages_dev_* (k_pages_decode,
k_pages_labels) and by the host reader (vs_pages.cpp) from the same bytes.  Plain functions taking (gpu_ctx, oracle) and the tables
of cases that name them.  An expectation is never the device's own output: for good pages it is the source arrays AND the host
reader's arrays, for bad pages the host reader's verdict and the table of MALFORMED.  Every comparison is exact."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from oracle import pages_py as PG

SENT = 0xFFFFFFFF
BITS = 2  # W code words = 32 W dimensions of 2 bits
EMU = bool(os.environ.get("VS_EMU"))


# ---- sources and relations -----------------------------------------------------------------------------------------------------------------
def make_source(O, n, W, R, seed, label_counts=None, label_pool=range(-3, 9), degrees=None, vectors=True):
    """n nodes of W code words and R neighbor slots -> dict of the arrays write_index takes, plus vecs / dim.  vectors=True: codes are
    the oracle's quantisation of random vectors (the index can be searched), else random words.  degrees[i] neighbors per row (default:
    random 0..R), label_counts[i] labels per node drawn sorted and distinct from label_pool (None: an unlabeled relation)."""
    rng = np.random.default_rng(seed)
    dim = 32 * W
    labels = 0 if label_counts is None else max(list(label_counts) + [0])
    assert 32 + 8 * W + 8 * R + 2 * labels <= 8100, "the item does not fit an 8 KB page"
    if vectors:
        vecs = rng.standard_normal((n, dim)).astype(np.float32)
        mean, m2, count = O.train(vecs, BITS)
        codes = O.quantize(mean, m2, count, BITS, vecs)
        assert codes.shape == (n, W)
    else:
        vecs = None
        codes = rng.integers(0, 1 << 63, (n, W), dtype=np.uint64) | (rng.integers(0, 2, (n, W), dtype=np.uint64) << np.uint64(63))
        mean, m2, count = rng.standard_normal(dim).astype(np.float32), rng.random(dim).astype(np.float32), n
    nbrs = np.full((n, R), SENT, np.uint32)
    for i in range(n):
        k = int(rng.integers(0, R + 1)) if degrees is None else int(degrees[i])
        k = min(k, n - 1)
        cand = rng.choice(n - 1, size=k, replace=False) if k else np.zeros(0, np.int64)
        cand[cand >= i] += 1  # no self loops
        nbrs[i, :k] = cand
    tids = (rng.integers(0, 1 << 31, n, dtype=np.uint64) << np.uint64(16)) | rng.integers(1, 200, n, dtype=np.uint64)
    tids[rng.random(n) < 0.1] &= ~np.uint64(0xFFFF)
    label_off = label_val = None
    if label_counts is not None:
        pool = np.array(list(label_pool), np.int16)
        label_off, vals = np.zeros(n + 1, np.uint32), []
        for i in range(n):
            vals.extend(sorted(int(v) for v in rng.choice(pool, size=int(label_counts[i]), replace=False)))
            label_off[i + 1] = len(vals)
        label_val = np.array(vals, np.int16)
    return dict(codes=codes, nbrs=nbrs, heap_tids=tids, mean=mean, m2=m2, count=count, label_off=label_off, label_val=label_val,
                vecs=vecs, dim=dim)


def write(src, **kw):
    return PG.write_index(**{k: src[k] for k in ("codes", "nbrs", "heap_tids", "mean", "m2", "count", "label_off", "label_val")}, **kw)


def feeds(nblk, calls):
    """[(first_block, n_blocks)] covering the relation in `calls` calls of add"""
    cuts = [nblk * i // calls for i in range(calls + 1)]
    return [(a, b - a) for a, b in zip(cuts, cuts[1:])]


# ---- the two readers -------------------------------------------------------------------------------------------------------------------------
def read_host(raw, has_labels, layout=None):
    """the host reader over the whole relation -> (arrays, info, reader); raises VsError as vs_pages_add / vs_pages_finish do"""
    from pgvectorscale_amd.pages import IndexPages
    rd = IndexPages(has_labels=has_labels, layout=layout)
    try:
        rd.add(raw)
        info = rd.finish()
        return rd.arrays(), info, rd
    except Exception:
        rd.close()
        raise


def stage(ctx, raw, nblk, calls=1, layout=None):
    from pgvectorscale_amd.pages import DevicePages
    dp = DevicePages(ctx, nblk, layout=layout)
    try:
        for fb, nb in feeds(nblk, calls):
            dp.add(raw[fb * PG.BLCKSZ:(fb + nb) * PG.BLCKSZ], first_block=fb)
    except Exception:
        dp.close()
        raise
    return dp


def start_node(src):
    """the node of the highest degree (the first of them): scans that start there go somewhere"""
    return int((src["nbrs"] != SENT).sum(axis=1).argmax())


def build_args(src, w, has_labels=None, **over):
    n, W = src["codes"].shape
    kw = dict(words=W, num_neighbors=src["nbrs"].shape[1], dim_index=src["dim"], bits=BITS, distance_type=1,
              default_start=w.node_ptrs[start_node(src)] if n else None, mean=src["mean"], m2=src["m2"], count=src["count"], vecs=src["vecs"],
              has_labels=src["label_off"] is not None if has_labels is None else has_labels)
    kw.update(over)
    return kw


def dev_arrays(ctx, ix, labeled):
    """what the device holds, downloaded -> dict like IndexPages.arrays()"""
    from pgvectorscale_amd import _lib
    out = {k: v for k, v in ix.download().items() if v is not None}
    if labeled:
        n = ix.desc.n
        out["label_off"] = ctx.download(ix.array(_lib.ARR_LABEL_OFF)[0], np.empty(n + 1, np.uint32))
        tot = int(out["label_off"][-1])
        out["label_val"] = ctx.download(ix.array(_lib.ARR_LABEL_VAL)[0], np.empty(tot, np.int16)) if tot else np.zeros(0, np.int16)
    return out


def same_arrays(a, b, labeled, what):
    keys = ("codes", "nbrs", "heap_tids") + (("label_off", "label_val") if labeled else ())
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and (x == y).all(), (what, k)


def decode_both(ctx, src, w, raw=None, calls=1, layout=None):
    """the relation through both readers -> (device arrays, host arrays); the quantizer, n and node_of are checked on the way"""
    raw = w.rel.tobytes() if raw is None else raw
    nblk = len(w.rel.pages)
    n = src["codes"].shape[0]
    labeled = src["label_off"] is not None
    host, info, rd = read_host(raw, labeled, layout)
    dp = stage(ctx, raw, nblk, calls, layout)
    try:
        ix = dp.build(**build_args(src, w))
        try:
            assert dp.info.n_nodes == n == info.n_nodes and dp.info.n_blocks == nblk
            for i in sorted({0, n // 2, n - 1} if n else ()):
                assert dp.node_of(*w.node_ptrs[i]) == i == rd.node_of(*w.node_ptrs[i])
            dev = dev_arrays(ctx, ix, labeled)
            mean, m2, cnt = ix.get_quantizer()
            assert (mean == src["mean"]).all() and (m2 == src["m2"]).all() and cnt == src["count"]
            hc, hmean, hm2 = rd.sbq_means(*w.means_ptr)
            dc, dmean, dm2 = dp.sbq_means(*w.means_ptr)
            assert hc == dc == src["count"] and (hmean == dmean).all() and (dmean == src["mean"]).all() and (hm2 == dm2).all() and \
                (dm2 == src["m2"]).all()
        finally:
            ix.close()
    finally:
        dp.close()
        rd.close()
    return dev, host


def check_search(ctx, O, src, w, raw=None, layout=None):
    """8 scans of the index built from the pages return the oracle's rows (ids, heap tids, visited nodes)"""
    R = src["nbrs"].shape[1]
    orc = O.OracleIndex(codes=src["codes"], nbrs=src["nbrs"], heap_tids=src["heap_tids"], vecs=src["vecs"], mean=src["mean"],
                        m2=src["m2"], count=src["count"], bits=BITS, dim_index=src["dim"], num_neighbors=R, distance_type=1,
                        default_start=start_node(src), label_off=src["label_off"], label_val=src["label_val"], label_starts={})
    q = np.random.default_rng(77).standard_normal((8, src["dim"])).astype(np.float32)
    dp = stage(ctx, w.rel.tobytes() if raw is None else raw, len(w.rel.pages), layout=layout)
    try:
        ix = dp.build(**build_args(src, w))
    finally:
        dp.close()
    try:
        gi, gt, gd, gst = ix.search_batch(q, search_list_size=20, rescore=10, k=5)
    finally:
        ix.close()
    oi, od, ost = orc.search_batch(q, L=20, rescore=10, k=5)
    assert (oi != SENT).all() and ost["visited_nodes"] >= 8 * 20, "the fabricated graph gives the scans nothing to do"
    assert (gi == oi).all() and gst["visited_nodes"] == ost["visited_nodes"]
    ok = oi != SENT
    assert (gt[ok] == src["heap_tids"][oi[ok]]).all()


def differential(ctx, O, src, w, calls=1, layout=None, search=True):
    dev, host = decode_both(ctx, src, w, calls=calls, layout=layout)
    labeled = src["label_off"] is not None
    same_arrays(dev, src, labeled, "device vs source")
    same_arrays(dev, host, labeled, "device vs host reader")
    assert (dev["nbrs"][src["nbrs"] == SENT] == SENT).all()  # (the sentinel tail, said once more in words)
    if search and src["vecs"] is not None:
        check_search(ctx, O, src, w, layout=layout)
    return dev


# ---- 2. well-formed pages ------------------------------------------------------------------------------------------------------------------
def case_one_trip(ctx, O):
    src = make_source(O, 300, 4, 32, seed=1)
    w = write(src, zero_page_every=97, means_first=False)
    assert sum(1 for p in w.rel.pages if not any(p[:24])) == 3 and w.means_ptr[0] > w.node_ptrs[-1][0]
    differential(ctx, O, src, w)


def case_w_boundary(W):
    def run(ctx, O):
        src = make_source(O, 120, W, 10, seed=W, vectors=False)
        differential(ctx, O, src, write(src))
    return run


def case_w_long(ctx, O):
    src = make_source(O, 64, 250, 7, seed=3, label_counts=np.arange(64) % 4, vectors=False)
    w = write(src)
    assert sum(1 for b in range(len(w.rel.pages)) if w.rel.page_type(b) == PG.PT_SBQ_MEANS) >= 8  # 8000 dimensions: 64 KB of means
    differential(ctx, O, src, w)


def case_r_boundary(R):
    def run(ctx, O):
        n = 200
        edges = [d for d in (0, 1, 62, 63, 64, 65, 66, 126, 127, 128, 129, R - 2, R - 1) if d <= R]  # around every wave boundary
        deg = [R if i % 2 == 0 else edges[i // 2] if i // 2 < len(edges) else (i * 7) % (R + 1) for i in range(n)]
        src = make_source(O, n, 2, R, seed=R, degrees=deg)
        differential(ctx, O, src, write(src))
    return run


def case_many_labels(ctx, O):
    counts = [(0, 1, 63, 64, 65, 130)[i % 6] for i in range(150)]
    src = make_source(O, 150, 2, 12, seed=5, label_counts=counts, label_pool=range(-100, 100))
    assert src["label_val"].min() < 0 < src["label_val"].max() and len(set(src["label_val"].tolist())) == 200
    differential(ctx, O, src, write(src))


def case_empty_sets(ctx, O):
    src = make_source(O, 90, 3, 8, seed=6, label_counts=[0] * 90)
    dev = differential(ctx, O, src, write(src))
    assert dev["label_off"].shape == (91,) and not dev["label_off"].any() and dev["label_val"].size == 0


def case_layout(ctx, O):
    import pgvectorscale_amd as P
    layout = (40, 32, 16, 0, 8)  # root size 40: neighbors | labels | bq_vector | (pad) | heap pointer
    src = make_source(O, 200, 3, 10, seed=11, label_counts=np.random.default_rng(11).integers(0, 7, 200))
    w = write(src, layout=layout)
    differential(ctx, O, src, w, layout=layout)
    # the same bytes under the default layout: refused by both readers (on the interpreter: without touching a guard page)
    with pytest.raises(P.VsError):
        read_host(w.rel.tobytes(), True)
    dp = stage(ctx, w.rel.tobytes(), len(w.rel.pages))
    try:
        with pytest.raises(P.VsError, match=r"block \d+ item \d+: "):
            dp.build(**build_args(src, w))
    finally:
        dp.close()


def case_tiny(ctx, O):
    src = make_source(O, 1, 1, 1, seed=8, vectors=False)
    dev = differential(ctx, O, src, write(src))
    assert dev["nbrs"].tolist() == [[SENT]]


def case_no_nodes(ctx, O):
    """n = 0, only the meta chain: the host reader gives an empty relation (tests/test_pages.py::test_empty_relation), and so does
    the device — an index of no rows is BUILT, not refused."""
    rel = PG.Relation()
    meta = PG.ChainTapeWriter(rel, PG.PT_META)
    meta.write(PG.rkyv_meta_header())
    meta.write(b"\0" * 64)
    host, info, rd = read_host(rel.tobytes(), False)
    rd.close()
    assert info.n_nodes == 0 and host["codes"].size == 0
    dp = stage(ctx, rel.tobytes(), 1)
    try:
        ix = dp.build(words=1, num_neighbors=1, dim_index=32, bits=BITS, distance_type=1, default_start=None,
                      mean=np.zeros(32, np.float32), m2=np.ones(32, np.float32), count=0)
        try:
            assert dp.info.n_nodes == 0 and ix.desc.n == 0
            dev = ix.download()
            assert dev["codes"].shape == (0, 1) and dev["nbrs"].shape == (0, 1) and dev["heap_tids"].shape == (0,)
        finally:
            ix.close()
    finally:
        dp.close()


def case_chunks(ctx, O):
    src = make_source(O, 300, 4, 32, seed=9, label_counts=np.random.default_rng(9).integers(0, 5, 300))
    w = write(src)
    nblk = len(w.rel.pages)
    assert nblk > 3
    first = None
    for calls in (1, 3, nblk):
        dev = differential(ctx, O, src, w, calls=calls, search=calls == 3)
        first = first or dev
        same_arrays(dev, first, True, f"{calls} calls of add vs one")


GOOD = {"one_trip": case_one_trip, "w64": case_w_boundary(64), "w65": case_w_boundary(65), "w_long": case_w_long,
        "r64": case_r_boundary(64), "r65": case_r_boundary(65), "r128": case_r_boundary(128), "r130": case_r_boundary(130),
        "many_labels": case_many_labels, "empty_sets": case_empty_sets, "layout": case_layout, "tiny": case_tiny,
        "no_nodes": case_no_nodes, "chunks": case_chunks}

# ---- the end of a neighbor list ------------------------------------------------------------------------------------------------------------
LIST_END_SLOTS = (0, 1, 62, 63, 64, 65, 127, 128, 129)
_cache = {}


def _list_end_relation(O):
    if "list_end" not in _cache:
        src = make_source(O, 150, 2, 130, seed=13, degrees=[130] * 150, vectors=False)
        assert (src["nbrs"] != SENT).all()
        _cache["list_end"] = (src, write(src))
    return _cache["list_end"]


def nbr_slots_at(w, raw, node, layout=PG.DEFAULT_NODE_LAYOUT):
    """byte position of neighbor slot 0 of `node` inside the relation's bytes, and the slot count"""
    blk, off = w.node_ptrs[node]
    s, l = w.rel.item_span(blk, off)
    fld = blk * PG.BLCKSZ + s + l - layout[0] + layout[3]
    rel_off, cnt = struct.unpack_from("<iI", raw, fld)
    return fld + rel_off, cnt


def case_list_end(s):
    def run(ctx, O):
        src, w = _list_end_relation(O)
        raw = bytearray(w.rel.tobytes())
        at, cnt = nbr_slots_at(w, raw, 7)
        assert cnt == 130
        raw[at + 8 * s:at + 8 * s + 8] = PG.rkyv_item_pointer(PG.INVALID_BLOCK, 0)
        if s + 1 < cnt:  # bytes after the end of the list: ignored, and not reported as dangling
            raw[at + 8 * (s + 1):at + 8 * (s + 1) + 8] = PG.rkyv_item_pointer(0, 1)
        want = src["nbrs"].copy()
        want[7, s:] = SENT
        dev, host = decode_both(ctx, src, w, raw=bytes(raw))
        assert (dev["nbrs"][7, :s] == src["nbrs"][7, :s]).all() and (dev["nbrs"][7, s:] == SENT).all()
        assert (dev["nbrs"][8] == src["nbrs"][8]).all()
        expect = dict(src, nbrs=want)
        same_arrays(dev, expect, False, "device vs source")
        same_arrays(host, expect, False, "host reader vs source")
    return run


# ---- 3. malformed pages ----------------------------------------------------------------------------------------------------------------------
# One relation of 60 nodes (W = 2, R = 6, up to four labels) on blocks meta | means | never-initialised | nodes: the node page is the
# LAST block of the staged buffer.  The corrupted item is node 40 ("mid"), the last item of the last node page ("last", node 59: it
# lies at pd_upper) or the page's first item ("edge", node 0: the item that ends at pd_special, eight bytes from the end of the staged
# buffer — where a read past the item leaves the allocation).  All three carry exactly two labels, so the items are 100 bytes long and
# 4 bytes of alignment padding follow each.
MAL_NODES = {"mid": 40, "last": 59, "edge": 0}
LP, BOUNDS, SHORT, VEC, WIDTH, SLOTS, DANGLING, LABELS, UNALIGNED = (
    "line pointer is not LP_NORMAL", r"item lies outside pd_upper\.\.pd_special", "item shorter than the archived node",
    "ArchivedVec points outside the item", "bq_vector length differs from the index's code width",
    "neighbor slot count differs from the index's num_neighbors", "neighbor points at something that is not an SbqNode item of this relation",
    "label set is not strictly increasing", "item or ArchivedVec is not 4-byte aligned")
# what the host reader says for the same reason (its texts carry more detail)
HOST_TEXT = {LP: "is not LP_NORMAL", BOUNDS: r"lies outside pd_upper\.\.pd_special", SHORT: "item shorter than the archived node",
             VEC: "points outside the item", WIDTH: "code width", SLOTS: "neighbor slot count", DANGLING: "not an SbqNode item",
             LABELS: "strictly increasing"}


def _mal_relation(O):
    if "mal" not in _cache:
        counts = np.random.default_rng(2).integers(0, 5, 60)
        for node in MAL_NODES.values():
            counts[node] = 2
        src = make_source(O, 60, 2, 6, seed=2, label_counts=counts, vectors=False)
        w = write(src, zero_page_every=30)
        rel = w.rel
        assert len(rel.pages) == 4 and rel.page_type(1) == PG.PT_SBQ_MEANS and rel.max_offset(2) == 60 and not any(rel.pages[3])
        # move the node page behind the never-initialised block: every neighbor pointer follows it
        rel.pages[2], rel.pages[3] = rel.pages[3], rel.pages[2]
        w.node_ptrs = [(3, off) for _, off in w.node_ptrs]
        patched = bytearray(rel.tobytes())
        for i in range(60):
            at, cnt = nbr_slots_at(w, patched, i)
            for j in range(cnt):
                b, o, _ = struct.unpack_from("<IHH", patched, at + 8 * j)
                if b != PG.INVALID_BLOCK:
                    assert b == 2
                    patched[at + 8 * j:at + 8 * j + 8] = PG.rkyv_item_pointer(3, o)
        rel.pages[3] = patched[3 * PG.BLCKSZ:]
        raw = rel.tobytes()
        host, info, rd = read_host(raw, True)
        rd.close()
        same_arrays(host, src, True, "host reader vs source")
        _cache["mal"] = (src, w, raw)
    return _cache["mal"]


class _Item:
    """where one item of the malformed relation lies: page base, line pointer, span, the three ArchivedVec fields"""

    def __init__(self, w, raw, node):
        self.blk, self.off = w.node_ptrs[node]
        self.base = self.blk * PG.BLCKSZ
        self.lp_at = self.base + 24 + 4 * (self.off - 1)
        self.s, self.l = w.rel.item_span(self.blk, self.off)
        root = self.base + self.s + self.l - 32
        self.f_code, self.f_nbr, self.f_lab = root + 8, root + 16, root + 24
        self.upper, self.special = struct.unpack_from("<HH", raw, self.base + 14)
        self.nblk = len(w.rel.pages)

    def fld_in_item(self, f):
        return f - self.base - self.s


def _set_lp(raw, it, off=None, flags=1, length=None):
    off = it.s if off is None else off
    length = it.l if length is None else length
    struct.pack_into("<I", raw, it.lp_at, off | (flags << 15) | (length << 17))


def _vec_off(raw, f, value=None, delta=None):
    cur = struct.unpack_from("<i", raw, f)[0]
    struct.pack_into("<i", raw, f, cur + delta if value is None else value)


def _vec_len(raw, f, n):
    struct.pack_into("<I", raw, f + 4, n)


def _ends_past(raw, it, f, elem):
    """move the ArchivedVec's target so that its last element ends 8 bytes past the item"""
    n = struct.unpack_from("<I", raw, f + 4)[0]
    _vec_off(raw, f, value=it.l + 8 - n * elem - it.fld_in_item(f))


def _nbr0(raw, it, ptr):
    at = it.f_nbr + struct.unpack_from("<i", raw, it.f_nbr)[0]
    raw[at:at + 8] = PG.rkyv_item_pointer(*ptr)


def _labels(raw, it, fn):
    at = it.f_lab + struct.unpack_from("<i", raw, it.f_lab)[0]
    a, b = struct.unpack_from("<hh", raw, at)
    struct.pack_into("<hh", raw, at, *fn(a, b))


def _shift_item(raw, it):
    """the whole item two bytes up, into its alignment padding, and the line pointer with it: the host reader decodes the same node"""
    assert it.l % 8 == 4
    a = it.base + it.s
    raw[a + 2:a + 2 + it.l] = raw[a:a + it.l]
    _set_lp(raw, it, off=it.s + 2)


# name -> (row of the issue's table, what to change, the device's reason, what the host reader does: None = the same reason, "accepts")
MALFORMED = {
    "lp_unused": (1, lambda r, it: _set_lp(r, it, flags=0), LP, None),
    "lp_redirect": (1, lambda r, it: _set_lp(r, it, flags=2), LP, None),
    "lp_dead": (1, lambda r, it: _set_lp(r, it, flags=3), LP, None),
    "lp_len_0": (1, lambda r, it: _set_lp(r, it, length=0), LP, None),
    "item_below_upper": (2, lambda r, it: _set_lp(r, it, off=it.upper - 8), BOUNDS, None),
    "item_past_special": (3, lambda r, it: _set_lp(r, it, off=it.special + 8 - it.l), BOUNDS, None),
    "item_short": (4, lambda r, it: _set_lp(r, it, off=it.s + it.l - 24, length=24), SHORT, None),
    "code_off_negative": (5, lambda r, it: _vec_off(r, it.f_code, value=-100000), VEC, None),
    "code_ends_past_item": (6, lambda r, it: _ends_past(r, it, it.f_code, 8), VEC, None),
    "nbr_ends_past_item": (7, lambda r, it: _ends_past(r, it, it.f_nbr, 8), VEC, None),
    "code_len_1": (8, lambda r, it: _vec_len(r, it.f_code, 1), WIDTH, None),
    "code_len_w_plus_1": (8, lambda r, it: _vec_len(r, it.f_code, 3), WIDTH, None),
    "nbr_len_r_minus_1": (9, lambda r, it: _vec_len(r, it.f_nbr, 5), SLOTS, None),
    "nbr_len_r_plus_1": (9, lambda r, it: _vec_len(r, it.f_nbr, 7), SLOTS, None),
    "nbr_to_item_200": (10, lambda r, it: _nbr0(r, it, (it.blk, 200)), DANGLING, None),
    "nbr_to_meta_page": (10, lambda r, it: _nbr0(r, it, (0, 1)), DANGLING, None),
    "nbr_to_zero_page": (10, lambda r, it: _nbr0(r, it, (2, 1)), DANGLING, None),
    "nbr_to_means_page": (10, lambda r, it: _nbr0(r, it, (1, 1)), DANGLING, None),
    "nbr_to_block_nblk": (10, lambda r, it: _nbr0(r, it, (it.nblk, 1)), DANGLING, None),
    "nbr_to_offset_0": (10, lambda r, it: _nbr0(r, it, (it.blk, 0)), DANGLING, None),
    "labels_off_negative": (11, lambda r, it: _vec_off(r, it.f_lab, value=-100000), VEC, None),
    "labels_len_5000": (11, lambda r, it: _vec_len(r, it.f_lab, 5000), VEC, None),
    "labels_swapped": (12, lambda r, it: _labels(r, it, lambda a, b: (b, a)), LABELS, None),
    "labels_equal": (12, lambda r, it: _labels(r, it, lambda a, b: (a, a)), LABELS, None),
    "item_unaligned": (13, _shift_item, UNALIGNED, "accepts"),
    "code_unaligned": (14, lambda r, it: _vec_off(r, it.f_code, delta=2), UNALIGNED, "accepts"),
}


def good_build(ctx, src, w, raw):
    dp = stage(ctx, raw, len(w.rel.pages))
    try:
        ix = dp.build(**build_args(src, w))
    finally:
        dp.close()
    try:
        same_arrays(dev_arrays(ctx, ix, src["label_off"] is not None), src, src["label_off"] is not None, "a good build after a refusal")
    finally:
        ix.close()


def case_malformed(name, where):
    def run(ctx, O):
        import pgvectorscale_amd as P
        row, damage, reason, host_does = MALFORMED[name]
        src, w, good = _mal_relation(O)
        node = MAL_NODES[where]
        raw = bytearray(good)
        it = _Item(w, raw, node)
        assert it.blk == len(w.rel.pages) - 1 and (where != "last" or it.off == w.rel.max_offset(it.blk)) and \
            (where != "edge" or it.s + it.l + 4 == it.special)
        damage(raw, it)
        raw = bytes(raw)
        assert sum(a != b for a, b in zip(raw, good)) > 0
        # the host reader's verdict
        if host_does == "accepts":
            host, _, rd = read_host(raw, True)
            rd.close()
            if name == "item_unaligned":
                same_arrays(host, src, True, "host reader vs source")
            else:  # the code words as the shifted bytes spell them; everything else as written
                at = it.f_code + struct.unpack_from("<i", raw, it.f_code)[0]
                want = dict(src, codes=src["codes"].copy())
                want["codes"][node] = np.frombuffer(raw, "<u8", 2, at)
                same_arrays(host, want, True, "host reader vs source")
        else:
            with pytest.raises(P.VsError) as e:
                read_host(raw, True)
            if where != "edge":  # (the page's first item also gives the host reader its geometry: refused, in other words)
                assert (f"node {node} neighbor slot 0 " if reason == DANGLING else f"block {it.blk} item {it.off}: ") in str(e.value)
                assert re.search(HOST_TEXT[reason], str(e.value)), str(e.value)
        # the device's
        dp = stage(ctx, raw, it.nblk)
        try:
            with pytest.raises(P.VsError, match=reason) as e:
                dp.build(**build_args(src, w))
            assert f"block {it.blk} item {it.off}: " in str(e.value), str(e.value)
        finally:
            dp.close()  # the same handle closes cleanly
        good_build(ctx, src, w, good)
    return run


# ---- wrong geometry and call sequence --------------------------------------------------------------------------------------------------------
def live_allocations():
    """device and pinned allocations alive on the interpreter (tests/emu counts every hipMalloc / hipHostMalloc); 0 on hardware, where
    there is no such counter and the sequence only has to run"""
    if not EMU:
        return 0
    from conftest import EMU_LIB
    lib = C.CDLL(EMU_LIB)
    lib.vs_emu_live_allocations.restype = C.c_size_t
    return int(lib.vs_emu_live_allocations())


def _refused(ctx, src, w, raw, match, layout=None, **over):
    import pgvectorscale_amd as P
    before = live_allocations()
    dp = stage(ctx, raw, len(w.rel.pages), layout=layout)
    try:
        with pytest.raises(P.VsError, match=match):
            dp.build(**build_args(src, w, **over))
        with pytest.raises(P.VsError):  # the raw pages are gone with the refusal
            dp.add(raw[:PG.BLCKSZ], first_block=0)
    finally:
        dp.close()
    assert live_allocations() == before, "an array of the refused index, or the staged pages, outlived the refusal"


def _geometry_relation(O):
    if "geo" not in _cache:
        src = make_source(O, 60, 2, 6, seed=21, vectors=False)
        w = write(src)
        _cache["geo"] = (src, w, w.rel.tobytes())
    return _cache["geo"]


def case_wrong_words(ctx, O):
    src, w, raw = _geometry_relation(O)
    good_build(ctx, src, w, raw)  # (the context's own lazily created resources come first)
    _refused(ctx, src, w, raw, WIDTH, words=3, dim_index=96, mean=np.zeros(96, np.float32), m2=np.ones(96, np.float32))
    good_build(ctx, src, w, raw)


def case_wrong_num_neighbors(ctx, O):
    src, w, raw = _geometry_relation(O)
    good_build(ctx, src, w, raw)
    _refused(ctx, src, w, raw, SLOTS, num_neighbors=5)
    good_build(ctx, src, w, raw)


def case_labels_on_unlabeled_pages(ctx, O):
    """has_labels = 1 over a relation of classic nodes.  A classic node's fourth field is its always-empty `_neighbor_vectors`
    (AM/sbq/node.rs:82), byte for byte a labeled node's empty label set — the empty_sets case above, which must build.  So the verdict
    is the host reader's: both readers decode every set as empty.  What IS refused, with a reason and with nothing left allocated, is a
    caller who hands over the classic layout (no labels field) and asks for labels."""
    from pgvectorscale_amd.pages import IndexPages
    src, w, raw = _geometry_relation(O)
    good_build(ctx, src, w, raw)
    host, info, rd = read_host(raw, True)
    rd.close()
    assert not host["label_off"].any() and host["label_val"].size == 0
    dp = stage(ctx, raw, len(w.rel.pages))
    try:
        ix = dp.build(**build_args(src, w, has_labels=True))
    finally:
        dp.close()
    try:
        dev = dev_arrays(ctx, ix, True)
    finally:
        ix.close()
    same_arrays(dev, dict(src, label_off=host["label_off"], label_val=host["label_val"]), True, "device vs source")
    same_arrays(dev, host, True, "device vs host reader")
    import pgvectorscale_amd as P
    before = live_allocations()
    dp = stage(ctx, raw, len(w.rel.pages), layout=IndexPages.default_layout(False))
    try:
        with pytest.raises(P.VsError, match="no labels field"):
            dp.build(**build_args(src, w, has_labels=True))
    finally:
        dp.close()
    assert live_allocations() == before
    good_build(ctx, src, w, raw)


def case_call_sequence(ctx, O):
    import pgvectorscale_amd as P
    from pgvectorscale_amd.pages import DevicePages, IndexPages
    src, w, raw = _geometry_relation(O)
    nblk = len(w.rel.pages)
    one = raw[:PG.BLCKSZ]
    good_build(ctx, src, w, raw)
    before = live_allocations()
    # add after build, a second build
    dp = stage(ctx, raw, nblk)
    try:
        ix = dp.build(**build_args(src, w))
        ix.close()
        with pytest.raises(P.VsError, match="vs_pages_dev_add after vs_pages_dev_build"):
            dp.add(one, first_block=nblk)
        with pytest.raises(P.VsError, match="already built"):
            dp.build(**build_args(src, w))
    finally:
        dp.close()
    # more blocks than the reader was opened for
    dp = stage(ctx, raw, nblk)
    try:
        with pytest.raises(P.VsError, match=f"more blocks than vs_pages_dev_open was told \\({nblk}\\)"):
            dp.add(one, first_block=nblk)
    finally:
        dp.close()
    # a first_block out of order: whatever vs_pages_add says to the same call
    rd = IndexPages()
    with pytest.raises(P.VsError) as host:
        rd.add(one, first_block=2)
    rd.close()
    dp = DevicePages(ctx, nblk)
    try:
        with pytest.raises(P.VsError) as dev:
            dp.add(one, first_block=2)
        assert str(dev.value) == str(host.value) and "in order" in str(dev.value)
        dp.add(raw)  # the refused call left the reader usable
        ix = dp.build(**build_args(src, w))
        try:
            same_arrays(dev_arrays(ctx, ix, False), src, False, "after a refused add")
        finally:
            ix.close()
    finally:
        dp.close()
    assert live_allocations() == before


SEQUENCE = {"wrong_words": case_wrong_words, "wrong_num_neighbors": case_wrong_num_neighbors,
            "labels_on_unlabeled_pages": case_labels_on_unlabeled_pages, "call_sequence": case_call_sequence}
