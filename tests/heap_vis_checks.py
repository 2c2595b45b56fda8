"""Shared fabricators of the heap-visibility tests (tests/test_gpu_zx_heap_vis.py) and a scalar Python restatement of the rule the
device evaluates (include/vsgpu.h: HeapTupleSatisfiesMVCC inside heap_hot_search_buffer, PostgreSQL 13-17).  Pages are made with
oracle/heap_py.py: tuples from form_tuple whose header bytes are patched here, line pointers from set_line_pointer.  Expectations
never come from the device."""
import struct

import numpy as np

from oracle import heap_py as HP

ONE_COL = [(-1, "i")]  # a table of nothing but a two-dimensional vector: 185 rows on an 8 KB page
INVALID, STATE = -1, -5

# t_infomask / t_infomask2
KEYSHR_LOCK, COMBOCID, EXCL_LOCK, LOCK_ONLY = 0x0010, 0x0020, 0x0040, 0x0080
XMIN_COMMITTED, XMIN_INVALID, FROZEN = 0x0100, 0x0200, 0x0300
XMAX_COMMITTED, XMAX_INVALID, IS_MULTI = 0x0400, 0x0800, 0x1000
MOVED_OFF, MOVED_IN = 0x4000, 0x8000
HOT_UPDATED, ONLY_TUPLE = 0x4000, 0x8000
REASONS = ("multixact", "subcommitted", "clog_range", "combocid", "moved", "suboverflow")  # VS_VIS_R_* in order
IN_PROGRESS, COMMITTED, ABORTED, SUB_COMMITTED = 0, 1, 2, 3
M32 = 0xFFFFFFFF


def tup(xmin, xmax=0, cid=0, m=0, m2=0, ctid_off=0):
    """a heap tuple of the one-column table with the given header: m / m2 are OR-ed into t_infomask / t_infomask2"""
    t = bytearray(HP.form_tuple(ONE_COL, [("inline", HP.vector_datum_body([1.0, 2.0]))]))
    struct.pack_into("<III", t, 0, xmin & M32, xmax & M32, cid & M32)
    struct.pack_into("<H", t, 16, ctid_off)
    struct.pack_into("<H", t, 18, 1 | m2)       # one attribute
    struct.pack_into("<H", t, 20, 0x0002 | m)   # HEAP_HASVARWIDTH
    return bytes(t)


def tid_of(blk, off):
    return (blk << 16) | off


def patch_header(rel, tid, **kw):
    """rewrite header fields of the tuple behind a tid in place (what an UPDATE / DELETE does to the old version)"""
    blk, off = tid >> 16, tid & 0xFFFF
    p = rel.pages[blk]
    lp = struct.unpack_from("<I", p, HP.SIZE_OF_PAGE_HEADER + 4 * (off - 1))[0]
    at = lp & 0x7FFF
    for k, (o, f) in {"xmin": (0, "<I"), "xmax": (4, "<I"), "cid": (8, "<I"), "ctid_off": (16, "<H"), "m2": (18, "<H"), "m": (20, "<H")}.items():
        if k in kw:
            v = kw[k] | (1 if k == "m2" else 0x0002 if k == "m" else 0)
            struct.pack_into(f, p, at + o, v & (M32 if f == "<I" else 0xFFFF))


class Clog:
    """a window of pg_xact: 2 bits per xid"""

    def __init__(self, first_xid, n_xids, default=IN_PROGRESS):
        assert first_xid % 4 == 0
        self.first, self.n = first_xid & M32, n_xids
        self.st = np.full(n_xids, default, np.uint8)

    def set(self, xid, status):
        i = (xid - self.first) & M32
        assert i < self.n, hex(xid)
        self.st[i] = status

    def get(self, xid):
        i = (xid - self.first) & M32
        return None if i >= self.n else int(self.st[i])

    def xact(self):
        s = np.zeros((self.n + 3) // 4 * 4, np.uint8)
        s[:self.n] = self.st
        s = s.reshape(-1, 4)
        return self.first, self.n, (s[:, 0] | (s[:, 1] << 2) | (s[:, 2] << 4) | (s[:, 3] << 6)).astype(np.uint8)


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------------
class Undecided(Exception):
    def __init__(self, reason):
        self.reason = reason


class Malformed(Exception):
    def __init__(self, blk, off, why):
        super().__init__(f"block {blk} item {off}: {why}")
        self.blk, self.off, self.why = blk, off, why


def _s32(x):
    x &= M32
    return x - (1 << 32) if x & 0x80000000 else x


def precedes(a, b):
    return _s32(a - b) < 0 if a >= 3 and b >= 3 else a < b


def follows_eq(a, b):
    return _s32(a - b) >= 0 if a >= 3 and b >= 3 else a >= b


def locked_only(m):
    return bool(m & LOCK_ONLY) or (m & (IS_MULTI | EXCL_LOCK | KEYSHR_LOCK)) == EXCL_LOCK


def did_commit(clog, x):
    if x in (1, 2):
        return True
    if x == 0:
        return False
    st = clog.get(x)
    if st is None:
        raise Undecided("clog_range")
    if st == SUB_COMMITTED:
        raise Undecided("subcommitted")
    return st == COMMITTED


def in_snapshot(s, x):
    if precedes(x, s["xmin"]):
        return False
    if follows_eq(x, s["xmax"]):
        return True
    xip, subxip = set(s.get("xip", ())), set(s.get("subxip", ()))
    if not s.get("taken_during_recovery"):
        if not s.get("suboverflowed"):
            return x in subxip or x in xip
        if x in xip:
            return True
        raise Undecided("suboverflow")
    if x in subxip:
        return True
    if s.get("suboverflowed"):
        raise Undecided("suboverflow")
    return False


def satisfies_mvcc(s, clog, xmin, xmax, cid, m):
    own = set(s.get("own_xids", ()))
    curcid = s.get("curcid", 0)
    if not m & XMIN_COMMITTED:
        if (m & FROZEN) == XMIN_INVALID:
            return False
        if m & (MOVED_OFF | MOVED_IN):
            raise Undecided("moved")
        if xmin in own:
            if m & COMBOCID:
                raise Undecided("combocid")
            if cid >= curcid:
                return False
            if m & XMAX_INVALID or locked_only(m):
                return True
            if m & IS_MULTI:
                raise Undecided("multixact")
            if xmax not in own:
                return True
            return cid >= curcid
        elif in_snapshot(s, xmin):
            return False
        elif not did_commit(clog, xmin):
            return False
    elif (m & FROZEN) != FROZEN and in_snapshot(s, xmin):
        return False
    if m & XMAX_INVALID or locked_only(m):
        return True
    if m & IS_MULTI:
        raise Undecided("multixact")
    if not m & XMAX_COMMITTED:
        if xmax in own:
            if m & COMBOCID:
                raise Undecided("combocid")
            return cid >= curcid
        if in_snapshot(s, xmax):
            return True
        if not did_commit(clog, xmax):
            return True
    elif in_snapshot(s, xmax):
        return True
    return False


def page_view(page, page_size, blk, off):
    lower, upper, special, psv = struct.unpack_from("<HHHH", page, 12)
    if upper == 0:
        return 0, 0, 0
    if (psv & 0xFF00) != page_size:
        raise Malformed(blk, off, "page size")
    if not (24 <= lower <= upper <= special <= page_size):
        raise Malformed(blk, off, "page header")
    return upper, special, (lower - 24) // 4


def hot_search(pages, page_size, n_blocks, tid, s, clog):
    """-> (kind, hops): kind in visible | invisible | deleted | not_found | dead_lp | one of REASONS"""
    blk, off = tid >> 16, tid & 0xFFFF
    if off == 0:
        return "deleted", 0
    if blk >= n_blocks:
        return "not_found", 0
    page = pages[blk]
    upper, special, nitems = page_view(page, page_size, blk, off)
    at_start, prev_xmax, members, rnd = True, 0, 0, 0
    while True:
        if not 1 <= off <= nitems:
            return ("not_found" if rnd == 0 else "invisible"), max(members - 1, 0)
        if rnd >= nitems:
            raise Malformed(blk, off, "cycle")
        lp = struct.unpack_from("<I", page, 24 + 4 * (off - 1))[0]
        lp_off, fl, lp_len = lp & 0x7FFF, (lp >> 15) & 3, lp >> 17
        if fl != HP.LP_NORMAL:
            if fl == HP.LP_REDIRECT and at_start:
                off, at_start, rnd = lp_off, False, rnd + 1
                continue
            return ("dead_lp" if rnd == 0 else "invisible"), max(members - 1, 0)
        if lp_off < upper or lp_off + lp_len > special or lp_len < 23:
            raise Malformed(blk, off, "item bounds")
        xmin, xmax, cid = struct.unpack_from("<III", page, lp_off)
        ctid_off, m2, m = struct.unpack_from("<HHH", page, lp_off + 16)
        members += 1
        hops = members - 1
        if at_start and m2 & ONLY_TUPLE:
            return "invisible", hops
        if prev_xmax != 0 and prev_xmax != (2 if (m & FROZEN) == FROZEN else xmin):
            return "invisible", hops
        try:
            if satisfies_mvcc(s, clog, xmin, xmax, cid, m):
                return "visible", hops
        except Undecided as u:
            return u.reason, hops
        if m2 & HOT_UPDATED and not m & XMAX_INVALID and (m & FROZEN) != XMIN_INVALID:
            if m & IS_MULTI and not locked_only(m):
                return "multixact", hops
            off, at_start, prev_xmax, rnd = ctid_off, False, xmax, rnd + 1
        else:
            return "invisible", hops


def empty_stats():
    d = {k: 0 for k in ("n_visible", "n_invisible", "n_undecided", "n_deleted", "n_not_found", "n_dead_line_pointer", "chain_hops")}
    d["undecided_by_reason"] = {r: 0 for r in REASONS}
    return d


def ref_visibility(pages, page_size, n_blocks, tids, s, clog):
    """the whole evaluation -> (mask uint8 [n], stats as VisStats.as_dict gives them, undecided nodes ascending, kind per node)"""
    mask = np.zeros(len(tids), np.uint8)
    st, und, kinds = empty_stats(), [], []
    for i, tid in enumerate(tids):
        kind, hops = hot_search(pages, page_size, n_blocks, int(tid), s, clog)
        kinds.append(kind)
        st["chain_hops"] += hops
        if kind == "visible":
            mask[i] = 1
            st["n_visible"] += 1
        elif kind in REASONS:
            mask[i] = 1
            st["n_undecided"] += 1
            st["undecided_by_reason"][kind] += 1
            und.append(i)
        else:
            st["n_invisible"] += 1
            if kind != "invisible":
                st[{"deleted": "n_deleted", "not_found": "n_not_found", "dead_lp": "n_dead_line_pointer"}[kind]] += 1
    return mask, st, np.array(und, np.uint32), kinds


# ---- the device side ------------------------------------------------------------------------------------------------------------------
def dev_visibility(ctx, heap, tids, s, clog, cap=None):
    """vs_heap_res_visibility over host tids through scratch device buffers whose bytes around [0, n) are checked for stray writes
    -> (mask, stats, undecided, n_undecided)"""
    tids = np.ascontiguousarray(tids, np.uint64)
    n = len(tids)
    guard = 64
    d_t, d_v = ctx.alloc(max(n, 1) * 8), ctx.alloc(n + 2 * guard)
    try:
        ctx.upload(d_t, tids)
        ctx.upload(d_v, np.full(n + 2 * guard, 0xA5, np.uint8))
        st, und, nu = heap.visibility(d_t, n, s, clog.xact(), type(d_v)(d_v.value + guard), cap=cap)
        buf = ctx.download(d_v, np.empty(n + 2 * guard, np.uint8))
        assert (buf[:guard] == 0xA5).all() and (buf[guard + n:] == 0xA5).all(), "a byte outside [0, n) was written"
        return buf[guard:guard + n].copy(), st, und, nu
    finally:
        ctx.free(d_t)
        ctx.free(d_v)


def resident(ctx, rel, capacity=0):
    from pgvectorscale_amd.pages import HeapResident
    h = HeapResident(ctx, capacity, page_size=rel.page_size)
    if rel.pages:
        h.put(rel.tobytes())
    return h


def check_against_ref(ctx, rel, tids, s, clog, heap=None, n_blocks=None):
    """device == restatement: the mask, every counter, the sorted undecided list -> (mask, stats, undecided, kinds) of the reference"""
    own = heap is None
    heap = resident(ctx, rel) if own else heap
    try:
        mask, st, und, nu = dev_visibility(ctx, heap, tids, s, clog)
    finally:
        if own:
            heap.close()
    rmask, rst, rund, kinds = ref_visibility(rel.pages, rel.page_size, len(rel.pages) if n_blocks is None else n_blocks, tids, s, clog)
    assert (mask == rmask).all(), np.flatnonzero(mask != rmask)[:10]
    assert st == rst, (st, rst)
    assert nu == len(rund) and und.dtype == np.uint32 and (und == rund).all()
    return rmask, rst, rund, kinds


# ---- the randomised corpus ------------------------------------------------------------------------------------------------------------
def random_corpus(n, seed, base=0):
    """n single-version rows (a few behind redirects, dead and unused line pointers) with random headers around a snapshot whose
    xids are shifted by `base` modulo 2^32 -> (relation, tids in heap order, snapshot dict, Clog).  The proportions are tuned so
    that the rule alone decides more than 80 % and every reason shows (asserted by the test on the reference's output)."""
    rng = np.random.default_rng(seed)
    B = lambda x: (x + base) & M32  # noqa: E731
    lo, xmin, xmax, hi = 800, 1000, 2000, 2200  # the clog window is [lo, hi)
    own = [1500, 1501, 1502]
    pool = [x for x in range(xmin, xmax) if x not in own]
    picks = rng.choice(pool, 60, replace=False)
    xip, subxip = [int(x) for x in picks[:40]], [int(x) for x in picks[40:]]
    clog = Clog(B(lo), hi - lo)
    for x in range(lo, hi):
        clog.set(B(x), int(rng.choice([COMMITTED, ABORTED, IN_PROGRESS, SUB_COMMITTED], p=[0.80, 0.13, 0.04, 0.03])))
    for x in own + xip[:30]:
        clog.set(B(x), IN_PROGRESS)
    snap = dict(xmin=B(xmin), xmax=B(xmax), xip=[B(x) for x in xip], subxip=[B(x) for x in subxip], own_xids=[B(x) for x in own], curcid=10)

    def draw_xid():
        r = rng.random()
        if r < 0.70:
            return int(rng.integers(lo, xmin))
        if r < 0.74:
            return int(rng.integers(xmin, xmax))
        if r < 0.80:
            return int(rng.choice(xip + subxip))
        if r < 0.85:
            return int(rng.integers(xmax, hi + 50))
        if r < 0.875:
            return int(rng.integers(lo - 200, lo))  # outside the window, before the snapshot
        if r < 0.97:
            return int(rng.choice(own))
        return None  # a special xid

    rel = HP.HeapRelation()
    tids = []
    for _ in range(n):
        m, m2, cid = 0, 0, int(rng.integers(0, 20))
        x = draw_xid()
        is_own = x in own
        xm = int(rng.integers(0, 3)) if x is None else B(x)
        r = rng.random()
        if r < 0.15:
            m |= FROZEN
        elif r < 0.45 and x is not None and clog.get(B(x)) == COMMITTED:
            m |= XMIN_COMMITTED
        elif r < 0.48:
            m |= XMIN_INVALID
        elif r < 0.50:
            m |= MOVED_OFF if rng.random() < 0.5 else MOVED_IN
        if is_own and rng.random() < 0.35:
            m |= COMBOCID
        xmx = 0
        if rng.random() < 0.55:
            m |= XMAX_INVALID
        else:
            y = draw_xid()
            xmx = int(rng.integers(0, 3)) if y is None else B(y)
            r = rng.random()
            if r < 0.10:
                m |= LOCK_ONLY
            elif r < 0.16:
                m |= EXCL_LOCK
            elif r < 0.20:
                m |= EXCL_LOCK | KEYSHR_LOCK
            elif r < 0.27:
                m |= IS_MULTI | (LOCK_ONLY if rng.random() < 0.3 else 0)
            elif r < 0.50 and y is not None and clog.get(B(y)) == COMMITTED:
                m |= XMAX_COMMITTED
            if y in own and rng.random() < 0.35:
                m |= COMBOCID
        blk, off = rel.add_item(tup(xm, xmx, cid, m, m2))
        r = rng.random()
        if r < 0.02:
            rel.set_line_pointer(blk, off, HP.LP_DEAD)
        elif r < 0.03:
            rel.set_line_pointer(blk, off, HP.LP_UNUSED)
        elif r < 0.06:  # a pruned root: the index's tid names a redirect to the row
            blk2, off2 = rel.add_item(tup(0, 0, 0, XMIN_INVALID))
            if blk2 == blk:
                rel.set_line_pointer(blk2, off2, HP.LP_REDIRECT, lp_off=off)
                off = off2
        tids.append(tid_of(blk, off))
    return rel, np.array(tids, np.uint64), snap, clog


def index_order(tids, seed=1, deleted=0.05):
    """index order is not heap order: shuffled, and a few index tuples deleted (vacuum: offset 0)"""
    rng = np.random.default_rng(seed)
    t = tids[rng.permutation(len(tids))].copy()
    t[rng.random(len(t)) < deleted] &= ~np.uint64(0xFFFF)
    return t
