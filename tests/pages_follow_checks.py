"""The numpy side of the follower tests (tests/test_gpu_zx_pages_follow.py): index states as flat arrays, the mutations a relation's
other writer makes to them (rows appended with neighbor lists, existing rows relinked — some to the appended ids —, heap offsets
cleared), both relations through the oracle's writer (oracle/pages_py.py::write_index) and what vs_pages_follow_info must say,
counted from the arrays.  Nothing here touches the library."""
import numpy as np

from helpers import make_vectors
from oracle import oracle_py as O
from oracle import pages_py as PG

B = PG.BLCKSZ
INV = 0xFFFFFFFF
OFFSET = np.uint64(0xFFFF)


class State:
    """one state of an index: the arrays a relation is written from"""

    def __init__(self, codes, nbrs, tids, vecs, start, label_off=None, label_val=None, label_starts=None):
        self.codes, self.nbrs, self.tids, self.vecs, self.start = codes, nbrs, tids, vecs, start
        self.label_off, self.label_val, self.label_starts = label_off, label_val, dict(label_starts or {})
        self.n = codes.shape[0]

    def label_sets(self):
        return [self.label_val[self.label_off[i]:self.label_off[i + 1]].tolist() for i in range(self.n)]


def _csr(sets):
    off = np.zeros(len(sets) + 1, np.uint32)
    off[1:] = np.cumsum([len(s) for s in sets])
    return off, np.array([l for s in sets for l in s], np.int16)


class Family:
    """n_max rows of one geometry — vectors, the quantizer trained over all of them, their codes, heap tids, label sets — of which a
    state holds a prefix"""

    def __init__(self, *, dim, bits, R, distance, n_max, seed, labeled=False, fresh_label=None):
        self.dim, self.bits, self.R, self.distance, self.n_max = dim, bits, R, distance, n_max
        self.vecs = make_vectors(n_max, dim, seed, "gauss")
        sl = self.vecs.copy()
        if distance == O.COSINE:
            for i in range(n_max):
                sl[i] = O.preprocess_cosine(sl[i])[0]
        self.mean, self.m2, self.count = O.train(sl, bits)
        self.codes = O.quantize(self.mean, self.m2, self.count, bits, sl)
        self.W = self.codes.shape[1]
        self.tids = ((np.arange(n_max, dtype=np.uint64) + 7) << np.uint64(16)) | np.uint64(1)
        self.sets = None
        self.fresh_label = fresh_label
        if labeled:
            rng = np.random.default_rng(seed + 500)
            self.sets = [sorted(set(int(v) for v in rng.integers(1, 7, int(rng.integers(0, 5))))) for _ in range(n_max)]

    def s0(self, n0):
        nbrs, start = O.build_graph(self.codes[:n0], num_neighbors=self.R, search_list_size=32)
        lo = lv = None
        starts = {}
        if self.sets is not None:
            lo, lv = _csr(self.sets[:n0])
            for i, s in enumerate(self.sets[:n0]):
                for l in s:
                    starts.setdefault(l, i)
        return State(self.codes[:n0].copy(), np.ascontiguousarray(nbrs[:, :self.R], np.uint32), self.tids[:n0].copy(), self.vecs[:n0].copy(),
                     int(start), lo, lv, starts)

    def mutate(self, s, m, k, d, seed):
        """s + m appended rows with neighbor lists, k existing rows relinked (every other one to an appended id when there is
        one), d heap offsets cleared"""
        rng = np.random.default_rng(seed)
        n0, n1, R = s.n, s.n + m, self.R
        assert n1 <= self.n_max
        nbrs = np.full((n1, R), INV, np.uint32)
        nbrs[:n0] = s.nbrs
        for t, i in enumerate(range(n0, n1)):
            deg = R if t == 0 else int(rng.integers(0 if t == 1 else 1, R + 1))  # (a full list, then maybe an empty one)
            deg = min(deg, n1 - 1)
            cand = rng.choice(n1 - 1, deg, replace=False)
            cand[cand >= i] += 1  # (no self loop)
            nbrs[i, :deg] = cand
        rows = rng.choice(n0, k, replace=False) if k else []
        for t, u in enumerate(rows):
            row = nbrs[u]
            deg = int((row != INV).sum())
            lo, hi = (n0, n1) if (m and t % 2 == 0) else (0, n0)
            free = [int(x) for x in rng.permutation(np.arange(lo, hi)) if x != u and x not in row]
            v = free[0] if free else next(int(x) for x in rng.permutation(n1) if x != u and x not in row)
            if deg < R and t % 3 == 0:
                row[deg] = v
            else:
                row[int(rng.integers(max(deg, 1)))] = v
                if t % 5 == 4 and deg >= 3:
                    row[deg - 1] = INV  # (a list that also got shorter)
        tids = self.tids[:n1].copy()
        tids[:n0] = s.tids
        live = [i for i in np.flatnonzero((s.tids & OFFSET) != 0) if i != s.start]
        for i in (rng.choice(live, d, replace=False) if d else []):
            tids[i] &= ~OFFSET
        lo = lv = None
        starts = dict(s.label_starts)
        if self.sets is not None:
            sets = [list(x) for x in self.sets[:n1]]
            if self.fresh_label is not None and m:
                sets[n0 + m // 2] = sorted(set(sets[n0 + m // 2] + [self.fresh_label]))
            assert sets[:n0] == s.label_sets()
            lo, lv = _csr(sets)
            for i in range(n0, n1):  # (update_start_nodes: a label first carried by a new node gets it as its start node)
                for l in sets[i]:
                    starts.setdefault(l, i)
        return State(self.codes[:n1].copy(), nbrs, tids, self.vecs[:n1].copy(), s.start, lo, lv, starts)

    def relation(self, s, zero_page_every=0):
        meta = dict(num_dimensions=self.dim, num_dimensions_to_index=self.dim, bq_num_bits_per_dimension=self.bits,
                    distance_type=self.distance, num_neighbors=self.R, default_start=s.start, labeled_starts=dict(s.label_starts),
                    extension_version="0.8.0", search_list_size=100, max_alpha=1.2)
        w = PG.write_index(codes=s.codes, nbrs=s.nbrs, heap_tids=s.tids, mean=self.mean, m2=self.m2, count=self.count, label_off=s.label_off,
                           label_val=s.label_val, means_first=True, meta=meta, zero_page_every=zero_page_every)
        return w.rel.tobytes(), w.node_ptrs

    def oracle(self, s):
        return O.OracleIndex(codes=s.codes, nbrs=s.nbrs, heap_tids=s.tids, vecs=s.vecs, mean=self.mean, m2=self.m2, count=self.count,
                             bits=self.bits, dim_index=self.dim, num_neighbors=self.R, distance_type=self.distance, default_start=s.start,
                             label_off=s.label_off, label_val=s.label_val, label_starts=s.label_starts)


def node_items(raw, b):
    """SbqNode items on block b of a relation (0: a new page, another page type)"""
    page = raw[b * B:(b + 1) * B]
    lower, upper = int.from_bytes(page[12:14], "little"), int.from_bytes(page[14:16], "little")
    if upper == 0 or page[B - 8] != PG.PT_SBQ_NODE:
        return 0
    return (lower - 24) // 4


def dirty(before, after):
    """the blocks of `after` that differ from `before` or lie past its end"""
    nb_b, nb_a = len(before) // B, len(after) // B
    return [b for b in range(nb_a) if b >= nb_b or after[b * B:(b + 1) * B] != before[b * B:(b + 1) * B]]


def expected_info(s0, s1, before, after, blocks):
    """vs_pages_follow_info for the step s0 -> s1, counted from the arrays"""
    n0 = s0.n
    cleared = ((s0.tids & OFFSET) != 0) & ((s1.tids[:n0] & OFFSET) == 0)
    return dict(n_blocks_before=len(before) // B, n_blocks_now=len(after) // B, pages_listed=len(blocks),
                node_pages_listed=sum(node_items(after, b) > 0 for b in blocks), n_before=n0, n_appended=s1.n - n0,
                rows_relinked=int((s0.nbrs != s1.nbrs[:n0]).any(1).sum()), tids_cleared=int(cleared.sum()),
                tids_changed=int(((s0.tids != s1.tids[:n0]) & ~cleared).sum()), codes_changed=int((s0.codes != s1.codes[:n0]).any(1).sum()),
                label_vals_appended=0 if s1.label_off is None else int(s1.label_off[s1.n]) - int(s0.label_off[n0]))


def gather(raw, blocks):
    return b"".join(raw[b * B:(b + 1) * B] for b in blocks)


def item_span(page, off):
    """(start, length) of item `off` of a page"""
    lp = int.from_bytes(page[24 + 4 * (off - 1):28 + 4 * (off - 1)], "little")
    return lp & 0x7FFF, lp >> 17


def field_at(page, off, field_off, root_size=32):
    """byte position of an 8-byte root field of item `off`, and of the ArchivedVec elements it points at"""
    s, l = item_span(page, off)
    fld = s + l - root_size + field_off
    rel = int.from_bytes(page[fld:fld + 4], "little", signed=True)
    return fld, fld + rel
