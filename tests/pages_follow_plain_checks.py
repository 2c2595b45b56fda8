"""The numpy side of the plain follower tests (tests/test_gpu_zx_pages_follow_plain.py), in the manner of tests/pages_follow_checks.py:
states of a `plain` storage index as flat arrays (the heap's raw rows, the node vectors the oracle derives from them, neighbor rows,
heap tids), the mutations a relation's other writer makes to them, both relations through the oracle's writer
(oracle/pages_py.py::write_plain_index) and what vs_pages_follow_info must say, counted from the arrays.  Nothing here touches the
library."""
import numpy as np

from helpers import make_vectors
from oracle import oracle_py as O
from oracle import pages_py as PG
from pages_follow_checks import B, INV, OFFSET, dirty, field_at, gather, item_span  # noqa: F401  (shared page arithmetic)


class State:
    """one state of a plain index: the arrays a relation is written from (vecs = the heap's rows, nodevecs = PlainNode.vector)"""

    def __init__(self, nbrs, tids, vecs, nodevecs, start):
        self.nbrs, self.tids, self.vecs, self.nodevecs, self.start = nbrs, tids, vecs, nodevecs, start
        self.n = nbrs.shape[0]


def node_vectors(rows, dim_index, distance):
    """PlainNode.vector as the oracle defines it: the first dim_index floats, for cosine preprocess_cosine of that slice"""
    out = np.ascontiguousarray(rows[:, :dim_index], np.float32).copy()
    if distance == O.COSINE:
        for i in range(out.shape[0]):
            out[i] = O.preprocess_cosine(out[i])[0]
    return out


def slice_divisors(rows, dim_index):
    """the divisor cache of the index slices (k_row_norms): the sum of squares in element order in f32; 0 = the slice is left alone
    (a sum below epsilon, or within dim_index x epsilon of 1), else its square root"""
    v = np.ascontiguousarray(rows[:, :dim_index], np.float32)
    norm = np.zeros(v.shape[0], np.float32)
    for c in range(v.shape[1]):
        norm = norm + v[:, c] * v[:, c]
    eps = np.float32(1.1920929e-07)
    adj = np.float32(eps * np.float32(dim_index))
    one = np.float32(1.0)
    keep = (norm < eps) | ((norm >= one - adj) & (norm <= one + adj))
    return np.where(keep, np.float32(0.0), np.sqrt(norm)).astype(np.float32)


def composed(rows, dim_index, distance):
    """the plain page writer's rule, restated: the first dim_index floats of the row, for cosine each divided (one correctly rounded
    f32 division) by the slice's divisor where that is not zero"""
    sl = np.ascontiguousarray(rows[:, :dim_index], np.float32).copy()
    if distance == O.COSINE:
        div = slice_divisors(rows, dim_index)
        nz = div != 0
        sl[nz] = (sl[nz] / div[nz, None]).astype(np.float32)
    return sl


def vectors_differing(rows, dim_index, distance, page_vectors):
    """codes_changed by the numpy restatement: rows whose page vector is not, bit for bit, what the writer would compose"""
    want = composed(rows, dim_index, distance).view(np.uint32)
    return int((want != np.ascontiguousarray(page_vectors, np.float32).view(np.uint32)).any(1).sum())


class Family:
    """n_max rows of one plain geometry, of which a state holds a prefix; zero_row: a row that is all zero (divisor 0)"""

    def __init__(self, *, dim, R, distance, n_max, seed, dim_index=None, zero_row=None):
        self.dim, self.dim_index, self.R, self.distance, self.n_max = dim, dim_index or dim, R, distance, n_max
        self.vecs = make_vectors(n_max, dim, seed, "gauss")
        self.vecs *= np.random.default_rng(seed + 900).uniform(0.2, 3.0, (n_max, 1)).astype(np.float32)  # un-normalised rows
        if zero_row is not None:
            self.vecs[zero_row] = 0
        self.nodevecs = node_vectors(self.vecs, self.dim_index, distance)
        # any connected graph will do: the oracle's SBQ builder over 2-bit codes of the index slices; the codes also size the oracle's view
        sl = np.ascontiguousarray(self.vecs[:, :self.dim_index])
        self.mean, self.m2, self.count = O.train(sl, 2)
        self.codes = O.quantize(self.mean, self.m2, self.count, 2, sl)
        self.tids = ((np.arange(n_max, dtype=np.uint64) + 7) << np.uint64(16)) | np.uint64(1)

    def s0(self, n0):
        nbrs, start = O.build_graph(self.codes[:n0], num_neighbors=self.R, search_list_size=32)
        nb = np.full((n0, self.R), INV, np.uint32)
        w = min(self.R, nbrs.shape[1])
        nb[:, :w] = nbrs[:, :w]
        return State(nb, self.tids[:n0].copy(), self.vecs[:n0].copy(), self.nodevecs[:n0].copy(), int(start))

    def mutate(self, s, m, k, d, seed):
        """s + m appended rows with neighbor lists (the first full, the second possibly empty), k existing rows relinked (every
        other one to an appended id when there is one), d heap offsets cleared"""
        rng = np.random.default_rng(seed)
        n0, n1, R = s.n, s.n + m, self.R
        assert n1 <= self.n_max
        nbrs = np.full((n1, R), INV, np.uint32)
        nbrs[:n0] = s.nbrs
        for t, i in enumerate(range(n0, n1)):
            deg = R if t == 0 else int(rng.integers(0 if t == 1 else 1, R + 1))
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
            v = free[0] if free else next((int(x) for x in rng.permutation(n1) if x != u and x not in row), None)
            if v is None:  # (the row names every other node: the list gets shorter instead)
                row[deg - 1] = INV
            elif deg < R and t % 3 == 0:
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
        return State(nbrs, tids, self.vecs[:n1].copy(), self.nodevecs[:n1].copy(), s.start)

    def relation(self, s):
        meta = dict(storage_type=0, num_dimensions=self.dim, num_dimensions_to_index=self.dim_index, bq_num_bits_per_dimension=1,
                    distance_type=self.distance, num_neighbors=self.R, default_start=s.start, labeled_starts={}, extension_version="0.8.0",
                    search_list_size=100, max_alpha=1.2)
        w = PG.write_plain_index(vectors=s.nodevecs, nbrs=s.nbrs, heap_tids=s.tids, num_neighbors=self.R, meta=meta)
        return w.rel.tobytes(), [tuple(p) for p in w.node_ptrs]

    def oracle(self, s):
        return O.OracleIndex(codes=self.codes[:s.n], nbrs=s.nbrs, heap_tids=s.tids, vecs=s.vecs, mean=self.mean, m2=self.m2, count=self.count,
                             bits=2, dim_index=self.dim_index, num_neighbors=self.R, distance_type=self.distance, default_start=s.start,
                             storage_plain=True)


def node_items(raw, b):
    """PlainNode items on block b of a relation (0: a new page, another page type)"""
    page = raw[b * B:(b + 1) * B]
    lower, upper = int.from_bytes(page[12:14], "little"), int.from_bytes(page[14:16], "little")
    if upper == 0 or page[B - 8] != PG.PT_NODE:
        return 0
    return (lower - 24) // 4


def block_counts(raw):
    return [node_items(raw, b) for b in range(len(raw) // B)]


def page_vectors(raw, ptrs, dim_index, vec_field=0):
    """PlainNode.vector of every node as the relation's bytes hold it"""
    out = np.empty((len(ptrs), dim_index), np.float32)
    for i, (blk, off) in enumerate(ptrs):
        page = raw[blk * B:(blk + 1) * B]
        _, at = field_at(page, off, vec_field)
        out[i] = np.frombuffer(page[at:at + 4 * dim_index], "<f4")
    return out


def expected_info(fam, s0, s1, before, after, blocks, ptrs1):
    """vs_pages_follow_info for the step s0 -> s1, counted from the arrays (codes_changed: the numpy restatement of the writer's rule
    over the resident rows against the vectors the after-relation holds, for the existing nodes on the listed pages)"""
    n0 = s0.n
    listed = set(blocks)
    on = [i for i in range(n0) if ptrs1[i][0] in listed]
    cleared = ((s0.tids & OFFSET) != 0) & ((s1.tids[:n0] & OFFSET) == 0)
    return dict(n_blocks_before=len(before) // B, n_blocks_now=len(after) // B, pages_listed=len(blocks),
                node_pages_listed=sum(node_items(after, b) > 0 for b in blocks), n_before=n0, n_appended=s1.n - n0,
                rows_relinked=int((s0.nbrs != s1.nbrs[:n0]).any(1).sum()), tids_cleared=int(cleared.sum()),
                tids_changed=int(((s0.tids != s1.tids[:n0]) & ~cleared).sum()),
                codes_changed=vectors_differing(s0.vecs[on], fam.dim_index, fam.distance,
                                                page_vectors(after, [ptrs1[i] for i in on], fam.dim_index)) if on else 0,
                label_vals_appended=0)
