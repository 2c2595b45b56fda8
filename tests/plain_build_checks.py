"""Two numpy restatements for the plain-storage build (tests/test_gpu_zy_plain_build.py).

PairRule restates the rule the device build scores with: the pair distance d(a -> b) is the oracle's distance_by_type on the two
PREPARED index slices (first dim_index dimensions, cosine-normalised on their own), keys order like f32::total_cmp, every order
is ascending (key, id); prune is add_neighbors + prune_neighbors in f32, mates the c nearest other rows of a range.

sequential_vamana is the quality yardstick: a plain sequential f32 Vamana (rows in order, greedy search from node 0, prune over
visited + final list, back-pointers appended while there is room, else prune(existing + new)).  It shares no code with the
library and is not bit-exact to anything; only its recall is used.

Nothing here calls the library under test."""
import os

import numpy as np

from lifecycle_checks import prepared_slice

INV = 0xFFFFFFFF
EMU = bool(os.environ.get("VS_EMU"))
EPS = np.float32(1.1920929e-07)  # f32::EPSILON
FMAX = np.float32(3.0e38)
# recall@10 of sequential_vamana on the quality shape (1 500 x 48 gauss, L2, R = 16, L = 32, 256 queries, oracle plain search at
# L = 32) over corpus seeds 9..13, measured once on a CPU with this file's code, and their spread (max - min): the margin of the
# quality and insert cases.  DESIGN.md section 6g records the same numbers.
SEQ_RECALL_BY_SEED = {9: 0.9203125, 10: 0.9109375, 11: 0.916015625, 12: 0.9109375, 13: 0.91953125}
SEQ_RECALL_SPREAD = 0.009375  # 0.9203125 - 0.9109375


def plain_key(d):
    """the monotone u32 image of f32::total_cmp (plain_key in vs_device.h)"""
    b = np.asarray(d, np.float32).view(np.int32).astype(np.int64)
    b = np.where(b < 0, b ^ 0x7FFFFFFF, b)
    return ((b & 0xFFFFFFFF) ^ 0x80000000).astype(np.uint32)


class PairRule:
    def __init__(self, O, X, distance, dim_index=None):
        self.O, self.distance = O, distance
        self.P = prepared_slice(O, X, distance, dim_index or X.shape[1])
        self._memo = {}

    def d(self, a, b):
        """d(a -> b): a's prepared slice is the query, b's the row"""
        k = (int(a), int(b))
        v = self._memo.get(k)
        if v is None:
            v = self._memo[k] = np.float32(self.O.distance_by_type(self.distance, self.P[k[0]], self.P[k[1]]))
        return v

    def key(self, a, b):
        return int(plain_key(self.d(a, b)))

    def sorted_candidates(self, p, cands):
        """each id once, never the point, ascending (key of d(p -> id), id)"""
        return sorted((self.key(p, c), int(c)) for c in set(int(c) for c in cands) if int(c) != int(p))

    def prune(self, p, cands, R, max_alpha):
        """what add_neighbors makes of the candidate set: the ids in list order"""
        items = self.sorted_candidates(p, cands)
        ids = [c for _, c in items]
        if len(ids) <= R:
            return ids
        dpc = [self.d(p, c) for c in ids]
        C = len(ids)
        maxf = np.zeros(C, np.float32)
        res = []
        max_alpha = np.float32(max_alpha)
        alpha = np.float32(1.0)
        while alpha <= max_alpha and len(res) < R:
            for i in range(C):
                if len(res) >= R:
                    break
                if maxf[i] > alpha:
                    continue
                maxf[i] = FMAX
                res.append(ids[i])
                for j in range(i + 1, C):
                    if maxf[j] > max_alpha:
                        continue
                    d_ec = self.d(ids[i], ids[j])  # the existing neighbour is the query
                    if d_ec < EPS:
                        factor = np.float32(1.0) if dpc[j] < EPS else FMAX
                    else:
                        factor = np.float32(dpc[j] / d_ec)
                    maxf[j] = np.fmax(maxf[j], factor)
            alpha = np.float32(alpha * np.float32(1.2))
        return res

    def mates(self, first, n, c):
        """for rows first .. first + n - 1 the c nearest other rows of the range by (key, row) -> (ids [n][c], dist f32 [n][c])"""
        ids = np.full((n, c), INV, np.uint32)
        dist = np.full((n, c), 0xFFFFFFFF, np.uint32).view(np.float32)
        for i in range(n):
            best = sorted((self.key(first + i, first + j), j) for j in range(n) if j != i)[:c]
            for t, (_, j) in enumerate(best):
                ids[i, t] = j
                dist[i, t] = self.d(first + i, first + j)
        return ids, dist


# ---- the sequential yardstick --------------------------------------------------------------------------------------------------
def _l2(X, ids, x):
    diff = X[ids] - x
    return np.einsum("ij,ij->i", diff, diff).astype(np.float32)


def _prune_f32(X, p, cand, R, max_alpha):
    """robust prune of candidate ids (each once, never p) around point p, f32 L2; returns the kept ids in order"""
    cand = np.asarray(sorted(set(int(c) for c in cand) - {int(p)}), np.int64)
    if cand.size == 0:
        return []
    dp = _l2(X, cand, X[p])
    order = np.lexsort((cand, dp))
    cand, dp = cand[order], dp[order]
    if cand.size <= R:
        return cand.tolist()
    maxf = np.zeros(cand.size, np.float32)
    res = []
    alpha = np.float32(1.0)
    while alpha <= np.float32(max_alpha) and len(res) < R:
        for i in range(cand.size):
            if len(res) >= R:
                break
            if maxf[i] > alpha:
                continue
            maxf[i] = FMAX
            res.append(int(cand[i]))
            tail = np.arange(i + 1, cand.size)
            if tail.size:
                dec = _l2(X, cand[tail], X[cand[i]])
                with np.errstate(divide="ignore", invalid="ignore"):
                    f = np.where(dec < EPS, np.where(dp[tail] < EPS, np.float32(1.0), FMAX), dp[tail] / dec).astype(np.float32)
                maxf[tail] = np.fmax(maxf[tail], f)
        alpha = np.float32(alpha * np.float32(1.2))
    return res


def sequential_vamana(X, R, L, max_alpha=1.2):
    """nbrs uint32 [n][R] (INV padded) of a sequential f32 L2 Vamana over the rows of X, start node 0"""
    X = np.ascontiguousarray(X, np.float32)
    n = X.shape[0]
    nbrs = [[] for _ in range(n)]
    for p in range(1, n):
        # greedy search from node 0 with list L
        d0 = float(_l2(X, np.array([0]), X[p])[0])
        lst = [(d0, 0)]
        seen = {0}
        visited = []
        expanded = set()
        while True:
            nxt = next((e for e in lst if e[1] not in expanded), None)
            if nxt is None:
                break
            v = nxt[1]
            expanded.add(v)
            visited.append(v)
            fresh = [u for u in nbrs[v] if u not in seen]
            if fresh:
                seen.update(fresh)
                dd = _l2(X, np.asarray(fresh, np.int64), X[p])
                lst.extend(zip(dd.tolist(), fresh))
                lst.sort()
                del lst[L:]
        nbrs[p] = _prune_f32(X, p, visited + [u for _, u in lst], R, max_alpha)
        for q in nbrs[p]:  # back-pointers
            if p in nbrs[q]:
                continue
            if len(nbrs[q]) < R:
                nbrs[q].append(p)
            else:
                nbrs[q] = _prune_f32(X, q, nbrs[q] + [p], R, max_alpha)
    out = np.full((n, R), INV, np.uint32)
    for i, r in enumerate(nbrs):
        out[i, :len(r)] = r
    return out


# ---- measuring a graph -------------------------------------------------------------------------------------------------------
def exact_top10(X, Q):
    d = ((Q[:, None, :].astype(np.float64) - X[None, :, :].astype(np.float64)) ** 2).sum(2)
    return np.argsort(d, axis=1, kind="stable")[:, :10]


def recall_at_10(O, X, nbrs, start, Q, truth, L, distance=None):
    """recall@10 of the oracle's plain search at list size L over the graph nbrs"""
    distance = O.L2 if distance is None else distance
    n, dim = X.shape
    tids = ((np.arange(n, dtype=np.uint64) + 1) << np.uint64(16)) | np.uint64(1)
    w = (dim + 63) // 64
    oidx = O.OracleIndex(codes=np.zeros((n, w), np.uint64), nbrs=nbrs, heap_tids=tids, vecs=X, mean=np.zeros(dim, np.float32),
                         m2=np.zeros(dim, np.float32), count=0, bits=1, dim_index=dim, num_neighbors=nbrs.shape[1],
                         distance_type=distance, default_start=start, storage_plain=True)
    got, _, _ = oidx.search_batch(Q, L=L, rescore=0, k=10)
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / 10 for a, b in zip(got, truth)]))


def sbq_graph(O, X, R, L):
    """the oracle's builder over 2-bit SBQ codes of the same vectors: the only graph a plain index could be given before"""
    mean, m2, cnt = O.train(X, 2)
    return O.build_graph(O.quantize(mean, m2, cnt, 2, X), num_neighbors=R, search_list_size=L)


def reach(nbrs, start):
    """the nodes a host walk from `start` finds (bool [n])"""
    n = nbrs.shape[0]
    seen = np.zeros(n, bool)
    if n == 0 or start == INV:
        return seen
    seen[start] = True
    stack = [int(start)]
    while stack:
        v = stack.pop()
        for u in nbrs[v]:
            if u != INV and not seen[u]:
                seen[u] = True
                stack.append(int(u))
    return seen
