"""The batch step of the SBQ build and insert (vs_build_graph / vs_index_insert over memory_optimized storage), restated sequentially
over plain numpy arrays (tests/test_gpu_zy_build_twin.py; DESIGN.md section 6b, rules 1 to 7).

_ham, _prune and _pmask are the pieces the consolidation restatement shares (tests/test_gpu_zw_consolidate.py).  batch_step is one
batch: the build searches over the graph as it stands (the oracle's own build search, oracle_py.search_for_build), the mates of an
insert, the out-edges, the back-edge requests in their stable sorted order and what every target makes of them.  build is the
schedule of vs_build_graph on top of it, without the repair pass.

Nothing here calls the library under test."""
import numpy as np

from oracle import oracle_py as O

INV = 0xFFFFFFFF


# ---- shared with the consolidation restatement -----------------------------------------------------------------------------------
def _ham(codes, ids, p):
    return np.bitwise_count(codes[ids] ^ codes[p]).sum(axis=1).astype(np.uint32)


def _prune(codes, ids, d, R, max_alpha, pm):
    """wave_prune's general loop: -> the selected candidate positions, in selection order"""
    C = len(ids)
    FMAX = np.float32(3.0e38)
    ma = np.float32(max_alpha)
    maxf = np.zeros(C, np.float32)
    sel = []
    alpha = np.float32(1.0)
    while alpha <= ma and len(sel) < R:
        for i in range(C):
            if len(sel) >= R:
                break
            if maxf[i] > alpha:
                continue
            maxf[i] = FMAX
            sel.append(i)
            js = np.arange(i + 1, C)
            go = ~(maxf[js] > ma)
            if pm is not None:
                go &= (pm[js] & ~pm[i]) == 0  # "Does it contain essential labels?"
            js = js[go]
            if js.size == 0:
                continue
            dij = _ham(codes, ids[js], ids[i])
            with np.errstate(divide="ignore", invalid="ignore"):
                factor = d[js].astype(np.float32) / dij.astype(np.float32)
            factor = np.where(dij == 0, np.where(d[js] == 0, np.float32(1.0), FMAX), factor).astype(np.float32)
            maxf[js] = np.maximum(maxf[js], factor)
        alpha = np.float32(alpha * np.float32(1.2))
    return sel


def _pmask(sets, p, node):
    """label_pmask: bit t <=> the t-th label of p (sorted) is in node's set"""
    m = 0
    for t, l in enumerate(sets[p]):
        if l in sets[node]:
            m |= 1 << t
    return m


# ---- capacities (BatchRunner::init) --------------------------------------------------------------------------------------------
def vmax_of(L):
    """the visited list keeps its closest vmax entries"""
    return max((3 * L + 64 + 63) // 64 * 64, 128)


def cmax_of(R):
    """a back-edge target weighs at most cmax candidates: the smallest power of two >= R + 128"""
    c = 1
    while c < R + 128:
        c <<= 1
    return c


def default_batch_max(n):
    return min(65536, max(1024, n // 64))


def label_starts_of(labels):
    """update_start_nodes over rows that arrive in id order: a label's start node is the smallest id that carries it"""
    first = {}
    for i, ls in enumerate(labels):
        for l in ls:
            first.setdefault(int(l), i)
    return first


def _csr(labels):
    off = np.zeros(len(labels) + 1, np.uint32)
    off[1:] = np.cumsum([len(s) for s in labels])
    return off, np.array([l for s in labels for l in s], np.int16)


def _choose(codes, of, ids, d, R, max_alpha, labels):
    """rule 4 / the end of rule 6: ids sorted ascending (d, id) -> the row: all of them when they fit, else _prune's selection"""
    if len(ids) <= R:
        return ids
    pm = None if labels is None else np.array([_pmask(labels, of, int(v)) for v in ids], np.uint64)
    return ids[_prune(codes, ids, d, R, max_alpha, pm)]


def _sorted_pairs(pairs):
    """[(d, id)] -> (ids int64, d uint32) ascending (d, id)"""
    pairs = sorted(pairs)
    return np.array([v for _, v in pairs], np.int64), np.array([h for h, _ in pairs], np.uint32)


def _mates(codes, b0, bn, c, labels):
    """rule 3: per row of the batch the c nearest other rows of the batch by (Hamming, id); labels (the filtered pass of a labeled
    set): only rows whose label sets overlap -> [[(d, id)]]"""
    out = []
    rows = np.arange(b0, b0 + bn)
    for p in range(b0, b0 + bn):
        ham = _ham(codes, rows, p)
        keys = [(int(ham[j]), b0 + j) for j in range(bn)
                if b0 + j != p and (labels is None or set(labels[p]) & set(labels[b0 + j]))]
        out.append(sorted(keys)[:c])
    return out


def _run(codes, nbrs, b0, bn, R, L, max_alpha, mates, labels, starts, filtered, merge_existing, trace):
    """one BatchRunner::run: searches over the rows as they stand, out-edges of rows b0 .. b0 + bn - 1, back-edges.  nbrs is changed
    in place.  labels None: k_build_prune_new; else k_build_prune_merge."""
    vmax, cmax = vmax_of(L), cmax_of(R)
    snap = nbrs.copy()  # every search of the batch sees the graph as it stood when the pass began
    off = val = None
    if filtered:
        off, val = _csr(labels)
    mate_rows = _mates(codes, b0, bn, mates, labels if filtered else None) if mates and bn > 1 else None
    requests = []  # (target, d, source) in (batch position, slot) order
    for b in range(bn):
        p = b0 + b
        # rule 2: the visited list of greedy_search_for_build, ascending Hamming, of equal ones the one visited later first (the
        # reference's visited.insert(partition_point(|x| x < head), head)), its first vmax
        if filtered:
            st = [starts[int(l)] for l in labels[p]]
            ids, ham = O.search_for_build(codes, snap, R, st, codes[p], L, off, val, np.array(labels[p], np.int16))
        else:
            ids, ham = O.search_for_build(codes, snap, R, [0], codes[p], L)
        order = sorted(range(len(ids)), key=lambda t: (int(ham[t]), -t))[:vmax]
        vis = [(int(ham[t]), int(ids[t])) for t in order]
        if mate_rows is not None:  # rule 3: each id once, never the row itself; a stable merge on Hamming, the visited first
            have = {v for _, v in vis}
            fresh = [(h, v) for h, v in mate_rows[b] if v != p and v not in have]
            vis = sorted([(h, 0, t, v) for t, (h, v) in enumerate(vis)] + [(h, 1, t, v) for t, (h, v) in enumerate(fresh)])[:vmax]
            vis = [(h, v) for h, _, _, v in vis]
        if labels is not None:  # rule 7
            vis = [(h, v) for h, v in vis if v != p]  # "remove myself"
            if merge_existing:
                have = {v for _, v in vis}
                row = [int(v) for v in nbrs[p] if v != INV and v != p and int(v) not in have]
                if row:
                    vis = vis + list(zip(_ham(codes, np.array(row), p).tolist(), row))
        if labels is not None:
            vis = sorted(vis)  # rule 7: re-sorted by (Hamming, id)
        ids, d = np.array([v for _, v in vis], np.int64), np.array([h for h, _ in vis], np.uint32)
        new = _choose(codes, p, ids, d, R, max_alpha, labels)  # rule 4
        nbrs[p] = INV
        nbrs[p, :len(new)] = new
        dof = dict(zip(ids.tolist(), d.tolist()))
        requests += [(int(q), dof[int(q)], p) for q in new]  # rule 5
    requests.sort(key=lambda r: (r[0], r[1]))  # stable: equal (target, d) keep (batch position, slot) order
    if trace is not None:
        trace.setdefault("targets", []).append(np.array([r[0] for r in requests], np.int64))
    # rule 6
    e = 0
    while e < len(requests):
        q = requests[e][0]
        m = 0
        while e + m < len(requests) and requests[e + m][0] == q:
            m += 1
        req = requests[e:e + m]
        e += m
        live = nbrs[q] != INV
        deg = int(np.argmin(live)) if not live.all() else R
        row = [int(v) for v in nbrs[q, :deg]]
        fresh = [r for r in req if r[2] not in row]
        if trace is not None and len(fresh) < m:
            trace["repeated"] = trace.get("repeated", 0) + m - len(fresh)
        if deg + m <= R:
            new = np.array(row + [r[2] for r in fresh], np.int64)
            if trace is not None:
                trace["appended"] = trace.get("appended", 0) + 1
        else:
            take = min(m, cmax - deg)
            if trace is not None:
                trace["repruned"] = trace.get("repruned", 0) + 1
                trace["cut"] = trace.get("cut", 0) + (take < m)
            pairs = list(zip(_ham(codes, np.array(row, np.int64), q).tolist(), row)) if row else []
            pairs += [(r[1], r[2]) for r in req[:take] if r[2] not in row]
            ids, d = _sorted_pairs(pairs)
            if trace is not None:
                trace["pruned"] = trace.get("pruned", 0) + (len(ids) > R)
            new = _choose(codes, q, ids, d, R, max_alpha, labels)
        nbrs[q] = INV
        nbrs[q, :len(new)] = new
        if trace is not None:
            trace.setdefault("rewritten", set()).add(q)
    return nbrs


def batch_step(codes, nbrs, b0, bn, R, L, max_alpha, mates, labels=None, label_starts=None, trace=None):
    """rows b0 .. b0 + bn - 1 join the graph nbrs (uint32 [>= b0 + bn][R], their own rows INV) -> the new neighbor array.
    codes: every row's code, the new rows' too.  mates: 0 for a build, VS_INSERT_MATES for an insert.  labels: one sorted label list
    per row (None: an unlabeled index); label_starts {label: node}, default the smallest id that carries the label.
    trace (a dict, optional) receives what the step did: 'targets' (one array of request targets per pass), 'appended', 'repruned',
    'cut' (targets with more requests than cmax - deg), 'pruned', 'repeated' (requests whose source the row held), 'rewritten'."""
    codes = np.ascontiguousarray(codes, np.uint64)
    out = np.array(nbrs, np.uint32, copy=True)
    assert out.shape[1] == R and out.shape[0] >= b0 + bn and (out[b0:b0 + bn] == INV).all()
    if labels is None:
        return _run(codes, out, b0, bn, R, L, max_alpha, mates, None, None, False, False, trace)
    starts = label_starts_of(labels) if label_starts is None else label_starts
    _run(codes, out, b0, bn, R, L, max_alpha, mates, labels, starts, True, False, trace)   # from the label start nodes, filtered
    return _run(codes, out, b0, bn, R, L, max_alpha, mates, labels, starts, False, True, trace)  # from node 0, merging


def anchor_batch(nbrs, b0, bn, R):
    """the anchoring of one insert batch (k_insert_anchor to its fixed point, then the placements of anchor_range, in node order):
    a new node is anchored when the row of an older node names it, or the row of an anchored node of the batch does, looking only
    at the rows of its own out-neighbors; an unanchored node takes a slot in the row of its closest old-or-anchored out-neighbor y:
    a free one, else the last one when that entry z keeps an in-edge from an old-or-anchored row other than y among the rows of
    z's own out-neighbors.  Sweeps repeat (flags recomputed from nothing) until nothing is unanchored or nothing can be placed, at
    most eight with placements.  -> (the new neighbor array, orphans placed, orphans left)"""
    nb = np.array(nbrs, np.uint32, copy=True)
    placed = left = 0

    def row(v):
        r = nb[v].tolist()
        return r[:r.index(INV)] if INV in r else r

    for sweep in range(9):
        anch = [False] * bn

        def solid(v):
            return v < b0 or (v - b0 < bn and anch[v - b0])

        grew = True
        while grew:
            grew = False
            for b in range(bn):
                if not anch[b] and any(solid(y) and (b0 + b) in nb[y] for y in row(b0 + b)):
                    anch[b] = grew = True
        left = anch.count(False)
        if left == 0 or sweep == 8:
            break
        done = 0
        for b in range(bn):
            if anch[b]:
                continue
            x = b0 + b
            ok = False
            for y in row(x):  # closest first
                if not solid(y):
                    continue
                if x in nb[y]:  # (a placement earlier in this sweep made y solid)
                    ok = True
                    break
                free = np.flatnonzero(nb[y] == INV)
                slot = int(free[0]) if free.size else -1
                if slot < 0:
                    z = int(nb[y, R - 1])
                    if any(w != y and solid(w) and z in nb[w] for w in row(z)):
                        slot = R - 1
                if slot < 0:
                    continue
                nb[y, slot] = x
                ok = True
                placed += 1
                done += 1
                break
            if ok:
                anch[b] = True
        if not done:
            break
    return nb, placed, left


def schedule(n, batch_max):
    """rule 1: (b0, bn) of the batches of vs_build_graph"""
    batch_max = batch_max or default_batch_max(n)
    b0, bsz = 1, 1
    while b0 < n:
        bn = min(bsz, batch_max, n - b0)
        yield b0, bn
        b0 += bn
        if bsz < batch_max:
            bsz = min(batch_max, bsz * 2)


def build(codes, R, L, max_alpha, batch_max, labels=None, trace=None):
    """vs_build_graph with VS_BUILD_REPAIR=0 -> nbrs uint32 [n][R]; default_start is 0"""
    n = len(codes)
    nbrs = np.full((n, R), INV, np.uint32)
    starts = None if labels is None else label_starts_of(labels)
    for b0, bn in schedule(n, batch_max):
        nbrs = batch_step(codes, nbrs, b0, bn, R, L, max_alpha, 0, labels, starts, trace)
    return nbrs


# ---- measuring a graph ---------------------------------------------------------------------------------------------------------
def reach_count(nbrs, start=0):
    seen = np.zeros(nbrs.shape[0], bool)
    seen[start] = True
    stack = [int(start)]
    while stack:
        v = stack.pop()
        for u in nbrs[v]:
            if u != INV and not seen[u]:
                seen[u] = True
                stack.append(int(u))
    return int(seen.sum())


def first_difference(got, want):
    """'' when the arrays are equal, else the first differing row with both versions of it"""
    bad = np.flatnonzero((got != want).any(1))
    if bad.size == 0:
        return ""
    r = int(bad[0])
    return f"{bad.size} rows differ; first is row {r}:\n device {got[r].tolist()}\n twin   {want[r].tolist()}"
