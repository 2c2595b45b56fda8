"""The numpy restatement of vs_index_consolidate_deletes_plain (tests/test_gpu_zw_consolidate_plain.py; DESIGN.md section 6d, "plain
storage"): `_twin` of tests/test_gpu_zw_consolidate.py with plain_build_checks.PairRule in place of _ham / _prune — the candidates of
a row ordered by PairRule.sorted_candidates (ascending (key of d(p -> w), id), every id once, never p), cut to the cap,
PairRule.prune when more than R remain, and the eight counters as the SBQ twin counts them.  It also says what a case needs to know
about its own input: which rewritten rows had candidates at equal distance, which a candidate at a zero pair distance, and which
arms of the FLT_EPSILON rule the prune took.

Nothing here calls the library under test."""
import numpy as np

from plain_build_checks import EPS, PairRule

INV = 0xFFFFFFFF
COUNTERS = ("tombstones", "tombstones_kept", "rows_rewritten", "edges_dropped", "edges_added", "rows_pruned", "rows_capped", "rows_emptied")


class WatchedRule(PairRule):
    """PairRule that notes the FLT_EPSILON arms its prune takes.  While `point` is set, a call d(a -> b) with a != point is the
    d(existing neighbour -> candidate) of prune's inner loop: below epsilon it is arm "one" when d(point -> b) is below epsilon too,
    else arm "fmax"."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.point = None
        self.arms = set()

    def d(self, a, b):
        v = super().d(a, b)
        if self.point is not None and int(a) != self.point and v < EPS:
            self.arms.add("one" if super().d(self.point, b) < EPS else "fmax")
        return v


def twin(rule, nbrs, tids, start, R, max_alpha=1.2, cand_max=0):
    """-> (rows uint32 [n][R], the eight counters, D bool [n], notes).  rule: a PairRule over the index's vectors; start: the default
    start node (a plain index has no per-label ones).  notes: "ties" = rewritten rows with two candidates at one key inside the cap,
    "zeros" = rewritten rows with a candidate at a pair distance below f32::EPSILON, "arms" = the arms of the epsilon rule taken."""
    n = len(tids)
    dead = (tids & np.uint64(0xFFFF)) == 0
    keep = ~dead
    keep[int(start)] = True                                                          # rule 1
    D = ~keep
    cap = cand_max or min(4 * R, 256)
    out = nbrs.copy()
    st = dict.fromkeys(COUNTERS, 0)
    st["tombstones"], st["tombstones_kept"] = int(dead.sum()), int((dead & keep).sum())
    notes = {"ties": [], "zeros": [], "arms": set()}
    watched = isinstance(rule, WatchedRule)
    for p in range(n):
        if D[p]:
            continue                                                                 # rule 2
        row = nbrs[p][nbrs[p] != INV]
        gone = row[D[row]]
        if gone.size == 0:
            continue                                                                 # rule 3
        st["rows_rewritten"] += 1
        st["edges_dropped"] += int(gone.size)
        cand = set(int(v) for v in row if keep[v])                                   # rule 4
        for d in gone:
            cand |= set(int(w) for w in nbrs[d] if w != INV and keep[w])
        items = rule.sorted_candidates(p, cand)                                      # rules 5, 6: never p, ascending (key, id)
        if len(items) > cap:                                                         # rule 7
            st["rows_capped"] += 1
            items = items[:cap]
        ids = [c for _, c in items]
        if any(a[0] == b[0] for a, b in zip(items, items[1:])):
            notes["ties"].append(p)
        if any(rule.d(p, c) < EPS for c in ids):
            notes["zeros"].append(p)
        if len(ids) <= R:                                                            # rule 8
            new = ids
        else:
            st["rows_pruned"] += 1
            if watched:
                rule.point = p
            new = rule.prune(p, ids, R, max_alpha)
            if watched:
                rule.point = None
        st["rows_emptied"] += int(len(new) == 0)
        st["edges_added"] += len(set(new) - set(row.tolist()))
        out[p] = INV
        out[p, :len(new)] = new
    if watched:
        notes["arms"] = set(rule.arms)
    return out, st, D, notes
