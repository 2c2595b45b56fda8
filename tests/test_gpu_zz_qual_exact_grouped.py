"""The exact and the flat qualified top-k under a group rule (vs_search_batch_qual_exact_grouped / vs_search_batch_qual_flat_grouped
and their _dev forms, vs_qual_group.h): of a scan's qualifying rows in (distance, node id) order, the first k that are not capped out.
The reference is the oracle's bruteforce with k = N on an oracle index with the rows outside C deleted (the `expect` of
tests/test_gpu_zz_qual_exact.py; for the flat call the `expect` of tests/test_gpu_zz_qual_flat.py at k = rescore), which gives C (or S)
in order; the cap is then applied in `capped` below.  Ids, rows and tids are compared with `==`, distances by bit pattern, the tail
included.  Also runs on the lockstep interpreter (tests/test_emu_qual_exact_grouped.py)."""
import numpy as np
import pytest

import test_gpu_zz_qual_exact as X
import test_gpu_zz_qual_flat as F
from helpers import make_vectors, tie_vectors
from oracle import oracle_py as O
from test_gpu_scan_bruteforce import DISTANCES, INV, _bits, _delete, _live_tids, _upload
from test_gpu_zz_qual import options

pytestmark = pytest.mark.gpu
N, NONE = X.N, 0xFFFFFFFF
INVALID, STATE = -1, -5


def capped(full, G, k, per_group):
    """full: (ids, tids, distance bits, ..) of every scan's C in order (an `expect` at k >= |C|) -> ids, tids, bits, rows under the cap"""
    nq = len(full[0])
    out = np.full((nq, k), INV, np.uint32), np.zeros((nq, k), np.uint64), np.full((nq, k), 0x7FC00000, np.uint32), np.zeros(nq, np.uint32)
    for q in range(nq):
        seen, keep = {}, []
        for j, i in enumerate(full[0][q]):
            if i == INV or len(keep) == k:
                break
            if G[i] != NONE:
                seen[G[i]] = seen.get(G[i], 0) + 1
                if seen[G[i]] > per_group:
                    continue
            keep.append(j)
        for o, f in zip(out[:3], full[:3]):
            o[q, :len(keep)] = f[q, keep]
        out[3][q] = len(keep)
    return out


def same_rows(got, exp, what=""):
    """two results of the device against each other"""
    X.assert_equal(got, (exp[0], exp[1], _bits(exp[2]), exp[3]), what)


RULES = [(1, 1), (10, 1), (10, 3), (64, 1), (64, 64)]
CASES = [(dim, d, st, *RULES[i % 5]) for i, (dim, d, st) in
         enumerate((dim, d, st) for dim in (8, 40, 96) for d in DISTANCES for st in ("sbq", "plain"))]


@pytest.mark.parametrize("dim,distance,storage,k,per_group", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_rule_over_list_lengths_tiles_and_k_with_deleted_and_hidden_rows(gpu_ctx, oracle, dim, distance, storage, k, per_group):
    """The shapes of the ungrouped test: seven qualifiers of their own list lengths plus slot 0 in one interleaved batch, TQ - 1 / TQ /
    TQ + 1 / 2 TQ + 1 scans per slot.  The group column is node % 37 with about 5 % ungrouped rows; the list of 32 rows lies in the
    groups 0, 1 and 2 alone, so that a cap below k leaves fewer than k rows of it."""
    dt, plain = DISTANCES[distance], storage == "plain"
    rng = np.random.default_rng(dim + k)
    vecs = make_vectors(N, dim, dim, "gauss") * rng.uniform(0.2, 3.0, (N, 1)).astype(np.float32)
    vecs[:40:4] = 0  # divisor 0
    tids = _live_tids(N)
    _delete(tids, rng.random(N) < 0.05)
    hidden = rng.random(N) < 0.05
    G = (np.arange(N) % 37).astype(np.uint32)
    G[rng.random(N) < 0.05] = NONE
    live = (tids & np.uint64(0xFFFF) != 0) & ~hidden
    free, gone = rng.permutation(np.flatnonzero(live)), np.flatnonzero(~live)
    few = free[G[free] < 3]
    quals, at = {}, 0
    for s, m in enumerate(X.LENGTHS(k), start=1):  # |C| = m; two deleted or hidden rows are named as well
        quals[s] = np.zeros(N, bool)
        quals[s][few[:m] if m == 32 else free[at:at + m]] = True
        quals[s][gone[2 * s:2 * s + 2]] = True
        at += m
    ix = _upload(gpu_ctx, vecs, tids, dt, plain)
    try:
        ix.set_visibility((~hidden).astype(np.uint8))
        ix.groups_put(G)
        for s, b in quals.items():
            ix.qual_put(s, b)
        tq = ix.search_batch_qual_exact(vecs[:1], np.zeros(1, np.uint32), k=k)[4]["tile_queries"]
        slots = rng.permutation(np.repeat(np.arange(8, dtype=np.uint32), [tq + 1, 1, tq - 1, tq, tq + 1, 2 * tq + 1, 1, tq]))
        q = make_vectors(len(slots), dim, dim + 1, "gauss")
        full = X.expect(vecs, tids, dt, plain, q, slots, quals, N, hidden)
        exp = capped(full, G, k, per_group)
        if per_group < k:  # preconditions, on the reference alone: the rule bites, leaves fewer than k rows of a list of >= k, ...
            assert (exp[0] != full[0][:, :k]).any()
            assert ((exp[3] < k) & (full[3] >= k)).any()
            kept = exp[0][exp[0] != INV]
            assert (G[kept] == 0).any() and (G[kept] == NONE).any()  # ... and keeps rows of group 0 and ungrouped rows
        X.assert_equal(ix.search_batch_qual_exact_grouped(q, slots, k=k, per_group=per_group), exp)
    finally:
        ix.close()


def test_forced_slices_and_tiles_change_no_row_on_a_tie_heavy_corpus(gpu_ctx, oracle):
    """40 distinct vectors over 200 listed rows in 7 groups: equal distances inside a group and across groups, rows of one group on
    both sides of the boundary of two slices (list place 128); under a cap of 2 the list of 10 is filled through replacements."""
    k, per_group, dim, nq = 10, 2, 40, 9
    vecs, q, tids = tie_vectors(N, 40, dim, 5), tie_vectors(nq, 40, dim, 7), _live_tids(N)
    G = (np.arange(N) % 7).astype(np.uint32)
    rows = np.sort(np.random.default_rng(8).choice(N, 200, replace=False))
    bits = np.isin(np.arange(N), rows)
    slots = np.ones(nq, np.uint32)
    full = X.expect(vecs, tids, O.L2, False, q, slots, {1: bits}, 200)
    exp = capped(full, G, k, per_group)
    tie = full[2][:, 1:] == full[2][:, :-1]
    same = G[full[0][:, 1:]] == G[full[0][:, :-1]]
    assert (tie & same).any() and (tie & ~same).any() and (exp[0] != full[0][:, :k]).any()
    place, g = np.searchsorted(rows, exp[0]), G[exp[0]]
    assert np.any([(g[:, a] == g[:, b]) & (place[:, a] < 128) & (place[:, b] >= 128) for a in range(k) for b in range(k)])
    ix = _upload(gpu_ctx, vecs, tids, O.L2)
    try:
        ix.qual_put(1, bits)
        ix.groups_put(G)
        for S in (1, 2, 7):
            for T in (1, 2, 4, 8, 16):  # every instantiation of the tile
                with options(VS_QUAL_EXACT_SLICES=S, VS_QUAL_EXACT_TQ=T):
                    got = ix.search_batch_qual_exact_grouped(q, slots, k=k, per_group=per_group)
                X.assert_equal(got, exp, f"{S} slices, tiles of {T}")
                assert (got[4]["slices"], got[4]["tile_queries"]) == (S, T)
    finally:
        ix.close()


@pytest.mark.parametrize("column", ["per_group_is_k", "all_ungrouped"])
def test_a_rule_that_cannot_bite_gives_the_ungrouped_rows(gpu_ctx, oracle, column):
    k, dim, dt = 10, 40, O.L2
    tids = _live_tids(N)
    bits = np.random.default_rng(4).random(N) < 0.1
    slots = (np.arange(11) % 2).astype(np.uint32)
    q = make_vectors(len(slots), dim, 9, "gauss")
    ix = F.upload(gpu_ctx, dim, dt, tids)
    try:
        ix.qual_put(1, bits)
        ix.groups_put(np.arange(N) % 3 if column == "per_group_is_k" else np.full(N, NONE))
        per_group = k if column == "per_group_is_k" else 1
        same_rows(ix.search_batch_qual_exact_grouped(q, slots, k=k, per_group=per_group), ix.search_batch_qual_exact(q, slots, k=k))
        same_rows(ix.search_batch_qual_flat_grouped(q, slots, k=k, per_group=per_group, rescore=33), ix.search_batch_qual_flat(q, slots, k=k, rescore=33))
    finally:
        ix.close()


@pytest.mark.parametrize("rescore", [16, 40, 4096])
def test_flat_grouped_caps_the_candidates_in_exact_order(gpu_ctx, oracle, rescore):
    """rescore 16 / 40: S is the oracle's (Hamming, node id) selection over the oracle's codes, taken without the rule; 4096 >= |C|:
    the rows of the exact grouped call."""
    k, per_group, dim, dt = 10, 2, 96, O.COSINE
    tids = _live_tids(N)
    _delete(tids, np.arange(N) % 17 == 3)
    bits = np.random.default_rng(4).random(N) < 0.1
    G = (np.arange(N) % 5).astype(np.uint32)
    G[::11] = NONE
    slots = (np.arange(11) % 2).astype(np.uint32)
    q = make_vectors(len(slots), dim, 9, "gauss")
    ix = F.upload(gpu_ctx, dim, dt, tids)
    try:
        ix.qual_put(1, bits)
        ix.groups_put(G)
        got = ix.search_batch_qual_flat_grouped(q, slots, k=k, per_group=per_group, rescore=rescore)
        if rescore == 4096:
            same_rows(got, ix.search_batch_qual_exact_grouped(q, slots, k=k, per_group=per_group))
        else:
            full = F.expect(dim, dt, tids, q, slots, {1: bits}, rescore, rescore)
            exp = capped(full, G, k, per_group)
            assert (exp[0] != full[0][:, :k]).any()  # precondition: the rule bites
            X.assert_equal(got, exp)
    finally:
        ix.close()


def _dev(gpu_ctx, call, q, slots, k, *rule):
    """a _dev form over poison-filled buffers of its own -> (ids, tids, dist, rows) or, refused, (code, whether nothing was written)"""
    import pgvectorscale_amd as P
    nq = len(q)
    outs = [np.empty((nq, k), np.uint32), np.empty((nq, k), np.uint64), np.empty((nq, k), np.float32), np.empty(nq, np.uint32)]
    bufs = [gpu_ctx.alloc(a.nbytes) for a in (q, slots, *outs)]
    try:
        gpu_ctx.upload(bufs[0], q)
        gpu_ctx.upload(bufs[1], slots)
        for b, a in zip(bufs[2:], outs):
            gpu_ctx.upload(b, np.full(a.nbytes, 0xA5, np.uint8))
        try:
            call(bufs[0], nq, k, *rule, bufs[1], bufs[2], bufs[5], d_out_tids=bufs[3], d_out_dist=bufs[4])
        except P.VsError as e:
            return e.code, all((gpu_ctx.download(b, a).view(np.uint8) == 0xA5).all() for b, a in zip(bufs[2:], outs))
        return [gpu_ctx.download(b, a) for b, a in zip(bufs[2:], outs)]
    finally:
        for b in bufs:
            gpu_ctx.free(b)


def test_the_device_entry_points_and_the_refusals(gpu_ctx, oracle):
    k, dim, dt = 10, 40, O.IP
    bits = np.random.default_rng(3).random(N) < 0.1
    slots = (np.arange(11) % 2).astype(np.uint32)
    q = make_vectors(len(slots), dim, 2, "gauss")
    ix = F.upload(gpu_ctx, dim, dt, _live_tids(N))
    try:
        ix.qual_put(1, bits)
        for code, kk, per_group in [(STATE, k, 1), (INVALID, k, 0), (INVALID, k, k + 1), (INVALID, 65, 1)]:  # (k = 65: the ungrouped call's)
            if code == INVALID:  # (STATE: no group column yet)
                ix.groups_put(np.arange(N) % 4)
            assert _dev(gpu_ctx, ix.search_batch_qual_exact_grouped_dev, q, slots, kk, per_group) == (code, True), (kk, per_group)
            assert _dev(gpu_ctx, ix.search_batch_qual_flat_grouped_dev, q, slots, kk, per_group, 70) == (code, True), (kk, per_group)
        same_rows(_dev(gpu_ctx, ix.search_batch_qual_exact_grouped_dev, q, slots, k, 2), ix.search_batch_qual_exact_grouped(q, slots, k=k, per_group=2))
        same_rows(_dev(gpu_ctx, ix.search_batch_qual_flat_grouped_dev, q, slots, k, 2, 33),
                  ix.search_batch_qual_flat_grouped(q, slots, k=k, per_group=2, rescore=33))
        assert ix.search_batch_qual_exact_grouped(q[:0], slots[:0], k=k)[3].size == 0  # nq = 0
    finally:
        ix.close()
