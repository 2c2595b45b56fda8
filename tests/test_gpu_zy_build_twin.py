"""The batch step of the SBQ build and insert against its sequential restatement (tests/build_twin.py; DESIGN.md section 6b, rules
1 to 7): the build-mode search's visited list on both search kernels, the candidate assembly of k_build_prune_new and
k_build_prune_merge, k_insert_merge_mates, the request keys with their stable sort and k_seg_heads, and k_build_backedges (append
versus re-prune, the cmax - deg cut, sources a row already holds, label masks relative to the target).

Every comparison is of whole neighbor arrays with ==; the message names the first differing row and shows both versions of it.  No
number in this file is a tolerance.  Every case asserts on the restatement's own trace that it reaches the branch it is about before
it looks at the device.  Also runs on the lockstep interpreter (tests/test_emu_build_twin.py)."""
import contextlib
import functools

import numpy as np
import pytest

import build_twin as T
from helpers import TestIndex, make_vectors
from lifecycle_checks import make_tids, well_formed

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF
ALPHA = 1.2
# (n, dim, bits, R, L, kind of data)
GEOMETRIES = {
    "general": (1500, 32, 2, 16, 40, "gauss"),
    "ties": (1200, 8, 1, 8, 40, "uniform"),          # at most 256 distinct codes: heavy ties in every order
    "w24": (400, 768, 2, 20, 30, "gauss"),           # 24-word codes: code rows staged in LDS, the register form of the prune
    "tiny_list": (800, 16, 2, 4, 1, "gauss"),
    "wide_row": (900, 32, 2, 100, 120, "gauss"),     # R > 64: the second trip of the row loops
}
LABELED = (1000, 32, 2, 24, 60, "gauss")
N_LABELS = 12
GROW = 70  # rows the two-kernel case inserts after the build


@contextlib.contextmanager
def _options(**kw):
    import pgvectorscale_amd as P
    try:
        for k, v in kw.items():
            P.set_option(k, v)
        yield
    finally:
        for k in kw:
            P.set_option(k, None)


def _label_sets(n, seed):
    rng = np.random.default_rng(seed)
    return [sorted(set(int(v) for v in rng.integers(1, N_LABELS + 1, int(rng.integers(1, 4))))) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _vectors(name):
    n, dim, _, _, _, kind = LABELED if name == "labeled" else GEOMETRIES[name]
    return make_vectors(n + GROW, dim, 100 + sorted(list(GEOMETRIES) + ["labeled"]).index(name), kind)


def _fresh(gpu_ctx, X, bits, R, labels=None):
    """an index over the rows of X on the device: norms, training, codes, label sets; no graph yet"""
    import pgvectorscale_amd as P
    n, dim = X.shape
    ix = P.DiskAnnIndex.alloc(gpu_ctx, n=n, dim_full=dim, bits=bits, num_neighbors=R, distance_type=P.VS_L2)
    vp, stride = ix.array(P._lib.ARR_VECS)
    Xp = np.zeros((n, stride), np.float32)
    Xp[:, :dim] = X
    gpu_ctx.upload(vp, Xp)
    ix.refresh_norms()
    ix.sbq_train()
    ix.sbq_quantize_corpus()
    if labels is not None:
        off, val = T._csr(labels)
        ix.set_labels(off, val)
    return ix


_TWINS = {}


def _twin_build(key, codes, R, L, batch_max, labels=None):
    """build_twin.build, computed once per (geometry, batch_max) and shared; the codes must be the ones it was computed for"""
    hit = _TWINS.get(key)
    if hit is None:
        trace = {}
        hit = _TWINS[key] = (codes.tobytes(), T.build(codes, R, L, ALPHA, batch_max, labels, trace), trace)
    assert hit[0] == codes.tobytes(), "the device quantised the same vectors differently"
    return hit[1], hit[2]


def _same(got, want, what=""):
    msg = T.first_difference(got, want)
    assert not msg, what + msg


def _insert_against_twin(ix, Xnew, R, L, mates, labels_all=None, new_labels=None, label_starts=None, trace=None, max_alpha=ALPHA,
                         may_place=False):
    """one insert batch -> (before, after, twin rows): batch_step on the state downloaded before the insert.  The conditions of an
    insert case are asserted here: one batch, no search re-run, no orphan placed or left.  may_place (the geometries that place
    orphans on every seed): the anchoring is restated too (build_twin.anchor_batch), and the counts must be the restatement's."""
    before = ix.download()
    n0, m = before["nbrs"].shape[0], len(Xnew)
    with _options(VS_INSERT_MATES=mates):
        st = ix.insert(Xnew, make_tids(n0, m), labels=new_labels, search_list_size=L, max_alpha=max_alpha, batch_max=m)
    after = ix.download()
    assert after["codes"][:n0].tobytes() == before["codes"].tobytes()
    assert st["batches"] == 1 and st["retries"] == 0, st
    grown = np.vstack([before["nbrs"], np.full((m, R), INV, np.uint32)])
    want = T.batch_step(after["codes"], grown, n0, m, R, L, max_alpha, mates, labels_all, label_starts, trace)
    placed = left = 0
    if may_place:
        want, placed, left = T.anchor_batch(want, n0, m, R)
        print("orphans placed", placed, "left", left)
    assert (st["orphans_placed"], st["orphans_left"]) == (placed, left), st
    return before, after, want


# ---- case 1: whole builds without the repair pass ----------------------------------------------------------------------------------
@pytest.mark.parametrize("batch_max", [0, 64])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_build_without_repair_equals_the_restatement(gpu_ctx, oracle, name, batch_max):
    n, dim, bits, R, L, _ = GEOMETRIES[name]
    ix = _fresh(gpu_ctx, _vectors(name)[:n], bits, R)
    with _options(VS_BUILD_REPAIR=0):
        ix.build_graph(search_list_size=L, max_alpha=ALPHA, batch_max=batch_max)
    host = ix.download()
    assert ix.desc.default_start == 0
    if name == "w24":
        assert host["codes"].shape[1] == 24
    if name == "ties":
        assert len({c.tobytes() for c in host["codes"]}) <= 256
    want, trace = _twin_build((name, batch_max), host["codes"], R, L, batch_max)
    print(name, batch_max, {k: v for k, v in trace.items() if isinstance(v, int)})
    assert trace["appended"] > 0 and trace["repruned"] > 0 and trace["pruned"] > 0  # both branches of the back-edge kernel
    _same(host["nbrs"], want)
    ix.close()


# ---- case 2: one insert batch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mates", [0, 16], ids=["no_mates", "default_mates"])
@pytest.mark.parametrize("name", ["general", "ties", "w24"])
def test_one_insert_batch_equals_the_restatement(gpu_ctx, oracle, name, mates):
    n, dim, bits, R, L, kind = GEOMETRIES[name]
    ti = TestIndex(n=n, dim_full=dim, bits=bits, R=R, distance=oracle.L2, seed=300 + len(name), kind=kind, L_build=L)
    ix = ti.upload(gpu_ctx)
    Xnew = make_vectors(64, dim, 400 + len(name), kind)
    trace = {}
    before, after, want = _insert_against_twin(ix, Xnew, R, L, mates, trace=trace, may_place=name == "ties")
    assert trace["repruned"] > 0  # an old row is full: a back-edge into it is a re-prune
    new_targets = sum(int((t >= n).sum()) for t in trace["targets"])
    assert (new_targets > 0) == (mates > 0)  # with mates a row of the batch is asked for back-edges
    _same(after["nbrs"], want)
    well_formed(after["nbrs"], R)
    ix.close()


# ---- case 3: a hub that receives more requests than cmax - deg ---------------------------------------------------------------------
def test_a_hub_keeps_only_its_closest_requests(gpu_ctx, oracle):
    n, dim, R, L, m = 600, 32, 8, 40, 300
    cmax = T.cmax_of(R)
    assert cmax == 256
    ti = TestIndex(n=n, dim_full=dim, bits=2, R=R, distance=oracle.L2, seed=31, kind="gauss", L_build=L)
    ix = ti.upload(gpu_ctx)
    rng = np.random.default_rng(32)
    Xnew = (make_vectors(1, dim, 33, "gauss") + 0.05 * rng.standard_normal((m, dim))).astype(np.float32)
    trace = {}
    before, after, want = _insert_against_twin(ix, Xnew, R, L, 0, trace=trace, may_place=True)
    counts = np.bincount(trace["targets"][0], minlength=n + m)
    hub = int(np.argmax(counts))
    print("requests of the busiest target:", int(counts[hub]), "target", hub, "targets cut", trace["cut"])
    assert counts[hub] > cmax - R and hub < n and trace["cut"] > 0  # the case is real: take_new < m at an old, full row
    # Nearly every source the hub drops is an orphan afterwards, and the hub is the closest old out-neighbor of each: the
    # placements go through the hub's own row.  So no row is left out of the comparison: the anchoring is restated as well, and
    # the hub's row is also compared as the back-edge kernel left it, in every slot but the last, the one a placement may take.
    step = T.batch_step(after["codes"], np.vstack([before["nbrs"], np.full((m, R), INV, np.uint32)]), n, m, R, L, ALPHA, 0)
    assert (step[hub] != INV).all()
    _same(after["nbrs"][hub:hub + 1, :R - 1], step[hub:hub + 1, :R - 1], f"the hub, row {hub}, before any placement: ")
    _same(after["nbrs"][hub:hub + 1], want[hub:hub + 1], f"the hub, row {hub}: ")
    _same(after["nbrs"], want)
    ix.close()


# ---- case 4: the append branch ------------------------------------------------------------------------------------------------------
def test_back_edges_are_appended_while_a_row_has_room(gpu_ctx, oracle):
    import pgvectorscale_amd as P
    n, dim, R, L = 700, 32, 32, 40
    X = make_vectors(n, dim, 41, "gauss")
    mean, m2, cnt = oracle.train(X, 2)
    codes = oracle.quantize(mean, m2, cnt, 2, X)
    nbrs, start = oracle.build_graph(codes, num_neighbors=R // 2, nbr_stride=R, search_list_size=L)  # rows at most half full
    assert ((nbrs != INV).sum(1) <= R // 2).all()
    ix = P.DiskAnnIndex.upload(gpu_ctx, codes=codes, nbrs=nbrs, heap_tids=make_tids(0, n), vecs=X, mean=mean, m2=m2, count=cnt, bits=2,
                               dim_index=dim, num_neighbors=R, distance_type=P.VS_L2, default_start=start)
    rng = np.random.default_rng(42)
    base = make_vectors(4, dim, 43, "gauss")
    first = np.repeat(base, 2, axis=0) + 0.05 * rng.standard_normal((8, dim)).astype(np.float32)  # four pairs: mutual mates
    second = first + 0.05 * rng.standard_normal((8, dim)).astype(np.float32)                       # the neighbors of the same vectors
    for Xnew in (first, second):
        trace = {}
        # max_alpha = 1: one strict pass of the prune leaves the new rows room too, so no target of the batch is ever full
        before, after, want = _insert_against_twin(ix, Xnew.astype(np.float32), R, L, 16, trace=trace, max_alpha=1.0)
        print({k: v for k, v in trace.items() if isinstance(v, int)})
        assert trace["appended"] > 0 and trace.get("repruned", 0) == 0  # every back-edge of this batch is appended
        assert trace.get("repeated", 0) > 0  # a mate asks for an edge its mate's row already holds: dropped, not appended twice
        _same(after["nbrs"], want)
        n0 = before["nbrs"].shape[0]
        for q in sorted(trace["rewritten"]):  # appended: the row as it was, then the sources in sorted order
            if q < n0:
                deg = int((before["nbrs"][q] != INV).sum())
                assert (after["nbrs"][q, :deg] == before["nbrs"][q, :deg]).all()
        well_formed(after["nbrs"], R)
    ix.close()


# ---- case 5: labeled sets -----------------------------------------------------------------------------------------------------------
def test_labeled_build_and_insert_equal_the_restatement(gpu_ctx, oracle):
    n, dim, bits, R, L, _ = LABELED
    X = _vectors("labeled")
    labels = _label_sets(n + 32, 51)
    assert set(l for s in labels[:n] for l in s) == set(range(1, N_LABELS + 1))  # the insert brings no new label
    ix = _fresh(gpu_ctx, X[:n], bits, R, labels[:n])
    with _options(VS_BUILD_REPAIR=0):
        ix.build_graph(search_list_size=L, max_alpha=ALPHA)
    host = ix.download()
    want, trace = _twin_build(("labeled", 0), host["codes"], R, L, 0, labels[:n])
    print({k: v for k, v in trace.items() if isinstance(v, int)})
    assert trace["repeated"] > 0 and trace["pruned"] > 0  # the second pass asks again for the back-edges of the first
    _same(host["nbrs"], want, "build: ")
    trace = {}
    before, after, want = _insert_against_twin(ix, X[n:n + 32], R, L, 16, labels_all=labels, new_labels=labels[n:],
                                             label_starts=T.label_starts_of(labels[:n]), trace=trace)
    assert trace["repeated"] > 0 and trace["repruned"] > 0
    _same(after["nbrs"], want, "insert: ")
    ix.close()


# ---- case 6: both search kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMETRIES) + ["labeled"])
def test_both_build_search_kernels_give_the_same_graph(gpu_ctx, oracle, name):
    n, dim, bits, R, L, _ = LABELED if name == "labeled" else GEOMETRIES[name]
    X = _vectors(name)
    labels = _label_sets(n + GROW, 51) if name == "labeled" else None
    graphs = {}
    for fast in ("1", "0"):
        with _options(VS_BUILD_FAST=fast):
            ix = _fresh(gpu_ctx, X[:n], bits, R, None if labels is None else labels[:n])
            ix.build_graph(search_list_size=L, max_alpha=ALPHA)
            built = ix.download()["nbrs"]
            st = ix.insert(X[n:], make_tids(n, GROW), labels=None if labels is None else labels[n:], search_list_size=L,
                           max_alpha=ALPHA)
            assert st["retries"] == 0, st
            graphs[fast] = (built, ix.download()["nbrs"], st)
            ix.close()
    assert graphs["1"][0].tobytes() == graphs["0"][0].tobytes(), "after the build: " + T.first_difference(graphs["1"][0], graphs["0"][0])
    assert graphs["1"][1].tobytes() == graphs["0"][1].tobytes(), "after the insert: " + T.first_difference(graphs["1"][1], graphs["0"][1])
    assert graphs["1"][2] == graphs["0"][2]


# ---- case 7: rows wider than a wave -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [65, 128])
def test_rows_wider_than_a_wave(gpu_ctx, oracle, R):
    n, dim, L, m = 500, 16, 100, 64
    X = make_vectors(n + m, dim, 70 + R, "gauss")
    ix = _fresh(gpu_ctx, X[:n], 2, R)
    with _options(VS_BUILD_REPAIR=0):
        ix.build_graph(search_list_size=L, max_alpha=ALPHA)
    host = ix.download()
    want, trace = _twin_build(("wide", R), host["codes"], R, L, 0)
    well_formed(host["nbrs"], R)
    assert ((host["nbrs"] != INV).sum(1).max() > 64) and trace["repruned"] > 0  # rows do take the second trip, and are re-pruned
    _same(host["nbrs"], want, "build: ")
    assert T.reach_count(host["nbrs"]) == T.reach_count(want)
    before, after, want = _insert_against_twin(ix, X[n:], R, L, 16)
    well_formed(after["nbrs"], R)
    _same(after["nbrs"], want, "insert: ")
    assert T.reach_count(after["nbrs"]) == T.reach_count(want)
    ix.close()
