"""vs_pages_follow_*: a device-resident index brought up to date from the blocks of its relation that something else changed.
Every expectation comes from tests/pages_follow_checks.py: a state S0 and its successor S1 as flat numpy arrays, both written as
relations by the oracle's writer, the dirty block list by a bytewise page compare, the info counters counted from the arrays.
After an apply (i) the downloaded codes, neighbor rows (padding included), tids, vectors, cosine divisors, label CSR and n are
S1's, (ii) they are, byte for byte, those of an index staged in full from the new relation with DevicePages, (iii) search_batch
rows and distance bits are the oracle's over S1, (iv) the counters are the numpy counts.  Also runs on the lockstep interpreter
(tests/test_emu_pages_follow.py)."""
import ctypes as C

import numpy as np
import pytest

import lifecycle_checks as LC
import pages_follow_checks as FC
from pages_follow_checks import B, INV

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

INVALID, STATE = -1, -5


# ---- the shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(oracle):
    """classic nodes, 24-word codes, R = 50: 12 items per page, so 130 rows leave 10 on the last page"""
    return FC.Family(dim=768, bits=2, R=50, distance=oracle.L2, n_max=190, seed=3)


@pytest.fixture(scope="module")
def narrow(oracle):
    """one-word codes, R = 4: 107 items per page — more items than lanes; code rows carry a padding word"""
    return FC.Family(dim=32, bits=2, R=4, distance=oracle.L2, n_max=500, seed=4)


@pytest.fixture(scope="module")
def labeled(oracle):
    """labeled nodes, 4-word codes, R = 8, 0..4 labels per row, cosine; one appended row carries label 300, which no old row has"""
    return FC.Family(dim=128, bits=2, R=8, distance=oracle.COSINE, n_max=590, seed=5, labeled=True, fresh_label=300)


# ---- staging, following, comparing ----------------------------------------------------------------------------------------------------
def _stage_full(ctx, raw, vecs):
    """an index staged in full from a relation with the device reader -> (index, reader)"""
    from pgvectorscale_amd.pages import DevicePages
    dp = DevicePages(ctx, len(raw) // B)
    dp.add(raw)
    return dp.build_from_meta(vecs=vecs), dp


def _staged(ctx, raw, vecs):
    """-> (index, follower)"""
    ix, dp = _stage_full(ctx, raw, vecs)
    fol = dp.follower(ix)
    dp.close()
    return ix, fol


def _bytes_of(ix):
    """everything the equality standard names, as the device holds it (rows at their device strides)"""
    from pgvectorscale_amd import _lib
    ix._refresh()
    n, ctx = ix.desc.n, ix.ctx
    out = {"n": n}
    for name, which, dt in (("codes", _lib.ARR_CODES, np.uint64), ("nbrs", _lib.ARR_NBRS, np.uint32), ("tids", _lib.ARR_TIDS, np.uint64),
                            ("vnorm", _lib.ARR_VNORM, np.float32)):
        ptr, stride = ix.array(which)
        out[name] = ctx.download(ptr, np.empty((n, stride), dt)).tobytes() if ptr.value and n else b""
    out["vecs"] = ix.download(codes=False, nbrs=False, tids=False, vecs=True)["vecs"].tobytes()
    if ix.desc.has_labels:
        off, val = LC.download_labels(ix)
        out["label_off"], out["label_val"] = off.tobytes(), val.tobytes()
    return out


def _equals_state(ix, fam, s, where=""):
    """(i): the arrays on the device are s's"""
    from pgvectorscale_amd import _lib
    ix._refresh()
    assert ix.desc.n == s.n, where
    host = ix.download(vecs=True)
    assert (host["codes"] == s.codes).all() and (host["heap_tids"] == s.tids).all() and host["vecs"].tobytes() == s.vecs.tobytes(), where
    ptr, stride = ix.array(_lib.ARR_NBRS)
    rows = ix.ctx.download(ptr, np.empty((s.n, stride), np.uint32))
    want = np.full((s.n, stride), INV, np.uint32)
    want[:, :fam.R] = s.nbrs
    assert (rows == want).all(), (where, "neighbor rows, padding included", np.flatnonzero((rows != want).any(1))[:4])
    ptr, stride = ix.array(_lib.ARR_CODES)
    rows = ix.ctx.download(ptr, np.empty((s.n, stride), np.uint64))
    assert (rows[:, fam.W:] == 0).all(), (where, "code row padding")
    vn = ix.array(_lib.ARR_VNORM)[0]
    if vn.value:
        assert ix.ctx.download(vn, np.empty(s.n, np.float32)).tobytes() == LC.cosine_divisors(s.vecs).tobytes(), (where, "vnorm")
    if s.label_off is not None:
        off, val = LC.download_labels(ix)
        assert (off == s.label_off).all() and (val == s.label_val).all(), (where, "label CSR")


def _follow(fol, before, after, new_vecs, want_info):
    """the dirty blocks of before -> after through the follower; the counters of stage and apply are want_info"""
    from pgvectorscale_amd.pages import dirty_blocks
    blocks = dirty_blocks(before, after)
    assert blocks.tolist() == FC.dirty(before, after)
    info = fol.stage(blocks, FC.gather(after, blocks), len(after) // B)
    assert info == want_info, (info, want_info)
    done = fol.apply(new_vecs)
    assert done == want_info
    return blocks


def _check_step(ctx, ix, fol, fam, s0, s1, before, after, q, where=""):
    """one followed step held to (i) .. (iv)"""
    blocks = FC.dirty(before, after)
    want = FC.expected_info(s0, s1, before, after, blocks)
    from pgvectorscale_amd.pages import dirty_blocks
    info = fol.stage(dirty_blocks(before, after), FC.gather(after, blocks), len(after) // B)
    assert info == want, (where, info, want)                                                         # (iv)
    tids = fol.new_tids()
    assert (tids == s1.tids[s0.n:]).all(), where
    untouched = _bytes_of(ix)
    assert untouched["n"] == s0.n, (where, "the check pass wrote")
    assert fol.apply(s1.vecs[s0.n:] if s1.n > s0.n else None) == want, where
    _equals_state(ix, fam, s1, where)                                                                # (i)
    if s1.label_off is not None:
        ix.set_start_nodes(s1.start, s1.label_starts)  # (the MetaPage is the caller's to decode)
    full, dp = _stage_full(ctx, after, s1.vecs)
    dp.close()
    try:
        assert _bytes_of(ix) == _bytes_of(full), (where, "differs from an index staged in full from the new relation")  # (ii)
    finally:
        full.close()
    LC.check_search_batch(ix, fam.oracle(s1), q, None, where)                                        # (iii)
    return want


# ---- 1, 2: appends across the page boundary -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 40])
def test_append_across_the_page_boundary(gpu_ctx, wide, m):
    """130 rows leave 10 on the last page: 1 fits, 2 fill it exactly, 3 open one page, 40 several; 30 rows relinked, 9 tids cleared"""
    fam = wide
    s0 = fam.s0(130)
    s1 = fam.mutate(s0, m, 30, 9, seed=10 + m)
    before, ptrs0 = fam.relation(s0)
    after, ptrs1 = fam.relation(s1)
    assert ptrs1[:130] == ptrs0 and ptrs0[129][1] == 10 and max(p[1] for p in ptrs0) == 12
    assert (len(after) - len(before)) // B == {1: 0, 2: 0, 3: 1, 40: 4}[m]
    ix, fol = _staged(gpu_ctx, before, s0.vecs)
    want = _check_step(gpu_ctx, ix, fol, fam, s0, s1, before, after, fam.vecs[120:152] * 1.01, ("append", m))
    assert want["rows_relinked"] == 30 and want["tids_cleared"] == 9 and want["n_appended"] == m and want["codes_changed"] == 0
    assert (s1.nbrs[:130][s1.nbrs[:130] != INV] >= 130).any(), "an old row names an appended node"
    fol.close()
    ix.close()


def test_full_last_page_then_one_row(gpu_ctx, wide):
    """24 rows fill two pages exactly: one more row is a new page and nothing else"""
    fam = wide
    s0 = fam.s0(24)
    s1 = fam.mutate(s0, 1, 0, 0, seed=2)
    before, ptrs0 = fam.relation(s0)
    after, _ = fam.relation(s1)
    assert ptrs0[23][1] == 12 and len(after) == len(before) + B and FC.dirty(before, after) == [len(before) // B]
    ix, fol = _staged(gpu_ctx, before, s0.vecs)
    _check_step(gpu_ctx, ix, fol, fam, s0, s1, before, after, fam.vecs[:32], "full last page")
    fol.close()
    ix.close()


# ---- 3, 5: more items than lanes; zero pages ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_page_every", [0, 97])
def test_more_items_than_lanes(gpu_ctx, narrow, zero_page_every):
    """107 one-word items per page; with zero_page_every = 97 all-zero blocks sit among the old pages and in the tail"""
    fam = narrow
    s0 = fam.s0(300)
    s1 = fam.mutate(s0, 200, 40, 12, seed=6)
    before, ptrs0 = fam.relation(s0, zero_page_every)
    after, ptrs1 = fam.relation(s1, zero_page_every)
    assert ptrs1[:300] == ptrs0
    if zero_page_every:
        new = [b for b in range(len(after) // B) if after[b * B + 14:b * B + 16] == b"\0\0"]
        assert any(b < len(before) // B for b in new) and any(b >= len(before) // B for b in new)
    else:
        assert max(p[1] for p in ptrs1) == 107
    ix, fol = _staged(gpu_ctx, before, s0.vecs)
    _check_step(gpu_ctx, ix, fol, fam, s0, s1, before, after, fam.vecs[280:312] * 1.01, ("narrow", zero_page_every))
    fol.close()
    ix.close()


# ---- 4: labeled nodes -----------------------------------------------------------------------------------------------------------------
def test_labeled_nodes(gpu_ctx, labeled):
    fam = labeled
    s0 = fam.s0(500)
    s1 = fam.mutate(s0, 90, 40, 12, seed=8)
    assert 300 not in s0.label_starts and s1.label_starts[300] == 545
    before, ptrs0 = fam.relation(s0)
    after, ptrs1 = fam.relation(s1)
    assert ptrs1[:500] == ptrs0
    ix, fol = _staged(gpu_ctx, before, s0.vecs)
    q = fam.vecs[480:512] * 1.01
    want = _check_step(gpu_ctx, ix, fol, fam, s0, s1, before, after, q, "labeled")
    assert want["label_vals_appended"] == int(s1.label_off[590]) - int(s0.label_off[500]) > 0
    # label-filtered scans after set_start_nodes, the label only an appended row carries among the keys
    keys = [[300] if i == 0 else [1 + i % 6] for i in range(len(q))]
    gi = LC.check_search_batch(ix, fam.oracle(s1), q, keys, "labeled, keyed")
    assert gi[0][0] == 545
    # an existing node's label bytes patched in its page: the CSR cannot change in place
    u = next(i for i in range(500) if s0.label_off[i + 1] > s0.label_off[i])
    blk, off = ptrs1[u]
    page = bytearray(after[blk * B:(blk + 1) * B])
    _, at = FC.field_at(page, off, 24)
    page[at] ^= 0x40
    held = _bytes_of(ix)
    import pgvectorscale_amd as P
    with pytest.raises(P.VsError) as e:
        fol.stage([blk], bytes(page), len(after) // B)
    assert e.value.code == INVALID and "label set of an existing node changed" in str(e.value)
    assert _bytes_of(ix) == held
    assert fol.stage([blk], after[blk * B:(blk + 1) * B], len(after) // B)["rows_relinked"] == 0  # (the page as it is: nothing to do)
    fol.close()
    ix.close()


# ---- 6: updates only ------------------------------------------------------------------------------------------------------------------
def test_updates_only_move_nothing(gpu_ctx, wide):
    from pgvectorscale_amd import _lib
    fam = wide
    s0 = fam.s0(130)
    s1 = fam.mutate(s0, 0, 0, 0, seed=1)
    for node in (3, 60, 125):  # (three pages)
        assert s1.tids[node] & FC.OFFSET
        s1.tids[node] &= ~FC.OFFSET
    before, ptrs = fam.relation(s0)
    after, _ = fam.relation(s1)
    assert FC.dirty(before, after) == sorted(ptrs[i][0] for i in (3, 60, 125)) and len(set(FC.dirty(before, after))) == 3
    ix, fol = _staged(gpu_ctx, before, s0.vecs)
    where = [ix.array(w)[0].value for w in (_lib.ARR_CODES, _lib.ARR_NBRS, _lib.ARR_TIDS, _lib.ARR_VECS)]
    cap = ix.capacity
    want = _check_step(gpu_ctx, ix, fol, fam, s0, s1, before, after, fam.vecs[:32], "updates only")
    assert want["n_appended"] == 0 and want["tids_cleared"] == 3 and want["rows_relinked"] == 0
    assert ix.desc.n == 130 and ix.capacity == cap
    assert [ix.array(w)[0].value for w in (_lib.ARR_CODES, _lib.ARR_NBRS, _lib.ARR_TIDS, _lib.ARR_VECS)] == where
    fol.close()
    ix.close()


# ---- 7: capacity ----------------------------------------------------------------------------------------------------------------------
def test_capacity_grows_by_the_inserts_rule(gpu_ctx, wide):
    """the same apply with and without a prior reserve: the same bytes; the arrays move only without it"""
    from pgvectorscale_amd import _lib
    fam = wide
    s0 = fam.s0(130)
    s1 = fam.mutate(s0, 40, 30, 9, seed=50)
    before, _ = fam.relation(s0)
    after, _ = fam.relation(s1)
    want = FC.expected_info(s0, s1, before, after, FC.dirty(before, after))
    got = []
    for reserve in (False, True):
        ix, fol = _staged(gpu_ctx, before, s0.vecs)
        assert ix.capacity == 130
        if reserve:
            ix.reserve(200)
        was = ix.array(_lib.ARR_NBRS)[0].value
        _follow(fol, before, after, s1.vecs[130:], want)
        moved = ix.array(_lib.ARR_NBRS)[0].value != was
        assert moved == (not reserve) and ix.capacity == (200 if reserve else 195)  # (by half: 130 + 65, enough for 170)
        _equals_state(ix, fam, s1, ("capacity", reserve))
        got.append(_bytes_of(ix))
        fol.close()
        ix.close()
    assert got[0] == got[1]


# ---- 8: two applies in a row ----------------------------------------------------------------------------------------------------------
def test_two_applies_through_one_follower(gpu_ctx, wide):
    fam = wide
    s0 = fam.s0(130)
    s1 = fam.mutate(s0, 15, 20, 5, seed=60)
    s2 = fam.mutate(s1, 25, 20, 5, seed=61)
    r0, r1, r2 = (fam.relation(s)[0] for s in (s0, s1, s2))
    ix, fol = _staged(gpu_ctx, r0, s0.vecs)
    q = fam.vecs[130:162] * 1.01
    _check_step(gpu_ctx, ix, fol, fam, s0, s1, r0, r1, q, "first step")
    want = _check_step(gpu_ctx, ix, fol, fam, s1, s2, r1, r2, q, "second step")  # (against the table the first apply advanced)
    assert want["n_before"] == 145 and want["n_blocks_before"] == len(r1) // B
    fol.close()
    ix.close()


# ---- 9: snapshots ---------------------------------------------------------------------------------------------------------------------
def test_a_snapshot_stored_before_hides_the_appended_rows(gpu_ctx, wide):
    import pgvectorscale_amd as P
    fam = wide
    s0 = fam.s0(130)
    s1 = fam.mutate(s0, 40, 30, 0, seed=70)
    before, _ = fam.relation(s0)
    after, _ = fam.relation(s1)
    ix, fol = _staged(gpu_ctx, before, s0.vecs)
    P._lib.check(ix._L.vs_index_snapshot_put(ix.h, 1, np.ones(130, np.uint8).ctypes.data_as(C.c_void_p)))
    ix.set_visibility(np.ones(130, np.uint8))
    _follow(fol, before, after, s1.vecs[130:], FC.expected_info(s0, s1, before, after, FC.dirty(before, after)))
    oidx = fam.oracle(s1)
    q = fam.vecs[130:162] * 1.01  # (the appended rows themselves)
    oidx.set_visibility(np.ones(170, np.uint8))
    gi = LC.check_search_batch(ix, oidx, q, None, "own mask")
    assert ((gi >= 130) & (gi != INV)).any()  # the library's own mask shows the new rows
    prev = C.c_void_p()
    P._lib.check(ix._L.vs_index_snapshot_use(ix.h, 1, C.byref(prev)))
    oidx.set_visibility(np.concatenate([np.ones(130, np.uint8), np.zeros(40, np.uint8)]))
    gi = LC.check_search_batch(ix, oidx, q, None, "snapshot 1")
    assert (gi[gi != INV] < 130).all()  # a snapshot stored before the apply cannot see them
    P._lib.check(ix._L.vs_index_set_visibility_dev(ix.h, prev))
    fol.close()
    ix.close()


# ---- 10: primary to standby with the project's own writer -----------------------------------------------------------------------------
def test_primary_to_standby_with_the_projects_own_writer(gpu_ctx, oracle):
    from pgvectorscale_amd.pages import PagesOut
    rng = np.random.default_rng(80)
    X = rng.standard_normal((400, 64)).astype(np.float32)
    new = rng.standard_normal((100, 64)).astype(np.float32)
    x = LC.fresh_index(gpu_ctx, X, distance=oracle.L2, bits=2, R=24, L=48, tids=LC.make_tids(0, 400))
    out = PagesOut(x)
    a = out.read().tobytes()
    base = out.baseline()
    out.close()
    y, fol = _staged(gpu_ctx, a, X)
    assert _bytes_of(y) == _bytes_of(x)
    x.insert(new, LC.make_tids(400, 100), search_list_size=48)
    out = PagesOut(x)
    blocks, nb_now, new_base = out.delta(base)
    pages = out.read_blocks(blocks)
    out.close()
    info = fol.stage(blocks, pages, nb_now)
    assert info["n_appended"] == 100 and info["rows_relinked"] > 0 and (fol.new_tids() == LC.make_tids(400, 100)).all()
    fol.apply(new)
    assert _bytes_of(y) == _bytes_of(x)
    for h in (base, new_base, fol, y, x):
        h.close()


# ---- 11: refusals ---------------------------------------------------------------------------------------------------------------------
def _refused(ix, code, text, fn):
    import pgvectorscale_amd as P
    held = _bytes_of(ix)
    with pytest.raises(P.VsError) as e:
        fn()
    assert e.value.code == code and text in str(e.value), str(e.value)
    assert _bytes_of(ix) == held, "a refused call wrote"


def test_refusals_leave_the_index_and_the_follower_as_they_were(gpu_ctx, wide):
    import pgvectorscale_amd as P
    from pgvectorscale_amd.pages import PagesFollower
    fam = wide
    s0 = fam.s0(130)
    s1 = fam.mutate(s0, 40, 30, 9, seed=90)
    before, ptrs0 = fam.relation(s0)
    after, ptrs1 = fam.relation(s1)
    blocks = FC.dirty(before, after)
    nb = len(after) // B
    good = FC.gather(after, blocks)
    first_node_blk, last_old_blk = ptrs0[0][0], ptrs0[129][0]
    assert first_node_blk in blocks and first_node_blk < last_old_blk and blocks[-1] == nb - 1 >= len(before) // B
    ix, fol = _staged(gpu_ctx, before, s0.vecs)

    def patched(blk, fn):
        """the list with block blk (added when it is not dirty) changed by fn(page)"""
        bl = sorted(set(blocks) | {blk})
        page = bytearray(after[blk * B:(blk + 1) * B])
        fn(page)
        return bl, b"".join(bytes(page) if b == blk else after[b * B:(b + 1) * B] for b in bl)

    def lower(delta):
        def fn(page):
            page[12:14] = (int.from_bytes(page[12:14], "little") + delta).to_bytes(2, "little")
        return fn

    def neighbor_past_n(page):
        _, at = FC.field_at(page, 1, 16)
        page[at:at + 6] = ptrs1[169][0].to_bytes(4, "little") + (ptrs1[169][1] + 1).to_bytes(2, "little")

    def code_width(page):
        fld, _ = FC.field_at(page, 2, 8)
        page[fld + 4:fld + 8] = (fam.W + 1).to_bytes(4, "little")

    def dead_line_pointer(page):
        lp = int.from_bytes(page[28:32], "little")
        page[28:32] = (lp | (3 << 15)).to_bytes(4, "little")

    swapped = [blocks[1], blocks[0]] + blocks[2:]
    _refused(ix, INVALID, "strictly ascending", lambda: fol.stage(swapped, FC.gather(after, swapped), nb))
    dup = [blocks[0]] + blocks
    _refused(ix, INVALID, "strictly ascending", lambda: fol.stage(dup, FC.gather(after, dup), nb))
    _refused(ix, INVALID, "must be", lambda: fol.stage(blocks[:-1], FC.gather(after, blocks[:-1]), nb))
    _refused(ix, INVALID, "shrank", lambda: fol.stage(blocks, good, len(before) // B - 1))
    _refused(ix, INVALID, "existing nodes would move", lambda: fol.stage(*patched(first_node_blk, lower(-4)), nb))
    _refused(ix, INVALID, "existing nodes would move", lambda: fol.stage(*patched(first_node_blk, lower(+4)), nb))
    _refused(ix, INVALID, "not an SbqNode item", lambda: fol.stage(*patched(first_node_blk, neighbor_past_n), nb))
    _refused(ix, INVALID, "code width", lambda: fol.stage(*patched(last_old_blk, code_width), nb))
    _refused(ix, INVALID, "LP_NORMAL", lambda: fol.stage(*patched(nb - 1, dead_line_pointer), nb))
    _refused(ix, STATE, "no list is staged", lambda: fol.apply(s1.vecs[130:]))  # (every refused stage left none)
    want = FC.expected_info(s0, s1, before, after, blocks)
    assert fol.stage(blocks, good, nb) == want
    _refused(ix, INVALID, "new_vecs is NULL", lambda: fol.apply(None))
    view = ix.view(gpu_ctx)
    _refused(ix, STATE, "view", lambda: fol.apply(s1.vecs[130:]))
    view.close()
    fol.discard()
    _refused(ix, STATE, "no list is staged", lambda: fol.apply(s1.vecs[130:]))
    # open: a block table that does not sum to n; a plain index
    cnt = [FC.node_items(before, b) for b in range(len(before) // B)]
    assert sum(cnt) == 130
    _refused(ix, INVALID, "the index holds 130", lambda: PagesFollower(ix, cnt[:-1]))
    plain = P.DiskAnnIndex._upload_plain(gpu_ctx, nbrs=s0.nbrs, heap_tids=s0.tids, vecs=s0.vecs, num_neighbors=fam.R,
                                         distance_type=fam.distance, default_start=s0.start)
    with pytest.raises(P.VsError) as e:
        PagesFollower(plain, cnt)
    assert e.value.code == INVALID and "plain" in str(e.value)
    plain.close()
    # the follower is as good as new: the step goes through and lands on S1
    _check_step(gpu_ctx, ix, fol, fam, s0, s1, before, after, fam.vecs[120:152] * 1.01, "after the refusals")
    fol.close()
    ix.close()
