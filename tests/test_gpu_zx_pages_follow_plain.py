"""vs_pages_follow_open_plain: a device-resident `plain` storage index brought up to date from the blocks of its relation that
something else changed (k_pages_follow_plain).  Every expectation comes from tests/pages_follow_plain_checks.py — a state S0 and its
successor S1 as flat numpy arrays, both written as relations by the oracle's writer (write_plain_index), the dirty block list by a
bytewise page compare, the info counters counted from the arrays — and is exact: no tolerance anywhere.  After an apply (i) the
downloaded neighbor rows (padding included), tids, vector rows (padding included), full-row divisors and n are S1's, (ii) the index
written back with the plain page writer is the after-relation byte for byte (which holds the slice divisors of the appended rows
too), (iii) a batch of plain scans returns the oracle's rows and f32 distance bits over S1, (iv) the counters are the numpy counts.
Items per page of the shapes used here: dim 10 R 4: 75; dim 67 R 8: 21; dim 768 R 50: 2; dim 1536 and 1930 R 50: 1; 24 of 40
dimensions R 6: 45.  Also runs on the lockstep interpreter (tests/test_emu_pages_follow_plain.py)."""
import numpy as np
import pytest

import pages_follow_plain_checks as FC
from oracle import oracle_py as O
from oracle import pages_py as PG
from pages_follow_plain_checks import B, INV

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

INVALID, STATE = -1, -5

# name -> (family arguments, n0, rows appended, rows relinked, offsets cleared)
SHAPES = {
    "d10": (dict(dim=10, R=4, distance=O.L2, n_max=200, seed=11), 130, 32, 20, 6),                 # > 64 items a page; D = 2 mod 4
    "d67": (dict(dim=67, R=8, distance=O.COSINE, n_max=64, seed=12, zero_row=5), 40, 9, 8, 3),     # cut last piece; divisor applied
    "d768": (dict(dim=768, R=50, distance=O.COSINE, n_max=24, seed=13, zero_row=2), 9, 5, 4, 2),   # K = 2: the last page is half full
    "d768even": (dict(dim=768, R=50, distance=O.COSINE, n_max=24, seed=13, zero_row=2), 8, 5, 4, 2),  # K = 2: starts on a fresh page
    "d1536": (dict(dim=1536, R=50, distance=O.IP, n_max=12, seed=14), 5, 3, 3, 2),                 # K = 1
    "d1930": (dict(dim=1930, R=50, distance=O.L2, n_max=8, seed=15), 3, 2, 2, 1),                  # the largest item a page holds
    "slice": (dict(dim=40, dim_index=24, R=6, distance=O.COSINE, n_max=90, seed=16, zero_row=7), 60, 12, 10, 4),  # vnorm_idx
}
FULL = [k for k, v in SHAPES.items() if v[0].get("dim_index") is None]
COSINE = [k for k, v in SHAPES.items() if v[0]["distance"] == O.COSINE]
_families = {}


@pytest.fixture(scope="module")
def shape(oracle):
    def get(name):
        args, n0, m, k, d = SHAPES[name]
        key = tuple(sorted(args.items()))
        if key not in _families:  # (d768 and d768even share one family; a family and its states are computed once and never changed)
            _families[key] = FC.Family(**args)
        return _families[key], n0, m, k, d
    return get


# ---- staging, following, comparing ----------------------------------------------------------------------------------------------------
def _staged(ctx, fam, s, raw, vecs):
    """Y: the host reader over the relation, upload_plain with the heap's rows (or, vecs None, the node vectors) -> (index, follower)"""
    from pgvectorscale_amd.pages import IndexPages
    rd = IndexPages(plain=True)
    rd.add(raw)
    info = rd.finish()
    assert info.n_nodes == s.n and info.words == fam.dim_index
    ix = rd.upload_plain(ctx, distance_type=fam.distance, default_start=s.start, vecs=vecs)
    fol = rd.follower(ix)
    assert fol.plain
    rd.close()
    return ix, fol


def _arrays_of(ix):
    """what the equality standard names, as the device holds it (rows at their device strides)"""
    from pgvectorscale_amd import _lib
    ix._refresh()
    n, ctx = ix.desc.n, ix.ctx
    out = {"n": n}
    for name, which, dt in (("nbrs", _lib.ARR_NBRS, np.uint32), ("tids", _lib.ARR_TIDS, np.uint64), ("vecs", _lib.ARR_VECS, np.uint32),
                            ("vnorm", _lib.ARR_VNORM, np.float32)):
        ptr, stride = ix.array(which)
        out[name] = ctx.download(ptr, np.empty((n, stride), dt)) if ptr.value and n else np.zeros((0, 1), dt)
    return out


def _bytes_of(ix):
    return {k: v if k == "n" else v.tobytes() for k, v in _arrays_of(ix).items()}


def _equals_state(ix, fam, s, rows, where=""):
    """(i): the arrays on the device are s's; rows = what the vector column must hold"""
    got = _arrays_of(ix)
    assert got["n"] == s.n == ix.desc.n, where
    want = np.full(got["nbrs"].shape, INV, np.uint32)
    want[:, :fam.R] = s.nbrs
    assert (got["nbrs"] == want).all(), (where, "neighbor rows, padding included", np.flatnonzero((got["nbrs"] != want).any(1))[:4])
    assert (got["tids"][:, 0] == s.tids).all(), (where, "tids")
    v = got["vecs"]
    assert v[:, :fam.dim].tobytes() == np.ascontiguousarray(rows, np.float32).view(np.uint32).tobytes(), (where, "vector rows")
    assert (v[:, fam.dim:] == 0).all(), (where, "vector row padding")
    if got["vnorm"].size:
        assert got["vnorm"][:, 0].tobytes() == FC.slice_divisors(rows, fam.dim).tobytes(), (where, "vnorm")


def _check_scans(ix, fam, s, where=""):
    """(iii), the way tests/test_gpu_zy_plain.py compares"""
    q = np.ascontiguousarray(fam.vecs[:16] * np.float32(1.01))
    gi, gt, gd, gst = ix.search_batch(q, search_list_size=20, rescore=10, k=8)
    oi, od, ost = fam.oracle(s).search_batch(q, L=20, rescore=10, k=8)
    assert (gi == oi).all(), (where, np.flatnonzero((gi != oi).any(1))[:4])
    assert (gd.view(np.uint32) == od.view(np.uint32)).all(), where
    live = gi != INV
    assert live.any() and (gt[live] == s.tids[gi[live]]).all(), where
    for key in ("visited_nodes", "candidate_nodes", "full_distance_comparisons", "node_reads"):
        assert gst[key] == ost[key], (where, key)


def _check_step(ix, fol, fam, s0, s1, before, after, where=""):
    """one followed step held to (i) .. (iv); the appended rows come from the caller (the heap's rows)"""
    from pgvectorscale_amd.pages import dirty_blocks
    _, ptrs0 = fam.relation(s0)
    _, ptrs1 = fam.relation(s1)
    assert ptrs1[:s0.n] == ptrs0, (where, "the plain Tape moved an existing node")
    blocks = FC.dirty(before, after)
    want = FC.expected_info(fam, s0, s1, before, after, blocks, ptrs1)
    assert want["codes_changed"] == 0
    listed = dirty_blocks(before, after)
    assert listed.tolist() == blocks
    info = fol.stage(listed, FC.gather(after, blocks), len(after) // B)
    assert info == want, (where, info, want)                                                         # (iv)
    assert (fol.new_tids() == s1.tids[s0.n:]).all(), where
    assert _arrays_of(ix)["n"] == s0.n, (where, "the check pass wrote")
    assert fol.apply(s1.vecs[s0.n:] if s1.n > s0.n else None) == want, where
    _equals_state(ix, fam, s1, s1.vecs, where)                                                       # (i)
    got = ix.write_pages(plain=True)
    assert got == after, (where, "written back", [b for b in range(len(after) // B) if got[b * B:(b + 1) * B] != after[b * B:(b + 1) * B]][:4])  # (ii)
    _check_scans(ix, fam, s1, where)                                                                 # (iii)
    return want


# ---- 1: the steps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", ["append", "relink", "clear", "all", "empty", "twice"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_steps(gpu_ctx, shape, name, step):
    fam, n0, m, k, d = shape(name)
    s0 = fam.s0(n0)
    before, ptrs0 = fam.relation(s0)
    K = max(o for _, o in ptrs0)
    assert K == {"d10": 75, "d67": 21, "d768": 2, "d768even": 2, "d1536": 1, "d1930": 1, "slice": 45}[name]
    if name == "d768":
        assert ptrs0[-1][1] == 1  # (the last page is half full: the append fills it first)
    if name == "d768even":
        assert ptrs0[-1][1] == 2  # (the last page is full: the append starts on a fresh one)
    ix, fol = _staged(gpu_ctx, fam, s0, before, s0.vecs)
    where = (name, step)
    if step == "empty":
        held = _bytes_of(ix)
        info = fol.stage([], b"", len(before) // B)
        nb = len(before) // B
        assert info == dict(n_blocks_before=nb, n_blocks_now=nb, pages_listed=0, node_pages_listed=0, n_before=n0, n_appended=0, rows_relinked=0,
                            tids_cleared=0, tids_changed=0, codes_changed=0, label_vals_appended=0)
        assert fol.new_tids().size == 0 and fol.apply(None) == info and _bytes_of(ix) == held
        _check_scans(ix, fam, s0, where)
    elif step == "twice":
        s1 = fam.mutate(s0, m, k, d, seed=21)
        s2 = fam.mutate(s1, m, k, d, seed=22)
        r1, r2 = fam.relation(s1)[0], fam.relation(s2)[0]
        _check_step(ix, fol, fam, s0, s1, before, r1, where + (1,))
        want = _check_step(ix, fol, fam, s1, s2, r1, r2, where + (2,))  # (against the table the first apply advanced)
        assert want["n_before"] == n0 + m and want["n_blocks_before"] == len(r1) // B
    else:
        mm, kk, dd = {"append": (m, 0, 0), "relink": (0, k, 0), "clear": (0, 0, d), "all": (m, k, d)}[step]
        s1 = fam.mutate(s0, mm, kk, dd, seed=20)
        after = fam.relation(s1)[0]
        if step in ("relink", "clear"):
            assert len(after) == len(before)  # (no new block)
        want = _check_step(ix, fol, fam, s0, s1, before, after, where)
        assert want["n_appended"] == mm and want["tids_cleared"] == dd and (want["rows_relinked"] > 0) == (kk > 0)
        if step == "append" and name == "d768":
            assert want["node_pages_listed"] == 3 and FC.dirty(before, after)[0] == ptrs0[-1][0]  # the half-full page, then two fresh ones
        if step == "append" and name == "d768even":
            assert want["node_pages_listed"] == 3 and FC.dirty(before, after)[0] == len(before) // B
    fol.close()
    ix.close()


# ---- 2: the appended rows' vectors from the pages ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FULL)
def test_vectors_from_the_pages(gpu_ctx, shape, name):
    """apply(None) with every dimension indexed: rows [n0, n1) of the vector column are the pages' node vectors bit for bit (the raw
    rows under L2 / inner product, the normalised ones under cosine), rows [0, n0) are untouched, the divisors are those of the rows"""
    fam, n0, m, k, d = shape(name)
    s0 = fam.s0(n0)
    s1 = fam.mutate(s0, m, k, d, seed=30)
    before, after = fam.relation(s0)[0], fam.relation(s1)[0]
    ix, fol = _staged(gpu_ctx, fam, s0, before, s0.vecs)
    was = _arrays_of(ix)
    blocks = FC.dirty(before, after)
    info = fol.stage(blocks, FC.gather(after, blocks), len(after) // B)
    assert info["n_appended"] == m
    assert fol.apply(None) == info
    rows = np.concatenate([s0.vecs, s1.nodevecs[n0:]])
    if fam.distance != O.COSINE:
        assert rows.tobytes() == s1.vecs.tobytes()
    else:
        assert (s1.nodevecs[n0:] != s1.vecs[n0:]).any()
    _equals_state(ix, fam, s1, rows, name)
    now = _arrays_of(ix)
    assert now["vecs"][:n0].tobytes() == was["vecs"].tobytes() and now["vnorm"][:n0].tobytes() == was["vnorm"].tobytes()
    fol.close()
    ix.close()


def test_an_index_uploaded_from_its_pages_alone_follows_them(gpu_ctx, shape):
    """a standby without the heap: Y's vector column is the node vectors (upload_plain(vecs=None)) and the appended rows come from
    the pages too; under the inner product the node vectors are the heap's rows, so the followed index is S1 in every byte"""
    fam, n0, m, k, d = shape("d1536")
    s0 = fam.s0(n0)
    s1 = fam.mutate(s0, m, k, d, seed=31)
    before, after = fam.relation(s0)[0], fam.relation(s1)[0]
    assert s1.nodevecs.tobytes() == s1.vecs.tobytes()
    ix, fol = _staged(gpu_ctx, fam, s0, before, None)
    _equals_state(ix, fam, s0, s0.nodevecs, "uploaded from the pages")
    blocks = FC.dirty(before, after)
    want = FC.expected_info(fam, s0, s1, before, after, blocks, fam.relation(s1)[1])
    assert fol.stage(blocks, FC.gather(after, blocks), len(after) // B) == want and want["codes_changed"] == 0
    assert fol.apply(None) == want
    _equals_state(ix, fam, s1, s1.nodevecs, "followed from the pages")
    assert ix.write_pages(plain=True) == after
    _check_scans(ix, fam, s1, "followed from the pages")
    fol.close()
    ix.close()


def test_vectors_cannot_come_from_the_pages_of_a_truncated_index(gpu_ctx, shape):
    import pgvectorscale_amd as P
    fam, n0, m, k, d = shape("slice")
    s0 = fam.s0(n0)
    s1 = fam.mutate(s0, m, k, d, seed=30)
    before, after = fam.relation(s0)[0], fam.relation(s1)[0]
    ix, fol = _staged(gpu_ctx, fam, s0, before, s0.vecs)
    blocks = FC.dirty(before, after)
    info = fol.stage(blocks, FC.gather(after, blocks), len(after) // B)
    held = _bytes_of(ix)
    with pytest.raises(P.VsError) as e:
        fol.apply(None)
    assert e.value.code == INVALID and "the pages hold only the index slice" in str(e.value)
    assert _bytes_of(ix) == held
    assert fol.apply(s1.vecs[n0:]) == info  # (the staged list is still there)
    _equals_state(ix, fam, s1, s1.vecs, "slice")
    assert ix.write_pages(plain=True) == after
    fol.close()
    ix.close()


# ---- 3: codes_changed -----------------------------------------------------------------------------------------------------------------------
def _flip(raw, ptr, j):
    """the relation with the lowest mantissa bit of float j of the node at ptr flipped"""
    blk, off = ptr
    page = bytearray(raw[blk * B:(blk + 1) * B])
    _, at = FC.field_at(page, off, 0)
    page[at + 4 * j] ^= 1
    return raw[:blk * B] + bytes(page) + raw[(blk + 1) * B:]


@pytest.mark.parametrize("name,mid", [("d67", 65), ("d768", 300)])
def test_a_changed_vector_is_reported_and_not_applied(gpu_ctx, shape, name, mid):
    """three existing nodes with one float changed in the after-relation: the first float of one, the last float of another (the cut
    piece of dim 67), one further in (dim 67: float 65; dim 768: float 300, in the piece loop's second trip)"""
    fam, n0, m, k, d = shape(name)
    s0 = fam.s0(n0)
    s1 = fam.mutate(s0, m, k, d, seed=40)
    before, ptrs0 = fam.relation(s0)
    after, ptrs1 = fam.relation(s1)
    a, b, c = (1, 4, n0 - 1) if n0 < 20 else (1, 23, n0 - 1)
    assert SHAPES[name][0]["zero_row"] not in (a, b, c)
    for node, j in ((a, 0), (b, fam.dim - 1), (c, mid)):
        after = _flip(after, ptrs1[node], j)
    blocks = FC.dirty(before, after)
    want = FC.expected_info(fam, s0, s1, before, after, blocks, ptrs1)
    assert want["codes_changed"] == 3  # (the numpy restatement of the writer's rule, before the device is asked)
    ix, fol = _staged(gpu_ctx, fam, s0, before, s0.vecs)
    was = _arrays_of(ix)
    info = fol.stage(blocks, FC.gather(after, blocks), len(after) // B)
    assert info == want, (info, want)
    assert fol.apply(s1.vecs[n0:]) == want
    _equals_state(ix, fam, s1, s1.vecs, name)  # (the resident rows, not the pages' changed floats)
    now = _arrays_of(ix)
    assert now["vecs"][:n0].tobytes() == was["vecs"].tobytes() and now["vnorm"][:n0].tobytes() == was["vnorm"].tobytes()
    assert ix.write_pages(plain=True) == fam.relation(s1)[0]  # (which covers vnorm_idx too: the writer divides by it)
    fol.close()
    ix.close()


@pytest.mark.parametrize("name", COSINE)
def test_every_row_the_oracle_normalised_is_what_the_device_composes(gpu_ctx, shape, name):
    """every block of an unchanged relation listed: codes_changed == 0 holds the device's division to the oracle's preprocess_cosine
    on every row, the all-zero one (divisor 0, slice left alone) included"""
    fam, n0, m, k, d = shape(name)
    s0 = fam.s0(n0)
    raw, ptrs = fam.relation(s0)
    zero = SHAPES[name][0]["zero_row"]
    assert zero < n0 and not s0.vecs[zero].any() and FC.slice_divisors(s0.vecs, fam.dim_index)[zero] == 0
    assert (FC.slice_divisors(s0.vecs, fam.dim_index) != 0).sum() == n0 - 1
    nb = len(raw) // B
    assert FC.vectors_differing(s0.vecs, fam.dim_index, fam.distance, FC.page_vectors(raw, ptrs, fam.dim_index)) == 0
    ix, fol = _staged(gpu_ctx, fam, s0, raw, s0.vecs)
    info = fol.stage(list(range(nb)), raw, nb)
    assert info["codes_changed"] == 0 and info["node_pages_listed"] == nb - 1 and info["rows_relinked"] == 0 and info["n_appended"] == 0
    fol.discard()
    fol.close()
    ix.close()


# ---- 4: refusals ----------------------------------------------------------------------------------------------------------------------------
def _refused(ix, code, text, fn):
    import pgvectorscale_amd as P
    held = _bytes_of(ix)
    with pytest.raises(P.VsError) as e:
        fn()
    assert e.value.code == code and text in str(e.value), str(e.value)
    assert _bytes_of(ix) == held, "a refused call wrote"


def test_refusals_leave_the_index_and_the_follower_as_they_were(gpu_ctx, oracle, shape):
    import pgvectorscale_amd as P
    from helpers import TestIndex
    from pgvectorscale_amd.pages import PagesFollower
    fam, n0, m, k, d = shape("d67")
    s0 = fam.s0(n0)
    s1 = fam.mutate(s0, m, 14, d, seed=90)
    before, ptrs0 = fam.relation(s0)
    after, ptrs1 = fam.relation(s1)
    blocks = FC.dirty(before, after)
    nb = len(after) // B
    good = FC.gather(after, blocks)
    first_node_blk, last_old_blk = ptrs0[0][0], ptrs0[n0 - 1][0]
    assert first_node_blk in blocks and first_node_blk < last_old_blk and blocks[-1] == nb - 1 >= len(before) // B and len(blocks) >= 3
    ix, fol = _staged(gpu_ctx, fam, s0, before, s0.vecs)

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
        page[at:at + 6] = ptrs1[s1.n - 1][0].to_bytes(4, "little") + (ptrs1[s1.n - 1][1] + 1).to_bytes(2, "little")

    def vector_length(page):
        fld, _ = FC.field_at(page, 2, 0)
        page[fld + 4:fld + 8] = (fam.dim_index + 1).to_bytes(4, "little")

    def neighbor_slots(page):
        fld, _ = FC.field_at(page, 2, 16)
        page[fld + 4:fld + 8] = (fam.R - 1).to_bytes(4, "little")

    def dead_line_pointer(page):
        lp = int.from_bytes(page[28:32], "little")
        page[28:32] = (lp | (3 << 15)).to_bytes(4, "little")

    def sbq_typed(page):
        assert page[B - 8] == PG.PT_NODE
        page[B - 8] = PG.PT_SBQ_NODE

    swapped = [blocks[1], blocks[0]] + blocks[2:]
    _refused(ix, INVALID, "strictly ascending", lambda: fol.stage(swapped, FC.gather(after, swapped), nb))
    dup = [blocks[0]] + blocks
    _refused(ix, INVALID, "strictly ascending", lambda: fol.stage(dup, FC.gather(after, dup), nb))
    past = blocks + [nb]
    _refused(ix, INVALID, f"of a relation of {nb} blocks", lambda: fol.stage(past, good + bytes(B), nb))
    _refused(ix, INVALID, "must be", lambda: fol.stage(blocks[:-1], FC.gather(after, blocks[:-1]), nb))
    _refused(ix, INVALID, "shrank", lambda: fol.stage(blocks, good, len(before) // B - 1))
    _refused(ix, INVALID, "existing nodes would move", lambda: fol.stage(*patched(first_node_blk, lower(-4)), nb))
    _refused(ix, INVALID, "existing nodes would move", lambda: fol.stage(*patched(first_node_blk, lower(+4)), nb))
    _refused(ix, INVALID, "existing nodes would move", lambda: fol.stage(*patched(first_node_blk, sbq_typed), nb))
    _refused(ix, INVALID, "vector length differs from the index's dimensions", lambda: fol.stage(*patched(last_old_blk, vector_length), nb))
    _refused(ix, INVALID, "neighbor slot count differs", lambda: fol.stage(*patched(last_old_blk, neighbor_slots), nb))
    _refused(ix, INVALID, "not a PlainNode item of this relation", lambda: fol.stage(*patched(first_node_blk, neighbor_past_n), nb))
    _refused(ix, INVALID, "LP_NORMAL", lambda: fol.stage(*patched(nb - 1, dead_line_pointer), nb))
    _refused(ix, STATE, "no list is staged", lambda: fol.apply(s1.vecs[n0:]))  # (every refused stage left none)
    want = FC.expected_info(fam, s0, s1, before, after, blocks, ptrs1)
    assert fol.stage(blocks, good, nb) == want
    view = ix.view(gpu_ctx)
    _refused(ix, STATE, "view", lambda: fol.apply(s1.vecs[n0:]))
    view.close()
    fol.discard()
    _refused(ix, STATE, "no list is staged", lambda: fol.apply(s1.vecs[n0:]))
    # open: a block table that does not sum to n; the other storage type on either call
    cnt = FC.block_counts(before)
    assert sum(cnt) == n0
    _refused(ix, INVALID, f"the index holds {n0}", lambda: PagesFollower(ix, cnt[:-1], plain=True))
    _refused(ix, INVALID, "vs_pages_follow_open_plain", lambda: PagesFollower(ix, cnt))
    with pytest.raises(P.VsError) as e:
        PagesFollower(ix, cnt)
    assert "plain" in str(e.value) and "vs_pages_follow_open: " in str(e.value)
    sbq = TestIndex(n=200, dim_full=32, bits=2, R=8, distance=oracle.L2, seed=9, kind="gauss", L_build=20).upload(gpu_ctx)
    with pytest.raises(P.VsError) as e:
        PagesFollower(sbq, [0, 200], plain=True)
    assert e.value.code == INVALID and "followed with vs_pages_follow_open" in str(e.value) and "vs_pages_follow_open_plain:" in str(e.value)
    sbq.close()
    # the follower is as good as new: the step goes through and lands on S1
    _check_step(ix, fol, fam, s0, s1, before, after, "after the refusals")
    fol.close()
    ix.close()


# ---- 5: the library's own pair -------------------------------------------------------------------------------------------------------------
def test_the_librarys_own_writer_and_follower(gpu_ctx):
    import pgvectorscale_amd as P
    from helpers import make_vectors
    from pgvectorscale_amd.pages import IndexPages, PagesOut
    n, dim, R = 200, 67, 16
    X = make_vectors(n + 32, dim, 81, "gauss") * np.float32(1.7)
    tids = (np.arange(1, n + 33, dtype=np.uint64) << np.uint64(16)) | np.uint64(1)
    x = P.DiskAnnIndex.alloc(gpu_ctx, n=n, dim_full=dim, num_neighbors=R, distance_type=P.VS_COSINE, storage_type=P._lib.VS_STORAGE_PLAIN)
    vp, stride = x.array(P._lib.ARR_VECS)
    rows = np.zeros((n, stride), np.float32)
    rows[:, :dim] = X[:n]
    gpu_ctx.upload(vp, rows)
    gpu_ctx.upload(x.array(P._lib.ARR_TIDS)[0], tids[:n])
    x.refresh_norms()
    x.build_graph(search_list_size=32, max_alpha=1.2)
    out = PagesOut(x, plain=True)
    a = out.read().tobytes()
    base = out.baseline()
    out.close()
    rd = IndexPages(plain=True)
    rd.add(a)
    rd.finish()
    _, d, _ = rd.meta()
    y = rd.upload_plain(gpu_ctx, distance_type=P.VS_COSINE, default_start=int(d.default_start), vecs=X[:n])
    fol = rd.follower(y)
    rd.close()
    assert _bytes_of(y) == _bytes_of(x)
    st = x.insert(X[n:], tids[n:], search_list_size=32, max_alpha=1.2)
    assert st["inserted"] == 32
    assert x.bulk_delete(tids[[5, 60, 61, 150, 199]])["tuples_removed"] == 5
    out = PagesOut(x, plain=True)
    blocks, nb_now, new_base = out.delta(base)
    pages = out.read_blocks(blocks)
    now = out.read().tobytes()
    out.close()
    info = fol.stage(blocks, pages, nb_now)
    assert info["n_appended"] == 32 and info["rows_relinked"] > 0 and info["tids_cleared"] == 5 and info["codes_changed"] == 0
    assert (fol.new_tids() == tids[n:]).all()
    fol.apply(X[n:])
    assert _bytes_of(y) == _bytes_of(x)  # neighbor rows, tids, vector rows and the divisors (dim_index = dim_full: there is no vnorm_idx)
    assert y.write_pages(plain=True) == now
    for h in (base, new_base, fol, y, x):
        h.close()
