"""vs_index_bulk_delete: ambulkdelete by heap TID (bulk_delete_for_storage, AM/vacuum.rs:80-136) — one kernel over the TID column,
a binary search in the sorted dead set, the three counters of IndexBulkDeleteResult.  The reference is numpy, here: np.isin on the
TID column among the nodes whose offset is not 0; the column afterwards is what vs_index_mark_deleted leaves on a second upload."""
import numpy as np
import pytest

from helpers import TestIndex

pytestmark = pytest.mark.gpu

OFF = np.uint64(0xFFFF)


@pytest.fixture(scope="module")
def ti(oracle):
    return TestIndex(n=1400, dim_full=96, dim_index=64, bits=2, R=24, distance=oracle.L2, seed=18, kind="gauss", deleted_frac=0.1, L_build=50)


def _dead_set(ti, size, seed):
    """`size` TIDs, unsorted: live nodes' TIDs, TIDs in the blocks of nodes that are deleted already, TIDs no node has, and
    duplicates of all three"""
    rng = np.random.default_rng(seed)
    if size == 0:
        return np.zeros(0, np.uint64)
    live = np.flatnonzero((ti.tids & OFF) != 0)
    gone = np.flatnonzero((ti.tids & OFF) == 0)
    if size == 1:
        return ti.tids[live[[len(live) // 2]]].copy()
    n_hit = min(size // 2, 400)
    n_gone = min(size // 10, len(gone))
    hits = ti.tids[rng.choice(live, n_hit, replace=False)]
    in_gone_blocks = ti.tids[rng.choice(gone, n_gone, replace=False)] | np.uint64(1)  # (block of a deleted node, offset 1: matches nobody)
    dups = rng.choice(np.concatenate([hits, in_gone_blocks]), size // 8)
    n_absent = size - n_hit - n_gone - len(dups)
    absent = ((rng.integers(10 ** 6, 10 ** 9, n_absent).astype(np.uint64)) << np.uint64(16)) | rng.integers(1, 200, n_absent).astype(np.uint64)
    dead = np.concatenate([hits, in_gone_blocks, dups, absent])
    assert dead.size == size
    rng.shuffle(dead)
    assert (np.diff(dead.astype(np.int64)) < 0).any() and len(np.unique(dead)) < size
    return dead


def _reference(tids, dead):
    live = (tids & OFF) != 0
    hit = live & np.isin(tids, dead)
    after = tids.copy()
    after[hit] &= ~OFF
    return dict(tuples_removed=int(hit.sum()), num_index_tuples=int((live & ~hit).sum()), already_deleted=int((~live).sum())), after, hit


@pytest.mark.parametrize("size", [0, 1, 257, 5000])
def test_counters_and_column_match_numpy_and_mark_deleted(gpu_ctx, ti, size):
    dead = _dead_set(ti, size, seed=size + 3)
    want, after, hit = _reference(ti.tids, dead)
    assert want["tuples_removed"] == (0 if size == 0 else 1 if size == 1 else min(size // 2, 400))
    assert want["already_deleted"] > 50
    if size == 5000:  # larger than the index, mostly TIDs no node has
        assert size > ti.n and np.isin(dead, ti.tids).sum() < size // 4
    ix = ti.upload(gpu_ctx)
    got = ix.bulk_delete(dead)
    assert got == want
    col = ix.download(codes=False, nbrs=False)["heap_tids"]
    assert (col == after).all()
    twin = ti.upload(gpu_ctx)
    twin.mark_deleted(np.flatnonzero(hit).astype(np.uint32))
    assert (twin.download(codes=False, nbrs=False)["heap_tids"] == col).all()
    twin.close()
    # the same call again removes nothing: what it removed the first time is deleted already now
    again = ix.bulk_delete(dead)
    assert again == dict(tuples_removed=0, num_index_tuples=want["num_index_tuples"],
                         already_deleted=want["already_deleted"] + want["tuples_removed"])
    assert (ix.download(codes=False, nbrs=False)["heap_tids"] == after).all()
    ix.close()


def test_an_offset_0_entry_is_refused_and_nothing_changes(gpu_ctx, ti):
    import pgvectorscale_amd as P
    dead = _dead_set(ti, 257, seed=9)
    dead[100] &= ~OFF
    ix = ti.upload(gpu_ctx)
    with pytest.raises(P.VsError) as e:
        ix.bulk_delete(dead)
    assert e.value.code == -1 and "offset 0" in str(e.value)
    assert (ix.download(codes=False, nbrs=False)["heap_tids"] == ti.tids).all()
    ix.close()


def test_search_afterwards_returns_the_oracles_rows(gpu_ctx, ti):
    dead = _dead_set(ti, 257, seed=11)
    want, after, hit = _reference(ti.tids, dead)
    ix = ti.upload(gpu_ctx)
    assert ix.bulk_delete(dead) == want
    oracle_ix = type(ti.oracle)(codes=ti.codes, nbrs=ti.nbrs, heap_tids=after, vecs=ti.vecs, mean=ti.mean, m2=ti.m2, count=ti.count,
                                bits=ti.bits, dim_index=ti.dim_index, num_neighbors=ti.R, distance_type=ti.distance, default_start=ti.start)
    q = ti.queries(32, seed=12, kind="gauss")
    gi, gt, gd, gst = ix.search_batch(q, search_list_size=40, rescore=20, k=10)
    oi, od, ost = oracle_ix.search_batch(q, L=40, rescore=20, k=10)
    bi, _, _ = ti.oracle.search_batch(q, L=40, rescore=20, k=10)
    assert (gi == oi).all() and (gd.view(np.uint32) == od.view(np.uint32)).all() and gst["visited_nodes"] == ost["visited_nodes"]
    assert not hit[gi[gi != 0xFFFFFFFF]].any() and (bi != oi).any()  # (the removed rows were among the answers before)
    ix.close()


def test_device_form_on_a_sorted_unique_array(gpu_ctx, ti):
    dead = _dead_set(ti, 5000, seed=13)
    want, after, _ = _reference(ti.tids, dead)
    su = np.unique(dead)
    d = gpu_ctx.alloc(su.nbytes)
    gpu_ctx.upload(d, su)
    ix = ti.upload(gpu_ctx)
    assert ix.bulk_delete_dev(d, su.size) == want
    assert (ix.download(codes=False, nbrs=False)["heap_tids"] == after).all()
    gpu_ctx.free(d)
    ix.close()


def test_plain_storage_index(gpu_ctx, ti):
    import pgvectorscale_amd as P
    plain = P.DiskAnnIndex.upload(gpu_ctx, codes=None, nbrs=ti.nbrs, heap_tids=ti.tids, vecs=ti.vecs, mean=None, m2=None, count=0, bits=1,
                                  dim_index=ti.dim_full, num_neighbors=ti.R, distance_type=ti.distance, default_start=ti.start,
                                  storage_type=P._lib.VS_STORAGE_PLAIN)
    dead = _dead_set(ti, 257, seed=14)
    want, after, _ = _reference(ti.tids, dead)
    assert plain.bulk_delete(dead) == want
    assert (plain.download(codes=False, nbrs=False)["heap_tids"] == after).all()
    plain.close()
