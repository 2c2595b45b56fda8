#!/usr/bin/env python3
"""Scans of different snapshots in one launch: what the visibility base and its overlays cost, next to the only way the same scans
could run before — one legacy mask per snapshot, one full vs_index_snapshot_eval each, one launch per mask — in one process on one box.

  1. --rows fixed-width tuples are fabricated as scripts/bench_heap_vis.py fabricates them (held to oracle/heap_py.py byte for byte
     at 1 000 rows), with a header mix whose class is known by construction: 94 % visible to all (90 % hinted committed, 4 %
     committed by pg_xact), 2 % invisible to all (deleted by an old committed transaction), 4 % "depends" (2 % inserted by xid 1200,
     2 % deleted by xid 1500: both at or after the horizon 1000, both committed in pg_xact, so a snapshot sees the row or not by
     whether the xid is in its xip);
  2. an SBQ index of --rows nodes over generated vectors (--dim), built on the device, whose tid column names those tuples in heap
     order and again in shuffled order;
  3. vs_index_vis_base_eval over every node; a refresh for 1 % of the heap blocks; vs_index_vis_slot_eval at the resulting r: HIP-event
     time of the rule's kernel (vs_profile_*) and the whole call's host time, warm, median of --reps; classes, r and one materialized
     mask per kind of snapshot are compared with the construction at the timed size;
  4. --scans scans at rescore > 0 dealt over --slots slots in ONE launch (vs_search_batch_dev_vis + finish): host time and the search
     kernel's HIP-event time;
  5. the same scans the old way: 15 legacy masks, one full vs_index_snapshot_eval each, then 15 launches of --scans / 15 scans under
     vs_index_snapshot_use.  (15 is all an index keeps; --slots snapshots would need several such rounds.)

No ratio is fixed in advance; both sides are measured in this one session.

    python scripts/bench_vis_overlay.py --out profiles/r21/vis_overlay_4m.txt
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_heap_vis as BH  # noqa: E402

XMIN_COMMITTED, XMAX_COMMITTED, XMAX_INVALID = BH.XMIN_COMMITTED, BH.XMAX_COMMITTED, BH.XMAX_INVALID
HORIZON = 1000
XACT = BH.XACT  # pg_xact window [800, 2200): everything committed
INS, DEL = 1200, 1500  # the two transactions "since the horizon"
KINDS = 100  # row i is of kind i % 100: 0-89 hinted committed, 90-93 committed by pg_xact, 94-95 deleted long ago, 96-97 inserted by INS, 98-99 deleted by DEL


def headers(n):
    k = np.arange(n) % KINDS
    xmin = np.where((k == 96) | (k == 97), INS, 900 + (np.arange(n) % 97)).astype("<u4")
    xmax = np.where((k == 94) | (k == 95), 950, np.where(k >= 98, DEL, 0)).astype("<u4")
    m = np.full(n, XMIN_COMMITTED | XMAX_INVALID, np.uint32)
    m[(k >= 90) & (k <= 93)] = XMAX_INVALID
    m[(k == 94) | (k == 95)] = XMIN_COMMITTED | XMAX_COMMITTED
    m[(k == 96) | (k == 97)] = XMAX_INVALID
    m[k >= 98] = XMIN_COMMITTED
    return xmin, xmax, m.astype("<u2"), (k < 94).astype(np.uint8)


def classes(n):
    k = np.arange(n) % KINDS
    return np.where(k < 94, 1, np.where(k < 96, 0, 2)).astype(np.uint8)


def snapshot(j):
    """snapshot j of the family: which of INS / DEL it still sees running"""
    xip = [x for b, x in ((1, INS), (2, DEL)) if j & b]
    return dict(xmin=HORIZON + (j % 7), xmax=2000 + j, xip=xip, curcid=1)


def mask_of(n, j):
    k = np.arange(n) % KINDS
    m = (k < 94).astype(np.uint8)
    m[(k == 96) | (k == 97)] = 0 if j & 1 else 1  # the inserter is in xip: not yet visible
    m[k >= 98] = 1 if j & 2 else 0                # the deleter is in xip: still visible
    return m


def read_mask(ix, ctx, sid, n):
    from pgvectorscale_amd import _lib
    prev, mine = C.c_void_p(), C.c_void_p()
    _lib.check(ix._L.vs_index_snapshot_use(ix.h, sid, C.byref(prev)))
    _lib.check(ix._L.vs_index_snapshot_use(ix.h, 0, C.byref(mine)))
    _lib.check(ix._L.vs_index_set_visibility_dev(ix.h, prev))
    return ctx.download(mine, np.empty(n, np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scans", type=int, default=8192)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--L", type=int, default=40)
    ap.add_argument("--rescore", type=int, default=20)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--build-L", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pgvectorscale_amd as P
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.datagen import DatagenParams, fill_device
    from pgvectorscale_amd.pages import HeapResident
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    med = lambda v: float(np.median(v))  # noqa: E731
    n, nq, ns = a.rows, a.scans, a.slots
    ctx = P.Context(0)
    say(f"bench_vis_overlay on {ctx.device_name()}: rows {n}, dim {a.dim}, scans {nq} over {ns} slots, L {a.L} rescore {a.rescore} k {a.k}, reps {a.reps}")
    BH.check_fabricator(headers=headers)  # the fabricator of bench_heap_vis.py with this file's header mix
    say("fabricator: byte-identical to oracle/heap_py.py at 1000 rows")
    pages, tids, _ = BH.fabricate(n, headers)
    cls = classes(n)
    say(f"fork: {n} tuples, {pages.nbytes / 1e6:.1f} MB in {pages.shape[0]} pages; by construction class 0 / 1 / 2 = "
        f"{int((cls == 0).sum())} / {int((cls == 1).sum())} / {int((cls == 2).sum())}")
    heap = HeapResident(ctx, pages.shape[0])
    heap.put(pages.reshape(-1))
    out = {"rows": n, "scans": nq, "slots": ns}

    # ---- the index: generated vectors, SBQ codes and a graph built on the device
    t0 = time.perf_counter()
    ix = P.DiskAnnIndex.alloc(ctx, n=n, dim_full=a.dim, num_neighbors=32, distance_type=P.VS_L2)
    gp = DatagenParams(seed=3, dim=a.dim, latent_dim=min(32, a.dim))
    vecs_ptr, _ = ix.array(_lib.ARR_VECS)
    fill_device(ctx, gp, 0, n, vecs_ptr)
    ix.refresh_norms()
    ix.sbq_train()
    ix.sbq_quantize_corpus()
    ix.build_graph(search_list_size=a.build_L)
    ctx.sync()
    say(f"index: {n} nodes, dim {a.dim}, {ix.desc.bits} bits, R 32, built on the device in {time.perf_counter() - t0:.1f} s")
    d_tids, _ = ix.array(_lib.ARR_TIDS)
    dq = ctx.alloc(nq * a.dim * 4)
    fill_device(ctx, gp, n, nq, dq)  # queries: rows of the same generator past the corpus
    d_ids, d_slots = ctx.alloc(nq * a.k * 4), ctx.alloc(nq * 4)
    slots = (np.arange(nq) % ns + 1).astype(np.uint32)
    ctx.upload(d_slots, slots)
    rng = np.random.default_rng(5)
    perm = rng.permutation(n)
    nb = pages.shape[0]
    changed = np.sort(rng.choice(nb, max(nb // 100, 1), replace=False)).astype(np.uint32)

    def timed(fn, kernel="pages_encode"):
        """-> (median kernel ms, median call ms) over --reps warm calls"""
        fn()
        ctx.profile_enable(True)
        kern, call = [], []
        for _ in range(a.reps):
            ctx.profile_read(reset=True)
            t = time.perf_counter()
            fn()
            ctx.sync()
            call.append(time.perf_counter() - t)
            kern.append(ctx.profile_read(reset=True)[kernel][0])
        ctx.profile_enable(False)
        return med(kern), med(call) * 1e3

    for name, order in (("heap order", None), ("shuffled order", perm)):
        key = "heap_order" if order is None else "shuffled"
        t_ix = tids if order is None else tids[order]
        want_cls = cls if order is None else cls[order]
        ctx.upload(d_tids, t_ix)
        # ---- the base: every node, then a refresh for 1 % of the blocks
        st = ix.vis_base_eval(heap, HORIZON, XACT)
        assert st["n_class"] == [int((want_cls == c).sum()) for c in range(3)] and st["n_undecided"] == 0, st
        _, dep = ix.vis_base_info()
        assert (dep == np.flatnonzero(want_cls == 2)).all(), "the depends list differs from the construction"
        r = len(dep)
        k_full, c_full = timed(lambda: ix.vis_base_eval(heap, HORIZON, XACT))
        k_ref, c_ref = timed(lambda: ix.vis_base_eval(heap, HORIZON, XACT, changed_blocks=changed))
        st = ix.vis_base_eval(heap, HORIZON, XACT, changed_blocks=changed)
        say(f"{name}: vs_index_vis_base_eval, every node: kernel {k_full:.3f} ms, call {c_full:.2f} ms; refresh for {len(changed)} of {nb} blocks "
            f"({st['n_walked']} nodes walked): kernel {k_ref:.3f} ms, call {c_ref:.2f} ms; r = {r} ({100.0 * r / n:.2f} % of the nodes), class shares "
            f"{[round(100.0 * v / n, 2) for v in st['n_class']]} %")
        # ---- one overlay, checked for every kind of snapshot; then all of them
        for j in range(4):
            ix.vis_slot_eval(heap, 1, snapshot(j), XACT, cap=0)
            ix.vis_materialize(1, 1)
            want = mask_of(n, j)
            assert (read_mask(ix, ctx, 1, n) == (want if order is None else want[order])).all(), f"materialized mask of snapshot {j}"
        k_slot, c_slot = timed(lambda: ix.vis_slot_eval(heap, 1, snapshot(3), XACT, cap=0))
        t = time.perf_counter()
        for s in range(1, ns + 1):
            ix.vis_slot_eval(heap, s, snapshot(s), XACT, cap=0)
        ctx.sync()
        all_slots = (time.perf_counter() - t) * 1e3
        say(f"{name}: vs_index_vis_slot_eval at r = {r}: kernel {k_slot:.3f} ms, call {c_slot:.2f} ms; {ns} overlays: {all_slots:.1f} ms, {ns * max(r, 1)} bytes")

        # ---- the new way: every scan names its slot, one launch
        def new_way():
            ix.search_batch_dev(dq, nq, a.L, a.rescore, a.k, d_ids, d_vis_slots=d_slots)
            return ix.search_batch_dev_finish()
        st_new = new_way()
        got_new = ctx.download(d_ids, np.empty((nq, a.k), np.uint32))
        k_new, c_new = timed(new_way, kernel="search")
        say(f"{name}: {nq} scans over {ns} slots in ONE launch: search kernel {k_new:.3f} ms, call (launch to rows) {c_new:.2f} ms "
            f"= {nq / c_new:.1f} k scans/s; {st_new['node_heap_reads']} heap reads in all")
        # ---- the old way: 15 masks, one full evaluation each, one launch per mask
        nm = 15
        per = nq // nm
        t = time.perf_counter()
        for sid in range(1, nm + 1):
            ix.snapshot_eval(heap, sid, snapshot(sid), XACT, cap=0)
        ctx.sync()
        evals = (time.perf_counter() - t) * 1e3
        k_ev, c_ev = timed(lambda: ix.snapshot_eval(heap, 1, snapshot(1), XACT, cap=0))

        def old_way():
            for sid in range(1, nm + 1):
                _lib.check(ix._L.vs_index_snapshot_use(ix.h, sid, None))
                ix.search_batch_dev(C.c_void_p(dq.value + (sid - 1) * per * a.dim * 4), per, a.L, a.rescore, a.k, d_ids)
                ix.search_batch_dev_finish()
            _lib.check(ix._L.vs_index_snapshot_use(ix.h, 0, None))
        k_old, c_old = timed(old_way, kernel="search")
        # the rows of a scan are the same either way (snapshot s and slot s hold the same snapshot)
        _lib.check(ix._L.vs_index_snapshot_use(ix.h, 1, None))
        ix.search_batch_dev(dq, nq, a.L, a.rescore, a.k, d_ids)
        ix.search_batch_dev_finish()
        _lib.check(ix._L.vs_index_snapshot_use(ix.h, 0, None))
        under_1 = ctx.download(d_ids, np.empty((nq, a.k), np.uint32))
        sel = slots == 1
        assert (under_1[sel] == got_new[sel]).all(), "rows under legacy mask 1 differ from the rows of the scans that named slot 1"
        say(f"{name}: the old way: {nm} x vs_index_snapshot_eval {evals:.1f} ms ({c_ev:.2f} ms a call, kernel {k_ev:.3f} ms), {nm * n} mask bytes; "
            f"{nm} launches of {per} scans: search kernels {k_old:.3f} ms, calls {c_old:.2f} ms = {nm * per / c_old:.1f} k scans/s")
        out[key] = dict(r=r, base_kernel_ms=round(k_full, 4), base_call_ms=round(c_full, 3), refresh_kernel_ms=round(k_ref, 4),
                        refresh_call_ms=round(c_ref, 3), slot_kernel_ms=round(k_slot, 4), slot_call_ms=round(c_slot, 3),
                        all_slots_ms=round(all_slots, 2), one_launch_kernel_ms=round(k_new, 4), one_launch_call_ms=round(c_new, 3),
                        legacy_evals_ms=round(evals, 2), legacy_eval_kernel_ms=round(k_ev, 4), legacy_launches_kernel_ms=round(k_old, 4),
                        legacy_launches_call_ms=round(c_old, 3))
    say(json.dumps(out))
    for p in (dq, d_ids, d_slots):
        ctx.free(p)
    ix.close()
    heap.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
