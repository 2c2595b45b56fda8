#!/usr/bin/env python3
"""Qualified scans (vs_search_batch_dev_qual): what `ORDER BY embedding <=> $1 LIMIT k` under a WHERE clause costs when the predicate
is a qualifier on the device, next to the way to the same rows before — vs_search_batch_dev at k, the rejected rows thrown away on the
host, then ScanPool.fetch rounds of k rows with the filter on the host until every scan has its k rows or has been taken to max_pops.
One process, one box, an SBQ index over generated vectors built on the device.

  new way   one vs_search_batch_dev_qual + finish over --scans scans per qualifier density: wall time (launch to finished outputs) and
            kernel time (HIP events of every kernel of the call), rounds and pops_launched; once with the wave-parallel window
            selection (VS_RERANK_FUSED=1) and once with the serial replay forced (=2)
  old way   --pool-scans of the same scans: one batch at k, then pool rounds; wall time, scaled per scan
  rows of the scans both sides ran are compared (node ids, tids, distance bits) before any time is reported

Medians of --reps warm repetitions with min .. max.  No ratio is fixed in advance.

    python scripts/bench_qual.py --out profiles/r22/qual_4m.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INV = 0xFFFFFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--R", type=int, default=50)
    ap.add_argument("--build-L", type=int, default=64)
    ap.add_argument("--scans", type=int, default=8192)
    ap.add_argument("--pool-scans", type=int, default=1024)
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--rescore", type=int, default=50)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--max-pops", type=int, default=2048)
    ap.add_argument("--densities", default="0.5,0.1,0.02")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pgvectorscale_amd as P
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.datagen import DatagenParams, fill_device
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def spread(v):
        return f"{np.median(v):.2f} ({min(v):.2f} .. {max(v):.2f})"

    n, nq, k, mp = a.rows, a.scans, a.k, a.max_pops
    npool = min(a.pool_scans, nq)
    ctx = P.Context(0)
    say(f"bench_qual on {ctx.device_name()}: rows {n}, dim {a.dim}, R {a.R}, scans {nq} (old way: {npool}), L {a.L} rescore {a.rescore} k {k} "
        f"max_pops {mp}, reps {a.reps}")
    t0 = time.perf_counter()
    ix = P.DiskAnnIndex.alloc(ctx, n=n, dim_full=a.dim, num_neighbors=a.R, distance_type=P.VS_L2)
    gp = DatagenParams(seed=3, dim=a.dim, latent_dim=min(32, a.dim))
    vecs_ptr, _ = ix.array(_lib.ARR_VECS)
    fill_device(ctx, gp, 0, n, vecs_ptr)
    ix.refresh_norms()
    ix.sbq_train()
    ix.sbq_quantize_corpus()
    ix.build_graph(search_list_size=a.build_L)
    ctx.sync()
    say(f"index: {n} nodes, dim {a.dim}, {ix.desc.bits} bits, R {a.R}, built on the device in {time.perf_counter() - t0:.1f} s")
    dq = ctx.alloc(nq * a.dim * 4)
    fill_device(ctx, gp, n, nq, dq)  # queries: rows of the same generator past the corpus
    hq = ctx.download(dq, np.empty((nq, a.dim), np.float32))
    d_ids, d_tids, d_dist = ctx.alloc(nq * k * 4), ctx.alloc(nq * k * 8), ctx.alloc(nq * k * 4)
    d_rows, d_pops, d_state, d_slots = (ctx.alloc(nq * 4) for _ in range(4))
    ctx.upload(d_slots, np.ones(nq, np.uint32))
    tids_all = ix.download(codes=False, nbrs=False, tids=True)["heap_tids"]
    rng = np.random.default_rng(7)
    out = {"rows": n, "dim": a.dim, "scans": nq, "pool_scans": npool, "L": a.L, "rescore": a.rescore, "k": k, "max_pops": mp, "densities": {}}

    def new_way():
        ix.search_batch_dev_qual(dq, nq, a.L, a.rescore, k, d_slots, mp, d_ids, d_rows, d_pops, d_state, d_out_tids=d_tids, d_out_dist=d_dist)
        return ix.search_batch_dev_qual_finish()

    def rows_new():
        return (ctx.download(d_ids, np.empty((nq, k), np.uint32)), ctx.download(d_tids, np.empty((nq, k), np.uint64)),
                ctx.download(d_dist, np.empty((nq, k), np.float32)), ctx.download(d_rows, np.empty(nq, np.uint32)),
                ctx.download(d_pops, np.empty(nq, np.uint32)), ctx.download(d_state, np.empty(nq, np.uint32)))

    def timed_new():
        new_way()
        ctx.profile_enable(True)
        wall, kern = [], []
        for _ in range(a.reps):
            ctx.profile_read(reset=True)
            t = time.perf_counter()
            _, qst = new_way()
            ctx.sync()
            wall.append((time.perf_counter() - t) * 1e3)
            kern.append(sum(v[0] for v in ctx.profile_read(reset=True).values()))
        ctx.profile_enable(False)
        return wall, kern, qst

    pool = P.ScanPool(ix, npool, search_list_size=a.L, rescore=a.rescore, kmax=max(k, 16))
    o_ids, o_tids, o_dist = ctx.alloc(npool * k * 4), ctx.alloc(npool * k * 8), ctx.alloc(npool * k * 4)

    def old_way(bits):
        """-> ids, tids, dist [npool, k], rows, pops, (launches, copies back)"""
        ids = np.full((npool, k), INV, np.uint32)
        td = np.zeros((npool, k), np.uint64)
        ds = np.full((npool, k), np.nan, np.float32)
        rows, pops = np.zeros(npool, np.uint32), np.zeros(npool, np.uint32)
        ix.search_batch_dev(dq, npool, a.L, a.rescore, k, o_ids, o_tids, o_dist)
        ix.search_batch_dev_finish()
        bi, bt, bd = (ctx.download(o_ids, np.empty((npool, k), np.uint32)), ctx.download(o_tids, np.empty((npool, k), np.uint64)),
                      ctx.download(o_dist, np.empty((npool, k), np.float32)))
        copies, fetches = 3, 0
        ended = np.zeros(npool, bool)

        def take(S, ri, rt, rd):
            """the host's post-filter over a block of rows [len(S), kk] of the unfinished scans S (vectorised: the filter is not what is timed)"""
            kk = ri.shape[1]
            valid = ri != INV
            nvalid = valid.cumprod(1).sum(1)  # rows before the scan's end
            allow = np.minimum(nvalid, mp - pops[S])
            inrange = np.arange(kk)[None, :] < allow[:, None]
            ps = inrange & bits[np.where(valid, ri, 0)]
            c = ps.cumsum(1)
            need = (k - rows[S])[:, None]
            keep = ps & (c <= need)
            reached = (c >= need) & inrange
            pops[S] += np.where(reached.any(1), reached.argmax(1) + 1, allow).astype(np.uint32)
            si, ji = np.nonzero(keep)
            dest = rows[S][si] + c[si, ji] - 1
            ids[S[si], dest], td[S[si], dest], ds[S[si], dest] = ri[si, ji], rt[si, ji], rd[si, ji]
            rows[S] += keep.sum(1).astype(np.uint32)
            ended[S] |= nvalid < kk
        take(np.arange(npool), bi, bt, bd)
        # the continuation: a pooled scan starts over, so its first k rows repeat the batch's and are skipped
        for s in range(npool):
            pool.rescan(s, hq[s])
        first = True
        while True:
            left = np.flatnonzero((rows < k) & (pops < mp) & ~ended)
            if first:
                left = np.arange(npool)
            if left.size == 0:
                break
            got, ri, rt, rd = pool.fetch(left, k)
            fetches += 1
            copies += 1
            assert (got >= 0).all(), f"pool errors {got[got < 0][:4]}"
            if not first:
                take(left, ri, rt, rd)
            first = False
        for s in range(npool):
            pool.endscan(s)
        return ids, td, ds, rows, pops, (1 + fetches, copies)

    for dens in (float(x) for x in a.densities.split(",")):
        bits = rng.random(n) < dens
        ix.qual_put(1, bits)
        res = {}
        for mode, name in (("1", "wave-parallel selection"), ("2", "forced replay")):
            P.set_option("VS_RERANK_FUSED", mode)
            wall, kern, qst = timed_new()
            P.set_option("VS_RERANK_FUSED", None)
            got = rows_new()
            if mode == "1":
                first = got
            else:
                assert all((x == y).all() for x, y in zip((g.view(np.uint32) if g.dtype == np.float32 else g for g in got),
                                                          (g.view(np.uint32) if g.dtype == np.float32 else g for g in first))), "modes differ"
            res[name] = dict(wall_ms=round(float(np.median(wall)), 3), kernel_ms=round(float(np.median(kern)), 3), **qst)
            say(f"density {dens}: new way, {name}: wall {spread(wall)} ms, kernels {spread(kern)} ms = {np.median(wall) * 1e3 / nq:.2f} us per scan; "
                f"rounds {qst['rounds']}, first_pops {qst['first_pops']}, scans_rerun {qst['scans_rerun']}, pops_launched {qst['pops_launched']}; "
                f"complete / ended / cut {qst['complete']} / {qst['ended']} / {qst['cut']}")
        # the old way over the first npool scans; rows must be identical before a time is reported
        oi, ot, od, orows, opops, work = old_way(bits)
        gi, gt, gd, grows, gpops, _ = first
        assert (orows == grows[:npool]).all() and (opops == gpops[:npool]).all(), "row / pop counts differ between the two ways"
        assert (oi == gi[:npool]).all() and (ot == gt[:npool]).all() and (od.view(np.uint32) == gd[:npool].view(np.uint32)).all(), "rows differ"
        assert (ot[oi != INV] == tids_all[oi[oi != INV]]).all()
        old = []
        for _ in range(max(a.reps // 2, 2)):
            t = time.perf_counter()
            work = old_way(bits)[5]
            old.append((time.perf_counter() - t) * 1e3)
        say(f"density {dens}: old way over {npool} scans: wall {spread(old)} ms = {np.median(old) * 1e3 / npool:.2f} us per scan; "
            f"{work[0]} launches, {work[1]} copies back; rows identical to the new way's")
        res["old_way"] = dict(wall_ms=round(float(np.median(old)), 3), scans=npool, launches=work[0], copies=work[1])
        out["densities"][str(dens)] = res
    say(json.dumps(out))
    pool.close()
    for p in (dq, d_ids, d_tids, d_dist, d_rows, d_pops, d_state, d_slots, o_ids, o_tids, o_dist):
        ctx.free(p)
    ix.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
