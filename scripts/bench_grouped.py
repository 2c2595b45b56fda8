#!/usr/bin/env python3
"""Grouped scans (vs_search_batch_grouped): what "the k nearest DOCUMENTS" costs over a corpus whose rows are chunks, next to the way to
the same rows without the call.  One process, one box, an SBQ index over generated vectors built on the device.

  leg (a)   one vs_search_batch_grouped (host queries in, host rows out) over --scans scans, per_group 1, k distinct groups
  leg (b)   vs_search_batch at k' = 2 k, the first row of every group kept on the host (vectorised numpy), the scans that are short of k
            groups run again from the start at twice the k', up to max_pops — all of it inside the clock
  the rows of the two legs are compared (node ids, tids, distance bits, rows, pops) before any time is reported

The chunk-of-a-document case: a group's rows are neighbours.  The generator draws a row's cluster from a hash of the row number, so the
rows are put in cluster order (a stable sort by the generator's own cluster number) and the j-th row of that order gets group
j // size — a group of mean size `size` whose rows share a cluster, which is node i -> i // size on a corpus stored in cluster order.
Mean group sizes 1, 4 and 16.  A sample is --inner calls of a leg back to back (the time per call is reported); medians of --reps warm
samples with min .. max, the legs alternating.  No ratio is fixed in advance.

    python scripts/bench_grouped.py --out profiles/r27/grouped_4m.txt
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


def first_of_each_group(g, valid):
    """g [m, kk] int64 group per row of a scan's rows, in scan order -> bool [m, kk]: the row is the first of its group in its scan"""
    order = np.argsort(g, axis=1, kind="stable")
    gs = np.take_along_axis(g, order, 1)
    firsts = np.ones(gs.shape, bool)
    firsts[:, 1:] = gs[:, 1:] != gs[:, :-1]
    keep = np.zeros(gs.shape, bool)
    np.put_along_axis(keep, order, firsts, 1)
    return keep & valid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--R", type=int, default=50)
    ap.add_argument("--build-L", type=int, default=64)
    ap.add_argument("--scans", type=int, default=8192)
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--rescore", type=int, default=50)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--max-pops", type=int, default=2048)
    ap.add_argument("--sizes", default="1,4,16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pgvectorscale_amd as P
    from pgvectorscale_amd import _lib, datagen
    from pgvectorscale_amd.datagen import DatagenParams, fill_device
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def spread(v):
        return f"{np.median(v):.2f} ({min(v):.2f} .. {max(v):.2f})"

    n, nq, k, mp = a.rows, a.scans, a.k, a.max_pops
    ctx = P.Context(0)
    say(f"bench_grouped on {ctx.device_name()}: rows {n}, dim {a.dim}, R {a.R}, scans {nq}, L {a.L} rescore {a.rescore} k {k} per_group 1 "
        f"max_pops {mp}, reps {a.reps} of {a.inner} calls")
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
    ctx.free(dq)
    cluster = (datagen._hash(gp.seed, np.arange(n, dtype=np.uint64), np.uint64(0)) % np.uint64(gp.n_clusters)).astype(np.int64)
    by_cluster = np.argsort(cluster, kind="stable")
    out = {"rows": n, "dim": a.dim, "scans": nq, "L": a.L, "rescore": a.rescore, "k": k, "max_pops": mp, "sizes": {}}

    def leg_a():
        return ix.search_batch_grouped(hq, k=k, per_group=1, max_pops=mp, search_list_size=a.L, rescore=a.rescore)

    def leg_b(groups):
        """-> ids, tids, dist [nq, k], rows, pops [nq], launches"""
        ids, td, ds = np.full((nq, k), INV, np.uint32), np.zeros((nq, k), np.uint64), np.full((nq, k), np.nan, np.float32)
        rows, pops = np.zeros(nq, np.uint32), np.zeros(nq, np.uint32)
        left, kk, launches = np.arange(nq), min(2 * k, mp), 0
        while left.size:
            ri, rt, rd = ix.search_batch(hq[left], search_list_size=a.L, rescore=a.rescore, k=kk)[:3]
            launches += 1
            valid = ri != INV
            g = np.where(valid, groups[np.where(valid, ri, 0)].astype(np.int64), (1 << 40) + np.arange(kk, dtype=np.int64)[None, :])
            keep = first_of_each_group(g, valid)
            c = keep.cumsum(1)
            keep &= c <= k
            done = (c[:, -1] >= k) | ~valid[:, -1] | (kk == mp)
            S, kd, cd = left[done], keep[done], c[done]
            si, ji = np.nonzero(kd)
            ids[S[si], cd[si, ji] - 1], td[S[si], cd[si, ji] - 1], ds[S[si], cd[si, ji] - 1] = ri[done][si, ji], rt[done][si, ji], rd[done][si, ji]
            rows[S] = kd.sum(1)
            full = cd[:, -1] >= k
            pops[S] = np.where(full, (cd >= k).argmax(1) + 1, valid[done].sum(1))
            left, kk = left[~done], min(2 * kk, mp)
        return ids, td, ds, rows, pops, launches

    for size in (int(x) for x in a.sizes.split(",")):
        groups = np.empty(n, np.uint32)
        groups[by_cluster] = (np.arange(n) // size).astype(np.uint32)
        ix.groups_put(groups)
        got = leg_a()
        old = leg_b(groups)
        assert (old[3] == got[3]).all() and (old[4] == got[4]).all(), "row / pop counts differ between the two legs"
        assert (old[0] == got[0]).all() and (old[1] == got[1]).all() and (old[2].view(np.uint32) == got[2].view(np.uint32)).all(), "rows differ"
        ta, tb = [], []
        for _ in range(a.reps):  # (alternating: other work shares the host)
            t = time.perf_counter()
            for _ in range(a.inner):
                qst = leg_a()[7]
            ta.append((time.perf_counter() - t) * 1e3 / a.inner)
            t = time.perf_counter()
            for _ in range(a.inner):
                launches = leg_b(groups)[5]
            tb.append((time.perf_counter() - t) * 1e3 / a.inner)
        complete = got[5] == 0
        ppk = float((got[4][complete] / k).mean()) if complete.any() else float("nan")
        say(f"group size {size}: (a) grouped call: wall {spread(ta)} ms = {np.median(ta) * 1e3 / nq:.2f} us per scan; rounds {qst['rounds']}, "
            f"first_pops {qst['first_pops']}, scans_rerun {qst['scans_rerun']}, pops_launched {qst['pops_launched']}; complete / ended / cut "
            f"{qst['complete']} / {qst['ended']} / {qst['cut']}; pops per kept row {ppk:.2f} (complete scans; max {int(got[4].max())} pops)")
        say(f"group size {size}: (b) search_batch + host dedupe: wall {spread(tb)} ms = {np.median(tb) * 1e3 / nq:.2f} us per scan; {launches} "
            f"batches; rows identical to (a)'s")
        out["sizes"][str(size)] = dict(a_wall_ms=round(float(np.median(ta)), 3), b_wall_ms=round(float(np.median(tb)), 3), b_batches=launches,
                                       pops_per_kept_row=round(ppk, 3), **qst)
    say(json.dumps(out))
    ix.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
