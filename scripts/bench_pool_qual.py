#!/usr/bin/env python3
"""Qualified scan pools (vs_scanpool_fetch_qual): what the pages of `ORDER BY embedding <=> $1 ... WHERE ...` cost when a pool continues
its scans to their next k QUALIFYING rows on the device, next to the way to the same rows before — ScanPool.fetch rounds of k rows
with the filter on the host (vectorised numpy), as scripts/bench_qual.py does — and, for the first page, next to the one-shot
vs_search_batch_qual on the same queries.  One process, one box, an SBQ index over generated vectors built on the device, one pool of
--slots scans shared by both pool ways (the same kmax, so the same rows per search round).

  (a) the first k qualifying rows of every scan           new: one fetch_qual     old: fetch rounds + host filter     batch: search_batch_qual
  (b) three further pages of k                            new: three fetch_qual   old: fetch rounds + host filter

What is timed is the fetch calls (and the host filter between them, for the old way); the vs_scanpool_rescan calls that open the scans
are outside the clock on every side.  Rows, tids and distance bits of all sides are compared, and must be equal, before any time is
printed.  Medians of --reps warm repetitions with min .. max; search rounds, window launches and copies back next to them.  No ratio
is fixed in advance.

    python scripts/bench_pool_qual.py --out profiles/r23/pool_qual_4m.txt
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
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--rescore", type=int, default=50)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--kmax", type=int, default=64)
    ap.add_argument("--pages", type=int, default=3, help="further pages after the first")
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

    n, G, k, mp, pages = a.rows, a.slots, a.k, a.max_pops, 1 + a.pages
    ctx = P.Context(0)
    say(f"bench_pool_qual on {ctx.device_name()}: rows {n}, dim {a.dim}, R {a.R}, pool slots {G}, L {a.L} rescore {a.rescore} k {k} kmax {a.kmax} "
        f"max_pops {mp}, pages 1 + {a.pages}, reps {a.reps}")
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
    dq = ctx.alloc(G * a.dim * 4)
    fill_device(ctx, gp, n, G, dq)  # queries: rows of the same generator past the corpus
    hq = ctx.download(dq, np.empty((G, a.dim), np.float32))
    ctx.free(dq)
    rng = np.random.default_rng(7)
    pool = P.ScanPool(ix, G, search_list_size=a.L, rescore=a.rescore, kmax=a.kmax)
    everybody = np.arange(G, dtype=np.uint32)
    ones = np.ones(G, np.uint32)
    out = {"rows": n, "dim": a.dim, "slots": G, "L": a.L, "rescore": a.rescore, "k": k, "kmax": a.kmax, "max_pops": mp, "pages": pages, "densities": {}}

    def open_scans():
        for s in range(G):
            pool.rescan(s, hq[s])

    def new_way():
        """-> per page (ids, tids, dist, rows, pops, state), per page qstats, ms of the first page, ms of the further pages"""
        open_scans()
        ctx.sync()
        got, stats, ms = [], [], []
        for _ in range(pages):
            t = time.perf_counter()
            rows, ids, tids, dist, pops, state, qst = pool.fetch_qual(everybody, k, ones, mp)
            ms.append((time.perf_counter() - t) * 1e3)
            assert (rows >= 0).all(), f"pool errors {rows[rows < 0][:4]}"
            got.append((ids, tids, dist, rows, pops, state))
            stats.append(qst)
        return got, stats, ms[0], sum(ms[1:])

    def old_way(bits):
        """fetch rounds of k rows, the qualifier applied on the host: -> the first pages * k qualifying rows per scan (ids, tids, dist
        [G, pages * k]), rows per scan, (fetches, copies back) up to the first page and in all, ms of the first page, ms of the rest"""
        open_scans()
        ctx.sync()
        want = pages * k
        ids = np.full((G, want), INV, np.uint32)
        td = np.zeros((G, want), np.uint64)
        ds = np.zeros((G, want), np.float32)
        have = np.zeros(G, np.int64)
        ended = np.zeros(G, bool)
        fetches, marks, ms = 0, [], []
        for pg in range(1, pages + 1):
            t = time.perf_counter()
            while True:
                left = np.flatnonzero((have < pg * k) & ~ended).astype(np.uint32)
                if left.size == 0:
                    break
                got, ri, rt, rd = pool.fetch(left, k)
                fetches += 1
                assert (got >= 0).all(), f"pool errors {got[got < 0][:4]}"
                # the host's post-filter over the block [len(left), k] (vectorised: the filter is a small part of what is timed)
                valid = np.arange(k)[None, :] < got[:, None]
                ps = valid & bits[np.where(valid, ri, 0)]
                dest = have[left][:, None] + ps.cumsum(1) - 1
                keep = ps & (dest < want)
                si, ji = np.nonzero(keep)
                ids[left[si], dest[si, ji]], td[left[si], dest[si, ji]], ds[left[si], dest[si, ji]] = ri[si, ji], rt[si, ji], rd[si, ji]
                have[left] += ps.sum(1)
                ended[left] |= got < k
            ms.append((time.perf_counter() - t) * 1e3)
            marks.append(fetches)
        return ids, td, ds, np.minimum(have, want), (marks[0], marks[-1]), ms[0], sum(ms[1:])

    def batch_way():
        t = time.perf_counter()
        r = ix.search_batch_qual(hq, ones, k=k, max_pops=mp, search_list_size=a.L, rescore=a.rescore)
        return r, (time.perf_counter() - t) * 1e3

    for dens in (float(x) for x in a.densities.split(",")):
        bits = rng.random(n) < dens
        ix.qual_put(1, bits)
        # ---- the rows of all sides, compared before any time is printed
        got, stats, _, _ = new_way()
        oi, ot, od, orows, _, _, _ = old_way(bits)
        assert all((g[5] == _lib.QUAL_COMPLETE).all() for g in got), "a scan did not complete within max_pops: raise --max-pops"
        for pg, (gi, gt, gd, grows, gpops, gstate) in enumerate(got):
            sl = slice(pg * k, (pg + 1) * k)
            assert (grows == k).all() and (orows == pages * k).all(), "row counts differ between the two pool ways"
            assert (gi == oi[:, sl]).all() and (gt == ot[:, sl]).all() and (gd.view(np.uint32) == od[:, sl].view(np.uint32)).all(), f"page {pg}: rows differ"
        (bi, bt, bd, brows, bpops, bstate, _, bq), _ = batch_way()
        assert (brows == k).all() and (bpops == got[0][4]).all() and (bstate == got[0][5]).all(), "the batch's counts differ from the first page's"
        assert (bi == got[0][0]).all() and (bt == got[0][1]).all() and (bd.view(np.uint32) == got[0][2].view(np.uint32)).all(), "batch rows differ"
        # ---- times
        new_a, new_b, old_a, old_b, bat = [], [], [], [], []
        for _ in range(a.reps):
            _, stats, ta, tb = new_way()
            new_a.append(ta)
            new_b.append(tb)
            *_, work, ta, tb = old_way(bits)
            old_a.append(ta)
            old_b.append(tb)
            bat.append(batch_way()[1])
        pops = [int(s["pops"]) for s in stats]
        rounds = [int(s["search_rounds"]) for s in stats]
        wins = [int(s["window_launches"]) for s in stats]
        say(f"density {dens}: (a) first {k} qualifying rows of {G} scans: fetch_qual wall {spread(new_a)} ms; P1 {stats[0]['first_pops']}, pops {pops[0]}, "
            f"{rounds[0]} search rounds, {wins[0]} window launches, 1 copy of rows back (+ {wins[0]} of the records)")
        say(f"density {dens}: (a) the parent's way, fetch rounds + host filter: wall {spread(old_a)} ms; {work[0]} fetches = {work[0]} window launches and copies back")
        say(f"density {dens}: (a) vs_search_batch_qual over the same {G} queries (host entry point): wall {spread(bat)} ms; rounds {bq['rounds']}, "
            f"scans_rerun {bq['scans_rerun']}, pops_launched {bq['pops_launched']}")
        say(f"density {dens}: (b) {a.pages} further pages of {k}: fetch_qual wall {spread(new_b)} ms; pops {sum(pops[1:])}, {sum(rounds[1:])} search rounds, "
            f"{sum(wins[1:])} window launches, {a.pages} copies of rows back (+ {sum(wins[1:])} of the records)")
        say(f"density {dens}: (b) the parent's way: wall {spread(old_b)} ms; {work[1] - work[0]} fetches = window launches and copies back")
        say(f"density {dens}: rows, tids and distance bits of all sides identical")
        out["densities"][str(dens)] = dict(
            new_first_ms=round(float(np.median(new_a)), 3), new_more_ms=round(float(np.median(new_b)), 3), old_first_ms=round(float(np.median(old_a)), 3),
            old_more_ms=round(float(np.median(old_b)), 3), batch_first_ms=round(float(np.median(bat)), 3), first_pops=int(stats[0]["first_pops"]), pops=pops,
            search_rounds=rounds, window_launches=wins, old_fetches_first=int(work[0]), old_fetches_all=int(work[1]), batch_rounds=int(bq["rounds"]))
    say(json.dumps(out))
    pool.close()
    ix.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
