#!/usr/bin/env python3
"""The wide-k qualified calls (vs_search_batch_qual_exact_wide_dev / vs_search_batch_qual_flat_wide_dev): what k up to 4096 costs
under a selective WHERE clause.  Nothing before them serves k > 64, so the yardstick is the narrow exact call at k = 64 on the same
index, batch and slots in the same process.  One box, an SBQ index over generated vectors on the device (no graph: none is walked).

  per density  the narrow exact call at k = 64, then the wide exact call at every k of --ks: wall time (call to synchronised outputs)
               and the profile spans — scan (the row lists), rerank (k_qwide_dist: the distances and keys), resort (k_qwide_pick:
               selection AND sort, one kernel); the ratio wide / narrow at k = 64 and the growth from k = 64 to the largest k
  flat         the flat wide call at every k with rescore = max(k, --rescore): wall, spans (search = Hamming, rerank_order = pick,
               rerank, resort = k_qflat_final_wide: the sort) and recall against the exact wide call's rows
  before any time: wide == narrow at k = 64, ids, distance bits and rows of every scan

Medians of --reps warm repetitions with min .. max, the calls alternating inside a repetition.  No number is fixed in advance.

    python scripts/bench_qual_wide.py --out profiles/r29/qual_wide_4m.txt
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
    ap.add_argument("--scans", type=int, default=8192)
    ap.add_argument("--ks", default="64,100,1000,4096")
    ap.add_argument("--rescore", type=int, default=200)
    ap.add_argument("--densities", default="0.05,0.01,0.001,0.0001")
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
        return f"{np.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"

    nq, dim, n = a.scans, a.dim, a.rows
    ks = [int(x) for x in a.ks.split(",")]
    kmax = max(ks + [64])
    ctx = P.Context(0)
    gp = DatagenParams(seed=3, dim=dim, latent_dim=min(32, dim))
    say(f"bench_qual_wide on {ctx.device_name()}: rows {n}, dim {dim}, scans {nq}, k {ks}, reps {a.reps}")
    dq, d_slots, d_rows = ctx.alloc(nq * dim * 4), ctx.alloc(nq * 4), ctx.alloc(nq * 4)
    d_ids, d_tids, d_dist = ctx.alloc(nq * kmax * 4), ctx.alloc(nq * kmax * 8), ctx.alloc(nq * kmax * 4)
    t0 = time.perf_counter()
    ix = P.DiskAnnIndex.alloc(ctx, n=n, dim_full=dim, num_neighbors=4, distance_type=P.VS_L2)
    fill_device(ctx, gp, 0, n, ix.array(_lib.ARR_VECS)[0])
    ix.refresh_norms()
    ix.sbq_train()
    ix.sbq_quantize_corpus()
    fill_device(ctx, gp, n, nq, dq)  # queries: rows of the same generator past the corpus
    ctx.sync()
    say(f"index: {n} nodes, dim {dim}, no graph, on the device in {time.perf_counter() - t0:.1f} s")

    def call(kind, k):
        if kind == "narrow":
            return ix.search_batch_qual_exact_dev(dq, nq, k, d_slots, d_ids, d_rows, d_out_tids=d_tids, d_out_dist=d_dist)
        if kind == "wide":
            return ix.search_batch_qual_exact_wide_dev(dq, nq, k, d_slots, d_ids, d_rows, d_out_tids=d_tids, d_out_dist=d_dist)
        return ix.search_batch_qual_flat_wide_dev(dq, nq, k, max(k, a.rescore), d_slots, d_ids, d_rows, d_out_tids=d_tids, d_out_dist=d_dist)

    def rows_back(k):
        return (ctx.download(d_ids, np.empty((nq, k), np.uint32)), ctx.download(d_dist, np.empty((nq, k), np.float32)).view(np.uint32),
                ctx.download(d_rows, np.empty(nq, np.uint32)))

    def timed(variants):
        """[(kind, k)] -> {(kind, k): (wall ms per repetition, {span: median ms})}, the variants alternating inside a repetition"""
        for v in variants:
            call(*v)
        ctx.sync()
        ctx.profile_enable(True)
        wall, spans = {v: [] for v in variants}, {v: [] for v in variants}
        for _ in range(a.reps):
            for v in variants:
                ctx.profile_read(reset=True)
                t = time.perf_counter()
                call(*v)
                ctx.sync()
                wall[v].append((time.perf_counter() - t) * 1e3)
                spans[v].append({name: ms for name, (ms, launches) in ctx.profile_read(reset=True).items() if launches})
        ctx.profile_enable(False)
        return {v: (wall[v], {name: float(np.median([s.get(name, 0.0) for s in spans[v]])) for name in spans[v][0]}) for v in variants}

    out = {"rows": n, "dim": dim, "scans": nq, "densities": {}}
    rng = np.random.default_rng(7)
    ctx.upload(d_slots, np.ones(nq, np.uint32))
    for dens in (float(x) for x in a.densities.split(",")):
        ix.qual_put(1, rng.random(n) < dens)
        call("narrow", 64)
        narrow = rows_back(64)
        call("wide", 64)
        assert all((g == e).all() for g, e in zip(rows_back(64), narrow)), "wide differs from narrow at k = 64"
        res = timed([("narrow", 64)] + [("wide", k) for k in ks])
        w64 = float(np.median(res[("narrow", 64)][0]))
        say(f"density {dens}: narrow exact k 64: wall {spread(res[('narrow', 64)][0])} ms, spans {res[('narrow', 64)][1]}; wide == narrow at k 64 on all {nq} scans")
        rec = {"narrow_64_ms": w64}
        for k in ks:
            wall, spans = res[("wide", k)]
            say(f"density {dens}: wide exact k {k}: wall {spread(wall)} ms = {np.median(wall) / w64:.3f} x narrow k 64; distance {spans.get('rerank', 0):.3f} ms, "
                f"selection + sort {spans.get('resort', 0):.3f} ms, lists {spans.get('scan', 0):.3f} ms")
            rec[f"wide_{k}"] = dict(wall_ms=float(np.median(wall)), ratio_to_narrow_64=float(np.median(wall)) / w64, **spans)
        if 64 in ks:
            say(f"density {dens}: growth k 64 -> {max(ks)}: {rec[f'wide_{max(ks)}']['wall_ms'] / rec['wide_64']['wall_ms']:.3f}")
        for k in ks:  # the flat wide call against the exact wide call's rows
            call("wide", k)
            ei, _, er = rows_back(k)
            wall, spans = timed([("flat", k)])[("flat", k)]
            fi = rows_back(k)[0]
            hit = sum(np.isin(ei[s, :er[s]], fi[s]).sum() for s in range(0, nq, max(nq // 256, 1)))
            tot = sum(int(er[s]) for s in range(0, nq, max(nq // 256, 1)))
            say(f"density {dens}: flat wide k {k}, rescore {max(k, a.rescore)}: wall {spread(wall)} ms; Hamming {spans.get('search', 0):.3f}, pick "
                f"{spans.get('rerank_order', 0):.3f}, rerank {spans.get('rerank', 0):.3f}, sort {spans.get('resort', 0):.3f} ms; recall@{k} "
                f"{hit / max(tot, 1):.4f} over {len(range(0, nq, max(nq // 256, 1)))} scans")
            rec[f"flat_{k}"] = dict(wall_ms=float(np.median(wall)), recall=hit / max(tot, 1), **spans)
        out["densities"][str(dens)] = rec
    say(json.dumps(out))
    for p in (dq, d_slots, d_rows, d_ids, d_tids, d_dist):
        ctx.free(p)
    ix.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
