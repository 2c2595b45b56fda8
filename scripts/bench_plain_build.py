#!/usr/bin/env python3
"""What building and growing a `plain` storage index on the device costs.  Nothing here asserts a speed.

Per shape (default 1M x 128 and 1M x 768, L2, R = 50, build L = 100): vs_build_graph seconds (host clock, device synchronised), then
once more with profiling on for the HIP-event milliseconds of the batch kernels (vs_index_build_kernel_ms: build-mode searches, prune
of the new nodes, back-edges; profiling adds an event synchronise per kernel, so that run's wall time is not the build time), nodes
left unreachable, recall@10 of a plain scan (L = 100) against the exact f32 top-10; then an insert of --rows new rows (default
10 000) in one call: seconds, rows/s, the HIP-event milliseconds of the plain mates kernel, the merge and the anchoring rounds
(vs_index_insert_kernel_ms) and of the shared batch kernels, vs_insert_stats, recall@10 of the grown set.

    python scripts/bench_plain_build.py --out profiles/plain_build_1m.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dims", default="128,768")
    ap.add_argument("--R", type=int, default=50)
    ap.add_argument("--rows", type=int, default=10_000)
    ap.add_argument("--build-list", type=int, default=100)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import pgvectorscale_amd as P
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.datagen import DatagenParams, fill_device

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def say(s):
        print(s, flush=True)
        if a.out:  # (line by line: a long run shows where it is)
            with open(a.out, "a") as f:
                f.write(s + "\n")

    ctx = P.Context(0)
    n, m, R, L, nq = a.n, a.rows, a.R, a.build_list, a.queries
    for dim in [int(x) for x in a.dims.split(",")]:
        p = DatagenParams(seed=1, dim=dim, latent_dim=32, n_clusters=1024)
        say(f"# plain build bench: n={n} dim={dim} R={R} build L={L} insert rows={m} on {ctx.device_name()}")

        def fresh(rows):
            ix = P.DiskAnnIndex.alloc(ctx, n=rows, dim_full=dim, num_neighbors=R, distance_type=P.VS_L2, storage_type=_lib.VS_STORAGE_PLAIN)
            fill_device(ctx, p, 0, rows, ix.array(_lib.ARR_VECS)[0])
            return ix

        d_q = ctx.alloc(nq * dim * 4)
        fill_device(ctx, p, 10 ** 9, nq, d_q)
        q = ctx.download(d_q, np.empty((nq, dim), np.float32))

        def recall(ix):
            gt = ix.bruteforce_topk(d_q, nq, 10)[0]
            gi = ix.search_batch(q, search_list_size=100, rescore=0, k=10)[0]
            return float(np.mean([len(set(g.tolist()) & set(t.tolist())) / 10 for g, t in zip(gi, gt)]))

        ix = fresh(n)
        ctx.sync()
        t0 = time.perf_counter()
        ix.build_graph(search_list_size=L, max_alpha=1.2)
        ctx.sync()
        say(f"vs_build_graph of {n} rows: {time.perf_counter() - t0:.2f} s; unreachable {ix.build_unreachable()}; recall@10 (L=100) {recall(ix):.4f}")

        ctx.profile_enable(True)
        ix.build_kernel_ms(reset=True)
        ix.build_graph(search_list_size=L, max_alpha=1.2)
        ctx.sync()
        ms = ix.build_kernel_ms()
        say(f"the same with profiling on: k_search<BUILD, PLAIN> {ms['search']:.1f} ms, k_build_prune_new<PLAIN> {ms['prune']:.1f} ms, "
            f"back-edges (sort + k_build_backedges<PLAIN>) {ms['back_edges']:.1f} ms")

        d_new = ctx.alloc(m * dim * 4)
        fill_device(ctx, p, n, m, d_new)
        new = ctx.download(d_new, np.empty((m, dim), np.float32))
        ctx.free(d_new)
        tids = (np.arange(n, n + m, dtype=np.uint64) << np.uint64(16)) | np.uint64(1)
        ix.reserve(n + m)
        ix.insert_kernel_ms(reset=True)
        ctx.sync()
        t0 = time.perf_counter()
        st = ix.insert(new, tids, search_list_size=L)
        ctx.sync()
        dt = time.perf_counter() - t0
        ims, bms = ix.insert_kernel_ms(), ix.build_kernel_ms()
        ctx.profile_enable(False)
        say(f"vs_index_insert of {m} rows in one call (profiling on): {dt:.3f} s = {m / dt:.0f} rows/s; k_batch_mates_plain {ims['batch_mates']:.2f} ms, "
            f"k_insert_merge_mates {ims['merge_mates']:.2f} ms, k_insert_anchor {ims['anchor']:.2f} ms, searches {bms['search']:.1f} ms, prune "
            f"{bms['prune']:.1f} ms, back-edges {bms['back_edges']:.1f} ms; {st}; recall@10 of the grown set {recall(ix):.4f}")
        ix.close()
        ctx.free(d_q)
    ctx.close()


if __name__ == "__main__":
    main()
