#!/usr/bin/env python3
"""What vs_index_insert costs on a device-built index, beside the only alternative there was: vs_build_graph of the grown set.

On an n x dim index (default: the plain bench's 4M x 768, SBQ 2 bit, R = 50) --rows new rows (default 65 536) are inserted in calls
of 1, 256 and 65 536 rows, each mode on a fresh copy of the same built index.  Per mode: rows/s and ms per call (host clock around
the calls, vectors from host memory: the PCIe leg is part of an aminsert), the HIP-event time of the three insert kernels
(vs_index_insert_kernel_ms; profiling is on, which adds an event synchronise per kernel), mate_edges / orphans_placed /
orphans_left, and recall@10 (L = 100, rescore 50) of a fixed query set against the exact f32 top-10 of the grown set, before and
after — overall, and of the ground-truth entries that are NEW rows (half of the queries are new rows' own neighbourhoods: rows of the
same stream that follow the inserted ones).  --single-calls bounds the number of one-row calls (the rest of that mode's rows is not
inserted; recall is then not comparable and says so).  --mates "0,8,16,32" repeats the 65 536- and 256-row modes per
VS_INSERT_MATES.  Last: vs_build_graph over all n + rows rows, timed, same recall.  Nothing here asserts a speed.

    python scripts/bench_insert.py --out profiles/r08/s3_insert_4m.txt
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
    ap.add_argument("--n", type=int, default=4_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--R", type=int, default=50)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--build-list", type=int, default=100)
    ap.add_argument("--single-calls", type=int, default=65536)
    ap.add_argument("--mates", default="16")
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import pgvectorscale_amd as P
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.datagen import DatagenParams, fill_device

    lines = []

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:  # (line by line: a long run shows where it is)
            with open(a.out, "a") as f:
                f.write(s + "\n")

    ctx = P.Context(0)
    n, m, dim, R, L = a.n, a.rows, a.dim, a.R, a.build_list
    p = DatagenParams(seed=1, dim=dim, latent_dim=32, n_clusters=1024)
    say(f"# insert bench: n={n} dim={dim} R={R} rows={m} build L={L} on {ctx.device_name()}")

    def fresh(rows):
        ix = P.DiskAnnIndex.alloc(ctx, n=rows, dim_full=dim, num_neighbors=R, distance_type=P.VS_L2)
        fill_device(ctx, p, 0, rows, ix.array(_lib.ARR_VECS)[0])
        return ix

    # the base index, built once; every mode starts from a copy of its graph and quantizer
    base = fresh(n)
    t0 = time.perf_counter()
    base.sbq_train()
    base.sbq_quantize_corpus()
    base.build_graph(search_list_size=L, max_alpha=1.2)
    ctx.sync()
    say(f"base index: train + quantise + vs_build_graph of {n} rows {time.perf_counter() - t0:.2f} s")
    quant = base.get_quantizer()
    gp, stride = base.array(_lib.ARR_NBRS)
    graph = ctx.download(gp, np.empty((n, stride), np.uint32))
    base.close()

    # the new rows (host memory) and the queries: half anywhere in the stream, half right behind the new rows
    d_new = ctx.alloc(m * dim * 4)
    fill_device(ctx, p, n, m, d_new)
    new = ctx.download(d_new, np.empty((m, dim), np.float32))
    ctx.free(d_new)
    tids = (np.arange(n, n + m, dtype=np.uint64) << np.uint64(16)) | np.uint64(1)
    nq = a.queries
    d_q = ctx.alloc(nq * dim * 4)
    fill_device(ctx, p, 10 ** 9, nq // 2, d_q)
    d_q2 = ctx.alloc((nq - nq // 2) * dim * 4)
    fill_device(ctx, p, n + m, nq - nq // 2, d_q2)
    q = np.concatenate([ctx.download(d_q, np.empty((nq // 2, dim), np.float32)), ctx.download(d_q2, np.empty((nq - nq // 2, dim), np.float32))])
    ctx.free(d_q2)
    ctx.free(d_q)
    d_q = ctx.alloc(nq * dim * 4)
    ctx.upload(d_q, q)

    def copy_of_base():
        ix = fresh(n)
        ix.set_quantizer(*quant)
        ix.sbq_quantize_corpus()
        ctx.upload(ix.array(_lib.ARR_NBRS)[0], graph)
        ix.set_start_nodes(0)
        return ix

    def recalls(ix, gt):
        gi = ix.search_batch(q, search_list_size=100, rescore=50, k=10)[0]
        hit = tot = hit_new = tot_new = 0
        for g, t in zip(gi, gt):
            s = set(g.tolist())
            for v in t.tolist():
                tot += 1
                hit += v in s
                if v >= n:
                    tot_new += 1
                    hit_new += v in s
        return hit / tot, (hit_new / tot_new if tot_new else float("nan")), tot_new

    # ground truth of the grown set, from an index that only needs the vectors
    full = fresh(n + m)
    gt_after = full.bruteforce_topk(d_q, nq, 10)[0]
    full.close()
    ix = copy_of_base()
    gt_before = ix.bruteforce_topk(d_q, nq, 10)[0]
    r0 = recalls(ix, gt_before)
    say(f"recall@10 before any insert (against the exact top-10 of the {n} rows): {r0[0]:.4f}")
    ix.close()

    ctx.profile_enable(True)
    for mates in [int(x) for x in a.mates.split(",")]:
        P.set_option("VS_INSERT_MATES", mates)
        for per_call in (65536, 256, 1):
            if per_call == 1 and mates != 16 and len(a.mates.split(",")) > 1:
                continue
            per_call = min(per_call, m)
            ncalls = (m + per_call - 1) // per_call
            if per_call == 1:
                ncalls = min(ncalls, a.single_calls)
            ix = copy_of_base()
            ix.reserve(n + m)  # (growth is a cost of its own: timed below, once)
            ix.insert_kernel_ms(reset=True)
            tot = dict(mate_edges=0, orphans_placed=0, orphans_left=0, batches=0, retries=0)
            ctx.sync()
            t0 = time.perf_counter()
            done = 0
            for c in range(ncalls):
                lo, hi = c * per_call, min(m, (c + 1) * per_call)
                st = ix.insert(new[lo:hi], tids[lo:hi], search_list_size=L)
                done += hi - lo
                for k in tot:
                    tot[k] += st[k]
            ctx.sync()
            dt = time.perf_counter() - t0
            ms = ix.insert_kernel_ms()
            line = (f"mates={mates} calls of {per_call}: {done} rows in {ncalls} calls, {dt:.3f} s = {done / dt:.0f} rows/s, {dt / ncalls * 1e3:.3f} ms per call; "
                    f"kernels: k_batch_mates {ms['batch_mates']:.2f} ms ({ms['batch_mates'] / dt / 10:.1f} %), k_insert_merge_mates "
                    f"{ms['merge_mates']:.2f} ms ({ms['merge_mates'] / dt / 10:.1f} %), k_insert_anchor {ms['anchor']:.2f} ms ({ms['anchor'] / dt / 10:.1f} %); "
                    f"batches {tot['batches']} retries {tot['retries']} mate_edges {tot['mate_edges']} orphans_placed {tot['orphans_placed']} "
                    f"orphans_left {tot['orphans_left']}")
            if done == m:
                r = recalls(ix, gt_after)
                line += f"; recall@10 after {r[0]:.4f}, of the {r[2]} ground-truth entries that are new rows {r[1]:.4f}"
            else:
                line += f"; recall not comparable ({m - done} rows not inserted)"
            say(line)
            ix.close()
    ctx.profile_enable(False)
    P.set_option("VS_INSERT_MATES", None)

    # growth on its own
    ix = copy_of_base()
    ctx.sync()
    t0 = time.perf_counter()
    ix.reserve(n + m)
    ctx.sync()
    say(f"vs_index_reserve from {n} to {n + m} rows: {(time.perf_counter() - t0) * 1e3:.1f} ms")
    ix.close()

    # the alternative: the whole grown set built again
    ix = fresh(n + m)
    ix.set_quantizer(*quant)
    ix.sbq_quantize_corpus()
    ctx.sync()
    t0 = time.perf_counter()
    ix.build_graph(search_list_size=L, max_alpha=1.2)
    ctx.sync()
    dt = time.perf_counter() - t0
    r = recalls(ix, gt_after)
    say(f"vs_build_graph of the grown set ({n + m} rows, same quantizer): {dt:.2f} s; recall@10 {r[0]:.4f}, of the new rows' entries {r[1]:.4f}")
    ix.close()
    ctx.free(d_q)
    ctx.close()


if __name__ == "__main__":
    main()
