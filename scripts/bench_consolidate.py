#!/usr/bin/env python3
"""What vs_index_consolidate_deletes costs and buys, on the device-built index of scripts/bench_pages_write.py (4M x 768, R = 50).

Per deleted fraction (10 % and 30 % of the rows, random TIDs, fixed seed, through vs_index_bulk_delete), each on the graph as built:
  (a) search_batch before the pass: QPS, recall@10 against vs_bruteforce_topk over the live rows alone, quantized distance comparisons
      per scan (L = 100, rescore = 50);
  (b) the call: wall time, and the HIP-event time of its two passes (flag pass, k_consolidate_rows) from vs_index_consolidate_kernel_ms;
  (c) the same searches after the pass;
  (d) vs_pages_out_delta against a baseline taken before the delete: dirty blocks of the total;
  (e) what a user does today: vs_build_graph over the live rows alone, same session (wall time, and its recall as the yardstick).
Nothing here asserts a number.  The expectations the lines are reported against: (b) is far cheaper than (e); the comparisons per
scan fall by about the deleted fraction; recall does not fall below (e)'s by more than the build's seed-to-seed spread (0.0117).

    python scripts/bench_consolidate.py --out profiles/r11/s1_consolidate_4m.txt

--plain: the same legs on a `plain` storage index built on the device (no SBQ training or codes; vs_index_consolidate_deletes_plain,
vs_pages_out_open_plain).  A plain scan compares no codes, so the work per scan is reported as full-precision distance comparisons, and
(b) adds the rows k_consolidate_rows rewrites per second of its own HIP-event time.

    python scripts/bench_consolidate.py --plain --n 1000000 --out profiles/consolidate_plain_1m.txt
"""
import argparse
import json
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
    ap.add_argument("--build-list", type=int, default=100)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fractions", default="0.1,0.3")
    ap.add_argument("--plain", action="store_true", help="a plain storage index: vs_index_consolidate_deletes_plain")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import pgvectorscale_amd as P
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.datagen import DatagenParams, fill_device
    from pgvectorscale_amd.pages import PagesOut

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = P.Context(0)
    p = DatagenParams(seed=8, dim=a.dim)
    work_key = "full_distance_comparisons" if a.plain else "quantized_distance_comparisons"
    say(f"# consolidate{' (plain storage)' if a.plain else ''}: n={a.n} dim={a.dim} R={a.R} build L={a.build_list} nq={a.nq} on {ctx.device_name()}")
    tids = ((np.arange(a.n, dtype=np.uint64) + 1) << np.uint64(16)) | np.uint64(1)

    host_rows = []  # the vector column on the host, fetched once (the rebuilds over the live rows upload a subset of it)

    def build(rows, src=None, keep=None):
        """an index over `rows` rows: generated in place, or the rows `keep` of the device vector array `src`"""
        ix = P.DiskAnnIndex.alloc(ctx, n=rows, dim_full=a.dim, num_neighbors=a.R, distance_type=P.VS_L2,
                                  storage_type=_lib.VS_STORAGE_PLAIN if a.plain else _lib.VS_STORAGE_SBQ)
        vp, stride = ix.array(_lib.ARR_VECS)
        if src is None:
            fill_device(ctx, p, 0, rows, vp)
        else:
            if not host_rows:
                host_rows.append(ctx.download(src, np.empty((a.n, stride), np.float32)))
            ctx.upload(vp, np.ascontiguousarray(host_rows[0][keep]))
        ix.refresh_norms()
        if not a.plain:
            ix.sbq_train()
            ix.sbq_quantize_corpus()
        ctx.sync()
        t0 = time.perf_counter()
        ix.build_graph(search_list_size=a.build_list, max_alpha=1.2)
        ctx.sync()
        return ix, time.perf_counter() - t0

    ix, t_build = build(a.n)
    ctx.upload(ix.array(_lib.ARR_TIDS)[0], tids)
    say(f"vs_build_graph over all {a.n} rows: {t_build:.2f} s")
    nbr_ptr, nbr_stride = ix.array(_lib.ARR_NBRS)
    graph0 = np.empty((a.n, nbr_stride), np.uint32)
    ctx.download(nbr_ptr, graph0)
    dq = ctx.alloc(a.nq * a.dim * 4)
    fill_device(ctx, p, 10 ** 9, a.nq, dq)
    q = ctx.download(dq, np.empty((a.nq, a.dim), np.float32))

    def searches(index, gt):
        index.search_batch(q[:256], search_list_size=100, rescore=50, k=10)  # warm-up
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            gi, _, _, st = index.search_batch(q, search_list_size=100, rescore=50, k=10)
            ts.append(time.perf_counter() - t0)
        rec = float(np.mean([len(set(x) & set(y)) / 10 for x, y in zip(gi.tolist(), gt.tolist())]))
        return dict(qps=round(a.nq / float(np.median(ts)), 1), recall10=round(rec, 4),
                    d_per_scan=round(st[work_key] / a.nq, 1))

    res = []
    for frac in [float(x) for x in a.fractions.split(",")]:
        # the graph as built, every row live again
        ctx.upload(nbr_ptr, graph0)
        ctx.upload(ix.array(_lib.ARR_TIDS)[0], tids)
        out = PagesOut(ix, search_list_size=a.build_list, plain=a.plain)
        base = out.baseline()
        n_blocks = out.n_blocks
        out.close()
        dead = np.flatnonzero(np.random.default_rng(12).random(a.n) < frac)
        dead = dead[dead != ix.desc.default_start]
        alive = np.setdiff1d(np.arange(a.n), dead)
        st_bd = ix.bulk_delete(tids[dead])
        # (e) first: its brute force over the live rows alone is the ground truth of every recall below
        live_ix, t_rebuild = build(alive.size, src=ix.array(_lib.ARR_VECS)[0], keep=alive)
        gt_local = live_ix.bruteforce_topk(dq, a.nq, 10)[0]
        rebuilt = searches(live_ix, gt_local)
        live_ix.close()
        gt = alive[gt_local]
        before = searches(ix, gt)
        ctx.profile_enable(True)
        ix.consolidate_kernel_ms(reset=True)
        t0 = time.perf_counter()
        st = ix.consolidate_deletes(plain=a.plain)
        t_call = time.perf_counter() - t0
        ms = ix.consolidate_kernel_ms(reset=True)
        ctx.profile_enable(False)
        after = searches(ix, gt)
        out = PagesOut(ix, search_list_size=a.build_list, plain=a.plain)
        blocks, nb_now, nbase = out.delta(base)
        nbase.close()
        base.close()
        out.close()
        say(f"--- {frac:.0%} deleted ({dead.size} rows; bulk_delete {st_bd})")
        say(f"(a) before the pass: {before}")
        rows_per_s = st["rows_rewritten"] / (ms["rows"] * 1e-3) if ms["rows"] > 0 else 0.0
        say(f"(b) vs_index_consolidate_deletes{'_plain' if a.plain else ''}: {t_call * 1e3:.1f} ms wall (repair pass included); kernels: "
            f"flag pass {ms['flag_pass']:.3f} ms, k_consolidate_rows {ms['rows']:.3f} ms = {rows_per_s:.0f} rows/s; {st}")
        say(f"(c) after the pass:  {after}; {work_key} per scan {after['d_per_scan'] / before['d_per_scan'] - 1:+.1%}")
        say(f"(d) vs_pages_out_delta against the baseline from before the delete: {blocks.size} dirty blocks of {n_blocks}")
        say(f"(e) vs_build_graph over the {alive.size} live rows alone: {t_rebuild:.2f} s = {t_rebuild / t_call:.1f} x the call; its searches: {rebuilt}")
        res.append(dict(frac=frac, dead=int(dead.size), call_ms=round(t_call * 1e3, 1), kernel_ms=ms, rows_per_s=round(rows_per_s), stats=st, before=before, after=after,
                        rebuilt=rebuilt, rebuild_s=round(t_rebuild, 2), dirty_blocks=int(blocks.size), blocks=int(n_blocks)))
    say(json.dumps(dict(plain=a.plain, n=a.n, dim=a.dim, R=a.R, build_s=round(t_build, 2), legs=res)))
    ctx.free(dq)
    ix.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
