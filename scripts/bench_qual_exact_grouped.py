#!/usr/bin/env python3
"""The exact and the flat qualified top-k under a group rule (vs_search_batch_qual_exact_grouped_dev / _flat_grouped_dev): what "the k
nearest DOCUMENTS of one tenant" costs — a selective qualifier and a per-group cap together — next to the three ways to it without the
calls.  One process, one box, an SBQ index over generated vectors built on the device; a group's rows are neighbours (the rows in the
generator's cluster order, group = place // size: scripts/bench_grouped.py).

  per density (one qualifier) and mean group size, k = --k, per_group 1 (and one point at per_group 3):
  exact     vs_search_batch_qual_exact_dev at k: the ungrouped call, whose kernels this change leaves as they were — the yardstick
  grouped   vs_search_batch_qual_exact_grouped_dev: wall, kernels, and the ratio to `exact`
  flat      vs_search_batch_qual_flat_grouped_dev at --rescore: wall, the scans short of k rows, the share of `grouped`'s rows found
  post      vs_search_batch_dev_grouped over the first --post-scans scans at max_pops --max-pops: wall, complete / ended / CUT
  dedupe    vs_search_batch_qual_exact_dev at k = 64, the cap applied on the host (inside the clock): wall, the scans that come back
            with fewer than k groups although more qualify
  before any time: the rows of `grouped` must equal those of `dedupe` on every scan where `dedupe` is complete

Wall: call to synchronised outputs.  Medians of --reps warm repetitions with min .. max, the variants alternating inside a repetition.
No number is fixed in advance.

    python scripts/bench_qual_exact_grouped.py --out profiles/r28/qual_exact_grouped_4m.txt
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


def dedupe(ids, groups, k, per_group):
    """ids [nq, kk] in (distance, id) order -> the first k rows under the cap [nq, k], and whether that is all the rule can give:
    k rows were found or the kk rows were every qualifying row"""
    valid = ids != INV
    g = groups[np.where(valid, ids, 0)].astype(np.int64)
    order = np.argsort(g, axis=1, kind="stable")
    gs = np.take_along_axis(g, order, 1)
    idx = np.arange(gs.shape[1])[None, :]
    head = np.ones(gs.shape, bool)
    head[:, 1:] = gs[:, 1:] != gs[:, :-1]
    in_cap = idx - np.maximum.accumulate(np.where(head, idx, 0), axis=1) < per_group  # place within the group's run
    keep = np.zeros(gs.shape, bool)
    np.put_along_axis(keep, order, in_cap, 1)
    keep &= valid
    c = keep.cumsum(1)
    keep &= c <= k
    out = np.full((len(ids), k), INV, np.uint32)
    si, ji = np.nonzero(keep)
    out[si, c[si, ji] - 1] = ids[si, ji]
    return out, (c[:, -1] >= k) | ~valid[:, -1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--R", type=int, default=50)
    ap.add_argument("--build-L", type=int, default=64)
    ap.add_argument("--scans", type=int, default=8192)
    ap.add_argument("--post-scans", type=int, default=1024)
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rescore", type=int, default=200)
    ap.add_argument("--max-pops", type=int, default=2048)
    ap.add_argument("--densities", default="0.05,0.01,0.001")
    ap.add_argument("--sizes", default="4,64")
    ap.add_argument("--reps", type=int, default=5)
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
        return f"{np.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"

    n, nq, k, dim, K2 = a.rows, a.scans, a.k, a.dim, 64
    npost = min(a.post_scans, nq)
    ctx = P.Context(0)
    say(f"bench_qual_exact_grouped on {ctx.device_name()}: rows {n}, dim {dim}, scans {nq}, k {k}, flat rescore {a.rescore}, post-filter over "
        f"{npost} scans at max_pops {a.max_pops}, reps {a.reps}")
    t0 = time.perf_counter()
    gp = DatagenParams(seed=3, dim=dim, latent_dim=min(32, dim))
    ix = P.DiskAnnIndex.alloc(ctx, n=n, dim_full=dim, num_neighbors=a.R, distance_type=P.VS_L2)
    fill_device(ctx, gp, 0, n, ix.array(_lib.ARR_VECS)[0])
    ix.refresh_norms()
    ix.sbq_train()
    ix.sbq_quantize_corpus()
    ix.build_graph(search_list_size=a.build_L)
    ctx.sync()
    say(f"index: {n} nodes, dim {dim}, graph built, on the device in {time.perf_counter() - t0:.1f} s")
    dq = ctx.alloc(nq * dim * 4)
    fill_device(ctx, gp, n, nq, dq)  # queries: rows of the same generator past the corpus
    d_ids, d_tids, d_dist = ctx.alloc(nq * K2 * 4), ctx.alloc(nq * K2 * 8), ctx.alloc(nq * K2 * 4)
    d_rows, d_pops, d_state, d_slots = (ctx.alloc(nq * 4) for _ in range(4))
    ctx.upload(d_slots, np.ones(nq, np.uint32))
    cluster = (datagen._hash(gp.seed, np.arange(n, dtype=np.uint64), np.uint64(0)) % np.uint64(gp.n_clusters)).astype(np.int64)
    by_cluster = np.argsort(cluster, kind="stable")
    outs = dict(d_out_tids=d_tids, d_out_dist=d_dist)

    def ids_back(m, kk):
        return ctx.download(d_ids, np.empty((m, kk), np.uint32)), ctx.download(d_rows, np.empty(m, np.uint32))

    def kernels_of(fn):
        ctx.profile_enable(True)
        ctx.profile_read(reset=True)
        fn()
        ctx.sync()
        ms = sum(v[0] for v in ctx.profile_read(reset=True).values())
        ctx.profile_enable(False)
        return ms

    out = {"rows": n, "dim": dim, "scans": nq, "k": k, "rescore": a.rescore, "points": {}}
    rng = np.random.default_rng(7)
    points = [(d, s, 1) for d in (float(x) for x in a.densities.split(",")) for s in (int(x) for x in a.sizes.split(","))]
    points.append((points[len(points) // 2][0], points[-1][1], 3))  # one point at per_group 3: the middle density, the largest groups
    at = (None, None)
    for dens, size, per_group in points:
        if at[0] != dens:
            ix.qual_put(1, rng.random(n) < dens)
        if at[1] != size:
            groups = np.empty(n, np.uint32)
            groups[by_cluster] = (np.arange(n) // size).astype(np.uint32)
            ix.groups_put(groups)
        at = (dens, size)

        def exact():
            return ix.search_batch_qual_exact_dev(dq, nq, k, d_slots, d_ids, d_rows, **outs)

        def grouped():
            return ix.search_batch_qual_exact_grouped_dev(dq, nq, k, per_group, d_slots, d_ids, d_rows, **outs)

        def flat():
            return ix.search_batch_qual_flat_grouped_dev(dq, nq, k, per_group, a.rescore, d_slots, d_ids, d_rows, **outs)

        def wide():
            ix.search_batch_qual_exact_dev(dq, nq, K2, d_slots, d_ids, d_rows, **outs)
            return dedupe(ids_back(nq, K2)[0], groups, k, per_group)

        def post():
            ix.search_batch_dev_grouped(dq, npost, a.L, 50, k, per_group, d_slots, a.max_pops, d_ids, d_rows, d_pops, d_state, **outs)
            return ix.search_batch_dev_grouped_finish()[1]

        st = grouped()
        want, want_rows = ids_back(nq, k)
        host, complete = wide()
        assert (want[complete] == host[complete]).all(), "the grouped call differs from the ungrouped call at k = 64 with the cap on the host"
        flat()
        got, got_rows = ids_back(nq, k)
        found = float(np.mean([np.isin(w[w != INV], g).mean() for w, g in zip(want, got) if (w != INV).any()]))
        legs = {"exact": exact, "grouped": grouped, "flat": flat, "dedupe": wide}
        try:
            post()
            legs["post"] = post
        except P.VsError as e:  # (the post-filter has limits of its own: the refusal is the finding)
            say(f"density {dens}, group size {size}: post-filter refused: {e}")
        wall = {name: [] for name in legs}
        for _ in range(a.reps):  # (alternating: other work shares the host)
            for name, fn in legs.items():
                t = time.perf_counter()
                r = fn()
                ctx.sync()
                wall[name].append((time.perf_counter() - t) * 1e3)
                if name == "post":
                    qst = r
        kern = {name: kernels_of(legs[name]) for name in ("exact", "grouped")}
        ratio = float(np.median(wall["grouped"]) / np.median(wall["exact"]))
        name = f"density {dens}, group size {size}, per_group {per_group}"
        say(f"{name}: exact (ungrouped, k {k}) wall {spread(wall['exact'])} ms, kernels {kern['exact']:.3f} ms; grouped wall "
            f"{spread(wall['grouped'])} ms, kernels {kern['grouped']:.3f} ms = {ratio:.3f} x exact; rows_listed {st['rows_listed']}, tiles "
            f"{st['tiles']}, slices {st['slices']}; scans short of k rows {int((want_rows < k).sum())}")
        say(f"{name}: flat grouped at rescore {a.rescore}: wall {spread(wall['flat'])} ms; scans short of k rows {int((got_rows < k).sum())}; "
            f"{100 * found:.1f} % of the grouped call's rows found")
        say(f"{name}: exact at k = {K2} + host dedupe: wall {spread(wall['dedupe'])} ms; {int((~complete).sum())} of {nq} scans come back with "
            f"fewer than k groups although more rows qualify; the others equal to the grouped call's rows")
        pt = dict(exact_wall_ms=float(np.median(wall["exact"])), grouped_wall_ms=float(np.median(wall["grouped"])), ratio=ratio,
                  exact_kernel_ms=kern["exact"], grouped_kernel_ms=kern["grouped"], flat_wall_ms=float(np.median(wall["flat"])),
                  flat_short=int((got_rows < k).sum()), flat_found=found, dedupe_wall_ms=float(np.median(wall["dedupe"])),
                  dedupe_incomplete=int((~complete).sum()))
        if "post" in legs:
            say(f"{name}: post-filter (vs_search_batch_dev_grouped) over {npost} scans: wall {spread(wall['post'])} ms = "
                f"{np.median(wall['post']) * 1e3 / npost:.2f} us per scan against {np.median(wall['grouped']) * 1e3 / nq:.2f} of grouped; "
                f"complete / ended / cut {qst['complete']} / {qst['ended']} / {qst['cut']} = {100 * qst['cut'] / npost:.1f} % CUT")
            pt.update(post_wall_ms=float(np.median(wall["post"])), post_scans=npost, post_cut=int(qst["cut"]))
        out["points"][f"{dens}/{size}/{per_group}"] = pt
    say(json.dumps(out))
    for p in (dq, d_ids, d_tids, d_dist, d_rows, d_pops, d_state, d_slots):
        ctx.free(p)
    ix.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
