#!/usr/bin/env python3
"""The exact qualified top-k (vs_search_batch_qual_exact_dev): what `ORDER BY embedding <=> $1 LIMIT k` under a SELECTIVE WHERE clause
costs when the plan is "fetch the qualifying rows, sort by exact distance" on the device, next to the post-filter
(vs_search_batch_dev_qual at max_pops = VS_QUAL_MAX_POPS) over the same scans, and next to vs_bruteforce_topk for slot 0.  One process,
one box, an SBQ index over generated vectors built on the device.

  slot 0      --bf-rows x dim, nq = 64 and 1024: the new call with every scan on slot 0 against vs_bruteforce_topk on the same inputs
              (ids and distance bits must be equal before a time is reported)
  throughput  --rows x dim, --scans scans over 1, 8 and 64 distinct qualifiers of each density: wall time (call to synchronised
              outputs), kernel time (HIP events of every kernel of the call), row_reads x row bytes / kernel time against --roofline
  tile        one configuration under VS_QUAL_EXACT_TQ = 4, 8, 16
  crossover   the first --post-scans of the same scans through the post-filter: wall time and the scans it left CUT / ENDED
  before any time of a configuration: the rows, distance bits and counts of --check scans against the oracle's bruteforce over the
  qualifier's rows (downloaded, renumbered in ascending node order)

Medians of --reps warm repetitions with min .. max.  No number is fixed in advance.

    python scripts/bench_qual_exact.py --out profiles/r24/qual_exact_4m.txt
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
    ap.add_argument("--bf-rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--R", type=int, default=50)
    ap.add_argument("--build-L", type=int, default=64)
    ap.add_argument("--scans", type=int, default=8192)
    ap.add_argument("--post-scans", type=int, default=1024)
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--rescore", type=int, default=50)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--densities", default="0.05,0.01,0.001,0.0001")
    ap.add_argument("--quals", default="1,8,64")
    ap.add_argument("--check", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--roofline", type=float, default=8.0, help="TB/s")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pgvectorscale_amd as P
    from oracle import oracle_py as O
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.datagen import DatagenParams, fill_device
    O.build()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def spread(v):
        return f"{np.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"

    nq, k, dim = a.scans, a.k, a.dim
    ctx = P.Context(0)
    gp = DatagenParams(seed=3, dim=dim, latent_dim=min(32, dim))
    say(f"bench_qual_exact on {ctx.device_name()}: rows {a.rows}, dim {dim}, scans {nq}, k {k}, reps {a.reps}, roofline {a.roofline} TB/s")
    dq = ctx.alloc(nq * dim * 4)
    d_ids, d_tids, d_dist = ctx.alloc(nq * k * 4), ctx.alloc(nq * k * 8), ctx.alloc(nq * k * 4)
    d_rows, d_pops, d_state, d_slots = (ctx.alloc(nq * 4) for _ in range(4))
    out = {"rows": a.rows, "dim": dim, "scans": nq, "k": k, "slot0": {}, "throughput": {}, "tile": {}, "crossover": {}}

    def fresh_index(n, graph):
        t0 = time.perf_counter()
        ix = P.DiskAnnIndex.alloc(ctx, n=n, dim_full=dim, num_neighbors=a.R, distance_type=P.VS_L2)
        fill_device(ctx, gp, 0, n, ix.array(_lib.ARR_VECS)[0])
        ix.refresh_norms()
        ix.sbq_train()
        ix.sbq_quantize_corpus()
        if graph:
            ix.build_graph(search_list_size=a.build_L)
        ctx.sync()
        fill_device(ctx, gp, n, nq, dq)  # queries: rows of the same generator past the corpus
        say(f"index: {n} nodes, dim {dim}, {'graph built' if graph else 'no graph'}, on the device in {time.perf_counter() - t0:.1f} s")
        return ix

    def exact(ix, m):
        return ix.search_batch_qual_exact_dev(dq, m, k, d_slots, d_ids, d_rows, d_out_tids=d_tids, d_out_dist=d_dist)

    def rows_back(m):
        return (ctx.download(d_ids, np.empty((m, k), np.uint32)), ctx.download(d_dist, np.empty((m, k), np.float32)).view(np.uint32),
                ctx.download(d_rows, np.empty(m, np.uint32)))

    def timed(fn):
        fn()
        ctx.profile_enable(True)
        wall, kern, st = [], [], None
        for _ in range(a.reps):
            ctx.profile_read(reset=True)
            t = time.perf_counter()
            st = fn()
            ctx.sync()
            wall.append((time.perf_counter() - t) * 1e3)
            kern.append(sum(v[0] for v in ctx.profile_read(reset=True).values()))
        ctx.profile_enable(False)
        return wall, kern, st

    def rate(st, kern):
        return st["row_reads"] * dim * 4 / (np.median(kern) * 1e-3) / 1e12

    def check_against_oracle(ix, slots, quals, got):
        """the first --check scans: the oracle's bruteforce over the scan's qualifying rows, renumbered in ascending node order"""
        hq = ctx.download(dq, np.empty((a.check, dim), np.float32))
        for s in range(a.check):
            rows = np.flatnonzero(quals[int(slots[s])])
            vecs = np.concatenate([ix.download(codes=False, nbrs=False, tids=False, vecs=True, row_begin=int(r), row_count=1)["vecs"] for r in rows]) \
                if rows.size else np.zeros((1, dim), np.float32)
            m = max(rows.size, 1)
            tids = ((np.arange(m, dtype=np.uint64) + 1) << np.uint64(16)) | np.uint64(1 if rows.size else 0)
            o = O.OracleIndex(codes=np.zeros((m, (dim + 63) // 64), np.uint64), nbrs=np.full((m, 4), INV, np.uint32), heap_tids=tids, vecs=vecs,
                              mean=np.zeros(dim, np.float32), m2=np.zeros(dim, np.float32), count=1, bits=1, dim_index=dim, num_neighbors=4,
                              distance_type=O.L2, default_start=0)
            oi, od = o.bruteforce(hq[s:s + 1], k=k)
            want = np.where(oi[0] != INV, rows[np.minimum(oi[0], m - 1)] if rows.size else INV, INV)
            assert (got[0][s] == want).all() and (got[1][s] == od.view(np.uint32)[0]).all() and got[2][s] == (oi[0] != INV).sum(), \
                f"scan {s} differs from the oracle"

    # ---- slot 0 against vs_bruteforce_topk --------------------------------------------------------------------------------------
    ix = fresh_index(a.bf_rows, graph=False)
    ctx.upload(d_slots, np.zeros(nq, np.uint32))
    for m in (min(64, nq), min(1024, nq)):
        w_new, k_new, st = timed(lambda: exact(ix, m))
        got = rows_back(m)
        bi, bd = ix.bruteforce_topk(dq, m, k)
        assert (got[0] == bi).all() and (got[1] == bd.view(np.uint32)).all(), "slot 0 differs from vs_bruteforce_topk"
        w_bf, k_bf, _ = timed(lambda: ix.bruteforce_topk(dq, m, k))
        say(f"slot 0, {a.bf_rows} rows, nq {m}: exact wall {spread(w_new)} ms, kernels {spread(k_new)} ms, {rate(st, k_new):.2f} TB/s of rows "
            f"(tile {st['tile_queries']}, tiles {st['tiles']}, slices {st['slices']}); vs_bruteforce_topk wall {spread(w_bf)} ms, kernels "
            f"{spread(k_bf)} ms (the rerank span only); rows and bits equal")
        out["slot0"][str(m)] = dict(exact_wall_ms=float(np.median(w_new)), exact_kernel_ms=float(np.median(k_new)), bf_wall_ms=float(np.median(w_bf)),
                                    tb_s=rate(st, k_new), **st)
    for tq in (4, 8, 16):
        P.set_option("VS_QUAL_EXACT_TQ", tq)
        w_new, k_new, st = timed(lambda: exact(ix, min(1024, nq)))
        P.set_option("VS_QUAL_EXACT_TQ", None)
        say(f"slot 0, nq {min(1024, nq)}, tile {st['tile_queries']}: wall {spread(w_new)} ms, kernels {spread(k_new)} ms, {rate(st, k_new):.2f} TB/s")
        out["tile"][f"slot0_tq{tq}"] = dict(wall_ms=float(np.median(w_new)), kernel_ms=float(np.median(k_new)), tb_s=rate(st, k_new))
    ix.close()

    # ---- throughput and crossover -------------------------------------------------------------------------------------------------
    n = a.rows
    ix = fresh_index(n, graph=True)
    rng = np.random.default_rng(7)
    npost = min(a.post_scans, nq)
    for dens in (float(x) for x in a.densities.split(",")):
        for nqual in (int(x) for x in a.quals.split(",")):
            quals = {s: rng.random(n) < dens for s in range(1, nqual + 1)}
            for s, b in quals.items():
                ix.qual_put(s, b)
            slots = (np.arange(nq, dtype=np.uint32) % nqual) + 1
            ctx.upload(d_slots, slots)
            exact(ix, nq)
            check_against_oracle(ix, slots, quals, rows_back(nq))
            wall, kern, st = timed(lambda: exact(ix, nq))
            name = f"density {dens}, {nqual} qualifier(s)"
            say(f"{name}: exact wall {spread(wall)} ms = {np.median(wall) * 1e3 / nq:.2f} us per scan, kernels {spread(kern)} ms; rows_listed "
                f"{st['rows_listed']}, tiles {st['tiles']}, slices {st['slices']}, row_reads {st['row_reads']} = {rate(st, kern):.2f} TB/s of rows "
                f"applied ({100 * rate(st, kern) / a.roofline:.0f} % of {a.roofline} if every one of them came from HBM; shared lists do not); {a.check} scans equal to the oracle")
            out["throughput"][f"{dens}/{nqual}"] = dict(wall_ms=float(np.median(wall)), kernel_ms=float(np.median(kern)), tb_s=rate(st, kern), **st)
            if dens == 0.001 and nqual == 8:
                for tq in (4, 8, 16):
                    P.set_option("VS_QUAL_EXACT_TQ", tq)
                    w2, k2, s2 = timed(lambda: exact(ix, nq))
                    P.set_option("VS_QUAL_EXACT_TQ", None)
                    say(f"{name}, tile {s2['tile_queries']}: wall {spread(w2)} ms, kernels {spread(k2)} ms, {rate(s2, k2):.2f} TB/s")
                    out["tile"][f"{dens}/{nqual}_tq{tq}"] = dict(wall_ms=float(np.median(w2)), kernel_ms=float(np.median(k2)), tb_s=rate(s2, k2))
            if nqual == 1:  # the post-filter over the first npost of the same scans
                def post():
                    ix.search_batch_dev_qual(dq, npost, a.L, a.rescore, k, d_slots, _lib.QUAL_MAX_POPS, d_ids, d_rows, d_pops, d_state,
                                             d_out_tids=d_tids, d_out_dist=d_dist)
                    return ix.search_batch_dev_qual_finish()[1]
                try:
                    post()
                except P.VsError as e:  # (the post-filter has limits of its own: the refusal is the finding)
                    say(f"{name}: post-filter over {npost} scans at max_pops {_lib.QUAL_MAX_POPS}: refused: {e}")
                    out["crossover"][str(dens)] = dict(post_refused=str(e), exact_us_per_scan=float(np.median(wall)) * 1e3 / nq)
                    continue
                pw = []
                for _ in range(max(a.reps // 2, 2)):
                    t = time.perf_counter()
                    qst = post()
                    ctx.sync()
                    pw.append((time.perf_counter() - t) * 1e3)
                say(f"{name}: post-filter over {npost} scans at max_pops {_lib.QUAL_MAX_POPS}: wall {spread(pw)} ms = "
                    f"{np.median(pw) * 1e3 / npost:.2f} us per scan; rounds {qst['rounds']}, complete / ended / cut {qst['complete']} / "
                    f"{qst['ended']} / {qst['cut']}")
                out["crossover"][str(dens)] = dict(post_wall_ms=float(np.median(pw)), post_scans=npost, exact_us_per_scan=float(np.median(wall)) * 1e3 / nq,
                                                   post_us_per_scan=float(np.median(pw)) * 1e3 / npost, **qst)
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
