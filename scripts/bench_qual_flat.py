#!/usr/bin/env python3
"""The qualified flat scan (vs_search_batch_qual_flat_dev): what `ORDER BY embedding <=> $1 LIMIT k` under a WHERE clause of middling
selectivity costs when the qualifier's rows are ranked by the Hamming distance of their SBQ codes and the best `rescore` rescored
exactly — next to the exact call (vs_search_batch_qual_exact_dev, which is also the true answer recall is counted against) and the
post-filter (vs_search_batch_dev_qual at max_pops = VS_QUAL_MAX_POPS) in the same session on the same scans.  One process, one box, an
SBQ index over generated vectors built on the device.

  per (density, qualifiers, rescore): wall time (call to synchronised outputs) and us per scan, kernel ms by profile span (scan = the
  row lists, search = k_qflat_ham, rerank_order = k_qflat_pick, rerank, resort = k_qflat_final), code_reads x code row bytes over the search
  span as "code bytes applied" (rows shared by tiles come from cache: not an HBM rate), recall@k against the exact call's rows
  before any time of a configuration: the rows, distance bits and counts of --check scans against the oracle (hamming_scan_topk over
  the downloaded codes of the qualifier's rows for S, bruteforce over the rows of S)

Medians of --reps warm repetitions with min .. max.  No number is fixed in advance.

    python scripts/bench_qual_flat.py --out profiles/r25/qual_flat_4m.txt
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
    ap.add_argument("--post-scans", type=int, default=1024)
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--post-rescore", type=int, default=50)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--densities", default="0.3,0.1,0.05,0.01,0.001")
    ap.add_argument("--quals", default="1,8")
    ap.add_argument("--rescores", default="50,200,575")
    ap.add_argument("--check", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
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

    nq, k, dim, n = a.scans, a.k, a.dim, a.rows
    ctx = P.Context(0)
    gp = DatagenParams(seed=3, dim=dim, latent_dim=min(32, dim))
    say(f"bench_qual_flat on {ctx.device_name()}: rows {n}, dim {dim}, scans {nq}, k {k}, reps {a.reps}")
    dq = ctx.alloc(nq * dim * 4)
    d_ids, d_tids, d_dist = ctx.alloc(nq * k * 4), ctx.alloc(nq * k * 8), ctx.alloc(nq * k * 4)
    d_rows, d_pops, d_state, d_slots = (ctx.alloc(nq * 4) for _ in range(4))
    t0 = time.perf_counter()
    ix = P.DiskAnnIndex.alloc(ctx, n=n, dim_full=dim, num_neighbors=a.R, distance_type=P.VS_L2)
    fill_device(ctx, gp, 0, n, ix.array(_lib.ARR_VECS)[0])
    ix.refresh_norms()
    ix.sbq_train()
    ix.sbq_quantize_corpus()
    ix.build_graph(search_list_size=a.build_L)
    ctx.sync()
    fill_device(ctx, gp, n, nq, dq)  # queries: rows of the same generator past the corpus
    say(f"index: {n} nodes, dim {dim}, graph built, on the device in {time.perf_counter() - t0:.1f} s")
    words = ix.desc.words
    codes = ix.download(codes=True, nbrs=False, tids=False)["codes"][:, :words]
    hq = ctx.download(dq, np.empty((a.check, dim), np.float32))
    hqc = ix.prepare_queries(hq)[1][:, :words]
    out = {"rows": n, "dim": dim, "scans": nq, "k": k, "configs": {}}

    def flat(rescore):
        return ix.search_batch_qual_flat_dev(dq, nq, k, rescore, d_slots, d_ids, d_rows, d_out_tids=d_tids, d_out_dist=d_dist)

    def exact():
        return ix.search_batch_qual_exact_dev(dq, nq, k, d_slots, d_ids, d_rows, d_out_tids=d_tids, d_out_dist=d_dist)

    def rows_back():
        return (ctx.download(d_ids, np.empty((nq, k), np.uint32)), ctx.download(d_dist, np.empty((nq, k), np.float32)).view(np.uint32),
                ctx.download(d_rows, np.empty(nq, np.uint32)))

    def timed(fn):
        fn()
        ctx.profile_enable(True)
        wall, spans, st = [], [], None
        for _ in range(a.reps):
            ctx.profile_read(reset=True)
            t = time.perf_counter()
            st = fn()
            ctx.sync()
            wall.append((time.perf_counter() - t) * 1e3)
            spans.append({name: v[0] for name, v in ctx.profile_read(reset=True).items() if v[1]})
        ctx.profile_enable(False)
        return wall, {name: float(np.median([s.get(name, 0.0) for s in spans])) for name in spans[0]}, st

    def check_against_oracle(slots, quals, rescore, got):
        """the first --check scans: S from the oracle's Hamming scan over the qualifier's rows, the rows from its bruteforce over S"""
        for s in range(a.check):
            live = np.where(quals[int(slots[s])], np.uint64(1 << 16 | 1), np.uint64(0))
            cand = O.hamming_scan_topk(codes, hqc[s:s + 1], rescore, heap_tids=live)[0][0]
            cand = np.sort(cand[cand != INV])
            m = max(cand.size, 1)
            vecs = np.concatenate([ix.download(codes=False, nbrs=False, tids=False, vecs=True, row_begin=int(r), row_count=1)["vecs"] for r in cand]) \
                if cand.size else np.zeros((1, dim), np.float32)
            tids = ((np.arange(m, dtype=np.uint64) + 1) << np.uint64(16)) | np.uint64(1 if cand.size else 0)
            o = O.OracleIndex(codes=np.zeros((m, (dim + 63) // 64), np.uint64), nbrs=np.full((m, 4), INV, np.uint32), heap_tids=tids, vecs=vecs,
                              mean=np.zeros(dim, np.float32), m2=np.zeros(dim, np.float32), count=1, bits=1, dim_index=dim, num_neighbors=4,
                              distance_type=O.L2, default_start=0)
            oi, od = o.bruteforce(hq[s:s + 1], k=k)
            want = np.where(oi[0] != INV, cand[np.minimum(oi[0], m - 1)] if cand.size else INV, INV)
            assert (got[0][s] == want).all() and (got[1][s] == od.view(np.uint32)[0]).all() and got[2][s] == (oi[0] != INV).sum(), \
                f"scan {s} differs from the oracle"

    rng = np.random.default_rng(7)
    npost = min(a.post_scans, nq)
    for dens in (float(x) for x in a.densities.split(",")):
        for nqual in (int(x) for x in a.quals.split(",")):
            quals = {s: rng.random(n) < dens for s in range(1, nqual + 1)}
            for s, b in quals.items():
                ix.qual_put(s, b)
            slots = (np.arange(nq, dtype=np.uint32) % nqual) + 1
            ctx.upload(d_slots, slots)
            name = f"density {dens}, {nqual} qualifier(s)"
            ex_wall, ex_spans, ex_st = timed(exact)
            truth = rows_back()
            say(f"{name}: exact wall {spread(ex_wall)} ms = {np.median(ex_wall) * 1e3 / nq:.2f} us per scan; rows_listed {ex_st['rows_listed']}")
            cfg = out["configs"][f"{dens}/{nqual}"] = dict(exact_wall_ms=float(np.median(ex_wall)), exact_us_per_scan=float(np.median(ex_wall)) * 1e3 / nq)
            for rescore in (int(x) for x in a.rescores.split(",")):
                flat(rescore)
                got = rows_back()
                check_against_oracle(slots, quals, rescore, got)
                hits = sum(np.isin(g[g != INV], t[t != INV]).sum() for g, t in zip(got[0], truth[0]))
                recall = hits / max(int(truth[2].sum()), 1)
                wall, spans, st = timed(lambda: flat(rescore))
                applied = st["code_reads"] * words * 8 / (spans.get("search", 0.0) * 1e-3) / 1e12 if spans.get("search") else 0.0
                say(f"{name}, rescore {rescore}: flat wall {spread(wall)} ms = {np.median(wall) * 1e3 / nq:.2f} us per scan; kernel ms "
                    + ", ".join(f"{s} {v:.3f}" for s, v in spans.items())
                    + f"; tile {st['tile_queries']}, tiles {st['tiles']}, slices {st['slices']}, chunks {st['chunks']}, code_reads {st['code_reads']} = "
                    f"{applied:.2f} TB/s of code bytes applied, reranked {st['reranked']}; recall@{k} {recall:.4f}; {a.check} scans equal to the oracle")
                cfg[f"rescore{rescore}"] = dict(wall_ms=float(np.median(wall)), us_per_scan=float(np.median(wall)) * 1e3 / nq, spans=spans,
                                                code_tb_s=applied, recall=float(recall), **st)
            if nqual != 1:
                continue

            def post():  # the post-filter over the first npost of the same scans
                ix.search_batch_dev_qual(dq, npost, a.L, a.post_rescore, k, d_slots, _lib.QUAL_MAX_POPS, d_ids, d_rows, d_pops, d_state,
                                         d_out_tids=d_tids, d_out_dist=d_dist)
                return ix.search_batch_dev_qual_finish()[1]
            try:
                post()
            except P.VsError as e:  # (the post-filter has limits of its own: the refusal is the finding)
                say(f"{name}: post-filter over {npost} scans at max_pops {_lib.QUAL_MAX_POPS}: refused: {e}")
                cfg["post_refused"] = str(e)
                continue
            pw = []
            for _ in range(max(a.reps // 2, 2)):
                t = time.perf_counter()
                qst = post()
                ctx.sync()
                pw.append((time.perf_counter() - t) * 1e3)
            say(f"{name}: post-filter over {npost} scans at L {a.L}, rescore {a.post_rescore}, max_pops {_lib.QUAL_MAX_POPS}: wall {spread(pw)} ms = "
                f"{np.median(pw) * 1e3 / npost:.2f} us per scan; rounds {qst['rounds']}, complete / ended / cut {qst['complete']} / {qst['ended']} / "
                f"{qst['cut']}")
            cfg.update(post_wall_ms=float(np.median(pw)), post_scans=npost, post_us_per_scan=float(np.median(pw)) * 1e3 / npost)
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
