#!/usr/bin/env python3
"""The latency-mode search kernel (VS_LAT_SCANS, k_search_lat: one SBQ scan per multi-wave workgroup) against the
parent's path — the option off — on small batches of one index: an SBQ index over generated vectors built on the device, one process.

  per (L, rescore) point and chunk size: option off and on in ALTERNATING rounds over the same scans, every shape warmed up first; per
  round the `search` (+ `search_fallback`) profile span per batch and the host time around vs_search_batch (upload, launches, the
  synchronise, rows back) per batch; the rows, tids and distance bits of every batch compared between the two
  reported: median (min .. max) over the rounds, the on / off ratio of both times, and — the run-to-run spread a ratio has to beat —
  the off rounds' own min .. max.  The largest chunk size at which on still wins is what a deployment gives VS_LAT_SCANS.

No number is fixed in advance.

    python scripts/bench_lat_kernel.py --out profiles/r26/lat_kernel_4m.txt
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
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--R", type=int, default=50)
    ap.add_argument("--build-L", type=int, default=64)
    ap.add_argument("--points", default="100/50,3/195", help="L/rescore pairs")
    ap.add_argument("--chunks", default="1,8,64,256")
    ap.add_argument("--scans", type=int, default=2048, help="scans per point and mode, at least")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--waves", type=int, default=0, help="VS_LAT_WAVES (0: the default)")
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
        return f"{np.median(v):.4f} ({min(v):.4f} .. {max(v):.4f})"

    n, dim, k = a.rows, a.dim, a.k
    chunks = [int(c) for c in a.chunks.split(",")]
    nqtot = max(a.scans, max(chunks) * a.rounds)
    ctx = P.Context(0)
    gp = DatagenParams(seed=3, dim=dim, latent_dim=min(32, dim))
    say(f"bench_lat_kernel on {ctx.device_name()}: rows {n}, dim {dim}, k {k}, >= {a.scans} scans per point and mode in {a.rounds} alternating rounds")
    t0 = time.perf_counter()
    ix = P.DiskAnnIndex.alloc(ctx, n=n, dim_full=dim, num_neighbors=a.R, distance_type=P.VS_L2)
    fill_device(ctx, gp, 0, n, ix.array(_lib.ARR_VECS)[0])
    ix.refresh_norms()
    ix.sbq_train()
    ix.sbq_quantize_corpus()
    ix.build_graph(search_list_size=a.build_L)
    ctx.sync()
    dq = ctx.alloc(nqtot * dim * 4)
    fill_device(ctx, gp, n, nqtot, dq)  # queries: rows of the same generator past the corpus
    hq = ctx.download(dq, np.empty((nqtot, dim), np.float32))
    ctx.free(dq)
    say(f"index: {n} nodes, dim {dim}, graph built, on the device in {time.perf_counter() - t0:.1f} s")
    if a.waves:
        P.set_option("VS_LAT_WAVES", a.waves)
    out = {"rows": n, "dim": dim, "k": k, "points": {}}

    def mode(on, chunk):
        P.set_option("VS_LAT_SCANS", chunk if on else None)

    for L, rescore in ((int(x) for x in p.split("/")) for p in a.points.split(",")):
        for chunk in chunks:
            per_round = max((a.scans + chunk * a.rounds - 1) // (chunk * a.rounds), 1)
            batches = [hq[b * chunk:(b + 1) * chunk] for b in range(min(per_round * a.rounds, nqtot // chunk))]
            per_round = len(batches) // a.rounds

            def run(q):
                return ix.search_batch(q, search_list_size=L, rescore=rescore, k=k)
            # warm-up of both shapes, and the rows of every batch under both
            info = None
            for b in batches:
                mode(False, chunk)
                off = run(b)
                mode(True, chunk)
                on = run(b)
                info = ix.last_search_info()
                assert info["kernel"] == _lib.VS_SEARCH_LAT_SBQ, info
                assert all((x.view(np.uint32) == y.view(np.uint32)).all() for x, y in zip(on[:3], off[:3])), "rows differ between on and off"
            ctx.profile_enable(True)
            kern, wall, fb = {False: [], True: []}, {False: [], True: []}, 0
            for r in range(a.rounds):
                for on in (False, True):
                    mode(on, chunk)
                    ctx.profile_read(reset=True)
                    t = time.perf_counter()
                    for b in batches[r * per_round:(r + 1) * per_round]:
                        fb += run(b)[3]["fallback_scans"] * int(on)
                    wall[on].append((time.perf_counter() - t) * 1e3 / per_round)
                    pr = ctx.profile_read(reset=True)
                    kern[on].append((pr["search"][0] + pr["search_fallback"][0]) / per_round)
            ctx.profile_enable(False)
            mode(False, chunk)
            rk, rw = np.median(kern[True]) / np.median(kern[False]), np.median(wall[True]) / np.median(wall[False])
            say(f"L {L} rescore {rescore} chunk {chunk}: {per_round * a.rounds} batches per mode; search span ms per batch off {spread(kern[False])} "
                f"on {spread(kern[True])} ratio {rk:.3f}; host ms per batch off {spread(wall[False])} on {spread(wall[True])} ratio {rw:.3f}; "
                f"rows identical; fallback_scans {fb}; on: {info['reserved'][0]} waves, cache {info['reserved'][1]}, lds {info['lds_bytes']} B, "
                f"heap_lds {info['heap_lds']}, dedup_slots {info['dedup_slots']}")
            out["points"][f"{L}/{rescore}/{chunk}"] = dict(search_off_ms=kern[False], search_on_ms=kern[True], host_off_ms=wall[False], host_on_ms=wall[True],
                                                          search_ratio=float(rk), host_ratio=float(rw), fallback_scans=int(fb), info=info)
    say(json.dumps(out))
    ix.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
