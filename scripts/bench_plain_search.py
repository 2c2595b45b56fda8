#!/usr/bin/env python3
"""What searching a `plain` storage index costs with and without k_search_plain.  Nothing here asserts a speed.

Index: n x dim (default 1M x 768), R = 50, L2 and cosine.  The graph is the SBQ device build (vs_build_graph on 2-bit codes) of the
same vectors, downloaded and uploaded as a plain index: parity and speed do not need a plain-built graph.  Operating points: --nq
scans per step (default 65 536), k = 10, search_list_size 100 and 30.  Legs run in one process in the order of --legs (values of
VS_PLAIN_FAST; default 1,0,1,0: each setting twice, so the spread between repeats of one leg is on the page).  Per leg: QPS over
--steps timed steps after --warmup, HIP-event milliseconds of vs_profile kinds 1 (first attempt) and 4 (hand-over) in a further step,
fallback_scans, the persistent grid's size, and the algorithmic bytes (full_distance_comparisons x 4 dim_index + visited_nodes x 4
nbr_stride) over the kernel time as a share of 8 TB/s — to be read beside the 5.5-5.8 TB/s the device reaches on random whole-row
gathers.  Rows (ids and distance bits) of every leg are compared with the first leg's.

The script uses only calls an older library has too (VS_LIB_PATH names it, VS_LIB_TOLERANT=1 lets it load; --legs 0,0 then):

    python scripts/bench_plain_search.py --out profiles/r16/plain_search_1m.txt
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
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--R", type=int, default=50)
    ap.add_argument("--nq", type=int, default=65536)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lists", default="100,30")
    ap.add_argument("--distances", default="l2,cosine")
    ap.add_argument("--legs", default="1,0,1,0")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--build-list", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import pgvectorscale_amd as P
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.datagen import DatagenParams, fill_device
    from pgvectorscale_amd.index import set_option

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def say(s):
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")

    ctx = P.Context(0)
    n, dim, R, nq, k = a.n, a.dim, a.R, a.nq, a.k
    p = DatagenParams(seed=1, dim=dim, latent_dim=32, n_clusters=1024)
    say(f"# plain search bench: n={n} dim={dim} R={R} nq={nq} k={k} on {ctx.device_name()}; library {os.path.basename(_lib.LIB_PATH)}")

    # the graph: SBQ device build of the same vectors
    t0 = time.perf_counter()
    sbq = P.DiskAnnIndex.alloc(ctx, n=n, dim_full=dim, num_neighbors=R, distance_type=P.VS_L2)
    vp = sbq.array(_lib.ARR_VECS)[0]
    fill_device(ctx, p, 0, n, vp)
    sbq.refresh_norms()
    sbq.sbq_train()
    sbq.sbq_quantize_corpus()
    sbq.build_graph(search_list_size=a.build_list, max_alpha=1.2)
    ctx.sync()
    host = sbq.download(codes=False, tids=False, vecs=True)
    nbrs, vecs = host["nbrs"], host["vecs"]
    start = int(sbq.desc.default_start)
    sbq.close()
    tids = ((np.arange(n, dtype=np.uint64) + 11) << np.uint64(16)) | np.uint64(1)
    say(f"graph: SBQ device build (2-bit codes, build L={a.build_list}) of the same vectors, {time.perf_counter() - t0:.1f} s with the download")

    d_q = ctx.alloc(nq * dim * 4)
    fill_device(ctx, p, 10 ** 9, nq, d_q)
    q = ctx.download(d_q, np.empty((nq, dim), np.float32))
    ctx.free(d_q)

    results = []
    for dname in a.distances.split(","):
        dist = {"l2": P.VS_L2, "cosine": P.VS_COSINE, "ip": P.VS_IP}[dname]
        ix = P.DiskAnnIndex.upload(ctx, codes=None, nbrs=nbrs, heap_tids=tids, vecs=vecs, mean=None, m2=None, count=0, bits=None, dim_index=dim,
                                   num_neighbors=R, distance_type=dist, default_start=start, storage_type=_lib.VS_STORAGE_PLAIN)
        nbr_stride = ix.array(_lib.ARR_NBRS)[1]
        for L in [int(x) for x in a.lists.split(",")]:
            first = None
            for leg, val in enumerate(a.legs.split(",")):
                set_option("VS_PLAIN_FAST", val)
                for _ in range(a.warmup):
                    ix.search_batch(q, search_list_size=L, rescore=0, k=k)
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    gi, _, gd, st = ix.search_batch(q, search_list_size=L, rescore=0, k=k)
                ctx.sync()
                dt = (time.perf_counter() - t0) / a.steps
                ctx.profile_enable(True)
                ctx.profile_read(reset=True)
                ix.search_batch(q, search_list_size=L, rescore=0, k=k)
                ctx.sync()
                prof = ctx.profile_read(reset=True)
                ctx.profile_enable(False)
                try:
                    info = ix.last_search_info()
                except AttributeError:  # (a library from before vs_index_last_search_info)
                    info = {"kernel": None, "resident": None, "lds_bytes": None}
                ms = {kind: float(v[0]) for kind, v in prof.items()} if isinstance(prof, dict) else {}
                k1 = next((v for key, v in ms.items() if str(key) in ("1", "search")), 0.0)
                k4 = next((v for key, v in ms.items() if str(key) in ("4", "search_fb", "search_fallback")), 0.0)
                alg = st["full_distance_comparisons"] * 4 * dim + st["visited_nodes"] * 4 * nbr_stride
                kms = k1 + k4
                tbs = alg / (kms * 1e-3) / 1e12 if kms > 0 else 0.0
                if first is None:
                    first, same = (gi.copy(), gd.view(np.uint32).copy()), True
                else:
                    same = bool((gi == first[0]).all() and (gd.view(np.uint32) == first[1]).all())
                r = dict(distance=dname, L=L, leg=leg, plain_fast=val, qps=round(nq / dt, 1), step_ms=round(dt * 1e3, 2), kernel_ms_first=round(k1, 3),
                         kernel_ms_handover=round(k4, 3), fallback_scans=st["fallback_scans"], kernel=info["kernel"], resident=info["resident"],
                         lds_bytes=info["lds_bytes"], algorithmic_GB=round(alg / 1e9, 2), algorithmic_TBps=round(tbs, 3),
                         share_of_8TBps=round(tbs / 8.0, 4), rows_identical_to_leg0=same, visited_per_scan=round(st["visited_nodes"] / nq, 1),
                         distances_per_scan=round(st["full_distance_comparisons"] / nq, 1), profile=ms)
                results.append(r)
                say(json.dumps(r))
            set_option("VS_PLAIN_FAST", None)
        ix.close()
    ctx.close()


if __name__ == "__main__":
    main()
