#!/usr/bin/env python3
"""What streaming rows out of a `plain` storage index through a scan pool costs with and without the resumable form of k_search_plain
(DESIGN.md section 7m).  Nothing here asserts a speed.

Index: n x dim (default 1M x 768), R = 50, L2.  The graph is the SBQ device build (vs_build_graph on 2-bit codes) of the same vectors,
downloaded and uploaded as a plain index, as scripts/bench_plain_search.py does (--graph-cache keeps the downloaded arrays in an .npz
so that a second process — another library — starts from the same graph without building it again).  Operating points: pools of
--pools slots (default 64 and 512), every slot streaming --rows rows (default 1 000) in chunks of --chunk (default 16), all slots named
in every fetch, search_list_size 100 and 30.  Legs run in one process in the order of --legs (values of VS_POOL_PLAIN_FAST; default
1,0,1,0: each setting twice, so the spread between repeats of one leg is on the page).  Per leg: wall time of the fetches of one
stream-out, then a second stream-out under vs_profile for the HIP-event milliseconds of kind 1 (the search launches of the rounds),
the pool's rounds and launches, which kernel it ran, whether the rows (ids, distance bits) equal the first leg's, and their CRC-32 (to
compare the rows of two processes).

The script uses only calls an older library has too when told to (VS_LIB_PATH names it, VS_LIB_TOLERANT=1 lets it load; --legs 0,0
then: the option is unknown to it and every leg is its general kernel):

    python scripts/bench_plain_pool.py --out profiles/r17/plain_pool_1m.txt
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--R", type=int, default=50)
    ap.add_argument("--pools", default="64,512")
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--rows-cap", type=int, default=1024)
    ap.add_argument("--lists", default="100,30")
    ap.add_argument("--legs", default="1,0,1,0")
    ap.add_argument("--build-list", type=int, default=100)
    ap.add_argument("--graph-cache", default=None)
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
    n, dim, R = a.n, a.dim, a.R
    p = DatagenParams(seed=1, dim=dim, latent_dim=32, n_clusters=1024)
    say(f"# plain pool bench: n={n} dim={dim} R={R} rows={a.rows} chunk={a.chunk} rows_cap={a.rows_cap} on {ctx.device_name()}; "
        f"library: {'another build, named by VS_LIB_PATH' if os.environ.get('VS_LIB_PATH') else os.path.relpath(_lib.LIB_PATH, ROOT)}")

    t0 = time.perf_counter()
    if a.graph_cache and os.path.exists(a.graph_cache):
        z = np.load(a.graph_cache)
        nbrs, vecs, start = z["nbrs"], z["vecs"], int(z["start"])
        say(f"graph: read from the cache of an earlier process, {time.perf_counter() - t0:.1f} s")
    else:
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
        say(f"graph: SBQ device build (2-bit codes, build L={a.build_list}) of the same vectors, {time.perf_counter() - t0:.1f} s with the download")
        if a.graph_cache:
            np.savez(a.graph_cache, nbrs=nbrs, vecs=vecs, start=np.int64(start))
    tids = ((np.arange(n, dtype=np.uint64) + 11) << np.uint64(16)) | np.uint64(1)

    pools = [int(x) for x in a.pools.split(",")]
    nq = max(pools)
    d_q = ctx.alloc(nq * dim * 4)
    fill_device(ctx, p, 10 ** 9, nq, d_q)
    q = ctx.download(d_q, np.empty((nq, dim), np.float32))
    ctx.free(d_q)

    ix = P.DiskAnnIndex.upload(ctx, codes=None, nbrs=nbrs, heap_tids=tids, vecs=vecs, mean=None, m2=None, count=0, bits=None, dim_index=dim,
                               num_neighbors=R, distance_type=P.VS_L2, default_start=start, storage_type=_lib.VS_STORAGE_PLAIN)

    def stream_out(pool, G, keep):
        """every slot pulls a.rows rows in chunks of a.chunk, all slots in every fetch; -> seconds spent in the fetches"""
        for i in range(G):
            pool.rescan(i, q[i])
        ctx.sync()
        slots = list(range(G))
        got_ids, got_bits = [], []
        handed, dt = 0, 0.0
        while handed < a.rows:
            kk = min(a.chunk, a.rows - handed)
            t0 = time.perf_counter()
            rows, ids, _, dist = pool.fetch(slots, kk)
            dt += time.perf_counter() - t0
            if not (rows == kk).all():
                raise RuntimeError(f"a slot handed out {int(rows.min())} of {kk} rows")
            if keep:
                got_ids.append(ids.copy())
                got_bits.append(dist.view(np.uint32).copy())
            handed += kk
        return dt, (np.concatenate(got_ids, 1), np.concatenate(got_bits, 1)) if keep else None

    for G in pools:
        for L in [int(x) for x in a.lists.split(",")]:
            first = None
            for leg, val in enumerate(a.legs.split(",")):
                set_option("VS_POOL_PLAIN_FAST", val)
                pool = P.ScanPool(ix, G, search_list_size=L, rescore=0, kmax=a.chunk, rows_cap=a.rows_cap)
                try:
                    info = pool.info()
                except AttributeError:  # (a library from before vs_scanpool_info)
                    info = {"kernel": None, "lds_bytes": None, "heap_lds": None, "dedup_slots": None}
                dt, got = stream_out(pool, G, True)
                w1 = pool.work()
                ctx.profile_enable(True)
                ctx.profile_read(reset=True)
                dt_prof, _ = stream_out(pool, G, False)
                pool.close()  # (waits for the round the last fetch may have launched ahead on the pool's own stream: its events are read below)
                ctx.sync()
                prof = ctx.profile_read(reset=True)
                ctx.profile_enable(False)
                ms = {str(kind): round(float(v[0]), 3) for kind, v in prof.items()} if isinstance(prof, dict) else {}
                k1 = next((v for key, v in ms.items() if key in ("1", "search")), 0.0)
                if first is None:
                    first, same = got, True
                else:
                    same = bool((got[0] == first[0]).all() and (got[1] == first[1]).all())
                r = dict(slots=G, L=L, leg=leg, pool_plain_fast=val, kernel=info["kernel"], wall_ms=round(dt * 1e3, 2),
                         rows_per_s=round(G * a.rows / dt, 1), search_kernel_ms=round(k1, 3), wall_ms_profiled=round(dt_prof * 1e3, 2),
                         rounds=w1["rounds"], launches=w1["launches"], lds_bytes=info["lds_bytes"], heap_lds=info["heap_lds"],
                         dedup_slots=info["dedup_slots"], rows_identical_to_leg0=same,
                         rows_crc32=zlib.crc32(got[1].tobytes(), zlib.crc32(got[0].tobytes())), profile=ms)
                say(json.dumps(r))
            set_option("VS_POOL_PLAIN_FAST", None)
    ix.close()
    ctx.close()


if __name__ == "__main__":
    main()
