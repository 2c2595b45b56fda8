#!/usr/bin/env python3
"""Following a relation from its changed pages (vs_pages_follow_*) against staging it again (vs_pages_dev_*), in one process.

  1. an index X is built on the device and written out as relation A; index Y is staged from A with the device reader (the
     "standby") and gets a follower; neither Y nor the re-staged indexes carry the vector column (the follower would move
     n_appended rows of it, the re-stage all of them: leaving it out keeps the comparison to the pages);
  2. X takes --rows rows with vs_index_insert (the "primary"); its page writer names the dirty blocks (delta) and hands out
     their bytes (read_blocks) and, for the other leg, the whole new relation;
  3. timed on the host clock (every call ends in a synchronise): vs_pages_follow_stage of the dirty blocks, --reps times (a later
     stage replaces the earlier one), then vs_pages_follow_apply once — a follower's table advances, so the apply cannot be
     repeated on one index; its kernel launch is a first launch;
  4. timed the same way, --reps times: vs_pages_dev_open + _add of the whole new relation + _build, the thing the follower
     replaces;
  5. Y's codes, neighbor rows and heap tids are compared with X's and with a re-staged index's.

Nothing asserts a speed and no ratio is fixed in advance.  The expectation reported against: the time follows the bytes moved.

    python scripts/bench_pages_follow.py --out profiles/r15/s1_pages_follow_4m.txt

--plain is the same experiment on a `plain` pair (vs_pages_follow_open_plain): X is a plain index made with vs_index_alloc and
build_graph and takes --rows rows with vs_index_insert; Y is uploaded from X's relation with IndexPages(plain=True).upload_plain and
follows X's delta / read_blocks, the appended rows handed over as the heap's rows; the leg it is compared with is what a plain
index has without a follower: IndexPages(plain=True) over the whole new relation (one host pass) + upload_plain.  Both legs carry
the vector column — a plain index is its vector column.  Y's neighbor rows, tids and vector rows are asserted equal to X's and to
the re-uploaded index's.  A plain page is about 85 % vector bytes (1M x 768 is 4 GB of pages), so the default --n is 200 000.

    python scripts/bench_pages_follow.py --plain --out profiles/r15/s2_pages_follow_plain_200k.txt
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
    ap.add_argument("--n", type=int, default=0, help="0 = 4 000 000, with --plain 200 000")
    ap.add_argument("--plain", action="store_true", help="a plain-storage pair (vs_pages_follow_open_plain)")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--bits", type=int, default=0, help="0 = the reference's default for the dimension")
    ap.add_argument("--R", type=int, default=50)
    ap.add_argument("--rows", type=int, default=1000, help="rows the twin takes with vs_index_insert")
    ap.add_argument("--build-list", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    a.n = a.n or (200_000 if a.plain else 4_000_000)
    if a.plain:
        return main_plain(a)

    import pgvectorscale_amd as P
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.datagen import DatagenParams, fill_device, rows_numpy
    from pgvectorscale_amd.pages import DevicePages, PagesOut

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = P.Context(0)
    say(f"# pages follow: n={a.n} dim={a.dim} R={a.R} rows={a.rows} on {ctx.device_name()}")
    t0 = time.perf_counter()
    x = P.DiskAnnIndex.alloc(ctx, n=a.n, dim_full=a.dim, bits=a.bits or None, num_neighbors=a.R, distance_type=P.VS_L2)
    fill_device(ctx, DatagenParams(seed=8, dim=a.dim), 0, a.n, x.array(_lib.ARR_VECS)[0])
    x.refresh_norms()
    x.sbq_train()
    x.sbq_quantize_corpus()
    x.build_graph(search_list_size=a.build_list, max_alpha=1.2)
    x.set_start_nodes(0, {})
    ctx.sync()
    say(f"index X built on the device in {time.perf_counter() - t0:.1f} s: bits={x.desc.bits} words={x.desc.words}")

    def stage(raw, nb):
        """the whole relation through the device reader -> (index, reader, seconds)"""
        t0 = time.perf_counter()
        dp = DevicePages(ctx, nb)
        dp.add(raw)
        ix = dp.build_from_meta(vecs=None)
        return ix, dp, time.perf_counter() - t0

    out = PagesOut(x, search_list_size=a.build_list)
    ps, nb_a = out.page_size, out.n_blocks
    rel_a = out.read()
    base = out.baseline()
    out.close()
    y, dp, t_first = stage(rel_a, nb_a)
    fol = dp.follower(y)
    dp.close()
    del rel_a
    say(f"relation A: {nb_a} blocks = {nb_a * ps / 1e9:.3f} GB; Y staged from it in {t_first * 1e3:.1f} ms (first launches)")

    new = rows_numpy(DatagenParams(seed=8, dim=a.dim), a.n, a.rows)
    new_tids = ((np.arange(a.n, a.n + a.rows, dtype=np.uint64) + 1) << np.uint64(16)) | np.uint64(1)
    t0 = time.perf_counter()
    ist = x.insert(new, new_tids, search_list_size=a.build_list)
    say(f"vs_index_insert of {a.rows} rows into X: {(time.perf_counter() - t0) * 1e3:.1f} ms; {ist}")
    out = PagesOut(x, search_list_size=a.build_list)
    blocks, nb_now, new_base = out.delta(base)
    pages = out.read_blocks(blocks)
    rel_b = out.read()
    out.close()
    moved, whole = int(blocks.size) * ps, nb_now * ps
    say(f"dirty blocks: {blocks.size} of {nb_now} = {moved / 1e6:.2f} MB of {whole / 1e9:.3f} GB ({whole / max(moved, 1):.1f}x fewer bytes)")

    t_stage = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        info = fol.stage(blocks, pages, nb_now)
        t_stage.append(time.perf_counter() - t0)
    assert (fol.new_tids() == new_tids).all()
    t0 = time.perf_counter()
    fol.apply(None)
    t_apply = time.perf_counter() - t0
    say(f"(a) vs_pages_follow_stage: {' '.join(f'{t * 1e3:.2f}' for t in t_stage)} ms; vs_pages_follow_apply (once): {t_apply * 1e3:.2f} ms; {info}")

    t_full, z = [], None
    for _ in range(a.reps):
        if z is not None:
            z.close()
        z, dp, t = stage(rel_b, nb_now)
        dp.close()
        t_full.append(t)
    say(f"(b) vs_pages_dev_open + _add + _build of the whole new relation: {' '.join(f'{t * 1e3:.1f}' for t in t_full)} ms")

    def arrays(ix):
        ix._refresh()
        h = ix.download()
        return h["codes"].tobytes(), h["nbrs"].tobytes(), h["heap_tids"].tobytes()

    ay = arrays(y)
    same = ay == arrays(x) and ay == arrays(z)
    follow = float(np.median(t_stage)) + t_apply
    full = float(np.median(t_full))
    say(f"stage (median) + apply = {follow * 1e3:.2f} ms against {full * 1e3:.1f} ms for the re-stage: {full / follow:.1f}x faster for "
        f"{whole / max(moved, 1):.1f}x fewer bytes; the followed index equals X and the re-staged one: {same}")
    say(json.dumps(dict(n=a.n, dim=a.dim, R=a.R, rows=a.rows, blocks_before=nb_a, blocks_now=nb_now, dirty=int(blocks.size), bytes_moved=moved,
                        bytes_whole=whole, stage_ms=[round(t * 1e3, 2) for t in t_stage], apply_ms=round(t_apply * 1e3, 2),
                        restage_ms=[round(t * 1e3, 1) for t in t_full], info=info, arrays_identical=same)))
    for h in (fol, base, new_base, z, y, x):
        h.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n\n")
    return 0 if same else 1


def main_plain(a):
    import pgvectorscale_amd as P
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.datagen import DatagenParams, fill_device, rows_numpy
    from pgvectorscale_amd.pages import IndexPages, PagesOut

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = P.Context(0)
    say(f"# pages follow, plain storage: n={a.n} dim={a.dim} R={a.R} rows={a.rows} on {ctx.device_name()}")
    t0 = time.perf_counter()
    x = P.DiskAnnIndex.alloc(ctx, n=a.n, dim_full=a.dim, num_neighbors=a.R, distance_type=P.VS_L2, storage_type=_lib.VS_STORAGE_PLAIN)
    assert x.array(_lib.ARR_VECS)[1] == a.dim, "the data generator fills rows of --dim floats: choose a --dim that is the row stride"
    fill_device(ctx, DatagenParams(seed=8, dim=a.dim), 0, a.n, x.array(_lib.ARR_VECS)[0])
    tids = ((np.arange(a.n + a.rows, dtype=np.uint64) + 1) << np.uint64(16)) | np.uint64(1)
    ctx.upload(x.array(_lib.ARR_TIDS)[0], tids[:a.n])
    x.refresh_norms()
    x.build_graph(search_list_size=a.build_list, max_alpha=1.2)
    ctx.sync()
    say(f"plain index X built on the device in {time.perf_counter() - t0:.1f} s")

    def upload(raw, vecs):
        """the whole relation through the host reader + upload_plain -> (index, reader, seconds)"""
        t0 = time.perf_counter()
        rd = IndexPages(plain=True)
        rd.add(raw)
        rd.finish()
        _, d, _ = rd.meta()
        ix = rd.upload_plain(ctx, distance_type=P.VS_L2, default_start=int(d.default_start), vecs=vecs)
        ctx.sync()
        return ix, rd, time.perf_counter() - t0

    out = PagesOut(x, search_list_size=a.build_list, plain=True)
    ps, nb_a = out.page_size, out.n_blocks
    rel_a = out.read()
    base = out.baseline()
    out.close()
    rows_a = x.download(codes=False, nbrs=False, tids=False, vecs=True)["vecs"]
    y, rd, t_first = upload(rel_a, rows_a)
    fol = rd.follower(y)
    rd.close()
    del rel_a
    say(f"relation A: {nb_a} blocks = {nb_a * ps / 1e9:.3f} GB; Y uploaded from it in {t_first * 1e3:.1f} ms (host reader + upload_plain)")

    new = rows_numpy(DatagenParams(seed=8, dim=a.dim), a.n, a.rows)
    t0 = time.perf_counter()
    ist = x.insert(new, tids[a.n:], search_list_size=a.build_list)
    say(f"vs_index_insert of {a.rows} rows into X: {(time.perf_counter() - t0) * 1e3:.1f} ms; {ist}")
    out = PagesOut(x, search_list_size=a.build_list, plain=True)
    blocks, nb_now, new_base = out.delta(base)
    pages = out.read_blocks(blocks)
    rel_b = out.read()
    out.close()
    moved, whole = int(blocks.size) * ps, nb_now * ps
    say(f"dirty blocks: {blocks.size} of {nb_now} = {moved / 1e6:.2f} MB of {whole / 1e9:.3f} GB ({whole / max(moved, 1):.1f}x fewer bytes)")

    t_stage = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        info = fol.stage(blocks, pages, nb_now)
        t_stage.append(time.perf_counter() - t0)
    assert (fol.new_tids() == tids[a.n:]).all()
    t0 = time.perf_counter()
    fol.apply(new)
    t_apply = time.perf_counter() - t0
    say(f"(a) vs_pages_follow_stage: {' '.join(f'{t * 1e3:.2f}' for t in t_stage)} ms; vs_pages_follow_apply (once, {a.rows} rows handed over): "
        f"{t_apply * 1e3:.2f} ms; {info}")

    rows_b = np.concatenate([rows_a, new])
    t_full, z = [], None
    for _ in range(a.reps):
        if z is not None:
            z.close()
        z, rd, t = upload(rel_b, rows_b)
        rd.close()
        t_full.append(t)
    say(f"(b) IndexPages(plain=True) over the whole new relation + upload_plain: {' '.join(f'{t * 1e3:.1f}' for t in t_full)} ms")

    def arrays(ix):
        ix._refresh()
        h = ix.download(codes=False, vecs=True)
        return h["nbrs"].tobytes(), h["heap_tids"].tobytes(), h["vecs"].tobytes()

    ay = arrays(y)
    same = ay == arrays(x) and ay == arrays(z)
    assert same, "the followed index differs from X or from the re-uploaded index"
    follow = float(np.median(t_stage)) + t_apply
    full = float(np.median(t_full))
    say(f"stage (median) + apply = {follow * 1e3:.2f} ms against {full * 1e3:.1f} ms for the re-upload: {full / follow:.1f}x faster for "
        f"{whole / max(moved, 1):.1f}x fewer bytes; the followed index equals X and the re-uploaded one: {same}")
    say(json.dumps(dict(plain=True, n=a.n, dim=a.dim, R=a.R, rows=a.rows, blocks_before=nb_a, blocks_now=nb_now, dirty=int(blocks.size),
                        bytes_moved=moved, bytes_whole=whole, stage_ms=[round(t * 1e3, 2) for t in t_stage], apply_ms=round(t_apply * 1e3, 2),
                        reupload_ms=[round(t * 1e3, 1) for t in t_full], info=info, arrays_identical=same)))
    for h in (fol, base, new_base, z, y, x):
        h.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
