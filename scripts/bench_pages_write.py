#!/usr/bin/env python3
"""How fast a device-resident index leaves as relation pages (vs_pages_out_*), on a device-built index.

  (a) k_pages_encode over the whole relation, composed into one device buffer (vs_pages_out_read_dev): kernel time from the HIP
      events of vs_profile (kind 7), as GB/s of pages written and as a share of the HBM peak on the algorithmic bytes
      (codes + neighbor rows + heap tids [+ label offsets and values] read, pages written; the node_block gathers of the
      labeled case are not counted: they are overhead of the method, not bytes the result needs);
  (b) vs_pages_out_read of the whole relation into a host buffer, end to end (host clock; the call ends in a synchronise);
  (c) vs_dev_download of a device buffer of the same number of bytes into the same host buffer: the copy floor.
(b) and (c) alternate, --reps times each.  The expectation (b) is reported against: (c) + the run-to-run spread of (c) + one chunk's
kernel time of pipeline fill.  Nothing here asserts a speed; the bytes of (b) are compared with the device-composed ones.

    python scripts/bench_pages_write.py --out profiles/r09/s1_pages_write_4m.txt
    python scripts/bench_pages_write.py --dim 1536 --labels 32 --cosine --append --out profiles/r09/s1_pages_write_4m.txt

--delta adds the page-by-page leg on the same index, in the same session as the legs above: baseline -> bulk_delete of 40 000 TIDs
drawn at random -> insert of 4 096 rows -> delta + read_blocks.  It records the digest pass against the full k_pages_encode pass
(HIP events, alternated --reps times), bulk_delete (host clock), delta + read_blocks end to end against vs_pages_out_read of the whole
relation (host clock, alternated), and the number of dirty blocks out of the total.  Two expectations are reported against, each
with the session's own spread as the margin: the digest pass does not take longer than the encode pass; delta + read_blocks beats
the full read by roughly the ratio of blocks moved.

    python scripts/bench_pages_write.py --delta --out profiles/r10/s1_pages_delta_4m.txt
    python scripts/bench_pages_write.py --delta --dim 1536 --labels 32 --cosine --append --out profiles/r10/s1_pages_delta_4m.txt

--open-only times vs_pages_out_open alone on an index whose arrays are allocated but not built (the layout depends on n, W, R and
the label sets only), so that the labeled open pass can be timed at a size whose build would take minutes:

    python scripts/bench_pages_write.py --open-only --n 50000000 --labels 32 --append --out profiles/r09/s1_pages_write_4m.txt

--plain writes a `plain` storage index instead (vs_pages_out_open_plain, k_pages_encode_plain; default 1M x 768, R = 50): legs (a)
and (b) only, as GB/s of pages produced.  The index is not built: its neighbor rows are filled with random node ids, full lists,
because what the writer does with a row does not depend on which nodes it names.  Run it next to the SBQ mode at the same --n in
one session to compare the two page rates:

    python scripts/bench_pages_write.py --n 1000000 --out out/pages_write_1m.txt
    python scripts/bench_pages_write.py --plain --append --out out/pages_write_1m.txt
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s (MI355X)
STAGING_BYTES = 32 << 20  # one buffer of the staging ring of a context made by vs_ctx_create (include/vsgpu.h), which Context(0) is:
#                           vs_pages_out_read encodes and copies that many bytes of node pages per chunk


def timed_open(P, PagesOut, ctx, ix, a, say):
    """vs_pages_out_open on the clock, and for labeled nodes its three parts: the two transfers are timed on their own with the
    calls the open itself uses (vs_dev_download of label_off, vs_dev_upload of node_block + lp_off), the host pass is the rest"""
    t0 = time.perf_counter()
    out = PagesOut(ix, search_list_size=a.build_list)
    t_open = time.perf_counter() - t0
    node_pages = int(out.info.pages_by_type[5])
    msg = f"vs_pages_out_open: {t_open * 1e3:.1f} ms"
    if a.labels:
        n = a.n
        h = np.zeros(6 * n + 4, np.uint8)
        dbuf = ctx.alloc(h.nbytes)
        ctx.upload(dbuf, h)  # warm-up
        t0 = time.perf_counter()
        ctx.download(dbuf, h[:4 * (n + 1)])
        t_down = time.perf_counter() - t0
        t0 = time.perf_counter()
        ctx.upload(dbuf, h[:4 * n])
        ctx.upload(dbuf, h[:2 * n])
        t_up = time.perf_counter() - t0
        ctx.free(dbuf)
        msg += (f" = download of label_off ({4 * (n + 1) / 1e6:.0f} MB) {t_down * 1e3:.1f} ms + upload of node_block and lp_off "
                f"({6 * n / 1e6:.0f} MB) {t_up * 1e3:.1f} ms + the rest {(t_open - t_down - t_up) * 1e3:.1f} ms: the sequential host "
                f"pass over {n} nodes ({(t_open - t_down - t_up) / n * 1e9:.1f} ns per node) and the allocations")
    else:
        msg += " (classic nodes: no pass over the nodes, no per-node arrays)"
    say(f"{msg}; relation = {out.n_blocks} blocks = {out.n_blocks * out.page_size / 1e9:.3f} GB, {node_pages} node pages, "
        f"{a.n / max(node_pages, 1):.2f} nodes per page")
    return out, t_open, node_pages


def delta_leg(P, PagesOut, ctx, ix, out, dbuf, host, a, say):
    """the page-by-page leg (module docstring); closes `out`, leaves the index mutated"""
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.datagen import DatagenParams, rows_numpy
    nb0 = out.n_blocks
    # the digest pass against the full encode pass, alternated
    base = out.baseline()  # warm-up: code object load
    base.close()
    ctx.profile_enable(True)
    ctx.profile_read(reset=True)
    dig_ms, enc_ms = [], []
    for rep in range(a.reps):
        base = out.baseline()
        dig_ms.append(ctx.profile_read(reset=True)["pages_encode"][0])
        out.read_dev(dbuf)
        enc_ms.append(ctx.profile_read(reset=True)["pages_encode"][0])
        if rep < a.reps - 1:
            base.close()
    ctx.profile_enable(False)
    spread = max(max(dig_ms) - min(dig_ms), max(enc_ms) - min(enc_ms))
    say(f"(d) digest pass (k_pages_encode<DIGEST>, {nb0} blocks): {' '.join(f'{x:.3f}' for x in dig_ms)} ms; full encode pass: "
        f"{' '.join(f'{x:.3f}' for x in enc_ms)} ms; expectation median(digest) <= median(encode) + spread ({spread:.3f} ms): "
        f"{'met' if np.median(dig_ms) <= np.median(enc_ms) + spread else 'NOT met'}")
    out.close()
    # vacuum: 40 000 live TIDs drawn at random, unsorted
    rng = np.random.default_rng(12)
    tids = ix.download(codes=False, nbrs=False)["heap_tids"]
    live = np.flatnonzero(tids & np.uint64(0xFFFF))
    dead = tids[rng.choice(live, min(40000, live.size), replace=False)]
    t0 = time.perf_counter()
    st = ix.bulk_delete(dead)
    t_bd = time.perf_counter() - t0
    say(f"(e) vs_index_bulk_delete of {dead.size} TIDs over {a.n} nodes: {t_bd * 1e3:.2f} ms (host clock, staging and sort included); {st}")
    # aminsert: 4 096 rows
    n_new = 4096
    new = rows_numpy(DatagenParams(seed=8, dim=a.dim), a.n, n_new)
    new_tids = ((np.arange(a.n, a.n + n_new, dtype=np.uint64) + 1) << np.uint64(16)) | np.uint64(1)
    labels = None
    if a.labels:
        from bench import zipf_labels
        lo, lv = zipf_labels(np, n_new, a.labels, 109, 1, 3)
        labels = [lv[lo[i]:lo[i + 1]].tolist() for i in range(n_new)]
    t0 = time.perf_counter()
    ist = ix.insert(new, new_tids, labels=labels, search_list_size=a.build_list)
    say(f"(f) vs_index_insert of {n_new} rows: {(time.perf_counter() - t0) * 1e3:.1f} ms; {ist}")
    out = PagesOut(ix, search_list_size=a.build_list)
    nb1 = out.n_blocks
    if nb1 * out.page_size > host.size:
        host = np.zeros(nb1 * out.page_size, np.uint8)
    blocks, nb_now, nbase = out.delta(base)  # warm-up
    nbase.close()
    out.read_blocks(blocks, out=host)
    out.read(out=host)
    td, tf = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        blocks, nb_now, nbase = out.delta(base)
        out.read_blocks(blocks, out=host)
        td.append(time.perf_counter() - t0)
        nbase.close()
        t0 = time.perf_counter()
        out.read(out=host)
        tf.append(time.perf_counter() - t0)
    # the patched blocks are the blocks of the full read
    full = out.read(out=host).reshape(nb1, out.page_size)
    same = bool((out.read_blocks(blocks).reshape(-1, out.page_size) == full[blocks]).all())
    ratio = nb1 / max(blocks.size, 1)
    speedup = np.median(tf) / np.median(td)
    margin = (max(tf) - min(tf)) + (max(td) - min(td))
    say(f"(g) dirty blocks: {blocks.size} of {nb1} ({100.0 * blocks.size / nb1:.2f} %; the relation grew from {nb0} blocks); delta + read_blocks: "
        f"{' '.join(f'{x * 1e3:.1f}' for x in td)} ms; vs_pages_out_read of the whole relation: {' '.join(f'{x * 1e3:.1f}' for x in tf)} ms; "
        f"medians {np.median(td) * 1e3:.1f} / {np.median(tf) * 1e3:.1f} ms = {speedup:.1f}x against {ratio:.1f}x fewer blocks moved "
        f"(spread of the two legs {margin * 1e3:.1f} ms); bytes identical to the full read: {same}")
    out.close()
    base.close()
    return dict(blocks_before=nb0, blocks_after=nb1, dirty=int(blocks.size), digest_ms=[round(x, 3) for x in dig_ms],
                encode_ms=[round(x, 3) for x in enc_ms], bulk_delete_ms=round(t_bd * 1e3, 2), delta_read_ms=[round(x * 1e3, 1) for x in td],
                full_read_ms=[round(x * 1e3, 1) for x in tf], bytes_identical=same)


def plain_leg(P, PagesOut, ctx, a, say):
    """--plain (module docstring) -> the result dict"""
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.datagen import DatagenParams, fill_device
    n = a.n
    ix = P.DiskAnnIndex.alloc(ctx, n=n, dim_full=a.dim, num_neighbors=a.R, distance_type=P.VS_COSINE if a.cosine else P.VS_L2,
                              storage_type=_lib.VS_STORAGE_PLAIN)
    vp, vec_stride = ix.array(_lib.ARR_VECS)
    fill_device(ctx, DatagenParams(seed=8, dim=a.dim), 0, n, vp)
    ix.refresh_norms()
    ctx.upload(ix.array(_lib.ARR_TIDS)[0], ((np.arange(n, dtype=np.uint64) + 1) << np.uint64(16)) | np.uint64(1))
    np_ptr, nbr_stride = ix.array(_lib.ARR_NBRS)
    rng = np.random.default_rng(13)
    step = 1 << 18
    for r0 in range(0, n, step):  # rows of nbr_stride ids: R random nodes, the sentinel behind them
        rows = np.full((min(step, n - r0), nbr_stride), 0xFFFFFFFF, np.uint32)
        rows[:, :a.R] = rng.integers(0, n, (rows.shape[0], a.R), dtype=np.uint32)
        ctx.upload(C.c_void_p(np_ptr.value + r0 * nbr_stride * 4), rows)
    ix.set_start_nodes(0, {})
    ctx.sync()
    t0 = time.perf_counter()
    out = PagesOut(ix, search_list_size=a.build_list, plain=True)
    t_open = time.perf_counter() - t0
    nb, ps = out.n_blocks, out.page_size
    node_pages = int(out.info.pages_by_type[1])
    total = nb * ps
    say(f"vs_pages_out_open_plain: {t_open * 1e3:.1f} ms; relation = {nb} blocks = {total / 1e9:.3f} GB, {node_pages} node pages, "
        f"{n / max(node_pages, 1):.2f} nodes per page")
    dbuf = ctx.alloc(total)
    out.read_dev(dbuf)  # warm-up: code object load
    ctx.profile_enable(True)
    ctx.profile_read(reset=True)
    k_ms = []
    for _ in range(a.reps):
        out.read_dev(dbuf)
        ms, launches = ctx.profile_read(reset=True)["pages_encode"]
        assert launches == 1
        k_ms.append(ms)
    ctx.profile_enable(False)
    read_bytes = n * (4 * ((a.dim + 3) // 4 * 4) + 4 * a.R + 8 + (4 if a.cosine else 0))
    written = node_pages * ps
    kb = min(k_ms)
    say(f"(a) k_pages_encode_plain, whole relation, one launch of {node_pages} workgroups: {' '.join(f'{x:.3f}' for x in k_ms)} ms; best {kb:.3f} ms = "
        f"{written / kb / 1e6:.1f} GB/s of pages written; algorithmic bytes {read_bytes / 1e9:.3f} GB read + {written / 1e9:.3f} GB written = "
        f"{(read_bytes + written) / kb / 1e6:.1f} GB/s = {(read_bytes + written) / (kb * 1e-3) / HBM_PEAK * 100:.1f} % of 8 TB/s")
    host = np.zeros(total, np.uint8)
    out.read(out=host)  # warm-up
    composed = ctx.download(dbuf, np.empty(total, np.uint8))
    same = bool((host == composed).all())
    del composed
    say(f"bytes of vs_pages_out_read == bytes composed in device memory: {same}")
    tb = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out.read(out=host)
        tb.append(time.perf_counter() - t0)
    say(f"(b) vs_pages_out_read, whole relation to the host: {' '.join(f'{x * 1e3:.1f}' for x in tb)} ms; median {np.median(tb) * 1e3:.1f} ms = "
        f"{total / np.median(tb) / 1e9:.2f} GB/s")
    ctx.free(dbuf)
    out.close()
    ix.close()
    return dict(plain=True, n=n, dim=a.dim, R=a.R, blocks=nb, node_pages=node_pages, open_ms=round(t_open * 1e3, 1),
                kernel_ms=[round(x, 3) for x in k_ms], kernel_gbs=round(written / kb / 1e6, 1), read_ms=[round(x * 1e3, 1) for x in tb],
                read_gbs=round(total / np.median(tb) / 1e9, 2), bytes_identical=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=None, help="default 4 000 000 (1 000 000 with --plain)")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--bits", type=int, default=0, help="0 = the reference's default for the dimension")
    ap.add_argument("--R", type=int, default=50)
    ap.add_argument("--labels", type=int, default=0, help="> 0: that many labels, Zipf, 1-3 per vector (label-aware build)")
    ap.add_argument("--cosine", action="store_true")
    ap.add_argument("--build-list", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--delta", action="store_true", help="add the baseline / bulk_delete / insert / delta + read_blocks leg")
    ap.add_argument("--open-only", action="store_true", help="time vs_pages_out_open on an allocated, unbuilt index and stop")
    ap.add_argument("--plain", action="store_true", help="a `plain` storage index through vs_pages_out_open_plain: legs (a) and (b)")
    a = ap.parse_args()
    if a.n is None:
        a.n = 1_000_000 if a.plain else 4_000_000
    if a.plain and (a.labels or a.delta or a.open_only):
        ap.error("--plain goes with neither --labels, --delta nor --open-only")

    import pgvectorscale_amd as P
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.datagen import DatagenParams, fill_device
    from pgvectorscale_amd.pages import PagesOut

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a" if a.append else "w") as f:
                f.write("\n".join(lines) + "\n\n")

    ctx = P.Context(0)
    dist = P.VS_COSINE if a.cosine else P.VS_L2
    if a.plain:
        say(f"# pages write, plain storage: n={a.n} dim={a.dim} R={a.R} on {ctx.device_name()}")
        res = plain_leg(P, PagesOut, ctx, a, say)
        say(json.dumps(res))
        ctx.close()
        flush()
        return 0 if res["bytes_identical"] else 1
    if a.open_only:
        say(f"# pages write, open only: n={a.n} dim={a.dim} R={a.R} labels={a.labels} on {ctx.device_name()}")
        ix = P.DiskAnnIndex.alloc(ctx, n=a.n, dim_full=a.dim, bits=a.bits or None, num_neighbors=a.R, distance_type=dist, with_vecs=False)
        if a.labels:
            from bench import zipf_labels
            lab_off, lab_val = zipf_labels(np, a.n, a.labels, 108, 1, 3)
            ix.set_labels(lab_off, lab_val)
        ctx.sync()
        out, t_open, node_pages = timed_open(P, PagesOut, ctx, ix, a, say)
        say(json.dumps(dict(open_only=True, n=a.n, dim=a.dim, R=a.R, labels=a.labels, blocks=out.n_blocks, node_pages=node_pages,
                            open_ms=round(t_open * 1e3, 1))))
        out.close()
        ix.close()
        ctx.close()
        flush()
        return 0
    say(f"# pages write: n={a.n} dim={a.dim} R={a.R} labels={a.labels} on {ctx.device_name()}")
    t0 = time.perf_counter()
    ix = P.DiskAnnIndex.alloc(ctx, n=a.n, dim_full=a.dim, bits=a.bits or None, num_neighbors=a.R, distance_type=dist)
    vp, _ = ix.array(_lib.ARR_VECS)
    fill_device(ctx, DatagenParams(seed=8, dim=a.dim), 0, a.n, vp)
    ix.refresh_norms()
    ix.sbq_train()
    ix.sbq_quantize_corpus()
    starts, n_label_vals = {}, 0
    if a.labels:
        from bench import label_start_nodes, zipf_labels
        lab_off, lab_val = zipf_labels(np, a.n, a.labels, 108, 1, 3)
        starts = label_start_nodes(np, lab_off, lab_val)
        n_label_vals = int(lab_off[-1])
        ix.set_labels(lab_off, lab_val)
    ix.build_graph(search_list_size=a.build_list, max_alpha=1.2)
    ix.set_start_nodes(0, starts)
    ctx.sync()
    d = ix.desc
    say(f"index built on the device in {time.perf_counter() - t0:.1f} s: bits={d.bits} words={d.words} has_labels={d.has_labels}")

    out, t_open, node_pages = timed_open(P, PagesOut, ctx, ix, a, say)
    nb, ps = out.n_blocks, out.page_size
    total = nb * ps

    # (a) the kernel alone
    dbuf = ctx.alloc(total)
    out.read_dev(dbuf)  # warm-up: code object load
    ctx.profile_enable(True)
    ctx.profile_read(reset=True)
    k_ms = []
    for _ in range(a.reps):
        out.read_dev(dbuf)
        ms, launches = ctx.profile_read(reset=True)["pages_encode"]
        assert launches == 1
        k_ms.append(ms)
    ctx.profile_enable(False)
    code_stride = d.words + (d.words & 1)
    read_bytes = a.n * (8 * code_stride + 4 * a.R + 8) + (4 * (a.n + 1) + 2 * n_label_vals if a.labels else 0)
    written = node_pages * ps
    kb = min(k_ms)
    say(f"(a) k_pages_encode, whole relation, one launch of {node_pages} workgroups: {' '.join(f'{x:.3f}' for x in k_ms)} ms; best {kb:.3f} ms = "
        f"{written / kb / 1e6:.1f} GB/s of pages written; algorithmic bytes {read_bytes / 1e9:.3f} GB read + {written / 1e9:.3f} GB written = "
        f"{(read_bytes + written) / kb / 1e6:.1f} GB/s = {(read_bytes + written) / (kb * 1e-3) / HBM_PEAK * 100:.1f} % of 8 TB/s")

    # (b) / (c) alternated, into one pre-faulted host buffer
    host = np.zeros(total, np.uint8)
    out.read(out=host)  # warm-up
    composed = ctx.download(dbuf, np.empty(total, np.uint8))
    same = bool((host == composed).all())
    del composed
    say(f"bytes of vs_pages_out_read == bytes composed in device memory: {same}")
    tb, tc = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out.read(out=host)
        tb.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ctx.download(dbuf, host)
        tc.append(time.perf_counter() - t0)
    chunk_pages = STAGING_BYTES // ps
    nchunks = (node_pages + chunk_pages - 1) // chunk_pages
    fill_ms = kb / max(nchunks, 1)
    say(f"(b) vs_pages_out_read, whole relation to the host: {' '.join(f'{x * 1e3:.1f}' for x in tb)} ms; median {np.median(tb) * 1e3:.1f} ms = "
        f"{total / np.median(tb) / 1e9:.2f} GB/s")
    say(f"(c) vs_dev_download of {total / 1e9:.3f} GB (copy floor): {' '.join(f'{x * 1e3:.1f}' for x in tc)} ms; median {np.median(tc) * 1e3:.1f} ms = "
        f"{total / np.median(tc) / 1e9:.2f} GB/s; spread {(max(tc) - min(tc)) * 1e3:.1f} ms")
    bound = np.median(tc) + (max(tc) - min(tc)) + fill_ms * 1e-3
    say(f"expectation: (b) <= (c) + spread of (c) + one chunk's kernel time ({nchunks} chunks, {fill_ms:.3f} ms) = {bound * 1e3:.1f} ms: "
        f"{'met' if np.median(tb) <= bound else 'NOT met'} ((b) - (c) = {(np.median(tb) - np.median(tc)) * 1e3:+.1f} ms)")
    res = dict(n=a.n, dim=a.dim, bits=int(d.bits), R=a.R, labels=a.labels, blocks=nb, node_pages=node_pages, open_ms=round(t_open * 1e3, 1),
               kernel_ms=[round(x, 3) for x in k_ms], read_ms=[round(x * 1e3, 1) for x in tb], download_ms=[round(x * 1e3, 1) for x in tc],
               bytes_identical=same)
    if a.delta:
        res["delta"] = delta_leg(P, PagesOut, ctx, ix, out, dbuf, host, a, say)
        out = None
    say(json.dumps(res))
    ctx.free(dbuf)
    if out is not None:
        out.close()
    ix.close()
    ctx.close()
    flush()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
