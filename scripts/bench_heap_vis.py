#!/usr/bin/env python3
"""Heap visibility from resident heap pages: the put of the fork, one evaluation (k_heap_vis), and what the library offered for the
same job before — vs_index_snapshot_put of an n-byte host mask — in one process on one box.

  1. --rows fixed-width tuples (one bigint column: 32 bytes a tuple, 226 to an 8 KB page; 4 M rows are about 145 MB of pages) are
     fabricated with numpy; the fabricator is first held to oracle/heap_py.py's pages byte for byte at 1 000 rows.  The headers are
     a mix whose verdict is known by construction: 70 % hinted committed, 10 % committed without the hint (pg_xact decides), 10 %
     inserted by a transaction of the snapshot's xip, 10 % deleted by an old committed transaction;
  2. vs_heap_res_put of the whole fork: host clock around calls that end in vs_ctx_sync, median of --reps;
  3. vs_index_snapshot_eval over an index of --rows nodes whose tid column is in heap order, and again in shuffled order: the
     kernel's HIP-event time (vs_profile_*), warm, median of --reps launches, with the whole call's host time next to it; the mask
     and every counter are compared with the construction at the timed size;
  4. vs_index_snapshot_put of a host mask of --rows bytes into the same index: host clock, median.

(4) is only the upload.  In a real shim it is preceded by one table_index_fetch_tuple per node on one backend core, which cannot be
run here (there is no PostgreSQL in this environment), so the comparison understates what the evaluation replaces.

The expectation to read the kernel time against is a derivation, not a measurement: per node the 8-byte tid, one line-pointer line
and one tuple-header line are gathered and one byte is written.  In heap order neighbouring lanes share those lines (4 + 32 bytes a
node: the pages are read about once); in shuffled order every node pulls two lines of its own.

    python scripts/bench_heap_vis.py --out profiles/r19/heap_vis_4m.txt
"""
import argparse
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import heap_py as HP  # noqa: E402

B = HP.BLCKSZ
ATTRS = [(8, "d")]
TLEN = 32
XMIN_COMMITTED, XMAX_COMMITTED, XMAX_INVALID = 0x0100, 0x0400, 0x0800
# the snapshot: xmin 1000, xmax 2000, xip {1500, 1200}; pg_xact window [800, 2200): everything committed
SNAP = dict(xmin=1000, xmax=2000, xip=[1500, 1200], curcid=1)
XACT = (800, 1400, np.full(350, 0x55, np.uint8))
KINDS = 10  # row i is of kind i % 10: 0-6 hinted committed, 7 committed by pg_xact, 8 xmin in xip, 9 deleted


def headers(n):
    """-> (xmin, xmax, infomask) per row and the verdict the rule gives each"""
    k = np.arange(n) % KINDS
    xmin = np.where(k == 8, 1200, 900 + (np.arange(n) % 97)).astype("<u4")
    xmax = np.where(k == 9, 950, 0).astype("<u4")
    m = np.full(n, XMIN_COMMITTED | XMAX_INVALID, np.uint32)
    m[k == 7] = XMAX_INVALID
    m[k == 8] = XMAX_INVALID
    m[k == 9] = XMIN_COMMITTED | XMAX_COMMITTED
    return xmin, xmax, m.astype("<u2"), (k < 8).astype(np.uint8)


def fabricate(n, headers=headers):
    """-> (pages uint8 [nb][B], tids uint64 [n] in heap order, expected mask) as HP.HeapRelation.add_item lays the same rows out;
    headers: the header mix (scripts/bench_vis_overlay.py brings its own)"""
    xmin, xmax, m, expect = headers(n)
    tup = np.zeros((n, TLEN), np.uint8)
    tup[:, 0:4] = xmin.view(np.uint8).reshape(n, 4)
    tup[:, 4:8] = xmax.view(np.uint8).reshape(n, 4)
    tup[:, 18:20] = np.frombuffer(struct.pack("<H", 1), np.uint8)
    tup[:, 20:22] = m.view(np.uint8).reshape(n, 2)
    tup[:, 22] = 24
    tup[:, 24:32] = np.arange(n).astype("<i8").view(np.uint8).reshape(n, 8)
    per = (B - 28 - TLEN) // (TLEN + 4) + 1  # add_item opens a new page when upper - lower - 4 < need
    nb = -(-n // per)
    pages = np.zeros((nb, B), np.uint8)
    ids = np.arange(n)
    for sl in range(min(per, n)):  # (slot by slot: the rows of one slot lie at one place of their pages)
        rows = tup[sl::per]
        at = B - TLEN * (sl + 1)
        pages[:rows.shape[0], at:at + TLEN] = rows
        pages[:rows.shape[0], 24 + 4 * sl:28 + 4 * sl] = np.frombuffer(struct.pack("<I", at | (HP.LP_NORMAL << 15) | (TLEN << 17)), np.uint8)
    full = np.minimum(per, n - np.arange(nb) * per)
    pages[:, 12:14] = (24 + 4 * full).astype("<u2").view(np.uint8).reshape(nb, 2)
    pages[:, 14:16] = (B - TLEN * full).astype("<u2").view(np.uint8).reshape(nb, 2)
    pages[:, 16:18] = np.frombuffer(struct.pack("<H", B), np.uint8)
    pages[:, 18:20] = np.frombuffer(struct.pack("<H", B | 4), np.uint8)
    tids = ((ids // per).astype(np.uint64) << np.uint64(16)) | (ids % per + 1).astype(np.uint64)
    return pages, tids, expect


def check_fabricator(rows=1000, headers=headers):
    pages, tids, _ = fabricate(rows, headers)
    xmin, xmax, m, _ = headers(rows)
    rel = HP.HeapRelation()
    otids = []
    for i in range(rows):
        t = bytearray(HP.form_tuple(ATTRS, [struct.pack("<q", i)]))
        struct.pack_into("<II", t, 0, int(xmin[i]), int(xmax[i]))
        struct.pack_into("<H", t, 20, int(m[i]))
        blk, off = rel.add_item(bytes(t))
        otids.append((blk << 16) | off)
    assert pages.tobytes() == rel.tobytes(), "pages differ from oracle/heap_py.py's"
    assert (tids == np.array(otids, np.uint64)).all()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pgvectorscale_amd as P
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.pages import HeapResident
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    med = lambda v: float(np.median(v))  # noqa: E731
    n = a.rows
    ctx = P.Context(0)
    say(f"bench_heap_vis on {ctx.device_name()}: rows {n}, reps {a.reps}")
    check_fabricator()
    say("fabricator: byte-identical to oracle/heap_py.py at 1000 rows")
    t0 = time.perf_counter()
    pages, tids, expect = fabricate(n)
    say(f"fork: {n} tuples of {TLEN} bytes, {pages.nbytes / 1e6:.1f} MB in {pages.shape[0]} pages (fabricated in {time.perf_counter() - t0:.1f} s)")
    flat = pages.reshape(-1)
    out = {"rows": n, "pages_MB": round(pages.nbytes / 1e6, 1)}

    # ---- the put of the whole fork
    heap = HeapResident(ctx, pages.shape[0])
    ts = []
    for _ in range(a.reps + 1):
        t = time.perf_counter()
        heap.put(flat)
        ctx.sync()
        ts.append(time.perf_counter() - t)
    ts = ts[1:]
    say(f"vs_heap_res_put of the whole fork: median {med(ts) * 1e3:.1f} ms (min {min(ts) * 1e3:.1f}, max {max(ts) * 1e3:.1f}) = "
        f"{pages.nbytes / med(ts) / 1e9:.1f} GB/s of pages")
    out["put_ms"] = round(med(ts) * 1e3, 2)
    one = flat[:B]
    t1 = []
    for _ in range(a.reps):
        t = time.perf_counter()
        heap.put(one, first_block=0)
        ctx.sync()
        t1.append(time.perf_counter() - t)
    say(f"vs_heap_res_put of one changed block: median {med(t1) * 1e6:.0f} us")
    out["put_one_block_us"] = round(med(t1) * 1e6, 1)

    # ---- the evaluation on an index of n nodes
    ix = P.DiskAnnIndex.alloc(ctx, n=n, dim_full=64, bits=1, num_neighbors=4, with_vecs=False)
    d_tids, _ = ix.array(_lib.ARR_TIDS)
    rng = np.random.default_rng(5)
    perm = rng.permutation(n)
    for name, order in (("heap order", None), ("shuffled order", perm)):
        t_ix = tids if order is None else tids[order]
        want = expect if order is None else expect[order]
        ctx.upload(d_tids, t_ix)
        st, und, nu = ix.snapshot_eval(heap, 1, SNAP, XACT)  # warm-up, and the check at the timed size
        prev, mine = _lib.C.c_void_p(), _lib.C.c_void_p()
        _lib.check(ix._L.vs_index_snapshot_use(ix.h, 1, _lib.C.byref(prev)))
        _lib.check(ix._L.vs_index_snapshot_use(ix.h, 0, _lib.C.byref(mine)))
        got = ctx.download(mine, np.empty(n, np.uint8))
        assert (got == want).all(), "the evaluated mask differs from the construction"
        assert st["n_visible"] == int(want.sum()) and st["n_invisible"] == n - int(want.sum()) and nu == 0 and st["chain_hops"] == 0, st
        ctx.profile_enable(True)
        kern, call = [], []
        for _ in range(a.reps):
            ctx.profile_read(reset=True)
            t = time.perf_counter()
            ix.snapshot_eval(heap, 1, SNAP, XACT, cap=0)
            call.append(time.perf_counter() - t)
            ms, launches = ctx.profile_read(reset=True)["pages_encode"]
            assert launches == 1
            kern.append(ms)
        ctx.profile_enable(False)
        k = med(kern)
        say(f"vs_index_snapshot_eval, {name}: mask and counters equal the construction ({st['n_visible']} visible, {st['n_invisible']} invisible); "
            f"k_heap_vis median {k:.3f} ms (min {min(kern):.3f}, max {max(kern):.3f}) = {n / k / 1e6:.2f} G nodes/s, "
            f"{pages.nbytes / k / 1e6:.0f} GB/s if the fork is read once, {45 * n / k / 1e6:.0f} GB/s of the 45 bytes a node needs; "
            f"the whole call {med(call) * 1e3:.2f} ms")
        key = "heap_order" if order is None else "shuffled"
        out[f"kernel_ms_{key}"], out[f"call_ms_{key}"] = round(k, 4), round(med(call) * 1e3, 3)

    # ---- what the library offered before: the upload of a host mask (the per-tuple fetch loop in front of it cannot be run here)
    mask = expect.copy()
    ts = []
    for _ in range(a.reps + 1):
        t = time.perf_counter()
        _lib.check(ix._L.vs_index_snapshot_put(ix.h, 2, mask.ctypes.data_as(_lib.C.c_void_p)))
        ctx.sync()
        ts.append(time.perf_counter() - t)
    ts = ts[1:]
    say(f"vs_index_snapshot_put of a {n}-byte host mask: median {med(ts) * 1e3:.2f} ms (min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f}) — the upload "
        f"alone; the host's table_index_fetch_tuple per node that precedes it in a shim is not part of this number (no PostgreSQL here)")
    out["snapshot_put_ms"] = round(med(ts) * 1e3, 3)
    say(json.dumps(out))
    ix.close()
    heap.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
