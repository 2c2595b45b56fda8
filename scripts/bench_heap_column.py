#!/usr/bin/env python3
"""The heap's vector column from heap and TOAST pages: the host reader + upload (vs_heap_*, vs_dev_upload) against the device reader
(vs_heap_dev_*), in one process on one box.

  1. a table of --rows x 768 rows is fabricated with numpy: six columns (id bigint, label smallint, tags, note, embedding, extra
     int4), every vector external in two TOAST chunks (1 996 + 1 080 bytes, two values on a TOAST page), 88 tuples on a heap page.
     The fabricator is first held to oracle/heap_py.py's pages byte for byte at 1 000 rows; the pages stay in host memory;
  2. one warm-up of each leg, then --reps alternating repetitions, host clock around work that ends in vs_ctx_sync:
       (a) vs_heap_open / _add / _toast_add / _finish into a host array, then vs_dev_upload of the rows into the device buffer;
       (b) vs_heap_dev_open / _add / _toast_add / _finish into the same device buffer, fed in calls of the pinned buffer's size;
  3. (b)'s rows are downloaded and compared with (a)'s and with the source vectors byte for byte at the timed size;
  4. one more run of (b) under vs_profile_enable reports the HIP-event time of the heap and the TOAST kernels, and the plain
     pinned-ring copy of the same page bytes (vs_dev_upload into a scratch buffer) is timed next to it: the line says whether the
     copy or the kernels bound (b).

Nothing fixes a ratio in advance; the script asserts only that (b) is not slower than (a) (median ratio >= 1.0) unless
--no-assert is given.  --inline-dim D adds one line for a table of D-dimensional vectors stored in line (D <= 400).

    python scripts/bench_heap_column.py --out profiles/r18/heap_column_262k.txt
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

ATTRS = [(8, "d"), (2, "s"), (-1, "i"), (-1, "i"), (-1, "i"), (4, "i")]
VEC_ATT = 5
B = HP.BLCKSZ
TAGS = struct.pack("<iiiii", 1, 0, 21, 3, 1)  # 20 bytes: a 1-byte varlena header
NOTE = b"abc"
STAGING = 32 << 20  # bytes per call of leg (b): the size of one of the context's two pinned buffers (vs_ctx_create)


def _tuple_header(natts, infomask, hoff=24):
    h = bytearray(hoff)
    struct.pack_into("<IIIIHHHB", h, 0, 700, 0, 0, 0, 0, natts, infomask, hoff)
    return np.frombuffer(bytes(h), np.uint8)


def fabricate(vecs, inline=False):
    """-> (heap pages uint8 [nh][B], TOAST pages uint8 [nt][B], tids uint64 [n]) as HP.Table.insert lays the same rows out"""
    n, dim = vecs.shape
    body = np.zeros((n, 4 + 4 * dim), np.uint8)
    body[:, 0:2] = np.frombuffer(struct.pack("<h", dim), np.uint8)
    body[:, 4:] = np.ascontiguousarray(vecs, "<f4").view(np.uint8).reshape(n, 4 * dim)
    ids = np.arange(n)
    # ---- the heap tuple: id @0, label @8, tags @10 (1-byte header), note @31 (1-byte header), the vector, extra int4 aligned
    fixed = np.zeros((n, 35), np.uint8)
    fixed[:, 0:8] = ids.astype("<i8").view(np.uint8).reshape(n, 8)
    fixed[:, 8:10] = (ids % 97).astype("<i2").view(np.uint8).reshape(n, 2)
    fixed[:, 10] = ((len(TAGS) + 1) << 1) | 1
    fixed[:, 11:31] = np.frombuffer(TAGS, np.uint8)
    fixed[:, 31] = ((len(NOTE) + 1) << 1) | 1
    fixed[:, 32:35] = np.frombuffer(NOTE, np.uint8)
    if inline:
        assert 127 <= body.shape[1] <= 1900
        at = (35 + 3) & ~3  # a 4-byte header at attalign 'i'
        vec = np.zeros((n, 4 + body.shape[1]), np.uint8)
        vec[:, 0:4] = np.frombuffer(struct.pack("<I", (body.shape[1] + 4) << 2), np.uint8)
        vec[:, 4:] = body
        infomask = HP.HEAP_XMIN_COMMITTED | HP.HEAP_XMAX_INVALID | HP.HEAP_HASVARWIDTH
    else:
        at = 35  # varatt_external is not aligned
        vec = np.zeros((n, 18), np.uint8)
        vec[:, 0], vec[:, 1] = 0x01, HP.VARTAG_ONDISK
        vec[:, 2:6] = np.frombuffer(struct.pack("<i", body.shape[1] + 4), np.uint8)
        vec[:, 6:10] = np.frombuffer(struct.pack("<I", body.shape[1]), np.uint8)
        vec[:, 10:14] = (20000 + ids).astype("<u4").view(np.uint8).reshape(n, 4)
        vec[:, 14:18] = np.frombuffer(struct.pack("<I", 16999), np.uint8)
        infomask = HP.HEAP_XMIN_COMMITTED | HP.HEAP_XMAX_INVALID | HP.HEAP_HASVARWIDTH | HP.HEAP_HASEXTERNAL
    extra_at = (at + vec.shape[1] + 3) & ~3
    tlen = 24 + extra_at + 4
    tup = np.zeros((n, tlen), np.uint8)
    tup[:, :24] = _tuple_header(6, infomask)
    tup[:, 24:24 + 35] = fixed
    tup[:, 24 + at:24 + at + vec.shape[1]] = vec
    tup[:, 24 + extra_at:] = ids.astype("<i4").view(np.uint8).reshape(n, 4)
    need = HP.maxalign(tlen)
    per = (B - 28 - need) // (need + 4) + 1  # add_item opens a new page when upper - lower - 4 < need
    nh = -(-n // per)
    heap = np.zeros((nh, B), np.uint8)
    blk, slot = ids // per, ids % per
    for sl in range(min(per, n)):  # (slot by slot: the rows of one slot lie at one place of their pages)
        rows = tup[sl::per]
        at_ = B - need * (sl + 1)
        heap[:rows.shape[0], at_:at_ + tlen] = rows
        heap[:rows.shape[0], 24 + 4 * sl:28 + 4 * sl] = np.frombuffer(struct.pack("<I", at_ | (HP.LP_NORMAL << 15) | (tlen << 17)), np.uint8)
    full = np.minimum(per, n - np.arange(nh) * per)
    heap[:, 12:14] = (24 + 4 * full).astype("<u2").view(np.uint8).reshape(nh, 2)
    heap[:, 14:16] = (B - need * full).astype("<u2").view(np.uint8).reshape(nh, 2)
    heap[:, 16:18] = np.frombuffer(struct.pack("<H", B), np.uint8)
    heap[:, 18:20] = np.frombuffer(struct.pack("<H", B | 4), np.uint8)
    tids = (blk.astype(np.uint64) << np.uint64(16)) | (slot + 1).astype(np.uint64)
    if inline:
        return heap, np.zeros((0, B), np.uint8), tids
    # ---- the TOAST relation: per value chunk 0 (1 996 bytes) and chunk 1 (the rest), two values = four items on a page
    chunk = HP.toast_max_chunk_size()
    rest = body.shape[1] - chunk
    assert 126 < rest <= chunk, "two chunks, both under 4-byte headers"
    la, lb = 24 + 8 + 4 + chunk, 24 + 8 + 4 + rest
    na, nb_ = HP.maxalign(la), HP.maxalign(lb)
    assert 2 * (na + nb_ + 8) + na + 4 > B - 24 >= 2 * (na + nb_ + 8), "two values a page"
    nt = -(-n // 2)
    toast = np.zeros((nt, B), np.uint8)
    th = _tuple_header(3, HP.HEAP_XMIN_COMMITTED | HP.HEAP_XMAX_INVALID | HP.HEAP_HASVARWIDTH)
    vid = (20000 + ids).astype("<u4").view(np.uint8).reshape(n, 4)
    for hf in (0, 1):  # (the first and the second value of every page)
        a_at = B - (na + nb_) * hf - na
        for at_, seq, lo, hi, ln in ((a_at, 0, 0, chunk, la), (a_at - nb_, 1, chunk, body.shape[1], lb)):
            k = len(range(hf, n, 2))
            toast[:k, at_:at_ + 24] = th
            toast[:k, at_ + 24:at_ + 28] = vid[hf::2]
            toast[:k, at_ + 28:at_ + 32] = np.frombuffer(struct.pack("<i", seq), np.uint8)
            toast[:k, at_ + 32:at_ + 36] = np.frombuffer(struct.pack("<I", (hi - lo + 4) << 2), np.uint8)
            toast[:k, at_ + 36:at_ + ln] = body[hf::2, lo:hi]
            sl = 2 * hf + seq
            toast[:k, 24 + 4 * sl:28 + 4 * sl] = np.frombuffer(struct.pack("<I", at_ | (HP.LP_NORMAL << 15) | (ln << 17)), np.uint8)
    items = np.minimum(4, 2 * (n - np.arange(nt) * 2))
    toast[:, 12:14] = (24 + 4 * items).astype("<u2").view(np.uint8).reshape(nt, 2)
    toast[:, 14:16] = (B - (na + nb_) * (items // 2)).astype("<u2").view(np.uint8).reshape(nt, 2)
    toast[:, 16:18] = np.frombuffer(struct.pack("<H", B), np.uint8)
    toast[:, 18:20] = np.frombuffer(struct.pack("<H", B | 4), np.uint8)
    return heap, toast, tids


def oracle_table(vecs, inline=False):
    t = HP.Table(ATTRS)
    tids = []
    for i, v in enumerate(vecs):
        tids.append(t.insert([struct.pack("<q", i), struct.pack("<h", i % 97), ("inline", TAGS), ("inline", NOTE),
                              ("inline", HP.vector_datum_body(v)), struct.pack("<i", i)]))
    return t.heap.tobytes(), t.toast.tobytes(), np.array(tids, np.uint64)


def check_fabricator(dim, inline, rows=1000):
    v = np.random.default_rng(3).standard_normal((rows, dim)).astype(np.float32)
    heap, toast, tids = fabricate(v, inline)
    oh, ot, otids = oracle_table(v, inline)
    assert heap.tobytes() == oh, "heap pages differ from oracle/heap_py.py's"
    assert toast.tobytes() == ot, "TOAST pages differ from oracle/heap_py.py's"
    assert (tids == otids).all()


def run(P, ctx, a, say, dim, inline):
    from pgvectorscale_amd.pages import HeapColumn, HeapColumnDev
    n = a.rows
    check_fabricator(dim, inline)
    say(f"fabricator: {dim} dimensions {'in line' if inline else 'external, two chunks'}: byte-identical to oracle/heap_py.py at 1000 rows")
    t0 = time.perf_counter()
    vecs = np.random.default_rng(7).standard_normal((n, dim), dtype=np.float32)
    heap, toast, tids = fabricate(vecs, inline)
    say(f"table: {n} x {dim}, heap {heap.nbytes / 1e6:.1f} MB in {heap.shape[0]} pages, TOAST {toast.nbytes / 1e6:.1f} MB in {toast.shape[0]} pages "
        f"(fabricated in {time.perf_counter() - t0:.1f} s)")
    heap_b, toast_b = heap.reshape(-1), toast.reshape(-1)
    d_out = ctx.alloc(n * dim * 4)
    per = max(STAGING // B, 1) * B

    def leg_a():
        t = time.perf_counter()
        hc = HeapColumn(ATTRS, VEC_ATT, dim, tids)
        hc.add(heap_b)
        hc.toast_add(toast_b)
        info, found = hc.finish()
        t1 = time.perf_counter()
        ctx.upload(d_out, hc.vecs)
        ctx.sync()
        t2 = time.perf_counter()
        rows = hc.vecs
        hc.close()
        return t2 - t, (t1 - t, t2 - t1), rows, info, found

    def leg_b(profile=False):
        t = time.perf_counter()
        hc = HeapColumnDev(ctx, ATTRS, VEC_ATT, dim, tids, d_out, dim)
        t1 = time.perf_counter()
        for at in range(0, heap_b.size, per):
            hc.add(heap_b[at:at + per], first_block=at // B)
        kern = {}
        if profile:
            kern["heap"] = ctx.profile_read(reset=True)["pages_encode"]
        t2 = time.perf_counter()
        for at in range(0, toast_b.size, per):
            hc.toast_add(toast_b[at:at + per], first_block=at // B)
        if profile:
            kern["toast"] = ctx.profile_read(reset=True)["pages_encode"]
        t3 = time.perf_counter()
        info, found, ncomp = hc.finish()
        ctx.sync()
        t4 = time.perf_counter()
        hc.close()
        return t4 - t, (t1 - t, t2 - t1, t3 - t2, t4 - t3), info, found, ncomp, kern

    leg_a(), leg_b()  # warm-up
    ta, tb, pa, pb = [], [], [], []
    for _ in range(a.reps):
        x = leg_a()
        ta.append(x[0]), pa.append(x[1])
        rows_a, info_a, found_a = x[2], x[3], x[4]
        y = leg_b()
        tb.append(y[0]), pb.append(y[1])
    got = ctx.download(d_out, np.empty((n, dim), np.float32))
    assert found_a.all() and y[3].all() and y[4] == 0 and y[2] == info_a, (y[2], info_a)
    assert got.tobytes() == rows_a.tobytes() == vecs.tobytes(), "the device reader's rows differ"
    say(f"rows: (b) == (a) == source, byte for byte, {n} x {dim}; info {y[2]}")
    med = lambda v: float(np.median(v))
    pam, pbm = np.median(np.array(pa), 0), np.median(np.array(pb), 0)
    say(f"(a) host reader + upload: median {med(ta) * 1e3:.1f} ms (min {min(ta) * 1e3:.1f}, max {max(ta) * 1e3:.1f}); decode {pam[0] * 1e3:.1f} ms, upload {pam[1] * 1e3:.1f} ms")
    say(f"(b) device reader:        median {med(tb) * 1e3:.1f} ms (min {min(tb) * 1e3:.1f}, max {max(tb) * 1e3:.1f}); open {pbm[0] * 1e3:.1f} ms, heap pass "
        f"{pbm[1] * 1e3:.1f} ms, TOAST pass {pbm[2] * 1e3:.1f} ms, finish {pbm[3] * 1e3:.1f} ms")
    ratio = med(ta) / med(tb)
    say(f"ratio (a) / (b) of the medians: {ratio:.2f}")
    # the kernels' own time (HIP events) and the bare copy of the same bytes
    ctx.profile_enable(True)
    ctx.profile_read(reset=True)
    kern = leg_b(profile=True)[5]
    ctx.profile_enable(False)
    d_scratch = ctx.alloc(max(heap_b.size, toast_b.size, 16))
    copy = {}
    for name, buf in (("heap", heap_b), ("toast", toast_b)):
        ts = []
        for _ in range(3):
            t = time.perf_counter()
            if buf.size:
                ctx.upload(d_scratch, buf)
            ctx.sync()
            ts.append(time.perf_counter() - t)
        copy[name] = med(ts)
    ctx.free(d_scratch)
    out = {"rows": n, "dim": dim, "inline": inline, "a_ms": [round(v * 1e3, 2) for v in ta], "b_ms": [round(v * 1e3, 2) for v in tb],
           "a_median_ms": round(med(ta) * 1e3, 2), "b_median_ms": round(med(tb) * 1e3, 2), "ratio": round(ratio, 3)}
    for name, buf in (("heap", heap_b), ("toast", toast_b)):
        ms, launches = kern.get(name, (0.0, 0))
        gbs_k = buf.size / ms / 1e6 if ms else 0.0
        gbs_c = buf.size / copy[name] / 1e9 if copy[name] and buf.size else 0.0
        say(f"{name} pages: {buf.size / 1e6:.1f} MB; kernels {ms:.2f} ms in {launches} launches = {gbs_k:.1f} GB/s of pages; "
            f"pinned-ring copy alone {copy[name] * 1e3:.1f} ms = {gbs_c:.1f} GB/s -> "
            f"{'the copy' if copy[name] * 1e3 > ms else 'the kernels'} bound this pass")
        out[f"{name}_kernel_ms"], out[f"{name}_kernel_GBps"] = round(ms, 3), round(gbs_k, 1)
        out[f"{name}_copy_ms"], out[f"{name}_copy_GBps"] = round(copy[name] * 1e3, 2), round(gbs_c, 1)
    ctx.free(d_out)
    say(json.dumps(out))
    return ratio


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inline-dim", type=int, default=0, help="also one line for vectors of this many dimensions stored in line (e.g. 128)")
    ap.add_argument("--no-assert", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pgvectorscale_amd as P
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = P.Context(0)
    say(f"bench_heap_column on {ctx.device_name()}: rows {a.rows}, reps {a.reps}")
    ratios = [run(P, ctx, a, say, 768, False)]
    if a.inline_dim:
        ratios.append(run(P, ctx, a, say, a.inline_dim, True))
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not a.no_assert:
        assert ratios[0] >= 1.0, f"the device reader is slower than the host reader + upload: ratio {ratios[0]:.2f}"


if __name__ == "__main__":
    main()
