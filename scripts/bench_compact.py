#!/usr/bin/env python3
"""What vs_index_compact's row mover costs, beside a plain device copy of the same traffic, on the device-built index of
scripts/bench_consolidate.py (4M x 768, R = 50), 30 % of the rows deleted (random TIDs, fixed seed) and consolidated.

  (a) the call: wall time, the HIP-event time of its two passes (keep flags + maps, the row mover) from vs_index_compact_kernel_ms,
      and the bytes the mover moved, read + written: every moved row is read from its column and written to staging, then read
      from staging and written to its place (4 x its width); every neighbor row is renamed, so that column counts all n_after rows;
  (b) the yardstick: plain device-to-device hipMemcpy calls that move the same number of bytes (a copy of S bytes reads S and
      writes S), timed with HIP events in the same process, between two buffers of --copy-mib;
  (c) vs_index_shrink_to_fit: wall time and the free device memory before and after.
Nothing here asserts a number and no ratio is fixed in advance: (b) is what (a)'s mover is read against.

    python scripts/bench_compact.py --out profiles/r12/s1_compact_4m.txt
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

D2D = 3  # hipMemcpyDeviceToDevice


def copy_ms(ctx, total_bytes, buf_bytes, reps):
    """median HIP-event milliseconds of device-to-device hipMemcpy calls that copy total_bytes / 2 (read + written = total_bytes)"""
    # the HIP runtime libvsgpu.so already runs on (two copies of libamdhip64 in one process do not share device pointers)
    with open("/proc/self/maps") as f:
        loaded = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    assert len(loaded) == 1, loaded
    hip = C.CDLL(loaded[0])
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    want = total_bytes // 2
    buf_bytes = max(min(buf_bytes, want), 1)
    src, dst = ctx.alloc(buf_bytes), ctx.alloc(buf_bytes)
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    out = []
    try:
        for _ in range(reps + 1):  # (the first round is the warm-up)
            assert hip.hipEventRecord(e0, None) == 0
            left = want
            while left > 0:
                part = min(left, buf_bytes)
                assert hip.hipMemcpy(dst, src, part, D2D) == 0
                left -= part
            assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
            ms = C.c_float(0)
            assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            out.append(float(ms.value))
    finally:
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
        ctx.free(src)
        ctx.free(dst)
    return float(np.median(out[1:])), out[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--R", type=int, default=50)
    ap.add_argument("--build-list", type=int, default=100)
    ap.add_argument("--frac", type=float, default=0.3)
    ap.add_argument("--stage-mib", type=int, default=0, help="stage_bytes of the call in MiB (0 = the library's default)")
    ap.add_argument("--copy-mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import pgvectorscale_amd as P
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.datagen import DatagenParams, fill_device

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = P.Context(0)
    p = DatagenParams(seed=8, dim=a.dim)
    say(f"# compact: n={a.n} dim={a.dim} R={a.R} build L={a.build_list} deleted {a.frac:.0%} on {ctx.device_name()}")
    tids = ((np.arange(a.n, dtype=np.uint64) + 1) << np.uint64(16)) | np.uint64(1)
    ix = P.DiskAnnIndex.alloc(ctx, n=a.n, dim_full=a.dim, num_neighbors=a.R, distance_type=P.VS_L2)
    fill_device(ctx, p, 0, a.n, ix.array(_lib.ARR_VECS)[0])
    ix.refresh_norms()
    ix.sbq_train()
    ix.sbq_quantize_corpus()
    ix.build_graph(search_list_size=a.build_list, max_alpha=1.2)
    ctx.upload(ix.array(_lib.ARR_TIDS)[0], tids)
    dead = np.flatnonzero(np.random.default_rng(12).random(a.n) < a.frac)
    dead = dead[dead != ix.desc.default_start]
    ix.bulk_delete(tids[dead])
    cons = ix.consolidate_deletes()
    say(f"consolidated: {cons}")
    widths = dict(codes=ix.array(_lib.ARR_CODES)[1] * 8, nbrs=ix.array(_lib.ARR_NBRS)[1] * 4, tids=8, vecs=ix.array(_lib.ARR_VECS)[1] * 4,
                  vnorm=4 if ix.array(_lib.ARR_VNORM)[0].value else 0)
    ctx.profile_enable(True)
    ix.compact_kernel_ms(reset=True)
    ctx.sync()
    t0 = time.perf_counter()
    st = ix.compact(stage_bytes=a.stage_mib << 20, check_edges=True)
    ctx.sync()
    t_call = time.perf_counter() - t0
    ms = ix.compact_kernel_ms(reset=True)
    ctx.profile_enable(False)
    one_way = st["rows_moved"] * (widths["codes"] + widths["tids"] + widths["vecs"] + widths["vnorm"]) + st["n_after"] * widths["nbrs"]
    moved = 4 * one_way
    say(f"(a) vs_index_compact: {t_call * 1e3:.1f} ms wall; kernels: maps {ms['maps']:.3f} ms, row mover {ms['rows']:.3f} ms; "
        f"{moved / 1e9:.3f} GB read + written = {moved / 1e6 / max(ms['rows'], 1e-9):.1f} GB/s; {st}")
    c_ms, c_all = copy_ms(ctx, moved, a.copy_mib << 20, a.reps)
    say(f"(b) hipMemcpy device to device, {moved / 2e9:.3f} GB copied = the same {moved / 1e9:.3f} GB read + written: "
        f"median {c_ms:.3f} ms of {[round(x, 3) for x in c_all]} = {moved / 1e6 / max(c_ms, 1e-9):.1f} GB/s; mover / copy = {ms['rows'] / max(c_ms, 1e-9):.2f}")
    free0 = ctx.mem_info()[0]
    t0 = time.perf_counter()
    ix.shrink_to_fit()
    t_shrink = time.perf_counter() - t0
    free1 = ctx.mem_info()[0]
    say(f"(c) vs_index_shrink_to_fit: {t_shrink * 1e3:.1f} ms wall; free device memory {free0 / 1e9:.3f} -> {free1 / 1e9:.3f} GB")
    say(json.dumps(dict(n=a.n, dim=a.dim, R=a.R, frac=a.frac, stats=st, call_ms=round(t_call * 1e3, 1), kernel_ms=ms, moved_bytes=int(moved),
                        copy_ms=round(c_ms, 3), shrink_ms=round(t_shrink * 1e3, 1), freed_bytes=int(free1 - free0))))
    ix.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
