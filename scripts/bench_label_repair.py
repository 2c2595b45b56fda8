#!/usr/bin/env python3
"""What label-filtered scans cannot reach, and what vs_index_repair_labels costs to mend it, on the device-built labeled index of the
other maintenance benches (4M x 768, 2 bits, R = 50) with 32 Zipf labels, built label-aware by vs_build_graph.

  (a) vs_index_label_reach after the build: lost (row, label) pairs and rows, sweeps, wall time;
  (b) vs_index_repair_labels: rounds, sweeps, placements, wall time, the HIP-event time of its four kernel groups
      (vs_index_label_repair_kernel_ms), and the source kernel's rate on its algorithmic traffic — source_tiles x n x (code row + 8 B
      of reach + 1 B of class) over its milliseconds;
  (c) the same after 30 % deletes (random TIDs, fixed seed) and vs_index_consolidate_deletes;
  (d) the yardstick: k_scan_topk at 4-query tiles on the same codes in the same process (vs_profile_read "scan"), n x code row per tile.
Nothing here asserts a number.

    python scripts/bench_label_repair.py --out profiles/r13/s1_label_repair_4m.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def zipf_label_sets(n, n_labels, seed):
    """1-3 labels per row, Zipf (s = 1) over 1..n_labels -> CSR (off uint32 [n + 1], val int16), each set sorted and de-duplicated"""
    rng = np.random.default_rng(seed)
    pz = 1.0 / np.arange(1, n_labels + 1)
    pz /= pz.sum()
    lab = (rng.choice(n_labels, (n, 3), p=pz) + 1).astype(np.int16)
    k = rng.integers(1, 4, n)
    lab[k < 3, 2] = lab[k < 3, 0]
    lab[k < 2, 1] = lab[k < 2, 0]
    lab.sort(axis=1)
    keep = np.ones((n, 3), bool)
    keep[:, 1:] = lab[:, 1:] != lab[:, :-1]
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum(keep.sum(1))
    return off, np.ascontiguousarray(lab[keep])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--R", type=int, default=50)
    ap.add_argument("--build-list", type=int, default=100)
    ap.add_argument("--labels", type=int, default=32)
    ap.add_argument("--delete", type=float, default=0.3)
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
    say(f"# label repair: n={a.n} dim={a.dim} R={a.R} build L={a.build_list} labels={a.labels} (Zipf) on {ctx.device_name()}")
    tids = ((np.arange(a.n, dtype=np.uint64) + 1) << np.uint64(16)) | np.uint64(1)
    off, val = zipf_label_sets(a.n, a.labels, 77)
    ix = P.DiskAnnIndex.alloc(ctx, n=a.n, dim_full=a.dim, num_neighbors=a.R, distance_type=P.VS_L2)
    fill_device(ctx, p, 0, a.n, ix.array(_lib.ARR_VECS)[0])
    ctx.upload(ix.array(_lib.ARR_TIDS)[0], tids)
    ix.set_labels(off, val)
    ix.refresh_norms()
    ix.sbq_train()
    ix.sbq_quantize_corpus()
    ctx.sync()
    t0 = time.perf_counter()
    ix.build_graph(search_list_size=a.build_list, max_alpha=1.2)
    ctx.sync()
    say(f"label-aware vs_build_graph: {time.perf_counter() - t0:.2f} s; unreachable from the default start node: {ix.build_unreachable()}")
    code_row = ix.array(_lib.ARR_CODES)[1] * 8
    res = []

    def leg(name):
        t0 = time.perf_counter()
        audit = ix.label_reach()
        t_audit = time.perf_counter() - t0
        per = audit.pop("per_label")
        worst = sorted(per.items(), key=lambda kv: -kv[1][1] / max(kv[1][0], 1))[:4]
        say(f"--- {name}")
        say(f"(a) vs_index_label_reach: {t_audit * 1e3:.1f} ms wall; {audit}; worst labels (label: carriers, lost): {worst}")
        ctx.profile_enable(True)
        ix.label_repair_kernel_ms(reset=True)
        t0 = time.perf_counter()
        st = ix.repair_labels()
        t_call = time.perf_counter() - t0
        ms = ix.label_repair_kernel_ms(reset=True)
        ctx.profile_enable(False)
        traffic = st["source_tiles"] * a.n * (code_row + 9)
        rate = traffic / (ms["sources"] * 1e-3) / 1e12 if ms["sources"] > 0 else 0.0
        say(f"(b) vs_index_repair_labels: {t_call * 1e3:.1f} ms wall (both audits, the unfiltered sweep and the list validation included); {st}")
        say(f"    kernels: {ms}; source kernel: {st['source_tiles']} tiles x {a.n} rows x {code_row + 9} B = {traffic / 1e9:.2f} GB in "
            f"{ms['sources']:.3f} ms = {rate:.3f} TB/s")
        res.append(dict(leg=name, audit=audit, audit_ms=round(t_audit * 1e3, 1), call_ms=round(t_call * 1e3, 1), stats=st, kernel_ms=ms,
                        source_tb_s=round(rate, 3)))

    leg("after the build")
    dead = np.flatnonzero(np.random.default_rng(12).random(a.n) < a.delete)
    dead = dead[dead != ix.desc.default_start]
    ix.bulk_delete(tids[dead])
    cst = ix.consolidate_deletes()
    say(f"{a.delete:.0%} deleted ({dead.size} rows), consolidated: {cst}")
    leg(f"after {a.delete:.0%} deletes + consolidate (on the repaired graph of the first leg)")
    # (d) the flat scan at 4-query tiles on the same codes
    nq = 64
    P.set_option("VS_SCAN_Q", 4)
    qc = ix.download(codes=True, nbrs=False, tids=False, row_begin=0, row_count=nq)["codes"]
    ix.scan_topk(qc, 10)  # warm-up
    ctx.profile_enable(True)
    ctx.profile_read(reset=True)
    ix.scan_topk(qc, 10)
    ctx.sync()
    scan_ms = ctx.profile_read(reset=True)["scan"][0]
    ctx.profile_enable(False)
    P.set_option("VS_SCAN_Q", None)
    scan_rate = (nq // 4) * a.n * code_row / (scan_ms * 1e-3) / 1e12 if scan_ms > 0 else 0.0
    say(f"(d) k_scan_topk, {nq} queries in tiles of 4, k = 10: {scan_ms:.3f} ms = {scan_rate:.3f} TB/s on n x code row per tile")
    say(json.dumps(dict(n=a.n, dim=a.dim, R=a.R, labels=a.labels, legs=res, scan_tb_s=round(scan_rate, 3))))
    ix.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
