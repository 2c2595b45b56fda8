#!/usr/bin/env python3
"""bench.py — QPS at recall@10 >= 0.99 of the StreamingDiskANN search hot path on MI355X, next to the CPU oracle.

One "step" = one pass of the hot path (query preparation + SBQ quantisation, streaming beam search with Hamming
scoring, f32 rerank, rescore window) over one batch of `--nq` synthetic queries that already sit in HBM.

  python bench.py                       # 1 GPU, the headline value only, on a 4M x 768 index (L2, SBQ 2 bit + rerank) that is
                                        # built on the device in seconds: set-up, warm-up, timed steps, the line
  python bench.py --full                # 50M x 768 (the configuration the metric of BASELINE.json is quoted on; 177 GB index
                                        # on ONE GPU; ~8 min, 3 of them the on-device index build) with everything else the
                                        # script measures: CPU baseline, flat-scan roofline, PCIe leg, extras
  python bench.py --n 50000000          # the headline value alone at 50M
  python bench.py --full --n 10000000 --distance cosine   # configs[2] (~1.5 min);   --n 1000000: configs[1] (~20 s)
  python bench.py --n 20000000 --dim 1536 --distance cosine --labels 32   # configs[4]: label-filtered scans
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W   # index replicated per GPU, queries sharded, RCCL all_gather of top-k

Prints ONE JSON line (rank 0).  Setup (corpus generation, SBQ training, quantisation, graph build, ground truth,
recall sweep) is outside the timed region.

A plain run does what the headline value needs and nothing else: set-up, warm-up, the timed steps, the recall check of
the rows the last timed step produced, the line.  Everything else the script can measure — the CPU baseline (the oracle,
a port of the reference path, on a bounded sample of the same queries on the host cores) with its closing row-identity
check, the flat SBQ scan roofline, the PCIe-inclusive leg and the extras (default GUCs, cursor pools, latency, the
harder corpus) — runs only with --full.  The 50M index takes three minutes to build, so it is the default corpus of a
--full run only; a plain run defaults to 4M vectors of the same generator (`config.n` in the line says which).
--dump-outputs DIR writes the rows of the last timed step as .npy files.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def log(*a):
    if int(os.environ.get("RANK", "0")) == 0:
        print("[bench]", *a, file=sys.stderr, flush=True)


class _DevArr:
    """zero-copy view of library-owned HBM for torch (ground truth only)"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


# Dry run of THIS SCRIPT's control flow without a GPU (tests/test_bench_dry_run.py): with VS_EMU=1 the library is the
# wave64 interpreter build of the same kernel sources (tests/emu/), "device" memory is host memory and torch stays on the
# CPU.  The JSON line then says so ("dry_run") and its numbers mean nothing; nothing else in this file depends on it.
EMU = bool(os.environ.get("VS_EMU"))


def _dev_tensor(torch, np, ptr, shape, dev, typestr="<f4"):
    if not EMU:
        return torch.as_tensor(_DevArr(ptr, shape, typestr), device=dev)
    count = int(shape[0]) * int(shape[1])
    ct = {"<f4": C.c_float, "<i4": C.c_int32}[typestr]
    return torch.from_numpy(np.ctypeslib.as_array((ct * count).from_address(int(ptr))).reshape(shape))


def graph_cache_path(args, n, dim, seed, bits, R):
    """Where the built neighbor array of this exact configuration is kept between runs (None = no cache)."""
    if args.graph_cache in (None, "", "none"):
        return None
    key = f"{n}x{dim}.{args.distance}.b{bits}.R{R}.L{args.build_l}.s{seed}" + ("" if getattr(args, "corpus", "lowrank") == "lowrank" else f".{args.corpus}") + (f".lab{args.labels}" if getattr(args, "labels", 0) else "")
    if args.graph_cache != "auto":
        return f"{args.graph_cache}.{key}"
    if n < 10_000_000:
        return None
    import hashlib
    import shutil
    import tempfile
    h = hashlib.sha1(kernel_source_hash().encode())
    h.update(open(os.path.join(ROOT, "pgvectorscale_amd", "datagen.py"), "rb").read())
    d = os.environ.get("TMPDIR") or tempfile.gettempdir()
    path = os.path.join(d, f"vs_graph_cache_{h.hexdigest()[:12]}.{key}")
    try:
        need = n * 64 * 4 * 2  # the padded neighbor array, twice (temporary + final name never coexist, but leave room)
        if not os.path.exists(path) and shutil.disk_usage(d).free < need + (8 << 30):
            return None
    except OSError:
        return None
    return path


def sample_rows(np, rows, row_bytes, budget):
    """row numbers to dump: all of them when they fit `budget` bytes, else a fixed (seed 0) sorted sample that does"""
    keep = max(1, budget // max(row_bytes, 1))
    if rows <= keep:
        return np.arange(rows)
    return np.sort(np.random.default_rng(0).choice(rows, size=keep, replace=False))


def kernel_source_hash():
    """12 hex digits over the device sources of libvsgpu and the host code that configures their launches (*.hip, *.h) — what a
    graph cache and a PMC measurement belong to; the host-only page / heap / broker readers (*.cpp) do not touch a kernel"""
    import hashlib
    h = hashlib.sha1()
    csrc = os.path.join(ROOT, "pgvectorscale_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")):
            h.update(open(os.path.join(csrc, f), "rb").read())
    return h.hexdigest()[:12]


def library_info(path, rebuilt):
    """which build of libvsgpu.so this process ran: its hash and age, the hash of the kernel sources beside it, and — with --rebuild —
    the compile that produced it on this box"""
    import hashlib
    try:
        st = os.stat(path)
        digest = hashlib.sha256(open(path, "rb").read()).hexdigest()[:12]
        return {"path": os.path.relpath(path, ROOT), "sha256_12": digest, "bytes": st.st_size,
                "built_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime(st.st_mtime)),
                "kernel_source_hash": kernel_source_hash(), "rebuilt_on_this_box": rebuilt}
    except OSError as e:
        return {"path": path, "error": repr(e)}


def usable_cores():
    """CPUs this process can really use: the affinity mask, capped by the cgroup CPU quota (a container on a 256-thread host
    is often limited to a few of them; os.cpu_count() reports the host)."""
    os_n = os.cpu_count() or 1
    try:
        aff = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        aff = os_n
    quota = None
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    quota = float(txt[0]) / float(txt[1])
            else:
                q_ = float(txt[0])
                if q_ > 0:
                    quota = q_ / float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read().split()[0])
            break
        except (OSError, ValueError, IndexError):
            continue
    usable = max(1, min(aff, int(quota + 0.5) if quota else aff))
    return {"os_cpu_count": os_n, "affinity": aff, "cgroup_quota": None if quota is None else round(quota, 2), "usable": usable}


def choose_operating_point(run_sample, k, target, sweep_log, err_type=Exception):
    """Cheapest (search_list_size, rescore) whose recall on the sample reaches `target`.

    Both knobs are the reference's query-time GUCs (diskann.query_search_list_size, diskann.query_rescore,
    AM/guc.rs:3-4).  Cost model of one scan: its MEASURED expansions (about 1.1 L before the first row + one per further
    row of the stream, M = rescore + k - 1 rows) plus one f32 row per stream entry for the rerank (about 0.12 of an
    expansion at 768 dims, from the kernel times of earlier runs).  Every grid point is tried on the recall sample (one
    launch of a thousand scans, milliseconds); the cheapest one that reaches the target is taken and its rescore is then
    bisected towards the next smaller grid value.  run_sample(L, S) -> (recall, stats dict).  Returns (L, S, recall);
    when nothing reaches the target, the point with the best recall."""
    tried = {}

    def cost_of(st, S):
        return st["visited_nodes"] / max(st["queries"], 1) + 0.12 * (S + k - 1 if S else k)

    def try_point(cl, cs):
        if (cl, cs) not in tried:
            try:
                r_, st_ = run_sample(cl, cs)
                tried[(cl, cs)] = (r_, cost_of(st_, cs))
                sweep_log.append((cl, cs, round(r_, 4)))
                log(f"recall sweep L={cl} rescore={cs}: recall@{k}={r_:.4f} cost={tried[(cl, cs)][1]:.1f}")
            except err_type as e:
                tried[(cl, cs)] = (0.0, float("inf"))
                log(f"L={cl} rescore={cs}: {e}")
        return tried[(cl, cs)]

    s_grid = [25, 50, 100, 200, 400]
    for cl in (3, 5, 10, 15, 25, 35, 50, 75, 100, 150, 200, 400):
        for cs in s_grid:
            r_, _ = try_point(cl, cs)
            if r_ >= target:
                break  # a larger rescore at this L only costs more
    ok = [(c_, p_) for p_, (r_, c_) in tried.items() if r_ >= target]
    if not ok:
        # nothing up to rescore 400 reaches the target (the `mid` corpus at 50M: 0.9876 at 400 / 400): the GUC goes to 1000
        # (AM/guc.rs:28-43), so the upper range is tried at the list sizes whose 400-row point came closest per unit of cost
        s_grid = s_grid + [600, 800, 1000]
        for cl in (3, 10, 50, 100):
            for cs in (600, 800, 1000):
                r_, _ = try_point(cl, cs)
                if r_ >= target:
                    break
        ok = [(c_, p_) for p_, (r_, c_) in tried.items() if r_ >= target]
    if not ok:
        (L, S), (rec, _) = max(tried.items(), key=lambda kv: kv[1][0])
        log(f"WARNING: recall target {target} not reached; using best L={L} rescore={S} ({rec:.4f})")
        return L, S, rec
    _, (L, S) = min(ok)
    lo = max([x for x in s_grid if x < S], default=0)  # the last grid value that failed at this L (or 0)
    while S - lo > max(4, S // 32):
        mid = (lo + S) // 2
        r_, _ = try_point(L, mid)
        if r_ >= target:
            S = mid
        else:
            lo = mid
    return L, S, tried[(L, S)][0]


def recall_stats(np, got, gt_ids, gt_ok):
    """recall@k of `got` [rows][k] against the exact top-k `gt_ids` (entries with gt_ok False do not exist: fewer than k rows
    satisfy a rare label key) -> {"recall": hits / wanted, "se": standard error of that ratio over the queries (the queries
    are the independent draws), "lower95": recall - 1.96 se, "queries": rows}."""
    got = np.asarray(got).astype(np.int64)
    gt = np.asarray(gt_ids).astype(np.int64)
    ok = np.asarray(gt_ok, bool)
    rows = gt.shape[0]
    if rows == 0:
        return {"recall": 0.0, "se": 0.0, "lower95": 0.0, "queries": 0}
    hit = ((got[:, :, None] == gt[:, None, :]) & ok[:, None, :]).any(axis=1).sum(axis=1).astype(np.float64)  # per query
    want = ok.sum(axis=1).astype(np.float64)
    tot = max(want.sum(), 1.0)
    rec = hit.sum() / tot
    # ratio estimator: Var(sum(hit) / sum(want)) ~ sum((hit - rec * want)^2) / tot^2
    se = float(np.sqrt(((hit - rec * want) ** 2).sum()) / tot) if rows > 1 else 0.0
    return {"recall": float(rec), "se": se, "lower95": float(rec - 1.96 * se), "queries": int(rows)}


def zipf_labels(np, rows, n_labels, seed, kmin, kmax):
    """Label sets for `rows` rows: kmin..kmax draws per row from n_labels labels (1-based) with Zipf(s = 1) frequencies,
    sorted and de-duplicated (LabelSet is a sorted set, AM/labels/mod.rs:15-37) -> (off[rows + 1] u32, val i16)."""
    rng = np.random.default_rng(seed)
    pz = 1.0 / np.arange(1, n_labels + 1)
    pz /= pz.sum()
    SENT = np.int16(32767)
    draws = (rng.choice(n_labels, size=(rows, kmax), p=pz) + 1).astype(np.int16)
    cnt = rng.integers(kmin, kmax + 1, size=rows)
    draws[np.arange(kmax)[None, :] >= cnt[:, None]] = SENT
    draws.sort(axis=1)
    dup = np.zeros_like(draws, dtype=bool)
    dup[:, 1:] = draws[:, 1:] == draws[:, :-1]
    draws[dup] = SENT
    draws.sort(axis=1)
    keep = draws != SENT
    off = np.zeros(rows + 1, np.uint32)
    np.cumsum(keep.sum(1), out=off[1:])
    return off, draws[keep]


def label_start_nodes(np, off, val):
    """first node carrying each label (the role of MetaPage start nodes per label, AM/graph/start_nodes.rs:39-48)"""
    owner = np.repeat(np.arange(off.size - 1, dtype=np.uint32), np.diff(off).astype(np.int64))
    labels, first = np.unique(val, return_index=True)
    return {int(l): int(owner[i]) for l, i in zip(labels, first)}


def label_masks(np, off, val):
    """one bit per label (n_labels <= 62) for the filtered ground truth"""
    assert (np.diff(off.astype(np.int64)) > 0).all()  # reduceat needs non-empty rows
    return np.bitwise_or.reduceat(np.int64(1) << val.astype(np.int64), off[:-1].astype(np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", "--corpus", dest="n", type=int, default=None,
                    help="corpus size (BASELINE configs: 1M / 10M / 50M).  Default with --full: the configuration BASELINE.json quotes "
                         "its metric on (50M x 768, L2): the whole index (177 GB) fits one MI355X; the on-device build takes "
                         "about 3 minutes of the run.  Default of a plain run: 4M, built in seconds.  --n 10000000 --distance cosine "
                         "is configs[2], --n 1000000 configs[1]")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, default=262144, help="queries per step per GPU (scans of one launch; a launch ends with a tail of "
                    "its last scans on a half-empty chip, which large batches amortise: 168.3 ms per 262144 scans against 2 x 88.2 ms per "
                    "131072 at 50M, profiles/r03/ab_nq262144_50m.txt)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything that is not needed for the headline value: the CPU baseline with its row-identity check "
                         "(unless --skip-cpu), the flat SBQ scan roofline (--scan-nq), the PCIe-inclusive leg (--pcie-steps) and the extras "
                         "(--extras), on the 50M corpus unless --n says otherwise.  Off by default: a plain run sets up, warms up, times "
                         "the steps and prints the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last timed step returned (rank 0's rows) to DIR/ids.npy (float64, [rows][k] "
                         "node ids) and DIR/distances.npy (float32, [rows][k]); at most 64 MB in all — of a larger block a fixed seeded "
                         "sample of the rows, their numbers in DIR/rows.npy (float64)")
    ap.add_argument("--scan-nq", type=int, default=64, help="with --full: queries of the flat SBQ scan (K5) roofline measurement, 0 = skip")
    ap.add_argument("--distance", default="l2", choices=["l2", "cosine", "ip"])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--recall-target", type=float, default=0.99)
    ap.add_argument("--recall-queries", type=int, default=1000, help="queries of the tuning sample (the operating-point grid runs on it)")
    ap.add_argument("--validate-queries", type=int, default=8192,
                    help="queries of the validation sample (disjoint from the tuning sample and from every timed batch): the operating "
                         "point is accepted only when the LOWER 95 %% confidence bound of recall@k on it reaches the target")
    ap.add_argument("--build-l", type=int, default=100)
    ap.add_argument("--fixed", default=None, help="L,rescore to use instead of the recall sweep")
    ap.add_argument("--skip-cpu", action="store_true", help="with --full: leave the CPU baseline out")
    ap.add_argument("--pipeline", type=int, default=1, choices=[1, 2],
                    help="batches in flight: 2 = the steps alternate between two views of the index (two streams), so the rerank of "
                         "a step runs under the search of the next one; the kernel times of the roofline then come from the "
                         "(sequential) warm-up steps")
    ap.add_argument("--graph-cache", default="auto",
                    help="file prefix to keep the built neighbor array in: loaded when present, written (by local rank 0) "
                         "after a build otherwise.  The build is deterministic and outside the timed region; the cache only "
                         "saves the minutes of rebuilding the same index in back-to-back runs on one box (N = 1, 2, 4, 8).  "
                         "'auto' (default): $TMPDIR/vs_graph_cache_<hash of the kernel sources> for n >= 10M when the "
                         "disk has room; 'none': always rebuild")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--parity-seconds", type=float, default=45.0,
                    help="the oracle re-runs a WHOLE step for the row-identity check when that takes at most this long at its measured rate")
    ap.add_argument("--heldout-queries", type=int, default=8192,
                    help="queries of the LAST TIMED batch whose exact top-k is computed (outside the timed region) so that the recall "
                         "of the timed results themselves is reported (recall_heldout); when it is below the target the rescore window "
                         "grows and ALL steps are timed again, so the printed value always belongs to results that meet the "
                         "target; 0 = skip")
    ap.add_argument("--corpus-kind", dest="corpus", default="lowrank", choices=["lowrank", "mid", "survey"],
                    help="lowrank (default): 1024 clusters in a 32-dimensional latent space projected to --dim, 10 %% isotropic noise "
                         "(intrinsic dimension ~32, like real text embeddings); mid: 1024 clusters in a 64-dimensional latent space, wider "
                         "clusters (intra 80 %%) and 30 %% isotropic noise — between 'a list of 3 suffices' and 'unsearchable'; survey: the mixture SURVEY.md 8(d) specifies — 1024 "
                         "cluster centres, isotropic full-rank spread with sigma_intra = 0.3 sigma_inter in all --dim dimensions "
                         "(distances concentrate: a much harder corpus for any ANN index)")
    ap.add_argument("--labels", type=int, default=0,
                    help="label-filtered scans (BASELINE configs[4]: --n 20000000 --dim 1536 --distance cosine --labels 32): every "
                         "vector carries 1-3 of this many labels (Zipf frequencies), query keys alternate between one and two "
                         "labels; ground truth is the exact filtered top-k")
    ap.add_argument("--latent-dim", type=int, default=0, help="override the corpus generator's latent dimension (1..128)")
    ap.add_argument("--noise-pct", type=int, default=-1, help="override the isotropic noise share (0..100)")
    ap.add_argument("--intra-pct", type=int, default=-1, help="override the within-cluster spread (0..100)")
    ap.add_argument("--pcie-steps", type=int, default=2,
                    help="with --full: steps of the PCIe-inclusive leg (queries start in pageable host memory, rows end there: vs_search_batch); "
                         "reported next to the value, never as the value; 0 = skip")
    ap.add_argument("--autotune", default="off", choices=["on", "off"],
                    help="off (default): the library's default launch variant — the one the committed rocprofv3 / PMC summaries under profiles/ "
                         "were taken on.  on: before the timed region the library times every exact launch variant of the search kernel on one "
                         "warm-up batch (vs_index_autotune: a variant must reproduce the default's rows, distance bits and counters on all "
                         "scans of that batch to qualify; the fastest qualified one is used when it beats the default by >= 3 %% twice), after "
                         "a child-process probe of the variants on a small index under a timeout (pgvectorscale_amd/tune_probe.py); the "
                         "line reports every candidate's time under `autotune`")
    ap.add_argument("--extras", default="auto", choices=["auto", "on", "off"],
                    help="with --full: three more objects in the JSON line, outside the headline value (N = 1 only): `cursor_pool` — 32 backend processes streaming "
                         "320 rows each through the shared-memory server, a cursor per scan against scan pools; `default_gucs` — the same index at the "
                         "reference's default GUCs (diskann.query_search_list_size = 100, diskann.query_rescore = 50, AM/guc.rs:3-4): QPS, "
                         "recall@k with its lower 95 %% bound, kernel fraction — and `harder_corpus` — a child run of this script on 10M vectors "
                         "of the `mid` corpus (its own operating point, QPS, recall bounds, CPU parity).  auto = on for the default workload "
                         "(50M, lowrank, no labels), off otherwise")
    ap.add_argument("--tune-reps", type=int, default=3, help="timed steps per variant (after one warm-up step each)")
    ap.add_argument("--probe-n", type=int, default=100_000, help="nodes of the probe child's index")
    ap.add_argument("--probe-timeout", type=float, default=240.0)
    ap.add_argument("--rebuild", action="store_true",
                    help="compile libvsgpu.so from its sources on THIS box first (make -B: every translation unit through hipcc "
                         "--offload-arch=gfx950), before anything is loaded; the line's `library` object says how long it took and "
                         "with which hipcc.  Off by default: the library travels prebuilt and the full build takes minutes of host time")
    args = ap.parse_args()
    if args.n is None:
        args.n = 50_000_000 if args.full else 4_000_000

    rebuilt = None
    if args.rebuild and int(os.environ.get("RANK", "0")) == 0 and not EMU:
        import subprocess
        t0 = time.time()
        csrc = os.path.join(ROOT, "pgvectorscale_amd", "csrc")
        jobs = max(2, min(usable_cores()["usable"], 16))
        subprocess.check_call(["make", "-C", csrc, "-B", "-s", f"-j{jobs}"])
        ver = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout.splitlines()
        rebuilt = {"seconds": round(time.time() - t0, 1), "hipcc": next((ln.strip() for ln in ver if "HIP version" in ln), None),
                   "command": "make -B (every *.hip through hipcc --offload-arch=gfx950)"}

    import numpy as np
    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        import torch.distributed as dist
        if EMU:
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    if EMU:
        from pgvectorscale_amd import _lib as _l
        _l.LIB_PATH = os.path.join(ROOT, "tests", "emu", "libvsgpu_emu.so")
        dev = torch.device("cpu")
        torch.cuda.synchronize = lambda *a_, **k_: None
    else:
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)

    import pgvectorscale_amd as P
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.datagen import DatagenParams, fill_device

    # ---- launch variants, step 1 (before this process owns anything on the device): every variant once in a CHILD process on a small
    # index of the same code width, under a timeout — a kernel that misbehaves there costs its variant, not this run
    tune = {"mode": args.autotune, "variant": "default", "probe": None, "candidates": None}
    tune_skip = None
    if args.autotune == "on":
        from pgvectorscale_amd import tune_probe
        t0 = time.time()
        pkw = dict(dim=args.dim, n=args.probe_n, nq=8192, device=local_rank, timeout=args.probe_timeout)
        if EMU:
            pkw.update(n=min(args.probe_n, 600), nq=16, rescore=20, build_l=20, device=0, lib=_l.LIB_PATH, timeout=900)
        tune_skip, prep = tune_probe.run(**pkw)
        tune["probe"] = {kk: prep.get(kk) for kk in ("ok", "error", "skip", "seconds", "index", "legs") if kk in prep}
        if prep.get("variants"):
            tune["probe"]["not_clean"] = {nm: v for nm, v in prep["variants"].items() if v["applicable"] and (not v["rows_identical"] or v["error"])}
        log(f"variant probe (child process, {time.time() - t0:.1f} s): {tune['probe']}")

    ctx = P.Context(0 if EMU else local_rank)
    log("device:", ctx.device_name())
    comm = None
    if world > 1:
        # N > 1: the data path runs behind the C ABI — vs_comm_* (RCCL over xGMI, loaded by libvsgpu itself) replicates the graph and
        # gathers the top-k blocks; torch.distributed only carries the launcher's control plane (this id, barriers, the timing
        # reductions).  CPU dry runs (VS_EMU) join the ranks with the stand-in RCCL of the test tier.
        import torch.distributed as dist
        from pgvectorscale_amd import multi as PM
        if EMU:
            os.environ.setdefault("VS_RCCL_LIB", os.path.join(ROOT, "tests", "emu", "libfakerccl.so"))
        # (the communicator is created by all ranks or by none: a rank where the library's RCCL cannot be loaded or initialised must not
        # leave the others waiting inside ncclCommInitRank, so the id travels only after every rank has reported that it can load it,
        # and a failure anywhere sends the whole job to the torch.distributed gather of pgvectorscale_amd/sharding.py — reported in
        # config.topk_gather, never silent)
        comm_err = None
        try:
            uid = [PM.comm_unique_id()]  # (every rank: it is also the probe that the library can load its RCCL here; rank 0's is used)
        except Exception as e:  # noqa: BLE001
            uid, comm_err = [None], repr(e)
        ok_ = torch.tensor([0 if comm_err else 1], dtype=torch.int32, device=dev)
        dist.all_reduce(ok_, op=dist.ReduceOp.MIN)
        if int(ok_.item()):
            dist.broadcast_object_list(uid, src=0)
            comm = PM.Comm(ctx, uid[0], rank, world)
        else:
            log(f"vs_comm unavailable on some rank ({comm_err}); the top-k gather and the graph broadcast fall back to torch.distributed")
    dt = {"l2": P.VS_L2, "cosine": P.VS_COSINE, "ip": P.VS_IP}[args.distance]
    n, dim, k = args.n, args.dim, args.k
    R = 50
    ix = P.DiskAnnIndex.alloc(ctx, n=n, dim_full=dim, num_neighbors=R, distance_type=dt)
    bits, W = ix.desc.bits, ix.desc.words
    seed = {1_000_000: 3, 10_000_000: 5, 50_000_000: 6}.get(n, 3)  # SURVEY.md 8(d) seeds
    gkw = {"lowrank": {}, "mid": dict(latent_dim=64, n_clusters=1024, intra_pct=80, noise_pct=30),
           "survey": dict(latent_dim=64, n_clusters=1024, intra_pct=0, noise_pct=30)}[args.corpus]
    if args.latent_dim:
        gkw["latent_dim"] = args.latent_dim
    if args.noise_pct >= 0:
        gkw["noise_pct"] = args.noise_pct
    if args.intra_pct >= 0:
        gkw["intra_pct"] = args.intra_pct
    gp = DatagenParams(seed=seed, dim=dim, **gkw)
    vecs_ptr, vstride = ix.array(_lib.ARR_VECS)

    setup = {}
    t0 = time.time()
    fill_device(ctx, gp, 0, n, vecs_ptr)
    ix.refresh_norms()
    setup["datagen_s"] = round(time.time() - t0, 3)
    t0 = time.time()
    ix.sbq_train()
    setup["sbq_train_s"] = round(time.time() - t0, 3)
    t0 = time.time()
    ix.sbq_quantize_corpus()
    setup["quantize_s"] = round(time.time() - t0, 3)
    NL = args.labels
    lab_off = lab_val = lab_starts = None
    if NL:
        assert 1 <= NL <= 62
        t0 = time.time()
        lab_off, lab_val = zipf_labels(np, n, NL, seed + 100, 1, 3)
        lab_starts = label_start_nodes(np, lab_off, lab_val)
        ix.set_labels(lab_off, lab_val)  # before the build: a labeled vector set is built label-aware (Graph::insert)
        setup["labels_s"] = round(time.time() - t0, 3)
    t0 = time.time()
    cache = graph_cache_path(args, n, dim, seed, bits, R)
    loaded = False
    if cache and os.path.exists(cache):
        try:
            ix.load_graph(cache)
            setup["graph_load_s"] = round(time.time() - t0, 3)
            loaded = True
        except Exception as e:  # a truncated / foreign file: rebuild
            log(f"graph cache {cache} unusable ({e!r}); rebuilding")
            t0 = time.time()
    rank0_has_graph = loaded
    if world > 1:  # one decision for all ranks: unless every rank found the cache, rank 0's array is broadcast
        import torch.distributed as dist
        t_ = torch.tensor([1 if loaded else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(t_, op=dist.ReduceOp.MIN)
        loaded = bool(int(t_.item()))
    if not loaded and world > 1:
        # N > 1: every rank holds the whole index, but only rank 0 builds it (3 minutes at 50M) — the neighbor array then goes
        # to the other ranks' HBM in one RCCL broadcast over xGMI (setup, outside the timed region; the build is deterministic,
        # so this is the array every rank would have built)
        import torch.distributed as dist
        if rank == 0 and not rank0_has_graph:
            ix.build_graph(search_list_size=args.build_l, max_alpha=1.2)
            setup["graph_build_s"] = round(time.time() - t0, 3)
        t1 = time.time()
        nptr, nstride = ix.array(_lib.ARR_NBRS)
        if comm is not None:
            comm.bcast(nptr, n * nstride * 4, 0)  # vs_comm_bcast: ncclBroadcast HBM -> HBM
            ctx.sync()
        else:
            nb = _dev_tensor(torch, np, nptr.value, (n, nstride), dev, "<i4")
            dist.broadcast(nb, src=0)
            torch.cuda.synchronize()
            del nb
        if rank != 0:
            ix.set_start_nodes(0)
        setup["graph_broadcast_s"] = round(time.time() - t1, 3)
    elif not loaded:
        ix.build_graph(search_list_size=args.build_l, max_alpha=1.2)
        setup["graph_build_s"] = round(time.time() - t0, 3)
    if not loaded and not rank0_has_graph:
        if cache and rank == 0:
            try:
                t1 = time.time()
                tmp = f"{cache}.tmp{os.getpid()}"
                ix.save_graph(tmp)
                os.replace(tmp, cache)
                setup["graph_cache_write_s"] = round(time.time() - t1, 3)
            except Exception as e:  # the cache is a convenience only
                log(f"graph cache not written: {e!r}")
                try:
                    os.remove(tmp)
                except OSError:
                    pass
    if NL:  # (a graph loaded from the cache carries no start nodes; after a build this repeats what the build set)
        ix.set_start_nodes(0, lab_starts)
    log("setup", setup)

    def query_keys(first_row, rows):
        """label keys of a query batch: one label (even rows) or two draws (odd rows) -> host CSR + device copies"""
        off, val = zipf_labels(np, rows, NL, seed + 200 + first_row % 1000003, 1, 2)
        # even rows keep their first label only
        cnt = np.diff(off.astype(np.int64))
        keep = np.ones(val.size, bool)
        two = np.nonzero((cnt == 2) & (np.arange(rows) % 2 == 0))[0]
        keep[off[two].astype(np.int64) + 1] = False
        cnt[two] = 1
        val = val[keep]
        off = np.zeros(rows + 1, np.uint32)
        np.cumsum(cnt, out=off[1:])
        d_val = ctx.alloc(max(val.size, 1) * 2)
        d_off = ctx.alloc((rows + 1) * 4)
        ctx.upload(d_val, np.ascontiguousarray(val, np.int16))
        ctx.upload(d_off, off)
        return off, val, d_val, d_off

    # ---- query batches resident in HBM (disjoint row range of the same stream) -------------------------------------
    nq = args.nq
    QBASE = 1 << 40
    n_batches = args.steps + args.warmup
    qbuf = [ctx.alloc(nq * dim * 4) for _ in range(n_batches)]
    for b in range(n_batches):
        fill_device(ctx, gp, QBASE + (rank * n_batches + b) * nq, nq, qbuf[b])
    qkeys = [query_keys((rank * n_batches + b) * nq, nq) for b in range(n_batches)] if NL else [None] * n_batches
    out_ids = torch.empty((nq, k), dtype=torch.int32, device=dev)  # u32 node ids (viewed as i32 for torch)
    out_dist = torch.empty((nq, k), dtype=torch.float32, device=dev)

    # ---- exact ground truth (torch matmul: plain library GEMM, not the product path) for three disjoint query sets:
    # "tune" (the operating point is searched on it), "validate" (the chosen point must hold there too, else the rescore
    # window grows) and "heldout" = the first rows of the LAST TIMED batch (only reported: recall of the timed results)
    nr = min(args.recall_queries, nq)
    nh = min(args.heldout_queries, nq)
    X = _dev_tensor(torch, np, vecs_ptr.value, (n, vstride), dev)[:, :dim]
    node_mask = torch.from_numpy(label_masks(np, lab_off, lab_val)).to(dev) if NL else None

    def ground_truth(q_ptr, rows, keys):
        """-> (ids [rows][k] int64, valid [rows][k] bool): exact (filtered) top-k of the first `rows` queries at q_ptr"""
        Qs = _dev_tensor(torch, np, q_ptr.value if hasattr(q_ptr, "value") else int(q_ptr), (rows, dim), dev)
        Qn = torch.nn.functional.normalize(Qs, dim=1) if dt == P.VS_COSINE else Qs
        best_d = torch.full((rows, k), float("inf"), device=dev)
        best_i = torch.zeros((rows, k), dtype=torch.int64, device=dev)
        q_mask = torch.from_numpy(label_masks(np, keys[0][:rows + 1], keys[1][:int(keys[0][rows])])).to(dev) if NL else None
        chunk = max(1 << 14, min(1 << 18, (1 << 29) // max(rows, 1)))
        for s0 in range(0, n, chunk):
            xc = X[s0:s0 + chunk]
            if dt == P.VS_L2:
                d = (xc * xc).sum(1)[None, :] - 2.0 * (Qn @ xc.T)
            elif dt == P.VS_COSINE:
                d = -(Qn @ torch.nn.functional.normalize(xc, dim=1).T)
            else:
                d = -(Qn @ xc.T)
            if NL:  # the predicate: the label sets overlap (AM/labels/mod.rs:124-142)
                d = d.masked_fill((node_mask[s0:s0 + chunk][None, :] & q_mask[:, None]) == 0, float("inf"))
            cd, ci = torch.topk(d, min(k, d.shape[1]), dim=1, largest=False)
            alld = torch.cat([best_d, cd], 1)
            alli = torch.cat([best_i, ci + s0], 1)
            sel = torch.topk(alld, k, dim=1, largest=False)
            best_d, best_i = sel.values, torch.gather(alli, 1, sel.indices)
        torch.cuda.synchronize()
        return best_i.cpu().numpy(), torch.isfinite(best_d).cpu().numpy()  # fewer than k rows may satisfy a rare key

    def recall_of(got, gt_ids, gt_ok):
        return recall_stats(np, got, gt_ids, gt_ok)["recall"]

    t0 = time.time()
    nv = max(1, min(args.validate_queries, nq))
    sets = {}
    for name, base, rows in (("tune", QBASE - (1 << 30), nr), ("validate", QBASE - (1 << 29), nv)):
        qp = ctx.alloc(rows * dim * 4)
        fill_device(ctx, gp, base, rows, qp)
        keys = query_keys(base, rows) if NL else None
        sets[name] = (qp, keys) + ground_truth(qp, rows, keys) + (rows,)
    held = None
    if nh:
        hb = n_batches - 1
        held = ground_truth(qbuf[hb], nh, qkeys[hb])
    setup["ground_truth_s"] = round(time.time() - t0, 3)
    if not EMU:
        torch.cuda.empty_cache()  # (the ground truth's temporaries go back to the device: the search workspace needs the room)
    del X
    if NL:
        del node_mask

    rq_ids = torch.empty((max(nr, nv), k), dtype=torch.int32, device=dev)

    def run_set(name, L, S):
        """-> (recall statistics of the set at this operating point, work counters)"""
        qp, keys, gt_ids, gt_ok, rows = sets[name]
        ix.search_batch_dev(qp, rows, L, S, k, C.c_void_p(rq_ids.data_ptr()), d_qlabels=keys and keys[2],
                            d_qlabel_off=keys and keys[3])
        st = ix.search_batch_dev_finish()
        return recall_stats(np, rq_ids[:rows].cpu().numpy().view(np.uint32), gt_ids, gt_ok), st

    def run_sample(L, S):
        rs, st = run_set("tune", L, S)
        return rs["recall"], st

    # ---- recall sweep: cheapest (L, rescore) reaching the target (choose_operating_point) --------------------------
    sweep_log = []
    if args.fixed:
        L, S = (int(x) for x in args.fixed.split(","))
        rec, st = run_sample(L, S)
        sweep_log.append((L, S, round(rec, 4)))
    else:
        L, S, rec = choose_operating_point(run_sample, k, args.recall_target, sweep_log, P.VsError)
    recall = rec
    # The point must hold on queries it was not searched on, and with statistical room: the LOWER 95 % bound of recall@k on the
    # validation sample (>= 8192 queries by default: one standard error is about 0.0003 there) has to reach the target; the
    # rescore window (diskann.query_rescore, README.md:382-394, AM/guc.rs:28-43) grows about 2 % a step until it does (a step costs
    # one launch of the validation sample, milliseconds; the window is the work of a query, so every step too many is QPS lost).
    val = run_set("validate", L, S)[0]
    sweep_log.append(("validate", L, S, round(val["recall"], 4), round(val["lower95"], 4)))
    bumps = 0
    while not args.fixed and val["lower95"] < args.recall_target and recall >= args.recall_target and bumps < 40 and S < 1000:
        S = min(1000, S + max(2, S // 48))
        bumps += 1
        recall, _ = run_sample(L, S)
        val = run_set("validate", L, S)[0]
        sweep_log.append(("validate", L, S, round(val["recall"], 4), round(val["lower95"], 4)))
    recall_validate = val["recall"]
    log(f"operating point: L={L} rescore={S} recall@{k}={recall:.4f} (tune, {nr} queries) {recall_validate:.4f} (validate, {nv} queries, "
        f"lower 95 % bound {val['lower95']:.4f}), {bumps} validation steps")

    def barrier():
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
        ctx.sync()
        torch.cuda.synchronize()

    # final top-k gather (the only collective on this path): vs_comm_gather_topk = one grouped ncclAllGather of the id and distance
    # blocks, enqueued on the context's stream behind the search that produced them; every rank ends a step with all world * nq rows
    gathered = None
    if world > 1:
        gathered = (torch.empty((world * nq, k), dtype=torch.int32, device=dev), torch.empty((world * nq, k), dtype=torch.float32, device=dev))

    def gather_topk(oi, od):
        n_ = oi.shape[0]
        if comm is None:  # (fallback, see above)
            from pgvectorscale_amd.sharding import gather_topk as torch_gather
            gi_, gd_ = torch_gather(oi, od)
            gathered[0][:gi_.shape[0]].copy_(gi_)
            gathered[1][:gd_.shape[0]].copy_(gd_)
            return
        comm.gather_topk(C.c_void_p(oi.data_ptr()), C.c_void_p(od.data_ptr()), n_, world * n_, k, C.c_void_p(gathered[0].data_ptr()),
                         C.c_void_p(gathered[1].data_ptr()))

    def step(b):
        ix.search_batch_dev(qbuf[b], nq, L, S, k, C.c_void_p(out_ids.data_ptr()), None, C.c_void_p(out_dist.data_ptr()),
                            d_qlabels=qkeys[b] and qkeys[b][2], d_qlabel_off=qkeys[b] and qkeys[b][3])
        st = ix.search_batch_dev_finish()  # waits for the kernels, checks overflow flags, sums the work counters
        if world > 1:  # final top-k gather over RCCL/xGMI (the only collective on this path)
            gather_topk(out_ids, out_dist)
        return st

    # a very wide operating point (a corpus on which the target is out of reach ends at L = 400 / rescore = 400) may not fit
    # 131072 scans into the workspace budget: halve the scans per step until a launch is accepted
    while True:
        try:
            step(0)
            break
        except P.VsError as e:
            if "workspace budget" not in str(e) or nq <= 1024:
                raise
            nq //= 2
            out_ids, out_dist = out_ids[:nq], out_dist[:nq]
            nh = min(nh, nq)
            log(f"{e}; continuing with {nq} scans per step")
    if world > 1:  # (once, untimed) the gathered block holds this rank's rows at this rank's place
        ctx.sync()
        torch.cuda.synchronize()
        assert torch.equal(gathered[0][rank * nq:(rank + 1) * nq], out_ids) and \
            torch.equal(gathered[1][rank * nq:(rank + 1) * nq].view(torch.int32), out_dist.view(torch.int32)), "top-k gather misplaced a shard"

    # --pipeline 2: two batches in flight — even steps through the index, odd steps through a view of it on a second context
    # (stream), each with its own output block; a step is collected after the next one has been submitted, so the bandwidth-bound
    # rerank of step i runs under the latency-bound search of step i + 1 and the step time tends to max(search, rerank + resort)
    # instead of their sum.  Kernel times are only meaningful when a kernel has the chip to itself, so the roofline's come from
    # sequential steps run right before the timed region (the warm-up steps), with the work counters that belong to them.
    pipe = {"ready": False}

    def pipe_setup():
        if not pipe["ready"]:
            pipe["ctx2"] = P.Context(0 if EMU else local_rank)
            pipe["ix2"] = ix.view(pipe["ctx2"])
            pipe["outs"] = [(out_ids, out_dist), (torch.empty_like(out_ids), torch.empty_like(out_dist))]
            pipe["lanes"] = [ix, pipe["ix2"]]
            pipe["ready"] = True

    def pipe_submit(b_):
        oi, od = pipe["outs"][b_ % 2]
        pipe["lanes"][b_ % 2].search_batch_dev(qbuf[b_], nq, L, S, k, C.c_void_p(oi.data_ptr()), None, C.c_void_p(od.data_ptr()),
                                               d_qlabels=qkeys[b_] and qkeys[b_][2], d_qlabel_off=qkeys[b_] and qkeys[b_][3])

    def pipe_collect(b_):
        st_ = pipe["lanes"][b_ % 2].search_batch_dev_finish()
        if world > 1:
            gather_topk(*pipe["outs"][b_ % 2])
        return st_

    def timed_pass():
        """W untimed steps, then exactly K timed steps between barriers -> (seconds (max over ranks), kernel profile, counters the
        profile belongs to, counters of the timed steps, the output block that holds the rows of the last timed step)"""
        last_out = (out_ids, out_dist)
        if args.pipeline == 1:
            for b_ in range(args.warmup):
                step(b_)
            ctx.profile_enable(True)
            ctx.profile_read(reset=True)
            tot_ = {}
            barrier()
            t0_ = time.perf_counter()
            for b_ in range(args.warmup, n_batches):
                st_ = step(b_)
                for kk, vv in st_.items():
                    tot_[kk] = tot_.get(kk, 0) + vv
            barrier()
            el_ = time.perf_counter() - t0_
            prof_ = ctx.profile_read(reset=True)
            ctx.profile_enable(False)
            ptot_ = tot_
        else:
            assert args.warmup >= 1, "--pipeline 2 takes the kernel times of the roofline from the warm-up steps"
            pipe_setup()
            pipe_submit(1 % n_batches)  # (the view sizes its launches from what its own first batch needed)
            pipe_collect(1 % n_batches)
            ctx.profile_enable(True)
            ctx.profile_read(reset=True)
            ptot_ = {}
            for b_ in range(args.warmup):
                st_ = step(b_)
                for kk, vv in st_.items():
                    ptot_[kk] = ptot_.get(kk, 0) + vv
            prof_ = ctx.profile_read(reset=True)
            ctx.profile_enable(False)
            tot_ = {}
            barrier()
            pipe["ctx2"].sync()
            t0_ = time.perf_counter()
            prev_ = None
            for b_ in range(args.warmup, n_batches):
                pipe_submit(b_)
                if prev_ is not None:
                    for kk, vv in pipe_collect(prev_).items():
                        tot_[kk] = tot_.get(kk, 0) + vv
                prev_ = b_
            for kk, vv in pipe_collect(prev_).items():
                tot_[kk] = tot_.get(kk, 0) + vv
            barrier()
            pipe["ctx2"].sync()
            el_ = time.perf_counter() - t0_
            last_out = pipe["outs"][(n_batches - 1) % 2]
        if world > 1:
            import torch.distributed as dist
            t_ = torch.tensor([el_], dtype=torch.float64, device=dev)
            dist.all_reduce(t_, op=dist.ReduceOp.MAX)
            el_ = float(t_.item())
        return el_, prof_, ptot_, tot_, last_out

    def heldout_stats(rows_t):
        """recall of the rows the LAST TIMED step produced (every rank checks its own batch; pooled over the ranks)"""
        hs_ = recall_stats(np, rows_t[:nh].cpu().numpy().view(np.uint32), held[0][:nh], held[1][:nh])
        if world > 1:
            import torch.distributed as dist
            t_ = torch.tensor([hs_["recall"], hs_["se"] ** 2], dtype=torch.float64, device=dev)
            dist.all_reduce(t_, op=dist.ReduceOp.SUM)
            rec_, se_ = float(t_[0]) / world, float(t_[1]) ** 0.5 / world
            hs_ = {"recall": rec_, "se": se_, "lower95": rec_ - 1.96 * se_, "queries": nh * world}
        return hs_

    # ---- launch variants, step 2: the variants the probe cleared, timed by the library on a warm-up batch of THIS index at THIS
    # operating point (all nq scans; rows, distance bits and counters held to the default's); the index keeps the fastest
    if args.autotune == "on" and tune_skip is not None:
        try:
            t0 = time.time()
            cand = ix.autotune(qbuf[0], nq, L, S, k, d_qlabels=qkeys[0] and qkeys[0][2], d_qlabel_off=qkeys[0] and qkeys[0][3],
                               reps=args.tune_reps, skip=tune_skip)
            tune["candidates"] = [c_ for c_ in cand if c_["applicable"] or c_["error"] or c_["name"] in tune_skip]
            tune["variant"] = ix.variant()
            tune["seconds"] = round(time.time() - t0, 2)
            log(f"autotune ({tune['seconds']} s): " + ", ".join(
                f"{c_['name']} {c_['step_ms']:.2f} ms" + ("" if c_["rows_identical"] else " (ROWS DIFFER: disqualified)") + (" <- chosen" if c_["chosen"] else "")
                for c_ in cand if c_["applicable"]))
        except Exception as e:  # noqa: BLE001 — the selection is an optimisation: whatever goes wrong, the default runs
            tune["error"] = repr(e)
            try:
                ix.search_batch_dev_finish()
            except Exception:  # noqa: BLE001
                pass
            ix.set_variant("default")
            tune["variant"] = "default"
            log(f"autotune failed ({e!r}); the library default is used")
    elif args.autotune == "on":
        log("the variant probe did not finish cleanly: no variant is launched in this process, the library default is used")

    # The printed value must belong to results that meet the target: when the rows of the timed steps themselves fall short
    # of it, the rescore window grows (as a user would raise diskann.query_rescore) and ALL K steps are timed again.
    try:  # what is left of the HBM with the index, every query batch and the sized workspace resident (how far --nq could grow)
        free_b, total_b = ctx.mem_info()
        setup["hbm_free_gb_at_timed_region"] = round(free_b / 1e9, 1)
        setup["hbm_total_gb"] = round(total_b / 1e9, 1)
    except Exception:  # noqa: BLE001
        pass
    K = args.steps
    retimed = 0
    hs = None
    while True:
        elapsed, prof, ptot, tot, (last_ids, last_dist) = timed_pass()
        if held is None:
            break
        hs = heldout_stats(last_ids)
        log(f"recall@{k} of the timed results (first {nh} queries of the last timed batch" + (f", x{world} ranks" if world > 1 else "")
            + f"): {hs['recall']:.4f} (lower 95 % bound {hs['lower95']:.4f}) at L={L} rescore={S}")
        # (accepted on the LOWER 95 % bound of the timed rows, like the validation set: a point estimate 0.0004 above the target
        # is not a met target)
        if hs["lower95"] >= args.recall_target or args.fixed or S >= 1000 or retimed >= 12 or recall < args.recall_target:
            break
        S = min(1000, S + max(2, S // 32))
        retimed += 1
        log(f"below the target: rescore -> {S}, timing all {K} steps again")
    if retimed:  # the reported tuning / validation recalls belong to the final point
        recall = run_sample(L, S)[0]
        val = run_set("validate", L, S)[0]
        recall_validate = val["recall"]
        sweep_log.append(("retimed", L, S, round(val["recall"], 4), round(val["lower95"], 4)))
    qps = world * nq * K / elapsed
    recall_heldout = None if hs is None else hs["recall"]
    if args.dump_outputs and rank == 0:  # what a caller of the timed path received from its last step
        os.makedirs(args.dump_outputs, exist_ok=True)
        ids_h = last_ids.cpu().numpy().view(np.uint32)
        dist_h = last_dist.cpu().numpy()
        keep = sample_rows(np, ids_h.shape[0], k * (8 + 4) + 8, 64 * 1000 * 1000)
        np.save(os.path.join(args.dump_outputs, "ids.npy"), ids_h[keep].astype(np.float64))
        np.save(os.path.join(args.dump_outputs, "distances.npy"), dist_h[keep].astype(np.float32))
        if keep.size < ids_h.shape[0]:
            np.save(os.path.join(args.dump_outputs, "rows.npy"), keep.astype(np.float64))

    # ---- roofline of the dominant kernel (k_search_fast): algorithmic bytes = visits*4R + d_quantized*8W of the scans
    # it completed (the few scans handed to the general kernel are accounted to "search_fallback") -------------------
    s_ms, s_n = prof["search"]
    f_ms, f_n = prof["search_fallback"]
    r_ms, r_n = prof["rerank"]
    # (ptot: the counters of the steps the kernel profile was taken over — the timed steps, or with --pipeline 2 the sequential
    # warm-up steps)
    fb_bytes = ptot.get("fallback_visited_nodes", 0) * 4 * R + ptot.get("fallback_quantized_distance_comparisons", 0) * 8 * W
    alg_bytes_search = ptot["visited_nodes"] * 4 * R + ptot["quantized_distance_comparisons"] * 8 * W - fb_bytes
    if NL:  # + the label set of every evaluated neighbor, 2 bytes per label (mean set size of this index)
        alg_bytes_search += int(ptot["quantized_distance_comparisons"] * 2 * (lab_val.size / n))
    alg_bytes_rerank = ptot["full_distance_comparisons"] * 4 * dim
    per_launch = alg_bytes_search / max(s_n, 1)
    avg_ms = s_ms / max(s_n, 1)
    achieved = per_launch / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
    # HBM bytes per launch from the TCC counters (scripts/pmc_traffic.sh: two rocprofv3 --pmc passes over this very script;
    # rocprofv3 cannot run inside this process): taken from the committed measurement of the same corpus / launch size /
    # operating point, and `traffic_source` says which file, which commit wrote it and whether the kernel sources it was
    # measured on are the ones of this build (hash over csrc/, the same one the graph cache uses).
    import glob
    traffic = None
    traffic_source = None
    traffic_ref = None  # the committed PMC measurement of the same corpus / launch size at another operating point
    src_hash = kernel_source_hash()
    for pmc_path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r0[3-9]", "pmc_search_traffic*.json"))):
        try:
            pj = json.load(open(pmc_path))
            if pj.get("n") == n and pj.get("nq") == nq and pj.get("dim", 768) == dim and bool(pj.get("labels", 0)) == bool(NL):
                src = {"file": os.path.relpath(pmc_path, ROOT), "commit": pj.get("commit"),
                       "kernel_source_hash": pj.get("kernel_source_hash"),
                       "same_kernel_sources_as_this_build": pj.get("kernel_source_hash") == src_hash,
                       "search_list_size": pj.get("L"), "rescore": pj.get("rescore")}
                src["variant"] = pj.get("variant", "default")
                if pj.get("L") == L and pj.get("rescore") == S and src["variant"] == tune["variant"]:
                    traffic = pj.get("hbm_bytes_per_launch")
                    traffic_source = src
                else:
                    traffic_ref = dict(src, hbm_bytes_per_launch=pj.get("hbm_bytes_per_launch"),
                                       alg_bytes_per_launch=pj.get("alg_bytes_per_launch"))
        except Exception:
            pass
    roofline = {"bound": "hbm", "kernel": "k_search_fast", "variant": tune["variant"], "achieved": round(achieved, 2), "peak": 8000.0, "unit": "GB/s",
                "frac": round(achieved / 8000.0, 5), "traffic": traffic, "traffic_source": traffic_source,
                "traffic_other_operating_point": traffic_ref,
                "alg_bytes_per_launch": int(per_launch), "avg_kernel_ms": round(avg_ms, 4), "launches": s_n,
                "scans_per_launch": nq, "kernel_ms_per_131072_scans": round(avg_ms * 131072 / max(nq, 1), 4),
                "alg_bytes_per_query": round(alg_bytes_search / max(ptot.get("queries", 1) - ptot.get("fallback_scans", 0), 1), 1),
                "timed_over": ("the timed steps" + ("" if traffic is None else
                               f"; `traffic` is NOT measured in this run (rocprofv3 cannot run inside it): it is read from {traffic_source['file']}, two "
                               f"--pmc passes over this script at this operating point on kernel sources with "
                               f"{'the same' if traffic_source['same_kernel_sources_as_this_build'] else 'ANOTHER'} hash as this build")) if args.pipeline == 1 else
                              f"{args.warmup} sequential warm-up steps (the timed steps overlap two batches: a kernel's duration there "
                              "includes the other stream's kernels)"}
    kernels = {name: {"ms_total": round(ms, 3), "launches": cnt} for name, (ms, cnt) in prof.items() if cnt}
    if r_ms > 0:
        kernels["rerank"]["achieved_GBps"] = round(alg_bytes_rerank / (r_ms * 1e-3) / 1e9, 2)
    if f_n and f_ms > 0:
        kernels["search_fallback"]["scans"] = ptot.get("fallback_scans", 0)

    # ---- K5: the flat SBQ scan (same codes, streamed instead of gathered): the bandwidth-bound form of the candidate scan
    # at every tile size of the kernel (VS_SCAN_Q = 4, 8, 16 queries per pass over the codes): bytes per launch fall with the
    # tile, so GB/s and queries/s pull in opposite directions — all three are reported, "fastest_per_query" names the tile a
    # caller should use, and the roofline entry of the metric ("SBQ-scan achieved HBM GB/s") is the one with the best GB/s.
    scan_roofline = None
    if args.full and args.scan_nq > 0 and rank == 0:
        try:
            qh_s = ctx.download(qbuf[0], np.empty((nq, dim), np.float32))[:args.scan_nq]
            if dt == P.VS_COSINE:
                qh_s = qh_s / np.linalg.norm(qh_s, axis=1, keepdims=True)
            qcodes = ix.quantize(qh_s)
            prev_q = P.get_option("VS_SCAN_Q")
            tiles_tried = []
            for qt in ((4, 8, 16) if prev_q is None else (int(prev_q),)):
                P.set_option("VS_SCAN_Q", qt)  # (through the C ABI: vs_set_option)
                ix.scan_topk(qcodes, k)  # warm-up
                ctx.profile_enable(True)
                ctx.profile_read(reset=True)
                for _ in range(5):
                    ix.scan_topk(qcodes, k)
                sp = ctx.profile_read(reset=True)
                ctx.profile_enable(False)
                sc_ms = sp["scan"][0] / max(sp["scan"][1], 1)
                tiles = (args.scan_nq + qt - 1) // qt
                cs = W + (W & 1)
                sc_bytes = tiles * n * 8 * cs
                sc_gbps = sc_bytes / (sc_ms * 1e-3) / 1e9
                tiles_tried.append({"queries_per_tile": qt, "tiles": tiles, "avg_kernel_ms": round(sc_ms, 4),
                                    "alg_bytes_per_launch": int(sc_bytes), "achieved": round(sc_gbps, 1),
                                    "frac": round(sc_gbps / 8000.0, 4),
                                    "queries_per_s": round(args.scan_nq / (sc_ms * 1e-3), 1)})
            if prev_q is None:
                P.set_option("VS_SCAN_Q", None)
            top = max(tiles_tried, key=lambda t: t["achieved"])
            fastest = min(tiles_tried, key=lambda t: t["avg_kernel_ms"])
            scan_roofline = {"bound": "hbm", "kernel": "k_scan_topk", "achieved": top["achieved"], "peak": 8000.0,
                             "unit": "GB/s", "frac": top["frac"], "traffic": None,
                             "alg_bytes_per_launch": top["alg_bytes_per_launch"], "avg_kernel_ms": top["avg_kernel_ms"],
                             "queries": args.scan_nq, "queries_per_tile": top["queries_per_tile"], "tiles": top["tiles"],
                             "by_tile": tiles_tried, "fastest_per_query": fastest["queries_per_tile"],
                             "note": "codes streamed once per tile of queries; exact (hamming, id) top-k; the headline entry is the "
                                     "tile with the best GB/s, 'fastest_per_query' the one with the fewest ms for the same queries"}
        except Exception as e:
            scan_roofline = {"error": repr(e)}

    # ---- PCIe-inclusive leg (never the value): the same step through the host-pointer entry point (vs_search_batch: queries
    # from pageable host memory through the pinned staging ring, rows back to the host)
    pcie = None
    if args.full and args.pcie_steps > 0 and rank == 0 and not NL:
        try:
            qh_p = ctx.download(qbuf[args.warmup], np.empty((nq, dim), np.float32))
            # one untimed step of the full size first, as the device-resident path gets its warm-up steps: the chunk pipeline's own
            # buffers (two query chunks, two row blocks) are allocated by the first call that needs them — the 1 024-query warm-up of
            # round 3 left that to the first timed step (-10 % where an A/B of the same entry point measured -5 %)
            ix.search_batch(qh_p, search_list_size=L, rescore=S, k=k)
            t1 = time.perf_counter()
            for _ in range(args.pcie_steps):
                ix.search_batch(qh_p, search_list_size=L, rescore=S, k=k)
            pt = (time.perf_counter() - t1) / args.pcie_steps
            pcie = {"value": round(nq / pt, 1), "unit": "queries/s", "ms_per_step": round(pt * 1e3, 3), "steps": args.pcie_steps,
                    "h2d_bytes_per_step": nq * dim * 4, "d2h_bytes_per_step": nq * k * 16,
                    "note": "vs_search_batch on host numpy buffers (pageable -> pinned ring -> HBM, rows copied back); one GPU, "
                            "rank 0; the headline value starts with the queries in HBM"}
            del qh_p
        except Exception as e:
            pcie = {"error": repr(e)}

    # ---- extras (never the value): the same index at the reference's DEFAULT GUCs (AM/guc.rs:3-4: search_list_size 100, rescore 50)
    extras_on = args.full and world == 1 and (args.extras == "on" or (args.extras == "auto" and n == 50_000_000 and args.corpus == "lowrank" and not NL
                                                         and dim == 768 and not args.fixed))
    default_gucs = None
    if extras_on and ix.desc.storage_type == _lib.VS_STORAGE_SBQ:
        try:
            Ld, Sd = 100, 50
            vd = run_set("validate", Ld, Sd)[0]

            def step_at(b_, L_, S_):
                ix.search_batch_dev(qbuf[b_], nq, L_, S_, k, C.c_void_p(out_ids.data_ptr()), None, C.c_void_p(out_dist.data_ptr()),
                                    d_qlabels=qkeys[b_] and qkeys[b_][2], d_qlabel_off=qkeys[b_] and qkeys[b_][3])
                return ix.search_batch_dev_finish()

            step_at(0, Ld, Sd)  # (sizes the launch from this point's own statistics)
            step_at(0, Ld, Sd)
            ctx.profile_enable(True)
            ctx.profile_read(reset=True)
            dsteps = min(2, n_batches)
            dtot = {}
            barrier()
            t1 = time.perf_counter()
            for b_ in range(dsteps):
                for kk, vv in step_at(n_batches - 1 - b_, Ld, Sd).items():
                    dtot[kk] = dtot.get(kk, 0) + vv
            barrier()
            d_el = time.perf_counter() - t1
            dprof = ctx.profile_read(reset=True)
            ctx.profile_enable(False)
            d_ms, d_n = dprof["search"]
            d_bytes = dtot["visited_nodes"] * 4 * R + dtot["quantized_distance_comparisons"] * 8 * W - (
                dtot.get("fallback_visited_nodes", 0) * 4 * R + dtot.get("fallback_quantized_distance_comparisons", 0) * 8 * W)
            d_ach = d_bytes / max(d_n, 1) / (d_ms / max(d_n, 1) * 1e-3) / 1e9 if d_ms > 0 else 0.0
            dh = None
            if held is not None and dsteps >= 1:  # (the last batch ran first: its rows are gone; the check runs it once more)
                step_at(n_batches - 1, Ld, Sd)
                dh = recall_stats(np, out_ids[:nh].cpu().numpy().view(np.uint32), held[0][:nh], held[1][:nh])
            default_gucs = {"search_list_size": Ld, "rescore": Sd, "value": round(nq * dsteps / d_el, 1), "unit": "queries/s",
                            "steps": dsteps, "ms_per_step": round(d_el / dsteps * 1e3, 3),
                            "recall_validate": round(vd["recall"], 4), "recall_validate_lower95": round(vd["lower95"], 4),
                            "recall_timed_rows": None if dh is None else round(dh["recall"], 4),
                            "recall_timed_rows_lower95": None if dh is None else round(dh["lower95"], 4),
                            "recall_target_met": bool(min(vd["lower95"], 1.0 if dh is None else dh["lower95"]) >= args.recall_target),
                            "roofline": {"kernel": "k_search_fast", "achieved": round(d_ach, 2), "peak": 8000.0, "unit": "GB/s",
                                         "frac": round(d_ach / 8000.0, 5), "avg_kernel_ms": round(d_ms / max(d_n, 1), 4), "launches": d_n,
                                         "alg_bytes_per_launch": int(d_bytes / max(d_n, 1))},
                            "work_per_query": {kk: round(vv / max(dtot.get("queries", 1), 1), 2) for kk, vv in dtot.items() if kk != "queries"},
                            "note": "the reference's default query GUCs (AM/guc.rs:3-4) on the index and query batches of the headline run; "
                                    "not the operating point the value is quoted at"}
            log(f"default GUCs (L=100 / rescore=50): {default_gucs['value']:.0f} QPS, recall {vd['recall']:.4f} (lower {vd['lower95']:.4f}), "
                f"kernel frac {default_gucs['roofline']['frac']}")
        except Exception as e:  # noqa: BLE001 — an extra never costs the headline line
            default_gucs = {"error": repr(e)}
            try:
                ix.search_batch_dev_finish()
            except Exception:  # noqa: BLE001
                pass

    # ---- extras (never the value): the amgettuple continuations of many backends at once — 32 backend PROCESSES stream 320 rows each
    # through the shared-memory server (the first chunk of a scan out of a shared launch, the rest by cursor requests), with a cursor per
    # scan on the dispatcher thread and out of scan pools (vs_scanpool.cpp: the requests of one dispatcher round share their launches)
    cursor_pool = None
    if extras_on and ix.desc.storage_type == _lib.VS_STORAGE_SBQ:
        try:
            from pgvectorscale_amd.shm_clients import stream_many
            nb, rows_each, chunk = (32, 320, 16) if not EMU else (3, 48, 16)
            qh_c = ctx.download(qbuf[0], np.empty((nq, dim), np.float32))[:nb]
            cursor_pool = {"backends": nb, "rows_per_scan": rows_each, "chunk": chunk, "search_list_size": 100, "rescore": 50}
            ref_rows = None
            for mode, kw in (("cursor_per_scan", dict(cursor_pool=0)), ("scan_pools", dict(cursor_pool=nb))):
                shm_name = f"/vs_bench_cp_{os.getpid()}_{mode}"
                srv = P.ShmServer(ix, shm_name, nslots=nb, kmax=chunk, max_batch=256, max_wait_us=100, **kw)
                try:
                    # (three passes each, the fastest counts: one pass is 32 processes woken 20 times each on 16 host cores, and a single
                    # late wake-up costs a whole dispatcher round — s29 measured 18.7 ms where four other sessions measured 11.0-11.1)
                    ones = [stream_many(shm_name, _lib.LIB_PATH, [qh_c[0]], 100, 50, rows_each, chunk, timeout=240) for _ in range(3)]
                    alls = [stream_many(shm_name, _lib.LIB_PATH, [qh_c[t] for t in range(nb)], 100, 50, rows_each, chunk, timeout=240)
                            for _ in range(3)]
                finally:
                    srv.close()
                wall1, out1 = min(ones, key=lambda r_: r_[0])
                walln, outn = min(alls, key=lambda r_: r_[0])
                if ref_rows is None:
                    ref_rows = outn
                cursor_pool[mode] = {"one_scan_ms": round(wall1, 2), "all_scans_ms": round(walln, 2), "ratio": round(walln / max(wall1, 1e-9), 2),
                                     "passes_ms": {"one_scan": [round(r_[0], 2) for r_ in ones], "all_scans": [round(r_[0], 2) for r_ in alls]},
                                     "rows_identical_to_cursor_per_scan": bool(all(r_[1] == ref_rows for r_ in alls) and
                                                                               all(r_[1][0] == ref_rows[0] for r_ in ones))}
            log(f"cursor continuations of {nb} backends: {cursor_pool['cursor_per_scan']['all_scans_ms']} ms with a cursor per scan, "
                f"{cursor_pool['scan_pools']['all_scans_ms']} ms out of scan pools (one scan: {cursor_pool['scan_pools']['one_scan_ms']} ms)")
        except Exception as e:  # noqa: BLE001 — an extra never costs the headline line
            cursor_pool = {"error": repr(e)}

    # ---- extras (never the value): LATENCY of `LIMIT k` scans, the quantity the reference's own claims are about (p95 latency and
    # throughput ratios, /root/reference/README.md:17-21; a scan = amrescan + k amgettuple calls, AM/scan.rs:335-436).  N backend PROCESSES —
    # plain C clients of the shared-memory server (pgvectorscale_amd/vs_shm_lat: no HIP, no device context, as a PostgreSQL backend) — run
    # scans in a closed loop at 1 / 8 / 64 / 512 backends: p50 / p95 / p99 per scan and scans/s, at the reference's default GUCs and at the
    # operating point of the headline value, the same 4096 queries at every level; the oracle's single-thread latency on the same
    # queries is added by the cpu_baseline leg below
    latency = None
    if extras_on and ix.desc.storage_type == _lib.VS_STORAGE_SBQ:
        try:
            import subprocess
            import tempfile
            lat_bin = os.path.join(ROOT, "pgvectorscale_amd", "vs_shm_lat")
            total = 4096 if not EMU else 12
            levels = (1, 8, 64, 512) if not EMU else (1, 3)
            qh_l = ctx.download(qbuf[0], np.empty((nq, dim), np.float32))[:total]
            total = len(qh_l)
            qf = tempfile.NamedTemporaryFile(prefix="vs_lat_q_", suffix=".f32", dir="/dev/shm" if os.path.isdir("/dev/shm") else None, delete=False)
            qf.write(np.ascontiguousarray(qh_l).tobytes())
            qf.close()
            shm_name = f"/vs_bench_lat_{os.getpid()}"
            latency = {"k": k, "scans_per_level": total, "gather_window_us": 50,
                       "transport": "vs_shm_* (POSIX shared memory + futex; the dispatcher groups the scans posted within the gather window into one "
                                    "launch); backends are processes (vs_shm_lat), closed loop, two untimed warm-up scans each",
                       "points": {}}
            srv = P.ShmServer(ix, shm_name, nslots=max(levels), kmax=max(k, 16), max_batch=512, max_wait_us=50)
            try:
                for pname, Lp, Sp in (("default_gucs", 100, 50), ("operating_point_of_the_value", L, S)):
                    rows_ = []
                    for nb_ in levels:
                        reps_ = max(total // nb_, 1)
                        cp = subprocess.run([lat_bin, shm_name, qf.name, str(dim), str(total), str(nb_), str(reps_), str(Lp), str(Sp), str(k)],
                                            capture_output=True, text=True, timeout=300)
                        line = [ln for ln in cp.stdout.splitlines() if ln.startswith("{")]
                        rows_.append(json.loads(line[-1]) if line else {"backends": nb_, "error": (cp.stderr or "no output")[-200:]})
                    cs = {r_.get("ids_checksum") for r_ in rows_ if r_.get("scans_per_backend", 0) * r_.get("backends", 0) == total}
                    latency["points"][pname] = {"search_list_size": Lp, "rescore": Sp, "levels": rows_, "same_rows_at_every_level": len(cs) <= 1}
            finally:
                srv.close()
                os.unlink(qf.name)
            p1 = latency["points"]["default_gucs"]["levels"]
            log("latency of LIMIT %d scans at the default GUCs: " % k + ", ".join(
                f"{r_.get('backends')} backends p50 {r_.get('p50_us', 0) / 1e3:.2f} / p95 {r_.get('p95_us', 0) / 1e3:.2f} ms ({r_.get('scans_per_s', 0):.0f}/s)" for r_ in p1))
        except Exception as e:  # noqa: BLE001 — an extra never costs the headline line
            latency = {"error": repr(e)}

    result = {
        "metric": f"QPS at recall@{k}>={args.recall_target:g}",
        "value": round(qps, 1),
        "unit": "queries/s",
        "n_gpus": world,
        "steps": K,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / K * 1e3, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u64 xor+popcount (SBQ) / f32 (rerank)",
        "data": "synthetic" if not EMU else "synthetic (DRY RUN on the wave64 interpreter: no GPU, numbers meaningless)",
        "config": {"corpus": f"{args.corpus}: {gp.n_clusters} clusters in a {gp.latent_dim}-dim latent space (within-cluster spread "
                             f"{gp.intra_pct} % of the centre spread) projected to all dims + {gp.noise_pct} % isotropic noise, unit norm"
                             + (" (the mixture SURVEY.md 8(d) specifies: distances concentrate)" if args.corpus == "survey" else ""),
                   "workload": f"{n}x{dim} synthetic clustered unit-norm f32, diskann index (SBQ {bits} bit, R={R}), "
                               f"{args.distance}, top-{k}" + (f", label-filtered scans ({NL} labels, Zipf, 1-3 per vector, keys of one / "
                                                             f"two labels; label-aware build: filtered + unfiltered insert pass, per-label start nodes)" if NL else ""),
                   "labels": NL, "n": n, "dim": dim, "bits": bits, "words": W,
                   "num_neighbors": R, "queries_per_step_per_gpu": nq, "search_list_size": L, "rescore": S, "k": k,
                   "parallelism": f"query-sharded x{world}, index replicated" if world > 1 else "single GPU",
                   "topk_gather": None if world == 1 else ("vs_comm_gather_topk (libvsgpu C ABI: one grouped ncclAllGather of the id + distance blocks per step)" if comm is not None
                                                            else "torch.distributed all_gather_into_tensor (FALLBACK: vs_comm_* could not be initialised on every rank)"),
                   "batches_in_flight": args.pipeline,
                   "workspace": "library default (the persistent grid's dedup tables + heap spill arrays sub-allocated from the index's "
                                "grow-only slab inside libvsgpu, chosen among probed candidates: VS_WS_SLAB_MB, VS_WS_SLAB_CANDIDATES)"},
        "recall_at_k": round(recall, 4),
        "recall_validate": round(recall_validate, 4),
        "recall_heldout": None if recall_heldout is None else round(recall_heldout, 4),
        "recall_heldout_queries": nh * world if recall_heldout is not None else 0,
        "recall_heldout_lower95": None if hs is None else round(hs["lower95"], 4),
        "recall_tune_queries": nr,
        "recall_validate_queries": nv,
        "recall_validate_lower95": round(val["lower95"], 4),
        "retimed_after_heldout_check": retimed,
        # met = the timed rows themselves reach the target, and so do the tuning sample and the LOWER 95 % bound of the
        # validation sample
        "recall_target_met": bool(min(recall, val["lower95"], 1.0 if hs is None else hs["lower95"]) >= args.recall_target),
        "recall_sweep": sweep_log,
        "roofline": roofline,
        "sbq_scan_roofline": scan_roofline,
        "pcie_inclusive": pcie,
        "kernels": kernels,
        "autotune": tune,
        "work_per_query": {kk: round(vv / max(tot.get("queries", 1), 1), 2) for kk, vv in tot.items() if kk != "queries"},
        "setup_s": setup,
        "library": library_info(_lib.LIB_PATH, rebuilt),
        "default_gucs": default_gucs,
        "cursor_pool": cursor_pool,
        "latency": latency,
        "harder_corpus": None,
    }

    # ---- CPU baseline: the oracle (port of the reference path on flat arrays) on the host cores --------------------
    if args.full and rank == 0 and world == 1 and not args.skip_cpu:
        try:
            from oracle import oracle_py as O
            O.build()
            t0 = time.time()
            host = ix.download(vecs=True)
            mean, m2, cnt = ix.get_quantizer()
            oidx = O.OracleIndex(codes=host["codes"], nbrs=host["nbrs"], heap_tids=host["heap_tids"], vecs=host["vecs"],
                                 mean=mean, m2=m2, count=cnt, bits=bits, dim_index=dim, num_neighbors=R,
                                 distance_type=dt, default_start=ix.desc.default_start, label_off=lab_off, label_val=lab_val,
                                 label_starts=lab_starts)
            hk = None
            if NL:
                ko, kv = qkeys[args.warmup][0], qkeys[args.warmup][1]
                hk = [kv[ko[i]:ko[i + 1]].tolist() for i in range(nq)]
            cores = usable_cores()
            qh = ctx.download(qbuf[args.warmup], np.empty((nq, dim), np.float32))
            log(f"cpu_baseline: index on host in {time.time() - t0:.1f}s, {cores['usable']} usable cores "
                f"(os.cpu_count {cores['os_cpu_count']}, affinity {cores['affinity']}, cgroup quota {cores['cgroup_quota']})")

            def cpu_run(rows, threads):
                t1 = time.time()
                r_ = oidx.search_batch(qh[:rows], L=L, rescore=S, k=k, threads=threads, qlabels=hk and hk[:rows])
                return time.time() - t1, r_

            # single-thread latency first (the reference is one backend per query, AM/mod.rs:63), then a thread sweep: the
            # budget (--cpu-seconds) is split over the points, each point runs enough queries for about its share
            # (round 6: an untimed warm pass first, then 512 queries — the 48 cold queries of round 5 put the single-thread rate 30 % below
            # the thread sweep's own one-thread point and `consistent` came out false)
            cpu_run(min(nq, 64), 1)
            one = min(nq, 512)
            t_one, _ = cpu_run(one, 1)
            cpu1 = t_one / one
            points = []
            tcount = 1
            while tcount < cores["usable"]:
                points.append(tcount)
                tcount *= 2
            points.append(cores["usable"])
            if cores["os_cpu_count"] > cores["usable"]:
                points.append(cores["os_cpu_count"])  # oversubscribed: what "one thread per visible CPU" gives on this box
            share = args.cpu_seconds / (len(points) + 1)
            sweep = []
            best = None
            for tc in points:
                rows = int(max(min(nq, 2 * tc), min(nq, share * tc * 0.7 / max(cpu1, 1e-9))))
                dt_, r_ = cpu_run(rows, tc)
                sweep.append({"threads": tc, "queries": rows, "qps": round(rows / dt_, 1)})
                if best is None or rows / dt_ > best[0]:
                    best = (rows / dt_, tc, rows, r_)
            cpu_qps, cpu_threads, sample, (o_ids, o_dist, o_st) = best
            cpu1 = min(cpu1, 1.0 / max(sweep[0]["qps"], 1e-9))  # (the first probe runs on cold caches: the sweep's one-thread point counts too)
            # the final sample for the parity check, at the best thread count: the WHOLE step when the oracle gets through it within
            # --parity-seconds at the rate just measured (50M x 768: 262 144 scans in about 20 s on 16 cores), else at least 2048 rows
            sample = int(min(nq, max(sample, 2048)))
            if nq / max(cpu_qps, 1e-9) <= args.parity_seconds:
                sample = nq
            cpu_t, (o_ids, o_dist, o_st) = cpu_run(sample, cpu_threads)
            cpu_qps = max(cpu_qps, sample / cpu_t)
            # and the same sample through the GPU path: identical rows expected
            g_ids = out_ids.cpu().numpy().view(np.uint32) if False else None
            ix.search_batch_dev(qbuf[args.warmup], nq, L, S, k, C.c_void_p(out_ids.data_ptr()), None,
                                C.c_void_p(out_dist.data_ptr()), d_qlabels=qkeys[args.warmup] and qkeys[args.warmup][2],
                                d_qlabel_off=qkeys[args.warmup] and qkeys[args.warmup][3])
            ix.search_batch_dev_finish()
            g_ids = out_ids.cpu().numpy().view(np.uint32)[:sample]
            g_dist = out_dist.cpu().numpy()[:sample]
            result["cpu_baseline"] = {
                "value": round(cpu_qps, 1), "unit": "queries/s", "cores": cpu_threads, "kind": "port",
                "sample": f"{sample} of the step's queries, same index/L/rescore, {cpu_threads} threads (one query per thread, the best "
                          f"point of the thread sweep); single-thread latency {cpu1 * 1e3:.2f} ms/query; flat arrays, no PostgreSQL "
                          f"buffer/heap cost",
                "host": cores,
                "single_thread_qps": round(1.0 / cpu1, 1),
                "thread_sweep": sweep,
                "parallel_efficiency": round(cpu_qps * cpu1 / cpu_threads, 3),  # value / (threads x single-thread rate)
                "consistent": bool(cpu_qps <= cpu_threads / cpu1 * 1.1),
                "micro_ns_per_call": O.micro_bench(),  # the reference's criterion bench shapes (benches/distance.rs), one thread
                "parity_rows": sample, "parity_covers_the_whole_step": bool(sample == nq),
                "gpu_rows_identical": bool((g_ids == o_ids).all()),
                "gpu_dist_bit_identical_frac": float((g_dist.view(np.uint32) == o_dist.view(np.uint32)).mean()),
            }
            if isinstance(result.get("latency"), dict) and "points" in result["latency"]:  # the oracle, one thread, the same queries
                try:
                    nlq = min(nq, 256)
                    t1 = time.time()
                    oidx.search_batch(qh[:nlq], L=100, rescore=50, k=k, threads=1, qlabels=hk and hk[:nlq])
                    result["latency"]["cpu_oracle_single_thread_ms"] = {"default_gucs": round((time.time() - t1) / nlq * 1e3, 3),
                                                                          "operating_point_of_the_value": round(cpu1 * 1e3, 3),
                                                                          "note": "oracle (port of the reference path on flat arrays), one thread, no PostgreSQL buffer / heap cost"}
                except Exception as e:  # noqa: BLE001
                    result["latency"]["cpu_oracle_single_thread_ms"] = {"error": repr(e)}
            result["speedup_vs_cpu_baseline"] = round(qps / cpu_qps, 1)
            result["speedup_vs_one_cpu_thread"] = round(qps * cpu1, 1)
        except Exception as e:  # the GPU numbers stay valid without the baseline
            result["cpu_baseline"] = {"value": None, "unit": "queries/s", "cores": usable_cores()["usable"], "kind": "port",
                                      "sample": f"failed: {e!r}"}

    if pipe["ready"]:
        pipe["ix2"].close()
        pipe["ctx2"].close()
    if comm is not None:
        comm.close()
    ix.close()
    ctx.close()
    # ---- extras: a harder corpus (never the value).  A child run of this script on 20M vectors (10M until round 5) of the `mid` corpus (64-dimensional latent
    # space, wider clusters, 30 % isotropic noise), after this process has given its HBM back: own index build, own operating point,
    # own recall checks and CPU parity; its line is embedded here in short
    if extras_on and rank == 0:
        import subprocess
        t0 = time.time()
        cmd = [sys.executable, os.path.abspath(__file__), "--full", "--n", "500" if EMU else "20000000", "--corpus-kind", "mid", "--extras", "off", "--steps", "3",
               "--warmup", "1", "--cpu-seconds", "4", "--pcie-steps", "0", "--scan-nq", "0", "--graph-cache", "none", "--distance", args.distance]
        if EMU:
            cmd += ["--nq", "16", "--dim", str(dim), "--recall-queries", "16", "--validate-queries", "16", "--heldout-queries", "16", "--build-l", "20"]
        try:
            del out_ids, out_dist, rq_ids
            if not EMU:
                torch.cuda.empty_cache()
            cp = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            line = [ln for ln in cp.stdout.splitlines() if ln.startswith("{")]
            hj = json.loads(line[-1])
            result["harder_corpus"] = {
                "command": " ".join(cmd[1:]), "seconds": round(time.time() - t0, 1),
                "workload": hj["config"]["workload"], "corpus": hj["config"]["corpus"],
                "search_list_size": hj["config"]["search_list_size"], "rescore": hj["config"]["rescore"],
                "queries_per_step": hj["config"]["queries_per_step_per_gpu"],
                "value": hj["value"], "unit": hj["unit"], "ms_per_step": hj["ms_per_step"], "steps": hj["steps"],
                "recall_at_k": hj["recall_at_k"], "recall_validate_lower95": hj["recall_validate_lower95"],
                "recall_heldout": hj["recall_heldout"], "recall_heldout_lower95": hj["recall_heldout_lower95"],
                "recall_target_met": hj["recall_target_met"],
                "roofline": {kk: hj["roofline"].get(kk) for kk in ("kernel", "achieved", "peak", "unit", "frac", "avg_kernel_ms", "launches",
                                                                   "alg_bytes_per_launch")},
                "cpu_baseline": {kk: (hj.get("cpu_baseline") or {}).get(kk) for kk in ("value", "cores", "kind", "gpu_rows_identical",
                                                                                         "gpu_dist_bit_identical_frac")},
                "gpu_rows_identical": (hj.get("cpu_baseline") or {}).get("gpu_rows_identical"),
                "setup_s": hj.get("setup_s"),
                "note": "a child run of this script after the headline index was freed; not the configuration the value is quoted on"}
            log(f"harder corpus (20M mid, {result['harder_corpus']['seconds']} s): {hj['value']:.0f} QPS at L={hj['config']['search_list_size']} "
                f"rescore={hj['config']['rescore']}, met={hj['recall_target_met']}")
        except Exception as e:  # noqa: BLE001
            result["harder_corpus"] = {"error": repr(e), "seconds": round(time.time() - t0, 1)}
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
