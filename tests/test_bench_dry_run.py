"""bench.py end to end without a GPU: its whole control flow (on-device index manufacture, ground truth, operating-point
search, timed steps, flat-scan section, CPU baseline + closing parity check, JSON
assembly) runs against the wave64 interpreter build of the kernels (VS_EMU=1).  The numbers of such a run mean nothing;
the point is that a typo in the benchmark cannot wait for the round-end GPU run to be found.  ~2 minutes: only with
VS_EMU_FULL=1."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.environ.get("VS_EMU_FULL"), reason="slow (about 2 minutes); set VS_EMU_FULL=1")
def test_bench_dry_run_on_the_interpreter():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "emu"), "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, VS_EMU="1", VS_F_LDS_MAX_INS="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--n", "6000", "--dim", "64", "--nq", "128", "--steps", "1", "--warmup", "1",
           "--recall-queries", "16", "--scan-nq", "8", "--cpu-seconds", "1", "--graph-cache", "none"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads(r.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in j, key
    assert "DRY RUN" in j["data"] and j["config"]["workload"]
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(j["roofline"])
    assert j["cpu_baseline"]["gpu_rows_identical"] is True and j["cpu_baseline"]["gpu_dist_bit_identical_frac"] == 1.0
    # (16 tuning queries: the 0.99 target is a matter of luck here; what is checked is that all three recalls are reported)
    assert isinstance(j["recall_target_met"], bool) and 0.9 < j["recall_heldout"] <= 1.0 and 0.9 < j["recall_validate"] <= 1.0
    assert j["cpu_baseline"]["parity_covers_the_whole_step"] is True and j["cpu_baseline"]["parity_rows"] == 128
    assert j["library"]["sha256_12"] and j["library"]["kernel_source_hash"] and j["library"]["rebuilt_on_this_box"] is None
    cb = j["cpu_baseline"]
    # (a 128-query sample takes milliseconds here: the consistency flag is only checked for being reported)
    assert cb["cores"] <= cb["host"]["os_cpu_count"] and cb["thread_sweep"] and isinstance(cb["consistent"], bool)


@pytest.mark.skipif(not os.environ.get("VS_EMU_FULL"), reason="slow (about 2 minutes); set VS_EMU_FULL=1")
def test_bench_dry_run_two_ranks():
    """the N > 1 launch line of the driver (torch.distributed.run, one rank per GPU), with gloo standing in for RCCL"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "emu"), "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, VS_EMU="1", VS_EMU_THREADS="4", VS_F_LDS_MAX_INS="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29519", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--corpus", "4000", "--dim", "64", "--nq", "64",
           "--steps", "1", "--warmup", "1", "--recall-queries", "16", "--scan-nq", "0", "--cpu-seconds", "1", "--graph-cache", "none",
           "--fixed", "100,50"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and "query-sharded x2" in j["config"]["parallelism"]


@pytest.mark.skipif(not os.environ.get("VS_EMU_FULL"), reason="slow (about 2 minutes); set VS_EMU_FULL=1")
def test_bench_dry_run_two_batches_in_flight():
    env = dict(os.environ, VS_EMU="1", VS_F_LDS_MAX_INS="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--n", "6000", "--dim", "64", "--nq", "128", "--steps", "3", "--warmup", "1",
           "--recall-queries", "16", "--scan-nq", "8", "--cpu-seconds", "1", "--graph-cache", "none", "--pipeline", "2"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["config"]["batches_in_flight"] == 2 and j["steps"] == 3
    assert j["cpu_baseline"]["gpu_rows_identical"] is True and 0.9 < j["recall_heldout"] <= 1.0


def test_bench_two_ranks_small():
    """DEFAULT CPU tier (about 20 s): the driver's N > 1 launch line on the interpreter (gloo for the launcher's control plane, tests/emu/libfakerccl.so for the library's vs_comm_*) — rank 0 builds
    the graph and broadcasts it, both ranks run their shard of the queries with two batches in flight (--pipeline 2), the held-out
    recall is pooled over the ranks, one vs_comm_gather_topk closes each step, rank 0 prints the line"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "emu"), "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, VS_EMU="1", VS_EMU_THREADS="4", VS_F_LDS_MAX_INS="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29523", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--corpus", "1500", "--dim", "32", "--nq", "32",
           "--steps", "2", "--warmup", "1", "--recall-queries", "8", "--validate-queries", "16", "--heldout-queries", "16",
           "--scan-nq", "0", "--cpu-seconds", "1", "--graph-cache", "none", "--fixed", "20,10", "--pipeline", "2"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and "query-sharded x2" in j["config"]["parallelism"]
    assert "vs_comm_gather_topk" in j["config"]["topk_gather"]  # the collective lives behind the C ABI (stand-in RCCL on the interpreter)
    assert j["config"]["batches_in_flight"] == 2 and j["steps"] == 2
    assert "graph_build_s" in j["setup_s"] and "graph_broadcast_s" in j["setup_s"]  # rank 0 built, the others received
    assert j["recall_heldout_queries"] == 32  # 16 per rank, pooled
    assert j["value"] > 0 and j["roofline"]["timed_over"].startswith("1 sequential warm-up")


def test_bench_extras_small():
    """DEFAULT CPU tier (about a minute): the three objects the default run adds outside the headline value — `default_gucs` (the
    reference's default GUCs on the same index), `cursor_pool` (backend PROCESSES streaming through the shared-memory server: a cursor
    per scan against scan pools, rows compared) and `harder_corpus` (a child run of the script on the `mid` corpus) — assembled by the
    script's own control flow on the interpreter"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "emu"), "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, VS_EMU="1", VS_F_LDS_MAX_INS="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--n", "2000", "--dim", "64", "--nq", "32", "--steps", "1", "--warmup", "1",
           "--recall-queries", "16", "--validate-queries", "16", "--heldout-queries", "16", "--scan-nq", "0", "--cpu-seconds", "1",
           "--graph-cache", "none", "--pcie-steps", "0", "--extras", "on", "--fixed", "20,10"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
    dg, cp, hc = j["default_gucs"], j["cursor_pool"], j["harder_corpus"]
    assert "error" not in dg and dg["search_list_size"] == 100 and dg["rescore"] == 50 and dg["value"] > 0
    assert isinstance(dg["recall_target_met"], bool) and set(("achieved", "frac", "avg_kernel_ms")) <= set(dg["roofline"])
    assert "error" not in cp, cp
    for mode in ("cursor_per_scan", "scan_pools"):
        assert cp[mode]["rows_identical_to_cursor_per_scan"] is True and cp[mode]["all_scans_ms"] > 0
    assert "error" not in hc, hc
    assert hc["gpu_rows_identical"] is True and isinstance(hc["recall_target_met"], bool) and "mid" in hc["corpus"]
    # the latency leg (round 6): backend processes (pgvectorscale_amd/vs_shm_lat, plain C clients of the shared-memory server) at two
    # concurrency levels, two operating points, the oracle's single-thread latency next to them
    lt = j["latency"]
    assert "error" not in lt, lt
    for point in ("default_gucs", "operating_point_of_the_value"):
        lv = lt["points"][point]["levels"]
        assert [r_["backends"] for r_ in lv] == [1, 3] and all("error" not in r_ and r_["p50_us"] > 0 and r_["p95_us"] >= r_["p50_us"] and r_["p99_us"] >= r_["p95_us"]
                                                                 for r_ in lv), lv
        assert lt["points"][point]["same_rows_at_every_level"] is True
    assert lt["cpu_oracle_single_thread_ms"]["default_gucs"] > 0 and lt["cpu_oracle_single_thread_ms"]["operating_point_of_the_value"] > 0
    assert j["cpu_baseline"]["consistent"] in (True, False) and j["cpu_baseline"]["single_thread_qps"] > 0


def test_bench_eight_emulated_devices():
    """DEFAULT CPU tier: the driver's N = 8 launch line (torch.distributed.run, one rank per GPU) on the interpreter — eight processes,
    rank 0 builds the graph and vs_comm_bcast hands it to the seven others over the stand-in RCCL, every rank searches its own block
    (a query count that does not divide by eight on purpose: the pooled held-out rows are uneven), one vs_comm_gather_topk per step,
    ONE JSON line from rank 0.  No 8-GPU node was available to any round: this is what `bench.py --gpus 8` has been through."""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "emu"), "-j8", "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, VS_EMU="1", VS_EMU_THREADS="1", VS_EMU_DEVICES="8", VS_F_LDS_MAX_INS="0", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
           "--master-port", "29531", os.path.join(ROOT, "bench.py"), "--gpus", "8", "--corpus", "900", "--dim", "32", "--nq", "12",
           "--steps", "2", "--warmup", "1", "--recall-queries", "6", "--validate-queries", "10", "--heldout-queries", "10",
           "--scan-nq", "0", "--cpu-seconds", "1", "--graph-cache", "none", "--fixed", "20,10"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line (rank 0)"
    j = json.loads(lines[-1])
    assert j["n_gpus"] == 8 and j["scaling"] == "weak" and "query-sharded x8" in j["config"]["parallelism"]
    assert "vs_comm_gather_topk" in j["config"]["topk_gather"]
    assert "graph_build_s" in j["setup_s"] and "graph_broadcast_s" in j["setup_s"]
    assert j["recall_heldout_queries"] == 80  # 10 per rank, pooled
    assert j["value"] > 0 and j["steps"] == 2
