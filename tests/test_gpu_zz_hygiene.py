"""Device-memory hygiene of the handles (a GPU broker process lives for weeks): whatever an index, its scans, cursors, brokers,
views and the autotuner allocated on the device or as pinned memory is returned when they are closed.  Counted by the wave64
interpreter's allocator (tests/emu: every hipMalloc / hipHostMalloc is one tracked mapping) — on hardware there is no such counter,
so there the test only runs the sequence (it must not fail or leave the context unusable)."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import TestIndex, make_vectors
from lifecycle_checks import label_csr, make_tids

pytestmark = pytest.mark.gpu
EMU = bool(os.environ.get("VS_EMU"))


def _live():
    if not EMU:
        return 0
    from conftest import EMU_LIB
    lib = C.CDLL(EMU_LIB)
    lib.vs_emu_live_allocations.restype = C.c_size_t
    return int(lib.vs_emu_live_allocations())


def _workout(ctx, ti, q, labeled):
    import pgvectorscale_amd as P
    ix = ti.upload(ctx)
    keys = [[1], [2, 3]] * (len(q) // 2) if labeled else None
    ix.search_batch(q, search_list_size=30, rescore=20, k=10, qlabels=keys)
    ix.stream_batch(q, search_list_size=5, m=150, qlabels=keys)  # long streams: heap spill + global dedup regions
    scan = ix.beginscan()
    scan.rescan(q[0], labels=keys and keys[0], search_list_size=10, rescore=5)
    for _ in range(70):
        scan.gettuple()
    scan.rescan(q[1], labels=keys and keys[1], search_list_size=4, rescore=0)
    for _ in range(20):
        scan.gettuple()
    scan.endscan()
    dq = ctx.alloc(q.nbytes)
    ctx.upload(dq, q)
    saved = {k: os.environ.get(k) for k in ("VS_F_LDS_MAX_INS", "VS_F_VR")}
    try:
        os.environ.update({"VS_F_LDS_MAX_INS": "0", "VS_F_VR": "0"})
        if not labeled:
            ix.autotune(dq, len(q), 10, 8, 10, reps=1, skip=())
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    ctx.free(dq)
    view_ctx = P.Context(0)
    v = ix.view(view_ctx)
    v.search_batch(q[:4], search_list_size=20, rescore=10, k=5)
    v.close()
    view_ctx.close()
    broker = P.Broker(ix, max_batch=8, max_wait_us=100)
    broker.search(q[0], search_list_size=20, rescore=10, k=10)
    bscan = broker.beginscan()
    bscan.rescan(q[1], search_list_size=8, rescore=4)
    for _ in range(40):
        bscan.gettuple()
    bscan.endscan()
    broker.close()
    ix.close()


@pytest.mark.parametrize("labeled", [False, True])
def test_handles_return_their_device_memory(gpu_ctx, labeled):
    kw = dict(n=1200, dim_full=768, bits=2, R=32, distance=1, seed=13, kind="gauss", L_build=40)
    if labeled:
        kw.update(n_labels=4, deleted_frac=0.05)
    ti = TestIndex(**kw)
    q = ti.queries(8, seed=5, kind="gauss")
    _workout(gpu_ctx, ti, q, labeled)  # first pass: the context's own lazily created resources (event pool, staging ring)
    before = _live()
    for _ in range(2):
        _workout(gpu_ctx, ti, q, labeled)
    after = _live()
    assert after == before, f"{after - before} device / pinned allocations outlived their handles"


# ---- graph build and maintenance: one fixed sequence over a device-built index ------------------------------------------------------
# 200 rows (32 dimensions at 2 bits, or 24 plain ones), R = 16, build L = 20, L2; 70 rows inserted, every 7th tid deleted: the smallest
# shapes at which every kernel of the sequence still runs (a batch of more than one row with mates, rows to rewrite, rows to move)
KINDS = ("sbq", "labeled", "plain")
_N, _GROW, _R, _L = 200, 70, 16, 20
_PAIRS = ([1, 2], [1, 3], [2, 3])


def _labels(first, n):
    """two of three labels per row; of the inserted rows every tenth is the first to bring label 4"""
    return [[1, 4] if i >= _N and i % 10 == 5 else _PAIRS[i % 3] for i in range(first, first + n)]


# a step prepares its arguments and returns the ONE library call it stands for (the allocation-failure sweep arms right before it)
def _step_build(S):
    import pgvectorscale_amd as P
    ctx, kind, X = S["ctx"], S["kind"], S["X"][:_N]
    plain = kind == "plain"
    ix = S["ix"] = P.DiskAnnIndex.alloc(ctx, n=_N, dim_full=X.shape[1], bits=None if plain else 2, num_neighbors=_R, distance_type=P.VS_L2,
                                        storage_type=P._lib.VS_STORAGE_PLAIN if plain else P._lib.VS_STORAGE_SBQ)
    vp, stride = ix.array(P._lib.ARR_VECS)
    Xp = np.zeros((_N, stride), np.float32)
    Xp[:, :X.shape[1]] = X
    ctx.upload(vp, Xp)
    ix.refresh_norms()
    if not plain:
        ix.sbq_train()
        ix.sbq_quantize_corpus()
    if kind == "labeled":
        ix.set_labels(*label_csr(_labels(0, _N)))
    ctx.upload(ix.array(P._lib.ARR_TIDS)[0], make_tids(0, _N))
    return lambda: ix.build_graph(search_list_size=_L, max_alpha=1.2)


def _step_insert(S):
    labels = _labels(_N, _GROW) if S["kind"] == "labeled" else None
    return lambda: S["ix"].insert(S["X"][_N:], make_tids(_N, _GROW), labels=labels, search_list_size=_L)


def _step_batch_mates(S):
    codes = S["ix"].download(nbrs=False, tids=False)["codes"][:65]
    return lambda: S["ix"].batch_mates(codes, 16)


def _step_batch_mates_filtered(S):
    codes = S["ix"].download(nbrs=False, tids=False)["codes"][:65]
    return lambda: S["ix"].batch_mates(codes, 16, labels=_labels(0, 65))


def _step_nearest_masked(S):
    n = S["ix"].desc.n
    skip = np.zeros(n, np.uint8)
    skip[::5] = 1
    return lambda: S["ix"].nearest_masked(np.arange(9, dtype=np.uint32), np.full(9, 3, np.uint64), np.arange(n, dtype=np.uint64) % 4, skip)


_STEPS = {
    "build": _step_build,
    "insert": _step_insert,
    "bulk_delete": lambda S: lambda: S["ix"].bulk_delete(make_tids(0, _N + _GROW)[::7]),
    "consolidate": lambda S: lambda: S["ix"].consolidate_deletes(plain=S["kind"] == "plain"),
    "repair": lambda S: lambda: S["ix"].repair(),
    "label_reach": lambda S: lambda: S["ix"].label_reach(per_node=True),
    "repair_labels": lambda S: lambda: S["ix"].repair_labels(),
    "compact": lambda S: lambda: S["ix"].compact(return_map=True),
    "batch_mates": _step_batch_mates,
    "batch_mates_filtered": _step_batch_mates_filtered,
    "batch_mates_plain": lambda S: lambda: S["ix"].batch_mates_plain(3, 70, 16),
    "prune_plain": lambda S: lambda: S["ix"].prune_plain(np.arange(10), [list(range(10, 50))] * 10),
    "nearest_masked": _step_nearest_masked,
}
_ORDER = {
    "sbq": ("build", "insert", "bulk_delete", "consolidate", "repair", "compact", "batch_mates", "batch_mates_filtered", "nearest_masked"),
    "labeled": ("build", "insert", "bulk_delete", "consolidate", "repair", "label_reach", "repair_labels", "compact", "batch_mates",
                "batch_mates_filtered", "nearest_masked"),
    "plain": ("build", "insert", "bulk_delete", "consolidate", "repair", "compact", "batch_mates_plain", "prune_plain"),
}
# step -> the *_kernel_ms getters it feeds and the stages that must have run (None: all of them; the others are only not negative)
_TIMED = {
    "build": {"build_kernel_ms": None},
    "insert": {"insert_kernel_ms": None, "build_kernel_ms": None},
    "consolidate": {"consolidate_kernel_ms": None},
    "compact": {"compact_kernel_ms": None},
    "repair_labels": {"label_repair_kernel_ms": ("sweeps",)},  # (stages 1-3 run only when pairs are lost)
}
# step -> the getters it must leave at zero: the audit runs the repair's sweeps, but vs_index_label_repair_kernel_ms is the repair's own
_NOT_TIMED = {"label_reach": ("label_repair_kernel_ms",)}


def _state(ctx, kind):
    return {"ctx": ctx, "kind": kind, "X": make_vectors(_N + _GROW, 24 if kind == "plain" else 32, 71, "gauss"), "ix": None}


def _sequence(ctx, kind, profiling=False):
    S = _state(ctx, kind)
    ctx.profile_enable(profiling)
    try:
        for name in _ORDER[kind]:
            call = _STEPS[name](S)
            timed = _TIMED.get(name, {}) if profiling else {}
            silent = _NOT_TIMED.get(name, ()) if profiling else ()
            for getter in (*timed, *silent):
                getattr(S["ix"], getter)(reset=True)
            call()
            for getter in silent:
                ms = getattr(S["ix"], getter)(reset=False)
                assert ms == dict.fromkeys(ms, 0.0), (name, getter, ms)
            for getter, ran in timed.items():
                ms = getattr(S["ix"], getter)(reset=True)
                assert all(v > 0 if ran is None or k in ran else v >= 0 for k, v in ms.items()), (name, getter, ms)
                assert getattr(S["ix"], getter)() == dict.fromkeys(ms, 0.0), (name, getter)
    finally:
        ctx.profile_enable(False)
        if S["ix"] is not None:
            S["ix"].close()


@pytest.mark.parametrize("kind,profiling", [("sbq", False), ("labeled", False), ("plain", False), ("labeled", True), ("plain", True)])
def test_maintenance_calls_return_their_device_memory(gpu_ctx, kind, profiling):
    """build -> insert -> bulk_delete -> consolidate -> repair (-> label_reach -> repair_labels) -> compact and the stand-alone kernels
    of the index kind, three times: what the calls allocated is back when the index is closed.  The labeled index is an SBQ index, so
    the two profiled cases time every stage there is."""
    _sequence(gpu_ctx, kind, profiling)  # first pass: the context's own lazily created resources
    before = _live()
    for _ in range(2):
        _sequence(gpu_ctx, kind, profiling)
        after = _live()
        assert after == before, f"{after - before} device / pinned allocations outlived the index"


# the calls that only read the index: a refused one leaves it as it was
_READ_ONLY = ("label_reach", "batch_mates", "batch_mates_filtered", "batch_mates_plain", "prune_plain", "nearest_masked")


@pytest.mark.skipif(not EMU, reason="allocation failures are injected by the interpreter's fake runtime only (VS_EMU)")
@pytest.mark.parametrize("kind", KINDS)
def test_every_allocation_failure_is_reported_and_nothing_leaks(gpu_ctx, kind):
    """for every call of the sequence and k = 1, 2, ...: an index prepared up to that call, the k-th device or pinned allocation of
    the call fails (vs_emu_fail_allocation) -> the library's error, the index closes (the interpreter aborts on a double free and
    faults on a freed buffer) and the live count is what it was before the index existed; until the call succeeds with the
    countdown still pending.  A refused read-only call must leave nothing allocated and the index as it was: the call and the rest
    of the sequence then run on that very index (which goes on to the next k when they only read it too).  A refused call that
    writes leaves an index only close() is promised for: the context then shows it still works in the next preparation, and runs
    the whole sequence once more after the sweep of each call — once per k would take four times as long.
    Allocations per call, printed and not asserted — before and after the scratch scope alike:
    sbq build 19, insert 26, bulk_delete 5, consolidate 8, repair 3, compact 8, batch_mates 2, filtered 4, nearest_masked 5;
    labeled 21, 32, 5, 8, 3, label_reach 15, repair_labels 22, compact 13, 2, 4, 5; plain 18, 23, 5, 8, 3, 8, mates 1, prune 1."""
    import pgvectorscale_amd as P
    from conftest import EMU_LIB
    lib = C.CDLL(EMU_LIB)
    lib.vs_emu_fail_allocation.restype = C.c_long
    lib.vs_emu_fail_allocation.argtypes = [C.c_long]
    _sequence(gpu_ctx, kind)
    base = _live()
    order, counts = _ORDER[kind], {}
    for i, name in enumerate(order):
        S, k, done = None, 0, False
        while not done:
            k += 1
            assert k < 200, f"{name}: still allocating after 199 injected failures"
            keep = False
            try:
                if S is None:
                    S = _state(gpu_ctx, kind)
                    for earlier in order[:i]:
                        _STEPS[earlier](S)()
                call = _STEPS[name](S)
                held, raised = _live(), None
                lib.vs_emu_fail_allocation(k)
                try:
                    call()
                except P.VsError as e:
                    raised = e
                done = lib.vs_emu_fail_allocation(0) > 0
                if done:
                    assert raised is None, f"{name}: failed with no allocation failure injected: {raised}"
                else:
                    assert raised is not None, f"{name}: allocation {k} failed and the call reported success"
                    if name in _READ_ONLY:
                        assert _live() == held, f"{name}: allocation {k} failed and {_live() - held} allocations outlived the call"
                        for later in order[i:]:
                            _STEPS[later](S)()
                        keep = all(later in _READ_ONLY for later in order[i:])
            finally:
                lib.vs_emu_fail_allocation(0)
                if S is not None and not keep:
                    if S["ix"] is not None:
                        S["ix"].close()
                    S = None
            assert keep or _live() == base, f"{name}: allocation {k} failed and {_live() - base} allocations outlived the index"
        counts[name] = k - 1
        _sequence(gpu_ctx, kind)
        assert _live() == base
    print(f"allocations per call ({kind}): {counts}")


def test_staging_ring_round_trip(gpu_ctx):
    """host -> pinned ring -> HBM -> pinned ring -> host: chunks of 8 MiB and more are copied into / out of the pinned buffers by several
    threads (stage_copy, csrc/vs_api.hip); sizes around the chunk (32 MiB) and the split boundaries must come back bit for bit"""
    rng = np.random.default_rng(3)
    # (sizes whose per-thread share is page aligned while the total is not: the split must still cover the last bytes)
    for nbytes in (5, (8 << 20) - 1, (8 << 20) + 4097, (32 << 20) + 12345, (70 << 20) + 1, 2 * 4096 * 1100 + 1, 3 * 4096 * 700 + 1,
                   4 * 4096 * 600 + 3, 5 * 4096 * 500 + 4, 16 * 4096 * 140 + 15):
        a = rng.integers(0, 256, nbytes, dtype=np.uint8)
        d = gpu_ctx.alloc(nbytes)
        gpu_ctx.upload(d, a)
        b = np.zeros(nbytes, np.uint8)
        gpu_ctx.download(d, b)
        gpu_ctx.free(d)
        assert (a == b).all(), nbytes


def test_row_wise_staging_pads_and_copies_every_row(gpu_ctx):
    """index upload through the public entry point: neighbor lists of R = 50 go into device rows of 64 through the pinned ring row by
    row, zero padded, and 9-dimensional vectors into rows of 12 floats; a chunk of 8 MiB and more is filled by several threads —
    every row must arrive (vs_index_download undoes the padding)"""
    import pgvectorscale_amd as P
    rng = np.random.default_rng(11)
    n, R, dim, W = 200_001, 50, 9, 1
    nbrs = ((np.arange(n, dtype=np.uint64)[:, None] + 1 + np.arange(R, dtype=np.uint64)[None, :] * 7919) % n).astype(np.uint32)
    nbrs[::17, 40:] = 0xFFFFFFFF  # some short lists (the list ends at the first invalid id)
    codes = rng.integers(0, 1 << 18, (n, W), dtype=np.uint64)
    tids = ((np.arange(n, dtype=np.uint64) + 3) << np.uint64(16)) | np.uint64(1)
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    ix = P.DiskAnnIndex.upload(gpu_ctx, codes=codes, nbrs=nbrs, heap_tids=tids, vecs=vecs, mean=np.zeros(dim, np.float32),
                               m2=np.ones(dim, np.float32), count=n, bits=2, dim_index=dim, num_neighbors=R, distance_type=P.VS_L2,
                               default_start=0)
    try:
        host = ix.download(vecs=True)
        assert (host["nbrs"] == nbrs).all()
        assert (host["codes"] == codes).all() and (host["heap_tids"] == tids).all()
        assert (host["vecs"].view(np.uint32) == vecs.view(np.uint32)).all()
    finally:
        ix.close()
