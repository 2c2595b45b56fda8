"""The RESUMABLE rescore window (next_with_resort, AM/scan.rs:244-305: a BinaryHeap<ResortData> ordered by f32::total_cmp) on tied
distances, negative distances and distances that are no ordinary numbers.  k_resort_cursor (the amgettuple cursor: one thread, the heap
kept in global memory between calls) and k_resort_cursor_batch (the scan pools' fetch: one wave per slot, the heap copied to LDS and
back, keys fetched ahead, rows gathered by k lanes) keep their heap from one call to the next, so a wrong tie rule or a wrong key shows
rows later, not at once — and the corpora of the other cursor, pool, broker and lanes tests (uniform, gauss, clustered; L2, cosine)
never produce two equal f32 distances or a negative one.  Every case compares node id, heap TID and the 32 bits of the distance row by
row with OracleIndex.scan(...).gettuple(), and the seven GreedySearchStats counters at checkpoints.  A NaN is compared like any other
distance: sign and payload included.

Corpora (tests/helpers.Corpus over tie_vectors: about ten copies of every vector):
  ties       1 500 x 40, L2: one 32-float step and a scalar tail
  ip         the same minus 0.5 under inner product: negative distances of several magnitudes, no zero row
  cosine     1 500 x 72, rows scaled by 0.5 / 1 / 3 / 8: the divisor runs, copies scaled by powers of two still tie
  truncated  1 500 x 64 with SBQ codes over the leading 48 dimensions
  special    trained, quantised and built on clean tie vectors; then rows of the VECTOR column are overwritten (oracle and upload
             alike), so the stream is the clean index's and only the rescore window sees the plants.  The victims are among the first
             40 stream rows of the test's own queries.  L2: a coordinate +inf, one -inf (in the tail), a NaN with the sign clear and
             one with it set, a copy of the query (+0.0), and a 1e-20-scaled row met by a 1e-20-scaled query (every square is
             denormal).  IP: the same, plus a zero row (-0.0) and two rows of +-denorm_min with the signs of the query and against
             them: every product underflows, to +0 in one row (distance -0.0) and to -0 in the other (distance +0.0; a sum that starts
             from +0 is -0 only if EVERY term is -0, which is why a row that is merely orthogonal to the query never gives +0.0).
             +inf and a NaN with the sign clear stay in the window until the stream ends, so these scans are pulled to their end.

What keeps a case honest depends on the oracle alone and is asserted, never skipped: a tie scan hands out at least 10 adjacent row pairs
with identical distance bits; an ip scan with a window returns at least two different negative distances within some `rescore`
consecutive rows; a special scan returns every class it plants, told by the bit pattern.

Also runs on the lockstep interpreter (tests/test_emu_cursor_window.py), all of it."""
import functools
import itertools

import numpy as np
import pytest

from helpers import Corpus, tie_vectors
from oracle import oracle_py as O
from test_gpu_zzz_rerank_window import check

pytestmark = pytest.mark.gpu

STAT_KEYS = ("visited_nodes", "candidate_nodes", "quantized_distance_comparisons", "full_distance_comparisons", "node_reads",
             "node_heap_reads", "next_calls")
L = 20          # the search list of every case but the restart's
CHUNKS = (1, 5, 70, 3, 1, 64, 65, 2)


def bits_of(d):
    return int(np.float32(d).view(np.uint32))


# ---- the classes a special corpus plants, told by the distance's bits
CLASSES = {
    "+inf": lambda b: b == 0x7F800000,
    "-inf": lambda b: b == 0xFF800000,
    "+nan": lambda b: (b >> 31) == 0 and (b & 0x7FFFFFFF) > 0x7F800000,
    "-nan": lambda b: (b >> 31) == 1 and (b & 0x7FFFFFFF) > 0x7F800000,
    "+0": lambda b: b == 0x00000000,
    "-0": lambda b: b == 0x80000000,
    "denormal": lambda b: (b & 0x7F800000) == 0 and (b & 0x007FFFFF) != 0,
}


def assert_classes(bits, wanted, where):
    for name in wanted:
        assert any(CLASSES[name](b) for b in bits), (where, "the scan never returned a distance of class", name)


def tied_pairs(bits):
    return sum(1 for a, b in zip(bits, bits[1:]) if a == b)


def assert_honest(kind, bits, rescore, where):
    """the conditions of the module docstring, on the oracle's rows"""
    if kind in ("ties", "cosine", "truncated", "ties3000", "ties6000"):
        assert tied_pairs(bits) >= 10, (where, "tied adjacent pairs", tied_pairs(bits))
    if kind == "ip" and rescore >= 4:  # (no window, or a window of one row, orders nothing)
        def negative(b):
            return (b >> 31) == 1 and b != 0x80000000 and (b & 0x7FFFFFFF) < 0x7F800000
        most = max(len({b for b in bits[i:i + rescore] if negative(b)}) for i in range(max(len(bits) - rescore, 0) + 1))
        assert most >= 2, (where, "different negative distances within one window's worth of rows", most)


# ---- corpora, built once per process
@functools.lru_cache(maxsize=None)
def corpus(kind):
    if kind == "ties":
        return Corpus(tie_vectors(1500, 150, 40, seed=21))
    if kind == "ip":
        X = tie_vectors(1500, 150, 40, seed=22) - np.float32(0.5)
        assert (X != 0).any(axis=1).all()
        return Corpus(X, distance=O.IP)
    if kind == "cosine":
        X = tie_vectors(1500, 150, 72, seed=23)
        f = np.array([0.5, 1.0, 3.0, 8.0], np.float32)[np.random.default_rng(24).integers(0, 4, 1500)]
        return Corpus(X * f[:, None], distance=O.COSINE)
    if kind == "truncated":
        return Corpus(tie_vectors(1500, 150, 64, seed=25), dim_index=48)
    if kind == "ties3000":
        return Corpus(tie_vectors(3000, 300, 40, seed=26))
    if kind == "ties6000":
        return Corpus(tie_vectors(6000, 600, 40, seed=27))
    if kind == "drain50":
        return Corpus(tie_vectors(50, 10, 40, seed=28), R=8, L_build=10)
    if kind == "drain9":
        return Corpus(tie_vectors(9, 4, 40, seed=29), R=8, L_build=10)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def queries(kind, nq=8):
    """row 0 is a corpus row (a run of equal distances heads the stream), the others are drawn like the corpus"""
    c = corpus(kind)
    q = np.random.default_rng(31).random((nq, c.dim), dtype=np.float32)
    if kind == "ip":
        q -= np.float32(0.5)
    q[0] = c.vecs[17]
    return q


@functools.lru_cache(maxsize=None)
def special(distance, n=1500):
    """-> (corpus with the plants in its vector column, queries [8][40], {query: classes its scan must return})"""
    ip = distance == O.IP
    shift = np.float32(0.5 if ip else 0.0)
    rng = np.random.default_rng(41)
    small = n <= 100  # (fewer copies and a denser graph: the oracle's scan has to reach most of so few rows)
    c = Corpus(tie_vectors(n, n // 2 if small else n // 10, 40, seed=42) - shift, distance=distance, R=16 if small else 24,
               L_build=30 if small else 40)
    q = rng.random((8, 40), dtype=np.float32) - shift
    q[1] = np.float32(1e-20) * (rng.random(40, dtype=np.float32) - shift)

    def head(query):  # the first 40 stream rows of the clean index: inside every window a test opens on that query
        s = c.oracle.scan(query, L=L, rescore=0)
        rows = [s.gettuple() for _ in range(40)]
        return [r[0] for r in rows if r is not None]

    taken = set()

    def victim(stream, at):
        for node in stream[at:] + stream[:at]:
            if node not in taken:
                taken.add(node)
                return node
        raise AssertionError("no stream row left to plant on")

    sa, sb = head(q[0]), head(q[1])
    assert len(sa) >= 30 and len(sb) >= 10
    sign = np.where(q[0] < 0, np.float32(-1), np.float32(1))
    V = c.vecs
    plants = []

    def coord(node, j, value):
        plants.append((node, V[node].copy()))
        plants[-1][1][j] = value

    def row(node, value):
        plants.append((node, np.ascontiguousarray(value, np.float32)))

    nan_set = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
    coord(victim(sa, 2), 3, np.float32(np.inf) * sign[3])      # L2: +inf.  IP: the dot product is +inf, the distance -inf
    coord(victim(sa, 9), 35, -np.float32(np.inf) * sign[35])   # (in the scalar tail) L2: +inf.  IP: +inf
    coord(victim(sa, 14), 10, np.float32(np.nan))
    coord(victim(sa, 20), 37, nan_set)
    row(victim(sa, 5), q[0])                                    # L2: +0.0
    row(victim(sb, 3), np.float32(1e-20) * (rng.random(40, dtype=np.float32) - shift))
    wanted = {0: ["+inf", "+nan", "-nan"] + (["-inf"] if ip else ["+0"]), 1: ["denormal"]}
    if ip:
        tiny = np.float32(1e-45)  # the smallest denormal: its product with |q| <= 0.5 rounds to a signed zero
        assert tiny > 0 and np.abs(q[0]).max() <= 0.5
        row(victim(sa, 24), np.zeros(40, np.float32))           # -0.0
        row(victim(sa, 27), sign * tiny)                        # every product +0: -0.0
        row(victim(sa, 12), -sign * tiny)                       # every product -0: +0.0
        wanted[0] += ["+0", "-0"]
    for node, value in plants:
        V[node] = value
        c.oracle.vecs[node] = value  # (the same array unless the oracle had to copy it)
    return c, q, wanted


# ---- the comparisons
def same_stats(g, o, where):
    for key in STAT_KEYS:
        assert g[key] == o[key], (where, key, g[key], o[key])


def pull_and_compare(scan, oscan, checkpoints, limit, where):
    """amgettuple by amgettuple -> ([(node, distance bits)], the scan ended)"""
    out = []
    while len(out) < limit:
        r, o = scan.gettuple(), oscan.gettuple()
        assert (r is None) == (o is None), (where, len(out))
        if r is None:
            return out, True
        assert r[1] == o[0] and r[0] == o[1], (where, len(out), r, o)
        assert bits_of(r[2]) == bits_of(o[2]), (where, len(out), hex(bits_of(r[2])), hex(bits_of(o[2])))
        out.append((o[0], bits_of(o[2])))
        if len(out) in checkpoints:
            same_stats(scan.stats(), oscan.stats(), (where, f"after {len(out)} rows"))
    return out, False


# ==== the direct cursor (k_resort_cursor), one row at a time
@pytest.mark.parametrize("rescore", [0, 1, 4, 30, 100])
@pytest.mark.parametrize("kind", ["ties", "ip", "cosine", "truncated"])
def test_cursor_rows_on_ties_and_negative_distances(gpu_ctx, kind, rescore):
    c, q = corpus(kind), queries(kind)
    ix = c.upload(gpu_ctx)
    scan = ix.beginscan()
    try:
        for qi in range(2):
            scan.rescan(q[qi], search_list_size=L, rescore=rescore)
            os_ = c.oracle.scan(q[qi], L=L, rescore=rescore)
            rows, ended = pull_and_compare(scan, os_, {1, 17, 65}, 200, (kind, rescore, qi))
            same_stats(scan.stats(), os_.stats(), (kind, rescore, qi, "at the end"))
            assert len(rows) == 200 and scan.work()["retries"] == 0
            assert_honest(kind, [b for _, b in rows], rescore, (kind, rescore, qi))
    finally:
        scan.endscan()
        ix.close()


@pytest.mark.parametrize("rescore", [4, 30])
@pytest.mark.parametrize("distance", [O.L2, O.IP], ids=["l2", "ip"])
def test_cursor_rows_on_special_distances(gpu_ctx, distance, rescore):
    c, q, wanted = special(distance)
    ix = c.upload(gpu_ctx)
    scan = ix.beginscan()
    try:
        for qi in (0, 1):
            scan.rescan(q[qi], search_list_size=L, rescore=rescore)
            os_ = c.oracle.scan(q[qi], L=L, rescore=rescore)
            rows, ended = pull_and_compare(scan, os_, {1, 17, 65}, 10_000, (distance, rescore, qi))
            assert ended
            same_stats(scan.stats(), os_.stats(), (distance, rescore, qi, "exhausted"))
            assert_classes([b for _, b in rows], wanted[qi], (distance, rescore, qi))
    finally:
        scan.endscan()
        ix.close()


@pytest.mark.parametrize("rescore", [4, 30])
def test_restarted_scan_replays_its_window_on_ties(gpu_ctx, monkeypatch, rescore):
    """capacities for a few dozen rows on a scan of thousands: after every restart the window runs again from row 0 and the rows
    already handed out are skipped — among them runs of equal distances, which must be skipped in the order they came"""
    monkeypatch.setenv("VS_CURSOR_HORIZON", "4")
    monkeypatch.setenv("VS_HL", "63")
    c = corpus("ties3000")
    q = queries("ties3000")
    ix = c.upload(gpu_ctx)
    scan = ix.beginscan()
    try:
        scan.rescan(q[1], search_list_size=4, rescore=rescore)
        os_ = c.oracle.scan(q[1], L=4, rescore=rescore)
        rows, ended = pull_and_compare(scan, os_, {1, 17, 65, 1000}, 10_000, ("restart", rescore))
        assert ended
        same_stats(scan.stats(), os_.stats(), ("restart", rescore, "exhausted"))
        assert scan.work()["retries"] >= 1
        nodes = [n for n, _ in rows]
        assert len(set(nodes)) == len(nodes) and len(nodes) > 1000  # every row the oracle reaches, once
        assert_honest("ties3000", [b for _, b in rows], rescore, ("restart", rescore))
    finally:
        scan.endscan()
        ix.close()


def test_one_prefetch_across_two_window_launches(gpu_ctx):
    """cursor_fetch runs k_resort_cursor with 4 096 rows and then with the rest, over one heap of 1 000 entries"""
    c, q = corpus("ties6000"), queries("ties6000")
    ix = c.upload(gpu_ctx)
    scan = ix.beginscan()
    try:
        scan.rescan(q[1], search_list_size=L, rescore=1000)
        scan.prefetch(5000)
        launches = scan.work()["launches"]
        os_ = c.oracle.scan(q[1], L=L, rescore=1000)
        rows, ended = pull_and_compare(scan, os_, {1, 4096, 4097, 5000}, 5200, "prefetch")
        assert len(rows) == 5200
        assert launches >= 1 and scan.work()["retries"] == 0
        same_stats(scan.stats(), os_.stats(), "prefetch, at the end")
        assert_honest("ties6000", [b for _, b in rows], 1000, "prefetch")
    finally:
        scan.endscan()
        ix.close()


# ==== the scan pools (k_resort_cursor_batch) under both of their search kernels
@pytest.fixture(params=["resumable_fast_kernel", "general_kernel"])
def pool_kernel(request, monkeypatch):
    """the VS_POOL_FAST switch as tests/test_gpu_zt_scanpool.py sets it (there for every test of the module, here for the pools')"""
    monkeypatch.setenv("VS_POOL_FAST", "1" if request.param == "resumable_fast_kernel" else "0")
    return request.param


def check_chunk(rows, ids, tids, dist, oscan, k, where):
    """the oracle's next k amgettuple calls against one slot's chunk; a short chunk only where the oracle's next row is None"""
    got = []
    for j in range(k):
        o = oscan.gettuple()
        if o is None:
            break
        assert j < rows, (where, "the pool ended the scan early", j, rows)
        assert ids[j] == o[0] and tids[j] == o[1], (where, j, int(ids[j]), o)
        assert int(dist[j].view(np.uint32)) == bits_of(o[2]), (where, j, hex(int(dist[j].view(np.uint32))), hex(bits_of(o[2])))
        got.append((o[0], bits_of(o[2])))
    assert rows == len(got), (where, rows, len(got))
    return got


@pytest.mark.parametrize("rescore", [1, 4, 30])
@pytest.mark.parametrize("kind", ["ties", "ip", "special_l2", "special_ip"])
def test_pool_chunks_on_ties_negative_and_special_distances(gpu_ctx, pool_kernel, kind, rescore):
    import pgvectorscale_amd as P
    wanted = {}
    if kind.startswith("special"):
        c, q, wanted = special(O.IP if kind == "special_ip" else O.L2)
        q = np.vstack([q[0:1], q[2:3], q[1:2], q[3:]])  # (slot 1 is rescanned midway: the two queries with plants sit on slots 0 and 2)
        wanted = {0: wanted[0], 2: wanted[1]}
    else:
        c, q = corpus(kind), queries(kind)
    G, spare, rounds = 6, 6, 16
    ix = c.upload(gpu_ctx)
    pool = P.ScanPool(ix, G, search_list_size=L, rescore=rescore, kmax=70, rows_cap=2048)
    try:
        oscans = []
        for i in range(G):
            pool.rescan(i, q[i])
            oscans.append(c.oracle.scan(q[i], L=L, rescore=rescore))
        handed = [[] for _ in range(G)]
        ended = [False] * G
        for rnd in itertools.count():
            alive = [i for i in range(G) if not ended[i] and (rnd < rounds or i in wanted)]  # (the planted scans go on to their end)
            if not alive:  # an empty slot list is refused
                break
            two = sorted({alive[(rnd // 2) % len(alive)], alive[(rnd // 2 + 3) % len(alive)]})
            who = alive if rnd % 2 == 0 else two
            kk = CHUNKS[(rnd + rnd // 8) % 8]  # (both kinds of round meet every chunk size)
            rows, ids, tids, dist = pool.fetch(who, kk)
            for a, i in enumerate(who):
                assert rows[a] >= 0, (rnd, i, rows[a])
                got = check_chunk(int(rows[a]), ids[a], tids[a], dist[a], oscans[i], kk, (kind, rescore, rnd, i))
                handed[i] += got
                ended[i] = len(got) < kk
                same_stats(pool.stats(i), oscans[i].stats(), (kind, rescore, rnd, i))
            if rnd == 5:  # slot 1 is rescanned while its window holds rows: the new scan's window starts empty
                assert len(handed[1]) >= 1 and not ended[1]
                pool.rescan(1, q[spare])
                oscans[1] = c.oracle.scan(q[spare], L=L, rescore=rescore)
                handed[1] = []
        for i in range(G):
            assert len(handed[i]) >= 150, (i, len(handed[i]))
            assert_honest(kind, [b for _, b in handed[i]], rescore, (kind, rescore, "slot", i))
        for i, classes in wanted.items():
            assert ended[i]
            assert_classes([b for _, b in handed[i]], classes, (kind, rescore, "slot", i))
    finally:
        pool.close()
        ix.close()


@pytest.mark.parametrize("kind,rescore,chunk", [("drain50", 30, 16), ("drain9", 50, 16)])
def test_pool_window_drains_and_never_fills(gpu_ctx, pool_kernel, kind, rescore, chunk):
    """50 rows, window 30: once the scan is exhausted the window empties below `rescore` chunk by chunk.  9 rows, window 50: the window
    never fills.  Fetches past the end return no rows."""
    import pgvectorscale_amd as P
    c = corpus(kind)
    q = np.random.default_rng(33).random((2, c.dim), dtype=np.float32)
    ix = c.upload(gpu_ctx)
    pool = P.ScanPool(ix, 2, search_list_size=L, rescore=rescore, kmax=chunk, rows_cap=256)
    try:
        for slot in (0, 1):
            pool.rescan(slot, q[slot])
            os_ = c.oracle.scan(q[slot], L=L, rescore=rescore)
            total = 0
            while True:
                rows, ids, tids, dist = pool.fetch([slot], chunk)
                got = check_chunk(int(rows[0]), ids[0], tids[0], dist[0], os_, chunk, (kind, slot, total))
                total += len(got)
                same_stats(pool.stats(slot), os_.stats(), (kind, slot, total))
                if len(got) < chunk:
                    break
            assert total >= 5
            for _ in range(2):
                rows, _, _, _ = pool.fetch([slot], chunk)
                assert rows[0] == 0 and os_.gettuple() is None
            same_stats(pool.stats(slot), os_.stats(), (kind, slot, "past the end"))
    finally:
        pool.close()
        ix.close()


def test_pool_at_its_widest(gpu_ctx, pool_kernel):
    """the largest window and the largest chunk a pool takes: 1 000 heap entries, 5 096 keys and 4 096 positions in LDS"""
    import pgvectorscale_amd as P
    c, q = corpus("ties6000"), queries("ties6000")
    ix = c.upload(gpu_ctx)
    pool = P.ScanPool(ix, 1, search_list_size=L, rescore=1000, kmax=4096, rows_cap=6000)
    try:
        pool.rescan(0, q[1])
        os_ = c.oracle.scan(q[1], L=L, rescore=1000)
        handed = []
        for kk in (4096, 500):
            rows, ids, tids, dist = pool.fetch([0], kk)
            handed += check_chunk(int(rows[0]), ids[0], tids[0], dist[0], os_, kk, ("widest", kk))
            same_stats(pool.stats(0), os_.stats(), ("widest", kk))
        assert len(handed) == 4596
        assert_honest("ties6000", [b for _, b in handed], 1000, "widest")
    finally:
        pool.close()
        ix.close()


# ==== a scan on a broker: rows 1 to 16 from the shared launch (k_rerank_window or the pair), the rest from the cursor that re-runs them
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("rescore", [1, 4, 30, 100])
def test_broker_scan_seam_on_ties(gpu_ctx, rescore, fused):
    import pgvectorscale_amd as P
    c, q = corpus("ties"), queries("ties")
    ix = c.upload(gpu_ctx)
    P.set_option("VS_RERANK_FUSED", fused)
    broker = P.Broker(ix, max_batch=4, max_wait_us=0)
    scan = broker.beginscan()
    try:
        for qi in range(4):  # four rescans on one descriptor
            scan.rescan(q[qi], search_list_size=L, rescore=rescore)
            os_ = c.oracle.scan(q[qi], L=L, rescore=rescore)
            # (statistics inside the shared window replay the scan on a cursor early: asked for on every other rescan only)
            rows, ended = pull_and_compare(scan, os_, {1, 17} if qi % 2 == 0 else set(), 60, ("broker", rescore, fused, qi))
            assert len(rows) == 60
            same_stats(scan.stats(), os_.stats(), ("broker", rescore, fused, qi, "at the end"))
            assert scan.work()["retries"] == 0
            assert_honest("ties", [b for _, b in rows], rescore, ("broker", rescore, fused, qi))
    finally:
        scan.endscan()
        broker.close()
        P.set_option("VS_RERANK_FUSED", None)
        ix.close()


# ==== the batch window (k_resort, k_rerank_window) on the special distances: tests/test_gpu_zzz_rerank_window.py has ties and inner
# products, but no +-inf, NaN, signed zero or denormal distance
@pytest.mark.parametrize("distance", [O.L2, O.IP], ids=["l2", "ip"])
def test_batch_window_on_special_distances(gpu_ctx, distance):
    ip = distance == O.IP
    c, q, _ = special(distance)
    # what leaves a window that the stream keeps refilling: the smallest keys
    # (the denormal distance is the smallest of its L2 scan; under IP it lies in the middle of the order)
    early = {0: ["-nan"] + (["-inf"] if ip else ["+0"]), 1: [] if ip else ["denormal"]}
    for rescore, k in ((4, 40), (30, 12)):  # (rescore + k - 1 > 40: every victim is pushed)
        oi, od = check(gpu_ctx, c, q, L=L, rescore=rescore, k=k)
        for qi, classes in early.items():
            assert_classes([int(b) for b in od[qi].view(np.uint32)], classes, ("batch", distance, rescore, qi))
    # 60 rows, k 70: the scans end inside the call and the window drains, +inf and the NaN with the sign clear included
    c, q, wanted = special(distance, n=60)
    for rescore in (4, 30):
        oi, od = check(gpu_ctx, c, q, L=L, rescore=rescore, k=70, expect_rows=lambda r: (r < 70).all() and (r >= 40).all())
        for qi, classes in wanted.items():
            live = oi[qi] != 0xFFFFFFFF
            assert_classes([int(b) for b in od[qi].view(np.uint32)[live]], classes, ("batch, drained", distance, rescore, qi))
