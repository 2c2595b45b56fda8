"""k_prepare_queries (and k_prepare_index_slice; k_row_norms at the end) on their own, bit for bit: what a search prepares of each
query — q_full and the SBQ code of the index slice — read back through vs_prepare_queries as the device rows lie, stride padding
included, against the oracle chain a search follows (preprocess_cosine of the full vector; preprocess_cosine of the raw index slice on
its own; quantize of that slice).  The cases are the launch's own edges: codes wider than the 64 words one store pass collects, the
dims at which the LDS slices drop the workgroup from 4 to 2 to 1 waves and into the opt-in LDS, the refusal past 160 KB, 2 and 4
rounds per workgroup, the scalar load of a misaligned device batch, and the special values of the cosine rule and of the quantiser.
No tolerance anywhere: u32 / u64 views, NaN equal to NaN.  Also runs on the lockstep interpreter (VS_EMU=1, tests/emu/README.md)."""
import numpy as np
import pytest

from helpers import cached_index

pytestmark = pytest.mark.gpu

EPS = np.float32(np.finfo(np.float32).eps)


def same_f32(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and bool(((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all())


def seq_norm2(v):
    """the f32 sum of squares in element order (preprocess_cosine_get_norm, AM/distance/mod.rs:225-226)"""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.cumsum(v * v, dtype=np.float32)[-1]


def stats(O, dims, bits, seed=None, unit_col=None):
    """mean / m2 / count of 300 seeded rows; column 0 constant (std == 0); unit_col: a column with mean 0 and m2 / count exactly 1"""
    rng = np.random.default_rng(dims * 10 + bits if seed is None else seed)
    X = rng.standard_normal((300, dims)).astype(np.float32)
    X[:, 0] = 0.5
    mean, m2, cnt = O.train(X, bits)
    assert mean[0] == np.float32(0.5) and m2[0] == 0
    if unit_col is not None:
        mean[unit_col], m2[unit_col] = 0.0, np.float32(cnt)
    return mean, m2, cnt


def sbq_index(ctx, O, dim_full, dim_index, bits, distance, mean, m2, cnt):
    """n = 4 rows without neighbours: the quantiser and the geometry are all a prepare needs"""
    import pgvectorscale_amd as P
    w = O.quantized_size(dim_index, bits)
    vecs = None if dim_full == dim_index else np.zeros((4, dim_full), np.float32)
    return P.DiskAnnIndex.upload(ctx, codes=np.zeros((4, w), np.uint64), nbrs=np.full((4, 4), 0xFFFFFFFF, np.uint32),
                                 heap_tids=np.ones(4, np.uint64), vecs=vecs, mean=mean, m2=m2, count=cnt, bits=bits,
                                 dim_index=dim_index, num_neighbors=4, distance_type=distance, default_start=0)


def reference(O, Q, dim_index, cosine, quantizer=None):
    """(q_full rows, index slices, codes or None) by the oracle, one query at a time"""
    Q = np.ascontiguousarray(Q, np.float32)
    full = np.stack([O.preprocess_cosine(q)[0] for q in Q]) if cosine else Q.copy()
    sl = np.ascontiguousarray(Q[:, :dim_index])
    if cosine:
        sl = np.stack([O.preprocess_cosine(s)[0] for s in sl])
    codes = None
    if quantizer is not None:
        mean, m2, cnt, bits = quantizer
        codes = O.quantize(mean, m2, cnt, bits, sl)
    return full, sl, codes


def check_rows(ix, Q, full, codes, sl=None):
    """the device rows against the reference, every word: payload bit-exact, padding zero"""
    gf, gc, gs = ix.prepare_queries(Q)
    nq, df = full.shape
    assert gf.shape[0] == nq and gf.shape[1] == (df + 3) // 4 * 4
    assert same_f32(gf[:, :df], full), np.argwhere(gf[:, :df].view(np.uint32) != full.view(np.uint32))[:5]
    assert (gf[:, df:].view(np.uint32) == 0).all(), "q_full stride padding is not zero"
    if codes is None:
        assert gc is None
    else:
        w = codes.shape[1]
        assert gc.shape == (nq, (w + 1) // 2 * 2)
        assert (gc[:, :w] == codes).all(), np.argwhere(gc[:, :w] != codes)[:5]
        assert (gc[:, w:] == 0).all(), "code stride padding is not zero"
    if sl is None:
        assert gs is None
    else:
        di = sl.shape[1]
        assert gs.shape == gf.shape and same_f32(gs[:, :di], sl)
        assert (gs[:, di:].view(np.uint32) == 0).all(), "q_index padding is not zero"


def prepare_case(ctx, O, dims, bits, nq, seed=0):
    mean, m2, cnt = stats(O, dims, bits)
    ix = sbq_index(ctx, O, dims, dims, bits, O.L2, mean, m2, cnt)
    try:
        rng = np.random.default_rng(1000 + dims + seed)
        Q = rng.standard_normal((nq, dims)).astype(np.float32)
        Q[0] = mean
        if nq > 2:
            Q[2, 0] = 0.6
            Q[2, -1] = 1e30
        full, _, codes = reference(O, Q, dims, False, (mean, m2, cnt, bits))
        check_rows(ix, Q, full, codes)
    finally:
        ix.close()


# 1 bit: 1, 63, 64, 65, 128, 129 and 250 words (64 words are collected on lanes per store pass); 2 bits: 63, 64, 65, 128; 3 bits: 3
# (dim_full % 4 != 0: the scalar load and its padding) and 66
@pytest.mark.parametrize("dims,bits", [(64, 1), (4032, 1), (4096, 1), (4160, 1), (8192, 1), (8256, 1), (16000, 1),
                                       (2016, 2), (2048, 2), (2080, 2), (4096, 2), (50, 3), (1400, 3)])
def test_code_widths(gpu_ctx, oracle, dims, bits):
    prepare_case(gpu_ctx, oracle, dims, bits, nq=5)


# launch_prepare_queries: bytes of LDS = shared + nw * per_wave, r = dims rounded up to 4.
#   2 bits: 8 r + nw (8 r + 16).  nw 4: 40 r + 64 <= 65536 <=> r <= 1636;  nw 2: 24 r + 32 <= 65536 <=> r <= 2729 (2728);
#           nw 1: 16 r + 16 <= 65536 <=> r <= 4095 (4092), beyond that the opt-in path up to 16 r + 16 <= 163840 <=> r <= 10239 (10236)
#   1 bit:  4 r + nw (4 r + 16).  nw 4: 20 r + 64 <= 65536 <=> r <= 3273 (3272);  nw 2: 12 r + 32 <= 65536 <=> r <= 5458 (5456);
#           nw 1: 8 r + 16 <= 65536 <=> r <= 8190 (8188)
# nq = 5: nw starts at 4 and the last workgroup is partial.
@pytest.mark.parametrize("dims,bits", [(1636, 2), (1640, 2), (2728, 2), (2732, 2), (4092, 2), (4096, 2), (10236, 2),
                                       (3272, 1), (3276, 1), (5456, 1), (5460, 1), (8188, 1), (8192, 1)])
def test_wave_count_boundaries(gpu_ctx, oracle, dims, bits):
    prepare_case(gpu_ctx, oracle, dims, bits, nq=5, seed=1)


@pytest.mark.parametrize("nq", [1, 2, 3])
@pytest.mark.parametrize("bits", [1, 2])
def test_fewer_queries_than_waves(gpu_ctx, oracle, nq, bits):
    prepare_case(gpu_ctx, oracle, 128, bits, nq=nq, seed=2)


def test_refusal_past_the_lds_limit(gpu_ctx, oracle):
    """2 bits, 10240 dims: 16 r + 16 = 163856 bytes > 160 KB.  The refusal is a host-side check in front of the launch; the handle
    stays usable for what needs no LDS staging."""
    import pgvectorscale_amd as P
    O, dims, bits = oracle, 10240, 2
    mean, m2, cnt = stats(O, dims, bits)
    ix = sbq_index(gpu_ctx, O, dims, dims, bits, O.L2, mean, m2, cnt)
    try:
        Q = np.random.default_rng(5).standard_normal((3, dims)).astype(np.float32)
        with pytest.raises(P.VsError, match="10240"):
            ix.prepare_queries(Q)
        with pytest.raises(P.VsError, match="10240"):
            ix.search_batch(Q, search_list_size=4, rescore=0, k=2)
        assert (ix.quantize(Q) == O.quantize(mean, m2, cnt, bits, Q)).all()
    finally:
        ix.close()


# rounds = 2 from 8192 queries, 4 from 65536: the staged statistics are reused and the last workgroup idles waves through the barriers
@pytest.mark.parametrize("nq", [8191, 8192, 8197, 65541])
@pytest.mark.parametrize("dims,bits", [(8, 1), (12, 2)])
def test_rounds(gpu_ctx, oracle, dims, bits, nq):
    O = oracle
    mean, m2, cnt = stats(O, dims, bits)
    ix = sbq_index(gpu_ctx, O, dims, dims, bits, O.L2, mean, m2, cnt)
    try:
        base = np.random.default_rng(nq).standard_normal((301, dims)).astype(np.float32)  # 301 distinct rows, tiled (301 is prime)
        base[0] = mean
        full, _, codes = reference(O, base, dims, False, (mean, m2, cnt, bits))
        rep = np.arange(nq) % 301
        check_rows(ix, base[rep], full[rep], codes[rep])
    finally:
        ix.close()


def quantiser_edge_queries(mean, m2, cnt, bits, dims):
    """one query per edge; columns: 0 has std == 0, 1 has mean 0 and std exactly 1, 5 is ordinary"""
    rng = np.random.default_rng(dims + bits)
    inf = np.float32(np.inf)
    rows = []

    def row(**at):
        q = rng.standard_normal(dims).astype(np.float32)
        for c, v in at.items():
            q[int(c[1:])] = v
        rows.append(q)

    rows.append(mean.copy())                                   # the query equal to the mean
    row(c0=mean[0])                                            # x == mean, std == 0: 0 / 0
    row(c0=np.nextafter(mean[0], inf), c5=np.nextafter(mean[5], inf))
    row(c0=np.nextafter(mean[0], -inf), c5=np.nextafter(mean[5], -inf))
    row(c5=mean[5])
    for v in (1e30, -1e30, np.inf, -np.inf, -0.0):
        rows.append(np.full(dims, v, np.float32))
        row(c0=v, c1=v, c5=v)
    # index = ((x - mu) / sigma + 2) / (4 / (bits + 1)) exactly on t = 1, 2, bits on column 1 (mu = 0, sigma = 1), and one step below
    step = np.float32(4.0) / np.float32(bits + 1)
    for t in (1, 2, bits):
        s = np.float32(t) * step
        x = s - np.float32(2.0)
        sigma = np.sqrt(m2[1] / np.float32(cnt))
        assert sigma == 1 and ((x - mean[1]) / sigma + np.float32(2.0)) / step == np.float32(t)   # the construction holds in f32
        row(c1=x)
        row(c1=np.nextafter(x, -inf))
        row(c1=np.nextafter(x, inf))
    return np.stack(rows)


@pytest.mark.parametrize("bits", [1, 2, 3])
@pytest.mark.parametrize("dims", [33, 65, 128])
def test_quantiser_edges(gpu_ctx, oracle, dims, bits):
    O = oracle
    mean, m2, cnt = stats(O, dims, bits, unit_col=1)
    ix = sbq_index(gpu_ctx, O, dims, dims, bits, O.L2, mean, m2, cnt)
    try:
        Q = quantiser_edge_queries(mean, m2, cnt, bits, dims)
        full, _, codes = reference(O, Q, dims, False, (mean, m2, cnt, bits))
        check_rows(ix, Q, full, codes)
        assert (ix.quantize(Q) == codes).all()   # the sibling kernel states the same operation
    finally:
        ix.close()


def around_the_unit_band(u, n_adj):
    """u scaled to the last scale inside and the first outside norm2 in [1 - EPS n, 1 + EPS n], on both sides (f32 sequential sum)"""
    adj = EPS * np.float32(n_adj)
    lo, hi = np.float32(1.0) - adj, np.float32(1.0) + adj
    inside = lambda s: lo <= seq_norm2(u * s) <= hi  # noqa: E731
    s0 = c = np.float32(1.0) / np.sqrt(seq_norm2(u))
    for toward in (np.float32(2.0), np.float32(0.0)):  # (one dimension: the band holds four floats, 1 / |u| may miss them by an ulp)
        c = s0
        for _ in range(8):
            if inside(s0):
                break
            c = np.nextafter(c, toward)
            s0 = c if inside(c) else s0
    assert inside(s0), "no scale near 1 / |u| puts the vector inside the band"
    out = []
    for toward in (np.float32(2.0), np.float32(0.0)):
        s = s0
        for _ in range(100000):
            nxt = np.nextafter(s, toward)
            if not inside(nxt):
                break
            s = nxt
        assert inside(s) and not inside(nxt)
        out += [u * s, u * nxt]
    return out


def cosine_edge_vectors(n, seed):
    """the vectors the cosine rule treats specially, of dimension n"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n).astype(np.float32)
    one_hot = np.zeros(n, np.float32)
    one_hot[n // 2] = 1.0
    nan = g.copy()
    nan[n - 1] = np.nan
    rows = [np.zeros(n, np.float32), np.full(n, 1e-5, np.float32), one_hot, g, np.full(n, 1e20, np.float32), nan,
            np.full(n, -0.0, np.float32)]
    rows += around_the_unit_band(g, n)
    assert seq_norm2(rows[1]) < EPS and np.isinf(seq_norm2(rows[4]))
    if n >= 2:  # norm2 exactly EPS (2^-24 + 2^-24): the first float that is NOT below the threshold
        at_eps = np.zeros(n, np.float32)
        at_eps[0] = at_eps[n - 1] = 2.0 ** -12
        assert seq_norm2(at_eps) == EPS
        rows.append(at_eps)
    return rows


def cosine_edge_queries(dim_full, dim_index, seed):
    rows = cosine_edge_vectors(dim_full, seed)
    if dim_index < dim_full:
        rng = np.random.default_rng(seed + 1)
        tail = dim_full - dim_index
        # the slice on each edge (all zero first) under a full vector whose norm is ordinary
        for s in cosine_edge_vectors(dim_index, seed + 2):
            rows.append(np.concatenate([s, rng.standard_normal(tail).astype(np.float32)]))
        # the reverse: an ordinary slice in front of a tail that is all zero / that overflows the full norm
        rows.append(np.concatenate([rng.standard_normal(dim_index).astype(np.float32), np.zeros(tail, np.float32)]))
        rows.append(np.concatenate([rng.standard_normal(dim_index).astype(np.float32), np.full(tail, 1e20, np.float32)]))
        rows.append(np.concatenate([np.zeros(dim_index, np.float32), np.full(tail, 1e20, np.float32)]))
    return np.stack(rows)


COSINE_SHAPES = [(3, 3), (64, 64), (100, 100), (96, 64), (10, 3)]


@pytest.mark.parametrize("dim_full,dim_index", COSINE_SHAPES)
def test_cosine_edges(gpu_ctx, oracle, dim_full, dim_index):
    """statistics trained on raw (L2-style) rows, distance cosine: two independent normalisations when dim_index < dim_full"""
    O, bits = oracle, 2
    mean, m2, cnt = stats(O, dim_index, bits, seed=dim_full)
    ix = sbq_index(gpu_ctx, O, dim_full, dim_index, bits, O.COSINE, mean, m2, cnt)
    try:
        Q = cosine_edge_queries(dim_full, dim_index, seed=dim_full * 7)
        full, _, codes = reference(O, Q, dim_index, True, (mean, m2, cnt, bits))
        check_rows(ix, Q, full, codes)
    finally:
        ix.close()


@pytest.mark.parametrize("dim_full,dim_index", [(96, 64), (10, 3)])
def test_plain_storage_index_slice(gpu_ctx, oracle, dim_full, dim_index):
    import pgvectorscale_amd as P
    O = oracle
    ix = P.DiskAnnIndex.upload(gpu_ctx, codes=None, nbrs=np.full((4, 4), 0xFFFFFFFF, np.uint32), heap_tids=np.ones(4, np.uint64),
                               vecs=np.zeros((4, dim_full), np.float32), mean=None, m2=None, count=0, bits=None, dim_index=dim_index,
                               num_neighbors=4, distance_type=P.VS_COSINE, default_start=0, storage_type=P._lib.VS_STORAGE_PLAIN)
    try:
        Q = cosine_edge_queries(dim_full, dim_index, seed=dim_full * 11)
        full, sl, _ = reference(O, Q, dim_index, True)
        check_rows(ix, Q, full, None, sl)
    finally:
        ix.close()


def test_misaligned_device_queries(gpu_ctx):
    """a device batch that starts 4 bytes into an allocation takes the scalar load at a dim that is a multiple of 4"""
    ti = cached_index(n=600, dim_full=128, bits=2, R=16, distance=1, seed=21, kind="gauss", L_build=32)
    ix = ti.upload(gpu_ctx)
    nq, L, rescore, k = 9, 20, 10, 6
    q = ti.queries(nq, seed=5, kind="gauss")
    oi, od, _ = ti.oracle.search_batch(q, L=L, rescore=rescore, k=k)
    d_q = gpu_ctx.alloc(q.nbytes + 16)
    d_ids, d_dist = gpu_ctx.alloc(nq * k * 4), gpu_ctx.alloc(nq * k * 4)
    try:
        got = []
        for shift in (0, 4):
            p = type(d_q)(d_q.value + shift)
            gpu_ctx.upload(p, q)
            ix.search_batch_dev(p, nq, L, rescore, k, d_ids, None, d_dist)
            ix.search_batch_dev_finish()
            got.append((gpu_ctx.download(d_ids, np.empty((nq, k), np.uint32)), gpu_ctx.download(d_dist, np.empty((nq, k), np.float32))))
        for gi, gd in got:
            assert (gi == oi).all() and same_f32(gd, od)
    finally:
        for p in (d_q, d_ids, d_dist):
            gpu_ctx.free(p)
        ix.close()


# ---- k_row_norms: the per-row cosine divisor every cosine rerank divides by ------------------------------------------------------
def reference_divisor(O, v):
    """0 where preprocess_cosine leaves the vector alone, else sqrt of the sequential f32 sum of squares; the rule is stated here
    because the oracle hands back the vector, not the divisor — and is held to the oracle's vector"""
    v = np.ascontiguousarray(v, np.float32)
    n2 = seq_norm2(v)
    adj = EPS * np.float32(v.size)
    s = np.float32(0.0)
    if not (n2 < EPS) and not (np.float32(1.0) - adj <= n2 <= np.float32(1.0) + adj):
        s = np.sqrt(n2)
    out, changed = O.preprocess_cosine(v)
    with np.errstate(all="ignore"):
        assert changed == (s != 0) and same_f32(out, v / s if s != 0 else v)
    return s


def norm_rows(n, dim, seed):
    pool = cosine_edge_vectors(dim, seed)
    rng = np.random.default_rng(seed)
    pool += [(rng.standard_normal(dim) * sc).astype(np.float32) for sc in (1e-3, 0.3, 1.0, 40.0, 1e15)]
    order = rng.permutation(len(pool))
    return np.stack([pool[order[i % len(pool)]] for i in range(n)])


@pytest.mark.parametrize("dim", [1, 3, 63, 64, 65, 130])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_row_norms(gpu_ctx, oracle, n, dim):
    import pgvectorscale_amd as P
    O = oracle
    X = norm_rows(n, dim, seed=n * 1000 + dim)
    w = O.quantized_size(dim, 1)
    ix = P.DiskAnnIndex.upload(gpu_ctx, codes=np.zeros((n, w), np.uint64), nbrs=np.full((n, 4), 0xFFFFFFFF, np.uint32),
                               heap_tids=np.ones(n, np.uint64), vecs=X, mean=np.zeros(dim, np.float32), m2=None, count=1, bits=1,
                               dim_index=dim, num_neighbors=4, distance_type=P.VS_COSINE, default_start=0)
    try:
        d_norm, _ = ix.array(P._lib.ARR_VNORM)
        got = gpu_ctx.download(d_norm, np.empty(n, np.float32))
        assert same_f32(got, np.array([reference_divisor(O, x) for x in X], np.float32))
        # the column overwritten through the device pointer, then refresh_norms
        Y = norm_rows(n, dim, seed=n * 1000 + dim + 500)[::-1]
        d_vecs, stride = ix.array(P._lib.ARR_VECS)
        padded = np.zeros((n, stride), np.float32)
        padded[:, :dim] = Y
        gpu_ctx.upload(d_vecs, padded)
        ix.refresh_norms()
        got = gpu_ctx.download(d_norm, np.empty(n, np.float32))
        assert same_f32(got, np.array([reference_divisor(O, y) for y in Y], np.float32))
    finally:
        ix.close()
