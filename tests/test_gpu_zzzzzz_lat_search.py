"""k_search_lat, the latency-mode SBQ search kernel (VS_LAT_SCANS; one scan per multi-wave workgroup): the stream, the
five reference counters and the rows against the oracle and against the same call with the option off, at the smallest shapes at
which the kernel can go wrong — W = 1, a partial last code word, rescore 0, a neighbor list longer than one wave, the headline code
width, deleted nodes under a visibility mask — and under every cost choice, capacity hand-over and case that must not take it."""
import contextlib

import numpy as np
import pytest

import pgvectorscale_amd as P
from helpers import cached_index
from test_gpu_parity import CONFIGS
from test_gpu_zy_plain import PlainIndex

pytestmark = pytest.mark.gpu

GEOMS = {name: CONFIGS[name] for name in ("tiny_L", "odd_words_1bit", "three_bits", "big_R", "cosine_768")}
GEOMS["deleted_masked"] = (dict(n=2000, dim_full=128, bits=2, R=32, distance=1, seed=26, kind="uniform", deleted_frac=0.1, L_build=64),
                           "uniform", 40, 20, 10)
COUNTERS = ("visited_nodes", "candidate_nodes", "quantized_distance_comparisons", "node_reads", "next_calls")


@contextlib.contextmanager
def options(**kw):
    try:
        for name, value in kw.items():
            P.set_option(name, value)
        yield
    finally:
        for name in kw:
            P.set_option(name, None)


@pytest.fixture(scope="module")
def state(gpu_ctx):
    """name -> (index arrays + oracle, uploaded index, 48 queries, the oracle's stream and the option-off rows per batch size)"""
    cache = {}

    def get(name):
        if name not in cache:
            kw, qkind, L, rescore, k = GEOMS[name]
            ti = cached_index(**kw)
            ix = ti.upload(gpu_ctx)
            if name == "deleted_masked":
                vis = (np.random.default_rng(5).random(ti.n) > 0.2).astype(np.uint8)
                ix.set_visibility(vis)
                ti.oracle.set_visibility(vis)
            q = ti.queries(48, seed=123, kind=qkind)
            ref = {}
            for nq in (1, 3, 48):  # (check_against calls this before it sets any option: the rows are the option-off path's)
                ref[nq] = (ti.oracle.stream_batch(q[:nq], L=L, m=rescore + k + 5), ix.search_batch(q[:nq], search_list_size=L, rescore=rescore, k=k))
                assert ix.last_search_info()["kernel"] != 3, "the reference rows must not come from the kernel under test"
            cache[name] = (ti, ix, q, ref)
        return cache[name]
    yield get
    for ti, ix, _, _ in cache.values():
        ti.oracle.set_visibility(None)
        ix.close()


def check_against(state, name, nq, fallback=False, **opts):
    """under VS_LAT_SCANS=64 and `opts`: the stream against the oracle's and the rows against the option-off rows (computed by the
    fixture before any option is set); -> the search info, the same after the stream and after the rows"""
    ti, ix, q, ref = state(name)
    _, _, L, rescore, k = GEOMS[name]
    (oi, oh, ost), (ri, rt, rd, rst) = ref[nq]
    with options(VS_LAT_SCANS=64, **opts):
        gi, gh, gst = ix.stream_batch(q[:nq], search_list_size=L, m=rescore + k + 5)
        info = ix.last_search_info()
        si, st, sd, sst = ix.search_batch(q[:nq], search_list_size=L, rescore=rescore, k=k)
        info2 = ix.last_search_info()  # (the launch that feeds rerank and the window: another stream length, the same kernel)
        assert all(info2[f] == info[f] for f in ("kernel", "resident", "reserved"))
    assert (gi == oi).all() and (gh == oh).all()
    for c in COUNTERS:
        assert gst[c] == ost[c], (c, gst[c], ost[c])
    assert (si == ri).all() and (st == rt).all() and (sd.view(np.uint32) == rd.view(np.uint32)).all()
    for c in COUNTERS:
        assert sst[c] == rst[c], (c, sst[c], rst[c])
    assert (gst["fallback_scans"] > 0) == fallback and (sst["fallback_scans"] > 0) == fallback
    return info


@pytest.mark.parametrize("nq", [1, 3, 48])
@pytest.mark.parametrize("name", list(GEOMS))
def test_stream_rows_and_counters(state, name, nq):
    info = check_against(state, name, nq)
    assert info["kernel"] == P._lib.VS_SEARCH_LAT_SBQ == 3  # (fails without the kernel: the parent runs the fast kernel here)
    assert info["resident"] == nq and info["reserved"][0] == 4 and info["reserved"][1] == 8


@pytest.mark.parametrize("spec", [1, 7])
@pytest.mark.parametrize("cache", [1, 8])
@pytest.mark.parametrize("waves", [2, 4, 8])
def test_cost_choices_change_nothing(state, waves, cache, spec):
    info = check_against(state, "big_R", 3, VS_LAT_WAVES=waves, VS_LAT_CACHE=cache, VS_LAT_SPEC=spec)
    assert info["kernel"] == 3 and list(info["reserved"]) == [waves, cache]


@pytest.mark.parametrize("option,value,fallback", [("VS_LAT_HEAP_LDS", 7, False), ("VS_LAT_DEDUP_SLOTS", 64, True), ("VS_LAT_VISITED", 4, True)])
def test_hand_over(state, option, value, fallback):
    """a heap that outgrows its LDS part spills and finishes; a scan that outgrows the dedup table or the visited list is re-run whole"""
    info = check_against(state, "odd_words_1bit", 48, fallback=fallback, **{option: value})
    assert info["kernel"] == 3 and (option != "VS_LAT_HEAP_LDS" or info["heap_lds"] == 7)


@pytest.mark.parametrize("case", ["65_scans", "label_keys", "plain", "unset"])
def test_not_taken(gpu_ctx, state, case):
    if case == "plain":
        pi = PlainIndex(n=600, dim=32, R=16, distance=1, seed=3, kind="uniform")
        ix, q, kw = pi.upload(gpu_ctx), np.random.default_rng(1).random((3, 32), dtype=np.float32), {}
    elif case == "label_keys":
        ti = cached_index(n=800, dim_full=32, bits=2, R=16, distance=1, seed=4, kind="uniform", n_labels=4)
        ix, q, kw = ti.upload(gpu_ctx), ti.queries(3, seed=7), dict(qlabels=[[1], [2, 3], [4]])
    else:
        ti, ix, q48, _ = state("tiny_L")
        q, kw = (np.concatenate([q48, q48[:17]]) if case == "65_scans" else q48[:3]), {}
    try:
        want = ix.search_batch(q, search_list_size=20, rescore=10, k=5, **kw)
        with options(**({} if case == "unset" else {"VS_LAT_SCANS": 64})):
            got = ix.search_batch(q, search_list_size=20, rescore=10, k=5, **kw)
            assert ix.last_search_info()["kernel"] != 3
        assert all((a.view(np.uint32) == b.view(np.uint32)).all() for a, b in zip(got[:3], want[:3]))
    finally:
        if case in ("plain", "label_keys"):
            ix.close()
