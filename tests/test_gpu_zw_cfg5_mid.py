"""BASELINE.json configs[4] at a size that exercises what the 20M x 1536 run exercises, inside the default GPU tier (VERDICT r04,
"driver-witnessed parity at scale for the label path"): 4M x 1536 unit-norm mixture, SBQ 1 bit (24-word codes), 32 labels with Zipf
frequencies and 1-3 labels per vector, the index manufactured ON THE DEVICE with the label-aware build (Graph::insert: filtered +
unfiltered pass, per-label start nodes), label-filtered scans in the TABLE-LESS regime with the neighbors' label masks next to the
neighbor rows (`nbr_mask`: the default above 8M nodes, forced here) — rows, distance bits and GreedySearchStats against the oracle on 256
one- and two-label keys, the SBQ-ordered stream, and the recall of that stream against the exact filtered Hamming top-k of the flat
scan (vs_scan_topk_filtered).  Filtered-DiskANN predicate = LabelSet overlap (AM/labels/mod.rs:124-142), start nodes per label
(AM/graph/start_nodes.rs:39-48), marking before the label test (AM/sbq/storage.rs:148-172).
The filtered flat scan that serves as ground truth here is itself held to the oracle in tests/test_gpu_scan.py and test_gpu_scan_steps.py."""
import os
import sys

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1200)]
EMU = bool(os.environ.get("VS_EMU"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_configs4_4m_x_1536_label_filtered_tableless_with_neighbor_masks(gpu_ctx, oracle, monkeypatch):
    import pgvectorscale_amd as P
    from pgvectorscale_amd import _lib
    from pgvectorscale_amd.datagen import DatagenParams, fill_device, rows_numpy
    sys.path.insert(0, ROOT)
    from bench import label_start_nodes, zipf_labels
    O = oracle
    n, dim, nq, NL = (4_000_000, 1536, 256, 32) if not EMU else (3000, 1536, 24, 32)
    monkeypatch.setenv("VS_F_LDS_MAX_INS", "0")  # the table-less regime (what 20M nodes run)
    monkeypatch.setenv("VS_F_NBRMASK", "1")      # ... with the neighbors' masks in the row (default only above 8M nodes)
    gp = DatagenParams(seed=8, dim=dim)
    ix = P.DiskAnnIndex.alloc(gpu_ctx, n=n, dim_full=dim, num_neighbors=50, distance_type=P.VS_COSINE)
    try:
        assert ix.desc.bits == 1 and ix.desc.words == 24
        vp, _ = ix.array(_lib.ARR_VECS)
        fill_device(gpu_ctx, gp, 0, n, vp)
        ix.refresh_norms()
        ix.sbq_train()
        ix.sbq_quantize_corpus()
        lab_off, lab_val = zipf_labels(np, n, NL, 108, 1, 3)
        starts = label_start_nodes(np, lab_off, lab_val)
        ix.set_labels(lab_off, lab_val)  # before the build: label-aware
        ix.build_graph(search_list_size=100, max_alpha=1.2)
        ix.set_start_nodes(0, starts)
        Q = rows_numpy(gp, (1 << 40) + 9 * (1 << 20), nq)
        rng = np.random.default_rng(10)
        pz = 1.0 / np.arange(1, NL + 1)
        pz /= pz.sum()
        keys = [sorted(set(int(x) + 1 for x in rng.choice(NL, 1 if i % 2 == 0 else 2, p=pz))) for i in range(nq)]
        keys[5] = [NL]  # the rarest label
        keys[6] = [1]   # the most frequent one
        host = ix.download(vecs=True)
        mean, m2, cnt = ix.get_quantizer()
        d = ix.desc
        oidx = O.OracleIndex(codes=host["codes"], nbrs=host["nbrs"], heap_tids=host["heap_tids"], vecs=host["vecs"], mean=mean, m2=m2,
                             count=cnt, bits=d.bits, dim_index=d.dim_index, num_neighbors=d.num_neighbors, distance_type=O.COSINE,
                             default_start=d.default_start, label_off=lab_off, label_val=lab_val, label_starts=starts)
        for L, S in ((100, 90), (100, 50)):  # the benchmark's operating point for configs[4] / the reference's default GUCs
            gi, gt, gd, gst = ix.search_batch(Q, search_list_size=L, rescore=S, k=10, qlabels=keys)
            oi, od, ost = oidx.search_batch(Q, L=L, rescore=S, k=10, qlabels=keys, threads=16)
            assert (gi == oi).all(), f"label-filtered top-10 ids differ from the oracle at L={L} rescore={S}"
            assert np.allclose(gd, od, rtol=1e-5, atol=1e-7, equal_nan=True)
            assert (gd.view(np.uint32) == od.view(np.uint32)).all()
            for c in ("visited_nodes", "candidate_nodes", "quantized_distance_comparisons", "full_distance_comparisons", "node_reads",
                      "next_calls"):
                assert gst[c] == ost[c], (L, S, c, gst[c], ost[c])
        if not EMU:
            assert ix._L.vs_index_has_neighbor_masks(ix.h) == 1, "the scans did not run with the neighbors' masks"
        # every returned row satisfies the predicate
        for i in range(nq):
            for v in gi[i][gi[i] != 0xFFFFFFFF]:
                assert set(lab_val[lab_off[v]:lab_off[v + 1]].tolist()) & set(keys[i])
        # the SBQ-ordered stream before the rerank ...
        si, sh, _ = ix.stream_batch(Q, search_list_size=100, m=99, qlabels=keys)
        ti_i, ti_h, _ = oidx.stream_batch(Q, L=100, m=99, qlabels=keys, threads=16)
        assert (si == ti_i).all() and (sh == ti_h).all()
        # ... and its recall against the EXACT filtered Hamming top-10 (flat scan with the same predicate): a stream row counts when it
        # is one of the exact rows or ties with the last of them
        qn = Q / np.linalg.norm(Q, axis=1, keepdims=True)
        ei, eh = ix.scan_topk(ix.quantize(qn), 10, qlabels=keys)
        hits = 0
        for i in range(nq):
            exact = set(ei[i].tolist())
            hits += sum(1 for v, h in zip(si[i][:10], sh[i][:10]) if int(v) in exact or h <= eh[i][9])
        sbq_recall = hits / (10.0 * nq)
        print(f"configs[4] mid size: filtered SBQ stream recall@10 against the exact filtered Hamming scan: {sbq_recall:.4f}")
        assert sbq_recall >= (0.9 if not EMU else 0.5), sbq_recall
    finally:
        ix.close()
