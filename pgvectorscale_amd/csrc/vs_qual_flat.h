// vs_qual_flat.h — the qualified flat scan (a part of vs_batch.hip kept in a file of its own, after vs_qual_exact.h, whose row lists,
// slot order and register list it uses): vs_search_batch_qual_flat / _dev.  The contract is the header's (include/vsgpu.h, "qualified
// flat scan"); DESIGN.md section 6p.
//
// The reference's candidate-then-rescore rule with the graph walk left out: per scan the `rescore` rows of the qualifier's list that are
// smallest by (Hamming distance of the SBQ codes, node id), then the k of those that are smallest by (exact distance, node id).  A code
// row is 1/16 of a vector row, so the list is read at 1/16 of the exact call's bytes and only `rescore` vector rows per scan follow.
//
// A Hamming distance is a small integer and the list ascends by node id, so the candidates are found by COUNTING, with no sorted list
// of `rescore` entries anywhere: k_qflat_ham gathers each code row of a slice once per tile of TQ scans, stores the distance as a u16 at
// ham[scan][list place] and counts it in the scan's histogram (LDS, then integer atomics into global memory: a sum, whatever the
// order); k_qflat_pick takes a prefix sum over the histogram to the threshold t — the smallest value with at least `rescore` rows at or
// below it — and emits, in ONE ordered pass over ham[scan][.], every place below t and the first (rescore - rows below t) places at t.
// A place's slot in the output is a popcount of the emitted places before it, so the output is the same whatever ran first.  The
// candidates' exact distances are k_rerank's (launch_rerank over the candidate arrays); k_qflat_final keeps the k smallest (key, id)
// in the register list of qx_offer and writes the scan's rows.
#pragma once
#include "vs_qual_exact.h"

enum {
    QF_WAVES = 4,
    QF_PASSES = 4,                          // 16-row passes in flight per wave
    QF_STEP = QF_WAVES * QF_PASSES * 16,    // list rows one workgroup takes per iteration
    QF_OUT_BYTES = 256 << 20,               // candidates + their distances of one chunk of scans
    QF_WS_MB = 1024                         // ham + histograms of one chunk of tiles (VS_QUAL_FLAT_WS_MB)
};

// one workgroup of k_qflat_ham: scans [p0, p0 + cnt) of the slot order against rows [r0, r1) of the list buffer; the slot's list is
// rows [lbase, lbase + m), scan p0 + j's distances ham[hoff + j m ..] and its histogram row h0 + j of the chunk
struct QfTile {
    uint64_t hoff;
    uint32_t p0, cnt, r0, r1, lbase, m, h0, pad_;
};
// one scan of a chunk, for k_qflat_pick: its distances ham[hoff .. hoff + m) over the list rows [lbase, lbase + m)
struct QfScan {
    uint64_t hoff;
    uint32_t lbase, m;
};

// ---------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------
// k_scan_topk's ownership with the rows taken through the list: 4 lanes x 16 B cover a 64-B sector of a code row, a wave 16 rows per
// pass, QF_PASSES passes in flight.  The ids of the NEXT iteration's rows are requested before this iteration's code rows are waited
// for, so an iteration waits for one dependent load, not two.  A code row wider than 8 NCH words takes several rounds of loads
// (the accumulators stay in registers).  The quad's sum is on all four of its lanes, so lane (grp, l4) reports pass l4's row: the 64
// lanes of a wave store 64 consecutive u16 of ham[scan][.] and make one LDS atomic each.  A scan beyond the tile's cnt has a zero code
// and is never reported; a row beyond r1 is never read.  bins = 64 code_stride + 1: no distance is outside the histogram.
template <int NCH, int TQ>
__global__ __launch_bounds__(QF_WAVES* WAVE) void k_qflat_ham(const uint64_t* __restrict__ codes, uint32_t code_stride, uint32_t bins,
                                                               const uint64_t* __restrict__ qcodes, const uint32_t* __restrict__ perm,
                                                               const uint32_t* __restrict__ list, const QfTile* __restrict__ tiles,
                                                               uint16_t* __restrict__ ham, uint32_t* __restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* qc = reinterpret_cast<uint64_t*>(smem);                            // [TQ][code_stride]
    uint32_t* lh = reinterpret_cast<uint32_t*>(qc + (size_t)TQ * code_stride);   // [TQ][bins]
    const QfTile t = tiles[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l4 = lane & 3, grp = lane >> 2;
    for (uint32_t i = tid; i < TQ * code_stride; i += blockDim.x) {
        const uint32_t qi = i / code_stride;
        qc[i] = qi < t.cnt ? qcodes[(size_t)perm[t.p0 + qi] * code_stride + (i - qi * code_stride)] : 0ull;
    }
    for (uint32_t i = tid; i < TQ * bins; i += blockDim.x) lh[i] = 0u;
    __syncthreads();

    const uint32_t lane_row = (uint32_t)(wave * 16 * QF_PASSES + grp);  // + 16 p: the row of pass p this lane helps to read
    uint32_t idn[QF_PASSES];
#pragma unroll
    for (int p = 0; p < QF_PASSES; ++p) {
        const uint32_t j = t.r0 + lane_row + 16u * (uint32_t)p;
        idn[p] = j < t.r1 ? list[j] : 0u;
    }
    for (uint32_t r = t.r0; r < t.r1; r += QF_STEP) {  // (the same trip count for every wave)
        uint32_t id[QF_PASSES];
        bool ok[QF_PASSES];
#pragma unroll
        for (int p = 0; p < QF_PASSES; ++p) {
            id[p] = idn[p];
            ok[p] = r + lane_row + 16u * (uint32_t)p < t.r1;
            const uint32_t jn = r + QF_STEP + lane_row + 16u * (uint32_t)p;
            idn[p] = jn < t.r1 ? list[jn] : 0u;
        }
        uint32_t acc[TQ][QF_PASSES];
#pragma unroll
        for (int qi = 0; qi < TQ; ++qi)
#pragma unroll
            for (int p = 0; p < QF_PASSES; ++p) acc[qi][p] = 0u;
        for (uint32_t w0 = 0; w0 < code_stride; w0 += 8u * NCH) {
            ulonglong2 rows[QF_PASSES][NCH];
#pragma unroll
            for (int p = 0; p < QF_PASSES; ++p) {
                const uint64_t* rp = codes + (size_t)id[p] * code_stride;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const uint32_t w = w0 + 2u * (uint32_t)l4 + 8u * (uint32_t)c;
                    rows[p][c] = (ok[p] && w < code_stride) ? *reinterpret_cast<const ulonglong2*>(rp + w) : make_ulonglong2(0, 0);
                }
            }
#pragma unroll
            for (int qi = 0; qi < TQ; ++qi) {
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const uint32_t w = w0 + 2u * (uint32_t)l4 + 8u * (uint32_t)c;
                    const ulonglong2 qv = w < code_stride ? *reinterpret_cast<const ulonglong2*>(qc + (size_t)qi * code_stride + w) : make_ulonglong2(0, 0);
#pragma unroll
                    for (int p = 0; p < QF_PASSES; ++p)
                        acc[qi][p] += (uint32_t)__popcll(rows[p][c].x ^ qv.x) + (uint32_t)__popcll(rows[p][c].y ^ qv.y);
                }
            }
        }
        const uint32_t j = r + (uint32_t)(wave * 16 * QF_PASSES + l4 * 16 + grp);  // the row this lane reports
#pragma unroll
        for (int qi = 0; qi < TQ; ++qi) {
            if ((uint32_t)qi >= t.cnt) continue;  // (wave-uniform)
            uint32_t v = 0;
#pragma unroll
            for (int p = 0; p < QF_PASSES; ++p) {
                const uint32_t h = quad_sum(acc[qi][p]);
                v = l4 == p ? h : v;
            }
            if (j < t.r1) {
                ham[t.hoff + (size_t)qi * t.m + (j - t.lbase)] = (uint16_t)v;
                atomicAdd(&lh[(uint32_t)qi * bins + v], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < t.cnt * bins; i += blockDim.x) {  // (the tile's histogram rows are consecutive)
        const uint32_t c = lh[i];
        if (c) atomicAdd(&hist[(size_t)t.h0 * bins + i], c);
    }
}

// One workgroup per scan of a chunk (block b: scan perm[b] of the batch, histogram row b).  Every wave finds the threshold for itself
// (a wave prefix sum over 64 bins at a time: no barrier), then the list is cut into four runs of consecutive places, one per wave: a
// count pass gives each wave the rows below and at the threshold before its run, a place pass the slot of every emitted place —
// (rows below t before it) + min(rows at t before it, quota) — as k_qual_list places its rows.  cand[scan][rescore] node ids,
// VS_INVALID_NODE past the |S| = min(rescore, m) emitted; cand_n[scan] = |S|.
__global__ __launch_bounds__(QF_WAVES* WAVE) void k_qflat_pick(const uint16_t* __restrict__ ham, const uint32_t* __restrict__ hist, uint32_t bins,
                                                                const QfScan* __restrict__ scans, const uint32_t* __restrict__ perm,
                                                                const uint32_t* __restrict__ list, uint32_t rescore, uint32_t* __restrict__ cand,
                                                                uint32_t* __restrict__ cand_n) {
    __shared__ uint32_t seg[QF_WAVES][2];
    const QfScan s = scans[blockIdx.x];
    const uint32_t q = perm[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t want = min(rescore, s.m);
    uint32_t* out = cand + (size_t)q * rescore;
    for (uint32_t i = want + (uint32_t)tid; i < rescore; i += blockDim.x) out[i] = VS_INVALID_NODE;
    if (tid == 0) cand_n[q] = want;
    if (want == 0) return;  // (the whole workgroup)
    const uint32_t* h = hist + (size_t)blockIdx.x * bins;
    uint32_t th = 0, below = 0;  // below: rows under the threshold
    for (uint32_t b0 = 0; b0 < bins; b0 += WAVE) {
        const uint32_t c = b0 + (uint32_t)lane < bins ? h[b0 + lane] : 0u;
        uint32_t inc = c;  // inclusive prefix over the lanes
        for (int d = 1; d < WAVE; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl((int)inc, lane >= d ? lane - d : lane, WAVE);
            if (lane >= d) inc += o;
        }
        const uint64_t reach = __ballot(below + inc >= want);
        if (reach) {
            const int src = __builtin_ctzll(reach);
            th = b0 + (uint32_t)src;
            below += (uint32_t)__builtin_amdgcn_readlane((int)(inc - c), src);
            break;
        }
        below += (uint32_t)__builtin_amdgcn_readlane((int)inc, WAVE - 1);
    }
    const uint32_t quota = want - min(below, want);  // rows AT the threshold that are taken, in list order
    const uint16_t* hr = ham + s.hoff;
    const uint32_t per = (s.m + QF_WAVES * WAVE - 1) / (QF_WAVES * WAVE) * WAVE;  // places per wave, whole 64s
    const uint32_t a = min((uint32_t)wave * per, s.m), e = min(a + per, s.m);
    uint32_t n_lt = 0, n_eq = 0;
    for (uint32_t i = a; i < e; i += WAVE) {  // (wave-uniform trip count: the ballots see every lane)
        const uint32_t v = i + (uint32_t)lane < e ? (uint32_t)hr[i + lane] : 0xFFFFFFFFu;
        n_lt += (uint32_t)__popcll(__ballot(v < th));
        n_eq += (uint32_t)__popcll(__ballot(v == th));
    }
    if (lane == 0) {
        seg[wave][0] = n_lt;
        seg[wave][1] = n_eq;
    }
    __syncthreads();
    uint32_t lt_run = 0, eq_run = 0;
    for (int w = 0; w < wave; ++w) {
        lt_run += seg[w][0];
        eq_run += seg[w][1];
    }
    const uint64_t lower = (1ull << lane) - 1;
    for (uint32_t i = a; i < e; i += WAVE) {
        const uint32_t v = i + (uint32_t)lane < e ? (uint32_t)hr[i + lane] : 0xFFFFFFFFu;
        const bool lt = v < th, eq = v == th;
        const uint64_t m_lt = __ballot(lt), m_eq = __ballot(eq);
        const uint32_t eq_before = eq_run + (uint32_t)__popcll(m_eq & lower);
        const uint32_t place = lt_run + (uint32_t)__popcll(m_lt & lower) + min(eq_before, quota);
        if ((lt || (eq && eq_before < quota)) && place < want) out[place] = list[s.lbase + i + lane];
        lt_run += (uint32_t)__popcll(m_lt);
        eq_run += (uint32_t)__popcll(m_eq);
    }
}

// One wave per scan q of the chunk: its cand_n[q] candidates with k_rerank's distances are offered, 64 at a time, to the register
// list; the k smallest by (total_cmp key, node id) are the scan's rows.  Entries past the rows returned: VS_INVALID_NODE / 0 / NaN.
__global__ __launch_bounds__(WAVE) void k_qflat_final(const uint32_t* __restrict__ cand, const uint32_t* __restrict__ cand_n,
                                                      const float* __restrict__ dist, uint32_t rescore, uint32_t k, const uint64_t* __restrict__ tids,
                                                      uint32_t* __restrict__ out_ids, uint64_t* __restrict__ out_tids, float* __restrict__ out_dist,
                                                      uint32_t* __restrict__ out_rows) {
    const int lane = threadIdx.x;
    const uint32_t q = blockIdx.x, n = min(cand_n[q], rescore);
    const uint32_t* ids = cand + (size_t)q * rescore;
    const float* d = dist + (size_t)q * rescore;
    uint64_t a = ~0ull, th = ~0ull;
    for (uint32_t i = 0; i < n; i += WAVE) {  // (wave-uniform trip count)
        const uint32_t j = i + (uint32_t)lane;
        const uint64_t e = j < n ? ((uint64_t)plain_key(d[j]) << 32) | ids[j] : ~0ull;
        qx_offer(a, th, e, k, lane);
    }
    const bool have = (uint32_t)lane < k && a != ~0ull;
    const uint32_t rows = (uint32_t)__popcll(__ballot(have));
    if ((uint32_t)lane < k) {
        const uint32_t id = have ? (uint32_t)a : VS_INVALID_NODE;
        const size_t o = (size_t)q * k + lane;
        if (out_ids) out_ids[o] = id;
        if (out_tids) out_tids[o] = have && tids ? tids[id] : 0ull;
        if (out_dist) out_dist[o] = have ? plain_unkey((uint32_t)(a >> 32)) : __uint_as_float(0x7FC00000u);
    }
    if (lane == 0) out_rows[q] = rows;
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static uint32_t qf_bins(const vs_index* ix) { return 64u * ix->code_stride + 1u; }

// the largest tile (8, 4, 2, 1) not above `want` whose query codes and histograms fit the LDS budget of the exact call; 0: not even one
static uint32_t qf_tile_queries(const vs_index* ix, uint32_t want) {
    const size_t per = (size_t)ix->code_stride * 8 + (size_t)qf_bins(ix) * 4;
    if (per > QX_LDS_BUDGET) return 0;
    uint32_t tq = 8;
    while (tq > 1 && (tq > want || (size_t)tq * per > QX_LDS_BUDGET)) tq >>= 1;
    return tq;
}

struct QfHamArgs {
    uint32_t blocks, bins;
    size_t lds;
    const uint32_t *perm, *list;
    const QfTile* tiles;
    uint16_t* ham;
    uint32_t* hist;
};
template <int NCH, int TQ>
static void qf_launch_ham(const vs_index* ix, const QfHamArgs& a) {
    hipLaunchKernelGGL((k_qflat_ham<NCH, TQ>), dim3(a.blocks), dim3(QF_WAVES * WAVE), a.lds, ix->ctx->stream, (const uint64_t*)ix->codes,
                       ix->code_stride, a.bins, (const uint64_t*)ix->ws.qcodes.p, a.perm, a.list, a.tiles, a.ham, a.hist);
}
template <int NCH>
static void qf_launch_ham_tq(const vs_index* ix, uint32_t tq, const QfHamArgs& a) {
    switch (tq) {
        case 8: qf_launch_ham<NCH, 8>(ix, a); break;
        case 4: qf_launch_ham<NCH, 4>(ix, a); break;
        case 2: qf_launch_ham<NCH, 2>(ix, a); break;
        default: qf_launch_ham<NCH, 1>(ix, a); break;
    }
}
// rows of up to 48 words are read in one round of loads, as k_scan_topk reads them; wider ones in rounds of 32 words
static void qf_launch_ham_any(const vs_index* ix, uint32_t tq, const QfHamArgs& a) {
    switch ((ix->code_stride + 7) / 8) {
        case 1: qf_launch_ham_tq<1>(ix, tq, a); break;
        case 2: qf_launch_ham_tq<2>(ix, tq, a); break;
        case 3: qf_launch_ham_tq<3>(ix, tq, a); break;
        case 5:
        case 6: qf_launch_ham_tq<6>(ix, tq, a); break;
        default: qf_launch_ham_tq<4>(ix, tq, a); break;
    }
}

// k_qflat_final under a group rule (vs_qual_group.h, included after this file): the same candidates and distances
static void gx_launch_final(const vs_index* ix, uint32_t cq, const uint32_t* d_cand, const uint32_t* d_cand_n, const float* d_dist, uint32_t rescore,
                            uint32_t k, const GroupRule& gr, uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, uint32_t* d_out_rows);
// ... and for k up to VS_QUAL_WIDE_MAX_K (vs_qual_wide.h, included after this file): k_qflat_final_wide sorts the candidates in LDS
static void qw_launch_final(const vs_index* ix, uint32_t cq, const uint32_t* d_cand, const uint32_t* d_cand_n, const float* d_dist, uint32_t rescore,
                            uint32_t k, uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, uint32_t* d_out_rows);

// a run of tiles whose distances and histograms fit the workspace budget together
struct QfChunk {
    uint32_t tile0 = 0, tiles = 0, p0 = 0, scans = 0;
    uint64_t ham = 0;  // u16 elements
};

// One chunk of scans: cq scans whose raw queries, and whose outputs, are on the device; slots HOST.  Leaves its launches on the stream.
// gr.grouped: k_qflat_final_grouped keeps the k best of the candidates under the rule; wide: k_qflat_final_wide keeps the k <=
// VS_QUAL_WIDE_MAX_K best; everything before it is the same.
static int qf_run_chunk(vs_index* ix, const QxLists& ls, const float* d_queries, const uint32_t* slots, uint32_t cq, uint32_t k, uint32_t rescore,
                        uint32_t tq, uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, uint32_t* d_out_rows, vs_qual_flat_stats* st,
                        const GroupRule& gr, bool wide) {
    vs_ctx* c = ix->ctx;
    SearchWorkspace& w = ix->ws;
    const uint32_t bins = qf_bins(ix);
    VS_TRY(devbuf_reserve(c, w.q_full, (size_t)cq * ix->vec_stride * 4));
    VS_TRY(devbuf_reserve(c, w.qcodes, (size_t)cq * ix->code_stride * 8));
    VS_TRY(launch_prepare_queries(ix, d_queries, cq, (float*)w.q_full.p, (uint64_t*)w.qcodes.p));
    std::vector<uint32_t> perm(cq), first;
    qx_slot_order(ls, slots, cq, perm.data(), &first);
    // slices: as many as fill the device given the tiles, every slice whole iterations of a workgroup; VS_QUAL_FLAT_SLICES forces it
    uint32_t n_tiles = 0;
    for (size_t i = 0; i < ls.slot.size(); ++i) n_tiles += (first[i + 1] - first[i] + tq - 1) / tq;
    const uint32_t forced = env_u32("VS_QUAL_FLAT_SLICES", 0);
    const uint32_t fill = (uint32_t)std::max(c->prop.multiProcessorCount, 1) * 4;
    const uint32_t want = forced ? forced : std::max<uint32_t>((fill + n_tiles - 1) / std::max<uint32_t>(n_tiles, 1), 1);
    const uint64_t budget = (uint64_t)env_u32("VS_QUAL_FLAT_WS_MB", QF_WS_MB) << 20;  // (0: every tile a chunk of its own)
    std::vector<QfTile> tiles;
    std::vector<QfScan> scans(cq);
    std::vector<QfChunk> chunks(1);
    uint64_t cost = 0, max_ham = 1;
    uint32_t max_scans = 1;
    for (size_t i = 0; i < ls.slot.size(); ++i) {
        const uint32_t m = ls.m[i], steps = (m + QF_STEP - 1) / QF_STEP;
        const uint32_t per = std::max<uint32_t>((steps + want - 1) / want, 1) * QF_STEP;  // rows per slice
        const uint32_t S = std::max<uint32_t>((m + per - 1) / per, 1);
        if (first[i + 1] > first[i]) st->slices = std::max<uint64_t>(st->slices, S);
        for (uint32_t p0 = first[i]; p0 < first[i + 1]; p0 += tq) {
            const uint32_t cnt = std::min(tq, first[i + 1] - p0);
            const uint64_t mine = (uint64_t)cnt * m * 2 + (uint64_t)cnt * bins * 4;
            if (chunks.back().scans && cost + mine > budget) {
                chunks.push_back(QfChunk{(uint32_t)tiles.size(), 0, p0, 0, 0});
                cost = 0;
            }
            QfChunk& ch = chunks.back();
            for (uint32_t j = 0; j < cnt; ++j) scans[p0 + j] = QfScan{ch.ham + (uint64_t)j * m, ls.off[i], m};
            for (uint32_t sl = 0; sl < S && m; ++sl) {
                tiles.push_back(QfTile{ch.ham, p0, cnt, ls.off[i] + (uint32_t)std::min<uint64_t>((uint64_t)sl * per, m), ls.off[i] + (uint32_t)std::min<uint64_t>(((uint64_t)sl + 1) * per, m),
                                       ls.off[i], m,
                                       p0 - ch.p0, 0});
                ch.tiles++;
            }
            ch.ham += (uint64_t)cnt * m;
            ch.scans += cnt;
            cost += mine;
            max_ham = std::max(max_ham, ch.ham);
            max_scans = std::max(max_scans, ch.scans);
            st->tiles++;
            st->code_reads += m;
            st->reranked += (uint64_t)cnt * std::min(rescore, m);
        }
    }
    // [scans | tiles | perm] in one upload; the candidates, their count and their distances of the cq scans
    const size_t scans_bytes = scans.size() * sizeof(QfScan), tiles_bytes = tiles.size() * sizeof(QfTile), perm_bytes = (size_t)cq * 4;
    std::vector<unsigned char> tab(scans_bytes + tiles_bytes + perm_bytes);
    memcpy(tab.data(), scans.data(), scans_bytes);
    if (tiles_bytes) memcpy(tab.data() + scans_bytes, tiles.data(), tiles_bytes);
    memcpy(tab.data() + scans_bytes + tiles_bytes, perm.data(), perm_bytes);
    VS_TRY(devbuf_reserve(c, w.qf_tab, tab.size()));
    VS_TRY(devbuf_reserve(c, w.qf_ham, max_ham * 2));
    VS_TRY(devbuf_reserve(c, w.qf_hist, (size_t)max_scans * bins * 4));
    const size_t cand_bytes = (size_t)cq * rescore * 4;
    VS_TRY(devbuf_reserve(c, w.qf_cand, 2 * cand_bytes + (size_t)cq * 4));
    VS_TRY(vs_dev_upload(c, w.qf_tab.p, tab.data(), tab.size()));
    const QfScan* d_scans = (const QfScan*)w.qf_tab.p;
    const QfTile* d_tiles = (const QfTile*)((const char*)w.qf_tab.p + scans_bytes);
    const uint32_t* d_perm = (const uint32_t*)((const char*)w.qf_tab.p + scans_bytes + tiles_bytes);
    uint32_t* d_cand = (uint32_t*)w.qf_cand.p;
    float* d_dist = (float*)((char*)w.qf_cand.p + cand_bytes);
    uint32_t* d_cand_n = (uint32_t*)((char*)w.qf_cand.p + 2 * cand_bytes);
    const size_t lds = (size_t)tq * ((size_t)ix->code_stride * 8 + (size_t)bins * 4);
    for (const QfChunk& ch : chunks) {
        if (!ch.scans) continue;
        hipEvent_t ev = prof_begin(c);
        VS_HIP(hipMemsetAsync(w.qf_hist.p, 0, (size_t)ch.scans * bins * 4, c->stream));
        if (ch.tiles)
            qf_launch_ham_any(ix, tq, QfHamArgs{ch.tiles, bins, lds, d_perm, (const uint32_t*)w.qx_list.p, d_tiles + ch.tile0, (uint16_t*)w.qf_ham.p,
                                                 (uint32_t*)w.qf_hist.p});
        prof_end(c, PK_SEARCH, ev);
        VS_HIP(hipGetLastError());
        ev = prof_begin(c);
        hipLaunchKernelGGL(k_qflat_pick, dim3(ch.scans), dim3(QF_WAVES * WAVE), 0, c->stream, (const uint16_t*)w.qf_ham.p, (const uint32_t*)w.qf_hist.p, bins,
                           d_scans + ch.p0, d_perm + ch.p0, (const uint32_t*)w.qx_list.p, rescore, d_cand, d_cand_n);
        prof_end(c, PK_ORDER, ev);
        VS_HIP(hipGetLastError());
        st->chunks++;
    }
    // the candidates' exact distances, the scans taken in slot order (the scans of a slot share rows), then the k best of each scan
    hipEvent_t ev = prof_begin(c);
    VS_TRY(launch_rerank(ix, (const float*)w.q_full.p, d_cand, nullptr, d_cand_n, rescore, cq, d_dist, 0, d_perm, false));
    prof_end(c, PK_RERANK, ev);
    ev = prof_begin(c);
    if (gr.grouped) gx_launch_final(ix, cq, d_cand, d_cand_n, d_dist, rescore, k, gr, d_out_ids, d_out_tids, d_out_dist, d_out_rows);
    else if (wide) qw_launch_final(ix, cq, d_cand, d_cand_n, d_dist, rescore, k, d_out_ids, d_out_tids, d_out_dist, d_out_rows);
    else
        hipLaunchKernelGGL(k_qflat_final, dim3(cq), dim3(WAVE), 0, c->stream, (const uint32_t*)d_cand, (const uint32_t*)d_cand_n, (const float*)d_dist, rescore, k,
                           (const uint64_t*)ix->tids, d_out_ids, d_out_tids, d_out_dist, d_out_rows);
    prof_end(c, PK_RESORT, ev);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

static int search_batch_qual_flat_impl(vs_index* ix, const float* queries, uint32_t nq, uint32_t k, uint32_t rescore, const uint32_t* qual_slots,
                                       uint32_t* out_ids, uint64_t* out_tids, float* out_dist, uint32_t* out_rows, vs_qual_flat_stats* stats,
                                       bool on_device, const char* what, const GroupRule& gr = GroupRule{}, bool wide = false) {
    VS_REQUIRE(qual_slots, "%s: qual_slots is NULL", what);
    VS_REQUIRE(out_rows, "%s: out_rows is NULL", what);
    const uint32_t max_k = wide ? VS_QUAL_WIDE_MAX_K : 64;
    VS_REQUIRE(k >= 1 && k <= max_k, "%s: k %u outside [1,%u]", what, k, max_k);
    VS_REQUIRE(rescore >= k && rescore <= VS_QUAL_FLAT_MAX_RESCORE, "%s: rescore %u outside [k = %u, %d]", what, rescore, k, VS_QUAL_FLAT_MAX_RESCORE);
    VS_REQUIRE(ix, "%s: index is NULL", what);
    VS_REQUIRE(nq == 0 || queries, "%s: queries is NULL", what);
    VS_REQUIRE_OWNER(ix, what);
    if (ix->ws.pending) {
        vs_set_error("%s: a batch of this handle is in flight (vs_search_batch_dev_finish first)", what);
        return VS_ERR_STATE;
    }
    if (ix->d.storage_type == VS_STORAGE_PLAIN || !ix->codes) {
        vs_set_error("%s: plain storage has no SBQ codes to rank by (vs_search_batch_qual_exact serves it)", what);
        return VS_ERR_STATE;
    }
    if (!ix->vecs) {
        vs_set_error("%s: needs the vector column on the device", what);
        return VS_ERR_STATE;
    }
    VS_REQUIRE(ix->d.words <= 1023, "%s: a Hamming distance over code rows of %u words does not fit 16 bits", what, ix->d.words);
    if (gr.grouped) VS_TRY(group_check(ix, what, k, gr.per_group));
    vs_ctx* c = ix->ctx;
    VS_HIP(hipSetDevice(c->device));
    std::vector<uint32_t> slots(nq);
    if (nq && on_device) VS_TRY(vs_dev_download(c, slots.data(), qual_slots, (size_t)nq * 4));  // (a bad slot is refused before any launch)
    else if (nq) memcpy(slots.data(), qual_slots, (size_t)nq * 4);
    bool all_zero = true;
    double density = 1.0;
    VS_TRY(qual_check_slots(ix, what, slots.data(), nq, &all_zero, &density));
    const uint32_t tq = qf_tile_queries(ix, std::max<uint32_t>(env_u32("VS_QUAL_FLAT_TQ", 8), 1));
    if (!tq) {
        vs_set_error("%s: one scan's histogram of %u bins does not fit the LDS", what, qf_bins(ix));
        return VS_ERR_CAPACITY;
    }
    vs_qual_flat_stats st{};
    st.tile_queries = tq;
    if (stats) *stats = st;
    if (nq == 0) return VS_OK;
    QxLists ls;
    VS_TRY(qx_build_lists(ix, slots, &ls));
    st.lists = ls.slot.size();
    for (uint32_t m : ls.m) st.rows_listed += m;
    SearchWorkspace& w = ix->ws;
    const uint32_t chunk = std::min<uint32_t>(std::min<uint32_t>(nq, QX_CHUNK_SCANS), std::max<uint32_t>(QF_OUT_BYTES / (8u * rescore), 1));
    const uint32_t dim = ix->d.dim_full;
    // (host form) [chunk][k] ids | tids | distances, then [chunk] rows
    const size_t o_tids = (size_t)chunk * k * 4, o_dist = o_tids + (size_t)chunk * k * 8, o_rows = o_dist + (size_t)chunk * k * 4;
    if (!on_device) {
        VS_TRY(devbuf_reserve(c, w.qual_out, o_rows + (size_t)chunk * 4));
        VS_TRY(devbuf_reserve(c, w.raw_q, (size_t)chunk * dim * 4));
    }
    for (uint32_t q0 = 0; q0 < nq; q0 += chunk) {
        const uint32_t cq = std::min(chunk, nq - q0);
        if (on_device) {
            VS_TRY(qf_run_chunk(ix, ls, queries + (size_t)q0 * dim, slots.data() + q0, cq, k, rescore, tq, out_ids ? out_ids + (size_t)q0 * k : nullptr,
                                out_tids ? out_tids + (size_t)q0 * k : nullptr, out_dist ? out_dist + (size_t)q0 * k : nullptr, out_rows + q0, &st, gr, wide));
            VS_HIP(hipStreamSynchronize(c->stream));  // (the next chunk's tables go into the buffers this one reads)
            continue;
        }
        char* ob = (char*)w.qual_out.p;
        VS_TRY(vs_dev_upload(c, w.raw_q.p, queries + (size_t)q0 * dim, (size_t)cq * dim * 4));
        VS_TRY(qf_run_chunk(ix, ls, (const float*)w.raw_q.p, slots.data() + q0, cq, k, rescore, tq, out_ids ? (uint32_t*)ob : nullptr,
                            out_tids ? (uint64_t*)(ob + o_tids) : nullptr, out_dist ? (float*)(ob + o_dist) : nullptr, (uint32_t*)(ob + o_rows), &st, gr, wide));
        if (out_ids) VS_TRY(vs_dev_download(c, out_ids + (size_t)q0 * k, ob, (size_t)cq * k * 4));
        if (out_tids) VS_TRY(vs_dev_download(c, out_tids + (size_t)q0 * k, ob + o_tids, (size_t)cq * k * 8));
        if (out_dist) VS_TRY(vs_dev_download(c, out_dist + (size_t)q0 * k, ob + o_dist, (size_t)cq * k * 4));
        VS_TRY(vs_dev_download(c, out_rows + q0, ob + o_rows, (size_t)cq * 4));
    }
    if (stats) *stats = st;
    return VS_OK;
}

extern "C" int vs_search_batch_qual_flat(vs_index* ix, const float* queries, uint32_t nq, uint32_t k, uint32_t rescore, const uint32_t* qual_slots,
                                         uint32_t* out_ids, uint64_t* out_tids, float* out_dist, uint32_t* out_rows, vs_qual_flat_stats* stats) {
    return vs_guard("vs_search_batch_qual_flat", [&] {
        return search_batch_qual_flat_impl(ix, queries, nq, k, rescore, qual_slots, out_ids, out_tids, out_dist, out_rows, stats, false,
                                           "vs_search_batch_qual_flat");
    });
}
extern "C" int vs_search_batch_qual_flat_dev(vs_index* ix, const float* d_queries, uint32_t nq, uint32_t k, uint32_t rescore,
                                             const uint32_t* d_qual_slots, uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist,
                                             uint32_t* d_out_rows, vs_qual_flat_stats* stats) {
    return vs_guard("vs_search_batch_qual_flat_dev", [&] {
        return search_batch_qual_flat_impl(ix, d_queries, nq, k, rescore, d_qual_slots, d_out_ids, d_out_tids, d_out_dist, d_out_rows, stats, true,
                                           "vs_search_batch_qual_flat_dev");
    });
}
