// vs_qual_group.h — the exact and the flat qualified top-k under a GROUP rule (a part of vs_batch.hip kept in a file of its own, after
// vs_qual_exact.h and vs_qual_flat.h, whose host code launches the kernels below when a call names a rule):
// vs_search_batch_qual_exact_grouped / _dev and vs_search_batch_qual_flat_grouped / _dev.  The contract is the header's
// (include/vsgpu.h, "exact and flat qualified top-k under a group rule"); DESIGN.md section 6r.
//
// "The first k rows in (key, id) order with at most per_group rows per group" — T(X) over a row set X — is a mergeable summary as plain
// top-k is: T(A u B) = T(T(A) u T(B)), and one row is inserted into T(X) without looking outside the list.  A row enters only if it
// beats entry k - 1; if its group already holds per_group entries of the list it replaces the LARGEST of them (which the row now caps
// out) or, larger than that one, is capped out itself; otherwise it is inserted in the ordinary way and the last entry falls off.  So the
// exact call's structure is kept whole — a register list per wave and query, the four lists of a workgroup merged through LDS, the
// slice partials merged per scan — and only the offer changes: gx_offer is qx_offer with each entry's group in a second register
// and the replacement.  The partial lists stay 64-bit (key, id) entries: a merge reads the groups of a list back from the column by
// node id, one gather per list, so the LDS and the workspace are sized as for the ungrouped call.
#pragma once
#include "vs_qual_flat.h"

// qx_offer under the rule.  Lane L holds entry L of the ascending list (lst, ~0 = empty) and that entry's group (grp); th is entry
// k - 1; lane L offers e with group eg.  The pre-filter stands: th never grows, so a row that does not beat it now never will.  Per
// offered (kk, gg): `same` are the lanes below k whose entry is of group gg — none for VS_GROUP_NONE, and an empty entry is of no
// group.  With per_group of them the candidate either loses to the last of them (dropped) or takes that one's place in the list: the
// entries from pos to the replaced lane move up one lane, the lanes beyond keep theirs.  With fewer, every lane from pos on moves up
// (last = 63), which is qx_offer's insertion.  Equal entries do not occur (a node is offered once).  Called in wave-uniform control flow.
__device__ __forceinline__ void gx_offer(uint64_t& lst, uint32_t& grp, uint64_t& th, uint64_t e, uint32_t eg, uint32_t k, uint32_t per_group, int lane) {
    uint64_t hit = __ballot(e < th);
    while (hit) {
        const int src = __builtin_ctzll(hit);
        hit &= hit - 1;
        const uint64_t kk = qx_readlane64(e, src);
        if (!(kk < th)) continue;
        const uint32_t gg = (uint32_t)__builtin_amdgcn_readlane((int)eg, src);
        const uint64_t same = gg == VS_GROUP_NONE ? 0ull : __ballot((uint32_t)lane < k && lst != ~0ull && grp == gg);
        int last = WAVE - 1;  // the last lane that takes its lower neighbour's entry
        if ((uint32_t)__popcll(same) >= per_group) {
            last = 63 - __builtin_clzll(same);
            if (kk > qx_readlane64(lst, last)) continue;  // per_group smaller rows of its group: capped out
        }
        const int pos = (int)__popcll(__ballot(lst < kk));  // (<= last: kk is below the entry there)
        const uint64_t up = __shfl(lst, lane - 1, WAVE);
        const uint32_t upg = (uint32_t)__shfl((int)grp, lane - 1, WAVE);
        const bool keep = lane < pos || lane > last;
        lst = keep ? lst : (lane == pos ? kk : up);
        grp = keep ? grp : (lane == pos ? gg : upg);
        th = qx_readlane64(lst, (int)k - 1);
    }
}

// the group of a list entry read back from the column (an empty entry names no node)
__device__ __forceinline__ uint32_t gx_group_of(const uint32_t* __restrict__ groups, uint64_t e) {
    return (uint32_t)e != VS_INVALID_NODE ? groups[(uint32_t)e] : VS_GROUP_NONE;
}

// the rows of a finished list (lane L: entry L) as scan q's output, as k_qual_exact_merge and k_qflat_final write them
__device__ __forceinline__ void gx_write_rows(uint64_t a, uint32_t q, uint32_t k, int lane, const uint64_t* __restrict__ tids,
                                              uint32_t* __restrict__ out_ids, uint64_t* __restrict__ out_tids, float* __restrict__ out_dist,
                                              uint32_t* __restrict__ out_rows) {
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

// k_qual_exact under the rule: its tiles, ownership, operation order and partial lists ([gridDim.x][TQ][k] 64-bit entries).  The row's
// group is loaded once per row beside its id — the 8 lanes of a row's group name one address — and every query's offer carries it; the
// lists of the four waves are merged through LDS with the groups read back from the column.
template <int TQ>
__global__ __launch_bounds__(256) void k_qual_exact_grouped(const float* __restrict__ vecs, uint32_t vec_stride, uint32_t dim_full,
                                                            const float* __restrict__ vnorm, uint32_t distance_type,
                                                            const float* __restrict__ q_full, const uint32_t* __restrict__ perm,
                                                            const uint32_t* __restrict__ list, const QxTile* __restrict__ tiles, uint32_t k,
                                                            const uint32_t* __restrict__ groups, uint32_t per_group,
                                                            uint64_t* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* qv = reinterpret_cast<float*>(smem);
    const QxTile t = tiles[blockIdx.x];
    for (int qi = 0; qi < TQ; ++qi) {
        const float* src = q_full + (size_t)((uint32_t)qi < t.cnt ? perm[t.p0 + qi] : 0u) * vec_stride;
        for (uint32_t i = threadIdx.x; i < vec_stride; i += 256) qv[(size_t)qi * vec_stride + i] = (uint32_t)qi < t.cnt ? src[i] : 0.0f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l8 = lane & 7, grp = lane >> 3;
    const uint32_t steps = dim_full / 32;
    uint64_t lst[TQ], th[TQ];
    uint32_t lg[TQ];
#pragma unroll
    for (int qi = 0; qi < TQ; ++qi) {
        lst[qi] = th[qi] = ~0ull;
        lg[qi] = VS_GROUP_NONE;
    }
    for (uint32_t r = t.r0; r < t.r1; r += QX_PASS) {  // (the same trip count for every wave)
        const uint32_t j = r + (uint32_t)(wave * 8 + grp);
        const bool valid = j < t.r1;
        const uint32_t id = valid ? list[j] : 0u;
        const uint32_t rg = valid ? groups[id] : VS_GROUP_NONE;
        const float* row = vecs + (size_t)id * vec_stride;
        float s = 0.0f;
        if (valid && distance_type == VS_COSINE) s = vnorm[id];
        float acc[TQ][4];
#pragma unroll
        for (int qi = 0; qi < TQ; ++qi) acc[qi][0] = acc[qi][1] = acc[qi][2] = acc[qi][3] = 0.f;
        if (valid) {
            if (distance_type == VS_L2) {
                for (uint32_t st = 0; st < steps; ++st) {
                    const float4 x = *reinterpret_cast<const float4*>(row + 32 * st + 4 * l8);
#pragma unroll
                    for (int qi = 0; qi < TQ; ++qi) {
                        const float4 y = *reinterpret_cast<const float4*>(qv + (size_t)qi * vec_stride + 32 * st + 4 * l8);
                        const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
                        const float p0 = d0 * d0, p1 = d1 * d1, p2 = d2 * d2, p3 = d3 * d3;
                        acc[qi][0] = acc[qi][0] + p0;
                        acc[qi][1] = acc[qi][1] + p1;
                        acc[qi][2] = acc[qi][2] + p2;
                        acc[qi][3] = acc[qi][3] + p3;
                    }
                }
            } else {
                for (uint32_t st = 0; st < steps; ++st) {
                    float4 x = *reinterpret_cast<const float4*>(row + 32 * st + 4 * l8);
                    if (s != 0.0f) {  // one division per element serves the TQ queries
                        x.x = x.x / s;
                        x.y = x.y / s;
                        x.z = x.z / s;
                        x.w = x.w / s;
                    }
#pragma unroll
                    for (int qi = 0; qi < TQ; ++qi) {
                        const float4 y = *reinterpret_cast<const float4*>(qv + (size_t)qi * vec_stride + 32 * st + 4 * l8);
                        acc[qi][0] = __builtin_fmaf(x.x, y.x, acc[qi][0]);
                        acc[qi][1] = __builtin_fmaf(x.y, y.y, acc[qi][1]);
                        acc[qi][2] = __builtin_fmaf(x.z, y.z, acc[qi][2]);
                        acc[qi][3] = __builtin_fmaf(x.w, y.w, acc[qi][3]);
                    }
                }
            }
        }
        const int g0 = lane & ~7;
#pragma unroll
        for (int qi = 0; qi < TQ; ++qi) {
            if ((uint32_t)qi >= t.cnt) continue;  // (wave-uniform)
            // horizontal_add_ps of accumulator j lives on lanes (2j, 2j+1) of the group, then the four sums left to right
            const float s0 = acc[qi][0] + __shfl(acc[qi][0], lane ^ 1, WAVE);
            const float s1 = acc[qi][1] + __shfl(acc[qi][1], lane ^ 1, WAVE);
            const float s2 = acc[qi][2] + __shfl(acc[qi][2], lane ^ 1, WAVE);
            const float s3 = acc[qi][3] + __shfl(acc[qi][3], lane ^ 1, WAVE);
            const float t0 = s0 + s1;
            const float t1 = s2 + s3;
            const float h = t0 + t1;
            const float h0 = __shfl(h, g0 + 0, WAVE), h1 = __shfl(h, g0 + 2, WAVE), h2 = __shfl(h, g0 + 4, WAVE), h3 = __shfl(h, g0 + 6, WAVE);
            float dist = h0 + h1;
            dist = dist + h2;
            dist = dist + h3;
            uint64_t e = ~0ull;
            if (valid && l8 == 0) {
                const float* y = qv + (size_t)qi * vec_stride;
                for (uint32_t i = steps * 32; i < dim_full; ++i) {  // scalar tail, in element order
                    float x = row[i];
                    if (distance_type == VS_L2) {
                        const float diff = x - y[i];
                        const float p = diff * diff;
                        dist = dist + p;
                    } else {
                        if (s != 0.0f) x = x / s;
                        const float p = x * y[i];
                        dist = dist + p;
                    }
                }
                float res;
                if (distance_type == VS_L2) res = dist;
                else if (distance_type == VS_IP) res = -dist;
                else res = fmaxf(1.0f - dist, 0.0f);
                e = ((uint64_t)plain_key(res) << 32) | id;
            }
            gx_offer(lst[qi], lg[qi], th[qi], e, rg, k, per_group, lane);
        }
    }
    // the four lists of a query become one: through LDS (the queries are done with), wave w merging the queries w, w + 4, ..  Wave 0's
    // list is the start, the other three are offered to it; the groups of all four come from the column.
    __syncthreads();
    uint64_t* mg = reinterpret_cast<uint64_t*>(smem);  // [4][TQ][k]
#pragma unroll
    for (int qi = 0; qi < TQ; ++qi)
        if ((uint32_t)lane < k) mg[((size_t)wave * TQ + qi) * k + lane] = lst[qi];
    __syncthreads();
    for (int qi = wave; qi < TQ; qi += 4) {
        uint64_t a = (uint32_t)lane < k ? mg[(size_t)qi * k + lane] : ~0ull;
        uint32_t ag = gx_group_of(groups, a);
        uint64_t ath = qx_readlane64(a, (int)k - 1);
        for (int w2 = 1; w2 < 4; ++w2) {
            const uint64_t e = (uint32_t)lane < k ? mg[((size_t)w2 * TQ + qi) * k + lane] : ~0ull;
            gx_offer(a, ag, ath, e, gx_group_of(groups, e), k, per_group, lane);
        }
        if ((uint32_t)lane < k) part[((size_t)blockIdx.x * TQ + qi) * k + lane] = a;
    }
}

// k_qual_exact_merge under the rule: one wave per scan p of the slot order folds its S partial lists (each the T of its slice) with
// gx_offer, the groups of every list gathered from the column by node id, and writes the rows of scan perm[p].
__global__ __launch_bounds__(WAVE) void k_qual_exact_merge_grouped(const uint64_t* __restrict__ part, const uint32_t* __restrict__ mbase,
                                                                   const uint32_t* __restrict__ mslices, const uint32_t* __restrict__ perm,
                                                                   uint32_t tq, uint32_t k, const uint32_t* __restrict__ groups,
                                                                   uint32_t per_group, const uint64_t* __restrict__ tids,
                                                                   uint32_t* __restrict__ out_ids, uint64_t* __restrict__ out_tids,
                                                                   float* __restrict__ out_dist, uint32_t* __restrict__ out_rows) {
    const int lane = threadIdx.x;
    const uint32_t p = blockIdx.x, S = mslices[p];
    const uint64_t* mine = part + (size_t)mbase[p] * k;
    uint64_t a = (uint32_t)lane < k ? mine[lane] : ~0ull;
    uint32_t ag = gx_group_of(groups, a);
    uint64_t th = qx_readlane64(a, (int)k - 1);
    for (uint32_t sl = 1; sl < S; ++sl) {
        const uint64_t e = (uint32_t)lane < k ? mine[(size_t)sl * tq * k + lane] : ~0ull;
        gx_offer(a, ag, th, e, gx_group_of(groups, e), k, per_group, lane);
    }
    gx_write_rows(a, perm[p], k, lane, tids, out_ids, out_tids, out_dist, out_rows);
}

// k_qflat_final under the rule: one wave per scan q of the chunk; its cand_n[q] candidates with k_rerank's distances and their groups,
// gathered beside the ids, are offered 64 at a time.  The rule applies to these candidates only (the Hamming selection knows no groups).
__global__ __launch_bounds__(WAVE) void k_qflat_final_grouped(const uint32_t* __restrict__ cand, const uint32_t* __restrict__ cand_n,
                                                              const float* __restrict__ dist, uint32_t rescore, uint32_t k,
                                                              const uint32_t* __restrict__ groups, uint32_t per_group,
                                                              const uint64_t* __restrict__ tids, uint32_t* __restrict__ out_ids,
                                                              uint64_t* __restrict__ out_tids, float* __restrict__ out_dist,
                                                              uint32_t* __restrict__ out_rows) {
    const int lane = threadIdx.x;
    const uint32_t q = blockIdx.x, n = min(cand_n[q], rescore);
    const uint32_t* ids = cand + (size_t)q * rescore;
    const float* d = dist + (size_t)q * rescore;
    uint64_t a = ~0ull, th = ~0ull;
    uint32_t ag = VS_GROUP_NONE;
    for (uint32_t i = 0; i < n; i += WAVE) {  // (wave-uniform trip count)
        const uint32_t j = i + (uint32_t)lane;
        const uint64_t e = j < n ? ((uint64_t)plain_key(d[j]) << 32) | ids[j] : ~0ull;
        gx_offer(a, ag, th, e, gx_group_of(groups, e), k, per_group, lane);
    }
    gx_write_rows(a, q, k, lane, tids, out_ids, out_tids, out_dist, out_rows);
}

// ---------------------------------------------------------------------------------------------------------------
// launches (declared in vs_qual_exact.h / vs_qual_flat.h, whose chunk runners call them when the batch names a rule)
// ---------------------------------------------------------------------------------------------------------------
template <int TQ>
static void gx_launch(const vs_index* ix, const QxScanLaunch& a, const GroupRule& gr) {
    hipLaunchKernelGGL(k_qual_exact_grouped<TQ>, dim3(a.blocks), dim3(256), a.lds, ix->ctx->stream, (const float*)ix->vecs, ix->vec_stride,
                       ix->d.dim_full, (const float*)ix->vnorm, ix->d.distance_type, (const float*)ix->ws.q_full.p, a.perm, a.list, a.tiles, a.k,
                       (const uint32_t*)ix->groups, gr.per_group, a.part);
}
static void gx_launch_scan(const vs_index* ix, uint32_t tq, const QxScanLaunch& a, const GroupRule& gr) {
    switch (tq) {
        case 16: gx_launch<16>(ix, a, gr); break;
        case 8: gx_launch<8>(ix, a, gr); break;
        case 4: gx_launch<4>(ix, a, gr); break;
        case 2: gx_launch<2>(ix, a, gr); break;
        default: gx_launch<1>(ix, a, gr); break;
    }
}
static void gx_launch_merge(const vs_index* ix, uint32_t cq, const uint64_t* d_part, const uint32_t* d_perm, uint32_t tq, uint32_t k, const GroupRule& gr,
                            uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, uint32_t* d_out_rows) {
    hipLaunchKernelGGL(k_qual_exact_merge_grouped, dim3(cq), dim3(WAVE), 0, ix->ctx->stream, d_part, d_perm + cq, d_perm + 2 * (size_t)cq, d_perm, tq, k,
                       (const uint32_t*)ix->groups, gr.per_group, (const uint64_t*)ix->tids, d_out_ids, d_out_tids, d_out_dist, d_out_rows);
}
static void gx_launch_final(const vs_index* ix, uint32_t cq, const uint32_t* d_cand, const uint32_t* d_cand_n, const float* d_dist, uint32_t rescore,
                            uint32_t k, const GroupRule& gr, uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, uint32_t* d_out_rows) {
    hipLaunchKernelGGL(k_qflat_final_grouped, dim3(cq), dim3(WAVE), 0, ix->ctx->stream, d_cand, d_cand_n, d_dist, rescore, k,
                       (const uint32_t*)ix->groups, gr.per_group, (const uint64_t*)ix->tids, d_out_ids, d_out_tids, d_out_dist, d_out_rows);
}

// ---------------------------------------------------------------------------------------------------------------
// the entry points: the ungrouped implementations with the rule (their checks first, then group_check's)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int vs_search_batch_qual_exact_grouped(vs_index* ix, const float* queries, uint32_t nq, uint32_t k, uint32_t per_group,
                                                  const uint32_t* qual_slots, uint32_t* out_ids, uint64_t* out_tids, float* out_dist,
                                                  uint32_t* out_rows, vs_qual_exact_stats* stats) {
    return vs_guard("vs_search_batch_qual_exact_grouped", [&] {
        return search_batch_qual_exact_impl(ix, queries, nq, k, qual_slots, out_ids, out_tids, out_dist, out_rows, stats, false,
                                            "vs_search_batch_qual_exact_grouped", GroupRule{true, per_group});
    });
}
extern "C" int vs_search_batch_qual_exact_grouped_dev(vs_index* ix, const float* d_queries, uint32_t nq, uint32_t k, uint32_t per_group,
                                                      const uint32_t* d_qual_slots, uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist,
                                                      uint32_t* d_out_rows, vs_qual_exact_stats* stats) {
    return vs_guard("vs_search_batch_qual_exact_grouped_dev", [&] {
        return search_batch_qual_exact_impl(ix, d_queries, nq, k, d_qual_slots, d_out_ids, d_out_tids, d_out_dist, d_out_rows, stats, true,
                                            "vs_search_batch_qual_exact_grouped_dev", GroupRule{true, per_group});
    });
}
extern "C" int vs_search_batch_qual_flat_grouped(vs_index* ix, const float* queries, uint32_t nq, uint32_t k, uint32_t per_group, uint32_t rescore,
                                                 const uint32_t* qual_slots, uint32_t* out_ids, uint64_t* out_tids, float* out_dist,
                                                 uint32_t* out_rows, vs_qual_flat_stats* stats) {
    return vs_guard("vs_search_batch_qual_flat_grouped", [&] {
        return search_batch_qual_flat_impl(ix, queries, nq, k, rescore, qual_slots, out_ids, out_tids, out_dist, out_rows, stats, false,
                                           "vs_search_batch_qual_flat_grouped", GroupRule{true, per_group});
    });
}
extern "C" int vs_search_batch_qual_flat_grouped_dev(vs_index* ix, const float* d_queries, uint32_t nq, uint32_t k, uint32_t per_group,
                                                     uint32_t rescore, const uint32_t* d_qual_slots, uint32_t* d_out_ids, uint64_t* d_out_tids,
                                                     float* d_out_dist, uint32_t* d_out_rows, vs_qual_flat_stats* stats) {
    return vs_guard("vs_search_batch_qual_flat_grouped_dev", [&] {
        return search_batch_qual_flat_impl(ix, d_queries, nq, k, rescore, d_qual_slots, d_out_ids, d_out_tids, d_out_dist, d_out_rows, stats, true,
                                           "vs_search_batch_qual_flat_grouped_dev", GroupRule{true, per_group});
    });
}
