// vs_qual_exact.h — the exact top-k over a qualifier's rows (a part of vs_batch.hip kept in a file of its own, next to vs_qual.h):
// vs_search_batch_qual_exact / _dev.  The contract is the header's (include/vsgpu.h, "exact qualified top-k"); DESIGN.md section 6o.
//
// No graph is walked.  Per distinct slot of the batch k_qual_list turns (bitmap AND live AND not hidden) into an ascending row list;
// the host groups the scans by slot (a stable permutation) and cuts each group into tiles of up to TQ scans and each list into S
// slices; k_qual_exact runs one workgroup per (tile, slice): it reads every row of its slice ONCE and applies it to the tile's TQ
// prepared queries held in LDS, in rerank_row_dist's operation order, so a distance has the bits k_rerank gives the row.  Selection
// never leaves the registers: lane L of a wave holds entry L of the wave's sorted list of (total_cmp key << 32 | node id) per query,
// an insertion is a ballot, a popcount and one shuffle, and there is no barrier inside the row loop.  (key, id) is a total order
// without equal entries, so the k smallest are the same set whichever wave, slice or order found them: the four lists of a workgroup
// are merged through LDS at the end of the slice, the S partial lists of a scan by k_qual_exact_merge, which also undoes the permutation.
#pragma once
#include "vs_device.h"

#define VS_QX_TQ 8       // scans per tile (the default; VS_QUAL_EXACT_TQ picks another instantiation for measurement)
#define VS_GX_TQ 4       // ... under a group rule: k_qual_exact_grouped<8> crosses 128 VGPRs and measured 1.8 x the time of <4>
#define VS_QX_TQ_MAX 16
enum { QX_PASS = 32, QX_LDS_BUDGET = 64 * 1024 - 256, QX_CHUNK_SCANS = 32768, QX_LIST_WORDS = 32, QX_LIST_BLOCKS = 4096 };

// ---------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------
// The rows of one slot, ascending.  A single-wave workgroup owns `wpb` consecutive words of the bitmap (bits == nullptr: slot 0, every
// word all ones); a word is 64 nodes, one per lane: the node passes when its bit is set, its tid offset is not InvalidOffsetNumber and
// the mask in force (visible, may be null) does not hide it.  One ballot per word.  Launched twice: list == nullptr counts
// (counts[b] = rows of workgroup b); list != nullptr places — the workgroup's base is the sum of the counts before it, a row's place
// the popcount of the passing lanes below it.  No atomic, so the order is the node order.
__global__ __launch_bounds__(WAVE) void k_qual_list(const uint64_t* __restrict__ bits, const uint64_t* __restrict__ tids,
                                                    const uint8_t* __restrict__ visible, uint32_t n, uint32_t wpb, uint32_t* __restrict__ counts,
                                                    uint32_t* __restrict__ list) {
    const uint32_t lane = threadIdx.x, b = blockIdx.x;
    const uint64_t n_words = ((uint64_t)n + 63) / 64;
    const uint64_t w0 = (uint64_t)b * wpb, w1 = min(w0 + wpb, n_words);
    uint32_t at = 0;
    if (list) {
        for (uint32_t j = lane; j < b; j += WAVE) at += counts[j];
        for (int m = 1; m < WAVE; m <<= 1) at += (uint32_t)__shfl_xor((int)at, m, WAVE);
    }
    for (uint64_t w = w0; w < w1; ++w) {  // (wave-uniform trip count: the ballot sees every lane)
        const uint64_t i = w * 64 + lane;
        const uint64_t word = bits ? bits[w] : ~0ull;
        bool pass = i < n && ((word >> lane) & 1ull);
        if (pass) pass = (!tids || (tids[i] & 0xFFFFull) != 0) && !(visible && visible[i] == 0);
        const uint64_t m = __ballot(pass);
        if (list && pass) list[at + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = (uint32_t)i;
        at += (uint32_t)__popcll(m);
    }
    if (!list && lane == 0) counts[b] = at;
}

// one workgroup of k_qual_exact: scans [p0, p0 + cnt) of the batch's slot order against rows [r0, r1) of the list buffer
struct QxTile {
    uint32_t p0, cnt, r0, r1;
};

__device__ __forceinline__ uint64_t qx_readlane64(uint64_t v, int src) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
}

// k_bf_fold's insertion with the list in registers: lane L holds entry L of an ascending list of 64 (~0 = empty), th is entry k - 1.
// Every lane whose e beats th is offered in lane order; an entry that still beats th goes to the place the popcount of the smaller
// entries gives it and the entries from there on move up one lane (the last falls off).  Called in wave-uniform control flow.
__device__ __forceinline__ void qx_offer(uint64_t& lst, uint64_t& th, uint64_t e, uint32_t k, int lane) {
    uint64_t hit = __ballot(e < th);
    while (hit) {
        const int src = __builtin_ctzll(hit);
        hit &= hit - 1;
        const uint64_t kk = qx_readlane64(e, src);
        if (kk < th) {
            const int pos = (int)__popcll(__ballot(lst < kk));
            const uint64_t up = __shfl(lst, lane - 1, WAVE);
            lst = lane < pos ? lst : (lane == pos ? kk : up);
            th = qx_readlane64(lst, (int)k - 1);
        }
    }
}

// The hot kernel.  4 waves; wave w, 8-lane group g take row r + 8 w + g of each 32-row pass, lane l8 of the group the elements
// 32 t + 4 l8 .. + 3 of every 32-float step: k_rerank's ownership.  The row's float4 is loaded (and, for cosine, divided by the row's
// divisor) once per step and applied to the TQ queries in LDS with four accumulators each; then, per query, rerank_row_dist's
// horizontal add, scalar tail and final form, and the offer to the wave's list.  A query beyond the tile's cnt is zeros in LDS and is
// never offered; a row beyond r1 is not read.  part: [gridDim.x][TQ][k] ascending partial lists.
template <int TQ>
__global__ __launch_bounds__(256) void k_qual_exact(const float* __restrict__ vecs, uint32_t vec_stride, uint32_t dim_full,
                                                    const float* __restrict__ vnorm, uint32_t distance_type, const float* __restrict__ q_full,
                                                    const uint32_t* __restrict__ perm, const uint32_t* __restrict__ list,
                                                    const QxTile* __restrict__ tiles, uint32_t k, uint64_t* __restrict__ part) {
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
#pragma unroll
    for (int qi = 0; qi < TQ; ++qi) lst[qi] = th[qi] = ~0ull;
    for (uint32_t r = t.r0; r < t.r1; r += QX_PASS) {  // (the same trip count for every wave)
        const uint32_t j = r + (uint32_t)(wave * 8 + grp);
        const bool valid = j < t.r1;
        const uint32_t id = valid ? list[j] : 0u;
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
            qx_offer(lst[qi], th[qi], e, k, lane);
        }
    }
    // the four lists of a query become one: through LDS (the queries are done with), wave w merging the queries w, w + 4, ..
    __syncthreads();
    uint64_t* mg = reinterpret_cast<uint64_t*>(smem);  // [4][TQ][k]
#pragma unroll
    for (int qi = 0; qi < TQ; ++qi)
        if ((uint32_t)lane < k) mg[((size_t)wave * TQ + qi) * k + lane] = lst[qi];
    __syncthreads();
    for (int qi = wave; qi < TQ; qi += 4) {
        uint64_t a = (uint32_t)lane < k ? mg[(size_t)qi * k + lane] : ~0ull;
        uint64_t ath = qx_readlane64(a, (int)k - 1);
        for (int w2 = 1; w2 < 4; ++w2) {
            const uint64_t e = (uint32_t)lane < k ? mg[((size_t)w2 * TQ + qi) * k + lane] : ~0ull;
            qx_offer(a, ath, e, k, lane);
        }
        if ((uint32_t)lane < k) part[((size_t)blockIdx.x * TQ + qi) * k + lane] = a;
    }
}

// One wave per scan p of the slot order: its S partial lists (TQ lists apart, the first at list number mbase[p]) become the k rows of
// scan perm[p] of the batch.  Entries past the rows returned: VS_INVALID_NODE / 0 / NaN.
__global__ __launch_bounds__(WAVE) void k_qual_exact_merge(const uint64_t* __restrict__ part, const uint32_t* __restrict__ mbase,
                                                           const uint32_t* __restrict__ mslices, const uint32_t* __restrict__ perm, uint32_t tq,
                                                           uint32_t k, const uint64_t* __restrict__ tids, uint32_t* __restrict__ out_ids,
                                                           uint64_t* __restrict__ out_tids, float* __restrict__ out_dist, uint32_t* __restrict__ out_rows) {
    const int lane = threadIdx.x;
    const uint32_t p = blockIdx.x, S = mslices[p];
    const uint64_t* mine = part + (size_t)mbase[p] * k;
    uint64_t a = (uint32_t)lane < k ? mine[lane] : ~0ull;
    uint64_t th = qx_readlane64(a, (int)k - 1);
    for (uint32_t sl = 1; sl < S; ++sl) {
        const uint64_t e = (uint32_t)lane < k ? mine[(size_t)sl * tq * k + lane] : ~0ull;
        qx_offer(a, th, e, k, lane);
    }
    const uint32_t q = perm[p];
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
// the largest instantiated tile (16, 8, 4, 2, 1) not above `want` whose queries — and whose four lists per query at the end of a
// slice — fit the LDS budget; the floor is one query
static uint32_t qx_tile_queries(const vs_index* ix, uint32_t k, uint32_t want) {
    const size_t per = std::max<size_t>((size_t)ix->vec_stride * 4, (size_t)4 * k * 8);
    uint32_t tq = VS_QX_TQ_MAX;
    while (tq > 1 && (tq > want || (size_t)tq * per > QX_LDS_BUDGET)) tq >>= 1;
    return tq;
}

template <int TQ>
static void qx_launch(const vs_index* ix, uint32_t blocks, size_t lds, const uint32_t* d_perm, const uint32_t* d_list, const QxTile* d_tiles, uint32_t k,
                      uint64_t* d_part) {
    hipLaunchKernelGGL(k_qual_exact<TQ>, dim3(blocks), dim3(256), lds, ix->ctx->stream, (const float*)ix->vecs, ix->vec_stride, ix->d.dim_full,
                       (const float*)ix->vnorm, ix->d.distance_type, (const float*)ix->ws.q_full.p, d_perm, d_list, d_tiles, k, d_part);
}

// The same grid and the same merge under a group rule (vs_qual_group.h, included after this file): k_qual_exact_grouped takes the
// tiles, the lists and the partial lists of k_qual_exact, k_qual_exact_merge_grouped the tables of k_qual_exact_merge.
struct QxScanLaunch {
    uint32_t blocks;
    size_t lds;
    const uint32_t *perm, *list;
    const QxTile* tiles;
    uint32_t k;
    uint64_t* part;
};
static void gx_launch_scan(const vs_index* ix, uint32_t tq, const QxScanLaunch& a, const GroupRule& gr);
static void gx_launch_merge(const vs_index* ix, uint32_t cq, const uint64_t* d_part, const uint32_t* d_perm, uint32_t tq, uint32_t k, const GroupRule& gr,
                            uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, uint32_t* d_out_rows);

// the rows of every distinct slot named (ascending slot numbers): list_off[i] .. + list_m[i] of ws.qx_list
struct QxLists {
    std::vector<uint32_t> slot, off, m;
};
static int qx_build_lists(vs_index* ix, const std::vector<uint32_t>& slots, QxLists* out) {
    vs_ctx* c = ix->ctx;
    SearchWorkspace& w = ix->ws;
    const uint32_t n = ix->d.n;
    bool named[VS_MAX_QUAL_SLOTS + 1] = {false};
    for (uint32_t s : slots) named[s] = true;
    size_t cap = 0;
    for (uint32_t s = 0; s <= VS_MAX_QUAL_SLOTS; ++s) {
        if (!named[s]) continue;
        out->slot.push_back(s);
        out->off.push_back((uint32_t)cap);
        cap += s ? (size_t)std::min<uint64_t>(ix->qs->info[s].n_set, n) : n;  // (a list is never longer than the bits set)
    }
    VS_REQUIRE(cap <= 0xFFFFFFFFull, "vs_search_batch_qual_exact: the named qualifiers list %zu rows together (at most 2^32 - 1)", cap);
    const uint64_t n_words = ((uint64_t)n + 63) / 64;
    const uint32_t nb = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n_words + QX_LIST_WORDS - 1) / QX_LIST_WORDS, 1), QX_LIST_BLOCKS);
    const uint32_t wpb = (uint32_t)((n_words + nb - 1) / nb);
    const size_t L = out->slot.size();
    VS_TRY(devbuf_reserve(c, w.qx_list, std::max<size_t>(cap, 1) * 4));
    VS_TRY(devbuf_reserve(c, w.qx_counts, L * nb * 4));
    hipEvent_t ev = prof_begin(c);
    for (size_t i = 0; i < L; ++i) {
        const uint32_t s = out->slot[i];
        uint32_t* cnt = (uint32_t*)w.qx_counts.p + i * nb;
        for (int pass = 0; pass < 2; ++pass) {
            hipLaunchKernelGGL(k_qual_list, dim3(nb), dim3(WAVE), 0, c->stream, s ? (const uint64_t*)ix->qs->bits[s] : (const uint64_t*)nullptr,
                               (const uint64_t*)ix->tids, ix->visible, n, wpb, cnt, pass ? (uint32_t*)w.qx_list.p + out->off[i] : (uint32_t*)nullptr);
        }
    }
    prof_end(c, PK_SCAN, ev);
    VS_HIP(hipGetLastError());
    std::vector<uint32_t> counts(L * nb);
    VS_TRY(vs_dev_download(c, counts.data(), w.qx_counts.p, counts.size() * 4));  // (waits for the stream)
    out->m.assign(L, 0);
    for (size_t i = 0; i < L; ++i)
        for (uint32_t b = 0; b < nb; ++b) out->m[i] += counts[i * nb + b];
    return VS_OK;
}

// the scans by slot, in their own order within a slot (a stable counting sort): perm[place] = scan, the scans of list i at the places
// first[i] .. first[i + 1]
static void qx_slot_order(const QxLists& ls, const uint32_t* slots, uint32_t cq, uint32_t* perm, std::vector<uint32_t>* first_out) {
    std::vector<uint32_t>& first = *first_out;
    first.assign(ls.slot.size() + 1, 0);
    uint32_t li_of[VS_MAX_QUAL_SLOTS + 1] = {0};
    for (size_t i = 0; i < ls.slot.size(); ++i) li_of[ls.slot[i]] = (uint32_t)i;
    for (uint32_t q = 0; q < cq; ++q) first[li_of[slots[q]] + 1]++;
    for (size_t i = 0; i < ls.slot.size(); ++i) first[i + 1] += first[i];
    std::vector<uint32_t> at(first.begin(), first.end() - 1);
    for (uint32_t q = 0; q < cq; ++q) perm[at[li_of[slots[q]]]++] = q;
}

// One chunk: cq scans whose raw queries, and whose outputs, are on the device; slots HOST.  Leaves its launches on the stream.
// gr.grouped: the same tiles and tables, the two kernels of vs_qual_group.h in place of k_qual_exact / k_qual_exact_merge.
static int qx_run_chunk(vs_index* ix, const QxLists& ls, const float* d_queries, const uint32_t* slots, uint32_t cq, uint32_t k, uint32_t tq,
                        uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, uint32_t* d_out_rows, vs_qual_exact_stats* st, const GroupRule& gr) {
    vs_ctx* c = ix->ctx;
    SearchWorkspace& w = ix->ws;
    VS_TRY(devbuf_reserve(c, w.q_full, (size_t)cq * ix->vec_stride * 4));
    VS_TRY(devbuf_reserve(c, w.qcodes, (size_t)cq * ix->code_stride * 8));
    VS_TRY(launch_prepare_queries(ix, d_queries, cq, (float*)w.q_full.p, (uint64_t*)w.qcodes.p));
    std::vector<uint32_t> tab((size_t)3 * cq), first;
    uint32_t* perm = tab.data();
    uint32_t *mbase = perm + cq, *mslices = mbase + cq;
    qx_slot_order(ls, slots, cq, perm, &first);
    // S: as many slices as fill the device given the tiles, every slice at least one pass; VS_QUAL_EXACT_SLICES forces it
    uint32_t n_tiles = 0;
    for (size_t i = 0; i < ls.slot.size(); ++i) n_tiles += (first[i + 1] - first[i] + tq - 1) / tq;
    const uint32_t forced = env_u32("VS_QUAL_EXACT_SLICES", 0);
    const uint32_t fill = (uint32_t)std::max(c->prop.multiProcessorCount, 1) * 4;
    const uint32_t want = forced ? forced : std::max<uint32_t>((fill + n_tiles - 1) / std::max<uint32_t>(n_tiles, 1), 1);
    std::vector<QxTile> tiles;
    for (size_t i = 0; i < ls.slot.size(); ++i) {
        const uint32_t m = ls.m[i], passes = (m + QX_PASS - 1) / QX_PASS;
        const uint32_t per = std::max<uint32_t>((passes + want - 1) / want, 1) * QX_PASS;  // rows per slice
        const uint32_t S = std::max<uint32_t>((m + per - 1) / per, 1);
        st->slices = std::max<uint64_t>(st->slices, S);
        for (uint32_t p0 = first[i]; p0 < first[i + 1]; p0 += tq) {
            const uint32_t cnt = std::min(tq, first[i + 1] - p0);
            for (uint32_t j = 0; j < cnt; ++j) {
                mbase[p0 + j] = (uint32_t)tiles.size() * tq + j;
                mslices[p0 + j] = S;
            }
            for (uint32_t sl = 0; sl < S; ++sl)
                tiles.push_back(QxTile{p0, cnt, ls.off[i] + std::min(sl * per, m), ls.off[i] + std::min((sl + 1) * per, m)});
            st->tiles++;
            st->row_reads += m;
        }
    }
    const size_t tab_bytes = tab.size() * 4, tiles_bytes = tiles.size() * sizeof(QxTile);
    VS_TRY(devbuf_reserve(c, w.qx_tab, tab_bytes + tiles_bytes));
    VS_TRY(devbuf_reserve(c, w.qx_part, tiles.size() * tq * k * 8));
    VS_TRY(vs_dev_upload(c, w.qx_tab.p, tab.data(), tab_bytes));
    VS_TRY(vs_dev_upload(c, (char*)w.qx_tab.p + tab_bytes, tiles.data(), tiles_bytes));
    const uint32_t* d_perm = (const uint32_t*)w.qx_tab.p;
    const QxTile* d_tiles = (const QxTile*)((const char*)w.qx_tab.p + tab_bytes);
    const size_t lds = (size_t)tq * std::max<size_t>((size_t)ix->vec_stride * 4, (size_t)4 * k * 8);
    const uint32_t blocks = (uint32_t)tiles.size();
    hipEvent_t ev = prof_begin(c);
    if (gr.grouped) {
        gx_launch_scan(ix, tq, QxScanLaunch{blocks, lds, d_perm, (const uint32_t*)w.qx_list.p, d_tiles, k, (uint64_t*)w.qx_part.p}, gr);
    } else {
        switch (tq) {
            case 16: qx_launch<16>(ix, blocks, lds, d_perm, (const uint32_t*)w.qx_list.p, d_tiles, k, (uint64_t*)w.qx_part.p); break;
            case 8: qx_launch<8>(ix, blocks, lds, d_perm, (const uint32_t*)w.qx_list.p, d_tiles, k, (uint64_t*)w.qx_part.p); break;
            case 4: qx_launch<4>(ix, blocks, lds, d_perm, (const uint32_t*)w.qx_list.p, d_tiles, k, (uint64_t*)w.qx_part.p); break;
            case 2: qx_launch<2>(ix, blocks, lds, d_perm, (const uint32_t*)w.qx_list.p, d_tiles, k, (uint64_t*)w.qx_part.p); break;
            default: qx_launch<1>(ix, blocks, lds, d_perm, (const uint32_t*)w.qx_list.p, d_tiles, k, (uint64_t*)w.qx_part.p); break;
        }
    }
    prof_end(c, PK_RERANK, ev);
    VS_HIP(hipGetLastError());
    ev = prof_begin(c);
    if (gr.grouped) gx_launch_merge(ix, cq, (const uint64_t*)w.qx_part.p, d_perm, tq, k, gr, d_out_ids, d_out_tids, d_out_dist, d_out_rows);
    else
        hipLaunchKernelGGL(k_qual_exact_merge, dim3(cq), dim3(WAVE), 0, c->stream, (const uint64_t*)w.qx_part.p, d_perm + cq, d_perm + 2 * (size_t)cq, d_perm, tq, k,
                           (const uint64_t*)ix->tids, d_out_ids, d_out_tids, d_out_dist, d_out_rows);
    prof_end(c, PK_RESORT, ev);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// The same entry checks, lists and chunks of scans for k up to VS_QUAL_WIDE_MAX_K (vs_qual_wide.h, included after vs_qual_flat.h):
// qw_run_chunk in place of qx_run_chunk, over a tile and a chunk of scans of its own choosing.
static uint32_t qw_tile_queries(const vs_index* ix, uint32_t want);
static uint32_t qw_chunk_scans(uint32_t nq, uint32_t k);
static int qw_run_chunk(vs_index* ix, const QxLists& ls, const float* d_queries, const uint32_t* slots, uint32_t cq, uint32_t k, uint32_t tq,
                        uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, uint32_t* d_out_rows, vs_qual_exact_stats* st);

static int search_batch_qual_exact_impl(vs_index* ix, const float* queries, uint32_t nq, uint32_t k, const uint32_t* qual_slots, uint32_t* out_ids,
                                        uint64_t* out_tids, float* out_dist, uint32_t* out_rows, vs_qual_exact_stats* stats, bool on_device,
                                        const char* what, const GroupRule& gr = GroupRule{}, bool wide = false) {
    VS_REQUIRE(qual_slots, "%s: qual_slots is NULL", what);
    VS_REQUIRE(out_rows, "%s: out_rows is NULL", what);
    const uint32_t max_k = wide ? VS_QUAL_WIDE_MAX_K : 64;
    VS_REQUIRE(k >= 1 && k <= max_k, "%s: k %u outside [1,%u]", what, k, max_k);
    VS_REQUIRE(ix, "%s: index is NULL", what);
    VS_REQUIRE(nq == 0 || queries, "%s: queries is NULL", what);
    VS_REQUIRE_OWNER(ix, what);
    if (ix->ws.pending) {
        vs_set_error("%s: a batch of this handle is in flight (vs_search_batch_dev_finish first)", what);
        return VS_ERR_STATE;
    }
    if (!ix->vecs) {
        vs_set_error("%s: needs the vector column on the device", what);
        return VS_ERR_STATE;
    }
    if (gr.grouped) VS_TRY(group_check(ix, what, k, gr.per_group));
    vs_ctx* c = ix->ctx;
    VS_HIP(hipSetDevice(c->device));
    std::vector<uint32_t> slots(nq);
    if (nq && on_device) VS_TRY(vs_dev_download(c, slots.data(), qual_slots, (size_t)nq * 4));  // (a bad slot is refused before any launch)
    else if (nq) memcpy(slots.data(), qual_slots, (size_t)nq * 4);
    bool all_zero = true;
    double density = 1.0;
    VS_TRY(qual_check_slots(ix, what, slots.data(), nq, &all_zero, &density));
    vs_qual_exact_stats st{};
    const uint32_t tq_want = std::max<uint32_t>(env_u32("VS_QUAL_EXACT_TQ", gr.grouped ? VS_GX_TQ : VS_QX_TQ), 1);
    const uint32_t tq = wide ? qw_tile_queries(ix, tq_want) : qx_tile_queries(ix, k, tq_want);
    st.tile_queries = tq;
    if (stats) *stats = st;
    if (nq == 0) return VS_OK;
    QxLists ls;
    VS_TRY(qx_build_lists(ix, slots, &ls));
    st.lists = ls.slot.size();
    for (uint32_t m : ls.m) st.rows_listed += m;
    SearchWorkspace& w = ix->ws;
    const uint32_t chunk = wide ? qw_chunk_scans(nq, k) : std::min<uint32_t>(nq, QX_CHUNK_SCANS);
    const uint32_t dim = ix->d.dim_full;
    auto run_chunk = [&](const float* d_q, const uint32_t* sl, uint32_t cq, uint32_t* o_ids, uint64_t* o_tid, float* o_dst, uint32_t* o_row) {
        return wide ? qw_run_chunk(ix, ls, d_q, sl, cq, k, tq, o_ids, o_tid, o_dst, o_row, &st)
                    : qx_run_chunk(ix, ls, d_q, sl, cq, k, tq, o_ids, o_tid, o_dst, o_row, &st, gr);
    };
    // (host form) [chunk][k] ids | tids | distances, then [chunk] rows
    const size_t o_tids = (size_t)chunk * k * 4, o_dist = o_tids + (size_t)chunk * k * 8, o_rows = o_dist + (size_t)chunk * k * 4;
    if (!on_device) {
        VS_TRY(devbuf_reserve(c, w.qual_out, o_rows + (size_t)chunk * 4));
        VS_TRY(devbuf_reserve(c, w.raw_q, (size_t)chunk * dim * 4));
    }
    for (uint32_t q0 = 0; q0 < nq; q0 += chunk) {
        const uint32_t cq = std::min(chunk, nq - q0);
        if (on_device) {
            VS_TRY(run_chunk(queries + (size_t)q0 * dim, slots.data() + q0, cq, out_ids ? out_ids + (size_t)q0 * k : nullptr,
                             out_tids ? out_tids + (size_t)q0 * k : nullptr, out_dist ? out_dist + (size_t)q0 * k : nullptr, out_rows + q0));
            VS_HIP(hipStreamSynchronize(c->stream));  // (the next chunk's tables go into the buffers this one reads)
            continue;
        }
        char* ob = (char*)w.qual_out.p;
        VS_TRY(vs_dev_upload(c, w.raw_q.p, queries + (size_t)q0 * dim, (size_t)cq * dim * 4));
        VS_TRY(run_chunk((const float*)w.raw_q.p, slots.data() + q0, cq, out_ids ? (uint32_t*)ob : nullptr,
                         out_tids ? (uint64_t*)(ob + o_tids) : nullptr, out_dist ? (float*)(ob + o_dist) : nullptr, (uint32_t*)(ob + o_rows)));
        if (out_ids) VS_TRY(vs_dev_download(c, out_ids + (size_t)q0 * k, ob, (size_t)cq * k * 4));
        if (out_tids) VS_TRY(vs_dev_download(c, out_tids + (size_t)q0 * k, ob + o_tids, (size_t)cq * k * 8));
        if (out_dist) VS_TRY(vs_dev_download(c, out_dist + (size_t)q0 * k, ob + o_dist, (size_t)cq * k * 4));
        VS_TRY(vs_dev_download(c, out_rows + q0, ob + o_rows, (size_t)cq * 4));
    }
    if (stats) *stats = st;
    return VS_OK;
}

extern "C" int vs_search_batch_qual_exact(vs_index* ix, const float* queries, uint32_t nq, uint32_t k, const uint32_t* qual_slots, uint32_t* out_ids,
                                          uint64_t* out_tids, float* out_dist, uint32_t* out_rows, vs_qual_exact_stats* stats) {
    return vs_guard("vs_search_batch_qual_exact", [&] {
        return search_batch_qual_exact_impl(ix, queries, nq, k, qual_slots, out_ids, out_tids, out_dist, out_rows, stats, false,
                                            "vs_search_batch_qual_exact");
    });
}
extern "C" int vs_search_batch_qual_exact_dev(vs_index* ix, const float* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_qual_slots,
                                              uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, uint32_t* d_out_rows,
                                              vs_qual_exact_stats* stats) {
    return vs_guard("vs_search_batch_qual_exact_dev", [&] {
        return search_batch_qual_exact_impl(ix, d_queries, nq, k, d_qual_slots, d_out_ids, d_out_tids, d_out_dist, d_out_rows, stats, true,
                                            "vs_search_batch_qual_exact_dev");
    });
}
