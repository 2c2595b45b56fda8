// vs_qual_wide.h — the exact and the flat qualified top-k for k up to VS_QUAL_WIDE_MAX_K (a part of vs_batch.hip kept in a file of its
// own, after vs_qual_flat.h): vs_search_batch_qual_exact_wide / _dev, vs_search_batch_qual_flat_wide / _dev.  The contract is the
// header's (include/vsgpu.h, "wide k"); DESIGN.md section 6s.
//
// The narrow calls keep their k rows as one entry per lane of a wave; a list of 4096 entries has no such home, and a shifting
// insertion into it would serialise the row loop.  Here NO list is kept while the rows are read: k_qwide_dist runs k_qual_exact's row
// loop and stores the 32-bit total_cmp key of every (scan, list place), counting it in the scan's histogram by its leading 10 bits;
// k_qwide_pick, one workgroup per scan, finds the key T of the k-th smallest entry by radix selection (10 + 11 + 11 bits: the first
// level from that histogram, two more by re-reading the scan's keys), emits in one ordered pass the places below T and the first
// places at T — the list ascends by node id, so that is the node-id tie rule — and sorts the <= 4096 survivors in LDS.  An emitted
// place's slot is a popcount of the emitted places before it and a histogram count is a sum, so nothing depends on what ran first.
// The flat call keeps k_qflat_ham -> k_qflat_pick -> rerank and ends in k_qflat_final_wide: the same sort over the candidates.
#pragma once
#include "vs_qual_flat.h"

enum {
    QW_BITS1 = 10,                // the leading digit, counted where the key is made
    QW_BITS = 11,                 // the second and the third digit
    QW_BINS1 = 1 << QW_BITS1,
    QW_BINS = 1 << QW_BITS,
    QW_THREADS = 1024,            // k_qwide_pick / k_qflat_final_wide: one workgroup per scan
    QW_WAVES = QW_THREADS / WAVE,
    QW_OUT_BYTES = 256 << 20,     // the [chunk][k] rows of one chunk of scans (host form: their staging)
    QW_WS_MB = 1024               // keys + histograms of one chunk of tiles (VS_QUAL_WIDE_WS_MB)
};

// ---------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------
// k_qual_exact's row loop, unchanged in its arithmetic (rerank_row_dist's order: four accumulators, horizontal add, scalar tail,
// final form; the cosine divisor once per element), over the tiles of the flat call: scans [p0, p0 + cnt) against rows [r0, r1) of a
// list [lbase, lbase + m).  Lane l8 == 0 of each 8-lane group ends with the distance of its row: it stores the key at
// keys[hoff + scan m + place] — the 8 groups of a wave 8 consecutive places, the four waves of a pass 32 (one 128-byte line) — and
// counts its leading digit in the scan's LDS histogram.  No barrier inside the row loop; the histograms go to global memory with one
// atomic per non-zero bin at the end of the slice (a sum, whatever the order).  LDS: [TQ][vec_stride] queries, [TQ][QW_BINS1] counts.
template <int TQ>
__global__ __launch_bounds__(256) void k_qwide_dist(const float* __restrict__ vecs, uint32_t vec_stride, uint32_t dim_full,
                                                    const float* __restrict__ vnorm, uint32_t distance_type, const float* __restrict__ q_full,
                                                    const uint32_t* __restrict__ perm, const uint32_t* __restrict__ list,
                                                    const QfTile* __restrict__ tiles, uint32_t* __restrict__ keys, uint32_t* __restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* qv = reinterpret_cast<float*>(smem);
    uint32_t* lh = reinterpret_cast<uint32_t*>(qv + (size_t)TQ * vec_stride);
    const QfTile t = tiles[blockIdx.x];
    for (int qi = 0; qi < TQ; ++qi) {
        const float* src = q_full + (size_t)((uint32_t)qi < t.cnt ? perm[t.p0 + qi] : 0u) * vec_stride;
        for (uint32_t i = threadIdx.x; i < vec_stride; i += 256) qv[(size_t)qi * vec_stride + i] = (uint32_t)qi < t.cnt ? src[i] : 0.0f;
    }
    for (uint32_t i = threadIdx.x; i < TQ * QW_BINS1; i += 256) lh[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l8 = lane & 7, grp = lane >> 3;
    const uint32_t steps = dim_full / 32;
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
                const uint32_t key = plain_key(res);
                keys[t.hoff + (uint64_t)qi * t.m + (j - t.lbase)] = key;
                atomicAdd(&lh[(uint32_t)qi * QW_BINS1 + (key >> (32 - QW_BITS1))], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < t.cnt * QW_BINS1; i += 256) {  // (the tile's histogram rows are consecutive)
        const uint32_t c = lh[i];
        if (c) atomicAdd(&hist[(size_t)t.h0 * QW_BINS1 + i], c);
    }
}

// One digit level of the selection, by every wave for itself (a wave prefix sum over 64 bins at a time: no barrier): the bin in
// which the running count first reaches `want` (>= 1, at most the sum of h), and the count of the bins before it.
__device__ __forceinline__ void qw_find(const uint32_t* h, uint32_t bins, uint32_t want, int lane, uint32_t& bin, uint32_t& before) {
    bin = bins - 1;
    before = 0;
    for (uint32_t b0 = 0; b0 < bins; b0 += WAVE) {  // (bins is whole 64s)
        const uint32_t c = h[b0 + lane];
        uint32_t inc = c;  // inclusive prefix over the lanes
        for (int d = 1; d < WAVE; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl((int)inc, lane >= d ? lane - d : lane, WAVE);
            if (lane >= d) inc += o;
        }
        const uint64_t reach = __ballot(before + inc >= want);
        if (reach) {
            const int src = __builtin_ctzll(reach);
            bin = b0 + (uint32_t)src;
            before += (uint32_t)__builtin_amdgcn_readlane((int)(inc - c), src);
            return;
        }
        before += (uint32_t)__builtin_amdgcn_readlane((int)inc, WAVE - 1);
    }
}

// The n <= 4096 entries (key << 32 | node id) in surv become ascending — a bitonic sort in LDS, padded with ~0 to a power of two (no
// entry equals ~0: no node has the id VS_INVALID_NODE) — and the first min(n, k) of them the rows of scan q of the batch; entries past
// them: VS_INVALID_NODE / 0 / NaN.  Called by every thread of the workgroup; surv needs no barrier before the call.
__device__ __forceinline__ void qw_sort_write(uint64_t* surv, uint32_t n, uint32_t k, uint32_t q, const uint64_t* __restrict__ tids,
                                              uint32_t* __restrict__ out_ids, uint64_t* __restrict__ out_tids, float* __restrict__ out_dist,
                                              uint32_t* __restrict__ out_rows) {
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    uint32_t P = WAVE;
    while (P < n) P <<= 1;
    for (uint32_t i = n + tid; i < P; i += nt) surv[i] = ~0ull;
    __syncthreads();
    for (uint32_t size = 2; size <= P; size <<= 1) {
        for (uint32_t stride = size >> 1; stride; stride >>= 1) {
            for (uint32_t t = tid; t < P / 2; t += nt) {
                const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const uint64_t a = surv[lo], b = surv[hi];
                if ((a > b) == ((lo & size) == 0)) {
                    surv[lo] = b;
                    surv[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    const uint32_t rows = min(n, k);
    for (uint32_t i = tid; i < k; i += nt) {
        const bool have = i < rows;
        const uint64_t e = have ? surv[i] : 0ull;
        const uint32_t id = have ? (uint32_t)e : VS_INVALID_NODE;
        const size_t o = (size_t)q * k + i;
        if (out_ids) out_ids[o] = id;
        if (out_tids) out_tids[o] = have && tids ? tids[id] : 0ull;
        if (out_dist) out_dist[o] = have ? plain_unkey((uint32_t)(e >> 32)) : __uint_as_float(0x7FC00000u);
    }
    if (tid == 0) out_rows[q] = rows;
}

// One workgroup per scan of a chunk (block b: scan perm[b] of the batch, histogram row b, keys[hoff .. hoff + m) over the list rows
// [lbase, lbase + m)).  m <= k: every place is emitted.  Otherwise T, the key of the k-th smallest entry, digit by digit: level 1 from
// the histogram k_qwide_dist left, levels 2 and 3 by counting in LDS the next digit of the keys that match the prefix so far; `below`
// ends as the number of keys < T.  Then k_qflat_pick's ordered emission: the list is cut into one run of consecutive places per wave,
// a count pass gives each wave the keys below and at T before its run, a place pass the slot of every emitted place.  The survivors
// go to LDS and through qw_sort_write.  Bound by the four reads of the scan's keys for long lists, by the sort's barriers for short ones.
__global__ __launch_bounds__(QW_THREADS) void k_qwide_pick(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ hist,
                                                           const QfScan* __restrict__ scans, const uint32_t* __restrict__ perm,
                                                           const uint32_t* __restrict__ list, uint32_t k, const uint64_t* __restrict__ tids,
                                                           uint32_t* __restrict__ out_ids, uint64_t* __restrict__ out_tids,
                                                           float* __restrict__ out_dist, uint32_t* __restrict__ out_rows) {
    __shared__ uint64_t surv[VS_QUAL_WIDE_MAX_K];
    __shared__ uint32_t lh[QW_BINS];
    __shared__ uint32_t seg[QW_WAVES][2];
    const QfScan s = scans[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t want = min(k, s.m);
    const uint32_t* kr = keys + s.hoff;
    uint32_t T = 0xFFFFFFFFu, quota = 0xFFFFFFFFu;  // (m <= k: every key is below T or at it, within the quota)
    if (s.m > k) {                                   // (the whole workgroup)
        uint32_t bin, before, below;
        qw_find(hist + (size_t)blockIdx.x * QW_BINS1, QW_BINS1, want, lane, bin, below);
        uint32_t prefix = bin;
        for (int level = 0; level < 2; ++level) {
            const uint32_t shift = level ? 0u : (uint32_t)QW_BITS;  // the digit counted; the bits above it are the prefix
            for (uint32_t i = tid; i < QW_BINS; i += QW_THREADS) lh[i] = 0u;
            __syncthreads();
            for (uint32_t i = tid; i < s.m; i += QW_THREADS) {
                const uint32_t key = kr[i];
                if ((key >> (shift + QW_BITS)) == prefix) atomicAdd(&lh[(key >> shift) & (QW_BINS - 1)], 1u);
            }
            __syncthreads();
            qw_find(lh, QW_BINS, want - below, lane, bin, before);
            below += before;
            prefix = (prefix << QW_BITS) | bin;
            __syncthreads();  // (every wave has read the counts before they are cleared)
        }
        T = prefix;
        quota = want - below;  // keys AT T that are taken, in list order
    }
    const uint64_t per = ((uint64_t)s.m + QW_THREADS - 1) / QW_THREADS * WAVE;  // places per wave, whole 64s
    const uint32_t a = (uint64_t)wave * per < s.m ? (uint32_t)(wave * per) : s.m, e = a + per < s.m ? (uint32_t)(a + per) : s.m;
    uint32_t n_lt = 0, n_eq = 0;
    for (uint32_t i = a; i < e; i += WAVE) {  // (wave-uniform trip count: the ballots see every lane)
        const bool in = i + (uint32_t)lane < e;
        const uint32_t v = in ? kr[i + lane] : 0u;
        n_lt += (uint32_t)__popcll(__ballot(in && v < T));
        n_eq += (uint32_t)__popcll(__ballot(in && v == T));
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
        const bool in = i + (uint32_t)lane < e;
        const uint32_t v = in ? kr[i + lane] : 0u;
        const bool lt = in && v < T, eq = in && v == T;
        const uint64_t m_lt = __ballot(lt), m_eq = __ballot(eq);
        const uint32_t eq_before = eq_run + (uint32_t)__popcll(m_eq & lower);
        const uint32_t place = lt_run + (uint32_t)__popcll(m_lt & lower) + min(eq_before, quota);
        if ((lt || (eq && eq_before < quota)) && place < want) surv[place] = ((uint64_t)v << 32) | list[s.lbase + i + lane];
        lt_run += (uint32_t)__popcll(m_lt);
        eq_run += (uint32_t)__popcll(m_eq);
    }
    qw_sort_write(surv, want, k, perm[blockIdx.x], tids, out_ids, out_tids, out_dist, out_rows);
}

// One workgroup per scan q of the chunk: its cand_n[q] <= rescore candidates with k_rerank's distances become (key << 32 | node id)
// in LDS; qw_sort_write keeps the first k.  Bound by the sort's barriers.
__global__ __launch_bounds__(QW_THREADS) void k_qflat_final_wide(const uint32_t* __restrict__ cand, const uint32_t* __restrict__ cand_n,
                                                                 const float* __restrict__ dist, uint32_t rescore, uint32_t k,
                                                                 const uint64_t* __restrict__ tids, uint32_t* __restrict__ out_ids,
                                                                 uint64_t* __restrict__ out_tids, float* __restrict__ out_dist,
                                                                 uint32_t* __restrict__ out_rows) {
    __shared__ uint64_t surv[VS_QUAL_FLAT_MAX_RESCORE];
    const uint32_t q = blockIdx.x, n = min(cand_n[q], rescore);
    const uint32_t* ids = cand + (size_t)q * rescore;
    const float* d = dist + (size_t)q * rescore;
    for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) surv[j] = ((uint64_t)plain_key(d[j]) << 32) | ids[j];
    qw_sort_write(surv, n, k, q, tids, out_ids, out_tids, out_dist, out_rows);
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
// the largest instantiated tile (8, 4, 2, 1) not above `want` whose queries and histograms fit the LDS budget (16 histograms alone
// fill it); the floor is one
static uint32_t qw_tile_queries(const vs_index* ix, uint32_t want) {
    const size_t per = (size_t)ix->vec_stride * 4 + (size_t)QW_BINS1 * 4;
    uint32_t tq = 8;
    while (tq > 1 && (tq > want || (size_t)tq * per > QX_LDS_BUDGET)) tq >>= 1;
    return tq;
}

// the scans of one launch of the host or device form: as many as the exact call takes, and no more than QW_OUT_BYTES of [scan][k] rows
static uint32_t qw_chunk_scans(uint32_t nq, uint32_t k) {
    return std::min<uint32_t>(std::min<uint32_t>(nq, QX_CHUNK_SCANS), std::max<uint32_t>((uint32_t)QW_OUT_BYTES / (16u * k), 1));
}

template <int TQ>
static void qw_launch_dist(const vs_index* ix, uint32_t blocks, size_t lds, const uint32_t* d_perm, const QfTile* d_tiles) {
    hipLaunchKernelGGL(k_qwide_dist<TQ>, dim3(blocks), dim3(256), lds, ix->ctx->stream, (const float*)ix->vecs, ix->vec_stride, ix->d.dim_full,
                       (const float*)ix->vnorm, ix->d.distance_type, (const float*)ix->ws.q_full.p, d_perm, (const uint32_t*)ix->ws.qx_list.p, d_tiles,
                       (uint32_t*)ix->ws.qw_keys.p, (uint32_t*)ix->ws.qw_hist.p);
}

// qx_run_chunk for k up to VS_QUAL_WIDE_MAX_K: the slot order, the tiles and the slices of the exact call, the chunks of TILES of the
// flat call (the keys of a chunk under VS_QUAL_WIDE_WS_MB; a chunk holds at least one tile).  Leaves its launches on the stream.
static int qw_run_chunk(vs_index* ix, const QxLists& ls, const float* d_queries, const uint32_t* slots, uint32_t cq, uint32_t k, uint32_t tq,
                        uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, uint32_t* d_out_rows, vs_qual_exact_stats* st) {
    vs_ctx* c = ix->ctx;
    SearchWorkspace& w = ix->ws;
    VS_TRY(devbuf_reserve(c, w.q_full, (size_t)cq * ix->vec_stride * 4));
    VS_TRY(devbuf_reserve(c, w.qcodes, (size_t)cq * ix->code_stride * 8));
    VS_TRY(launch_prepare_queries(ix, d_queries, cq, (float*)w.q_full.p, (uint64_t*)w.qcodes.p));
    std::vector<uint32_t> perm(cq), first;
    qx_slot_order(ls, slots, cq, perm.data(), &first);
    uint32_t n_tiles = 0;
    for (size_t i = 0; i < ls.slot.size(); ++i) n_tiles += (first[i + 1] - first[i] + tq - 1) / tq;
    const uint32_t forced = env_u32("VS_QUAL_EXACT_SLICES", 0);
    const uint32_t fill = (uint32_t)std::max(c->prop.multiProcessorCount, 1) * 4;
    const uint32_t want = forced ? forced : std::max<uint32_t>((fill + n_tiles - 1) / std::max<uint32_t>(n_tiles, 1), 1);
    const uint64_t budget = (uint64_t)env_u32("VS_QUAL_WIDE_WS_MB", QW_WS_MB) << 20;  // (0: every tile a chunk of its own)
    std::vector<QfTile> tiles;
    std::vector<QfScan> scans(cq);
    std::vector<QfChunk> chunks(1);
    uint64_t cost = 0, max_keys = 1;
    uint32_t max_scans = 1;
    for (size_t i = 0; i < ls.slot.size(); ++i) {
        const uint32_t m = ls.m[i], passes = (m + QX_PASS - 1) / QX_PASS;
        const uint32_t per = std::max<uint32_t>((passes + want - 1) / want, 1) * QX_PASS;  // rows per slice
        const uint32_t S = std::max<uint32_t>((m + per - 1) / per, 1);
        st->slices = std::max<uint64_t>(st->slices, S);
        for (uint32_t p0 = first[i]; p0 < first[i + 1]; p0 += tq) {
            const uint32_t cnt = std::min(tq, first[i + 1] - p0);
            const uint64_t mine = (uint64_t)cnt * m * 4 + (uint64_t)cnt * QW_BINS1 * 4;
            if (chunks.back().scans && cost + mine > budget) {
                chunks.push_back(QfChunk{(uint32_t)tiles.size(), 0, p0, 0, 0});
                cost = 0;
            }
            QfChunk& ch = chunks.back();
            for (uint32_t j = 0; j < cnt; ++j) scans[p0 + j] = QfScan{ch.ham + (uint64_t)j * m, ls.off[i], m};
            for (uint32_t sl = 0; sl < S && m; ++sl) {
                tiles.push_back(QfTile{ch.ham, p0, cnt, ls.off[i] + (uint32_t)std::min<uint64_t>((uint64_t)sl * per, m),
                                       ls.off[i] + (uint32_t)std::min<uint64_t>(((uint64_t)sl + 1) * per, m), ls.off[i], m, p0 - ch.p0, 0});
                ch.tiles++;
            }
            ch.ham += (uint64_t)cnt * m;
            ch.scans += cnt;
            cost += mine;
            max_keys = std::max(max_keys, ch.ham);
            max_scans = std::max(max_scans, ch.scans);
            st->tiles++;
            st->row_reads += m;
        }
    }
    // [scans | tiles | perm] in one upload
    const size_t scans_bytes = scans.size() * sizeof(QfScan), tiles_bytes = tiles.size() * sizeof(QfTile), perm_bytes = (size_t)cq * 4;
    std::vector<unsigned char> tab(scans_bytes + tiles_bytes + perm_bytes);
    memcpy(tab.data(), scans.data(), scans_bytes);
    if (tiles_bytes) memcpy(tab.data() + scans_bytes, tiles.data(), tiles_bytes);
    memcpy(tab.data() + scans_bytes + tiles_bytes, perm.data(), perm_bytes);
    VS_TRY(devbuf_reserve(c, w.qw_tab, tab.size()));
    VS_TRY(devbuf_reserve(c, w.qw_keys, max_keys * 4));
    VS_TRY(devbuf_reserve(c, w.qw_hist, (size_t)max_scans * QW_BINS1 * 4));
    VS_TRY(vs_dev_upload(c, w.qw_tab.p, tab.data(), tab.size()));
    const QfScan* d_scans = (const QfScan*)w.qw_tab.p;
    const QfTile* d_tiles = (const QfTile*)((const char*)w.qw_tab.p + scans_bytes);
    const uint32_t* d_perm = (const uint32_t*)((const char*)w.qw_tab.p + scans_bytes + tiles_bytes);
    const size_t lds = (size_t)tq * ((size_t)ix->vec_stride * 4 + (size_t)QW_BINS1 * 4);
    for (const QfChunk& ch : chunks) {
        if (!ch.scans) continue;
        hipEvent_t ev = prof_begin(c);
        VS_HIP(hipMemsetAsync(w.qw_hist.p, 0, (size_t)ch.scans * QW_BINS1 * 4, c->stream));
        if (ch.tiles) {
            switch (tq) {
                case 8: qw_launch_dist<8>(ix, ch.tiles, lds, d_perm, d_tiles + ch.tile0); break;
                case 4: qw_launch_dist<4>(ix, ch.tiles, lds, d_perm, d_tiles + ch.tile0); break;
                case 2: qw_launch_dist<2>(ix, ch.tiles, lds, d_perm, d_tiles + ch.tile0); break;
                default: qw_launch_dist<1>(ix, ch.tiles, lds, d_perm, d_tiles + ch.tile0); break;
            }
        }
        prof_end(c, PK_RERANK, ev);
        VS_HIP(hipGetLastError());
        ev = prof_begin(c);
        hipLaunchKernelGGL(k_qwide_pick, dim3(ch.scans), dim3(QW_THREADS), 0, c->stream, (const uint32_t*)w.qw_keys.p, (const uint32_t*)w.qw_hist.p,
                           d_scans + ch.p0, d_perm + ch.p0, (const uint32_t*)w.qx_list.p, k, (const uint64_t*)ix->tids, d_out_ids, d_out_tids, d_out_dist,
                           d_out_rows);
        prof_end(c, PK_RESORT, ev);
        VS_HIP(hipGetLastError());
    }
    return VS_OK;
}

static void qw_launch_final(const vs_index* ix, uint32_t cq, const uint32_t* d_cand, const uint32_t* d_cand_n, const float* d_dist, uint32_t rescore,
                            uint32_t k, uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, uint32_t* d_out_rows) {
    uint32_t threads = WAVE;  // a thread per compare-exchange of a sort stage, within [one wave, QW_THREADS]
    while (threads < QW_THREADS && 2 * threads < rescore) threads <<= 1;
    hipLaunchKernelGGL(k_qflat_final_wide, dim3(cq), dim3(threads), 0, ix->ctx->stream, d_cand, d_cand_n, d_dist, rescore, k, (const uint64_t*)ix->tids,
                       d_out_ids, d_out_tids, d_out_dist, d_out_rows);
}

extern "C" int vs_search_batch_qual_exact_wide(vs_index* ix, const float* queries, uint32_t nq, uint32_t k, const uint32_t* qual_slots, uint32_t* out_ids,
                                               uint64_t* out_tids, float* out_dist, uint32_t* out_rows, vs_qual_exact_stats* stats) {
    return vs_guard("vs_search_batch_qual_exact_wide", [&] {
        return search_batch_qual_exact_impl(ix, queries, nq, k, qual_slots, out_ids, out_tids, out_dist, out_rows, stats, false,
                                            "vs_search_batch_qual_exact_wide", GroupRule{}, true);
    });
}
extern "C" int vs_search_batch_qual_exact_wide_dev(vs_index* ix, const float* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_qual_slots,
                                                   uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, uint32_t* d_out_rows,
                                                   vs_qual_exact_stats* stats) {
    return vs_guard("vs_search_batch_qual_exact_wide_dev", [&] {
        return search_batch_qual_exact_impl(ix, d_queries, nq, k, d_qual_slots, d_out_ids, d_out_tids, d_out_dist, d_out_rows, stats, true,
                                            "vs_search_batch_qual_exact_wide_dev", GroupRule{}, true);
    });
}
extern "C" int vs_search_batch_qual_flat_wide(vs_index* ix, const float* queries, uint32_t nq, uint32_t k, uint32_t rescore, const uint32_t* qual_slots,
                                              uint32_t* out_ids, uint64_t* out_tids, float* out_dist, uint32_t* out_rows, vs_qual_flat_stats* stats) {
    return vs_guard("vs_search_batch_qual_flat_wide", [&] {
        return search_batch_qual_flat_impl(ix, queries, nq, k, rescore, qual_slots, out_ids, out_tids, out_dist, out_rows, stats, false,
                                           "vs_search_batch_qual_flat_wide", GroupRule{}, true);
    });
}
extern "C" int vs_search_batch_qual_flat_wide_dev(vs_index* ix, const float* d_queries, uint32_t nq, uint32_t k, uint32_t rescore,
                                                  const uint32_t* d_qual_slots, uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist,
                                                  uint32_t* d_out_rows, vs_qual_flat_stats* stats) {
    return vs_guard("vs_search_batch_qual_flat_wide_dev", [&] {
        return search_batch_qual_flat_impl(ix, d_queries, nq, k, rescore, d_qual_slots, d_out_ids, d_out_tids, d_out_dist, d_out_rows, stats, true,
                                           "vs_search_batch_qual_flat_wide_dev", GroupRule{}, true);
    });
}
