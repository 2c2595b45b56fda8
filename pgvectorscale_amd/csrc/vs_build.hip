// vs_build.hip — batched Vamana construction over SBQ codes on the GPU (a "next" row: index build is
// NOT the reference's search path, but a device-resident index of 1M..50M nodes cannot be manufactured any other way
// inside a benchmark run).  It is the batch-parallel counterpart of
//   Graph::insert / insert_internal        AM/graph/mod.rs:637-717
//   greedy_search_for_build                AM/graph/mod.rs:285-327   (k_search<BUILD=true>)
//   add_neighbors + prune_neighbors        AM/graph/mod.rs:212-266,392-488 (alpha ladder 1.0, 1.2 .. max_alpha)
//   update_back_pointer                    AM/graph/mod.rs:719-735
// with SBQ Hamming distances between nodes exactly like SbqNodeDistanceMeasure (AM/sbq/mod.rs:161-190).
// Nodes are inserted in heap order; node 0 is the default start node (first inserted node, as in the reference).
// Batches: sizes double until `batch_max`; every node of a batch searches the graph of all previous batches, its
// out-edges are pruned, then back-edges are grouped per target (radix sort) and each target's list is re-pruned once.
// The result is deterministic for a given (codes, parameters); it is not claimed to be edge-identical to the
// reference's sequential build (which is itself HashSet-order dependent, AM/graph/mod.rs:317-326).
// Labeled vector sets (vs_index_set_labels before the build): as in Graph::insert (AM/graph/mod.rs:637-662) every node is
// inserted twice — from the start nodes of its labels with the label filter on, then from the default start node without
// it, the second pass merging into the list the first one left — a node is the start node of every label it is the first
// to carry (update_start_nodes, AM/graph/mod.rs:490-531), and prune_neighbors only lets an existing neighbor occlude a
// candidate when it carries every label the candidate shares with the point (contains_intersection,
// AM/labels/mod.rs:85-111, used at AM/graph/mod.rs:442-456).
// `plain` storage (no codes): the same batches, pruning and back-edges score with the full-precision pair distance of
// IndexFullDistanceMeasure instead (PlainPair below; DESIGN.md section 6g has the rule).
#include <algorithm>
#include <cstdlib>
#include <map>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "vs_device.h"

__device__ __forceinline__ uint32_t ham_words(const uint64_t* a, const uint64_t* b, uint32_t stride) {
    uint32_t acc = 0;
    if (stride == 24) {  // 768 x 2 bit / 1536 x 1 bit: fully unrolled so the 24 loads are in flight together
        ulonglong2 x[12], y[12];
#pragma unroll
        for (int t = 0; t < 12; ++t) {
            x[t] = *reinterpret_cast<const ulonglong2*>(a + 2 * t);
            y[t] = *reinterpret_cast<const ulonglong2*>(b + 2 * t);
        }
#pragma unroll
        for (int t = 0; t < 12; ++t) acc += (uint32_t)__popcll(x[t].x ^ y[t].x) + (uint32_t)__popcll(x[t].y ^ y[t].y);
        return acc;
    }
    for (uint32_t w = 0; w < stride; w += 2) {
        const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(a + w);
        const ulonglong2 y = *reinterpret_cast<const ulonglong2*>(b + w);
        acc += (uint32_t)__popcll(x.x ^ y.x) + (uint32_t)__popcll(x.y ^ y.y);
    }
    return acc;
}

// copy the codes of C candidates into LDS: all 16-byte chunks of all rows are spread over the wave, 4 loads in flight per
// lane (a row-at-a-time loop pays one HBM latency per candidate, which dominated the build)
__device__ __forceinline__ void stage_codes(uint64_t* ccode, const uint64_t* __restrict__ codes, const uint32_t* cid,
                                            uint32_t C, uint32_t stride, int lane) {
    const uint32_t cpr = stride >> 1;  // 16-byte chunks per row (stride is even)
    const uint32_t total = C * cpr;
    for (uint32_t base = 0; base < total; base += 4 * WAVE) {
        ulonglong2 v[4];
        uint32_t dst[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t idx = base + (uint32_t)u * WAVE + (uint32_t)lane;
            dst[u] = 0xFFFFFFFFu;
            if (idx < total) {
                const uint32_t j = idx / cpr, w = 2u * (idx - j * cpr);
                v[u] = *reinterpret_cast<const ulonglong2*>(codes + (size_t)cid[j] * stride + w);
                dst[u] = j * stride + w;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (dst[u] != 0xFFFFFFFFu) *reinterpret_cast<ulonglong2*>(ccode + dst[u]) = v[u];
    }
}

// contains_intersection(existing, candidate, point) for label sets relative to ONE point: bit t of a node's mask says that
// the point's t-th label is in the node's set, so  (candidate ∩ point) ⊆ existing  <=>  (mask[candidate] & ~mask[existing]) == 0.
// (a point carries at most 64 labels: vs_build_graph checks)
__device__ __forceinline__ uint64_t label_pmask(const uint32_t* __restrict__ label_off, const int16_t* __restrict__ label_val,
                                                uint32_t of, uint32_t node) {
    const uint32_t ob = label_off[of], oe = label_off[of + 1];
    uint32_t j = label_off[node];
    const uint32_t je = label_off[node + 1];
    uint64_t m = 0;
    for (uint32_t t = ob; t < oe && j < je;) {
        const int16_t x = label_val[t], y = label_val[j];
        if (x == y) {
            m |= 1ull << (t - ob);
            ++t;
            ++j;
        } else if (x < y) {
            ++t;
        } else {
            ++j;
        }
    }
    return m;
}

// ---- the pair distance of the build: what wave_prune, the back-edge kernel and the candidate keys score with ----------------
// A policy names G, the lanes that score one candidate together (the tail of a selected candidate is walked 64 / G candidates per
// pass), select(i) — candidate i was taken: its side of the pairs that follow — and factor(j, key of d(point -> j), act):
// get_factor (AM/graph/neighbor_with_distance.rs:55-65) of candidate j against the selected one, a call every lane makes and
// whose value counts on the first lane of j's group.
// HamPair: SbqNodeDistanceMeasure (AM/sbq/mod.rs:161-190), xor + popcount of two code rows, one lane per candidate.
struct PlainVecs {  // what a kernel needs of a plain index to score pairs (all zero for the SBQ forms)
    const float* vecs;
    const float* vdiv;  // cosine: the divisors of the index slices (vnorm, or vnorm_idx when dim_index < dim_full); else nullptr
    uint32_t vec_stride, dim, distance_type;
};
struct HamPair {
    static constexpr uint32_t G = 1;
    const uint64_t* ccode;  // LDS copy of the candidate codes [C][stride], or nullptr: rows are read from global memory
    const uint64_t* __restrict__ codes;
    const uint32_t* cand_id;
    uint32_t stride;
    const uint64_t* ci;
    __device__ __forceinline__ void select(uint32_t i, int) { ci = ccode ? ccode + (size_t)i * stride : codes + (size_t)cand_id[i] * stride; }
    __device__ __forceinline__ float factor(uint32_t j, uint32_t dpc, bool act, int) const {
        if (!act) return 0.0f;
        const uint64_t* cj = ccode ? ccode + (size_t)j * stride : codes + (size_t)cand_id[j] * stride;
        const uint32_t dij = ham_words(cj, ci, stride);
        if (dij == 0) return dpc == 0 ? 1.0f : 3.0e38f;
        return (float)dpc / (float)dij;
    }
};
// PlainPair: IndexFullDistanceMeasure of `plain` storage.  d(a -> b) is what a plain scan whose query is
// node a's raw row gives row b: the query side is a's index slice prepared as k_prepare_index_slice prepares a query (for cosine
// divided by the divisor preprocess_cosine derives — the one k_row_norms cached for the row, same sum in the same order), held in
// LDS as the qv of plain_dist8; the row side is b's raw row and its cached divisor.  Eight lanes score one candidate, so a pass
// covers eight rows, each read from global memory in 16-byte pieces.  Keys are plain_key(d), distances come back with plain_unkey.
struct PlainPair {
    static constexpr uint32_t G = 8;
    const float* __restrict__ vecs;
    const float* __restrict__ vdiv;  // per-row cosine divisor of the index slice; nullptr for the other distance types
    const uint32_t* cand_id;
    float* qv;  // LDS [round_up(dim, 4)]
    uint32_t vec_stride, dim, distance_type;
    // node's prepared index slice becomes the query side (barriers on both ends: qv may still be read, and is read next)
    __device__ __forceinline__ void stage(uint32_t node, int lane) const {
        __syncthreads();
        const float* row = vecs + (size_t)node * vec_stride;
        const float s = vdiv ? vdiv[node] : 0.0f;
        for (uint32_t i = 4u * (uint32_t)lane; i < dim; i += 4u * WAVE) {  // (rows are 16-byte aligned and padded to four floats)
            float4 x = *reinterpret_cast<const float4*>(row + i);
            if (s != 0.0f) {
                x.x = x.x / s;
                x.y = x.y / s;
                x.z = x.z / s;
                x.w = x.w / s;
            }
            *reinterpret_cast<float4*>(qv + i) = x;
        }
        __syncthreads();
    }
    // d(staged node -> node), valid on the first lane of each 8-lane group
    __device__ __forceinline__ float dist(uint32_t node, bool act, int lane) const {
        const float sdiv = (act && vdiv) ? vdiv[node] : 0.0f;
        return plain_dist8(vecs + (size_t)(act ? node : 0u) * vec_stride, sdiv, qv, dim, distance_type, lane, act);
    }
    __device__ __forceinline__ void select(uint32_t i, int lane) const { stage(cand_id[i], lane); }
    __device__ __forceinline__ float factor(uint32_t j, uint32_t dpc_key, bool act, int lane) const {
        const float d_ec = dist(act ? cand_id[j] : 0u, act, lane);  // the existing neighbour is the query (AM/graph/mod.rs:434-465)
        const float d_pc = plain_unkey(dpc_key);
        const float eps = 1.1920929e-07f;  // f32::EPSILON
        if (d_ec < eps) return d_pc < eps ? 1.0f : 3.0e38f;
        return d_pc / d_ec;
    }
};

// prune_neighbors for one node by one wave.  cand_id/cand_d: C candidates sorted ascending by distance (LDS) — candidates.sort() of
// prune_neighbors is stable on the distance alone, the order among equal distances is the caller's: (distance, id) everywhere but
// in k_build_prune_new, which takes the visited list as the search left it; pd: the pair distance (above).  Writes up to R selected candidate *positions* into sel[] (LDS) and returns their number.
template <class P>
__device__ uint32_t wave_prune(P& pd, const uint32_t* cand_d, uint32_t C, uint32_t R, float max_alpha, float* maxf /*LDS [C]*/,
                               uint32_t* sel /*LDS [R]*/, int lane,
                               const uint64_t* pm = nullptr /*LDS [C] label masks (label_pmask) or nullptr*/) {
    const float FMAX = 3.0e38f;
    for (uint32_t j = lane; j < C; j += WAVE) maxf[j] = 0.0f;
    __syncthreads();
    uint32_t nres = 0;
    float alpha = 1.0f;
    while (alpha <= max_alpha && nres < R) {
        for (uint32_t i = 0; i < C && nres < R; ++i) {
            float mf = maxf[i];
            if (mf > alpha) continue;
            __syncthreads();
            if (lane == 0) {
                maxf[i] = FMAX;
                sel[nres] = i;
            }
            nres++;
            pd.select(i, lane);
            for (uint32_t j0 = i + 1; j0 < C; j0 += WAVE / P::G) {  // (uniform trip count: factor() is a call of the whole wave)
                const uint32_t j = j0 + (uint32_t)lane / P::G;
                bool act = j < C;
                float mj = 0.0f;
                if (act) {
                    mj = maxf[j];
                    act = !(mj > max_alpha);
                    if (act && pm && (pm[j] & ~pm[i]) != 0) act = false;  // "Does it contain essential labels?" (AM/graph/mod.rs:442-456)
                }
                const float factor = pd.factor(j, act ? cand_d[j] : 0u, act, lane);
                if (act && ((uint32_t)lane & (P::G - 1)) == 0) maxf[j] = fmaxf(mj, factor);
            }
            __syncthreads();
        }
        alpha *= 1.2f;
    }
    __syncthreads();
    return nres;
}

// the SBQ form: the register loop for 24-word codes, else wave_prune<HamPair>.  ccode: optional LDS copy of the candidate codes
// [C][stride] (nullptr => read codes from global).
__device__ uint32_t wave_prune_ham(const uint32_t* cand_id, const uint32_t* cand_d, uint32_t C, const uint64_t* ccode,
                                   const uint64_t* __restrict__ codes, uint32_t stride, uint32_t R, float max_alpha,
                                   float* maxf /*LDS [C]*/, uint32_t* sel /*LDS [R]*/, int lane,
                                   const uint64_t* pm = nullptr /*LDS [C] label masks (label_pmask) or nullptr*/) {
    const float FMAX = 3.0e38f;
    if (ccode && stride == 24 && C <= WAVE) {
        // register form of the same loop (768 x 2 bit / 1536 x 1 bit codes, at most one candidate per lane): lane j keeps
        // candidate j's code, distance and max-factor in registers; only the selected candidate's code is read from LDS
        // (a broadcast read).  Same arithmetic in the same order as the general loop below.
        const bool mine_ok = (uint32_t)lane < C;
        ulonglong2 mine[12];
#pragma unroll
        for (int t = 0; t < 12; ++t)
            mine[t] = mine_ok ? *reinterpret_cast<const ulonglong2*>(ccode + (size_t)lane * 24 + 2 * t) : make_ulonglong2(0, 0);
        const uint32_t myd = mine_ok ? cand_d[lane] : 0u;
        const uint64_t mypm = (pm && mine_ok) ? pm[lane] : 0ull;
        float mymax = 0.0f;
        uint32_t nres = 0;
        float alpha = 1.0f;
        while (alpha <= max_alpha && nres < R) {
            for (uint32_t i = 0; i < C && nres < R; ++i) {
                const float mf = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mymax), (int)i));
                if (mf > alpha) continue;
                if ((uint32_t)lane == i) mymax = FMAX;
                if (lane == 0) sel[nres] = i;
                nres++;
                // "Does it contain essential labels?" (AM/graph/mod.rs:442-456)
                const bool essential = pm ? (mypm & ~pm[i]) != 0 : false;
                if ((uint32_t)lane > i && mine_ok && !(mymax > max_alpha) && !essential) {
                    const uint64_t* ci = ccode + (size_t)i * 24;
                    uint32_t dij = 0;
#pragma unroll
                    for (int t = 0; t < 12; ++t) {
                        const ulonglong2 c = *reinterpret_cast<const ulonglong2*>(ci + 2 * t);
                        dij += (uint32_t)__popcll(mine[t].x ^ c.x) + (uint32_t)__popcll(mine[t].y ^ c.y);
                    }
                    float factor;
                    if (dij == 0) factor = myd == 0 ? 1.0f : FMAX;
                    else factor = (float)myd / (float)dij;
                    mymax = fmaxf(mymax, factor);
                }
            }
            alpha *= 1.2f;
        }
        __syncthreads();
        return nres;
    }
    HamPair pd{ccode, codes, cand_id, stride, nullptr};
    return wave_prune(pd, cand_d, C, R, max_alpha, maxf, sel, lane, pm);
}

// ---- out-edges of the new nodes of one batch ------------------------------------------------------------------
// one wave per new node p = b0 + blockIdx.x.  Input: its visited list from the build-mode search (either kernel), in the order of
// ListSearchResult's visited vector — ascending distance, of equal distances the node visited later first
// (visited.insert(partition_point(|x| x < head), head), AM/graph/mod.rs:167-168) — with the mates of an insert merged in; it is pruned in
// that order.
// PLAIN: the candidates' keys are plain_key(d(p -> candidate)) and pruning scores with PlainPair; the area behind sel[] holds the
// selected candidate's prepared vector instead of code rows.
template <bool PLAIN>
__global__ __launch_bounds__(WAVE) void k_build_prune_new(const uint64_t* __restrict__ codes, uint32_t stride,
                                                          uint32_t* __restrict__ nbrs, uint32_t nbr_stride, uint32_t R,
                                                          float max_alpha, uint32_t b0, uint32_t bn,
                                                          const uint32_t* __restrict__ vis_ids,
                                                          const uint32_t* __restrict__ vis_d,
                                                          const uint32_t* __restrict__ vis_cnt, uint32_t vmax,
                                                          uint32_t use_lds_codes, uint64_t* __restrict__ edge_q,
                                                          uint64_t* __restrict__ edge_pd, PlainVecs pv) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    if (b >= bn) return;
    const uint32_t p = b0 + b;
    uint32_t C = min(vis_cnt[b], vmax);
    uint32_t* cid = reinterpret_cast<uint32_t*>(smem);
    uint32_t* cd = cid + vmax;
    float* maxf = reinterpret_cast<float*>(cd + vmax);
    uint32_t* sel = reinterpret_cast<uint32_t*>(maxf + vmax);
    uint64_t* ccode = reinterpret_cast<uint64_t*>(sel + round_up_u32(R, 4));
    for (uint32_t j = lane; j < C; j += WAVE) {
        cid[j] = vis_ids[(size_t)b * vmax + j];
        cd[j] = vis_d[(size_t)b * vmax + j];
    }
    __syncthreads();
    if (!PLAIN && use_lds_codes) {
        stage_codes(ccode, codes, cid, C, stride, lane);
        __syncthreads();
    }
    uint32_t nres;
    if (C <= R) {  // Graph::add_neighbors prunes only a candidate list longer than num_neighbors (AM/graph/mod.rs:243-256)
        for (uint32_t t = lane; t < C; t += WAVE) sel[t] = t;
        nres = C;
        __syncthreads();
    } else if constexpr (PLAIN) {
        PlainPair pd{pv.vecs, pv.vdiv, cid, reinterpret_cast<float*>(ccode), pv.vec_stride, pv.dim, pv.distance_type};
        nres = wave_prune(pd, cd, C, R, max_alpha, maxf, sel, lane);
    } else {
        nres = wave_prune_ham(cid, cd, C, use_lds_codes ? ccode : nullptr, codes, stride, R, max_alpha, maxf, sel, lane);
    }
    uint32_t* row = nbrs + (size_t)p * nbr_stride;
    for (uint32_t t = lane; t < nbr_stride; t += WAVE) row[t] = t < nres ? cid[sel[t]] : VS_INVALID_NODE;
    // back-edge requests (q <- p, d)
    for (uint32_t t = lane; t < R; t += WAVE) {
        size_t e = (size_t)b * R + t;
        if (t < nres) {
            edge_q[e] = ((uint64_t)cid[sel[t]] << 32) | cd[sel[t]];  // sort key: target, then distance (closest requests first)
            edge_pd[e] = ((uint64_t)cd[sel[t]] << 32) | p;
        } else {
            edge_q[e] = ~0ull;
            edge_pd[e] = 0;
        }
    }
}

// segment heads of the sorted back-edge list
__global__ void k_seg_heads(const uint64_t* __restrict__ q_sorted, uint32_t ne, uint32_t* __restrict__ seg_start,
                            uint32_t* __restrict__ nseg) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ne) return;
    uint32_t q = (uint32_t)(q_sorted[i] >> 32);
    if (q == VS_INVALID_NODE) return;
    if (i == 0 || (uint32_t)(q_sorted[i - 1] >> 32) != q) seg_start[atomicAdd(nseg, 1u)] = i;
}

// in-LDS bitonic sort of u64 keys (n padded to pow2 with ~0)
__device__ void wave_bitonic_sort(uint64_t* keys, uint32_t npow2, int lane) {
    for (uint32_t k = 2; k <= npow2; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = lane; i < npow2; i += WAVE) {
                uint32_t ixj = i ^ j;
                if (ixj > i) {
                    uint64_t a = keys[i], b = keys[ixj];
                    bool up = (i & k) == 0;
                    if ((a > b) == up) {
                        keys[i] = b;
                        keys[ixj] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// ---- out-edges of the new nodes of one batch, labeled vector sets -------------------------------------------------
// Same job as k_build_prune_new with what Graph::insert does for a labeled vector (AM/graph/mod.rs:637-662, 212-266): the
// node itself is dropped from its candidates (it is the start node of a label it is the first to carry), the second pass
// (merge_existing) adds the neighbors the filtered pass left in the row, and pruning uses the label rule.  Candidates are
// re-sorted by (distance, id) after the merge.  cap = power of two >= vmax + R.
__global__ __launch_bounds__(WAVE) void k_build_prune_merge(const uint64_t* __restrict__ codes, uint32_t stride,
                                                            uint32_t* __restrict__ nbrs, uint32_t nbr_stride, uint32_t R,
                                                            float max_alpha, uint32_t b0, uint32_t bn,
                                                            const uint32_t* __restrict__ vis_ids,
                                                            const uint32_t* __restrict__ vis_d,
                                                            const uint32_t* __restrict__ vis_cnt, uint32_t vmax, uint32_t cap,
                                                            uint32_t use_lds_codes, uint32_t merge_existing,
                                                            const uint32_t* __restrict__ label_off,
                                                            const int16_t* __restrict__ label_val,
                                                            uint64_t* __restrict__ edge_q, uint64_t* __restrict__ edge_pd) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    if (b >= bn) return;
    const uint32_t p = b0 + b;
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);  // [cap]
    uint64_t* pm = keys + cap;                            // [cap]
    uint32_t* cid = reinterpret_cast<uint32_t*>(pm + cap);
    uint32_t* cd = cid + cap;
    float* maxf = reinterpret_cast<float*>(cd + cap);
    uint32_t* sel = reinterpret_cast<uint32_t*>(maxf + cap);
    uint64_t* ccode = reinterpret_cast<uint64_t*>(sel + round_up_u32(R, 4));
    const uint32_t C0 = min(vis_cnt[b], vmax);
    for (uint32_t t = lane; t < cap; t += WAVE) {
        uint64_t key = ~0ull;
        if (t < C0) {
            const uint32_t id = vis_ids[(size_t)b * vmax + t];
            if (id != p) key = ((uint64_t)vis_d[(size_t)b * vmax + t] << 32) | id;  // "remove myself"
        }
        keys[t] = key;
    }
    __syncthreads();
    uint32_t* row = nbrs + (size_t)p * nbr_stride;
    if (merge_existing) {  // add_neighbors: the list so far + the new candidates, each id once
        const uint64_t* cp = codes + (size_t)p * stride;
        for (uint32_t t = lane; t < R; t += WAVE) {
            const uint32_t id = row[t];
            if (id == VS_INVALID_NODE || id == p) continue;
            bool dup = false;
            for (uint32_t u = 0; u < C0 && !dup; ++u) dup = (uint32_t)keys[u] == id && keys[u] != ~0ull;
            if (!dup) keys[C0 + t] = ((uint64_t)ham_words(codes + (size_t)id * stride, cp, stride) << 32) | id;
        }
        __syncthreads();
    }
    wave_bitonic_sort(keys, cap, lane);
    uint32_t T = 0;
    for (uint32_t t0 = 0; t0 < cap; t0 += WAVE) T += (uint32_t)__popcll(__ballot(keys[t0 + lane] != ~0ull));
    for (uint32_t t = lane; t < T; t += WAVE) {
        cid[t] = (uint32_t)keys[t];
        cd[t] = (uint32_t)(keys[t] >> 32);
        pm[t] = label_off ? label_pmask(label_off, label_val, p, (uint32_t)keys[t]) : 0ull;
    }
    __syncthreads();
    if (use_lds_codes) {
        stage_codes(ccode, codes, cid, T, stride, lane);
        __syncthreads();
    }
    uint32_t nres;
    if (T <= R) {  // Graph::add_neighbors prunes only a candidate list longer than num_neighbors (AM/graph/mod.rs:243-256)
        for (uint32_t t = lane; t < T; t += WAVE) sel[t] = t;
        nres = T;
        __syncthreads();
    } else {
        nres = wave_prune_ham(cid, cd, T, use_lds_codes ? ccode : nullptr, codes, stride, R, max_alpha, maxf, sel, lane,
                          label_off ? pm : nullptr);
    }
    for (uint32_t t = lane; t < nbr_stride; t += WAVE) row[t] = t < nres ? cid[sel[t]] : VS_INVALID_NODE;
    for (uint32_t t = lane; t < R; t += WAVE) {  // back-edge requests (q <- p, d)
        const size_t e = (size_t)b * R + t;
        if (t < nres) {
            edge_q[e] = ((uint64_t)cid[sel[t]] << 32) | cd[sel[t]];  // sort key: target, then distance (closest requests first)
            edge_pd[e] = ((uint64_t)cd[sel[t]] << 32) | p;
        } else {
            edge_q[e] = ~0ull;
            edge_pd[e] = 0;
        }
    }
}

// ---- back-edges: one wave per target node q ---------------------------------------------------------------------
// PLAIN: a request carries the forward key plain_key(d(p -> q)) (update_back_pointer reuses it), the target's existing
// neighbours are scored d(q -> v) with q's prepared vector staged in LDS, eight of them per pass.
template <bool PLAIN>
__global__ __launch_bounds__(WAVE) void k_build_backedges(const uint64_t* __restrict__ codes, uint32_t stride,
                                                          uint32_t* __restrict__ nbrs, uint32_t nbr_stride, uint32_t R,
                                                          float max_alpha, const uint64_t* __restrict__ q_sorted,
                                                          const uint64_t* __restrict__ pd_sorted, uint32_t ne,
                                                          const uint32_t* __restrict__ seg_start,
                                                          const uint32_t* __restrict__ nseg_p, uint32_t cmax,
                                                          uint32_t use_lds_codes, const uint32_t* __restrict__ label_off,
                                                          const int16_t* __restrict__ label_val, PlainVecs pv) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const uint32_t nseg = *nseg_p;
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);  // [cmax] (pow2)
    uint64_t* pm = keys + cmax;                           // [cmax] label masks relative to the target (labeled sets only)
    uint32_t* cid = reinterpret_cast<uint32_t*>(pm + cmax);
    uint32_t* cd = cid + cmax;
    float* maxf = reinterpret_cast<float*>(cd + cmax);
    uint32_t* sel = reinterpret_cast<uint32_t*>(maxf + cmax);
    uint64_t* ccode = reinterpret_cast<uint64_t*>(sel + round_up_u32(R, 4));
    for (uint32_t sidx = blockIdx.x; sidx < nseg; sidx += gridDim.x) {
        const uint32_t e0 = seg_start[sidx];
        const uint32_t q = (uint32_t)(q_sorted[e0] >> 32);
        uint32_t* row = nbrs + (size_t)q * nbr_stride;
        // existing degree
        uint32_t deg = 0;
        for (uint32_t c0 = 0; c0 < R; c0 += WAVE) {
            uint32_t t = c0 + lane;
            uint32_t v = t < R ? row[t] : VS_INVALID_NODE;
            uint64_t inval = __ballot(v == VS_INVALID_NODE);
            if (inval) {
                deg = c0 + (uint32_t)__builtin_ctzll(inval);
                break;
            }
            deg = c0 + WAVE;
        }
        deg = min(deg, R);
        // segment length
        uint32_t m = 0;
        while (e0 + m < ne && (uint32_t)(q_sorted[e0 + m] >> 32) == q) ++m;  // uniform scalar loop (short)
        // add_neighbors takes every id once (AM/graph/mod.rs:227-235): a source that already is in the list — the second
        // pass of a labeled set asks again for the back-edges its first pass created — is dropped
        auto in_row = [&](uint32_t pid) -> bool {
            for (uint32_t u = 0; u < deg; ++u)
                if (row[u] == pid) return true;
            return false;
        };
        if (deg + m <= R) {  // room: append in (sorted) order
            uint32_t w = deg;
            for (uint32_t base = 0; base < m; base += WAVE) {
                const uint32_t t = base + lane;
                const uint32_t pid = t < m ? (uint32_t)pd_sorted[e0 + t] : VS_INVALID_NODE;
                const bool ok = t < m && !in_row(pid);
                const uint64_t okm = __ballot(ok);
                if (ok) row[w + (uint32_t)__popcll(okm & ((1ull << lane) - 1ull))] = pid;
                w += (uint32_t)__popcll(okm);
            }
            continue;
        }
        // candidates = existing neighbors (distance computed) + new sources.  A hub can receive more requests in one batch than
        // the candidate array holds: the requests of a target are sorted by distance, so the ones kept are its closest
        const uint32_t take_new = min(m, cmax - deg);
        const uint32_t T = deg + take_new;
        uint32_t np2 = 1;
        while (np2 < T) np2 <<= 1;
        const uint64_t* cq = codes + (size_t)q * stride;
        PlainPair ppd{pv.vecs, pv.vdiv, cid, reinterpret_cast<float*>(ccode), pv.vec_stride, pv.dim, pv.distance_type};
        for (uint32_t t = lane; t < np2; t += WAVE) {
            uint64_t key = ~0ull;
            if (t < deg) {
                uint32_t id = row[t];
                if (!PLAIN) key = ((uint64_t)ham_words(codes + (size_t)id * stride, cq, stride) << 32) | id;
            } else if (t < T) {
                uint64_t pd = pd_sorted[e0 + (t - deg)];
                if (!in_row((uint32_t)pd)) key = pd;  // (dist << 32) | p
            }
            keys[t] = key;
        }
        if constexpr (PLAIN) {
            ppd.stage(q, lane);
            for (uint32_t t0 = 0; t0 < deg; t0 += WAVE / 8) {
                const uint32_t t = t0 + (uint32_t)lane / 8;
                const bool act = t < deg;
                const uint32_t id = act ? row[t] : 0u;
                const float d = ppd.dist(id, act, lane);
                if (act && (lane & 7) == 0) keys[t] = ((uint64_t)plain_key(d) << 32) | id;
            }
        }
        __syncthreads();
        wave_bitonic_sort(keys, np2, lane);
        uint32_t Tv = 0;  // candidates left once the repeated sources are gone (they sorted to the end)
        for (uint32_t t0 = 0; t0 < np2; t0 += WAVE) Tv += (uint32_t)__popcll(__ballot(t0 + lane < np2 && keys[t0 + lane] != ~0ull));
        for (uint32_t t = lane; t < Tv; t += WAVE) {
            cid[t] = (uint32_t)keys[t];
            cd[t] = (uint32_t)(keys[t] >> 32);
            if (label_off) pm[t] = label_pmask(label_off, label_val, q, (uint32_t)keys[t]);  // add_neighbors(q, from_labels = q's)
        }
        __syncthreads();
        if (!PLAIN && use_lds_codes) {
            stage_codes(ccode, codes, cid, Tv, stride, lane);
            __syncthreads();
        }
        uint32_t nres;
        if (Tv <= R) {  // (only repeated sources made the list look too long)
            for (uint32_t t = lane; t < Tv; t += WAVE) sel[t] = t;
            nres = Tv;
            __syncthreads();
        } else if constexpr (PLAIN) {
            nres = wave_prune(ppd, cd, Tv, R, max_alpha, maxf, sel, lane);
        } else {
            nres = wave_prune_ham(cid, cd, Tv, use_lds_codes ? ccode : nullptr, codes, stride, R, max_alpha, maxf, sel, lane,
                              label_off ? pm : nullptr);
        }
        for (uint32_t t = lane; t < nbr_stride; t += WAVE) row[t] = t < nres ? cid[sel[t]] : VS_INVALID_NODE;
        __syncthreads();
    }
}

// ---- repair pass: nodes no scan can reach ---------------------------------------------------------------------------
// Nodes of one batch do not see each other, so of two (near-)identical vectors that arrive together one can lose every
// back-edge to the other (the target prunes it as covered) without gaining the edge between the two that sequential
// insertion gives; a node that cannot be reached from the start node is never returned by a scan.  After the last batch
// the reachable set is computed (level-synchronous sweeps over the neighbor array) and every node outside it is given a
// slot in the list of its closest reachable out-neighbor (vs_build_graph).
__global__ void k_reach_sweep(const uint32_t* __restrict__ nbrs, uint32_t nbr_stride, uint32_t R, uint32_t n,
                              uint8_t* __restrict__ reached, uint32_t level, uint32_t* __restrict__ changed) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * R) return;
    if (reached[i / R] != level) return;  // reached[] holds 1 + the BFS level: only the frontier expands
    const uint32_t v = nbrs[(i / R) * nbr_stride + (i % R)];
    if (v != VS_INVALID_NODE && !reached[v]) {
        reached[v] = (uint8_t)(level + 1);
        *changed = 1;
    }
}

// in-edges that come from reachable nodes of a strictly LOWER BFS level than their target: such a source is reached on a
// path that does not pass through the target, so a target that keeps one of these edges stays reachable whatever else it loses
__global__ void k_count_reached_sources(const uint32_t* __restrict__ nbrs, uint32_t nbr_stride, uint32_t R, uint32_t n,
                                        const uint8_t* __restrict__ reached, uint32_t* __restrict__ indeg) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * R) return;
    const uint8_t ls = reached[i / R];
    if (!ls) return;
    const uint32_t v = nbrs[(i / R) * nbr_stride + (i % R)];
    if (v != VS_INVALID_NODE && reached[v] > ls) atomicAdd(&indeg[v], 1u);
}

// ---- insert: the batch sees itself ----------------------------------------------------------------------------------
// vs_build_graph can let the nodes of one batch ignore each other because a sweep over the whole graph follows it; an insert
// into a 50M-node index cannot afford that sweep, so the nodes of an insert batch are made candidates of one another first.
// k_batch_mates: for every row i of `n` code rows, the c nearest OTHER rows by (Hamming, row number), ties to the lower row.
// A tiled all-pairs xor + popcount: one wave owns 64 rows and walks the column tiles of 64 rows; the two tiles of a chunk of
// KW code words sit in LDS, a lane accumulates an 8 x 8 block of pairs in registers, the finished 64 x 64 distances go
// through LDS to the per-row top-c lists (sorted keys (hamming << 32) | row, kept in LDS across the column tiles).  A tile
// only touches a row's list when one of its 64 candidates beats the list's last entry.  Rows are `stride` words (zero
// padded), any W; rows past n read as absent.  c <= 64.
#define MATES_KW 8
// one row's sorted top-c list (LDS) takes in a tile's 64 keys, one per lane (~0: none): every entry ranks itself among the 128
__device__ __forceinline__ void mates_merge(uint64_t* best_row /*LDS [c]*/, uint32_t c, uint64_t key, uint64_t* scratch /*LDS [128]*/, int lane) {
    const uint64_t mine = (uint32_t)lane < c ? best_row[lane] : ~0ull;
    scratch[lane] = mine;
    scratch[64 + lane] = key;
    __syncthreads();
    uint32_t rk_m = 0, rk_k = 0;  // keys are distinct (a row number occurs once); absent entries rank nowhere
    for (uint32_t t = 0; t < 128; ++t) {
        const uint64_t o = scratch[t];
        rk_m += o < mine;
        rk_k += o < key;
    }
    __syncthreads();
    if (mine != ~0ull && rk_m < c) best_row[rk_m] = mine;
    if (key != ~0ull && rk_k < c) best_row[rk_k] = key;
    __syncthreads();
}
// label_off != nullptr (the filtered pass of a labeled set): row r is node label_base + r, and only rows whose label sets overlap
// are mates — what the label filter of the pass's search admits.
__global__ __launch_bounds__(WAVE) void k_batch_mates(const uint64_t* __restrict__ codes, uint32_t stride, uint32_t n, uint32_t c,
                                                      uint32_t* __restrict__ out_ids, uint32_t* __restrict__ out_ham,
                                                      const uint32_t* __restrict__ label_off, const int16_t* __restrict__ label_val,
                                                      uint32_t label_base) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* ta = reinterpret_cast<uint64_t*>(smem);          // [64][MATES_KW + 1]
    uint64_t* tb = ta + 64 * (MATES_KW + 1);                   // [64][MATES_KW + 1]
    uint64_t* scratch = tb + 64 * (MATES_KW + 1);              // [128]
    uint64_t* best = scratch + 128;                            // [64][c]
    uint32_t* dist = reinterpret_cast<uint32_t*>(best + 64 * c);  // [64][65]
    const int lane = threadIdx.x;
    const uint32_t i0 = blockIdx.x * 64u;
    if (i0 >= n) return;
    const uint32_t ty = (uint32_t)lane >> 3, tx = (uint32_t)lane & 7u;
    for (uint32_t t = lane; t < 64 * c; t += WAVE) best[t] = ~0ull;
    __syncthreads();
    for (uint32_t j0 = 0; j0 < n; j0 += 64) {
        uint32_t acc[8][8];
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b) acc[a][b] = 0;
        for (uint32_t w0 = 0; w0 < stride; w0 += MATES_KW) {
            for (uint32_t t = lane; t < 64 * MATES_KW; t += WAVE) {
                const uint32_t r = t / MATES_KW, w = t % MATES_KW;
                const bool wok = w0 + w < stride;
                ta[r * (MATES_KW + 1) + w] = (wok && i0 + r < n) ? codes[(size_t)(i0 + r) * stride + w0 + w] : 0ull;
                tb[r * (MATES_KW + 1) + w] = (wok && j0 + r < n) ? codes[(size_t)(j0 + r) * stride + w0 + w] : 0ull;
            }
            __syncthreads();
            for (uint32_t w = 0; w < MATES_KW; ++w) {
                uint64_t xa[8], xb[8];
#pragma unroll
                for (int a = 0; a < 8; ++a) xa[a] = ta[(ty * 8 + a) * (MATES_KW + 1) + w];
#pragma unroll
                for (int b = 0; b < 8; ++b) xb[b] = tb[(tx * 8 + b) * (MATES_KW + 1) + w];
#pragma unroll
                for (int a = 0; a < 8; ++a)
#pragma unroll
                    for (int b = 0; b < 8; ++b) acc[a][b] += (uint32_t)__popcll(xa[a] ^ xb[b]);
            }
            __syncthreads();
        }
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b) dist[(ty * 8 + a) * 65 + tx * 8 + b] = acc[a][b];
        __syncthreads();
        for (uint32_t r = 0; r < 64 && i0 + r < n; ++r) {  // (uniform: the block is one wave)
            const uint32_t j = j0 + (uint32_t)lane;
            uint64_t key = (j < n && j != i0 + r) ? ((uint64_t)dist[r * 65 + lane] << 32) | j : ~0ull;
            const uint64_t last = best[r * c + c - 1];
            if (label_off && key < last && label_pmask(label_off, label_val, label_base + i0 + r, label_base + j) == 0) key = ~0ull;
            if (!__ballot(key < last)) continue;
            mates_merge(best + r * c, c, key, scratch, lane);
        }
        __syncthreads();
    }
    for (uint32_t t = lane; t < 64 * c; t += WAVE) {
        const uint32_t r = t / c;
        if (i0 + r >= n) continue;
        const uint64_t k = best[t];
        out_ids[(size_t)(i0 + r) * c + (t - r * c)] = k == ~0ull ? VS_INVALID_NODE : (uint32_t)k;
        out_ham[(size_t)(i0 + r) * c + (t - r * c)] = k == ~0ull ? 0xFFFFFFFFu : (uint32_t)(k >> 32);
    }
}
static size_t mates_lds_bytes(uint32_t c) { return (size_t)(2 * 64 * (MATES_KW + 1) + 128 + 64 * c) * 8 + 64 * 65 * 4; }

// k_batch_mates_plain: the same for rows first .. first + n - 1 of a plain index, by (plain_key(d(row -> other)), row).  The pair
// distance has to come out of plain_dist8's accumulation order, so this is no tiled product: a wave owns MATESP_ROWS rows, stages
// one of them at a time as the query side and walks all n rows eight per pass (8-lane groups, 16-byte loads); a tile of 64 keys
// goes through LDS to the row's top-c list exactly as above.  out_key holds the keys (0xFFFFFFFF where there is no mate).
#define MATESP_ROWS 16
__global__ __launch_bounds__(WAVE) void k_batch_mates_plain(PlainVecs pv, uint32_t first, uint32_t n, uint32_t c,
                                                            uint32_t* __restrict__ out_ids, uint32_t* __restrict__ out_key) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* scratch = reinterpret_cast<uint64_t*>(smem);            // [128]
    uint64_t* best = scratch + 128;                                    // [MATESP_ROWS][c]
    uint32_t* dist = reinterpret_cast<uint32_t*>(best + MATESP_ROWS * c);  // [64]
    float* qv = reinterpret_cast<float*>(dist + 64);                   // [round_up(dim, 4)]
    const int lane = threadIdx.x;
    const uint32_t i0 = blockIdx.x * MATESP_ROWS;
    if (i0 >= n) return;
    for (uint32_t t = lane; t < MATESP_ROWS * c; t += WAVE) best[t] = ~0ull;
    PlainPair pd{pv.vecs, pv.vdiv, nullptr, qv, pv.vec_stride, pv.dim, pv.distance_type};
    for (uint32_t r = 0; r < MATESP_ROWS && i0 + r < n; ++r) {  // (uniform: the block is one wave)
        pd.stage(first + i0 + r, lane);
        for (uint32_t j0 = 0; j0 < n; j0 += 64) {
            for (uint32_t p0 = 0; p0 < 64; p0 += WAVE / 8) {
                const uint32_t jj = p0 + (uint32_t)lane / 8;
                const bool act = j0 + jj < n;
                const float d = pd.dist(act ? first + j0 + jj : 0u, act, lane);
                if ((lane & 7) == 0) dist[jj] = act ? plain_key(d) : 0xFFFFFFFFu;
            }
            __syncthreads();
            const uint32_t j = j0 + (uint32_t)lane;
            const uint64_t key = (j < n && j != i0 + r) ? ((uint64_t)dist[lane] << 32) | j : ~0ull;
            const uint64_t last = best[r * c + c - 1];
            if (__ballot(key < last)) mates_merge(best + r * c, c, key, scratch, lane);
            __syncthreads();
        }
    }
    __syncthreads();
    for (uint32_t t = lane; t < MATESP_ROWS * c; t += WAVE) {
        const uint32_t r = t / c;
        if (i0 + r >= n) continue;
        const uint64_t k = best[t];
        out_ids[(size_t)(i0 + r) * c + (t - r * c)] = k == ~0ull ? VS_INVALID_NODE : (uint32_t)k;
        out_key[(size_t)(i0 + r) * c + (t - r * c)] = k == ~0ull ? 0xFFFFFFFFu : (uint32_t)(k >> 32);
    }
}
static size_t mates_plain_lds_bytes(uint32_t c, uint32_t dim) { return (size_t)(128 + MATESP_ROWS * c) * 8 + 64 * 4 + (size_t)round_up_u32(dim, 4) * 4; }

// k_prune_plain: what add_neighbors makes of a caller's candidate set for point p (vs_prune_plain): every id once, never p,
// keyed plain_key(d(p -> id)), sorted by (key, id) — a repeated id repeats its key, so it sorts next to itself and is dropped
// there — then all of them when they fit the list, else wave_prune.  One wave per point; cap (a power of two) bounds the set.
__global__ __launch_bounds__(WAVE) void k_prune_plain(PlainVecs pv, uint32_t R, float max_alpha, const uint32_t* __restrict__ points,
                                                      const uint32_t* __restrict__ cand_off, const uint32_t* __restrict__ cand_ids,
                                                      uint32_t np, uint32_t cap, uint32_t* __restrict__ out_rows,
                                                      uint32_t* __restrict__ out_len) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);  // [cap]
    uint32_t* cid = reinterpret_cast<uint32_t*>(keys + cap);
    uint32_t* cd = cid + cap;
    float* maxf = reinterpret_cast<float*>(cd + cap);
    uint32_t* sel = reinterpret_cast<uint32_t*>(maxf + cap);
    float* qv = reinterpret_cast<float*>(sel + round_up_u32(R, 4));
    const int lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    if (b >= np) return;
    const uint32_t p = points[b], c0 = cand_off[b], C0 = min(cand_off[b + 1] - c0, cap);
    PlainPair pd{pv.vecs, pv.vdiv, cid, qv, pv.vec_stride, pv.dim, pv.distance_type};
    for (uint32_t t = lane; t < cap; t += WAVE) keys[t] = ~0ull;
    pd.stage(p, lane);
    for (uint32_t t0 = 0; t0 < C0; t0 += WAVE / 8) {
        const uint32_t t = t0 + (uint32_t)lane / 8;
        const uint32_t id = t < C0 ? cand_ids[c0 + t] : p;
        const bool act = id != p;  // "remove myself"
        const float d = pd.dist(act ? id : 0u, act, lane);
        if (act && (lane & 7) == 0) keys[t] = ((uint64_t)plain_key(d) << 32) | id;
    }
    __syncthreads();
    wave_bitonic_sort(keys, cap, lane);
    uint32_t T = 0;
    for (uint32_t t0 = 0; t0 < cap; t0 += WAVE) {
        const uint32_t t = t0 + (uint32_t)lane;
        const uint64_t k = keys[t];
        const bool ok = k != ~0ull && (t == 0 || keys[t - 1] != k);
        const uint64_t okm = __ballot(ok);
        if (ok) {
            const uint32_t pos = T + (uint32_t)__popcll(okm & ((1ull << lane) - 1ull));
            cid[pos] = (uint32_t)k;
            cd[pos] = (uint32_t)(k >> 32);
        }
        T += (uint32_t)__popcll(okm);
    }
    __syncthreads();
    uint32_t nres;
    if (T <= R) {  // Graph::add_neighbors prunes only a candidate list longer than num_neighbors (AM/graph/mod.rs:243-256)
        for (uint32_t t = lane; t < T; t += WAVE) sel[t] = t;
        nres = T;
        __syncthreads();
    } else {
        nres = wave_prune(pd, cd, T, R, max_alpha, maxf, sel, lane);
    }
    for (uint32_t t = lane; t < R; t += WAVE) out_rows[(size_t)b * R + t] = t < nres ? cid[sel[t]] : VS_INVALID_NODE;
    if (lane == 0) out_len[b] = nres;
}
static size_t prune_plain_lds_bytes(uint32_t cap, uint32_t R, uint32_t dim) {
    return (size_t)cap * 20 + (size_t)round_up_u32(R, 4) * 4 + (size_t)round_up_u32(dim, 4) * 4;
}

// k_insert_merge_mates: the mates of new node b0 + b (row numbers inside the batch, sorted by (Hamming, row)) join its candidate
// list (vis_ids / vis_d of the build-mode search: ascending by distance, of equal distances the node visited later first) before
// pruning: every id once, never the node itself, the first vmax kept.  The merge is the stable one on the distance alone, an entry
// of the visited list before a mate at the same distance.  (Places used to come from whole (distance, id) keys.  That is the same
// merge while every visited id is below every mate's — always, unless the second pass of a labeled set visits rows of its own
// batch — but the list is not ordered by id among equal distances, so such keys are not monotone along it in general.)  One
// wave per node; both lists are staged in LDS and every entry computes its own place in the merged order (its index + the
// entries of the other list that come before it).
__global__ __launch_bounds__(WAVE) void k_insert_merge_mates(uint32_t b0, uint32_t bn, uint32_t* __restrict__ vis_ids,
                                                             uint32_t* __restrict__ vis_d, uint32_t* __restrict__ vis_cnt, uint32_t vmax,
                                                             const uint32_t* __restrict__ mate_ids, const uint32_t* __restrict__ mate_ham,
                                                             uint32_t c) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* vk = reinterpret_cast<uint64_t*>(smem);  // [vmax]
    uint64_t* mk = vk + vmax;                           // [64]
    const int lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    if (b >= bn) return;
    const uint32_t p = b0 + b;
    const uint32_t C0 = min(vis_cnt[b], vmax);
    for (uint32_t t = lane; t < C0; t += WAVE) vk[t] = ((uint64_t)vis_d[(size_t)b * vmax + t] << 32) | vis_ids[(size_t)b * vmax + t];
    __syncthreads();
    // the mates that are new to the list, packed in their order
    uint64_t key = ~0ull;
    if ((uint32_t)lane < c) {
        const uint32_t m = mate_ids[(size_t)b * c + lane];
        if (m != VS_INVALID_NODE && b0 + m != p) {
            key = ((uint64_t)mate_ham[(size_t)b * c + lane] << 32) | (b0 + m);
            for (uint32_t t = 0; t < C0; ++t)
                if ((uint32_t)vk[t] == b0 + m) key = ~0ull;
        }
    }
    const uint64_t okm = __ballot(key != ~0ull);
    const uint32_t nm = (uint32_t)__popcll(okm);
    if (nm == 0) return;  // (uniform)
    const uint32_t mpos = (uint32_t)__popcll(okm & ((1ull << lane) - 1ull));
    if (key != ~0ull) mk[mpos] = key;
    __syncthreads();
    const uint32_t T = min(C0 + nm, vmax);
    for (uint32_t t = lane; t < C0; t += WAVE) {
        const uint64_t k = vk[t];
        uint32_t before = 0;
        for (uint32_t u = 0; u < nm; ++u) before += (uint32_t)(mk[u] >> 32) < (uint32_t)(k >> 32);  // mates strictly closer
        const uint32_t pos = t + before;
        if (pos < T) {
            vis_ids[(size_t)b * vmax + pos] = (uint32_t)k;
            vis_d[(size_t)b * vmax + pos] = (uint32_t)(k >> 32);
        }
    }
    if ((uint32_t)lane < nm) {
        const uint64_t k = mk[lane];
        uint32_t lo = 0, hi = C0;  // entries of the visited list at most as far as k
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((uint32_t)(vk[mid] >> 32) <= (uint32_t)(k >> 32)) lo = mid + 1;
            else hi = mid;
        }
        const uint32_t pos = (uint32_t)lane + lo;
        if (pos < T) {
            vis_ids[(size_t)b * vmax + pos] = (uint32_t)k;
            vis_d[(size_t)b * vmax + pos] = (uint32_t)(k >> 32);
        }
    }
    if (lane == 0) vis_cnt[b] = T;
}

// k_insert_anchor: one round of the anchoring rule over the new nodes b0 .. b0 + bn - 1.  A new node is ANCHORED when the row of
// an old node (id < b0) names it, or the row of an already anchored node of the range does; of the rows that could, the ones
// looked at are those of the node's own out-neighbors (a back-edge is only ever asked of those): R rows, one ballot per 64
// entries.  Two new nodes that only name each other never become anchored.  The host repeats the launch until a round changes
// nothing (flags only go 0 -> 1, so the fixed point does not depend on the order the waves run in).  mate_cnt (may be null):
// += the out-edges of the range that point into the range.
__global__ __launch_bounds__(WAVE) void k_insert_anchor(const uint32_t* __restrict__ nbrs, uint32_t nbr_stride, uint32_t R, uint32_t b0,
                                                        uint32_t bn, uint32_t* __restrict__ anch, uint32_t* __restrict__ changed,
                                                        uint32_t* __restrict__ mate_cnt) {
    const int lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    if (b >= bn) return;
    const uint32_t x = b0 + b;
    const uint32_t* rowx = nbrs + (size_t)x * nbr_stride;
    if (mate_cnt) {
        uint32_t m = 0;
        for (uint32_t c0 = 0; c0 < R; c0 += WAVE) {
            const uint32_t v = c0 + lane < R ? rowx[c0 + lane] : VS_INVALID_NODE;
            m += (uint32_t)__popcll(__ballot(v != VS_INVALID_NODE && v >= b0 && v - b0 < bn));
        }
        if (lane == 0 && m) atomicAdd(mate_cnt, m);
    }
    if (anch[b]) return;
    for (uint32_t t = 0; t < R; ++t) {
        const uint32_t y = rowx[t];  // (uniform)
        if (y == VS_INVALID_NODE) break;
        if (y >= b0 && (y - b0 >= bn || !anch[y - b0])) continue;
        const uint32_t* rowy = nbrs + (size_t)y * nbr_stride;
        bool found = false;
        for (uint32_t c0 = 0; c0 < R && !found; c0 += WAVE) {
            const uint32_t v = c0 + lane < R ? rowy[c0 + lane] : VS_INVALID_NODE;
            found = __ballot(v == x) != 0;
        }
        if (found) {
            if (lane == 0) {
                anch[b] = 1;
                *changed = 1;
            }
            return;
        }
    }
}

// what the kernels need of a plain index to score pairs, or why this index cannot be scored
static int plain_pair_args(vs_index* ix, const char* what, PlainVecs* pv) {
    VS_REQUIRE(ix, "%s: index is NULL", what);
    VS_REQUIRE(ix->d.storage_type == VS_STORAGE_PLAIN, "%s: plain storage indexes only", what);
    VS_REQUIRE(ix->vecs && ix->vnorm, "%s: needs the vector column on the device", what);
    // DistanceWithTieBreak::new asserts distance >= 0 (AM/graph/neighbor_with_distance.rs), which -dot violates: the reference has
    // no build-time behaviour for the inner product on plain storage
    VS_REQUIRE(ix->d.distance_type != VS_IP, "%s: plain storage has no build-time pair distance for the inner-product distance", what);
    const bool truncated = ix->d.dim_index < ix->d.dim_full;
    VS_REQUIRE(ix->d.distance_type != VS_COSINE || !truncated || ix->vnorm_idx, "%s: the index has no divisors for its index slices", what);
    pv->vecs = ix->vecs;
    pv->vdiv = ix->d.distance_type == VS_COSINE ? (truncated ? ix->vnorm_idx : ix->vnorm) : nullptr;
    pv->vec_stride = ix->vec_stride;
    pv->dim = ix->d.dim_index;
    pv->distance_type = ix->d.distance_type;
    return VS_OK;
}

// ---- what the entry points below share ------------------------------------------------------------------------------------
// The states a call that rewrites or moves the index refuses to work in (VS_ERR_STATE), each with the caller's reason in its text.
static int state_error(const char* what, const char* fmt, const char* arg = "") {
    char msg[256];
    snprintf(msg, sizeof msg, fmt, arg);
    vs_set_error("%s: %s", what, msg);
    return VS_ERR_STATE;
}
static int require_no_batch(vs_index* ix, const char* what) {
    return ix->ws.pending ? state_error(what, "a batch of this handle is in flight (vs_search_batch_dev_finish first)") : VS_OK;
}
// why: what the writer fixed at open that the call would change
static int require_no_writer(vs_index* ix, const char* what, const char* why) {
    return vs_index_open_writers(ix) > 0 ? state_error(what, "a vs_pages_out writer of this index is open (%s; vs_pages_out_close first)", why) : VS_OK;
}
// done: what the call would have to do to a mask the library does not own ("grown", "compacted")
static int require_own_mask(vs_index* ix, const char* what, const char* done) {
    if (!ix->visible || ix->visible == ix->visible_own) return VS_OK;
    for (const uint8_t* sp : ix->snap)
        if (sp == ix->visible) return VS_OK;
    return state_error(what, "a caller-owned device visibility mask is in force and cannot be %s by the library (clear or replace it)", done);
}
static const char* const WRITER_ROWS_MIX = "its pages would mix rows from before and after";

// The nodes scans start from — the default start node and every per-label one — ascending and unique.  label_nodes: the host copy of
// ls_nodes when the caller has fetched it already.
static int collect_start_nodes(vs_index* ix, const char* what, std::vector<uint32_t>* starts, const uint32_t* label_nodes = nullptr) {
    const size_t ns = ix->d.n_label_starts;
    starts->assign(1 + ns, ix->d.default_start);
    if (ns && label_nodes) memcpy(starts->data() + 1, label_nodes, ns * 4);
    else if (ns) VS_HIP(hipMemcpy(starts->data() + 1, ix->ls_nodes, ns * 4, hipMemcpyDeviceToHost));
    std::sort(starts->begin(), starts->end());
    starts->erase(std::unique(starts->begin(), starts->end()), starts->end());
    VS_REQUIRE(starts->back() < ix->d.n, "%s: start node %u of an index of %u nodes", what, starts->back(), ix->d.n);
    return VS_OK;
}

// the label sets of n rows as a caller hands them over: CSR offsets from 0, at most 64 labels per row, each set ascending
static int validate_label_csr(const char* what, const uint32_t* label_off, const int16_t* label_val, uint32_t n) {
    VS_REQUIRE(label_off[0] == 0, "%s: label_off[0] must be 0", what);
    for (uint32_t i = 0; i < n; ++i) {
        VS_REQUIRE(label_off[i] <= label_off[i + 1], "%s: label_off must be non-decreasing", what);
        VS_REQUIRE(label_off[i + 1] - label_off[i] <= 64, "%s: row %u carries more than 64 labels", what, i);
        VS_REQUIRE(label_off[i + 1] == label_off[i] || label_val, "%s: label_val is NULL", what);
        for (uint32_t j = label_off[i] + 1; j < label_off[i + 1]; ++j)
            VS_REQUIRE(label_val[j - 1] < label_val[j], "%s: row %u: label set must be sorted and de-duplicated", what, i);
    }
    return VS_OK;
}

// What the default start node reaches (k_reach_sweep, one BFS level per sweep): mark[i] = 1 + the level of node i, 0 = not reached.
// mark holds n + 8 bytes: the flags, then (4-byte aligned) the `changed` word.  *converged = false: more than 254 levels deep.
static int reach_from_default_start(vs_index* ix, uint8_t* mark, bool* converged) {
    hipStream_t st = ix->ctx->stream;
    const uint32_t n = ix->d.n, R = ix->d.num_neighbors;
    uint32_t* d_changed = reinterpret_cast<uint32_t*>(mark + (((size_t)n + 3) & ~(size_t)3));
    const dim3 cgrid((unsigned)(((size_t)n * R + 255) / 256));
    VS_HIP(hipMemsetAsync(mark, 0, (size_t)n + 8, st));
    const uint8_t one = 1;
    VS_HIP(hipMemcpyAsync(mark + ix->d.default_start, &one, 1, hipMemcpyHostToDevice, st));
    *converged = false;
    for (uint32_t level = 1; level < 255 && !*converged; ++level) {
        uint32_t changed = 0;
        VS_HIP(hipMemsetAsync(d_changed, 0, 4, st));
        hipLaunchKernelGGL(k_reach_sweep, cgrid, dim3(256), 0, st, (const uint32_t*)ix->nbrs, ix->nbr_stride, R, n, mark, level, d_changed);
        VS_HIP(hipGetLastError());
        VS_HIP(hipMemcpyAsync(&changed, d_changed, 4, hipMemcpyDeviceToHost, st));
        VS_HIP(hipStreamSynchronize(st));
        *converged = changed == 0;
    }
    return VS_OK;
}

// the five vs_index_*_kernel_ms getters: what accumulated in acc[0 .. n), cleared on request
static int read_kernel_ms(const char* what, vs_index* ix, double* acc, int n, double* ms, int reset) {
    VS_REQUIRE(ix && ms, "%s: bad args", what);
    for (int k = 0; k < n; ++k) {
        ms[k] = acc[k];
        if (reset) acc[k] = 0;
    }
    return VS_OK;
}

// the scratch of the batch machinery (non-owning: every buffer belongs to the DevScope of the call)
struct BuildBufs {
    uint32_t *vis_ids = nullptr, *vis_d = nullptr, *vis_cnt = nullptr, *stats = nullptr, *status = nullptr;
    uint32_t* hash = nullptr;
    uint64_t* heap_g = nullptr;
    uint32_t *seg_start = nullptr, *nseg = nullptr;
    uint64_t *edge_q = nullptr, *edge_q_sorted = nullptr;  // (target << 32) | distance
    uint64_t *edge_pd = nullptr, *edge_pd_sorted = nullptr;
    void* cub_tmp = nullptr;
    size_t cub_bytes = 0;
    uint32_t *f_ghash = nullptr, *f_heap = nullptr, *f_pool = nullptr;  // fast-kernel overflow table / heap spill / pool counter
    uint32_t *mate_ids = nullptr, *mate_ham = nullptr;                   // insert: [batch][c] mates of the batch's nodes
    uint32_t* anch = nullptr;                                            // insert: [rows of the call] anchored flags, then `changed`, then the mate-edge count
};

// The batch machinery shared by vs_build_graph and vs_index_insert: capacities and buffers of the build-mode search (init), and one
// batch (run): searches for the new nodes b0 .. b0 + bn - 1 over the graph as it stands, their out-edges, the back-edges.
struct BatchRunner {
    vs_index* ix = nullptr;
    DevScope* sc = nullptr;
    BuildBufs B;
    hipStream_t st = nullptr;
    uint32_t R = 0, stride = 0, L = 0, batch_max = 0;
    float max_alpha = 1.0f;
    bool labeled = false;
    bool plain = false;  // `plain` storage: full-precision pair distances (PlainPair), the general search kernel only
    PlainVecs pv{nullptr, nullptr, 0, 0, 0};
    uint32_t vmax = 0, hl = 512, lh = 0, hcap = 0, hashcap = 0, cmax = 1, mcap = 0;
    uint32_t use_lds_new = 0, use_lds_back = 0, use_lds_merge = 0;
    size_t lds_new = 0, lds_back = 0, lds_merge = 0, hash_alloc = 0, ids_alloc = 0;
    FastLaunch f{};
    bool use_fast = true;
    uint32_t retries = 0;
    // insert only: mates per node (0: the nodes of a batch do not see each other, as in vs_build_graph) and HIP-event time of the
    // three insert kernels (ms[0] k_batch_mates, [1] k_insert_merge_mates, [2] k_insert_anchor)
    // ms[3..5] (build and insert alike, while vs_profile_enable is on): the build-mode searches, the prune of the new nodes, the
    // back-edges (sort, segment heads, k_build_backedges)
    uint32_t mates = 0;
    double ms[6] = {0, 0, 0, 0, 0, 0};
    StageTimer tm;
    const char* what = "";  // the entry point, for its error texts

    // n: the nodes the graph will have when the last batch is in (sizes the default batch and picks the dedup regime)
    int init(vs_index* ix_, DevScope& sc_, const char* what_, uint32_t L_, float max_alpha_, uint32_t batch_max_, uint32_t n) {
        what = what_;
        ix = ix_;
        sc = &sc_;
        vs_ctx* c = ix->ctx;
        st = c->stream;
        R = ix->d.num_neighbors;
        stride = ix->code_stride;
        L = L_;
        max_alpha = max_alpha_;
        labeled = ix->label_off != nullptr;
        plain = ix->d.storage_type == VS_STORAGE_PLAIN;
        if (plain) VS_TRY(plain_pair_args(ix, "vs_build_graph", &pv));
        batch_max = batch_max_;
        if (batch_max == 0) batch_max = std::min<uint32_t>(65536, std::max<uint32_t>(1024, n / 64));
        // capacities of the build-mode search
        vmax = std::max<uint32_t>(round_up_u32(3 * L + 64, 64), 128);      // visited list cap (candidates of prune)
        hcap = (2 * L + 64) * R;                                // heap capacity (global spill beyond hl)
        hashcap = std::max<uint32_t>(next_pow2_u32(2ull * hcap), 256);
        while (cmax < R + 128) cmax <<= 1;  // back-edge candidate cap (pow2, >= R + new sources kept)
        const size_t code_bytes = (size_t)stride * 8;
        use_lds_new = (vmax * code_bytes + vmax * 12 + R * 4 + 64 <= 150 * 1024) ? 1 : 0;
        use_lds_back = (cmax * code_bytes + cmax * 28 + R * 4 + 64 <= 150 * 1024) ? 1 : 0;
        lds_new = (size_t)vmax * 12 + round_up_u32(R, 4) * 4 + (use_lds_new ? vmax * code_bytes : 0) + 64;
        lds_back = (size_t)cmax * 28 + round_up_u32(R, 4) * 4 + (use_lds_back ? cmax * code_bytes : 0) + 64;
        mcap = next_pow2_u32((uint64_t)vmax + R);  // candidates of k_build_prune_merge
        use_lds_merge = (mcap * code_bytes + mcap * 28 + R * 4 + 64 <= 150 * 1024) ? 1 : 0;
        lds_merge = (size_t)mcap * 28 + round_up_u32(R, 4) * 4 + (use_lds_merge ? mcap * code_bytes : 0) + 64;
        if (plain) {  // no code rows in LDS: the area behind sel[] holds one prepared vector
            const size_t qv_bytes = (size_t)round_up_u32(pv.dim, 4) * 4;
            use_lds_new = use_lds_back = 0;
            lds_new = (size_t)vmax * 12 + round_up_u32(R, 4) * 4 + qv_bytes + 64;
            lds_back = (size_t)cmax * 28 + round_up_u32(R, 4) * 4 + qv_bytes + 64;
            VS_REQUIRE(lds_new <= 160 * 1024 && lds_back <= 160 * 1024, "vs_build_graph: %u dimensions do not fit the prune kernels' LDS", pv.dim);
            VS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_build_prune_new<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            VS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_build_backedges<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            VS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_batch_mates_plain),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            // the batch's own rows, prepared as queries, are what k_search<BUILD, PLAIN> reads from the workspace
            VS_TRY(devbuf_reserve(c, ix->d.dim_index < ix->d.dim_full ? ix->ws.q_index : ix->ws.q_full,
                                  (size_t)std::max<uint32_t>(batch_max, 1) * ix->vec_stride * 4));
        }
        VS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_build_prune_new<false>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        VS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_build_backedges<false>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        VS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_build_prune_merge),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));

        const size_t bm = batch_max;
        VS_TRY(sc->alloc(&B.vis_ids, bm * vmax * 4, what));
        VS_TRY(sc->alloc(&B.vis_d, bm * vmax * 4, what));
        VS_TRY(sc->alloc(&B.vis_cnt, bm * 4, what));
        VS_TRY(sc->alloc(&B.stats, bm * ST_N * 4, what));
        VS_TRY(sc->alloc(&B.status, bm * 4, what));
        VS_TRY(sc->alloc(&B.edge_q, bm * R * 8, what));
        VS_TRY(sc->alloc(&B.edge_q_sorted, bm * R * 8, what));
        VS_TRY(sc->alloc(&B.edge_pd, bm * R * 8, what));
        VS_TRY(sc->alloc(&B.edge_pd_sorted, bm * R * 8, what));
        VS_TRY(sc->alloc(&B.seg_start, bm * R * 4, what));
        VS_TRY(sc->alloc(&B.nseg, 4, what));
        VS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, B.cub_bytes, B.edge_q, B.edge_q_sorted, B.edge_pd,
                                                  B.edge_pd_sorted, (int)(bm * R), 0, 64, st));
        VS_TRY(sc->alloc(&B.cub_tmp, B.cub_bytes + 16, what));

        // The searches of a batch run on the LDS-resident kernel (vs_search_fast.hip, BUILD variant); the general kernel only
        // re-runs the scans that outgrow it.  Same operating-point rule as for queries: dedup table in LDS for small graphs,
        // table-less (global table, high occupancy) once a search inserts more ids than an LDS table should hold.
        use_fast = vs_opt_get("VS_BUILD_FAST") ? atoi(vs_opt_get("VS_BUILD_FAST")) != 0 : true;
        if (plain) use_fast = false;  // (the LDS-resident kernel scores codes)
        else {
            const uint64_t nbits = (uint64_t)ix->d.dim_index * ix->d.bits;
            const uint32_t typ_ins = (L + L / 4 + 16) * std::min<uint32_t>(R, 16);
            const bool lds_table = n <= 4000000u && typ_ins <= 3072;
            f.L = L;
            f.M = vmax;
            f.hl = 1023;
            f.hcap = std::max(hcap, f.hl);  // small L * R: the whole heap fits the LDS part (the launcher wants hcap >= hl)
            f.gstride = round_up_u32(f.hcap - f.hl + 2, 2);
            f.lh = lds_table ? std::max<uint32_t>(round_up_u32(typ_ins, 64), 256) : 0;
            f.gcap = next_pow2_u32(std::max<uint32_t>(4 * typ_ins, 1024));
            f.sb = 0;
            while ((1ull << f.sb) < (uint64_t)f.lh + f.gcap) f.sb++;
            f.vr = 0;
            f.vcap = vmax + 64;
            f.minw = 1;
            f.build = 1;
            if (nbits >= (1ull << (32 - f.sb)) || fast_lds_bytes(ix, f) > 64 * 1024) use_fast = false;
            if (use_fast) {
                VS_TRY(sc->alloc(&B.f_ghash, bm * f.gcap * 4, what));
                VS_TRY(sc->alloc(&B.f_heap, bm * f.gstride * 4, what));
                VS_TRY(sc->alloc(&B.f_pool, 64, what));
            }
        }
        return tm.start(*sc, c->profiling, ms, what);  // (vs_profile_enable: HIP-event time of the batch kernels)
    }

    // filtered: the pass from the label start nodes with the label filter (labeled sets only); otherwise from the default
    // start node.  A labeled set's unfiltered pass merges into the rows the filtered pass wrote.  with_mates (insert): the c
    // nearest nodes of the same batch join every node's candidates before pruning.
    int run(uint32_t b0, uint32_t bn, bool filtered, bool with_mates = false) {
        const uint64_t* qcodes = ix->codes + (size_t)b0 * stride;
        // label keys of the searches = the new nodes' own label sets (CSR offsets are absolute into label_val)
        const int16_t* ql = filtered ? ix->label_val : nullptr;
        const uint32_t* qlo = filtered ? ix->label_off + b0 : nullptr;
        if (plain) {  // the new rows as queries: their index slices, prepared as a scan's query is
            DevBuf& qb = ix->d.dim_index < ix->d.dim_full ? ix->ws.q_index : ix->ws.q_full;
            VS_TRY(launch_prepare_index_slice(ix, ix->vecs + (size_t)b0 * ix->vec_stride, bn, (float*)qb.p, ix->vec_stride));
        }
        for (int attempt = 0;; ++attempt) {
            if ((size_t)bn * hashcap * 4 > hash_alloc || !B.hash) {
                sc->free(B.hash);
                hash_alloc = (size_t)batch_max * hashcap * 4;
                VS_TRY(sc->alloc(&B.hash, hash_alloc, what));
            }
            const size_t hg = hcap > hl ? hcap - hl : 0;
            if ((size_t)bn * hg * 8 > ids_alloc || !B.heap_g) {
                sc->free(B.heap_g);
                ids_alloc = std::max<size_t>((size_t)batch_max * hg * 8, 16);
                VS_TRY(sc->alloc(&B.heap_g, ids_alloc, what));
            }
            SearchLaunch s;
            s.nq = bn;
            s.L = L;
            s.M = vmax;
            s.hl = hl;
            s.hcap = hcap;
            s.vcap = vmax + 64;
            s.lh = lh;
            s.hashcap = hashcap;
            s.g0 = std::min<uint32_t>(4096, hashcap);  // first level of the dedup ladder (small L * R: the whole table)
            s.qcodes = qcodes;
            s.qlabels = ql;
            s.qlabel_off = qlo;
            s.heap_g = B.heap_g;
            s.hash = B.hash;
            s.out_ids = B.vis_ids;
            s.out_ham = B.vis_d;
            s.out_cnt = B.vis_cnt;
            s.stats = B.stats;
            s.status = B.status;
            tm.tick();
            if (use_fast && attempt == 0) {
                f.nq = bn;
                f.hcap = std::max(std::min(hcap, f.hl + f.gstride - 2), f.hl);  // (the spill area was sized before the loop)
                f.qcodes = s.qcodes;
                f.qlabels = ql;
                f.qlabel_off = qlo;
                f.heap_g = B.f_heap;
                f.ghash = B.f_ghash;
                f.pool_counter = B.f_pool;
                f.pool_slots = bn;
                f.out_ids = B.vis_ids;
                f.out_ham = B.vis_d;
                f.out_cnt = B.vis_cnt;
                f.stats = B.stats;
                f.status = B.status;
                VS_HIP(hipMemsetAsync(B.f_pool, 0, 64, st));
                VS_TRY(launch_search_fast(ix, f));
            }
            // after the fast kernel (or a failed attempt) only the scans whose status is non-zero are (re)run
            s.only_failed = (use_fast || attempt > 0) ? 1u : 0u;
            VS_TRY(launch_search(ix, s, true));
            tm.tock(3);
            std::vector<uint32_t> status(bn);
            VS_HIP(hipMemcpyAsync(status.data(), B.status, (size_t)bn * 4, hipMemcpyDeviceToHost, st));
            VS_HIP(hipStreamSynchronize(st));
            uint32_t ovf = 0;
            for (uint32_t v : status) ovf |= v;
            if (!ovf) {
                retries += (uint32_t)attempt;
                break;
            }
            if (attempt >= 5) {
                vs_set_error("vs_build_graph: search structures overflowed (flags 0x%x)", ovf);
                return VS_ERR_CAPACITY;
            }
            if (ovf & OVF_VISITED) {
                // the visited list outgrew the prune candidate cap (the build-mode fast kernel truncates to the closest
                // entries itself; this is the general kernel's ring at vcap = vmax + 64): not a combination the LDS holds
                vs_set_error("vs_build_graph: visited list overflow (search_list_size too large for LDS)");
                return VS_ERR_CAPACITY;
            }
            if (ovf & OVF_HEAP) hcap *= 2;
            if (ovf & OVF_HASH) hashcap *= 2;
        }
        if (with_mates && mates && bn > 1) {
            const uint32_t c = mates;
            tm.tick();
            if (plain)
                hipLaunchKernelGGL(k_batch_mates_plain, dim3((bn + MATESP_ROWS - 1) / MATESP_ROWS), dim3(WAVE), mates_plain_lds_bytes(c, pv.dim), st,
                                   pv, b0, bn, c, B.mate_ids, B.mate_ham);
            else
                hipLaunchKernelGGL(k_batch_mates, dim3((bn + 63) / 64), dim3(WAVE), mates_lds_bytes(c), st, ix->codes + (size_t)b0 * stride,
                                   stride, bn, c, B.mate_ids, B.mate_ham, filtered ? ix->label_off : nullptr,
                                   filtered ? ix->label_val : nullptr, b0);
            VS_HIP(hipGetLastError());
            tm.tock(0);
            tm.tick();
            hipLaunchKernelGGL(k_insert_merge_mates, dim3(bn), dim3(WAVE), ((size_t)vmax + 64) * 8, st, b0, bn, B.vis_ids, B.vis_d,
                               B.vis_cnt, vmax, B.mate_ids, B.mate_ham, c);
            VS_HIP(hipGetLastError());
            tm.tock(1);
        }
        // out-edges of the new nodes + back-edge requests
        tm.tick();
        if (labeled)
            hipLaunchKernelGGL(k_build_prune_merge, dim3(bn), dim3(WAVE), lds_merge, st, ix->codes, stride, ix->nbrs,
                               ix->nbr_stride, R, max_alpha, b0, bn, B.vis_ids, B.vis_d, B.vis_cnt, vmax, mcap, use_lds_merge,
                               filtered ? 0u : 1u, ix->label_off, ix->label_val, B.edge_q, B.edge_pd);
        else if (plain)
            hipLaunchKernelGGL(k_build_prune_new<true>, dim3(bn), dim3(WAVE), lds_new, st, ix->codes, stride, ix->nbrs,
                               ix->nbr_stride, R, max_alpha, b0, bn, B.vis_ids, B.vis_d, B.vis_cnt, vmax, 0u, B.edge_q, B.edge_pd, pv);
        else
            hipLaunchKernelGGL(k_build_prune_new<false>, dim3(bn), dim3(WAVE), lds_new, st, ix->codes, stride, ix->nbrs,
                               ix->nbr_stride, R, max_alpha, b0, bn, B.vis_ids, B.vis_d, B.vis_cnt, vmax, use_lds_new,
                               B.edge_q, B.edge_pd, pv);
        VS_HIP(hipGetLastError());
        tm.tock(4);
        tm.tick();
        const uint32_t ne = bn * R;
        size_t tmp_bytes = B.cub_bytes;
        VS_HIP(hipcub::DeviceRadixSort::SortPairs(B.cub_tmp, tmp_bytes, B.edge_q, B.edge_q_sorted, B.edge_pd,
                                                  B.edge_pd_sorted, (int)ne, 0, 64, st));
        VS_HIP(hipMemsetAsync(B.nseg, 0, 4, st));
        hipLaunchKernelGGL(k_seg_heads, dim3((ne + 255) / 256), dim3(256), 0, st, B.edge_q_sorted, ne, B.seg_start, B.nseg);
        VS_HIP(hipGetLastError());
        uint32_t grid = std::min<uint32_t>(ne, 16384);
        if (plain)
            hipLaunchKernelGGL(k_build_backedges<true>, dim3(grid), dim3(WAVE), lds_back, st, ix->codes, stride, ix->nbrs,
                               ix->nbr_stride, R, max_alpha, B.edge_q_sorted, B.edge_pd_sorted, ne, B.seg_start, B.nseg, cmax, 0u,
                               (const uint32_t*)nullptr, (const int16_t*)nullptr, pv);
        else
            hipLaunchKernelGGL(k_build_backedges<false>, dim3(grid), dim3(WAVE), lds_back, st, ix->codes, stride, ix->nbrs,
                               ix->nbr_stride, R, max_alpha, B.edge_q_sorted, B.edge_pd_sorted, ne, B.seg_start, B.nseg, cmax,
                               use_lds_back, labeled ? ix->label_off : nullptr, labeled ? ix->label_val : nullptr, pv);
        VS_HIP(hipGetLastError());
        tm.tock(5);
        return VS_OK;
    }
};

// repair pass (see k_reach_sweep): rounds of { reachable set, in-edges for the nodes outside it } until a sweep finds every
// node (at most eight); what the last sweep still could not reach is reported by vs_index_build_unreachable()
// cls (vs_index_consolidate_deletes only; nullptr: every node counts, as always): per node 0 = live, 1 = a tombstone the consolidation
// dropped from the graph, 2 = a tombstone kept as a start node.  A dropped tombstone is not "lost": it is meant to be unreachable and
// is never handed an in-edge; build_unreachable then counts the LIVE nodes the sweep did not reach.
static int repair_graph(vs_index* ix, DevScope& sc, const uint8_t* cls = nullptr) {
    const char* what = "vs_build_graph (repair)";
    hipStream_t st = ix->ctx->stream;
    const uint32_t n = ix->d.n, R = ix->d.num_neighbors;
    if (n <= 2) return VS_OK;  // (nothing a sweep could find)
    ix->build_unreachable = 0;
    uint8_t* mark = nullptr;  // node is reachable from the start node
    VS_TRY(sc.alloc(&mark, (size_t)n + 8, what));
    std::vector<uint8_t> reached(n);
    std::vector<uint32_t> lost, indeg, row0(R);
    const size_t cells = (size_t)n * R;
    const dim3 cgrid((unsigned)((cells + 255) / 256));
    for (int round = 0; round < 8; ++round) {
        bool converged = false;
        VS_TRY(reach_from_default_start(ix, mark, &converged));
        if (!converged) {  // more than 254 levels deep: not a graph this pass can judge
            ix->build_unreachable = 0xFFFFFFFFu;
            break;
        }
        VS_HIP(hipMemcpyAsync(reached.data(), mark, n, hipMemcpyDeviceToHost, st));
        VS_HIP(hipStreamSynchronize(st));
        lost.clear();
        uint32_t lost_live = 0;
        for (uint32_t i = 0; i < n; ++i)
            if (!reached[i] && !(cls && cls[i] == 1)) {
                lost.push_back(i);
                lost_live += !cls || cls[i] == 0;
            }
        ix->build_unreachable = cls ? lost_live : (uint32_t)lost.size();  // (what the last completed sweep found; 0 when the loop ends here)
        if (lost.empty() || round == 7) break;
        // Each of them takes a slot in the list of its closest reachable out-neighbor — a free one, else that of the last
        // entry that keeps an in-edge from a node of a strictly lower BFS level (indeg[] counts only those: a lower-level
        // source is reached without passing through the entry, so the entry cannot be stranded by losing this edge —
        // counting every reachable source would let two nodes that only reach each other vouch for one another).  Rare
        // (none on the bench corpora), so this runs on the host, in node order; the sweep of the next round re-checks.
        uint32_t* d_indeg = nullptr;
        VS_TRY(sc.alloc(&d_indeg, (size_t)n * 4, what));
        indeg.assign(n, 0);
        VS_HIP(hipMemsetAsync(d_indeg, 0, (size_t)n * 4, st));
        hipLaunchKernelGGL(k_count_reached_sources, cgrid, dim3(256), 0, st, ix->nbrs, ix->nbr_stride, R, n, mark, d_indeg);
        VS_HIP(hipGetLastError());
        VS_HIP(hipMemcpyAsync(indeg.data(), d_indeg, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        VS_HIP(hipStreamSynchronize(st));
        sc.free(d_indeg);
        // the lists of the lost nodes, so that what becomes reachable through a node that was just given a way in is known
        // without another sweep
        std::vector<uint32_t> lrows(lost.size() * (size_t)R), lidx(n, 0xFFFFFFFFu), stack, level(n);
        for (uint32_t i = 0; i < n; ++i) level[i] = reached[i];  // 1 + BFS level (0: not reached); grows past 255 on the host
        for (size_t oi = 0; oi < lost.size(); ++oi) {
            lidx[lost[oi]] = (uint32_t)oi;
            VS_HIP(hipMemcpy(&lrows[oi * R], ix->nbrs + (size_t)lost[oi] * ix->nbr_stride, (size_t)R * 4, hipMemcpyDeviceToHost));
        }
        for (bool progress = true; progress;) {
            progress = false;
            for (size_t oi = 0; oi < lost.size(); ++oi) {
                const uint32_t x = lost[oi];
                if (reached[x]) continue;
                const uint32_t* rowx = &lrows[oi * R];
                bool placed = false;
                for (uint32_t c = 0; c < R && !placed && rowx[c] != VS_INVALID_NODE; ++c) {  // closest first
                    const uint32_t n0 = rowx[c];
                    if (!reached[n0]) continue;
                    uint32_t* rown = lidx[n0] != 0xFFFFFFFFu ? &lrows[(size_t)lidx[n0] * R] : row0.data();
                    if (rown == row0.data())
                        VS_HIP(hipMemcpy(row0.data(), ix->nbrs + (size_t)n0 * ix->nbr_stride, (size_t)R * 4, hipMemcpyDeviceToHost));
                    int slot = -1;
                    for (uint32_t t = 0; t < R && slot < 0; ++t)
                        if (rown[t] == VS_INVALID_NODE) slot = (int)t;
                    for (int t = (int)R - 1; t >= 0 && slot < 0; --t) {
                        const uint32_t y = rown[t];
                        const uint32_t mine = (reached[y] && level[n0] < level[y]) ? 1u : 0u;  // is n0 -> y one of the counted edges?
                        if (indeg[y] >= mine + 1u) slot = t;
                    }
                    if (slot < 0) continue;
                    if (rown[slot] != VS_INVALID_NODE && reached[rown[slot]] && level[n0] < level[rown[slot]]) indeg[rown[slot]]--;
                    rown[slot] = x;
                    level[x] = level[n0] + 1;
                    indeg[x]++;
                    placed = true;
                    VS_HIP(hipMemcpy(ix->nbrs + (size_t)n0 * ix->nbr_stride, rown, (size_t)R * 4, hipMemcpyHostToDevice));
                }
                if (!placed) continue;
                progress = true;
                reached[x] = 1;
                stack.assign(1, x);
                while (!stack.empty()) {  // everything x leads to is reachable now
                    const uint32_t u = stack.back();
                    stack.pop_back();
                    const uint32_t* rowu = &lrows[(size_t)lidx[u] * R];
                    for (uint32_t t = 0; t < R && rowu[t] != VS_INVALID_NODE; ++t) {
                        const uint32_t v = rowu[t];
                        if (cls && cls[v] == 1) continue;  // (a stale edge to a dropped tombstone leads nowhere a scan should go)
                        if (!reached[v]) {
                            reached[v] = 1;
                            level[v] = level[u] + 1;
                            indeg[v]++;
                            stack.push_back(v);
                        } else if (level[u] < level[v]) {
                            indeg[v]++;
                        }
                    }
                }
            }
        }
    }
    return VS_OK;
}

static int build_graph_impl(vs_index* ix, uint32_t L, double max_alpha_d, uint32_t batch_max, DevScope& sc, BatchRunner& br) {
    vs_ctx* c = ix->ctx;
    hipStream_t st = c->stream;
    const uint32_t n = ix->d.n;
    // (every check and every allocation that can refuse the call comes before the first byte of nbrs is written)
    if (n == 0) {
        VS_HIP(hipMemsetAsync(ix->nbrs, 0xFF, (size_t)ix->nbr_stride * 4, st));
        ix->d.default_start = VS_INVALID_NODE;
        return VS_OK;
    }
    const bool labeled = ix->label_off != nullptr;
    if (labeled) {
        // update_start_nodes (AM/graph/mod.rs:490-531): a node is the start node of every label it is the first to carry;
        // nodes arrive in id order, so that is the smallest id per label
        std::vector<uint32_t> off((size_t)n + 1);
        VS_HIP(hipMemcpy(off.data(), ix->label_off, off.size() * 4, hipMemcpyDeviceToHost));
        std::vector<int16_t> val(std::max<size_t>(off[n], 1));
        if (off[n]) VS_HIP(hipMemcpy(val.data(), ix->label_val, (size_t)off[n] * 2, hipMemcpyDeviceToHost));
        std::map<int16_t, uint32_t> first;
        for (uint32_t i = 0; i < n; ++i) {
            VS_REQUIRE(off[i + 1] - off[i] <= 64, "vs_build_graph: node %u carries more than 64 labels", i);
            for (uint32_t j = off[i]; j < off[i + 1]; ++j) first.emplace(val[j], i);
        }
        std::vector<int16_t> sl;
        std::vector<uint32_t> sn;
        for (const auto& kv : first) {
            sl.push_back(kv.first);
            sn.push_back(kv.second);
        }
        VS_TRY(vs_index_set_start_nodes(ix, 0, sl.data(), sn.data(), (uint32_t)sl.size()));
    }
    if (ix->d.storage_type == VS_STORAGE_PLAIN) {  // the divisors the pair distance divides by, from the rows as they stand
        VS_TRY(launch_row_norms(ix));
        VS_TRY(launch_slice_norms_range(ix, 0, n));
    }
    VS_TRY(br.init(ix, sc, "vs_build_graph", L, (float)max_alpha_d, batch_max, n));
    batch_max = br.batch_max;
    VS_HIP(hipMemsetAsync(ix->nbrs, 0xFF, (size_t)n * ix->nbr_stride * 4, st));
    ix->d.default_start = 0;

    uint32_t b0 = 1;  // node 0 is the start node and has no one to link to yet
    uint32_t bsz = 1;
    while (b0 < n) {
        const uint32_t bn = std::min<uint32_t>(std::min<uint32_t>(bsz, batch_max), n - b0);
        if (labeled) VS_TRY(br.run(b0, bn, true));  // Graph::insert: first with the label filter ...
        VS_TRY(br.run(b0, bn, false));              // ... then from the default start node without it
        b0 += bn;
        if (bsz < batch_max) bsz = std::min<uint32_t>(batch_max, bsz * 2);
    }
    VS_HIP(hipStreamSynchronize(st));

    const char* rep_env = vs_opt_get("VS_BUILD_REPAIR");
    if (!(rep_env && *rep_env == '0')) VS_TRY(repair_graph(ix, sc));
    return VS_OK;
}

static int vs_build_graph_impl(vs_index* ix, uint32_t search_list_size, double max_alpha, uint32_t batch_max, uint64_t seed) {
    (void)seed;
    VS_REQUIRE(ix, "vs_build_graph: index is NULL");
    VS_REQUIRE(search_list_size >= 1 && search_list_size <= 1000, "vs_build_graph: search_list_size outside [1,1000]");
    VS_REQUIRE(max_alpha >= 1.0 && max_alpha <= 5.0, "vs_build_graph: max_alpha outside [1,5]");
    VS_REQUIRE(ix->nbrs, "vs_build_graph: the index has no neighbor lists");
    if (ix->d.storage_type == VS_STORAGE_PLAIN) {  // IndexFullDistanceMeasure: pair distances over the vector column
        PlainVecs pv;
        VS_TRY(plain_pair_args(ix, "vs_build_graph", &pv));
        VS_REQUIRE(!ix->label_off, "vs_build_graph: Plain storage does not support label filters");
        VS_TRY(require_no_batch(ix, "vs_build_graph"));
    }
    VS_HIP(hipSetDevice(ix->ctx->device));
    ix->nbr_mask_valid = false;  // (the neighbor lists are about to change: what was derived from them is stale)
    int r;
    {
        DevScope sc(ix->ctx->stream);
        BatchRunner br;
        r = build_graph_impl(ix, search_list_size, max_alpha, batch_max, sc, br);
        for (int k = 0; k < 3; ++k) ix->build_ms[k] += br.ms[3 + k];  // (vs_index_build_kernel_ms)
    }
    // the scan kernels rely on every neighbor list naming a node at most once (as vs_index_upload checks for staged
    // indexes): a list that does not is a defect of this builder, not something to search on
    if (r == VS_OK) r = vs_validate_graph(ix);
    return r;
}
extern "C" int vs_build_graph(vs_index* ix, uint32_t search_list_size, double max_alpha, uint32_t batch_max, uint64_t seed) {
    return vs_guard("vs_build_graph", [&] { return vs_build_graph_impl(ix, search_list_size, max_alpha, batch_max, seed); });
}

// the repair pass on its own: after many inserts, at the caller's choice (an insert only anchors its own rows; what its re-prunes
// cost older rows is what this sweep over the whole graph finds)
static int vs_index_repair_impl(vs_index* ix, uint32_t* unreachable) {
    VS_REQUIRE(ix, "vs_index_repair: index is NULL");
    VS_REQUIRE_OWNER(ix, "vs_index_repair");
    VS_REQUIRE_NO_VIEWS(ix, "vs_index_repair");
    VS_REQUIRE(ix->nbrs, "vs_index_repair: the index has no neighbor lists");
    VS_HIP(hipSetDevice(ix->ctx->device));
    ix->build_unreachable = 0;
    if (ix->d.default_start != VS_INVALID_NODE) {
        ix->nbr_mask_valid = false;
        {
            DevScope sc(ix->ctx->stream);
            VS_TRY(repair_graph(ix, sc));
        }
        VS_TRY(vs_validate_graph(ix));
    }
    if (unreachable) *unreachable = ix->build_unreachable;
    return VS_OK;
}
extern "C" int vs_index_repair(vs_index* ix, uint32_t* unreachable) {
    return vs_guard("vs_index_repair", [&] { return vs_index_repair_impl(ix, unreachable); });
}

// ---- vs_batch_mates: k_batch_mates on its own --------------------------------------------------------------------------
static int vs_batch_mates_impl(vs_index* ix, const uint64_t* codes, const uint32_t* label_off, const int16_t* label_val, uint32_t n,
                               uint32_t c, uint32_t* out_ids, uint32_t* out_ham) {
    VS_REQUIRE(ix && (n == 0 || (codes && out_ids)), "vs_batch_mates: bad args");
    VS_REQUIRE(c >= 1 && c <= 64, "vs_batch_mates: %u mates per row outside [1,64]", c);
    if (n == 0) return VS_OK;
    vs_ctx* ctx = ix->ctx;
    VS_HIP(hipSetDevice(ctx->device));
    const uint32_t stride = ix->code_stride;
    uint64_t* d_codes = nullptr;
    uint32_t *d_out = nullptr, *d_off = nullptr;  // ids, then Hamming distances; the rows' label sets (filtered form)
    int16_t* d_val = nullptr;
    if (label_off) VS_TRY(validate_label_csr("vs_batch_mates_filtered", label_off, label_val, n));
    DevScope sc(ctx->stream);
    VS_TRY(sc.alloc(&d_codes, (size_t)n * stride * 8, "vs_batch_mates"));
    VS_TRY(sc.alloc(&d_out, (size_t)n * c * 8, "vs_batch_mates"));
    VS_TRY(vs_upload_rows(ctx, d_codes, stride * 8ull, codes, ix->d.words * 8ull, ix->d.words * 8ull, n));
    if (label_off) {
        VS_TRY(sc.alloc(&d_off, ((size_t)n + 1) * 4, "vs_batch_mates"));
        VS_TRY(sc.alloc(&d_val, std::max<size_t>(label_off[n], 1) * 2, "vs_batch_mates"));
        VS_TRY(vs_dev_upload(ctx, d_off, label_off, ((size_t)n + 1) * 4));
        if (label_off[n]) VS_TRY(vs_dev_upload(ctx, d_val, label_val, (size_t)label_off[n] * 2));
    }
    hipLaunchKernelGGL(k_batch_mates, dim3((n + 63) / 64), dim3(WAVE), mates_lds_bytes(c), ctx->stream, d_codes, stride, n, c, d_out,
                       d_out + (size_t)n * c, (const uint32_t*)d_off, (const int16_t*)d_val, 0u);
    VS_HIP(hipGetLastError());
    VS_TRY(vs_dev_download(ctx, out_ids, d_out, (size_t)n * c * 4));
    if (out_ham) VS_TRY(vs_dev_download(ctx, out_ham, d_out + (size_t)n * c, (size_t)n * c * 4));
    sc.drained();  // (vs_dev_download returns when the bytes are on the host)
    return VS_OK;
}
extern "C" int vs_batch_mates(vs_index* ix, const uint64_t* codes, uint32_t n, uint32_t c, uint32_t* out_ids, uint32_t* out_ham) {
    return vs_guard("vs_batch_mates", [&] { return vs_batch_mates_impl(ix, codes, nullptr, nullptr, n, c, out_ids, out_ham); });
}
extern "C" int vs_batch_mates_filtered(vs_index* ix, const uint64_t* codes, const uint32_t* label_off, const int16_t* label_val, uint32_t n,
                                       uint32_t c, uint32_t* out_ids, uint32_t* out_ham) {
    return vs_guard("vs_batch_mates_filtered", [&]() -> int {
        VS_REQUIRE(label_off, "vs_batch_mates_filtered: label_off is NULL");
        return vs_batch_mates_impl(ix, codes, label_off, label_val, n, c, out_ids, out_ham);
    });
}

// ---- vs_batch_mates_plain / vs_prune_plain: the two plain-storage build kernels on their own (read-only on the index) --------
static int vs_batch_mates_plain_impl(vs_index* ix, uint32_t first_node, uint32_t n, uint32_t c, uint32_t* out_ids, float* out_dist) {
    PlainVecs pv;
    VS_TRY(plain_pair_args(ix, "vs_batch_mates_plain", &pv));
    VS_REQUIRE(n == 0 || out_ids, "vs_batch_mates_plain: out_ids is NULL");
    VS_REQUIRE(c >= 1 && c <= 64, "vs_batch_mates_plain: %u mates per row outside [1,64]", c);
    VS_REQUIRE((uint64_t)first_node + n <= ix->d.n, "vs_batch_mates_plain: rows %u .. %llu are not all in the index (%u nodes)", first_node,
               (unsigned long long)first_node + n, ix->d.n);
    if (n == 0) return VS_OK;
    vs_ctx* ctx = ix->ctx;
    VS_HIP(hipSetDevice(ctx->device));
    const size_t lds = mates_plain_lds_bytes(c, pv.dim);
    VS_REQUIRE(lds <= 160 * 1024, "vs_batch_mates_plain: %u dimensions do not fit LDS", pv.dim);
    VS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_batch_mates_plain), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    DevScope sc(ctx->stream);
    uint32_t* d_out = nullptr;  // ids, then keys
    VS_TRY(sc.alloc(&d_out, (size_t)n * c * 8, "vs_batch_mates_plain"));
    hipLaunchKernelGGL(k_batch_mates_plain, dim3((n + MATESP_ROWS - 1) / MATESP_ROWS), dim3(WAVE), lds, ctx->stream, pv, first_node, n, c, d_out,
                       d_out + (size_t)n * c);
    VS_HIP(hipGetLastError());
    VS_TRY(vs_dev_download(ctx, out_ids, d_out, (size_t)n * c * 4));
    if (out_dist) {
        VS_TRY(vs_dev_download(ctx, out_dist, d_out + (size_t)n * c, (size_t)n * c * 4));
        // keys -> the f32 distances, bit for bit (the total_cmp image undoes itself); the padding keeps 0xFFFFFFFF
        uint32_t* k = reinterpret_cast<uint32_t*>(out_dist);
        for (size_t i = 0; i < (size_t)n * c; ++i)
            if (out_ids[i] != VS_INVALID_NODE) {
                uint32_t b = k[i] ^ 0x80000000u;
                b ^= (uint32_t)((int32_t)b >> 31) >> 1;
                k[i] = b;
            }
    }
    return VS_OK;
}
extern "C" int vs_batch_mates_plain(vs_index* ix, uint32_t first_node, uint32_t n, uint32_t c, uint32_t* out_ids, float* out_dist) {
    return vs_guard("vs_batch_mates_plain", [&] { return vs_batch_mates_plain_impl(ix, first_node, n, c, out_ids, out_dist); });
}

static int vs_prune_plain_impl(vs_index* ix, const uint32_t* points, const uint32_t* cand_off, const uint32_t* cand_ids, uint32_t np,
                               double max_alpha, uint32_t* out_rows, uint32_t* out_len) {
    PlainVecs pv;
    VS_TRY(plain_pair_args(ix, "vs_prune_plain", &pv));
    VS_REQUIRE(np == 0 || (points && cand_off && out_rows && out_len), "vs_prune_plain: bad args");
    VS_REQUIRE(max_alpha >= 1.0 && max_alpha <= 5.0, "vs_prune_plain: max_alpha outside [1,5]");
    if (np == 0) return VS_OK;
    VS_REQUIRE(cand_off[0] == 0, "vs_prune_plain: cand_off[0] must be 0");
    uint32_t longest = 0;
    for (uint32_t i = 0; i < np; ++i) {
        VS_REQUIRE(points[i] < ix->d.n, "vs_prune_plain: point %u out of range", points[i]);
        VS_REQUIRE(cand_off[i] <= cand_off[i + 1], "vs_prune_plain: cand_off must be non-decreasing");
        longest = std::max(longest, cand_off[i + 1] - cand_off[i]);
    }
    const uint32_t total = cand_off[np];
    VS_REQUIRE(total == 0 || cand_ids, "vs_prune_plain: cand_ids is NULL");
    for (uint32_t i = 0; i < total; ++i) VS_REQUIRE(cand_ids[i] < ix->d.n, "vs_prune_plain: candidate id %u out of range", cand_ids[i]);
    VS_REQUIRE(longest <= 4096, "vs_prune_plain: %u candidates for one point (at most 4096)", longest);
    const uint32_t R = ix->d.num_neighbors, cap = std::max<uint32_t>(next_pow2_u32(longest), 64);
    const size_t lds = prune_plain_lds_bytes(cap, R, pv.dim);
    VS_REQUIRE(lds <= 160 * 1024, "vs_prune_plain: %u candidates of %u dimensions do not fit LDS", longest, pv.dim);
    vs_ctx* ctx = ix->ctx;
    VS_HIP(hipSetDevice(ctx->device));
    VS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_prune_plain), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    DevScope sc(ctx->stream);
    uint32_t* d_buf = nullptr;  // points | cand_off | cand_ids | out_len | out_rows
    const size_t words = (size_t)np + (np + 1) + std::max<uint32_t>(total, 1) + np + (size_t)np * R;
    VS_TRY(sc.alloc(&d_buf, words * 4, "vs_prune_plain"));
    uint32_t *d_points = d_buf, *d_off = d_points + np, *d_ids = d_off + np + 1, *d_len = d_ids + std::max<uint32_t>(total, 1), *d_rows = d_len + np;
    VS_TRY(vs_dev_upload(ctx, d_points, points, (size_t)np * 4));
    VS_TRY(vs_dev_upload(ctx, d_off, cand_off, ((size_t)np + 1) * 4));
    if (total) VS_TRY(vs_dev_upload(ctx, d_ids, cand_ids, (size_t)total * 4));
    hipLaunchKernelGGL(k_prune_plain, dim3(np), dim3(WAVE), lds, ctx->stream, pv, R, (float)max_alpha, d_points, d_off, d_ids, np, cap, d_rows, d_len);
    VS_HIP(hipGetLastError());
    VS_TRY(vs_dev_download(ctx, out_len, d_len, (size_t)np * 4));
    return vs_dev_download(ctx, out_rows, d_rows, (size_t)np * R * 4);
}
extern "C" int vs_prune_plain(vs_index* ix, const uint32_t* points, const uint32_t* cand_off, const uint32_t* cand_ids, uint32_t np,
                              double max_alpha, uint32_t* out_rows, uint32_t* out_len) {
    return vs_guard("vs_prune_plain", [&] { return vs_prune_plain_impl(ix, points, cand_off, cand_ids, np, max_alpha, out_rows, out_len); });
}

// ---- vs_index_insert: aminsert (AM/build.rs:464-558) for rows that arrive after the index is resident -----------------------
// The anchoring rule over the new nodes r0 .. r0 + rn - 1 (k_insert_anchor to its fixed point), then, on the host and in node order
// (placement is rare), a slot for every node that stayed unanchored in the list of its closest old-or-anchored out-neighbor: a free
// one, else that of the list's last entry y — but only when y keeps another in-edge among the rows of y's own out-neighbors whose
// source is old or anchored and is not the row being edited.  The flags are recomputed from nothing after every sweep of placements,
// so that a node whose anchor was the evicted edge is seen.  *left = nodes still unanchored at the end (reported, never hidden).
static int anchor_range(BatchRunner& br, uint32_t r0, uint32_t rn, bool count_mates, uint32_t* mate_edges, uint32_t* placed,
                        uint32_t* left) {
    vs_index* ix = br.ix;
    BuildBufs& B = br.B;
    hipStream_t st = br.st;
    const uint32_t R = br.R, ns = ix->nbr_stride;
    uint32_t* d_changed = B.anch + rn;
    uint32_t* d_mates = B.anch + rn + 1;
    std::vector<uint32_t> anch(rn), rowx(R), rowy(R), rowz(R), roww(R);
    auto get_row = [&](uint32_t node, std::vector<uint32_t>& row) -> int {
        VS_HIP(hipMemcpy(row.data(), ix->nbrs + (size_t)node * ns, (size_t)R * 4, hipMemcpyDeviceToHost));
        return VS_OK;
    };
    *left = 0;
    for (int sweep = 0; sweep <= 8; ++sweep) {  // (the ninth pass only recomputes: *left is what the final graph shows)
        VS_HIP(hipMemsetAsync(B.anch, 0, ((size_t)rn + 2) * 4, st));
        br.tm.tick();
        for (uint32_t round = 0; round <= rn; ++round) {  // (a round that anchors nobody ends it; rn rounds is the longest chain)
            uint32_t changed = 0;
            VS_HIP(hipMemsetAsync(d_changed, 0, 4, st));
            hipLaunchKernelGGL(k_insert_anchor, dim3(rn), dim3(WAVE), 0, st, ix->nbrs, ns, R, r0, rn, B.anch, d_changed,
                               (count_mates && sweep == 0 && round == 0) ? d_mates : nullptr);
            VS_HIP(hipGetLastError());
            VS_HIP(hipMemcpyAsync(&changed, d_changed, 4, hipMemcpyDeviceToHost, st));
            VS_HIP(hipStreamSynchronize(st));
            if (!changed) break;
        }
        br.tm.tock(2);
        VS_HIP(hipMemcpy(anch.data(), B.anch, (size_t)rn * 4, hipMemcpyDeviceToHost));
        if (count_mates && sweep == 0) {
            uint32_t m = 0;
            VS_HIP(hipMemcpy(&m, d_mates, 4, hipMemcpyDeviceToHost));
            *mate_edges += m;
        }
        uint32_t un = 0;
        for (uint32_t v : anch) un += v == 0;
        *left = un;
        if (un == 0 || sweep == 8) return VS_OK;
        auto solid = [&](uint32_t v) { return v < r0 || (v - r0 < rn && anch[v - r0]); };  // old, or anchored
        uint32_t done = 0;
        for (uint32_t b = 0; b < rn; ++b) {
            if (anch[b]) continue;
            const uint32_t x = r0 + b;
            VS_TRY(get_row(x, rowx));
            bool ok = false;
            for (uint32_t t = 0; t < R && !ok && rowx[t] != VS_INVALID_NODE; ++t) {  // closest first
                const uint32_t y = rowx[t];
                if (!solid(y)) continue;
                VS_TRY(get_row(y, rowy));
                int slot = -1;
                bool named = false;
                for (uint32_t u = 0; u < R; ++u) {
                    named |= rowy[u] == x;
                    if (rowy[u] == VS_INVALID_NODE && slot < 0) slot = (int)u;
                }
                if (named) {  // (a placement earlier in this sweep made y solid: x is anchored already)
                    ok = true;
                    break;
                }
                if (slot < 0) {
                    const uint32_t z = rowy[R - 1];
                    VS_TRY(get_row(z, rowz));
                    bool kept = false;
                    for (uint32_t u = 0; u < R && !kept && rowz[u] != VS_INVALID_NODE; ++u) {
                        const uint32_t w = rowz[u];
                        if (w == y || !solid(w)) continue;
                        VS_TRY(get_row(w, roww));
                        for (uint32_t q = 0; q < R && !kept; ++q) kept = roww[q] == z;
                    }
                    if (kept) slot = (int)R - 1;
                }
                if (slot < 0) continue;
                rowy[slot] = x;
                VS_HIP(hipMemcpy(ix->nbrs + (size_t)y * ns, rowy.data(), (size_t)R * 4, hipMemcpyHostToDevice));
                ok = true;
                ++*placed;
                ++done;
            }
            if (ok) anch[b] = 1;
        }
        if (!done) return VS_OK;  // (nothing more can be placed: *left stands)
    }
    return VS_OK;
}

// the batches of one vs_index_insert call over the staged rows n_old .. n - 1, then the anchoring rule over all of them
static int insert_link_rows(vs_index* ix, DevScope& sc, BatchRunner& br, uint32_t L, double max_alpha, uint32_t batch_max, uint32_t n_old,
                            uint32_t n_new, bool new_label, vs_insert_stats& s) {
    const char* what = "vs_index_insert";
    const uint32_t n = n_old + n_new;
    const bool labeled = ix->label_off != nullptr;
    // (the buffers are sized by the batch: a one-row call must not allocate what a 65 536-row batch needs)
    if (batch_max == 0) batch_max = std::min<uint32_t>(65536, std::max<uint32_t>(1024, n / 64));
    batch_max = std::max(1u, std::min(std::min<uint32_t>(batch_max, 65536), n_new));
    VS_TRY(br.init(ix, sc, what, L, (float)max_alpha, batch_max, n));
    br.mates = std::min<uint32_t>(env_u32("VS_INSERT_MATES", 16), 64);
    const uint32_t bm = std::min(br.batch_max, n_new);
    if (br.mates) {
        VS_TRY(sc.alloc(&br.B.mate_ids, (size_t)bm * br.mates * 4, what));
        VS_TRY(sc.alloc(&br.B.mate_ham, (size_t)bm * br.mates * 4, what));
    }
    VS_TRY(sc.alloc(&br.B.anch, ((size_t)n_new + 2) * 4, what));
    // batches as in vs_build_graph: none is larger than the graph it searches (node 0 of an empty index has no one to link to)
    // For a label the call is the first to bring, the graph under that label's filter IS empty: the batches then double from one
    // row, as vs_build_graph's do, so that the label's carriers find the ones before them.
    uint32_t b0 = std::max(n_old, 1u), bsz = new_label ? 1u : br.batch_max;
    while (b0 < n) {
        const uint32_t bn = std::min(std::min(std::min(br.batch_max, bsz), b0), n - b0);
        if (bsz < br.batch_max) bsz = std::min(br.batch_max, bsz * 2);
        s.batches++;
        s.orphans_left = 0;
        if (labeled) VS_TRY(br.run(b0, bn, true, true));  // Graph::insert: first with the label filter (mates: the batch's rows it admits) ...
        VS_TRY(br.run(b0, bn, false, true));              // ... then from the default start node, the batch's mates among the candidates
        VS_TRY(anchor_range(br, b0, bn, true, &s.mate_edges, &s.orphans_placed, &s.orphans_left));
        b0 += bn;
    }
    // later batches re-prune rows that anchored the earlier ones: the rule once more over every row of the call, against the graph
    // as it was before the call
    // (node 0 of an index that was empty is the entry point itself)
    if (s.batches > 1) VS_TRY(anchor_range(br, std::max(n_old, 1u), n - std::max(n_old, 1u), false, &s.mate_edges, &s.orphans_placed, &s.orphans_left));
    return VS_OK;
}

static int index_insert_impl(vs_index* ix, const float* vectors, bool vectors_on_device, const uint64_t* heap_tids,
                             const uint32_t* label_off, const int16_t* label_val, uint32_t n_new, uint32_t L, double max_alpha,
                             uint32_t batch_max, vs_insert_stats* out) {
    const char* what = "vs_index_insert";
    VS_REQUIRE(ix, "%s: index is NULL", what);
    if (out) memset(out, 0, sizeof(*out));
    VS_REQUIRE_OWNER(ix, what);
    VS_REQUIRE_NO_VIEWS(ix, what);
    const bool plain = ix->d.storage_type == VS_STORAGE_PLAIN;
    VS_REQUIRE(ix->codes && ix->nbrs && ix->tids && ix->vecs, "%s: needs codes, neighbor lists, heap tids and the vector column on the device", what);
    if (plain) {  // no quantizer, no labels; linked with full-precision pair distances
        VS_REQUIRE(!label_off && !ix->label_off, "%s: Plain storage does not support label filters", what);
        PlainVecs pv;
        VS_TRY(plain_pair_args(ix, what, &pv));
        // an uploaded plain index mirrors a relation: the refusal predates vs_pages_out_open_plain, which can write the rows back now;
        // lifting it (and testing an insert into a staged relation) is follow-up work
        VS_REQUIRE(!ix->uploaded, "%s: an uploaded plain index does not take rows yet (vs_pages_out_open_plain writes plain storage back; "
                   "inserting into a staged relation is follow-up work); plain indexes allocated on the device (vs_index_alloc) take rows", what);
    }
    VS_REQUIRE(n_new == 0 || (vectors && heap_tids), "%s: vectors / heap_tids are NULL", what);
    VS_REQUIRE(L >= 1 && L <= 1000, "%s: search_list_size outside [1,1000]", what);
    VS_REQUIRE(max_alpha >= 1.0 && max_alpha <= 5.0, "%s: max_alpha outside [1,5]", what);
    const uint32_t n_old = ix->d.n;
    VS_REQUIRE((uint64_t)n_old + n_new < VS_INVALID_NODE, "%s: %u + %u nodes reach the end-of-list sentinel", what, n_old, n_new);
    const bool labeled = ix->label_off != nullptr;
    VS_REQUIRE(labeled == (label_off != nullptr), labeled ? "%s: the index is labeled, the rows carry no label sets" : "%s: label sets for an index without labels", what);
    if (labeled && n_new) {
        VS_TRY(validate_label_csr(what, label_off, label_val, n_new));
        VS_REQUIRE(ix->n_label_vals + label_off[n_new] < (1ull << 32), "%s: more than 2^32 label values", what);
    }
    if (!plain && ix->count == 0) {
        vs_set_error("%s: the quantizer is untrained (vs_sbq_train / vs_index_set_quantizer first; an insert never trains)", what);
        return VS_ERR_STATE;
    }
    // an insert may move every array an open writer (vs_pages_out_open / _open_plain) holds pointers into
    VS_TRY(require_no_batch(ix, what));
    VS_TRY(require_no_writer(ix, what, "its layout and array pointers were fixed at open"));
    VS_TRY(require_own_mask(ix, what, "grown"));
    if (n_new == 0) {
        if (out) out->first_node = n_old;
        return VS_OK;
    }
    vs_ctx* c = ix->ctx;
    hipStream_t st = c->stream;
    VS_HIP(hipSetDevice(c->device));
    const uint32_t n = n_old + n_new;
    uint32_t grew = 0;
    if (n > ix->capacity) {  // geometric growth, at least to fit
        const uint64_t want = std::max<uint64_t>(n, (uint64_t)ix->capacity + ix->capacity / 2);
        VS_TRY(vs_index_reserve_impl(ix, (uint32_t)std::min<uint64_t>(want, VS_INVALID_NODE - 1), what));
        grew = 1;
    }
    // the label CSR of the grown set (the only array that is not sized by rows): built aside, swapped in when everything else is staged
    DevScope sc(st);
    int16_t* new_val = nullptr;
    const uint64_t old_vals = ix->n_label_vals, add_vals = labeled ? label_off[n_new] : 0;
    if (labeled && add_vals) {
        VS_TRY(sc.alloc(&new_val, (old_vals + add_vals) * 2, what));
        if (old_vals) VS_HIP(hipMemcpyAsync(new_val, ix->label_val, old_vals * 2, hipMemcpyDeviceToDevice, st));
        VS_HIP(hipStreamSynchronize(st));
        VS_TRY(vs_dev_upload(c, new_val + old_vals, label_val, add_vals * 2));
    }
    // stage the rows: vectors (device rows are vec_stride floats, zero padded), heap tids, empty neighbor lists, visibility
    if (vectors_on_device) {
        VS_HIP(hipMemsetAsync(ix->vecs + (size_t)n_old * ix->vec_stride, 0, (size_t)n_new * ix->vec_stride * 4, st));
        VS_HIP(hipMemcpy2DAsync(ix->vecs + (size_t)n_old * ix->vec_stride, ix->vec_stride * 4ull, vectors, ix->d.dim_full * 4ull,
                                ix->d.dim_full * 4ull, n_new, hipMemcpyDeviceToDevice, st));
    } else {
        VS_TRY(vs_upload_rows(c, ix->vecs + (size_t)n_old * ix->vec_stride, ix->vec_stride * 4ull, vectors, ix->d.dim_full * 4ull,
                              ix->d.dim_full * 4ull, n_new));
    }
    VS_TRY(vs_dev_upload(c, ix->tids + n_old, heap_tids, (size_t)n_new * 8));
    VS_HIP(hipMemsetAsync(ix->nbrs + (size_t)n_old * ix->nbr_stride, 0xFF, (size_t)n_new * ix->nbr_stride * 4, st));
    // a new tuple is visible to the library's own mask and to no snapshot that was stored before it existed
    if (ix->visible_own) VS_HIP(hipMemsetAsync(ix->visible_own + n_old, 1, n_new, st));
    for (int sn = 1; sn < VS_MAX_SNAPSHOTS; ++sn)
        if (ix->snap[sn]) VS_HIP(hipMemsetAsync(ix->snap[sn] + n_old, 0, n_new, st));
    // norms and codes of the new rows only, with the quantizer as it stands (preprocess_cosine rule of vs_index_refresh_norms)
    VS_TRY(launch_row_norms_range(ix, n_old, n_new));
    if (plain) VS_TRY(launch_slice_norms_range(ix, n_old, n_new));  // (nothing touches codes: the rows past n stay zero)
    else VS_TRY(vs_quantize_row_range(ix, n_old, n_new));
    if (labeled) {
        std::vector<uint32_t> off(n_new);
        for (uint32_t i = 0; i < n_new; ++i) off[i] = (uint32_t)(old_vals + label_off[i + 1]);
        if (n_old == 0) {
            const uint32_t zero = 0;
            VS_HIP(hipMemcpy(ix->label_off, &zero, 4, hipMemcpyHostToDevice));
        }
        VS_TRY(vs_dev_upload(c, ix->label_off + n_old + 1, off.data(), (size_t)n_new * 4));
        if (new_val) {
            VS_HIP(hipStreamSynchronize(st));
            if (ix->label_val) (void)hipFree(ix->label_val);
            ix->label_val = sc.release(new_val);  // (the index's own from here on)
            ix->n_label_vals = old_vals + add_vals;
        }
    }
    ix->d.n = n;
    // what was derived from the old row count is stale: the label masks (re-derived now), the neighbor masks (dropped, re-derived
    // lazily at the new size), what the launch planner remembered of the last batches
    if (ix->nbr_mask) {
        VS_HIP(hipStreamSynchronize(st));
        (void)hipFree(ix->nbr_mask);
        ix->nbr_mask = nullptr;
    }
    ix->nbr_mask_valid = false;
    ix->nbr_mask_tried = false;
    ix->obs = ScanObs{};
    ix->last_fast = FastSig{};
    ix->last_ins_limit = 0;
    if (labeled) VS_TRY(vs_refresh_label_masks(ix));
    bool new_label = false;  // the call brings a label no older row carries
    // start nodes (update_start_nodes, AM/graph/mod.rs:490-531): an empty index gets node 0 as the default start; a label that an
    // inserted node is the first to carry gets that node
    {
        std::map<int16_t, uint32_t> starts;
        const uint32_t ns0 = ix->d.n_label_starts;
        if (ns0) {
            std::vector<int16_t> sl(ns0);
            std::vector<uint32_t> sn(ns0);
            VS_HIP(hipMemcpy(sl.data(), ix->ls_labels, (size_t)ns0 * 2, hipMemcpyDeviceToHost));
            VS_HIP(hipMemcpy(sn.data(), ix->ls_nodes, (size_t)ns0 * 4, hipMemcpyDeviceToHost));
            for (uint32_t i = 0; i < ns0; ++i) starts.emplace(sl[i], sn[i]);
        }
        bool changed = ix->d.default_start == VS_INVALID_NODE;
        const size_t labels_before = starts.size();
        if (labeled)
            for (uint32_t i = 0; i < n_new; ++i)
                for (uint32_t j = label_off[i]; j < label_off[i + 1]; ++j) changed |= starts.emplace(label_val[j], n_old + i).second;
        new_label = starts.size() != labels_before;
        if (changed) {
            std::vector<int16_t> sl;
            std::vector<uint32_t> sn;
            for (const auto& kv : starts) {
                sl.push_back(kv.first);
                sn.push_back(kv.second);
            }
            VS_TRY(vs_index_set_start_nodes(ix, ix->d.default_start == VS_INVALID_NODE ? 0u : ix->d.default_start, sl.data(), sn.data(),
                                            (uint32_t)sl.size()));
        }
    }
    vs_insert_stats s{};
    s.first_node = n_old;
    s.inserted = n_new;
    s.grew = grew;
    BatchRunner br;
    int r = insert_link_rows(ix, sc, br, L, max_alpha, batch_max, n_old, n_new, new_label, s);
    s.retries = br.retries;
    sc.close();
    if (r == VS_OK) r = vs_validate_graph(ix);
    for (int k = 0; k < 3; ++k) {
        ix->insert_ms[k] += br.ms[k];
        ix->build_ms[k] += br.ms[3 + k];
    }
    if (out) *out = s;
    return r;
}
extern "C" int vs_index_insert(vs_index* ix, const float* vectors, const uint64_t* heap_tids, const uint32_t* label_off,
                               const int16_t* label_val, uint32_t n_new, uint32_t search_list_size, double max_alpha, uint32_t batch_max,
                               vs_insert_stats* out) {
    return vs_guard("vs_index_insert", [&] {
        return index_insert_impl(ix, vectors, false, heap_tids, label_off, label_val, n_new, search_list_size, max_alpha, batch_max, out);
    });
}
extern "C" int vs_index_insert_dev(vs_index* ix, const float* d_vectors, const uint64_t* heap_tids, const uint32_t* label_off,
                                   const int16_t* label_val, uint32_t n_new, uint32_t search_list_size, double max_alpha,
                                   uint32_t batch_max, vs_insert_stats* out) {
    return vs_guard("vs_index_insert", [&] {
        return index_insert_impl(ix, d_vectors, true, heap_tids, label_off, label_val, n_new, search_list_size, max_alpha, batch_max, out);
    });
}
extern "C" int vs_index_insert_kernel_ms(vs_index* ix, double* ms /*[3]*/, int reset) {
    return read_kernel_ms("vs_index_insert_kernel_ms", ix, ix ? ix->insert_ms : nullptr, 3, ms, reset);
}

extern "C" int vs_index_build_kernel_ms(vs_index* ix, double* ms /*[3]*/, int reset) {
    return read_kernel_ms("vs_index_build_kernel_ms", ix, ix ? ix->build_ms : nullptr, 3, ms, reset);
}

// ---------------------------------------------------------------------------------------------------------------
// ambulkdelete by heap TID (AM/vacuum.rs:80-136): bulk_delete_for_storage walks the node pages and asks the callback about every
// live node's heap_item_pointer; here the dead TIDs are one sorted array and every node looks itself up.  One kernel over the TID
// column on the context's stream: a node whose offset is InvalidOffsetNumber already is skipped (is_deleted(), :112), a binary
// search in the dead set decides for the others, a hit clears the offset — what vs_index_mark_deleted writes.  The three counters
// of IndexBulkDeleteResult are ballots summed per wave and leave as one atomic per wave and counter.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bulk_delete(uint64_t* __restrict__ tids, uint32_t n, const uint64_t* __restrict__ dead, uint64_t n_dead,
                                                     unsigned long long* __restrict__ counters) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / WAVE, n_waves = (uint64_t)gridDim.x * (256 / WAVE);
    uint32_t removed = 0, stay = 0, already = 0;
    for (uint64_t i0 = wave * WAVE; i0 < n; i0 += n_waves * WAVE) {  // (wave-uniform trip count: the ballots below see every lane)
        const uint64_t i = i0 + lane;
        bool hit = false, live = false, gone = false;
        if (i < n) {
            const uint64_t t = tids[i];
            if ((t & 0xFFFFull) == 0) {
                gone = true;
            } else {
                uint64_t lo = 0, hi = n_dead;
                while (lo < hi) {
                    const uint64_t mid = lo + ((hi - lo) >> 1);
                    if (dead[mid] < t) lo = mid + 1;
                    else hi = mid;
                }
                hit = lo < n_dead && dead[lo] == t;
                live = !hit;
                if (hit) tids[i] = t & ~0xFFFFull;  // heap_item_pointer.offset = InvalidOffsetNumber
            }
        }
        removed += (uint32_t)__popcll(__ballot(hit));
        stay += (uint32_t)__popcll(__ballot(live));
        already += (uint32_t)__popcll(__ballot(gone));
    }
    if (lane == 0) {
        if (removed) atomicAdd(&counters[0], (unsigned long long)removed);
        if (stay) atomicAdd(&counters[1], (unsigned long long)stay);
        if (already) atomicAdd(&counters[2], (unsigned long long)already);
    }
}

static int bulk_delete_impl(vs_index* ix, const char* what, const uint64_t* dead, uint64_t n_dead, bool on_device, vs_bulk_delete_stats* out) {
    VS_REQUIRE(ix, "%s: index is NULL", what);
    if (out) memset(out, 0, sizeof(*out));
    VS_REQUIRE(n_dead == 0 || dead, "%s: dead_tids is NULL", what);
    VS_REQUIRE(n_dead <= 0x7FFFFFFFull, "%s: %llu dead tids in one call (at most 2^31 - 1)", what, (unsigned long long)n_dead);
    VS_REQUIRE(ix->tids || ix->d.n == 0, "%s: the index holds no heap tids", what);
    if (!on_device)
        for (uint64_t i = 0; i < n_dead; ++i)
            VS_REQUIRE((dead[i] & 0xFFFFull) != 0, "%s: dead_tids[%llu] has offset 0 (InvalidOffsetNumber)", what, (unsigned long long)i);
    VS_TRY(require_no_batch(ix, what));
    vs_ctx* c = ix->ctx;
    hipStream_t st = c->stream;
    VS_HIP(hipSetDevice(c->device));
    DevScope sc(st);
    uint64_t *d_in = nullptr, *d_sorted = nullptr;
    uint8_t* d_pay = nullptr;
    void* d_tmp = nullptr;
    unsigned long long* d_cnt = nullptr;
    unsigned long long h_cnt[3] = {0, 0, 0};
    const uint64_t* d_dead = dead;
    if (!on_device && n_dead) {
        // staged through the pinned ring, sorted on the device (the radix sort the build already uses: pairs, here with one byte
        // of payload nobody reads); duplicates stay, a binary search does not mind them
        VS_TRY(sc.alloc(&d_in, n_dead * 8, what));
        VS_TRY(sc.alloc(&d_sorted, n_dead * 8, what));
        VS_TRY(sc.alloc(&d_pay, n_dead * 2, what));
        VS_HIP(hipMemsetAsync(d_pay, 0, n_dead * 2, st));
        VS_TRY(vs_dev_upload(c, d_in, dead, n_dead * 8));
        size_t tmp_bytes = 0;
        VS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (const uint64_t*)d_in, d_sorted, (const uint8_t*)d_pay, d_pay + n_dead,
                                                  (int)n_dead, 0, 64, st));
        VS_TRY(sc.alloc(&d_tmp, tmp_bytes + 16, what));
        VS_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp_bytes, (const uint64_t*)d_in, d_sorted, (const uint8_t*)d_pay, d_pay + n_dead,
                                                  (int)n_dead, 0, 64, st));
        d_dead = d_sorted;
    }
    VS_TRY(sc.alloc(&d_cnt, sizeof h_cnt, what));
    VS_HIP(hipMemsetAsync(d_cnt, 0, sizeof h_cnt, st));
    if (ix->d.n) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)ix->d.n + 255) / 256, 8192);
        hipLaunchKernelGGL(k_bulk_delete, dim3(grid), dim3(256), 0, st, ix->tids, ix->d.n, d_dead, n_dead, d_cnt);
        VS_HIP(hipGetLastError());
    }
    VS_HIP(hipMemcpyAsync(h_cnt, d_cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st));
    VS_HIP(hipStreamSynchronize(st));  // (the only wait: the three counters)
    sc.drained();
    if (out) {
        out->tuples_removed = h_cnt[0];
        out->num_index_tuples = h_cnt[1];
        out->already_deleted = h_cnt[2];
    }
    return VS_OK;
}
extern "C" int vs_index_bulk_delete(vs_index* ix, const uint64_t* dead_tids, uint64_t n_dead, vs_bulk_delete_stats* out) {
    return vs_guard("vs_index_bulk_delete", [&] { return bulk_delete_impl(ix, "vs_index_bulk_delete", dead_tids, n_dead, false, out); });
}
extern "C" int vs_index_bulk_delete_dev(vs_index* ix, const uint64_t* d_dead_tids_sorted, uint64_t n_dead, vs_bulk_delete_stats* out) {
    return vs_guard("vs_index_bulk_delete_dev", [&] { return bulk_delete_impl(ix, "vs_index_bulk_delete_dev", d_dead_tids_sorted, n_dead, true, out); });
}

// ---------------------------------------------------------------------------------------------------------------
// vs_index_consolidate_deletes: the consolidation pass of streaming DiskANN over the tombstones ambulkdelete leaves behind
// (DESIGN.md section 6d has the rule).  K = the nodes that stay in the graph (live, or a start node), D = the other tombstones.
// Every row of K that names a node of D is rewritten from { its entries in K } + { the entries in K of the rows of its D
// entries }, one level deep, sorted by (Hamming to the row's node, id), cut to cand_max and pruned like any other candidate
// list.  Rows of D are never written and rows of K read only their own list and lists of D nodes: the pass runs in place.
// vs_index_consolidate_deletes_plain: the same pass over a `plain` index, "Hamming" read as the PlainPair distance d(p -> w) —
// sorted by (plain_key(d), id), pruned with wave_prune<PlainPair>; no labels.  One implementation (consolidate_impl), two entries.
// ---------------------------------------------------------------------------------------------------------------
enum { CN_TOMB = 0, CN_KEPT, CN_EDGES_DROPPED, CN_EDGES_ADDED, CN_PRUNED, CN_CAPPED, CN_EMPTIED, CN_WIDE_LABELS, CN_N = 8 };

// node classes from the tid column: 0 live, 1 tombstone (k_cons_keep_starts turns the start nodes among them into 2)
__global__ __launch_bounds__(256) void k_cons_classify(const uint64_t* __restrict__ tids, const uint32_t* __restrict__ label_off, uint32_t n,
                                                       uint8_t* __restrict__ cls, unsigned long long* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    bool dead = false, wide = false;
    if (i < n) {
        dead = (tids[i] & 0xFFFFull) == 0;
        cls[i] = dead ? 1 : 0;
        if (label_off) wide = label_off[i + 1] - label_off[i] > 64;  // (label_pmask holds a point's labels in one 64-bit mask)
    }
    const uint64_t md = __ballot(dead), mw = __ballot(wide);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        if (md) atomicAdd(&cnt[CN_TOMB], (unsigned long long)__popcll(md));
        if (mw) atomicAdd(&cnt[CN_WIDE_LABELS], (unsigned long long)__popcll(mw));
    }
}
// starts: the default start node and the per-label start nodes, every node once (the host de-duplicates)
__global__ void k_cons_keep_starts(const uint32_t* __restrict__ starts, uint32_t ns, uint8_t* __restrict__ cls,
                                   unsigned long long* __restrict__ cnt) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ns) return;
    const uint32_t s = starts[t];
    if (cls[s] == 1) {
        cls[s] = 2;
        atomicAdd(&cnt[CN_KEPT], 1ull);
    }
}
// the flag pass over the n x R neighbor cells: a kept row that names a dropped tombstone is work; the cells that do are edges_dropped
__global__ __launch_bounds__(256) void k_cons_flag(const uint32_t* __restrict__ nbrs, uint32_t nbr_stride, uint32_t R, uint32_t n,
                                                   const uint8_t* __restrict__ cls, uint8_t* __restrict__ flag,
                                                   unsigned long long* __restrict__ cnt) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool hit = false;
    if (i < (size_t)n * R) {
        const size_t row = i / R;
        if (cls[row] != 1) {
            const uint32_t v = nbrs[row * nbr_stride + (i % R)];
            hit = v < n && cls[v] == 1;
            if (hit) flag[row] = 1;
        }
    }
    const uint64_t m = __ballot(hit);
    if ((threadIdx.x & (WAVE - 1)) == 0 && m) atomicAdd(&cnt[CN_EDGES_DROPPED], (unsigned long long)__popcll(m));
}
// The flagged rows as an ascending work list — flagged rows per wave of 64 rows (ballot), one exclusive scan over the waves' counts,
// then every flagged row writes itself at its wave's offset + its rank among the wave's flagged lanes (the three passes
// vs_pages_out_delta compacts its dirty pages with): the order is the rows' own, not that of an atomic slot counter.
__global__ __launch_bounds__(256) void k_cons_work_count(const uint8_t* __restrict__ flag, uint32_t n, uint32_t* __restrict__ wave_cnt) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint64_t m = __ballot(i < n && flag[i] != 0);
    if ((threadIdx.x & (WAVE - 1)) == 0 && i < n) wave_cnt[i / WAVE] = (uint32_t)__popcll(m);
}
// one workgroup: v[0 .. m) becomes its exclusive prefix sums, v[m] the total
__global__ __launch_bounds__(256) void k_cons_work_scan(uint32_t* __restrict__ v, uint32_t m) {
    __shared__ uint32_t part[256];
    const uint32_t per = (m + 255) / 256, lo = min(threadIdx.x * per, m), hi = min(lo + per, m);
    uint32_t s = 0;
    for (uint32_t i = lo; i < hi; ++i) s += v[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t t = 0; t < 256; ++t) {
            const uint32_t c = part[t];
            part[t] = run;
            run += c;
        }
        v[m] = run;
    }
    __syncthreads();
    uint32_t run = part[threadIdx.x];
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t c = v[i];
        v[i] = run;
        run += c;
    }
}
__global__ __launch_bounds__(256) void k_cons_work_scatter(const uint8_t* __restrict__ flag, uint32_t n, const uint32_t* __restrict__ wave_off,
                                                           uint32_t* __restrict__ work) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & (WAVE - 1);
    const bool f = i < n && flag[i] != 0;
    const uint64_t m = __ballot(f);
    if (f) work[wave_off[i / WAVE] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
}

// LDS of k_consolidate_rows (bytes): two key lists of cap entries (the merge writes one from the other), the keys of the rows being
// gathered, the arrays wave_prune works on, and the code rows — of the <= R rows in flight while merging, of the surviving
// candidates while pruning (the same area; cap > R).  The plain form has no code rows and no label masks: the area behind gid[]
// holds one prepared vector of round_up(dim_index, 4) floats (cons_lds_plain).
struct ConsLds {
    uint32_t cap4, R4, code_rows;
    size_t bytes;
};
static ConsLds cons_lds(uint32_t cap, uint32_t R, uint32_t stride, bool labeled, bool lds_codes, bool stage_rows) {
    ConsLds l;
    l.cap4 = round_up_u32(cap, 4);
    l.R4 = round_up_u32(R, 4);
    l.code_rows = lds_codes ? l.cap4 : (stage_rows ? l.R4 : 0);
    l.bytes = (size_t)l.cap4 * (16 + (labeled ? 8 : 0) + 12) + (size_t)l.R4 * (8 + 16) + (size_t)l.code_rows * stride * 8;
    return l;
}
static ConsLds cons_lds_plain(uint32_t cap, uint32_t R, uint32_t dim) {
    ConsLds l = cons_lds(cap, R, 0, false, false, false);
    l.bytes += (size_t)round_up_u32(dim, 4) * 4;
    return l;
}

// one wave per work-list entry p
// PLAIN: keys are (plain_key(d(p -> w)) << 32) | w with the PlainPair distance — p's prepared index slice is the staged query side
// of every merge of the work item, eight lanes score one gathered row straight from global memory (a gathered row is read once
// per merge, so there is no stage_rows / use_lds_codes choice) — and the prune is wave_prune<PlainPair>.  That prune overwrites
// the staged vector with each candidate it selects: every key of a work item is finished before it, and p is staged again at the
// top of every iteration of the grid-stride loop.
template <bool PLAIN>
__global__ __launch_bounds__(WAVE) void k_consolidate_rows(const uint64_t* __restrict__ codes, uint32_t stride, uint32_t* nbrs,
                                                           uint32_t nbr_stride, uint32_t R, uint32_t n, float max_alpha, uint32_t cap,
                                                           const uint32_t* __restrict__ work, uint32_t nwork,
                                                           const uint8_t* __restrict__ cls, uint32_t use_lds_codes, uint32_t stage_rows,
                                                           const uint32_t* __restrict__ label_off, const int16_t* __restrict__ label_val,
                                                           unsigned long long* __restrict__ cnt, PlainVecs pv) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t cap4 = round_up_u32(cap, 4), R4 = round_up_u32(R, 4);
    uint64_t* ka = reinterpret_cast<uint64_t*>(smem);  // [cap4] sorted keys (distance << 32) | id ...
    uint64_t* kb = ka + cap4;                           // [cap4] ... and the list the next merge writes
    uint64_t* inc = kb + cap4;                          // [R4] keys of the rows being merged in
    uint64_t* pm = inc + R4;                            // [cap4] label masks relative to p (labeled sets only)
    uint32_t* cid = reinterpret_cast<uint32_t*>(pm + (label_off ? cap4 : 0));
    uint32_t* cd = cid + cap4;
    float* maxf = reinterpret_cast<float*>(cd + cap4);
    uint32_t* sel = reinterpret_cast<uint32_t*>(maxf + cap4);  // [R4] (while merging: the duplicate marks of inc[])
    uint32_t* oldrow = sel + R4;                                // [R4] p's list as it was
    uint32_t* tomb = oldrow + R4;                               // [R4] its entries in D
    uint32_t* gid = tomb + R4;                                  // [R4] ids of the rows being gathered
    uint64_t* ccode = reinterpret_cast<uint64_t*>(gid + R4);    // (PLAIN: the prepared vector qv[round_up(dim, 4)])
    PlainPair ppd{pv.vecs, pv.vdiv, cid, reinterpret_cast<float*>(ccode), pv.vec_stride, pv.dim, pv.distance_type};
    for (uint32_t wi = blockIdx.x; wi < nwork; wi += gridDim.x) {
        const uint32_t p = work[wi];
        uint32_t* row = nbrs + (size_t)p * nbr_stride;
        if constexpr (PLAIN) ppd.stage(p, lane);  // (the prune of the work item before left its last selected candidate there)
        const uint64_t* cp = codes + (size_t)p * stride;
        ulonglong2 pc[12];  // p's code (768 x 2 bit / 1536 x 1 bit): every distance of this row is taken against it
        if (!PLAIN && stride == 24) {
#pragma unroll
            for (int t = 0; t < 12; ++t) pc[t] = *reinterpret_cast<const ulonglong2*>(cp + 2 * t);
        }
        [[maybe_unused]] auto dist_to_p = [&](const uint64_t* c) -> uint32_t {  // (the SBQ form's distance)
            if (stride != 24) return ham_words(c, cp, stride);
            ulonglong2 x[12];
#pragma unroll
            for (int t = 0; t < 12; ++t) x[t] = *reinterpret_cast<const ulonglong2*>(c + 2 * t);
            uint32_t acc = 0;
#pragma unroll
            for (int t = 0; t < 12; ++t) acc += (uint32_t)__popcll(x[t].x ^ pc[t].x) + (uint32_t)__popcll(x[t].y ^ pc[t].y);
            return acc;
        };
        uint64_t* cur = ka;
        uint64_t* nxt = kb;
        uint32_t T = 0;
        bool capped = false;
        // gid[0 .. ng) -> keys, each new id once, merged into the sorted list cur[0 .. T), the closest `cap` kept
        auto merge_gathered = [&](uint32_t ng) {
            if (ng == 0) return;  // (uniform)
            if constexpr (PLAIN) {
                for (uint32_t t0 = 0; t0 < ng; t0 += WAVE / 8) {  // (uniform trip count: dist() is a call of the whole wave)
                    const uint32_t t = t0 + (uint32_t)lane / 8;
                    const bool act = t < ng;
                    const uint32_t id = act ? gid[t] : 0u;
                    const float d = ppd.dist(id, act, lane);
                    if (act && (lane & 7) == 0) inc[t] = ((uint64_t)plain_key(d) << 32) | id;
                }
            } else {
                if (stage_rows) {  // the rows' codes in flight together, not one latency per candidate
                    stage_codes(ccode, codes, gid, ng, stride, lane);
                    __syncthreads();
                }
                for (uint32_t t = lane; t < ng; t += WAVE) {
                    const uint32_t id = gid[t];
                    inc[t] = ((uint64_t)dist_to_p(stage_rows ? ccode + (size_t)t * stride : codes + (size_t)id * stride) << 32) | id;
                }
            }
            __syncthreads();
            for (uint32_t t = lane; t < ng; t += WAVE) {  // an equal key is a duplicate (the distance is a function of the id)
                const uint64_t k = inc[t];
                uint32_t lo = 0, hi = T;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (cur[mid] < k) lo = mid + 1;
                    else hi = mid;
                }
                bool dup = lo < T && cur[lo] == k;
                for (uint32_t u = 0; u < t && !dup; ++u) dup = inc[u] == k;
                sel[t] = dup ? 1u : 0u;
            }
            __syncthreads();
            uint32_t m = 0;
            for (uint32_t t0 = 0; t0 < ng; t0 += WAVE) {
                const uint32_t t = t0 + lane;
                const bool ok = t < ng && sel[t] == 0;
                if (t < ng && !ok) inc[t] = ~0ull;
                m += (uint32_t)__popcll(__ballot(ok));
            }
            __syncthreads();
            if (m == 0) return;  // (uniform)
            for (uint32_t i = lane; i < T; i += WAVE) {  // every entry's place in the merged order
                const uint64_t a = cur[i];
                uint32_t before = 0;
                for (uint32_t u = 0; u < ng; ++u) before += inc[u] < a;
                if (i + before < cap) nxt[i + before] = a;
            }
            for (uint32_t t = lane; t < ng; t += WAVE) {
                const uint64_t k = inc[t];
                if (k == ~0ull) continue;
                uint32_t lo = 0, hi = T;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (cur[mid] < k) lo = mid + 1;
                    else hi = mid;
                }
                uint32_t before = 0;
                for (uint32_t u = 0; u < ng; ++u) before += inc[u] < k;
                if (lo + before < cap) nxt[lo + before] = k;
            }
            __syncthreads();
            capped |= T + m > cap;
            T = min(T + m, cap);
            uint64_t* sw = cur;
            cur = nxt;
            nxt = sw;
        };
        // p's own list: the entries in K are the first candidates, the entries in D the rows to take over
        uint32_t nt = 0, ng = 0;
        for (uint32_t c0 = 0; c0 < R; c0 += WAVE) {
            const uint32_t t = c0 + lane;
            const uint32_t v = t < R ? row[t] : VS_INVALID_NODE;
            if (t < R) oldrow[t] = v;
            const bool isd = v < n && cls[v] == 1;
            const bool keep = v < n && !isd && v != p;
            const uint64_t dm = __ballot(isd), km = __ballot(keep);
            if (isd) tomb[nt + (uint32_t)__popcll(dm & below)] = v;
            if (keep) gid[ng + (uint32_t)__popcll(km & below)] = v;
            nt += (uint32_t)__popcll(dm);
            ng += (uint32_t)__popcll(km);
        }
        __syncthreads();
        merge_gathered(ng);
        for (uint32_t ti = 0; ti < nt; ++ti) {  // one level only: a tombstone's tombstone neighbors are not followed
            const uint32_t* drow = nbrs + (size_t)tomb[ti] * nbr_stride;
            ng = 0;
            for (uint32_t c0 = 0; c0 < R; c0 += WAVE) {
                const uint32_t t = c0 + lane;
                const uint32_t w = t < R ? drow[t] : VS_INVALID_NODE;
                const bool keep = w < n && cls[w] != 1 && w != p;
                const uint64_t km = __ballot(keep);
                if (keep) gid[ng + (uint32_t)__popcll(km & below)] = w;
                ng += (uint32_t)__popcll(km);
            }
            __syncthreads();
            merge_gathered(ng);
        }
        for (uint32_t t = lane; t < T; t += WAVE) {
            const uint64_t k = cur[t];
            cid[t] = (uint32_t)k;
            cd[t] = (uint32_t)(k >> 32);
            if (label_off) pm[t] = label_pmask(label_off, label_val, p, (uint32_t)k);  // as k_build_backedges: relative to the row's node
        }
        __syncthreads();
        uint32_t nres;
        if (T <= R) {  // Graph::add_neighbors prunes only a candidate list longer than num_neighbors (AM/graph/mod.rs:243-256)
            for (uint32_t t = lane; t < T; t += WAVE) sel[t] = t;
            nres = T;
            __syncthreads();
        } else if constexpr (PLAIN) {
            nres = wave_prune(ppd, cd, T, R, max_alpha, maxf, sel, lane);
        } else {
            if (use_lds_codes) {
                stage_codes(ccode, codes, cid, T, stride, lane);
                __syncthreads();
            }
            nres = wave_prune_ham(cid, cd, T, use_lds_codes ? ccode : nullptr, codes, stride, R, max_alpha, maxf, sel, lane,
                              label_off ? pm : nullptr);
        }
        uint32_t added = 0;  // entries of the new list the old one did not hold
        for (uint32_t t0 = 0; t0 < nres; t0 += WAVE) {
            const uint32_t t = t0 + lane;
            bool fresh = t < nres;
            if (fresh) {
                const uint32_t id = cid[sel[t]];
                for (uint32_t u = 0; u < R && fresh; ++u) fresh = oldrow[u] != id;
            }
            added += (uint32_t)__popcll(__ballot(fresh));
        }
        for (uint32_t t = lane; t < nbr_stride; t += WAVE) row[t] = t < nres ? cid[sel[t]] : VS_INVALID_NODE;
        if (lane == 0) {
            if (added) atomicAdd(&cnt[CN_EDGES_ADDED], (unsigned long long)added);
            if (T > R) atomicAdd(&cnt[CN_PRUNED], 1ull);
            if (capped) atomicAdd(&cnt[CN_CAPPED], 1ull);
            if (nres == 0) atomicAdd(&cnt[CN_EMPTIED], 1ull);
        }
        __syncthreads();
    }
}

// plain: the call is vs_index_consolidate_deletes_plain — a plain storage index, keys and prune by the PlainPair distance
static int consolidate_impl(vs_index* ix, double max_alpha, uint32_t cand_max, uint32_t flags, vs_consolidate_stats* out, bool plain) {
    const char* what = plain ? "vs_index_consolidate_deletes_plain" : "vs_index_consolidate_deletes";
    VS_REQUIRE(ix, "%s: index is NULL", what);
    if (out) memset(out, 0, sizeof(*out));
    VS_REQUIRE_OWNER(ix, what);
    VS_REQUIRE_NO_VIEWS(ix, what);
    PlainVecs pv{nullptr, nullptr, 0, 0, 0};
    if (plain) {
        VS_REQUIRE(ix->d.storage_type == VS_STORAGE_PLAIN,
                   "%s: plain storage indexes only (vs_index_consolidate_deletes is the call for a memory_optimized index)", what);
        VS_TRY(plain_pair_args(ix, what, &pv));
        VS_REQUIRE(ix->nbrs && ix->tids, "%s: needs neighbor lists and heap tids on the device", what);
    } else {
        VS_REQUIRE(ix->d.storage_type == VS_STORAGE_SBQ,
                   "%s: plain storage is not supported (memory_optimized indexes only; vs_index_consolidate_deletes_plain is the call for it)", what);
        VS_REQUIRE(ix->codes && ix->nbrs && ix->tids, "%s: needs codes, neighbor lists and heap tids on the device", what);
    }
    VS_REQUIRE(max_alpha >= 1.0 && max_alpha <= 5.0, "%s: max_alpha outside [1,5]", what);
    VS_REQUIRE((flags & ~(uint32_t)VS_CONSOLIDATE_NO_REPAIR) == 0, "%s: unknown flags 0x%x", what, flags);
    const uint32_t n = ix->d.n, R = ix->d.num_neighbors, stride = ix->code_stride;
    if (cand_max == 0) cand_max = std::min<uint32_t>(4 * R, 256);
    VS_REQUIRE(cand_max > R && cand_max <= 1024, "%s: cand_max %u outside (num_neighbors = %u, 1024]", what, cand_max, R);
    VS_TRY(require_no_batch(ix, what));
    VS_TRY(require_no_writer(ix, what, WRITER_ROWS_MIX));
    vs_consolidate_stats s{};
    s.unreachable_live = (flags & VS_CONSOLIDATE_NO_REPAIR) ? 0xFFFFFFFFu : 0u;
    if (n == 0 || ix->d.default_start == VS_INVALID_NODE) {
        if (out) *out = s;
        return VS_OK;
    }
    vs_ctx* c = ix->ctx;
    hipStream_t st = c->stream;
    VS_HIP(hipSetDevice(c->device));
    // K keeps the default start node and every per-label start node whatever their state: scans begin there
    std::vector<uint32_t> starts;
    VS_TRY(collect_start_nodes(ix, what, &starts));
    const bool labeled = ix->label_off != nullptr;
    // the candidate codes sit in LDS while a row is pruned when they fit; failing that, at least the <= R rows a merge gathers
    bool lds_codes = !plain && cons_lds(cand_max, R, stride, labeled, true, true).bytes <= 150 * 1024;
    bool stage_rows = !plain && (lds_codes || cons_lds(cand_max, R, stride, labeled, false, true).bytes <= 150 * 1024);
    const ConsLds lds = plain ? cons_lds_plain(cand_max, R, pv.dim) : cons_lds(cand_max, R, stride, labeled, lds_codes, stage_rows);
    VS_REQUIRE(lds.bytes <= 160 * 1024, "%s: num_neighbors %u / cand_max %u need %zu bytes of LDS", what, R, cand_max, lds.bytes);
    const uint32_t n_waves = (n + WAVE - 1) / WAVE;
    unsigned long long h_cnt[CN_N] = {0};
    uint32_t nwork = 0;
    auto run = [&]() -> int {  // (the stats are filled from what it got to, whatever it returns)
        DevScope sc(st);
        StageTimer tm;
        VS_TRY(tm.start(sc, c->profiling, ix->consolidate_ms, what));
        uint8_t *d_cls = nullptr, *d_flag = nullptr;
        uint32_t *d_wave = nullptr, *d_work = nullptr, *d_starts = nullptr;
        unsigned long long* d_cnt = nullptr;
        VS_TRY(sc.alloc(&d_cls, (size_t)n, what));
        VS_TRY(sc.alloc(&d_flag, (size_t)n, what));
        VS_TRY(sc.alloc(&d_wave, ((size_t)n_waves + 1) * 4, what));
        VS_TRY(sc.alloc(&d_starts, starts.size() * 4, what));
        VS_TRY(sc.alloc(&d_cnt, sizeof h_cnt, what));
        VS_HIP(hipMemcpyAsync(d_starts, starts.data(), starts.size() * 4, hipMemcpyHostToDevice, st));
        VS_HIP(hipMemsetAsync(d_cnt, 0, sizeof h_cnt, st));
        VS_HIP(hipMemsetAsync(d_flag, 0, (size_t)n, st));
        if (plain) {  // the divisors the pair distance divides by, from the rows as they stand (as vs_build_graph derives them)
            VS_TRY(launch_row_norms(ix));
            VS_TRY(launch_slice_norms_range(ix, 0, n));
        }
        tm.tick();
        const dim3 ngrid((n + 255) / 256);
        hipLaunchKernelGGL(k_cons_classify, ngrid, dim3(256), 0, st, (const uint64_t*)ix->tids, (const uint32_t*)ix->label_off, n, d_cls, d_cnt);
        VS_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_cons_keep_starts, dim3(((uint32_t)starts.size() + 255) / 256), dim3(256), 0, st, (const uint32_t*)d_starts,
                           (uint32_t)starts.size(), d_cls, d_cnt);
        VS_HIP(hipGetLastError());
        const size_t cells = (size_t)n * R;
        hipLaunchKernelGGL(k_cons_flag, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, (const uint32_t*)ix->nbrs, ix->nbr_stride, R, n,
                           (const uint8_t*)d_cls, d_flag, d_cnt);
        VS_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_cons_work_count, ngrid, dim3(256), 0, st, (const uint8_t*)d_flag, n, d_wave);
        VS_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_cons_work_scan, dim3(1), dim3(256), 0, st, d_wave, n_waves);
        VS_HIP(hipGetLastError());
        VS_HIP(hipMemcpyAsync(&nwork, d_wave + n_waves, 4, hipMemcpyDeviceToHost, st));
        VS_HIP(hipMemcpyAsync(h_cnt, d_cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st));
        VS_HIP(hipStreamSynchronize(st));
        VS_REQUIRE(h_cnt[CN_WIDE_LABELS] == 0, "%s: %llu node(s) carry more than 64 labels", what, h_cnt[CN_WIDE_LABELS]);
        if (nwork) {
            VS_TRY(sc.alloc(&d_work, (size_t)nwork * 4, what));
            hipLaunchKernelGGL(k_cons_work_scatter, ngrid, dim3(256), 0, st, (const uint8_t*)d_flag, n, (const uint32_t*)d_wave, d_work);
            VS_HIP(hipGetLastError());
        }
        tm.tock(0);
        if (nwork) {
            const void* kern = plain ? reinterpret_cast<const void*>(k_consolidate_rows<true>) : reinterpret_cast<const void*>(k_consolidate_rows<false>);
            VS_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            ix->nbr_mask_valid = false;  // (the neighbor lists are about to change: what was derived from them is stale)
            tm.tick();
            const dim3 rgrid(std::min<uint32_t>(nwork, 1u << 20));
            if (plain)
                hipLaunchKernelGGL(k_consolidate_rows<true>, rgrid, dim3(WAVE), lds.bytes, st, (const uint64_t*)nullptr, 0u, ix->nbrs, ix->nbr_stride,
                                   R, n, (float)max_alpha, cand_max, (const uint32_t*)d_work, nwork, (const uint8_t*)d_cls, 0u, 0u,
                                   (const uint32_t*)nullptr, (const int16_t*)nullptr, d_cnt, pv);
            else
                hipLaunchKernelGGL(k_consolidate_rows<false>, rgrid, dim3(WAVE), lds.bytes, st, (const uint64_t*)ix->codes, stride, ix->nbrs,
                                   ix->nbr_stride, R, n, (float)max_alpha, cand_max, (const uint32_t*)d_work, nwork, (const uint8_t*)d_cls,
                                   lds_codes ? 1u : 0u, stage_rows ? 1u : 0u, (const uint32_t*)ix->label_off, (const int16_t*)ix->label_val,
                                   d_cnt, pv);
            VS_HIP(hipGetLastError());
            tm.tock(1);
            VS_HIP(hipMemcpyAsync(h_cnt, d_cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st));
            VS_HIP(hipStreamSynchronize(st));
        }
        if (!(flags & VS_CONSOLIDATE_NO_REPAIR)) {
            std::vector<uint8_t> cls(n);
            VS_HIP(hipMemcpy(cls.data(), d_cls, n, hipMemcpyDeviceToHost));
            ix->nbr_mask_valid = false;
            ix->build_unreachable = 0;
            VS_TRY(repair_graph(ix, sc, cls.data()));
            s.unreachable_live = ix->build_unreachable;
        }
        return VS_OK;
    };
    int rc = run();
    s.tombstones = h_cnt[CN_TOMB];
    s.tombstones_kept = h_cnt[CN_KEPT];
    s.rows_rewritten = nwork;
    s.edges_dropped = h_cnt[CN_EDGES_DROPPED];
    s.edges_added = h_cnt[CN_EDGES_ADDED];
    s.rows_pruned = h_cnt[CN_PRUNED];
    s.rows_capped = h_cnt[CN_CAPPED];
    s.rows_emptied = h_cnt[CN_EMPTIED];
    if (out) *out = s;
    if (rc == VS_OK) rc = vs_validate_graph(ix);
    return rc;
}
extern "C" int vs_index_consolidate_deletes(vs_index* ix, double max_alpha, uint32_t cand_max, uint32_t flags, vs_consolidate_stats* out) {
    return vs_guard("vs_index_consolidate_deletes", [&] { return consolidate_impl(ix, max_alpha, cand_max, flags, out, false); });
}
extern "C" int vs_index_consolidate_deletes_plain(vs_index* ix, double max_alpha, uint32_t cand_max, uint32_t flags,
                                                  vs_consolidate_stats* out) {
    return vs_guard("vs_index_consolidate_deletes_plain", [&] { return consolidate_impl(ix, max_alpha, cand_max, flags, out, true); });
}
extern "C" int vs_index_consolidate_kernel_ms(vs_index* ix, double* ms /*[2]*/, int reset) {
    return read_kernel_ms("vs_index_consolidate_kernel_ms", ix, ix ? ix->consolidate_ms : nullptr, 2, ms, reset);
}

// ---------------------------------------------------------------------------------------------------------------
// vs_index_compact: the tombstones consolidation left behind leave the arrays (DESIGN.md section 6e has the rule).  K is the K of
// the consolidation (k_cons_classify + k_cons_keep_starts), new_of[i] = the number of K nodes below i, and every per-node column
// keeps exactly the rows of K in their order.  Rows move INSIDE their arrays, chunk by chunk through a bounded staging buffer:
// for the kept rows with new ids [a, b) one launch gathers their source rows (old ids old_of[a .. b)) into staging, a device copy
// puts staging at [a, b).  A destination slot j in [a, b) is the source only of a kept row with new id <= j (old_of[j'] >= j' and
// old_of ascends): that row went with an earlier chunk or is in staging already.  The neighbor form renames while it gathers.
// ---------------------------------------------------------------------------------------------------------------
// extra counters of the pass, behind those of the classification (CN_*): kept nodes, the first dropped node, label values kept
enum { CP_N_AFTER = CN_N, CP_FIRST, CP_LABEL_VALS, CP_N };

// kept nodes (class != 1) per wave of 64 nodes, and the lowest dropped node (one atomic per wave that has one)
__global__ __launch_bounds__(256) void k_compact_keep_count(const uint8_t* __restrict__ cls, uint32_t n, uint32_t* __restrict__ wave_cnt,
                                                            unsigned long long* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n, keep = in && cls[i] != 1;
    const uint64_t mk = __ballot(keep), md = __ballot(in && !keep);
    if ((threadIdx.x & (WAVE - 1)) == 0 && in) {
        wave_cnt[i / WAVE] = (uint32_t)__popcll(mk);
        if (md) atomicMin(&cnt[CP_FIRST], (unsigned long long)(i + (uint32_t)__builtin_ctzll(md)));
    }
}
// wave_off: the exclusive scan of the counts (k_cons_work_scan).  new_of[old] for every node, old_of[new] for every kept one.
__global__ __launch_bounds__(256) void k_compact_maps(const uint8_t* __restrict__ cls, uint32_t n, const uint32_t* __restrict__ wave_off,
                                                      uint32_t* __restrict__ new_of, uint32_t* __restrict__ old_of) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & (WAVE - 1);
    const bool keep = i < n && cls[i] != 1;
    const uint64_t m = __ballot(keep);
    if (i >= n) return;
    if (keep) {
        const uint32_t j = wave_off[i / WAVE] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        new_of[i] = j;
        old_of[j] = i;
    } else {
        new_of[i] = VS_INVALID_NODE;
    }
}

// The row mover for the wide columns (codes, vectors): rows [a, b) of the compacted order are gathered through old_of into staging,
// lanes over the 16-byte pieces of a row.  lpr_log2 < 6: 1 << lpr_log2 lanes per row (the power of two that holds its `pieces`),
// 64 >> lpr_log2 rows per wave; lpr_log2 == 6: one row per wave, the lanes stride over its pieces.  The host chooses from the width.
__global__ __launch_bounds__(256) void k_compact_rows(const uint4* __restrict__ src, uint32_t pieces, uint32_t lpr_log2,
                                                      const uint32_t* __restrict__ old_of, uint32_t a, uint32_t b, uint4* __restrict__ stage) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / WAVE, n_waves = (uint64_t)gridDim.x * (256 / WAVE);
    const uint32_t rpw = WAVE >> lpr_log2, sub = lane >> lpr_log2, first = lane & ((1u << lpr_log2) - 1u), step = 1u << lpr_log2;
    const uint64_t rows = b - a;
    for (uint64_t r = wave * rpw + sub; r < rows; r += n_waves * rpw) {
        const uint4* from = src + (size_t)old_of[a + r] * pieces;
        uint4* to = stage + (size_t)r * pieces;
        for (uint32_t p = first; p < pieces; p += step) to[p] = from[p];
    }
}
// the narrow columns (heap tids 8 B, cosine divisors 4 B, the byte masks): a lane per row
template <typename T>
__global__ __launch_bounds__(256) void k_compact_narrow(const T* __restrict__ src, const uint32_t* __restrict__ old_of, uint32_t a, uint32_t b,
                                                        T* __restrict__ stage) {
    const uint64_t rows = b - a;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * 256) stage[r] = src[old_of[a + r]];
}
// The neighbor form: a lane per entry, seg (16, 32 or 64, a divisor of 64) lanes per row — the whole row when nbr_stride == seg, else
// one row per wave in rounds of 64 entries with the running length carried over.  An entry v becomes new_of[v]; one that names a
// dropped node is cut and the list closes up in its order: a surviving entry's place is the count of survivors before it (ballot,
// popcount below the lane, within the lane's segment).  The tail is VS_INVALID_NODE.  Counters: one atomic per wave and counter.
__global__ __launch_bounds__(256) void k_compact_nbrs(const uint32_t* __restrict__ nbrs, uint32_t nbr_stride, uint32_t R, uint32_t seg, uint32_t n_before,
                                                      const uint32_t* __restrict__ old_of, const uint32_t* __restrict__ new_of, uint32_t a,
                                                      uint32_t b, uint32_t* __restrict__ stage, unsigned long long* __restrict__ cnt) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / WAVE, n_waves = (uint64_t)gridDim.x * (256 / WAVE);
    const uint32_t rpw = WAVE / seg, sub = lane / seg, e0 = lane % seg;
    const uint64_t segmask = seg == WAVE ? ~0ull : ((1ull << seg) - 1ull) << (sub * seg);
    const uint64_t below = segmask & ((1ull << lane) - 1ull);
    const uint64_t rows = b - a;
    uint32_t cut_total = 0, emptied = 0;
    for (uint64_t r0 = wave * rpw; r0 < rows; r0 += n_waves * rpw) {  // (wave-uniform trip count: the ballots see every lane)
        const uint64_t r = r0 + sub;
        const bool row_in = r < rows;
        const uint32_t* from = row_in ? nbrs + (size_t)old_of[a + r] * nbr_stride : nullptr;
        uint32_t* to = stage + (size_t)r * nbr_stride;
        uint32_t len = 0, cut_row = 0;
        for (uint32_t c0 = 0; c0 < nbr_stride; c0 += seg) {
            const uint32_t e = c0 + e0;
            const uint32_t v = row_in && e < R ? from[e] : VS_INVALID_NODE;  // (only the first R entries of a row are its list)
            const uint32_t w = v < n_before ? new_of[v] : VS_INVALID_NODE;
            const bool stays = w != VS_INVALID_NODE, cut = v < n_before && !stays;
            const uint64_t ms = __ballot(stays), mc = __ballot(cut);
            if (stays) to[len + (uint32_t)__popcll(ms & below)] = w;
            len += (uint32_t)__popcll(ms & segmask);
            cut_row += (uint32_t)__popcll(mc & segmask);
            cut_total += (uint32_t)__popcll(mc);  // (the wave's: a lane without a row cuts nothing)
        }
        if (row_in)
            for (uint32_t e = len + e0; e < nbr_stride; e += seg) to[e] = VS_INVALID_NODE;
        emptied += (uint32_t)__popcll(__ballot(row_in && e0 == 0 && cut_row != 0 && len == 0));
    }
    if (lane == 0) {
        if (cut_total) atomicAdd(&cnt[CN_EDGES_DROPPED], (unsigned long long)cut_total);
        if (emptied) atomicAdd(&cnt[CN_EMPTIED], (unsigned long long)emptied);
    }
}
// The label CSR of K, out of place (its rows have variable length).  First the label values of the kept nodes per wave of 64 nodes ...
__global__ __launch_bounds__(256) void k_compact_label_count(const uint8_t* __restrict__ cls, const uint32_t* __restrict__ label_off, uint32_t n,
                                                             uint32_t* __restrict__ wave_cnt) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t len = i < n && cls[i] != 1 ? label_off[i + 1] - label_off[i] : 0;
    for (int k = 1; k < WAVE; k <<= 1) len += __shfl_xor(len, k);
    if ((threadIdx.x & (WAVE - 1)) == 0 && i < n) wave_cnt[i / WAVE] = len;
}
// ... then, with their exclusive scan, every kept node writes its new offset and copies its set (a lane per node; sets are short)
__global__ __launch_bounds__(256) void k_compact_labels(const uint8_t* __restrict__ cls, const uint32_t* __restrict__ label_off,
                                                        const int16_t* __restrict__ label_val, uint32_t n, const uint32_t* __restrict__ wave_off,
                                                        const uint32_t* __restrict__ new_of, uint32_t n_after, uint32_t* __restrict__ out_off,
                                                        int16_t* __restrict__ out_val) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & (WAVE - 1);
    const bool keep = i < n && cls[i] != 1;
    const uint32_t lo = keep ? label_off[i] : 0, len = keep ? label_off[i + 1] - lo : 0;
    uint32_t incl = len;
    for (uint32_t k = 1; k < WAVE; k <<= 1) {  // inclusive prefix sum over the wave
        const uint32_t t = __shfl(incl, (int)(lane >= k ? lane - k : lane));
        if (lane >= k) incl += t;
    }
    if (!keep) return;
    const uint32_t at = wave_off[i / WAVE] + incl - len, j = new_of[i];
    out_off[j] = at;
    if (j + 1 == n_after) out_off[n_after] = at + len;
    for (uint32_t t = 0; t < len; ++t) out_val[at + t] = label_val[lo + t];
}
// the per-label start nodes under their new ids (every one of them is in K)
__global__ void k_compact_map_ids(uint32_t* __restrict__ ids, uint32_t n_ids, const uint32_t* __restrict__ new_of) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_ids) ids[t] = new_of[ids[t]];
}

#define VS_COMPACT_STAGE_DEFAULT (256ull << 20)

static int compact_impl(vs_index* ix, uint64_t stage_bytes, uint32_t flags, uint32_t* out_new_of, vs_compact_stats* out) {
    const char* what = "vs_index_compact";
    VS_REQUIRE(ix, "%s: index is NULL", what);
    if (out) memset(out, 0, sizeof(*out));
    VS_REQUIRE_OWNER(ix, what);
    VS_REQUIRE_NO_VIEWS(ix, what);
    VS_REQUIRE((flags & ~(uint32_t)VS_COMPACT_KEEP_EDGES_CHECK) == 0, "%s: unknown flags 0x%x", what, flags);
    VS_REQUIRE(ix->nbrs && ix->tids, "%s: needs neighbor lists and heap tids on the device", what);
    VS_TRY(require_no_batch(ix, what));
    VS_TRY(require_no_writer(ix, what, WRITER_ROWS_MIX));
    VS_TRY(require_own_mask(ix, what, "compacted"));
    const uint32_t n = ix->d.n;
    if (stage_bytes == 0) stage_bytes = VS_COMPACT_STAGE_DEFAULT;
    // the per-node columns (the list vs_index_reserve_impl copies, less the label CSR, which is rebuilt aside)
    struct Col {
        void* p;
        size_t row_bytes;
        int form;  // 0 wide (16-byte pieces), 2 the neighbor lists, 8 / 4 / 1 narrow (bytes of a row)
    };
    std::vector<Col> cols;
    auto add = [&](void* p, size_t row_bytes, int form) {
        if (p) cols.push_back(Col{p, row_bytes, form});
    };
    add(ix->nbrs, ix->nbr_stride * 4ull, 2);
    add(ix->codes, ix->code_stride * 8ull, 0);
    add(ix->tids, 8, 8);
    add(ix->vecs, ix->vec_stride * 4ull, 0);
    add(ix->vnorm, 4, 4);
    add(ix->vnorm_idx, 4, 4);
    add(ix->visible_own, 1, 1);
    for (int sn = 1; sn < VS_MAX_SNAPSHOTS; ++sn) add(ix->snap[sn], 1, 1);
    size_t widest = 0;
    for (const Col& cl : cols) {
        widest = std::max(widest, cl.row_bytes);
        VS_REQUIRE(cl.form != 0 || cl.row_bytes % 16 == 0, "%s: a row of %zu bytes is no multiple of 16", what, cl.row_bytes);
    }
    VS_REQUIRE(stage_bytes >= widest, "%s: stage_bytes %llu holds no row of %zu bytes", what, (unsigned long long)stage_bytes, widest);
    VS_REQUIRE(ix->nbr_stride % 16 == 0, "%s: neighbor rows of %u entries", what, ix->nbr_stride);
    // Dropped by every compaction that goes ahead, but not by one VS_COMPACT_KEEP_EDGES_CHECK refuses ("every byte as it was"): the
    // classes and the depends list name rows by their old numbers, and so do the qualifiers (a bit per OLD node number)
    auto drop_numbered = [&]() {
        vs_vis_base_drop(ix);
        vs_qual_drop_all(ix);
    };
    vs_compact_stats s{};
    s.n_before = s.n_after = n;
    if (n == 0 || ix->d.default_start == VS_INVALID_NODE) {
        drop_numbered();
        if (out) *out = s;
        return VS_OK;
    }
    vs_ctx* c = ix->ctx;
    hipStream_t st = c->stream;
    VS_HIP(hipSetDevice(c->device));
    std::vector<uint32_t> starts;
    VS_TRY(collect_start_nodes(ix, what, &starts));
    const bool labeled = ix->label_off != nullptr;
    const uint32_t n_waves = (n + WAVE - 1) / WAVE;
    unsigned long long h_cnt[CP_N] = {0};
    uint32_t new_default = ix->d.default_start, chunks = 0;
    bool moved = false;  // the first byte has moved: an error from here on leaves the index undefined
    auto run = [&]() -> int {  // (the stats are filled from what it got to, whatever it returns)
        DevScope sc(st);
        StageTimer tm;
        VS_TRY(tm.start(sc, c->profiling, ix->compact_ms, what));
        uint8_t *d_cls = nullptr, *d_flag = nullptr, *d_stage = nullptr;
        uint32_t *d_wave = nullptr, *d_lwave = nullptr, *d_starts = nullptr, *d_new_of = nullptr, *d_old_of = nullptr, *new_off = nullptr;
        int16_t* new_val = nullptr;
        unsigned long long* d_cnt = nullptr;
        VS_TRY(sc.alloc(&d_cls, (size_t)n, what));
        VS_TRY(sc.alloc(&d_wave, ((size_t)n_waves + 1) * 4, what));
        VS_TRY(sc.alloc(&d_starts, starts.size() * 4, what));
        VS_TRY(sc.alloc(&d_cnt, sizeof h_cnt, what));
        VS_TRY(sc.alloc(&d_new_of, (size_t)n * 4, what));
        VS_TRY(sc.alloc(&d_old_of, (size_t)n * 4, what));
        if (labeled) VS_TRY(sc.alloc(&d_lwave, ((size_t)n_waves + 1) * 4, what));
        if (flags & VS_COMPACT_KEEP_EDGES_CHECK) {
            VS_TRY(sc.alloc(&d_flag, (size_t)n, what));
            VS_HIP(hipMemsetAsync(d_flag, 0, (size_t)n, st));
        }
        VS_HIP(hipMemcpyAsync(d_starts, starts.data(), starts.size() * 4, hipMemcpyHostToDevice, st));
        h_cnt[CP_FIRST] = n;
        VS_HIP(hipMemsetAsync(d_cnt, 0, sizeof h_cnt, st));
        VS_HIP(hipMemcpyAsync(&d_cnt[CP_FIRST], &h_cnt[CP_FIRST], 8, hipMemcpyHostToDevice, st));  // (the atomicMin starts from n)
        VS_HIP(hipStreamSynchronize(st));
        tm.tick();
        const dim3 ngrid((n + 255) / 256);
        hipLaunchKernelGGL(k_cons_classify, ngrid, dim3(256), 0, st, (const uint64_t*)ix->tids, (const uint32_t*)ix->label_off, n, d_cls, d_cnt);
        VS_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_cons_keep_starts, dim3(((uint32_t)starts.size() + 255) / 256), dim3(256), 0, st, (const uint32_t*)d_starts,
                           (uint32_t)starts.size(), d_cls, d_cnt);
        VS_HIP(hipGetLastError());
        if (d_flag) {  // the read-only pass of VS_COMPACT_KEEP_EDGES_CHECK: the cells of kept rows that name a dropped node
            const size_t cells = (size_t)n * ix->d.num_neighbors;
            hipLaunchKernelGGL(k_cons_flag, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, (const uint32_t*)ix->nbrs, ix->nbr_stride,
                               ix->d.num_neighbors, n, (const uint8_t*)d_cls, d_flag, d_cnt);
            VS_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(k_compact_keep_count, ngrid, dim3(256), 0, st, (const uint8_t*)d_cls, n, d_wave, d_cnt);
        VS_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_cons_work_scan, dim3(1), dim3(256), 0, st, d_wave, n_waves);
        VS_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_compact_maps, ngrid, dim3(256), 0, st, (const uint8_t*)d_cls, n, (const uint32_t*)d_wave, d_new_of, d_old_of);
        VS_HIP(hipGetLastError());
        if (labeled) {
            hipLaunchKernelGGL(k_compact_label_count, ngrid, dim3(256), 0, st, (const uint8_t*)d_cls, (const uint32_t*)ix->label_off, n, d_lwave);
            VS_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_cons_work_scan, dim3(1), dim3(256), 0, st, d_lwave, n_waves);
            VS_HIP(hipGetLastError());
            VS_HIP(hipMemcpyAsync(&d_cnt[CP_LABEL_VALS], d_lwave + n_waves, 4, hipMemcpyDeviceToDevice, st));
        }
        // the totals join the counters (little endian: the low half of a zeroed u64), so that one copy brings everything back
        VS_HIP(hipMemcpyAsync(&d_cnt[CP_N_AFTER], d_wave + n_waves, 4, hipMemcpyDeviceToDevice, st));
        VS_HIP(hipMemcpyAsync(h_cnt, d_cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st));
        VS_HIP(hipStreamSynchronize(st));
        tm.tock(0);
        const uint32_t n_after = (uint32_t)h_cnt[CP_N_AFTER], first = (uint32_t)h_cnt[CP_FIRST];
        s.n_after = n_after;
        s.tombstones = h_cnt[CN_TOMB];
        s.tombstones_kept = h_cnt[CN_KEPT];
        s.edges_cut = h_cnt[CN_EDGES_DROPPED];
        if (d_flag && s.edges_cut) {
            s.n_after = n;
            vs_set_error("%s: %llu entries of kept rows name a dropped node (VS_COMPACT_KEEP_EDGES_CHECK; vs_index_consolidate_deletes first)",
                         what, (unsigned long long)s.edges_cut);
            return VS_ERR_STATE;
        }
        drop_numbered();
        VS_REQUIRE(n_after >= 1 && n_after <= n && (n_after == n) == (first == n), "%s: %u of %u nodes kept, first dropped %u", what, n_after, n, first);
        if (out_new_of) VS_HIP(hipMemcpy(out_new_of, d_new_of, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (n_after == n) return VS_OK;  // nothing in D: nothing is written
        // every allocation before the first byte moves: the staging buffer and the label arrays of K
        size_t need = 0;
        for (const Col& cl : cols) {
            const size_t rows = cl.form == 2 ? n_after : n_after - first;
            need = std::max(need, std::min<size_t>(rows, stage_bytes / cl.row_bytes) * cl.row_bytes);
        }
        VS_TRY(sc.alloc(&d_stage, std::max<size_t>(need, 16), what));
        const uint64_t vals_after = h_cnt[CP_LABEL_VALS];
        if (labeled) {
            VS_TRY(sc.alloc(&new_off, ((size_t)std::max(n, ix->capacity) + 1) * 4, what));
            VS_TRY(sc.alloc(&new_val, std::max<uint64_t>(vals_after, 1) * 2, what));
        }
        if (labeled) {  // (reads the label CSR as it stands, writes the fresh arrays: nothing of the index has changed yet)
            hipLaunchKernelGGL(k_compact_labels, ngrid, dim3(256), 0, st, (const uint8_t*)d_cls, (const uint32_t*)ix->label_off,
                               (const int16_t*)ix->label_val, n, (const uint32_t*)d_lwave, (const uint32_t*)d_new_of, n_after, new_off, new_val);
            VS_HIP(hipGetLastError());
        }
        VS_HIP(hipMemcpyAsync(&new_default, d_new_of + ix->d.default_start, 4, hipMemcpyDeviceToHost, st));
        VS_HIP(hipStreamSynchronize(st));
        moved = true;
        ix->nbr_mask_valid = false;
        tm.tick();
        for (const Col& cl : cols) {
            const uint32_t from = cl.form == 2 ? 0 : first;  // (every neighbor row is renamed; the other columns start at the first hole)
            const uint32_t per = (uint32_t)std::min<uint64_t>(stage_bytes / cl.row_bytes, n_after - from);
            uint32_t col_chunks = 0;
            for (uint32_t a = from; a < n_after; a += per, ++col_chunks) {
                const uint32_t b = (uint32_t)std::min<uint64_t>((uint64_t)a + per, n_after), rows = b - a;
                char* col = static_cast<char*>(cl.p);
                if (cl.form == 2) {
                    const uint32_t seg = ix->nbr_stride == 16 || ix->nbr_stride == 32 ? ix->nbr_stride : WAVE;
                    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)rows + 4 * (WAVE / seg) - 1) / (4 * (WAVE / seg)), 1u << 16);
                    hipLaunchKernelGGL(k_compact_nbrs, dim3(grid), dim3(256), 0, st, (const uint32_t*)ix->nbrs, ix->nbr_stride, ix->d.num_neighbors, seg,
                                       n, (const uint32_t*)d_old_of, (const uint32_t*)d_new_of, a, b, reinterpret_cast<uint32_t*>(d_stage), d_cnt);
                } else if (cl.form == 0) {
                    const uint32_t pieces = (uint32_t)(cl.row_bytes / 16);
                    uint32_t lpr_log2 = 0;
                    while (lpr_log2 < 6 && (1u << lpr_log2) < pieces) ++lpr_log2;
                    const uint32_t rpb = 4 * (WAVE >> lpr_log2);  // rows a workgroup of four waves handles per round
                    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)rows + rpb - 1) / rpb, 1u << 16);
                    hipLaunchKernelGGL(k_compact_rows, dim3(grid), dim3(256), 0, st, reinterpret_cast<const uint4*>(cl.p), pieces, lpr_log2,
                                       (const uint32_t*)d_old_of, a, b, reinterpret_cast<uint4*>(d_stage));
                } else {
                    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)rows + 255) / 256, 1u << 16);
                    if (cl.form == 8)
                        hipLaunchKernelGGL(k_compact_narrow<uint64_t>, dim3(grid), dim3(256), 0, st, (const uint64_t*)cl.p, (const uint32_t*)d_old_of, a,
                                           b, reinterpret_cast<uint64_t*>(d_stage));
                    else if (cl.form == 4)
                        hipLaunchKernelGGL(k_compact_narrow<uint32_t>, dim3(grid), dim3(256), 0, st, (const uint32_t*)cl.p, (const uint32_t*)d_old_of, a,
                                           b, reinterpret_cast<uint32_t*>(d_stage));
                    else
                        hipLaunchKernelGGL(k_compact_narrow<uint8_t>, dim3(grid), dim3(256), 0, st, (const uint8_t*)cl.p, (const uint32_t*)d_old_of, a,
                                           b, d_stage);
                }
                VS_HIP(hipGetLastError());
                VS_HIP(hipMemcpyAsync(col + (size_t)a * cl.row_bytes, d_stage, (size_t)rows * cl.row_bytes, hipMemcpyDeviceToDevice, st));
            }
            if (cl.row_bytes == widest) chunks = std::max(chunks, col_chunks);
        }
        if (ix->d.n_label_starts) {
            hipLaunchKernelGGL(k_compact_map_ids, dim3((ix->d.n_label_starts + 255) / 256), dim3(256), 0, st, ix->ls_nodes, ix->d.n_label_starts,
                               (const uint32_t*)d_new_of);
            VS_HIP(hipGetLastError());
        }
        // (the counters of the first copy stand; the neighbor form has added edges_cut — unless the check pass counted them — and rows_emptied)
        VS_HIP(hipMemcpyAsync(h_cnt, d_cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st));
        VS_HIP(hipStreamSynchronize(st));
        tm.tock(1);
        if (labeled) {
            (void)hipFree(ix->label_off);
            (void)hipFree(ix->label_val);
            ix->label_off = sc.release(new_off);  // (the index's own from here on)
            ix->label_val = sc.release(new_val);
            ix->n_label_vals = vals_after;
        }
        ix->d.default_start = new_default;
        ix->d.n = n_after;
        ix->codes_epoch++;  // (rows have new numbers)
        s.rows_moved = n_after - first;
        s.edges_cut = h_cnt[CN_EDGES_DROPPED];
        s.rows_emptied = h_cnt[CN_EMPTIED];
        s.chunks = chunks;
        // what was derived from the old numbering is stale, as after an insert: the neighbor masks go (re-derived lazily), the
        // launch planner forgets the last batches, the label masks are re-derived now
        if (ix->nbr_mask) {
            (void)hipFree(ix->nbr_mask);
            ix->nbr_mask = nullptr;
        }
        ix->nbr_mask_valid = false;
        ix->nbr_mask_tried = false;
        ix->obs = ScanObs{};
        ix->last_fast = FastSig{};
        ix->last_ins_limit = 0;
        if (labeled) VS_TRY(vs_refresh_label_masks(ix));
        return VS_OK;
    };
    int rc = run();
    if (out) *out = s;
    if (rc == VS_OK && moved) rc = vs_validate_graph(ix);
    return rc;
}
extern "C" int vs_index_compact(vs_index* ix, uint64_t stage_bytes, uint32_t flags, uint32_t* out_new_of, vs_compact_stats* out) {
    return vs_guard("vs_index_compact", [&] { return compact_impl(ix, stage_bytes, flags, out_new_of, out); });
}
extern "C" int vs_index_compact_kernel_ms(vs_index* ix, double* ms /*[2]*/, int reset) {
    return read_kernel_ms("vs_index_compact_kernel_ms", ix, ix ? ix->compact_ms : nullptr, 2, ms, reset);
}

// vs_index_shrink_to_fit: the arrays one at a time at d.n rows — allocate, copy device to device, swap, free the old one — so the
// peak extra memory is one array.  Narrowest row first, the vectors last: what the smaller arrays gave back is free when the
// largest one asks.
static int shrink_impl(vs_index* ix) {
    const char* what = "vs_index_shrink_to_fit";
    VS_REQUIRE(ix, "%s: index is NULL", what);
    VS_REQUIRE_OWNER(ix, what);
    VS_REQUIRE_NO_VIEWS(ix, what);
    if (ix->ws.pending) {
        vs_set_error("%s: a batch of this handle is in flight (vs_search_batch_dev_finish first)", what);
        return VS_ERR_STATE;
    }
    const uint32_t n = ix->d.n;
    if (n == 0 || ix->capacity <= n) return VS_OK;
    vs_ctx* c = ix->ctx;
    VS_HIP(hipSetDevice(c->device));
    VS_HIP(hipStreamSynchronize(c->stream));
    struct Item {
        void** slot;
        size_t row_bytes, extra_rows;
    };
    std::vector<Item> items;
    auto add = [&](void* slot, size_t row_bytes, size_t extra = 0) {
        void** sl = reinterpret_cast<void**>(slot);
        if (*sl) items.push_back(Item{sl, row_bytes, extra});
    };
    add(&ix->visible_own, 1);
    for (int sn = 1; sn < VS_MAX_SNAPSHOTS; ++sn) add(&ix->snap[sn], 1);
    add(&ix->vnorm, 4);
    add(&ix->vnorm_idx, 4);
    add(&ix->label_off, 4, 1);
    add(&ix->tids, 8);
    add(&ix->nbrs, ix->nbr_stride * 4ull);
    add(&ix->codes, ix->code_stride * 8ull);
    add(&ix->vecs, ix->vec_stride * 4ull);
    std::stable_sort(items.begin(), items.end(), [](const Item& x, const Item& y) { return x.row_bytes < y.row_bytes; });
    int r = VS_OK;
    for (Item& it : items) {
        const size_t bytes = ((size_t)n + it.extra_rows) * it.row_bytes;
        void* fresh = nullptr;
        hipError_t e = hipMalloc(&fresh, bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(fresh, *it.slot, bytes, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (fresh) (void)hipFree(fresh);
            vs_set_error("%s: shrinking to %u nodes failed: %s", what, n, hipGetErrorString(e));
            r = e == hipErrorOutOfMemory ? VS_ERR_OOM : VS_ERR_HIP;
            break;
        }
        if (ix->visible && ix->visible == *it.slot) ix->visible = static_cast<const uint8_t*>(fresh);  // (the mask in force moved too)
        (void)hipFree(*it.slot);
        *it.slot = fresh;
        // from the first swapped array on, n rows is all that every array is known to hold: an insert must reserve before it writes
        ix->capacity = n;
    }
    return r;
}
extern "C" int vs_index_shrink_to_fit(vs_index* ix) {
    return vs_guard("vs_index_shrink_to_fit", [&] { return shrink_impl(ix); });
}

// ---------------------------------------------------------------------------------------------------------------
// vs_index_label_reach / vs_index_repair_labels: what a label-filtered scan can reach, and in-edges for what it cannot
// (DESIGN.md section 6f has the rule).  A scan with key {l} starts at l's start node and only ever enqueues carriers of l, so a
// row is returned under {l} only if a chain of carriers leads to it from there.  reach[i] = the labels under whose single-label
// key node i is reached (64 labels per group, one bit each), need[x] = the labels a live x carries and is not reached under.
// The repair hands every lost x one in-edge per group and round, from the nearest row that is already reached under a label x
// still needs; a row serves one node per group and round, and the entry it gives up keeps another in-edge from a row that is
// reached under everything the entry carries.
// ---------------------------------------------------------------------------------------------------------------
enum { LR_PLACED_FREE = 0, LR_PLACED_DROPPED, LR_PLACED_VICTIM, LR_BLOCKED, LR_CONTENDED, LR_ALREADY, LR_COUNT, LR_N = 8 };
#define NEAR_WAVES 4   // waves per workgroup of k_nearest_masked
#define NEAR_PASSES 4  // 16-row passes in flight per wave

// per-group masks from the label CSR: table[label] = the label's bit in this group, 0xFF = not one of the group's labels
__global__ __launch_bounds__(256) void k_lr_group_masks(const uint32_t* __restrict__ off, const int16_t* __restrict__ val, uint32_t n,
                                                        const uint8_t* __restrict__ table, uint64_t* __restrict__ mask) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint64_t m = 0;
    for (uint32_t j = off[i]; j < off[i + 1]; ++j) {
        const uint32_t b = table[(uint16_t)val[j]];
        if (b < 64) m |= 1ull << b;
    }
    mask[i] = m;
}
// a scan with key {l} starts at l's start node whether or not that node carries l (every node once: the host merges the bits)
__global__ void k_lr_seed(const uint32_t* __restrict__ nodes, const uint64_t* __restrict__ bits, uint32_t ns, uint64_t* __restrict__ reach,
                          uint64_t* __restrict__ fresh) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ns) return;
    reach[nodes[t]] = bits[t];
    fresh[nodes[t]] = bits[t];
}
// one lane per list cell u -> v: the bits u gained in the last sweep (fresh_in) that v carries and lacks go into reach[v]; what the
// atomic really added is v's frontier for the next sweep.  The fixed point does not depend on the order of the atomics.
__global__ __launch_bounds__(256) void k_lr_sweep(const uint32_t* __restrict__ nbrs, uint32_t nbr_stride, uint32_t R, uint32_t n,
                                                  const uint64_t* __restrict__ mask, uint64_t jmask, uint64_t* reach,
                                                  const uint64_t* __restrict__ fresh_in, uint64_t* fresh_out, uint32_t* __restrict__ changed) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * R) return;
    const size_t u = i / R;
    const uint64_t f = fresh_in[u];
    if (!f) return;
    const uint32_t v = nbrs[u * nbr_stride + (i % R)];
    if (v >= n) return;
    const uint64_t add = f & mask[v] & jmask & ~reach[v];
    if (!add) return;
    const uint64_t old = atomicOr(reinterpret_cast<unsigned long long*>(reach + v), (unsigned long long)add);
    const uint64_t nw = add & ~old;
    if (nw) {
        atomicOr(reinterpret_cast<unsigned long long*>(fresh_out + v), (unsigned long long)nw);
        *changed = 1;
    }
}
// need[] and the per-bit counters (bitcnt[b] live carriers of bit b, bitcnt[64 + b] lost ones), through an LDS histogram per workgroup;
// flag[] marks the lost nodes for the count / scan / scatter passes, any[] (may be null) collects them over the groups
__global__ __launch_bounds__(256) void k_lr_need(const uint8_t* __restrict__ cls, const uint64_t* __restrict__ mask, uint64_t jmask,
                                                 const uint64_t* __restrict__ reach, uint32_t n, uint64_t* __restrict__ need,
                                                 uint8_t* __restrict__ flag, uint8_t* __restrict__ any, uint32_t* __restrict__ bitcnt) {
    __shared__ uint32_t h[128];
    if (threadIdx.x < 128) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        uint64_t nd = 0;
        if (cls[i] == 0) {
            uint64_t m = mask[i];
            nd = m & jmask & ~reach[i];
            for (; m; m &= m - 1) atomicAdd(&h[__builtin_ctzll(m)], 1u);
            for (uint64_t t = nd; t; t &= t - 1) atomicAdd(&h[64 + __builtin_ctzll(t)], 1u);
        }
        need[i] = nd;
        flag[i] = nd != 0;
        if (nd && any) any[i] = 1;
    }
    __syncthreads();
    if (threadIdx.x < 128 && h[threadIdx.x]) atomicAdd(&bitcnt[threadIdx.x], h[threadIdx.x]);
}
// nodes with flag[i] != 0 (and, with cls, class 0)
__global__ __launch_bounds__(256) void k_lr_count(const uint8_t* __restrict__ flag, uint32_t want, const uint8_t* __restrict__ cls, uint32_t n,
                                                  unsigned long long* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint64_t m = __ballot(i < n && (flag[i] != 0) == (want != 0) && (!cls || cls[i] == 0));
    if ((threadIdx.x & (WAVE - 1)) == 0 && m) atomicAdd(out, (unsigned long long)__popcll(m));
}
// strong[y]: in-edges q -> y from rows outside D that are reached under every label y carries in this group
__global__ __launch_bounds__(256) void k_lr_strong(const uint32_t* __restrict__ nbrs, uint32_t nbr_stride, uint32_t R, uint32_t n,
                                                   const uint8_t* __restrict__ cls, const uint64_t* __restrict__ mask, uint64_t jmask,
                                                   const uint64_t* __restrict__ reach, uint32_t* __restrict__ strong) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * R) return;
    const size_t q = i / R;
    if (cls[q] == 1) return;
    const uint32_t y = nbrs[q * nbr_stride + (i % R)];
    if (y >= n) return;
    if ((mask[y] & jmask & ~reach[q]) == 0) atomicAdd(&strong[y], 1u);
}

// k_nearest_masked: for each query node x the minimum of (Hamming(code[x], code[p]) << 32) | p over the rows p != x with
// bits[p] & want != 0 and skip[p] != 1.  A flat pass over every code row per tile of Q queries, laid out as k_scan_topk (vs_scan.hip):
// the tile's codes, want words and node ids sit in LDS, 4 lanes x 16 B cover a 64-B sector of a row, 16 rows per wave per pass,
// NEAR_PASSES passes in flight, a contiguous row range per wave.  Top-1 needs no list: every lane keeps one running minimum per query
// in registers, a wave folds them with shuffles at the end and publishes with one 64-bit atomicMin per query (the minimum does not
// depend on the order).  Algorithmic traffic per tile: n x (code row + 8 B of bits + 1 B of skip).
struct NearArgs {
    const uint64_t* codes;
    uint32_t code_stride, n;
    const uint32_t* qnodes;  // [nq]
    uint32_t nq;
    const uint64_t* want;    // [nq], or per node with want_by_node
    uint32_t want_by_node;
    const uint64_t* bits;    // [n]
    const uint8_t* skip;     // [n] or null; 1 = never a source
    uint32_t rows_per_wave;  // multiple of 16 * NEAR_PASSES
    unsigned long long* out_key;  // [nq], ~0 before the launch
};
__device__ __forceinline__ void near_stage_tile(const NearArgs& a, uint32_t q0, uint32_t Q, uint64_t* qc, uint64_t* qw, uint32_t* qn) {
    const uint32_t nqt = min(Q, a.nq - q0);
    for (uint32_t i = threadIdx.x; i < Q * a.code_stride; i += blockDim.x) {
        const uint32_t qi = i / a.code_stride;
        qc[i] = qi < nqt ? a.codes[(size_t)a.qnodes[q0 + qi] * a.code_stride + (i - qi * a.code_stride)] : 0ull;
    }
    if (threadIdx.x < Q) {
        const uint32_t qi = threadIdx.x;
        const uint32_t node = qi < nqt ? a.qnodes[q0 + qi] : VS_INVALID_NODE;
        qn[qi] = node;
        qw[qi] = qi < nqt ? (a.want_by_node ? a.want[node] : a.want[q0 + qi]) : 0ull;  // (a query past the tile's end wants nothing)
    }
    __syncthreads();
}
__device__ __forceinline__ void near_publish(const NearArgs& a, uint32_t q, uint64_t best, int lane) {
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)best, sh, WAVE);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), sh, WAVE);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        best = o < best ? o : best;
    }
    if (lane == 0 && best != ~0ull && q < a.nq) atomicMin(a.out_key + q, (unsigned long long)best);
}
template <int NCH, int Q>
__global__ __launch_bounds__(NEAR_WAVES* WAVE) void k_nearest_masked(NearArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* qc = reinterpret_cast<uint64_t*>(smem);          // [Q][code_stride]
    uint64_t* qw = qc + (size_t)Q * a.code_stride;             // [Q]
    uint32_t* qn = reinterpret_cast<uint32_t*>(qw + Q);        // [Q]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t q0 = blockIdx.x * Q;
    near_stage_tile(a, q0, Q, qc, qw, qn);
    const uint32_t gw = blockIdx.y * NEAR_WAVES + wave;
    const uint32_t r_begin = (uint32_t)min<uint64_t>((uint64_t)gw * a.rows_per_wave, a.n);
    const uint32_t r_end = (uint32_t)min<uint64_t>((uint64_t)r_begin + a.rows_per_wave, a.n);
    const int l4 = lane & 3, grp = lane >> 2;
    uint64_t best[Q];
#pragma unroll
    for (int qi = 0; qi < Q; ++qi) best[qi] = ~0ull;
    for (uint32_t r0 = r_begin; r0 < r_end; r0 += 16 * NEAR_PASSES) {
        ulonglong2 rows[NEAR_PASSES][NCH];
        uint64_t rb[NEAR_PASSES];  // the row's bits, 0 for a row that is out of range or skipped
#pragma unroll
        for (int p = 0; p < NEAR_PASSES; ++p) {
            const uint32_t row = r0 + (uint32_t)p * 16 + grp;
            const bool ok = row < r_end;
            const uint64_t* rp = a.codes + (size_t)(ok ? row : r_begin) * a.code_stride;
#pragma unroll
            for (int t = 0; t < NCH; ++t) {
                const uint32_t w = 2u * (uint32_t)l4 + 8u * (uint32_t)t;
                rows[p][t] = (ok && w < a.code_stride) ? *reinterpret_cast<const ulonglong2*>(rp + w) : make_ulonglong2(0, 0);
            }
            rb[p] = (ok && !(a.skip && a.skip[row] == 1)) ? a.bits[row] : 0ull;
        }
#pragma unroll
        for (int qi = 0; qi < Q; ++qi) {
            ulonglong2 qv[NCH];
#pragma unroll
            for (int t = 0; t < NCH; ++t) {
                const uint32_t w = 2u * (uint32_t)l4 + 8u * (uint32_t)t;
                qv[t] = w < a.code_stride ? *reinterpret_cast<const ulonglong2*>(qc + (size_t)qi * a.code_stride + w) : make_ulonglong2(0, 0);
            }
            const uint64_t want = qw[qi];
            const uint32_t self = qn[qi];
#pragma unroll
            for (int p = 0; p < NEAR_PASSES; ++p) {
                uint32_t acc = 0;
#pragma unroll
                for (int t = 0; t < NCH; ++t)
                    acc += (uint32_t)__popcll(rows[p][t].x ^ qv[t].x) + (uint32_t)__popcll(rows[p][t].y ^ qv[t].y);
                const uint32_t row = r0 + (uint32_t)p * 16 + grp;
                const uint64_t key = ((uint64_t)quad_sum(acc) << 32) | row;
                if ((rb[p] & want) != 0 && row != self && key < best[qi]) best[qi] = key;
            }
        }
    }
#pragma unroll
    for (int qi = 0; qi < Q; ++qi) near_publish(a, q0 + (uint32_t)qi, best[qi], lane);
}
// code rows of more than 48 words: the same pass with the words of a row walked in a loop (ham_row4), one 16-row pass at a time
template <int Q>
__global__ __launch_bounds__(NEAR_WAVES* WAVE) void k_nearest_masked_wide(NearArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* qc = reinterpret_cast<uint64_t*>(smem);
    uint64_t* qw = qc + (size_t)Q * a.code_stride;
    uint32_t* qn = reinterpret_cast<uint32_t*>(qw + Q);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t q0 = blockIdx.x * Q;
    near_stage_tile(a, q0, Q, qc, qw, qn);
    const uint32_t gw = blockIdx.y * NEAR_WAVES + wave;
    const uint32_t r_begin = (uint32_t)min<uint64_t>((uint64_t)gw * a.rows_per_wave, a.n);
    const uint32_t r_end = (uint32_t)min<uint64_t>((uint64_t)r_begin + a.rows_per_wave, a.n);
    const int l4 = lane & 3, grp = lane >> 2;
    uint64_t best[Q];
#pragma unroll
    for (int qi = 0; qi < Q; ++qi) best[qi] = ~0ull;
    for (uint32_t r0 = r_begin; r0 < r_end; r0 += 16) {
        const uint32_t row = r0 + grp;
        const bool ok = row < r_end;
        const uint64_t* rp = a.codes + (size_t)(ok ? row : r_begin) * a.code_stride;
        const uint64_t rb = (ok && !(a.skip && a.skip[row] == 1)) ? a.bits[row] : 0ull;
#pragma unroll
        for (int qi = 0; qi < Q; ++qi) {
            const uint64_t key = ((uint64_t)ham_row4(rp, qc + (size_t)qi * a.code_stride, l4, a.code_stride, ok) << 32) | row;
            if ((rb & qw[qi]) != 0 && row != qn[qi] && key < best[qi]) best[qi] = key;
        }
    }
#pragma unroll
    for (int qi = 0; qi < Q; ++qi) near_publish(a, q0 + (uint32_t)qi, best[qi], lane);
}
template <int NCH, int Q>
static int launch_near_tq(vs_index* ix, const NearArgs& a, dim3 grid, size_t lds) {
    if (NCH == 0) hipLaunchKernelGGL((k_nearest_masked_wide<Q>), grid, dim3(NEAR_WAVES * WAVE), lds, ix->ctx->stream, a);
    else hipLaunchKernelGGL((k_nearest_masked<(NCH ? NCH : 1), Q>), grid, dim3(NEAR_WAVES * WAVE), lds, ix->ctx->stream, a);
    VS_HIP(hipGetLastError());
    return VS_OK;
}
template <int NCH>
static int launch_near_t(vs_index* ix, const NearArgs& a, uint32_t Q, dim3 grid, size_t lds) {
    return Q == 4 ? launch_near_tq<NCH, 4>(ix, a, grid, lds) : launch_near_tq<NCH, 8>(ix, a, grid, lds);
}
// d_keys [nq] is set to ~0 and receives the minimum keys; every pointer is a device pointer
static int launch_nearest_masked(vs_index* ix, const uint32_t* d_qnodes, uint32_t nq, const uint64_t* d_want, bool want_by_node,
                                 const uint64_t* d_bits, const uint8_t* d_skip, unsigned long long* d_keys, uint64_t* tiles = nullptr) {
    if (nq == 0) return VS_OK;
    vs_ctx* c = ix->ctx;
    const uint32_t n = ix->d.n, stride = ix->code_stride;
    VS_HIP(hipMemsetAsync(d_keys, 0xFF, (size_t)nq * 8, c->stream));
    // queries per tile: the codes stream once per tile (the flat scan is issue bound from about 8 queries at 24-word codes)
    const uint32_t Q = nq <= 4 ? 4u : 8u;
    const uint32_t step = 16 * NEAR_PASSES;
    uint32_t waves = (uint32_t)c->prop.multiProcessorCount * 8u;
    uint32_t rows_per_wave = (uint32_t)(((uint64_t)n + waves - 1) / std::max(waves, 1u));
    rows_per_wave = std::max(step, round_up_u32(rows_per_wave, step));
    waves = (uint32_t)(((uint64_t)n + rows_per_wave - 1) / rows_per_wave);
    NearArgs a;
    a.codes = ix->codes;
    a.code_stride = stride;
    a.n = n;
    a.qnodes = d_qnodes;
    a.nq = nq;
    a.want = d_want;
    a.want_by_node = want_by_node ? 1u : 0u;
    a.bits = d_bits;
    a.skip = d_skip;
    a.rows_per_wave = rows_per_wave;
    a.out_key = d_keys;
    const dim3 grid((nq + Q - 1) / Q, (waves + NEAR_WAVES - 1) / NEAR_WAVES);
    if (tiles) *tiles += grid.x;
    const size_t lds = (size_t)Q * stride * 8 + (size_t)Q * 12;
    VS_REQUIRE(lds <= 48 * 1024, "vs_nearest_masked: code rows of %u words do not fit a tile in LDS", stride);
    switch ((stride + 7) / 8) {
        case 1: return launch_near_t<1>(ix, a, Q, grid, lds);
        case 2: return launch_near_t<2>(ix, a, Q, grid, lds);
        case 3: return launch_near_t<3>(ix, a, Q, grid, lds);
        case 4: return launch_near_t<4>(ix, a, Q, grid, lds);
        case 5:
        case 6: return launch_near_t<6>(ix, a, Q, grid, lds);
        default: return launch_near_t<0>(ix, a, Q, grid, lds);
    }
}

// each source row serves one node per group and round: of the nodes that picked it, the smallest id
__global__ __launch_bounds__(256) void k_lr_claim(const uint32_t* __restrict__ lost, uint32_t nlost, const unsigned long long* __restrict__ key,
                                                  uint32_t* __restrict__ claim) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nlost) return;
    const unsigned long long k = key[t];
    if (k != ~0ull) atomicMin(&claim[(uint32_t)k], lost[t]);
}
// one wave per lost node x; the wave whose x won the claim on its source p edits p's row: reads p's row, cls, mask, reach, strong,
// writes one entry of p's row.  No two waves write the same row and nobody reads a row another wave writes.
__global__ __launch_bounds__(WAVE) void k_lr_apply(const uint32_t* __restrict__ lost, uint32_t nlost, const unsigned long long* __restrict__ key,
                                                   const uint32_t* __restrict__ claim, uint32_t* nbrs, uint32_t nbr_stride, uint32_t R,
                                                   uint32_t n, const uint8_t* __restrict__ cls, const uint64_t* __restrict__ mask,
                                                   uint64_t jmask, const uint64_t* __restrict__ reach, const uint32_t* __restrict__ strong,
                                                   uint8_t* __restrict__ rowchg, unsigned long long* __restrict__ cnt) {
    const uint32_t t = blockIdx.x;
    if (t >= nlost) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t x = lost[t];
    const unsigned long long k = key[t];
    if (k == ~0ull) {  // (no admissible source: the start node of a needed label always is one, so this is a row of its own making)
        if (lane == 0) atomicAdd(&cnt[LR_BLOCKED], 1ull);
        return;
    }
    const uint32_t p = (uint32_t)k;
    if (claim[p] != x) {
        if (lane == 0) atomicAdd(&cnt[LR_CONTENDED], 1ull);
        return;
    }
    uint32_t* row = nbrs + (size_t)p * nbr_stride;
    uint32_t len = R;
    uint64_t named = 0;
    for (uint32_t c0 = 0; c0 < R && len == R; c0 += WAVE) {
        const uint32_t j = c0 + lane;
        const uint32_t e = j < R ? row[j] : VS_INVALID_NODE;
        const uint64_t inv = __ballot(e == VS_INVALID_NODE);  // (lanes past R read as the sentinel)
        const uint64_t below = inv ? ((1ull << __builtin_ctzll(inv)) - 1ull) : ~0ull;
        named |= __ballot(e == x) & below;
        if (inv) len = min(R, c0 + (uint32_t)__builtin_ctzll(inv));
    }
    if (named) {
        if (lane == 0) atomicAdd(&cnt[LR_ALREADY], 1ull);
        return;
    }
    uint32_t slot = VS_INVALID_NODE, kind = LR_PLACED_FREE;
    if (len < R) {
        slot = len;
    } else {
        const uint64_t rp = reach[p];
        for (uint32_t pass = 0; pass < 2 && slot == VS_INVALID_NODE; ++pass) {  // from the last entry backwards
            kind = pass == 0 ? LR_PLACED_DROPPED : LR_PLACED_VICTIM;
            for (uint32_t c0 = (R - 1) / WAVE * WAVE; slot == VS_INVALID_NODE; c0 -= WAVE) {
                const uint32_t j = c0 + lane;
                const uint32_t y = j < R ? row[j] : VS_INVALID_NODE;
                bool hit = false;
                if (y < n) {
                    if (pass == 0) hit = cls[y] == 1;
                    else hit = strong[y] >= 1u + ((mask[y] & jmask & ~rp) == 0 ? 1u : 0u);
                }
                const uint64_t m = __ballot(hit);
                if (m) slot = c0 + 63u - (uint32_t)__builtin_clzll(m);
                if (c0 == 0) break;
            }
        }
    }
    if (lane == 0) {
        if (slot == VS_INVALID_NODE) {
            atomicAdd(&cnt[LR_BLOCKED], 1ull);
        } else {
            row[slot] = x;
            rowchg[p] = 1;
            atomicAdd(&cnt[kind], 1ull);
        }
    }
}

struct LrState {  // (non-owning: every buffer belongs to the DevScope of the call)
    vs_index* ix = nullptr;
    const char* what = "";
    hipStream_t st = nullptr;
    uint32_t n = 0, R = 0, n_waves = 0;
    // the labels judged, ascending; groups of 64 in that order
    std::vector<int16_t> labels;
    std::vector<uint32_t> lstart;   // the label's start node, VS_INVALID_NODE = none
    std::vector<uint8_t> carried;   // the label is in some node's set
    uint32_t without_start = 0, ngroups = 0;
    bool own_masks = false;         // one group: the index's own label_mask / label_bit
    std::vector<uint8_t> own_bit, table;
    // the group in hand
    const uint64_t* mask = nullptr;
    uint64_t jmask = 0;             // bits of the group's labels that are carried and have a start node
    uint8_t bit[64];
    uint32_t sweeps = 0;
    // device
    uint8_t *cls = nullptr, *flag = nullptr, *any = nullptr, *rowchg = nullptr, *d_table = nullptr, *mark = nullptr;
    uint64_t *mask_buf = nullptr, *reach = nullptr, *fresh[2] = {nullptr, nullptr}, *need = nullptr, *seed_bits = nullptr;
    uint32_t *wave = nullptr, *strong = nullptr, *claim = nullptr, *lost = nullptr, *seed_nodes = nullptr, *bitcnt = nullptr, *changed = nullptr,
             *d_starts = nullptr;
    unsigned long long *cnt = nullptr, *keys = nullptr, *cons_cnt = nullptr;
    size_t lost_cap = 0;
    StageTimer tm;
};

// the labels, the node classes and the buffers every pass needs (repair: also those of steps 2-5)
// ms [4]: where the stage times of the passes accumulate while the context is profiling
static int lr_init(LrState& S, vs_index* ix, DevScope& sc, const char* what, bool repair, double* ms) {
    S.ix = ix;
    S.what = what;
    S.st = ix->ctx->stream;
    const uint32_t n = S.n = ix->d.n;
    S.R = ix->d.num_neighbors;
    S.n_waves = (n + WAVE - 1) / WAVE;
    vs_ctx* c = ix->ctx;
    // carried labels: from the index's own label -> bit table when it has one, else from the CSR's values
    std::vector<uint8_t> present(65536, 0);
    if (ix->label_mask && ix->label_bit) {
        S.own_bit.resize(65536);
        VS_TRY(vs_dev_download(c, S.own_bit.data(), ix->label_bit, 65536));
        for (uint32_t v = 0; v < 65536; ++v) present[v] = S.own_bit[v] != 0xFF;
    } else {
        uint32_t nv = 0;
        VS_TRY(vs_dev_download(c, &nv, ix->label_off + n, 4));
        std::vector<int16_t> val(std::max<uint32_t>(nv, 1));
        if (nv) VS_TRY(vs_dev_download(c, val.data(), ix->label_val, (size_t)nv * 2));
        for (uint32_t j = 0; j < nv; ++j) present[(uint16_t)val[j]] = 1;
    }
    std::map<int16_t, uint32_t> start_of;
    const uint32_t ns = ix->d.n_label_starts;
    std::vector<int16_t> sl(ns);
    std::vector<uint32_t> sn(ns), starts;
    if (ns) {
        VS_TRY(vs_dev_download(c, sl.data(), ix->ls_labels, (size_t)ns * 2));
        VS_TRY(vs_dev_download(c, sn.data(), ix->ls_nodes, (size_t)ns * 4));
        for (uint32_t t = 0; t < ns; ++t) {
            VS_REQUIRE(sn[t] < n, "%s: start node %u of label %d in an index of %u nodes", what, sn[t], (int)sl[t], n);
            start_of.emplace(sl[t], sn[t]);
        }
    }
    VS_REQUIRE(ix->d.default_start < n, "%s: default start node %u of an index of %u nodes", what, ix->d.default_start, n);
    VS_TRY(collect_start_nodes(ix, what, &starts, sn.data()));
    for (int v = -32768; v <= 32767; ++v) {
        const bool car = present[(uint16_t)(int16_t)v] != 0;
        const auto it = start_of.find((int16_t)v);
        if (!car && it == start_of.end()) continue;
        S.labels.push_back((int16_t)v);
        S.carried.push_back(car);
        S.lstart.push_back(it == start_of.end() ? VS_INVALID_NODE : it->second);
        S.without_start += car && it == start_of.end();
    }
    S.ngroups = ((uint32_t)S.labels.size() + 63) / 64;
    S.own_masks = S.ngroups <= 1 && !S.own_bit.empty();
    VS_TRY(S.tm.start(sc, c->profiling, ms, what));
    VS_TRY(sc.alloc(&S.cls, n, what));
    VS_TRY(sc.alloc(&S.flag, n, what));
    VS_TRY(sc.alloc(&S.any, n, what));
    VS_TRY(sc.alloc(&S.reach, (size_t)n * 8, what));
    VS_TRY(sc.alloc(&S.fresh[0], (size_t)n * 8, what));
    VS_TRY(sc.alloc(&S.fresh[1], (size_t)n * 8, what));
    VS_TRY(sc.alloc(&S.need, (size_t)n * 8, what));
    VS_TRY(sc.alloc(&S.wave, ((size_t)S.n_waves + 1) * 4, what));
    VS_TRY(sc.alloc(&S.seed_nodes, 64 * 4, what));
    VS_TRY(sc.alloc(&S.seed_bits, 64 * 8, what));
    VS_TRY(sc.alloc(&S.bitcnt, 128 * 4, what));
    VS_TRY(sc.alloc(&S.changed, 4, what));
    VS_TRY(sc.alloc(&S.cnt, LR_N * 8, what));
    VS_TRY(sc.alloc(&S.cons_cnt, CN_N * 8, what));
    VS_TRY(sc.alloc(&S.d_starts, starts.size() * 4, what));
    VS_HIP(hipMemsetAsync(S.cnt, 0, LR_N * 8, S.st));
    VS_HIP(hipMemsetAsync(S.cons_cnt, 0, CN_N * 8, S.st));
    if (!S.own_masks) {
        VS_TRY(sc.alloc(&S.mask_buf, (size_t)n * 8, what));
        VS_TRY(sc.alloc(&S.d_table, 65536, what));
        S.table.resize(65536);
    }
    if (repair) {
        VS_TRY(sc.alloc(&S.rowchg, n, what));
        VS_TRY(sc.alloc(&S.strong, (size_t)n * 4, what));
        VS_TRY(sc.alloc(&S.claim, (size_t)n * 4, what));
        VS_TRY(sc.alloc(&S.mark, (size_t)n + 8, what));
        VS_HIP(hipMemsetAsync(S.rowchg, 0, n, S.st));
    }
    // the node classes of section 6d
    VS_HIP(hipMemcpyAsync(S.d_starts, starts.data(), starts.size() * 4, hipMemcpyHostToDevice, S.st));
    hipLaunchKernelGGL(k_cons_classify, dim3((n + 255) / 256), dim3(256), 0, S.st, (const uint64_t*)ix->tids, (const uint32_t*)nullptr, n, S.cls,
                       S.cons_cnt);
    VS_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cons_keep_starts, dim3(((uint32_t)starts.size() + 255) / 256), dim3(256), 0, S.st, (const uint32_t*)S.d_starts,
                       (uint32_t)starts.size(), S.cls, S.cons_cnt);
    VS_HIP(hipGetLastError());
    VS_HIP(hipStreamSynchronize(S.st));  // (starts is a local)
    return VS_OK;
}

// steps 1 of a group: masks, reach to its fixed point, need, the per-bit counters and the number of lost nodes (flag[] and the
// scanned wave counts are left for the scatter)
static int lr_group_reach(LrState& S, uint32_t g, bool collect_any, uint32_t* nlost, uint32_t* h_bitcnt /*[128]*/) {
    vs_index* ix = S.ix;
    const uint32_t n = S.n, R = S.R;
    const uint32_t lo = g * 64, hi = std::min<uint32_t>(lo + 64, (uint32_t)S.labels.size());
    std::map<uint32_t, uint64_t> seeds;
    S.jmask = 0;
    if (!S.own_masks) std::fill(S.table.begin(), S.table.end(), (uint8_t)0xFF);
    for (uint32_t li = lo; li < hi; ++li) {
        const uint8_t b = !S.carried[li] ? (uint8_t)0xFF : S.own_masks ? S.own_bit[(uint16_t)S.labels[li]] : (uint8_t)(li - lo);
        S.bit[li - lo] = b;
        if (b == 0xFF) continue;
        if (!S.own_masks) S.table[(uint16_t)S.labels[li]] = b;
        if (S.lstart[li] != VS_INVALID_NODE) {
            S.jmask |= 1ull << b;
            seeds[S.lstart[li]] |= 1ull << b;
        }
    }
    if (S.own_masks) {
        S.mask = ix->label_mask;
    } else {
        VS_HIP(hipMemcpyAsync(S.d_table, S.table.data(), 65536, hipMemcpyHostToDevice, S.st));
        hipLaunchKernelGGL(k_lr_group_masks, dim3((n + 255) / 256), dim3(256), 0, S.st, (const uint32_t*)ix->label_off,
                           (const int16_t*)ix->label_val, n, (const uint8_t*)S.d_table, S.mask_buf);
        VS_HIP(hipGetLastError());
        S.mask = S.mask_buf;
    }
    VS_HIP(hipMemsetAsync(S.reach, 0, (size_t)n * 8, S.st));
    VS_HIP(hipMemsetAsync(S.fresh[0], 0, (size_t)n * 8, S.st));
    VS_HIP(hipMemsetAsync(S.fresh[1], 0, (size_t)n * 8, S.st));
    std::vector<uint32_t> sn;
    std::vector<uint64_t> sb;
    for (const auto& kv : seeds) {
        sn.push_back(kv.first);
        sb.push_back(kv.second);
    }
    if (!sn.empty()) {
        VS_HIP(hipMemcpyAsync(S.seed_nodes, sn.data(), sn.size() * 4, hipMemcpyHostToDevice, S.st));
        VS_HIP(hipMemcpyAsync(S.seed_bits, sb.data(), sb.size() * 8, hipMemcpyHostToDevice, S.st));
        hipLaunchKernelGGL(k_lr_seed, dim3(1), dim3(64), 0, S.st, (const uint32_t*)S.seed_nodes, (const uint64_t*)S.seed_bits, (uint32_t)sn.size(),
                           S.reach, S.fresh[0]);
        VS_HIP(hipGetLastError());
        VS_HIP(hipStreamSynchronize(S.st));  // (sn / sb are locals)
        const size_t cells = (size_t)n * R;
        S.tm.tick();
        int in = 0;
        for (uint64_t it = 0;; ++it) {  // no level cap: a rare label's chain is deep
            if (it > n) {  // (every sweep that changes something lengthens some label's chain, and a chain has at most n nodes)
                vs_set_error("%s: the reach sweeps did not settle after %u sweeps", S.what, n);
                return VS_ERR_CAPACITY;
            }
            uint32_t changed = 0;
            VS_HIP(hipMemsetAsync(S.changed, 0, 4, S.st));
            hipLaunchKernelGGL(k_lr_sweep, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, S.st, (const uint32_t*)ix->nbrs, ix->nbr_stride, R, n,
                               S.mask, S.jmask, S.reach, (const uint64_t*)S.fresh[in], S.fresh[in ^ 1], S.changed);
            VS_HIP(hipGetLastError());
            VS_HIP(hipMemcpyAsync(&changed, S.changed, 4, hipMemcpyDeviceToHost, S.st));
            VS_HIP(hipMemsetAsync(S.fresh[in], 0, (size_t)n * 8, S.st));
            VS_HIP(hipStreamSynchronize(S.st));
            S.sweeps++;
            in ^= 1;
            if (!changed) break;
        }
        S.tm.tock(0);
    }
    VS_HIP(hipMemsetAsync(S.bitcnt, 0, 128 * 4, S.st));
    const dim3 ngrid((n + 255) / 256);
    hipLaunchKernelGGL(k_lr_need, ngrid, dim3(256), 0, S.st, (const uint8_t*)S.cls, S.mask, S.jmask, (const uint64_t*)S.reach, n, S.need, S.flag,
                       collect_any ? S.any : (uint8_t*)nullptr, S.bitcnt);
    VS_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cons_work_count, ngrid, dim3(256), 0, S.st, (const uint8_t*)S.flag, n, S.wave);
    VS_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cons_work_scan, dim3(1), dim3(256), 0, S.st, S.wave, S.n_waves);
    VS_HIP(hipGetLastError());
    // the one small copy per group: how many lost, and the per-bit counters
    VS_HIP(hipMemcpyAsync(nlost, S.wave + S.n_waves, 4, hipMemcpyDeviceToHost, S.st));
    VS_HIP(hipMemcpyAsync(h_bitcnt, S.bitcnt, 128 * 4, hipMemcpyDeviceToHost, S.st));
    VS_HIP(hipStreamSynchronize(S.st));
    return VS_OK;
}

static int lr_count_flags(LrState& S, const uint8_t* flag, uint32_t want, const uint8_t* cls, uint32_t* out) {
    unsigned long long v = 0;
    VS_HIP(hipMemsetAsync(S.cnt + LR_COUNT, 0, 8, S.st));
    hipLaunchKernelGGL(k_lr_count, dim3((S.n + 255) / 256), dim3(256), 0, S.st, flag, want, cls, S.n, S.cnt + LR_COUNT);
    VS_HIP(hipGetLastError());
    VS_HIP(hipMemcpyAsync(&v, S.cnt + LR_COUNT, 8, hipMemcpyDeviceToHost, S.st));
    VS_HIP(hipStreamSynchronize(S.st));
    *out = (uint32_t)v;
    return VS_OK;
}

// the audit over all groups on the graph as it stands; carriers / lost: per label of S.labels, or null
static int lr_audit(LrState& S, uint64_t* pairs, uint32_t* nodes, uint32_t* carriers, uint32_t* lost) {
    *pairs = 0;
    VS_HIP(hipMemsetAsync(S.any, 0, S.n, S.st));
    for (uint32_t g = 0; g < S.ngroups; ++g) {
        uint32_t nl = 0, bc[128];
        VS_TRY(lr_group_reach(S, g, true, &nl, bc));
        for (uint32_t li = g * 64; li < std::min<size_t>((size_t)g * 64 + 64, S.labels.size()); ++li) {
            const uint8_t b = S.bit[li - g * 64];
            if (carriers) carriers[li] = b == 0xFF ? 0u : bc[b];
            if (lost) lost[li] = b == 0xFF ? 0u : bc[64 + b];
            if (b != 0xFF) *pairs += bc[64 + b];
        }
    }
    return lr_count_flags(S, S.any, 1, nullptr, nodes);
}

static int label_reach_impl(vs_index* ix, vs_label_reach_stats* out, int16_t* out_labels, uint32_t* out_carriers, uint32_t* out_lost,
                            uint32_t cap, uint8_t* out_node_lost) {
    const char* what = "vs_index_label_reach";
    VS_REQUIRE(ix, "%s: index is NULL", what);
    if (out) memset(out, 0, sizeof(*out));
    VS_REQUIRE(ix->label_off && ix->label_val, "%s: the index has no label sets", what);
    VS_REQUIRE(ix->nbrs && ix->tids, "%s: the index has no neighbor lists", what);
    VS_TRY(require_no_batch(ix, what));
    vs_label_reach_stats s{};
    if (ix->d.n == 0 || ix->d.default_start == VS_INVALID_NODE) {
        if (out) *out = s;
        return VS_OK;
    }
    VS_HIP(hipSetDevice(ix->ctx->device));
    LrState S;
    std::vector<uint32_t> carriers, lost;
    {
        DevScope sc(ix->ctx->stream);
        double audit_ms[4] = {0, 0, 0, 0};  // (vs_index_label_repair_kernel_ms reports the repair's kernels only)
        VS_TRY(lr_init(S, ix, sc, what, false, audit_ms));
        carriers.assign(S.labels.size(), 0);
        lost.assign(S.labels.size(), 0);
        VS_TRY(lr_audit(S, &s.lost_pairs, &s.lost_nodes, carriers.data(), lost.data()));
        if (out_node_lost) VS_TRY(vs_dev_download(ix->ctx, out_node_lost, S.any, S.n));
    }
    s.labels = (uint32_t)S.labels.size();
    s.labels_without_start = S.without_start;
    s.sweeps = S.sweeps;
    for (uint32_t li = 0; li < std::min<uint32_t>(cap, s.labels); ++li) {
        if (out_labels) out_labels[li] = S.labels[li];
        if (out_carriers) out_carriers[li] = carriers[li];
        if (out_lost) out_lost[li] = lost[li];
    }
    if (out) *out = s;
    return VS_OK;
}
extern "C" int vs_index_label_reach(vs_index* ix, vs_label_reach_stats* out, int16_t* out_labels, uint32_t* out_carriers, uint32_t* out_lost,
                                    uint32_t cap, uint8_t* out_node_lost) {
    return vs_guard("vs_index_label_reach", [&] { return label_reach_impl(ix, out, out_labels, out_carriers, out_lost, cap, out_node_lost); });
}

static int repair_labels_impl(vs_index* ix, uint32_t max_rounds, uint32_t flags, vs_label_repair_stats* out) {
    const char* what = "vs_index_repair_labels";
    VS_REQUIRE(ix, "%s: index is NULL", what);
    if (out) memset(out, 0, sizeof(*out));
    VS_REQUIRE_OWNER(ix, what);
    VS_REQUIRE_NO_VIEWS(ix, what);
    VS_REQUIRE(ix->d.storage_type == VS_STORAGE_SBQ, "%s: plain storage is not supported (memory_optimized indexes only)", what);
    VS_REQUIRE(ix->codes && ix->nbrs && ix->tids, "%s: needs codes, neighbor lists and heap tids on the device", what);
    VS_REQUIRE(ix->label_off && ix->label_val, "%s: the index has no label sets", what);
    VS_REQUIRE(flags == 0, "%s: unknown flags 0x%x", what, flags);
    VS_REQUIRE(max_rounds <= 64, "%s: max_rounds %u outside [0,64]", what, max_rounds);
    if (max_rounds == 0) max_rounds = 16;
    VS_TRY(require_no_batch(ix, what));
    VS_TRY(require_no_writer(ix, what, WRITER_ROWS_MIX));
    vs_label_repair_stats s{};
    if (ix->d.n == 0 || ix->d.default_start == VS_INVALID_NODE) {
        if (out) *out = s;
        return VS_OK;
    }
    VS_HIP(hipSetDevice(ix->ctx->device));
    LrState S;
    DevScope sc(ix->ctx->stream);
    const uint32_t n = ix->d.n, R = ix->d.num_neighbors;
    bool wrote = false;
    auto run = [&]() -> int {  // (the stats are filled from what it got to, whatever it returns)
        VS_TRY(lr_init(S, ix, sc, what, true, ix->label_repair_ms));
        hipStream_t st = S.st;
        VS_TRY(lr_audit(S, &s.lost_pairs_before, &s.lost_nodes_before, nullptr, nullptr));
        s.lost_pairs_after = s.lost_pairs_before;
        s.lost_nodes_after = s.lost_nodes_before;
        const size_t cells = (size_t)n * R;
        const dim3 cgrid((unsigned)((cells + 255) / 256)), ngrid((n + 255) / 256);
        for (uint32_t round = 0; s.lost_pairs_before && round < max_rounds; ++round) {
            bool any_lost = false;
            for (uint32_t g = 0; g < S.ngroups; ++g) {  // a later group sees what an earlier one wrote
                uint32_t nl = 0, bc[128];
                VS_TRY(lr_group_reach(S, g, false, &nl, bc));
                if (!nl) continue;
                any_lost = true;
                if (nl > S.lost_cap) {
                    sc.free(S.lost);
                    sc.free(S.keys);
                    S.lost_cap = 0;
                    VS_TRY(sc.alloc(&S.lost, (size_t)nl * 4, what));
                    VS_TRY(sc.alloc(&S.keys, (size_t)nl * 8, what));
                    S.lost_cap = nl;
                }
                hipLaunchKernelGGL(k_cons_work_scatter, ngrid, dim3(256), 0, st, (const uint8_t*)S.flag, n, (const uint32_t*)S.wave, S.lost);
                VS_HIP(hipGetLastError());
                S.tm.tick();
                VS_HIP(hipMemsetAsync(S.strong, 0, (size_t)n * 4, st));
                hipLaunchKernelGGL(k_lr_strong, cgrid, dim3(256), 0, st, (const uint32_t*)ix->nbrs, ix->nbr_stride, R, n, (const uint8_t*)S.cls, S.mask,
                                   S.jmask, (const uint64_t*)S.reach, S.strong);
                VS_HIP(hipGetLastError());
                S.tm.tock(1);
                S.tm.tick();
                VS_TRY(launch_nearest_masked(ix, S.lost, nl, S.need, true, S.reach, S.cls, S.keys, &s.source_tiles));
                S.tm.tock(2);
                S.tm.tick();
                VS_HIP(hipMemsetAsync(S.claim, 0xFF, (size_t)n * 4, st));
                hipLaunchKernelGGL(k_lr_claim, dim3((nl + 255) / 256), dim3(256), 0, st, (const uint32_t*)S.lost, nl,
                                   (const unsigned long long*)S.keys, S.claim);
                VS_HIP(hipGetLastError());
                ix->nbr_mask_valid = false;  // (the neighbor lists are about to change: what was derived from them is stale)
                wrote = true;
                hipLaunchKernelGGL(k_lr_apply, dim3(nl), dim3(WAVE), 0, st, (const uint32_t*)S.lost, nl, (const unsigned long long*)S.keys,
                                   (const uint32_t*)S.claim, ix->nbrs, ix->nbr_stride, R, n, (const uint8_t*)S.cls, S.mask, S.jmask,
                                   (const uint64_t*)S.reach, (const uint32_t*)S.strong, S.rowchg, S.cnt);
                VS_HIP(hipGetLastError());
                S.tm.tock(3);
            }
            if (!any_lost) break;
            s.rounds++;
        }
        if (s.rounds) VS_TRY(lr_audit(S, &s.lost_pairs_after, &s.lost_nodes_after, nullptr, nullptr));
        // one unfiltered sweep from the default start node: no live row may have lost its way in
        bool converged = false;
        VS_TRY(reach_from_default_start(ix, S.mark, &converged));
        s.unreachable_live = 0xFFFFFFFFu;
        if (converged) VS_TRY(lr_count_flags(S, S.mark, 0, S.cls, &s.unreachable_live));
        uint32_t rc_rows = 0;
        VS_TRY(lr_count_flags(S, S.rowchg, 1, nullptr, &rc_rows));
        s.rows_changed = rc_rows;
        return VS_OK;
    };
    int rc = run();
    (void)hipStreamSynchronize(sc.st);
    sc.drained();
    unsigned long long h[LR_N] = {0};
    if (S.cnt) (void)hipMemcpy(h, S.cnt, sizeof h, hipMemcpyDeviceToHost);  // (the placement counters as far as the call got)
    sc.close();
    s.placed_free = h[LR_PLACED_FREE];
    s.placed_over_dropped = h[LR_PLACED_DROPPED];
    s.placed_victim = h[LR_PLACED_VICTIM];
    s.blocked = h[LR_BLOCKED];
    s.contended = h[LR_CONTENDED];
    s.sweeps = S.sweeps;
    s.labels_without_start = S.without_start;
    if (out) *out = s;
    if (rc == VS_OK && wrote) rc = vs_validate_graph(ix);
    return rc;
}
extern "C" int vs_index_repair_labels(vs_index* ix, uint32_t max_rounds, uint32_t flags, vs_label_repair_stats* out) {
    return vs_guard("vs_index_repair_labels", [&] { return repair_labels_impl(ix, max_rounds, flags, out); });
}
extern "C" int vs_index_label_repair_kernel_ms(vs_index* ix, double* ms /*[4]*/, int reset) {
    return read_kernel_ms("vs_index_label_repair_kernel_ms", ix, ix ? ix->label_repair_ms : nullptr, 4, ms, reset);
}

// ---- vs_nearest_masked: k_nearest_masked on its own -------------------------------------------------------------------------
static int nearest_masked_impl(vs_index* ix, const uint32_t* nodes, const uint64_t* want, uint32_t nq, const uint64_t* node_bits,
                               const uint8_t* skip, uint32_t* out_ids, uint32_t* out_ham) {
    const char* what = "vs_nearest_masked";
    VS_REQUIRE(ix && (nq == 0 || (nodes && want && node_bits && out_ids)), "%s: bad args", what);
    VS_REQUIRE(ix->d.storage_type == VS_STORAGE_SBQ && ix->codes, "%s: needs SBQ codes on the device", what);
    if (nq == 0) return VS_OK;
    const uint32_t n = ix->d.n;
    for (uint32_t q = 0; q < nq; ++q) VS_REQUIRE(nodes[q] < n, "%s: query %u names node %u of an index of %u nodes", what, q, nodes[q], n);
    vs_ctx* c = ix->ctx;
    VS_HIP(hipSetDevice(c->device));
    uint32_t* d_nodes = nullptr;
    uint64_t *d_want = nullptr, *d_bits = nullptr;
    uint8_t* d_skip = nullptr;
    unsigned long long* d_keys = nullptr;
    std::vector<unsigned long long> keys(nq);
    {
        DevScope sc(c->stream);
        VS_TRY(sc.alloc(&d_nodes, (size_t)nq * 4, what));
        VS_TRY(sc.alloc(&d_want, (size_t)nq * 8, what));
        VS_TRY(sc.alloc(&d_bits, (size_t)n * 8, what));
        VS_TRY(sc.alloc(&d_keys, (size_t)nq * 8, what));
        VS_TRY(vs_dev_upload(c, d_nodes, nodes, (size_t)nq * 4));
        VS_TRY(vs_dev_upload(c, d_want, want, (size_t)nq * 8));
        VS_TRY(vs_dev_upload(c, d_bits, node_bits, (size_t)n * 8));
        if (skip) {
            std::vector<uint8_t> sk(n);
            for (uint32_t i = 0; i < n; ++i) sk[i] = skip[i] != 0;
            VS_TRY(sc.alloc(&d_skip, n, what));
            VS_TRY(vs_dev_upload(c, d_skip, sk.data(), n));
        }
        VS_TRY(launch_nearest_masked(ix, d_nodes, nq, d_want, false, d_bits, d_skip, d_keys));
        VS_TRY(vs_dev_download(c, keys.data(), d_keys, (size_t)nq * 8));
    }
    for (uint32_t q = 0; q < nq; ++q) {
        out_ids[q] = keys[q] == ~0ull ? VS_INVALID_NODE : (uint32_t)keys[q];
        if (out_ham) out_ham[q] = keys[q] == ~0ull ? 0xFFFFFFFFu : (uint32_t)(keys[q] >> 32);
    }
    return VS_OK;
}
extern "C" int vs_nearest_masked(vs_index* ix, const uint32_t* nodes, const uint64_t* want, uint32_t nq, const uint64_t* node_bits,
                                 const uint8_t* skip, uint32_t* out_ids, uint32_t* out_ham) {
    return vs_guard("vs_nearest_masked", [&] { return nearest_masked_impl(ix, nodes, want, nq, node_bits, skip, out_ids, out_ham); });
}
