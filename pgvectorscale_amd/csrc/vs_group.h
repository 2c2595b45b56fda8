// vs_group.h — the rescore window under a GROUP rule (a part of vs_kernels.hip kept in a file of its own): the kernels of
// vs_search_batch_grouped (vs_qual.h; the contract is the header's, include/vsgpu.h "grouped scans") and their launches.
//
// The window pops up to P rows per scan, as the qualified one does (k_rerank_window_qual / k_resort_qual), but whether a popped row is
// kept depends on the rows kept before it: a row that passes the scan's qualifier is kept iff its group G[node] is VS_GROUP_NONE or
// fewer than per_group of the rows kept so far carry the same value.  The rule needs, per pop, the group of the popped node and a count
// over up to k kept groups; both are arranged so that the rule adds no global read to the serial selection loop of a scan:
//   * the group of every stream row is gathered into LDS (sg[]) by all 256 threads at the head of the rerank pass, a thread per row and
//     every row's two loads (stream id -> G[id]) in flight together, beside the query's own loads and 4 bytes against a row of
//     4 dim_full bytes — the selection loop would otherwise wait for those two dependent global round trips on every pop.  (Loading
//     G[id] in the lane that stores the row's distance holds a register across the row's dot product: under the 80 registers of
//     __launch_bounds__(256, 6) that came out as 2 spilled registers and 12 bytes of scratch, so the gather got a loop of its own);
//   * the groups of the kept rows sit in LDS (kg[]), kept row r written and read by lane r & 63 ONLY: the count is a compare per lane,
//     a ballot and a popcount per 64 kept rows, no lane ever reads what another lane wrote, and no lane order shows.
// The kernels an unqualified or a qualified batch runs are not touched.
#pragma once

// rows kept so far in group g, as far as the rule needs to know: true iff fewer than per_group.  kg[r] for r < kept is read by lane
// r & 63 (its writer).  Wave-uniform arguments, wave-uniform result; every lane of the wave takes part.
__device__ __forceinline__ bool group_has_room(const uint32_t* kg, uint32_t kept, uint32_t g, uint32_t lane, uint32_t per_group) {
    uint32_t c = 0;
    for (uint32_t b = 0; b < kept && c < per_group; b += WAVE) {
        const uint32_t r = b + lane;
        c += (uint32_t)__popcll(__ballot(r < kept && kg[r] == g));
    }
    return c < per_group;
}

// One pop of window_replay_until as a step that can be taken again: the pushes the reference makes before a pop (while the heap holds
// fewer than `rescore` entries and the stream has rows), then the pop.  len / pos: entries in the heap / stream rows pushed, 0 at the
// start.  false: the window is dry (amgettuple returns None).  The same heap code, so the same layout and the same row on ties.
__device__ __forceinline__ bool window_pop(uint64_t* h, const float* sd, uint32_t n, uint32_t rescore, uint32_t& len, uint32_t& pos, uint32_t* sp) {
    auto kof = [](uint64_t e) { return (int32_t)(uint32_t)(e >> 32); };
    auto sift_up = [&](uint32_t p, uint64_t elem) {
        while (p > 0) {
            uint32_t parent = (p - 1) >> 1;
            uint64_t pe = h[parent];
            if (kof(pe) <= kof(elem)) break;
            h[p] = pe;
            p = parent;
        }
        h[p] = elem;
    };
    while (len < rescore && pos < n) {
        uint64_t e = ((uint64_t)(uint32_t)total_key(sd[pos]) << 32) | pos;
        uint32_t p = len++;
        sift_up(p, e);
        ++pos;
    }
    if (len == 0) return false;
    uint64_t item = h[--len];
    uint64_t top = item;
    if (len > 0) {
        top = h[0];
        uint32_t end = len, p = 0, child = 1;
        uint32_t lim = end >= 2 ? end - 2 : 0;
        while (child <= lim) {
            uint64_t le = h[child], ri = h[child + 1];
            uint32_t pick = (kof(ri) <= kof(le)) ? 1u : 0u;
            child += pick;
            h[p] = pick ? ri : le;
            p = child;
            child = 2 * p + 1;
        }
        if (child == end - 1) {
            h[p] = h[child];
            p = child;
        }
        sift_up(p, item);
    }
    *sp = (uint32_t)top;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------
// k_rerank_window under a group rule: one workgroup of 4 waves per scan, k_rerank_window's rerank pass and ownership, the groups of
// the stream rows gathered beside it.  Wave 0 then selects as k_rerank_window_qual does — the popped position is known to every lane —
// and decides wave-uniformly: the qualifier bit is read as there (only where the scan names a qualifier), the group comes from sg[]
// and the count from kg[].  kept and pops are wave-uniform registers of wave 0.  A minimum held by two live entries
// sends the scan to the serial replay from the start, where lane 0 applies the same rule alone (it then writes and reads kg[] itself).
// LDS: k_rerank_window's, with [M] u32 groups between the distances and the positions and [k] u32 kept groups at the end.
// ---------------------------------------------------------------------------------------------------------------
__host__ __device__ static inline size_t rerank_window_grouped_lds(uint32_t vec_stride, uint32_t M, uint32_t rescore, uint32_t k) {
    return rerank_window_lds(vec_stride, M, rescore, k) + (size_t)M * 4 + (size_t)k * 4;
}

__global__ __launch_bounds__(256, 6) void k_rerank_window_grouped(const float* __restrict__ vecs, uint32_t vec_stride, uint32_t dim_full,
                                                               const float* __restrict__ vnorm, uint32_t distance_type,
                                                               const float* __restrict__ q_full, const uint32_t* __restrict__ stream,
                                                               const uint32_t* __restrict__ cnt, uint32_t M, uint32_t rescore, uint32_t k,
                                                               uint32_t nq, const uint64_t* __restrict__ tids, uint32_t* __restrict__ out_ids,
                                                               uint64_t* __restrict__ out_tids, float* __restrict__ out_dist, uint32_t mode,
                                                               const uint32_t* __restrict__ perm, uint32_t deal, GroupLaunch gl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* qv = reinterpret_cast<float*>(smem);
    uint64_t* hh = reinterpret_cast<uint64_t*>(qv + vec_stride);
    float* sd = reinterpret_cast<float*>(hh + rescore);
    uint32_t* sg = reinterpret_cast<uint32_t*>(sd + M);
    uint32_t* sps = sg + M;
    uint32_t* kg = sps + k + 1;
    const uint32_t slot = rerank_slot(blockIdx.x, nq, deal);
    if (slot >= nq) return;
    const uint32_t w = perm ? perm[slot] : slot;
    const uint32_t n = min(cnt[w], M);
    const uint32_t* sid = stream + (size_t)w * M;
    // the groups of the scan's stream rows, a thread per row: issued with the query's loads, back before the first row's distance is
    for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) {
        const uint32_t id = sid[j];
        sg[j] = id != VS_INVALID_NODE ? gl.groups[id] : VS_GROUP_NONE;
    }
    for (uint32_t i = threadIdx.x; i < vec_stride; i += blockDim.x) qv[i] = q_full[(size_t)w * vec_stride + i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l8 = lane & 7, grp = lane >> 3;
    const uint32_t steps = dim_full / 32;
    for (uint32_t base = 0; base < n; base += 32) {
        const uint32_t j = base + (uint32_t)(wave * 8 + grp);
        bool valid = j < n;
        const uint32_t id = valid ? sid[j] : VS_INVALID_NODE;
        if (id == VS_INVALID_NODE) valid = false;
        const float* row = vecs + (size_t)(valid ? id : 0) * vec_stride;
        float s = 0.0f;
        if (valid && distance_type == VS_COSINE) s = vnorm[id];
        const float r = rerank_row_dist(row, qv, s, distance_type, steps, dim_full, lane, l8, valid);
        if (j < n && l8 == 0) sd[j] = valid ? r : __int_as_float(0x7fc00000);
    }
    __syncthreads();
    const QualLaunch& ql = gl.ql;
    const uint32_t q = ql.map ? ql.map[w] : ql.q_base + w;
    const uint32_t P = ql.pops, per_group = gl.per_group;
    uint32_t kept = 0, pops = 0;  // (wave-uniform in wave 0, which is the only one to use them)
    if (wave == 0) {
        const uint64_t* bits = qual_bits_of(ql, q);
        bool replay = mode == 2;
        if (!replay) {
            uint64_t taken = 0;  // bit j: this lane's position lane + 64 j has been popped (M <= 4096)
            for (uint32_t i = 0; i < P && kept < k; ++i) {
                const uint32_t limit = min(rescore + i, n);
                if (limit <= i) break;  // the heap is empty
                const int64_t none = 0x7fffffffffffffffll;
                int64_t best = none;
                uint32_t bj = 0, c = 0;
                for (uint32_t j = 0, p = (uint32_t)lane; p < limit; ++j, p += 64) {
                    if ((taken >> j) & 1ull) continue;
                    const int64_t key = total_key(sd[p]);
                    if (key < best) {
                        best = key;
                        bj = j;
                        c = 1;
                    } else if (key == best) {
                        ++c;
                    }
                }
                int64_t wbest = best;
                for (int m = 1; m < WAVE; m <<= 1) {
                    const int64_t o = __shfl_xor(wbest, m, WAVE);
                    wbest = o < wbest ? o : wbest;
                }
                const bool mine = best == wbest && best != none;
                const uint64_t holders = __ballot(mine);
                if (__popcll(holders) != 1 || __ballot(mine && c > 1) != 0) {
                    replay = true;
                    break;
                }
                if (mine) taken |= 1ull << bj;
                const int holder = (int)__builtin_ctzll(holders);
                const uint32_t sp = (uint32_t)holder + 64u * (uint32_t)__shfl((int)bj, holder, WAVE);
                ++pops;
                if (bits && !qual_passes(bits, sid[sp])) continue;  // (wave-uniform)
                const uint32_t g = sg[sp];
                if (g != VS_GROUP_NONE && !group_has_room(kg, kept, g, (uint32_t)lane, per_group)) continue;
                if ((uint32_t)lane == (kept & 63u)) kg[kept] = g;
                if (lane == 0) sps[kept] = sp;
                ++kept;
            }
        }
        if (replay) {  // (from the start: rows kept before the tie are produced again)
            kept = 0;
            uint32_t kk = 0, pp = 0;
            if (lane == 0) {
                pp = window_replay_until(hh, sd, n, rescore, P, [&](uint32_t sp) {
                    if (qual_passes(bits, sid[sp])) {
                        const uint32_t g = sg[sp];
                        uint32_t c = 0;
                        if (g != VS_GROUP_NONE)
                            for (uint32_t r = 0; r < kk && c < per_group; ++r) c += kg[r] == g ? 1u : 0u;
                        if (c < per_group) {
                            kg[kk] = g;
                            sps[kk++] = sp;
                        }
                    }
                    return kk == k;
                });
            }
            kept = (uint32_t)__shfl((int)kk, 0, WAVE);
            pops = (uint32_t)__shfl((int)pp, 0, WAVE);
        }
    }
    __syncthreads();  // (the positions lane 0 stored, for all of wave 0)
    if (wave != 0) return;
    const size_t o = (size_t)q * k;
    for (uint32_t j = (uint32_t)lane; j < k; j += WAVE) {
        uint32_t id = VS_INVALID_NODE;
        uint64_t tid = 0;
        float d = __int_as_float(0x7fc00000);
        if (j < kept) {
            const uint32_t sp = sps[j];
            id = sid[sp];
            if (out_tids) tid = tids[id];
            d = sd[sp];
        }
        out_ids[o + j] = id;
        if (out_tids) out_tids[o + j] = tid;
        if (out_dist) out_dist[o + j] = d;
    }
    if (lane == 0) {
        ql.out_rows[q] = kept;
        ql.out_pops[q] = pops;
        ql.out_state[q] = qual_state(kept, k, pops, P, ql.final);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// k_resort under a group rule: ONE WAVE per scan of the launch (the windows the fused kernel does not take, VS_RERANK_FUSED=0, and
// rescore == 0, where the stream order is the output order).  Lane 0 steps the heap (window_pop on the scan's strip of heap_ws) and
// hands the popped position to the wave; every lane then reads the row's id, qualifier bit and group (one address: one request) and
// the wave counts the kept rows of that group in its LDS strip kg[k] as the fused kernel does.  One thread per scan, k_resort_qual's
// shape, would walk up to k kept groups per pop alone.  Lane 0 writes the rows.  As in k_resort_qual, a stream row below cnt[w] is a
// node id, never VS_INVALID_NODE (the search kernels count the rows they wrote), so the popped id indexes G, tids and the bitmap unguarded.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WAVE) void k_resort_grouped(uint32_t nq, uint32_t M, uint32_t rescore, uint32_t k, const uint32_t* __restrict__ stream,
                                                         const uint32_t* __restrict__ cnt, const float* __restrict__ dist,
                                                         const uint64_t* __restrict__ tids, uint64_t* __restrict__ heap_ws,
                                                         uint32_t* __restrict__ out_ids, uint64_t* __restrict__ out_tids, float* __restrict__ out_dist,
                                                         const uint32_t* __restrict__ plain_keys, GroupLaunch gl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* kg = reinterpret_cast<uint32_t*>(smem);  // [k]
    const uint32_t w = blockIdx.x, lane = threadIdx.x;
    if (w >= nq) return;
    const QualLaunch& ql = gl.ql;
    const uint32_t q = ql.map ? ql.map[w] : ql.q_base + w;
    const uint64_t* bits = qual_bits_of(ql, q);
    const uint32_t P = ql.pops, per_group = gl.per_group;
    const uint32_t n = min(cnt[w], M);
    const uint32_t* sid = stream + (size_t)w * M;
    const float* sd = dist ? dist + (size_t)w * M : nullptr;
    uint64_t* h = heap_ws + (size_t)w * rescore;
    const size_t o = (size_t)q * k;
    uint32_t kept = 0, pops = 0, len = 0, pos = 0;  // (kept, pops wave-uniform; len, pos lane 0's)
    while (pops < P && kept < k) {
        uint32_t sp = VS_INVALID_NODE;
        if (rescore == 0) {
            if (pops < n) sp = pops;
        } else {
            if (lane == 0 && !window_pop(h, sd, n, rescore, len, pos, &sp)) sp = VS_INVALID_NODE;
            sp = (uint32_t)__shfl((int)sp, 0, WAVE);
        }
        if (sp == VS_INVALID_NODE) break;  // the scan has ended
        ++pops;
        const uint32_t id = sid[sp];
        if (!qual_passes(bits, id)) continue;
        const uint32_t g = gl.groups[id];
        if (g != VS_GROUP_NONE && !group_has_room(kg, kept, g, lane, per_group)) continue;
        if (lane == (kept & 63u)) kg[kept] = g;
        if (lane == 0) {
            out_ids[o + kept] = id;
            if (out_tids) out_tids[o + kept] = tids[id];
            if (out_dist)
                out_dist[o + kept] = rescore ? sd[sp] : plain_keys ? plain_unkey(plain_keys[(size_t)w * M + sp]) : __int_as_float(0x7fc00000);
        }
        ++kept;
    }
    for (uint32_t j = kept + lane; j < k; j += WAVE) {
        out_ids[o + j] = VS_INVALID_NODE;
        if (out_tids) out_tids[o + j] = 0;
        if (out_dist) out_dist[o + j] = __int_as_float(0x7fc00000);
    }
    if (lane == 0) {
        ql.out_rows[q] = kept;
        ql.out_pops[q] = pops;
        ql.out_state[q] = qual_state(kept, k, pops, P, ql.final);
    }
}

// rows [first, first + count) of a group column read VS_GROUP_NONE: the rows past an index's n, which no _put or _patch has named yet
__global__ __launch_bounds__(256) void k_group_fill(uint32_t* __restrict__ groups, size_t first, size_t count) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) groups[first + i] = VS_GROUP_NONE;
}

// ---------------------------------------------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------------------------------------------
// the fused kernel's own line: rerank_window_fits' 24 KB and 4096 rows, against an LDS block that is 4 M + 4 k bytes larger
bool rerank_window_grouped_fits(const vs_index* idx, uint32_t M, uint32_t rescore, uint32_t k) {
    return M <= 4096 && rerank_window_grouped_lds(idx->vec_stride, M, rescore, k) <= 24 * 1024;
}

int launch_rerank_window_grouped(vs_index* idx, const float* d_q_full, const uint32_t* d_stream_ids, const uint32_t* d_cnt, uint32_t M,
                                 uint32_t rescore, uint32_t k, uint32_t nq, uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist,
                                 uint32_t mode, const uint32_t* d_perm, bool deal, const GroupLaunch& gl) {
    if (nq == 0) return VS_OK;
    VS_REQUIRE(idx->vecs != nullptr, "index has no vector column: rerank impossible");
    VS_REQUIRE(gl.groups && gl.per_group >= 1 && gl.ql.pops >= 1, "grouped rerank: no group column or rule");
    VS_REQUIRE(rescore > 0 && rerank_window_grouped_fits(idx, M, rescore, k), "fused grouped rerank: window of %u rows does not fit", M);
    const size_t lds = rerank_window_grouped_lds(idx->vec_stride, M, rescore, k);
    hipLaunchKernelGGL(k_rerank_window_grouped, dim3(rerank_grid(nq, deal)), dim3(256), lds, idx->ctx->stream, idx->vecs, idx->vec_stride,
                       idx->d.dim_full, idx->vnorm, idx->d.distance_type, d_q_full, d_stream_ids, d_cnt, M, rescore, k, nq, idx->tids,
                       d_out_ids, d_out_tids, d_out_dist, mode, d_perm, deal ? 1u : 0u, gl);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int launch_resort_grouped(vs_index* idx, uint32_t nq, uint32_t M, uint32_t rescore, uint32_t k, const uint32_t* d_stream_ids, const uint32_t* d_cnt,
                          const float* d_dist, uint64_t* d_heap_ws, uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, const GroupLaunch& gl) {
    if (nq == 0) return VS_OK;
    VS_REQUIRE(gl.groups && gl.per_group >= 1 && gl.ql.pops >= 1, "grouped resort: no group column or rule");
    VS_REQUIRE(k <= VS_GROUP_MAX_K, "grouped resort: k %u above %d (the kept groups of a scan stay in LDS)", k, VS_GROUP_MAX_K);
    const uint32_t* plain_keys = (idx->d.storage_type == VS_STORAGE_PLAIN && idx->d.dim_index == idx->d.dim_full)
                                     ? (const uint32_t*)idx->ws.stream_ham.p : nullptr;
    hipLaunchKernelGGL(k_resort_grouped, dim3(nq), dim3(WAVE), (size_t)k * 4, idx->ctx->stream, nq, M, rescore, k, d_stream_ids, d_cnt, d_dist,
                       idx->tids, d_heap_ws, d_out_ids, d_out_tids, d_out_dist, plain_keys, gl);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int launch_group_fill(vs_index* idx, uint32_t* d_groups, size_t first, size_t count) {
    if (count == 0) return VS_OK;
    const uint32_t grid = (uint32_t)std::min<size_t>((count + 255) / 256, 4096);
    hipLaunchKernelGGL(k_group_fill, dim3(grid), dim3(256), 0, idx->ctx->stream, d_groups, first, count);
    VS_HIP(hipGetLastError());
    return VS_OK;
}
