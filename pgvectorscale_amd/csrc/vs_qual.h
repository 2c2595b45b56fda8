// vs_qual.h — qualified scans (a part of vs_batch.hip kept in a file of its own): the qualifiers of an index, one bit per node
// (vs_index_qual_*), and the batches that return the first k rows of a scan whose node passes the qualifier the scan names
// (vs_search_batch_qual, vs_search_batch_dev_qual).  The contract is the header's (include/vsgpu.h, "qualified scans").
//
// A batch runs in rounds.  A round is the batch pipeline of vs_search_batch_dev with a stream long enough for P pops, whose window —
// k_rerank_window_qual, or k_resort_qual where the fused kernel does not take the window or rescore is 0 (vs_kernels.hip) — pops up
// to P rows per scan, reads the popped node's bit of the scan's qualifier AFTER each pop, keeps the row if it is set and stops at k
// kept rows: a rejected row has held its place in the rescore window like any other.  Scans that are neither complete nor ended after
// P pops are gathered (k_qual_gather, their label keys on the host) and re-run from the start at twice the pops; the sequence is
// prefix-consistent in P, so the re-run is exact.  The kernels an unqualified batch runs are not touched.
#pragma once
#include "vs_device.h"

// ---------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------
// A lane per node, a wave per 64 nodes = one word of the bitmap.  A node whose tid offset is InvalidOffsetNumber never qualifies;
// otherwise a binary search in the sorted set decides (the set is small and stays in L2, as in k_bulk_delete).  One ballot is the
// word, stored by lane 0; no atomic touches the bitmap.  hit[j] = 1 marks the FIRST entry of a run of equal tids that a live node
// carries (plain stores of the same byte), for k_qual_unmatched.  counters[0] += bits set: a popcount and one atomic per wave.
__global__ __launch_bounds__(256) void k_qual_from_tids(const uint64_t* __restrict__ tids, uint32_t n, const uint64_t* __restrict__ set,
                                                        uint64_t n_set, uint64_t* __restrict__ bits, uint8_t* __restrict__ hit,
                                                        unsigned long long* __restrict__ counters) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / WAVE, n_waves = (uint64_t)gridDim.x * (256 / WAVE);
    uint32_t total = 0;
    for (uint64_t i0 = wave * WAVE; i0 < n; i0 += n_waves * WAVE) {  // (wave-uniform trip count: the ballot sees every lane)
        const uint64_t i = i0 + lane;
        bool pass = false;
        if (i < n) {
            const uint64_t t = tids[i];
            if ((t & 0xFFFFull) != 0) {
                uint64_t lo = 0, hi = n_set;
                while (lo < hi) {
                    const uint64_t mid = lo + ((hi - lo) >> 1);
                    if (set[mid] < t) lo = mid + 1;
                    else hi = mid;
                }
                pass = lo < n_set && set[lo] == t;
                if (pass) hit[lo] = 1;
            }
        }
        const uint64_t word = __ballot(pass);
        if (lane == 0) bits[i0 >> 6] = word;
        total += (uint32_t)__popcll(word);
    }
    if (lane == 0 && total) atomicAdd(&counters[0], (unsigned long long)total);
}

// counters[1] += the distinct tids of the sorted list that no live node carries (a lane per entry; runs of equal tids count once,
// at their first entry, which is where k_qual_from_tids left its mark)
__global__ __launch_bounds__(256) void k_qual_unmatched(const uint64_t* __restrict__ set, uint64_t n_set, const uint8_t* __restrict__ hit,
                                                        unsigned long long* __restrict__ counters) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / WAVE, n_waves = (uint64_t)gridDim.x * (256 / WAVE);
    uint32_t total = 0;
    for (uint64_t j0 = wave * WAVE; j0 < n_set; j0 += n_waves * WAVE) {
        const uint64_t j = j0 + lane;
        const bool lost = j < n_set && (j == 0 || set[j - 1] != set[j]) && hit[j] == 0;
        total += (uint32_t)__popcll(__ballot(lost));
    }
    if (lane == 0 && total) atomicAdd(&counters[1], (unsigned long long)total);
}

// the caller's words made a qualifier: bits at positions >= n are cleared (the last word is masked, later words are zero already),
// counters[0] += bits set.  A lane per word.
__global__ __launch_bounds__(256) void k_qual_seal(uint64_t* __restrict__ bits, uint32_t n, unsigned long long* __restrict__ counters) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint64_t n_words = ((uint64_t)n + 63) / 64;
    const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / WAVE, n_waves = (uint64_t)gridDim.x * (256 / WAVE);
    uint32_t total = 0;
    for (uint64_t w0 = wave * WAVE; w0 < n_words; w0 += n_waves * WAVE) {
        const uint64_t w = w0 + lane;
        uint32_t c = 0;
        if (w < n_words) {
            uint64_t v = bits[w];
            if (w == n_words - 1 && (n & 63u)) {
                v &= (1ull << (n & 63u)) - 1;
                bits[w] = v;
            }
            c = (uint32_t)__popcll(v);
        }
        for (int m = 1; m < WAVE; m <<= 1) c += (uint32_t)__shfl_xor((int)c, m, WAVE);
        total += c;
    }
    if (lane == 0 && total) atomicAdd(&counters[0], (unsigned long long)total);
}

// dst[i] = src[map[i]] for rows of `dim` floats: the queries of the scans a later round runs again
__global__ __launch_bounds__(256) void k_qual_gather(const float* __restrict__ src, uint32_t dim, const uint32_t* __restrict__ map, uint32_t m,
                                                     float* __restrict__ dst) {
    const uint64_t total = (uint64_t)m * dim;
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256) {
        const uint32_t i = (uint32_t)(e / dim), c = (uint32_t)(e % dim);
        dst[e] = src[(size_t)map[i] * dim + c];
    }
}

// A batch that names no qualifier at all (every slot 0) at P == k runs the unqualified pipeline straight into the caller's rows; what
// is left to say is how many rows each scan has.  A lane per scan: rows[q] = pops[q] = the rows before the first VS_INVALID_NODE,
// COMPLETE at k of them, else ENDED (amgettuple returned None within k calls).
__global__ __launch_bounds__(256) void k_qual_count(const uint32_t* __restrict__ ids, uint32_t k, uint32_t q_base, uint32_t m,
                                                    uint32_t* __restrict__ out_rows, uint32_t* __restrict__ out_pops, uint32_t* __restrict__ out_state) {
    const uint32_t w = blockIdx.x * 256 + threadIdx.x;
    if (w >= m) return;
    const uint32_t q = q_base + w;
    uint32_t rows = 0;
    while (rows < k && ids[(size_t)q * k + rows] != VS_INVALID_NODE) ++rows;
    out_rows[q] = rows;
    out_pops[q] = rows;
    out_state[q] = rows == k ? (uint32_t)VS_QUAL_COMPLETE : (uint32_t)VS_QUAL_ENDED;
}

// ---------------------------------------------------------------------------------------------------------------
// the qualifiers of an index
// ---------------------------------------------------------------------------------------------------------------
static inline uint32_t qual_grid(uint64_t lanes) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((lanes + 255) / 256, 1), 8192); }

void vs_qual_drop_all(vs_index* ix) {
    if (!ix || !ix->qs) return;
    (void)hipSetDevice(ix->ctx->device);
    (void)hipStreamSynchronize(ix->ctx->stream);
    for (uint64_t* p : ix->qs->bits)
        if (p) (void)hipFree(p);
    if (ix->qs->tab) (void)hipFree(ix->qs->tab);
    delete ix->qs;
    ix->qs = nullptr;
}

// the checks every vs_index_qual_* call that writes shares; nothing has been written when one fails
static int qual_check_write(vs_index* ix, uint32_t slot, const char* what) {
    VS_REQUIRE(slot >= 1 && slot <= VS_MAX_QUAL_SLOTS, "%s: slot %u outside [1,%d] (slot 0 is \"no qualifier\")", what, slot, VS_MAX_QUAL_SLOTS);
    VS_REQUIRE(ix, "%s: index is NULL", what);
    VS_REQUIRE_OWNER(ix, what);
    if (ix->ws.pending) {
        vs_set_error("%s: a batch of this handle is in flight (vs_search_batch_dev_finish first)", what);
        return VS_ERR_STATE;
    }
    return VS_OK;
}

// the record, the device table of the slots, and room for `capacity` nodes in every slot that is filled
static int qual_prepare(vs_index* ix, const char* what) {
    if (!ix->qs) ix->qs = new QualSet();
    QualSet* s = ix->qs;
    if (!s->tab) {
        VS_HIP(hipMalloc(&s->tab, sizeof s->bits));
        VS_HIP(hipMemset(s->tab, 0, sizeof s->bits));
    }
    const size_t need = std::max<size_t>(((size_t)std::max(ix->d.n, ix->capacity) + 63) / 64, 1);
    if (need <= s->words) return VS_OK;
    VS_HIP(hipStreamSynchronize(ix->ctx->stream));
    for (uint32_t sl = 1; sl <= VS_MAX_QUAL_SLOTS; ++sl) {  // (an index whose arrays grew without vs_index_reserve: the slots follow)
        if (!s->bits[sl]) continue;
        uint64_t* fresh = nullptr;
        VS_HIP(hipMalloc(&fresh, need * 8));
        VS_HIP(hipMemset(fresh, 0, need * 8));
        VS_HIP(hipMemcpy(fresh, s->bits[sl], s->words * 8, hipMemcpyDeviceToDevice));
        (void)hipFree(s->bits[sl]);
        s->bits[sl] = fresh;
    }
    s->words = need;
    VS_HIP(hipMemcpy(s->tab, s->bits, sizeof s->bits, hipMemcpyHostToDevice));
    (void)what;
    return VS_OK;
}

// `fresh` (words of the set's size, filled on the stream) becomes the slot's bitmap
static int qual_install(vs_index* ix, uint32_t slot, uint64_t* fresh, const vs_qual_info& info) {
    QualSet* s = ix->qs;
    if (s->bits[slot]) (void)hipFree(s->bits[slot]);
    s->bits[slot] = fresh;
    s->info[slot] = info;
    VS_HIP(hipMemcpy(s->tab, s->bits, sizeof s->bits, hipMemcpyHostToDevice));
    return VS_OK;
}

static int qual_put_impl(vs_index* ix, uint32_t slot, const uint64_t* bits, bool on_device, const char* what) {
    VS_TRY(qual_check_write(ix, slot, what));
    VS_REQUIRE(bits || ix->d.n == 0, "%s: bits is NULL", what);
    vs_ctx* c = ix->ctx;
    hipStream_t st = c->stream;
    VS_HIP(hipSetDevice(c->device));
    VS_TRY(qual_prepare(ix, what));
    const uint32_t n = ix->d.n;
    const size_t n_words = ((size_t)n + 63) / 64;
    DevScope sc(st);
    uint64_t* fresh = nullptr;
    unsigned long long *d_cnt = nullptr, h_cnt[2] = {0, 0};
    VS_TRY(sc.alloc(&fresh, ix->qs->words * 8, what));
    VS_TRY(sc.alloc(&d_cnt, sizeof h_cnt, what));
    VS_HIP(hipMemsetAsync(fresh, 0, ix->qs->words * 8, st));
    VS_HIP(hipMemsetAsync(d_cnt, 0, sizeof h_cnt, st));
    if (n_words) {
        if (on_device) {
            VS_HIP(hipMemcpyAsync(fresh, bits, n_words * 8, hipMemcpyDeviceToDevice, st));
        } else {
            VS_HIP(hipStreamSynchronize(st));  // (the staged copy runs on the copy stream: behind the clear)
            VS_TRY(vs_dev_upload(c, fresh, bits, n_words * 8));
        }
        hipLaunchKernelGGL(k_qual_seal, dim3(qual_grid(n_words)), dim3(256), 0, st, fresh, n, d_cnt);
        VS_HIP(hipGetLastError());
    }
    VS_HIP(hipMemcpyAsync(h_cnt, d_cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st));
    VS_HIP(hipStreamSynchronize(st));
    vs_qual_info info{n, h_cnt[0], 0};
    return qual_install(ix, slot, sc.release(fresh), info);
}

static int qual_from_tids_impl(vs_index* ix, uint32_t slot, const uint64_t* list, size_t n_list, bool on_device, vs_qual_info* out, const char* what) {
    VS_TRY(qual_check_write(ix, slot, what));
    if (out) memset(out, 0, sizeof(*out));
    VS_REQUIRE(n_list == 0 || list, "%s: heap_tids is NULL", what);
    VS_REQUIRE(n_list <= 0x7FFFFFFFull, "%s: %zu tids in one call (at most 2^31 - 1)", what, n_list);
    VS_REQUIRE(ix->tids || ix->d.n == 0, "%s: the index holds no heap tids", what);
    vs_ctx* c = ix->ctx;
    hipStream_t st = c->stream;
    VS_HIP(hipSetDevice(c->device));
    VS_TRY(qual_prepare(ix, what));
    const uint32_t n = ix->d.n;
    DevScope sc(st);
    uint64_t *fresh = nullptr, *d_set = nullptr;
    uint8_t* d_hit = nullptr;
    unsigned long long *d_cnt = nullptr, h_cnt[2] = {0, 0};
    VS_TRY(sc.alloc(&fresh, ix->qs->words * 8, what));
    VS_TRY(sc.alloc(&d_cnt, sizeof h_cnt, what));
    VS_TRY(sc.alloc(&d_hit, std::max<size_t>(n_list, 1), what));
    const uint64_t* d_list = list;
    if (!on_device && n_list) {  // a TID bitmap's worth of tids: sorted and de-duplicated on the host, staged through the pinned ring
        std::vector<uint64_t> sorted(list, list + n_list);
        std::sort(sorted.begin(), sorted.end());
        sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
        n_list = sorted.size();
        VS_TRY(sc.alloc(&d_set, n_list * 8, what));
        VS_TRY(vs_dev_upload(c, d_set, sorted.data(), n_list * 8));
        d_list = d_set;
    }
    VS_HIP(hipMemsetAsync(fresh, 0, ix->qs->words * 8, st));
    VS_HIP(hipMemsetAsync(d_cnt, 0, sizeof h_cnt, st));
    VS_HIP(hipMemsetAsync(d_hit, 0, std::max<size_t>(n_list, 1), st));
    if (n) {
        hipLaunchKernelGGL(k_qual_from_tids, dim3(qual_grid(n)), dim3(256), 0, st, (const uint64_t*)ix->tids, n, d_list, (uint64_t)n_list, fresh, d_hit, d_cnt);
        VS_HIP(hipGetLastError());
    }
    if (n_list) {
        hipLaunchKernelGGL(k_qual_unmatched, dim3(qual_grid(n_list)), dim3(256), 0, st, d_list, (uint64_t)n_list, (const uint8_t*)d_hit, d_cnt);
        VS_HIP(hipGetLastError());
    }
    VS_HIP(hipMemcpyAsync(h_cnt, d_cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st));
    VS_HIP(hipStreamSynchronize(st));
    vs_qual_info info{n, h_cnt[0], h_cnt[1]};
    if (out) *out = info;
    return qual_install(ix, slot, sc.release(fresh), info);
}

static int qual_slot_filled(const vs_index* ix, uint32_t slot, const char* what) {
    VS_REQUIRE(slot >= 1 && slot <= VS_MAX_QUAL_SLOTS, "%s: slot %u outside [1,%d]", what, slot, VS_MAX_QUAL_SLOTS);
    VS_REQUIRE(ix, "%s: index is NULL", what);
    if (!ix->qs || !ix->qs->bits[slot]) {
        vs_set_error("%s: slot %u holds no qualifier (vs_index_qual_put / vs_index_qual_from_tids)", what, slot);
        return VS_ERR_STATE;
    }
    return VS_OK;
}

extern "C" int vs_index_qual_put(vs_index* ix, uint32_t slot, const uint64_t* bits) {
    return vs_guard("vs_index_qual_put", [&] { return qual_put_impl(ix, slot, bits, false, "vs_index_qual_put"); });
}
extern "C" int vs_index_qual_put_dev(vs_index* ix, uint32_t slot, const uint64_t* d_bits) {
    return vs_guard("vs_index_qual_put_dev", [&] { return qual_put_impl(ix, slot, d_bits, true, "vs_index_qual_put_dev"); });
}
extern "C" int vs_index_qual_from_tids(vs_index* ix, uint32_t slot, const uint64_t* heap_tids, size_t n_tids, vs_qual_info* info) {
    return vs_guard("vs_index_qual_from_tids", [&] { return qual_from_tids_impl(ix, slot, heap_tids, n_tids, false, info, "vs_index_qual_from_tids"); });
}
extern "C" int vs_index_qual_from_tids_dev(vs_index* ix, uint32_t slot, const uint64_t* d_heap_tids_sorted, size_t n_tids, vs_qual_info* info) {
    return vs_guard("vs_index_qual_from_tids_dev",
                    [&] { return qual_from_tids_impl(ix, slot, d_heap_tids_sorted, n_tids, true, info, "vs_index_qual_from_tids_dev"); });
}
extern "C" int vs_index_qual_info(const vs_index* ix, uint32_t slot, vs_qual_info* info) {
    VS_REQUIRE(info, "vs_index_qual_info: info is NULL");
    VS_TRY(qual_slot_filled(ix, slot, "vs_index_qual_info"));
    *info = ix->qs->info[slot];
    return VS_OK;
}
extern "C" int vs_index_qual_get(vs_index* ix, uint32_t slot, uint64_t* bits) {
    VS_REQUIRE(bits, "vs_index_qual_get: bits is NULL");
    VS_TRY(qual_slot_filled(ix, slot, "vs_index_qual_get"));
    VS_HIP(hipSetDevice(ix->ctx->device));
    return vs_dev_download(ix->ctx, bits, ix->qs->bits[slot], (((size_t)ix->d.n + 63) / 64) * 8);
}
extern "C" int vs_index_qual_drop(vs_index* ix, uint32_t slot) {
    VS_TRY(qual_check_write(ix, slot, "vs_index_qual_drop"));
    VS_TRY(qual_slot_filled(ix, slot, "vs_index_qual_drop"));
    VS_HIP(hipSetDevice(ix->ctx->device));
    VS_HIP(hipStreamSynchronize(ix->ctx->stream));  // (no launch may still read it)
    (void)hipFree(ix->qs->bits[slot]);
    ix->qs->bits[slot] = nullptr;
    ix->qs->info[slot] = vs_qual_info{};
    VS_HIP(hipMemcpy(ix->qs->tab, ix->qs->bits, sizeof ix->qs->bits, hipMemcpyHostToDevice));
    return VS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// the batch
// ---------------------------------------------------------------------------------------------------------------
// The slots a batch names (HOST [nq]): each within the table and, unless 0, filled.  *all_zero: no scan names a qualifier;
// *density: n_set / n of the sparsest qualifier named (1 without one).
static int qual_check_slots(const vs_index* ix, const char* what, const uint32_t* slots, uint32_t nq, bool* all_zero, double* density) {
    *all_zero = true;
    *density = 1.0;
    for (uint32_t q = 0; q < nq; ++q) {
        const uint32_t sl = slots[q];
        VS_REQUIRE(sl <= VS_MAX_QUAL_SLOTS, "%s: scan %u names qualifier slot %u outside [0,%d]", what, q, sl, VS_MAX_QUAL_SLOTS);
        if (!sl) continue;
        if (!ix->qs || !ix->qs->bits[sl]) {
            vs_set_error("%s: scan %u names qualifier slot %u, which is empty (vs_index_qual_put / vs_index_qual_from_tids)", what, q, sl);
            return VS_ERR_STATE;
        }
        *all_zero = false;
        *density = std::min(*density, ix->d.n ? (double)ix->qs->info[sl].n_set / (double)ix->d.n : 0.0);
    }
    return VS_OK;
}

// P1: pops after which a scan of the sparsest qualifier named is expected to have its k rows — the mean of the pops the k-th success
// of independent trials of probability `density` takes, k / density, plus two standard deviations sqrt(k (1 - density)) / density.
// A cost choice only: every result is the same for any P1 in [k, max_pops].
static uint32_t qual_first_pops(uint32_t k, uint32_t max_pops, double density) {
    if (const uint32_t v = env_u32("VS_QUAL_FIRST_POPS", 0)) return std::min(std::max(v, k), max_pops);
    if (density >= 1.0) return k;
    if (density <= 0.0) return max_pops;
    const double want = std::ceil(((double)k + 2.0 * std::sqrt((double)k * (1.0 - density))) / density);
    return (uint32_t)std::min<double>(std::max<double>(want, (double)k), (double)max_pops);
}

// (the same rule for the scan pools' qualified fetch, vs_scanpool.cpp)
uint32_t vs_qual_first_pops(uint32_t k, uint32_t max_pops, double density) { return qual_first_pops(k, max_pops, density); }

// (what needs no index comes first: a bad slot array or pop limit is named whatever the handle is)
static int qual_check_gucs(const vs_index* ix, const char* what, const uint32_t* slots, uint32_t L, uint32_t rescore, uint32_t k, uint32_t max_pops) {
    VS_REQUIRE(slots, "%s: qual_slots is NULL (the unqualified calls exist for that)", what);
    VS_REQUIRE(L >= 1 && L <= 10000, "%s: diskann.query_search_list_size %u outside [1,10000]", what, L);
    VS_REQUIRE(rescore <= 1000, "%s: diskann.query_rescore %u outside [0,1000]", what, rescore);
    VS_REQUIRE(k >= 1, "%s: k must be >= 1", what);
    VS_REQUIRE(max_pops >= k && max_pops <= VS_QUAL_MAX_POPS, "%s: max_pops %u outside [k = %u, %d]", what, max_pops, k, VS_QUAL_MAX_POPS);
    VS_REQUIRE(ix, "%s: index is NULL", what);
    VS_REQUIRE_OWNER(ix, what);
    return VS_OK;
}

static void qual_add_stats(vs_stats* into, const vs_stats& s) {
    static_assert(sizeof(vs_stats) % sizeof(uint64_t) == 0, "vs_stats is a record of u64 counters");
    uint64_t* a = reinterpret_cast<uint64_t*>(into);
    const uint64_t* b = reinterpret_cast<const uint64_t*>(&s);
    for (size_t i = 0; i < sizeof(vs_stats) / sizeof(uint64_t); ++i) a[i] += b[i];
}

// scans one launch of a round at P pops may hold: what the batch pipeline takes at this stream length
static uint32_t qual_launch_scans(vs_index* ix, uint32_t L, uint32_t rescore, uint32_t P, uint32_t m) {
    uint32_t rs = rescore;
    if (ix->d.storage_type == VS_STORAGE_PLAIN && ix->d.dim_index == ix->d.dim_full) rs = 0;
    const uint32_t M = stream_len(rs, P);
    const Caps caps = initial_caps(ix, L, M);
    return std::max<uint32_t>(std::min(chunk_queries(ix, caps, M, m), m), 1);
}

// One launch of a round: scans [s0, s0 + cnt) of the round's m, at P pops.  direct (every slot 0, P == k, round 1): the unqualified
// pipeline, rows straight to the caller's; otherwise the window under ql keeps k of up to P rows and writes row map[w] / s0 + w of the
// batch's outputs itself.
struct QualRoundLaunch {
    bool direct;
    QualLaunch ql;
    uint32_t* ids;
    uint64_t* tids;
    float* dist;
};
static QualRoundLaunch qual_round_launch(const vs_index* ix, const PendingQual& pq, uint32_t P, uint32_t s0, const uint32_t* d_map) {
    QualRoundLaunch r{};
    r.direct = pq.all_zero && P == pq.k && !d_map;
    r.ids = pq.d_out_ids;
    r.tids = pq.d_out_tids;
    r.dist = pq.d_out_dist;
    if (r.direct) {
        r.ids += (size_t)s0 * pq.k;
        if (r.tids) r.tids += (size_t)s0 * pq.k;
        if (r.dist) r.dist += (size_t)s0 * pq.k;
        return r;
    }
    r.ql.pops = P;
    r.ql.q_base = s0;
    r.ql.map = d_map ? d_map + s0 : nullptr;
    r.ql.slots = pq.d_slots;
    r.ql.tab = (!pq.all_zero && ix->qs) ? (const uint64_t* const*)ix->qs->tab : nullptr;
    r.ql.final = P == pq.max_pops ? 1u : 0u;
    r.ql.out_rows = pq.d_out_rows;
    r.ql.out_pops = pq.d_out_pops;
    r.ql.out_state = pq.d_out_state;
    return r;
}

// The rounds of one batch whose queries, label keys, slots and outputs are on the device (pq).  pq.launched: round 1 is already in
// flight as one launch over all nq scans.  Synchronises; *st accumulates the device's work, *qs the rounds.
static int qual_run_rounds(vs_index* ix, const PendingQual& pq, vs_stats* st, vs_qual_batch_stats* qs) {
    vs_ctx* c = ix->ctx;
    SearchWorkspace& w = ix->ws;
    hipStream_t stream = c->stream;
    const uint32_t nq = pq.nq, k = pq.k, dim = ix->d.dim_full;
    uint32_t P = pq.first_pops, m = nq;
    const float* d_q = pq.d_queries;
    const int16_t* d_lab = pq.d_qlabels;
    const uint32_t* d_off = pq.d_qlabel_off;
    const uint32_t* d_map = nullptr;
    std::vector<uint32_t> active, state(nq), h_off;  // active: the scan numbers of this round (empty: all of them, in order)
    std::vector<int16_t> h_lab;
    bool in_flight = pq.launched;
    for (;;) {
        const uint32_t final = P == pq.max_pops ? 1u : 0u;
        const uint32_t per = in_flight ? m : qual_launch_scans(ix, pq.L, pq.rescore, P, m);
        for (uint32_t s0 = 0; s0 < m; s0 += per) {
            const uint32_t cnt = std::min(per, m - s0);
            const QualRoundLaunch r = qual_round_launch(ix, pq, P, s0, d_map);
            if (!in_flight)  // (else: round 1, launched by vs_search_batch_dev_qual with the same plan)
                VS_TRY(vs_search_batch_dev_impl(ix, d_q + (size_t)s0 * dim, d_lab, d_off ? d_off + s0 : nullptr, cnt, pq.L, pq.rescore, k, r.ids, r.tids,
                                                r.dist, nullptr, r.direct ? nullptr : &r.ql));
            in_flight = false;
            vs_stats one{};
            VS_TRY(vs_search_batch_dev_finish_impl(ix, &one));
            if (st) qual_add_stats(st, one);
            if (r.direct) {
                hipLaunchKernelGGL(k_qual_count, dim3((cnt + 255) / 256), dim3(256), 0, stream, (const uint32_t*)pq.d_out_ids, k, s0, cnt, pq.d_out_rows,
                                   pq.d_out_pops, pq.d_out_state);
                VS_HIP(hipGetLastError());
            }
        }
        VS_TRY(vs_dev_download(c, state.data(), pq.d_out_state, (size_t)nq * 4));  // (waits for the stream)
        qs->rounds++;
        qs->pops_launched += (uint64_t)m * P;
        if (d_map) qs->scans_rerun += m;
        std::vector<uint32_t> next;
        if (active.empty()) {
            for (uint32_t q = 0; q < nq; ++q)
                if (state[q] == VS_QUAL_MORE) next.push_back(q);
        } else {
            for (uint32_t q : active)
                if (state[q] == VS_QUAL_MORE) next.push_back(q);
        }
        if (next.empty() || final) break;
        // the next round: the unfinished scans from the start, at twice the pops
        P = (uint32_t)std::min<uint64_t>(2ull * P, pq.max_pops);
        m = (uint32_t)next.size();
        VS_TRY(devbuf_reserve(c, w.qual_map, (size_t)m * 4));
        VS_TRY(vs_dev_upload(c, w.qual_map.p, next.data(), (size_t)m * 4));
        VS_TRY(devbuf_reserve(c, w.qual_q, (size_t)m * dim * 4));
        hipLaunchKernelGGL(k_qual_gather, dim3(qual_grid((uint64_t)m * dim)), dim3(256), 0, stream, pq.d_queries, dim, (const uint32_t*)w.qual_map.p, m,
                           (float*)w.qual_q.p);
        VS_HIP(hipGetLastError());
        if (pq.d_qlabel_off) {  // their label keys: the batch's CSR comes back once, the round's is cut from it on the host
            if (h_off.empty()) {
                h_off.resize((size_t)nq + 1);
                VS_TRY(vs_dev_download(c, h_off.data(), pq.d_qlabel_off, h_off.size() * 4));
                h_lab.resize(std::max<size_t>(h_off[nq] - h_off[0], 1));
                if (h_off[nq] > h_off[0]) VS_TRY(vs_dev_download(c, h_lab.data(), pq.d_qlabels + h_off[0], (size_t)(h_off[nq] - h_off[0]) * 2));
            }
            std::vector<uint32_t> off(m + 1, 0);
            std::vector<int16_t> vals;
            for (uint32_t i = 0; i < m; ++i) {
                const uint32_t q = next[i];
                vals.insert(vals.end(), h_lab.begin() + (h_off[q] - h_off[0]), h_lab.begin() + (h_off[q + 1] - h_off[0]));
                off[i + 1] = (uint32_t)vals.size();
            }
            VS_TRY(devbuf_reserve(c, w.qual_lab, std::max<size_t>(vals.size(), 1) * 2));
            VS_TRY(devbuf_reserve(c, w.qual_laboff, off.size() * 4));
            if (!vals.empty()) VS_TRY(vs_dev_upload(c, w.qual_lab.p, vals.data(), vals.size() * 2));
            VS_TRY(vs_dev_upload(c, w.qual_laboff.p, off.data(), off.size() * 4));
            d_lab = (const int16_t*)w.qual_lab.p;
            d_off = (const uint32_t*)w.qual_laboff.p;
        }
        d_q = (const float*)w.qual_q.p;
        d_map = (const uint32_t*)w.qual_map.p;
        active.swap(next);
    }
    for (uint32_t q = 0; q < nq; ++q) {
        if (state[q] == VS_QUAL_COMPLETE) qs->complete++;
        else if (state[q] == VS_QUAL_ENDED) qs->ended++;
        else qs->cut++;
    }
    return VS_OK;
}

static int search_batch_dev_qual_impl(vs_index* ix, const float* d_queries, const int16_t* d_qlabels, const uint32_t* d_qlabel_off, uint32_t nq,
                                      uint32_t L, uint32_t rescore, uint32_t k, const uint32_t* d_slots, uint32_t max_pops, uint32_t* d_out_ids,
                                      uint64_t* d_out_tids, float* d_out_dist, uint32_t* d_out_rows, uint32_t* d_out_pops, uint32_t* d_out_state) {
    const char* what = "vs_search_batch_dev_qual";
    VS_TRY(qual_check_gucs(ix, what, d_slots, L, rescore, k, max_pops));
    VS_REQUIRE(nq == 0 || (d_queries && d_out_ids && d_out_rows && d_out_pops && d_out_state), "%s: null argument", what);
    if (ix->d.storage_type == VS_STORAGE_PLAIN) VS_REQUIRE(!d_qlabel_off, "Plain storage does not support label filters");
    SearchWorkspace& w = ix->ws;
    w.pending = false;
    w.qual_pending = false;
    if (nq == 0) return VS_OK;
    VS_HIP(hipSetDevice(ix->ctx->device));
    std::vector<uint32_t> slots(nq);  // the slots come back once: an empty slot is refused before anything is launched
    VS_TRY(vs_dev_download(ix->ctx, slots.data(), d_slots, (size_t)nq * 4));
    PendingQual pq;
    double density = 1.0;
    VS_TRY(qual_check_slots(ix, what, slots.data(), nq, &pq.all_zero, &density));
    pq.d_queries = d_queries;
    pq.d_qlabels = d_qlabels;
    pq.d_qlabel_off = d_qlabel_off;
    pq.d_slots = d_slots;
    pq.nq = nq;
    pq.L = L;
    pq.rescore = rescore;
    pq.k = k;
    pq.max_pops = max_pops;
    pq.first_pops = qual_first_pops(k, max_pops, density);
    pq.d_out_ids = d_out_ids;
    pq.d_out_tids = d_out_tids;
    pq.d_out_dist = d_out_dist;
    pq.d_out_rows = d_out_rows;
    pq.d_out_pops = d_out_pops;
    pq.d_out_state = d_out_state;
    // round 1 goes out now when it is one launch; a round that has to be cut waits for the finish
    const uint32_t P = pq.first_pops;
    if (qual_launch_scans(ix, L, rescore, P, nq) == nq) {
        const QualRoundLaunch r = qual_round_launch(ix, pq, P, 0, nullptr);
        VS_TRY(vs_search_batch_dev_impl(ix, d_queries, d_qlabels, d_qlabel_off, nq, L, rescore, k, r.ids, r.tids, r.dist, nullptr, r.direct ? nullptr : &r.ql));
        pq.launched = true;
    }
    w.pending = true;
    w.qual_pending = true;
    w.qpend = pq;
    return VS_OK;
}

static int search_batch_dev_qual_finish_impl(vs_index* ix, vs_stats* stats, vs_qual_batch_stats* qstats) {
    const char* what = "vs_search_batch_dev_qual_finish";
    VS_REQUIRE(ix, "%s: index is NULL", what);
    SearchWorkspace& w = ix->ws;
    if (!w.qual_pending) {
        vs_set_error("%s: no qualified batch in flight", what);
        return VS_ERR_STATE;
    }
    const PendingQual pq = w.qpend;
    w.qual_pending = false;
    if (!pq.launched) w.pending = false;
    VS_HIP(hipSetDevice(ix->ctx->device));
    vs_stats st{};
    vs_qual_batch_stats qs{};
    qs.first_pops = pq.first_pops;
    const int r = qual_run_rounds(ix, pq, &st, &qs);
    w.pending = false;
    VS_TRY(r);
    ix->last_stats = st;
    if (stats) *stats = st;
    if (qstats) *qstats = qs;
    return VS_OK;
}

static int search_batch_qual_impl(vs_index* ix, const float* queries, const int16_t* qlabels, const uint32_t* qlabel_off, uint32_t nq, uint32_t L,
                                  uint32_t rescore, uint32_t k, const uint32_t* qual_slots, uint32_t max_pops, uint32_t* out_ids, uint64_t* out_tids,
                                  float* out_dist, uint32_t* out_rows, uint32_t* out_pops, uint32_t* out_state, vs_stats* stats,
                                  vs_qual_batch_stats* qstats) {
    const char* what = "vs_search_batch_qual";
    VS_TRY(qual_check_gucs(ix, what, qual_slots, L, rescore, k, max_pops));
    VS_REQUIRE(nq == 0 || (queries && out_ids && out_rows && out_pops && out_state), "%s: null argument", what);
    if (ix->d.storage_type == VS_STORAGE_PLAIN) VS_REQUIRE(!qlabel_off, "Plain storage does not support label filters");
    if (ix->ws.pending) {
        vs_set_error("%s: a batch of this handle is in flight (vs_search_batch_dev_finish first)", what);
        return VS_ERR_STATE;
    }
    bool all_zero = true;
    double density = 1.0;
    VS_TRY(qual_check_slots(ix, what, qual_slots, nq, &all_zero, &density));
    if (stats) memset(stats, 0, sizeof(*stats));
    if (qstats) memset(qstats, 0, sizeof(*qstats));
    vs_stats st{};
    vs_qual_batch_stats qs{};
    qs.first_pops = qual_first_pops(k, max_pops, density);
    if (qstats) *qstats = qs;
    if (nq == 0) return VS_OK;
    vs_ctx* c = ix->ctx;
    VS_HIP(hipSetDevice(c->device));
    SearchWorkspace& w = ix->ws;
    const int16_t* d_lab = nullptr;
    const uint32_t* d_off = nullptr;
    VS_TRY(upload_label_keys(ix, qlabels, qlabel_off, nq, &d_lab, &d_off));
    VS_TRY(devbuf_reserve(c, w.qual_slots, (size_t)nq * 4));
    VS_TRY(vs_dev_upload(c, w.qual_slots.p, qual_slots, (size_t)nq * 4));
    // the chunks of a host batch, by the rule of vs_search_batch (VS_HOST_CHUNKS / VS_HOST_CHUNK_MIN); each runs its own rounds
    uint32_t chunk = nq;
    {
        const uint32_t want = std::max<uint32_t>(env_u32("VS_HOST_CHUNKS", 4), 1);
        const uint32_t floor_q = env_u32("VS_HOST_CHUNK_MIN", 32768);
        chunk = std::min(nq, std::max<uint32_t>(std::max<uint32_t>((nq + want - 1) / want, floor_q), 1));
    }
    const size_t qrow = (size_t)ix->d.dim_full * 4;
    // [chunk][k] ids | tids | distances, then [chunk] rows | pops | states
    const size_t o_tids = (size_t)chunk * k * 4, o_dist = o_tids + (size_t)chunk * k * 8, o_rows = o_dist + (size_t)chunk * k * 4;
    VS_TRY(devbuf_reserve(c, w.qual_out, o_rows + (size_t)chunk * 12));
    VS_TRY(devbuf_reserve(c, w.raw_q, (size_t)chunk * qrow));
    for (uint32_t q0 = 0; q0 < nq; q0 += chunk) {
        const uint32_t cq = std::min(chunk, nq - q0);
        VS_TRY(vs_dev_upload(c, w.raw_q.p, queries + (size_t)q0 * ix->d.dim_full, (size_t)cq * qrow));
        char* ob = (char*)w.qual_out.p;
        PendingQual pq;
        pq.d_queries = (const float*)w.raw_q.p;
        pq.d_qlabels = d_lab;
        pq.d_qlabel_off = d_off ? d_off + q0 : nullptr;
        pq.d_slots = (const uint32_t*)w.qual_slots.p + q0;
        pq.nq = cq;
        pq.L = L;
        pq.rescore = rescore;
        pq.k = k;
        pq.max_pops = max_pops;
        pq.first_pops = qs.first_pops;
        pq.all_zero = all_zero;
        pq.d_out_ids = (uint32_t*)ob;
        pq.d_out_tids = out_tids ? (uint64_t*)(ob + o_tids) : nullptr;
        pq.d_out_dist = out_dist ? (float*)(ob + o_dist) : nullptr;
        pq.d_out_rows = (uint32_t*)(ob + o_rows);
        pq.d_out_pops = pq.d_out_rows + chunk;
        pq.d_out_state = pq.d_out_pops + chunk;
        VS_TRY(qual_run_rounds(ix, pq, &st, &qs));
        VS_TRY(vs_dev_download(c, out_ids + (size_t)q0 * k, pq.d_out_ids, (size_t)cq * k * 4));
        if (out_tids) VS_TRY(vs_dev_download(c, out_tids + (size_t)q0 * k, pq.d_out_tids, (size_t)cq * k * 8));
        if (out_dist) VS_TRY(vs_dev_download(c, out_dist + (size_t)q0 * k, pq.d_out_dist, (size_t)cq * k * 4));
        VS_TRY(vs_dev_download(c, out_rows + q0, pq.d_out_rows, (size_t)cq * 4));
        VS_TRY(vs_dev_download(c, out_pops + q0, pq.d_out_pops, (size_t)cq * 4));
        VS_TRY(vs_dev_download(c, out_state + q0, pq.d_out_state, (size_t)cq * 4));
    }
    ix->last_stats = st;
    if (stats) *stats = st;
    if (qstats) *qstats = qs;
    return VS_OK;
}

extern "C" int vs_search_batch_qual(vs_index* ix, const float* queries, const int16_t* qlabels, const uint32_t* qlabel_off, uint32_t nq, uint32_t L,
                                    uint32_t rescore, uint32_t k, const uint32_t* qual_slots, uint32_t max_pops, uint32_t* out_ids, uint64_t* out_tids,
                                    float* out_dist, uint32_t* out_rows, uint32_t* out_pops, uint32_t* out_state, vs_stats* stats,
                                    vs_qual_batch_stats* qstats) {
    return vs_guard("vs_search_batch_qual", [&] {
        return search_batch_qual_impl(ix, queries, qlabels, qlabel_off, nq, L, rescore, k, qual_slots, max_pops, out_ids, out_tids, out_dist, out_rows,
                                      out_pops, out_state, stats, qstats);
    });
}
extern "C" int vs_search_batch_dev_qual(vs_index* ix, const float* d_queries, const int16_t* d_qlabels, const uint32_t* d_qlabel_off, uint32_t nq,
                                        uint32_t L, uint32_t rescore, uint32_t k, const uint32_t* d_qual_slots, uint32_t max_pops, uint32_t* d_out_ids,
                                        uint64_t* d_out_tids, float* d_out_dist, uint32_t* d_out_rows, uint32_t* d_out_pops, uint32_t* d_out_state) {
    return vs_guard("vs_search_batch_dev_qual", [&] {
        return search_batch_dev_qual_impl(ix, d_queries, d_qlabels, d_qlabel_off, nq, L, rescore, k, d_qual_slots, max_pops, d_out_ids, d_out_tids,
                                          d_out_dist, d_out_rows, d_out_pops, d_out_state);
    });
}
extern "C" int vs_search_batch_dev_qual_finish(vs_index* ix, vs_stats* stats, vs_qual_batch_stats* qstats) {
    return vs_guard("vs_search_batch_dev_qual_finish", [&] { return search_batch_dev_qual_finish_impl(ix, stats, qstats); });
}
