// vs_heap_vis.h — heap visibility decided ON the device from a resident copy of the heap's main fork (vs_heap_res_*,
// vs_index_snapshot_eval / _put_dev / _patch); part of vs_pages_dev.hip, which includes it behind vs_heap_dev.h.
//
// The rescore window drops every candidate whose heap tuple the scan's snapshot cannot see (AM/scan.rs:258-272,
// UT/table_slot.rs:19-53); the library carries that verdict as one byte per node (vs_index_set_visibility, vs_index_snapshot_put).
// Producing the bytes on the host is one table_index_fetch_tuple per node per snapshot.  Here the heap's main fork — line pointers
// and 23-byte tuple headers; the vectors live in TOAST — stays in HBM, indexed by block number and refreshed block by block
// (vs_heap_res_put), and a snapshot's mask is one pass of k_heap_vis over memory that is already there: a lane per node walks what
// heap_hot_search_buffer walks (the tid's line pointer, an LP_REDIRECT at the start, the HOT chain through t_ctid within the page)
// and judges every member as HeapTupleSatisfiesMVCC does, with the snapshot's xip / subxip / own-xid arrays sorted by the host and a
// window of pg_xact (2 bits per xid) next to them.  Hint bits are never written: the pages are read-only copies and the verdict
// does not depend on them.  What the device cannot decide — multixact members, pg_subtrans, combo command ids, the pre-9.0 MOVED
// bits, an xid outside the pg_xact window — is "undecided": the byte is 1 (the conservative value of INTEGRATION.md 3.1), the node
// is counted by reason and appended to a list through one counter; the list is sorted before it is handed out, so no output depends
// on scheduling.  Every offset read from a page is checked before it is used (heap_page_view, heap_item_in_bounds of vs_heap_dev.h):
// a malformed page ends in the error record of heap_error, never in a read outside the resident buffer.
#pragma once

enum { VV_INVISIBLE = 0, VV_VISIBLE = 1, VV_UNDECIDED = 2 /* + VS_VIS_R_* */ };
// heap_hot_search_buffer's verdict with the class vs_vis_stats counts it in
enum { VK_VISIBLE = 0, VK_INVISIBLE, VK_UNDECIDED, VK_DELETED, VK_NOT_FOUND, VK_DEAD_LP, VK_ERROR };

// counters of one evaluation in device memory (u32 words): the error record of heap_error in front, then u64 sums
enum { VC_NLIST = 5 /* entries appended to the undecided list */, VC_SUMS = 6 /* u64 each, 8-byte aligned */, VSUM_VISIBLE = 0, VSUM_INVISIBLE,
       VSUM_UNDECIDED, VSUM_DELETED, VSUM_NOT_FOUND, VSUM_DEAD_LP, VSUM_HOPS, VSUM_REASON, VSUM_N = VSUM_REASON + VS_VIS_R_N, VC_N = VC_SUMS + 2 * VSUM_N };

// t_infomask / t_infomask2 (access/htup_details.h)
enum : uint32_t { HV_KEYSHR_LOCK = 0x0010, HV_COMBOCID = 0x0020, HV_EXCL_LOCK = 0x0040, HV_XMAX_LOCK_ONLY = 0x0080, HV_XMIN_COMMITTED = 0x0100,
                  HV_XMIN_INVALID = 0x0200, HV_XMIN_FROZEN = 0x0300, HV_XMAX_COMMITTED = 0x0400, HV_XMAX_INVALID = 0x0800,
                  HV_XMAX_IS_MULTI = 0x1000, HV_MOVED = 0xC000, HV2_HOT_UPDATED = 0x4000, HV2_ONLY_TUPLE = 0x8000 };

struct HeapVisArgs {
    const uint8_t* pages;  // [n_blocks][page_size], the resident fork
    uint32_t page_size, n_blocks;
    const uint64_t* tids;  // [n] (block << 16) | offset
    uint32_t n;
    // SnapshotData; xip, subxip and own ascending (as unsigned numbers: they are only searched for equality)
    uint32_t xmin, xmax, xcnt, subxcnt, n_own, curcid;
    const uint32_t *xip, *subxip, *own;
    int32_t suboverflowed, recovery;
    uint32_t clog_first, clog_n;  // the window of pg_xact
    const uint8_t* clog;
    uint8_t* visible;     // [n]
    uint32_t* undecided;  // [n] in the order the waves appended, or nullptr: the list is not wanted
    uint32_t* ctr;
    // k_heap_vis_base only: the horizon the consulted xids are held against, and the bitmap of changed blocks (one bit per block below
    // map_blocks; nullptr: every node is walked)
    uint32_t horizon;
    const uint32_t* block_map;
    uint32_t map_blocks;
};

// TransactionIdPrecedes / TransactionIdFollowsOrEquals (access/transam.c): modulo-2^32 for normal xids, plain for the special ones
__device__ __forceinline__ bool vis_precedes(uint32_t a, uint32_t b) { return (a >= 3 && b >= 3) ? (int32_t)(a - b) < 0 : a < b; }
__device__ __forceinline__ bool vis_follows_eq(uint32_t a, uint32_t b) { return (a >= 3 && b >= 3) ? (int32_t)(a - b) >= 0 : a >= b; }
// HEAP_XMAX_IS_LOCKED_ONLY
__device__ __forceinline__ bool vis_locked_only(uint32_t m) {
    return (m & HV_XMAX_LOCK_ONLY) || (m & (HV_XMAX_IS_MULTI | HV_EXCL_LOCK | HV_KEYSHR_LOCK)) == HV_EXCL_LOCK;
}
__device__ __forceinline__ bool vis_member(const uint32_t* __restrict__ v, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && v[lo] == x;
}
// TransactionIdDidCommit over the window of pg_xact (TransactionLogFetch: the bootstrap and frozen xids committed, the invalid one
// did not); sub-committed needs pg_subtrans -> VV_INVISIBLE (no) / VV_VISIBLE (yes) / VV_UNDECIDED + reason
// What the base evaluation (k_heap_vis_base) remembers of a walk: whether any normal xid handed to own(), in_snapshot() or
// did_commit() follows or equals the horizon.  The snapshot evaluation (k_heap_vis) tracks nothing: TRACK = false compiles to the rule alone.
template <bool TRACK>
__device__ __forceinline__ void vis_consult(const HeapVisArgs& a, uint32_t x, bool& recent) {
    if (TRACK && x >= 3u && vis_follows_eq(x, a.horizon)) recent = true;
}
// TransactionIdIsCurrentTransactionId over the backend's own xids
template <bool TRACK>
__device__ __forceinline__ bool vis_own(const HeapVisArgs& a, uint32_t x, bool& recent) {
    vis_consult<TRACK>(a, x, recent);
    return vis_member(a.own, a.n_own, x);
}
template <bool TRACK>
__device__ __forceinline__ uint32_t vis_did_commit(const HeapVisArgs& a, uint32_t x, bool& recent) {
    vis_consult<TRACK>(a, x, recent);
    if (x == 1u || x == 2u) return VV_VISIBLE;
    if (x == 0u) return VV_INVISIBLE;
    const uint32_t i = x - a.clog_first;
    if (i >= a.clog_n) return VV_UNDECIDED + VS_VIS_R_CLOG_RANGE;
    const uint32_t st = (a.clog[i >> 2] >> ((i & 3u) * 2u)) & 3u;
    if (st == 3u) return VV_UNDECIDED + VS_VIS_R_SUBCOMMITTED;
    return st == 1u ? VV_VISIBLE : VV_INVISIBLE;
}
// XidInMVCCSnapshot (utils/time/snapmgr.c) -> no / yes / undecided, encoded as above
template <bool TRACK>
__device__ __forceinline__ uint32_t vis_in_snapshot(const HeapVisArgs& a, uint32_t x, bool& recent) {
    vis_consult<TRACK>(a, x, recent);
    if (vis_precedes(x, a.xmin)) return VV_INVISIBLE;
    if (vis_follows_eq(x, a.xmax)) return VV_VISIBLE;
    if (!a.recovery) {
        if (!a.suboverflowed) {
            if (vis_member(a.subxip, a.subxcnt, x)) return VV_VISIBLE;
            return vis_member(a.xip, a.xcnt, x) ? VV_VISIBLE : VV_INVISIBLE;
        }
        if (vis_member(a.xip, a.xcnt, x)) return VV_VISIBLE;
        return VV_UNDECIDED + VS_VIS_R_SUBOVERFLOW;  // SubTransGetTopmostTransaction
    }
    if (vis_member(a.subxip, a.subxcnt, x)) return VV_VISIBLE;
    return a.suboverflowed ? VV_UNDECIDED + VS_VIS_R_SUBOVERFLOW : VV_INVISIBLE;
}

// HeapTupleSatisfiesMVCC (access/heap/heapam_visibility.c), statement by statement, without the hint-bit writes
template <bool TRACK>
__device__ __forceinline__ uint32_t vis_satisfies_mvcc(const HeapVisArgs& a, uint32_t xmin, uint32_t xmax, uint32_t cid, uint32_t m, bool& recent) {
    if (!(m & HV_XMIN_COMMITTED)) {
        if (m & HV_XMIN_INVALID) return VV_INVISIBLE;
        if (m & HV_MOVED) return VV_UNDECIDED + VS_VIS_R_MOVED;  // HEAP_MOVED_OFF / HEAP_MOVED_IN: pre-9.0 VACUUM FULL
        if (vis_own<TRACK>(a, xmin, recent)) {                  // TransactionIdIsCurrentTransactionId(xmin)
            if (m & HV_COMBOCID) return VV_UNDECIDED + VS_VIS_R_COMBOCID;
            if (cid >= a.curcid) return VV_INVISIBLE;  // inserted after the scan started
            if (m & HV_XMAX_INVALID) return VV_VISIBLE;
            if (vis_locked_only(m)) return VV_VISIBLE;
            if (m & HV_XMAX_IS_MULTI) return VV_UNDECIDED + VS_VIS_R_MULTIXACT;  // HeapTupleGetUpdateXid
            if (!vis_own<TRACK>(a, xmax, recent)) return VV_VISIBLE;            // the deleting subtransaction must have aborted
            return cid >= a.curcid ? VV_VISIBLE : VV_INVISIBLE;                  // deleted after / before the scan started
        }
        const uint32_t s = vis_in_snapshot<TRACK>(a, xmin, recent);
        if (s != VV_INVISIBLE) return s == VV_VISIBLE ? (uint32_t)VV_INVISIBLE : s;
        const uint32_t c = vis_did_commit<TRACK>(a, xmin, recent);
        if (c != VV_VISIBLE) return c;  // aborted or crashed: invisible; or undecided
    } else if ((m & HV_XMIN_FROZEN) != HV_XMIN_FROZEN) {  // xmin is committed, but maybe not according to our snapshot
        const uint32_t s = vis_in_snapshot<TRACK>(a, xmin, recent);
        if (s != VV_INVISIBLE) return s == VV_VISIBLE ? (uint32_t)VV_INVISIBLE : s;
    }
    // by here, the inserting transaction has committed
    if (m & HV_XMAX_INVALID) return VV_VISIBLE;
    if (vis_locked_only(m)) return VV_VISIBLE;
    if (m & HV_XMAX_IS_MULTI) return VV_UNDECIDED + VS_VIS_R_MULTIXACT;
    if (!(m & HV_XMAX_COMMITTED)) {
        if (vis_own<TRACK>(a, xmax, recent)) {
            if (m & HV_COMBOCID) return VV_UNDECIDED + VS_VIS_R_COMBOCID;
            return cid >= a.curcid ? VV_VISIBLE : VV_INVISIBLE;
        }
        const uint32_t s = vis_in_snapshot<TRACK>(a, xmax, recent);
        if (s != VV_INVISIBLE) return s;  // the deleter is still running for us: visible; or undecided
        const uint32_t c = vis_did_commit<TRACK>(a, xmax, recent);
        if (c != VV_VISIBLE) return c == VV_INVISIBLE ? (uint32_t)VV_VISIBLE : c;  // it aborted or crashed: visible
    } else {
        const uint32_t s = vis_in_snapshot<TRACK>(a, xmax, recent);
        if (s != VV_INVISIBLE) return s;
    }
    return VV_INVISIBLE;  // the deleting transaction committed
}

// heap_hot_search_buffer (access/heap/heapam.c; what table_index_fetch_tuple runs) for one tid -> VK_*; reason: VS_VIS_R_* of
// VK_UNDECIDED; hops: chain members whose header was read beyond the first
template <bool TRACK>
__device__ __forceinline__ uint32_t vis_hot_search(const HeapVisArgs& a, uint64_t tid, uint32_t& reason, uint32_t& hops, bool& recent) {
    reason = 0;
    hops = 0;
    uint32_t off = (uint32_t)(tid & 0xFFFFu);
    if (off == 0) return VK_DELETED;  // a vacuumed index tuple
    const uint64_t blk64 = tid >> 16;
    if (blk64 >= a.n_blocks) return VK_NOT_FOUND;
    const uint32_t blk = (uint32_t)blk64;
    const uint8_t* page = a.pages + (size_t)blk * a.page_size;
    HeapPage pg;
    uint32_t detail = 0;
    const uint32_t pe = heap_page_view(page, a.page_size, pg, detail);
    if (pe != HE_OK) {
        heap_error(a.ctr, pe, 0, blk, off, detail);
        return VK_ERROR;
    }
    bool at_start = true;
    uint32_t prev_xmax = 0, members = 0;
    for (uint32_t round = 0;; ++round) {
        if (off < 1 || off > pg.nitems) return round == 0 ? VK_NOT_FOUND : VK_INVISIBLE;
        if (round >= pg.nitems) {  // every line pointer of the page could have been visited once by now
            heap_error(a.ctr, HE_CHAIN_CYCLE, 0, blk, off, round);
            return VK_ERROR;
        }
        const uint32_t lp = ld32(page + 24 + 4 * (off - 1));
        const uint32_t lp_off = lp & 0x7FFFu, fl = (lp >> 15) & 3u, lp_len = lp >> 17;
        if (fl != 1u) {
            if (fl == 2u && at_start) {  // LP_REDIRECT is only allowed at the start of a chain
                off = lp_off;
                at_start = false;
                continue;
            }
            return (round == 0 && fl != 2u) ? VK_DEAD_LP : VK_INVISIBLE;
        }
        if (!heap_item_in_bounds(pg, lp_off, lp_len)) {
            heap_error(a.ctr, HE_ITEM_BOUNDS, 0, blk, off, lp);
            return VK_ERROR;
        }
        const uint8_t* t = page + lp_off;  // (tuples are MAXALIGNed by PageAddItem; a fabricated offset need not be)
        const uint32_t xmin = ldu32(t), xmax = ldu32(t + 4), cid = ldu32(t + 8);
        const uint32_t m2 = ldu16(t + 18), m = ldu16(t + 20);
        hops += members ? 1u : 0u;
        ++members;
        if (at_start && (m2 & HV2_ONLY_TUPLE)) return VK_INVISIBLE;  // a heap-only tuple cannot start a chain
        // the xmin must match the previous member's xmax, else the chain is broken (HeapTupleHeaderGetXmin: a frozen xmin reads as 2)
        if (prev_xmax != 0 && prev_xmax != ((m & HV_XMIN_FROZEN) == HV_XMIN_FROZEN ? 2u : xmin)) return VK_INVISIBLE;
        const uint32_t r = vis_satisfies_mvcc<TRACK>(a, xmin, xmax, cid, m, recent);
        if (r == VV_VISIBLE) return VK_VISIBLE;
        if (r >= VV_UNDECIDED) {
            reason = r - VV_UNDECIDED;
            return VK_UNDECIDED;
        }
        // HeapTupleIsHotUpdated: HOT_UPDATED, an xmax, and an xmin that is not known aborted
        if ((m2 & HV2_HOT_UPDATED) && !(m & HV_XMAX_INVALID) && (m & HV_XMIN_FROZEN) != HV_XMIN_INVALID) {
            if ((m & HV_XMAX_IS_MULTI) && !vis_locked_only(m)) {  // HeapTupleHeaderGetUpdateXid needs the members
                reason = VS_VIS_R_MULTIXACT;
                return VK_UNDECIDED;
            }
            off = ldu16(t + 16);  // ItemPointerGetOffsetNumber(&t_ctid): a HOT chain stays on its page
            at_start = false;
            prev_xmax = xmax;
        } else {
            return VK_INVISIBLE;
        }
    }
}

// a lane per node, 64 nodes a round of a wave.  The counters are reduced per wave — ballots counted into wave-uniform sums over all
// the rounds of the wave, one butterfly for the hops at the end — and added with one atomic per wave and counter when the wave is
// done (an atomic per round and counter on the same few words serialises the whole grid: measured 1.59 ms at 4 M nodes, DESIGN.md
// 7o).  The undecided nodes of a round are appended behind one atomic on the list's counter.
__global__ __launch_bounds__(WAVE) void k_heap_vis(HeapVisArgs a) {
    const uint32_t lane = threadIdx.x;
    uint32_t sum[VSUM_N] = {0};  // (a wave judges fewer than 2^32 nodes)
    uint32_t hops_lane = 0;
    for (uint32_t base = blockIdx.x * WAVE; base < a.n; base += gridDim.x * WAVE) {
        const uint32_t i = base + lane;
        uint32_t kind = VK_ERROR, reason = 0, hops = 0;
        if (i < a.n) {
            bool unused = false;
            kind = vis_hot_search<false>(a, a.tids[i], reason, hops, unused);
            a.visible[i] = (kind == VK_VISIBLE || kind == VK_UNDECIDED) ? 1 : 0;
        }
        hops_lane += hops;
        const uint64_t m_und = __ballot(kind == VK_UNDECIDED);
        const uint32_t n_del = (uint32_t)__popcll(__ballot(kind == VK_DELETED)), n_nf = (uint32_t)__popcll(__ballot(kind == VK_NOT_FOUND));
        const uint32_t n_dead = (uint32_t)__popcll(__ballot(kind == VK_DEAD_LP));
        sum[VSUM_VISIBLE] += (uint32_t)__popcll(__ballot(kind == VK_VISIBLE));
        sum[VSUM_INVISIBLE] += (uint32_t)__popcll(__ballot(kind == VK_INVISIBLE)) + n_del + n_nf + n_dead;
        sum[VSUM_DELETED] += n_del;
        sum[VSUM_NOT_FOUND] += n_nf;
        sum[VSUM_DEAD_LP] += n_dead;
        if (m_und) {  // (wave-uniform)
            sum[VSUM_UNDECIDED] += (uint32_t)__popcll(m_und);
            for (uint32_t r = 0; r < VS_VIS_R_N; ++r) sum[VSUM_REASON + r] += (uint32_t)__popcll(__ballot(kind == VK_UNDECIDED && reason == r));
            if (a.undecided) {
                uint32_t at = 0;
                if (lane == 0) at = atomicAdd(&a.ctr[VC_NLIST], (uint32_t)__popcll(m_und));
                at = __shfl(at, 0);
                // (at most one entry per node: at + popc <= n, the list's size)
                if (kind == VK_UNDECIDED) a.undecided[at + (uint32_t)__popcll(m_und & ((1ull << lane) - 1ull))] = i;
            }
        }
    }
    for (uint32_t o = WAVE / 2; o; o >>= 1) hops_lane += __shfl_xor(hops_lane, o);
    sum[VSUM_HOPS] = hops_lane;
    if (lane == 0) {
        unsigned long long* sums = reinterpret_cast<unsigned long long*>(a.ctr + VC_SUMS);
        for (uint32_t k = 0; k < VSUM_N; ++k)
            if (sum[k]) atomicAdd(&sums[k], (unsigned long long)sum[k]);
    }
}

// snapshot_patch: mask[nodes[i]] = values[i] != 0 (the host has left one entry per node)
__global__ __launch_bounds__(256) void k_mask_patch(uint8_t* __restrict__ mask, const uint32_t* __restrict__ nodes,
                                                    const uint8_t* __restrict__ values, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) mask[nodes[i]] = values[i] ? 1 : 0;
}

// ---- the resident fork ------------------------------------------------------------------------------------------------------------
struct vs_heap_res {
    vs_ctx* ctx = nullptr;
    uint32_t page_size = VS_BLCKSZ, cap_blocks = 0, n_blocks = 0;  // n_blocks: one past the highest block ever put
    uint8_t* d_pages = nullptr;                                    // [cap_blocks][page_size]; a block never put is all zero
    hipEvent_t ev = nullptr;                                       // orders the copy stream behind the kernels that read the pages
};

static void heap_res_free(vs_heap_res* h) {
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->copy_stream);
    (void)hipStreamSynchronize(h->ctx->stream);
    if (h->d_pages) (void)hipFree(h->d_pages);
    if (h->ev) (void)hipEventDestroy(h->ev);
    delete h;
}

extern "C" int vs_heap_res_open(vs_ctx* ctx, uint32_t page_size, uint32_t n_blocks_capacity, vs_heap_res** out) {
    VS_REQUIRE(ctx && out, "vs_heap_res_open: bad arguments");
    VS_REQUIRE(page_size >= 512 && page_size <= 32768 && !(page_size & (page_size - 1)), "vs_heap_res_open: page size %u", page_size);
    *out = nullptr;
    VS_REQUIRE(ctx->pinned_bytes >= page_size, "vs_heap_res_open: the context's staging buffers (%zu bytes) do not hold one page", ctx->pinned_bytes);
    return vs_guard("vs_heap_res_open", [&]() -> int {
        vs_heap_res* h = new vs_heap_res();
        h->ctx = ctx;
        h->page_size = page_size;
        h->cap_blocks = std::max(n_blocks_capacity, 1u);
        auto run = [&]() -> int {
            VS_HIP(hipSetDevice(ctx->device));
            VS_HIP(hipEventCreateWithFlags(&h->ev, hipEventDisableTiming));
            VS_HIP(hipMalloc(&h->d_pages, (size_t)h->cap_blocks * page_size));
            VS_HIP(hipMemsetAsync(h->d_pages, 0, (size_t)h->cap_blocks * page_size, ctx->stream));
            VS_HIP(hipStreamSynchronize(ctx->stream));
            return VS_OK;
        };
        const int r = run();
        if (r != VS_OK) {
            heap_res_free(h);
            return r;
        }
        *out = h;
        return VS_OK;
    });
}

// room for `blocks` blocks: the growth rule of vs_index_reserve (by half, at least to fit, device to device; the pointers change
// hands only when every step has succeeded)
static int heap_res_reserve(vs_heap_res* h, uint32_t blocks) {
    if (blocks <= h->cap_blocks) return VS_OK;
    vs_ctx* c = h->ctx;
    const uint32_t cap = (uint32_t)std::max<uint64_t>(blocks, std::min<uint64_t>((uint64_t)h->cap_blocks + h->cap_blocks / 2, 0xFFFFFFFFull));
    const size_t total = (size_t)cap * h->page_size, keep = (size_t)h->n_blocks * h->page_size;
    uint8_t* fresh = nullptr;
    hipError_t e = hipMalloc(&fresh, total);
    if (e == hipSuccess && keep) e = hipMemcpyAsync(fresh, h->d_pages, keep, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(fresh + keep, 0, total - keep, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        vs_set_error("vs_heap_res_put: growing to %u blocks failed: %s", cap, hipGetErrorString(e));
        (void)hipGetLastError();
        (void)hipStreamSynchronize(c->stream);
        if (fresh) (void)hipFree(fresh);
        return e == hipErrorOutOfMemory ? VS_ERR_OOM : VS_ERR_HIP;
    }
    (void)hipFree(h->d_pages);
    h->d_pages = fresh;
    h->cap_blocks = cap;
    return VS_OK;
}

extern "C" int vs_heap_res_put(vs_heap_res* h, uint32_t first_block, const void* pages, uint32_t n_blocks) {
    VS_REQUIRE(h && (pages || !n_blocks), "vs_heap_res_put: null argument");
    VS_REQUIRE((uint64_t)first_block + n_blocks <= 0xFFFFFFFFull, "vs_heap_res_put: blocks %u + %u pass the end of a relation", first_block, n_blocks);
    if (!n_blocks) return VS_OK;
    return vs_guard("vs_heap_res_put", [&]() -> int {
        vs_ctx* c = h->ctx;
        VS_HIP(hipSetDevice(c->device));
        VS_TRY(heap_res_reserve(h, first_block + n_blocks));
        // the copies overwrite pages an evaluation on the compute stream may still be reading
        VS_HIP(hipEventRecord(h->ev, c->stream));
        VS_HIP(hipStreamWaitEvent(c->copy_stream, h->ev, 0));
        const uint32_t per = (uint32_t)(c->pinned_bytes / h->page_size);
        const uint8_t* src = static_cast<const uint8_t*>(pages);
        uint8_t* dst = h->d_pages + (size_t)first_block * h->page_size;
        int s = 0;
        for (uint32_t b0 = 0; b0 < n_blocks; b0 += per, s ^= 1) {
            const size_t bytes = (size_t)std::min(per, n_blocks - b0) * h->page_size, at = (size_t)b0 * h->page_size;
            VS_HIP(hipEventSynchronize(c->pinned_ev[s]));  // the pinned buffer's last copy has left it
            stage_copy(c->pinned[s], src + at, bytes);
            VS_HIP(hipMemcpyAsync(dst + at, c->pinned[s], bytes, hipMemcpyHostToDevice, c->copy_stream));
            VS_HIP(hipEventRecord(c->pinned_ev[s], c->copy_stream));
            VS_HIP(hipStreamWaitEvent(c->stream, c->pinned_ev[s], 0));  // an evaluation that follows sees the new pages
        }
        h->n_blocks = std::max(h->n_blocks, first_block + n_blocks);
        return VS_OK;
    });
}

extern "C" uint32_t vs_heap_res_blocks(const vs_heap_res* h) { return h ? h->n_blocks : 0; }
extern "C" void vs_heap_res_close(vs_heap_res* h) { heap_res_free(h); }

// ---- the evaluation ---------------------------------------------------------------------------------------------------------------
// the argument checks every entry point makes before any device call
static int heap_vis_check(const char* what, const vs_mvcc_snapshot* s, const vs_xact_status* x, const uint32_t* undecided_nodes, uint32_t cap) {
    VS_REQUIRE(s && x, "%s: the snapshot and the transaction status window are required", what);
    VS_REQUIRE((s->xip || !s->xcnt) && (s->subxip || !s->subxcnt) && (s->own_xids || !s->n_own), "%s: a snapshot array is NULL with a count above 0", what);
    VS_REQUIRE(s->xcnt <= (1u << 28) && s->subxcnt <= (1u << 28) && s->n_own <= (1u << 28), "%s: a snapshot array of more than 2^28 xids", what);
    VS_REQUIRE(!(x->first_xid & 3u), "%s: first_xid %u is not a multiple of 4", what, x->first_xid);
    VS_REQUIRE(x->bits || !x->n_xids, "%s: the transaction status bits are NULL with n_xids above 0", what);
    VS_REQUIRE(undecided_nodes || !cap, "%s: undecided_nodes is NULL with a capacity above 0", what);
    return VS_OK;
}

static int heap_vis_run(vs_heap_res* h, const uint64_t* d_tids, uint32_t n, const vs_mvcc_snapshot* s, const vs_xact_status* x, uint8_t* d_visible,
                        vs_vis_stats* out, uint32_t* undecided_nodes, uint32_t cap, uint32_t* n_undecided) {
    vs_ctx* c = h->ctx;
    hipStream_t st = c->stream;
    VS_HIP(hipSetDevice(c->device));
    // one upload: xip | subxip | own, each sorted, then the status bits
    const size_t n_x = (size_t)s->xcnt + s->subxcnt + s->n_own, clog_bytes = ((size_t)x->n_xids + 3) / 4;
    std::vector<uint32_t> aux(n_x + (clog_bytes + 3) / 4 + 1, 0u);
    if (s->xcnt) memcpy(aux.data(), s->xip, (size_t)s->xcnt * 4);
    if (s->subxcnt) memcpy(aux.data() + s->xcnt, s->subxip, (size_t)s->subxcnt * 4);
    if (s->n_own) memcpy(aux.data() + s->xcnt + s->subxcnt, s->own_xids, (size_t)s->n_own * 4);
    std::sort(aux.begin(), aux.begin() + s->xcnt);
    std::sort(aux.begin() + s->xcnt, aux.begin() + s->xcnt + s->subxcnt);
    std::sort(aux.begin() + s->xcnt + s->subxcnt, aux.begin() + n_x);
    if (clog_bytes) memcpy(aux.data() + n_x, x->bits, clog_bytes);
    uint32_t *d_aux = nullptr, *d_ctr = nullptr, *d_list = nullptr, *d_sorted = nullptr, *d_vals = nullptr;
    void* d_tmp = nullptr;
    uint32_t h_ctr[VC_N] = {0};
    uint32_t n_list = 0;
    auto run = [&]() -> int {
        VS_HIP(hipMalloc(&d_aux, aux.size() * 4));
        VS_HIP(hipMalloc(&d_ctr, VC_N * 4));
        if (cap && n) VS_HIP(hipMalloc(&d_list, (size_t)n * 4));
        VS_TRY(vs_dev_upload(c, d_aux, aux.data(), aux.size() * 4));
        VS_HIP(hipMemsetAsync(d_ctr, 0, VC_N * 4, st));
        if (n) {
            HeapVisArgs a{};
            a.pages = h->d_pages;
            a.page_size = h->page_size;
            a.n_blocks = h->n_blocks;
            a.tids = d_tids;
            a.n = n;
            a.xmin = s->xmin;
            a.xmax = s->xmax;
            a.xcnt = s->xcnt;
            a.subxcnt = s->subxcnt;
            a.n_own = s->n_own;
            a.curcid = s->curcid;
            a.xip = d_aux;
            a.subxip = d_aux + s->xcnt;
            a.own = d_aux + s->xcnt + s->subxcnt;
            a.suboverflowed = s->suboverflowed;
            a.recovery = s->taken_during_recovery;
            a.clog_first = x->first_xid;
            a.clog_n = x->n_xids;
            a.clog = reinterpret_cast<const uint8_t*>(d_aux + n_x);
            a.visible = d_visible;
            a.undecided = d_list;
            a.ctr = d_ctr;
            hipEvent_t ev = prof_begin(c);
            // as many waves as the device holds at once (32 a CU), each walking its rounds of 64 nodes
            const uint64_t resident = (uint64_t)std::max(c->prop.multiProcessorCount, 1) * 32;
            hipLaunchKernelGGL(k_heap_vis, dim3((uint32_t)std::min<uint64_t>(((uint64_t)n + WAVE - 1) / WAVE, resident)), dim3(WAVE), 0, st, a);
            VS_HIP(hipGetLastError());
            prof_end(c, PK_PAGES, ev);
        }
        VS_HIP(hipMemcpyAsync(h_ctr, d_ctr, VC_N * 4, hipMemcpyDeviceToHost, st));
        VS_HIP(hipStreamSynchronize(st));
        if (h_ctr[HC_ERR] != HE_OK) {
            const uint32_t* e = h_ctr + HC_ERR;
            vs_set_error("heap block %u item %u: %s (detail %u)", e[1], e[2], kHeapErrorText[e[0] <= HE_LAST ? e[0] : 0], e[3]);
            return VS_ERR_INVALID;
        }
        n_list = d_list ? std::min(h_ctr[VC_NLIST], n) : 0;
        if (n_list) {  // ascending, whatever order the waves appended in
            VS_HIP(hipMalloc(&d_sorted, (size_t)n_list * 4));
            VS_HIP(hipMalloc(&d_vals, (size_t)n_list * 4));
            size_t tmp_bytes = 0;
            VS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (const uint32_t*)d_list, d_sorted, (const uint32_t*)d_list, d_vals,
                                                      (int)n_list, 0, 32, st));
            VS_HIP(hipMalloc(&d_tmp, tmp_bytes + 16));
            VS_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp_bytes, (const uint32_t*)d_list, d_sorted, (const uint32_t*)d_list, d_vals,
                                                      (int)n_list, 0, 32, st));
            VS_HIP(hipStreamSynchronize(st));
            VS_TRY(vs_dev_download(c, undecided_nodes, d_sorted, (size_t)std::min(n_list, cap) * 4));
        }
        return VS_OK;
    };
    const int r = run();
    if (r != VS_OK) (void)hipStreamSynchronize(st);
    void* ptrs[] = {d_aux, d_ctr, d_list, d_sorted, d_vals, d_tmp};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    VS_TRY(r);
    uint64_t sums[VSUM_N];
    memcpy(sums, h_ctr + VC_SUMS, sizeof(sums));
    if (out) {
        vs_vis_stats S{};
        S.n_visible = sums[VSUM_VISIBLE];
        S.n_invisible = sums[VSUM_INVISIBLE];
        S.n_undecided = sums[VSUM_UNDECIDED];
        S.n_deleted = sums[VSUM_DELETED];
        S.n_not_found = sums[VSUM_NOT_FOUND];
        S.n_dead_line_pointer = sums[VSUM_DEAD_LP];
        S.chain_hops = sums[VSUM_HOPS];
        for (int k = 0; k < VS_VIS_R_N; ++k) S.undecided_by_reason[k] = sums[VSUM_REASON + k];
        *out = S;
    }
    if (n_undecided) *n_undecided = (uint32_t)sums[VSUM_UNDECIDED];
    return VS_OK;
}

extern "C" int vs_heap_res_visibility(vs_heap_res* h, const uint64_t* d_heap_tids, uint32_t n, const vs_mvcc_snapshot* snapshot,
                                      const vs_xact_status* xact, uint8_t* d_visible, vs_vis_stats* out, uint32_t* undecided_nodes, uint32_t cap,
                                      uint32_t* n_undecided) {
    VS_REQUIRE(h && (!n || (d_heap_tids && d_visible)), "vs_heap_res_visibility: null argument");
    VS_REQUIRE(n <= 0x7FFFFFFFu, "vs_heap_res_visibility: %u nodes", n);
    VS_TRY(heap_vis_check("vs_heap_res_visibility", snapshot, xact, undecided_nodes, cap));
    return vs_guard("vs_heap_res_visibility",
                    [&] { return heap_vis_run(h, d_heap_tids, n, snapshot, xact, d_visible, out, undecided_nodes, cap, n_undecided); });
}

// ---- on the index -----------------------------------------------------------------------------------------------------------------
// the refusals of vs_index_snapshot_put, and a batch in flight (its launches read the masks)
static int snapshot_write_check(const char* what, vs_index* ix, uint32_t snapshot) {
    VS_REQUIRE(ix && snapshot >= 1 && snapshot < VS_MAX_SNAPSHOTS, "%s: snapshot id outside [1,%d]", what, VS_MAX_SNAPSHOTS - 1);
    if (ix->ws.pending) {
        vs_set_error("%s: a batch of this handle is in flight (vs_search_batch_dev_finish first)", what);
        return VS_ERR_STATE;
    }
    return VS_OK;
}
// the library-owned mask of a snapshot id, allocated as vs_index_snapshot_put allocates it: at capacity, so that an insert can grow it
static int snapshot_mask(vs_index* ix, uint32_t snapshot, bool* fresh) {
    *fresh = !ix->snap[snapshot];
    if (*fresh) VS_HIP(hipMalloc(&ix->snap[snapshot], std::max<size_t>(std::max(ix->d.n, ix->capacity), 1)));
    else VS_HIP(hipStreamSynchronize(ix->ctx->stream));  // (replacing a mask a launch may still be reading)
    return VS_OK;
}
static void snapshot_drop(vs_index* ix, uint32_t snapshot) {
    (void)hipStreamSynchronize(ix->ctx->stream);
    if (ix->visible == ix->snap[snapshot]) ix->visible = nullptr;
    (void)hipFree(ix->snap[snapshot]);
    ix->snap[snapshot] = nullptr;
}

extern "C" int vs_index_snapshot_eval(vs_index* ix, vs_heap_res* h, uint32_t snapshot, const vs_mvcc_snapshot* snap, const vs_xact_status* xact,
                                      vs_vis_stats* out, uint32_t* undecided_nodes, uint32_t cap, uint32_t* n_undecided) {
    VS_TRY(snapshot_write_check("vs_index_snapshot_eval", ix, snapshot));
    VS_REQUIRE(h, "vs_index_snapshot_eval: the resident heap fork is NULL");
    VS_REQUIRE(h->ctx == ix->ctx, "vs_index_snapshot_eval: the index and the resident heap fork belong to different contexts");
    VS_TRY(heap_vis_check("vs_index_snapshot_eval", snap, xact, undecided_nodes, cap));
    VS_REQUIRE(ix->tids || !ix->d.n, "vs_index_snapshot_eval: the index has no heap tid column");
    return vs_guard("vs_index_snapshot_eval", [&]() -> int {
        VS_HIP(hipSetDevice(ix->ctx->device));
        bool fresh = false;
        VS_TRY(snapshot_mask(ix, snapshot, &fresh));
        const int r = heap_vis_run(h, ix->tids, ix->d.n, snap, xact, ix->snap[snapshot], out, undecided_nodes, cap, n_undecided);
        if (r != VS_OK) snapshot_drop(ix, snapshot);  // (a mask half written is no mask)
        return r;
    });
}

extern "C" int vs_index_snapshot_put_dev(vs_index* ix, uint32_t snapshot, const uint8_t* d_visible) {
    VS_TRY(snapshot_write_check("vs_index_snapshot_put_dev", ix, snapshot));
    VS_REQUIRE(d_visible || !ix->d.n, "vs_index_snapshot_put_dev: the mask is NULL (vs_index_snapshot_put(NULL) drops a mask)");
    return vs_guard("vs_index_snapshot_put_dev", [&]() -> int {
        VS_HIP(hipSetDevice(ix->ctx->device));
        bool fresh = false;
        VS_TRY(snapshot_mask(ix, snapshot, &fresh));
        if (ix->d.n) VS_HIP(hipMemcpyAsync(ix->snap[snapshot], d_visible, ix->d.n, hipMemcpyDeviceToDevice, ix->ctx->stream));
        VS_HIP(hipStreamSynchronize(ix->ctx->stream));  // (the caller's buffer is its own again)
        return VS_OK;
    });
}

extern "C" int vs_index_snapshot_patch(vs_index* ix, uint32_t snapshot, const uint32_t* nodes, const uint8_t* values, uint32_t n) {
    VS_TRY(snapshot_write_check("vs_index_snapshot_patch", ix, snapshot));
    VS_REQUIRE((nodes && values) || !n, "vs_index_snapshot_patch: null argument");
    if (!ix->snap[snapshot]) {
        vs_set_error("vs_index_snapshot_patch: snapshot %u has no visibility mask (vs_index_snapshot_eval / _put)", snapshot);
        return VS_ERR_STATE;
    }
    for (uint32_t i = 0; i < n; ++i) VS_REQUIRE(nodes[i] < ix->d.n, "vs_index_snapshot_patch: node %u of %u", nodes[i], ix->d.n);
    if (!n) return VS_OK;
    return vs_guard("vs_index_snapshot_patch", [&]() -> int {
        // one entry per node, the last one given: the scatter writes no byte twice
        std::vector<std::pair<uint32_t, uint32_t>> order(n);
        for (uint32_t i = 0; i < n; ++i) order[i] = {nodes[i], i};
        std::sort(order.begin(), order.end());
        std::vector<uint32_t> un;
        std::vector<uint8_t> uv;
        for (uint32_t i = 0; i < n; ++i)
            if (i + 1 == n || order[i + 1].first != order[i].first) {
                un.push_back(order[i].first);
                uv.push_back(values[order[i].second]);
            }
        vs_ctx* c = ix->ctx;
        VS_HIP(hipSetDevice(c->device));
        uint32_t* d_nodes = nullptr;
        uint8_t* d_vals = nullptr;
        auto run = [&]() -> int {
            VS_HIP(hipMalloc(&d_nodes, un.size() * 4));
            VS_HIP(hipMalloc(&d_vals, uv.size()));
            VS_TRY(vs_dev_upload(c, d_nodes, un.data(), un.size() * 4));
            VS_TRY(vs_dev_upload(c, d_vals, uv.data(), uv.size()));
            hipLaunchKernelGGL(k_mask_patch, dim3(heap_dev_grid(un.size(), 256)), dim3(256), 0, c->stream, ix->snap[snapshot],
                               (const uint32_t*)d_nodes, (const uint8_t*)d_vals, (uint32_t)un.size());
            VS_HIP(hipGetLastError());
            VS_HIP(hipStreamSynchronize(c->stream));
            return VS_OK;
        };
        const int r = run();
        if (r != VS_OK) (void)hipStreamSynchronize(c->stream);
        if (d_nodes) (void)hipFree(d_nodes);
        if (d_vals) (void)hipFree(d_vals);
        return r;
    });
}

// ---- the base and its overlays (vs_index_vis_base_eval, vs_index_vis_slot_*; include/vsgpu.h has the rule) -----------------------------
// Almost every tuple is visible, or invisible, to every snapshot that can exist: only rows touched at or after the oldest-running horizon
// depend on who asks.  k_heap_vis_base walks every node once per heap state under the synthetic snapshot xmin = xmax = horizon and
// gives it a class byte; the class-2 nodes form the ascending depends list, and a snapshot's overlay is the rule run under that
// snapshot over the list's r nodes only (k_heap_vis over the gathered tids).  The search kernels read the class byte where they read
// a mask byte and look a class-2 node up in the list (vis_hidden, vs_device.h).
enum { BSUM_WALKED = 0, BSUM_DELETED, BSUM_NOT_FOUND, BSUM_DEAD_LP, BSUM_RECENT, BSUM_UNDECIDED, BSUM_HOPS, BSUM_REASON, BSUM_N = BSUM_REASON + VS_VIS_R_N,
       BC_N = VC_SUMS + 2 * BSUM_N };
enum { LC_CLASS = 0 /* three counts */, LC_NLIST = 3, LC_N = 4 };  // counters of k_vis_list (u32)

// k_heap_vis with the class for a verdict: a lane per node, the counters reduced per wave.  With a block bitmap only the nodes whose
// tid lies on a listed block are walked; every other class byte is left as it is.
__global__ __launch_bounds__(WAVE) void k_heap_vis_base(HeapVisArgs a) {
    const uint32_t lane = threadIdx.x;
    uint32_t sum[BSUM_N] = {0};
    uint32_t hops_lane = 0;
    for (uint32_t base = blockIdx.x * WAVE; base < a.n; base += gridDim.x * WAVE) {
        const uint32_t i = base + lane;
        uint32_t kind = VK_ERROR, reason = 0, hops = 0;
        bool walk = false, recent = false;
        if (i < a.n) {
            const uint64_t tid = a.tids[i];
            walk = true;
            if (a.block_map) {
                const uint64_t blk = tid >> 16;
                walk = blk < a.map_blocks && ((a.block_map[blk >> 5] >> (blk & 31u)) & 1u) != 0;
            }
            if (walk) {
                kind = vis_hot_search<true>(a, tid, reason, hops, recent);
                a.visible[i] = (kind == VK_UNDECIDED || recent) ? VIS_CLASS_DEPENDS : kind == VK_VISIBLE ? VIS_CLASS_ALL : VIS_CLASS_NONE;
            }
        }
        hops_lane += hops;
        const uint64_t m_und = __ballot(walk && kind == VK_UNDECIDED);
        sum[BSUM_WALKED] += (uint32_t)__popcll(__ballot(walk));
        sum[BSUM_DELETED] += (uint32_t)__popcll(__ballot(walk && kind == VK_DELETED));
        sum[BSUM_NOT_FOUND] += (uint32_t)__popcll(__ballot(walk && kind == VK_NOT_FOUND));
        sum[BSUM_DEAD_LP] += (uint32_t)__popcll(__ballot(walk && kind == VK_DEAD_LP));
        sum[BSUM_RECENT] += (uint32_t)__popcll(__ballot(walk && recent && kind != VK_UNDECIDED && kind != VK_ERROR));
        if (m_und) {  // (wave-uniform)
            sum[BSUM_UNDECIDED] += (uint32_t)__popcll(m_und);
            for (uint32_t r = 0; r < VS_VIS_R_N; ++r) sum[BSUM_REASON + r] += (uint32_t)__popcll(__ballot(walk && kind == VK_UNDECIDED && reason == r));
        }
    }
    for (uint32_t o = WAVE / 2; o; o >>= 1) hops_lane += __shfl_xor(hops_lane, o);
    sum[BSUM_HOPS] = hops_lane;
    if (lane == 0) {
        unsigned long long* sums = reinterpret_cast<unsigned long long*>(a.ctr + VC_SUMS);
        for (uint32_t k = 0; k < BSUM_N; ++k)
            if (sum[k]) atomicAdd(&sums[k], (unsigned long long)sum[k]);
    }
}

// the classes counted and the class-2 nodes appended behind one counter (sorted afterwards: nothing depends on scheduling)
__global__ __launch_bounds__(WAVE) void k_vis_list(const uint8_t* __restrict__ cls, uint32_t n, uint32_t* __restrict__ list, uint32_t* __restrict__ ctr) {
    const uint32_t lane = threadIdx.x;
    uint32_t n0 = 0, n1 = 0;
    for (uint32_t base = blockIdx.x * WAVE; base < n; base += gridDim.x * WAVE) {
        const uint32_t i = base + lane;
        const uint32_t c = i < n ? (uint32_t)cls[i] : 0xFFu;
        n0 += (uint32_t)__popcll(__ballot(c == VIS_CLASS_NONE));
        n1 += (uint32_t)__popcll(__ballot(c == VIS_CLASS_ALL));
        const uint64_t m2 = __ballot(c == VIS_CLASS_DEPENDS);
        if (m2) {  // (wave-uniform)
            uint32_t at = 0;
            if (lane == 0) at = atomicAdd(&ctr[LC_NLIST], (uint32_t)__popcll(m2));
            at = __shfl(at, 0);
            // (at most one entry per node: at + popc <= n, the list's size)
            if (c == VIS_CLASS_DEPENDS) list[at + (uint32_t)__popcll(m2 & ((1ull << lane) - 1ull))] = i;
        }
    }
    if (lane == 0) {
        if (n0) atomicAdd(&ctr[LC_CLASS + 0], n0);
        if (n1) atomicAdd(&ctr[LC_CLASS + 1], n1);
    }
}

__global__ __launch_bounds__(256) void k_vis_gather_tids(const uint64_t* __restrict__ tids, const uint32_t* __restrict__ dep, uint32_t r,
                                                         uint64_t* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < r; i += gridDim.x * blockDim.x) out[i] = tids[dep[i]];
}

// the byte mask of a legacy snapshot id from the base and one overlay: what vis_hidden tells a scan of that slot, node by node
__global__ __launch_bounds__(256) void k_vis_materialize(const uint8_t* __restrict__ cls, const uint32_t* __restrict__ dep, uint32_t r,
                                                         const uint8_t* __restrict__ ov, uint8_t* __restrict__ mask, uint32_t n) {
    const ScanVis s{cls, dep, ov, r};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) mask[i] = vis_hidden(s, i, cls[i]) ? 0 : 1;
}

// TransactionIdPrecedes on the host (the admission of a snapshot against the stored horizon)
static inline bool vis_precedes_host(uint32_t a, uint32_t b) { return (a >= 3 && b >= 3) ? (int32_t)(a - b) < 0 : a < b; }

// the scratch buffers of vis_base_run in VisBase::wk: the block bitmap + pg_xact window, both kernels' counters, the unsorted list,
// and what the radix sort wants (the interface of the sort used here takes values with its keys)
enum { VW_AUX = 0, VW_CTR, VW_LIST, VW_VALS, VW_TMP, VW_N };
static int vis_wk(VisBase* b, int which, size_t bytes, void** out) {
    if (b->wk_bytes[which] < bytes) {
        if (b->wk[which]) (void)hipFree(b->wk[which]);
        b->wk[which] = nullptr;
        b->wk_bytes[which] = 0;
        const size_t want = bytes + bytes / 2;  // (by half, as the index's arrays grow)
        VS_HIP(hipMalloc(&b->wk[which], want));
        b->wk_bytes[which] = want;
    }
    *out = b->wk[which];
    return VS_OK;
}
static void vis_wk_free(VisBase* b) {
    for (int k = 0; k < VW_N; ++k) {
        if (b->wk[k]) (void)hipFree(b->wk[k]);
        b->wk[k] = nullptr;
        b->wk_bytes[k] = 0;
    }
}

static void vis_overlays_drop(VisBase* b) {
    for (uint32_t s = 0; s < VS_MAX_VIS_SLOTS; ++s)
        if (b->overlay[s]) {
            (void)hipFree(b->overlay[s]);
            b->overlay[s] = nullptr;
        }
    if (b->tab) (void)hipMemset(b->tab, 0, sizeof(uint8_t*) * VS_MAX_VIS_SLOTS);
}
void vs_vis_base_drop(vs_index* ix) {
    VisBase* b = ix->vb;
    if (!b || ix->is_view) return;
    (void)hipSetDevice(ix->ctx->device);
    (void)hipStreamSynchronize(ix->ctx->stream);  // no launch may still read them
    vis_overlays_drop(b);
    if (b->cls) (void)hipFree(b->cls);
    if (b->dep) (void)hipFree(b->dep);
    vis_wk_free(b);
    b->cls = nullptr;
    b->dep = nullptr;
    b->dep_cap = 0;
    b->dep_host.clear();
    b->cls_rows = 0;
    b->n = b->r = b->horizon = 0;
}
void vs_vis_base_free(vs_index* ix) {
    if (!ix->vb || ix->is_view) return;
    vs_vis_base_drop(ix);
    if (ix->vb->tab) (void)hipFree(ix->vb->tab);
    delete ix->vb;
    ix->vb = nullptr;
}

// the refusals every call that writes the base or an overlay shares: a view handle, a batch in flight
static int vis_write_check(const char* what, vs_index* ix) {
    VS_REQUIRE(ix, "%s: index is NULL", what);
    if (ix->is_view) {
        vs_set_error("%s: this handle is a view; the base and its overlays belong to the index it was made from", what);
        return VS_ERR_STATE;
    }
    if (ix->ws.pending) {
        vs_set_error("%s: a batch of this handle is in flight (vs_search_batch_dev_finish first)", what);
        return VS_ERR_STATE;
    }
    return VS_OK;
}
static int vis_slot_check(const char* what, vs_index* ix, uint32_t slot) {
    VS_TRY(vis_write_check(what, ix));
    VS_REQUIRE(slot >= 1 && slot < VS_MAX_VIS_SLOTS, "%s: slot %u outside [1,%d]", what, slot, VS_MAX_VIS_SLOTS - 1);
    return VS_OK;
}
static int vis_need_base(const char* what, const vs_index* ix) {
    if (!ix->vb || !ix->vb->cls) {
        vs_set_error("%s: the index has no visibility base (vs_index_vis_base_eval)", what);
        return VS_ERR_STATE;
    }
    return VS_OK;
}
// one entry of the device table of overlay pointers
static int vis_tab_set(vs_index* ix, uint32_t slot, uint8_t* p) {
    VS_HIP(hipMemcpyAsync(ix->vb->tab + slot, &p, sizeof(p), hipMemcpyHostToDevice, ix->ctx->stream));
    VS_HIP(hipStreamSynchronize(ix->ctx->stream));
    return VS_OK;
}

static int vis_base_run(vs_index* ix, vs_heap_res* h, uint32_t horizon, const vs_xact_status* x, const uint32_t* changed, uint32_t n_changed,
                        vs_vis_base_stats* out) {
    vs_ctx* c = ix->ctx;
    hipStream_t st = c->stream;
    VS_HIP(hipSetDevice(c->device));
    VS_HIP(hipStreamSynchronize(st));  // (replacing classes a launch may still be reading)
    if (!ix->vb) ix->vb = new VisBase();
    VisBase* b = ix->vb;
    if (!b->tab) {
        VS_HIP(hipMalloc(&b->tab, sizeof(uint8_t*) * VS_MAX_VIS_SLOTS));
        VS_HIP(hipMemset(b->tab, 0, sizeof(uint8_t*) * VS_MAX_VIS_SLOTS));
    }
    vis_overlays_drop(b);  // overlays index positions of the list that is about to be rebuilt
    const uint32_t n = ix->d.n;
    const bool refresh = changed != nullptr;
    const size_t rows = std::max<size_t>(std::max(n, ix->capacity), 1);
    if (!refresh || b->cls_rows < rows) {  // (a refresh after the index grew past the array: the kept classes move, the new rows read 0)
        uint8_t* fresh = nullptr;
        VS_HIP(hipMalloc(&fresh, rows));
        VS_HIP(hipMemsetAsync(fresh, 0, rows, st));
        if (refresh && b->n) VS_HIP(hipMemcpyAsync(fresh, b->cls, std::min<size_t>(b->n, rows), hipMemcpyDeviceToDevice, st));
        VS_HIP(hipStreamSynchronize(st));
        if (b->cls) (void)hipFree(b->cls);
        b->cls = fresh;
        b->cls_rows = rows;
    }
    b->dep_host.clear();
    b->r = 0;
    const size_t clog_bytes = ((size_t)x->n_xids + 3) / 4;
    // The bitmap covers the resident fork and no more: a tid on a block at or beyond n_blocks is "not found" whether it is walked or
    // not (class 0, as it was), so a listed block out there changes nothing and costs no bit.  (ascending: the last is the highest)
    const uint32_t map_blocks = n_changed ? (uint32_t)std::min<uint64_t>((uint64_t)changed[n_changed - 1] + 1, h->n_blocks) : 0u;
    const size_t map_words = ((size_t)map_blocks + 31) / 32;
    std::vector<uint32_t> aux(map_words + (clog_bytes + 3) / 4 + 1, 0u);
    uint32_t n_listed = 0;  // changed blocks inside the fork
    for (uint32_t i = 0; i < n_changed && changed[i] < map_blocks; ++i, ++n_listed) aux[changed[i] >> 5] |= 1u << (changed[i] & 31u);
    if (clog_bytes) memcpy(aux.data() + map_words, x->bits, clog_bytes);
    uint32_t *d_aux = nullptr, *d_ctr = nullptr, *d_lctr = nullptr, *d_list = nullptr, *d_vals = nullptr;
    void* d_tmp = nullptr;
    uint32_t h_ctr[BC_N] = {0}, h_lctr[LC_N] = {0};
    const uint64_t resident = (uint64_t)std::max(c->prop.multiProcessorCount, 1) * 32;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(std::min<uint64_t>(((uint64_t)n + WAVE - 1) / WAVE, resident), 1);
    auto run = [&]() -> int {
        VS_TRY(vis_wk(b, VW_AUX, aux.size() * 4, (void**)&d_aux));
        VS_TRY(vis_wk(b, VW_CTR, (size_t)(BC_N + LC_N) * 4, (void**)&d_ctr));
        d_lctr = d_ctr + BC_N;
        if (n) VS_TRY(vis_wk(b, VW_LIST, (size_t)n * 4, (void**)&d_list));
        VS_TRY(vs_dev_upload(c, d_aux, aux.data(), aux.size() * 4));
        VS_HIP(hipMemsetAsync(d_ctr, 0, BC_N * 4, st));
        VS_HIP(hipMemsetAsync(d_lctr, 0, LC_N * 4, st));
        if (n && (!refresh || n_listed)) {
            HeapVisArgs a{};
            a.pages = h->d_pages;
            a.page_size = h->page_size;
            a.n_blocks = h->n_blocks;
            a.tids = ix->tids;
            a.n = n;
            a.xmin = a.xmax = a.horizon = horizon;  // S_H: empty xip / subxip / own xids, not suboverflowed, not in recovery
            a.xip = a.subxip = a.own = d_aux;       // (counts of 0: never read)
            a.clog_first = x->first_xid;
            a.clog_n = x->n_xids;
            a.clog = reinterpret_cast<const uint8_t*>(d_aux + map_words);
            a.visible = b->cls;
            a.ctr = d_ctr;
            a.block_map = refresh ? d_aux : nullptr;
            a.map_blocks = map_blocks;
            hipEvent_t ev = prof_begin(c);
            hipLaunchKernelGGL(k_heap_vis_base, dim3(grid), dim3(WAVE), 0, st, a);
            VS_HIP(hipGetLastError());
            prof_end(c, PK_PAGES, ev);
        }
        VS_HIP(hipMemcpyAsync(h_ctr, d_ctr, BC_N * 4, hipMemcpyDeviceToHost, st));
        VS_HIP(hipStreamSynchronize(st));
        if (h_ctr[HC_ERR] != HE_OK) {
            const uint32_t* e = h_ctr + HC_ERR;
            vs_set_error("heap block %u item %u: %s (detail %u)", e[1], e[2], kHeapErrorText[e[0] <= HE_LAST ? e[0] : 0], e[3]);
            return VS_ERR_INVALID;
        }
        if (n) {
            hipLaunchKernelGGL(k_vis_list, dim3(grid), dim3(WAVE), 0, st, (const uint8_t*)b->cls, n, d_list, d_lctr);
            VS_HIP(hipGetLastError());
        }
        VS_HIP(hipMemcpyAsync(h_lctr, d_lctr, LC_N * 4, hipMemcpyDeviceToHost, st));
        VS_HIP(hipStreamSynchronize(st));
        const uint32_t r = std::min(h_lctr[LC_NLIST], n);
        if (!b->dep || b->dep_cap < std::max(r, 1u)) {
            if (b->dep) (void)hipFree(b->dep);
            b->dep = nullptr;
            b->dep_cap = 0;
            const size_t cap = (size_t)std::max(r, 1u) + r / 8;
            VS_HIP(hipMalloc(&b->dep, cap * 4));
            b->dep_cap = cap;
        }
        b->dep_host.assign(r, 0u);
        if (r) {  // ascending, whatever order the waves appended in
            VS_TRY(vis_wk(b, VW_VALS, (size_t)r * 4, (void**)&d_vals));
            size_t tmp_bytes = 0;
            VS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (const uint32_t*)d_list, b->dep, (const uint32_t*)d_list, d_vals, (int)r, 0, 32, st));
            VS_TRY(vis_wk(b, VW_TMP, tmp_bytes + 16, &d_tmp));
            VS_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp_bytes, (const uint32_t*)d_list, b->dep, (const uint32_t*)d_list, d_vals, (int)r, 0, 32, st));
            VS_HIP(hipStreamSynchronize(st));
            VS_TRY(vs_dev_download(c, b->dep_host.data(), b->dep, (size_t)r * 4));
        }
        b->r = r;
        return VS_OK;
    };
    const int rc = run();
    if (rc != VS_OK) (void)hipStreamSynchronize(st);
    if (rc != VS_OK) {
        vs_vis_base_drop(ix);  // (classes half written are no base)
        return rc;
    }
    b->n = n;
    b->horizon = horizon;
    if (out) {
        uint64_t sums[BSUM_N];
        memcpy(sums, h_ctr + VC_SUMS, sizeof(sums));
        vs_vis_base_stats S{};
        S.n_class[0] = h_lctr[LC_CLASS + 0];
        S.n_class[1] = h_lctr[LC_CLASS + 1];
        S.n_class[2] = b->r;
        S.r = b->r;
        S.n_walked = sums[BSUM_WALKED];
        S.n_deleted = sums[BSUM_DELETED];
        S.n_not_found = sums[BSUM_NOT_FOUND];
        S.n_dead_line_pointer = sums[BSUM_DEAD_LP];
        S.n_recent = sums[BSUM_RECENT];
        S.n_undecided = sums[BSUM_UNDECIDED];
        S.chain_hops = sums[BSUM_HOPS];
        for (int k = 0; k < VS_VIS_R_N; ++k) S.undecided_by_reason[k] = sums[BSUM_REASON + k];
        *out = S;
    }
    return VS_OK;
}

extern "C" int vs_index_vis_base_eval(vs_index* ix, vs_heap_res* h, uint32_t horizon_xid, const vs_xact_status* xact, const uint32_t* changed_blocks,
                                      uint32_t n_changed, vs_vis_base_stats* out) {
    const char* what = "vs_index_vis_base_eval";
    VS_TRY(vis_write_check(what, ix));
    VS_REQUIRE(h, "%s: the resident heap fork is NULL", what);
    VS_REQUIRE(h->ctx == ix->ctx, "%s: the index and the resident heap fork belong to different contexts", what);
    VS_REQUIRE(xact, "%s: the transaction status window is required", what);
    VS_REQUIRE(!(xact->first_xid & 3u), "%s: first_xid %u is not a multiple of 4", what, xact->first_xid);
    VS_REQUIRE(xact->bits || !xact->n_xids, "%s: the transaction status bits are NULL with n_xids above 0", what);
    VS_REQUIRE(horizon_xid >= 3u, "%s: the horizon %u is no normal xid", what, horizon_xid);
    VS_REQUIRE(changed_blocks || !n_changed, "%s: changed_blocks is NULL with n_changed above 0", what);
    for (uint32_t i = 1; i < n_changed; ++i)
        VS_REQUIRE(changed_blocks[i - 1] < changed_blocks[i], "%s: changed_blocks must be ascending and distinct (entry %u)", what, i);
    VS_REQUIRE(!n_changed || changed_blocks[n_changed - 1] != 0xFFFFFFFFu, "%s: block 0xFFFFFFFF is no block of a relation", what);
    VS_REQUIRE(ix->tids || !ix->d.n, "%s: the index has no heap tid column", what);
    VS_REQUIRE(ix->d.n <= 0x7FFFFFFFu, "%s: %u nodes", what, ix->d.n);
    if (changed_blocks) VS_TRY(vis_need_base(what, ix));
    return vs_guard(what, [&] { return vis_base_run(ix, h, horizon_xid, xact, changed_blocks, n_changed, out); });
}

extern "C" int vs_index_vis_base_drop(vs_index* ix) {
    VS_TRY(vis_write_check("vs_index_vis_base_drop", ix));
    vs_vis_base_drop(ix);
    return VS_OK;
}

extern "C" int vs_index_vis_base_info(const vs_index* ix, uint32_t* horizon_xid, uint32_t* r, uint32_t* depends_nodes, uint32_t cap) {
    VS_REQUIRE(ix && (depends_nodes || !cap), "vs_index_vis_base_info: null argument");
    VS_TRY(vis_need_base("vs_index_vis_base_info", ix));
    const VisBase* b = ix->vb;
    if (horizon_xid) *horizon_xid = b->horizon;
    if (r) *r = b->r;
    if (cap) memcpy(depends_nodes, b->dep_host.data(), (size_t)std::min(cap, b->r) * 4);
    return VS_OK;
}

extern "C" int vs_index_vis_slot_drop(vs_index* ix, uint32_t slot) {
    VS_TRY(vis_slot_check("vs_index_vis_slot_drop", ix, slot));
    VisBase* b = ix->vb;
    if (!b || !b->overlay[slot]) return VS_OK;
    return vs_guard("vs_index_vis_slot_drop", [&]() -> int {
        VS_HIP(hipSetDevice(ix->ctx->device));
        VS_HIP(hipStreamSynchronize(ix->ctx->stream));  // no launch may still read it
        VS_TRY(vis_tab_set(ix, slot, nullptr));
        (void)hipFree(b->overlay[slot]);
        b->overlay[slot] = nullptr;
        return VS_OK;
    });
}

extern "C" int vs_index_vis_slot_eval(vs_index* ix, vs_heap_res* h, uint32_t slot, const vs_mvcc_snapshot* snap, const vs_xact_status* xact,
                                      vs_vis_stats* out, uint32_t* undecided_nodes, uint32_t cap, uint32_t* n_undecided) {
    const char* what = "vs_index_vis_slot_eval";
    VS_TRY(vis_slot_check(what, ix, slot));
    VS_REQUIRE(h, "%s: the resident heap fork is NULL", what);
    VS_REQUIRE(h->ctx == ix->ctx, "%s: the index and the resident heap fork belong to different contexts", what);
    VS_TRY(heap_vis_check(what, snap, xact, undecided_nodes, cap));
    VS_TRY(vis_need_base(what, ix));
    VisBase* b = ix->vb;
    // the base holds for snapshots that cannot see behind its horizon: xmin and every own xid at or after it
    VS_REQUIRE(!vis_precedes_host(snap->xmin, b->horizon), "%s: the snapshot's xmin %u precedes the base's horizon %u", what, snap->xmin, b->horizon);
    for (uint32_t i = 0; i < snap->n_own; ++i)
        VS_REQUIRE(!vis_precedes_host(snap->own_xids[i], b->horizon), "%s: the own xid %u precedes the base's horizon %u", what, snap->own_xids[i], b->horizon);
    return vs_guard(what, [&]() -> int {
        vs_ctx* c = ix->ctx;
        VS_HIP(hipSetDevice(c->device));
        VS_HIP(hipStreamSynchronize(c->stream));  // (replacing an overlay a launch may still be reading)
        const uint32_t r = b->r;
        uint64_t* d_tids = nullptr;
        std::vector<uint32_t> und(std::min(cap, r));
        uint32_t nu = 0;
        auto run = [&]() -> int {
            if (!b->overlay[slot]) {
                uint8_t* p = nullptr;
                VS_HIP(hipMalloc(&p, std::max(r, 1u)));
                b->overlay[slot] = p;
                VS_TRY(vis_tab_set(ix, slot, p));
            }
            VS_HIP(hipMalloc(&d_tids, (size_t)std::max(r, 1u) * 8));
            if (r) {
                hipLaunchKernelGGL(k_vis_gather_tids, dim3(heap_dev_grid(r, 256)), dim3(256), 0, c->stream, (const uint64_t*)ix->tids, (const uint32_t*)b->dep, r, d_tids);
                VS_HIP(hipGetLastError());
            }
            // the list positions of the undecided come back ascending; so are their nodes, the list being ascending
            return heap_vis_run(h, d_tids, r, snap, xact, b->overlay[slot], out, und.data(), (uint32_t)und.size(), &nu);
        };
        const int rc = run();
        if (rc != VS_OK) (void)hipStreamSynchronize(c->stream);
        if (d_tids) (void)hipFree(d_tids);
        if (rc != VS_OK) {  // (an overlay half written is no overlay)
            if (b->overlay[slot]) {
                (void)vis_tab_set(ix, slot, nullptr);
                (void)hipFree(b->overlay[slot]);
                b->overlay[slot] = nullptr;
            }
            return rc;
        }
        for (size_t i = 0; i < und.size() && i < nu; ++i) undecided_nodes[i] = b->dep_host[und[i]];
        if (n_undecided) *n_undecided = nu;
        return VS_OK;
    });
}

extern "C" int vs_index_vis_slot_patch(vs_index* ix, uint32_t slot, const uint32_t* nodes, const uint8_t* values, uint32_t n) {
    const char* what = "vs_index_vis_slot_patch";
    VS_TRY(vis_slot_check(what, ix, slot));
    VS_REQUIRE((nodes && values) || !n, "%s: null argument", what);
    VS_TRY(vis_need_base(what, ix));
    VisBase* b = ix->vb;
    if (!b->overlay[slot]) {
        vs_set_error("%s: slot %u has no overlay (vs_index_vis_slot_eval)", what, slot);
        return VS_ERR_STATE;
    }
    return vs_guard(what, [&]() -> int {
        // node -> its position in the depends list; one entry per position, the last one given
        std::vector<std::pair<uint32_t, uint32_t>> order(n);
        for (uint32_t i = 0; i < n; ++i) {
            const auto it = std::lower_bound(b->dep_host.begin(), b->dep_host.end(), nodes[i]);
            VS_REQUIRE(it != b->dep_host.end() && *it == nodes[i], "%s: node %u is not on the depends list", what, nodes[i]);
            order[i] = {(uint32_t)(it - b->dep_host.begin()), i};
        }
        if (!n) return VS_OK;
        std::sort(order.begin(), order.end());
        std::vector<uint32_t> up;
        std::vector<uint8_t> uv;
        for (uint32_t i = 0; i < n; ++i)
            if (i + 1 == n || order[i + 1].first != order[i].first) {
                up.push_back(order[i].first);
                uv.push_back(values[order[i].second]);
            }
        vs_ctx* c = ix->ctx;
        VS_HIP(hipSetDevice(c->device));
        uint32_t* d_pos = nullptr;
        uint8_t* d_vals = nullptr;
        auto run = [&]() -> int {
            VS_HIP(hipMalloc(&d_pos, up.size() * 4));
            VS_HIP(hipMalloc(&d_vals, uv.size()));
            VS_TRY(vs_dev_upload(c, d_pos, up.data(), up.size() * 4));
            VS_TRY(vs_dev_upload(c, d_vals, uv.data(), uv.size()));
            hipLaunchKernelGGL(k_mask_patch, dim3(heap_dev_grid(up.size(), 256)), dim3(256), 0, c->stream, b->overlay[slot], (const uint32_t*)d_pos,
                               (const uint8_t*)d_vals, (uint32_t)up.size());
            VS_HIP(hipGetLastError());
            VS_HIP(hipStreamSynchronize(c->stream));
            return VS_OK;
        };
        const int rc = run();
        if (rc != VS_OK) (void)hipStreamSynchronize(c->stream);
        if (d_pos) (void)hipFree(d_pos);
        if (d_vals) (void)hipFree(d_vals);
        return rc;
    });
}

extern "C" int vs_index_vis_materialize(vs_index* ix, uint32_t slot, uint32_t snapshot) {
    const char* what = "vs_index_vis_materialize";
    VS_TRY(vis_slot_check(what, ix, slot));
    VS_TRY(snapshot_write_check(what, ix, snapshot));
    VS_TRY(vis_need_base(what, ix));
    VisBase* b = ix->vb;
    if (!b->overlay[slot]) {
        vs_set_error("%s: slot %u has no overlay (vs_index_vis_slot_eval)", what, slot);
        return VS_ERR_STATE;
    }
    return vs_guard(what, [&]() -> int {
        vs_ctx* c = ix->ctx;
        VS_HIP(hipSetDevice(c->device));
        bool fresh = false;
        VS_TRY(snapshot_mask(ix, snapshot, &fresh));
        const uint32_t n = ix->d.n;  // (rows past the evaluated ones read class 0: hidden, as in every stored mask)
        if (n) {
            hipLaunchKernelGGL(k_vis_materialize, dim3(heap_dev_grid(n, 256)), dim3(256), 0, c->stream, (const uint8_t*)b->cls, (const uint32_t*)b->dep, b->r,
                               (const uint8_t*)b->overlay[slot], ix->snap[snapshot], n);
            VS_HIP(hipGetLastError());
        }
        VS_HIP(hipStreamSynchronize(c->stream));
        return VS_OK;
    });
}

// a view takes the base and the overlays of its source over, as vs_index_snapshot_share hands over the masks
extern "C" int vs_index_vis_share(vs_index* view, const vs_index* src) {
    VS_REQUIRE(view && src && view->is_view, "vs_index_vis_share: needs a view and its source");
    view->vb = src->vb;
    return VS_OK;
}
