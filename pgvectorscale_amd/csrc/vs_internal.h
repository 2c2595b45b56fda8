// vs_internal.h — shared declarations of libvsgpu.so (HIP / gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <atomic>
#include <mutex>
#include <vector>

#include "../../include/vsgpu.h"
#include "vs_q16.h"

#define VS_EMPTY 0xFFFFFFFFu

void vs_set_error(const char* fmt, ...);
// vs_options.cpp: the option table (vs_set_option, else a snapshot of the VS_* environment refreshed only when it changes); nullptr = unset
const char* vs_opt_get(const char* name);

#define VS_HIP(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            vs_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);   \
            return (_e == hipErrorOutOfMemory) ? VS_ERR_OOM : VS_ERR_HIP;                              \
        }                                                                                              \
    } while (0)

#define VS_REQUIRE(cond, ...)         \
    do {                              \
        if (!(cond)) {                \
            vs_set_error(__VA_ARGS__);\
            return VS_ERR_INVALID;    \
        }                             \
    } while (0)

#define VS_REQUIRE_OOM(cond, ...)     \
    do {                              \
        if (!(cond)) {                \
            vs_set_error(__VA_ARGS__);\
            return VS_ERR_OOM;        \
        }                             \
    } while (0)

#define VS_TRY(expr)            \
    do {                        \
        int _r = (expr);        \
        if (_r != VS_OK) return _r; \
    } while (0)

// extern "C" entry points never let a C++ exception cross the boundary (vsgpu.h: errors are return codes)
#include <exception>
#include <new>
template <class F>
static inline int vs_guard(const char* what, F&& f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        vs_set_error("%s: out of host memory", what);
        return VS_ERR_OOM;
    } catch (const std::exception& e) {
        vs_set_error("%s: %s", what, e.what());
        return VS_ERR_INVALID;
    }
}

// ---- the device scratch and HIP events of one call ----------------------------------------------------------------------
// What a call allocates for its own duration is registered here and goes with the scope, on every way out: a return code, or an
// exception on its way to vs_guard.  The destructor first waits for the stream once (kernels in flight may still use the buffers),
// unless the call has told it that its last step was such a wait (drained()).
struct DevScope {
    hipStream_t st;
    explicit DevScope(hipStream_t stream) : st(stream) {}
    DevScope(const DevScope&) = delete;
    DevScope& operator=(const DevScope&) = delete;
    ~DevScope() { close(); }
    // what the destructor does, for a call that goes on after its device work (a later alloc() or event() opens the scope again)
    void close() {
        if (!is_drained) (void)hipStreamSynchronize(st);
        for (void* p : bufs) (void)hipFree(p);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        bufs.clear();
        events.clear();
        is_drained = true;
    }
    template <class T>
    int alloc(T** p, size_t bytes, const char* what) {
        bufs.push_back(nullptr);  // (the slot before the allocation: nothing between it and its registration can throw)
        is_drained = false;
        const hipError_t e = hipMalloc(&bufs.back(), bytes);
        if (e != hipSuccess) {
            bufs.pop_back();
            vs_set_error("%s: hipMalloc of %zu bytes failed: %s", what, bytes, hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? VS_ERR_OOM : VS_ERR_HIP;
        }
        *p = static_cast<T*>(bufs.back());
        return VS_OK;
    }
    // a buffer leaves the scope: release() hands it to the caller (scratch that becomes the index's own), free() returns it to the
    // device now (the sites that grow a buffer); both leave p null
    template <class T>
    T* release(T*& p) {
        T* const out = p;
        for (size_t i = 0; i < bufs.size(); ++i)
            if (bufs[i] == static_cast<void*>(out)) {
                bufs.erase(bufs.begin() + (long)i);
                break;
            }
        p = nullptr;
        return out;
    }
    template <class T>
    void free(T*& p) {
        if (p) (void)hipFree(release(p));
    }
    int event(hipEvent_t* ev, const char* what) {
        events.push_back(nullptr);
        is_drained = false;
        const hipError_t e = hipEventCreate(&events.back());
        if (e != hipSuccess) {
            events.pop_back();
            *ev = nullptr;
            vs_set_error("%s: hipEventCreate failed: %s", what, hipGetErrorString(e));
            return VS_ERR_HIP;
        }
        *ev = events.back();
        return VS_OK;
    }
    void drained() { is_drained = true; }

private:
    std::vector<void*> bufs;
    std::vector<hipEvent_t> events;
    bool is_drained = false;
};

// HIP-event time of a call's stages (vs_profile_enable): tock(which) adds the milliseconds since the last tick() to ms[which] of the
// caller's array.  Inert — no event, no wait — unless the context is profiling when start() is called.
struct StageTimer {
    hipStream_t st = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double* ms = nullptr;
    int start(DevScope& sc, bool profiling, double* ms_, const char* what) {
        st = sc.st;
        ms = ms_;
        if (!profiling) return VS_OK;
        hipEvent_t a = nullptr;
        VS_TRY(sc.event(&a, what));
        VS_TRY(sc.event(&ev[1], what));
        ev[0] = a;
        return VS_OK;
    }
    void tick() {
        if (ev[0]) (void)hipEventRecord(ev[0], st);
    }
    void tock(int which) {
        float t = 0.f;
        if (ev[0] && hipEventRecord(ev[1], st) == hipSuccess && hipEventSynchronize(ev[1]) == hipSuccess &&
            hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess)
            ms[which] += t;
    }
};

__host__ __device__ static inline uint32_t round_up_u32(uint32_t x, uint32_t m) { return (x + m - 1) / m * m; }
static inline uint32_t next_pow2_u32(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return (uint32_t)p;
}

struct vs_ctx {
    int device = -1;
    hipStream_t stream = nullptr;       // compute
    hipStream_t copy_stream = nullptr;  // H2D/D2H staging
    void* pinned[2] = {nullptr, nullptr};
    size_t pinned_bytes = 0;
    hipEvent_t pinned_ev[2] = {nullptr, nullptr};
    hipDeviceProp_t prop;
    // optional per-kernel event timing (vs_profile_*)
    bool profiling = false;
    struct ProfSpan { int kind; hipEvent_t a, b; };
    std::vector<ProfSpan> spans;
    std::vector<hipEvent_t> event_pool;
    double prof_ms[8] = {0};
    uint64_t prof_launches[8] = {0};
};
enum { PK_PREPARE = 0, PK_SEARCH = 1, PK_RERANK = 2, PK_RESORT = 3, PK_SEARCH_FB = 4, PK_SCAN = 5, PK_ORDER = 6, PK_PAGES = 7 };
hipEvent_t prof_begin(vs_ctx* c);
void prof_end(vs_ctx* c, int kind, hipEvent_t a);

// growable device scratch buffer
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool in_slab = false;  // a chunk of the index's WsSlab (never freed on its own)
};

// The hot, randomly accessed per-workgroup regions of the search workspace (dedup tables, heap spill arrays of the persistent grid:
// 0.7 GB at 50M) run fastest packed at the start of ONE large device allocation: allocation history moved k_search_fast by +-10 % at
// identical bytes while the regions lived in allocations of their own size (profiles/r04/s7_diag_state_50m.txt,
// s11_diag_spread_50m.txt).  One grow-only slab per index, allocated by the first search that needs it and shared with every view
// of the index (cursor lanes, second streams, the own-device shard of a vs_multi); chunks are bump-allocated, never returned one
// by one, and the slab goes when the last handle that holds it does.
struct WsSlab {
    std::mutex mu;
    // two regions: [0] the dedup tables, [1] the heap spill arrays — halves of one allocation, or two allocations when the probe found a
    // pair of places that beats every single one
    void* base[2] = {nullptr, nullptr};
    size_t bytes[2] = {0, 0}, used[2] = {0, 0};
    void* owned[2] = {nullptr, nullptr};  // what is hipFree'd with the slab (nothing for the caller's memory)
    int refs = 1;
    int device = 0;
    bool tried = false;  // the allocation failed once: handles fall back to allocations of their own
    bool external = false;  // the caller's memory (vs_index_set_slab): used whatever VS_WS_SLAB_MB / the size rule say
};

// ---- a batch of scans (vs_batch.hip) ----------------------------------------------------------------------------
// capacities of a batch's launches
struct Caps {
    uint32_t hl, hcap, vcap, lh, hashcap, g0;  // general kernel (vs_search.hip)
    // fast kernel (vs_search_fast.hip); f_lh == 0: no LDS dedup table (every id in the global table)
    bool f_on;
    uint32_t f_hl, f_hcap, f_gstride, f_lh, f_gcap, f_sb, f_vr, f_vcap;
    double f_pool_frac;  // share of the scans expected to need a global dedup-overflow table
};
// The qualifier side of a launch (vs_search_batch_qual, vs_qual.h).  pops == 0: an unqualified launch.  Otherwise the window pops up to
// `pops` rows per scan — the stream is M = stream_len(rescore, pops) rows long — and keeps the rows whose node passes the scan's
// qualifier, up to k.  Scan w of the launch is scan map[w] (or q_base + w) of the BATCH: slots, the output rows and out_* are indexed by
// the batch's scan numbers.  All pointers DEVICE.
enum { VS_QUAL_MORE = 3 };  // out_state between rounds: `pops` rows popped, fewer than k kept, the scan not ended, pops < max_pops: run it again
struct QualLaunch {
    uint32_t pops = 0;
    uint32_t q_base = 0;
    const uint32_t* map = nullptr;
    const uint32_t* slots = nullptr;
    const uint64_t* const* tab = nullptr;  // [VS_MAX_QUAL_SLOTS + 1] bitmaps, entry 0 null (QualSet::tab); null: every node passes
    uint32_t final = 0;                    // the batch's last round: a scan neither complete nor ended after `pops` rows is CUT
    uint32_t* out_rows = nullptr;
    uint32_t* out_pops = nullptr;
    uint32_t* out_state = nullptr;
};
// one launch (a chunk of the batch): nq scans of search list L that each leave a stream of M rows
enum { BV_INDEX_MASK = 0, BV_NONE = 1, BV_SLOTS = 2 };
struct BatchPlan {
    uint32_t nq, L, rescore, k, M;
    bool stream_only;  // vs_stream_batch: no rerank
    // heap visibility of the chunk's scans: BV_INDEX_MASK the mask in force on the index (vs_index_set_visibility*, vs_index_snapshot_use),
    // BV_NONE the caller named slots and every one is 0, BV_SLOTS d_slots (DEVICE [nq]) names each scan's slot (vs_search_batch_vis)
    uint32_t vis_mode = 0;
    const uint32_t* d_slots = nullptr;
    QualLaunch qual;  // (pops > 0: the window keeps the rows that pass a qualifier; the d_out_* of the launch are the batch's)
};

// ---- what a launch knows about heap visibility (vs_heap_vis.h) ----------------------------------------------------
// Legacy mode (slots == nullptr): bytes is one mask for the whole launch, a node with bytes[node] == 0 is hidden; bytes == nullptr:
// every tuple visible.  Classed mode (slots != nullptr): bytes is the class byte of the base (VIS_CLASS_*), dep the ascending depends
// list of r nodes, overlay[slot] the r bytes of a slot's overlay and slots[q] the slot scan q runs under (0: every tuple visible).
enum { VIS_CLASS_NONE = 0, VIS_CLASS_ALL = 1, VIS_CLASS_DEPENDS = 2 };
struct VisView {
    const uint8_t* bytes = nullptr;
    const uint32_t* slots = nullptr;
    const uint32_t* dep = nullptr;
    const uint8_t* const* overlay = nullptr;
    uint32_t r = 0;
};
// the base of an index (vs_index_vis_base_eval) and the overlays of its slots; shared by the views that took it over
struct VisBase {
    uint8_t* cls = nullptr;     // DEVICE, one class byte per node, allocated at capacity: rows past the evaluated ones read 0
    size_t cls_rows = 0;        // rows cls has room for
    uint32_t n = 0;             // nodes the last evaluation saw
    uint32_t* dep = nullptr;    // DEVICE [r] ascending
    std::vector<uint32_t> dep_host;
    uint32_t r = 0, horizon = 0;
    uint8_t* overlay[VS_MAX_VIS_SLOTS] = {nullptr};  // DEVICE [r] each (host mirror of tab)
    uint8_t** tab = nullptr;    // DEVICE [VS_MAX_VIS_SLOTS]
    size_t dep_cap = 0;         // entries dep has room for
    // DEVICE scratch of an evaluation, kept between the rounds of a shim and grown on demand (VW_*; freed with the base)
    void* wk[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t wk_bytes[5] = {0, 0, 0, 0, 0};
};
// plan + capacities + the caller's device pointers of the batch in flight between vs_search_batch_dev and its finish
struct PendingBatch {
    BatchPlan bp;
    Caps caps;
    const int16_t* d_qlabels;
    const uint32_t* d_qlabel_off;
    uint32_t* d_out_ids;
    uint64_t* d_out_tids;
    float* d_out_dist;
};

// ---- qualifiers of an index and the qualified batch in flight (vs_qual.h) -------------------------------------------
// bits[slot]: DEVICE, `words` u64 each (room for the index's capacity), null = empty slot; bits at positions >= the index's n are 0.
// tab: DEVICE [VS_MAX_QUAL_SLOTS + 1] mirror of bits for the kernels (entry 0 stays null: every node passes)
struct QualSet {
    uint64_t* bits[VS_MAX_QUAL_SLOTS + 1] = {nullptr};
    vs_qual_info info[VS_MAX_QUAL_SLOTS + 1] = {};
    size_t words = 0;
    uint64_t** tab = nullptr;
};
// what vs_search_batch_dev_qual leaves for its finish: the caller's device pointers and the plan of the rounds
struct PendingQual {
    const float* d_queries = nullptr;
    const int16_t* d_qlabels = nullptr;
    const uint32_t* d_qlabel_off = nullptr;
    const uint32_t* d_slots = nullptr;
    uint32_t nq = 0, L = 0, rescore = 0, k = 0, max_pops = 0, first_pops = 0;
    bool all_zero = false;   // every scan names slot 0
    bool launched = false;   // round 1 is in flight as one launch of the batch pipeline
    uint32_t *d_out_ids = nullptr, *d_out_rows = nullptr, *d_out_pops = nullptr, *d_out_state = nullptr;
    uint64_t* d_out_tids = nullptr;
    float* d_out_dist = nullptr;
};

struct SearchWorkspace {
    DevBuf q_full, qcodes, qlabels, qlabel_off, hash, heap_g, heap_g4, ghash4, heap_g4b, ghash4b, pool_ctr, fb_flag, phase, timeline, stream_ids, stream_ham, stream_cnt, stats, status,
        rr_dist, out_ids, out_tids, out_dist, resort_heap, raw_q, misc, q_index,
        raw_q2, out_ids2, out_tids2, out_dist2,  // second set of a pipelined host batch (search_host)
        red,                                      // RED_N u64 sums of the last launch's per-scan arrays (k_reduce_stats)
        order_work, order_perm,                   // VS_RERANK_ORDER: keys + counting-sort tables, and the batch's rerank order
        order_labels,                             // ... and the region label (u16: nearest seed row) of corpus rows [0, lab_rows)
        vis_slots,                                // the visibility slots of a host batch's scans (vs_search_batch_vis)
        qual_q, qual_map, qual_lab, qual_laboff,  // vs_search_batch_qual: the gathered queries, scan numbers and label keys of a later round
        qual_slots, qual_out;                     // ... the slots of a host batch, and its rows, counts and states before they go back
    uint32_t order_nq = 0;         // scans of the last batch's rerank order in order_perm (0: it took the scans' own order)
    // what order_labels was built from: the seed rows s * lab_step for s < lab_S of the codes at epoch lab_epoch (vs_index::codes_epoch)
    uint32_t lab_rows = 0, lab_S = 0, lab_step = 0;
    uint64_t lab_epoch = 0;
    uint64_t* red_host = nullptr;  // pinned; the sums land here (this handle's own: two handles of one context may each have a batch in flight)
    bool fb_valid = false;  // fb_flag holds the fallback marks of the last chunk
    // pending async call (vs_search_batch_dev)
    bool pending = false;
    PendingBatch pend{};
    bool qual_pending = false;  // ... of vs_search_batch_dev_qual (pending stays true with it: the same entry points refuse)
    PendingQual qpend{};
};

// what the last batches needed (per search_list_size / stream length): sizes the LDS dedup table of the next launch
struct ScanObs {
    bool valid = false;
    uint32_t L = 0, M = 0;
    double ins_mean = 0, ins_max = 0;  // inserted ids per scan
    double ov_frac = 1.0;              // fraction of scans that outgrew the LDS table
};

// the launch variant of k_search_fast an index prefers (vs_index_autotune / vs_index_set_variant): -1 = the library default;
// a VS_F_* environment variable still overrides the field it names
struct TuneVariant {
    int virgin = -1, minw = -1, persist = -1;
    int lds_max_ins = -1;  // 0: the table-less regime even for scans whose dedup table would fit LDS
    int vr = -1;           // 0: the LDS-ring visited list also where the register-resident one is the default (LDS-table regime)
    uint32_t gcap = 0;
    char name[40] = "default";
};
// what the last first-attempt launch of k_search_fast really was (a variant that does not exist for an index / operating point
// silently launches the default's instantiation: the autotuner reads this to tell)
struct FastSig {
    uint32_t vwords = 0, minw = 0, gcap = 0, lh = 0, vr = 0, ran = 0;
    bool operator==(const FastSig& o) const {
        return vwords == o.vwords && minw == o.minw && gcap == o.gcap && lh == o.lh && vr == o.vr && ran == o.ran;
    }
};

struct vs_index {
    vs_ctx* ctx = nullptr;
    bool is_view = false;  // vs_index_view: the device arrays belong to another handle
    bool uploaded = false; // vs_index_upload staged it from host arrays (a relation's pages), vs_index_alloc did not
    vs_index* view_of = nullptr;  // ... that one (never dereferenced: the owner may be gone)
    uint64_t owner_id = 0;        // key of the owner in the registry of live views (unique per vs_index_alloc / replica, never reused)
    WsSlab* slab = nullptr;       // shared by an index and its views (reference counted)
    vs_index_desc d{};
    uint32_t capacity = 0;     // rows the per-node arrays have room for (>= d.n; vs_index_reserve / vs_index_insert grow it)
    uint32_t code_stride = 0;  // u64 words per code row (W rounded up to even, zero padded)
    uint32_t nbr_stride = 0;   // u32 per neighbor row (R rounded up to 16)
    uint32_t vec_stride = 0;   // floats per vector row (dim_full rounded up to 4)
    uint64_t* codes = nullptr;
    // moves whenever the codes of existing rows or the row numbers may have changed (training / quantising, a write hand-out of the
    // array, page loads, broadcasts, compaction; not an insert, which only appends rows): what was derived from the codes and is kept
    // between batches (SearchWorkspace::order_labels) is rebuilt when it finds its epoch gone
    uint64_t codes_epoch = 0;
    uint32_t* nbrs = nullptr;
    uint64_t* tids = nullptr;
    double insert_ms[3] = {0, 0, 0};   // HIP-event time of k_batch_mates / k_insert_merge_mates / k_insert_anchor (vs_profile_enable; vs_index_insert_kernel_ms)
    double build_ms[3] = {0, 0, 0};    // HIP-event time of the batch machinery's searches / prune of new nodes / back-edges, vs_build_graph and vs_index_insert alike (vs_index_build_kernel_ms)
    double consolidate_ms[2] = {0, 0}; // HIP-event time of the flag pass / k_consolidate_rows (vs_profile_enable; vs_index_consolidate_kernel_ms)
    double compact_ms[2] = {0, 0};     // HIP-event time of the keep flags + maps / the row mover (vs_profile_enable; vs_index_compact_kernel_ms)
    double label_repair_ms[4] = {0, 0, 0, 0};  // HIP-event time of the reach sweeps / strong[] / k_nearest_masked / claim + apply (vs_index_label_repair_kernel_ms)
    uint32_t build_unreachable = 0;    // nodes the last vs_build_graph left unreachable from the start node (0xFFFFFFFF: not judged)
    const uint8_t* visible = nullptr;  // per node, 0 = the heap fetch finds nothing under the scan's snapshot (nullptr: all visible)
    uint8_t* visible_own = nullptr;    // the library's own copy (vs_index_set_visibility)
    uint8_t* snap[VS_MAX_SNAPSHOTS] = {nullptr};  // per-snapshot masks of shared launches (vs_index_snapshot_put); slot 0 unused
    QualSet* qs = nullptr;     // the qualifiers of an owner (vs_index_qual_*); a view holds none
    VisBase* vb = nullptr;     // the visibility base and its overlays (vs_index_vis_base_eval); a view's is its source's (vs_index_vis_share)
    float* vecs = nullptr;
    float* vnorm = nullptr;  // per node: 0 => leave vector alone, else divisor sqrt(norm) (preprocess_cosine)
    float* vnorm_idx = nullptr;  // the same for the index slice (plain storage, cosine, num_dimensions_to_index < num_dimensions)
    float* mean = nullptr;
    float* m2 = nullptr;
    uint64_t count = 0;
    uint32_t* label_off = nullptr;
    int16_t* label_val = nullptr;
    uint64_t* label_mask = nullptr;  // per node: bit label_bit[l] set <=> label l in its set; only when the index uses <= 64 distinct labels
    uint8_t* label_bit = nullptr;    // [65536] label (as u16) -> its bit, 0xFF = the label occurs nowhere in the index
    // [n][nbr_stride] label masks of every node's neighbors in list order (a cache derived from nbrs + label_mask for the
    // label-filtered scans; rebuilt lazily by vs_refresh_neighbor_masks when nbr_mask_valid is false)
    uint64_t* nbr_mask = nullptr;
    bool nbr_mask_valid = false;
    bool nbr_mask_tried = false;     // the array did not fit the device: the scans load the masks per neighbor
    uint64_t n_label_vals = 0;
    int16_t* ls_labels = nullptr;
    uint32_t* ls_nodes = nullptr;
    SearchWorkspace ws;
    ScanObs obs;
    uint32_t last_ins_limit = 0;  // LDS-table admission limit of the last fast launch
    TuneVariant tune;
    FastSig last_fast;
    vs_search_info last_info{};  // what the first attempt of the last chunk ran (vs_index_last_search_info)
    bool last_info_valid = false;
    vs_stats last_stats{};
};

// "done once per device" for function-scope statics (hipFuncSetAttribute is per device; one thread per device may launch the same
// instantiation at once through vs_multi_*): pending() is true where the calling device's bit is not set yet, done() records it.
// Setting an attribute twice is harmless, so two threads of one device racing through the unset state are fine.
struct DeviceOnce {
    std::atomic<uint64_t> mask{0};
    bool pending(int device) const { return device < 0 || device >= 64 || !((mask.load(std::memory_order_acquire) >> device) & 1ull); }
    void done(int device) {
        if (device >= 0 && device < 64) mask.fetch_or(1ull << device, std::memory_order_acq_rel);
    }
};
int devbuf_reserve(vs_ctx* ctx, DevBuf& b, size_t bytes);
int devbuf_reserve_hot(vs_index* ix, DevBuf& b, size_t bytes, int which);  // from region `which` of the index's slab when it has one (else as devbuf_reserve)
uint64_t vs_new_owner_id();
WsSlab* vs_slab_new(int device);
void vs_slab_release(WsSlab* s);
int vs_index_live_views(vs_index* ix);  // views made of ix that have not been freed yet
int vs_index_open_writers(const vs_index* ix);  // vs_pages_out writers opened on ix (or a view of it) that have not been closed yet
void vs_index_writer_opened(uint64_t owner_id);
void vs_index_writer_closed(uint64_t owner_id);
// the entry points that free or move the arrays of an index refuse view handles and owners with live views
#define VS_REQUIRE_OWNER(ix, what)                                                                                                     \
    do {                                                                                                                                \
        if ((ix)->is_view) {                                                                                                            \
            vs_set_error("%s: this handle is a view; the arrays belong to the index it was made from", what);                         \
            return VS_ERR_STATE;                                                                                                        \
        }                                                                                                                               \
    } while (0)
#define VS_REQUIRE_NO_VIEWS(ix, what)                                                                                                  \
    do {                                                                                                                                \
        const int _nv = vs_index_live_views(ix);                                                                                        \
        if (_nv > 0) {                                                                                                                  \
            vs_set_error("%s: %d view(s) of this index are alive (cursor lanes, a second stream, a vs_multi shard) and hold its device " \
                         "pointers; free them first",                                                                                  \
                         what, _nv);                                                                                                    \
            return VS_ERR_STATE;                                                                                                        \
        }                                                                                                                               \
    } while (0)
int vs_index_reserve_impl(vs_index* ix, uint32_t capacity, const char* what);  // vs_api.hip: arrays may move
// row-wise staging through the pinned ring (device rows may be wider than host rows) / neighbor-list validation
int vs_upload_rows(vs_ctx* c, void* dst, size_t dev_row_bytes, const void* src, size_t host_row_bytes, size_t copy_bytes, size_t rows);
int vs_validate_graph(vs_index* ix);
bool vs_neighbor_masks_wanted(const vs_index* ix);  // policy: > 8M nodes, or VS_F_NBRMASK=1 / 0
int vs_refresh_neighbor_masks(vs_index* ix);  // (re)derives nbr_mask when it is stale (no-op for a view or when it does not fit)
int vs_refresh_label_masks(vs_index* ix);  // (re)derives label_mask / label_bit from the label CSR, or drops them when the index uses more than 64 distinct labels
void devbuf_free(DevBuf& b);
// ---- shared by the host-side translation units (vs_api / vs_slab / vs_batch / vs_tune / vs_cursor .hip) ----------
// an option as a number (vs_options.cpp: vs_set_option, else the snapshot of the VS_* environment), else the default
static inline uint32_t env_u32(const char* name, uint32_t dflt) {
    const char* v = vs_opt_get(name);
    return v && *v ? (uint32_t)strtoul(v, nullptr, 10) : dflt;
}
size_t slab_bytes_wanted(const vs_index* ix);                      // vs_slab.hip: 0 = this index gets no slab
void slab_select(vs_index* ix, WsSlab* s, size_t slab_bytes);     // vs_slab.hip: probes the candidates (caller holds s->mu)
hipEvent_t pool_event(vs_ctx* c);                                  // vs_api.hip: an event from the context's pool
int download_async_rows(vs_ctx* c, void* dst, const void* src, size_t bytes);  // vs_api.hip: rows back through the pinned ring
void stage_copy(void* dst, const void* src, size_t n);                         // vs_api.hip: pageable <-> pinned, split over VS_STAGE_THREADS
int vs_search_batch_dev_impl(vs_index* ix, const float* d_queries, const int16_t* d_qlabels, const uint32_t* d_qlabel_off, uint32_t nq,
                             uint32_t L, uint32_t rescore, uint32_t k, uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist,
                             const uint32_t* d_scan_slots = nullptr,   // vs_batch.hip; d_scan_slots: vs_search_batch_dev_vis
                             const QualLaunch* qual = nullptr);        // qual: a round of vs_search_batch_qual (k kept rows of up to qual->pops)
int vs_search_batch_dev_finish_impl(vs_index* ix, vs_stats* stats);  // vs_batch.hip
void vs_vis_base_drop(vs_index* ix);  // vs_heap_vis.h: frees the base and every overlay of an owner (synchronises its stream first)
void vs_vis_base_free(vs_index* ix);  // ... and the record itself (vs_index_free)
void vs_qual_drop_all(vs_index* ix);  // vs_qual.h: frees every qualifier of an owner and the record (synchronises its stream first)

// ---- kernel launch wrappers (defined in the .hip files) -------------------------------------------------------
struct SearchLaunch {
    uint32_t nq, L, M;
    uint32_t hl;       // candidate-heap entries resident in LDS (heap positions [0, hl))
    uint32_t hcap;     // total candidate-heap capacity; positions [hl, hcap) live in heap_g
    uint32_t vcap;     // visited-list capacity (LDS)
    uint32_t lh;       // slots of the LDS-resident exact dedup table (power of two, 0 = none)
    uint32_t hashcap;  // slots reserved per scan for the global overflow dedup ladder
    uint32_t g0;       // slots of the ladder's first level (power of two); level j has g0 << j slots
    const uint64_t* qcodes;        // [nq][code_stride]
    const int16_t* qlabels;        // may be null
    const uint32_t* qlabel_off;    // may be null => no label keys
    uint64_t* heap_g;              // [nq][hcap - hl]  (untouched unless a heap outgrows LDS)
    uint32_t* hash;                // [nq][hashcap]    (lazily cleared by the kernel when first needed)
    uint32_t* out_ids;             // [nq][M]
    uint32_t* out_ham;             // [nq][M]
    uint32_t* out_cnt;             // [nq]
    uint32_t* stats;               // [nq][8]
    uint32_t* status;              // [nq]
    uint32_t only_failed = 0;      // 1: run only the scans whose status[q] != 0 (left over by the fast kernel)
    uint32_t* pool_counter = nullptr;  // non-null: heap_g / hash hold pool_slots regions claimed with an atomic counter
    uint32_t pool_slots = 0;
    uint32_t* fb_flag = nullptr;   // [nq] set to 1 for every scan this launch ran in only_failed mode
    VisView vis;  // rows whose node it hides (vis_hidden, vs_device.h) are counted and left out of the stream
    // resumable scans (the amgettuple cursor, AM/scan.rs:162-174,370-405): resume[q * resume_stride ..] is scan q's saved state —
    // header RS_* + the LDS image (heap top, LDS dedup table, visited list); its heap spill array / dedup ladder are region q of
    // heap_g / hash and live on between launches.  A launch continues the scan for M more rows (written to out_ids[q][0..M)).
    uint32_t* resume = nullptr;
    uint32_t resume_stride = 0;
    uint32_t* row_stats = nullptr;     // [nq][M][ST_N] the work counters as they stood when each row was emitted (or null)
};
// header of a saved scan (u32 words), followed by the LDS image
enum { RS_INIT = 0, RS_HLEN, RS_HMAX, RS_VLEN, RS_GLEV, RS_NINS_L, RS_NINS_G, RS_NINS_TOP, RS_VISITS, RS_CAND, RS_DQ, RS_READS,
       RS_NEXT, RS_INVIS, RS_STATUS, RS_EMITTED, RS_HDR = 16 };
size_t search_resume_words(const SearchLaunch& s);  // u32 words of one saved scan at these capacities
// fast path (vs_search_fast.hip): all hot state in LDS
struct FastLaunch {
    uint32_t nq, L, M;
    uint32_t hl;       // heap positions resident in LDS, 2^k - 1
    uint32_t hcap;     // total heap capacity; positions [hl, hcap) live in heap_g
    uint32_t gstride;  // u32 per scan in heap_g (even, >= hcap - hl + 2)
    uint32_t lh;       // slots of the LDS dedup table (multiple of 4)
    uint32_t gcap;     // slots of the per-scan global overflow dedup table (a multiple of 256), handles lh .. lh + gcap - 1
    uint32_t glimit = 0;  // ids the global table may hold when a visit starts (gcap x load limit - one wave of inserts); a scan beyond it is handed to the second attempt
    uint32_t sb;       // bits of a slot handle inside a heap entry (lh + gcap <= 1 << sb)
    uint32_t vr;       // visited list: 8 = eight register pairs (512 entries), 0 = LDS ring of vcap entries
    uint32_t vcap;     // visited ring capacity (vr == 0)
    uint32_t minw;     // register cap variant: waves per SIMD to leave room for (1 = unconstrained)
    uint32_t rc = 0;   // entries of the LDS cache of ids known to be in the table (table-less regime; 0 or a power of two)
    uint32_t persist = 0;  // != 0: persistent grid of `persist` workgroups taking scans from scan_counter; regions of heap_g / ghash are per workgroup
    uint32_t vwords = 0;  // != 0: words of the LDS bitmap of written buckets (one bit per four slots of gcap): tables are neither cleared nor read before their first write
    uint32_t vslot = 0;   // with vwords: the bitmap has one bit per SLOT (gcap / 32 words) and the table is probed slot by slot (linear probing)
                          // 2: ... and the table holds 16-BIT entries in buckets of eight (quotienting, see fast_scan VG == 3)
    // vslot == 2: an id is mapped by a bijection on qd bits to x; bucket = x / qe = mulhi(x, qm) >> qs (gcap / 8 buckets, any number),
    // the entry is the remainder x - bucket qe (qe <= 2^16, vs_q16.h); ids whose bucket is full go to an overflow table of ocap 32-bit
    // slots behind the buckets (handles gcap ..); gregion = u32 words per region (gcap / 2 + ocap)
    uint32_t qd = 0, qe = 0, qm = 0, qs = 0, ocap = 0, gregion = 0;
    uint32_t build = 0; // 1: greedy_search_for_build (the visited list is the output; needs vr == 0)
    uint32_t flags = 0; // FAST_* (measurement switches)
    // second attempt of the scans a first launch gave up on (bigger capacities): only scans whose status[q] != 0 run, their
    // heap spill array comes with the dedup table region claimed from the pool (heap_g is [pool_slots][gstride] then), and
    // fb_flag[q] is set for the statistics
    uint32_t only_failed = 0;
    uint32_t* fb_flag = nullptr;
    VisView vis;  // rows whose node it hides (vis_hidden, vs_device.h) are counted and left out of the stream
    const uint64_t* qcodes;
    const int16_t* qlabels;
    const uint32_t* qlabel_off;
    uint32_t* heap_g;  // [nq][gstride] heap positions >= hl
    // the global dedup overflow table is claimed on first need from a pool of pool_slots tables
    uint32_t* ghash;   // [pool_slots][gcap] (cleared by the claiming wave)
    uint32_t* pool_counter;
    uint32_t pool_slots;
    uint32_t* out_ids;
    uint32_t* out_ham;
    uint32_t* out_cnt;
    uint32_t* stats;
    uint32_t* status;
    uint64_t* phase = nullptr;  // optional [nq][8] per-phase shader-clock sums (VS_PHASE=1, diagnostics only)
    uint32_t* scan_counter = nullptr;  // persist: next scan to run (zero before the launch)
    uint64_t* timeline = nullptr;  // optional [nq][2] start / end of every scan in 100 MHz ticks (VS_TIMELINE=1, diagnostics only)
    // resumable scans (the scan pools; as SearchLaunch::resume): resume[q * resume_stride ..] is scan q's saved state — header RSF_* + the
    // LDS image; region q of heap_g / ghash lives on between launches; status[q] != 0 on entry marks the scans that run.  A launch
    // continues a scan for M more rows (out_ids[q][0..M)); row_stats: [nq][M][ST_N] the work counters as each row was emitted.
    uint32_t* resume = nullptr;
    uint32_t resume_stride = 0;
    uint32_t* row_stats = nullptr;
};
enum { RSF_INIT = 0, RSF_HLEN, RSF_VHEAD, RSF_VLEN, RSF_NINS_G, RSF_N_OVF, RSF_HMAX, RSF_VISITS, RSF_CAND, RSF_POPS, RSF_INVIS, RSF_STATUS,
       RSF_NEXT, RSF_ENDED, RSF_HDR = 16 };
size_t fast_resume_words(const FastLaunch& s);
enum {
    // (1 was FAST_PLAIN_ROW_LOADS until round 5: code rows through the normal cache policy; the loads are non-temporal at compile time now)
    FAST_FULL_VARIANT = 8,     // run the instantiation that handles label keys and a visibility mask even when the batch has neither
};
size_t fast_lds_bytes(const vs_index* idx, const FastLaunch& s);
// The 16-bit table form (vslot == 2) of a launch whose gcap is set (any multiple of 256 slots): fills ocap, vwords, vslot, sb, qd, qe, qm,
// qs and gregion as fast_scan (VG == 3) lays the tables out (q16_geometry).  false: the form cannot be represented for this index —
// fewer than 2^(qd - 16) buckets (an entry of more than 16 bits), more than 32 hashed bits, or no room for the Hamming key beside a
// slot handle in a heap entry.
static inline bool fast_tables16_geometry(const vs_index* idx, FastLaunch& f) {
    Q16Geometry g;
    const bool ok = q16_geometry(idx->d.n, f.gcap, &g);
    f.qd = g.qd;
    f.qe = g.qe;
    f.qm = g.qm;
    f.qs = g.qs;
    f.ocap = g.ocap;
    f.vwords = g.vwords;
    f.vslot = 2;
    f.gregion = g.gregion;
    f.sb = g.sb;
    const uint64_t nbits = (uint64_t)idx->d.dim_index * idx->d.bits;
    return ok && nbits < (1ull << (32 - f.sb));
}
int launch_search_fast(vs_index* idx, const FastLaunch& s);
int fast_resident_scans(vs_index* idx, const FastLaunch& s, uint32_t* out);  // size of a persistent grid for this instantiation
// plain storage (vs_search.hip, k_search_plain): one wave per scan on a persistent grid, all state of a scan in LDS or in the
// workgroup's own regions of heap_g / table_g, which are never cleared
struct PlainLaunch {
    uint32_t nq, L, M;
    uint32_t hl;         // candidate-heap entries (8 bytes each) resident in LDS: heap positions [0, hl)
    uint32_t hcap;       // total heap capacity; positions [hl, hcap) live in the workgroup's region of heap_g
    uint32_t vcap;       // visited-list capacity (LDS)
    uint32_t slots;      // slots of the dedup table (a power of two >= 64); one occupancy bit per slot in LDS
    uint32_t ins_limit;  // ids the table may hold (<= 3/4 of the slots); 0xFFFFFFFF: the index has fewer rows than that
    uint32_t lds_table;  // 1: the table's ids live in LDS as well, 0: in the workgroup's region of table_g
    uint32_t persist;    // workgroups of the persistent grid: min(resident, nq)
    uint32_t resident = 0;  // (host side) single-wave workgroups of this LDS size the device holds at once
    VisView vis;
    uint64_t* heap_g = nullptr;       // [persist][hcap - hl]
    uint32_t* table_g = nullptr;      // [persist][slots] (lds_table == 0)
    uint32_t* scan_counter = nullptr;  // next scan to run (zero before the launch)
    uint32_t* out_ids = nullptr;
    uint32_t* out_ham = nullptr;
    uint32_t* out_cnt = nullptr;
    uint32_t* stats = nullptr;
    uint32_t* status = nullptr;
    // the prepared queries [nq][vec_stride] (for a truncated index: the index slices); null: the batch workspace's
    const float* q_prepared = nullptr;
    // resumable scans (the scan pools; k_search_plain_rs, as FastLaunch::resume): one single-wave workgroup per pool slot, no
    // persistent grid and no scan_counter.  status[q] != 0 on entry marks the scans that run.  resume[q * resume_stride ..] is scan
    // q's saved state — header RSP_* + the LDS image (heap top, occupancy bits, LDS table, visited keys and nodes); region q of
    // heap_g / table_g belongs to the SLOT and lives on between launches.  A launch continues the scan for M more rows
    // (out_ids[q][0..M)); row_stats: [nq][M][ST_N] the work counters as each row left next() (or null).
    uint32_t* resume = nullptr;
    uint32_t resume_stride = 0;
    uint32_t* row_stats = nullptr;
};
// header of a saved plain scan (u32 words), followed by the LDS image; RSP_ENDED: next() has returned None (the stream is over for good)
enum { RSP_INIT = 0, RSP_HLEN, RSP_HMAX, RSP_VHEAD, RSP_VLEN, RSP_NINS, RSP_VISITS, RSP_CAND, RSP_DQ, RSP_READS, RSP_NEXT, RSP_INVIS,
       RSP_STATUS, RSP_EMITTED, RSP_ENDED, RSP_HDR = 16 };
static_assert((int)RSP_HDR == (int)RS_HDR && (int)RSP_HDR == (int)RSF_HDR, "a pool clears one header size at amrescan, whichever kernel continues its scans");
static const uint32_t PLAIN_LDS_TABLE_MAX = 1024;  // slots up to which the dedup table's ids live in LDS (4 KB)
size_t plain_lds_bytes(const vs_index* idx, const PlainLaunch& s);
size_t plain_resume_words(const PlainLaunch& s);  // u32 words of one saved scan at these capacities (a multiple of 4)
int launch_search_plain(vs_index* idx, const PlainLaunch& s);
int launch_search_plain_rs(vs_index* idx, const PlainLaunch& s);  // grid = s.nq pool slots; persist / scan_counter are not used
int plain_resident_scans(vs_index* idx, const PlainLaunch& s, uint32_t* out);  // workgroups of k_search_plain the device holds at once
enum { ST_VISITS = 0, ST_CAND = 1, ST_DQ = 2, ST_READS = 3, ST_NEXT = 4, ST_GSPILL = 5, ST_INVIS = 6, ST_INS = 7 /* ids the fast kernel inserted */, ST_N = 8 };
enum { OVF_HEAP = 1, OVF_VISITED = 2, OVF_HASH = 4, OVF_POOL = 8,
       OVF_KEY = 16 };  // (fast kernel only) the scan key has more labels than its LDS slot holds: the general kernel runs the scan
size_t search_lds_bytes(const vs_index* idx, const SearchLaunch& s);

int launch_prepare_queries(vs_index* idx, const float* d_raw, uint32_t nq, float* d_q_full, uint64_t* d_qcodes);
int launch_quantize_rows(vs_index* idx, const float* d_rows, uint32_t row_stride, uint32_t nrows, uint64_t* d_codes,
                         uint32_t code_stride);
int launch_hamming_gather(vs_index* idx, const uint64_t* d_qcodes, const uint32_t* d_ids, const uint32_t* d_off,
                          uint32_t nq, uint32_t* d_out);
int launch_rerank(vs_index* idx, const float* d_q_full, const uint32_t* d_ids, const uint32_t* d_off,
                  const uint32_t* d_cnt, uint32_t fixed_m, uint32_t nq, float* d_out, uint32_t row_base = 0,
                  const uint32_t* d_perm = nullptr, bool deal = false);  // d_perm / deal: as launch_rerank_window
int launch_search(vs_index* idx, const SearchLaunch& s, bool build_mode = false);
int launch_resort(vs_index* idx, uint32_t nq, uint32_t M, uint32_t rescore, uint32_t k, const uint32_t* d_stream_ids,
                  const uint32_t* d_cnt, const float* d_dist, uint64_t* d_heap_ws, uint32_t* d_out_ids,
                  uint64_t* d_out_tids, float* d_out_dist);
// rerank + rescore window of a batch in one launch (rescore > 0; mode 2: the serial heap replay for every scan)
bool rerank_window_fits(const vs_index* idx, uint32_t M, uint32_t rescore, uint32_t k);
int launch_rerank_window(vs_index* idx, const float* d_q_full, const uint32_t* d_stream_ids, const uint32_t* d_cnt, uint32_t M,
                         uint32_t rescore, uint32_t k, uint32_t nq, uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist,
                         uint32_t mode, const uint32_t* d_perm = nullptr, bool deal = false);
int launch_rerank_window_qual(vs_index* idx, const float* d_q_full, const uint32_t* d_stream_ids, const uint32_t* d_cnt, uint32_t M,
                              uint32_t rescore, uint32_t k, uint32_t nq, uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist,
                              uint32_t mode, const uint32_t* d_perm, bool deal, const QualLaunch& ql);
int launch_resort_qual(vs_index* idx, uint32_t nq, uint32_t M, uint32_t rescore, uint32_t k, const uint32_t* d_stream_ids, const uint32_t* d_cnt,
                       const float* d_dist, uint64_t* d_heap_ws, uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, const QualLaunch& ql);
// VS_RERANK_ORDER: the order in which a batch's rerank workgroups take the scans.  d_perm (null = the scans' own order): place ->
// scan number; deal: workgroup b takes place (b % 8) * ceil(nq / 8) + b / 8, a contiguous eighth of the order per XCD
bool scan_order_fits(const vs_index* idx);  // the index has codes k_scan_regions can tile (code rows of up to 38 words)
size_t scan_order_work_bytes(uint32_t nq, uint32_t S);
int launch_scan_order(vs_index* idx, const uint64_t* d_qcodes, uint32_t nq, uint32_t S, uint32_t* d_work, uint32_t* d_perm);
// The same order from labels kept per corpus row: d_labels[i] = the seed row (of S, seed_step rows apart) nearest to row i's code.
// launch_region_labels fills rows [row_begin, row_begin + rows); launch_label_order sorts the scans by (label of the first row of
// their stream, scan number), scans without a row last (key S: d_work holds scan_order_work_bytes(nq, S + 1) bytes).
int launch_region_labels(vs_index* idx, uint32_t S, uint32_t seed_step, uint32_t row_begin, uint32_t rows, uint16_t* d_labels);
int launch_label_order(vs_index* idx, const uint16_t* d_labels, uint32_t lab_rows, uint32_t S, const uint32_t* d_stream_ids,
                       const uint32_t* d_cnt, uint32_t M, uint32_t nq, uint32_t* d_work, uint32_t* d_perm);
// the per-scan arrays a batch's finish reads, summed on the device (k_reduce_stats)
enum { RED_STATUS = 0, RED_VISITS, RED_CAND, RED_DQ, RED_READS, RED_NEXT, RED_FB_SCANS, RED_FB_VISITS, RED_FB_DQ, RED_HEAP_ROWS,
       RED_INS_SUM, RED_INS_MAX, RED_INS_FAST, RED_INS_OV, RED_N = 16 };
int launch_reduce_stats(vs_index* idx, const uint32_t* d_stats, const uint32_t* d_fb, const uint32_t* d_cnt, const uint32_t* d_status,
                        uint32_t nq, uint32_t M, uint32_t rescore, bool windowed, bool has_visible, uint32_t ins_limit, uint64_t* d_red);
int launch_resort_cursor(vs_index* idx, uint32_t n, bool exhausted, uint32_t rescore, uint32_t k, const uint32_t* d_stream,
                         const float* d_dist, const uint32_t* d_keys, uint64_t* d_heap, uint32_t* d_cur, uint32_t* d_out_ids,
                         uint64_t* d_out_tids, float* d_out_dist);
int launch_resort_cursor_batch(vs_index* idx, uint32_t n, const uint32_t* d_list, uint32_t rescore, uint32_t k, const uint32_t* d_stream,
                               const float* d_dist, const uint32_t* d_keys, uint32_t row_stride, uint64_t* d_heap, uint32_t* d_cur,
                               uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, uint32_t out_stride);
int launch_pool_append(vs_index* idx, uint32_t nq, const uint32_t* d_cnt, const uint32_t* d_off, const uint32_t* d_stage, uint32_t stage_kind_stride, uint32_t M,
                       uint32_t* d_all, uint32_t all_kind_stride, uint32_t rows_cap);
// the resumable window under a qualifier (k_resort_cursor_batch_qual, vs_kernels.hip): what a launch reports per scan next to the
// public states, and the most pops one launch may make within 64 KB of LDS (0: the window does not fit at all)
enum { VS_PQ_LIMIT = 2, VS_PQ_STARVED = 4 };
uint32_t resort_cursor_qual_max_chunk(uint32_t rescore, uint32_t k, uint32_t rows_cap);
int launch_resort_cursor_batch_qual(vs_index* idx, uint32_t n, const uint32_t* d_list, uint32_t rescore, uint32_t k, uint32_t chunk,
                                    const uint64_t* const* d_qtab, const uint32_t* d_stream, const float* d_dist, const uint32_t* d_keys,
                                    uint32_t row_stride, uint64_t* d_heap, uint32_t* d_cur, uint32_t* d_rec, uint32_t* d_out_ids,
                                    uint64_t* d_out_tids, float* d_out_dist, uint32_t out_stride);
// P1 of a qualified scan (vs_qual.h): the pops after which a scan under a qualifier of this density is expected to have its k rows
uint32_t vs_qual_first_pops(uint32_t k, uint32_t max_pops, double density);
int launch_row_norms(vs_index* idx);
int launch_row_norms_range(vs_index* idx, uint32_t row_begin, uint32_t rows);  // the same for rows [row_begin, row_begin + rows)
int vs_quantize_row_range(vs_index* ix, uint32_t row_begin, uint32_t rows);     // vs_extra.hip: vs_sbq_quantize_corpus over a row range
int launch_slice_norms(vs_index* idx, float* d_out);  // divisor of the first dim_index dims of every heap vector
// raw_stride: floats between two raw rows (0: dim_full, a caller's packed queries; vec_stride: rows of the index's own vector column)
int launch_prepare_index_slice(vs_index* idx, const float* d_raw, uint32_t nq, float* d_q_index, uint32_t raw_stride = 0);
int launch_slice_norms_range(vs_index* idx, uint32_t row_begin, uint32_t rows);  // vnorm_idx of rows [row_begin, row_begin + rows)
int launch_validate_nbrs(vs_index* idx, uint32_t* d_flag);
int launch_scan_topk(vs_index* idx, const uint64_t* d_qcodes, uint32_t nq, uint32_t k, uint32_t* d_out_ids,
                     uint32_t* d_out_ham, const int16_t* d_qlabels = nullptr, const uint32_t* d_qlabel_off = nullptr,
                     bool live_only = false);
