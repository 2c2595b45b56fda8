/*
 * vsgpu.h — C ABI of libvsgpu.so: the MI355X (gfx950) implementation of pgvectorscale's StreamingDiskANN
 * *search* hot path (SBQ Hamming candidate scoring inside the greedy graph search + f32 rerank), i.e. the work
 * done between `amrescan` and `amgettuple` of the `diskann` access method.
 *
 * Citations are relative to /root/reference/pgvectorscale/src/access_method/ ("AM/").
 *
 * The reference has NO FFI seam on this path (storages / distance functions are statically dispatched Rust,
 * AM/storage.rs:41-142, AM/distance/mod.rs:8); its only C-ABI surface is the IndexAmRoutine filled in by
 * `amhandler` (AM/mod.rs:27-92).  This header therefore declares what a PGRX shim would bind from inside those
 * callbacks (the Rust `extern "C"` block is shown in INTEGRATION.md):
 *
 *   ambeginscan (AM/scan.rs:308-333) -> vs_beginscan        amrescan  (AM/scan.rs:335-367) -> vs_rescan
 *   amgettuple  (AM/scan.rs:369-436) -> vs_gettuple         amendscan (AM/scan.rs:438-456) -> vs_endscan
 *
 * plus the batched entry points (many backends' queries at once; what a GPU broker process would call) and the
 * individual kernels K1..K5 of SURVEY.md §2.
 *
 * Rules: plain C types only; every call returns 0 (VS_OK) or a negative vs_status and never throws / longjmps;
 * vs_last_error() gives a thread-local message (the Rust side turns it into pgrx::error!); the caller owns every
 * host buffer; the library owns device memory and pinned staging buffers; calls are synchronous unless their name
 * ends in _async; one thread per vs_ctx at a time.  There is NO CPU fallback: without a HIP device every compute
 * entry point fails with VS_ERR_HIP.
 */
#ifndef VSGPU_H
#define VSGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VS_INVALID_NODE 0xFFFFFFFFu /* InvalidBlockNumber sentinel ending a neighbor list, AM/sbq/node.rs:260-285 */

enum vs_distance_type { VS_COSINE = 0, VS_L2 = 1, VS_IP = 2 }; /* AM/distance/mod.rs:11-15 */
/* memory_optimized (SbqSpeedupStorage: SBQ Hamming in the graph search + f32 rerank, the hot path of this library) or
 * plain (PlainStorage, AM/plain/storage.rs: the graph search scores candidates with the full-precision distance to the
 * vector stored in the node (its index slice when num_dimensions_to_index < num_dimensions, then the rows are resorted on the
 * full vectors); no label filters) */
enum vs_storage_type { VS_STORAGE_SBQ = 0, VS_STORAGE_PLAIN = 1 };

enum vs_status {
    VS_OK = 0,
    VS_ERR_INVALID = -1,  /* bad argument / malformed index (e.g. duplicate ids inside one neighbor list) */
    VS_ERR_HIP = -2,      /* HIP runtime error or no device */
    VS_ERR_OOM = -3,      /* device or pinned-host allocation failed */
    VS_ERR_CAPACITY = -4, /* a per-query search structure overflowed even after the automatic retries */
    VS_ERR_STATE = -5     /* call sequence error (e.g. vs_gettuple before vs_rescan) */
};

typedef struct vs_ctx vs_ctx;     /* one HIP device + streams + staging buffers */
typedef struct vs_index vs_index; /* one diskann index resident in HBM */
typedef struct vs_scan vs_scan;   /* one IndexScanDesc's opaque state (TSVScanState, AM/scan.rs:40-89) */

/* Index geometry = the MetaPage fields that parameterise the search (AM/meta_page.rs:179-210). */
typedef struct vs_index_desc {
    uint32_t n;             /* index nodes; node id = dense position (stands in for the ItemPointer)            */
    uint32_t dim_full;      /* num_dimensions                                                                 */
    uint32_t dim_index;     /* num_dimensions_to_index (<= dim_full)                                          */
    uint32_t bits;          /* num_bits_per_dimension; default 2 if dim_index < 900 else 1 (:312-323)         */
    uint32_t words;         /* W = ceil(dim_index*bits/64) u64 words per SBQ code (AM/sbq/quantize.rs:37-45) */
    uint32_t num_neighbors; /* R (default 50, :284-294)                                                       */
    uint32_t distance_type; /* vs_distance_type                                                               */
    uint32_t has_labels;    /* MetaPage.has_labels                                                            */
    uint32_t default_start; /* StartNodes.default_node or VS_INVALID_NODE for an empty graph                  */
    uint32_t n_label_starts;/* entries of StartNodes.labeled_nodes (AM/graph/start_nodes.rs:17-22)            */
    uint32_t storage_type;  /* vs_storage_type: which Storage the index was built with (AM/storage.rs)        */
} vs_index_desc;

/* Host-side flat arrays an exporter produces from the index relation's pages (SbqNode items, AM/sbq/node.rs:26-42;
 * SbqMeans chain, AM/sbq/mod.rs:62-121) and from the heap's vector column. */
typedef struct vs_index_host {
    const uint64_t* codes;     /* [n][words]            ArchivedSbqNode.bq_vector                             */
    const uint32_t* nbrs;      /* [n][nbr_stride]       neighbor_index_pointers, list ends at VS_INVALID_NODE */
    uint32_t nbr_stride;       /* row stride of `nbrs` in elements (>= num_neighbors)                         */
    const uint64_t* heap_tids; /* [n] (block<<16)|offset; offset==0 (InvalidOffsetNumber) => deleted tuple    */
    const float* vecs;         /* [n][dim_full] heap vectors (raw); NULL => no rerank possible (rescore must be 0) */
    const float* mean;         /* [dim_index]           SbqMeans.means                                        */
    const float* m2;           /* [dim_index]           SbqMeans.m2 (bits>1; may be NULL when bits==1)        */
    uint64_t count;            /* SbqMeans.count                                                              */
    const uint32_t* label_off; /* [n+1] CSR offsets into label_val (has_labels)                               */
    const int16_t* label_val;  /* per-node sorted, de-duplicated label sets (AM/labels/mod.rs:15-37)          */
    const int16_t* label_start_labels; /* [n_label_starts] sorted keys of StartNodes.labeled_nodes            */
    const uint32_t* label_start_nodes; /* [n_label_starts] their start nodes                                  */
} vs_index_host;

/* GreedySearchStats + TSVResponseIterator counters (AM/stats.rs:68-125, AM/scan.rs:461-472), summed over the call */
typedef struct vs_stats {
    uint64_t queries;
    uint64_t visited_nodes;                  /* "visits"       */
    uint64_t candidate_nodes;                /* "candidate"    */
    uint64_t quantized_distance_comparisons; /* "d_quantized"  */
    uint64_t full_distance_comparisons;      /* "d_full"       */
    uint64_t node_reads;                     /* "reads_index"  */
    uint64_t node_heap_reads;                /* "reads_heap"   */
    uint64_t next_calls;                     /* "next"         */
    uint64_t retries;                        /* capacity-overflow relaunches (ours; 0 in steady state) */
    uint64_t fallback_scans;                 /* scans the LDS-resident fast kernel handed to the general kernel (ours) */
    uint64_t fallback_visited_nodes;         /* their share of visited_nodes */
    uint64_t fallback_quantized_distance_comparisons; /* their share of quantized_distance_comparisons */
} vs_stats;

const char* vs_last_error(void);

/* Which kernel the first attempt of a handle's last batch (its last chunk) ran, and with which planned capacities.  Read-only: it
 * changes no launch.  VS_ERR_INVALID for NULL arguments, VS_ERR_STATE before the first batch of the handle. */
enum { VS_SEARCH_GENERAL = 0, VS_SEARCH_FAST_SBQ = 1, VS_SEARCH_FAST_PLAIN = 2 };
typedef struct vs_search_info {
    uint32_t kernel;       /* what the first attempt of the last batch (chunk) ran */
    uint32_t resident;     /* scans in flight on the persistent grid (0: general kernel) */
    uint32_t lds_bytes;    /* dynamic LDS per scan of that launch */
    uint32_t heap_lds, dedup_slots, visited_cap;  /* the planned on-chip capacities (0 where not applicable) */
    uint32_t reserved[2];
} vs_search_info;
int vs_index_last_search_info(const vs_index* idx, vs_search_info* out);

/* Tuning options (launch variants, capacities, slab placement, diagnostics), process wide.  `name` is one of the
 * VS_* names listed there, `value` its text ("3", "0", a path ...; NULL unsets it again).  An option set here wins over the environment
 * variable of the same name; the environment itself is only SNAPSHOT — at the first lookup and again when the process's VS_* variables
 * change — never searched on the launch path.  No reference counterpart: these are the knobs of this implementation (the reference's
 * own GUCs, diskann.query_search_list_size and diskann.query_rescore, are arguments of vs_rescan / vs_search_batch).  Thread safe.
 * vs_get_option: 1 = set (copied to out, truncated to cap), 0 = set nowhere (out = "").
 * VS_RERANK_FUSED: how a batch reranks and runs the rescore window — "1" (default) one fused launch, "2" fused with the serial heap
 * replay for every scan, "0" the separate rerank and window kernels; the rows are the same under all three.
 * VS_RERANK_ORDER: the order in which a batch's rerank takes its scans — "1" (default) grouped by corpus neighbourhood when the batch
 * re-reads rows (nq x rows per scan >= 2 n and nq >= 16384), "2" / "3" always, "0" never (the scans' own order).  The neighbourhood
 * of a scan: under "1" and "3" the region label of the first row of its stream — a label per corpus row (its nearest seed row), built
 * by the first batch that needs it and rebuilt when the codes or the row numbers have changed; under "2" (and on a view handle) the
 * seed row nearest to the query's own code, computed per batch.  VS_RERANK_SEEDS corpus rows define the neighbourhoods (up to 4096;
 * default 2048 for the labels, 1024 for the per-batch seed pass); VS_RERANK_DEAL "0" keeps the order but not the per-XCD split.  The
 * rows returned are the same, bit for bit, under every setting.
 * VS_PLAIN_FAST: which kernel a batch over a `plain` storage index tries first — "1" (default) k_search_plain, one wave per scan on a
 * persistent grid with the scan's state on chip, the general kernel re-running the scans that outgrow it (counted in
 * vs_stats.fallback_scans); "0" the general kernel alone.  Rows, distance bits and the reference counters are the same under both.
 * Its capacities, for tests and measurement (0 / unset = planned from n, num_neighbors, the search list size and the stream length):
 * VS_PF_HEAP_LDS (heap entries kept in LDS), VS_PF_HEAP_CAP (heap entries in all), VS_PF_DEDUP_SLOTS (slots of the dedup table,
 * rounded up to a power of two), VS_PF_VISITED (visited-list capacity), VS_PF_SCANS_PER_CU (upper bound of the persistent grid).
 * VS_POOL_PLAIN_FAST: which kernel continues the scans of a scan pool (vs_scanpool_*) over a `plain` storage index — "1" (default) the
 * resumable form of k_search_plain, one wave per pool slot with the scan's state on chip during a launch and saved per slot between
 * launches, where that state fits 96 KB of LDS; "0" (or VS_POOL_FAST "0") the general kernel.  Read when a pool is created, as
 * are VS_PF_HEAP_LDS / VS_PF_HEAP_CAP / VS_PF_DEDUP_SLOTS / VS_PF_VISITED, which override the pool's planned capacities too (a pooled
 * scan that outgrows one fails with VS_ERR_CAPACITY).  Rows, distance bits and the reference counters are the same under both.
 * VS_POOL_QUAL_CHUNK: the pops ONE window launch of vs_scanpool_fetch_qual may make per scan (default 4096, capped so that the launch
 * stays within 64 KB of LDS); a fetch that needs more launches again.  A cost choice: no row, count or state depends on it. */
int vs_set_option(const char* name, const char* value);
int vs_get_option(const char* name, char* out, size_t cap);
const char* vs_version(void);

/* ---- context ------------------------------------------------------------------------------------------------- */
int vs_ctx_create(int device, vs_ctx** out);            /* staging ring: 2 x 32 MiB of pinned host memory */
/* the same with a staging ring of 2 x staging_bytes: the contexts of cursor lanes and other handles that move a few rows per call
 * (vs_broker_config.cursor_lanes creates up to 64 of them per broker) take 2 x 1 MiB instead of 2 x 32 MiB */
int vs_ctx_create_staging(int device, size_t staging_bytes, vs_ctx** out);
void vs_ctx_destroy(vs_ctx* ctx);
int vs_ctx_sync(vs_ctx* ctx);          /* wait for the compute stream */
void* vs_ctx_stream(vs_ctx* ctx);      /* the hipStream_t all kernels of this ctx are launched on */
int vs_ctx_device_name(vs_ctx* ctx, char* buf, size_t len);
int vs_ctx_mem_info(vs_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes);

/* per-kernel timing with HIP events recorded on the ctx stream around every launch of the batched-scan pipeline
 * (what bench.py's roofline figure is computed from).  kind: 0 prepare_queries, 1 search (the LDS-resident fast
 * kernel; the general kernel when the fast path is off), 2 rerank, 3 resort, 4 search fallback (general kernel re-running
 * the scans the fast kernel handed over), 5 flat SBQ scan (vs_scan_topk), 6 rerank order, 7 page encode (vs_pages_out_*). */
typedef struct vs_profile {
    double ms[8];        /* accumulated kernel time per kind */
    uint64_t launches[8];
} vs_profile;
int vs_profile_enable(vs_ctx* ctx, int on);
int vs_profile_read(vs_ctx* ctx, vs_profile* out, int reset); /* synchronises the stream */

/* raw device buffers (so callers can keep inputs resident in HBM across calls) */
int vs_dev_alloc(vs_ctx* ctx, size_t bytes, void** out);
int vs_dev_free(vs_ctx* ctx, void* p);
int vs_dev_upload(vs_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);   /* pinned staging + hipMemcpyAsync */
int vs_dev_download(vs_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);

/* ---- index ---------------------------------------------------------------------------------------------------- */
/* Stage host arrays chunk-wise through pinned buffers to HBM (hipMemcpyAsync, double-buffered) and validate them. */
int vs_index_upload(vs_ctx* ctx, const vs_index_desc* desc, const vs_index_host* host, vs_index** out);
/* Allocate an index whose arrays are produced on the device (vs_datagen_*, vs_sbq_train, vs_sbq_quantize_corpus,
 * vs_build_graph); contents are undefined until filled.  desc->storage_type == VS_STORAGE_PLAIN allocates a `plain` index: it
 * needs with_vecs and takes no labels (has_labels 0; vs_index_set_labels refuses it); its graph comes from vs_build_graph and
 * vs_index_insert, which score with full-precision distances on the vector column. */
int vs_index_alloc(vs_ctx* ctx, const vs_index_desc* desc, int with_vecs, vs_index** out);
void vs_index_free(vs_index* idx);
/* A second handle on the SAME device arrays with its own search workspace, bound to `ctx` (another HIP stream of the same device):
 * batches submitted through different views run concurrently — the bandwidth-bound rerank of one under the latency-bound search
 * of the next.  The reference has one backend per scan and nothing to share (AM/scan.rs:308-333); this is the handle a GPU broker
 * gives each of its submission lanes.  The arrays stay owned by `src`: no upload / build / visibility change while a view has a
 * batch in flight, and every view is freed before `src`. */
int vs_index_view(vs_index* src, vs_ctx* ctx, vs_index** out);
/* The search workspace's randomly accessed part (the persistent grid's per-workgroup dedup tables and heap spill arrays) lives in ONE
 * grow-only slab per index, shared with its views (VS_WS_SLAB_MB, default 2 GiB per kind from 4M nodes; chosen by the first search among VS_WS_SLAB_CANDIDATES probed allocations).
 * vs_index_set_slab hands the library the CALLER's device memory for it instead (before the handle's first search; the memory stays the
 * caller's and must outlive the handle and the views made of it afterwards) — for a host that manages HBM itself, or one that has
 * measured where those regions run fastest: vs_ws_probe times the same request shapes (random 16-byte loads, 4-byte stores, 8-byte
 * loads in 24 private shares per CU) on any device region of at least 64 MiB.  No reference counterpart (PostgreSQL's buffer manager
 * places the reference's pages); placement moves k_search_fast by several percent at identical bytes ("State"). */
int vs_index_set_slab(vs_index* idx, void* d_mem, size_t bytes);
int vs_ws_probe(vs_ctx* ctx, void* d_mem, size_t bytes, uint32_t iters, float* ms_out);
/* ... and vs_ws_probe_mix the kernel's WHOLE request mix, with the neighbor rows and code rows read from this index's arrays and the
 * private state on the region (tables at its start, heap arrays in its second half): what the library itself uses to choose its slab
 * among VS_WS_SLAB_CANDIDATES allocations (default 8, spread over the free device memory by spacers) at the first search of an index of 4M nodes or more. */
int vs_ws_probe_mix(vs_index* idx, void* d_mem, size_t bytes, uint32_t iters, float* ms_out);
/* Chooses the slab NOW instead of inside the first search (after the index's arrays are uploaded / loaded; a no-op for an index that
 * has its slab, has none by the size rule, or is a view).  The probing holds its candidates and spacers for a fraction of a second:
 * at most VS_WS_SLAB_PROBE_PCT (default 50) per cent of the device memory that is free at that moment and never the last
 * VS_WS_SLAB_KEEP_FREE_MB (default 12 GiB) — a host that shares the device calls this at index load, when nobody else allocates. */
int vs_index_prepare_workspace(vs_index* idx);
int vs_index_get_desc(const vs_index* idx, vs_index_desc* out);
enum vs_array { VS_ARR_CODES = 0, VS_ARR_NBRS = 1, VS_ARR_TIDS = 2, VS_ARR_VECS = 3, VS_ARR_MEAN = 4, VS_ARR_M2 = 5,
                VS_ARR_VNORM = 6, VS_ARR_LABEL_OFF = 7, VS_ARR_LABEL_VAL = 8 };
/* device pointer + row stride (in elements) of one of the index arrays.  The caller may write through the pointer, so a hand-out of
 * VS_ARR_NBRS or VS_ARR_CODES marks what the library derived from that array as stale (the neighbors' label masks; the region labels
 * of VS_RERANK_ORDER, rebuilt by the next batch that orders by them: milliseconds at 4M rows) — also when the call only wanted the
 * stride.  It costs time, never a result; a caller on a hot path asks once and keeps the answer. */
int vs_index_array(const vs_index* idx, int which, void** dev_ptr, uint32_t* row_stride);
/* diagnostics: the rerank order of the handle's last batch (VS_RERANK_ORDER) — place -> scan number, *out_n entries (0: that batch
 * took the scans' own order), at most cap of them copied to out_perm.  Synchronises the stream. */
int vs_index_rerank_order(vs_index* idx, uint32_t* out_perm, uint32_t cap, uint32_t* out_n);
int vs_index_set_quantizer(vs_index* idx, const float* mean, const float* m2, uint64_t count);
int vs_index_set_start_nodes(vs_index* idx, uint32_t default_start, const int16_t* labels, const uint32_t* nodes, uint32_t n);
int vs_index_set_labels(vs_index* idx, const uint32_t* label_off, const int16_t* label_val);
/* Heap visibility under the scan's snapshot, one byte per node (0 = index_fetch_tuple finds no tuple this snapshot can see).
 * Replaces the `None` arm of get_full_distance_for_resort (AM/sbq/storage.rs:313-317, AM/plain/storage.rs:181-184, reached
 * from next_with_resort, AM/scan.rs:258-272): with query_rescore > 0 such a candidate is fetched (counted as a heap read and a
 * full-distance comparison) and dropped BEFORE it enters the rescore window; with query_rescore = 0 the access method does not
 * look at the heap (the executor does) and the mask is ignored.  `visible` is a host array of n bytes, NULL = every tuple
 * visible (the default).  The mask applies to every scan started afterwards (a PGRX shim sets it per snapshot / batch). */
int vs_index_set_visibility(vs_index* idx, const uint8_t* visible);
/* the same with the mask already in device memory (n bytes, kept by the caller until replaced; NULL clears it) */
int vs_index_set_visibility_dev(vs_index* idx, const uint8_t* d_visible);
/* Shared launches (vs_broker / vs_shm) serve backends with DIFFERENT snapshots, so one mask per index is not enough there: the
 * index keeps up to VS_MAX_SNAPSHOTS - 1 masks (ids 1 .. VS_MAX_SNAPSHOTS - 1; `visible` = n host bytes, NULL drops the mask) and
 * a launch runs under the one its scans name; id 0 = every tuple visible.  vs_index_snapshot_use makes snapshot `id` the
 * mask of the launches that follow and returns the mask that was in force (restore it with vs_index_set_visibility_dev).
 * Same threading rule as every index call: with a broker attached only its dispatcher may call these — clients go through
 * vs_broker_snapshot_put / vs_shm_server_snapshot_put. */
#define VS_MAX_SNAPSHOTS 16
int vs_index_snapshot_put(vs_index* idx, uint32_t snapshot, const uint8_t* visible);
int vs_index_snapshot_use(vs_index* idx, uint32_t snapshot, const uint8_t** previous /* may be NULL */);
/* (for the lanes of a broker) a view takes over the snapshot masks its source holds right now — the masks stay the source's */
int vs_index_snapshot_share(vs_index* view, const vs_index* src);
int vs_index_device(const vs_index* idx); /* the HIP device of the index's context */
/* 1 when the label masks of every node's neighbors are cached next to the neighbor rows: label-filtered scans on an index of
 * <= 64 distinct labels and more than 8M nodes build the cache on first use when device memory allows (+6.7 % at 20M, +0.6 % at
 * 5M, where the masks are cache resident anyway); VS_F_NBRMASK=1 / 0 forces it on / off */
int vs_index_has_neighbor_masks(const vs_index* idx);
int vs_index_get_quantizer(const vs_index* idx, float* mean, float* m2, uint64_t* count);
/* copy index arrays back to host (tests / cpu_baseline leg); any pointer may be NULL */
int vs_index_download(const vs_index* idx, uint64_t* codes, uint32_t* nbrs /*[n][num_neighbors]*/, uint64_t* heap_tids,
                      float* vecs, uint32_t row_begin, uint32_t row_count);
/* (re)compute the per-node cosine divisor cache from the vector column (exact preprocess_cosine semantics,
 * AM/distance/mod.rs:225-253), and on a plain cosine index with dim_index < dim_full the cache of the index slices' divisors too;
 * called by upload automatically */
int vs_index_refresh_norms(vs_index* idx);
/* Gives an index that was made without a vector column (vs_pages_dev_build / vs_index_upload with vecs == NULL) a zeroed one: the
 * stride and rows vs_index_alloc(with_vecs = 1) would choose, plus the cosine divisor cache.  The caller fills the rows through
 * vs_index_array(VS_ARR_VECS) (vs_heap_dev_* writes there directly) and calls vs_index_refresh_norms; searches with rescore > 0 and
 * vs_rerank then work as if the index had been uploaded with the column.  VS_OK and nothing done if the column exists.
 * VS_ERR_STATE: a view handle, live views, a batch in flight, an open page writer.  A column that does not fit leaves the index as
 * it was (VS_ERR_OOM). */
int vs_index_alloc_vecs(vs_index* idx);
/* mark heap tuples deleted (what ambulkdelete does to heap_item_pointer, AM/vacuum.rs:24-78) */
int vs_index_mark_deleted(vs_index* idx, const uint32_t* nodes, uint32_t n);
/* ambulkdelete by heap TID (bulk_delete_for_storage, AM/vacuum.rs:80-136: every live node's heap_item_pointer is put to the
 * callback, a dead one has its pointer invalidated and the page is committed only `if modified`).  dead_tids: host array of
 * (block << 16) | offset, unsorted, duplicates allowed; an entry with offset 0 (InvalidOffsetNumber) is VS_ERR_INVALID and
 * nothing is changed.  The library stages the array through the pinned ring and sorts it on the device; the _dev form takes a
 * device array that is already sorted ascending and de-duplicated.  One kernel over the TID column on the context's stream:
 * a node whose offset is 0 already is skipped (is_deleted(), :112), a binary search in the dead set decides for the others, a
 * hit clears the low 16 bits — exactly what vs_index_mark_deleted writes.  The block number STAYS (the reference invalidates
 * it too, ItemPointerSetInvalid; here the pages written by vs_pages_out_* keep it, and is_deleted() only looks at the offset).
 * The call is ordered on the context's stream after whatever that stream has in flight and synchronises only to hand back the
 * three counters; VS_ERR_STATE while a batch of this handle is in flight (vs_search_batch_dev_finish first).  SBQ and plain
 * storage alike: only the heap tids are touched.  The library's visibility masks are left alone: the scans drop a deleted
 * node by the rule of AM/scan.rs:231-234 already. */
typedef struct vs_bulk_delete_stats { /* IndexBulkDeleteResult, AM/vacuum.rs:122-129 */
    uint64_t tuples_removed;          /* live nodes whose heap TID was in the dead set: marked now    */
    uint64_t num_index_tuples;        /* live nodes that stay                                          */
    uint64_t already_deleted;         /* nodes skipped because is_deleted() (counted in neither, :112) */
} vs_bulk_delete_stats;
int vs_index_bulk_delete(vs_index* idx, const uint64_t* dead_tids, uint64_t n_dead, vs_bulk_delete_stats* out /* may be NULL */);
int vs_index_bulk_delete_dev(vs_index* idx, const uint64_t* d_dead_tids_sorted, uint64_t n_dead, vs_bulk_delete_stats* out);
/* ---- consolidation of deleted rows (what a PGRX shim calls from amvacuumcleanup, after ambulkdelete) -------------------------
 * Neither the reference nor vs_index_bulk_delete cleans up after a delete: a tombstone (heap offset 0) keeps its neighbor list
 * and every in-edge live rows hold to it, so scans still gather, score, visit and expand it (only `consume` drops it,
 * AM/scan.rs:231-234) and an insert links new rows to it.  The reference's only cure is REINDEX.  This call is the consolidation
 * pass of streaming DiskANN instead: every row that names a deleted neighbor takes over that neighbor's neighbors and is pruned
 * again.  The rule, evaluated on the graph as it stands when the call starts:
 *   K = every node whose heap offset is not 0, plus the default start node and every per-label start node even when deleted
 *       (scans begin there whatever their state); D = every other node.
 *   Rows of D are never written.  Rows of K that name no node of D stay byte-identical.
 *   A row p of K that names a node of D gets the candidates { v in N(p), v in K } + { w in N(d), d in N(p) and D, w in K }, without
 *   p, every id once — one level: a tombstone's tombstone neighbors are not followed — sorted ascending by (Hamming(code[p],
 *   code[w]), id), cut to the first cand_max (0 = min(4 * num_neighbors, 256); VS_ERR_INVALID unless num_neighbors < cand_max <=
 *   1024).  At most num_neighbors candidates: they are the row, in that order (add_neighbors, AM/graph/mod.rs:243-256).  More: the
 *   row is what prune_neighbors selects, in selection order (alpha ladder 1.0, x 1.2f while <= max_alpha; contains_intersection
 *   relative to p for a labeled index), exactly as vs_build_graph prunes.  The row is padded with VS_INVALID_NODE.
 *   Then, unless VS_CONSOLIDATE_NO_REPAIR is set, the repair pass of vs_build_graph runs with one difference: a node of D is not
 *   "lost" — it is meant to be unreachable and is never handed an in-edge again.  CALLING vs_index_repair AFTER A CONSOLIDATION
 *   WOULD RE-LINK THE TOMBSTONES (it knows no D); use this call's own repair.
 * What it does not do: it never reclaims a tombstone's node (n and the page layout stay, D rows keep their bytes, so their pages
 * stay clean for vs_pages_out_delta; vs_index_compact below is the call that reclaims them); it does not re-elect a deleted start node (it stays in K with a clean list); it gives no
 * guarantee for label-filtered reachability beyond what Graph::insert gives (vs_index_label_reach audits it, vs_index_repair_labels repairs it).
 * Refusals leave every byte as it was: VS_ERR_INVALID for plain storage (vs_index_consolidate_deletes_plain below is the call
 * for it), an index without codes / neighbor lists / heap tids, a
 * node with more than 64 labels, max_alpha outside [1,5], a bad cand_max or unknown flags; VS_ERR_STATE while a view of the index
 * is alive, a batch of this handle is in flight, or a writer opened with vs_pages_out_open / _open_plain has not been closed.  n does not change
 * and no array moves, but open vs_scans, scan pools and brokers of the index must be ended or rescanned afterwards: their device
 * state names rows that changed.  Not thread safe against any other call on the index; ordered on the context's stream.
 * An error after the first rewritten row (a HIP error, memory running out for the repair pass) leaves a usable graph: every row
 * is rewritten whole by one wave from rows nobody writes, so each row is either its old list or its new one, both valid lists;
 * calling again finishes the work (a rewritten row names no node of D and is skipped).  `out` then holds what was counted. */
#define VS_CONSOLIDATE_NO_REPAIR 1u   /* flags: stop after the row rewrite (tests; callers that run the repair themselves) */
typedef struct vs_consolidate_stats {
    uint64_t tombstones;         /* nodes whose heap offset is 0 */
    uint64_t tombstones_kept;    /* of those: default / per-label start nodes, which stay in the graph */
    uint64_t rows_rewritten;     /* kept nodes whose list named >= 1 dropped tombstone */
    uint64_t edges_dropped;      /* list entries that named a dropped tombstone */
    uint64_t edges_added;        /* entries of the new lists that the old lists did not hold */
    uint64_t rows_pruned;        /* rewritten rows whose candidates exceeded num_neighbors (went through prune) */
    uint64_t rows_capped;        /* rewritten rows whose de-duplicated candidates exceeded cand_max */
    uint64_t rows_emptied;       /* rewritten rows left without a neighbor */
    uint32_t unreachable_live;   /* live nodes the default start node does not reach at return (0xFFFFFFFF: not judged, as
                                  * vs_index_build_unreachable; also with VS_CONSOLIDATE_NO_REPAIR) */
} vs_consolidate_stats;
int vs_index_consolidate_deletes(vs_index* idx, double max_alpha, uint32_t cand_max /* 0 = default */, uint32_t flags,
                                 vs_consolidate_stats* out /* may be NULL */);
/* The same pass over a `plain` index (VS_STORAGE_PLAIN): the same K and D, the same candidates one level deep, the same cut to
 * cand_max (same default, same bound), the same counters, the same repair pass and flag.  The one difference is the distance: the
 * candidates of row p are sorted ascending by (key of d(p -> w), id), d the full-precision pair distance vs_build_graph scores a
 * plain index with (p's prepared index slice is the query side, w's raw row the row side; keys order like f32::total_cmp), and
 * pruned with that distance ("plain storage").  A plain index has no labels, so there is no label rule.
 * Only neighbor lists are written.  Indexes made with vs_index_alloc, vs_index_upload or from pages are taken alike: a mirrored
 * relation stays writable with vs_pages_out_open_plain.  The cosine divisors of the rows are recomputed from the vector column
 * first, as vs_build_graph does (a derived cache, not a byte of the index).
 * Refusals leave every byte as it was: VS_ERR_INVALID for an SBQ index (vs_index_consolidate_deletes is the call for it), an
 * index the pair distance cannot score (the inner-product distance, no vector column on the device, a cosine index with dim_index
 * < dim_full that holds no divisors of its index slices), an index without neighbor lists / heap tids, max_alpha outside [1,5], a
 * bad cand_max, unknown flags, or a num_neighbors / cand_max / dim_index whose LDS layout exceeds 160 KiB; VS_ERR_STATE for a view
 * handle, live views, a batch in flight, or an open writer of either kind.  Everything else said above holds unchanged. */
int vs_index_consolidate_deletes_plain(vs_index* idx, double max_alpha, uint32_t cand_max /* 0 = default */, uint32_t flags,
                                       vs_consolidate_stats* out /* may be NULL */);
/* HIP-event milliseconds of the two passes on this index since the last reset, collected while vs_profile_enable is on:
 * ms[0] the flag pass (node classes, flags, work list), ms[1] k_consolidate_rows (either form) */
int vs_index_consolidate_kernel_ms(vs_index* idx, double* ms, int reset);
/* ---- compaction: the tombstones leave the arrays and the nodes are renumbered in place (after the consolidation above) --------
 * The last step of delete -> consolidate -> compact -> insert into the freed room.  Node ids are internal: what leaves the boundary
 * is the heap tid, and no search ordering depends on an id beyond the id-ordered tie-breaks, which a stable renumbering keeps.
 * The rule, exact:
 *   1. K = every node whose heap offset is not 0, plus the default start node and every per-label start node even when deleted —
 *      the K of vs_index_consolidate_deletes.  D = the rest.
 *   2. new_of[i] = the number of K nodes below i for i in K, VS_INVALID_NODE for i in D: the compaction is stable.
 *   3. Every per-node column keeps exactly the rows of K, in order: codes, neighbor lists, heap tids, vectors, the cosine divisors
 *      (both), the library's own visibility mask and every stored snapshot mask.  A column the index does not hold is skipped
 *      (a plain index has no codes).
 *   4. A neighbor row handles its entries in list order: an entry v becomes new_of[v]; an entry with v in D is removed and the list
 *      closes up, order preserved; the row is padded to its stride with VS_INVALID_NODE.  CONSOLIDATE FIRST: after
 *      vs_index_consolidate_deletes (on a plain index: vs_index_consolidate_deletes_plain) with its repair no K row names a D node, nothing is cut and every list is a pure rename.
 *      Without it the cut is legal but the edges are simply lost — nothing takes over the dropped node's neighbors, rows may end
 *      up empty (rows_emptied) and live rows unreachable.  With VS_COMPACT_KEEP_EDGES_CHECK a first read-only pass counts edges_cut
 *      and the call returns VS_ERR_STATE with every byte as it was when it is not 0.
 *   5. The label CSR keeps the sets of K (built aside, swapped in); the label masks are re-derived; the neighbors' label masks are
 *      dropped as an insert drops them; default_start and the per-label start nodes are mapped through new_of (all of them in K).
 *   6. n = n_after.  The capacity and the allocations STAY: the freed tail is room for the next vs_index_insert (give it back with
 *      vs_index_shrink_to_fit).  What the launch planner remembered of the last batches is dropped; the workspace slab stays.
 *   7. Nothing in D: nothing is written, rows_moved == 0, every array byte-identical.
 * Rows move inside their own arrays through a staging buffer of at most stage_bytes (0 = 256 MiB): every column moves as many rows
 * per chunk as fit; VS_ERR_INVALID if one row of the widest column does not fit.  Rows below the first dropped node are not touched
 * (their neighbor lists are renamed).  out_new_of (host, [n_before], may be NULL) receives the map whenever the call gets as far as
 * computing it.
 * Refusals leave every byte as it was: VS_ERR_STATE for a view handle, live views, a batch in flight, an open vs_pages_out writer,
 * a caller-owned device visibility mask in force, or the edge check above; VS_ERR_INVALID for unknown flags, an index without
 * neighbor lists / heap tids, a stage_bytes below one row.  SBQ and plain storage alike.
 * Open vs_scans, scan pools and brokers of the index must be ENDED before the call (their device state names old ids); a baseline
 * of vs_pages_out taken before stays usable for vs_pages_out_delta — item pointers of the written relation change, so the delta
 * names nearly every node page and the relation shrinks.  Not thread safe against any other call on the index; ordered on the
 * context's stream.
 * NOT ATOMIC.  Every allocation (maps, staging, the new label arrays) happens before the first byte moves, and an error up to
 * there leaves the index as it was.  A HIP error after that point leaves the index UNDEFINED: only vs_index_free is safe. */
#define VS_COMPACT_KEEP_EDGES_CHECK 1u  /* refuse (VS_ERR_STATE, nothing changed) if any kept row names a dropped node */
typedef struct vs_compact_stats {
    uint32_t n_before, n_after;
    uint64_t tombstones;        /* heap offset 0 */
    uint64_t tombstones_kept;   /* of those: default / per-label start nodes */
    uint64_t rows_moved;        /* kept rows whose id changed */
    uint64_t edges_cut;         /* entries of kept rows that named a dropped node */
    uint64_t rows_emptied;      /* kept rows left without a neighbor by the cut */
    uint32_t chunks;            /* staged chunks the row mover ran (the widest column) */
} vs_compact_stats;
int vs_index_compact(vs_index* idx, uint64_t stage_bytes /* 0 = default */, uint32_t flags,
                     uint32_t* out_new_of /* host, [n_before], may be NULL */, vs_compact_stats* out /* may be NULL */);
/* HIP-event milliseconds of the two passes on this index since the last reset, collected while vs_profile_enable is on:
 * ms[0] the keep flags and the two maps, ms[1] the row mover (every column's gathers and staging copies) */
int vs_index_compact_kernel_ms(vs_index* idx, double* ms, int reset);
/* gives the room behind n back to the device: the per-node arrays one at a time at n rows — allocate, copy device to device, swap,
 * free — narrowest row first and the vectors last, so the peak extra memory is one array and the largest one asks when everything
 * else has been returned.  Afterwards capacity == n.  If an allocation fails the call reports VS_ERR_OOM and the index stays fully
 * usable: the arrays already done stay smaller, the others keep their size, and capacity is n all the same (n rows is what every
 * array is known to hold; the next insert that needs room reserves).  Refusals as vs_index_reserve: a view handle, live views, a
 * batch in flight.  The arrays MOVE: pointers taken with vs_index_array must be asked for again, scans ended or rescanned.  A
 * separate call because a caller who expects inserts wants the room kept. */
int vs_index_shrink_to_fit(vs_index* idx);

/* ---- index relation pages -> vs_index_host (the exporter the arrays above come from) ------
 * The reference reaches a node through the buffer manager, one page pin per neighbor (ItemPointer::read_bytes,
 * util/mod.rs:152-155; ReadablePage::get_item_unchecked, util/page.rs:270-283; rkyv::archived_root,
 * pgvectorscale_derive/src/lib.rs:35-40).  Here the blocks of the index relation's main fork are handed over in bulk,
 * in block order (from ReadBufferExtended copies, or straight from the relation's segment files after a CHECKPOINT);
 * every SbqNode item (AM/sbq/node.rs:26-42) is decoded on the host cores into the flat arrays, neighbor ItemPointers
 * become dense node ids (node id = SbqNode items on earlier blocks + offset - 1), and vs_index_upload streams the
 * result to HBM.  Host-only code: these calls work without a device. */
#define VS_BLCKSZ 8192u
enum vs_page_type { /* PageType, util/page.rs:28-39 */
    VS_PAGE_META_V1 = 0, VS_PAGE_NODE = 1, VS_PAGE_PQ_QUANTIZER_DEF = 2, VS_PAGE_PQ_QUANTIZER_VECTOR = 3,
    VS_PAGE_SBQ_MEANS_V1 = 4, VS_PAGE_SBQ_NODE = 5, VS_PAGE_META_V2 = 6, VS_PAGE_SBQ_MEANS = 7, VS_PAGE_META = 8 };

/* Byte offsets of the fields inside the archived root object of an SbqNode item (the last root_size bytes of the
 * item).  rkyv 0.7 archives ClassicSbqNode / LabeledSbqNode as repr(Rust) structs of four 8-byte, 4-aligned fields;
 * vs_node_layout_default() assumes declaration order.  Nothing in the reference pins that order, so a PGRX shim
 * should pass core::mem::offset_of!(ArchivedLabeledSbqNode, ...) values instead. */
typedef struct vs_node_layout {
    uint32_t root_size;                   /* size_of::<ArchivedClassicSbqNode>() = 32                       */
    uint32_t off_heap_item_pointer;       /* ArchivedItemPointer {u32 block_number, u16 offset} (util/mod.rs:17-23) */
    uint32_t off_bq_vector;               /* ArchivedVec<u64>  = {i32 relative offset, u32 len}              */
    uint32_t off_neighbor_index_pointers; /* ArchivedVec<ArchivedItemPointer>                                */
    uint32_t off_labels;                  /* ArchivedLabelSet = ArchivedVec<i16> (LabeledSbqNode); 0xFFFFFFFF otherwise */
} vs_node_layout;
int vs_node_layout_default(int has_labels, vs_node_layout* out);

typedef struct vs_pages_info {
    uint32_t n_blocks;
    uint32_t n_nodes;          /* -> vs_index_desc.n                                                          */
    uint32_t words;            /* bq_vector.len() of every node -> vs_index_desc.words                        */
    uint32_t num_neighbors;    /* neighbor_index_pointers.len() of every node -> vs_index_desc.num_neighbors  */
    uint32_t has_labels;
    uint32_t n_deleted;        /* nodes whose heap_item_pointer.offset == InvalidOffsetNumber                 */
    uint64_t n_label_vals;
    uint32_t pages_by_type[9]; /* indexed by vs_page_type                                                     */
    uint32_t new_pages;        /* all-zero blocks (PageIsNew)                                                 */
    uint32_t meta_magic;       /* MetaPageHeader (block 0, item 1; AM/meta_page.rs:166-174), 0 if block 0 is no meta page */
    uint32_t meta_version;
} vs_pages_info;

typedef struct vs_pages vs_pages; /* reader over the main fork of one diskann index relation */
/* has_labels = MetaPage.has_labels (selects LabeledSbqNode); layout NULL = vs_node_layout_default; threads 0 = all cores (<= 32) */
int vs_pages_open(uint32_t page_size, int has_labels, const vs_node_layout* layout, uint32_t threads, vs_pages** out);
/* `plain` storage (PageType::Node pages of PlainNode items, AM/plain/node.rs:15-22): the same reader, with vs_pages_info.words =
 * the dimensions of PlainNode.vector and vs_index_host.vecs = those vectors (the cosine-normalised index slice the graph
 * distances are computed on, AM/plain/storage.rs:239-247) instead of codes; no labels (AM/plain/storage.rs:262).  layout NULL =
 * vs_plain_layout_default (off_bq_vector names the vector field, off_labels is unused). */
int vs_plain_layout_default(vs_node_layout* out);
int vs_pages_open_plain(uint32_t page_size, const vs_node_layout* layout, uint32_t threads, vs_pages** out);
/* append blocks first_block .. first_block+n_blocks-1 (must continue where the previous call stopped; the bytes are
 * not referenced after the call returns).  A failing call leaves the reader unchanged. */
int vs_pages_add(vs_pages* p, uint32_t first_block, const void* pages, uint32_t n_blocks);
/* translate neighbor ItemPointers to node ids, check the MetaPageHeader magic; info may be NULL */
int vs_pages_finish(vs_pages* p, vs_pages_info* info);
/* borrowed pointers (valid until vs_pages_close): codes, nbrs, nbr_stride, heap_tids, label_off, label_val; the
 * caller fills vecs (heap column), mean / m2 / count (vs_pages_sbq_means) and the start-node arrays, then calls
 * vs_index_upload */
int vs_pages_host(const vs_pages* p, vs_index_host* host);
/* IndexPointer <-> node id (start nodes of the MetaPage, AM/graph/start_nodes.rs:17-22) */
int vs_pages_node_of(const vs_pages* p, uint32_t block, uint32_t offset, uint32_t* node);
int vs_pages_item_pointer_of(const vs_pages* p, uint32_t node, uint32_t* block, uint32_t* offset);
/* ChainItemIterator (util/chain.rs:159-185): concatenated payload of the chain that starts at (block, offset);
 * page_type VS_PAGE_SBQ_MEANS or VS_PAGE_META; buf may be NULL to query *len */
int vs_pages_read_chain(const vs_pages* p, uint32_t block, uint32_t offset, int page_type, void* buf, size_t cap, size_t* len);
/* SbqMeans::load (AM/sbq/mod.rs:85-121) at MetaPage.quantizer_metadata: chained SbqMeans or single-item SbqMeansV1 */
int vs_pages_sbq_means(const vs_pages* p, uint32_t block, uint32_t offset, float* mean, float* m2, uint32_t dim_cap,
                       uint32_t* dim, uint64_t* count);
void vs_pages_close(vs_pages* p);
/* keep only the block table (page type / item count per block) and the metadata pages: node items are decoded elsewhere */
int vs_pages_headers_only(vs_pages* p);
int vs_pages_block_table(const vs_pages* p, const uint32_t** blk_base, const uint32_t** blk_cnt, uint32_t* n_blocks);

/* ---- the MetaPage body (AM/meta_page.rs:176-210): item 2 of block 0, a chained rkyv archive (store / load, :344-378) ----
 * Byte offsets of the fields inside ArchivedMetaPage (the last root_size bytes of the chain's payload).  rkyv 0.7 archives are
 * repr(Rust): vs_meta_layout_default() lays the fields out in declaration order with C alignment; a PGRX shim passes
 * core::mem::offset_of!(ArchivedMetaPage, ...) instead (oracle/ref_kat.rs prints them).  The archived forms
 * restated from rkyv 0.7.43: ArchivedString = 8 bytes (<= 7 bytes inline, else {u32 len, i32 offset}); ArchivedOption =
 * {u8 tag, T at T's alignment}; ArchivedStartNodes = {ArchivedItemPointer default_node, ArchivedBTreeMap<i16, ItemPointer>
 * {u32 len, i32 root}} with B-tree nodes {u16 meta (bit 15: inner), u32 size, i32 ptr} + LeafNodeEntry {i16 key, ItemPointer}
 * / InnerNodeEntry {i32 ptr, i16 key}; relative pointers count from the position of the pointer itself. */
typedef struct vs_meta_layout {
    uint32_t root_size;                    /* size_of::<ArchivedMetaPage>() = 80 */
    uint32_t off_magic_number, off_version, off_extension_version_when_built, off_distance_type, off_num_dimensions,
        off_num_dimensions_to_index, off_bq_num_bits_per_dimension, off_storage_type, off_num_neighbors, off_search_list_size,
        off_max_alpha, off_start_nodes, off_quantizer_metadata, off_has_labels;
} vs_meta_layout;
int vs_meta_layout_default(vs_meta_layout* out);
typedef struct vs_meta_page {
    uint32_t magic_number, version;
    char extension_version_when_built[64];  /* NUL terminated (longer strings are cut)                                     */
    uint32_t distance_type;                 /* DistanceType as stored (u16): 0 cosine, 1 l2, 2 inner product                 */
    uint32_t num_dimensions, num_dimensions_to_index, bq_num_bits_per_dimension;
    uint32_t storage_type;                  /* StorageType as stored (u8): 0 plain, 1 (retired), 2 SbqCompression           */
    uint32_t num_neighbors, search_list_size;
    double max_alpha;
    uint32_t has_start_nodes;               /* Option<StartNodes> is Some                                                    */
    uint32_t default_start_block, default_start_offset;   /* StartNodes.default_node                                        */
    uint32_t n_labeled_start_nodes;         /* StartNodes.labeled_nodes.len()                                                */
    uint32_t quantizer_block, quantizer_offset;            /* quantizer_metadata (SbqMeans chain; vs_pages_sbq_means)        */
    uint32_t has_labels;
} vs_meta_page;
/* rkyv::from_bytes::<MetaPage> over `bytes` (the chain payload).  The labeled start nodes come out in key order:
 * start_labels / start_blocks / start_offsets hold `cap` entries each (any may be NULL); more entries than cap is an error
 * unless all three are NULL (query n_labeled_start_nodes first).  layout NULL = vs_meta_layout_default.  Host-only. */
int vs_meta_page_decode(const void* bytes, size_t len, const vs_meta_layout* layout, vs_meta_page* out, int16_t* start_labels,
                        uint32_t* start_blocks, uint32_t* start_offsets, uint32_t cap);
/* MetaPage::fetch for a reader (after vs_pages_finish): reads the chain at (0, 2), decodes it and fills the geometry of
 * `desc` (n from the pages, distance / dims / bits / words / R / storage / has_labels from the MetaPage, default_start and the
 * labeled start nodes translated to node ids; an index without rows has default_start = VS_INVALID_NODE).  start_labels /
 * start_nodes: cap entries (may be NULL to query desc->n_label_starts).  meta may be NULL.  Only PageType::Meta (version 3)
 * relations: MetaV1 / MetaV2 pages are what the reference itself rewrites on first use. */
int vs_pages_meta(const vs_pages* p, const vs_meta_layout* layout, vs_meta_page* meta, vs_index_desc* desc, int16_t* start_labels,
                  uint32_t* start_nodes, uint32_t cap);

/* ---- the heap's vector column (vs_heap.cpp; host-only) ----------------------------------------------------------------------
 * vs_index_host.vecs — what the rescore window reads through table_index_fetch_tuple + slot_getattr + pg_detoast_datum_copy per
 * candidate (UT/table_slot.rs:19-42, AM/pg_vector.rs:125-135, AM/sbq/storage.rs:304-328) — is staged once, in bulk, from the
 * pages of the table the index points into: the heap's main fork streams past in block order (vs_heap_add), then its TOAST
 * relation's (vs_heap_toast_add; a 768-dimensional vector is 3 KB and lives there, chunked).  For every index node the tuple
 * its heap TID names is deformed up to the vector attribute exactly as heap_deform_tuple does (null bitmap, alignment padding,
 * 1-byte / 4-byte / external / pglz-compressed varlena forms; LP_REDIRECT line pointers are followed) and the float4s land in
 * row `node` of out_vecs.  Visibility is not decided here (vs_index_set_visibility). */
typedef struct vs_heap_attr {  /* pg_attribute.attlen / attalign of one column of the table, in attnum order */
    int16_t attlen;   /* > 0 fixed length, -1 varlena, -2 cstring */
    char attalign;    /* 'c' 1, 's' 2, 'i' 4, 'd' 8 */
} vs_heap_attr;
typedef struct vs_heap_info {
    uint32_t n_nodes, heap_blocks, toast_blocks;
    uint32_t n_inline;            /* vectors found inside their heap tuple                                            */
    uint32_t n_external;          /* vectors assembled from TOAST chunks                                              */
    uint32_t n_deleted;           /* index tuples with an invalid heap offset (vacuumed): no row, left zero           */
    uint32_t n_null;              /* the row exists, its vector column is NULL                                        */
    uint32_t n_dead_line_pointer; /* the TID names an unused / dead line pointer                                      */
    uint32_t n_not_found;         /* the TID lies beyond the blocks that were added                                   */
    uint32_t n_toast_incomplete;  /* an external vector whose chunks did not all arrive                               */
    uint64_t n_chunks;            /* TOAST chunk rows consumed                                                        */
} vs_heap_info;
typedef struct vs_heap vs_heap;
/* attrs / natts: the table's tuple descriptor; vector_attno: the indexed column (1-based attnum, IndexInfo.ii_IndexAttrNumbers);
 * heap_tids [n]: ArchivedSbqNode.heap_item_pointer of every node, (block << 16) | offset, as vs_pages_host returns them;
 * out_vecs [n][out_stride] floats (out_stride >= dim), zeroed here, filled by the calls below; kept by the caller. */
int vs_heap_open(uint32_t page_size, const vs_heap_attr* attrs, uint32_t natts, uint32_t vector_attno, uint32_t dim,
                 const uint64_t* heap_tids, uint32_t n, float* out_vecs, uint32_t out_stride, vs_heap** out);
int vs_heap_add(vs_heap* h, uint32_t first_block, const void* pages, uint32_t n_blocks);        /* heap main fork, in block order */
int vs_heap_toast_add(vs_heap* h, uint32_t first_block, const void* pages, uint32_t n_blocks);  /* then the TOAST relation's       */
/* found [n] (may be NULL): 1 where the node's vector was read.  Everything else is counted in info. */
int vs_heap_finish(vs_heap* h, vs_heap_info* info, uint8_t* found);
void vs_heap_close(vs_heap* h);

/* ---- the same column decoded ON the device (vs_heap_dev.h, part of vs_pages_dev.hip) -----------------------------------------------
 * The host copies pages and does nothing else: they go through the context's pinned ring to HBM as they are, chunk by chunk (two
 * staged chunks, never retained), and kernels deform the tuples and scatter the floats straight into device rows — a buffer from
 * vs_dev_alloc, or the index's own column (vs_index_alloc_vecs, vs_index_array(VS_ARR_VECS) plus a row offset).  No host copy of
 * the column exists at any time: host memory is O(1) in n beyond heap_tids, device memory a few tens of bytes per node.
 * The semantics are those of vs_heap_* above (vs_heap.cpp is the specification: line pointers with LP_REDIRECT followed for at most
 * 8 hops, heap_deform_tuple up to the vector attribute, in-line vectors under 1-byte and 4-byte headers, external ones assembled
 * from their TOAST chunks with every check the host makes), with these differences:
 *   - block ranges need not be contiguous: first_block must be >= the end of the previous call of the same pass (else
 *     VS_ERR_INVALID), gaps are allowed.  A tid on a block that was never fed is n_not_found, a referenced value whose chunks were
 *     never fed is n_toast_incomplete; heap_blocks / toast_blocks report the end of the last range fed.  A follower reads only the
 *     blocks its new rows live on.
 *   - compressed vectors (pglz or lz4; in line, VARATT_IS_4B_C, or external with extsize < rawsize) are NOT decoded: the row stays
 *     zero with found = 0 and is counted in *n_compressed and in no field of vs_heap_info; its TOAST chunks are skipped and not
 *     counted in n_chunks.  The caller reads those rows with vs_heap_* over heap_tids[found == 0] and uploads them.  (pgvector's own
 *     storage is `external`, which never compresses.)  n_inline + n_external + n_deleted + n_null + n_dead_line_pointer +
 *     n_not_found + n_toast_incomplete + n_compressed == n.
 *   - a malformed page, item or tuple is VS_ERR_INVALID with the relation (heap / TOAST), the block, the offset and the reason in
 *     vs_last_error; it may be returned by the add that fed the page, by a later add, or by the finish at the latest (the copy of
 *     chunk i+1 runs under the kernel of chunk i).  When several items are malformed, which one is named is unspecified.  After an
 *     error only vs_heap_dev_close is defined.  A malformed page never makes a kernel read or write outside its buffers.
 * Open: the argument checks of vs_heap_open; the first dim floats of every target row are zeroed, the padding floats
 * [dim, out_stride) are never written.  Finish: info and found[] as vs_heap_finish fills them; EVERY row that is not found is zero,
 * a value whose chunks did not all arrive included.  No output depends on the order in which waves or pages are scheduled.
 * heap_tids: HOST [n], (block << 16) | offset; d_out_vecs: DEVICE [n][out_stride] floats, out_stride >= dim. */
typedef struct vs_heap_dev vs_heap_dev;
int vs_heap_dev_open(vs_ctx* ctx, uint32_t page_size, const vs_heap_attr* attrs, uint32_t natts, uint32_t vector_attno, uint32_t dim,
                     const uint64_t* heap_tids, uint32_t n, float* d_out_vecs, uint32_t out_stride, vs_heap_dev** out);
int vs_heap_dev_add(vs_heap_dev* h, uint32_t first_block, const void* pages, uint32_t n_blocks);        /* heap main fork  */
int vs_heap_dev_toast_add(vs_heap_dev* h, uint32_t first_block, const void* pages, uint32_t n_blocks);  /* then TOAST      */
int vs_heap_dev_finish(vs_heap_dev* h, vs_heap_info* info, uint8_t* found /* host [n], may be NULL */, uint32_t* n_compressed /* may be NULL */);
void vs_heap_dev_close(vs_heap_dev* h);

/* ---- heap visibility decided ON the device from resident heap pages (vs_heap_vis.h, part of vs_pages_dev.hip) ------------------------
 * The one byte per node of vs_index_set_visibility / vs_index_snapshot_put is what table_index_fetch_tuple would say for the node's
 * heap tid under the scan's snapshot.  Visibility needs only the heap's MAIN fork (line pointers and 23-byte tuple headers; the
 * vectors live in TOAST), the snapshot and the commit log.  vs_heap_res keeps that fork in HBM, indexed by block number: the shim
 * puts the whole fork once and afterwards only the blocks that changed; a snapshot's mask is then one kernel pass (k_heap_vis, a
 * lane per node) over memory that is already there, and nothing crosses PCIe but the snapshot.
 *
 * vs_heap_res_put: host pages, any order, through the context's pinned ring; a later put of a block overwrites it; a put beyond the
 * capacity grows the buffer by the rule of vs_index_reserve (by half, at least to fit, device to device; a growth that fails leaves
 * the buffer as it was); a block never put is all zero, which reads as PageIsNew: no items.  vs_heap_res_blocks: one past the
 * highest block ever put.  Argument checks are those of vs_heap_dev_open / _add and come before any device call.
 *
 * THE RULE (PostgreSQL 13-17; little endian).  Tuple header: t_xmin at 0, t_xmax at 4, t_cid at 8, the offset number of t_ctid at
 * 16..17, t_infomask2 at 18 (HOT_UPDATED 0x4000, ONLY_TUPLE 0x8000), t_infomask at 20: XMIN_COMMITTED 0x0100, XMIN_INVALID 0x0200
 * (both = frozen), XMAX_COMMITTED 0x0400, XMAX_INVALID 0x0800, XMAX_IS_MULTI 0x1000, XMAX_LOCK_ONLY 0x0080, EXCL_LOCK 0x0040,
 * KEYSHR_LOCK 0x0010, COMBOCID 0x0020, MOVED_OFF 0x4000, MOVED_IN 0x8000.
 *   normal(x)       = x >= 3
 *   precedes(a,b)   = normal(a) && normal(b) ? (int32)(a-b) < 0  : a < b          (TransactionIdPrecedes)
 *   follows_eq(a,b) = normal(a) && normal(b) ? (int32)(a-b) >= 0 : a >= b         (TransactionIdFollowsOrEquals)
 *   locked_only(m)  = (m & LOCK_ONLY) || (m & (IS_MULTI|EXCL_LOCK|KEYSHR_LOCK)) == EXCL_LOCK   (HEAP_XMAX_IS_LOCKED_ONLY)
 *   did_commit(x)   = x==1||x==2 -> yes; x==0 -> no; outside the window -> UNDECIDED(CLOG_RANGE); status 3 -> UNDECIDED(SUBCOMMITTED);
 *                     status==1                                                   (TransactionIdDidCommit)
 *   in_snapshot(x)  = precedes(x,xmin) -> no; follows_eq(x,xmax) -> yes;          (XidInMVCCSnapshot)
 *                     not recovery: !suboverflowed: x in subxip -> yes, else x in xip
 *                                    suboverflowed: x in xip -> yes, else UNDECIDED(SUBOVERFLOW)
 *                     recovery:     x in subxip -> yes; else suboverflowed ? UNDECIDED(SUBOVERFLOW) : no
 *   own(x)          = x in own_xids                                               (TransactionIdIsCurrentTransactionId)
 *   HeapTupleSatisfiesMVCC(t):
 *     if !(m & XMIN_COMMITTED):
 *         if (m & 0x0300) == XMIN_INVALID: invisible
 *         if m & (MOVED_OFF|MOVED_IN): UNDECIDED(MOVED)
 *         if own(xmin):
 *             if m & COMBOCID: UNDECIDED(COMBOCID)
 *             if cid >= curcid: invisible
 *             if m & XMAX_INVALID: visible;  if locked_only(m): visible
 *             if m & IS_MULTI: UNDECIDED(MULTIXACT)
 *             if !own(xmax): visible
 *             return cid >= curcid ? visible : invisible
 *         else if in_snapshot(xmin): invisible
 *         else if !did_commit(xmin): invisible
 *     else if (m & 0x0300) != 0x0300 && in_snapshot(xmin): invisible
 *     if m & XMAX_INVALID: visible;  if locked_only(m): visible
 *     if m & IS_MULTI: UNDECIDED(MULTIXACT)
 *     if !(m & XMAX_COMMITTED):
 *         if own(xmax): (COMBOCID -> UNDECIDED) return cid >= curcid ? visible : invisible
 *         if in_snapshot(xmax): visible
 *         if !did_commit(xmax): visible
 *     else if in_snapshot(xmax): visible
 *     invisible
 *   heap_hot_search_buffer(tid):      (what table_index_fetch_tuple runs; all within the tid's page)
 *     off = tid.offset; at_start = true; prev_xmax = 0
 *     loop (at most as many rounds as the page has line pointers; more is a cycle -> VS_ERR_INVALID):
 *         off outside 1..nitems -> invisible
 *         lp not NORMAL: if REDIRECT && at_start { off = lp_off; at_start = false; continue } else invisible
 *         if at_start && (m2 & ONLY_TUPLE): invisible
 *         if prev_xmax != 0 && prev_xmax != (frozen ? 2 : xmin): invisible
 *         r = HeapTupleSatisfiesMVCC(t):  visible -> visible;  UNDECIDED -> UNDECIDED
 *         if (m2 & HOT_UPDATED) && !(m & XMAX_INVALID) && (m & 0x0300) != XMIN_INVALID:
 *             if (m & IS_MULTI) && !locked_only(m): UNDECIDED(MULTIXACT)
 *             off = ctid.offset; at_start = false; prev_xmax = xmax
 *         else invisible
 * An undecided inner answer makes the whole verdict undecided with that reason.  Hint bits are never written: the pages are
 * read-only copies and the verdict does not depend on them.
 *
 * A node's byte is 1 (visible) or 0 (invisible).  An UNDECIDED node — multixact members, pg_subtrans, combo command ids and the
 * MOVED bits are not evaluated; an xid may lie outside the pg_xact window — gets 1, the conservative value, is counted by reason and
 * appears in undecided_nodes, ascending (the first `cap` of them; *n_undecided is their full number): the shim settles those few
 * with index_fetch_tuple and vs_index_snapshot_patch.  Parts of n_invisible: a tid with offset 0 (a vacuumed index tuple) is
 * n_deleted; a block at or beyond vs_heap_res_blocks, or an offset beyond the page's line pointers, is n_not_found; a first line
 * pointer that is LP_UNUSED / LP_DEAD is n_dead_line_pointer.  n_visible + n_invisible + n_undecided == n.  chain_hops: tuple headers
 * read beyond the first of each node.  No output depends on how the lanes are scheduled.
 * A malformed page — a wrong pd_pagesize_version, an inconsistent page header, an LP_NORMAL item outside pd_upper..pd_special or
 * shorter than 23 bytes, a HOT chain that cycles — is VS_ERR_INVALID naming the block, the offset and the reason (when several are
 * malformed, which one is unspecified); d_visible is then unspecified.  A malformed page never makes the kernel read outside the
 * resident buffer.  The kernel runs on the context's stream; the call synchronises to hand back the counters and the list.
 * d_heap_tids: DEVICE [n] (vs_index_array(VS_ARR_TIDS)); d_visible: DEVICE [n]; xip / subxip / own_xids: HOST, unsorted as
 * PostgreSQL keeps them (the library sorts copies). */
typedef struct vs_heap_res vs_heap_res;
int vs_heap_res_open(vs_ctx* ctx, uint32_t page_size, uint32_t n_blocks_capacity, vs_heap_res** out);
int vs_heap_res_put(vs_heap_res* h, uint32_t first_block, const void* pages, uint32_t n_blocks); /* host pages, any order */
uint32_t vs_heap_res_blocks(const vs_heap_res* h);                                              /* one past the highest block ever put */
void vs_heap_res_close(vs_heap_res* h);

typedef struct vs_mvcc_snapshot { /* SnapshotData of an MVCC snapshot, plus what the backend knows about itself */
    uint32_t xmin, xmax;
    const uint32_t* xip; /* unsorted, as PostgreSQL keeps it */
    uint32_t xcnt;
    const uint32_t* subxip;
    uint32_t subxcnt;
    int32_t suboverflowed, taken_during_recovery;
    const uint32_t* own_xids; /* every xid TransactionIdIsCurrentTransactionId says yes to */
    uint32_t n_own;
    uint32_t curcid;
} vs_mvcc_snapshot;
typedef struct vs_xact_status { /* a window of pg_xact: 2 bits per xid, 4 xids per byte, xid % 4 lowest first */
    uint32_t first_xid;         /* multiple of 4 */
    uint32_t n_xids;            /* the window is (xid - first_xid) mod 2^32 < n_xids */
    const uint8_t* bits;        /* 0 in progress, 1 committed, 2 aborted, 3 sub-committed */
} vs_xact_status;
enum { VS_VIS_R_MULTIXACT, VS_VIS_R_SUBCOMMITTED, VS_VIS_R_CLOG_RANGE, VS_VIS_R_COMBOCID, VS_VIS_R_MOVED, VS_VIS_R_SUBOVERFLOW, VS_VIS_R_N };
typedef struct vs_vis_stats {
    uint64_t n_visible, n_invisible, n_undecided;
    uint64_t n_deleted, n_not_found, n_dead_line_pointer; /* parts of n_invisible, classified as vs_heap_info classifies them */
    uint64_t chain_hops;                                  /* members looked at beyond the first, summed */
    uint64_t undecided_by_reason[VS_VIS_R_N];
} vs_vis_stats;
int vs_heap_res_visibility(vs_heap_res* h, const uint64_t* d_heap_tids, uint32_t n, const vs_mvcc_snapshot* snapshot,
                           const vs_xact_status* xact, uint8_t* d_visible /* device [n] */, vs_vis_stats* out /* may be NULL */,
                           uint32_t* undecided_nodes /* host, may be NULL */, uint32_t cap, uint32_t* n_undecided /* may be NULL */);
/* The same over the index's own heap tid column, written straight into the library-owned mask of snapshot id 1 ..
 * VS_MAX_SNAPSHOTS - 1 (allocated as vs_index_snapshot_put allocates it, at capacity: rows inserted later read 0 in it).
 * vs_index_snapshot_put_dev: vs_index_snapshot_put with the n bytes already in device memory (copied; the buffer stays the
 * caller's).  vs_index_snapshot_patch: mask[nodes[i]] = values[i] != 0 for host arrays of n entries (the last entry of a node
 * wins) — how the shim settles the undecided few after index_fetch_tuple.  Refusals are those of vs_index_snapshot_put, plus
 * VS_ERR_STATE while a batch of the handle is in flight and, for _patch, when the id has no mask or a node is >= n; a refused call
 * changes nothing.  An evaluation that ends in VS_ERR_INVALID (a malformed page) drops the mask of that id.  With a broker attached
 * only its dispatcher may call these (vs_broker_call). */
int vs_index_snapshot_eval(vs_index* idx, vs_heap_res* h, uint32_t snapshot, const vs_mvcc_snapshot* snap, const vs_xact_status* xact,
                           vs_vis_stats* out, uint32_t* undecided_nodes, uint32_t cap, uint32_t* n_undecided);
int vs_index_snapshot_put_dev(vs_index* idx, uint32_t snapshot, const uint8_t* d_visible);
int vs_index_snapshot_patch(vs_index* idx, uint32_t snapshot, const uint32_t* nodes, const uint8_t* values, uint32_t n);

/* ---- Scans of different snapshots in one launch: a base of classes and per-snapshot overlays --------------------------------------
 * A mask is one byte per node and one pass of the rule per snapshot, and a launch runs under one mask: with writers about, every
 * READ COMMITTED statement has a snapshot of its own and would get a launch of its own.  But almost every tuple is visible, or
 * invisible, to every snapshot that can exist; only rows touched at or after the oldest-running horizon depend on who asks.
 *
 * THE CLASS RULE (next to THE RULE above, whose functions it uses unchanged).  vs_index_vis_base_eval walks
 * heap_hot_search_buffer(tid) for every node under the synthetic snapshot S_H: xmin = xmax = horizon, xip / subxip / own_xids empty,
 * not suboverflowed, not taken during recovery.  It remembers whether any normal xid x (x >= 3) that the walk hands to own(),
 * in_snapshot() or did_commit() has follows_eq(x, horizon) — "recent".  The node's class byte is
 *     0  invisible to all: the verdict is invisible and nothing recent was consulted (includes offset 0, not found, a dead or unused
 *        first line pointer)
 *     1  visible to all:   the verdict is visible and nothing recent was consulted
 *     2  depends:          something recent was consulted, or the verdict is UNDECIDED for any reason
 * Soundness: under any snapshot with xmin >= horizon and every own xid >= horizon, a consulted x < horizon gives own(x) = no,
 * in_snapshot(x) = no (precedes(x, xmin) decides first in every mode) and did_commit(x) a settled fact, and command ids are compared
 * only under own(): the verdict of a class-0 / class-1 node does not depend on the snapshot.
 * PRECONDITION (the caller's): horizon <= the oldest xid still running — what RecentXmin / GetOldestNonRemovableTransactionId give
 * the shim.  The class-2 nodes are also kept as the ascending "depends list" of r entries (vs_index_vis_base_info reads it back);
 * nothing about it depends on how the lanes are scheduled, and xids compare modulo 2^32 as in THE RULE.
 * changed_blocks != NULL (ascending, distinct heap block numbers; n_changed may be 0) refreshes a base that exists: only nodes whose
 * tid lies on a listed block are walked again, every other node keeps its class — with a later horizon that is conservative, never
 * wrong — the list is rebuilt from the classes and the horizon passed is stored.  changed_blocks == NULL walks every node.
 * Stats: n_class[] and r count the whole index after the call; the other fields count the nodes this call walked (n_walked):
 * the parts of the invisible verdicts as vs_vis_stats names them, n_recent (class 2 with a decided verdict), n_undecided and its
 * reasons (class 2 whatever was consulted), chain_hops.
 * LIFETIME: every base evaluation, full or refresh, drops every overlay (overlays index list positions).  Rows inserted later read
 * class 0 until the next evaluation that walks them, as in stored masks.  vs_index_compact drops the base and the overlays;
 * vs_index_vis_base_drop frees them.  A malformed page is reported as by vs_index_snapshot_eval and the base is dropped.
 *
 * OVERLAYS.  vs_index_vis_slot_eval gathers the tids of the depends list and runs THE RULE under `snap` over those r nodes only;
 * the result is the slot's overlay, r bytes (1 visible, 0 invisible; UNDECIDED gets 1, is counted in *out and listed ascending as
 * NODE ids exactly as vs_index_snapshot_eval lists them; *out counts the r nodes).  Slots are 1 .. VS_MAX_VIS_SLOTS - 1; slot 0 means
 * every tuple visible and holds no overlay.  vs_index_vis_slot_patch settles nodes of the depends list (overlay[pos(node)] =
 * values[i] != 0, the last entry of a node wins); a node that is not on the list is VS_ERR_INVALID.  vs_index_vis_slot_drop drops
 * one overlay.  vs_index_vis_materialize writes the byte mask of legacy snapshot id 1 .. VS_MAX_SNAPSHOTS - 1 from the base and the
 * slot's overlay: the bridge for what still runs under a legacy id (cursors, scan pools, vs_scan_set_snapshot, the shm server).
 * Refusals, each changing nothing: a snapshot whose xmin or any own xid precedes the stored horizon (VS_ERR_INVALID naming the xid);
 * no base, or for _patch / _materialize no overlay (VS_ERR_STATE); a batch of the handle in flight (VS_ERR_STATE); a view handle
 * (VS_ERR_STATE); the argument checks of vs_index_snapshot_eval.  With a broker attached only its dispatcher may call these
 * (vs_broker_call).  vs_index_vis_share: a view takes the base and overlays of its source over, as vs_index_snapshot_share hands
 * over the masks. */
#define VS_MAX_VIS_SLOTS 1024
typedef struct vs_vis_base_stats {
    uint64_t n_class[3];                                  /* nodes of class 0 / 1 / 2 in the whole index after the call */
    uint64_t r;                                           /* entries of the depends list == n_class[2] */
    uint64_t n_walked;                                    /* nodes this call walked: all, or those on the changed blocks */
    uint64_t n_deleted, n_not_found, n_dead_line_pointer; /* of the walked: parts of the invisible verdicts, as in vs_vis_stats */
    uint64_t n_recent;                                    /* of the walked: decided, but a consulted xid is at or after the horizon */
    uint64_t n_undecided;                                 /* of the walked: UNDECIDED verdicts */
    uint64_t undecided_by_reason[VS_VIS_R_N];
    uint64_t chain_hops;
} vs_vis_base_stats;
int vs_index_vis_base_eval(vs_index* idx, vs_heap_res* h, uint32_t horizon_xid, const vs_xact_status* xact,
                           const uint32_t* changed_blocks /* host, NULL: every node */, uint32_t n_changed, vs_vis_base_stats* out /* may be NULL */);
int vs_index_vis_base_drop(vs_index* idx);
/* the stored horizon, r and the first `cap` nodes of the depends list (each output may be NULL); VS_ERR_STATE without a base */
int vs_index_vis_base_info(const vs_index* idx, uint32_t* horizon_xid, uint32_t* r, uint32_t* depends_nodes /* host */, uint32_t cap);
int vs_index_vis_slot_eval(vs_index* idx, vs_heap_res* h, uint32_t slot, const vs_mvcc_snapshot* snap, const vs_xact_status* xact,
                           vs_vis_stats* out, uint32_t* undecided_nodes, uint32_t cap, uint32_t* n_undecided);
int vs_index_vis_slot_patch(vs_index* idx, uint32_t slot, const uint32_t* nodes, const uint8_t* values, uint32_t n);
int vs_index_vis_slot_drop(vs_index* idx, uint32_t slot);
int vs_index_vis_materialize(vs_index* idx, uint32_t slot, uint32_t snapshot);
int vs_index_vis_share(vs_index* view, const vs_index* src);
/* vs_search_batch / vs_search_batch_dev with a slot per scan: scan_slots[q] (HOST for _vis, DEVICE for _dev_vis, where it must stay
 * valid until the finish) names the overlay scan q runs under.  rescore == 0: the heap is not looked at and the slots do not matter.
 * Slot 0: every tuple visible.  Otherwise node v is hidden iff class[v] == 0, or class[v] == 2 and the slot's overlay says 0; a
 * hidden row is fetched, counted and dropped before the rescore window exactly as under a mask.  The index's mask in force
 * (vs_index_set_visibility*, vs_index_snapshot_use) is not consulted by these calls.  A slot >= VS_MAX_VIS_SLOTS is VS_ERR_INVALID
 * and a slot without an overlay VS_ERR_STATE, before anything is launched (the device slots are read back once for that).  A batch
 * whose slots are all 0 launches what a batch without any mask launches.  Follow-up, not built yet: slots in the shm server's
 * request layout, in scan pools and in cursors — those run under a materialized legacy id. */
int vs_search_batch_vis(vs_index* idx, const float* queries, const int16_t* qlabels, const uint32_t* qlabel_off, const uint32_t* scan_slots,
                        uint32_t nq, uint32_t search_list_size, uint32_t rescore, uint32_t k, uint32_t* out_ids, uint64_t* out_tids,
                        float* out_dist, vs_stats* stats);
int vs_search_batch_dev_vis(vs_index* idx, const float* d_queries, const int16_t* d_qlabels, const uint32_t* d_qlabel_off,
                            const uint32_t* d_scan_slots, uint32_t nq, uint32_t search_list_size, uint32_t rescore, uint32_t k,
                            uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist);
int vs_search_batch_dev_vis_finish(vs_index* idx, vs_stats* stats);

/* The same, decoded ON the device (vs_pages_dev.hip): the blocks are copied to HBM as they are (pinned ring,
 * hipMemcpyAsync), the host only reads the page headers on the way past, and one kernel (a wave per node page) walks the
 * line pointers and rkyv relative pointers and writes codes / neighbor ids / heap tids into the index arrays; label sets
 * (desc->has_labels, LabeledSbqNode) take a count pass and a copy pass over the same staged pages.  memory_optimized
 * indexes.  layout NULL = the default layout for desc->has_labels.  n_blocks_total = RelationGetNumberOfBlocks (the raw pages stay in HBM until the build). */
typedef struct vs_pages_dev vs_pages_dev;
int vs_pages_dev_open(vs_ctx* ctx, uint32_t page_size, const vs_node_layout* layout, uint32_t n_blocks_total, vs_pages_dev** out);
int vs_pages_dev_add(vs_pages_dev* d, uint32_t first_block, const void* pages, uint32_t n_blocks); /* in block order */
int vs_pages_dev_node_of(const vs_pages_dev* d, uint32_t block, uint32_t offset, uint32_t* node);
int vs_pages_dev_sbq_means(const vs_pages_dev* d, uint32_t block, uint32_t offset, float* mean, float* m2, uint32_t dim_cap,
                           uint32_t* dim, uint64_t* count);
/* MetaPage::fetch on the metadata pages the host kept (after the last vs_pages_dev_add): as vs_pages_meta */
int vs_pages_dev_meta(vs_pages_dev* d, const vs_meta_layout* layout, vs_meta_page* meta, vs_index_desc* desc, int16_t* start_labels,
                      uint32_t* start_nodes, uint32_t cap);
/* desc: the MetaPage fields (vs_pages_dev_meta, or by hand: n is taken from the pages, default_start is a node id from vs_pages_dev_node_of);
 * extras: vecs / mean / m2 / count / label_start_labels / label_start_nodes (node ids); frees the raw pages */
int vs_pages_dev_build(vs_pages_dev* d, const vs_index_desc* desc, const vs_index_host* extras, vs_pages_info* info, vs_index** out);
void vs_pages_dev_close(vs_pages_dev* d);
/* the block table the host read off the page headers, as vs_pages_block_table (borrowed pointers, valid until vs_pages_dev_close:
 * the table outlives vs_pages_dev_build) */
int vs_pages_dev_block_table(const vs_pages_dev* d, const uint32_t** blk_base, const uint32_t** blk_cnt, uint32_t* n_blocks);

/* ---- following a relation that something else writes (vs_pages_dev.hip): a streaming-replication standby (WAL replay changes
 * page images and nothing else), a primary where the CPU extension keeps aminsert and vacuum, any restart.  A follower knows the
 * block table of the relation its index was staged from; it takes an ascending list of the blocks that changed, with their
 * bytes as they are now, checks them on the device without touching the index (stage) and then scatters them into the resident
 * arrays (apply).  That works because the reference only appends nodes at the end of the relation (Tape), patches neighbor
 * lists in place at unchanged item size and clears heap offsets in place: node ids (SbqNode items on earlier blocks + offset - 1)
 * are stable.  The rule, checked on the page headers: a listed block's item count may not shrink; it may grow only on a block
 * behind which no block held nodes in the old table; every block in [n_blocks_before, n_blocks_total) must be listed (all-zero
 * and non-node pages count 0 items); n_blocks_total < n_blocks_before is refused.  vs_pages_follow_open: memory_optimized (SBQ)
 * indexes, classic and labeled nodes; it refuses a plain index (VS_ERR_INVALID), which vs_pages_follow_open_plain follows.
 * NOT read from the pages: the start nodes and the quantizer.  Block 0 is not interpreted — the caller decodes the MetaPage
 * (vs_meta_page_decode) and calls vs_index_set_start_nodes / vs_index_set_quantizer after the apply, as it does at staging. */
typedef struct vs_pages_follow vs_pages_follow;
typedef struct vs_pages_follow_info {
    uint32_t n_blocks_before, n_blocks_now, pages_listed, node_pages_listed;
    uint32_t n_before, n_appended;
    uint32_t rows_relinked;   /* existing nodes whose neighbour row differs from the resident one */
    uint32_t tids_cleared;    /* existing nodes whose heap offset went from != 0 to 0 */
    uint32_t tids_changed;    /* any other change of an existing heap tid */
    uint32_t codes_changed;   /* existing nodes whose code row differs (the reference never does this; reported, applied); on a plain
                               * follower: whose PlainNode.vector differs from the writer's composition (reported, NOT applied) */
    uint64_t label_vals_appended;
} vs_pages_follow_info;
/* blk_cnt [n_blocks]: SbqNode items per block of the relation the index was staged from (vs_pages_block_table /
 * vs_pages_dev_block_table); the counts must sum to the index's n.  layout NULL = the default for the index's has_labels.
 * The index must outlive the follower. */
int vs_pages_follow_open(vs_index* idx, uint32_t page_size, const vs_node_layout* layout, const uint32_t* blk_cnt, uint32_t n_blocks,
                         vs_pages_follow** out);
/* The plain twin, in the manner of vs_pages_out_open_plain: a follower of a `plain` index (VS_STORAGE_PLAIN) whose relation holds
 * PlainNode items (AM/plain/node.rs:15-22) on PageType::Node pages.  The handle is an ordinary vs_pages_follow: stage, new_tids, apply,
 * discard and close work on it unchanged, and the rule checked on the page headers is the one above with VS_PAGE_NODE pages as the
 * node pages (an SbqNode-typed page counts 0 items).  blk_cnt [n_blocks]: PlainNode items per block, the table vs_pages_open_plain +
 * vs_pages_block_table report.  layout NULL = vs_plain_layout_default (off_bq_vector names the vector field, off_labels is ignored).
 * It makes no difference whether vs_index_alloc or vs_index_upload made the index.  The pages are checked and scattered by
 * k_pages_follow_plain (a wave per listed page).
 * vs_pages_follow_info on a plain follower: every field keeps its meaning; label_vals_appended is 0; codes_changed counts the EXISTING
 * nodes (on the listed pages) whose PlainNode.vector differs, bit for bit, from what the plain page writer would compose for that node
 * from the resident row — the first dim_index floats of the row, for cosine each float divided by the divisor of that slice (vnorm,
 * or vnorm_idx when dim_index < dim_full) where the divisor is not zero: k_pages_encode_plain's rule, evaluated by the same code
 * under the same flags.  That difference is REPORTED, NOT APPLIED: the reference never rewrites a node's vector, the vector column
 * holds the heap's raw rows, and a normalised slice cannot be turned back into one — so on an existing node the write pass writes
 * the heap tid and the neighbor row only, and the resident vector row, vnorm and vnorm_idx stay byte for byte.  The count is meaningful
 * where the vector column holds the heap's rows, or the node vectors under L2 / inner product; for a cosine index uploaded with the
 * node vectors as its column it counts the rows whose second normalisation is not the identity.
 * Appended rows: vs_pages_follow_apply with new_vecs stages the rows behind n as for an SBQ index and computes the divisors as
 * vs_index_insert does for a plain index (vnorm, and vnorm_idx where the index keeps one).  With new_vecs == NULL and dim_index ==
 * dim_full the write pass copies the appended nodes' vectors FROM THE PAGES into the vector column (for cosine these are the
 * normalised vectors) and the divisors are computed over those rows; either way a row's padding floats [dim_full, vec_stride) are
 * zero.  With dim_index < dim_full a NULL new_vecs on an append is VS_ERR_INVALID, nothing written: the pages hold only the index slice.
 * VS_ERR_INVALID with nothing allocated: an SBQ index (vs_pages_follow_open follows those), an index without vector column /
 * neighbor lists / heap tids, a cosine index without the divisor cache, a block table that does not sum to n, a layout whose
 * offsets do not fit the root. */
int vs_pages_follow_open_plain(vs_index* idx, uint32_t page_size, const vs_node_layout* layout, const uint32_t* blk_cnt, uint32_t n_blocks,
                               vs_pages_follow** out);
/* blocks [n] strictly ascending; pages: n pages, page i = block blocks[i] as it is now.  The host reads the page headers only;
 * the pages go to HBM through the pinned ring and the check pass fills `info` (may be NULL).  Nothing of the index is written;
 * a malformed item is reported as the device reader reports it.  A second stage replaces the first; a refused one leaves none. */
int vs_pages_follow_stage(vs_pages_follow* f, const uint32_t* blocks, const void* pages, uint32_t n, uint32_t n_blocks_total,
                          vs_pages_follow_info* info);
/* the appended nodes' heap tids in node order: the heap_tids array vs_heap_open takes, to read their vectors before the apply */
int vs_pages_follow_new_tids(const vs_pages_follow* f, uint64_t* tids, uint32_t cap);
/* VS_ERR_STATE without a staged list, on a view, while a view exists or a batch is in flight.  new_vecs [n_appended][vec_stride]
 * floats: required when the index holds a vector column and rows are appended (else VS_ERR_INVALID, nothing written; ignored
 * otherwise; a plain follower whose index has dim_index == dim_full takes NULL as "the vectors are in the pages", see
 * vs_pages_follow_open_plain).  Capacity grows as vs_index_insert grows it; codes are taken from the pages, norms computed for the new rows,
 * label sets appended, the own visibility mask gets 1 and every stored snapshot 0 for the new rows; derived state is treated as
 * vs_index_insert treats it.  The follower's table advances only on success. */
int vs_pages_follow_apply(vs_pages_follow* f, const float* new_vecs, uint32_t vec_stride, vs_pages_follow_info* info);
/* vs_pages_follow_apply with the appended rows already in DEVICE memory (d_new_vecs [n_appended][vec_stride], e.g. what vs_heap_dev_*
 * read over vs_pages_follow_new_tids): a strided device-to-device copy in place of the upload.  Every other rule is unchanged and the
 * result is byte-identical to the host form given the same rows (padding floats of the new rows zero). */
int vs_pages_follow_apply_dev(vs_pages_follow* f, const float* d_new_vecs, uint32_t vec_stride, vs_pages_follow_info* info);
int vs_pages_follow_discard(vs_pages_follow* f);  /* forget the staged list */
void vs_pages_follow_close(vs_pages_follow* f);

/* ---- the way back: a device-resident index written out as the pages of a `diskann` index relation (vs_pages.cpp,
 * vs_pages_dev.hip) — the layout the reference's ambuild leaves behind: block 0 = Meta chain (MetaPageHeader item 1, MetaPage
 * item 2; MetaPage::store, AM/meta_page.rs:344-365), the chained SbqMeans item (AM/sbq/mod.rs:123-137), then the SbqNode items
 * in node order on PageType::SbqNode pages filled by the Tape rule (a new page when aligned free space < item size,
 * util/tape.rs:53-76); a MetaPage that has outgrown block 0 (hundreds of labeled start nodes) chains onto fresh pages after
 * the last node page.  Every node item carries num_neighbors ItemPointers, (InvalidBlockNumber, 0) from the list's end on;
 * deleted tuples keep heap offset 0; no all-zero block is emitted.  memory_optimized (SBQ) indexes, classic and labeled nodes.
 * The node pages are composed ON the device (k_pages_encode: a workgroup per page, neighbor ids become ItemPointers there)
 * and leave through the pinned ring, the encode of one chunk under the copy of the previous one; the few metadata pages are
 * encoded on the host.  Classic nodes all have one size, so node -> (block, offset) is arithmetic; label sets make the item
 * size vary, so vs_pages_out_open computes the page breaks in one sequential host pass over the label offsets (4 bytes per
 * node down, 6 bytes per node up and kept on the device until vs_pages_out_close).  The field order inside the archived
 * structs stays a parameter (vs_node_layout / vs_meta_layout), as for the readers. */
typedef struct vs_pages_out vs_pages_out;
typedef struct vs_pages_out_params {
    uint32_t page_size;                 /* VS_BLCKSZ (the only size the writer lays out)                                  */
    const vs_node_layout* node_layout;  /* NULL = vs_node_layout_default(has_labels); for classic nodes off_labels, when it
                                         * names a slot, is where the always-empty _neighbor_vectors field goes             */
    const vs_meta_layout* meta_layout;  /* NULL = vs_meta_layout_default                                                   */
    const char* extension_version;      /* MetaPage.extension_version_when_built (NULL = "", at most 63 bytes)             */
    uint32_t search_list_size;          /* build-time MetaPage fields the index handle does not keep                       */
    double max_alpha;
} vs_pages_out_params;
/* fixes the whole layout: info->n_blocks is the relation's size, the other fields are what a reader of the result reports.
 * The index's arrays, start nodes and quantizer must not change until vs_pages_out_close.  VS_ERR_INVALID for an index of
 * another storage type (a `plain` index goes through vs_pages_out_open_plain) or without codes / neighbors. */
int vs_pages_out_open(vs_index* idx, const vs_pages_out_params* p, vs_pages_out** out, vs_pages_info* info);
/* The writer-side twin of vs_pages_open_plain: a `plain` index (VS_STORAGE_PLAIN) written out as the relation the reference's
 * ambuild leaves behind for plain storage — block 0 = Meta chain (storage_type 0, quantizer_metadata invalid, has_labels 0, start
 * nodes None while default_start is VS_INVALID_NODE, else the node's ItemPointer without labeled entries), NO SbqMeans chain, then
 * from block 1 on the PlainNode items (AM/plain/node.rs:15-22) in node order on PageType::Node pages filled by the Tape rule; the
 * first node page exists even for an index of zero rows (vs_index_alloc makes one: 2 blocks).  An item is the dim_index floats of
 * PlainNode.vector, the empty pq_vector, num_neighbors ItemPointers and the archived root: 4 * dim_index + 8 * num_neighbors +
 * root_size bytes for every node, so node -> (block, offset) is arithmetic.  PlainNode.vector is the first dim_index floats of the
 * row in the vector column, for cosine divided by the divisor of that slice where it has one (preprocess_cosine, as the plain
 * scans apply it).  p->node_layout: NULL = vs_plain_layout_default (off_bq_vector names the vector field; off_labels is ignored,
 * the pq_vector field takes the lowest free 8-byte slot of the root).  The node pages are composed on the device
 * (k_pages_encode_plain).  The handle is an ordinary vs_pages_out: every call below works on it unchanged, and it counts among the
 * index's open writers.  info is what vs_pages_open_plain + vs_pages_finish report for the written bytes (words = dim_index,
 * pages_by_type[VS_PAGE_NODE]).  It makes no difference whether vs_index_alloc or vs_index_upload made the index.
 * VS_ERR_INVALID, nothing written and no writer opened: an SBQ index (vs_pages_out_open writes those), an index without vector
 * column / neighbor lists / heap tids, a cosine index without the divisor cache, page_size != VS_BLCKSZ, an item that does not
 * fit a fresh page (with the default layout and 50 neighbor slots: more than 1930 dimensions). */
int vs_pages_out_open_plain(vs_index* idx, const vs_pages_out_params* p, vs_pages_out** out, vs_pages_info* info);
/* blocks first_block .. first_block + n_blocks - 1 into the host buffer `pages`: any range, in any order, any number of
 * times, always the same bytes (stream to a file or to smgrextend in chunks of the caller's choosing) */
int vs_pages_out_read(vs_pages_out* w, uint32_t first_block, uint32_t n_blocks, void* pages);
/* the same into DEVICE memory (vs_dev_alloc): the node pages are composed in place by one launch, nothing crosses PCIe but
 * the metadata pages */
int vs_pages_out_read_dev(vs_pages_out* w, uint32_t first_block, uint32_t n_blocks, void* d_pages);
int vs_pages_out_item_pointer_of(const vs_pages_out* w, uint32_t node, uint32_t* block, uint32_t* offset);
void vs_pages_out_close(vs_pages_out* w);
/* ---- page by page: only the blocks an insert or a vacuum changed are written back.  The reference persists that way at every
 * point: bulk_delete_for_storage commits a page only `if modified` (AM/vacuum.rs:80-136), aminsert dirties the pages of the new
 * node and of the nodes whose neighbor lists it rewrote (AM/build.rs:464-558).  A BASELINE records what the relation looked like
 * when it was last written: n_blocks, one 128-bit digest per node page (16 bytes per block, kept in device memory) and verbatim
 * copies of the few pages the host encodes (Meta chain, SbqMeans chain).  The digest is taken over the BYTES OF THE FINISHED
 * PAGE — the digest pass is k_pages_encode composing the page in LDS with the digest as its tail instead of the 8 KB of stores —
 * so it cannot miss a way a page changes: neighbor ItemPointers that moved because other nodes did, page breaks that moved
 * because an earlier label set grew, vs_index_insert's back-pointers, vs_index_repair, vs_index_set_labels, a rebuild.  It reads
 * what an encode reads and writes 16 bytes per page.  The function is in DESIGN.md section 6; the odds that a changed page keeps
 * its digest are 2^-128 per changed page for changes that were not made to collide (it is not a cryptographic hash).
 * A baseline belongs to the device of the writer's context, not to the writer or the index: it survives vs_pages_out_close,
 * vs_index_insert moving every array, vs_index_reserve and vs_index_free; vs_pages_base_free releases it.
 * Out of scope: a baseline of pages something else wrote (the relation files an index was staged from carry pd_lsn, checksums
 * and the reference's own page fill).  A baseline describes a relation THIS writer produced; a writer opened with other
 * vs_pages_out_params simply finds every page changed, which is correct, not an error. */
typedef struct vs_pages_base vs_pages_base;
/* digests of the relation exactly as `w` would write it now: one digest-pass launch + copies of the host-encoded pages */
int vs_pages_out_baseline(vs_pages_out* w, vs_pages_base** out);
void vs_pages_base_free(vs_pages_base* b);
uint32_t vs_pages_base_blocks(const vs_pages_base* b);
/* the blocks of w's relation that are not, byte for byte, what `base` recorded: every block >= base's n_blocks, every block whose
 * digest (node pages) or bytes (host-encoded pages) differ, every block whose kind changed (node page <-> host-encoded page).
 * Ascending (the list is compacted on the device by a prefix scan, not by an atomic counter).  *n_dirty = how many; the list
 * stays with the writer until the next delta call or vs_pages_out_close (vs_pages_out_delta_blocks copies it out; cap < *n_dirty
 * is VS_ERR_INVALID).  new_base (may be NULL) receives the baseline of the relation as it is NOW — the pass has computed every
 * digest anyway — so a caller advances without a second pass.  A relation that got shorter is legal: *n_blocks_now (may be NULL)
 * tells the caller where to truncate. */
int vs_pages_out_delta(vs_pages_out* w, const vs_pages_base* base, uint32_t* n_dirty, uint32_t* n_blocks_now, vs_pages_base** new_base);
int vs_pages_out_delta_blocks(const vs_pages_out* w, uint32_t* blocks, uint32_t cap);
/* the gathered form of vs_pages_out_read / _read_dev: pages[i] = block blocks[i]; any list, any order, repeats allowed.  The node
 * pages go through the same double-buffered pinned ring, chunks cut from the list (k_pages_encode takes its pages from an indirect
 * list); host-encoded pages are served from the layout.  A block >= n_blocks anywhere in the list is VS_ERR_INVALID and nothing is
 * written. */
int vs_pages_out_read_blocks(vs_pages_out* w, const uint32_t* blocks, uint32_t n, void* pages);
int vs_pages_out_read_blocks_dev(vs_pages_out* w, const uint32_t* blocks, uint32_t n, void* d_pages);
/* rkyv::to_bytes::<MetaPage> (host-only; the counterpart of vs_meta_page_decode): the labeled start nodes in key order,
 * written as the archived B-tree when meta->has_start_nodes; meta->n_labeled_start_nodes is ignored in favour of n_starts.
 * *len = bytes needed; buf may be NULL to query it; a buf of cap < *len is an error and nothing is written. */
int vs_meta_page_encode(const vs_meta_page* meta, const int16_t* start_labels, const uint32_t* start_blocks,
                        const uint32_t* start_offsets, uint32_t n_starts, const vs_meta_layout* layout, void* buf, size_t cap,
                        size_t* len);

/* ---- K4: SBQ quantisation of queries (SbqQuantizer::quantize, AM/sbq/quantize.rs:52-102) --------------------- */
/* q: host [nq][dim_index], already cosine-normalised by the caller if applicable; out: host [nq][words] */
int vs_quantize(vs_index* idx, const float* q, uint32_t nq, uint64_t* out_codes);

/* ---- K1: XOR+popcount of query codes against gathered node codes (distance_xor_optimized, AM/distance/mod.rs:266-323)
 * ids/off: CSR — query i is scored against ids[off[i] .. off[i+1]).  out: one u32 per id. */
int vs_hamming_gather(vs_index* idx, const uint64_t* qcodes, const uint32_t* ids, const uint32_t* off, uint32_t nq,
                      uint32_t* out);

/* ---- K2: full-precision rerank distances (get_full_distance_for_resort, AM/sbq/storage.rs:304-328 with
 * distance_l2 / distance_cosine / distance_inner_product in the reference's AVX2 accumulation order,
 * AM/distance/mod.rs:325-435).  q_full: host [nq][dim_full] RAW queries (cosine-normalised inside, as
 * PgVector::from_datum does, AM/pg_vector.rs:153-155). */
int vs_rerank(vs_index* idx, const float* q_full, const uint32_t* ids, const uint32_t* off, uint32_t nq, float* out);

/* ---- K4a on its own: what a search prepares of each query before its first expansion (PgVector::from_datum +
 * SbqSearchDistanceMeasure::new): the device rows as they lie, padding included.  queries: host [nq][dim_full] RAW queries.
 * out_q_full [nq][vec_stride] floats, out_codes [nq][code_stride] words (NULL allowed; always NULL-tolerant on plain storage, whose
 * rows carry no code), out_q_index [nq][vec_stride] floats, only for plain storage with dim_index < dim_full (NULL otherwise).  The
 * strides are those vs_index_array reports for VS_ARR_VECS / VS_ARR_CODES. */
int vs_prepare_queries(vs_index* idx, const float* queries, uint32_t nq, float* out_q_full, uint64_t* out_codes, float* out_q_index);

/* ---- K5: flat scan — top-k of Hamming distance over ALL codes, order (hamming asc, node id asc) ------------- */
int vs_scan_topk(vs_index* idx, const uint64_t* qcodes, uint32_t nq, uint32_t k, uint32_t* out_ids, uint32_t* out_ham);
/* The same with the scan's predicate: only rows whose label set overlaps the query's key (qlabels / qlabel_off: CSR per query, an
 * empty key filters nothing — LabelSetView::overlaps, AM/labels/mod.rs:124-142, AM/scan.rs:189) and, with live_only, whose heap
 * tuple is not deleted (AM/scan.rs:231-234) are ranked: the EXACT filtered SBQ top-k, what the label-filtered graph walk
 * approximates.  An explicit entry point (ground truth of the SBQ ranking, exact mode for very selective keys); the access-method
 * callbacks never switch to it on their own, because their rows must be the reference's graph walk's. */
int vs_scan_topk_filtered(vs_index* idx, const uint64_t* qcodes, const int16_t* qlabels, const uint32_t* qlabel_off, int live_only,
                          uint32_t nq, uint32_t k, uint32_t* out_ids, uint32_t* out_ham);

/* ---- K3 (+K2 + resort window): batched scans ------------------------------------------------------------------
 * For each query: exactly the rows the reference returns from the first k amgettuple calls after amrescan
 * (TSVResponseIterator::next_with_resort, AM/scan.rs:244-305) with GUCs diskann.query_search_list_size =
 * search_list_size and diskann.query_rescore = rescore (AM/guc.rs:3-4).
 *   queries   host [nq][dim_full] raw f32
 *   qlabels / qlabel_off: CSR of the smallint[] scan keys, qlabel_off == NULL => no scan key on any query.  A key may hold any
 *             number of labels, as in the reference (LabelSet, AM/labels/mod.rs:19-37): up to 64 distinct labels ride in on-chip
 *             memory, a wider key is read from global memory by the general kernel (the LDS-resident kernel hands such scans
 *             over: vs_stats.fallback_scans).  Only the label-aware BUILD limits a node to 64 labels (VS_ERR_INVALID beyond).
 *   out_ids   [nq][k] node ids (VS_INVALID_NODE past the end of a scan), out_tids [nq][k] heap TIDs (may be NULL),
 *   out_dist  [nq][k] reranked f32 distance (NaN when rescore == 0) (may be NULL)                               */
int vs_search_batch(vs_index* idx, const float* queries, const int16_t* qlabels, const uint32_t* qlabel_off, uint32_t nq,
                    uint32_t search_list_size, uint32_t rescore, uint32_t k, uint32_t* out_ids, uint64_t* out_tids,
                    float* out_dist, vs_stats* stats);
/* the raw SBQ-ordered stream: first m results of TSVResponseIterator::next (AM/scan.rs:210-242) */
int vs_stream_batch(vs_index* idx, const float* queries, const int16_t* qlabels, const uint32_t* qlabel_off, uint32_t nq,
                    uint32_t search_list_size, uint32_t m, uint32_t* out_ids, uint32_t* out_ham, vs_stats* stats);
/* device-resident variant: d_queries [nq][dim_full] and the outputs are device pointers (vs_dev_alloc); label keys
 * must already be sorted + de-duplicated per query.  Enqueues on the ctx stream and returns; vs_ctx_sync() (or
 * vs_search_batch_dev_finish for the stats / error check) completes it. */
int vs_search_batch_dev(vs_index* idx, const float* d_queries, const int16_t* d_qlabels, const uint32_t* d_qlabel_off,
                        uint32_t nq, uint32_t search_list_size, uint32_t rescore, uint32_t k, uint32_t* d_out_ids,
                        uint64_t* d_out_tids, float* d_out_dist);
int vs_search_batch_dev_finish(vs_index* idx, vs_stats* stats);

/* ---- launch-variant selection (ours; the reference has no counterpart — its only query-time knobs are the two GUCs above,
 * AM/guc.rs:3-43, and they stay the caller's).  The search kernel exists in several EXACT instantiations that differ only in
 * how a scan keeps its private state (dedup tables cleared per scan, a written-bucket bitmap, an occupancy bit per slot; for small
 * scans: dedup table in LDS or not; DESIGN.md 3.1 / 4, docs/LAB_NOTEBOOK.md 10b).  Which is fastest depends on the index size and on the box, so it is measured
 * where it runs: vs_index_autotune runs every applicable variant on the caller's own device-resident batch (the arguments of
 * vs_search_batch_dev), `reps` timed steps each after one warm-up, holds every row, every distance bit and every work counter of
 * a variant to the library default's on the same batch, DISQUALIFIES a variant that differs anywhere (rows_identical = 0) and
 * makes the fastest qualified one the index's choice when it beats the default by at least 3 % and does so again on a second timing.  VS_F_* environment
 * variables still override the choice per call.  report (may be NULL) receives one entry per variant, the default first.
 * A caller that cannot afford a misbehaving kernel in its own process probes the variants in a child process first
 * (pgvectorscale_amd/tune_probe.py: a small index of the same code width, every variant, a hard timeout) and passes the ones
 * that did not come back clean as `skip`. */
typedef struct vs_tune_entry {
    char name[40];
    float step_ms;          /* best device time of one step (search + rerank + rescore window), HIP events on the ctx stream */
    float search_ms;        /* of which the search kernel(s) of the first attempt */
    uint32_t applicable;    /* 0: the variant does not exist for this index / operating point (launched the default's kernel) */
    uint32_t rows_identical;/* ids, distance bits and work counters equal the default's on the whole batch */
    uint32_t chosen;
    int32_t error;          /* VS_OK, or the error the variant's launch returned (it is then not eligible) */
} vs_tune_entry;
int vs_index_autotune(vs_index* idx, const float* d_queries, const int16_t* d_qlabels, const uint32_t* d_qlabel_off,
                      uint32_t nq, uint32_t search_list_size, uint32_t rescore, uint32_t k, uint32_t reps,
                      const char* skip /* comma-separated variant names not to launch at all, or NULL */,
                      vs_tune_entry* report, uint32_t report_cap, uint32_t* n_report);
/* name the variant by hand ("default", or a name vs_index_autotune reports) / read the current choice */
int vs_index_set_variant(vs_index* idx, const char* name);
int vs_index_get_variant(vs_index* idx, char* buf, size_t len);

/* ---- the amrescan / amgettuple mirror (one row at a time) ----------------------------------------------------
 * A scan keeps what TSVScanState keeps between amgettuple calls (lsr + resort_buffer, AM/scan.rs:162-174) on the device and
 * CONTINUES the beam search when the executor asks for more rows (AM/scan.rs:370-405): it is never run again from the start
 * (except after a capacity overflow, vs_stats.retries), and the rows prefetched ahead of the executor stay within ~6 % of
 * what was pulled.  One thread per scan; scans of one index share its vs_ctx stream. */
int vs_beginscan(vs_index* idx, vs_scan** out);                                  /* ambeginscan */
/* query == NULL is the SQL-NULL query (zero vector, labels ignored; AM/labels/mod.rs:214-216).
 * has_label_key: nkeys == 1 (sets xs_recheck, AM/scan.rs:350-352); labels may be unsorted / contain duplicates. */
int vs_rescan(vs_scan* scan, const float* query, const int16_t* labels, uint32_t n_labels, int has_label_key,
              uint32_t search_list_size, uint32_t rescore);                       /* amrescan */
/* returns 1 and fills the outputs for the next row, 0 at end of scan, <0 on error */
int vs_gettuple(vs_scan* scan, uint64_t* heap_tid, uint32_t* node, float* dist); /* amgettuple */
/* optional hint: the executor will pull `rows` rows in all (a LIMIT it knows): they are produced by one continuation instead
 * of several.  Fewer rows become available when the scan ends first; never an error to ask for more than exist. */
int vs_scan_prefetch(vs_scan* scan, uint32_t rows);
int vs_scan_xs_recheck(const vs_scan* scan);
/* GreedySearchStats as the reference's scan holds them after the amgettuple calls made so far (AM/stats.rs:68-125,
 * AM/scan.rs:461-472): the counters are recorded per emitted row, so prefetched rows do not show (zero on a broker scan). */
int vs_scan_get_stats(const vs_scan* scan, vs_stats* out);
/* what the device really did for the scan since vs_rescan (prefetched rows and restarts included); launches may be NULL */
int vs_scan_get_work(const vs_scan* scan, vs_stats* out, uint32_t* launches);
void vs_endscan(vs_scan* scan);                                                   /* amendscan */

/* ---- many streamed scans continued TOGETHER (vs_scanpool.cpp) ------------------------------------------------
 * A single cursor continues its scan with a launch of its own: one wave on the chip and half a millisecond of launch / copy
 * overhead per continuation, and 64 backends streaming at once are 64 such launches per round.  A scan pool keeps what
 * TSVResponseIterator keeps per scan (lsr + resort_buffer, AM/scan.rs:162-174) for up to `capacity` scans in pooled device arrays,
 * so that ONE resumed launch (plus one rerank launch) continues every scan that asked for rows in this round — what a GPU broker
 * does with the amgettuple calls of many backends that arrive together.  Rows and GreedySearchStats are the single cursor's, row
 * for row.  All scans of a pool share the GUCs (search_list_size, rescore) and the visibility mask in force; scan keys are per
 * scan (slot).  kmax = most rows one fetch asks for; rows_cap = most stream rows a pooled scan may produce (0: 4096) — a scan that
 * needs more fails with VS_ERR_CAPACITY in its out_rows entry and is continued by a vs_scan of its own.  One thread at a time.
 * Which kernel continues the scans is decided at creation: for SBQ storage the resumable instantiation of the fast kernel, for
 * `plain` storage the resumable form of k_search_plain (VS_POOL_PLAIN_FAST, above) — both sized for the worst case of a scan of
 * rows_cap rows — and the general kernel where neither applies (wide codes, a state beyond 96 KB of LDS, VS_POOL_FAST "0").  The
 * plain form clamps its capacities to the n of the pool's creation: after vs_index_insert has grown a plain index, free the pool and
 * create it again (one that is kept and rescanned may fail scans the grown index makes longer with VS_ERR_CAPACITY). */
typedef struct vs_scan_pool vs_scan_pool;
int vs_scanpool_create(vs_index* idx, uint32_t capacity, uint32_t search_list_size, uint32_t rescore, uint32_t kmax, uint32_t rows_cap,
                       vs_scan_pool** out);
void vs_scanpool_free(vs_scan_pool* pool);
int vs_scanpool_rescan(vs_scan_pool* pool, uint32_t slot, const float* query, const int16_t* labels, uint32_t n_labels,
                       int has_label_key);                                                                   /* amrescan of one slot */
int vs_scanpool_endscan(vs_scan_pool* pool, uint32_t slot);
/* amgettuple x k for the n listed slots at once: out_*[i][0 .. out_rows[i]) are the next rows of slots[i] (fewer than k: its scan
 * has ended; a negative VS_ERR_*: that scan failed, the others are served).  out_tids / out_ids / out_dist may be NULL. */
int vs_scanpool_fetch(vs_scan_pool* pool, const uint32_t* slots, uint32_t n, uint32_t k, uint64_t* out_tids, uint32_t* out_ids,
                      float* out_dist, int32_t* out_rows);
int vs_scanpool_get_stats(const vs_scan_pool* pool, uint32_t slot, vs_stats* out);  /* as vs_scan_get_stats */
int vs_scanpool_get_work(const vs_scan_pool* pool, uint64_t* launches, uint64_t* rounds);  /* shared search launches / rounds so far */
/* Which kernel the pool's continuations run (kernel: VS_SEARCH_GENERAL / _FAST_SBQ / _FAST_PLAIN) — valid before the first fetch.
 * resident = the pool's capacity for the two fast kernels (one single-wave workgroup per slot), 0 for the general one; lds_bytes =
 * dynamic LDS per scan; heap_lds / dedup_slots / visited_cap = the planned on-chip capacities of the fast kernels (0 for the general
 * one).  Read-only.  VS_ERR_INVALID for NULL arguments. */
int vs_scanpool_info(const vs_scan_pool* pool, vs_search_info* out);

/* ---- coalescing concurrent scans into batched launches (vs_broker.cpp) -------------------
 * The reference serves one query per single-threaded backend (amcanparallel = false, AM/mod.rs:63); a GPU needs thousands
 * of scans per launch.  A broker owns the index (its dispatcher thread is the only thread that touches the vs_ctx); any
 * number of client threads call vs_broker_search(), which blocks until the scan's rows are ready.  The dispatcher
 * gathers requests for at most max_wait_us after the oldest one (or until max_batch are waiting) and runs every group
 * that shares (search_list_size, rescore, k, label key present, snapshot) as one vs_search_batch().  Heap visibility: scans of
 * different backends see different snapshots, so a request names the snapshot mask it runs under (vs_broker_search_snapshot;
 * masks are handed to the dispatcher with vs_broker_snapshot_put) and only scans of one snapshot share a launch; plain
 * vs_broker_search = snapshot 0 = every tuple visible.  The index-level mask of vs_index_set_visibility is not consulted by a
 * broker (it is left as it was).  In a PGRX deployment the queue lives in shared memory and the dispatcher is a background
 * worker. */
typedef struct vs_broker vs_broker;
typedef struct vs_broker_config {
    uint32_t max_batch;   /* scans per launch at most (0 = 8192)                                  */
    uint32_t max_wait_us; /* how long the oldest waiting scan may be held back to let others join */
    uint32_t cursor_lanes; /* 0 (default): the continuations of the scans' cursors (amgettuple past the shared first rows) run on
                            * the dispatcher thread, one at a time, between two shared launches.  n > 0: on n lanes — threads of the
                            * broker with a HIP stream and a view of the index each — so that n scans continue concurrently on the
                            * device and none of them waits behind a shared launch (a scan stays on its lane).  vs_shm_server:
                            * the streamed scans of client processes, by (client pid, scan id).  Cost per lane: a context
                            * with 2 x 1 MiB of pinned staging memory and the device workspace of the scans it continues.
                            * (VS_BROKER_LANES in the environment: the lane count of brokers created with 0 — how the test tier
                            * runs every broker test on lanes; leave it unset in production.)                         */
    uint32_t cursor_pool; /* (vs_shm_server) n > 0: the streamed scans of the client processes live in scan pools of n slots
                           * (vs_scanpool_*: one pool per (search_list_size, rescore, snapshot) in use, four at most) and the
                           * amgettuple continuations that arrive in one dispatcher round are served by SHARED launches — 64
                           * backends streaming at once cost about what one costs.  Scans a pool cannot take (no free pool for
                           * their GUCs, more than 4096 stream rows) fall back to a cursor of their own.  (VS_SHM_CURSOR_POOL in
                           * the environment: the pool size of servers created with 0 — test tier.)                          */
} vs_broker_config;
typedef struct vs_broker_stats {
    uint64_t batches;   /* vs_search_batch calls made                */
    uint64_t scans;     /* scans served                              */
    uint64_t max_batch; /* largest number of scans in one launch     */
    uint64_t tasks;     /* single-scan pieces of work run by the dispatcher between launches (cursor continuations) */
    uint64_t cursors;   /* (vs_shm_server) scan cursors the serving process holds open right now */
} vs_broker_stats;
int vs_broker_create(vs_index* idx, const vs_broker_config* cfg /* NULL = defaults */, vs_broker** out);
/* one scan: the rows of its first k amgettuple calls (as vs_search_batch).  query == NULL: the SQL-NULL query (label keys
 * ignored).  Thread safe; blocks.  out_tids / out_dist may be NULL. */
int vs_broker_search(vs_broker* b, const float* query, const int16_t* labels, uint32_t n_labels, int has_label_key,
                     uint32_t search_list_size, uint32_t rescore, uint32_t k, uint32_t* out_ids, uint64_t* out_tids,
                     float* out_dist);
/* the same under snapshot mask `snapshot` (0 = every tuple visible; an id without a mask fails with VS_ERR_STATE) */
int vs_broker_search_snapshot(vs_broker* b, const float* query, const int16_t* labels, uint32_t n_labels, int has_label_key,
                              uint32_t search_list_size, uint32_t rescore, uint32_t k, uint32_t snapshot, uint32_t* out_ids,
                              uint64_t* out_tids, float* out_dist);
/* the same for a scan that names a visibility slot (vs_index_vis_slot_eval; 0 = every tuple visible): such scans group by
 * (search_list_size, rescore, k, label key present) only — the snapshot leaves the key — and run as one vs_search_batch_vis(), each
 * scan under the overlay of its own slot.  A slot >= VS_MAX_VIS_SLOTS is VS_ERR_INVALID; a slot without an overlay fails the launch
 * it joined with VS_ERR_STATE.  The base and the overlays are evaluated on the dispatcher thread (vs_broker_call_exclusive with
 * vs_index_vis_base_eval / vs_index_vis_slot_eval ... on vs_broker_index); cursor lanes take them over before every task as they
 * take over the masks.  Follow-up, not built yet: slots in the shm server's request layout, in scan pools and in cursors — those
 * run under a materialized legacy id (vs_index_vis_materialize). */
int vs_broker_search_vis(vs_broker* b, const float* query, const int16_t* labels, uint32_t n_labels, int has_label_key,
                         uint32_t search_list_size, uint32_t rescore, uint32_t k, uint32_t slot, uint32_t* out_ids, uint64_t* out_tids,
                         float* out_dist);
/* hands a snapshot's mask (n host bytes; NULL drops it) to the dispatcher; returns when it is in place.  Thread safe. */
int vs_broker_snapshot_put(vs_broker* b, uint32_t snapshot, const uint8_t* visible);
int vs_broker_get_stats(vs_broker* b, vs_broker_stats* out);
vs_index* vs_broker_index(vs_broker* b);
/* the amrescan / amgettuple mirror on top of a broker: like vs_beginscan, but the scan's first 16 rows come out of a launch
 * shared with the scans of other threads (backends) — a LIMIT <= 16 never needs more — and an executor that keeps pulling gets a
 * cursor of its own on the device, opened, continued and released on the dispatcher thread (vs_broker_call): from then on the
 * scan is continued, never re-run, and vs_scan_get_stats is exact as for a direct scan (for a scan that only ever used the
 * shared launch it replays the scan on a cursor when asked).  vs_rescan / vs_gettuple / vs_endscan as usual; end a broker's
 * scans before vs_broker_destroy. */
int vs_beginscan_on_broker(vs_broker* b, vs_scan** out);
/* the visibility mask (vs_broker_snapshot_put) a scan on a broker runs under, from its next vs_rescan on (0 = every tuple
 * visible, the default).  A direct scan runs under the index's current mask instead. */
int vs_scan_set_snapshot(vs_scan* scan, uint32_t snapshot);
/* runs fn(arg) on the dispatcher thread between two launches and returns its result (the error text comes along): the way work
 * on ONE scan's device state reaches the only thread that may touch the index.  Thread safe; blocks. */
int vs_broker_call(vs_broker* b, int (*fn)(void*), void* arg);
/* The same, run while no cursor lane is inside a task (what vs_broker_snapshot_put does for a mask): for work that REWRITES what
 * lanes read — vs_index_snapshot_eval / _patch, vs_index_vis_base_eval, vs_index_vis_slot_eval / _patch / _drop and
 * vs_index_vis_materialize into a legacy id that a cursor may be scanning under.  Through plain vs_broker_call such a call may run
 * while a lane's cursor reads the mask it rewrites in place, or while a lane takes the base over; on a broker with cursor lanes use
 * this one.  VS_ERR_STATE when called from inside a dispatcher task. */
int vs_broker_call_exclusive(vs_broker* b, int (*fn)(void*), void* arg);
void vs_broker_destroy(vs_broker* b); /* serves what is queued, then stops the dispatcher */

/* ---- the same across PROCESSES (vs_shm.cpp): PostgreSQL backends are processes, so the request queue is a POSIX shared-memory
 * segment (`name`, "/..."): one slot per in-flight scan (query vector, keys, GUCs, the k result rows, a futex).  The process that
 * owns the vs_ctx / vs_index creates the segment and runs the dispatcher (groups posted scans exactly like vs_broker); a client
 * needs no HIP: it maps the segment, posts a scan with vs_shm_client_search() and sleeps until its rows are in the slot.  In a
 * PGRX deployment the segment is a DSM segment, the futex a latch, the dispatcher a background worker. */
typedef struct vs_shm_server vs_shm_server;
typedef struct vs_shm_client vs_shm_client;
int vs_shm_server_create(vs_index* idx, const char* name, uint32_t nslots /* scans in flight at most (max_connections) */,
                         uint32_t kmax /* rows per scan at most */, const vs_broker_config* cfg /* NULL = defaults */,
                         vs_shm_server** out);
int vs_shm_server_get_stats(vs_shm_server* s, vs_broker_stats* out);
/* the scan pools of a server (cfg->cursor_pool != 0): out[0] = pools alive, out[1] = shared fetch rounds so far, out[2] = pools re-keyed
 * at the cap of four (an empty pool gives way to a new (search_list_size, rescore, snapshot) combination), out[3] = scans living in pools */
int vs_shm_server_pool_stats(vs_shm_server* s, uint64_t out[4]);
void vs_shm_server_destroy(vs_shm_server* s); /* fails what is still posted, unlinks the segment */
int vs_shm_client_open(const char* name, vs_shm_client** out);
uint32_t vs_shm_client_dim(const vs_shm_client* c); /* dim_full of the index behind the segment */
/* one scan: the rows of its first k amgettuple calls (as vs_search_batch).  query == NULL: the SQL-NULL query (label keys
 * ignored).  Blocks; one call at a time per client handle.  out_tids / out_dist may be NULL. */
int vs_shm_client_search(vs_shm_client* c, const float* query, const int16_t* labels, uint32_t n_labels, int has_label_key,
                         uint32_t search_list_size, uint32_t rescore, uint32_t k, uint32_t* out_ids, uint64_t* out_tids,
                         float* out_dist);
/* the same under snapshot mask `snapshot` of the serving process (vs_shm_server_snapshot_put; 0 = every tuple visible) */
int vs_shm_client_search_snapshot(vs_shm_client* c, const float* query, const int16_t* labels, uint32_t n_labels, int has_label_key,
                                  uint32_t search_list_size, uint32_t rescore, uint32_t k, uint32_t snapshot, uint32_t* out_ids,
                                  uint64_t* out_tids, float* out_dist);
/* amgettuple beyond the first rows, across processes: rows [skip, skip + k) of the scan this process calls `scan_id` (k <= kmax;
 * *n_rows < k: the scan has ended).  The serving process keeps a cursor on the device for the scan (lsr + resort_buffer of
 * AM/scan.rs:162-174) and continues it from request to request; every request carries the whole scan description, so a cursor
 * the server no longer has — or never had, because the first rows came from vs_shm_client_search — is opened and fast-forwarded
 * to `skip` (one replay) and continued from there.  vs_shm_client_end_scan drops the cursor (so does the death of the client). */
int vs_shm_client_fetch(vs_shm_client* c, uint64_t scan_id, const float* query, const int16_t* labels, uint32_t n_labels,
                        int has_label_key, uint32_t search_list_size, uint32_t rescore, uint32_t snapshot, uint32_t skip, uint32_t k,
                        uint32_t* out_ids, uint64_t* out_tids, float* out_dist, uint32_t* n_rows);
int vs_shm_client_end_scan(vs_shm_client* c, uint64_t scan_id);
/* serving process: a snapshot's mask (n host bytes, copied; NULL drops it); in place before the next group is formed */
int vs_shm_server_snapshot_put(vs_shm_server* s, uint32_t snapshot, const uint8_t* visible);
void vs_shm_client_close(vs_shm_client* c);

/* ---- multi-GPU (BASELINE.json north_star: "query batches shard embarrassingly across the 8 GPUs of one node
 * with RCCL over xGMI used only for a final top-k gather").  The reference has nothing to mirror here — AM/mod.rs:63
 * amcanparallel = false, one backend runs one scan (AM/scan.rs:308-456) — so this is the seam a PGRX host binds when one
 * PostgreSQL instance fronts several devices.  The path shards by QUERY: every device holds the whole index, device g takes a
 * contiguous block of the batch (vs_shard_range), no collective touches the data path, one gather of the [nq][k] blocks ends
 * the step.  Two deployments, neither needs torch:
 *   vs_multi_*  ONE process owns N devices (a broker / background worker): the index is replicated device to device
 *               (hipMemcpyPeerAsync over xGMI: one build or upload, N - 1 copies), one host thread per device runs its shard of a
 *               host batch and writes its rows into the caller's buffers at the shard's offset.
 *   vs_comm_*   one PROCESS per device: RCCL (ncclAllGather of the id / distance blocks; ncclBroadcast to replicate an index
 *               from the rank that holds it).  librccl is dlopen'ed by the first vs_comm_* call (VS_RCCL_LIB overrides the
 *               name); the 128-byte communicator id travels between the processes by the host's own means. */
int vs_shard_range(uint32_t nq_total, uint32_t world, uint32_t rank, uint32_t* begin, uint32_t* end); /* blocks differ by <= 1 */
/* a full copy of `src` (arrays, quantizer, label sets + start map, visibility masks) on dst_ctx's device, device to device;
 * the copy is an ordinary index (vs_index_free).  Works between two contexts of one device as well. */
int vs_index_replicate(vs_index* src, vs_ctx* dst_ctx, vs_index** out);

typedef struct vs_multi vs_multi;
#define VS_MULTI_COPY_ALWAYS 1u /* also the source's own device gets a replica instead of a view of the source's arrays */
/* one context + one copy of `src` per entry of devices[] (the first entry naming src's own device reads src's arrays through
 * a view; src must outlive the vs_multi and must not be mutated while it exists) */
int vs_multi_create(vs_index* src, const int* devices, uint32_t n_devices, uint32_t flags, vs_multi** out);
uint32_t vs_multi_size(const vs_multi* m);
vs_index* vs_multi_index(vs_multi* m, uint32_t i); /* shard i's index / context: device-resident work is driven per device */
vs_ctx* vs_multi_ctx(vs_multi* m, uint32_t i);
/* vs_search_batch / vs_stream_batch over all devices: same arguments, same rows in the same order as one device returns for the
 * whole batch (scans are independent); stats are summed over the shards */
int vs_multi_search_batch(vs_multi* m, const float* queries, const int16_t* qlabels, const uint32_t* qlabel_off, uint32_t nq,
                          uint32_t search_list_size, uint32_t rescore, uint32_t k, uint32_t* out_ids, uint64_t* out_tids,
                          float* out_dist, vs_stats* stats);
int vs_multi_stream_batch(vs_multi* m, const float* queries, const int16_t* qlabels, const uint32_t* qlabel_off, uint32_t nq,
                          uint32_t search_list_size, uint32_t mrows, uint32_t* out_ids, uint32_t* out_ham, vs_stats* stats);
void vs_multi_destroy(vs_multi* m);

typedef struct vs_comm vs_comm;
#define VS_COMM_ID_BYTES 128
int vs_comm_unique_id(uint8_t* id /* [VS_COMM_ID_BYTES] */);  /* one rank calls it (ncclGetUniqueId), every rank gets the bytes */
int vs_comm_create(vs_ctx* ctx, const uint8_t* id, uint32_t rank, uint32_t world, vs_comm** out); /* collective: ncclCommInitRank */
uint32_t vs_comm_rank(const vs_comm* c);
uint32_t vs_comm_world(const vs_comm* c);
/* the final top-k gather: this rank's device-resident [nq_local][k] blocks -> [nq_total][k] on every rank, shards in rank order
 * (nq_local must be this rank's vs_shard_range of nq_total; d_dist / d_out_dist may both be NULL).  Enqueued on ctx's stream
 * behind the search that produced the blocks (vs_search_batch_dev); vs_ctx_sync completes it.  No host synchronisation. */
int vs_comm_gather_topk(vs_comm* c, const uint32_t* d_ids, const float* d_dist, uint32_t nq_local, uint32_t nq_total, uint32_t k,
                        uint32_t* d_out_ids, float* d_out_dist);
int vs_comm_bcast(vs_comm* c, void* d_buf, size_t bytes, uint32_t root); /* one device array from root to every rank (enqueued) */
/* every rank passes an index of the same geometry on the communicator's device (root: the built / uploaded one, the others:
 * vs_index_alloc); on return every rank holds root's index (arrays, quantizer, label sets + masks, start map, visibility) */
int vs_comm_replicate_index(vs_comm* c, vs_index* idx, uint32_t root);
void vs_comm_destroy(vs_comm* c);

/* ---- build-side helpers (SURVEY.md §8f "next" rows; needed to manufacture device-resident indexes) ---------- */
/* Welford pass over rows [0,n) in heap order, bit-exact to SbqQuantizer::add_sample (AM/sbq/quantize.rs:115-148):
 * one lane per dimension, sequential over rows.  Uses the (cosine-normalised) first dim_index dims of the vectors. */
int vs_sbq_train(vs_index* idx);
/* codes[i] = quantize(normalised index slice of vecs[i]) for all nodes */
int vs_sbq_quantize_corpus(vs_index* idx);
/* Batched Vamana build over the SBQ codes (greedy search + robust prune with alpha ladder, Hamming distances),
 * the GPU counterpart of Graph::insert / prune_neighbors (AM/graph/mod.rs:392-488,637-717).  With label sets attached
 * (vs_index_set_labels before the call) the build is label-aware as Graph::insert is: a filtered pass from the label start
 * nodes, an unfiltered pass from the default start node, contains_intersection in the pruning rule, and a node becomes the
 * start node of every label it is the first to carry (at most 64 labels per node).
 * On a `plain` index (VS_STORAGE_PLAIN, no codes) the same batched build scores with the full-precision pair distance of the
 * reference's IndexFullDistanceMeasure: d(a -> b) is what a plain scan whose query is node a's raw row gives row b, over the first
 * dim_index dimensions; keys are ordered like f32::total_cmp, every order is ascending (key, id).  The
 * cosine divisors of the rows are recomputed from the vector column first.  Node 0 is the default start; the repair pass and the
 * validation of the lists run as for SBQ.
 * Every argument check and every refusal comes before the first byte of the neighbor lists is written: VS_ERR_INVALID for a
 * search_list_size outside [1,1000], a max_alpha outside [1,5], a node with more than 64 labels, and on a plain index for the
 * inner-product distance (DistanceWithTieBreak::new asserts distance >= 0, which -dot violates: the reference has no behaviour to
 * mirror; IP search on an uploaded plain index is unaffected), label sets, or a missing vector column — the index is left byte
 * for byte as it was.  Still refused for plain storage, unchanged: the SBQ forms of calls that have a plain one
 * (vs_index_consolidate_deletes: a plain index is consolidated with vs_index_consolidate_deletes_plain; vs_pages_out_open: it is
 * written back with vs_pages_out_open_plain; vs_pages_follow_open: it is followed with vs_pages_follow_open_plain).  vs_index_repair_labels does not apply: plain storage has no labels. */
int vs_build_graph(vs_index* idx, uint32_t search_list_size, double max_alpha, uint32_t batch_max, uint64_t seed);
/* nodes the last vs_build_graph could not make reachable from the default start node (its repair pass gives every such
 * node an in-edge where that strands nobody else; 0 on well-formed input, 0xFFFFFFFF = graph deeper than the pass can judge).
 * The reference's build gives no reachability guarantee either (AM/graph/mod.rs:700-715 only warns about orphans). */
uint32_t vs_index_build_unreachable(const vs_index* idx);

/* ---- rows that arrive after the index is resident: aminsert (AM/build.rs:464-558) ------------------------------------------
 * The reference's aminsert loads the trained quantizer without touching it (SbqSpeedupStorage::load_for_insert), writes the node
 * (create_node) and links it with Graph::insert (AM/graph/mod.rs:637-735).  vs_index_insert does the same for a batch of rows on
 * the device: the rows become nodes n .. n + n_new - 1 in input order, their cosine divisors and SBQ codes are computed with the
 * quantizer as it stands (mean / m2 / count never change), label sets are appended, a label first carried by an inserted node gets
 * it as its start node and an empty index gets node 0 as the default start (update_start_nodes, AM/graph/mod.rs:490-531).  The
 * rows are then linked in batches of at most batch_max with the machinery of vs_build_graph (build-mode search over the graph
 * as it stands, prune_neighbors, update_back_pointer per target; labeled sets: the filtered pass, then the unfiltered one) and
 * three steps a whole-graph build replaces by its repair sweep, which an insert into 50M nodes cannot afford:
 *   - the batch sees itself: the VS_INSERT_MATES (vs_set_option; default 16, 0 = off, at most 64) nearest nodes of the same
 *     batch by (Hamming, id) join every node's candidates before pruning;
 *   - no new row may be unfindable: a new node is ANCHORED when the row of a node older than its batch names it, or the row of an
 *     anchored node of its batch does — two new nodes that only name each other are not.  A node that is not anchored is given a slot
 *     in the list of its closest old-or-anchored out-neighbor (a free one, else that of the list's last entry when that entry keeps
 *     another such in-edge); what cannot be placed is counted in orphans_left, never hidden.
 * Indexes with the vector column on the device.  A `plain` index (VS_STORAGE_PLAIN) takes the same path without the SBQ parts: the
 * rows are staged behind n with their tids and cosine divisors (of the full row, and of the index slice when dim_index <
 * dim_full), nothing touches the codes, there is no quantizer to be trained (count == 0 is no obstacle), label_off must be NULL,
 * and searches, pruning, back-edges and the batch's mates score with the pair distance of vs_build_graph's plain form (mates by
 * (key of d(row -> other), id)); vs_insert_stats is filled the same way.  VS_ERR_INVALID, the index left byte for byte as it was,
 * for a plain index whose distance is the inner product (see vs_build_graph), that is handed label sets, or that came from
 * vs_index_upload: such an index mirrors a relation; the refusal predates vs_pages_out_open_plain, which writes plain storage
 * back, and lifting it is follow-up work — only plain indexes made with vs_index_alloc take rows (vs_build_graph and
 * vs_index_consolidate_deletes_plain take both).  VS_ERR_STATE: the
 * quantizer of an SBQ index is untrained (count == 0), a view of the index is alive, a batch is in flight, a vs_pages_out writer of the
 * index is open (SBQ and plain alike: the insert may move the arrays it points into), or a caller-owned device visibility
 * mask (vs_index_set_visibility_dev) is in force — the library cannot grow it; clear or replace it first.  New rows are visible
 * (1) in the library's own mask and invisible (0) in every stored snapshot mask: a snapshot taken before the insert cannot see the
 * tuple.  An insert changes n and may MOVE every array: open vs_scans, scan pools (vs_scanpool_*, whose prefetched round must have
 * been settled — no pool call in flight) and brokers of the index must be ended or rescanned afterwards, pointers taken with
 * vs_index_array asked for again, and a writer opened with vs_pages_out_open / _open_plain closed first; vs_pages_out_* afterwards writes the
 * grown relation.  Not thread safe against any other call on the index.
 * The refusals above (and a growth that fails) leave the index exactly as it was.  An error AFTER the rows were staged — device
 * memory running out for the batch buffers, VS_ERR_CAPACITY from a batch's searches, a HIP error — cannot be undone, because
 * older rows may already name the new nodes: the index then has its n + n_new nodes, label sets and start nodes, with the rows
 * of the unfinished batches unlinked (empty lists: scans do not find them, nothing dangles).  Run the insert's remaining work
 * again by rebuilding (vs_build_graph), or accept the unlinked rows and call vs_index_repair.
 *
 * vs_index_reserve makes room for `capacity` nodes in every per-node array (codes, neighbor lists, heap tids, vectors, cosine
 * divisors, label offsets, the library's visibility masks): allocate, copy device to device on the context's stream, free; a
 * failed growth leaves the index as it was.  vs_index_alloc / vs_index_upload allocate exactly n (capacity == n); an insert that
 * does not fit grows by half, at least to fit. */
int vs_index_reserve(vs_index* idx, uint32_t capacity);
uint32_t vs_index_capacity(const vs_index* idx);
typedef struct vs_insert_stats {
    uint32_t first_node, inserted;         /* the new rows are nodes first_node .. first_node + inserted - 1, in input order */
    uint32_t batches, retries;             /* insert batches run; capacity-overflow relaunches of their searches              */
    uint32_t mate_edges;                   /* out-edges of new nodes that point at a node of the same batch                   */
    uint32_t orphans_placed, orphans_left; /* new nodes the anchoring rule had to place / could not place                     */
    uint32_t grew;                         /* 1 if the arrays were reallocated by this call                                   */
} vs_insert_stats;
/* vectors: host [n_new][dim_full] raw f32; heap_tids [n_new]; label_off [n_new + 1] / label_val: CSR of the rows' sorted,
 * de-duplicated label sets (at most 64 labels per row) for a labeled index, NULL otherwise; batch_max 0 = as vs_build_graph;
 * out may be NULL */
int vs_index_insert(vs_index* idx, const float* vectors, const uint64_t* heap_tids, const uint32_t* label_off, const int16_t* label_val,
                    uint32_t n_new, uint32_t search_list_size, double max_alpha, uint32_t batch_max, vs_insert_stats* out);
/* the same with the vectors already in device memory (d_vectors [n_new][dim_full]; every other argument stays a host pointer) */
int vs_index_insert_dev(vs_index* idx, const float* d_vectors, const uint64_t* heap_tids, const uint32_t* label_off,
                        const int16_t* label_val, uint32_t n_new, uint32_t search_list_size, double max_alpha, uint32_t batch_max,
                        vs_insert_stats* out);
/* HIP-event milliseconds the three insert kernels took on this index since the last reset, collected while vs_profile_enable is on:
 * ms[0] the batch's mates (k_batch_mates, or the plain form on a plain index), ms[1] their merge into the candidate lists, ms[2] the anchoring rounds */
int vs_index_insert_kernel_ms(vs_index* idx, double* ms, int reset);
/* the same for the batch machinery vs_build_graph and vs_index_insert share (SBQ and plain alike): ms[0] the build-mode searches,
 * ms[1] the prune of the new nodes' out-edges, ms[2] the back-edges (sort, segment heads, re-prune per target) */
int vs_index_build_kernel_ms(vs_index* idx, double* ms, int reset);
/* the batch-mates kernel on its own (as vs_hamming_gather / vs_rerank expose theirs): for each of n code rows (host [n][words]) the c
 * (1..64) nearest OTHER rows by (Hamming, row number), ties to the lower row; out_ids / out_ham [n][c], padded with VS_INVALID_NODE
 * (out_ham may be NULL) */
int vs_batch_mates(vs_index* idx, const uint64_t* codes, uint32_t n, uint32_t c, uint32_t* out_ids, uint32_t* out_ham);
/* the form the filtered pass of a labeled insert runs (as vs_scan_topk_filtered is to vs_scan_topk): only rows whose label sets
 * overlap are mates (LabelSetView::overlaps, AM/labels/mod.rs:124-142); label_off [n + 1] / label_val: CSR of the rows' sorted,
 * de-duplicated label sets, at most 64 labels per row; a row without labels has no mates */
int vs_batch_mates_filtered(vs_index* idx, const uint64_t* codes, const uint32_t* label_off, const int16_t* label_val, uint32_t n,
                            uint32_t c, uint32_t* out_ids, uint32_t* out_ham);
/* The two kernels of the plain-storage build on their own, so that they can be pinned exactly; both only read the index (a plain
 * index with its cosine divisors in place: uploaded, built or inserted into; VS_ERR_INVALID otherwise and for the inner product).
 * vs_batch_mates_plain: for rows first_node .. first_node + n - 1 of the index the c (1..64) nearest OTHER rows of that range by
 * (key of d(row -> other), row), ties to the lower row; out_ids [n][c] are row numbers inside the range, padded with
 * VS_INVALID_NODE; out_dist [n][c] (may be NULL) the f32 pair distances, bits 0xFFFFFFFF in the padding.
 * vs_prune_plain: for each of np points what add_neighbors + prune_neighbors make of its candidate set cand_ids[cand_off[i] ..
 * cand_off[i + 1]) (any ids of the index, at most 4096 per point): every id once, never the point, sorted by (key of d(point ->
 * id), id); all of them in that order when they fit num_neighbors, else the alpha ladder 1.0, x1.2 while <= max_alpha with
 * get_factor on d(existing -> candidate).  out_rows [np][num_neighbors] padded with VS_INVALID_NODE, out_len [np]. */
int vs_batch_mates_plain(vs_index* idx, uint32_t first_node, uint32_t n, uint32_t c, uint32_t* out_ids, float* out_dist);
int vs_prune_plain(vs_index* idx, const uint32_t* points, const uint32_t* cand_off, const uint32_t* cand_ids, uint32_t np,
                   double max_alpha, uint32_t* out_rows, uint32_t* out_len);
/* the repair pass of vs_build_graph on its own (after many inserts, at the caller's choice): every node the default start node does
 * not reach is given an in-edge where that strands nobody else; *unreachable (may be NULL) = what vs_index_build_unreachable reports.
 * It treats a tombstone like any node: after vs_index_consolidate_deletes it would hand the dropped tombstones in-edges again. */
int vs_index_repair(vs_index* idx, uint32_t* unreachable);

/* ---- label-filtered reachability: the audit and the repair (what a PGRX shim calls after ambuild, and after amvacuumcleanup's
 * consolidation) ----------------------------------------------------------------------------------------------------------------
 * Build, insert, consolidation and compaction keep every live row reachable from the DEFAULT start node.  A label-filtered scan
 * starts at the start node of each label of its key (StartNodes::get_for_node, AM/graph/start_nodes.rs:39-48) and never enqueues
 * a neighbor whose label set misses the key (AM/sbq/storage.rs:148-172): a row that carries label l is returned under the key {l}
 * only if a path leads to it from l's start node through rows that all carry l.  Single-label keys are the strictest case (a row
 * reached under {l} is reached under every key that contains l).  Definitions, on the graph as it stands:
 *   Node classes are those of vs_index_consolidate_deletes: live (heap offset not 0), kept tombstone (offset 0, but the default
 *   or a per-label start node), dropped tombstone D (every other node with offset 0).
 *   Labels judged: every distinct label of some node's set or of the start map, ascending, in GROUPS of 64.  A label that is
 *   carried but has no start node is not judged (get_for_node gives its key no start at all): it is counted in
 *   labels_without_start and has no bit in what follows.
 *   mask[i]  = the judged labels of the group that node i carries.
 *   reach[i] = the least fixed point of: reach[s_l] holds l for every judged label l of the group, s_l its start node, whether or
 *              not s_l carries l; for every entry u -> v of a neighbor list, reach[v] holds reach[u] & mask[v].  Every node
 *              propagates, dropped tombstones included: scans expand them as long as an edge leads there.
 *   need[x]  = mask[x] & ~reach[x] for a live x, 0 otherwise.  A live x with need[x] != 0 is LOST.
 * vs_index_label_reach is the audit: read-only, works on a view, touches no index array.  out_labels / out_carriers / out_lost
 * (each may be NULL, `cap` entries) receive, per label in ascending order, the label, its live carriers and how many of them are
 * lost (stats.labels of them exist; a label without a start node reports 0 lost); out_node_lost (host, [n], may be NULL): 1 = the
 * node is lost under at least one label.  VS_ERR_INVALID for an index without label sets or neighbor lists, VS_ERR_STATE while a
 * batch of the handle is in flight. */
typedef struct vs_label_reach_stats {
    uint64_t lost_pairs;            /* (row, label) pairs: a live row not reached under a label it carries */
    uint32_t lost_nodes;            /* live rows lost under at least one label */
    uint32_t labels;                /* distinct labels of the node sets and the start map */
    uint32_t labels_without_start;  /* carried labels that have no start node: not judged */
    uint32_t sweeps;                /* launches of the reach sweep */
} vs_label_reach_stats;
int vs_index_label_reach(vs_index* idx, vs_label_reach_stats* out /* may be NULL */, int16_t* out_labels, uint32_t* out_carriers,
                         uint32_t* out_lost, uint32_t cap, uint8_t* out_node_lost);
/* vs_index_repair_labels hands the lost rows in-edges, at the caller's choice (no other call runs it).  One ROUND takes the groups
 * in ascending order, a later group sees what an earlier one wrote.  Per group:
 *   1. reach and need as above; nothing lost: the group is done.
 *   2. strong[y] = the entries q -> y with q not in D and mask[y] & ~reach[q] == 0: in-edges from rows that are themselves
 *      reached under every label y carries in the group.
 *   3. every lost x picks the source p with the least (Hamming(code[x], code[p]) << 32) | p among the nodes p != x, p not in D,
 *      reach[p] & need[x] != 0: the nearest row already reached under a label x still needs (the start node of a needed label
 *      always qualifies).
 *   4. a source serves one node per group and round: of the nodes that picked p the smallest id wins, the others (contended) wait
 *      for the next round.
 *   5. p's row, edited by one writer that reads only p's row and the arrays of steps 1-2: nothing if it names x already; else x
 *      goes into the first free slot (placed_free); else, scanning from the last entry backwards, over the first entry that names
 *      a dropped tombstone (placed_over_dropped); else over the first entry y with strong[y] >= 1 + (mask[y] & ~reach[p] == 0 ? 1
 *      : 0), which keeps another strong in-edge besides this one (placed_victim); else nothing (blocked).  The list keeps its
 *      order otherwise.  Rows of D are never written and no node of D is given an in-edge.
 * Rounds repeat until a round finds nothing lost in any group, or max_rounds (0 = 16, at most 64).  A victim can be stranded when
 * the strong edges of one round vouched for each other; the next round's audit finds it.  Then the audit runs again
 * (lost_*_after: what could not be fixed is reported, never hidden) and one unfiltered sweep from the default start node counts
 * unreachable_live (0xFFFFFFFF: not judged, as elsewhere).
 * Only the neighbor lists are written: n, codes, tids, label sets and start nodes stay; the neighbors' label masks are dropped as
 * an insert drops them.  Open vs_scans, scan pools and brokers of the index must be ended or rescanned afterwards.  An error
 * between rounds leaves a valid graph: every row is either its old or its new list.  No guarantee survives later inserts or
 * deletes: run the audit again.
 * Refusals leave every byte as it was: VS_ERR_INVALID for plain storage, an index without codes / neighbor lists / label sets,
 * unknown flags (none are defined), max_rounds > 64; VS_ERR_STATE for a view handle, live views, a batch in flight or an open
 * vs_pages_out writer. */
typedef struct vs_label_repair_stats {
    uint64_t lost_pairs_before, lost_pairs_after;
    uint64_t placed_free, placed_over_dropped, placed_victim;  /* entries written, by the slot rule that chose them */
    uint64_t blocked;       /* claimed sources whose row had no slot to give (summed over groups and rounds) */
    uint64_t contended;     /* lost nodes that lost the claim on their source and waited a round (summed) */
    uint64_t rows_changed;  /* distinct rows written */
    uint64_t source_tiles;  /* tiles of lost nodes (8, or 4 when at most 4 are lost) the source kernel streamed every code row for */
    uint32_t lost_nodes_before, lost_nodes_after;
    uint32_t rounds;        /* rounds that found something lost */
    uint32_t sweeps;        /* launches of the reach sweep, both audits included */
    uint32_t labels_without_start;
    uint32_t unreachable_live;
} vs_label_repair_stats;
int vs_index_repair_labels(vs_index* idx, uint32_t max_rounds /* 0 = 16 */, uint32_t flags /* 0 */, vs_label_repair_stats* out /* may be NULL */);
/* HIP-event milliseconds on this index since the last reset, collected while vs_profile_enable is on: ms[0] the reach sweeps,
 * ms[1] strong[], ms[2] the source kernel, ms[3] claim + apply */
int vs_index_label_repair_kernel_ms(vs_index* idx, double* ms, int reset);
/* the source kernel on its own (as vs_batch_mates / vs_scan_topk_filtered expose theirs); every argument is a host array.  For
 * each query node nodes[q] the nearest OTHER row p by (Hamming between the two code rows, id) with node_bits[p] & want[q] != 0 and
 * (skip == NULL or skip[p] == 0); out_ids[q] = VS_INVALID_NODE and out_ham[q] = 0xFFFFFFFF when there is none (out_ham may be
 * NULL).  node_bits / skip have one entry per node.  Any code width. */
int vs_nearest_masked(vs_index* idx, const uint32_t* nodes, const uint64_t* want, uint32_t nq, const uint64_t* node_bits,
                      const uint8_t* skip, uint32_t* out_ids, uint32_t* out_ham);

/* ---- synthetic corpora generated in HBM (bench / tests; bit-reproducible on the CPU, see pgvectorscale_amd/datagen.py) */
typedef struct vs_datagen_params {
    uint64_t seed;
    uint32_t dim;          /* vector dimensionality                                   */
    uint32_t latent_dim;   /* intrinsic dimensionality of the mixture                 */
    uint32_t n_clusters;   /* mixture components                                      */
    uint32_t intra_pct;    /* within-cluster latent spread, percent of between-cluster spread */
    uint32_t noise_pct;    /* isotropic ambient noise, percent of signal scale        */
    uint32_t normalize;    /* 1 => unit L2 norm                                       */
} vs_datagen_params;
/* fills d_out[row_begin .. row_begin+rows) (row stride = dim floats) with rows `first_row + i` of the stream */
int vs_datagen_fill(vs_ctx* ctx, const vs_datagen_params* p, uint64_t first_row, uint64_t rows, float* d_out);
/* exact brute-force f32 top-k on the device (ground truth for recall): d_queries [nq][dim_full] raw */
int vs_bruteforce_topk(vs_index* idx, const float* d_queries, uint32_t nq, uint32_t k, uint32_t* out_ids, float* out_dist);

/* ---- qualified scans: the first k rows of a scan that pass a per-scan node bitmap (vs_qual.h) ----
 * `ORDER BY embedding <=> $1 LIMIT k` under an ordinary WHERE clause: the executor post-filters the rows the index returns.  Here the
 * predicate lives on the device as a QUALIFIER, one bit per node, and a batch keeps popping rows until k of them pass.
 *
 * SEMANTICS.  For scan q let r0, r1, ... be the rows the reference returns from successive amgettuple calls after amrescan with the
 * GUCs search_list_size and rescore, under the mask in force on the index (vs_index_set_visibility*, vs_index_snapshot_use): the rows
 * vs_search_batch returns, for any k.  Let Q be the qualifier scan q names.  The qualified scan returns the first k rows r_i with bit
 * node(r_i) set in Q, in that order, with the tid and the distance bits vs_search_batch gives them.  A rejected row is left out AFTER
 * its pop: it has taken its place in the rescore window and has been reranked like any other.  That is why a qualifier is no
 * visibility mask, which hides a row BEFORE the window.  The scan never looks past r_(max_pops - 1).  Per scan:
 *   out_rows[q]   rows returned (<= k); the remaining entries are VS_INVALID_NODE / 0 / NaN, as in vs_search_batch
 *   out_pops[q]   amgettuple calls the reference would have made that returned a row: for a complete scan the index of its k-th
 *                 qualifying row + 1, otherwise the number of rows the scan was taken to
 *   out_state[q]  VS_QUAL_COMPLETE  k rows were returned
 *                 VS_QUAL_ENDED     the scan returned None within max_pops calls, before k rows had passed: every row was looked at
 *                 VS_QUAL_CUT       max_pops rows were looked at, fewer than k passed, and no call had returned None yet
 * Slot 0 is "no qualifier": every node passes, and the rows are the first k rows of vs_search_batch bit for bit.
 *
 * QUALIFIERS.  Slots 1 .. VS_MAX_QUAL_SLOTS of an index hold one bit per node, node i at bit (i & 63) of word (i >> 6), in device
 * memory allocated at the index's capacity.  vs_index_qual_put takes (n + 63) / 64 HOST words, _put_dev DEVICE words; bits at
 * positions >= n are cleared by the library whatever the caller left there.  vs_index_qual_from_tids sets the bit of every LIVE node
 * (tid offset != 0) whose heap tid is in the list — (block << 16) | offset, unsorted, duplicates allowed, the convention of
 * vs_index_bulk_delete; _from_tids_dev takes a DEVICE array sorted ascending (duplicates allowed).  vs_qual_info: n_nodes the nodes
 * of the index when the slot was filled, n_set the bits set, tids_unmatched the distinct tids of the list that no live node carries
 * (0 after a _put).  vs_index_qual_info reads the record of a slot, vs_index_qual_drop frees it (VS_ERR_STATE for an empty slot).
 * LIFETIME: vs_index_reserve and growing inserts carry the qualifiers over, rows added later read 0 and do not qualify;
 * vs_index_compact renumbers the nodes and DROPS every qualifier (one that VS_COMPACT_KEEP_EDGES_CHECK refuses drops none: every byte
 * stays as it was).  Refusals, each before anything is written: NULL arguments, slot 0
 * or a slot > VS_MAX_QUAL_SLOTS (VS_ERR_INVALID); a view handle, a batch of the handle in flight (VS_ERR_STATE).
 *
 * THE BATCH.  vs_search_batch_qual(.., k, qual_slots [nq] HOST, max_pops, ..): max_pops in [k, VS_QUAL_MAX_POPS] and qual_slots != NULL,
 * else VS_ERR_INVALID (the unqualified calls exist for that); a slot > VS_MAX_QUAL_SLOTS is VS_ERR_INVALID and an empty slot
 * VS_ERR_STATE, before anything is launched.  Owner handles only.  A scan needs an unknown number of pops, so the batch runs in
 * ROUNDS: round 1 takes every scan to P1 pops, the scans that are neither complete nor ended are gathered and re-run from the start
 * at twice the pops, up to max_pops (the row sequence is prefix-consistent in the number of pops, so a re-run is exact).  P1 follows
 * from the density of the sparsest qualifier named, n_set / n: ceil(k / density) plus two standard deviations of that count, clamped to
 * [k, max_pops] (max_pops for an empty qualifier); the option VS_QUAL_FIRST_POPS overrides it.  The rule is a cost choice: no row,
 * count or state depends on it.  A round is the batch pipeline of vs_search_batch_dev with a stream long enough for P pops — the
 * planners see the longer stream as they would for a larger k — whose rescore window (k_rerank_window_qual, or k_resort_qual for
 * windows the fused kernel does not take, VS_RERANK_FUSED "0" and rescore == 0) reads the popped node's bit after each pop, keeps
 * the row if it is set and stops at k kept rows.  A batch whose slots are all 0 launches what vs_search_batch_dev launches
 * (vs_index_last_search_info is equal), straight into the caller's rows.  vs_qual_batch_stats: rounds run, first_pops (P1), scans_rerun (scans of rounds 2 ..), pops_launched (sum over rounds
 * of scans x P) and the scans per final state.  *stats accumulates the DEVICE's work over all rounds, re-runs included, as it does
 * over capacity retries: it is not the reference's GreedySearchStats of the qualified scan.
 * vs_search_batch_dev_qual takes DEVICE queries, label keys (sorted and de-duplicated per query, as vs_search_batch_dev), slots and
 * outputs (all of which stay valid until the finish); it checks the arguments and launches round 1;
 * vs_search_batch_dev_qual_finish runs the remaining rounds and fills the outputs.  Scan pools take qualifiers through
 * vs_scanpool_fetch_qual (below).  Per-scan visibility slots together with qualifiers, and the single cursor (vs_gettuple), the broker,
 * the shm server and vs_multi with qualifiers are not built. */
#define VS_MAX_QUAL_SLOTS 64
#define VS_QUAL_MAX_POPS 65536
enum { VS_QUAL_COMPLETE = 0, VS_QUAL_ENDED = 1, VS_QUAL_CUT = 2 };
typedef struct vs_qual_info {
    uint64_t n_nodes;
    uint64_t n_set;
    uint64_t tids_unmatched;
} vs_qual_info;
typedef struct vs_qual_batch_stats {
    uint64_t rounds;
    uint64_t first_pops;
    uint64_t scans_rerun;
    uint64_t pops_launched;
    uint64_t complete, ended, cut;
} vs_qual_batch_stats;
int vs_index_qual_put(vs_index* idx, uint32_t slot, const uint64_t* bits);
int vs_index_qual_put_dev(vs_index* idx, uint32_t slot, const uint64_t* d_bits);
int vs_index_qual_from_tids(vs_index* idx, uint32_t slot, const uint64_t* heap_tids, size_t n_tids, vs_qual_info* info /* may be NULL */);
int vs_index_qual_from_tids_dev(vs_index* idx, uint32_t slot, const uint64_t* d_heap_tids_sorted, size_t n_tids, vs_qual_info* info);
int vs_index_qual_info(const vs_index* idx, uint32_t slot, vs_qual_info* info);
int vs_index_qual_get(vs_index* idx, uint32_t slot, uint64_t* bits /* host, (n + 63) / 64 words */);
int vs_index_qual_drop(vs_index* idx, uint32_t slot);
int vs_search_batch_qual(vs_index* idx, const float* queries, const int16_t* qlabels, const uint32_t* qlabel_off, uint32_t nq,
                         uint32_t search_list_size, uint32_t rescore, uint32_t k, const uint32_t* qual_slots, uint32_t max_pops,
                         uint32_t* out_ids, uint64_t* out_tids, float* out_dist, uint32_t* out_rows, uint32_t* out_pops,
                         uint32_t* out_state, vs_stats* stats, vs_qual_batch_stats* qstats);
int vs_search_batch_dev_qual(vs_index* idx, const float* d_queries, const int16_t* d_qlabels, const uint32_t* d_qlabel_off, uint32_t nq,
                             uint32_t search_list_size, uint32_t rescore, uint32_t k, const uint32_t* d_qual_slots, uint32_t max_pops,
                             uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, uint32_t* d_out_rows, uint32_t* d_out_pops,
                             uint32_t* d_out_state);
int vs_search_batch_dev_qual_finish(vs_index* idx, vs_stats* stats, vs_qual_batch_stats* qstats);

/* ---- qualified scan pools: a pooled scan continued to its next k qualifying rows (vs_scanpool.cpp) ----
 * vs_search_batch_qual is one-shot: it re-runs a scan that has not finished at P pops from the start at 2 P, and a scan that comes
 * back VS_QUAL_CUT can only be taken further by running it again.  A scan pool continues its scans on the device and never re-runs
 * one, so here a qualified scan costs the pops it needs, a CUT scan is resumable, and the next k qualifying rows — `FETCH k` from a
 * cursor over `ORDER BY embedding <=> $1 ... WHERE ...` — are one call.
 *
 * SEMANTICS.  Let slot s have made c amgettuple calls so far, those of earlier vs_scanpool_fetch AND vs_scanpool_fetch_qual calls
 * alike: the two share one cursor and may be interleaved freely.  The call makes the reference's calls c, c + 1, ... and stops at the
 * first of four events: k of the returned rows have their node's bit set in qualifier qual_slots[i] (0: every node passes); a call
 * returns None; max_pops calls of THIS fetch have returned a row; the pool's row budget is reached.  The rows that pass are returned
 * in that order with the tid and the distance bits vs_scanpool_fetch would have given them.  A rejected row is consumed: it was
 * reranked, it held its place in the rescore window, and it counts as a call.  Per listed slot:
 *   out_rows[i]   rows returned (<= k), or a negative VS_ERR_* as in vs_scanpool_fetch (that scan failed, the others are served);
 *                 entries past out_rows[i] are not written, as in vs_scanpool_fetch
 *   out_pops[i]   calls of this fetch that returned a row
 *   out_state[i]  VS_QUAL_COMPLETE  k rows were returned
 *                 VS_QUAL_ENDED     a call returned None.  That call is booked as vs_scanpool_fetch books it; a further fetch_qual of the
 *                                   slot returns 0 rows, 0 pops and ENDED (and books one more such call)
 *                 VS_QUAL_CUT       max_pops rows were looked at in this fetch; the next fetch goes on from there
 *                 VS_QUAL_BUDGET    the scan has not been seen to end and its next pop would stand on more than rows_cap stream rows:
 *                                   the rows kept so far are returned, the cursor has advanced by out_pops, and any later fetch of the
 *                                   slot returns VS_ERR_CAPACITY, as it does today.  A slot that can make no pop at all returns
 *                                   VS_ERR_CAPACITY at once.
 * After any sequence of fetch and fetch_qual calls vs_scanpool_get_stats equals the reference scan's GreedySearchStats after the same
 * amgettuple calls (the counters are per emitted stream row: stream rows carried ahead do not show).  A fetch whose slots are all 0
 * returns vs_scanpool_fetch's rows bit for bit, with pops = rows.
 *
 * HOW.  Per listed scan a pop target P starts at P1 — the rule of vs_search_batch_qual from the density of the scan's OWN qualifier,
 * VS_QUAL_FIRST_POPS overrides it — clamped to what max_pops and the row budget allow.  The pool's rounds (shared resumed search
 * launches, a prefetched round included) bring every unfinished scan to the stream rows P pops stand on, one window launch
 * (k_resort_cursor_batch_qual, a wave per scan) pops past the rejected rows, only the small per-scan records come back, and scans
 * that are neither final nor at their limit go on at 2 P.  The rows are copied back once, at the end.  Nothing is re-run.  P1 and
 * VS_POOL_QUAL_CHUNK (the pops one window launch may make) are cost choices: no row, count or state depends on them.
 *
 * REFUSALS, each before anything is launched or any cursor moves: NULL slots, qual_slots, out_rows, out_pops or out_state; k outside
 * [1, kmax]; max_pops outside [k, VS_QUAL_MAX_POPS]; a qualifier slot > VS_MAX_QUAL_SLOTS (all VS_ERR_INVALID); an empty qualifier
 * slot, a pool on a view handle that names a non-zero slot (VS_ERR_STATE); a pool slot that is not open or is listed twice.
 * vs_pool_qual_stats covers this call only: search rounds waited for, window launches, the largest P1 of the listed scans, the pops
 * made, and the scans per final state.
 * Not built: qualifiers in the broker, the shm server, vs_multi and the single cursor (vs_gettuple), and per-scan visibility slots in
 * pools. */
#define VS_QUAL_BUDGET 3
typedef struct vs_pool_qual_stats {
    uint64_t search_rounds;
    uint64_t window_launches;
    uint64_t first_pops;
    uint64_t pops;
    uint64_t complete, ended, cut, budget;
} vs_pool_qual_stats;
int vs_scanpool_fetch_qual(vs_scan_pool* pool, const uint32_t* slots, uint32_t n, uint32_t k,
                           const uint32_t* qual_slots /* [n] host, 0 = no qualifier */, uint32_t max_pops,
                           uint64_t* out_tids, uint32_t* out_ids, float* out_dist,   /* [n][k], may be NULL */
                           int32_t* out_rows, uint32_t* out_pops, uint32_t* out_state, /* [n] */
                           vs_pool_qual_stats* qstats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* VSGPU_H */
