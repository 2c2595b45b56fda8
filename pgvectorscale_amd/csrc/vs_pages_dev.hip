// vs_pages_dev.hip — index relation pages decoded ON the device (the MI355X-first form of the staging path).
//
// vs_pages.cpp decodes SbqNode items on the host cores and uploads flat arrays.  Here the host only copies: the blocks of
// the relation go through the pinned ring to HBM as they are (hipMemcpyAsync), the host keeps nothing but the block table
// it reads off the page headers on the way past (page type + item count per block -> dense id of each block's first
// node; vs_pages_headers_only) and copies of the few metadata pages, and one kernel — a wave per node page — walks the
// line pointers, follows the rkyv relative pointers of every archived node (same layout facts and the same bounds checks
// as the host reader, vs_pages.cpp) and writes codes / neighbor ids / heap tids straight into the index arrays, neighbor
// IndexPointers translated through the block table.  33 GB of pages for a 50M-node index is 0.6 s of PCIe instead of
// tens of seconds of host decoding.  Label sets (LabeledSbqNode) take two more passes over the staged pages: count, then copy.
#include <algorithm>
#include <vector>

#include "vs_device.h"
#include "vs_pages_out.h"

struct vs_pages_dev {
    vs_ctx* ctx = nullptr;
    vs_pages* hdr = nullptr;  // host side: block table + metadata pages
    uint8_t* d_pages = nullptr;
    uint32_t page_size = VS_BLCKSZ;
    uint32_t cap_blocks = 0, n_blocks = 0;
    vs_node_layout lay{};
    bool layout_given = false;
};

enum { PE_OK = 0, PE_LINE_POINTER = 1, PE_ITEM_BOUNDS = 2, PE_SHORT_ITEM = 3, PE_VEC_BOUNDS = 4, PE_CODE_WIDTH = 5, PE_NEIGHBOR_SLOTS = 6,
       PE_DANGLING = 7, PE_LABELS = 8, PE_LABELS_CHANGED = 9, PE_VECTOR_DIM = 10, PE_DANGLING_PLAIN = 11, PE_UNALIGNED = 12, PE_LAST = PE_UNALIGNED };
static const char* const kPageErrorText[] = {"", "line pointer is not LP_NORMAL", "item lies outside pd_upper..pd_special",
                                             "item shorter than the archived node", "ArchivedVec points outside the item",
                                             "bq_vector length differs from the index's code width",
                                             "neighbor slot count differs from the index's num_neighbors",
                                             "neighbor points at something that is not an SbqNode item of this relation",
                                             "label set is not strictly increasing", "label set of an existing node changed",
                                             "vector length differs from the index's dimensions",
                                             "neighbor points at something that is not a PlainNode item of this relation",
                                             "item or ArchivedVec is not 4-byte aligned"};
static_assert(sizeof kPageErrorText / sizeof kPageErrorText[0] == PE_LAST + 1, "one text per reason code");

__device__ __forceinline__ uint32_t ld16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) {  // items are MAXALIGNed: 4-byte aligned words
    return *reinterpret_cast<const uint32_t*>(p);
}

#include "vs_heap_dev.h"  // vs_heap_dev_*: the heap's vector column from heap and TOAST pages (kernels and their host code)
#include "vs_heap_vis.h"  // vs_heap_res_*, vs_index_snapshot_eval: heap visibility from a resident copy of the heap's main fork

// err[0] = first error code (0 = none), err[1] = block, err[2] = item, err[3] = detail
__device__ __forceinline__ void page_error(uint32_t* err, uint32_t code, uint32_t blk, uint32_t item, uint32_t detail) {
    if (atomicCAS(&err[0], 0u, code) == 0u) {
        err[1] = blk;
        err[2] = item;
        err[3] = detail;
    }
}

// Where item `off` of a page lies and what every reader of it may rely on: PageGetItemId / PageGetItem (UT/ports.rs:56-77) with the
// bounds the reference leaves to PostgreSQL, and room for the archived root (rkyv::archived_root: the root object is the tail of
// the item).  Shared by k_pages_decode and k_pages_follow.  -> PE_OK, or the reason with its detail word.
struct PageItem {
    const uint8_t* item;
    uint32_t len, root;
};
__device__ __forceinline__ uint32_t page_item_at(const uint8_t* page, uint32_t upper, uint32_t special, uint32_t off, uint32_t root_size,
                                                 PageItem& it, uint32_t& detail) {
    const uint32_t lp = ld32(page + 24 + 4 * (off - 1));
    const uint32_t lp_off = lp & 0x7FFFu, lp_flags = (lp >> 15) & 3u, len = lp >> 17;
    detail = lp;
    if (lp_flags != 1u || len == 0) return PE_LINE_POINTER;
    if (lp_off < upper || lp_off + len > special) return PE_ITEM_BOUNDS;
    if (lp_off & 3u) return PE_UNALIGNED;  // (the host reader memcpys and accepts; ld32 here is an aligned dword load)
    detail = len;
    if (len < root_size) return PE_SHORT_ITEM;
    it.item = page + lp_off;
    it.len = len;
    it.root = len - root_size;
    return PE_OK;
}
// ArchivedVec<8-byte element> = {i32 offset relative to the field, u32 len} at byte `field_off` of the root: `want` elements (else
// `mismatch`), all of them inside the item.  tgt = where the first element starts.
__device__ __forceinline__ uint32_t page_item_vec8(const PageItem& it, uint32_t field_off, uint32_t want, uint32_t mismatch, int64_t& tgt,
                                                   uint32_t& detail) {
    const uint32_t fld = it.root + field_off;
    tgt = (int64_t)fld + (int32_t)ld32(it.item + fld);
    const uint32_t n = ld32(it.item + fld + 4);
    detail = n;
    if (n != want) return mismatch;
    detail = fld;
    if (tgt < 0 || (uint64_t)tgt + (uint64_t)n * 8 > it.len) return PE_VEC_BOUNDS;
    if (tgt & 3) return PE_UNALIGNED;
    return PE_OK;
}

// The same for an ArchivedVec<4-byte element> (PlainNode.vector: f32): `want` elements, all of them inside the item, 4-byte aligned.
__device__ __forceinline__ uint32_t page_item_vec4(const PageItem& it, uint32_t field_off, uint32_t want, uint32_t mismatch, int64_t& tgt,
                                                   uint32_t& detail) {
    const uint32_t fld = it.root + field_off;
    tgt = (int64_t)fld + (int32_t)ld32(it.item + fld);
    const uint32_t n = ld32(it.item + fld + 4);
    detail = n;
    if (n != want) return mismatch;
    detail = fld;
    if (tgt < 0 || (uint64_t)tgt + (uint64_t)n * 4 > it.len) return PE_VEC_BOUNDS;
    if (tgt & 3) return PE_UNALIGNED;
    return PE_OK;
}

// one wave per block; blocks that hold no SbqNode items are skipped
__global__ __launch_bounds__(WAVE) void k_pages_decode(const uint8_t* __restrict__ pages, uint32_t page_size, uint32_t n_blocks,
                                                       const uint32_t* __restrict__ blk_base, const uint32_t* __restrict__ blk_cnt,
                                                       vs_node_layout lay, uint32_t W, uint32_t R, uint64_t* __restrict__ codes,
                                                       uint32_t code_stride, uint32_t* __restrict__ nbrs, uint32_t nbr_stride,
                                                       uint64_t* __restrict__ tids, uint32_t* __restrict__ err) {
    const int lane = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const uint32_t cnt = blk_cnt[b];
        if (cnt == 0) continue;
        const uint8_t* page = pages + (size_t)b * page_size;
        const uint32_t upper = ld16(page + 14), special = ld16(page + 16);
        for (uint32_t off = 1; off <= cnt; ++off) {
            const uint32_t node = blk_base[b] + off - 1;
            PageItem it;
            uint32_t detail;
            int64_t tgt;
            uint32_t pe = page_item_at(page, upper, special, off, lay.root_size, it, detail);
            if (pe != PE_OK) {
                if (lane == 0) page_error(err, pe, b, off, detail);
                continue;
            }
            const uint8_t* item = it.item;
            // heap_item_pointer
            if (lane == 0) {
                const uint8_t* hp = item + it.root + lay.off_heap_item_pointer;
                tids[node] = ((uint64_t)ld32(hp) << 16) | ld16(hp + 4);
            }
            // bq_vector: ArchivedVec<u64>
            pe = page_item_vec8(it, lay.off_bq_vector, W, PE_CODE_WIDTH, tgt, detail);
            if (pe != PE_OK) {
                if (lane == 0) page_error(err, pe, b, off, detail);
                continue;
            }
            for (uint32_t w = lane; w < W; w += WAVE) {
                const uint8_t* src = item + tgt + 8 * w;
                codes[(size_t)node * code_stride + w] = (uint64_t)ld32(src) | ((uint64_t)ld32(src + 4) << 32);
            }
            // neighbor_index_pointers: ArchivedVec<ArchivedItemPointer {u32 block, u16 offset, pad}>, the list ends at the
            // first InvalidBlockNumber (AM/sbq/node.rs:260-285)
            pe = page_item_vec8(it, lay.off_neighbor_index_pointers, R, PE_NEIGHBOR_SLOTS, tgt, detail);
            if (pe != PE_OK) {
                if (lane == 0) page_error(err, pe, b, off, detail);
                continue;
            }
            bool ended = false;
            for (uint32_t j0 = 0; j0 < R && !ended; j0 += WAVE) {
                const uint32_t j = j0 + (uint32_t)lane;
                uint32_t nb = 0xFFFFFFFFu, no = 0;
                if (j < R) {
                    nb = ld32(item + tgt + 8 * j);
                    no = ld16(item + tgt + 8 * j + 4);
                }
                const uint64_t inval = __ballot(nb == 0xFFFFFFFFu);
                const uint32_t nvalid = inval ? (uint32_t)__builtin_ctzll(inval) : WAVE;
                if (nvalid < WAVE) ended = true;
                if ((uint32_t)lane < nvalid) {
                    if (nb >= n_blocks || no < 1 || no > blk_cnt[nb]) page_error(err, PE_DANGLING, b, off, j);
                    else nbrs[(size_t)node * nbr_stride + j] = blk_base[nb] + no - 1;
                }
            }
        }
    }
}

// LabeledSbqNode.labels (ArchivedLabelSet = ArchivedVec<i16>, sorted and de-duplicated, AM/labels/mod.rs:15-37): WRITE = false
// counts the labels of every node (and checks them), WRITE = true copies them to label_val[label_off[node] ..].  The items
// were located and bounds-checked by k_pages_decode before.
template <bool WRITE>
__global__ __launch_bounds__(WAVE) void k_pages_labels(const uint8_t* __restrict__ pages, uint32_t page_size, uint32_t n_blocks,
                                                       const uint32_t* __restrict__ blk_base, const uint32_t* __restrict__ blk_cnt,
                                                       vs_node_layout lay, uint32_t* __restrict__ label_cnt,
                                                       const uint32_t* __restrict__ label_off, int16_t* __restrict__ label_val,
                                                       uint32_t* __restrict__ err) {
    const int lane = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const uint32_t cnt = blk_cnt[b];
        if (cnt == 0) continue;
        const uint8_t* page = pages + (size_t)b * page_size;
        for (uint32_t off = 1; off <= cnt; ++off) {
            const uint32_t node = blk_base[b] + off - 1;
            const uint32_t lp = ld32(page + 24 + 4 * (off - 1));
            const uint32_t lp_off = lp & 0x7FFFu, len = lp >> 17;
            const uint8_t* item = page + lp_off;
            const uint32_t fld = len - lay.root_size + lay.off_labels;
            const int64_t tgt = (int64_t)fld + (int32_t)ld32(item + fld);
            const uint32_t n = ld32(item + fld + 4);
            if (n && (tgt < 0 || (uint64_t)tgt + (uint64_t)n * 2 > len || (tgt & 1))) {
                if (lane == 0) page_error(err, PE_VEC_BOUNDS, b, off, fld);
                if (!WRITE && lane == 0) label_cnt[node] = 0;
                continue;
            }
            if (!WRITE) {
                for (uint32_t j = 1 + (uint32_t)lane; j < n; j += WAVE)
                    if ((int16_t)ld16(item + tgt + 2 * j) <= (int16_t)ld16(item + tgt + 2 * j - 2)) page_error(err, PE_LABELS, b, off, j);
                if (lane == 0) label_cnt[node] = n;
            } else {
                const uint32_t o = label_off[node];
                for (uint32_t j = lane; j < n; j += WAVE) label_val[o + j] = (int16_t)ld16(item + tgt + 2 * j);
            }
        }
    }
}

extern "C" int vs_pages_dev_open(vs_ctx* ctx, uint32_t page_size, const vs_node_layout* layout, uint32_t n_blocks_total,
                                 vs_pages_dev** out) {
    VS_REQUIRE(ctx && out, "vs_pages_dev_open: bad args");
    *out = nullptr;
    vs_pages_dev* d = new vs_pages_dev();
    d->ctx = ctx;
    d->page_size = page_size;
    int r = vs_pages_open(page_size, 0, layout, 1, &d->hdr);
    if (r == VS_OK) r = vs_pages_headers_only(d->hdr);
    if (r != VS_OK) {
        vs_pages_close(d->hdr);
        delete d;
        return r;
    }
    d->layout_given = layout != nullptr;
    if (layout) d->lay = *layout;
    else vs_node_layout_default(0, &d->lay);
    d->cap_blocks = std::max<uint32_t>(n_blocks_total, 1);
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc(&d->d_pages, (size_t)d->cap_blocks * page_size);
    if (e != hipSuccess) {
        vs_set_error("vs_pages_dev_open: %zu bytes for the raw pages: %s", (size_t)d->cap_blocks * page_size, hipGetErrorString(e));
        vs_pages_close(d->hdr);
        delete d;
        return e == hipErrorOutOfMemory ? VS_ERR_OOM : VS_ERR_HIP;
    }
    *out = d;
    return VS_OK;
}

extern "C" void vs_pages_dev_close(vs_pages_dev* d) {
    if (!d) return;
    if (d->d_pages) (void)hipFree(d->d_pages);
    vs_pages_close(d->hdr);
    delete d;
}

extern "C" int vs_pages_dev_add(vs_pages_dev* d, uint32_t first_block, const void* pages, uint32_t n_blocks) {
    VS_REQUIRE(d && (pages || !n_blocks), "vs_pages_dev_add: bad args");
    VS_REQUIRE(d->d_pages, "vs_pages_dev_add after vs_pages_dev_build");
    VS_REQUIRE((uint64_t)first_block + n_blocks <= d->cap_blocks, "vs_pages_dev_add: more blocks than vs_pages_dev_open was told (%u)",
               d->cap_blocks);
    VS_TRY(vs_pages_add(d->hdr, first_block, pages, n_blocks));  // header checks, block table, metadata pages (host)
    VS_TRY(vs_dev_upload(d->ctx, d->d_pages + (size_t)first_block * d->page_size, pages, (size_t)n_blocks * d->page_size));
    d->n_blocks = first_block + n_blocks;
    return VS_OK;
}

extern "C" int vs_pages_dev_node_of(const vs_pages_dev* d, uint32_t block, uint32_t offset, uint32_t* node) {
    VS_REQUIRE(d, "vs_pages_dev_node_of: null reader");
    return vs_pages_node_of(d->hdr, block, offset, node);
}

extern "C" int vs_pages_dev_sbq_means(const vs_pages_dev* d, uint32_t block, uint32_t offset, float* mean, float* m2, uint32_t dim_cap,
                                      uint32_t* dim, uint64_t* count) {
    VS_REQUIRE(d, "vs_pages_dev_sbq_means: null reader");
    return vs_pages_sbq_means(d->hdr, block, offset, mean, m2, dim_cap, dim, count);
}

extern "C" int vs_pages_dev_meta(vs_pages_dev* d, const vs_meta_layout* layout, vs_meta_page* meta, vs_index_desc* desc,
                                 int16_t* start_labels, uint32_t* start_nodes, uint32_t cap) {
    VS_REQUIRE(d, "vs_pages_dev_meta: null reader");
    VS_TRY(vs_pages_finish(d->hdr, nullptr));  // (block table complete: every block has been added)
    return vs_pages_meta(d->hdr, layout, meta, desc, start_labels, start_nodes, cap);
}

// desc: the MetaPage fields (n is taken from the pages); extras: vecs / mean / m2 / count / start-node arrays (node ids)
extern "C" int vs_pages_dev_build(vs_pages_dev* d, const vs_index_desc* desc, const vs_index_host* extras, vs_pages_info* info,
                                  vs_index** out) {
    VS_REQUIRE(d && desc && extras && out, "vs_pages_dev_build: bad args");
    VS_REQUIRE(d->d_pages, "vs_pages_dev_build: already built");
    if (!d->layout_given) vs_node_layout_default(desc->has_labels ? 1 : 0, &d->lay);
    VS_REQUIRE(!desc->has_labels || (d->lay.off_labels <= d->lay.root_size && d->lay.root_size - d->lay.off_labels >= 8),
               "vs_pages_dev_build: the node layout has no labels field");
    VS_REQUIRE(desc->storage_type == VS_STORAGE_SBQ, "vs_pages_dev_build: memory_optimized (SBQ) indexes only");
    *out = nullptr;
    vs_pages_info pi{};
    VS_TRY(vs_pages_finish(d->hdr, &pi));
    if (info) *info = pi;
    VS_REQUIRE(pi.n_nodes > 0 || pi.pages_by_type[VS_PAGE_NODE] == 0,
               "the relation holds `plain` storage nodes (PageType::Node); this path reads memory_optimized (SBQ) indexes");
    vs_ctx* c = d->ctx;
    VS_HIP(hipSetDevice(c->device));
    vs_index_desc dd = *desc;
    dd.n = pi.n_nodes;
    vs_index* ix = nullptr;
    VS_TRY(vs_index_alloc(c, &dd, extras->vecs != nullptr, &ix));  // neighbor rows start as all-sentinel, codes as zero
    const uint32_t *h_base = nullptr, *h_cnt = nullptr;
    uint32_t nb = 0;
    uint32_t *d_base = nullptr, *d_cnt = nullptr, *d_err = nullptr;
    int r = vs_pages_block_table(d->hdr, &h_base, &h_cnt, &nb);
    auto hip_ok = [&](hipError_t e, const char* what) {
        if (r == VS_OK && e != hipSuccess) {
            vs_set_error("vs_pages_dev_build: %s: %s", what, hipGetErrorString(e));
            r = e == hipErrorOutOfMemory ? VS_ERR_OOM : VS_ERR_HIP;
        }
    };
    uint32_t herr[4] = {0, 0, 0, 0};
    if (r == VS_OK && nb > 0 && pi.n_nodes > 0) {
        hip_ok(hipMalloc(&d_base, (size_t)nb * 4), "block table");
        hip_ok(hipMalloc(&d_cnt, (size_t)nb * 4), "block table");
        hip_ok(hipMalloc(&d_err, 16), "error record");
        if (r == VS_OK) r = vs_dev_upload(c, d_base, h_base, (size_t)nb * 4);
        if (r == VS_OK) r = vs_dev_upload(c, d_cnt, h_cnt, (size_t)nb * 4);
        if (r == VS_OK) hip_ok(hipMemsetAsync(d_err, 0, 16, c->stream), "error record");
        if (r == VS_OK) {
            const uint32_t grid = std::min<uint32_t>(nb, 1u << 20);
            hipLaunchKernelGGL(k_pages_decode, dim3(grid), dim3(WAVE), 0, c->stream, d->d_pages, d->page_size, nb, d_base, d_cnt,
                               d->lay, dd.words, dd.num_neighbors, ix->codes, ix->code_stride, ix->nbrs, ix->nbr_stride, ix->tids,
                               d_err);
            hip_ok(hipGetLastError(), "k_pages_decode");
            ix->codes_epoch++;
            hip_ok(hipMemcpyAsync(herr, d_err, 16, hipMemcpyDeviceToHost, c->stream), "error record");
            hip_ok(hipStreamSynchronize(c->stream), "k_pages_decode");
        }
    }
    // labels: count per node, prefix sum on the host (4 bytes per node), then the values
    if (r == VS_OK && herr[0] == PE_OK && desc->has_labels && pi.n_nodes > 0) {
        const uint32_t n = pi.n_nodes;
        const uint32_t grid = std::min<uint32_t>(nb, 1u << 20);
        uint32_t* d_lcnt = nullptr;
        hip_ok(hipMalloc(&d_lcnt, (size_t)n * 4), "label counts");
        if (r == VS_OK) {
            hipLaunchKernelGGL((k_pages_labels<false>), dim3(grid), dim3(WAVE), 0, c->stream, d->d_pages, d->page_size, nb, d_base, d_cnt,
                               d->lay, d_lcnt, (const uint32_t*)nullptr, (int16_t*)nullptr, d_err);
            hip_ok(hipGetLastError(), "k_pages_labels");
        }
        std::vector<uint32_t> off((size_t)n + 1, 0);
        if (r == VS_OK) r = vs_dev_download(c, off.data() + 1, d_lcnt, (size_t)n * 4);
        if (r == VS_OK) hip_ok(hipMemcpy(herr, d_err, 16, hipMemcpyDeviceToHost), "error record");
        if (d_lcnt) (void)hipFree(d_lcnt);
        if (r == VS_OK && herr[0] == PE_OK) {
            uint64_t tot = 0;
            for (uint32_t i = 0; i < n; ++i) {
                tot += off[i + 1];
                off[i + 1] = (uint32_t)tot;
            }
            if (tot >= 0xFFFFFFFFull) {
                vs_set_error("label CSR exceeds 2^32 entries");
                r = VS_ERR_INVALID;
            }
            if (r == VS_OK) {
                hip_ok(hipMalloc(&ix->label_off, ((size_t)n + 1) * 4), "label offsets");
                hip_ok(hipMalloc(&ix->label_val, std::max<uint64_t>(tot, 1) * 2), "label values");
            }
            if (r == VS_OK) r = vs_dev_upload(c, ix->label_off, off.data(), ((size_t)n + 1) * 4);
            if (r == VS_OK) {
                hipLaunchKernelGGL((k_pages_labels<true>), dim3(grid), dim3(WAVE), 0, c->stream, d->d_pages, d->page_size, nb, d_base,
                                   d_cnt, d->lay, (uint32_t*)nullptr, (const uint32_t*)ix->label_off, ix->label_val, d_err);
                hip_ok(hipGetLastError(), "k_pages_labels");
                hip_ok(hipStreamSynchronize(c->stream), "k_pages_labels");
                ix->n_label_vals = tot;
                ix->d.has_labels = 1;
                if (r == VS_OK) r = vs_refresh_label_masks(ix);
            }
        }
    }
    if (d_base) (void)hipFree(d_base);
    if (d_cnt) (void)hipFree(d_cnt);
    if (d_err) (void)hipFree(d_err);
    if (r == VS_OK && herr[0] != PE_OK) {
        vs_set_error("block %u item %u: %s (detail %u)", herr[1], herr[2], kPageErrorText[herr[0] <= PE_LAST ? herr[0] : 0], herr[3]);
        r = VS_ERR_INVALID;
    }
    // the raw pages are no longer needed
    (void)hipFree(d->d_pages);
    d->d_pages = nullptr;
    if (r == VS_OK && extras->vecs) {
        void* dv = nullptr;
        uint32_t stride = 0;
        r = vs_index_array(ix, VS_ARR_VECS, &dv, &stride);
        if (r == VS_OK) r = vs_upload_rows(c, dv, (size_t)stride * 4, extras->vecs, (size_t)dd.dim_full * 4, (size_t)dd.dim_full * 4, dd.n);
    }
    if (r == VS_OK && extras->mean) r = vs_index_set_quantizer(ix, extras->mean, extras->m2, extras->count);
    if (r == VS_OK)
        r = vs_index_set_start_nodes(ix, desc->default_start, extras->label_start_labels, extras->label_start_nodes, desc->n_label_starts);
    if (r == VS_OK) r = vs_validate_graph(ix);
    if (r == VS_OK) r = vs_index_refresh_norms(ix);
    if (r != VS_OK) {
        vs_index_free(ix);
        return r;
    }
    *out = ix;
    return VS_OK;
}

extern "C" int vs_pages_dev_block_table(const vs_pages_dev* d, const uint32_t** blk_base, const uint32_t** blk_cnt, uint32_t* n_blocks) {
    VS_REQUIRE(d, "vs_pages_dev_block_table: null reader");
    return vs_pages_block_table(d->hdr, blk_base, blk_cnt, n_blocks);
}

// ---------------------------------------------------------------------------------------------------------------
// Following a relation that something else writes (vs_pages_follow_*): the blocks that changed, scattered into the resident arrays.
//
// The reference only ever appends nodes at the end of the relation (Tape), patches neighbor lists in place at unchanged item size
// and clears heap offsets in place, so a node id — SbqNode items on earlier blocks + offset - 1 — never moves as long as item
// counts grow only where no node page follows (the rule vs_pages_follow_stage enforces on the page headers).  k_pages_follow takes
// its pages from the staged list (slot i holds block blocks[i]), locates and checks every item as k_pages_decode does, translates
// neighbor pointers through the NEW block table, and splits at n_before: WRITE = false compares an existing node with the resident
// row (one ballot per row kind, one atomic per wave and counter at the end) and leaves an appended node's heap tid in new_tids;
// WRITE = true scatters.  Listed pages are distinct and a node lives on one page: the write pass has no race and no atomically
// assigned slot.
// ---------------------------------------------------------------------------------------------------------------
enum { FC_RELINKED = 0, FC_TIDS_CLEARED, FC_TIDS_CHANGED, FC_CODES_CHANGED, FC_NODE_PAGES, FC_N = 8 };
struct PagesFollowArgs {
    const uint8_t* pages;     // [n_listed][page_size]
    const uint32_t* blocks;   // [n_listed] ascending
    const uint2* tab;         // [n_blocks] {dense id of the block's first node, SbqNode items on it} of the relation as it is now
    uint32_t n_listed, page_size, n_blocks;
    vs_node_layout lay;
    uint32_t W, R, n_before, has_labels;
    uint64_t* codes;
    uint32_t* nbrs;
    uint64_t* tids;
    uint32_t code_stride, nbr_stride;
    const uint32_t* label_off;  // check: the resident CSR; write: the offsets with the appended rows' behind them
    int16_t* label_val;         // check: the resident values (read); write: the grown array
    uint32_t* label_cnt;        // check: [n_appended] label count of every appended node
    uint64_t* new_tids;         // check: [n_appended]
    uint32_t* ctr;              // [FC_N]
    uint32_t* err;
};

template <bool WRITE>
__global__ __launch_bounds__(WAVE) void k_pages_follow(PagesFollowArgs a) {
    const int lane = threadIdx.x;
    const vs_node_layout lay = a.lay;
    uint32_t c_relinked = 0, c_cleared = 0, c_changed = 0, c_codes = 0, c_pages = 0;  // (wave-uniform)
    for (uint32_t i = blockIdx.x; i < a.n_listed; i += gridDim.x) {
        const uint32_t b = a.blocks[i];
        const uint2 ent = a.tab[b];
        const uint32_t cnt = ent.y;
        if (cnt == 0) continue;
        c_pages++;
        const uint8_t* page = a.pages + (size_t)i * a.page_size;
        const uint32_t upper = ld16(page + 14), special = ld16(page + 16);
        for (uint32_t off = 1; off <= cnt; ++off) {  // (107 one-word items fit a page: the items, not the lanes, bound the loop)
            const uint32_t node = ent.x + off - 1;
            const bool old = node < a.n_before;
            PageItem it;
            uint32_t detail;
            int64_t tgt;
            uint32_t pe = page_item_at(page, upper, special, off, lay.root_size, it, detail);
            if (pe != PE_OK) {
                if (lane == 0) page_error(a.err, pe, b, off, detail);
                continue;
            }
            const uint8_t* item = it.item;
            int64_t tgt_nbr;
            pe = page_item_vec8(it, lay.off_bq_vector, a.W, PE_CODE_WIDTH, tgt, detail);
            if (pe == PE_OK) pe = page_item_vec8(it, lay.off_neighbor_index_pointers, a.R, PE_NEIGHBOR_SLOTS, tgt_nbr, detail);
            if (pe != PE_OK) {  // (nothing of a malformed item is written, by either pass)
                if (lane == 0) page_error(a.err, pe, b, off, detail);
                continue;
            }
            // heap_item_pointer
            {
                const uint8_t* hp = item + it.root + lay.off_heap_item_pointer;
                const uint64_t tid = ((uint64_t)ld32(hp) << 16) | ld16(hp + 4);
                if (WRITE) {
                    if (lane == 0) a.tids[node] = tid;
                } else if (old) {
                    const uint64_t was = a.tids[node];
                    if (was != tid) {
                        if ((was & 0xFFFFu) != 0 && (tid & 0xFFFFu) == 0) c_cleared++;
                        else c_changed++;
                    }
                } else if (lane == 0) {
                    a.new_tids[node - a.n_before] = tid;
                }
            }
            // bq_vector: the row's padding words stay zero
            {
                bool diff = false;
                uint64_t* row = a.codes + (size_t)node * a.code_stride;
                for (uint32_t w = lane; w < a.code_stride; w += WAVE) {
                    uint64_t v = 0;
                    if (w < a.W) {
                        const uint8_t* src = item + tgt + 8 * w;
                        v = (uint64_t)ld32(src) | ((uint64_t)ld32(src + 4) << 32);
                    }
                    if (WRITE) row[w] = v;
                    else if (old && w < a.W) diff |= row[w] != v;
                }
                if (!WRITE && old && __ballot(diff)) c_codes++;
            }
            // neighbor_index_pointers: the list ends at the first InvalidBlockNumber; the row is padded to nbr_stride with the sentinel
            {
                bool diff = false, ended = false;
                uint32_t* row = a.nbrs + (size_t)node * a.nbr_stride;
                for (uint32_t j0 = 0; j0 < a.nbr_stride; j0 += WAVE) {
                    const uint32_t j = j0 + (uint32_t)lane;
                    uint32_t nb = 0xFFFFFFFFu, no = 0;
                    if (j < a.R && !ended) {
                        nb = ld32(item + tgt_nbr + 8 * j);
                        no = ld16(item + tgt_nbr + 8 * j + 4);
                    }
                    const uint64_t inval = __ballot(nb == 0xFFFFFFFFu);
                    const uint32_t nvalid = inval ? (uint32_t)__builtin_ctzll(inval) : WAVE;
                    if (nvalid < WAVE) ended = true;
                    uint32_t id = VS_INVALID_NODE;
                    if ((uint32_t)lane < nvalid) {
                        uint2 t = make_uint2(0, 0);
                        if (nb < a.n_blocks) t = a.tab[nb];
                        if (no < 1 || no > t.y) page_error(a.err, PE_DANGLING, b, off, j);
                        else id = t.x + no - 1;
                    }
                    if (j < a.nbr_stride) {
                        if (WRITE) row[j] = id;
                        else if (old && j < a.R) diff |= row[j] != id;
                    }
                }
                if (!WRITE && old && __ballot(diff)) c_relinked++;
            }
            // labels (LabeledSbqNode): an existing node's set is the resident CSR slice, an appended node's is counted, then copied
            if (a.has_labels) {
                const uint32_t fld = it.root + lay.off_labels;
                const int64_t tl = (int64_t)fld + (int32_t)ld32(item + fld);
                const uint32_t n = ld32(item + fld + 4);
                if (n && (tl < 0 || (uint64_t)tl + (uint64_t)n * 2 > it.len || (tl & 1))) {
                    if (lane == 0) page_error(a.err, PE_VEC_BOUNDS, b, off, fld);
                    if (!WRITE && !old && lane == 0) a.label_cnt[node - a.n_before] = 0;
                    continue;
                }
                if (old) {
                    if (!WRITE) {
                        const uint32_t o = a.label_off[node], have = a.label_off[node + 1] - o;
                        bool diff = n != have;
                        if (!diff)
                            for (uint32_t j = lane; j < n; j += WAVE) diff |= (int16_t)ld16(item + tl + 2 * j) != a.label_val[o + j];
                        if (__ballot(diff) && lane == 0) page_error(a.err, PE_LABELS_CHANGED, b, off, n);
                    }
                } else if (!WRITE) {
                    for (uint32_t j = 1 + (uint32_t)lane; j < n; j += WAVE)
                        if ((int16_t)ld16(item + tl + 2 * j) <= (int16_t)ld16(item + tl + 2 * j - 2)) page_error(a.err, PE_LABELS, b, off, j);
                    if (lane == 0) a.label_cnt[node - a.n_before] = n;
                } else {
                    const uint32_t o = a.label_off[node];
                    for (uint32_t j = lane; j < n; j += WAVE) a.label_val[o + j] = (int16_t)ld16(item + tl + 2 * j);
                }
            }
        }
    }
    if (!WRITE && lane == 0) {
        if (c_relinked) atomicAdd(&a.ctr[FC_RELINKED], c_relinked);
        if (c_cleared) atomicAdd(&a.ctr[FC_TIDS_CLEARED], c_cleared);
        if (c_changed) atomicAdd(&a.ctr[FC_TIDS_CHANGED], c_changed);
        if (c_codes) atomicAdd(&a.ctr[FC_CODES_CHANGED], c_codes);
        if (c_pages) atomicAdd(&a.ctr[FC_NODE_PAGES], c_pages);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The same for `plain` storage (vs_pages_follow_open_plain): PlainNode items on PageType::Node pages.  k_pages_follow_plain is
// k_pages_follow's sibling — its grid (a wave per listed page), list convention, table, split at n_before, counters and error record
// — with the vector where the code row was.  PlainNode.vector is an ArchivedVec<f32> of D = num_dimensions_to_index floats; the
// resident side is the vector column (rows of vec_stride floats, a multiple of 4: 16-byte loads and stores), the page side is
// MAXALIGNed (an item starts on 8 bytes): 4-byte loads there.  A lane owns pieces of 4 floats, the piece loop runs until the vector
// ends (1930 floats fit a page: 483 pieces, 8 trips); the last piece of a D that is no multiple of 4 is cut at D — the neighbor
// pointers start there.
//   check, existing node: the page's floats against what k_pages_encode_plain would compose from the resident row — the index slice,
//     for cosine each float divided by the slice's divisor (one wave-uniform load per item) where that is not zero; the `/` below is
//     the one of k_pages_encode_plain, in this translation unit under its flags.  Bit patterns are compared; one ballot per item.
//   write, existing node: tid and neighbor row.  The vector row and the divisors are NOT written: the reference never rewrites a
//     node's vector, and a normalised slice cannot be turned back into the heap's row.
//   write, appended node: tid, neighbor row and — copy_vecs, when the caller handed no rows and D = dim_full — the D floats of the page
//     into the row, its padding floats [D, vec_stride) zero, which is what vs_upload_rows leaves there.
// ---------------------------------------------------------------------------------------------------------------
struct PagesFollowPlainArgs {
    const uint8_t* pages;    // [n_listed][page_size]
    const uint32_t* blocks;  // [n_listed] ascending
    const uint2* tab;        // [n_blocks] {dense id of the block's first node, PlainNode items on it} of the relation as it is now
    uint32_t n_listed, page_size, n_blocks;
    vs_node_layout lay;      // off_bq_vector names the vector field
    uint32_t D, R, n_before;
    float* vecs;
    const float* vdiv;       // cosine: the divisor of every resident node's index slice (0 = the slice is left alone); else null
    uint32_t* nbrs;
    uint64_t* tids;
    uint32_t vec_stride, nbr_stride;
    uint32_t copy_vecs;      // write: the appended nodes' vectors come from the pages
    uint64_t* new_tids;      // check: [n_appended]
    uint32_t* ctr;           // [FC_N]
    uint32_t* err;
};

template <bool WRITE>
__global__ __launch_bounds__(WAVE) void k_pages_follow_plain(PagesFollowPlainArgs a) {
    const int lane = threadIdx.x;
    const vs_node_layout lay = a.lay;
    const uint32_t P = (a.D + 3) / 4;  // 16-byte pieces of a vector
    uint32_t c_relinked = 0, c_cleared = 0, c_changed = 0, c_vecs = 0, c_pages = 0;  // (wave-uniform)
    for (uint32_t i = blockIdx.x; i < a.n_listed; i += gridDim.x) {
        const uint32_t b = a.blocks[i];
        const uint2 ent = a.tab[b];
        const uint32_t cnt = ent.y;
        if (cnt == 0) continue;
        c_pages++;
        const uint8_t* page = a.pages + (size_t)i * a.page_size;
        const uint32_t upper = ld16(page + 14), special = ld16(page + 16);
        for (uint32_t off = 1; off <= cnt; ++off) {  // (about 75 items fit a page at 10 dimensions and 4 slots: the items bound the loop)
            const uint32_t node = ent.x + off - 1;
            const bool old = node < a.n_before;
            PageItem it;
            uint32_t detail;
            int64_t tgt, tgt_nbr;
            uint32_t pe = page_item_at(page, upper, special, off, lay.root_size, it, detail);
            if (pe == PE_OK) pe = page_item_vec4(it, lay.off_bq_vector, a.D, PE_VECTOR_DIM, tgt, detail);
            if (pe == PE_OK) pe = page_item_vec8(it, lay.off_neighbor_index_pointers, a.R, PE_NEIGHBOR_SLOTS, tgt_nbr, detail);
            if (pe != PE_OK) {  // (nothing of a malformed item is written, by either pass)
                if (lane == 0) page_error(a.err, pe, b, off, detail);
                continue;
            }
            const uint8_t* item = it.item;
            // heap_item_pointer
            {
                const uint8_t* hp = item + it.root + lay.off_heap_item_pointer;
                const uint64_t tid = ((uint64_t)ld32(hp) << 16) | ld16(hp + 4);
                if (WRITE) {
                    if (lane == 0) a.tids[node] = tid;
                } else if (old) {
                    const uint64_t was = a.tids[node];
                    if (was != tid) {
                        if ((was & 0xFFFFu) != 0 && (tid & 0xFFFFu) == 0) c_cleared++;
                        else c_changed++;
                    }
                } else if (lane == 0) {
                    a.new_tids[node - a.n_before] = tid;
                }
            }
            // vector
            if (!WRITE && old) {
                const float s = a.vdiv ? a.vdiv[node] : 0.0f;
                const float* row = a.vecs + (size_t)node * a.vec_stride;
                const uint8_t* src = item + tgt;
                bool diff = false;
                for (uint32_t q = lane; q < P; q += WAVE) {
                    float4 v = *reinterpret_cast<const float4*>(row + 4 * q);
                    if (s != 0.0f) {
                        v.x = v.x / s;
                        v.y = v.y / s;
                        v.z = v.z / s;
                        v.w = v.w / s;
                    }
                    const uint32_t have = a.D - 4 * q;  // floats of this piece that belong to the vector (>= 1)
                    diff |= ld32(src + 16 * q) != __float_as_uint(v.x);
                    if (have > 1) diff |= ld32(src + 16 * q + 4) != __float_as_uint(v.y);
                    if (have > 2) diff |= ld32(src + 16 * q + 8) != __float_as_uint(v.z);
                    if (have > 3) diff |= ld32(src + 16 * q + 12) != __float_as_uint(v.w);
                }
                if (__ballot(diff)) c_vecs++;
            } else if (WRITE && !old && a.copy_vecs) {
                float* row = a.vecs + (size_t)node * a.vec_stride;
                const uint8_t* src = item + tgt;
                for (uint32_t q = lane; 4 * q < a.vec_stride; q += WAVE) {
                    const uint32_t have = 4 * q < a.D ? a.D - 4 * q : 0u;
                    uint4 v = make_uint4(0, 0, 0, 0);
                    if (have > 0) v.x = ld32(src + 16 * q);
                    if (have > 1) v.y = ld32(src + 16 * q + 4);
                    if (have > 2) v.z = ld32(src + 16 * q + 8);
                    if (have > 3) v.w = ld32(src + 16 * q + 12);
                    *reinterpret_cast<uint4*>(row + 4 * q) = v;
                }
            }
            // neighbor_index_pointers: the list ends at the first InvalidBlockNumber; the row is padded to nbr_stride with the sentinel
            {
                bool diff = false, ended = false;
                uint32_t* row = a.nbrs + (size_t)node * a.nbr_stride;
                for (uint32_t j0 = 0; j0 < a.nbr_stride; j0 += WAVE) {
                    const uint32_t j = j0 + (uint32_t)lane;
                    uint32_t nb = 0xFFFFFFFFu, no = 0;
                    if (j < a.R && !ended) {
                        nb = ld32(item + tgt_nbr + 8 * j);
                        no = ld16(item + tgt_nbr + 8 * j + 4);
                    }
                    const uint64_t inval = __ballot(nb == 0xFFFFFFFFu);
                    const uint32_t nvalid = inval ? (uint32_t)__builtin_ctzll(inval) : WAVE;
                    if (nvalid < WAVE) ended = true;
                    uint32_t id = VS_INVALID_NODE;
                    if ((uint32_t)lane < nvalid) {
                        uint2 t = make_uint2(0, 0);
                        if (nb < a.n_blocks) t = a.tab[nb];
                        if (no < 1 || no > t.y) page_error(a.err, PE_DANGLING_PLAIN, b, off, j);
                        else id = t.x + no - 1;
                    }
                    if (j < a.nbr_stride) {
                        if (WRITE) row[j] = id;
                        else if (old && j < a.R) diff |= row[j] != id;
                    }
                }
                if (!WRITE && old && __ballot(diff)) c_relinked++;
            }
        }
    }
    if (!WRITE && lane == 0) {
        if (c_relinked) atomicAdd(&a.ctr[FC_RELINKED], c_relinked);
        if (c_cleared) atomicAdd(&a.ctr[FC_TIDS_CLEARED], c_cleared);
        if (c_changed) atomicAdd(&a.ctr[FC_TIDS_CHANGED], c_changed);
        if (c_vecs) atomicAdd(&a.ctr[FC_CODES_CHANGED], c_vecs);
        if (c_pages) atomicAdd(&a.ctr[FC_NODE_PAGES], c_pages);
    }
}

struct vs_pages_follow {
    vs_index* ix = nullptr;
    vs_ctx* ctx = nullptr;
    uint32_t page_size = VS_BLCKSZ;
    vs_node_layout lay{};
    bool labeled = false;
    bool plain = false;  // PlainNode items on PageType::Node pages (vs_pages_follow_open_plain): k_pages_follow_plain
    // the block table of the relation the index mirrors now (host), and the same on the device as {base, count} per block
    std::vector<uint32_t> cnt, base;
    uint32_t n = 0;
    uint2* d_tab = nullptr;
    uint32_t tab_cap = 0;
    // a staged list
    bool staged = false;
    uint32_t tail0 = 0;  // first block whose device entry is the staged one, not the current one
    std::vector<uint32_t> s_cnt, s_base;  // the table as the staged pages make it
    std::vector<uint32_t> s_label_off;    // labeled: label_off[n_before + 1 ..] of the grown index
    std::vector<uint64_t> s_new_tids;
    vs_pages_follow_info info{};
    uint8_t* d_pages = nullptr;
    size_t pages_cap = 0;
    uint32_t* d_list = nullptr;
    size_t list_cap = 0;
    uint64_t* d_new_tids = nullptr;
    uint32_t* d_lcnt = nullptr;
    size_t new_cap = 0;
    uint32_t* d_ctr = nullptr;  // FC_N counters, then the error record
};

static void follow_table_entries(const std::vector<uint32_t>& base, const std::vector<uint32_t>& cnt, uint32_t b0, uint32_t b1,
                                 std::vector<uint2>& out) {
    out.resize(b1 - b0);
    for (uint32_t b = b0; b < b1; ++b) out[b - b0] = make_uint2(base[b], cnt[b]);
}

// the device table is the current one again (the entries a staged list replaced are uploaded from the host's table)
static int follow_unstage(vs_pages_follow* f) {
    if (!f->staged) return VS_OK;
    f->staged = false;
    const uint32_t nb = (uint32_t)f->cnt.size();
    if (f->tail0 < nb) {
        std::vector<uint2> ent;
        follow_table_entries(f->base, f->cnt, f->tail0, nb, ent);
        VS_TRY(vs_dev_upload(f->ctx, f->d_tab + f->tail0, ent.data(), ent.size() * 8));
    }
    return VS_OK;
}

extern "C" void vs_pages_follow_close(vs_pages_follow* f) {
    if (!f) return;
    if (f->ctx) (void)hipSetDevice(f->ctx->device);
    if (f->d_tab) (void)hipFree(f->d_tab);
    if (f->d_pages) (void)hipFree(f->d_pages);
    if (f->d_list) (void)hipFree(f->d_list);
    if (f->d_new_tids) (void)hipFree(f->d_new_tids);
    if (f->d_lcnt) (void)hipFree(f->d_lcnt);
    if (f->d_ctr) (void)hipFree(f->d_ctr);
    delete f;
}

static int follow_open_impl(vs_pages_follow* f, const uint32_t* blk_cnt, uint32_t n_blocks, const char* what = "vs_pages_follow_open") {
    vs_ctx* c = f->ctx;
    VS_HIP(hipSetDevice(c->device));
    f->cnt.assign(blk_cnt, blk_cnt + n_blocks);
    f->base.resize(n_blocks);
    uint64_t sum = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        f->base[b] = (uint32_t)sum;
        sum += blk_cnt[b];
        VS_REQUIRE(sum < VS_INVALID_NODE, "%s: the block table counts more than %u nodes", what, VS_INVALID_NODE - 1);
    }
    VS_REQUIRE(sum == f->ix->d.n, "%s: the block table counts %llu nodes, the index holds %u", what, (unsigned long long)sum, f->ix->d.n);
    f->n = (uint32_t)sum;
    f->tab_cap = n_blocks + n_blocks / 2 + 64;
    VS_HIP(hipMalloc(&f->d_tab, (size_t)f->tab_cap * 8));
    VS_HIP(hipMalloc(&f->d_ctr, (FC_N + 4) * 4));
    if (n_blocks) {
        std::vector<uint2> ent;
        follow_table_entries(f->base, f->cnt, 0, n_blocks, ent);
        VS_TRY(vs_dev_upload(c, f->d_tab, ent.data(), ent.size() * 8));
    }
    return VS_OK;
}

extern "C" int vs_pages_follow_open(vs_index* idx, uint32_t page_size, const vs_node_layout* layout, const uint32_t* blk_cnt,
                                    uint32_t n_blocks, vs_pages_follow** out) {
    VS_REQUIRE(idx && out && (blk_cnt || !n_blocks), "vs_pages_follow_open: bad args");
    *out = nullptr;
    VS_REQUIRE(idx->d.storage_type == VS_STORAGE_SBQ, "vs_pages_follow_open: memory_optimized (SBQ) indexes only; a `plain` index keeps its "
               "vectors in the nodes and is followed with vs_pages_follow_open_plain");
    VS_REQUIRE(idx->codes && idx->nbrs && idx->tids, "vs_pages_follow_open: the index holds no codes / neighbors");
    VS_REQUIRE(page_size >= 512 && page_size <= 32768 && !(page_size & (page_size - 1)), "vs_pages_follow_open: page_size %u is not a PostgreSQL block size",
               page_size);
    return vs_guard("vs_pages_follow_open", [&] {
        vs_pages_follow* f = new vs_pages_follow();
        f->ix = idx;
        f->ctx = idx->ctx;
        f->page_size = page_size;
        f->labeled = idx->label_off != nullptr;
        if (layout) f->lay = *layout;
        else vs_node_layout_default(f->labeled ? 1 : 0, &f->lay);
        const vs_node_layout& l = f->lay;
        const uint32_t offs[4] = {l.off_heap_item_pointer, l.off_bq_vector, l.off_neighbor_index_pointers, l.off_labels};
        int r = VS_OK;
        for (int i = 0; i < (f->labeled ? 4 : 3) && r == VS_OK; ++i)
            if (offs[i] > l.root_size || l.root_size - offs[i] < 8 || l.root_size > 4096 || (offs[i] & 3u)) {
                vs_set_error("vs_pages_follow_open: field offset %u does not fit a %u-byte archived node", offs[i], l.root_size);
                r = VS_ERR_INVALID;
            }
        if (r == VS_OK) r = follow_open_impl(f, blk_cnt, n_blocks);
        if (r != VS_OK) {
            vs_pages_follow_close(f);
            return r;
        }
        *out = f;
        return (int)VS_OK;
    });
}

extern "C" int vs_pages_follow_open_plain(vs_index* idx, uint32_t page_size, const vs_node_layout* layout, const uint32_t* blk_cnt,
                                          uint32_t n_blocks, vs_pages_follow** out) {
    const char* what = "vs_pages_follow_open_plain";
    VS_REQUIRE(idx && out && (blk_cnt || !n_blocks), "%s: bad args", what);
    *out = nullptr;
    VS_REQUIRE(idx->d.storage_type == VS_STORAGE_PLAIN, "%s: `plain` indexes only; a memory_optimized (SBQ) index is followed with "
               "vs_pages_follow_open", what);
    VS_REQUIRE(idx->vecs && idx->nbrs && idx->tids, "%s: the index holds no vector column / neighbors / heap tids", what);
    VS_REQUIRE(idx->d.distance_type != VS_COSINE || (idx->d.dim_index < idx->d.dim_full ? idx->vnorm_idx : idx->vnorm),
               "%s: the index has no divisors for its index slices (vs_index_refresh_norms)", what);
    VS_REQUIRE(idx->vec_stride % 4 == 0 && idx->d.dim_index <= idx->d.dim_full && idx->d.dim_full <= idx->vec_stride,
               "%s: vector rows of %u floats for %u dimensions", what, idx->vec_stride, idx->d.dim_index);
    VS_REQUIRE(page_size >= 512 && page_size <= 32768 && !(page_size & (page_size - 1)), "%s: page_size %u is not a PostgreSQL block size", what,
               page_size);
    return vs_guard(what, [&] {
        vs_pages_follow* f = new vs_pages_follow();
        f->ix = idx;
        f->ctx = idx->ctx;
        f->page_size = page_size;
        f->plain = true;
        if (layout) f->lay = *layout;
        else vs_plain_layout_default(&f->lay);
        const vs_node_layout& l = f->lay;
        const uint32_t offs[3] = {l.off_heap_item_pointer, l.off_bq_vector, l.off_neighbor_index_pointers};  // (off_labels is ignored)
        int r = VS_OK;
        for (int i = 0; i < 3 && r == VS_OK; ++i)
            if (offs[i] > l.root_size || l.root_size - offs[i] < 8 || l.root_size > 4096 || (offs[i] & 3u)) {
                vs_set_error("%s: field offset %u does not fit a %u-byte archived node", what, offs[i], l.root_size);
                r = VS_ERR_INVALID;
            }
        if (r == VS_OK) r = follow_open_impl(f, blk_cnt, n_blocks, what);
        if (r != VS_OK) {
            vs_pages_follow_close(f);
            return r;
        }
        *out = f;
        return (int)VS_OK;
    });
}

template <class T>
static int follow_reserve(T** p, size_t* cap, size_t n) {
    if (n <= *cap) return VS_OK;
    if (*p) VS_HIP(hipFree(*p));
    *p = nullptr;
    *cap = 0;
    VS_HIP(hipMalloc(p, n * sizeof(T)));
    *cap = n;
    return VS_OK;
}

static int follow_launch(vs_pages_follow* f, bool write, const PagesFollowArgs& a) {
    vs_ctx* c = f->ctx;
    const uint32_t grid = std::min<uint32_t>(a.n_listed, 1u << 20);
    hipEvent_t ev = prof_begin(c);
    if (write) hipLaunchKernelGGL((k_pages_follow<true>), dim3(grid), dim3(WAVE), 0, c->stream, a);
    else hipLaunchKernelGGL((k_pages_follow<false>), dim3(grid), dim3(WAVE), 0, c->stream, a);
    VS_HIP(hipGetLastError());
    prof_end(c, PK_PAGES, ev);
    return VS_OK;
}

static int follow_launch_plain(vs_pages_follow* f, bool write, const PagesFollowPlainArgs& a) {
    vs_ctx* c = f->ctx;
    const uint32_t grid = std::min<uint32_t>(a.n_listed, 1u << 20);
    hipEvent_t ev = prof_begin(c);
    if (write) hipLaunchKernelGGL((k_pages_follow_plain<true>), dim3(grid), dim3(WAVE), 0, c->stream, a);
    else hipLaunchKernelGGL((k_pages_follow_plain<false>), dim3(grid), dim3(WAVE), 0, c->stream, a);
    VS_HIP(hipGetLastError());
    prof_end(c, PK_PAGES, ev);
    return VS_OK;
}

static PagesFollowPlainArgs follow_args_plain(const vs_pages_follow* f, uint32_t n_listed, uint32_t n_blocks_now, bool copy_vecs) {
    const vs_index* ix = f->ix;
    const vs_index_desc& d = ix->d;
    PagesFollowPlainArgs a{};
    a.pages = f->d_pages;
    a.blocks = f->d_list;
    a.tab = f->d_tab;
    a.n_listed = n_listed;
    a.page_size = f->page_size;
    a.n_blocks = n_blocks_now;
    a.lay = f->lay;
    a.D = d.dim_index;
    a.R = d.num_neighbors;
    a.n_before = f->n;
    a.vecs = ix->vecs;
    a.vdiv = d.distance_type == VS_COSINE ? (d.dim_index < d.dim_full ? ix->vnorm_idx : ix->vnorm) : nullptr;  // (as the page writer)
    a.nbrs = ix->nbrs;
    a.tids = ix->tids;
    a.vec_stride = ix->vec_stride;
    a.nbr_stride = ix->nbr_stride;
    a.copy_vecs = copy_vecs ? 1u : 0u;
    a.new_tids = f->d_new_tids;
    a.ctr = f->d_ctr;
    a.err = f->d_ctr + FC_N;
    return a;
}

static PagesFollowArgs follow_args(const vs_pages_follow* f, uint32_t n_listed, uint32_t n_blocks_now) {
    const vs_index* ix = f->ix;
    PagesFollowArgs a{};
    a.pages = f->d_pages;
    a.blocks = f->d_list;
    a.tab = f->d_tab;
    a.n_listed = n_listed;
    a.page_size = f->page_size;
    a.n_blocks = n_blocks_now;
    a.lay = f->lay;
    a.W = ix->d.words;
    a.R = ix->d.num_neighbors;
    a.n_before = f->n;
    a.has_labels = f->labeled ? 1u : 0u;
    a.codes = ix->codes;
    a.nbrs = ix->nbrs;
    a.tids = ix->tids;
    a.code_stride = ix->code_stride;
    a.nbr_stride = ix->nbr_stride;
    a.label_off = ix->label_off;
    a.label_val = ix->label_val;
    a.label_cnt = f->d_lcnt;
    a.new_tids = f->d_new_tids;
    a.ctr = f->d_ctr;
    a.err = f->d_ctr + FC_N;
    return a;
}

// what a pass reported (after the stream has been synchronised)
static int follow_page_error(const uint32_t* herr, const char* what) {
    if (herr[0] == PE_OK) return VS_OK;
    vs_set_error("%s: block %u item %u: %s (detail %u)", what, herr[1], herr[2], kPageErrorText[herr[0] <= PE_LAST ? herr[0] : 0], herr[3]);
    return VS_ERR_INVALID;
}

static int follow_stage_impl(vs_pages_follow* f, const uint32_t* blocks, const void* pages, uint32_t n, uint32_t n_blocks_total,
                             vs_pages_follow_info* info) {
    const char* what = "vs_pages_follow_stage";
    vs_ctx* c = f->ctx;
    vs_index* ix = f->ix;
    VS_HIP(hipSetDevice(c->device));
    VS_TRY(follow_unstage(f));  // (a second stage replaces the first, a refused one leaves none)
    if (f->n != ix->d.n) {
        vs_set_error("%s: the index holds %u nodes, the follower's table %u: something else changed the index (open a new follower)", what,
                     ix->d.n, f->n);
        return VS_ERR_STATE;
    }
    const uint32_t nb_before = (uint32_t)f->cnt.size();
    VS_REQUIRE(n_blocks_total >= nb_before, "%s: the relation shrank from %u to %u blocks", what, nb_before, n_blocks_total);
    VS_REQUIRE(n_blocks_total < 0xFFFFFFFFu, "%s: block number overflow", what);
    // the last block that held nodes: an item count may grow there and behind it, nowhere else
    uint32_t last_node_block = 0;
    bool any_node_block = false;
    for (uint32_t b = nb_before; b-- > 0;)
        if (f->cnt[b]) {
            last_node_block = b;
            any_node_block = true;
            break;
        }
    const uint8_t* src = static_cast<const uint8_t*>(pages);
    std::vector<uint32_t> l_cnt(n);
    uint32_t tail_listed = 0, first_changed = n_blocks_total;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t b = blocks[i];
        VS_REQUIRE(i == 0 || blocks[i - 1] < b, "%s: blocks[%u] = %u after %u: the list must be strictly ascending", what, i, b, blocks[i - 1]);
        VS_REQUIRE(b < n_blocks_total, "%s: blocks[%u] = %u of a relation of %u blocks", what, i, b, n_blocks_total);
        VS_TRY(vs_pages_header_items_of(src + (size_t)i * f->page_size, f->page_size, b, f->plain ? VS_PAGE_NODE : VS_PAGE_SBQ_NODE, &l_cnt[i]));
        const uint32_t was = b < nb_before ? f->cnt[b] : 0;
        VS_REQUIRE(l_cnt[i] >= was, "%s: block %u held %u nodes and holds %u now: existing nodes would move", what, b, was, l_cnt[i]);
        VS_REQUIRE(l_cnt[i] == was || !any_node_block || b >= last_node_block,
                   "%s: block %u gained %u item(s) in front of the node page %u: existing nodes would move", what, b, l_cnt[i] - was, last_node_block);
        if (b >= nb_before) tail_listed++;
        if (l_cnt[i] != was || b >= nb_before) first_changed = std::min(first_changed, b);
    }
    VS_REQUIRE(tail_listed == n_blocks_total - nb_before, "%s: %u of the %u blocks the relation grew by are in the list (every block from %u on must be)",
               what, tail_listed, n_blocks_total - nb_before, nb_before);
    first_changed = std::min(first_changed, nb_before);
    // the table as it is now
    f->s_cnt = f->cnt;
    f->s_cnt.resize(n_blocks_total, 0);
    for (uint32_t i = 0; i < n; ++i) f->s_cnt[blocks[i]] = l_cnt[i];
    f->s_base = f->base;
    f->s_base.resize(n_blocks_total, 0);
    uint64_t sum = first_changed < nb_before ? f->base[first_changed] : f->n;
    for (uint32_t b = first_changed; b < n_blocks_total; ++b) {
        f->s_base[b] = (uint32_t)sum;
        sum += f->s_cnt[b];
        VS_REQUIRE(sum < VS_INVALID_NODE, "%s: more than %u index nodes", what, VS_INVALID_NODE - 1);
    }
    const uint32_t n_app = (uint32_t)sum - f->n;
    vs_pages_follow_info fi{};
    fi.n_blocks_before = nb_before;
    fi.n_blocks_now = n_blocks_total;
    fi.pages_listed = n;
    fi.n_before = f->n;
    fi.n_appended = n_app;
    // device side: the table's tail, the list, the pages (through the pinned ring)
    if (n_blocks_total > f->tab_cap) {
        uint2* fresh = nullptr;
        const uint32_t cap = n_blocks_total + n_blocks_total / 2 + 64;
        VS_HIP(hipMalloc(&fresh, (size_t)cap * 8));
        (void)hipFree(f->d_tab);
        f->d_tab = fresh;
        f->tab_cap = cap;
        first_changed = 0;
    }
    f->tail0 = first_changed;
    f->staged = true;  // (from here on the device table may differ from the current one: every way out below goes through follow_unstage)
    auto run = [&]() -> int {
        if (first_changed < n_blocks_total) {
            std::vector<uint2> ent;
            follow_table_entries(f->s_base, f->s_cnt, first_changed, n_blocks_total, ent);
            VS_TRY(vs_dev_upload(c, f->d_tab + first_changed, ent.data(), ent.size() * 8));
        }
        VS_HIP(hipMemsetAsync(f->d_ctr, 0, (FC_N + 4) * 4, c->stream));
        uint32_t h[FC_N + 4] = {0};
        if (n) {
            VS_TRY(follow_reserve(&f->d_list, &f->list_cap, (size_t)n));
            VS_TRY(follow_reserve(&f->d_pages, &f->pages_cap, (size_t)n * f->page_size));
            if (n_app > f->new_cap) {
                size_t cap_t = f->new_cap, cap_l = f->new_cap;
                VS_TRY(follow_reserve(&f->d_new_tids, &cap_t, (size_t)n_app));
                VS_TRY(follow_reserve(&f->d_lcnt, &cap_l, (size_t)n_app));
                f->new_cap = n_app;
            }
            VS_TRY(vs_dev_upload(c, f->d_list, blocks, (size_t)n * 4));
            VS_TRY(vs_dev_upload(c, f->d_pages, pages, (size_t)n * f->page_size));
            if (f->plain) VS_TRY(follow_launch_plain(f, false, follow_args_plain(f, n, n_blocks_total, false)));
            else VS_TRY(follow_launch(f, false, follow_args(f, n, n_blocks_total)));
            VS_HIP(hipMemcpyAsync(h, f->d_ctr, sizeof h, hipMemcpyDeviceToHost, c->stream));
        }
        VS_HIP(hipStreamSynchronize(c->stream));
        VS_TRY(follow_page_error(h + FC_N, what));
        fi.node_pages_listed = h[FC_NODE_PAGES];
        fi.rows_relinked = h[FC_RELINKED];
        fi.tids_cleared = h[FC_TIDS_CLEARED];
        fi.tids_changed = h[FC_TIDS_CHANGED];
        fi.codes_changed = h[FC_CODES_CHANGED];
        f->s_new_tids.resize(n_app);
        f->s_label_off.clear();
        if (n_app) VS_TRY(vs_dev_download(c, f->s_new_tids.data(), f->d_new_tids, (size_t)n_app * 8));
        if (f->labeled && n_app) {
            f->s_label_off.resize(n_app);
            VS_TRY(vs_dev_download(c, f->s_label_off.data(), f->d_lcnt, (size_t)n_app * 4));
            uint64_t tot = ix->n_label_vals;
            for (uint32_t i = 0; i < n_app; ++i) {
                tot += f->s_label_off[i];
                f->s_label_off[i] = (uint32_t)tot;
            }
            VS_REQUIRE(tot < 0xFFFFFFFFull, "%s: label CSR exceeds 2^32 entries", what);
            fi.label_vals_appended = tot - ix->n_label_vals;
        }
        return VS_OK;
    };
    const int rc = run();
    if (rc != VS_OK) {
        (void)hipStreamSynchronize(c->stream);
        (void)follow_unstage(f);
        return rc;
    }
    f->info = fi;
    if (info) *info = fi;
    return VS_OK;
}

extern "C" int vs_pages_follow_stage(vs_pages_follow* f, const uint32_t* blocks, const void* pages, uint32_t n, uint32_t n_blocks_total,
                                     vs_pages_follow_info* info) {
    VS_REQUIRE(f && (n == 0 || (blocks && pages)), "vs_pages_follow_stage: bad args");
    if (info) memset(info, 0, sizeof *info);
    return vs_guard("vs_pages_follow_stage", [&] { return follow_stage_impl(f, blocks, pages, n, n_blocks_total, info); });
}

extern "C" int vs_pages_follow_new_tids(const vs_pages_follow* f, uint64_t* tids, uint32_t cap) {
    VS_REQUIRE(f, "vs_pages_follow_new_tids: null follower");
    if (!f->staged) {
        vs_set_error("vs_pages_follow_new_tids: no list is staged");
        return VS_ERR_STATE;
    }
    VS_REQUIRE(cap >= f->s_new_tids.size() && (tids || f->s_new_tids.empty()), "vs_pages_follow_new_tids: room for %u of %zu tids", cap,
               f->s_new_tids.size());
    if (!f->s_new_tids.empty()) memcpy(tids, f->s_new_tids.data(), f->s_new_tids.size() * 8);
    return VS_OK;
}

extern "C" int vs_pages_follow_discard(vs_pages_follow* f) {
    VS_REQUIRE(f, "vs_pages_follow_discard: null follower");
    return vs_guard("vs_pages_follow_discard", [&]() -> int {
        VS_HIP(hipSetDevice(f->ctx->device));
        return follow_unstage(f);
    });
}

// new_in_hbm: new_vecs is device memory (vs_pages_follow_apply_dev); the rows then reach the column by a strided copy on the device
static int follow_apply_impl(vs_pages_follow* f, const float* new_vecs, uint32_t vec_stride, vs_pages_follow_info* info, bool new_in_hbm) {
    const char* what = new_in_hbm ? "vs_pages_follow_apply_dev" : "vs_pages_follow_apply";
    vs_index* ix = f->ix;
    vs_ctx* c = f->ctx;
    hipStream_t st = c->stream;
    auto state_error = [&](const char* msg) {
        vs_set_error("%s: %s", what, msg);
        return VS_ERR_STATE;
    };
    if (!f->staged) return state_error("no list is staged (vs_pages_follow_stage first)");
    VS_REQUIRE_OWNER(ix, what);
    VS_REQUIRE_NO_VIEWS(ix, what);
    if (ix->ws.pending) return state_error("a batch of this handle is in flight (vs_search_batch_dev_finish first)");
    if (f->n != ix->d.n) return state_error("the index changed after the list was staged (open a new follower)");
    const uint32_t n_old = f->n, n_app = f->info.n_appended, n = n_old + n_app;
    if (n_app && ix->visible && ix->visible != ix->visible_own) {
        bool ours = false;
        for (const uint8_t* sp : ix->snap) ours |= sp == ix->visible;
        if (!ours) return state_error("a caller-owned device visibility mask is in force and cannot be grown by the library (clear or replace it)");
    }
    bool want_vecs = ix->vecs != nullptr && n_app > 0;
    // a plain relation carries the appended nodes' vectors itself when every dimension is indexed: without rows from the caller the
    // write pass copies them out of the pages (what IndexPages.upload_plain(vecs=None) does for a whole index)
    const bool vecs_from_pages = f->plain && want_vecs && !new_vecs && ix->d.dim_index == ix->d.dim_full;
    VS_REQUIRE(!(f->plain && want_vecs && !new_vecs) || vecs_from_pages, "%s: %u rows are appended and new_vecs is NULL: the pages hold only the "
               "index slice (%u of %u dimensions; vs_pages_follow_new_tids names the heap tuples to read)", what, n_app, ix->d.dim_index,
               ix->d.dim_full);
    if (vecs_from_pages) want_vecs = false;
    VS_REQUIRE(!want_vecs || new_vecs, "%s: the index holds a vector column and %u rows are appended: new_vecs is NULL (vs_pages_follow_new_tids "
               "names the heap tuples to read)", what, n_app);
    VS_REQUIRE(!want_vecs || vec_stride >= ix->d.dim_full, "%s: vec_stride %u < num_dimensions %u", what, vec_stride, ix->d.dim_full);
    VS_HIP(hipSetDevice(c->device));
    if (n > ix->capacity) {  // the insert's rule: by half, at least to fit; a failed growth leaves the index as it was
        const uint64_t want = std::max<uint64_t>(n, (uint64_t)ix->capacity + ix->capacity / 2);
        VS_TRY(vs_index_reserve_impl(ix, (uint32_t)std::min<uint64_t>(want, VS_INVALID_NODE - 1), what));
    }
    // the grown label CSR: the values are built aside and swapped in at the end, the offsets are appended behind the live ones
    int16_t* new_val = nullptr;
    const uint64_t old_vals = ix->n_label_vals, add_vals = f->info.label_vals_appended;
    if (f->labeled && add_vals) {
        VS_HIP(hipMalloc(&new_val, (old_vals + add_vals) * 2));
        hipError_t e = hipSuccess;
        if (old_vals) e = hipMemcpyAsync(new_val, ix->label_val, old_vals * 2, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) {
            (void)hipFree(new_val);
            vs_set_error("%s: copying the label sets failed: %s", what, hipGetErrorString(e));
            return VS_ERR_HIP;
        }
    }
    auto run = [&]() -> int {
        if (f->labeled && n_app) {
            if (n_old == 0) {
                const uint32_t zero = 0;
                VS_HIP(hipMemcpy(ix->label_off, &zero, 4, hipMemcpyHostToDevice));
            }
            VS_TRY(vs_dev_upload(c, ix->label_off + n_old + 1, f->s_label_off.data(), (size_t)n_app * 4));
        }
        if (want_vecs && new_in_hbm) {
            const uint64_t total = (uint64_t)n_app * ix->vec_stride;
            hipLaunchKernelGGL(k_rows_copy_pad, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, 4096)), dim3(256), 0, st,
                               ix->vecs + (size_t)n_old * ix->vec_stride, ix->vec_stride, new_vecs, vec_stride, ix->d.dim_full, n_app);
            VS_HIP(hipGetLastError());
        } else if (want_vecs) {
            VS_TRY(vs_upload_rows(c, ix->vecs + (size_t)n_old * ix->vec_stride, ix->vec_stride * 4ull, new_vecs, vec_stride * 4ull,
                                  ix->d.dim_full * 4ull, n_app));
        }
        uint32_t herr[4] = {0, 0, 0, 0};
        if (f->info.pages_listed) {
            VS_HIP(hipMemsetAsync(f->d_ctr, 0, (FC_N + 4) * 4, st));
            if (f->plain) {  // (nothing of an existing node's vector is written: codes_changed is a report)
                VS_TRY(follow_launch_plain(f, true, follow_args_plain(f, f->info.pages_listed, f->info.n_blocks_now, vecs_from_pages)));
            } else {
                PagesFollowArgs a = follow_args(f, f->info.pages_listed, f->info.n_blocks_now);  // (after the reserve: the arrays may have moved)
                if (new_val) a.label_val = new_val;
                VS_TRY(follow_launch(f, true, a));
                if (f->info.codes_changed) ix->codes_epoch++;
            }
            VS_HIP(hipMemcpyAsync(herr, f->d_ctr + FC_N, 16, hipMemcpyDeviceToHost, st));
        }
        if (n_app) {
            // a new tuple is visible to the library's own mask and to no snapshot that was stored before it existed
            if (ix->visible_own) VS_HIP(hipMemsetAsync(ix->visible_own + n_old, 1, n_app, st));
            for (int sn = 1; sn < VS_MAX_SNAPSHOTS; ++sn)
                if (ix->snap[sn]) VS_HIP(hipMemsetAsync(ix->snap[sn] + n_old, 0, n_app, st));
            VS_TRY(launch_row_norms_range(ix, n_old, n_app));  // (the codes come from the pages: nothing is quantized again)
            if (f->plain) VS_TRY(launch_slice_norms_range(ix, n_old, n_app));  // (as vs_index_insert does for a plain index)
        }
        VS_HIP(hipStreamSynchronize(st));
        return follow_page_error(herr, what);  // (the check pass saw the same bytes: this does not happen)
    };
    const int rc = run();
    if (rc != VS_OK) {
        (void)hipStreamSynchronize(st);
        if (new_val) (void)hipFree(new_val);
        return rc;
    }
    if (new_val) {
        if (ix->label_val) (void)hipFree(ix->label_val);
        ix->label_val = new_val;
        ix->n_label_vals = old_vals + add_vals;
    }
    ix->d.n = n;
    // derived state, as vs_index_insert leaves it: the neighbor masks dropped, the label masks re-derived, the planner's memory reset
    if (ix->nbr_mask) {
        (void)hipFree(ix->nbr_mask);
        ix->nbr_mask = nullptr;
    }
    ix->nbr_mask_valid = false;
    ix->nbr_mask_tried = false;
    ix->obs = ScanObs{};
    ix->last_fast = FastSig{};
    ix->last_ins_limit = 0;
    // the follower's table advances: the device already holds it
    f->cnt.swap(f->s_cnt);
    f->base.swap(f->s_base);
    f->n = n;
    f->staged = false;
    if (info) *info = f->info;
    if (f->labeled) VS_TRY(vs_refresh_label_masks(ix));
    return VS_OK;
}

extern "C" int vs_pages_follow_apply(vs_pages_follow* f, const float* new_vecs, uint32_t vec_stride, vs_pages_follow_info* info) {
    VS_REQUIRE(f, "vs_pages_follow_apply: null follower");
    return vs_guard("vs_pages_follow_apply", [&] { return follow_apply_impl(f, new_vecs, vec_stride, info, false); });
}

extern "C" int vs_pages_follow_apply_dev(vs_pages_follow* f, const float* d_new_vecs, uint32_t vec_stride, vs_pages_follow_info* info) {
    VS_REQUIRE(f, "vs_pages_follow_apply_dev: null follower");
    return vs_guard("vs_pages_follow_apply_dev", [&] { return follow_apply_impl(f, d_new_vecs, vec_stride, info, true); });
}

// ---------------------------------------------------------------------------------------------------------------
// The way back (vs_pages_out_*): the index arrays composed into SbqNode pages ON the device.
//
// k_pages_encode: one workgroup (four waves) per node page.  The page is put together in 8 KB of LDS — zeroed, then the
// PageHeaderData, the TsvPageOpaqueData special area, one line pointer per item and the items themselves: a wave per item, its
// lanes over the 16-byte pieces of the code row and of the neighbor row (four neighbor ids become four ArchivedItemPointers: block and
// offset of a classic node are arithmetic, those of a labeled node are gathered from node_block / page_first), then the label set
// and the four 8-byte fields of the archived root — and leaves for global memory as 512 full-lane 16-byte stores.  Items are
// MAXALIGNed (8 bytes) from pd_special = page_size - 8 downwards, so an item starts on an 8-byte, not a 16-byte boundary: the
// LDS side of the copy is 8 bytes per store.  What the page must look like is restated in vs_pages.cpp (PageAddItemExtended,
// Tape::write, rkyv to_bytes of ClassicSbqNode / LabeledSbqNode: code words, neighbor pointers, labels, root at the end).
// ---------------------------------------------------------------------------------------------------------------
struct PagesEncodeArgs {
    const uint64_t* codes;
    const uint32_t* nbrs;
    const uint64_t* tids;
    const uint32_t* label_off;   // labeled nodes only
    const int16_t* label_val;
    const uint32_t* page_first;  // labeled: first node of every node page (+ n at the end)
    const uint32_t* node_block;  // labeled: block of every node's item
    const uint16_t* node_lpoff;  // labeled: lp_off of every node's item
    uint32_t code_stride, nbr_stride;
    uint32_t n, W, R;
    uint32_t K, item_size;       // classic: items per page, bytes per item
    uint32_t first_node_block;
    uint32_t root_size, o_heap, o_code, o_nbr, o_last;
    uint32_t has_labels;
};
enum { PO_OK = 0, PO_NEIGHBOR = 1, PO_LAYOUT = 2 };
constexpr uint32_t kOutPage = VS_BLCKSZ, kOutSpecial = VS_BLCKSZ - 8, kOutThreads = 256;

typedef uint64_t __attribute__((may_alias)) po_u64;
typedef uint32_t __attribute__((may_alias)) po_u32;
typedef uint16_t __attribute__((may_alias)) po_u16;

// ArchivedItemPointer {u32 block_number, u16 offset, 2 B pad} as one little-endian word
__device__ __forceinline__ uint64_t item_pointer_word(uint32_t block, uint32_t offset) { return (uint64_t)block | ((uint64_t)offset << 32); }

// The digest of a finished page: the page is 512 pieces of 16 bytes (lo, hi: two little-endian u64); piece i
// contributes, in each of two independently keyed lanes, a strong 64-bit finaliser of its bytes and its position,
//     A_i = fmixA(fmixA(lo + KA + (i + 1) * GA) ^ hi),   B_i = fmixB(fmixB(lo + KB + (i + 1) * GB) ^ hi)
// (fmixA: the splitmix64 finaliser, fmixB: MurmurHash3's fmix64), and the digest is (sum A_i, sum B_i) modulo 2^64: addition
// commutes, so neither the order of the in-wave shuffles nor that of the cross-wave sum through LDS matters.
__device__ __forceinline__ uint64_t digest_fmix_a(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ uint64_t digest_fmix_b(uint64_t x) {
    x ^= x >> 33;
    x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33;
    x *= 0xC4CEB9FE1A85EC53ull;
    return x ^ (x >> 33);
}
__device__ __forceinline__ void digest_piece(uint32_t i, uint64_t lo, uint64_t hi, uint64_t& sa, uint64_t& sb) {
    sa += digest_fmix_a(digest_fmix_a(lo + 0x243F6A8885A308D3ull + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull) ^ hi);
    sb += digest_fmix_b(digest_fmix_b(lo + 0x13198A2E03707344ull + (uint64_t)(i + 1) * 0xC2B2AE3D27D4EB4Full) ^ hi);
}

// where the digest instantiation leaves its result, and what it is compared against
struct PagesDigestArgs {
    uint64_t* digest;             // [n_blocks][2] of the relation as it is now: node page p lands at block first_node_block + p
    const uint64_t* base_digest;  // [base_n_blocks][2] of the baseline (null: nothing to compare with)
    uint8_t* dirty;               // [n_node_pages] 1 = the block is not what the baseline recorded (null without a baseline)
    uint32_t base_n_blocks, base_first_node_block, base_n_node_pages;
};

// ---- what k_pages_encode and k_pages_encode_plain share: everything about a node page that does not depend on what its items hold ----
// PageInit + cnt x PageAddItemExtended as the header sees them (pd_lsn, pd_checksum, pd_flags, pd_prune_xid stay zero) and the
// TsvPageOpaqueData special area; one thread, on the zeroed page
__device__ __forceinline__ void page_out_header(uint8_t* pg, uint32_t cnt, uint32_t upper, uint32_t page_type) {
    *reinterpret_cast<po_u32*>(pg + 12) = (24 + 4 * cnt) | (upper << 16);        // pd_lower, pd_upper
    *reinterpret_cast<po_u32*>(pg + 16) = kOutSpecial | ((kOutPage | 4u) << 16);  // pd_special, pd_pagesize_version
    *reinterpret_cast<po_u32*>(pg + kOutSpecial) = page_type | (0xAE24u << 16);
}
// the line pointer of item k (0-based): LP_NORMAL
__device__ __forceinline__ void page_out_line_pointer(uint8_t* pg, uint32_t k, uint32_t lp_off, uint32_t size) {
    *reinterpret_cast<po_u32*>(pg + 24 + 4 * k) = lp_off | (1u << 15) | (size << 17);
}
// One wave turns a neighbor row into the R ArchivedItemPointers at `nb` (8-byte aligned LDS): the list ends at the first
// VS_INVALID_NODE, (InvalidBlockNumber, 0) from there on.  pointer_of(u) = the item pointer word of node u < n.  An id the index does
// not have is written as an invalid pointer; the item's lowest such slot is the one reported (PO_NEIGHBOR at block blk, item item_no).
template <class PointerOf>
__device__ __forceinline__ void page_out_neighbors(const uint32_t* __restrict__ nrow, uint8_t* nb, uint32_t R, uint32_t n, uint32_t lane,
                                                   uint32_t* __restrict__ err, uint32_t blk, uint32_t item_no, PointerOf&& pointer_of) {
    bool ended = false;
    for (uint32_t j0 = 0; j0 < R; j0 += 4 * WAVE) {
        const uint32_t j = j0 + 4 * lane;
        uint4 v = make_uint4(VS_INVALID_NODE, VS_INVALID_NODE, VS_INVALID_NODE, VS_INVALID_NODE);
        if (j < R) v = *reinterpret_cast<const uint4*>(nrow + j);  // (rows are nbr_stride = a multiple of 16 ids: 64-byte aligned)
        const uint32_t ids[4] = {v.x, v.y, v.z, v.w};
        uint32_t fi = 4;  // first slot of this lane's four that ends the list (or lies past R)
        for (int t = 3; t >= 0; --t)
            if (j + t >= R || ids[t] == VS_INVALID_NODE) fi = (uint32_t)t;
        const uint64_t enders = __ballot(fi < 4);
        const uint32_t fl = enders ? (uint32_t)__builtin_ctzll(enders) : WAVE;
        const uint32_t nvalid = ended ? 0u : (lane < fl ? 4u : (lane == fl ? fi : 0u));
        uint32_t bad = 4;
        for (int t = 3; t >= 0; --t)
            if ((uint32_t)t < nvalid && ids[t] >= n) bad = (uint32_t)t;
        const uint64_t bads = __ballot(bad < 4);
        if (bads && lane == (uint32_t)__builtin_ctzll(bads)) page_error(err, PO_NEIGHBOR, blk, item_no, j + bad);
        for (uint32_t t = 0; t < 4; ++t) {
            if (j + t >= R) break;
            uint64_t word = item_pointer_word(0xFFFFFFFFu, 0);
            if (t < nvalid && ids[t] < n) word = pointer_of(ids[t]);
            *reinterpret_cast<po_u64*>(nb + 8 * (j + t)) = word;
        }
        if (enders) ended = true;
    }
}
// The way out of a finished page (after the workgroup's barrier).  DIGEST = false: 512 full-lane 16-byte stores into slot blockIdx.x
// of `out`; true: the 128-bit digest of the page's bytes goes to dg.digest[block b] and, against a baseline, the dirty-byte rule to
// dg.dirty[p] (red: 2 * kOutThreads / WAVE words of LDS).
template <bool DIGEST>
__device__ __forceinline__ void page_out_leave(const uint4* pg4, uint4* __restrict__ out, const PagesDigestArgs& dg, uint64_t* red, uint32_t b,
                                               uint32_t p) {
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    if (!DIGEST) {
        uint4* dst = out + (size_t)blockIdx.x * (kOutPage / 16);
        dst[tid] = pg4[tid];
        dst[tid + kOutThreads] = pg4[tid + kOutThreads];
        return;
    }
    uint64_t sa = 0, sb = 0;
    for (uint32_t i = tid; i < kOutPage / 16; i += kOutThreads) {
        const uint4 v = pg4[i];
        digest_piece(i, (uint64_t)v.x | ((uint64_t)v.y << 32), (uint64_t)v.z | ((uint64_t)v.w << 32), sa, sb);
    }
    for (int m = 1; m < WAVE; m <<= 1) {
        sa += __shfl_xor(sa, m);
        sb += __shfl_xor(sb, m);
    }
    if (lane == 0) {
        red[2 * wave] = sa;
        red[2 * wave + 1] = sb;
    }
    __syncthreads();
    if (tid == 0) {
        sa = sb = 0;
        for (uint32_t w = 0; w < kOutThreads / WAVE; ++w) {
            sa += red[2 * w];
            sb += red[2 * w + 1];
        }
        dg.digest[2 * (size_t)b] = sa;
        dg.digest[2 * (size_t)b + 1] = sb;
        if (dg.dirty) {
            // the byte rule for a node page: past the baseline's end, not a node page then, or other bytes
            bool same = b < dg.base_n_blocks && b >= dg.base_first_node_block && b - dg.base_first_node_block < dg.base_n_node_pages;
            if (same) same = dg.base_digest[2 * (size_t)b] == sa && dg.base_digest[2 * (size_t)b + 1] == sb;
            dg.dirty[p] = same ? 0 : 1;
        }
    }
}

// DIGEST = false: the page leaves as 512 full-lane 16-byte stores (slot blockIdx.x of `out`); true: 16 bytes of digest leave instead.
// page_list (may be null: pages page0, page0 + 1, ...): the node page of every workgroup; VS_INVALID_NODE = this slot is not a node page
template <bool DIGEST>
__global__ __launch_bounds__(kOutThreads) void k_pages_encode(PagesEncodeArgs a, uint32_t page0, const uint32_t* __restrict__ page_list,
                                                              uint4* __restrict__ out, PagesDigestArgs dg, uint32_t* __restrict__ err) {
    __shared__ uint4 pg4[kOutPage / 16];
    __shared__ uint64_t red[2 * kOutThreads / WAVE];
    uint8_t* pg = reinterpret_cast<uint8_t*>(pg4);
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const uint32_t p = page_list ? page_list[blockIdx.x] : page0 + blockIdx.x;  // node page number: block first_node_block + p
    if (p == VS_INVALID_NODE) return;  // (the whole workgroup)
    pg4[tid] = make_uint4(0, 0, 0, 0);
    pg4[tid + kOutThreads] = make_uint4(0, 0, 0, 0);
    uint32_t first, cnt;
    if (a.has_labels) {
        first = a.page_first[p];
        cnt = a.page_first[p + 1] - first;
    } else {
        first = p * a.K;
        cnt = first < a.n ? min(a.K, a.n - first) : 0u;
    }
    __syncthreads();
    const uint32_t body0 = 8 * a.W + 8 * a.R;
    const uint32_t classic_step = (a.item_size + 7u) & ~7u;
    if (tid == 0) {
        uint32_t upper = kOutSpecial;
        if (cnt) upper = a.has_labels ? (uint32_t)a.node_lpoff[first + cnt - 1] : kOutSpecial - cnt * classic_step;
        page_out_header(pg, cnt, upper, (uint32_t)VS_PAGE_SBQ_NODE);
    }
    for (uint32_t k = wave; k < cnt; k += kOutThreads / WAVE) {
        const uint32_t node = first + k;
        uint32_t L = 0, lo = 0, lp_off;
        if (a.has_labels) {
            lo = a.label_off[node];
            L = a.label_off[node + 1] - lo;
            lp_off = a.node_lpoff[node];
        } else {
            lp_off = kOutSpecial - (k + 1) * classic_step;
        }
        const uint32_t root = (body0 + 2 * L + 3u) & ~3u;
        const uint32_t size = root + a.root_size;
        // the layout was fixed at open from the label sets as they were then: an item that no longer fits where it was planned
        // (or would run into the line pointers) is left out and reported, never written
        const uint32_t above = k == 0 ? kOutSpecial : (a.has_labels ? (uint32_t)a.node_lpoff[node - 1] : lp_off + classic_step);
        if (L > 0x8000u || lp_off + ((size + 7u) & ~7u) != above || lp_off < 24 + 4 * cnt || lp_off > kOutSpecial) {
            if (lane == 0) page_error(err, PO_LAYOUT, a.first_node_block + p, k + 1, node);
            continue;
        }
        uint8_t* item = pg + lp_off;
        if (lane == 0) page_out_line_pointer(pg, k, lp_off, size);
        // bq_vector: code rows are code_stride (even) words, 16-byte aligned
        const uint64_t* crow = a.codes + (size_t)node * a.code_stride;
        for (uint32_t w = 2 * lane; w < a.W; w += 2 * WAVE) {
            const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(crow + w);
            *reinterpret_cast<po_u64*>(item + 8 * w) = v.x;
            if (w + 1 < a.W) *reinterpret_cast<po_u64*>(item + 8 * w + 8) = v.y;
        }
        // neighbor_index_pointers: R slots, the list ends at the first VS_INVALID_NODE, (InvalidBlockNumber, 0) from there on
        const uint32_t* nrow = a.nbrs + (size_t)node * a.nbr_stride;  // nbr_stride is a multiple of 16: 64-byte aligned rows
        page_out_neighbors(nrow, item + 8 * a.W, a.R, a.n, lane, err, a.first_node_block + p, k + 1, [&](uint32_t u) {
            if (a.has_labels) {
                const uint32_t blk = a.node_block[u];
                return item_pointer_word(blk, u - a.page_first[blk - a.first_node_block] + 1);
            }
            return item_pointer_word(a.first_node_block + u / a.K, u % a.K + 1);
        });
        // labels (ArchivedLabelSet = ArchivedVec<i16>)
        for (uint32_t j = lane; j < L; j += WAVE) *reinterpret_cast<po_u16*>(item + body0 + 2 * j) = (uint16_t)a.label_val[lo + j];
        // the archived root: heap_item_pointer and three ArchivedVec {i32 offset relative to the field, u32 len}
        if (lane < 4) {
            uint32_t fld, w0, w1;
            if (lane == 0) {
                const uint64_t tid64 = a.tids[node];
                fld = a.o_heap;
                w0 = (uint32_t)(tid64 >> 16);
                w1 = (uint32_t)(tid64 & 0xFFFFu);
            } else if (lane == 1) {
                fld = a.o_code;
                w0 = 0u - (root + fld);
                w1 = a.W;
            } else if (lane == 2) {
                fld = a.o_nbr;
                w0 = 8 * a.W - (root + fld);
                w1 = a.R;
            } else {
                fld = a.o_last;
                w0 = body0 - (root + fld);
                w1 = L;
            }
            *reinterpret_cast<po_u32*>(item + root + fld) = w0;
            *reinterpret_cast<po_u32*>(item + root + fld + 4) = w1;
        }
    }
    __syncthreads();
    page_out_leave<DIGEST>(pg4, out, dg, red, a.first_node_block + p, p);
}

// ---------------------------------------------------------------------------------------------------------------
// The same for `plain` storage (vs_pages_out_open_plain): PlainNode items (AM/plain/node.rs:15-22) on PageType::Node pages.  An item
// is D = num_dimensions_to_index floats, the empty pq_vector, R ArchivedItemPointers and the archived root — 4D + 8R + root_size
// bytes for every node, so K items fill a page and node -> (block, offset) is arithmetic, as for classic SBQ nodes.
//
// k_pages_encode_plain: k_pages_encode's grid, page list convention, error record and way out.  What differs is where the bytes are:
// the vector is most of the page (3 KB of a 3.5 KB item at 768 dimensions, K = 2; K = 1 at 1536), so a wave per item would leave
// three waves idle where it matters.  The vector copy runs over (item, 64 pieces of 16 bytes) units dealt to the four waves: one
// unit is one item's divisor (wave-uniform, loaded once) and one 16-byte global load per lane — rows are vec_stride floats, a
// multiple of 4, so 16-byte aligned; the piece that holds the last floats of an odd D is cut so that nothing is written past 4D.
// Items are MAXALIGNed, not 16-byte aligned: the LDS side is two 8-byte stores per piece.  A 16-lane group of an 8-byte LDS store
// meets 32 banks of 4 bytes; lanes 16 bytes apart would put lanes l and l + 8 on one bank, so lanes 8 .. 15 of every group store
// their high half first and their low half second: each store of a group then covers the 32 banks once.
// PlainNode.vector is the index slice of the row, for cosine divided by the slice's divisor where it has one (preprocess_cosine:
// vnorm, or vnorm_idx when D < dim_full): the `/` of lds_preprocess_cosine, correctly rounded under this unit's compile flags.
// Line pointer, neighbor pointers and the root stay a wave per item.
// ---------------------------------------------------------------------------------------------------------------
struct PagesEncodePlainArgs {
    const float* vecs;
    const float* vdiv;  // cosine: the divisor of every node's index slice (0 = leave the slice alone); else null
    const uint32_t* nbrs;
    const uint64_t* tids;
    uint32_t vec_stride, nbr_stride;
    uint32_t n, D, R;
    uint32_t K, item_size;  // items per page, bytes per item
    uint32_t first_node_block;
    uint32_t root_size, o_heap, o_vec, o_nbr, o_pq;
};

template <bool DIGEST>
__global__ __launch_bounds__(kOutThreads) void k_pages_encode_plain(PagesEncodePlainArgs a, uint32_t page0, const uint32_t* __restrict__ page_list,
                                                                    uint4* __restrict__ out, PagesDigestArgs dg, uint32_t* __restrict__ err) {
    __shared__ uint4 pg4[kOutPage / 16];
    __shared__ uint64_t red[2 * kOutThreads / WAVE];
    uint8_t* pg = reinterpret_cast<uint8_t*>(pg4);
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = rfl(tid / WAVE);
    const uint32_t p = page_list ? page_list[blockIdx.x] : page0 + blockIdx.x;  // node page number: block first_node_block + p
    if (p == VS_INVALID_NODE) return;  // (the whole workgroup)
    pg4[tid] = make_uint4(0, 0, 0, 0);
    pg4[tid + kOutThreads] = make_uint4(0, 0, 0, 0);
    const uint32_t first = p * a.K;
    const uint32_t cnt = first < a.n ? min(a.K, a.n - first) : 0u;
    __syncthreads();
    const uint32_t root = 4 * a.D + 8 * a.R, size = root + a.root_size;
    const uint32_t step = (a.item_size + 7u) & ~7u;
    if (tid == 0) page_out_header(pg, cnt, kOutSpecial - cnt * step, (uint32_t)VS_PAGE_NODE);
    // the layout was fixed at open: an item that is not where it was planned, or would run into the line pointers, is left out and
    // reported (by the wave that owns the item), never written
    auto planned = [&](uint32_t k, uint32_t& lp_off) {
        const uint32_t used = (k + 1) * step;  // (size <= step: the item ends at or below the one above it)
        lp_off = kOutSpecial - used;
        return size == a.item_size && used <= kOutSpecial - 24 - 4 * cnt;
    };
    // the vectors: unit u = 64 pieces of item u / C
    const uint32_t P = (a.D + 3) / 4, C = (P + WAVE - 1) / WAVE;
    for (uint32_t u = wave; u < cnt * C; u += kOutThreads / WAVE) {
        const uint32_t k = u / C, q = (u % C) * WAVE + lane;
        uint32_t lp_off;
        if (!planned(k, lp_off)) continue;
        const uint32_t node = first + k;
        const float s = a.vdiv ? a.vdiv[node] : 0.0f;
        if (q >= P) continue;
        float4 v = *reinterpret_cast<const float4*>(a.vecs + (size_t)node * a.vec_stride + 4 * q);
        if (s != 0.0f) {
            v.x = v.x / s;
            v.y = v.y / s;
            v.z = v.z / s;
            v.w = v.w / s;
        }
        const uint32_t have = a.D - 4 * q;  // floats of this piece that belong to the vector (>= 1)
        const bool hi_first = (lane & 8u) != 0;
        uint8_t* dst = pg + lp_off + 16 * q;
        for (int t = 0; t < 2; ++t) {
            const bool hi = (t == 0) == hi_first;
            const uint32_t f0 = __float_as_uint(hi ? v.z : v.x), f1 = __float_as_uint(hi ? v.w : v.y), at = hi ? 2u : 0u;
            if (have >= at + 2) *reinterpret_cast<po_u64*>(dst + 4 * at) = (uint64_t)f0 | ((uint64_t)f1 << 32);
            else if (have > at) *reinterpret_cast<po_u32*>(dst + 4 * at) = f0;
        }
    }
    for (uint32_t k = wave; k < cnt; k += kOutThreads / WAVE) {
        const uint32_t node = first + k;
        uint32_t lp_off;
        if (!planned(k, lp_off)) {
            if (lane == 0) page_error(err, PO_LAYOUT, a.first_node_block + p, k + 1, node);
            continue;
        }
        uint8_t* item = pg + lp_off;
        if (lane == 0) page_out_line_pointer(pg, k, lp_off, size);
        page_out_neighbors(a.nbrs + (size_t)node * a.nbr_stride, item + 4 * a.D, a.R, a.n, lane, err, a.first_node_block + p, k + 1,
                           [&](uint32_t v) { return item_pointer_word(a.first_node_block + v / a.K, v % a.K + 1); });
        // the archived root: heap_item_pointer and three ArchivedVec {i32 offset relative to the field, u32 len}; the empty pq_vector
        // points at the end of the vector, where rkyv's serializer stood when it met it
        if (lane < 4) {
            uint32_t fld, w0, w1;
            if (lane == 0) {
                const uint64_t tid64 = a.tids[node];
                fld = a.o_heap;
                w0 = (uint32_t)(tid64 >> 16);
                w1 = (uint32_t)(tid64 & 0xFFFFu);
            } else if (lane == 1) {
                fld = a.o_vec;
                w0 = 0u - (root + fld);
                w1 = a.D;
            } else if (lane == 2) {
                fld = a.o_nbr;
                w0 = 4 * a.D - (root + fld);
                w1 = a.R;
            } else {
                fld = a.o_pq;
                w0 = 4 * a.D - (root + fld);
                w1 = 0;
            }
            *reinterpret_cast<po_u32*>(item + root + fld) = w0;
            *reinterpret_cast<po_u32*>(item + root + fld + 4) = w1;
        }
    }
    __syncthreads();
    page_out_leave<DIGEST>(pg4, out, dg, red, a.first_node_block + p, p);
}

// The dirty node pages as an ascending list of block numbers.  Three passes, so that the order is the pages' own and not that of an
// atomic slot counter: dirty pages per wave of 64 pages (ballot), one exclusive scan over the waves' counts, then every dirty page
// writes itself at its wave's offset + its rank among the wave's dirty lanes.
__global__ __launch_bounds__(256) void k_pages_dirty_count(const uint8_t* __restrict__ dirty, uint32_t n, uint32_t* __restrict__ wave_cnt) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint64_t m = __ballot(i < n && dirty[i] != 0);
    if ((threadIdx.x & (WAVE - 1)) == 0) wave_cnt[i / WAVE] = (uint32_t)__popcll(m);
}
// one workgroup: v[0 .. m) becomes its exclusive prefix sums, v[m] the total
__global__ __launch_bounds__(256) void k_pages_scan_counts(uint32_t* __restrict__ v, uint32_t m) {
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
__global__ __launch_bounds__(256) void k_pages_dirty_scatter(const uint8_t* __restrict__ dirty, uint32_t n, const uint32_t* __restrict__ wave_off,
                                                             uint32_t first_node_block, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & (WAVE - 1);
    const bool d = i < n && dirty[i] != 0;
    const uint64_t m = __ballot(d);
    if (d) out[wave_off[i / WAVE] + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = first_node_block + i;
}

// nodes whose heap_item_pointer.offset is InvalidOffsetNumber
__global__ __launch_bounds__(256) void k_pages_count_deleted(const uint64_t* __restrict__ tids, uint32_t n, uint32_t* __restrict__ out) {
    uint32_t c = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) c += (tids[i] & 0xFFFFu) == 0;
    if (c) atomicAdd(out, c);
}

struct vs_pages_out {
    vs_index* ix = nullptr;
    vs_ctx* ctx = nullptr;
    PagesOutPlan plan;
    PagesEncodeArgs args{};
    PagesEncodePlainArgs plain_args{};  // plan.plain: what k_pages_encode_plain takes instead
    uint32_t* d_page_first = nullptr;
    uint32_t* d_node_block = nullptr;
    uint16_t* d_node_lpoff = nullptr;
    uint8_t* d_stage[2] = {nullptr, nullptr};  // one chunk of node pages each, as large as a pinned staging buffer
    uint32_t* d_err = nullptr;
    hipEvent_t ev_done[2] = {nullptr, nullptr};  // the encode of the chunk in d_stage[i] has finished
    uint32_t chunk_pages = 0;
    uint32_t* d_list = nullptr;  // the node pages of a vs_pages_out_read_blocks call (grow-only)
    size_t list_cap = 0;
    std::vector<uint32_t> delta;  // the dirty blocks of the last vs_pages_out_delta (ascending)
    uint64_t owner_id = 0;        // != 0: counted among the open writers of that index (vs_index_open_writers)
};

extern "C" void vs_pages_out_close(vs_pages_out* w) {
    if (!w) return;
    if (w->owner_id) vs_index_writer_closed(w->owner_id);
    if (w->ctx) (void)hipSetDevice(w->ctx->device);
    if (w->d_page_first) (void)hipFree(w->d_page_first);
    if (w->d_node_block) (void)hipFree(w->d_node_block);
    if (w->d_node_lpoff) (void)hipFree(w->d_node_lpoff);
    for (int i = 0; i < 2; ++i) {
        if (w->d_stage[i]) (void)hipFree(w->d_stage[i]);
        if (w->ev_done[i]) (void)hipEventDestroy(w->ev_done[i]);
    }
    if (w->d_err) (void)hipFree(w->d_err);
    if (w->d_list) (void)hipFree(w->d_list);
    delete w;
}

static int pages_out_open_finish(vs_index* ix, vs_pages_out* w, vs_pages_info* info);

static int pages_out_open_impl(vs_index* ix, const vs_pages_out_params* p, vs_pages_out* w, vs_pages_info* info) {
    vs_ctx* c = ix->ctx;
    const vs_index_desc& d = ix->d;
    VS_HIP(hipSetDevice(c->device));
    VS_REQUIRE(c->pinned_bytes >= p->page_size, "vs_pages_out_open: the context's staging buffers (%zu bytes) do not hold one page", c->pinned_bytes);
    // what the host half needs: quantizer, label offsets (labeled nodes), the labeled start nodes
    std::vector<float> mean(d.dim_index), m2(d.dim_index);
    uint64_t count = 0;
    VS_TRY(vs_index_get_quantizer(ix, mean.data(), m2.data(), &count));
    std::vector<uint32_t> label_off;
    if (d.has_labels) {
        VS_REQUIRE(ix->label_off && ix->label_val, "vs_pages_out_open: the index says has_labels but holds no label sets");
        label_off.resize((size_t)d.n + 1);
        VS_TRY(vs_dev_download(c, label_off.data(), ix->label_off, ((size_t)d.n + 1) * 4));
    }
    std::vector<int16_t> ls_labels(d.n_label_starts);
    std::vector<uint32_t> ls_nodes(d.n_label_starts);
    if (d.n_label_starts) {
        VS_TRY(vs_dev_download(c, ls_labels.data(), ix->ls_labels, (size_t)d.n_label_starts * 2));
        VS_TRY(vs_dev_download(c, ls_nodes.data(), ix->ls_nodes, (size_t)d.n_label_starts * 4));
    }
    VS_TRY(vs_pages_out_plan(d, *p, mean.data(), m2.data(), count, d.has_labels ? label_off.data() : nullptr, ls_labels.data(), ls_nodes.data(),
                             w->plan));
    PagesOutPlan& plan = w->plan;
    if (plan.has_labels) {
        VS_HIP(hipMalloc(&w->d_page_first, plan.page_first.size() * 4));
        VS_HIP(hipMalloc(&w->d_node_block, std::max<size_t>(plan.node_block.size(), 1) * 4));
        VS_HIP(hipMalloc(&w->d_node_lpoff, std::max<size_t>(plan.node_lpoff.size(), 1) * 2));
        VS_TRY(vs_dev_upload(c, w->d_page_first, plan.page_first.data(), plan.page_first.size() * 4));
        VS_TRY(vs_dev_upload(c, w->d_node_block, plan.node_block.data(), plan.node_block.size() * 4));
        VS_TRY(vs_dev_upload(c, w->d_node_lpoff, plan.node_lpoff.data(), plan.node_lpoff.size() * 2));
        std::vector<uint32_t>().swap(plan.node_block);  // the host keeps page_first only (vs_pages_out_item_pointer_of)
        std::vector<uint16_t>().swap(plan.node_lpoff);
    }
    PagesEncodeArgs& a = w->args;
    a.codes = ix->codes;
    a.nbrs = ix->nbrs;
    a.tids = ix->tids;
    a.label_off = plan.has_labels ? ix->label_off : nullptr;
    a.label_val = plan.has_labels ? ix->label_val : nullptr;
    a.page_first = w->d_page_first;
    a.node_block = w->d_node_block;
    a.node_lpoff = w->d_node_lpoff;
    a.code_stride = ix->code_stride;
    a.nbr_stride = ix->nbr_stride;
    a.n = d.n;
    a.W = d.words;
    a.R = d.num_neighbors;
    a.K = plan.K;
    a.item_size = plan.item_size;
    a.first_node_block = plan.first_node_block;
    a.root_size = plan.lay.root_size;
    a.o_heap = plan.lay.off_heap_item_pointer;
    a.o_code = plan.lay.off_bq_vector;
    a.o_nbr = plan.lay.off_neighbor_index_pointers;
    a.o_last = plan.lay.off_labels;
    a.has_labels = plan.has_labels ? 1u : 0u;
    return pages_out_open_finish(ix, w, info);
}

// what both opens end with, the plan made: the staging chunks, the error record, and what a reader of the result reports
static int pages_out_open_finish(vs_index* ix, vs_pages_out* w, vs_pages_info* info) {
    vs_ctx* c = ix->ctx;
    const vs_index_desc& d = ix->d;
    const PagesOutPlan& plan = w->plan;
    w->chunk_pages = (uint32_t)std::min<size_t>(c->pinned_bytes / plan.page_size, std::max<uint32_t>(plan.n_node_pages, 1));
    for (int i = 0; i < 2; ++i) {
        VS_HIP(hipMalloc(&w->d_stage[i], (size_t)w->chunk_pages * plan.page_size));
        VS_HIP(hipEventCreateWithFlags(&w->ev_done[i], hipEventDisableTiming));
    }
    VS_HIP(hipMalloc(&w->d_err, 32));
    VS_HIP(hipMemsetAsync(w->d_err, 0, 32, c->stream));
    // n_deleted, as a reader of the result counts it
    uint32_t n_deleted = 0;
    if (d.n) {
        hipLaunchKernelGGL(k_pages_count_deleted, dim3(std::min<uint32_t>((d.n + 255) / 256, 1024)), dim3(256), 0, c->stream, (const uint64_t*)ix->tids,
                           d.n, w->d_err + 4);
        VS_HIP(hipGetLastError());
        VS_HIP(hipMemcpyAsync(&n_deleted, w->d_err + 4, 4, hipMemcpyDeviceToHost, c->stream));
    }
    VS_HIP(hipStreamSynchronize(c->stream));
    if (info) {
        memset(info, 0, sizeof *info);
        info->n_blocks = plan.n_blocks;
        info->n_nodes = d.n;
        info->words = plan.W;
        info->num_neighbors = d.num_neighbors;
        info->has_labels = plan.has_labels;
        info->n_deleted = n_deleted;
        info->n_label_vals = plan.n_label_vals;
        for (int t = 0; t < 9; ++t) info->pages_by_type[t] = plan.pages_by_type[t];
        info->meta_magic = 768756476u;  // TSV_MAGIC_NUMBER (AM/meta_page.rs:22)
        info->meta_version = 3;
    }
    return VS_OK;
}

extern "C" int vs_pages_out_open(vs_index* ix, const vs_pages_out_params* p, vs_pages_out** out, vs_pages_info* info) {
    VS_REQUIRE(ix && p && out, "vs_pages_out_open: bad args");
    *out = nullptr;
    VS_REQUIRE(ix->d.storage_type == VS_STORAGE_SBQ, "vs_pages_out_open: memory_optimized (SBQ) indexes only; a `plain` index is written with vs_pages_out_open_plain");
    VS_REQUIRE(ix->codes && ix->nbrs && ix->tids, "vs_pages_out_open: the index holds no codes / neighbors");
    return vs_guard("vs_pages_out_open", [&] {
        vs_pages_out* w = new vs_pages_out();
        w->ix = ix;
        w->ctx = ix->ctx;
        const int r = pages_out_open_impl(ix, p, w, info);
        if (r != VS_OK) {
            vs_pages_out_close(w);
            return r;
        }
        w->owner_id = ix->owner_id;
        vs_index_writer_opened(w->owner_id);
        *out = w;
        return (int)VS_OK;
    });
}

static int pages_out_open_plain_impl(vs_index* ix, const vs_pages_out_params* p, vs_pages_out* w, vs_pages_info* info) {
    vs_ctx* c = ix->ctx;
    const vs_index_desc& d = ix->d;
    VS_HIP(hipSetDevice(c->device));
    VS_REQUIRE(c->pinned_bytes >= p->page_size, "vs_pages_out_open_plain: the context's staging buffers (%zu bytes) do not hold one page", c->pinned_bytes);
    VS_TRY(vs_pages_out_plan_plain(d, *p, w->plan));
    const PagesOutPlan& plan = w->plan;
    PagesEncodePlainArgs& a = w->plain_args;
    a.vecs = ix->vecs;
    a.vdiv = d.distance_type == VS_COSINE ? (d.dim_index < d.dim_full ? ix->vnorm_idx : ix->vnorm) : nullptr;
    a.nbrs = ix->nbrs;
    a.tids = ix->tids;
    a.vec_stride = ix->vec_stride;
    a.nbr_stride = ix->nbr_stride;
    a.n = d.n;
    a.D = d.dim_index;
    a.R = d.num_neighbors;
    a.K = plan.K;
    a.item_size = plan.item_size;
    a.first_node_block = plan.first_node_block;
    a.root_size = plan.lay.root_size;
    a.o_heap = plan.lay.off_heap_item_pointer;
    a.o_vec = plan.lay.off_bq_vector;
    a.o_nbr = plan.lay.off_neighbor_index_pointers;
    a.o_pq = plan.lay.off_labels;
    return pages_out_open_finish(ix, w, info);
}

extern "C" int vs_pages_out_open_plain(vs_index* ix, const vs_pages_out_params* p, vs_pages_out** out, vs_pages_info* info) {
    VS_REQUIRE(ix && p && out, "vs_pages_out_open_plain: bad args");
    *out = nullptr;
    VS_REQUIRE(ix->d.storage_type == VS_STORAGE_PLAIN, "vs_pages_out_open_plain: `plain` indexes only; a memory_optimized (SBQ) index is written with "
               "vs_pages_out_open");
    VS_REQUIRE(ix->vecs && ix->nbrs && ix->tids, "vs_pages_out_open_plain: the index holds no vector column / neighbors / heap tids");
    VS_REQUIRE(ix->d.distance_type != VS_COSINE || (ix->d.dim_index < ix->d.dim_full ? ix->vnorm_idx : ix->vnorm),
               "vs_pages_out_open_plain: the index has no divisors for its index slices (vs_index_refresh_norms)");
    VS_REQUIRE(ix->vec_stride % 4 == 0 && ix->d.dim_index <= ix->d.dim_full, "vs_pages_out_open_plain: vector rows of %u floats for %u dimensions",
               ix->vec_stride, ix->d.dim_index);
    return vs_guard("vs_pages_out_open_plain", [&] {
        vs_pages_out* w = new vs_pages_out();
        w->ix = ix;
        w->ctx = ix->ctx;
        const int r = pages_out_open_plain_impl(ix, p, w, info);
        if (r != VS_OK) {
            vs_pages_out_close(w);
            return r;
        }
        w->owner_id = ix->owner_id;
        vs_index_writer_opened(w->owner_id);
        *out = w;
        return (int)VS_OK;
    });
}

extern "C" int vs_pages_out_item_pointer_of(const vs_pages_out* w, uint32_t node, uint32_t* block, uint32_t* offset) {
    VS_REQUIRE(w, "vs_pages_out_item_pointer_of: null writer");
    return vs_pages_out_plan_item_pointer(w->plan, node, block, offset);
}

// node pages [p0, p0 + np) — or, with d_list, the np pages it names — into d_out, on the compute stream
static int launch_pages_encode(vs_pages_out* w, uint32_t p0, const uint32_t* d_list, uint32_t np, void* d_out) {
    vs_ctx* c = w->ctx;
    hipEvent_t ev = prof_begin(c);
    if (w->plan.plain)
        hipLaunchKernelGGL((k_pages_encode_plain<false>), dim3(np), dim3(kOutThreads), 0, c->stream, w->plain_args, p0, d_list,
                           reinterpret_cast<uint4*>(d_out), PagesDigestArgs{}, w->d_err);
    else
        hipLaunchKernelGGL((k_pages_encode<false>), dim3(np), dim3(kOutThreads), 0, c->stream, w->args, p0, d_list, reinterpret_cast<uint4*>(d_out),
                           PagesDigestArgs{}, w->d_err);
    VS_HIP(hipGetLastError());
    prof_end(c, PK_PAGES, ev);
    return VS_OK;
}

// after the stream has been synchronised: what the kernels reported
static int pages_out_check(vs_pages_out* w) {
    uint32_t herr[4] = {0, 0, 0, 0};
    VS_HIP(hipMemcpy(herr, w->d_err, 16, hipMemcpyDeviceToHost));
    if (herr[0] == PO_OK) return VS_OK;
    VS_HIP(hipMemset(w->d_err, 0, 16));
    if (herr[0] == PO_NEIGHBOR) vs_set_error("block %u item %u: neighbor slot %u names a node the index does not have", herr[1], herr[2], herr[3]);
    else if (w->plan.plain) vs_set_error("block %u item %u (node %u): the item does not lie where vs_pages_out_open_plain planned it", herr[1], herr[2], herr[3]);
    else vs_set_error("block %u item %u (node %u): the label sets changed after vs_pages_out_open fixed the layout", herr[1], herr[2], herr[3]);
    return VS_ERR_INVALID;
}

// the metadata pages inside [first_block, first_block + n_blocks): fn(block, bytes)
template <class F>
static int pages_out_host_pages(const vs_pages_out* w, uint32_t first_block, uint32_t n_blocks, F&& fn) {
    for (const auto& hp : w->plan.host_pages)
        if (hp.first >= first_block && hp.first - first_block < n_blocks) VS_TRY(fn(hp.first, hp.second.data()));
    return VS_OK;
}

static int pages_out_range(const vs_pages_out* w, const char* what, uint32_t first_block, uint32_t n_blocks, const void* pages, uint32_t* p0,
                           uint32_t* np) {
    VS_REQUIRE(w && (pages || !n_blocks), "%s: bad args", what);
    VS_REQUIRE((uint64_t)first_block + n_blocks <= w->plan.n_blocks, "%s: blocks %u .. %llu of a relation of %u blocks", what, first_block,
               (unsigned long long)first_block + n_blocks, w->plan.n_blocks);
    const uint32_t fnb = w->plan.first_node_block, end = first_block + n_blocks;
    const uint32_t lo = std::max(first_block, fnb), hi = std::min(end, fnb + w->plan.n_node_pages);
    *p0 = lo < hi ? lo - fnb : 0;
    *np = lo < hi ? hi - lo : 0;
    return VS_OK;
}

// np node pages through the pinned ring.  Chunk i is encoded into d_stage[i & 1] on the compute stream (launch(q0, qn, d_stage)),
// copied to pinned[i & 1] on the copy stream once its kernel has finished, and drained to the caller's buffer (drain(q0, qn, pinned))
// when its slot comes round again: the kernel of chunk i + 1 runs under the copy of chunk i, the host's copy out of one pinned buffer
// under the transfer into the other (as vs_dev_download).  The kernel of chunk i is queued BEFORE the host drains chunk i - 2 out of
// pinned[i & 1]: it waits on the device for that chunk's transfer (d_stage[i & 1] is free then), not for the host's memcpy; only the
// transfer into pinned[i & 1] comes after the drain.
template <class Launch, class Drain>
static int pages_out_pump(vs_pages_out* w, uint32_t np, Launch&& launch, Drain&& drain) {
    vs_ctx* c = w->ctx;
    const size_t ps = w->plan.page_size;
    const uint32_t nchunks = (np + w->chunk_pages - 1) / w->chunk_pages;
    uint32_t pend_q0[2] = {0, 0}, pend_n[2] = {0, 0};
    auto pump = [&]() -> int {
        for (uint32_t i = 0; i < nchunks + 2; ++i) {
            const int slot = (int)(i & 1);
            const uint32_t q0 = i * w->chunk_pages, qn = i < nchunks ? std::min(w->chunk_pages, np - q0) : 0;
            if (qn) {
                if (pend_n[slot]) VS_HIP(hipStreamWaitEvent(c->stream, c->pinned_ev[slot], 0));
                VS_TRY(launch(q0, qn, w->d_stage[slot]));
                VS_HIP(hipEventRecord(w->ev_done[slot], c->stream));
            }
            if (pend_n[slot]) {
                VS_HIP(hipEventSynchronize(c->pinned_ev[slot]));
                drain(pend_q0[slot], pend_n[slot], static_cast<const uint8_t*>(c->pinned[slot]));
                pend_n[slot] = 0;
            }
            if (qn) {
                VS_HIP(hipStreamWaitEvent(c->copy_stream, w->ev_done[slot], 0));
                VS_HIP(hipMemcpyAsync(c->pinned[slot], w->d_stage[slot], (size_t)qn * ps, hipMemcpyDeviceToHost, c->copy_stream));
                VS_HIP(hipEventRecord(c->pinned_ev[slot], c->copy_stream));
                pend_q0[slot] = q0;
                pend_n[slot] = qn;
            }
        }
        return VS_OK;
    };
    const int rc = pump();
    if (rc != VS_OK) {  // nothing may still be on its way into the context's pinned buffers when the call returns
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamSynchronize(c->copy_stream);
        return rc;
    }
    VS_HIP(hipStreamSynchronize(c->stream));
    return pages_out_check(w);
}

static int pages_out_read_impl(vs_pages_out* w, uint32_t first_block, uint32_t n_blocks, void* pages) {
    uint32_t p0 = 0, np = 0;
    VS_TRY(pages_out_range(w, "vs_pages_out_read", first_block, n_blocks, pages, &p0, &np));
    vs_ctx* c = w->ctx;
    const size_t ps = w->plan.page_size;
    uint8_t* dst = static_cast<uint8_t*>(pages);
    VS_HIP(hipSetDevice(c->device));
    VS_TRY(pages_out_host_pages(w, first_block, n_blocks, [&](uint32_t blk, const uint8_t* bytes) {
        memcpy(dst + (size_t)(blk - first_block) * ps, bytes, ps);
        return (int)VS_OK;
    }));
    if (np == 0) return VS_OK;
    uint8_t* node_dst = dst + (size_t)(w->plan.first_node_block + p0 - first_block) * ps;
    return pages_out_pump(
        w, np, [&](uint32_t q0, uint32_t qn, uint8_t* d_stage) { return launch_pages_encode(w, p0 + q0, nullptr, qn, d_stage); },
        [&](uint32_t q0, uint32_t qn, const uint8_t* pinned) { stage_copy(node_dst + (size_t)q0 * ps, pinned, (size_t)qn * ps); });
}

extern "C" int vs_pages_out_read(vs_pages_out* w, uint32_t first_block, uint32_t n_blocks, void* pages) {
    return vs_guard("vs_pages_out_read", [&] { return pages_out_read_impl(w, first_block, n_blocks, pages); });
}

static int pages_out_read_dev_impl(vs_pages_out* w, uint32_t first_block, uint32_t n_blocks, void* d_pages) {
    uint32_t p0 = 0, np = 0;
    VS_TRY(pages_out_range(w, "vs_pages_out_read_dev", first_block, n_blocks, d_pages, &p0, &np));
    vs_ctx* c = w->ctx;
    const size_t ps = w->plan.page_size;
    uint8_t* dst = static_cast<uint8_t*>(d_pages);
    VS_REQUIRE(((uintptr_t)dst & 15) == 0, "vs_pages_out_read_dev: the device buffer must be 16-byte aligned");
    VS_HIP(hipSetDevice(c->device));
    if (np) VS_TRY(launch_pages_encode(w, p0, nullptr, np, dst + (size_t)(w->plan.first_node_block + p0 - first_block) * ps));
    VS_TRY(pages_out_host_pages(w, first_block, n_blocks, [&](uint32_t blk, const uint8_t* bytes) {
        return vs_dev_upload(c, dst + (size_t)(blk - first_block) * ps, bytes, ps);
    }));
    VS_HIP(hipStreamSynchronize(c->stream));
    return pages_out_check(w);
}

extern "C" int vs_pages_out_read_dev(vs_pages_out* w, uint32_t first_block, uint32_t n_blocks, void* d_pages) {
    return vs_guard("vs_pages_out_read_dev", [&] { return pages_out_read_dev_impl(w, first_block, n_blocks, d_pages); });
}

// ---------------------------------------------------------------------------------------------------------------
// Page by page (vs_pages_out_baseline / _delta / _read_blocks): what bulk_delete_for_storage (AM/vacuum.rs:80-136, page.commit()
// only `if modified`) and aminsert (AM/build.rs:464-558) do to the relation — only the pages a change touched are written.  A
// baseline is one digest per block of the relation as this writer last produced it; the digest pass is k_pages_encode with the
// digest as its tail instead of the 8 KB of stores, so whatever decides a page's bytes decides its digest.
// ---------------------------------------------------------------------------------------------------------------
extern "C" void vs_pages_base_free(vs_pages_base* b) {
    if (!b) return;
    if (b->d_digest) {
        (void)hipSetDevice(b->device);
        (void)hipFree(b->d_digest);
    }
    delete b;
}

extern "C" uint32_t vs_pages_base_blocks(const vs_pages_base* b) { return b ? b->n_blocks : 0; }

// One digest pass over every node page of w.  base (may be null): the dirty blocks land in w->delta; out (may be null): the
// baseline of the relation as it is now.
static int pages_out_digest_impl(vs_pages_out* w, const char* what, const vs_pages_base* base, vs_pages_base** out) {
    vs_ctx* c = w->ctx;
    const PagesOutPlan& plan = w->plan;
    VS_HIP(hipSetDevice(c->device));
    if (base) {
        VS_REQUIRE(base->device == c->device, "%s: the baseline lives on device %d, the writer on device %d", what, base->device, c->device);
        VS_REQUIRE(base->page_size == plan.page_size, "%s: the baseline is one of %u-byte pages", what, base->page_size);
    }
    const uint32_t np = plan.n_node_pages;
    const uint32_t waves = (np + 255) / 256 * (256 / WAVE);
    uint64_t* d_digest = nullptr;
    uint8_t* d_dirty = nullptr;
    uint32_t *d_wave = nullptr, *d_blocks = nullptr;
    auto release = [&] {
        if (d_digest) (void)hipFree(d_digest);
        if (d_dirty) (void)hipFree(d_dirty);
        if (d_wave) (void)hipFree(d_wave);
        if (d_blocks) (void)hipFree(d_blocks);
    };
    std::vector<uint32_t> node_dirty;
    auto run = [&]() -> int {
        VS_HIP(hipMalloc(&d_digest, (size_t)std::max<uint32_t>(plan.n_blocks, 1) * 16));
        VS_HIP(hipMemsetAsync(d_digest, 0, (size_t)std::max<uint32_t>(plan.n_blocks, 1) * 16, c->stream));
        if (base && np) {
            VS_HIP(hipMalloc(&d_dirty, np));
            VS_HIP(hipMalloc(&d_wave, ((size_t)waves + 1) * 4));
            VS_HIP(hipMalloc(&d_blocks, (size_t)np * 4));
        }
        uint32_t n_dirty = 0;
        if (np) {
            PagesDigestArgs dg{};
            dg.digest = d_digest;
            dg.base_digest = base ? base->d_digest : nullptr;
            dg.dirty = d_dirty;
            dg.base_n_blocks = base ? base->n_blocks : 0;
            dg.base_first_node_block = base ? base->first_node_block : 0;
            dg.base_n_node_pages = base ? base->n_node_pages : 0;
            hipEvent_t ev = prof_begin(c);
            if (plan.plain)
                hipLaunchKernelGGL((k_pages_encode_plain<true>), dim3(np), dim3(kOutThreads), 0, c->stream, w->plain_args, 0u,
                                   (const uint32_t*)nullptr, (uint4*)nullptr, dg, w->d_err);
            else
                hipLaunchKernelGGL((k_pages_encode<true>), dim3(np), dim3(kOutThreads), 0, c->stream, w->args, 0u, (const uint32_t*)nullptr,
                                   (uint4*)nullptr, dg, w->d_err);
            VS_HIP(hipGetLastError());
            prof_end(c, PK_PAGES, ev);
            if (base) {
                hipLaunchKernelGGL(k_pages_dirty_count, dim3((np + 255) / 256), dim3(256), 0, c->stream, (const uint8_t*)d_dirty, np, d_wave);
                VS_HIP(hipGetLastError());
                hipLaunchKernelGGL(k_pages_scan_counts, dim3(1), dim3(256), 0, c->stream, d_wave, waves);
                VS_HIP(hipGetLastError());
                hipLaunchKernelGGL(k_pages_dirty_scatter, dim3((np + 255) / 256), dim3(256), 0, c->stream, (const uint8_t*)d_dirty, np,
                                   (const uint32_t*)d_wave, plan.first_node_block, d_blocks);
                VS_HIP(hipGetLastError());
                VS_HIP(hipMemcpyAsync(&n_dirty, d_wave + waves, 4, hipMemcpyDeviceToHost, c->stream));
            }
        }
        VS_HIP(hipStreamSynchronize(c->stream));
        VS_TRY(pages_out_check(w));
        VS_REQUIRE(n_dirty <= np, "%s: the dirty list holds %u of %u node pages", what, n_dirty, np);
        node_dirty.resize(n_dirty);
        if (n_dirty) VS_TRY(vs_dev_download(c, node_dirty.data(), d_blocks, (size_t)n_dirty * 4));
        return VS_OK;
    };
    const int rc = run();
    if (rc != VS_OK) {
        (void)hipStreamSynchronize(c->stream);
        release();
        return rc;
    }
    if (base) {
        std::vector<uint32_t> host_dirty;
        vs_pages_out_host_delta(plan, *base, host_dirty);
        w->delta.resize(node_dirty.size() + host_dirty.size());
        std::merge(node_dirty.begin(), node_dirty.end(), host_dirty.begin(), host_dirty.end(), w->delta.begin());
    }
    if (out) {
        vs_pages_base* nb = new vs_pages_base();
        nb->device = c->device;
        nb->page_size = plan.page_size;
        nb->n_blocks = plan.n_blocks;
        nb->first_node_block = plan.first_node_block;
        nb->n_node_pages = np;
        nb->host_pages = plan.host_pages;
        nb->d_digest = d_digest;
        d_digest = nullptr;
        *out = nb;
    }
    release();
    return VS_OK;
}

extern "C" int vs_pages_out_baseline(vs_pages_out* w, vs_pages_base** out) {
    VS_REQUIRE(w && out, "vs_pages_out_baseline: bad args");
    *out = nullptr;
    return vs_guard("vs_pages_out_baseline", [&] { return pages_out_digest_impl(w, "vs_pages_out_baseline", nullptr, out); });
}

extern "C" int vs_pages_out_delta(vs_pages_out* w, const vs_pages_base* base, uint32_t* n_dirty, uint32_t* n_blocks_now,
                                  vs_pages_base** new_base) {
    VS_REQUIRE(w && base && n_dirty, "vs_pages_out_delta: bad args");
    if (new_base) *new_base = nullptr;
    *n_dirty = 0;
    w->delta.clear();
    const int rc = vs_guard("vs_pages_out_delta", [&] { return pages_out_digest_impl(w, "vs_pages_out_delta", base, new_base); });
    if (rc != VS_OK) {
        w->delta.clear();
        return rc;
    }
    *n_dirty = (uint32_t)w->delta.size();
    if (n_blocks_now) *n_blocks_now = w->plan.n_blocks;
    return VS_OK;
}

extern "C" int vs_pages_out_delta_blocks(const vs_pages_out* w, uint32_t* blocks, uint32_t cap) {
    VS_REQUIRE(w && (blocks || w->delta.empty()), "vs_pages_out_delta_blocks: bad args");
    VS_REQUIRE(cap >= w->delta.size(), "vs_pages_out_delta_blocks: room for %u of %zu blocks", cap, w->delta.size());
    if (!w->delta.empty()) memcpy(blocks, w->delta.data(), w->delta.size() * 4);
    return VS_OK;
}

// what every block of the list is: the host-encoded page (host[i] != null) or node page list[i]; nothing has been written when
// a block fails the check
static int pages_out_classify(const vs_pages_out* w, const char* what, const uint32_t* blocks, uint32_t n, const void* pages,
                              std::vector<uint32_t>& list, std::vector<const uint8_t*>& host) {
    VS_REQUIRE(w && (n == 0 || (blocks && pages)), "%s: bad args", what);
    const PagesOutPlan& plan = w->plan;
    list.assign(n, VS_INVALID_NODE);
    host.assign(n, nullptr);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t b = blocks[i];
        VS_REQUIRE(b < plan.n_blocks, "%s: blocks[%u] = %u of a relation of %u blocks", what, i, b, plan.n_blocks);
        if (b >= plan.first_node_block && b - plan.first_node_block < plan.n_node_pages) {
            list[i] = b - plan.first_node_block;
        } else {
            host[i] = vs_pages_out_plan_host_page(plan, b);
            VS_REQUIRE(host[i], "%s: block %u is neither a node page nor a page the host encoded", what, b);
        }
    }
    return VS_OK;
}

static int pages_out_list_reserve(vs_pages_out* w, size_t n) {
    if (n <= w->list_cap) return VS_OK;
    if (w->d_list) VS_HIP(hipFree(w->d_list));
    w->d_list = nullptr;
    w->list_cap = 0;
    VS_HIP(hipMalloc(&w->d_list, n * 4));
    w->list_cap = n;
    return VS_OK;
}

static int pages_out_read_blocks_impl(vs_pages_out* w, const uint32_t* blocks, uint32_t n, void* pages) {
    std::vector<uint32_t> list;
    std::vector<const uint8_t*> host;
    VS_TRY(pages_out_classify(w, "vs_pages_out_read_blocks", blocks, n, pages, list, host));
    vs_ctx* c = w->ctx;
    const size_t ps = w->plan.page_size;
    uint8_t* dst = static_cast<uint8_t*>(pages);
    VS_HIP(hipSetDevice(c->device));
    // the node pages of the list, in list order, and the slot of the output each one goes to
    std::vector<uint32_t> node_pages, slot;
    for (uint32_t i = 0; i < n; ++i) {
        if (host[i]) {
            memcpy(dst + (size_t)i * ps, host[i], ps);
        } else {
            node_pages.push_back(list[i]);
            slot.push_back(i);
        }
    }
    const uint32_t np = (uint32_t)node_pages.size();
    if (np == 0) return VS_OK;
    VS_TRY(pages_out_list_reserve(w, np));
    VS_TRY(vs_dev_upload(c, w->d_list, node_pages.data(), (size_t)np * 4));
    // chunks are cut from the list; a chunk's pages go to their slots run by run (neighbours in the list are neighbours in the output
    // unless a host-encoded page sits between them)
    return pages_out_pump(
        w, np, [&](uint32_t q0, uint32_t qn, uint8_t* d_stage) { return launch_pages_encode(w, 0, w->d_list + q0, qn, d_stage); },
        [&](uint32_t q0, uint32_t qn, const uint8_t* pinned) {
            for (uint32_t j = 0; j < qn;) {
                uint32_t e = j + 1;
                while (e < qn && slot[q0 + e] == slot[q0 + e - 1] + 1) e++;
                stage_copy(dst + (size_t)slot[q0 + j] * ps, pinned + (size_t)j * ps, (size_t)(e - j) * ps);
                j = e;
            }
        });
}

extern "C" int vs_pages_out_read_blocks(vs_pages_out* w, const uint32_t* blocks, uint32_t n, void* pages) {
    return vs_guard("vs_pages_out_read_blocks", [&] { return pages_out_read_blocks_impl(w, blocks, n, pages); });
}

static int pages_out_read_blocks_dev_impl(vs_pages_out* w, const uint32_t* blocks, uint32_t n, void* d_pages) {
    std::vector<uint32_t> list;
    std::vector<const uint8_t*> host;
    VS_TRY(pages_out_classify(w, "vs_pages_out_read_blocks_dev", blocks, n, d_pages, list, host));
    if (n == 0) return VS_OK;
    vs_ctx* c = w->ctx;
    const size_t ps = w->plan.page_size;
    uint8_t* dst = static_cast<uint8_t*>(d_pages);
    VS_REQUIRE(((uintptr_t)dst & 15) == 0, "vs_pages_out_read_blocks_dev: the device buffer must be 16-byte aligned");
    VS_HIP(hipSetDevice(c->device));
    // one launch over the whole list: workgroup i composes slot i in place, the slots of host-encoded pages are skipped by it
    VS_TRY(pages_out_list_reserve(w, n));
    VS_TRY(vs_dev_upload(c, w->d_list, list.data(), (size_t)n * 4));
    VS_TRY(launch_pages_encode(w, 0, w->d_list, n, dst));
    for (uint32_t i = 0; i < n; ++i)
        if (host[i]) VS_TRY(vs_dev_upload(c, dst + (size_t)i * ps, host[i], ps));
    VS_HIP(hipStreamSynchronize(c->stream));
    return pages_out_check(w);
}

extern "C" int vs_pages_out_read_blocks_dev(vs_pages_out* w, const uint32_t* blocks, uint32_t n, void* d_pages) {
    return vs_guard("vs_pages_out_read_blocks_dev", [&] { return pages_out_read_blocks_dev_impl(w, blocks, n, d_pages); });
}
