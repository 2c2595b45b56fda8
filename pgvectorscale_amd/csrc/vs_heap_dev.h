// vs_heap_dev.h — the heap's vector column decoded ON the device (vs_heap_dev_*); part of vs_pages_dev.hip, which includes it.
//
// vs_heap.cpp reads the column on one host thread into a host array that is uploaded afterwards: 153.6 GB at 50M x 768, more than a
// host holds.  Here the host only copies: the blocks of the heap's main fork, then of its TOAST relation, go through the context's
// pinned ring into two staged chunks in HBM as they are (the copy of chunk i+1 runs under the kernel of chunk i) and are never
// retained.  k_heap_dev_heap — a wave per fed page — finds the wanted tids of its block in the sorted (tid, node) table by binary
// search, resolves each through its line pointer (LP_REDIRECT followed), deforms the tuple up to the vector attribute one tuple per
// lane (heap_locate_attr restates locate_attr of vs_heap.cpp: natts of the tuple, null bitmap, attalign padding told by the pad
// byte, 1-byte / 4-byte / external headers, cstring, fixed widths), copies every in-line vector to row `node` with the whole wave
// and appends every external one (varatt_external) to a table of references through one atomic counter.  Before the first TOAST
// block that table is sorted by value id (hipcub radix sort; a value id named twice is an error), so nothing depends on the order
// in which the heap kernel's waves appended.  k_heap_dev_toast — a wave per fed page, a chunk row per lane — looks every chunk_id
// up in it, checks the chunk as the host does and copies it to byte chunk_seq * TOAST_MAX_CHUNK_SIZE - 4 of its row with the whole
// wave; the chunks of a value write disjoint words and add their bytes to the value's counter.  k_heap_dev_finish classifies,
// counts and zeroes the rows of values whose chunks did not all arrive.
//
// Every offset and length read from a page is checked against the page / item / tuple it must lie in before it is used as an
// address: a malformed page ends in an error record (first error wins), never in an access outside the staged chunk.
// Differences from the host reader (include/vsgpu.h): block ranges may have gaps; compressed vectors are counted, not decoded.
#pragma once
#include <hipcub/hipcub.hpp>

enum : uint8_t { HS_PENDING = 0, HS_INLINE = 1, HS_WAIT_TOAST = 2, HS_NULL = 3, HS_DEAD_LP = 4, HS_NOT_FOUND = 5, HS_DELETED = 6,
                 HS_COMPRESSED = 7, HS_EXTERNAL = 8, HS_N = 9 };

enum { HE_OK = 0, HE_PAGE_SIZE, HE_PAGE_HEADER, HE_ITEM_BOUNDS, HE_TUPLE_SHORT, HE_HOFF, HE_DESC_SHORT, HE_ATTR_START, HE_EXT_TRUNC,
       HE_VARTAG, HE_1B_ZERO, HE_4B_TRUNC, HE_4B_SHORT, HE_CSTRING, HE_ATTLEN, HE_ATTR_PAST, HE_DATUM_SHORT, HE_DIM, HE_DATUM_SIZE,
       HE_RAWSIZE, HE_EXT_RAW, HE_EXTSIZE, HE_REF_TABLE, HE_CHUNK_NULL, HE_CHUNK_EXTERNAL, HE_CHUNK_COMPRESSED, HE_CHUNK_RANGE,
       HE_CHUNK_BYTES, HE_DUP_VALUE, HE_CHAIN_CYCLE, HE_LAST = HE_CHAIN_CYCLE };
static const char* const kHeapErrorText[] = {
    "", "pd_pagesize_version does not say the reader's pagesize", "inconsistent page header (pd_lower, pd_upper, pd_special)",
    "item lies outside pd_upper..pd_special", "tuple shorter than its header", "t_hoff does not fit the tuple and its attributes",
    "the tuple descriptor has fewer attributes than the vector's attribute number", "attribute starts past the end of the tuple",
    "truncated external varlena", "varlena tag on disk is not VARTAG_ONDISK", "1-byte varlena header of size 0",
    "truncated varlena header", "4-byte varlena of fewer than 4 bytes", "unterminated cstring attribute",
    "attribute length 0 / below -2 in the tuple descriptor", "attribute runs past the tuple's data bytes",
    "vector datum of fewer than 4 data bytes", "vector of other dimensions than the index has",
    "vector data bytes do not match the dimensions", "va_rawsize below the varlena header",
    "external vector's raw size does not match the dimensions", "external size above raw size",
    "more external vectors than wanted tuples", "NULL in a chunk row", "external chunk data", "compressed chunk data",
    "chunk does not fit its value (negative chunk_seq, short non-final chunk or bytes past the value's size)",
    "more chunk bytes than the value's size", "TOAST value is referenced by two heap tuples",
    "HOT chain visits more members than the page has line pointers (a cycle)"};
static_assert(sizeof(kHeapErrorText) / sizeof(kHeapErrorText[0]) == HE_LAST + 1, "one text per HE_* code");

// counters / records of a reader in device memory (u32 words)
enum { HC_ERR = 0 /* code, block, offset, detail, relation (0 heap, 1 TOAST) */, HC_NREFS = 5, HC_CHUNKS = 6 /* u64 */,
       HC_STATE = 8 /* HS_N counts, filled by k_heap_dev_finish */, HC_N = 20 };

struct HeapAttrDev {
    int32_t attlen;
    uint32_t align;
};

__device__ __forceinline__ uint32_t ldu16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ __forceinline__ uint32_t ldu32(const uint8_t* p) {  // (tuple data is not aligned: a short varlena header shifts everything behind it)
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__device__ __forceinline__ void heap_error(uint32_t* ctr, uint32_t code, uint32_t rel, uint32_t blk, uint32_t off, uint32_t detail) {
    if (atomicCAS(&ctr[HC_ERR], 0u, code) == 0u) {
        ctr[HC_ERR + 1] = blk;
        ctr[HC_ERR + 2] = off;
        ctr[HC_ERR + 3] = detail;
        ctr[HC_ERR + 4] = rel;
    }
}

// PageHeaderData as view() of vs_heap.cpp reads it: an all-zero (new) page holds nothing; otherwise pd_pagesize_version must name the
// reader's page size and pd_lower <= pd_upper <= pd_special <= page_size.  nitems line pointers then lie in [24, pd_lower).
struct HeapPage {
    uint32_t upper, special, nitems;
};
__device__ __forceinline__ uint32_t heap_page_view(const uint8_t* page, uint32_t page_size, HeapPage& v, uint32_t& detail) {
    const uint32_t lower = ld16(page + 12);
    v.upper = ld16(page + 14);
    v.special = ld16(page + 16);
    v.nitems = 0;
    if (v.upper == 0) return HE_OK;  // PageIsNew
    detail = ld16(page + 18);
    if ((detail & 0xFF00u) != page_size) return HE_PAGE_SIZE;
    detail = lower;
    if (!(lower >= 24 && lower <= v.upper && v.upper <= v.special && v.special <= page_size)) return HE_PAGE_HEADER;
    v.nitems = (lower - 24) / 4;
    return HE_OK;
}

// an LP_NORMAL line pointer names bytes that can hold a tuple: inside pd_upper..pd_special and no shorter than the 23-byte header
__device__ __forceinline__ bool heap_item_in_bounds(const HeapPage& pg, uint32_t lp_off, uint32_t lp_len) {
    return lp_off >= pg.upper && lp_off + lp_len <= pg.special && lp_len >= 23;
}

// heap_deform_tuple up to attribute `want` (0-based) of the tuple of `len` bytes at byte t0 of the page (t0 + len <= pd_special was
// checked): locate_attr of vs_heap.cpp, statement by statement.  at: byte offset of the attribute inside the PAGE.
struct HeapSpan {
    uint32_t at, size;
    bool is_null;
};
__device__ __forceinline__ uint32_t heap_locate_attr(const uint8_t* page, uint32_t t0, uint32_t len, const HeapAttrDev* __restrict__ attrs,
                                                     uint32_t natts_desc, uint32_t want, HeapSpan& out, uint32_t& detail) {
    out.at = 0;
    out.size = 0;
    out.is_null = false;
    detail = len;
    if (len < 23) return HE_TUPLE_SHORT;
    const uint8_t* t = page + t0;
    const uint32_t natts = ldu16(t + 18) & 0x07FFu;  // HeapTupleHeaderGetNatts
    const uint32_t infomask = ldu16(t + 20);
    const uint32_t hoff = t[22];
    const bool hasnull = (infomask & 0x0001u) != 0;
    detail = hoff;
    if (hoff < 23 + (hasnull ? (natts + 7) / 8 : 0) || hoff > len || (hoff & 7)) return HE_HOFF;
    if (want >= natts) {  // a column added after the row was written
        out.is_null = true;
        return HE_OK;
    }
    uint32_t off = 0;  // relative to t + hoff
    const uint8_t* tp = t + hoff;
    const uint32_t dl = len - hoff;
    for (uint32_t a = 0; a <= want; ++a) {
        detail = a + 1;
        if (a >= natts_desc) return HE_DESC_SHORT;
        if (hasnull && !((t[23 + (a >> 3)] >> (a & 7)) & 1)) {  // att_isnull (23 + a / 8 < hoff <= len)
            if (a == want) {
                out.is_null = true;
                return HE_OK;
            }
            continue;
        }
        const int32_t attlen = attrs[a].attlen;
        const uint32_t al = attrs[a].align;  // 1, 2, 4 or 8
        uint32_t size;
        if (attlen == -1) {
            if (off >= dl) return HE_ATTR_START;
            if (tp[off] == 0) off = (off + al - 1) & ~(al - 1);  // att_align_pointer: a pad byte, so a 4-byte header follows at attalign
            if (off >= dl) return HE_ATTR_START;
            const uint32_t b0 = tp[off];
            if (b0 == 0x01u) {  // VARATT_IS_1B_E
                if (off + 2 > dl) return HE_EXT_TRUNC;
                detail = tp[off + 1];
                if (detail != 18u) return HE_VARTAG;  // VARTAG_ONDISK
                size = 2 + 16;
            } else if (b0 & 0x01u) {
                size = (b0 >> 1) & 0x7Fu;  // VARSIZE_1B (includes the header byte)
                if (size == 0) return HE_1B_ZERO;
            } else {
                if (off + 4 > dl) return HE_4B_TRUNC;
                size = (ldu32(tp + off) >> 2) & 0x3FFFFFFFu;  // VARSIZE_4B
                if (size < 4) return HE_4B_SHORT;
            }
        } else if (attlen == -2) {  // cstring
            off = (off + al - 1) & ~(al - 1);
            uint32_t e = off;
            while (e < dl && tp[e]) ++e;
            if (e >= dl) return HE_CSTRING;
            size = e - off + 1;
        } else if (attlen > 0) {
            off = (off + al - 1) & ~(al - 1);
            size = (uint32_t)attlen;
        } else {
            return HE_ATTLEN;
        }
        detail = a + 1;
        if ((uint64_t)off + size > dl) return HE_ATTR_PAST;
        if (a == want) {
            out.at = t0 + hoff + off;
            out.size = size;
            return HE_OK;
        }
        off += size;
    }
    return HE_OK;
}

// nbytes (a multiple of 4) from src to the 4-byte aligned dst with the whole wave: 16-byte accesses where both sides allow it
// (after the words that bring dst to a 16-byte boundary), 4-byte words where the source is word aligned, bytes otherwise (the
// body behind a 1-byte varlena header)
__device__ __forceinline__ void heap_wave_copy(uint8_t* dst, const uint8_t* src, uint32_t nbytes, uint32_t lane) {
    const uint32_t nw = nbytes >> 2;
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    if ((uintptr_t)src & 3u) {
        for (uint32_t w = lane; w < nw; w += WAVE) d[w] = ldu32(src + 4 * w);
        return;
    }
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    const uint32_t head = min(nw, (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u) >> 2);
    if (((uintptr_t)(s + head) & 15u) != 0) {
        for (uint32_t w = lane; w < nw; w += WAVE) d[w] = s[w];
        return;
    }
    if (lane < head) d[lane] = s[lane];
    const uint32_t nv = (nw - head) >> 2;
    const uint4* s4 = reinterpret_cast<const uint4*>(s + head);
    uint4* d4 = reinterpret_cast<uint4*>(d + head);
    for (uint32_t v = lane; v < nv; v += WAVE) d4[v] = s4[v];
    for (uint32_t w = head + 4 * nv + lane; w < nw; w += WAVE) d[w] = s[w];
}

__device__ __forceinline__ uint32_t heap_lower_bound64(const uint64_t* __restrict__ keys, uint32_t n, uint64_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct HeapDevArgs {
    const uint8_t* pages;  // [n_blocks][page_size], the staged chunk
    uint32_t page_size, first_block, n_blocks;
    const uint64_t* keys;   // [n] heap tids ascending (deleted tids parked at the end as ~0)
    const uint32_t* nodes;  // [n] the node of keys[i]
    uint32_t n;
    const HeapAttrDev* attrs;  // [natts] the table's, then the TOAST relation's three
    uint32_t natts, vec_att, dim, stride, chunk;
    float* out;
    uint8_t* state;  // [n] by node
    // heap pass: the references are appended here; TOAST pass: ref_vid / ref_idx are the table sorted by value id
    uint32_t *ref_vid, *ref_node, *ref_ext, *ref_blk;
    const uint32_t* ref_idx;
    uint32_t* got;  // [n_refs] chunk bytes received, by sorted position
    uint32_t ref_cap, n_refs;
    uint32_t* ctr;
};

// what one lane found behind its tid
struct HeapHit {
    uint32_t st;   // HS_*, or HS_N: an error was recorded, the state stays as it is
    uint32_t src;  // byte offset of the floats of an in-line vector inside the page (st == HS_INLINE)
};
__device__ __forceinline__ HeapHit heap_resolve(const HeapDevArgs& a, const uint8_t* page, const HeapPage& pg, uint32_t blk, uint32_t off,
                                                uint32_t node) {
    HeapHit hit{HS_NOT_FOUND, 0};
    for (int hop = 0; hop < 8; ++hop) {
        if (off < 1 || off > pg.nitems) break;
        const uint32_t lp = ld32(page + 24 + 4 * (off - 1));
        const uint32_t lp_off = lp & 0x7FFFu, fl = (lp >> 15) & 3u, lp_len = lp >> 17;
        if (fl == 2u) {  // LP_REDIRECT: the root of a pruned HOT chain
            off = lp_off;
            continue;
        }
        if (fl != 1u) {
            hit.st = HS_DEAD_LP;
            break;
        }
        hit.st = HS_N;
        if (!heap_item_in_bounds(pg, lp_off, lp_len)) {
            heap_error(a.ctr, HE_ITEM_BOUNDS, 0, blk, off, lp);
            break;
        }
        HeapSpan sp;
        uint32_t detail = 0;
        const uint32_t he = heap_locate_attr(page, lp_off, lp_len, a.attrs, a.natts, a.vec_att, sp, detail);
        if (he != HE_OK) {
            heap_error(a.ctr, he, 0, blk, off, detail);
            break;
        }
        if (sp.is_null) {
            hit.st = HS_NULL;
            break;
        }
        const uint8_t* v = page + sp.at;
        const uint32_t b0 = v[0];
        uint32_t body, blen;
        if (b0 == 0x01u) {  // varatt_external (18 bytes, inside the tuple): va_rawsize, va_extinfo, va_valueid, va_toastrelid
            const int32_t va_rawsize = (int32_t)ldu32(v + 2);
            const uint32_t va_extinfo = ldu32(v + 6);
            const uint32_t extsize = va_extinfo & 0x3FFFFFFFu;
            if (va_rawsize < 4) {
                heap_error(a.ctr, HE_RAWSIZE, 0, blk, off, (uint32_t)va_rawsize);
                break;
            }
            const uint32_t rawsize = (uint32_t)va_rawsize - 4;
            if (rawsize != 4 + 4 * a.dim) {
                heap_error(a.ctr, HE_EXT_RAW, 0, blk, off, rawsize);
                break;
            }
            if (extsize > rawsize) {
                heap_error(a.ctr, HE_EXTSIZE, 0, blk, off, extsize);
                break;
            }
            if (extsize < rawsize) {  // compressed (pglz or lz4): left to the host reader
                hit.st = HS_COMPRESSED;
                break;
            }
            const uint32_t slot = atomicAdd(&a.ctr[HC_NREFS], 1u);
            if (slot >= a.ref_cap) {  // (one reference per wanted tid at the most: this does not happen)
                heap_error(a.ctr, HE_REF_TABLE, 0, blk, off, slot);
                break;
            }
            a.ref_vid[slot] = ldu32(v + 10);
            a.ref_node[slot] = node;
            a.ref_ext[slot] = extsize;
            a.ref_blk[slot] = blk;
            hit.st = HS_WAIT_TOAST;
            break;
        }
        if (b0 & 0x01u) {  // short header: the body is not aligned
            body = sp.at + 1;
            blen = sp.size - 1;
        } else {
            if ((ldu32(v) & 0x03u) == 0x02u) {  // VARATT_IS_4B_C: compressed in line
                hit.st = HS_COMPRESSED;
                break;
            }
            body = sp.at + 4;
            blen = sp.size - 4;
        }
        if (blen < 4) {
            heap_error(a.ctr, HE_DATUM_SHORT, 0, blk, off, blen);
            break;
        }
        const int32_t dim = (int32_t)(int16_t)ldu16(page + body);
        if ((uint32_t)dim != a.dim) {
            heap_error(a.ctr, HE_DIM, 0, blk, off, (uint32_t)dim);
            break;
        }
        if (blen != 4 + 4 * a.dim) {
            heap_error(a.ctr, HE_DATUM_SIZE, 0, blk, off, blen);
            break;
        }
        hit.st = HS_INLINE;
        hit.src = body + 4;  // (body + 4 + 4 * dim <= the end of the attribute <= the end of the tuple)
        break;
    }
    return hit;
}

// one wave per fed heap page; a wanted tuple per lane, then every in-line vector with the whole wave
__global__ __launch_bounds__(WAVE) void k_heap_dev_heap(HeapDevArgs a) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < a.n_blocks; b += gridDim.x) {
        const uint32_t blk = a.first_block + b;
        const uint32_t lo = heap_lower_bound64(a.keys, a.n, (uint64_t)blk << 16);
        const uint32_t hi = heap_lower_bound64(a.keys, a.n, ((uint64_t)blk + 1) << 16);
        if (lo == hi) continue;
        const uint8_t* page = a.pages + (size_t)b * a.page_size;
        HeapPage pg;
        uint32_t detail = 0;
        const uint32_t pe = heap_page_view(page, a.page_size, pg, detail);
        if (pe != HE_OK) {
            if (lane == 0) heap_error(a.ctr, pe, 0, blk, 0, detail);
            continue;
        }
        for (uint32_t e0 = lo; e0 < hi; e0 += WAVE) {  // (a page of narrow rows holds more wanted tuples than the wave has lanes)
            const uint32_t e = e0 + lane;
            HeapHit hit{HS_N, 0};
            uint32_t node = 0;
            if (e < hi) {
                node = a.nodes[e];
                hit = heap_resolve(a, page, pg, blk, (uint32_t)(a.keys[e] & 0xFFFFu), node);
                if (hit.st != HS_N) a.state[node] = (uint8_t)hit.st;
            }
            uint64_t m = __ballot(hit.st == HS_INLINE);
            while (m) {
                const int l = __builtin_ctzll(m);
                m &= m - 1;
                const uint32_t src = __shfl(hit.src, l);
                const uint32_t nd = __shfl(node, l);
                heap_wave_copy(reinterpret_cast<uint8_t*>(a.out + (size_t)nd * a.stride), page + src, 4 * a.dim, lane);
            }
        }
    }
}

// one wave per fed TOAST page; a chunk row (chunk_id oid, chunk_seq int4, chunk_data bytea) per lane, then every chunk with the whole wave
__global__ __launch_bounds__(WAVE) void k_heap_dev_toast(HeapDevArgs a) {
    const uint32_t lane = threadIdx.x;
    const HeapAttrDev* tattrs = a.attrs + a.natts;
    for (uint32_t b = blockIdx.x; b < a.n_blocks; b += gridDim.x) {
        const uint32_t blk = a.first_block + b;
        const uint8_t* page = a.pages + (size_t)b * a.page_size;
        HeapPage pg;
        uint32_t detail = 0;
        const uint32_t pe = heap_page_view(page, a.page_size, pg, detail);
        if (pe != HE_OK) {
            if (lane == 0) heap_error(a.ctr, pe, 1, blk, 0, detail);
            continue;
        }
        for (uint32_t o0 = 1; o0 <= pg.nitems; o0 += WAVE) {
            const uint32_t off = o0 + lane;
            bool taken = false;
            uint32_t src = 0, nbytes = 0, node = 0, dst = 0;
            do {
                if (off > pg.nitems) break;
                const uint32_t lp = ld32(page + 24 + 4 * (off - 1));
                const uint32_t lp_off = lp & 0x7FFFu, fl = (lp >> 15) & 3u, lp_len = lp >> 17;
                if (fl != 1u) break;
                if (!heap_item_in_bounds(pg, lp_off, lp_len)) {
                    heap_error(a.ctr, HE_ITEM_BOUNDS, 1, blk, off, lp);
                    break;
                }
                HeapSpan id, seq, data;
                uint32_t he = heap_locate_attr(page, lp_off, lp_len, tattrs, 3, 0, id, detail);
                if (he == HE_OK) he = heap_locate_attr(page, lp_off, lp_len, tattrs, 3, 1, seq, detail);
                if (he == HE_OK) he = heap_locate_attr(page, lp_off, lp_len, tattrs, 3, 2, data, detail);
                if (he == HE_OK && (id.is_null || seq.is_null || data.is_null)) he = HE_CHUNK_NULL;
                if (he != HE_OK) {
                    heap_error(a.ctr, he, 1, blk, off, detail);
                    break;
                }
                const uint32_t vid = ldu32(page + id.at);
                uint32_t lo = 0, hi = a.n_refs;
                while (lo < hi) {
                    const uint32_t mid = lo + ((hi - lo) >> 1);
                    if (a.ref_vid[mid] < vid) lo = mid + 1;
                    else hi = mid;
                }
                if (lo >= a.n_refs || a.ref_vid[lo] != vid) break;  // a value of another column / row
                taken = true;
                const uint32_t ri = a.ref_idx[lo];
                const uint32_t ext = a.ref_ext[ri];
                const int32_t s = (int32_t)ldu32(page + seq.at);
                const uint32_t d0 = page[data.at];
                uint32_t body, blen;
                if (d0 == 0x01u) {
                    heap_error(a.ctr, HE_CHUNK_EXTERNAL, 1, blk, off, vid);
                    break;
                }
                if (d0 & 1u) {
                    body = data.at + 1;
                    blen = data.size - 1;
                } else {
                    if ((ldu32(page + data.at) & 3u) != 0) {
                        heap_error(a.ctr, HE_CHUNK_COMPRESSED, 1, blk, off, vid);
                        break;
                    }
                    body = data.at + 4;
                    blen = data.size - 4;
                }
                const uint64_t at = (uint64_t)(s < 0 ? 0 : s) * a.chunk;
                if (s < 0 || at + blen > ext || (blen != a.chunk && at + blen != ext)) {
                    heap_error(a.ctr, HE_CHUNK_RANGE, 1, blk, off, (uint32_t)s);
                    break;
                }
                // value bytes: [0,2) dim, [2,4) unused, [4, ..) the floats
                if (at == 0 && blen >= 2 && (uint32_t)(int32_t)(int16_t)ldu16(page + body) != a.dim) {
                    heap_error(a.ctr, HE_DIM, 1, blk, off, ldu16(page + body));
                    break;
                }
                const uint32_t before = atomicAdd(&a.got[lo], blen);
                if ((uint64_t)before + blen > ext) {
                    heap_error(a.ctr, HE_CHUNK_BYTES, 1, blk, off, vid);
                    break;
                }
                node = a.ref_node[ri];
                if (before + blen == ext) a.state[node] = HS_EXTERNAL;
                // (ext = 4 + 4 * dim and the chunk size are multiples of 4, so is every checked chunk; at + blen <= ext keeps it in the row)
                const uint32_t skip = at == 0 ? min(4u, blen) : 0u;
                src = body + skip;
                nbytes = blen - skip;
                dst = (uint32_t)at + skip - 4;
            } while (false);
            const uint64_t mt = __ballot(taken);
            if (lane == 0 && mt) atomicAdd(reinterpret_cast<unsigned long long*>(a.ctr + HC_CHUNKS), (unsigned long long)__popcll(mt));
            uint64_t m = __ballot(nbytes != 0);
            while (m) {
                const int l = __builtin_ctzll(m);
                m &= m - 1;
                const uint32_t s_ = __shfl(src, l), n_ = __shfl(nbytes, l), nd = __shfl(node, l), d_ = __shfl(dst, l);
                heap_wave_copy(reinterpret_cast<uint8_t*>(a.out + (size_t)nd * a.stride) + d_, page + s_, n_, lane);
            }
        }
    }
}

// open: the (tid, node) pairs as the radix sort takes them; a deleted index tuple (offset 0) is parked behind every block
__global__ __launch_bounds__(256) void k_heap_dev_prep(const uint64_t* __restrict__ tids, uint32_t n, uint64_t* __restrict__ keys,
                                                       uint32_t* __restrict__ nodes, uint8_t* __restrict__ state) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint64_t t = tids[i];
        const bool deleted = (t & 0xFFFFull) == 0;
        keys[i] = deleted ? ~0ull : t;
        nodes[i] = i;
        state[i] = deleted ? HS_DELETED : HS_PENDING;
    }
}
__global__ __launch_bounds__(256) void k_heap_dev_iota(uint32_t* __restrict__ v, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) v[i] = i;
}
// the first `dim` floats of rows [0, n); the padding floats of a row are the caller's
__global__ __launch_bounds__(256) void k_heap_dev_zero_rows(float* __restrict__ out, uint32_t stride, uint32_t dim, uint32_t n) {
    const uint64_t total = (uint64_t)n * dim;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x)
        out[(i / dim) * stride + (i % dim)] = 0.f;
}
// the sorted table names no value id twice
__global__ __launch_bounds__(256) void k_heap_dev_dups(const uint32_t* __restrict__ vid, const uint32_t* __restrict__ idx,
                                                       const uint32_t* __restrict__ ref_blk, uint32_t n_refs, uint32_t* __restrict__ ctr) {
    for (uint32_t i = 1 + blockIdx.x * blockDim.x + threadIdx.x; i < n_refs; i += gridDim.x * blockDim.x)
        if (vid[i] == vid[i - 1]) heap_error(ctr, HE_DUP_VALUE, 0, ref_blk[idx[i]], 0, vid[i]);
}
// a wave per 64 nodes: the states counted (one atomic per wave and state), found[] written, and the row of every value whose
// chunks did not all arrive zeroed again (the only rows that were written without being complete)
__global__ __launch_bounds__(WAVE) void k_heap_dev_finish(const uint8_t* __restrict__ state, uint32_t n, float* __restrict__ out,
                                                          uint32_t stride, uint32_t dim, uint8_t* __restrict__ found,
                                                          uint32_t* __restrict__ ctr) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t base = blockIdx.x * WAVE; base < n; base += gridDim.x * WAVE) {
        const uint32_t i = base + lane;
        const uint32_t st = i < n ? state[i] : (uint32_t)HS_N;
        if (i < n && found) found[i] = (st == HS_INLINE || st == HS_EXTERNAL) ? 1 : 0;
        for (uint32_t k = 0; k < HS_N; ++k) {
            const uint64_t m = __ballot(st == k);
            if (lane == 0 && m) atomicAdd(&ctr[HC_STATE + k], (uint32_t)__popcll(m));
        }
        uint64_t m = __ballot(st == HS_WAIT_TOAST);
        while (m) {
            const int l = __builtin_ctzll(m);
            m &= m - 1;
            float* row = out + (size_t)(base + (uint32_t)l) * stride;
            for (uint32_t c = lane; c < dim; c += WAVE) row[c] = 0.f;
        }
    }
}
// rows [0, rows) of a strided device array into rows of the vector column, padding floats zero (vs_pages_follow_apply_dev: what
// vs_upload_rows leaves behind for host rows)
__global__ __launch_bounds__(256) void k_rows_copy_pad(float* __restrict__ dst, uint32_t dst_stride, const float* __restrict__ src,
                                                       uint32_t src_stride, uint32_t dim, uint32_t rows) {
    const uint64_t total = (uint64_t)rows * dst_stride;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / dst_stride;
        const uint32_t c = (uint32_t)(i % dst_stride);
        dst[i] = c < dim ? src[r * src_stride + c] : 0.f;
    }
}

struct vs_heap_dev {
    vs_ctx* ctx = nullptr;
    uint32_t page_size = VS_BLCKSZ, natts = 0, vec_att = 0, dim = 0, n = 0, stride = 0, chunk = 0;
    float* d_out = nullptr;
    HeapAttrDev* d_attrs = nullptr;
    uint64_t* d_keys = nullptr;
    uint32_t* d_nodes = nullptr;
    uint8_t* d_state = nullptr;
    uint32_t *d_ref_vid = nullptr, *d_ref_node = nullptr, *d_ref_ext = nullptr, *d_ref_blk = nullptr;  // [n] in the order the waves appended
    uint32_t *d_sref_vid = nullptr, *d_sref_idx = nullptr, *d_got = nullptr;                           // [n_refs] by value id
    uint32_t* d_ctr = nullptr;
    uint32_t* h_ctr = nullptr;  // pinned: the error record as it stood after the last kernel that has finished
    uint8_t* d_stage[2] = {nullptr, nullptr};  // two staged chunks of pages
    hipEvent_t stage_ev[2] = {nullptr, nullptr};  // the kernel that read d_stage[i] has finished
    size_t stage_bytes = 0;
    int slot = 0;
    uint32_t n_refs = 0;
    bool toast_begun = false, failed = false, finished = false;
    uint32_t next_block[2] = {0, 0};
};

static void heap_dev_free(vs_heap_dev* h) {
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->copy_stream);
    (void)hipStreamSynchronize(h->ctx->stream);
    void* ptrs[] = {h->d_attrs, h->d_keys, h->d_nodes, h->d_state, h->d_ref_vid, h->d_ref_node, h->d_ref_ext, h->d_ref_blk, h->d_sref_vid,
                    h->d_sref_idx, h->d_got, h->d_ctr, h->d_stage[0], h->d_stage[1]};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (h->h_ctr) (void)hipHostFree(h->h_ctr);
    for (hipEvent_t e : h->stage_ev)
        if (e) (void)hipEventDestroy(e);
    delete h;
}

// the error record the kernels left, as VS_ERR_INVALID with the relation, the block, the offset and the reason
static int heap_dev_report(vs_heap_dev* h) {
    const uint32_t* e = h->h_ctr + HC_ERR;
    if (e[0] == HE_OK) return VS_OK;
    h->failed = true;
    (void)hipStreamSynchronize(h->ctx->stream);  // (the copy that brought the code has brought the other words)
    const uint32_t code = e[0] <= HE_LAST ? e[0] : 0;
    if (code == HE_DUP_VALUE) vs_set_error("TOAST value %u is referenced by two heap tuples (one of them on heap block %u)", e[3], e[1]);
    else if (code == HE_DIM) vs_set_error("%s block %u item %u: vector of %d dimensions, the index has %u", e[4] ? "TOAST" : "heap", e[1], e[2], (int)(int16_t)e[3], h->dim);
    else vs_set_error("%s block %u item %u: %s (detail %u)", e[4] ? "TOAST" : "heap", e[1], e[2], kHeapErrorText[code], e[3]);
    return VS_ERR_INVALID;
}

static uint32_t heap_dev_grid(uint64_t items, uint32_t per_block) {
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + per_block - 1) / per_block, 1), 4096);
}

static int heap_dev_open_impl(vs_heap_dev* h, const vs_heap_attr* attrs, const uint64_t* heap_tids) {
    vs_ctx* c = h->ctx;
    hipStream_t st = c->stream;
    const uint32_t n = h->n;
    VS_HIP(hipSetDevice(c->device));
    std::vector<HeapAttrDev> ha(h->natts + 3);
    for (uint32_t i = 0; i < h->natts; ++i) {
        const char al = attrs[i].attalign;
        ha[i] = HeapAttrDev{attrs[i].attlen, al == 'd' ? 8u : (al == 'i' ? 4u : (al == 's' ? 2u : 1u))};
    }
    ha[h->natts] = HeapAttrDev{4, 4};       // chunk_id oid
    ha[h->natts + 1] = HeapAttrDev{4, 4};   // chunk_seq int4
    ha[h->natts + 2] = HeapAttrDev{-1, 4};  // chunk_data bytea
    VS_HIP(hipMalloc(&h->d_attrs, ha.size() * sizeof(HeapAttrDev)));
    VS_HIP(hipMemcpy(h->d_attrs, ha.data(), ha.size() * sizeof(HeapAttrDev), hipMemcpyHostToDevice));
    VS_HIP(hipMalloc(&h->d_ctr, HC_N * 4));
    VS_HIP(hipMemsetAsync(h->d_ctr, 0, HC_N * 4, st));
    VS_HIP(hipHostMalloc(&h->h_ctr, HC_N * 4, hipHostMallocDefault));
    memset(h->h_ctr, 0, HC_N * 4);
    for (hipEvent_t& e : h->stage_ev) VS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    h->stage_bytes = std::max<size_t>(c->pinned_bytes / h->page_size, 1) * h->page_size;
    for (uint8_t*& p : h->d_stage) VS_HIP(hipMalloc(&p, h->stage_bytes));
    const size_t rows = std::max<uint32_t>(n, 1);
    VS_HIP(hipMalloc(&h->d_keys, rows * 8));
    VS_HIP(hipMalloc(&h->d_nodes, rows * 4));
    VS_HIP(hipMalloc(&h->d_state, rows));
    if (n == 0) return VS_OK;
    // the pairs sorted by tid, as vs_index_bulk_delete sorts its dead set
    uint64_t *d_tids = nullptr, *d_k = nullptr;
    uint32_t* d_v = nullptr;
    void* d_tmp = nullptr;
    auto run = [&]() -> int {
        VS_HIP(hipMalloc(&d_tids, rows * 8));
        VS_HIP(hipMalloc(&d_k, rows * 8));
        VS_HIP(hipMalloc(&d_v, rows * 4));
        VS_TRY(vs_dev_upload(c, d_tids, heap_tids, (size_t)n * 8));
        hipLaunchKernelGGL(k_heap_dev_prep, dim3(heap_dev_grid(n, 256)), dim3(256), 0, st, (const uint64_t*)d_tids, n, d_k, d_v, h->d_state);
        VS_HIP(hipGetLastError());
        size_t tmp_bytes = 0;
        VS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (const uint64_t*)d_k, h->d_keys, (const uint32_t*)d_v, h->d_nodes, (int)n, 0,
                                                  64, st));
        VS_HIP(hipMalloc(&d_tmp, tmp_bytes + 16));
        VS_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp_bytes, (const uint64_t*)d_k, h->d_keys, (const uint32_t*)d_v, h->d_nodes, (int)n, 0,
                                                  64, st));
        hipLaunchKernelGGL(k_heap_dev_zero_rows, dim3(heap_dev_grid((uint64_t)n * h->dim, 256)), dim3(256), 0, st, h->d_out, h->stride, h->dim, n);
        VS_HIP(hipGetLastError());
        VS_HIP(hipStreamSynchronize(st));
        return VS_OK;
    };
    const int r = run();
    if (r != VS_OK) (void)hipStreamSynchronize(st);
    if (d_tids) (void)hipFree(d_tids);
    if (d_k) (void)hipFree(d_k);
    if (d_v) (void)hipFree(d_v);
    if (d_tmp) (void)hipFree(d_tmp);
    VS_TRY(r);
    // (one reference per wanted tid at the most)
    VS_HIP(hipMalloc(&h->d_ref_vid, rows * 4));
    VS_HIP(hipMalloc(&h->d_ref_node, rows * 4));
    VS_HIP(hipMalloc(&h->d_ref_ext, rows * 4));
    VS_HIP(hipMalloc(&h->d_ref_blk, rows * 4));
    return VS_OK;
}

extern "C" int vs_heap_dev_open(vs_ctx* ctx, uint32_t page_size, const vs_heap_attr* attrs, uint32_t natts, uint32_t vector_attno, uint32_t dim,
                                const uint64_t* heap_tids, uint32_t n, float* d_out_vecs, uint32_t out_stride, vs_heap_dev** out) {
    VS_REQUIRE(ctx && attrs && out && natts != 0 && vector_attno >= 1 && vector_attno <= natts && dim != 0 && dim <= 16000 &&
                   (!n || (heap_tids && d_out_vecs)) && out_stride >= dim,
               "vs_heap_dev_open: bad arguments");
    VS_REQUIRE(page_size >= 512 && page_size <= 32768 && !(page_size & (page_size - 1)), "vs_heap_dev_open: page size %u", page_size);
    VS_REQUIRE(attrs[vector_attno - 1].attlen == -1, "vs_heap_dev_open: attribute %u is not a varlena (pgvector's vector is)", vector_attno);
    VS_REQUIRE(n <= 0x7FFFFFFFu, "vs_heap_dev_open: %u nodes", n);
    *out = nullptr;
    VS_REQUIRE(ctx->pinned_bytes >= page_size, "vs_heap_dev_open: the context's staging buffers (%zu bytes) do not hold one page", ctx->pinned_bytes);
    return vs_guard("vs_heap_dev_open", [&]() -> int {
        vs_heap_dev* h = new vs_heap_dev();
        h->ctx = ctx;
        h->page_size = page_size;
        h->natts = natts;
        h->vec_att = vector_attno - 1;
        h->dim = dim;
        h->n = n;
        h->stride = out_stride;
        h->d_out = d_out_vecs;
        // EXTERN_TUPLE_MAX_SIZE - MAXALIGN(SizeofHeapTupleHeader) - sizeof(Oid) - sizeof(int32) - VARHDRSZ (access/heaptoast.h)
        const uint32_t per_tuple = ((page_size - ((24 + 4 * 4 + 7) & ~7u)) / 4) & ~7u;
        h->chunk = per_tuple - 24 - 4 - 4 - 4;
        const int r = heap_dev_open_impl(h, attrs, heap_tids);
        if (r != VS_OK) {
            heap_dev_free(h);
            return r;
        }
        *out = h;
        return VS_OK;
    });
}

static HeapDevArgs heap_dev_args(const vs_heap_dev* h) {
    HeapDevArgs a{};
    a.page_size = h->page_size;
    a.keys = h->d_keys;
    a.nodes = h->d_nodes;
    a.n = h->n;
    a.attrs = h->d_attrs;
    a.natts = h->natts;
    a.vec_att = h->vec_att;
    a.dim = h->dim;
    a.stride = h->stride;
    a.chunk = h->chunk;
    a.out = h->d_out;
    a.state = h->d_state;
    a.ref_node = h->d_ref_node;
    a.ref_ext = h->d_ref_ext;
    a.ref_blk = h->d_ref_blk;
    a.ref_cap = h->n;
    a.ctr = h->d_ctr;
    if (h->toast_begun) {
        a.ref_vid = h->d_sref_vid;
        a.ref_idx = h->d_sref_idx;
        a.got = h->d_got;
        a.n_refs = h->n_refs;
    } else {
        a.ref_vid = h->d_ref_vid;
    }
    return a;
}

// the blocks through the pinned ring into the two staged chunks: the copy of chunk i + 1 runs under the kernel of chunk i, also
// across calls (nothing here waits for a kernel; an error record is picked up by a later call, or by the finish)
static int heap_dev_feed(vs_heap_dev* h, bool toast, uint32_t first_block, const void* pages, uint32_t n_blocks) {
    vs_ctx* c = h->ctx;
    VS_HIP(hipSetDevice(c->device));
    VS_TRY(heap_dev_report(h));
    const uint32_t per = (uint32_t)(h->stage_bytes / h->page_size);
    const uint8_t* src = static_cast<const uint8_t*>(pages);
    for (uint32_t b0 = 0; b0 < n_blocks && (h->n || toast); b0 += per) {
        const uint32_t nb = std::min(per, n_blocks - b0);
        const size_t bytes = (size_t)nb * h->page_size;
        const int s = h->slot;
        VS_HIP(hipEventSynchronize(c->pinned_ev[s]));  // the pinned buffer's last copy has left it
        stage_copy(c->pinned[s], src + (size_t)b0 * h->page_size, bytes);
        VS_HIP(hipStreamWaitEvent(c->copy_stream, h->stage_ev[s], 0));  // the kernel that read this staged chunk has finished
        VS_HIP(hipMemcpyAsync(h->d_stage[s], c->pinned[s], bytes, hipMemcpyHostToDevice, c->copy_stream));
        VS_HIP(hipEventRecord(c->pinned_ev[s], c->copy_stream));
        VS_HIP(hipStreamWaitEvent(c->stream, c->pinned_ev[s], 0));
        HeapDevArgs a = heap_dev_args(h);
        a.pages = h->d_stage[s];
        a.first_block = first_block + b0;
        a.n_blocks = nb;
        hipEvent_t ev = prof_begin(c);
        if (toast) hipLaunchKernelGGL(k_heap_dev_toast, dim3(nb), dim3(WAVE), 0, c->stream, a);
        else hipLaunchKernelGGL(k_heap_dev_heap, dim3(nb), dim3(WAVE), 0, c->stream, a);
        VS_HIP(hipGetLastError());
        prof_end(c, PK_PAGES, ev);
        VS_HIP(hipMemcpyAsync(h->h_ctr, h->d_ctr, (HC_ERR + 5) * 4, hipMemcpyDeviceToHost, c->stream));
        VS_HIP(hipEventRecord(h->stage_ev[s], c->stream));
        h->slot ^= 1;
    }
    h->next_block[toast ? 1 : 0] = first_block + n_blocks;
    return heap_dev_report(h);
}

static int heap_dev_usable(vs_heap_dev* h, const char* what) {
    if (h->failed || h->finished) {
        vs_set_error("%s: the reader %s (only vs_heap_dev_close is defined)", what, h->failed ? "has reported an error" : "was finished");
        return VS_ERR_STATE;
    }
    return VS_OK;
}

extern "C" int vs_heap_dev_add(vs_heap_dev* h, uint32_t first_block, const void* pages, uint32_t n_blocks) {
    VS_REQUIRE(h && (pages || !n_blocks), "vs_heap_dev_add: null argument");
    VS_TRY(heap_dev_usable(h, "vs_heap_dev_add"));
    VS_REQUIRE(!h->toast_begun, "vs_heap_dev_add: the TOAST pass has begun");
    VS_REQUIRE(first_block >= h->next_block[0] && (uint64_t)first_block + n_blocks <= 0xFFFFFFFFull,
               "vs_heap_dev_add: block %u lies below the end of the previous range (%u): ranges ascend, gaps are allowed", first_block,
               h->next_block[0]);
    return vs_guard("vs_heap_dev_add", [&] { return heap_dev_feed(h, false, first_block, pages, n_blocks); });
}

// the heap pass is over: the references sorted by value id, none named twice
static int heap_dev_begin_toast(vs_heap_dev* h) {
    vs_ctx* c = h->ctx;
    hipStream_t st = c->stream;
    VS_HIP(hipSetDevice(c->device));
    VS_HIP(hipMemcpyAsync(h->h_ctr, h->d_ctr, HC_N * 4, hipMemcpyDeviceToHost, st));
    VS_HIP(hipStreamSynchronize(st));
    VS_TRY(heap_dev_report(h));
    const uint32_t nr = std::min(h->h_ctr[HC_NREFS], h->n);
    h->n_refs = nr;
    h->toast_begun = true;
    if (nr == 0) return VS_OK;
    VS_HIP(hipMalloc(&h->d_sref_vid, (size_t)nr * 4));
    VS_HIP(hipMalloc(&h->d_sref_idx, (size_t)nr * 4));
    VS_HIP(hipMalloc(&h->d_got, (size_t)nr * 4));
    VS_HIP(hipMemsetAsync(h->d_got, 0, (size_t)nr * 4, st));
    uint32_t* d_iota = nullptr;
    void* d_tmp = nullptr;
    auto run = [&]() -> int {
        VS_HIP(hipMalloc(&d_iota, (size_t)nr * 4));
        hipLaunchKernelGGL(k_heap_dev_iota, dim3(heap_dev_grid(nr, 256)), dim3(256), 0, st, d_iota, nr);
        VS_HIP(hipGetLastError());
        size_t tmp_bytes = 0;
        VS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (const uint32_t*)h->d_ref_vid, h->d_sref_vid, (const uint32_t*)d_iota,
                                                  h->d_sref_idx, (int)nr, 0, 32, st));
        VS_HIP(hipMalloc(&d_tmp, tmp_bytes + 16));
        VS_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp_bytes, (const uint32_t*)h->d_ref_vid, h->d_sref_vid, (const uint32_t*)d_iota,
                                                  h->d_sref_idx, (int)nr, 0, 32, st));
        hipLaunchKernelGGL(k_heap_dev_dups, dim3(heap_dev_grid(nr, 256)), dim3(256), 0, st, (const uint32_t*)h->d_sref_vid,
                           (const uint32_t*)h->d_sref_idx, (const uint32_t*)h->d_ref_blk, nr, h->d_ctr);
        VS_HIP(hipGetLastError());
        VS_HIP(hipMemcpyAsync(h->h_ctr, h->d_ctr, (HC_ERR + 5) * 4, hipMemcpyDeviceToHost, st));
        VS_HIP(hipStreamSynchronize(st));
        return VS_OK;
    };
    const int r = run();
    if (r != VS_OK) (void)hipStreamSynchronize(st);
    if (d_iota) (void)hipFree(d_iota);
    if (d_tmp) (void)hipFree(d_tmp);
    VS_TRY(r);
    return heap_dev_report(h);
}

extern "C" int vs_heap_dev_toast_add(vs_heap_dev* h, uint32_t first_block, const void* pages, uint32_t n_blocks) {
    VS_REQUIRE(h && (pages || !n_blocks), "vs_heap_dev_toast_add: null argument");
    VS_TRY(heap_dev_usable(h, "vs_heap_dev_toast_add"));
    VS_REQUIRE(first_block >= h->next_block[1] && (uint64_t)first_block + n_blocks <= 0xFFFFFFFFull,
               "vs_heap_dev_toast_add: block %u lies below the end of the previous range (%u): ranges ascend, gaps are allowed", first_block,
               h->next_block[1]);
    return vs_guard("vs_heap_dev_toast_add", [&]() -> int {
        if (!h->toast_begun) {
            const int r = heap_dev_begin_toast(h);
            if (r != VS_OK) {
                h->failed = true;
                return r;
            }
        }
        if (h->n_refs == 0) {  // (no external vector is wanted: nothing on these pages is)
            h->next_block[1] = first_block + n_blocks;
            return VS_OK;
        }
        return heap_dev_feed(h, true, first_block, pages, n_blocks);
    });
}

extern "C" int vs_heap_dev_finish(vs_heap_dev* h, vs_heap_info* info, uint8_t* found, uint32_t* n_compressed) {
    VS_REQUIRE(h, "vs_heap_dev_finish: null reader");
    VS_TRY(heap_dev_usable(h, "vs_heap_dev_finish"));
    return vs_guard("vs_heap_dev_finish", [&]() -> int {
        vs_ctx* c = h->ctx;
        hipStream_t st = c->stream;
        VS_HIP(hipSetDevice(c->device));
        uint8_t* d_found = nullptr;
        if (found && h->n) VS_HIP(hipMalloc(&d_found, h->n));
        auto run = [&]() -> int {
            if (h->n) {
                hipLaunchKernelGGL(k_heap_dev_finish, dim3(heap_dev_grid(h->n, WAVE)), dim3(WAVE), 0, st, (const uint8_t*)h->d_state, h->n, h->d_out,
                                   h->stride, h->dim, d_found, h->d_ctr);
                VS_HIP(hipGetLastError());
            }
            VS_HIP(hipMemcpyAsync(h->h_ctr, h->d_ctr, HC_N * 4, hipMemcpyDeviceToHost, st));
            VS_HIP(hipStreamSynchronize(st));
            VS_TRY(heap_dev_report(h));
            if (d_found) VS_TRY(vs_dev_download(c, found, d_found, h->n));
            return VS_OK;
        };
        const int r = run();
        if (r != VS_OK) (void)hipStreamSynchronize(st);
        if (d_found) (void)hipFree(d_found);
        h->failed = h->failed || r != VS_OK;
        VS_TRY(r);
        h->finished = true;
        const uint32_t* s = h->h_ctr + HC_STATE;
        vs_heap_info I{};
        I.n_nodes = h->n;
        I.heap_blocks = h->next_block[0];
        I.toast_blocks = h->next_block[1];
        I.n_inline = s[HS_INLINE];
        I.n_external = s[HS_EXTERNAL];
        I.n_deleted = s[HS_DELETED];
        I.n_null = s[HS_NULL];
        I.n_dead_line_pointer = s[HS_DEAD_LP];
        I.n_not_found = s[HS_NOT_FOUND] + s[HS_PENDING];
        I.n_toast_incomplete = s[HS_WAIT_TOAST];
        memcpy(&I.n_chunks, h->h_ctr + HC_CHUNKS, 8);
        if (info) *info = I;
        if (n_compressed) *n_compressed = s[HS_COMPRESSED];
        return VS_OK;
    });
}

extern "C" void vs_heap_dev_close(vs_heap_dev* h) { heap_dev_free(h); }
