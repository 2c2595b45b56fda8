// vs_pages_out.h — the host half of the page writer (vs_pages.cpp), shared with its device half (vs_pages_dev.hip).
// Plain C++: no HIP in here.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/vsgpu.h"

// vs_pages_add's header checks over one page outside a reader -> the SbqNode items on it (0: a new page, another page type)
extern "C" int vs_pages_header_items(const void* page, uint32_t page_size, uint32_t block, uint32_t* sbq_items);
// the same with the page type that counts named: VS_PAGE_SBQ_NODE, or VS_PAGE_NODE for the PlainNode items of a `plain` relation
extern "C" int vs_pages_header_items_of(const void* page, uint32_t page_size, uint32_t block, uint32_t node_page_type, uint32_t* items);

// The whole layout of the relation a vs_pages_out writes, fixed at open.
struct PagesOutPlan {
    uint32_t page_size = VS_BLCKSZ;
    uint32_t n = 0, W = 0, R = 0;  // plain: W = the dimensions of PlainNode.vector (num_dimensions_to_index)
    bool has_labels = false;
    bool plain = false;          // PlainNode items on PageType::Node pages, no SbqMeans chain (vs_pages_out_plan_plain)
    vs_node_layout lay{};        // off_labels = where the last 8-byte field goes (labels, the empty _neighbor_vectors, or a plain
                                 // node's empty pq_vector)
    uint32_t first_node_block = 0, n_node_pages = 0, n_blocks = 0;
    // classic and plain nodes: every item has item_size bytes, K of them fill a page
    uint32_t item_size = 0, K = 0;
    // labeled nodes: first node of every node page (n_node_pages + 1 entries, the last one = n) and, until the device half has
    // taken them over, block and lp_off of every node's item
    std::vector<uint32_t> page_first;
    std::vector<uint32_t> node_block;
    std::vector<uint16_t> node_lpoff;
    // Meta chain and SbqMeans chain, by block number (ascending)
    std::vector<std::pair<uint32_t, std::vector<uint8_t>>> host_pages;
    uint32_t pages_by_type[9] = {0};
    uint64_t n_label_vals = 0;
};

// label_off: host copy of the index's label offsets (n + 1 entries) for labeled nodes, else null; ls_labels / ls_nodes: the
// labeled start nodes (d.n_label_starts entries, node ids)
int vs_pages_out_plan(const vs_index_desc& d, const vs_pages_out_params& p, const float* mean, const float* m2, uint64_t count,
                      const uint32_t* label_off, const int16_t* ls_labels, const uint32_t* ls_nodes, PagesOutPlan& plan);
// the same for a `plain` index (vs_pages_out_open_plain): Meta chain on block 0, node pages from block 1 on
int vs_pages_out_plan_plain(const vs_index_desc& d, const vs_pages_out_params& p, PagesOutPlan& plan);
int vs_pages_out_plan_item_pointer(const PagesOutPlan& plan, uint32_t node, uint32_t* block, uint32_t* offset);

// What a relation looked like when it was last written (vs_pages_out_baseline / vs_pages_out_delta): one 128-bit digest per block
// in device memory (node pages; the entries of host-encoded blocks stay zero) and the host-encoded pages themselves.  Belongs to a
// device, not to a writer or an index: it outlives both.
struct vs_pages_base {
    int device = 0;
    uint32_t page_size = VS_BLCKSZ;
    uint32_t n_blocks = 0, first_node_block = 0, n_node_pages = 0;
    uint64_t* d_digest = nullptr;  // [n_blocks][2]
    std::vector<std::pair<uint32_t, std::vector<uint8_t>>> host_pages;  // as PagesOutPlan::host_pages
};
// the host-encoded pages of `plan` that are not, byte for byte, what `base` recorded at the same block (ascending)
void vs_pages_out_host_delta(const PagesOutPlan& plan, const vs_pages_base& base, std::vector<uint32_t>& dirty);
// the host-encoded page at `block`, or nullptr when the block is a node page
const uint8_t* vs_pages_out_plan_host_page(const PagesOutPlan& plan, uint32_t block);
