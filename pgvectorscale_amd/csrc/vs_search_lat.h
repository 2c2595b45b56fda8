// vs_search_lat.h — k_search_lat, the latency-mode SBQ search kernel: a part of vs_search.hip kept in a file of its own (it uses
// PlainHeap, psync() and the address-space typedefs defined there).
//
// Every other search kernel here runs one wave per scan and lives off thousands of scans hiding each other's memory latency.  A lone
// scan is a serial chain of expansions, each two dependent memory round trips (the neighbor row, then the code rows it names) with
// nothing to overlap with.  k_search_lat gives ONE scan a workgroup of several waves and takes the round trips off the chain:
//
//   * wave 0, the OWNER, holds the scan: candidate heap (PlainHeap: [0, hl) in LDS, the rest in the workgroup's spill region),
//     dedup set (open addressing, one occupancy bit per slot, ids in LDS; only the bits are cleared per scan), visited list (sorted
//     (key, node) arrays with a moving head), stream and counters — k_search_plain's structures with the Hamming key in place of the
//     f32 key.  Nobody else touches them;
//   * an EXPANSION CACHE in LDS: per entry a node id, its neighbor list in list order and Hamming(query, code row) of every listed
//     neighbor, with a ready flag.  Hamming(query, node) is a pure function of immutable arrays, so a value that was computed early,
//     twice, or for a neighbor the dedup set rejects later cannot change a result.
//
// Work goes in rounds between two workgroup barriers:
//   FILL     the owner has published up to `spec` targets: the heap root and the following heap ARRAY positions (up to 6) whose nodes
//            have no entry — the second-best candidate is always a child of the root.  Target t is filled by wave t % waves (the
//            owner takes the root, so one entry and one target are still a complete kernel): a wave requests the neighbor rows of all
//            its targets at once, then gathers the code rows of every listed neighbor, 4 lanes x 16 B per row step, 16 rows x 2 steps
//            in flight, and stores ids and distances into the entry.
//   CONSUME  while the root has a ready entry, the owner makes the exact expansion from LDS alone: pop, visited insert, then in list
//            order per neighbor the dedup test-and-insert, the counters and the push with the cached distance — the reference's
//            rules, applied here and only here.  Rows leave through next() as in k_search.  A root without an entry ends the phase;
//            the owner picks the next targets and the entries they overwrite (empty ones first, never one holding a node at the top
//            of the heap unless the root itself would go without).
// One pair of round trips so serves several expansions, issued by several waves at once, and consecutive hits run back to back.
//
// Waves meet at __syncthreads() only: every wave executes the same barriers, and the owner's "finished" word is read by all of them
// after a barrier.  No wave spins on a flag.  Cache size, target count, wave count and victim choice are cost choices: no row, count
// or status depends on them.  A scan that outgrows a capacity publishes an empty stream and its status and is re-run whole by
// k_search (run_search_chunk).
struct LatArgs {
    const uint64_t* codes;
    const uint32_t* nbrs;
    const uint64_t* tids;
    uint32_t code_stride, nbr_stride, R, n, default_start;
    LatLaunch s;
};

#define LAT_MAX_WAVES 8
#define LAT_MAX_SPEC 7   // the root and heap array positions 1..6
#define LAT_WAVE_TARGETS 4  // targets one wave may be dealt: ceil(LAT_MAX_SPEC / 2 waves)
enum { LAT_FIN = 0, LAT_NT = 1, LAT_TNODE = 4, LAT_TENT = 12, LAT_CTL_WORDS = 20 };

// Hamming distances of four code rows (one per pass of 16 rows) against the query code in LDS, by groups of 4 lanes as ham_row4
// (vs_device.h), two 16-byte steps of every row requested before the first is consumed
__device__ __forceinline__ void lat_ham4x4(const uint64_t* const rows[4], const bool valid[4], const uint64_t* qc, int l4, uint32_t code_stride,
                                           uint32_t out[4]) {
    uint32_t acc[4] = {0u, 0u, 0u, 0u};
    for (uint32_t w = 2u * (uint32_t)l4; w < code_stride; w += 16) {
        ulonglong2 r0[4], r1[4];
        const bool two = w + 8 < code_stride;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            r0[p] = make_ulonglong2(0, 0);
            r1[p] = make_ulonglong2(0, 0);
            if (valid[p]) {
                r0[p] = load_stream16(rows[p] + w);
                if (two) r1[p] = load_stream16(rows[p] + w + 8);
            }
        }
        const ulonglong2 q0 = *reinterpret_cast<const ulonglong2*>(qc + w);
        ulonglong2 q1 = make_ulonglong2(0, 0);
        if (two) q1 = *reinterpret_cast<const ulonglong2*>(qc + w + 8);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (valid[p]) {
                acc[p] += (uint32_t)__popcll(r0[p].x ^ q0.x) + (uint32_t)__popcll(r0[p].y ^ q0.y);
                if (two) acc[p] += (uint32_t)__popcll(r1[p].x ^ q1.x) + (uint32_t)__popcll(r1[p].y ^ q1.y);
            }
        }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) out[p] = quad_sum(acc[p]);
}

// fills one cache entry: the neighbor list of `node` in list order (row0: its first 64 slots, already requested), its length up to
// the first InvalidBlockNumber, and the Hamming distance of the query code to every listed neighbor.  One wave; ids / ham are the
// entry's arrays of nbr_stride words in LDS.
__device__ __forceinline__ uint32_t lat_fill(const LatArgs& a, const uint64_t* qc, uint32_t node, uint32_t row0, uint32_t* ids, uint32_t* ham,
                                             int lane) {
    const uint32_t* nrow = a.nbrs + (size_t)node * a.nbr_stride;
    uint32_t cnt = 0;
    bool list_ended = false;
    for (uint32_t c0 = 0; c0 < a.R && !list_ended; c0 += WAVE) {
        const uint32_t slot = c0 + (uint32_t)lane;
        const uint32_t nid = c0 == 0 ? row0 : (slot < a.R ? load_stream32(nrow + slot) : VS_INVALID_NODE);
        const uint64_t inval = __ballot(nid == VS_INVALID_NODE);
        const uint32_t nvalid = inval ? (uint32_t)__builtin_ctzll(inval) : WAVE;
        if (nvalid < WAVE) list_ended = true;
        if ((uint32_t)lane < nvalid) *(pl_u32*)(ids + slot) = nid;
        psync();
        const uint64_t* rows[4];
        bool valid[4];
        uint32_t d[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const uint32_t j = (uint32_t)p * 16u + (uint32_t)(lane >> 2);
            valid[p] = j < nvalid;
            // (a listed id is a row of the index: the clamp only keeps a damaged list from reading beyond the codes)
            const uint32_t id = valid[p] ? min(*(const pl_u32*)(ids + c0 + j), a.n - 1u) : 0u;
            rows[p] = a.codes + (size_t)id * a.code_stride;
        }
        lat_ham4x4(rows, valid, qc, lane & 3, a.code_stride, d);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const uint32_t j = (uint32_t)p * 16u + (uint32_t)(lane >> 2);
            if (valid[p] && (lane & 3) == 0) *(pl_u32*)(ham + c0 + j) = d[p];
        }
        cnt += nvalid;
    }
    return cnt;
}

__global__ __launch_bounds__(LAT_MAX_WAVES* WAVE) void k_search_lat(LatArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tid = threadIdx.x, nthreads = blockDim.x;
    const int lane = (int)(tid & 63u);
    const uint32_t wave = tid >> 6, nwaves = nthreads >> 6;
    const uint32_t q = blockIdx.x;
    const LatLaunch& s = a.s;
    if (q >= s.nq) return;  // (the whole workgroup)
    const uint32_t C = s.cache;
    // ---- LDS carve (lat_lds_bytes; every offset a multiple of 16 B) ----
    uint64_t* qc = reinterpret_cast<uint64_t*>(smem);                                // code_stride words (even)
    uint64_t* heap_l = qc + a.code_stride;                                           // hl + 2 entries
    uint32_t* bm = reinterpret_cast<uint32_t*>(heap_l + round_up_u32(s.hl + 2, 2));  // one bit per dedup slot
    uint32_t* ltab = bm + round_up_u32(s.slots / 32, 4);                             // the ids
    uint32_t* vkey = ltab + s.slots;
    uint32_t* vid = vkey + round_up_u32(s.vcap, 4);
    uint32_t* ctl = vid + round_up_u32(s.vcap, 4);  // LAT_*: finished, target count, target nodes, target entries
    uint32_t* enode = ctl + LAT_CTL_WORDS;          // per cache entry: its node (VS_INVALID_NODE: empty) ...
    uint32_t* ecnt = enode + round_up_u32(C, 4);    // ... the length of its list ...
    uint32_t* eready = ecnt + round_up_u32(C, 4);   // ... and whether ids / distances are filled
    uint32_t* eids = eready + round_up_u32(C, 4);   // [C][nbr_stride]
    uint32_t* eham = eids + (size_t)C * a.nbr_stride;

    for (uint32_t i = tid; i < a.code_stride; i += nthreads) qc[i] = s.qcodes[(size_t)q * a.code_stride + i];
    for (uint32_t i = tid; i < s.slots / 32; i += nthreads) bm[i] = 0u;
    for (uint32_t i = tid; i < C; i += nthreads) {
        enode[i] = VS_INVALID_NODE;
        eready[i] = 0u;
    }
    __syncthreads();

    // ---- the owner's state (wave 0; the other waves carry it unused) ----
    const ScanVis svis = vis_of_scan(s.vis, q);
    const uint32_t smask = s.slots - 1;
    uint32_t nins = 0;
    PlainHeap heap{heap_l, s.heap_g + (size_t)q * (s.hcap > s.hl ? s.hcap - s.hl : 0), s.hl, 0, 0};
    uint32_t vhead = 0, vlen = 0, emitted = 0, status = 0;
    uint32_t st_visits = 0, st_cand = 0, st_dq = 0, st_reads = 0, st_next = 0, st_invis = 0;
    bool in_next = false;  // inside a call of TSVResponseIterator::next (st_next counted, no row handed out yet)

    // HashSet::insert for the active lanes' node ids (as k_search_plain: the caller has checked the table's room)
    auto prepare_insert = [&](uint32_t nid, bool act) -> bool {
        bool fresh = false, pending = act;
        uint32_t slot = hash_u32(nid) & smask;
        while (__ballot(pending)) {
            if (pending) {
                const uint32_t bit = 1u << (slot & 31u);
                const uint32_t old = atomicOr(&bm[slot >> 5], bit);
                if (!(old & bit)) {  // first write of this slot by this scan: whatever an earlier scan left there is never read
                    *(pl_u32*)(ltab + slot) = nid;
                    fresh = true;
                    pending = false;
                }
            }
            psync();
            if (pending) {
                const uint32_t v = *(const pl_u32*)(ltab + slot);
                if (v == nid) pending = false;
                else slot = (slot + 1) & smask;
            }
        }
        nins += (uint32_t)__popcll(__ballot(fresh));
        return fresh;
    };

    // ---- ListSearchResult::new from the default start node (AM/graph/mod.rs:97-124); empty() when there is none ----
    if (wave == 0 && a.default_start != VS_INVALID_NODE && a.n != 0) {
        const uint32_t sn = a.default_start;
        prepare_insert(sn, lane == 0);
        st_reads++;
        const uint32_t d = rfl(ham_row4(a.codes + (size_t)sn * a.code_stride, qc, lane & 3, a.code_stride, lane < 4));
        st_dq++;
        st_cand++;
        if (s.hcap == 0) status |= OVF_HEAP;
        else heap.push(((uint64_t)d << 32) | sn, lane);
    }

    for (;;) {
        if (wave == 0) {
            // ================= CONSUME: the scan itself, from LDS alone =================
            bool fin = false;
            for (;;) {
                if (!in_next) {  // TSVResponseIterator::next, repeated until M rows are emitted (AM/scan.rs:210-242)
                    if (emitted >= s.M || status) { fin = true; break; }
                    st_next++;
                    in_next = true;
                }
                // visit_closest(L) (AM/graph/mod.rs:153-170)
                bool can = heap.len > 0;
                uint32_t rootn = VS_INVALID_NODE;
                if (can) {
                    const uint64_t root = heap.get(0);
                    rootn = rfl((uint32_t)root);
                    if (vlen > s.L && rfl(PlainHeap::key(root)) >= rfl(vkey[vhead + s.L - 1])) can = false;
                }
                if (can) {
                    if (vlen + 1 > s.vcap) { status |= OVF_VISITED; fin = true; break; }
                    const uint64_t hit = __ballot((uint32_t)lane < C && enode[lane] == rootn && eready[lane] != 0u);
                    if (!hit) break;  // the root's list is not on chip yet: a fill round
                    const uint32_t e = (uint32_t)__builtin_ctzll(hit);
                    const uint64_t head = heap.pop(lane);
                    const uint32_t hd = rfl(PlainHeap::key(head));
                    const uint32_t node = rfl((uint32_t)head);
                    // visited.insert(partition_point(|x| *x < head), head): before the first element >= head
                    {
                        uint32_t idx = 0;
                        for (uint32_t base = 0; base < vlen; base += WAVE) {
                            const uint32_t i = base + lane;
                            const bool lt = i < vlen && vkey[vhead + i] < hd;
                            idx += (uint32_t)__popcll(__ballot(lt));
                        }
                        uint32_t at;
                        if (vhead > 0 && (2 * idx <= vlen || vhead + vlen >= s.vcap)) {
                            // shift [0, idx) left by one into the room consume left at the head, bottom chunk first
                            for (uint32_t lo = 0; lo < idx; lo += WAVE) {
                                const uint32_t i = lo + lane;
                                uint32_t td = 0, ti = 0;
                                if (i < idx) { td = vkey[vhead + i]; ti = vid[vhead + i]; }
                                psync();
                                if (i < idx) { vkey[vhead + i - 1] = td; vid[vhead + i - 1] = ti; }
                                psync();
                            }
                            vhead--;
                            at = vhead + idx;
                        } else {
                            uint32_t hi = vlen;
                            while (hi > idx) {  // shift [idx, vlen) right by one, top chunk first
                                const uint32_t lo = (hi - idx > WAVE) ? hi - WAVE : idx;
                                const uint32_t i = lo + lane;
                                uint32_t td = 0, ti = 0;
                                if (i < hi) { td = vkey[vhead + i]; ti = vid[vhead + i]; }
                                psync();
                                if (i < hi) { vkey[vhead + i + 1] = td; vid[vhead + i + 1] = ti; }
                                psync();
                                hi = lo;
                            }
                            at = vhead + idx;
                        }
                        if (lane == 0) { vkey[at] = hd; vid[at] = node; }
                        vlen++;
                        psync();
                    }
                    st_visits++;
                    // ---- visit_lsn_internal, Disk arm (AM/sbq/storage.rs:135-190), from the entry ----
                    st_reads++;  // SbqNode::read(visiting)
                    const uint32_t cnt = rfl(ecnt[e]);
                    const uint32_t* ids = eids + (size_t)e * a.nbr_stride;
                    const uint32_t* ham = eham + (size_t)e * a.nbr_stride;
                    for (uint32_t c0 = 0; c0 < cnt && status == 0; c0 += WAVE) {
                        const uint32_t nvalid = min(cnt - c0, (uint32_t)WAVE);
                        const bool act = (uint32_t)lane < nvalid;
                        const uint32_t nid = act ? *(const pl_u32*)(ids + c0 + lane) : VS_INVALID_NODE;
                        const uint32_t nd = act ? *(const pl_u32*)(ham + c0 + lane) : 0u;
                        if (s.ins_limit != 0xFFFFFFFFu && nins + nvalid > s.ins_limit) { status |= OVF_HASH; break; }
                        // prepare_insert; a distance is counted (and the node read) only for an id new to the set
                        const bool fresh = prepare_insert(nid, act);
                        uint64_t pm = __ballot(fresh);
                        const uint32_t c = (uint32_t)__popcll(pm);
                        st_reads += c;  // SbqNode::read(neighbor)
                        if (c == 0) continue;
                        st_dq += c;
                        st_cand += c;
                        if (heap.len + c > s.hcap) { status |= OVF_HEAP; break; }
                        // insert_neighbor in list order (AM/graph/mod.rs:144-147)
                        while (pm) {
                            const int j = __builtin_ctzll(pm);
                            pm &= pm - 1;
                            const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)nd, j);
                            const uint32_t id = (uint32_t)__builtin_amdgcn_readlane((int)nid, j);
                            heap.push(((uint64_t)d << 32) | id, lane);
                        }
                    }
                    if (lane == 0) enode[e] = VS_INVALID_NODE;  // a node is expanded once: its entry is free again
                    psync();
                    if (status) { fin = true; break; }
                    continue;
                }
                // ---- consume (AM/graph/mod.rs:174-184) + return_lsn (AM/sbq/storage.rs:404-414): visited.remove(0) moves the head ----
                if (vlen == 0) { fin = true; break; }  // None
                const uint32_t fd = rfl(vkey[vhead]);
                const uint32_t fnode = rfl(vid[vhead]);
                vhead++;
                vlen--;
                if (vlen == 0) vhead = 0;
                st_reads++;
                const uint64_t tidw = a.tids[fnode];
                if ((tidw & 0xFFFFull) == 0) continue;  // InvalidOffsetNumber: deleted tuple (AM/scan.rs:231-234)
                if (vis_hidden(svis, fnode)) {  // get_full_distance_for_resort -> None (AM/scan.rs:268-272)
                    st_invis++;
                    st_next++;  // the caller's loop asks `next` again
                    continue;
                }
                if (lane == 0) {
                    s.out_ids[(size_t)q * s.M + emitted] = fnode;
                    s.out_ham[(size_t)q * s.M + emitted] = fd;
                }
                emitted++;
                in_next = false;
            }
            // ================= the next round's targets: the root, then the heap array positions behind it =================
            uint32_t nt = 0;
            if (!fin) {
                const uint32_t np = min(heap.len, (uint32_t)LAT_MAX_SPEC);
                const uint32_t tn = (uint32_t)lane < np ? (uint32_t)heap.get((uint32_t)lane) : VS_INVALID_NODE;
                const uint32_t en = (uint32_t)lane < C ? enode[lane] : VS_INVALID_NODE;
                uint64_t prot = 0, miss = 0;
                for (uint32_t p = 0; p < np; ++p) {
                    const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)tn, (int)p);
                    const uint64_t h = __ballot((uint32_t)lane < C && en == x);
                    if (h) prot |= h;
                    else miss |= 1ull << p;
                }
                const uint64_t all = C >= 64 ? ~0ull : ((1ull << C) - 1ull);
                uint64_t empty = __ballot((uint32_t)lane < C && en == VS_INVALID_NODE);
                uint64_t avail = all & ~prot;
                for (uint32_t p = 0; p < np && nt < s.spec; ++p) {
                    if (!((miss >> p) & 1ull)) continue;
                    uint64_t pick = (avail & empty) ? (avail & empty) : avail;
                    if (!pick && p == 0) pick = all;  // the root never goes without: it takes the entry of a node behind it
                    if (!pick) break;
                    const uint32_t e = (uint32_t)__builtin_ctzll(pick);
                    avail &= ~(1ull << e);
                    empty &= ~(1ull << e);
                    const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)tn, (int)p);
                    if (lane == 0) {
                        ctl[LAT_TNODE + nt] = x;
                        ctl[LAT_TENT + nt] = e;
                        enode[e] = x;
                        eready[e] = 0u;
                    }
                    nt++;
                }
            }
            if (lane == 0) {
                ctl[LAT_FIN] = fin ? 1u : 0u;
                ctl[LAT_NT] = nt;
            }
        }
        __syncthreads();  // the targets (or the end of the scan) are published
        if (rfl(ctl[LAT_FIN])) break;
        // ================= FILL: target t belongs to wave t % nwaves =================
        {
            const uint32_t nt = rfl(ctl[LAT_NT]);
            uint32_t tnode[LAT_WAVE_TARGETS], tent[LAT_WAVE_TARGETS], row0[LAT_WAVE_TARGETS];
#pragma unroll
            for (int k = 0; k < LAT_WAVE_TARGETS; ++k) {  // the rows of all this wave's targets are requested before the first is used
                const uint32_t t = wave + (uint32_t)k * nwaves;
                tnode[k] = t < nt ? rfl(ctl[LAT_TNODE + t]) : VS_INVALID_NODE;
                tent[k] = t < nt ? rfl(ctl[LAT_TENT + t]) : 0u;
                row0[k] = VS_INVALID_NODE;
                if (tnode[k] != VS_INVALID_NODE && (uint32_t)lane < a.R) row0[k] = load_stream32(a.nbrs + (size_t)tnode[k] * a.nbr_stride + lane);
            }
#pragma unroll
            for (int k = 0; k < LAT_WAVE_TARGETS; ++k) {
                if (tnode[k] == VS_INVALID_NODE) continue;  // (wave-uniform)
                const uint32_t e = tent[k];
                const uint32_t cnt = lat_fill(a, qc, tnode[k], row0[k], eids + (size_t)e * a.nbr_stride, eham + (size_t)e * a.nbr_stride, lane);
                if (lane == 0) {
                    ecnt[e] = cnt;
                    eready[e] = 1u;
                }
            }
        }
        __syncthreads();  // the entries are ready
    }

    if (wave != 0) return;
    // a scan that outgrew a capacity publishes an empty stream: the general kernel re-runs it whole
    if (status) emitted = 0;
    for (uint32_t i = emitted + lane; i < s.M; i += WAVE) {
        s.out_ids[(size_t)q * s.M + i] = VS_INVALID_NODE;
        s.out_ham[(size_t)q * s.M + i] = 0xFFFFFFFFu;
    }
    if (lane == 0) {
        s.out_cnt[q] = emitted;
        s.status[q] = status;
        uint32_t* st = s.stats + (size_t)q * ST_N;
        st[ST_VISITS] = st_visits;
        st[ST_CAND] = st_cand;
        st[ST_DQ] = st_dq;
        st[ST_READS] = st_reads;
        st[ST_NEXT] = st_next;
        st[ST_GSPILL] = heap.maxlen;
        st[ST_INVIS] = st_invis;
        st[ST_INS] = nins;
    }
}

// LDS of one scan of k_search_lat, in bytes:
//   8 * code_stride                      the query code
// + 8 * round_up(hl + 2, 2)              the heap's LDS part
// + 4 * round_up(slots / 32, 4)          one occupancy bit per dedup slot
// + 4 * slots                            the dedup table's ids
// + 8 * round_up(vcap, 4)                visited list (keys, nodes)
// + 4 * LAT_CTL_WORDS                    the round's control words
// + 12 * round_up(cache, 4)              per entry: node, list length, ready flag
// + 8 * cache * nbr_stride               per entry: the listed ids and their distances
size_t lat_lds_bytes(const vs_index* idx, const LatLaunch& s) {
    const size_t b = (size_t)idx->code_stride * 8 + (size_t)round_up_u32(s.hl + 2, 2) * 8 + (size_t)round_up_u32(s.slots / 32, 4) * 4 +
                     (size_t)s.slots * 4 + 2 * (size_t)round_up_u32(s.vcap, 4) * 4 + LAT_CTL_WORDS * 4 + 3 * (size_t)round_up_u32(s.cache, 4) * 4 +
                     2 * (size_t)s.cache * idx->nbr_stride * 4;
    return (b + 15) / 16 * 16;
}

int launch_search_lat(vs_index* idx, const LatLaunch& s) {
    if (s.nq == 0) return VS_OK;
    VS_REQUIRE(idx->d.storage_type != VS_STORAGE_PLAIN && idx->codes && idx->d.n > 0, "latency search kernel: not an SBQ index with its codes");
    VS_REQUIRE(s.waves >= 2 && s.waves <= LAT_MAX_WAVES && s.cache >= 1 && s.cache <= 64 && s.spec >= 1 && s.spec <= LAT_MAX_SPEC,
               "latency search kernel: 2..8 waves, 1..64 cache entries and 1..7 targets per round");
    VS_REQUIRE(s.slots >= 64 && (s.slots & (s.slots - 1)) == 0 && (s.ins_limit == 0xFFFFFFFFu ? idx->d.n < s.slots : s.ins_limit <= s.slots / 4 * 3),
               "latency search kernel: the dedup table must be a power of two of slots with room beyond its limit");
    VS_REQUIRE(s.vcap >= 1 && s.L >= 1 && s.hl <= s.hcap && s.heap_g && s.qcodes, "latency search kernel: bad capacities or buffers");
    const size_t lds = lat_lds_bytes(idx, s);
    VS_REQUIRE(lds <= LAT_LDS_BUDGET, "latency search state does not fit LDS (%zu B)", lds);
    static DeviceOnce attr_set;
    const int attr_dev = idx->ctx->device;
    if (attr_set.pending(attr_dev)) {
        VS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_search_lat), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set.done(attr_dev);
    }
    LatArgs a;
    a.codes = idx->codes;
    a.nbrs = idx->nbrs;
    a.tids = idx->tids;
    a.code_stride = idx->code_stride;
    a.nbr_stride = idx->nbr_stride;
    a.R = idx->d.num_neighbors;
    a.n = idx->d.n;
    a.default_start = idx->d.default_start;
    a.s = s;
    hipLaunchKernelGGL(k_search_lat, dim3(s.nq), dim3(s.waves * WAVE), lds, idx->ctx->stream, a);
    VS_HIP(hipGetLastError());
    return VS_OK;
}
