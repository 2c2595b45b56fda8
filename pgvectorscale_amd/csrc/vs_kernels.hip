// vs_kernels.hip — hand-written gfx950 (CDNA4, wave64) kernels of the StreamingDiskANN search path.
//
//   K4 k_prepare_queries / k_quantize_rows : SbqQuantizer::quantize            (AM/sbq/quantize.rs:52-102)
//   K1 k_hamming_gather                    : distance_xor_optimized on gathers (AM/distance/mod.rs:266-323)
//   K2 k_rerank                            : distance_l2/cosine/inner_product in the reference's AVX2 accumulation
//                                            order (AM/distance/mod.rs:325-435, AM/sbq/storage.rs:304-328)
//   K3 k_search (vs_search.hip)            : ListSearchResult + greedy_search_iterate + visit_lsn_internal +
//                                            TSVResponseIterator::next (AM/graph/mod.rs:74-185,357-385,
//                                            AM/sbq/storage.rs:135-190, AM/scan.rs:210-242)
//      k_resort                            : the rescore window of next_with_resort (AM/scan.rs:244-305)
//
// All of this is HBM-latency / bandwidth bound integer + f32 dot work: no MFMA.  One wave64 owns one query in
// K3 (the search is a serial chain of dependent expansions), lanes cooperate on the R gathered neighbor codes
// (4 lanes x 16 B per code row), the candidate heap / visited list live in LDS, the dedup hash set in L2.
// Compiled with -ffp-contract=off: the reference's L2 kernel uses separate mul+add, its dot kernel FMA.
#include "vs_internal.h"
#include "vs_device.h"

// ---------------------------------------------------------------------------------------------------------------
// preprocess_cosine on a vector held in LDS (AM/distance/mod.rs:225-253): sequential f32 sum of squares (the owner's lane 0),
// then the owner's lanes divide (lane, lane + stride, ...).  buf is normalised in place.  The barriers are workgroup wide: every
// thread of the workgroup calls this, `active` = this thread's wave owns a vector (one wave per workgroup: always).
// ---------------------------------------------------------------------------------------------------------------
__device__ void lds_preprocess_cosine(float* buf, uint32_t n, int lane, uint32_t stride, float* bcast /* LDS scratch [1] */, bool active = true) {
    __syncthreads();
    if (active && lane == 0) {
        float norm = 0.0f;
        for (uint32_t i = 0; i < n; ++i) {
            float p = buf[i] * buf[i];
            norm = norm + p;
        }
        const float eps = 1.1920929e-07f;  // f32::EPSILON
        float adj = eps * (float)n;
        float s = 0.0f;  // 0 => leave alone
        if (!(norm < eps) && !(norm >= 1.0f - adj && norm <= 1.0f + adj)) s = sqrtf(norm);
        *bcast = s;
    }
    __syncthreads();
    if (active) {
        float s = *bcast;
        if (s != 0.0f)
            for (uint32_t i = lane; i < n; i += stride) buf[i] = buf[i] / s;
    }
    __syncthreads();
}

// SbqQuantizer::quantize of a vector in LDS, one wave: lane = bit position inside the output word (ballot packs).
__device__ void wave_quantize(const float* v, uint32_t dims, uint32_t bits, const float* __restrict__ mean,
                              const float* __restrict__ m2, float count_f, uint64_t* out, uint32_t words,
                              uint32_t out_stride, int lane) {
    for (uint32_t w = 0; w < out_stride; ++w) {
        uint64_t word = 0;
        if (w < words) {
            uint32_t g = w * 64u + (uint32_t)lane;  // global bit index
            uint32_t dim = g / bits;
            uint32_t j = g - dim * bits;
            bool bit = false;
            if (dim < dims) {
                float x = v[dim];
                float mu = mean[dim];
                if (bits == 1) {
                    bit = x > mu;
                } else {
                    float variance = m2[dim] / count_f;
                    float std_dev = sqrtf(variance);
                    float ranges = (float)(bits + 1);
                    float z = (x - mu) / std_dev;
                    float index = (z + 2.0f) / (4.0f / ranges);
                    uint32_t ones = 0;
                    if (!(index < 1.0f)) {  // NaN falls through like Rust's `if index < 1.0 {} else {..}`
                        float fl = floorf(index);
                        // `fl as usize` saturating, NaN -> 0; then min(bits)
                        if (fl != fl) ones = 0;
                        else if (fl >= (float)bits) ones = bits;
                        else if (fl <= 0.0f) ones = 0;
                        else ones = (uint32_t)fl;
                    }
                    bit = j < ones;
                }
            }
            word = __ballot(bit);
        }
        if (lane == 0) out[w] = word;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// K4a: query preparation = PgVector::from_datum(index=true, full=true) (AM/pg_vector.rs:162-199) +
//      SbqSearchDistanceMeasure::new (AM/sbq/mod.rs:145-148).
// A workgroup of NW waves prepares NW queries per round (one per wave, each in its own LDS slice) for `rounds` rounds.  What belongs
// to the index and not to the query is staged once per workgroup: the means and the per-dimension standard deviations
// sqrtf(m2 / count) — the expression of SbqQuantizer::quantize, so every bit stays — instead of a square root and a division per
// output BIT of every query.  Per query the number of one-bits of a dimension is computed once per dimension (lane = dimension), the
// words are then packed with ballots (lane = bit) and stored 64 at a time by all lanes; q_full goes out as float4.
// Barriers are workgroup wide and every wave passes the same ones (a wave without a query idles through them).
// (The deviations are not cached per index: mean / m2 are written through vs_index_set_quantizer, training, broadcasts, clones AND the
// device pointers vs_index_array hands out, so a derived array could go stale unseen; 16 queries per workgroup amortise them instead.
// q_full is still written for every distance type: the second attempts, the general kernel on plain storage and a finish that
// redoes the window read w.q_full after the call has returned, when the caller's query buffer is no longer the library's to read.)
// LDS: [dim_index] mean | [dim_index] std (bits > 1) | per wave: [r4(dim_full)] full | [r4(dim_index)] index slice (if different) |
//      [r4(dim_index)] u32 ones (bits > 1) | [4] scratch.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_prepare_queries(const float* __restrict__ raw, uint32_t nq,
                                                         uint32_t dim_full, uint32_t dim_index, uint32_t vec_stride,
                                                         uint32_t distance_type, uint32_t bits,
                                                         const float* __restrict__ mean, const float* __restrict__ m2,
                                                         float count_f, uint32_t words, uint32_t code_stride, uint32_t rounds,
                                                         uint32_t vec4, float* __restrict__ q_full, uint64_t* __restrict__ qcodes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t nw = blockDim.x >> 6;
    const bool same = dim_full == dim_index;
    const bool quant = words != 0, multi = quant && bits != 1;
    const uint32_t rf = round_up_u32(dim_full, 4), ri = round_up_u32(dim_index, 4);
    float* mu = reinterpret_cast<float*>(smem);
    float* sdv = mu + (quant ? ri : 0u);
    float* wbase = sdv + (multi ? ri : 0u);
    const uint32_t per_wave = rf + (same ? 0u : ri) + (multi ? ri : 0u) + 4u;
    float* full = wbase + (size_t)wave * per_wave;
    float* idxv = same ? full : full + rf;
    uint32_t* ones = reinterpret_cast<uint32_t*>((same ? full : idxv) + (same ? rf : ri));
    float* bc = reinterpret_cast<float*>(ones + (multi ? ri : 0u));
    if (quant)
        for (uint32_t i = threadIdx.x; i < dim_index; i += blockDim.x) {
            mu[i] = mean[i];
            if (multi) {
                float variance = m2[i] / count_f;
                sdv[i] = sqrtf(variance);
            }
        }
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t q = (blockIdx.x * rounds + r) * nw + (uint32_t)wave;
        const bool active = q < nq;
        __syncthreads();  // (the staged statistics; the slices of the round before)
        if (active) {
            const float* src = raw + (size_t)q * dim_full;
            if (vec4) {
                for (uint32_t i = lane; i < dim_full / 4; i += WAVE)
                    reinterpret_cast<float4*>(full)[i] = reinterpret_cast<const float4*>(src)[i];
            } else {
                for (uint32_t i = lane; i < rf; i += WAVE) full[i] = i < dim_full ? src[i] : 0.0f;
            }
            if (!same)
                for (uint32_t i = lane; i < dim_index; i += WAVE) idxv[i] = src[i];
        }
        if (distance_type == VS_COSINE) {
            lds_preprocess_cosine(full, dim_full, lane, WAVE, bc, active);
            if (!same) lds_preprocess_cosine(idxv, dim_index, lane, WAVE, bc, active);
        } else {
            __syncthreads();
        }
        if (active) {
            float* qf = q_full + (size_t)q * vec_stride;  // (vec_stride = r4(dim_full); rows are 16-byte aligned)
            for (uint32_t i = lane; i < vec_stride / 4; i += WAVE) reinterpret_cast<float4*>(qf)[i] = reinterpret_cast<const float4*>(full)[i];
            if (multi) {
                const float ranges = (float)(bits + 1);
                for (uint32_t dim = lane; dim < dim_index; dim += WAVE) {
                    float x = idxv[dim];
                    float z = (x - mu[dim]) / sdv[dim];
                    float index = (z + 2.0f) / (4.0f / ranges);
                    uint32_t o = 0;
                    if (!(index < 1.0f)) {  // NaN falls through like Rust's `if index < 1.0 {} else {..}`
                        float fl = floorf(index);
                        // `fl as usize` saturating, NaN -> 0; then min(bits)
                        if (fl != fl) o = 0;
                        else if (fl >= (float)bits) o = bits;
                        else if (fl <= 0.0f) o = 0;
                        else o = (uint32_t)fl;
                    }
                    ones[dim] = o;
                }
            }
        }
        __syncthreads();
        if (active) {
            uint64_t* out = qcodes + (size_t)q * code_stride;
            uint64_t mine = 0;
            for (uint32_t w = 0; w < code_stride; ++w) {
                uint64_t word = 0;
                if (w < words) {
                    const uint32_t g = w * 64u + (uint32_t)lane;  // global bit index
                    const uint32_t dim = g / bits;
                    const uint32_t j = g - dim * bits;
                    bool bit = false;
                    if (dim < dim_index) bit = multi ? j < ones[dim] : idxv[dim] > mu[dim];
                    word = __ballot(bit);
                }
                if ((uint32_t)lane == (w & 63u)) mine = word;
                if ((w & 63u) == 63u || w + 1 == code_stride) {
                    const uint32_t w0 = w & ~63u;
                    if (w0 + (uint32_t)lane <= w) out[w0 + lane] = mine;
                }
            }
        }
    }
}

// plain storage with num_dimensions_to_index < num_dimensions: the graph search compares the INDEX slice of the query,
// cosine-normalised on its own (PgVector::from_datum, AM/pg_vector.rs:143-157), with the stored index-slice vectors
__global__ __launch_bounds__(WAVE) void k_prepare_index_slice(const float* __restrict__ raw, uint32_t nq, uint32_t dim_full,
                                                              uint32_t dim_index, uint32_t vec_stride, uint32_t distance_type,
                                                              float* __restrict__ q_index) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* idxv = reinterpret_cast<float*>(smem);
    float* bc = idxv + round_up_u32(dim_index, 4);
    const int lane = threadIdx.x;
    const uint32_t q = blockIdx.x;
    if (q >= nq) return;
    for (uint32_t i = lane; i < dim_index; i += WAVE) idxv[i] = raw[(size_t)q * dim_full + i];
    __syncthreads();
    if (distance_type == VS_COSINE) lds_preprocess_cosine(idxv, dim_index, lane, blockDim.x, bc);
    for (uint32_t i = lane; i < vec_stride; i += WAVE) q_index[(size_t)q * vec_stride + i] = i < dim_index ? idxv[i] : 0.0f;
}

// K4b: quantize rows that are already prepared (normalised if cosine): one wave per row.
__global__ __launch_bounds__(WAVE) void k_quantize_rows(const float* __restrict__ rows, uint32_t row_stride,
                                                        uint32_t nrows, uint32_t dims, uint32_t bits,
                                                        const float* __restrict__ mean, const float* __restrict__ m2,
                                                        float count_f, uint32_t words, uint32_t code_stride,
                                                        uint64_t* __restrict__ codes) {
    const int lane = threadIdx.x;
    for (uint32_t r = blockIdx.x; r < nrows; r += gridDim.x)
        wave_quantize(rows + (size_t)r * row_stride, dims, bits, mean, m2, count_f, codes + (size_t)r * code_stride,
                      words, code_stride, lane);
}

// ---------------------------------------------------------------------------------------------------------------
// K1: Hamming distances of gathered code rows.  One wave per query; 16 rows per pass.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WAVE) void k_hamming_gather(const uint64_t* __restrict__ codes, uint32_t code_stride,
                                                         const uint64_t* __restrict__ qcodes,
                                                         const uint32_t* __restrict__ ids,
                                                         const uint32_t* __restrict__ off, uint32_t nq,
                                                         uint32_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* qc = reinterpret_cast<uint64_t*>(smem);
    const int lane = threadIdx.x;
    const uint32_t q = blockIdx.x;
    if (q >= nq) return;
    for (uint32_t w = lane; w < code_stride; w += WAVE) qc[w] = qcodes[(size_t)q * code_stride + w];
    __syncthreads();
    const uint32_t b = off[q], e = off[q + 1];
    for (uint32_t base = b; base < e; base += 16) {
        uint32_t j = base + (uint32_t)(lane >> 2);
        bool valid = j < e;
        uint32_t id = valid ? ids[j] : 0;
        uint32_t d = ham_row4(codes + (size_t)id * code_stride, qc, lane & 3, code_stride, valid);
        if (valid && (lane & 3) == 0) out[j] = d;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// K2: rerank.  One workgroup (4 waves) per query, query vector staged in LDS; 8 lanes per candidate row, float4
// loads: lane l8 owns elements 32t+4*l8..+3 of every 32-float step, i.e. exactly 4 of the 32 "virtual AVX2 lanes"
// (4 accumulators x 8 lanes) of distance_l2_simd_body!/inner_product_simd_body! (AM/distance/mod.rs:325-435).
// Final reduction replays horizontal_add_ps per accumulator and the left-to-right sum of the 4 accumulators, so the
// result is the same f32 the AVX2 reference produces (bit-for-bit, given the same hadd lane order).
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float shfl_f(float v, int src) { return __shfl(v, src, WAVE); }

// distance of one candidate row to the query in LDS, computed by the 8 lanes of a group (all 64 lanes call it; !valid groups idle).
// The result is returned on the group's lane l8 == 0 (other lanes: unspecified).  s = the row's cosine divisor (0: leave alone).
__device__ __forceinline__ float rerank_row_dist(const float* __restrict__ row, const float* qv, float s, uint32_t distance_type,
                                                 uint32_t steps, uint32_t dim_full, int lane, int l8, bool valid) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (valid) {
        if (distance_type == VS_L2) {
            for (uint32_t t = 0; t < steps; ++t) {
                float4 x = *reinterpret_cast<const float4*>(row + 32 * t + 4 * l8);
                float4 y = *reinterpret_cast<const float4*>(qv + 32 * t + 4 * l8);
                float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
                float p0 = d0 * d0, p1 = d1 * d1, p2 = d2 * d2, p3 = d3 * d3;
                a0 = a0 + p0;
                a1 = a1 + p1;
                a2 = a2 + p2;
                a3 = a3 + p3;
            }
        } else {
            for (uint32_t t = 0; t < steps; ++t) {
                float4 x = *reinterpret_cast<const float4*>(row + 32 * t + 4 * l8);
                float4 y = *reinterpret_cast<const float4*>(qv + 32 * t + 4 * l8);
                if (s != 0.0f) {
                    x.x = x.x / s;
                    x.y = x.y / s;
                    x.z = x.z / s;
                    x.w = x.w / s;
                }
                a0 = __builtin_fmaf(x.x, y.x, a0);
                a1 = __builtin_fmaf(x.y, y.y, a1);
                a2 = __builtin_fmaf(x.z, y.z, a2);
                a3 = __builtin_fmaf(x.w, y.w, a3);
            }
        }
    }
    // horizontal_add_ps of accumulator j lives on lanes (2j, 2j+1) of the 8-lane group:
    // s_c = a_c + a_{c+4}; h = (s0+s1)+(s2+s3)
    float s0 = a0 + shfl_f(a0, lane ^ 1);
    float s1 = a1 + shfl_f(a1, lane ^ 1);
    float s2 = a2 + shfl_f(a2, lane ^ 1);
    float s3 = a3 + shfl_f(a3, lane ^ 1);
    float t0 = s0 + s1;
    float t1 = s2 + s3;
    float h = t0 + t1;
    const int g0 = lane & ~7;
    float h0 = shfl_f(h, g0 + 0), h1 = shfl_f(h, g0 + 2), h2 = shfl_f(h, g0 + 4), h3 = shfl_f(h, g0 + 6);
    float dist = h0 + h1;
    dist = dist + h2;
    dist = dist + h3;
    float r = dist;
    if (valid && l8 == 0) {
        for (uint32_t i = steps * 32; i < dim_full; ++i) {  // scalar tail, in element order
            float x = row[i];
            if (distance_type == VS_L2) {
                float diff = x - qv[i];
                float p = diff * diff;
                dist = dist + p;
            } else {
                if (s != 0.0f) x = x / s;
                float p = x * qv[i];
                dist = dist + p;
            }
        }
        if (distance_type == VS_L2) r = dist;
        else if (distance_type == VS_IP) r = -dist;
        else r = fmaxf(1.0f - dist, 0.0f);
    }
    return r;
}

// Which place of a batch's rerank order workgroup b takes (VS_RERANK_ORDER, k_scan_regions below).  deal == 0: place b.  deal != 0:
// the hardware hands consecutive workgroups to the 8 XCDs in turn, so workgroup b takes place (b % 8) * ceil(nq / 8) + b / 8 — each
// XCD walks its own contiguous eighth of the order and scans that share rows meet in one L2.  The grid is 8 * ceil(nq / 8) then; places
// >= nq do not exist.
__device__ static inline uint32_t rerank_slot(uint32_t b, uint32_t nq, uint32_t deal) {
    if (!deal) return b;
    const uint32_t per = (nq + 7) / 8;
    return (b & 7u) * per + (b >> 3);
}

static inline uint32_t rerank_grid(uint32_t nq, bool deal) { return deal ? (nq + 7) / 8 * 8 : nq; }

__global__ __launch_bounds__(256) void k_rerank(const float* __restrict__ vecs, uint32_t vec_stride, uint32_t dim_full,
                                                const float* __restrict__ vnorm, uint32_t distance_type,
                                                const float* __restrict__ q_full, const uint32_t* __restrict__ ids,
                                                const uint32_t* __restrict__ off, const uint32_t* __restrict__ cnt,
                                                uint32_t fixed_m, uint32_t nq, float* __restrict__ out, uint32_t row_base,
                                                const uint32_t* __restrict__ perm, uint32_t deal) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* qv = reinterpret_cast<float*>(smem);
    const uint32_t slot = rerank_slot(blockIdx.x, nq, deal);
    if (slot >= nq) return;
    const uint32_t q = perm ? perm[slot] : slot;
    for (uint32_t i = threadIdx.x; i < vec_stride; i += blockDim.x) qv[i] = q_full[(size_t)q * vec_stride + i];
    __syncthreads();
    uint32_t b, e;
    if (off) {
        b = off[q];
        e = off[q + 1];
    } else {
        b = q * fixed_m;
        e = b + (cnt ? min(cnt[q], fixed_m) : fixed_m);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l8 = lane & 7, grp = lane >> 3;
    const uint32_t steps = dim_full / 32;
    for (uint32_t base = b; base < e; base += 32) {
        uint32_t j = base + (uint32_t)(wave * 8 + grp);
        bool valid = j < e;
        // ids == nullptr: the contiguous rows row_base .. row_base + fixed_m - 1 (exact brute force, vs_bruteforce_topk)
        uint32_t id = valid ? (ids ? ids[j] : row_base + (j - b)) : VS_INVALID_NODE;
        if (id == VS_INVALID_NODE) valid = false;
        const float* row = vecs + (size_t)(valid ? id : 0) * vec_stride;
        float s = 0.0f;
        if (valid && distance_type == VS_COSINE) s = vnorm[id];
        const float r = rerank_row_dist(row, qv, s, distance_type, steps, dim_full, lane, l8, valid);
        // (a row without a node is skipped, as ever: its slot of `out` keeps what it held.  The search kernels never emit one inside
        // cnt[q]; k_rerank_window gives such a row NaN, which no window of real rows would tell apart)
        if (valid && l8 == 0) out[j] = r;
    }
}

// per-node cosine divisor cache: exact preprocess_cosine_get_norm (sequential f32 sum).  A wave owns 64 rows;
// a [64 rows][64 dims] tile is staged through LDS so global reads stay coalesced while each lane walks one row
// in element order.
__global__ __launch_bounds__(WAVE) void k_row_norms(const float* __restrict__ vecs, uint32_t vec_stride, uint32_t dim,
                                                    uint32_t n, float* __restrict__ vnorm) {
    __shared__ float tile[64][65];
    const int lane = threadIdx.x;
    for (uint32_t row0 = blockIdx.x * 64u; row0 < n; row0 += gridDim.x * 64u) {
        float norm = 0.0f;
        for (uint32_t d0 = 0; d0 < dim; d0 += 64) {
            for (int r = 0; r < 64; ++r) {
                uint32_t row = row0 + r;
                uint32_t d = d0 + lane;
                tile[r][lane] = (row < n && d < dim) ? vecs[(size_t)row * vec_stride + d] : 0.0f;
            }
            __syncthreads();
            uint32_t lim = min(64u, dim - d0);
            for (uint32_t c = 0; c < lim; ++c) {
                float v = tile[lane][c];
                float p = v * v;
                norm = norm + p;
            }
            __syncthreads();
        }
        uint32_t row = row0 + lane;
        if (row < n) {
            const float eps = 1.1920929e-07f;
            float adj = eps * (float)dim;
            float s = 0.0f;
            if (!(norm < eps) && !(norm >= 1.0f - adj && norm <= 1.0f + adj)) s = sqrtf(norm);
            vnorm[row] = s;
        }
    }
}

// duplicate ids inside one neighbor list would make the wave-parallel dedup order-dependent: reject them at upload.
__global__ void k_validate_nbrs(const uint32_t* __restrict__ nbrs, uint32_t nbr_stride, uint32_t R, uint32_t n,
                                uint32_t* flag) {
    uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const uint32_t* r = nbrs + (size_t)row * nbr_stride;
    uint32_t deg = 0;
    while (deg < R && r[deg] != VS_INVALID_NODE) {
        if (r[deg] >= n) atomicOr(flag, 2u);
        ++deg;
    }
    for (uint32_t i = 1; i < deg; ++i)
        for (uint32_t j = 0; j < i; ++j)
            if (r[i] == r[j]) atomicOr(flag, 1u);
}

// ---------------------------------------------------------------------------------------------------------------
// Rescore window of next_with_resort (AM/scan.rs:244-305): BinaryHeap<ResortData> with
// cmp(self, other) = other.distance.total_cmp(self.distance)  (AM/scan.rs:111-117).  One thread per query.
// heap entries: (total_cmp key as i32 in the high word, stream position in the low word).
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t total_key(float f) {
    int32_t b = __float_as_int(f);
    b ^= (int32_t)(((uint32_t)(b >> 31)) >> 1);
    return b;
}

// The window as the reference runs it: pushes while the heap holds fewer than `rescore` entries and the stream has rows, then one pop
// per output row.  h: room for `rescore` entries; sd: the n reranked distances in stream order; emit(sp) takes the stream position of
// every row popped.  Returns the number of rows popped (<= k).  Serial: one thread.
template <class Emit>
__device__ __forceinline__ uint32_t window_replay(uint64_t* h, const float* sd, uint32_t n, uint32_t rescore, uint32_t k, Emit emit) {
    uint32_t produced = 0, len = 0, pos = 0;
    // le(a,b) (Rust a <= b for ResortData) == key(b) <= key(a)
    auto kof = [](uint64_t e) { return (int32_t)(uint32_t)(e >> 32); };
    auto sift_up = [&](uint32_t p, uint64_t elem) {
        while (p > 0) {
            uint32_t parent = (p - 1) >> 1;
            uint64_t pe = h[parent];
            if (kof(pe) <= kof(elem)) break;  // elem <= parent
            h[p] = pe;
            p = parent;
        }
        h[p] = elem;
    };
    while (produced < k) {
        while (len < rescore && pos < n) {
            uint64_t e = ((uint64_t)(uint32_t)total_key(sd[pos]) << 32) | pos;
            uint32_t p = len++;
            sift_up(p, e);
            ++pos;
        }
        if (len == 0) break;
        uint64_t item = h[--len];
        uint64_t top = item;
        if (len > 0) {
            top = h[0];
            uint32_t end = len, p = 0, child = 1;
            uint32_t lim = end >= 2 ? end - 2 : 0;
            while (child <= lim) {
                uint64_t le = h[child], ri = h[child + 1];
                uint32_t pick = (kof(ri) <= kof(le)) ? 1u : 0u;  // data[child] <= data[child+1]
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
        emit((uint32_t)top);
        ++produced;
    }
    return produced;
}

__global__ void k_resort(uint32_t nq, uint32_t M, uint32_t rescore, uint32_t k, const uint32_t* __restrict__ stream,
                         const uint32_t* __restrict__ cnt, const float* __restrict__ dist, const uint64_t* __restrict__ tids,
                         uint64_t* __restrict__ heap_ws, uint32_t* __restrict__ out_ids, uint64_t* __restrict__ out_tids,
                         float* __restrict__ out_dist, const uint32_t* __restrict__ plain_keys) {
    uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const uint32_t n = min(cnt[q], M);
    const uint32_t* sid = stream + (size_t)q * M;
    const float* sd = dist ? dist + (size_t)q * M : nullptr;
    uint32_t produced = 0;
    if (rescore == 0) {  // resort_buffer.capacity() == 0 -> plain next()
        for (; produced < k && produced < n; ++produced) {
            uint32_t id = sid[produced];
            out_ids[(size_t)q * k + produced] = id;
            if (out_tids) out_tids[(size_t)q * k + produced] = tids[id];
            if (out_dist) {
                float d = __int_as_float(0x7fc00000);
                if (plain_keys) {  // plain storage: the graph distance IS the full-precision distance (key = total_cmp image)
                    int32_t b = (int32_t)(plain_keys[(size_t)q * M + produced] ^ 0x80000000u);
                    b ^= (int32_t)(((uint32_t)(b >> 31)) >> 1);
                    d = __int_as_float(b);
                }
                out_dist[(size_t)q * k + produced] = d;
            }
        }
    } else {
        uint32_t row = 0;
        produced = window_replay(heap_ws + (size_t)q * rescore, sd, n, rescore, k, [&](uint32_t sp) {
            uint32_t id = sid[sp];
            out_ids[(size_t)q * k + row] = id;
            if (out_tids) out_tids[(size_t)q * k + row] = tids[id];
            if (out_dist) out_dist[(size_t)q * k + row] = sd[sp];
            ++row;
        });
    }
    for (; produced < k; ++produced) {
        out_ids[(size_t)q * k + produced] = VS_INVALID_NODE;
        if (out_tids) out_tids[(size_t)q * k + produced] = 0;
        if (out_dist) out_dist[(size_t)q * k + produced] = __int_as_float(0x7fc00000);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// K2 + window in one launch (the batch path, rescore > 0): k_rerank's shape and row-distance code, but the distances of the scan's
// n <= M stream rows stay in LDS and wave 0 runs the rescore window over them after a barrier, while the other workgroups of the CU
// keep the memory system busy.  No rr_dist round trip, no heap in global memory, no second launch.
//
// The window is selected wave-parallel: pop i of the reference happens when stream positions < min(rescore + i, n) have been
// pushed, and returns an entry with the smallest key among those not popped yet.  While that smallest key is held by ONE live
// entry, every BinaryHeap layout must return that entry (a heap's pop returns a greatest element of the order, and here there is
// only one), so the set of live entries after the pop does not depend on the layout either; by induction over the pops the
// selection equals the replay as long as every pop so far found its minimum unique.  Equal keys that are not the minimum of a pop
// decide nothing at that pop — they are seen when (if) they become the minimum of a later one.  The first pop whose minimum is
// held by more than one live entry is where the layout starts to matter: the scan is then replayed serially from the start
// (window_replay on an LDS heap), which is k_resort's own sequence.  mode 2 forces the replay for every scan (A/B, tests).
// LDS: [vec_stride] f32 query | [rescore] u64 heap | [M] f32 distances | [k + 1] u32 stream positions of the rows, row count.
// ---------------------------------------------------------------------------------------------------------------
__host__ __device__ static inline size_t rerank_window_lds(uint32_t vec_stride, uint32_t M, uint32_t rescore, uint32_t k) {
    return (size_t)vec_stride * 4 + (size_t)rescore * 8 + (size_t)M * 4 + ((size_t)k + 1) * 4;
}

__global__ __launch_bounds__(256, 6) void k_rerank_window(const float* __restrict__ vecs, uint32_t vec_stride, uint32_t dim_full,
                                                       const float* __restrict__ vnorm, uint32_t distance_type,
                                                       const float* __restrict__ q_full, const uint32_t* __restrict__ stream,
                                                       const uint32_t* __restrict__ cnt, uint32_t M, uint32_t rescore, uint32_t k,
                                                       uint32_t nq, const uint64_t* __restrict__ tids, uint32_t* __restrict__ out_ids,
                                                       uint64_t* __restrict__ out_tids, float* __restrict__ out_dist, uint32_t mode,
                                                       const uint32_t* __restrict__ perm, uint32_t deal) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* qv = reinterpret_cast<float*>(smem);
    uint64_t* hh = reinterpret_cast<uint64_t*>(qv + vec_stride);  // (vec_stride is a multiple of 4 floats)
    float* sd = reinterpret_cast<float*>(hh + rescore);
    uint32_t* sps = reinterpret_cast<uint32_t*>(sd + M);
    const uint32_t slot = rerank_slot(blockIdx.x, nq, deal);
    if (slot >= nq) return;
    const uint32_t q = perm ? perm[slot] : slot;
    for (uint32_t i = threadIdx.x; i < vec_stride; i += blockDim.x) qv[i] = q_full[(size_t)q * vec_stride + i];
    const uint32_t n = min(cnt[q], M);
    const uint32_t* sid = stream + (size_t)q * M;
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
    if (wave == 0) {
        bool replay = mode == 2;
        uint32_t produced = 0;
        if (!replay) {
            uint64_t taken = 0;  // bit j: this lane's position lane + 64 j has been popped (M <= 4096)
            for (uint32_t i = 0; i < k; ++i) {
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
                if (mine) {
                    taken |= 1ull << bj;
                    sps[i] = (uint32_t)lane + 64u * bj;
                }
                ++produced;
            }
        }
        if (replay && lane == 0) {  // (from the start: rows selected before the tie are produced again)
            uint32_t row = 0;
            produced = window_replay(hh, sd, n, rescore, k, [&](uint32_t sp) { sps[row++] = sp; });
        }
        if (lane == 0) sps[k] = produced;
    }
    __syncthreads();
    if (wave == 0) {
        const uint32_t produced = sps[k];
        for (uint32_t j = (uint32_t)lane; j < k; j += WAVE) {
            uint32_t id = VS_INVALID_NODE;
            uint64_t tid = 0;
            float d = __int_as_float(0x7fc00000);
            if (j < produced) {
                const uint32_t sp = sps[j];
                id = sid[sp];
                if (out_tids) tid = tids[id];
                d = sd[sp];
            }
            out_ids[(size_t)q * k + j] = id;
            if (out_tids) out_tids[(size_t)q * k + j] = tid;
            if (out_dist) out_dist[(size_t)q * k + j] = d;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The window under a QUALIFIER (vs_search_batch_qual, vs_qual.h): siblings of k_resort and k_rerank_window, kernels of their own so
// that the ones an unqualified batch runs come out of the compiler as they were.  The window pops up to P rows instead of k; after
// each pop the popped node's bit of the scan's qualifier is read and the row is kept if it is set; the scan stops at k kept rows.
// A rejected row has been pushed, reranked and popped like any other — it is left out AFTER the pop, which is what tells a qualifier
// from a visibility mask.  Scan w of the launch is scan q = map[w] (or q_base + w) of the batch: its qualifier is tab[slots[q]]
// (slot 0: every node passes) and its rows, counts and state go to row q of the outputs.  state: VS_QUAL_COMPLETE at k kept rows;
// VS_QUAL_ENDED when the window ran dry before P pops (amgettuple returned None); after P pops without either, VS_QUAL_CUT when
// this launch is the batch's last round (final), else VS_QUAL_MORE: the host runs the scan again at more pops.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ const uint64_t* qual_bits_of(const QualLaunch& ql, uint32_t q) {
    const uint32_t slot = ql.slots ? ql.slots[q] : 0u;
    return (ql.tab && slot && slot <= VS_MAX_QUAL_SLOTS) ? ql.tab[slot] : nullptr;
}
__device__ __forceinline__ bool qual_passes(const uint64_t* bits, uint32_t id) { return !bits || ((bits[id >> 6] >> (id & 63u)) & 1ull); }
__device__ __forceinline__ uint32_t qual_state(uint32_t kept, uint32_t k, uint32_t pops, uint32_t P, uint32_t final) {
    return kept == k ? (uint32_t)VS_QUAL_COMPLETE : pops < P ? (uint32_t)VS_QUAL_ENDED : final ? (uint32_t)VS_QUAL_CUT : (uint32_t)VS_QUAL_MORE;
}

// window_replay with the keep / stop rule: emit(sp) takes every row popped and returns true when the scan has what it wants.
// Returns the number of rows popped (<= P).
template <class Emit>
__device__ __forceinline__ uint32_t window_replay_until(uint64_t* h, const float* sd, uint32_t n, uint32_t rescore, uint32_t P, Emit emit) {
    uint32_t popped = 0, len = 0, pos = 0;
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
    while (popped < P) {
        while (len < rescore && pos < n) {
            uint64_t e = ((uint64_t)(uint32_t)total_key(sd[pos]) << 32) | pos;
            uint32_t p = len++;
            sift_up(p, e);
            ++pos;
        }
        if (len == 0) break;
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
        ++popped;
        if (emit((uint32_t)top)) break;
    }
    return popped;
}

// k_resort under a qualifier: one thread per scan of the launch (the windows the fused kernel does not take, and rescore == 0, where
// the stream order is the output order and the qualifier filters it directly)
__global__ void k_resort_qual(uint32_t nq, uint32_t M, uint32_t rescore, uint32_t k, const uint32_t* __restrict__ stream,
                              const uint32_t* __restrict__ cnt, const float* __restrict__ dist, const uint64_t* __restrict__ tids,
                              uint64_t* __restrict__ heap_ws, uint32_t* __restrict__ out_ids, uint64_t* __restrict__ out_tids,
                              float* __restrict__ out_dist, const uint32_t* __restrict__ plain_keys, QualLaunch ql) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nq) return;
    const uint32_t q = ql.map ? ql.map[w] : ql.q_base + w;
    const uint64_t* bits = qual_bits_of(ql, q);
    const uint32_t P = ql.pops;
    const uint32_t n = min(cnt[w], M);
    const uint32_t* sid = stream + (size_t)w * M;
    const float* sd = dist ? dist + (size_t)w * M : nullptr;
    const size_t o = (size_t)q * k;
    uint32_t kept = 0, pops = 0;
    if (rescore == 0) {
        for (; pops < P && pops < n && kept < k; ++pops) {
            const uint32_t id = sid[pops];
            if (!qual_passes(bits, id)) continue;
            out_ids[o + kept] = id;
            if (out_tids) out_tids[o + kept] = tids[id];
            if (out_dist) out_dist[o + kept] = plain_keys ? plain_unkey(plain_keys[(size_t)w * M + pops]) : __int_as_float(0x7fc00000);
            ++kept;
        }
    } else {
        pops = window_replay_until(heap_ws + (size_t)w * rescore, sd, n, rescore, P, [&](uint32_t sp) {
            const uint32_t id = sid[sp];
            if (qual_passes(bits, id)) {
                out_ids[o + kept] = id;
                if (out_tids) out_tids[o + kept] = tids[id];
                if (out_dist) out_dist[o + kept] = sd[sp];
                ++kept;
            }
            return kept == k;
        });
    }
    for (uint32_t j = kept; j < k; ++j) {
        out_ids[o + j] = VS_INVALID_NODE;
        if (out_tids) out_tids[o + j] = 0;
        if (out_dist) out_dist[o + j] = __int_as_float(0x7fc00000);
    }
    ql.out_rows[q] = kept;
    ql.out_pops[q] = pops;
    ql.out_state[q] = qual_state(kept, k, pops, P, ql.final);
}

// k_rerank_window under a qualifier.  The rerank is k_rerank_window's; wave 0 then runs the selection for up to P pops: the popped
// position is known to every lane (its holder's lane and bit), so the node id, the qualifier bit and the count of kept rows are
// wave-uniform and sps[] still holds at most k positions — the LDS layout and size are k_rerank_window's at the same (M, rescore, k).
// A minimum held by two live entries sends the scan to the serial replay from the start, with the same keep / stop rule.
// The rows kept and the pops made are wave-uniform registers of wave 0.
__global__ __launch_bounds__(256, 6) void k_rerank_window_qual(const float* __restrict__ vecs, uint32_t vec_stride, uint32_t dim_full,
                                                            const float* __restrict__ vnorm, uint32_t distance_type,
                                                            const float* __restrict__ q_full, const uint32_t* __restrict__ stream,
                                                            const uint32_t* __restrict__ cnt, uint32_t M, uint32_t rescore, uint32_t k,
                                                            uint32_t nq, const uint64_t* __restrict__ tids, uint32_t* __restrict__ out_ids,
                                                            uint64_t* __restrict__ out_tids, float* __restrict__ out_dist, uint32_t mode,
                                                            const uint32_t* __restrict__ perm, uint32_t deal, QualLaunch ql) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* qv = reinterpret_cast<float*>(smem);
    uint64_t* hh = reinterpret_cast<uint64_t*>(qv + vec_stride);
    float* sd = reinterpret_cast<float*>(hh + rescore);
    uint32_t* sps = reinterpret_cast<uint32_t*>(sd + M);
    const uint32_t slot = rerank_slot(blockIdx.x, nq, deal);
    if (slot >= nq) return;
    const uint32_t w = perm ? perm[slot] : slot;
    for (uint32_t i = threadIdx.x; i < vec_stride; i += blockDim.x) qv[i] = q_full[(size_t)w * vec_stride + i];
    const uint32_t n = min(cnt[w], M);
    const uint32_t* sid = stream + (size_t)w * M;
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
    const uint32_t q = ql.map ? ql.map[w] : ql.q_base + w;
    const uint32_t P = ql.pops;
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
                if (qual_passes(bits, sid[sp])) {  // (wave-uniform)
                    if (lane == 0) sps[kept] = sp;
                    ++kept;
                }
            }
        }
        if (replay) {  // (from the start: rows kept before the tie are produced again)
            kept = 0;
            uint32_t kk = 0, pp = 0;
            if (lane == 0) {
                pp = window_replay_until(hh, sd, n, rescore, P, [&](uint32_t sp) {
                    if (qual_passes(bits, sid[sp])) sps[kk++] = sp;
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
// The order in which a batch's rerank workgroups take the scans (VS_RERANK_ORDER).  A batch whose scans fetch more rows than the
// corpus has (nq * M > n) reads every row several times; the repeats only hit cache when the scans that share a row run at the same
// time.  So the scans are grouped by where in the corpus they look: S seed rows (the SBQ codes of corpus rows i * (n / S), read in place
// — the key of the seed pass is a pure function of the codes as they stand, nothing is cached, nothing can go stale; the labels the same
// kernel writes per corpus row ARE kept, with the codes epoch they were built at: launch_region_labels, vs_batch.hip), key(q) = the seed whose code is
// nearest to q's code by Hamming distance (the lowest seed index among equals), perm = the scan numbers stably sorted by key.  Only
// the order of the workgroups changes: every output stays indexed by the scan's own number, and no result depends on a key.
//
// k_scan_regions is tiled like a small GEMM: a workgroup keeps the codes of REG_T scans in LDS, streams the seed codes past them in
// tiles of REG_T and each thread scores 4 x 4 (scan, seed) pairs per code word (xor + popcount: about 4 VALU operations per pair and
// word).  LDS: 2 tiles of [code_stride][REG_P] u64 (rows padded to REG_P so the transposing stores spread over the banks) + REG_T u32.
// ---------------------------------------------------------------------------------------------------------------
enum { REG_T = 64, REG_P = 66, ORD_CHUNK = 1024 };
__host__ __device__ static inline size_t scan_regions_lds(uint32_t code_stride) { return (size_t)2 * code_stride * REG_P * 8 + REG_T * 4; }

// (K: uint32_t for the keys of a batch's scans, uint16_t for the labels kept per corpus row)
template <class K>
__global__ __launch_bounds__(256) void k_scan_regions(const uint64_t* __restrict__ codes, uint32_t code_stride, uint32_t seed_step, uint32_t S,
                                                      const uint64_t* __restrict__ qcodes, uint32_t nq, K* __restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* qs = reinterpret_cast<uint64_t*>(smem);           // [code_stride][REG_P]: word w of the tile's scan i at w * REG_P + i
    uint64_t* ss = qs + (size_t)code_stride * REG_P;            // the same for the seed tile
    uint32_t* bestq = reinterpret_cast<uint32_t*>(ss + (size_t)code_stride * REG_P);
    const uint32_t tid = threadIdx.x, q0 = blockIdx.x * REG_T;
    // (a tile is loaded 8 rows at a time, 32 lanes along a row: coalesced, no division)
    for (uint32_t r = tid >> 5; r < REG_T; r += 8)
        for (uint32_t w = tid & 31u; w < code_stride; w += 32) qs[w * REG_P + r] = q0 + r < nq ? qcodes[(size_t)(q0 + r) * code_stride + w] : 0ull;
    if (tid < REG_T) bestq[tid] = 0xFFFFFFFFu;
    const uint32_t tq = (tid & 15u) * 4, ts = (tid >> 4) * 4;
    uint32_t best[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};  // (Hamming distance << 16) | seed, smallest so far
    for (uint32_t s0 = 0; s0 < S; s0 += REG_T) {
        __syncthreads();  // (the previous tile has been read; first pass: the scan tile is written)
        for (uint32_t r = tid >> 5; r < REG_T; r += 8) {
            const uint32_t s = s0 + r;
            for (uint32_t w = tid & 31u; w < code_stride; w += 32) ss[w * REG_P + r] = s < S ? codes[(size_t)s * seed_step * code_stride + w] : 0ull;
        }
        __syncthreads();
        uint32_t acc[4][4];
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) acc[a][b] = 0;
        for (uint32_t w = 0; w < code_stride; ++w) {
            const uint64_t* qp = qs + w * REG_P + tq;
            const uint64_t* sp = ss + w * REG_P + ts;
            const uint64_t qa[4] = {qp[0], qp[1], qp[2], qp[3]}, sa[4] = {sp[0], sp[1], sp[2], sp[3]};
            for (int a = 0; a < 4; ++a)
                for (int b = 0; b < 4; ++b) acc[a][b] += (uint32_t)__popcll(qa[a] ^ sa[b]);
        }
        for (int b = 0; b < 4; ++b) {
            const uint32_t s = s0 + ts + (uint32_t)b;
            if (s >= S) break;
            for (int a = 0; a < 4; ++a) best[a] = min(best[a], (acc[a][b] << 16) | s);
        }
    }
    for (int a = 0; a < 4; ++a) atomicMin(&bestq[tq + a], best[a]);
    __syncthreads();
    if (tid < REG_T && q0 + tid < nq) keys[q0 + tid] = (K)(bestq[tid] & 0xFFFFu);
}

// The key of a scan from the labels kept per corpus row: the first row of its stream lies beside the query, so that row's nearest
// seed stands for the scan's.  A scan without a row (and a row the labels do not cover) gets key S: last in the order.
__global__ __launch_bounds__(256) void k_order_label_keys(const uint16_t* __restrict__ labels, uint32_t lab_rows, uint32_t S,
                                                          const uint32_t* __restrict__ stream_ids, const uint32_t* __restrict__ cnt, uint32_t M,
                                                          uint32_t nq, uint32_t* __restrict__ keys) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    uint32_t key = S;
    if (cnt[q] > 0) {
        const uint32_t id = stream_ids[(size_t)q * M];
        if (id < lab_rows) key = min((uint32_t)labels[id], S);
    }
    keys[q] = key;
}

// perm = the scan numbers sorted by (key, scan number), a counting sort in three small launches over chunks of ORD_CHUNK scans:
// k_order_count: cnt[key][chunk] = scans of the chunk with that key; k_order_scan: every key's row of cnt becomes its exclusive prefix
// over the chunks, total[key] its sum; k_order_scatter: place = (scans with a smaller key) + (same key, earlier chunk) + (same key,
// earlier in the chunk).  No place is handed out by an atomic, so perm is the same in every run.
__global__ __launch_bounds__(256) void k_order_count(const uint32_t* __restrict__ keys, uint32_t nq, uint32_t S, uint32_t nchunks,
                                                     uint32_t* __restrict__ cnt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(smem);  // [S]
    const uint32_t c = blockIdx.x;
    for (uint32_t s = threadIdx.x; s < S; s += 256) hist[s] = 0;
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < ORD_CHUNK; e += 256) {
        const uint32_t q = c * ORD_CHUNK + e;
        if (q < nq) atomicAdd(&hist[keys[q]], 1u);
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < S; s += 256) cnt[(size_t)s * nchunks + c] = hist[s];
}

// exclusive prefix sum of x over the wave's lanes
__device__ static inline uint32_t wave_exclusive_sum(uint32_t x, int lane) {
    uint32_t incl = x;
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint32_t o = __shfl(incl, lane >= d ? lane - d : lane, WAVE);
        if (lane >= d) incl += o;
    }
    return incl - x;
}

__global__ __launch_bounds__(WAVE) void k_order_scan(uint32_t* __restrict__ cnt, uint32_t nchunks, uint32_t* __restrict__ total) {
    const int lane = threadIdx.x;
    uint32_t* row = cnt + (size_t)blockIdx.x * nchunks;
    const uint32_t per = (nchunks + WAVE - 1) / WAVE, b = min((uint32_t)lane * per, nchunks), e = min(b + per, nchunks);
    uint32_t sum = 0;
    for (uint32_t i = b; i < e; ++i) sum += row[i];
    uint32_t run = wave_exclusive_sum(sum, lane);
    for (uint32_t i = b; i < e; ++i) {
        const uint32_t v = row[i];
        row[i] = run;
        run += v;
    }
    if (lane == WAVE - 1) total[blockIdx.x] = run;  // (the last lane's run ends at the row's sum, whether or not it owns entries)
}

__global__ __launch_bounds__(256) void k_order_scatter(const uint32_t* __restrict__ keys, uint32_t nq, uint32_t S, uint32_t nchunks,
                                                       const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ total,
                                                       uint32_t* __restrict__ perm) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* kk = reinterpret_cast<uint32_t*>(smem);  // [ORD_CHUNK] the chunk's keys
    uint32_t* base = kk + ORD_CHUNK;                    // [S] first place of (key, this chunk)
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    for (uint32_t e = tid; e < ORD_CHUNK; e += 256) {
        const uint32_t q = c * ORD_CHUNK + e;
        kk[e] = q < nq ? keys[q] : 0xFFFFFFFFu;
    }
    if (tid < WAVE) {  // wave 0: exclusive prefix of total[] over the keys
        const uint32_t per = (S + WAVE - 1) / WAVE, b = min(tid * per, S), e = min(b + per, S);
        uint32_t sum = 0;
        for (uint32_t s = b; s < e; ++s) sum += total[s];
        uint32_t run = wave_exclusive_sum(sum, (int)tid);
        for (uint32_t s = b; s < e; ++s) {
            base[s] = run + cnt[(size_t)s * nchunks + c];
            run += total[s];
        }
    }
    __syncthreads();
    const uint4* kk4 = reinterpret_cast<const uint4*>(kk);
    for (uint32_t e = tid; e < ORD_CHUNK; e += 256) {
        const uint32_t q = c * ORD_CHUNK + e;
        if (q >= nq) break;
        const uint32_t key = kk[e];
        uint32_t rank = 0;  // scans of this chunk before e with the same key
        for (uint32_t i = 0; i < e / 4; ++i) {
            const uint4 v = kk4[i];
            rank += (v.x == key) + (v.y == key) + (v.z == key) + (v.w == key);
        }
        for (uint32_t i = e & ~3u; i < e; ++i) rank += kk[i] == key;
        perm[base[key] + rank] = q;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// What a batch's finish needs of the per-scan arrays (work counters [nq][ST_N], fallback marks, stream lengths, status words), summed
// on the device into RED_N u64 words: a few hundred bytes go to the host instead of nq x 44 B.  All integer: sums of u32 counters are
// exact in u64, so the doubles the host derives (mean / maximum of the inserted ids) are the ones it used to compute from the copies.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_reduce_stats(const uint32_t* __restrict__ stats, const uint32_t* __restrict__ fb,
                                                      const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ status, uint32_t nq,
                                                      uint32_t M, uint32_t rescore, uint32_t windowed, uint32_t has_visible,
                                                      uint32_t ins_limit, unsigned long long* __restrict__ red) {
    unsigned long long v[RED_N];
    for (int i = 0; i < RED_N; ++i) v[i] = 0;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += gridDim.x * blockDim.x) {
        const uint4 lo = *reinterpret_cast<const uint4*>(stats + (size_t)q * ST_N);
        const uint4 hi = *reinterpret_cast<const uint4*>(stats + (size_t)q * ST_N + 4);
        static_assert(ST_N == 8 && ST_VISITS == 0 && ST_CAND == 1 && ST_DQ == 2 && ST_READS == 3 && ST_NEXT == 4 && ST_INVIS == 6 && ST_INS == 7,
                      "k_reduce_stats reads a scan's counters as two uint4");
        const uint32_t visits = lo.x, cand = lo.y, dq = lo.z, reads = lo.w, next = hi.x, invis = hi.z, ins = hi.w;
        const uint32_t f = fb ? fb[q] : 0u, cq = cnt[q];
        v[RED_STATUS] |= status[q];
        v[RED_VISITS] += visits;
        v[RED_CAND] += cand;
        v[RED_DQ] += dq;
        v[RED_READS] += reads;
        unsigned long long next_calls = next;
        if (windowed && cq < M && next > 0) {
            // an exhausted stream under next_with_resort: see collect_stats
            const long long C = cq, S = rescore, kk = (long long)M - rescore + 1;
            const long long J = kk < C + 1 ? kk : C + 1, j0 = C - S + 2 > 1 ? C - S + 2 : 1;
            const long long extra = J - j0 + 1 > 1 ? J - j0 + 1 : 1;
            next_calls = next_calls - 1 + (unsigned long long)extra;
        }
        v[RED_NEXT] += next_calls;
        if (f) {
            v[RED_FB_SCANS] += 1;
            v[RED_FB_VISITS] += visits;
            v[RED_FB_DQ] += dq;
            v[RED_INS_OV] += 1;
        } else {
            v[RED_INS_SUM] += ins;
            v[RED_INS_FAST] += 1;
            v[RED_INS_OV] += ins > ins_limit ? 1u : 0u;
        }
        v[RED_INS_MAX] = v[RED_INS_MAX] > ins ? v[RED_INS_MAX] : ins;
        if (windowed) v[RED_HEAP_ROWS] += min(cq, M) + (has_visible ? invis : 0u);
    }
    for (int i = 0; i < RED_N; ++i) {
        unsigned long long x = v[i];
        for (int m = 1; m < WAVE; m <<= 1) {
            const unsigned long long o = __shfl_xor(x, m, WAVE);
            x = i == RED_STATUS ? (x | o) : i == RED_INS_MAX ? (x > o ? x : o) : x + o;
        }
        if ((threadIdx.x & 63) == 0 && x) {
            if (i == RED_STATUS) atomicOr(&red[i], x);
            else if (i == RED_INS_MAX) atomicMax(&red[i], x);
            else atomicAdd(&red[i], x);
        }
    }
}

// The same window, resumable (the amgettuple cursor): the BinaryHeap<ResortData> of ONE scan lives in heap_ws between calls,
// cur[0] = its length, cur[1] = stream rows pushed so far, cur[2] = rows handed out so far.  `stream` / `dist` / `keys` hold every
// row the scan has emitted so far (n of them; `exhausted` = there will be no more).  Produces up to k more rows; a window that
// cannot be refilled because the rows are not there yet (n too small, scan not exhausted) stops early — the host fetches so
// that this never happens (rows >= rescore + handed out + k - 1).  cur[3] = rows produced by this call.
__global__ void k_resort_cursor(uint32_t n, uint32_t exhausted, uint32_t rescore, uint32_t k, const uint32_t* __restrict__ stream,
                                const float* __restrict__ dist, const uint32_t* __restrict__ keys, uint32_t plain_keys,
                                const uint64_t* __restrict__ tids, uint64_t* __restrict__ h, uint32_t* __restrict__ cur,
                                uint32_t* __restrict__ out_ids, uint64_t* __restrict__ out_tids, float* __restrict__ out_dist) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t len = cur[0], pos = cur[1];
    uint32_t produced = 0;
    if (rescore == 0) {  // resort_buffer.capacity() == 0 -> plain next()
        for (; produced < k && pos < n; ++produced, ++pos) {
            const uint32_t id = stream[pos];
            out_ids[produced] = id;
            out_tids[produced] = tids[id];
            float d = __int_as_float(0x7fc00000);
            if (plain_keys) {
                int32_t b = (int32_t)(keys[pos] ^ 0x80000000u);
                b ^= (int32_t)(((uint32_t)(b >> 31)) >> 1);
                d = __int_as_float(b);
            }
            out_dist[produced] = d;
        }
    } else {
        auto kof = [](uint64_t e) { return (int32_t)(uint32_t)(e >> 32); };
        auto sift_up = [&](uint32_t p, uint64_t elem) {
            while (p > 0) {
                const uint32_t parent = (p - 1) >> 1;
                const uint64_t pe = h[parent];
                if (kof(pe) <= kof(elem)) break;
                h[p] = pe;
                p = parent;
            }
            h[p] = elem;
        };
        while (produced < k) {
            while (len < rescore && pos < n) {
                const uint64_t e = ((uint64_t)(uint32_t)total_key(dist[pos]) << 32) | pos;
                sift_up(len++, e);
                ++pos;
            }
            if (len < rescore && !exhausted) break;  // the window cannot be filled yet
            if (len == 0) break;
            const uint64_t item = h[--len];
            uint64_t top = item;
            if (len > 0) {
                top = h[0];
                const uint32_t end = len;
                uint32_t p = 0, child = 1;
                const uint32_t lim = end >= 2 ? end - 2 : 0;
                while (child <= lim) {
                    const uint64_t le = h[child], ri = h[child + 1];
                    const uint32_t pick = (kof(ri) <= kof(le)) ? 1u : 0u;
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
            const uint32_t sp = (uint32_t)top;
            const uint32_t id = stream[sp];
            out_ids[produced] = id;
            out_tids[produced] = tids[id];
            out_dist[produced] = dist[sp];
            ++produced;
        }
    }
    cur[0] = len;
    cur[1] = pos;
    cur[2] += produced;
    cur[3] = produced;
}

// The resumable window for MANY scans in one launch (the scan pools' fetch, vs_scanpool.cpp): one wave per listed scan, scans side by
// side on the chip instead of one single-thread launch per scan.  list[3 b ..] = (pool slot, stream rows the scan has emitted so
// far, exhausted); the arrays of slot q are row q of the pool's 2-D arrays (strides below).  Inside a scan the heap mechanics are
// serial — Rust's BinaryHeap<ResortData>, AM/scan.rs:111-117,244-305, replayed exactly as in k_resort_cursor — but they run on an LDS
// copy of the heap (one coalesced load, one store) against keys the wave fetched ahead (total_cmp images of the distances the
// refills will push), and the k result rows are gathered by k lanes at once afterwards (stream id, heap tid, distance: two
// dependent round trips in all instead of three per row).  cur[] as in k_resort_cursor.
__global__ __launch_bounds__(WAVE) void k_resort_cursor_batch(const uint32_t* __restrict__ list, uint32_t rescore, uint32_t k,
                                                               const uint32_t* __restrict__ stream_base, const float* __restrict__ dist_base,
                                                               const uint32_t* __restrict__ keys_base, uint32_t row_stride, uint32_t plain_keys,
                                                               const uint64_t* __restrict__ tids, uint64_t* __restrict__ heap_base,
                                                               uint32_t* __restrict__ cur_base, uint32_t* __restrict__ out_ids_base,
                                                               uint64_t* __restrict__ out_tids_base, float* __restrict__ out_dist_base,
                                                               uint32_t out_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* hh = reinterpret_cast<uint64_t*>(smem);                 // rescore entries
    uint32_t* kk = reinterpret_cast<uint32_t*>(hh + rescore);        // rescore + k keys of the rows the refills will push
    uint32_t* sps = kk + rescore + k;                                // k stream positions of the rows produced
    const uint32_t lane = threadIdx.x;
    const uint32_t q = list[3 * blockIdx.x], n = list[3 * blockIdx.x + 1], exhausted = list[3 * blockIdx.x + 2];
    const uint32_t* stream = stream_base + (size_t)q * row_stride;
    const float* dist = dist_base + (size_t)q * row_stride;
    const uint32_t* keys = keys_base + (size_t)q * row_stride;
    uint64_t* h = heap_base + (size_t)q * rescore;
    uint32_t* cur = cur_base + (size_t)q * 4;
    uint32_t* out_ids = out_ids_base + (size_t)q * out_stride;
    uint64_t* out_tids = out_tids_base + (size_t)q * out_stride;
    float* out_dist = out_dist_base + (size_t)q * out_stride;
    uint32_t len = cur[0], pos = cur[1];
    uint32_t produced = 0;
    if (rescore == 0) {  // resort_buffer.capacity() == 0 -> plain next(): rows pos .. pos + k - 1 as they are
        produced = min(k, n > pos ? n - pos : 0u);
        for (uint32_t j = lane; j < produced; j += WAVE) sps[j] = pos + j;
        pos += produced;
    } else {
        const uint32_t pos0 = pos;
        const uint32_t ahead = min(n > pos ? n - pos : 0u, rescore - len + k);  // (a call pushes at most that many rows)
        for (uint32_t i = lane; i < len; i += WAVE) hh[i] = h[i];
        for (uint32_t i = lane; i < ahead; i += WAVE) kk[i] = (uint32_t)total_key(dist[pos0 + i]);
        __syncthreads();
        if (lane == 0) {
            auto kof = [](uint64_t e) { return (int32_t)(uint32_t)(e >> 32); };
            auto sift_up = [&](uint32_t p, uint64_t elem) {
                while (p > 0) {
                    const uint32_t parent = (p - 1) >> 1;
                    const uint64_t pe = hh[parent];
                    if (kof(pe) <= kof(elem)) break;
                    hh[p] = pe;
                    p = parent;
                }
                hh[p] = elem;
            };
            while (produced < k) {
                while (len < rescore && pos < n) {
                    const uint64_t e = ((uint64_t)kk[pos - pos0] << 32) | pos;
                    sift_up(len++, e);
                    ++pos;
                }
                if (len < rescore && !exhausted) break;  // the window cannot be filled yet
                if (len == 0) break;
                const uint64_t item = hh[--len];
                uint64_t top = item;
                if (len > 0) {
                    top = hh[0];
                    const uint32_t end = len;
                    uint32_t p = 0, child = 1;
                    const uint32_t lim = end >= 2 ? end - 2 : 0;
                    while (child <= lim) {
                        const uint64_t le = hh[child], ri = hh[child + 1];
                        const uint32_t pick = (kof(ri) <= kof(le)) ? 1u : 0u;
                        child += pick;
                        hh[p] = pick ? ri : le;
                        p = child;
                        child = 2 * p + 1;
                    }
                    if (child == end - 1) {
                        hh[p] = hh[child];
                        p = child;
                    }
                    sift_up(p, item);
                }
                sps[produced++] = (uint32_t)top;
            }
            sps[k] = produced;  // (one word past the k positions: the hand-over to the other lanes)
            sps[k + 1] = len;
            sps[k + 2] = pos;
        }
        __syncthreads();
        produced = sps[k];
        len = sps[k + 1];
        pos = sps[k + 2];
        for (uint32_t i = lane; i < len; i += WAVE) h[i] = hh[i];
    }
    __syncthreads();
    for (uint32_t j = lane; j < produced; j += WAVE) {
        const uint32_t sp = sps[j];
        const uint32_t id = stream[sp];
        out_ids[j] = id;
        out_tids[j] = tids[id];
        float d = __int_as_float(0x7fc00000);
        if (rescore != 0) d = dist[sp];
        else if (plain_keys) {
            int32_t b = (int32_t)(keys[sp] ^ 0x80000000u);
            b ^= (int32_t)(((uint32_t)(b >> 31)) >> 1);
            d = __int_as_float(b);
        }
        out_dist[j] = d;
    }
    if (lane == 0) {
        cur[0] = len;
        cur[1] = pos;
        cur[2] += produced;
        cur[3] = produced;
    }
}

// The resumable window under a QUALIFIER (vs_scanpool_fetch_qual, vs_scanpool.cpp): k_resort_cursor_batch that pops PAST rows whose node
// does not carry the bit of the qualifier its scan names, and keeps the rows that do.  A kernel of its own, so that the unqualified one
// comes out of the compiler as it did.  list[6 b ..] = (pool slot, stream rows emitted so far, exhausted, qualifier slot, the pops of
// this FETCH the scan may be taken to by this launch, 1 = first launch of the fetch); rec[4 q ..] = (rows kept, pops, state) of the
// fetch in progress, carried from launch to launch; `chunk` = the pops ONE launch may make (it sizes the key slots in LDS).
//
// The heap is replayed by lane 0 on its LDS copy exactly as above — a rejected row has held its place in the window like any other —
// but whether the loop goes on depends on the popped node's bit, and two dependent global round trips per pop (stream id, qualifier
// word) on the serial path would cost more than the heap does.  So the wave resolves the bit of every row this launch can pop BEFORE the
// loop, in parallel: the `len` rows in the heap and the `ahead` rows the refills will push, a lane per row, stream id then qualifier
// word (two round trips for the whole wave), into an LDS bitmap indexed by STREAM POSITION (rows_cap bits; set with LDS atomicOr, so the
// order of the lanes does not show).  The loop reads LDS only.  Qualifier slot 0 skips the test.
//
// A launch stops when the rows kept reach k (VS_QUAL_COMPLETE), when a pop finds the heap empty and the stream at its end
// (VS_QUAL_ENDED), when the pops reach list[..+4] (VS_PQ_LIMIT: the host decides between CUT, the row budget and a longer stream), or
// when the window cannot be refilled yet or `chunk` pops are made (VS_PQ_STARVED: the host launches again).  The kept rows are gathered
// lane-parallel behind those of the fetch's earlier launches.  cur[] as above, except that cur[2] advances by the POPS (each is an
// amgettuple call that returned a row) and cur[3] = rows kept by this launch.
__global__ __launch_bounds__(WAVE) void k_resort_cursor_batch_qual(const uint32_t* __restrict__ list, uint32_t rescore, uint32_t k, uint32_t chunk,
                                                                    uint32_t bm_words, const uint64_t* const* __restrict__ qtab,
                                                                    const uint32_t* __restrict__ stream_base, const float* __restrict__ dist_base,
                                                                    const uint32_t* __restrict__ keys_base, uint32_t row_stride, uint32_t plain_keys,
                                                                    const uint64_t* __restrict__ tids, uint64_t* __restrict__ heap_base,
                                                                    uint32_t* __restrict__ cur_base, uint32_t* __restrict__ rec_base,
                                                                    uint32_t* __restrict__ out_ids_base, uint64_t* __restrict__ out_tids_base,
                                                                    float* __restrict__ out_dist_base, uint32_t out_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* hh = reinterpret_cast<uint64_t*>(smem);            // rescore entries
    uint32_t* kk = reinterpret_cast<uint32_t*>(hh + rescore);    // rescore + chunk keys of the rows the refills will push
    uint32_t* bm = kk + rescore + chunk;                         // bm_words: bit p = the node of stream row p passes
    uint32_t* sps = bm + bm_words;                               // k stream positions of the rows kept, then the hand-over words
    const uint32_t lane = threadIdx.x;
    const uint32_t* const le = list + 6 * (size_t)blockIdx.x;
    const uint32_t q = le[0], n = le[1], exhausted = le[2], qslot = le[3], target = le[4], fresh = le[5];
    const uint32_t* stream = stream_base + (size_t)q * row_stride;
    const float* dist = dist_base + (size_t)q * row_stride;
    const uint32_t* keys = keys_base + (size_t)q * row_stride;
    uint64_t* h = heap_base + (size_t)q * rescore;
    uint32_t* cur = cur_base + (size_t)q * 4;
    uint32_t* rec = rec_base + (size_t)q * 4;
    const uint64_t* const qbits = (qslot != 0 && qtab != nullptr) ? qtab[qslot] : nullptr;
    const uint32_t kept0 = fresh ? 0u : rec[0], pops0 = fresh ? 0u : rec[1];
    const uint32_t allow = min(chunk, target > pops0 ? target - pops0 : 0u);  // pops this launch may make
    uint32_t len = cur[0], pos = cur[1];
    const uint32_t pos0 = pos;
    // rows this launch can push (window) or pop (no window): at most that many
    const uint32_t ahead = min(n > pos ? n - pos : 0u, rescore != 0 ? rescore - len + allow : allow);
    if (rescore != 0) {
        for (uint32_t i = lane; i < len; i += WAVE) hh[i] = h[i];
        for (uint32_t i = lane; i < ahead; i += WAVE) kk[i] = (uint32_t)total_key(dist[pos0 + i]);
    } else {
        len = 0;
    }
    if (qbits) {
        for (uint32_t i = lane; i < bm_words; i += WAVE) bm[i] = 0;
        __syncthreads();
        for (uint32_t i = lane; i < len + ahead; i += WAVE) {
            const uint32_t sp = i < len ? (uint32_t)hh[i] : pos0 + (i - len);
            const uint32_t id = stream[sp];
            if ((qbits[id >> 6] >> (id & 63u)) & 1ull) atomicOr(&bm[sp >> 5], 1u << (sp & 31u));
        }
    }
    __syncthreads();
    if (lane == 0) {
        uint32_t kept = 0, pops = 0, state = VS_PQ_STARVED;
        auto passes = [&](uint32_t sp) { return qbits == nullptr || ((bm[sp >> 5] >> (sp & 31u)) & 1u) != 0; };
        auto kof = [](uint64_t e) { return (int32_t)(uint32_t)(e >> 32); };
        auto sift_up = [&](uint32_t p, uint64_t elem) {
            while (p > 0) {
                const uint32_t parent = (p - 1) >> 1;
                const uint64_t pe = hh[parent];
                if (kof(pe) <= kof(elem)) break;
                hh[p] = pe;
                p = parent;
            }
            hh[p] = elem;
        };
        for (;;) {
            if (kept0 + kept >= k) {
                state = VS_QUAL_COMPLETE;
                break;
            }
            if (pops >= allow) {
                state = pops0 + pops >= target ? (uint32_t)VS_PQ_LIMIT : (uint32_t)VS_PQ_STARVED;
                break;
            }
            uint32_t sp;
            if (rescore == 0) {  // resort_buffer.capacity() == 0 -> plain next(): the rows as they are
                if (pos >= n) {
                    state = exhausted ? (uint32_t)VS_QUAL_ENDED : (uint32_t)VS_PQ_STARVED;
                    break;
                }
                sp = pos++;
            } else {
                while (len < rescore && pos < n) {
                    const uint64_t e = ((uint64_t)kk[pos - pos0] << 32) | pos;
                    sift_up(len++, e);
                    ++pos;
                }
                if (len < rescore && !exhausted) break;  // the window cannot be filled yet
                if (len == 0) {
                    state = VS_QUAL_ENDED;
                    break;
                }
                const uint64_t item = hh[--len];
                uint64_t top = item;
                if (len > 0) {
                    top = hh[0];
                    const uint32_t end = len;
                    uint32_t p = 0, child = 1;
                    const uint32_t lim = end >= 2 ? end - 2 : 0;
                    while (child <= lim) {
                        const uint64_t lc = hh[child], ri = hh[child + 1];
                        const uint32_t pick = (kof(ri) <= kof(lc)) ? 1u : 0u;
                        child += pick;
                        hh[p] = pick ? ri : lc;
                        p = child;
                        child = 2 * p + 1;
                    }
                    if (child == end - 1) {
                        hh[p] = hh[child];
                        p = child;
                    }
                    sift_up(p, item);
                }
                sp = (uint32_t)top;
            }
            ++pops;
            if (passes(sp)) sps[kept++] = sp;
        }
        sps[k] = kept;  // (past the k positions: the hand-over to the other lanes)
        sps[k + 1] = len;
        sps[k + 2] = pos;
        sps[k + 3] = pops;
        sps[k + 4] = state;
    }
    __syncthreads();
    const uint32_t kept = sps[k], pops = sps[k + 3];
    len = sps[k + 1];
    pos = sps[k + 2];
    for (uint32_t i = lane; i < len; i += WAVE) h[i] = hh[i];
    uint32_t* out_ids = out_ids_base + (size_t)q * out_stride + kept0;
    uint64_t* out_tids = out_tids_base + (size_t)q * out_stride + kept0;
    float* out_dist = out_dist_base + (size_t)q * out_stride + kept0;
    for (uint32_t j = lane; j < kept; j += WAVE) {
        const uint32_t sp = sps[j];
        const uint32_t id = stream[sp];
        out_ids[j] = id;
        out_tids[j] = tids[id];
        float d = __int_as_float(0x7fc00000);
        if (rescore != 0) d = dist[sp];
        else if (plain_keys) {
            int32_t b = (int32_t)(keys[sp] ^ 0x80000000u);
            b ^= (int32_t)(((uint32_t)(b >> 31)) >> 1);
            d = __int_as_float(b);
        }
        out_dist[j] = d;
    }
    if (lane == 0) {
        cur[0] = len;
        cur[1] = pos;
        cur[2] += pops;
        cur[3] = kept;
        rec[0] = kept0 + kept;
        rec[1] = pops0 + pops;
        rec[2] = sps[k + 4];
    }
}

// ===============================================================================================================
// launch wrappers
// ===============================================================================================================
static float count_as_f32(uint64_t c) { return (float)c; }

int launch_prepare_queries(vs_index* idx, const float* d_raw, uint32_t nq, float* d_q_full, uint64_t* d_qcodes) {
    if (nq == 0) return VS_OK;
    const vs_index_desc& d = idx->d;
    const uint32_t words = d.storage_type == VS_STORAGE_PLAIN ? 0u : d.words;  // plain: no SBQ code
    const bool same = d.dim_full == d.dim_index, multi = words && d.bits != 1;
    const uint32_t rf = round_up_u32(d.dim_full, 4), ri = round_up_u32(d.dim_index, 4);
    const size_t shared = ((words ? ri : 0u) + (multi ? ri : 0u)) * sizeof(float);
    const size_t per_wave = ((size_t)rf + (same ? 0u : ri) + (multi ? ri : 0u) + 4u) * sizeof(float);
    // four queries in flight per workgroup while their slices fit the 64 KB a launch gets without opting in
    uint32_t nw = nq >= 4 ? 4 : nq >= 2 ? 2 : 1;
    while (nw > 1 && shared + nw * per_wave > 64 * 1024) nw >>= 1;
    const size_t lds = shared + nw * per_wave;
    VS_REQUIRE(lds <= 160 * 1024, "query too large for LDS staging (%u dims)", d.dim_full);
    if (lds > 64 * 1024) {  // (one very wide query per workgroup: beyond what a launch gets without opting in)
        static DeviceOnce attr_set;
        if (attr_set.pending(idx->ctx->device)) {
            VS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_prepare_queries), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            attr_set.done(idx->ctx->device);
        }
    }
    // rounds: the per-workgroup staging is shared by nw x rounds queries, the grid still covers the device several times over
    const uint32_t rounds = nq >= 65536 ? 4 : nq >= 8192 ? 2 : 1;
    const uint32_t grid = (nq + nw * rounds - 1) / (nw * rounds);
    const uint32_t vec4 = (d.dim_full % 4 == 0 && ((uintptr_t)d_raw & 15) == 0) ? 1u : 0u;
    hipLaunchKernelGGL(k_prepare_queries, dim3(grid), dim3(nw * WAVE), lds, idx->ctx->stream, d_raw, nq, d.dim_full,
                       d.dim_index, idx->vec_stride, d.distance_type, d.bits, idx->mean, idx->m2,
                       count_as_f32(idx->count), words, idx->code_stride, rounds, vec4, d_q_full, d_qcodes);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int launch_prepare_index_slice(vs_index* idx, const float* d_raw, uint32_t nq, float* d_q_index, uint32_t raw_stride) {
    if (nq == 0) return VS_OK;
    const vs_index_desc& d = idx->d;
    const size_t lds = (round_up_u32(d.dim_index, 4) + 4) * sizeof(float);
    VS_REQUIRE(lds <= 64 * 1024, "index slice too large for LDS staging (%u dims)", d.dim_index);
    // (the kernel only strides by its dim_full argument)
    hipLaunchKernelGGL(k_prepare_index_slice, dim3(nq), dim3(WAVE), lds, idx->ctx->stream, d_raw, nq, raw_stride ? raw_stride : d.dim_full, d.dim_index,
                       idx->vec_stride, d.distance_type, d_q_index);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int launch_quantize_rows(vs_index* idx, const float* d_rows, uint32_t row_stride, uint32_t nrows, uint64_t* d_codes,
                         uint32_t code_stride) {
    if (nrows == 0) return VS_OK;
    const vs_index_desc& d = idx->d;
    uint32_t grid = nrows < 65536u * 16 ? nrows : 65536u * 16;
    hipLaunchKernelGGL(k_quantize_rows, dim3(grid), dim3(WAVE), 0, idx->ctx->stream, d_rows, row_stride, nrows,
                       d.dim_index, d.bits, idx->mean, idx->m2, count_as_f32(idx->count), d.words, code_stride, d_codes);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int launch_hamming_gather(vs_index* idx, const uint64_t* d_qcodes, const uint32_t* d_ids, const uint32_t* d_off,
                          uint32_t nq, uint32_t* d_out) {
    if (nq == 0) return VS_OK;
    size_t lds = (size_t)idx->code_stride * 8;
    hipLaunchKernelGGL(k_hamming_gather, dim3(nq), dim3(WAVE), lds, idx->ctx->stream, idx->codes, idx->code_stride,
                       d_qcodes, d_ids, d_off, nq, d_out);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int launch_rerank(vs_index* idx, const float* d_q_full, const uint32_t* d_ids, const uint32_t* d_off,
                  const uint32_t* d_cnt, uint32_t fixed_m, uint32_t nq, float* d_out, uint32_t row_base, const uint32_t* d_perm,
                  bool deal) {
    if (nq == 0) return VS_OK;
    VS_REQUIRE(idx->vecs != nullptr, "index has no vector column: rerank impossible");
    size_t lds = (size_t)idx->vec_stride * 4;
    hipLaunchKernelGGL(k_rerank, dim3(rerank_grid(nq, deal)), dim3(256), lds, idx->ctx->stream, idx->vecs, idx->vec_stride,
                       idx->d.dim_full, idx->vnorm, idx->d.distance_type, d_q_full, d_ids, d_off, d_cnt, fixed_m, nq,
                       d_out, row_base, d_perm, deal ? 1u : 0u);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int launch_resort(vs_index* idx, uint32_t nq, uint32_t M, uint32_t rescore, uint32_t k, const uint32_t* d_stream_ids,
                  const uint32_t* d_cnt, const float* d_dist, uint64_t* d_heap_ws, uint32_t* d_out_ids,
                  uint64_t* d_out_tids, float* d_out_dist) {
    if (nq == 0) return VS_OK;
    // plain storage without truncation: the graph distance IS the full-precision distance (no resort, AM/scan.rs:392-399)
    const uint32_t* plain_keys = (idx->d.storage_type == VS_STORAGE_PLAIN && idx->d.dim_index == idx->d.dim_full)
                                     ? (const uint32_t*)idx->ws.stream_ham.p : nullptr;
    hipLaunchKernelGGL(k_resort, dim3((nq + 63) / 64), dim3(64), 0, idx->ctx->stream, nq, M, rescore, k, d_stream_ids,
                       d_cnt, d_dist, idx->tids, d_heap_ws, d_out_ids, d_out_tids, d_out_dist, plain_keys);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// The fused kernel keeps one query, one window heap and M distances in LDS.  Registers, not waves, limit both kernels: k_rerank takes
// 80 VGPRs = 6 waves per SIMD = 6 workgroups of 256 threads per CU, and k_rerank_window is held to the same 80 (launch bounds: 6 waves
// per SIMD; no scratch — left alone the compiler takes 92 and one workgroup fewer).  Six workgroups share the CU's 160 KB of LDS while
// each stays under 160 / 6 = 26.6 KB; the fused kernel is taken up to 24 KB (room for the allocation granule): 12 M + 3 KB at 768
// dimensions, M <= ~1 790 — every rescore the GUC allows (<= 1000) with k up to several hundred.  Beyond that (and past 4096
// rows, the width of the per-lane pop masks) the pair runs.
bool rerank_window_fits(const vs_index* idx, uint32_t M, uint32_t rescore, uint32_t k) {
    return M <= 4096 && rerank_window_lds(idx->vec_stride, M, rescore, k) <= 24 * 1024;
}

int launch_rerank_window(vs_index* idx, const float* d_q_full, const uint32_t* d_stream_ids, const uint32_t* d_cnt, uint32_t M,
                         uint32_t rescore, uint32_t k, uint32_t nq, uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist,
                         uint32_t mode, const uint32_t* d_perm, bool deal) {
    if (nq == 0) return VS_OK;
    VS_REQUIRE(idx->vecs != nullptr, "index has no vector column: rerank impossible");
    VS_REQUIRE(rescore > 0 && rerank_window_fits(idx, M, rescore, k), "fused rerank: window of %u rows does not fit", M);
    const size_t lds = rerank_window_lds(idx->vec_stride, M, rescore, k);
    hipLaunchKernelGGL(k_rerank_window, dim3(rerank_grid(nq, deal)), dim3(256), lds, idx->ctx->stream, idx->vecs, idx->vec_stride,
                       idx->d.dim_full, idx->vnorm, idx->d.distance_type, d_q_full, d_stream_ids, d_cnt, M, rescore, k, nq, idx->tids,
                       d_out_ids, d_out_tids, d_out_dist, mode, d_perm, deal ? 1u : 0u);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// the same two launches under a qualifier (ql.pops > 0): d_out_* are the BATCH's rows, indexed by the batch's scan numbers
int launch_resort_qual(vs_index* idx, uint32_t nq, uint32_t M, uint32_t rescore, uint32_t k, const uint32_t* d_stream_ids, const uint32_t* d_cnt,
                       const float* d_dist, uint64_t* d_heap_ws, uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, const QualLaunch& ql) {
    if (nq == 0) return VS_OK;
    const uint32_t* plain_keys = (idx->d.storage_type == VS_STORAGE_PLAIN && idx->d.dim_index == idx->d.dim_full)
                                     ? (const uint32_t*)idx->ws.stream_ham.p : nullptr;
    hipLaunchKernelGGL(k_resort_qual, dim3((nq + 63) / 64), dim3(64), 0, idx->ctx->stream, nq, M, rescore, k, d_stream_ids, d_cnt, d_dist,
                       idx->tids, d_heap_ws, d_out_ids, d_out_tids, d_out_dist, plain_keys, ql);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int launch_rerank_window_qual(vs_index* idx, const float* d_q_full, const uint32_t* d_stream_ids, const uint32_t* d_cnt, uint32_t M,
                              uint32_t rescore, uint32_t k, uint32_t nq, uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist,
                              uint32_t mode, const uint32_t* d_perm, bool deal, const QualLaunch& ql) {
    if (nq == 0) return VS_OK;
    VS_REQUIRE(idx->vecs != nullptr, "index has no vector column: rerank impossible");
    VS_REQUIRE(rescore > 0 && rerank_window_fits(idx, M, rescore, k), "fused rerank: window of %u rows does not fit", M);
    const size_t lds = rerank_window_lds(idx->vec_stride, M, rescore, k);
    hipLaunchKernelGGL(k_rerank_window_qual, dim3(rerank_grid(nq, deal)), dim3(256), lds, idx->ctx->stream, idx->vecs, idx->vec_stride,
                       idx->d.dim_full, idx->vnorm, idx->d.distance_type, d_q_full, d_stream_ids, d_cnt, M, rescore, k, nq, idx->tids,
                       d_out_ids, d_out_tids, d_out_dist, mode, d_perm, deal ? 1u : 0u, ql);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// The rerank order of a batch (k_scan_regions + the counting sort): d_perm[nq] = the scan numbers by (nearest of S seed rows, scan
// number).  d_work: scan_order_work_bytes(nq, S) bytes.  S <= min(n, 4096) (a key and a Hamming distance share a 32-bit word).
bool scan_order_fits(const vs_index* idx) { return idx->codes != nullptr && idx->d.n > 0 && scan_regions_lds(idx->code_stride) <= 40 * 1024; }
size_t scan_order_work_bytes(uint32_t nq, uint32_t S) {
    const size_t nchunks = (nq + ORD_CHUNK - 1) / ORD_CHUNK;
    return ((size_t)nq + S + (size_t)S * nchunks) * 4;
}
// counting sort of nq scans by (key < NK, scan number): d_work = keys[nq], then the sort's tables
static void launch_order_sort(hipStream_t st, uint32_t* d_work, uint32_t nq, uint32_t NK, uint32_t* d_perm) {
    const uint32_t nchunks = (nq + ORD_CHUNK - 1) / ORD_CHUNK;
    uint32_t *d_keys = d_work, *d_total = d_keys + nq, *d_cnt = d_total + NK;
    hipLaunchKernelGGL(k_order_count, dim3(nchunks), dim3(256), (size_t)NK * 4, st, d_keys, nq, NK, nchunks, d_cnt);
    hipLaunchKernelGGL(k_order_scan, dim3(NK), dim3(WAVE), 0, st, d_cnt, nchunks, d_total);
    hipLaunchKernelGGL(k_order_scatter, dim3(nchunks), dim3(256), (size_t)(ORD_CHUNK + NK) * 4, st, d_keys, nq, NK, nchunks, d_cnt, d_total,
                       d_perm);
}
int launch_scan_order(vs_index* idx, const uint64_t* d_qcodes, uint32_t nq, uint32_t S, uint32_t* d_work, uint32_t* d_perm) {
    if (nq == 0) return VS_OK;
    VS_REQUIRE(scan_order_fits(idx) && S >= 1 && S <= 4096 && S <= idx->d.n, "rerank order: %u seeds of %u-word codes not supported", S,
               idx->code_stride);
    hipStream_t st = idx->ctx->stream;
    hipLaunchKernelGGL(k_scan_regions<uint32_t>, dim3((nq + REG_T - 1) / REG_T), dim3(256), scan_regions_lds(idx->code_stride), st, idx->codes,
                       idx->code_stride, idx->d.n / S, S, d_qcodes, nq, d_work);
    launch_order_sort(st, d_work, nq, S, d_perm);
    VS_HIP(hipGetLastError());
    return VS_OK;
}
// (in chunks of 2^20 rows: a launch of about the length of a search step's other kernels, whatever the corpus)
int launch_region_labels(vs_index* idx, uint32_t S, uint32_t seed_step, uint32_t row_begin, uint32_t rows, uint16_t* d_labels) {
    VS_REQUIRE(scan_order_fits(idx) && S >= 1 && S <= 4096 && seed_step >= 1 && (uint64_t)(S - 1) * seed_step < idx->d.n &&
                   (uint64_t)row_begin + rows <= idx->d.n,
               "region labels: %u seeds %u rows apart, rows %u + %u of %u not supported", S, seed_step, row_begin, rows, idx->d.n);
    hipStream_t st = idx->ctx->stream;
    for (uint32_t r0 = row_begin, end = row_begin + rows; r0 < end;) {
        const uint32_t nr = std::min<uint32_t>(end - r0, 1u << 20);
        hipLaunchKernelGGL(k_scan_regions<uint16_t>, dim3((nr + REG_T - 1) / REG_T), dim3(256), scan_regions_lds(idx->code_stride), st,
                           idx->codes, idx->code_stride, seed_step, S, idx->codes + (size_t)r0 * idx->code_stride, nr, d_labels + r0);
        r0 += nr;
    }
    VS_HIP(hipGetLastError());
    return VS_OK;
}
int launch_label_order(vs_index* idx, const uint16_t* d_labels, uint32_t lab_rows, uint32_t S, const uint32_t* d_stream_ids,
                       const uint32_t* d_cnt, uint32_t M, uint32_t nq, uint32_t* d_work, uint32_t* d_perm) {
    if (nq == 0) return VS_OK;
    VS_REQUIRE(d_labels && S >= 1 && S <= 4096 && M >= 1, "rerank order: no labels of %u seeds", S);
    hipStream_t st = idx->ctx->stream;
    hipLaunchKernelGGL(k_order_label_keys, dim3((nq + 255) / 256), dim3(256), 0, st, d_labels, lab_rows, S, d_stream_ids, d_cnt, M, nq, d_work);
    launch_order_sort(st, d_work, nq, S + 1, d_perm);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// d_red: RED_N u64 words, zeroed by the caller on the same stream
int launch_reduce_stats(vs_index* idx, const uint32_t* d_stats, const uint32_t* d_fb, const uint32_t* d_cnt, const uint32_t* d_status,
                        uint32_t nq, uint32_t M, uint32_t rescore, bool windowed, bool has_visible, uint32_t ins_limit, uint64_t* d_red) {
    if (nq == 0) return VS_OK;
    const uint32_t blocks = (nq + 255) / 256 < 256 ? (nq + 255) / 256 : 256;
    hipLaunchKernelGGL(k_reduce_stats, dim3(blocks), dim3(256), 0, idx->ctx->stream, d_stats, d_fb, d_cnt, d_status, nq, M, rescore,
                       windowed ? 1u : 0u, has_visible ? 1u : 0u, ins_limit, (unsigned long long*)d_red);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int launch_resort_cursor(vs_index* idx, uint32_t n, bool exhausted, uint32_t rescore, uint32_t k, const uint32_t* d_stream,
                         const float* d_dist, const uint32_t* d_keys, uint64_t* d_heap, uint32_t* d_cur, uint32_t* d_out_ids,
                         uint64_t* d_out_tids, float* d_out_dist) {
    const uint32_t plain_keys = (idx->d.storage_type == VS_STORAGE_PLAIN && idx->d.dim_index == idx->d.dim_full) ? 1u : 0u;
    hipLaunchKernelGGL(k_resort_cursor, dim3(1), dim3(64), 0, idx->ctx->stream, n, exhausted ? 1u : 0u, rescore, k, d_stream, d_dist,
                       d_keys, plain_keys, idx->tids, d_heap, d_cur, d_out_ids, d_out_tids, d_out_dist);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// The new stream rows of one scan-pool round, moved from the round's staging rows to the slots' stream arrays: workgroup q copies
// cnt[q] rows of each of the three kinds (ids, Hamming keys, distances) from stage[kind][q][0..] to all[kind][q][off[q]..].  The row
// counts are read on the device, so the round needs no host round trip between its search launch and this one (round 6; until then:
// one hipMemcpy2DAsync per slot after the counts had come back).  A slot that did not run, failed or ended at once has cnt 0.
__global__ __launch_bounds__(WAVE) void k_pool_append(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off, const uint32_t* __restrict__ stage,
                                                      uint32_t stage_kind_stride, uint32_t M, uint32_t* __restrict__ all, uint32_t all_kind_stride,
                                                      uint32_t rows_cap) {
    const uint32_t q = blockIdx.x;
    const uint32_t n = min(cnt[q], M), o = off[q];
    if (n == 0 || o >= rows_cap) return;
    const uint32_t m = min(n, rows_cap - o);
    for (uint32_t kind = 0; kind < 3; ++kind) {
        const uint32_t* src = stage + (size_t)kind * stage_kind_stride + (size_t)q * M;
        uint32_t* dst = all + (size_t)kind * all_kind_stride + (size_t)q * rows_cap + o;
        for (uint32_t i = threadIdx.x; i < m; i += WAVE) dst[i] = src[i];
    }
}
int launch_pool_append(vs_index* idx, uint32_t nq, const uint32_t* d_cnt, const uint32_t* d_off, const uint32_t* d_stage, uint32_t stage_kind_stride, uint32_t M,
                       uint32_t* d_all, uint32_t all_kind_stride, uint32_t rows_cap) {
    if (nq == 0) return VS_OK;
    hipLaunchKernelGGL(k_pool_append, dim3(nq), dim3(WAVE), 0, idx->ctx->stream, d_cnt, d_off, d_stage, stage_kind_stride, M, d_all, all_kind_stride, rows_cap);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// d_list: [n][3] (pool slot, rows emitted, exhausted) on the device; the per-scan arrays are rows of 2-D arrays (see the kernel)
int launch_resort_cursor_batch(vs_index* idx, uint32_t n, const uint32_t* d_list, uint32_t rescore, uint32_t k, const uint32_t* d_stream,
                               const float* d_dist, const uint32_t* d_keys, uint32_t row_stride, uint64_t* d_heap, uint32_t* d_cur,
                               uint32_t* d_out_ids, uint64_t* d_out_tids, float* d_out_dist, uint32_t out_stride) {
    if (n == 0) return VS_OK;
    const uint32_t plain_keys = (idx->d.storage_type == VS_STORAGE_PLAIN && idx->d.dim_index == idx->d.dim_full) ? 1u : 0u;
    const size_t lds = (size_t)rescore * 8 + ((size_t)rescore + k) * 4 + ((size_t)k + 4) * 4;
    VS_REQUIRE(lds <= 64 * 1024, "resort window of %u rows / %u rows per fetch does not fit LDS", rescore, k);
    hipLaunchKernelGGL(k_resort_cursor_batch, dim3(n), dim3(WAVE), lds, idx->ctx->stream, d_list, rescore, k, d_stream, d_dist, d_keys, row_stride,
                       plain_keys, idx->tids, d_heap, d_cur, d_out_ids, d_out_tids, d_out_dist, out_stride);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// the pops one launch of k_resort_cursor_batch_qual may make so that its LDS stays within 64 KB: heap entries, keys, bitmap, positions
uint32_t resort_cursor_qual_max_chunk(uint32_t rescore, uint32_t k, uint32_t rows_cap) {
    const size_t fixed = (size_t)rescore * 12 + (size_t)((rows_cap + 31) / 32) * 4 + ((size_t)k + 8) * 4;
    return fixed + 4 > 64 * 1024 ? 0u : (uint32_t)((64 * 1024 - fixed) / 4);
}

// d_list: [n][6] (pool slot, rows emitted, exhausted, qualifier slot, pops to take the fetch to, first launch) on the device; d_rec:
// [slots][4] (kept, pops, state) of the fetch in progress; d_qtab: the owner's table of qualifier bitmaps (null: no scan names one)
int launch_resort_cursor_batch_qual(vs_index* idx, uint32_t n, const uint32_t* d_list, uint32_t rescore, uint32_t k, uint32_t chunk,
                                    const uint64_t* const* d_qtab, const uint32_t* d_stream, const float* d_dist, const uint32_t* d_keys,
                                    uint32_t row_stride, uint64_t* d_heap, uint32_t* d_cur, uint32_t* d_rec, uint32_t* d_out_ids,
                                    uint64_t* d_out_tids, float* d_out_dist, uint32_t out_stride) {
    if (n == 0) return VS_OK;
    const uint32_t plain_keys = (idx->d.storage_type == VS_STORAGE_PLAIN && idx->d.dim_index == idx->d.dim_full) ? 1u : 0u;
    const uint32_t bm_words = (row_stride + 31) / 32;
    const size_t lds = (size_t)rescore * 8 + ((size_t)rescore + chunk) * 4 + (size_t)bm_words * 4 + ((size_t)k + 8) * 4;
    VS_REQUIRE(chunk >= 1 && lds <= 64 * 1024, "qualified resort window of %u rows / %u rows per fetch / %u pops per launch does not fit LDS", rescore, k, chunk);
    hipLaunchKernelGGL(k_resort_cursor_batch_qual, dim3(n), dim3(WAVE), lds, idx->ctx->stream, d_list, rescore, k, chunk, bm_words, d_qtab, d_stream,
                       d_dist, d_keys, row_stride, plain_keys, idx->tids, d_heap, d_cur, d_rec, d_out_ids, d_out_tids, d_out_dist, out_stride);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int launch_row_norms(vs_index* idx) {
    if (!idx->vecs || idx->d.n == 0) return VS_OK;
    uint32_t blocks = (idx->d.n + 63) / 64;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_row_norms, dim3(blocks), dim3(WAVE), 0, idx->ctx->stream, idx->vecs, idx->vec_stride,
                       idx->d.dim_full, idx->d.n, idx->vnorm);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int launch_row_norms_range(vs_index* idx, uint32_t row_begin, uint32_t rows) {
    if (!idx->vecs || rows == 0) return VS_OK;
    const uint32_t blocks = (rows + 63) / 64 > 8192 ? 8192 : (rows + 63) / 64;
    hipLaunchKernelGGL(k_row_norms, dim3(blocks), dim3(WAVE), 0, idx->ctx->stream, idx->vecs + (size_t)row_begin * idx->vec_stride,
                       idx->vec_stride, idx->d.dim_full, rows, idx->vnorm + row_begin);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int launch_slice_norms_range(vs_index* idx, uint32_t row_begin, uint32_t rows) {
    if (!idx->vecs || !idx->vnorm_idx || rows == 0) return VS_OK;
    const uint32_t blocks = (rows + 63) / 64 > 8192 ? 8192 : (rows + 63) / 64;
    hipLaunchKernelGGL(k_row_norms, dim3(blocks), dim3(WAVE), 0, idx->ctx->stream, idx->vecs + (size_t)row_begin * idx->vec_stride,
                       idx->vec_stride, idx->d.dim_index, rows, idx->vnorm_idx + row_begin);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int launch_validate_nbrs(vs_index* idx, uint32_t* d_flag) {
    if (idx->d.n == 0) return VS_OK;
    hipLaunchKernelGGL(k_validate_nbrs, dim3((idx->d.n + 255) / 256), dim3(256), 0, idx->ctx->stream, idx->nbrs,
                       idx->nbr_stride, idx->d.num_neighbors, idx->d.n, d_flag);
    VS_HIP(hipGetLastError());
    return VS_OK;
}
