// vs_device.h — device helpers shared by the gfx950 kernels (wave64).
#pragma once
#include "vs_internal.h"

#define WAVE 64

// ---------------------------------------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// add the value held by the lane with index (lane ^ 1) / (lane ^ 2) via DPP quad_perm (no LDS traffic)
__device__ __forceinline__ uint32_t quad_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1 /*quad_perm [1,0,3,2]*/, 0xF, 0xF, true);
    v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E /*quad_perm [2,3,0,1]*/, 0xF, 0xF, true);
    return v;
}

// 16 bytes of a code row read once per scan: a non-temporal load (global_load_dwordx4 ... nt), so the stream of gathered
// rows does not push the scans' own working sets (dedup tables, heap spill) out of L2
// (the address space is spelled out: a pointer that went through in_vgpr() — or any other opaque step — is a generic one to the compiler,
// and its load a FLAT load, which also counts against the LDS counter and waits for it: round 6 found every stream load of
// k_search_fast compiled that way)
typedef __attribute__((address_space(1))) __uint128_t vs_glb_u128;
typedef __attribute__((address_space(1))) uint64_t vs_glb_u64;
typedef __attribute__((address_space(1))) uint32_t vs_glb_u32;
__device__ __forceinline__ ulonglong2 load_stream16(const uint64_t* p) {
    const __uint128_t v = __builtin_nontemporal_load((const vs_glb_u128*)p);
    return make_ulonglong2((unsigned long long)v, (unsigned long long)(v >> 64));
}

// the same for data a scan reads once and never again: its visit's neighbor row (and the neighbors' label masks next to it), a heap tid
__device__ __forceinline__ uint32_t load_stream32(const uint32_t* p) { return __builtin_nontemporal_load((const vs_glb_u32*)p); }
__device__ __forceinline__ uint64_t load_stream64(const uint64_t* p) { return __builtin_nontemporal_load((const vs_glb_u64*)p); }

// per 16-bit half: min(a, b) (v_pk_min_u16).  Written with the GCC vector extension so that the host build of the test interpreter
// compiles it too.
typedef unsigned short vs_u16x2 __attribute__((vector_size(4)));
__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b) {
    vs_u16x2 x, y;
    __builtin_memcpy(&x, &a, 4);
    __builtin_memcpy(&y, &b, 4);
    const vs_u16x2 m = x < y ? x : y;
    uint32_t r;
    __builtin_memcpy(&r, &m, 4);
    return r;
}
// A wave-uniform value the compiler is told nothing about, held in a VECTOR register: scalar registers are what k_search_fast runs
// out of (106 with 226 spilled in round 5), vector registers it has to spare, and a vector instruction takes its operand from
// either file at the same cost — so the loop-invariant constants that only ever feed vector instructions (array base pointers, hash
// masks) are parked there by hand instead of being re-read from the kernel arguments inside the loop (s_load + s_waitcnt).
template <class T>
__device__ __forceinline__ T in_vgpr(T x) {
    asm volatile("" : "+v"(x));
    return x;
}
// a wave-uniform 64-bit lane mask as a per-lane condition (no vector instruction: the mask goes straight into exec)
__device__ __forceinline__ bool lane_of(uint64_t mask) { return __builtin_amdgcn_inverse_ballot_w64(mask); }

__device__ __forceinline__ uint32_t hash_u32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352dU;
    x ^= x >> 15;
    x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}

// ---- heap visibility of one scan of a launch (VisView, vs_internal.h) ----------------------------------------------
// bytes == nullptr: nothing is hidden from this scan.  ov == nullptr: legacy mode, a node is hidden iff its byte is 0.  Otherwise the
// byte is the node's class, and only a class-2 node is looked up in the ascending depends list for the scan's overlay byte.
struct ScanVis {
    const uint8_t* bytes;
    const uint32_t* dep;
    const uint8_t* ov;
    uint32_t r;
};
__device__ __forceinline__ ScanVis vis_of_scan(const VisView& v, uint32_t q) {
    ScanVis s{v.bytes, nullptr, nullptr, 0u};
    if (v.slots && v.bytes) {
        const uint32_t slot = v.slots[q];  // (wave-uniform: one scan per wave)
        if (slot == 0 || slot >= VS_MAX_VIS_SLOTS) {
            s.bytes = nullptr;  // slot 0: every tuple visible (the host has refused anything beyond the table)
        } else {
            s.dep = v.dep;
            s.ov = v.overlay[slot];
            s.r = v.r;
        }
    }
    return s;
}
// is `node` hidden from the scan, given its byte of s.bytes (the fast kernel requests that byte ahead of its use)
__device__ __forceinline__ bool vis_hidden(const ScanVis& s, uint32_t node, uint32_t byte) {
    if (!s.ov) return byte == 0;
    if (byte != VIS_CLASS_DEPENDS) return byte == VIS_CLASS_NONE;
    uint32_t lo = 0, hi = s.r;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (s.dep[mid] < node) lo = mid + 1;
        else hi = mid;
    }
    return lo >= s.r || s.dep[lo] != node || s.ov[lo] == 0;  // (a class-2 node is always on the list: the list is built from the classes)
}
__device__ __forceinline__ bool vis_hidden(const ScanVis& s, uint32_t node) { return s.bytes && vis_hidden(s, node, s.bytes[node]); }

// Hamming distance of one code row against the query code held in LDS, computed by a group of 4 lanes
// (lane l4 covers words 2*l4 + 8t, 2*l4+1 + 8t: 16 B per lane per step, 64 B contiguous per group per step).
// Rows are code_stride (even) words, zero padded, so the padded tail contributes popcount(0^0)=0.
__device__ __forceinline__ uint32_t ham_row4(const uint64_t* __restrict__ row, const uint64_t* qc, int l4,
                                             uint32_t code_stride, bool active) {
    uint32_t acc = 0;
    if (active) {
        for (uint32_t w = 2u * (uint32_t)l4; w < code_stride; w += 8) {
            const ulonglong2 r = *reinterpret_cast<const ulonglong2*>(row + w);
            const ulonglong2 qq = *reinterpret_cast<const ulonglong2*>(qc + w);
            acc += (uint32_t)__popcll(r.x ^ qq.x) + (uint32_t)__popcll(r.y ^ qq.y);
        }
    }
    return quad_sum(acc);
}

// monotone u32 image of f32::total_cmp (DistanceWithTieBreak compares distances with total_cmp,
// AM/graph/neighbor_with_distance.rs:74-83): heap / visited keys of the plain-storage search
__device__ __forceinline__ uint32_t plain_key(float f) {
    int32_t b = __float_as_int(f);
    b ^= (int32_t)(((uint32_t)(b >> 31)) >> 1);
    return (uint32_t)b ^ 0x80000000u;
}

// the inverse of plain_key: the f32 distance a key stands for (the transform only flips the low 31 bits of negative values, so
// it undoes itself once the sign bit is back)
__device__ __forceinline__ float plain_unkey(uint32_t k) {
    int32_t b = (int32_t)(k ^ 0x80000000u);
    b ^= (int32_t)(((uint32_t)(b >> 31)) >> 1);
    return __int_as_float(b);
}

// PlainDistanceMeasure::calculate_distance (AM/plain/storage.rs:239-247,273-281): distance_fn(query index slice, node
// vector) for the row each 8-lane group points at, in the reference's AVX2 accumulation order — the same arithmetic as
// k_rerank (vs_kernels.hip): lane l8 owns elements 32t + 4 l8 .. +3, i.e. 4 of the 32 virtual AVX2 lanes; L2 is mul + add,
// dot is FMA; horizontal_add_ps per accumulator, the four accumulators summed left to right, then the scalar tail.  The
// stored vector is the cosine-normalised insert-time vector: the raw row divided by its cached norm.  Valid on l8 == 0.
__device__ __forceinline__ float plain_dist8(const float* __restrict__ row, float sdiv, const float* qv, uint32_t dim,
                                             uint32_t distance_type, int lane, bool valid) {
    const int l8 = lane & 7;
    const uint32_t steps = dim / 32;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (valid) {
        if (distance_type == VS_L2) {
            for (uint32_t t = 0; t < steps; ++t) {
                const float4 x = *reinterpret_cast<const float4*>(row + 32 * t + 4 * l8);
                const float4 y = *reinterpret_cast<const float4*>(qv + 32 * t + 4 * l8);
                const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
                const float p0 = d0 * d0, p1 = d1 * d1, p2 = d2 * d2, p3 = d3 * d3;
                a0 = a0 + p0;
                a1 = a1 + p1;
                a2 = a2 + p2;
                a3 = a3 + p3;
            }
        } else {
            for (uint32_t t = 0; t < steps; ++t) {
                float4 x = *reinterpret_cast<const float4*>(row + 32 * t + 4 * l8);
                const float4 y = *reinterpret_cast<const float4*>(qv + 32 * t + 4 * l8);
                if (sdiv != 0.0f) {
                    x.x = x.x / sdiv;
                    x.y = x.y / sdiv;
                    x.z = x.z / sdiv;
                    x.w = x.w / sdiv;
                }
                a0 = __builtin_fmaf(x.x, y.x, a0);
                a1 = __builtin_fmaf(x.y, y.y, a1);
                a2 = __builtin_fmaf(x.z, y.z, a2);
                a3 = __builtin_fmaf(x.w, y.w, a3);
            }
        }
    }
    const float s0 = a0 + __shfl(a0, lane ^ 1, WAVE);
    const float s1 = a1 + __shfl(a1, lane ^ 1, WAVE);
    const float s2 = a2 + __shfl(a2, lane ^ 1, WAVE);
    const float s3 = a3 + __shfl(a3, lane ^ 1, WAVE);
    const float t0 = s0 + s1;
    const float t1 = s2 + s3;
    const float h = t0 + t1;
    const int g0 = lane & ~7;
    const float h0 = __shfl(h, g0 + 0, WAVE), h1 = __shfl(h, g0 + 2, WAVE), h2 = __shfl(h, g0 + 4, WAVE), h3 = __shfl(h, g0 + 6, WAVE);
    float dist = h0 + h1;
    dist = dist + h2;
    dist = dist + h3;
    float r = 0.0f;
    if (valid && l8 == 0) {
        for (uint32_t i = steps * 32; i < dim; ++i) {  // scalar tail, in element order
            float x = row[i];
            if (distance_type == VS_L2) {
                const float diff = x - qv[i];
                const float p = diff * diff;
                dist = dist + p;
            } else {
                if (sdiv != 0.0f) x = x / sdiv;
                const float p = x * qv[i];
                dist = dist + p;
            }
        }
        if (distance_type == VS_L2) r = dist;
        else if (distance_type == VS_IP) r = -dist;
        else r = fmaxf(1.0f - dist, 0.0f);
    }
    return r;
}
