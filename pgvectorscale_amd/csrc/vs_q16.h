// vs_q16.h — the 16-bit dedup tables of k_search_fast (FastLaunch::vslot == 2, fast_scan VG == 3): their geometry and the mapping
// between a node id and its (bucket, entry).  Plain C++ without a HIP header: the launch planning, the kernel and host-only tests all
// include this one file, so there is one copy of every constant and of every step.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__host__)
#define VS_Q16_HD __host__ __device__ static inline
#else
#define VS_Q16_HD static inline
#endif

// the bijection on qd bits: multiply, xor-shift, multiply, xor-shift (each step invertible mod 2^qd), and the multipliers' inverses mod 2^32
#define VS_Q16_A 0x9E3779B1u
#define VS_Q16_B 0x85EBCA6Bu
#define VS_Q16_AI 0x0E8B2F51u
#define VS_Q16_BI 0xA5CB9243u
static_assert((uint32_t)(VS_Q16_A * VS_Q16_AI) == 1u && (uint32_t)(VS_Q16_B * VS_Q16_BI) == 1u, "inverse multipliers");

// qdm = 2^qd - 1, qxs = (qd + 1) / 2 (2 qxs >= qd: x ^= x >> qxs is its own inverse)
VS_Q16_HD uint32_t q16_mask(uint32_t qd) { return qd >= 32 ? 0xFFFFFFFFu : (1u << qd) - 1u; }
VS_Q16_HD uint32_t q16_xshift(uint32_t qd) { return (qd + 1u) >> 1; }
VS_Q16_HD uint32_t q16_fwd(uint32_t id, uint32_t qdm, uint32_t qxs) {
    uint32_t x = (id * VS_Q16_A) & qdm;
    x ^= x >> qxs;
    x = (x * VS_Q16_B) & qdm;
    x ^= x >> qxs;
    return x;
}
VS_Q16_HD uint32_t q16_inv(uint32_t x, uint32_t qdm, uint32_t qxs) {
    x ^= x >> qxs;
    x = (x * VS_Q16_BI) & qdm;
    x ^= x >> qxs;
    return (x * VS_Q16_AI) & qdm;
}

// The cut of x < 2^qd into (bucket, entry) for ANY number of buckets NB = gcap / 8: with qe = ceil(2^qd / NB) entries per bucket,
//   bucket = x / qe (< NB, since NB qe >= 2^qd),   entry = x - bucket qe (< qe <= 2^16),   x = bucket qe + entry,
// one to one between [0, 2^qd) and the pairs it reaches.  The division is a multiply-high and a shift by constants of the launch:
// for 2^qs < qe <= 2^(qs + 1), qm = ceil(2^(32 + qs) / qe) fits 32 bits and floor(x qm / 2^(32 + qs)) = floor(x / qe) for every
// x < 2^qd as long as (qm qe - 2^(32 + qs)) 2^qd <= 2^(32 + qs) — always for qd <= 31, checked by q16_geometry for qd == 32.
// A power-of-two NB is the same code: qe = 2^(qd - lb), qm = 2^31, the bucket is x >> (qd - lb) and the entry the bits below.
// The preferred slot stays x & 7: x runs through qe >= 8 consecutive values inside a bucket, so its low bits spread over the slots.
VS_Q16_HD uint32_t q16_mul24(uint32_t a, uint32_t b) {  // both below 2^24 (buckets: gcap / 8 <= 2^19, entries per bucket <= 2^16)
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return a * b;
#endif
}
VS_Q16_HD uint32_t q16_bucket(uint32_t x, uint32_t qm, uint32_t qs) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(x, qm) >> (qs & 31u);
#else
    return (uint32_t)(((uint64_t)x * qm) >> 32) >> (qs & 31u);
#endif
}
VS_Q16_HD uint32_t q16_entry(uint32_t x, uint32_t bucket, uint32_t qe) { return x - q16_mul24(bucket, qe); }
VS_Q16_HD uint32_t q16_join(uint32_t bucket, uint32_t entry, uint32_t qe) { return q16_mul24(bucket, qe) + entry; }

struct Q16Geometry {
    uint32_t qd;       // bits the bijection works on: ceil(log2 n), at least three more than ceil(log2 buckets)
    uint32_t qe;       // entries per bucket, 8 .. 65536
    uint32_t qm, qs;   // bucket = mulhi(x, qm) >> qs
    uint32_t ocap;     // slots of the overflow table of whole ids behind the buckets
    uint32_t vwords;   // u32 words of occupancy bits: one bit per slot of the buckets, then of the overflow table
    uint32_t gregion;  // u32 words of one table: gcap / 2 + ocap
    uint32_t sb;       // bits of a slot handle: gcap + ocap <= 2^sb
};
// gcap: slots of the buckets, a multiple of 256 (>= 1024 wherever the launch planning chooses it).  false: no 16-bit form for an index
// of n rows at this gcap — an entry would need more than 16 bits (gcap / 8 < 2^(qd - 16)), or more than 32 hashed bits.
static inline bool q16_geometry(uint64_t n, uint32_t gcap, Q16Geometry* g) {
    *g = Q16Geometry{};
    if (gcap < 256 || gcap % 256 != 0 || gcap > (1u << 26)) return false;
    const uint32_t nb = gcap >> 3;
    uint32_t qd = 1, lb = 0;
    while (qd < 40 && (1ull << qd) < (n > 2 ? n : 2)) qd++;
    while ((1u << lb) < nb) lb++;
    if (qd < lb + 3) qd = lb + 3;  // (a small index: more hash bits than id bits — the bijection works on any width)
    g->qd = qd;
    // overflow table: a sixteenth of the buckets' slots, at least 256, in steps of 128 slots (of 32 before round 20; every power-of-two
    // gcap gets what it got).  128 slots are four occupancy words: gcap / 32 is a multiple of eight, so vwords stays a multiple of four
    // for any gcap, which the resumable scans need — their LDS image ends with the occupancy words and is copied in 16-byte steps
    // (the launch wrapper checks it).
    const uint32_t o = (gcap / 16 + 127) / 128 * 128;
    g->ocap = o > 256 ? o : 256;
    g->vwords = (gcap + g->ocap) / 32;
    g->gregion = (gcap >> 1) + g->ocap;
    g->sb = 0;
    while ((1ull << g->sb) < (uint64_t)gcap + g->ocap) g->sb++;
    g->qe = g->qm = g->qs = 0;
    if (qd > 32) return false;
    const uint64_t qe = ((1ull << qd) + nb - 1) / nb;
    if (qe > 65536) return false;  // nb < 2^(qd - 16)
    uint32_t qs = 0;
    while ((2ull << qs) < qe) qs++;  // 2^qs < qe <= 2^(qs + 1)   (qe >= 8: qs >= 2)
    const uint64_t two = 1ull << (32 + qs);
    const uint64_t qm = (two + qe - 1) / qe;
    if (qm >> 32 || ((qm * qe - two) << qd) > two) return false;
    g->qe = (uint32_t)qe;
    g->qm = (uint32_t)qm;
    g->qs = qs;
    return true;
}
