// Host-only check of the 16-bit dedup tables' geometry and id mapping (pgvectorscale_amd/csrc/vs_q16.h), built and run by
// tests/test_q16_geometry.py with the host compiler's address and undefined-behaviour sanitizers.
//   q16_check <n> <gcap> ...   one line per (n, gcap):
//   n gcap accepted qd qe qm qs ocap vwords gregion sb bad_bucket bad_entry bad_inverse bad_hash
#include <cstdio>
#include <cstdlib>

#include "vs_q16.h"

int main(int argc, char** argv) {
    // the host inverse of the id hash is the kernel's: one set of multipliers, and each pair multiplies to 1 mod 2^32
    const uint32_t pa = (uint32_t)(VS_Q16_A * VS_Q16_AI), pb = (uint32_t)(VS_Q16_B * VS_Q16_BI);
    printf("products %u %u\n", pa, pb);
    for (int i = 1; i + 1 < argc; i += 2) {
        const uint64_t n = strtoull(argv[i], nullptr, 10);
        const uint32_t gcap = (uint32_t)strtoul(argv[i + 1], nullptr, 10);
        Q16Geometry g;
        const bool ok = q16_geometry(n, gcap, &g);
        uint64_t bad_bucket = 0, bad_entry = 0, bad_inverse = 0, bad_hash = 0;
        if (ok) {
            const uint32_t nb = gcap >> 3, qdm = q16_mask(g.qd), qxs = q16_xshift(g.qd);
            auto check = [&](uint64_t x64) {
                const uint32_t x = (uint32_t)x64;
                const uint32_t b = q16_bucket(x, g.qm, g.qs), e = q16_entry(x, b, g.qe);
                bad_bucket += b >= nb || b != x64 / g.qe;
                bad_entry += e >= 65536u;
                bad_inverse += q16_join(b, e, g.qe) != x;
                bad_hash += q16_inv(q16_fwd(x, qdm, qxs), qdm, qxs) != x || q16_fwd(x, qdm, qxs) > qdm;
            };
            const uint64_t end = 1ull << g.qd;
            if (g.qd <= 26) {
                for (uint64_t x64 = 0; x64 < end; ++x64) check(x64);
            } else {  // a sampled walk: every 251st x, and both sides of every bucket boundary (where a wrong quotient shows first)
                for (uint64_t x64 = 0; x64 < end; x64 += 251) check(x64);
                for (uint64_t bk = 1; bk * g.qe < end; ++bk) {
                    check(bk * g.qe - 1);
                    check(bk * g.qe);
                }
                check(end - 1);
            }
        }
        printf("%llu %u %d %u %u %u %u %u %u %u %u %llu %llu %llu %llu\n", (unsigned long long)n, gcap, ok ? 1 : 0, g.qd, g.qe, g.qm, g.qs, g.ocap,
               g.vwords, g.gregion, g.sb, (unsigned long long)bad_bucket, (unsigned long long)bad_entry, (unsigned long long)bad_inverse,
               (unsigned long long)bad_hash);
    }
    return 0;
}
