// TEST INFRASTRUCTURE: host build of the analysis kernels' log10 (lpcnet_amd/csrc/lpcnet_log10.h) next to glibc's log10, the
// function the reference calls (src/lpcnet_enc.c:512-513: `Ly[i] = log10(1e-2+Ex[i])` stored to float).
//   g++ -O2 -ffp-contract=off -shared -fPIC -I lpcnet_amd/csrc tests/tools/log10_host.cpp -o <tmp>/liblog10_host.so
#include <cmath>
#include <cstdint>
#include <cstring>
#include "lpcnet_log10.h"

static inline uint64_t rng_next(uint64_t &s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static inline bool same(double a, long *bad, double *first /*[64]*/)
{
    const float ours = lpcn_log10f_of_double(a), ref = (float)log10(a);
    if (memcmp(&ours, &ref, 4) == 0) return true;
    if (*bad < 64) first[*bad] = a;        // the first 64 differing arguments
    ++*bad;
    return false;
}

extern "C" {
void log10_engine(const double *a, float *out, long n) { for (long i = 0; i < n; ++i) out[i] = lpcn_log10f_of_double(a[i]); }
void log10_glibc(const double *a, float *out, long n) { for (long i = 0; i < n; ++i) out[i] = (float)log10(a[i]); }
double log_unit_engine(double x) { return lpcn_log_unit(x); }

// n doubles, log-uniform over [1e-2, 1e12] with random mantissas.  counts = {evaluations, differing floats}
void log10_sweep_random(uint64_t seed, long n, long *counts, double *first_bad)
{
    long bad = 0;
    uint64_t s = seed ? seed : 1;
    const double lo = log2(1e-2), span = log2(1e12) - lo;
    for (long i = 0; i < n; ++i) {
        const double u = (double)(rng_next(s) >> 11) * 0x1p-53;
        double a = exp2(lo + span * u);
        uint64_t b;
        memcpy(&b, &a, 8);
        b = (b & ~0xfffffffull) | (rng_next(s) & 0xfffffffull);      // (exp2's low bits are not random enough)
        memcpy(&a, &b, 8);
        if (a < 1e-2) a = 1e-2;
        same(a, &bad, first_bad);
    }
    counts[0] = n; counts[1] = bad;
}

// a = 1e-2 + (double)e for every `stride`-th non-negative float e up to 1e12, and the doubles on either side of a
void log10_sweep_adjacent(int stride, long *counts, double *first_bad)
{
    long n = 0, bad = 0;
    float top = 1e12f;
    uint32_t top_bits;
    memcpy(&top_bits, &top, 4);
    for (uint32_t b = 0; b <= top_bits; b += (uint32_t)stride) {
        float e;
        memcpy(&e, &b, 4);
        const double a = 1e-2 + (double)e;
        same(a, &bad, first_bad); same(nextafter(a, 0.0), &bad, first_bad); same(nextafter(a, HUGE_VAL), &bad, first_bad);
        n += 3;
    }
    counts[0] = n; counts[1] = bad;
}

// arguments next to float rounding boundaries of the result: for every `stride`-th float f in [-2, 12] the midpoint m of f and its
// successor, a0 = the double nearest 10^m, and a0 moved by `min_steps` .. `max_steps` doubles to either side
void log10_sweep_boundaries(int stride, int min_steps, int max_steps, long *counts, double *first_bad)
{
    long n = 0, bad = 0;
    for (int sign = 0; sign < 2; ++sign) {
        float lim = sign ? 2.f : 12.f;
        uint32_t lim_bits, b0;
        float tiny = 1e-6f;
        memcpy(&lim_bits, &lim, 4);
        memcpy(&b0, &tiny, 4);
        for (uint32_t b = b0; b < lim_bits; b += (uint32_t)stride) {
            float f, g;
            uint32_t b1 = b + 1;
            memcpy(&f, &b, 4); memcpy(&g, &b1, 4);
            const double m = (sign ? -1.0 : 1.0) * 0.5 * ((double)f + (double)g);
            double a0 = pow(10.0, m);
            if (a0 < 1e-2 || a0 > 1e12) continue;
            double up = a0, dn = a0;
            for (int s = 0; s <= max_steps; ++s) {
                if (s >= min_steps) { same(up, &bad, first_bad); ++n; if (s) { same(dn, &bad, first_bad); ++n; } }
                up = nextafter(up, HUGE_VAL); dn = nextafter(dn, 0.0);
            }
        }
    }
    counts[0] = n; counts[1] = bad;
}
}
