// (float)log10(a) for a double a, as the reference's host computes it, without a math library.
//
// Why: the analysis takes `Ly[i] = log10(1e-2 + Ex[i])` in double and stores it to float (src/lpcnet_enc.c:512-513).  The
// PARITY TARGET is what the reference computes on its host: glibc's log10, which is NOT correctly rounded -- it is fdlibm's
//     z = y*log10_2lo + ivln10*log(x);  return z + y*log10_2hi;          (a = 2^y * x, x in [1,2) for y >= 0, [0.5,1) below)
// on top of glibc's own log (< 0.52 ULP), some 2 ULP in all.  A correctly rounded log10 therefore gives a DIFFERENT float
// whenever the exact value lies within those 2 ULP of a float rounding boundary: 2^-27 per call, one band every ten seconds
// at 8192 streams x 100 frames x 18 bands per second.  So this routine does what lpcnet_exp10.h does one level further down:
// it restates fdlibm's three roundings operation for operation and puts a log(x) under them that is correctly rounded for
// all practical purposes (double-double centre table, argument reduction and series: ~2^-68 relative before the rounding
// to double).  What is left is an argument for which glibc's log(x) is not the correctly rounded double (it claims
// 0.519 ULP, not 0.5) AND whose last bit decides the float.  Measured (tests/test_analysis_host.py): no differing float
// over 1.2e7 random arguments of the reachable range [1e-2, 1e12] and over 4e7 doubles adjacent to 1e-2 + float; among 3.4e6
// arguments CONSTRUCTED to put the result within half a double-ULP of a float rounding boundary 43 differ, and for every one
// of them 80-digit arithmetic shows glibc's log(x) 0.500..0.508 ULP off while this routine's is the correctly rounded one.
// That is ~1e-5 of the 2^-28 of all calls whose last double bit matters: about one band per hour at 8192 streams x 100 frames
// x 18 bands per second; the analysis has no feedback, so such a difference stays in that one coefficient of that one frame.
// A host whose libm differs (another glibc, musl) has the same exposure against THAT libm.
//
//   x = c*(1 + r), c = 1 + i/128 the nearest centre, |r| <= 2^-8:  log(x) = log(c) + (r - r^2/2 + r^3/3 - ...)
#pragma once
#include <stdint.h>
#include <string.h>
#include "lpcnet_exp10.h"      // LPCN_EXP10_TABLE_QUAL / LPCN_EXP10_FN: the host / device qualifiers
#include "lpcnet_analysis_tables_gen.h"

// log(x) for x in [0.5, 2), rounded to double
LPCN_EXP10_FN double lpcn_log_unit(const double x)
{
    const bool low = x < 1.0;
    const double m = low ? x * 2.0 : x;                        // [1, 2), exact
    const int i = (int)((m - 1.0) * 128.0 + 0.5);              // nearest centre, 0..128
    const double c = 1.0 + (double)i * 0.0078125;
    const double d = m - c;                                    // exact: |d| <= 2^-8, both multiples of 2^-52
    const double ic_hi = lpcn_log_tab[i][2], ic_lo = lpcn_log_tab[i][3];
    // r = d / c as r_hi + r_lo
    const double r_hi = d * ic_hi;
    const double r_lo = fma(d, ic_hi, -r_hi) + d * ic_lo;
    // r^2 as a pair: its half is 2^-9 of r, too large for one double's rounding
    const double r2_hi = r_hi * r_hi;
    const double r2_lo = fma(r_hi, r_hi, -r2_hi) + 2.0 * (r_hi * r_lo);
    // r^3/3 - r^4/4 + ... - r^10/10 (|r| <= 2^-8: the first dropped term is 2^-80 of r)
    const double q = r_hi * r2_hi * (1.0 / 3 + r_hi * (-1.0 / 4 + r_hi * (1.0 / 5 + r_hi * (-1.0 / 6 + r_hi * (1.0 / 7 + r_hi * (-1.0 / 8
                     + r_hi * (1.0 / 9 + r_hi * (-1.0 / 10))))))));
    const double h2 = -0.5 * r2_hi;
    const double s_hi = r_hi + h2;                             // fast two-sum, |r_hi| >= |h2|
    const double s_lo = h2 - (s_hi - r_hi);
    const double p_lo = s_lo + (r_lo + (q - 0.5 * r2_lo));
    // log(c), minus ln 2 for the lower half (centre 128 cancels exactly: its entry IS ln 2)
    double c_hi = lpcn_log_tab[i][0], c_lo = lpcn_log_tab[i][1];
    if (low) {
        const double t = c_hi - LPCN_LOG_LN2_HI;               // two-sum
        const double bb = t - c_hi;
        const double e = (c_hi - (t - bb)) + (-LPCN_LOG_LN2_HI - bb);
        c_lo = e + (c_lo - LPCN_LOG_LN2_LO);
        c_hi = t;
    }
    const double t = c_hi + s_hi;                              // two-sum
    const double bb = t - c_hi;
    const double e = (c_hi - (t - bb)) + (s_hi - bb);
    return t + (e + (c_lo + p_lo));
}

// (float)log10(a), a finite and positive (the analysis passes 1e-2 + a band energy)
LPCN_EXP10_FN float lpcn_log10f_of_double(const double a)
{
    if (!(a < HUGE_VAL)) return (float)(a + a);                // infinity, NaN (a float input beyond any PCM range)
    uint64_t bits;
    memcpy(&bits, &a, 8);
    int k = (int)((bits >> 52) & 0x7ff) - 1023;
    const int below = k < 0 ? 1 : 0;
    bits = (bits & 0x000fffffffffffffull) | ((uint64_t)(0x3ff - below) << 52);
    double x;
    memcpy(&x, &bits, 8);
    const double y = (double)(k + below);
    const double z = y * 3.69423907715893078616e-13 + 4.34294481903251816668e-01 * lpcn_log_unit(x);      // log10_2lo, ivln10
    return (float)(z + y * 3.01029995663611771306e-01);                                                   // log10_2hi
}
