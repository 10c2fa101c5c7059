// Burg's method as the packet-loss concealment uses it: silk_burg_analysis(A, x, 1e-3, 79, 1, 16) of src/burg.c:98-245, called by
// compute_burg_cepstrum (src/freq.c:156-188) on the 79 pre-emphasised differences of one 80-sample half frame.  One subframe, order 16.
// Every sum is in double in the reference's order; the two products the reference forms in float (src/burg.c:137-138) are formed in
// float.  Plain C++: the same lines compile for the host, where they were checked against the reference's silk_burg_analysis on random,
// silent, constant and pulse inputs.  The translation unit MUST be compiled with -ffp-contract=off.
#pragma once
#include "lpcnet_math.h"      // LPCN_HD

#define LPCN_BURG_LEN   79
#define LPCN_BURG_ORDER 16
// doubles of working storage the recursion needs (the device keeps them in LDS: dynamically indexed arrays would go to scratch)
#define LPCN_BURG_WORK  (2 * LPCN_BURG_ORDER + 2 * (LPCN_BURG_ORDER + 1) + LPCN_BURG_ORDER)

// silk_energy_FLP / silk_inner_product_FLP (src/burg.c:43-95): four products added left to right, then accumulated; the rest one by one.
// A float x float product is exact in double.
LPCN_HD double lpcn_burg_inner(const float *a, const float *b, const int n)
{
    double result = 0.0;
    int i = 0;
    for (; i < n - 3; i += 4)
        result += a[i] * (double)b[i] + a[i + 1] * (double)b[i + 1] + a[i + 2] * (double)b[i + 2] + a[i + 3] * (double)b[i + 3];
    for (; i < n; ++i) result += a[i] * (double)b[i];
    return result;
}

// The recursion (src/burg.c:131-244) from the autocorrelations c[0] = C0, c[n] = C_first_row[n - 1]; A receives the 16 prediction
// coefficients, the residual energy is returned.  work: LPCN_BURG_WORK doubles.
LPCN_HD float lpcn_burg_recursion(float *A, const float *x, const double *c, double *work)
{
    const int L = LPCN_BURG_LEN, D = LPCN_BURG_ORDER;
    double *Cf = work, *Cl = Cf + D, *CAf = Cl + D, *CAb = CAf + D + 1, *Af = CAb + D + 1;
    const double minInvGain = (double)1e-3f;      // (the parameter is a float, src/burg.c:102)
    double C0 = c[0];
    for (int k = 0; k < D; ++k) { Cf[k] = c[k + 1]; Cl[k] = c[k + 1]; }
    CAb[0] = CAf[0] = C0 + (double)1e-5f * C0 + (double)1e-9f;
    double invGain = 1.0, nrg_f, nrg_b, num, rc, tmp1, tmp2, Atmp;
    int reached_max_gain = 0;
    for (int n = 0; n < D; ++n) {
        tmp1 = x[n];
        tmp2 = x[L - n - 1];
        for (int k = 0; k < n; ++k) {
            const float pf = x[n] * x[n - k - 1], pl = x[L - n - 1] * x[L - n + k];      // float products (src/burg.c:137-138)
            Cf[k] -= (double)pf;
            Cl[k] -= (double)pl;
            Atmp = Af[k];
            tmp1 += x[n - k - 1] * Atmp;
            tmp2 += x[L - n + k] * Atmp;
        }
        for (int k = 0; k <= n; ++k) {
            CAf[k] -= tmp1 * x[n - k];
            CAb[k] -= tmp2 * x[L - n + k - 1];
        }
        tmp1 = Cf[n];
        tmp2 = Cl[n];
        for (int k = 0; k < n; ++k) {
            Atmp = Af[k];
            tmp1 += Cl[n - k - 1] * Atmp;
            tmp2 += Cf[n - k - 1] * Atmp;
        }
        CAf[n + 1] = tmp1;
        CAb[n + 1] = tmp2;
        num = CAb[n + 1];
        nrg_b = CAb[0];
        nrg_f = CAf[0];
        for (int k = 0; k < n; ++k) {
            Atmp = Af[k];
            num += CAb[n - k] * Atmp;
            nrg_b += CAb[k + 1] * Atmp;
            nrg_f += CAf[k + 1] * Atmp;
        }
        rc = -2.0 * num / (nrg_f + nrg_b);
        tmp1 = invGain * (1.0 - rc * rc);
        if (tmp1 <= minInvGain) {
            rc = sqrt(1.0 - minInvGain / invGain);
            if (num > 0) rc = -rc;
            invGain = minInvGain;
            reached_max_gain = 1;
        } else {
            invGain = tmp1;
        }
        for (int k = 0; k < (n + 1) >> 1; ++k) {
            tmp1 = Af[k];
            tmp2 = Af[n - k - 1];
            Af[k] = tmp1 + rc * tmp2;
            Af[n - k - 1] = tmp2 + rc * tmp1;
        }
        Af[n] = rc;
        if (reached_max_gain) {
            for (int k = n + 1; k < D; ++k) Af[k] = 0.0;
            break;
        }
        for (int k = 0; k <= n + 1; ++k) {
            tmp1 = CAf[k];
            CAf[k] += rc * CAb[n - k + 1];
            CAb[n - k + 1] += rc * tmp1;
        }
    }
    if (reached_max_gain) {
        for (int k = 0; k < D; ++k) A[k] = (float)(-Af[k]);
        C0 -= lpcn_burg_inner(x, x, D);
        nrg_f = C0 * invGain;
    } else {
        nrg_f = CAf[0];
        tmp1 = 1.0;
        for (int k = 0; k < D; ++k) {
            Atmp = Af[k];
            nrg_f += CAf[k + 1] * Atmp;
            tmp1 += Atmp * Atmp;
            A[k] = (float)(-Atmp);
        }
        nrg_f -= (double)1e-5f * C0 * tmp1;
    }
    return (float)nrg_f;
}
