// Device helpers the frame, analysis and PLC kernels share: the 320-point FFT of the reference's kiss FFT and lpc_from_cepstrum, by one wavefront.
#pragma once
#include <hip/hip_runtime.h>
#include "lpcnet_engine.h"
#include "lpcnet_math.h"
#include "lpcnet_exp10.h"
#include "kernel_params.h"

#define LPCN_MAX16(a, b) ((a) > (b) ? (a) : (b))      // the reference's MAX16 (src/arch.h), same operand roles

namespace lpcn {

struct cpx { float r, i; };
__device__ __forceinline__ cpx cmul(cpx a, cpx b) { cpx m; m.r = a.r * b.r - a.i * b.i; m.i = a.r * b.i + a.i * b.r; return m; }
__device__ __forceinline__ cpx cadd(cpx a, cpx b) { cpx m; m.r = a.r + b.r; m.i = a.i + b.i; return m; }
__device__ __forceinline__ cpx csub(cpx a, cpx b) { cpx m; m.r = a.r - b.r; m.i = a.i - b.i; return m; }

// The radix-4 (m = 1, 4, 16) and radix-5 (m = 64) passes of opus_fft_impl for nfft = 320 (src/kiss_fft.c:111-168, :232-305), in place on F
// (digit-reversed, scaled input) by one wavefront.  Contains workgroup barriers: every wavefront of the workgroup calls it; F is complete
// for all lanes on return.  Shared by lpc_kernel and the analysis kernel (analysis_kernels.hip.h).
__device__ __forceinline__ void fft320_passes(cpx *F, const cpx *TW, const int lane)
{
    // radix-4, m = 1: 80 butterflies with unit twiddles (src/kiss_fft.c:111-131)
    for (int b = lane; b < 80; b += 64) {
        cpx *f = F + 4 * b;
        cpx f0 = f[0], f1 = f[1], f2 = f[2], f3 = f[3];
        cpx s0 = csub(f0, f2);
        f0 = cadd(f0, f2);
        cpx s1 = cadd(f1, f3);
        f2 = csub(f0, s1);
        f0 = cadd(f0, s1);
        s1 = csub(f1, f3);
        f1.r = s0.r + s1.i; f1.i = s0.i - s1.r;
        f3.r = s0.r - s1.i; f3.i = s0.i + s1.r;
        f[0] = f0; f[1] = f1; f[2] = f2; f[3] = f3;
    }
    __syncthreads();
    // radix-4 stages m = 4 (fstride 20) and m = 16 (fstride 5) (src/kiss_fft.c:132-168)
#pragma unroll
    for (int stage = 0; stage < 2; ++stage) {
        const int m = stage == 0 ? 4 : 16, fs = stage == 0 ? 20 : 5;
        for (int b = lane; b < 80; b += 64) {
            const int blk = b / m, j = b % m;
            cpx *f = F + blk * 4 * m + j;
            const cpx a = cmul(f[m], TW[j * fs]), bb = cmul(f[2 * m], TW[2 * j * fs]), cc = cmul(f[3 * m], TW[3 * j * fs]);
            cpx f0 = f[0];
            const cpx d = csub(f0, bb);
            f0 = cadd(f0, bb);
            const cpx e = cadd(a, cc), g = csub(a, cc);
            f[2 * m] = csub(f0, e);
            f[0] = cadd(f0, e);
            cpx o1, o3;
            o1.r = d.r + g.i; o1.i = d.i - g.r;
            o3.r = d.r - g.i; o3.i = d.i + g.r;
            f[m] = o1; f[3 * m] = o3;
        }
        __syncthreads();
    }
    // radix-5, m = 64 (src/kiss_fft.c:232-305)
    {
        const cpx ya = TW[64], yb = TW[128];
        const int u = lane;
        cpx *F0 = F + u, *F1 = F0 + 64, *F2 = F0 + 128, *F3 = F0 + 192, *F4 = F0 + 256;
        const cpx s0 = *F0;
        const cpx s1 = cmul(*F1, TW[u]), s2 = cmul(*F2, TW[2 * u]), s3 = cmul(*F3, TW[3 * u]), s4 = cmul(*F4, TW[4 * u]);
        const cpx s7 = cadd(s1, s4), s10 = csub(s1, s4), s8 = cadd(s2, s3), s9 = csub(s2, s3);
        cpx o0, s5, s6, s11, s12;
        o0.r = s0.r + (s7.r + s8.r);
        o0.i = s0.i + (s7.i + s8.i);
        s5.r = s0.r + (s7.r * ya.r + s8.r * yb.r);
        s5.i = s0.i + (s7.i * ya.r + s8.i * yb.r);
        s6.r = s10.i * ya.i + s9.i * yb.i;
        s6.i = -(s10.r * ya.i + s9.r * yb.i);
        s11.r = s0.r + (s7.r * yb.r + s8.r * ya.r);
        s11.i = s0.i + (s7.i * yb.r + s8.i * ya.r);
        s12.r = s9.i * ya.i - s10.i * yb.i;
        s12.i = s10.r * yb.i - s9.r * ya.i;
        __syncthreads();
        *F0 = o0; *F1 = csub(s5, s6); *F4 = cadd(s5, s6); *F2 = cadd(s11, s12); *F3 = csub(s11, s12);
    }
    __syncthreads();
}

// lpc_from_cepstrum (src/freq.c:310-320, without lpc_weighting) by one wavefront: the 16 coefficients are left in lane 0's `lpc` when `active`.
// c: the 18 cepstral coefficients (c0 without the +4); F [320], ex [18], xr [164]: the wavefront's LDS.  Contains workgroup barriers.
__device__ __forceinline__ void lpc_from_cepstrum_wave(const LpcnFrameModel &M, const float *c, cpx *F, float *ex, float *xr, const int lane,
                                                       const bool active, float lpc[LPCN_LPC_ORDER])
{
    const cpx *TW = (const cpx *)M.tab_tw;
    static const short band_edge[LPCN_NB_BANDS] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 34, 40};   // src/freq.c:46-49
    static const float band_comp[LPCN_NB_BANDS] = {0.8f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 0.666667f, 0.5f, 0.5f, 0.5f,
                                                   0.333333f, 0.25f, 0.25f, 0.2f, 0.166667f, 0.173913f};             // src/freq.c:51-53
    // inverse DCT of the cepstrum (+4 on c0) and 10^x with the band compensation (src/freq.c:230-240, :317-318)
    if (lane < LPCN_NB_BANDS) {
        float sum = 0.f;
        for (int j = 0; j < LPCN_NB_BANDS; ++j) {
            float cj = c[j];
            if (j == 0) cj = cj + 4.f;
            sum = sum + cj * M.tab_idct[lane * LPCN_NB_BANDS + j];
        }
        const float e = (float)((double)sum * sqrt(2. / LPCN_NB_BANDS));
        // pow(10.f, e) in double, then the product with the band compensation rounded to float (src/freq.c:317-318);
        // lpcn_exp10 is this engine's own correctly rounded 10^e (lpcnet_exp10.h), not the device math library's pow
        ex[lane] = (float)(lpcn_exp10(e) * (double)band_comp[lane]);
    }
    __syncthreads();
    // band interpolation (src/freq.c:202-215); bin 160 forced to 0 (:286)
    for (int k = lane; k < 161; k += 64) {
        float v = 0.f;
        if (k < 160) {
            int b = 0;
            while (b < LPCN_NB_BANDS - 2 && k >= band_edge[b + 1] * 4) ++b;
            const int size = (band_edge[b + 1] - band_edge[b]) * 4, j = k - band_edge[b] * 4;
            const float frac = (float)j / (float)size;
            v = (1.f - frac) * ex[b] + frac * ex[b + 1];
        }
        xr[k] = v;
    }
    __syncthreads();
    // Hermitian extension + digit-reversal copy with the 1/320 scale (src/freq.c:260-266, src/kiss_fft.c:579-584)
    for (int k = lane; k < 320; k += 64) {
        const float re = k < 161 ? xr[k] : xr[320 - k];
        const float im = k < 161 ? 0.f : -0.f;
        cpx v; v.r = 0.0031250000f * re; v.i = 0.0031250000f * im;
        F[M.tab_bitrev[k]] = v;
    }
    __syncthreads();
    fft320_passes(F, TW, lane);
    // autocorrelation lags 0..16 (reversed read, src/freq.c:268-272), noise floor, lag window, Levinson
    if (lane == 0 && active) {
        float ac[LPCN_LPC_ORDER + 1];
        ac[0] = 320.f * F[0].r;
        for (int k = 1; k <= LPCN_LPC_ORDER; ++k) ac[k] = 320.f * F[320 - k].r;
        ac[0] = (float)((double)ac[0] + ((double)ac[0] * 1e-4 + 320 / 12 / 38.));      // src/freq.c:291
        for (int k = 1; k <= LPCN_LPC_ORDER; ++k) ac[k] = (float)((double)ac[k] * (1 - 6e-5 * k * k));
        for (int k = 0; k < LPCN_LPC_ORDER; ++k) lpc[k] = 0.f;
        float err = ac[0];
        if (ac[0] != 0.f) {
            for (int k = 0; k < LPCN_LPC_ORDER; ++k) {                                   // src/freq.c:86-127, float build
                float rr = 0.f;
                for (int j = 0; j < k; ++j) rr = rr + lpc[j] * ac[k - j];
                rr = rr + ac[k + 1];
                const float r = -rr / err;
                lpc[k] = r;
                for (int j = 0; j < (k + 1) >> 1; ++j) {
                    const float t1 = lpc[j], t2 = lpc[k - 1 - j];
                    lpc[j] = t1 + r * t2;
                    lpc[k - 1 - j] = t2 + r * t1;
                }
                err = err - (r * r) * err;
                if (err < .001f * ac[0]) break;
            }
        }
    }
}

}  // namespace lpcn
