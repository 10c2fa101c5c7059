// Debug probes and test seams: the per-sample trace, the phase profile, and the exp10 / arithmetic-identity / quantisation-sweep kernels.
#include "engine_core.h"
#include "lpcnet_exp10.h"

// debug trace (tests only): allocate / fetch the per-sample trace of workgroup 0, stream 0
extern "C" int lpcn_batch_dev_debug_trace(lpcn_batch_dev *b, int n_samples, float *host_out)
{
    DeviceGuard guard(b->e->device);
    if (host_out == nullptr) {
        { int rcw = wait_all(b); if (rcw) return rcw; }
        b->d_dbg.release();
        return n_samples > 0 ? b->d_dbg.alloc((size_t)n_samples * LPCN_DBG_STRIDE, true) : 0;
    }
    if (!b->d_dbg) { snprintf(g_err, sizeof(g_err), "trace not enabled"); return LPCN_E_ARG; }
    { int rcw = wait_all(b); if (rcw) return rcw; }
    HIP_TRY(hipMemcpy(host_out, b->d_dbg, sizeof(float) * (size_t)n_samples * LPCN_DBG_STRIDE, hipMemcpyDeviceToHost));
    return 0;
}

// per-phase shader-clock totals of workgroup 0 / wave 0 (out == NULL: enable + zero; else fetch 8 values)
extern "C" int lpcn_batch_dev_profile(lpcn_batch_dev *b, unsigned long long *out)
{
    DeviceGuard guard(b->e->device);
    if (!b->d_prof) { int rca = b->d_prof.alloc(96); if (rca) return rca; }
    { int rcw = wait_all(b); if (rcw) return rcw; }
    if (!out) { HIP_TRY(hipMemset(b->d_prof, 0, 96 * sizeof(unsigned long long))); return 0; }
    HIP_TRY(hipMemcpy(out, b->d_prof, 96 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}

namespace lpcn {
// test seam: lpcn_exp10 on the device for an array of arguments (tests/test_exp10.py sweeps it against glibc)
__global__ __launch_bounds__(256) void exp10_kernel(const float *x, double *out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = lpcn_exp10(x[i]);
}
}  // namespace lpcn

// test seam: the device's 10^x (lpcnet_exp10.h) for host arrays
extern "C" int lpcn_debug_exp10(int device, const float *x, double *out, size_t n)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { snprintf(g_err, sizeof(g_err), "no such HIP device"); return LPCN_E_NODEVICE; }
    DeviceGuard guard(device);
    DevBuf<float> dx;
    DevBuf<double> dy;
    int rc = 0;
    if ((rc = dx.alloc(n)) || (rc = dy.alloc(n))) return rc;
    if (hipMemcpy(dx, x, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = LPCN_E_HIP;
    if (!rc) {
        hipLaunchKernelGGL(lpcn::exp10_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const float *)dx, dy.p, n);
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, dy, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = LPCN_E_HIP;
    }
    if (rc) snprintf(g_err, sizeof(g_err), "exp10 test kernel failed");
    return rc;
}

// test seam: the arithmetic identities PARITY rests on, evaluated with THIS library's compile flags and float mode.
//   * v_mfma_f32_4x4x1(A, B, C = -0.0): register k of lane j of a quad == v_mul_f32(A of lane k, B of lane j), bit for bit
//     (the GRU-A items of the float PARITY kernels form their products there, sample_kernel.hip.h: mac());
//   * each half of v_pk_mul_f32 / v_pk_add_f32 == v_mul_f32 / v_add_f32 (GRU-B's block loop, the items' sums).
// n lanes (a multiple of 64).  out_mfma / out_mul: [n][4] bit patterns (k = 0..3: A from lane 4*(i/4) + k, B from lane i);
// out_pk / out_sc: [n][4] = {pk_mul half 0, half 1, pk_add half 0, half 1} and the scalar instructions' results on the same operands
// (half 0: (a[i], b[i]), half 1: (a[i^1], b[i^1])).
__global__ void lpcn_arith_identity_kernel(const float *a, const float *b, uint32_t *out_mfma, uint32_t *out_mul, uint32_t *out_pk, uint32_t *out_sc)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    f4 negz = {-0.f, -0.f, -0.f, -0.f};
    asm volatile("" : "+v"(negz));                         // (the same guard as the kernel's: the addend must reach the instruction as -0.0)
    const float av = a[i], bv = b[i];
    const f4 p = __builtin_amdgcn_mfma_f32_4x4x1f32(av, bv, negz, 0, 0, 0);
    // (element-wise copies first: hipcc's __builtin_bit_cast of an ext-vector ELEMENT reads element 0 whatever the index)
    const float pe[4] = {p[0], p[1], p[2], p[3]};
    const size_t q = i & ~(size_t)3;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float ak = a[q + k], m;
        asm volatile("v_mul_f32 %0, %1, %2" : "=v"(m) : "v"(ak), "v"(bv));
        out_mfma[i * 4 + k] = __float_as_uint(pe[k]);
        out_mul[i * 4 + k] = __float_as_uint(m);
    }
    const float a2 = a[i ^ 1], b2 = b[i ^ 1];
    f2 x = {av, a2}, y = {bv, b2}, pm, pa;
    asm volatile("v_pk_mul_f32 %0, %1, %2" : "=v"(pm) : "v"(x), "v"(y));
    asm volatile("v_pk_add_f32 %0, %1, %2" : "=v"(pa) : "v"(x), "v"(y));
    float m0, m1, s0, s1;
    asm volatile("v_mul_f32 %0, %1, %2" : "=v"(m0) : "v"(av), "v"(bv));
    asm volatile("v_mul_f32 %0, %1, %2" : "=v"(m1) : "v"(a2), "v"(b2));
    asm volatile("v_add_f32 %0, %1, %2" : "=v"(s0) : "v"(av), "v"(bv));
    asm volatile("v_add_f32 %0, %1, %2" : "=v"(s1) : "v"(a2), "v"(b2));
    const float pk0 = pm[0], pk1 = pm[1], pk2 = pa[0], pk3 = pa[1];
    out_pk[i * 4 + 0] = __float_as_uint(pk0); out_pk[i * 4 + 1] = __float_as_uint(pk1);
    out_pk[i * 4 + 2] = __float_as_uint(pk2); out_pk[i * 4 + 3] = __float_as_uint(pk3);
    out_sc[i * 4 + 0] = __float_as_uint(m0); out_sc[i * 4 + 1] = __float_as_uint(m1);
    out_sc[i * 4 + 2] = __float_as_uint(s0); out_sc[i * 4 + 3] = __float_as_uint(s1);
}

extern "C" int lpcn_debug_arith_identities(int device, const float *a, const float *b, uint32_t *out_mfma, uint32_t *out_mul,
                                           uint32_t *out_pk, uint32_t *out_sc, size_t n)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { snprintf(g_err, sizeof(g_err), "no such HIP device"); return LPCN_E_NODEVICE; }
    if (!n || n % 64) { snprintf(g_err, sizeof(g_err), "operand count must be a positive multiple of 64"); return LPCN_E_ARG; }
    DeviceGuard guard(device);
    DevBuf<float> d_in;
    DevBuf<uint32_t> d_out;
    int rc = 0;
    if ((rc = d_in.alloc(2 * n)) || (rc = d_out.alloc(16 * n))) return rc;
    if (hipMemcpy(d_in, a, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_in + n, b, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = LPCN_E_HIP;
    if (!rc) {
        hipLaunchKernelGGL(lpcn_arith_identity_kernel, dim3((unsigned)(n / 64)), dim3(64), 0, 0, (const float *)d_in, (const float *)(d_in + n),
                           d_out, d_out + 4 * n, d_out + 8 * n, d_out + 12 * n);
        uint32_t *const dst[4] = {out_mfma, out_mul, out_pk, out_sc};
        if (hipGetLastError() != hipSuccess) rc = LPCN_E_HIP;
        for (int k = 0; k < 4 && !rc; ++k)
            if (hipMemcpy(dst[k], d_out + (size_t)k * 4 * n, 4 * n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) rc = LPCN_E_HIP;
    }
    if (rc) snprintf(g_err, sizeof(g_err), "arithmetic identity test kernel failed");
    return rc;
}

// test seam: the state re-quantisation of the int8 kernels.  The reference computes (int)floor(.5 + t) with t = 127 x rounded to float and the
// sum in DOUBLE (src/vec.h:311-316: exact, 0.5 + t needs at most 31 bits); the kernels use ONE instruction, v_cvt_rpi_i32_f32 ("round to
// nearest, ties toward +infinity" = floor(t + 0.5) evaluated exactly), when LPCN_QUANT_RPI is set.  This sweep compares both on ALL 2^32 bit
// patterns: out[0] = mismatches among the finite t with |t| < 2^31, out[1] = mismatches inside the reachable range |t| <= 127.5 (|x| <= 1),
// out[2] = one mismatching bit pattern (if any).
__global__ void lpcn_quant_sweep_kernel(unsigned long long *out)
{
    const uint32_t base = (blockIdx.x * blockDim.x + threadIdx.x) * 256u;
    unsigned bad = 0, bad_in = 0;
    for (uint32_t k = 0; k < 256u; ++k) {
        const uint32_t u = base + k;
        const float t = __uint_as_float(u);
        if (!(fabsf(t) < 2147483648.f)) continue;            // NaN, infinities and |t| >= 2^31: the C conversion is undefined there
        const int want = (int)floor(.5 + (double)t);
        int got;
        asm volatile("v_cvt_rpi_i32_f32 %0, %1" : "=v"(got) : "v"(t));
        if (got != want) { ++bad; if (fabsf(t) <= 127.5f) ++bad_in; out[2] = u; }
    }
    if (bad) atomicAdd(&out[0], (unsigned long long)bad);
    if (bad_in) atomicAdd(&out[1], (unsigned long long)bad_in);
}

extern "C" int lpcn_debug_quant_sweep(int device, unsigned long long *out3)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { snprintf(g_err, sizeof(g_err), "no such HIP device"); return LPCN_E_NODEVICE; }
    DeviceGuard guard(device);
    DevBuf<unsigned long long> d;
    int rc = d.alloc(3);
    if (rc) return rc;
    if (hipMemset(d, 0, 3 * sizeof(unsigned long long)) != hipSuccess) rc = LPCN_E_HIP;
    if (!rc) {
        hipLaunchKernelGGL(lpcn_quant_sweep_kernel, dim3(65536), dim3(256), 0, 0, d.p);      // 2^16 x 2^8 threads x 2^8 patterns
        if (hipGetLastError() != hipSuccess || hipMemcpy(out3, d, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) rc = LPCN_E_HIP;
    }
    if (rc) snprintf(g_err, sizeof(g_err), "quantisation sweep kernel failed");
    return rc;
}
