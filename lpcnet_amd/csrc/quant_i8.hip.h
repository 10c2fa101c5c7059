// int8 (DOT_PROD) arithmetic of the reference's generic-C build, src/vec.h:274-339, as the sample kernels and the PLC network share it:
//   x_q = (signed char)(int)floor(.5 + 127*x)   (float product, double sum)
//   out = out*(128*127);  out += (w0*x0 + w1*x1 + w2*x2 + w3*x3) per block (exact integer);  out *= 1/128/127
#pragma once
#include <hip/hip_runtime.h>

namespace lpcn {

constexpr float QS = 128.f * 127.f, QS1 = 1.f / 128.f / 127.f;
__device__ __forceinline__ int quant_s8(float x)
{
    const float t = 127.f * x;
    // floor(.5 + t) as ONE instruction, v_cvt_rpi_i32_f32 (round to nearest, ties toward +infinity): == (int)floor(.5 + (double)t) for every finite t
    // (lpcnet_hip_quant_sweep_device: all 2^32 bit patterns on the device)
    int q;
    asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(q) : "v"(t));
    return q & 0xFF;
}

}  // namespace lpcn
